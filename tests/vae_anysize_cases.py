"""Shapes and inputs of the any-size VAE attention tests: token counts that are no multiple of 64 (vae_attn_kernel<true> of csrc/vae.hip,
through RF_VAE_OP_ATTN_CORE_RAGGED / RF_VAE_OP_ATTN_BLOCK_RAGGED and rf_vae_decode / rf_vae_encode).  Shared by
tests/test_vae_anysize_cpu.py (yardsticks, refusals) and tests/test_vae_anysize_gpu.py (the kernels).  The generic inputs, the fp64
references and the fp32 yardsticks are tests/vae_kernel_cases.py's, as they stand.  Plain torch on the CPU, deterministic."""
import torch

from tests import vae_kernel_cases as K

BF = torch.bfloat16
VA_C = K.VA_C

# one partial tile (1, 2, 31), a full tile + 1 key (33), the 32 / 64 boundaries +- 1 (31, 33, 63, 65, 95, 97, 127, 129), a last workgroup
# with one query (65, 129, 321), ten tiles + 1 key (321), a tail of 16 / 30 keys in the middle of a tile (48, 190)
CORE_S = (1, 2, 31, 33, 48, 63, 65, 95, 97, 127, 129, 190, 321)
BLOCK_HW = ((1, 1), (1, 2), (5, 7), (6, 8), (9, 9), (3, 43), (7, 19))


def s_pad(S):
    return (S + 63) // 64 * 64


def ragged_routing_inputs(S):
    """tests/vae_kernel_cases.py::routing_inputs for ANY S >= 1: k_j = 32 e_c(j), q_i = 32 e_c(pi(i)) -- the hit scores 1024 / sqrt(512) =
    45.3, every other key 0 (weight e^-45 each: below half an ulp of any |v| >= 2^-6 in fp32 summed over 321 keys), so out[i] must be
    BIT-EQUAL to v[pi(i)].  c(j) is that helper's channel map (injective for S <= 512).  pi(i) = (i + S - 1) mod S: a permutation without
    a fixed point for S > 1 in which query 0 -- a query of the FIRST workgroup -- selects the LAST key S - 1 (the one next to the pad),
    and every query of the last workgroup selects a key of the tail tile.  Returns q, k, v, pi, c."""
    j = torch.arange(S)
    c = 8 * ((37 * j) % 64) + ((j // 64 + j) % 8)
    assert len(set(c.tolist())) == S
    pi = (j + S - 1) % S
    assert sorted(pi.tolist()) == list(range(S)) and int(pi[0]) == S - 1 and (S == 1 or not bool((pi == j).any()))
    k = torch.zeros(S, VA_C)
    k[j, c] = 32.0
    q = torch.zeros(S, VA_C)
    q[j, c[pi]] = 32.0
    v = torch.randn(S, VA_C, generator=K.gen(61, S))
    v = torch.sign(v) * (v.abs() + 2.0 ** -6)
    return q.to(BF), k.to(BF), v.to(BF), pi, c


def winning_pad_key(c):
    """a K row that scores 32 * 32 / sqrt(512) against EVERY query of ragged_routing_inputs (32 at each hit channel): as much as the
    query's true hit, so an unmasked pad key takes half of the row's weight (two of them two thirds, ...)"""
    row = torch.zeros(VA_C)
    row[c] = 32.0
    return row.to(BF)
