"""Test helper (not a test): reference and yardstick for rf_attention_bwd in the condition modes 1 and 2.

Operands are the kernels' own: q (carrying softmax_scale * log2 e), k, v as [heads, S, 128], bf16 values held in fp32, so the scores
are s2 = q k^T in the log2 domain and the attention is softmax(s2 * ln 2 + mask).  The mask is built the way the reference's
attn_forward builds it (train_flux/flux/block.py:106-122): a boolean mask with the two (main <-> condition) blocks False for
`union_cond_attn: false` (mode 2), or a zero matrix with log(c_factor) on those two blocks when the attention module carries a
c_factor (mode 1).

  reference()  fp32 autograd through softmax(q k^T ln2 + mask) v
  yardstick()  the same mathematics in fp32 with the kernels' rounding points: P rounded to bf16 where it feeds dV, g = P o (dP - D)
               rounded to bf16 where it feeds dq / dK, bf16 outputs (and D from the bf16 forward output).  What it misses of the
               reference is what ANY implementation with these roundings misses; the GPU test's bound must hold for it first.
"""
import math

import torch

LN2 = math.log(2.0)
BF = torch.bfloat16

# (heads, S, n_main): the smallest shapes at which the per-element region logic can fail
SHAPES = [(2, 112, 64),     # aligned boundary, ragged tail
          (2, 147, 83),     # nothing aligned
          (3, 256, 128),
          (2, 200, 7),      # main smaller than any tile
          (2, 200, 195),    # five condition rows
          (2, 640, 512)]    # large enough for the 192-key and 256-query forms
# (name, mode, cross_bias)
MODES = [("mask", 2, 0.0), ("bias_half", 1, math.log(0.5)), ("bias_3", 1, math.log(3.0))]
BOUND = 1.2e-2              # rel-L2 per gradient: tests/test_train_gpu.py::test_attention_bwd_vs_fp32_autograd
LSE_BOUND = 2e-2            # forward lse against fp64, log2 units (same test)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def attn_mask(S: int, n_main: int, mode: int, cross_bias: float, device=None) -> torch.Tensor:
    """the additive fp32 [S, S] form of block.py:106-122's attention_mask (-inf where the boolean mask is False)"""
    cn = S - n_main
    if mode == 2:
        m = torch.ones(S, S, dtype=torch.bool, device=device)
        m[-cn:, :-cn] = False
        m[:-cn, -cn:] = False
        return torch.zeros(S, S, device=device).masked_fill(~m, float("-inf"))
    m = torch.zeros(S, S, device=device)
    if mode == 1:
        m[-cn:, :-cn] = cross_bias
        m[:-cn, -cn:] = cross_bias
    return m


def reference(q, k, v, dout, mode: int, n_main: int, cross_bias: float):
    """q, k, v, dout: [H, S, 128] (any float dtype).  -> (out, dq, dk, dv) fp32, and lse2 [H, S] fp64 (log2 sum_k 2^(s2 + mask / ln2))"""
    S = q.shape[1]
    mask = attn_mask(S, n_main, mode, cross_bias, q.device)
    qf, kf, vf = (t.detach().float().clone().requires_grad_(True) for t in (q, k, v))
    out = torch.softmax(qf @ kf.transpose(1, 2) * LN2 + mask, -1) @ vf
    out.backward(dout.float())
    s2 = qf.detach().double() @ kf.detach().double().transpose(1, 2) + mask.double() / LN2
    lse2 = torch.logsumexp(s2 * LN2, -1) / LN2
    return out.detach(), qf.grad, kf.grad, vf.grad, lse2


def yardstick(q, k, v, dout, mode: int, n_main: int, cross_bias: float):
    """(dq, dk, dv) fp32 holding bf16 values: fp32 arithmetic with the kernels' rounding points"""
    r = lambda t: t.to(BF).float()   # noqa: E731
    S = q.shape[1]
    mask2 = attn_mask(S, n_main, mode, cross_bias, q.device) / LN2
    qf, kf, vf, do = q.float(), k.float(), v.float(), dout.float()
    s2 = qf @ kf.transpose(1, 2) + mask2
    lse2 = torch.logsumexp(s2 * LN2, -1, keepdim=True) / LN2
    P = torch.exp2(s2 - lse2)                              # masked pairs: exp2(-inf) = 0
    o = r(P @ vf)                                          # the forward's bf16 output
    D = (do * o).sum(-1, keepdim=True)
    g = r(P * (do @ vf.transpose(1, 2) - D))
    dq = r(LN2 * (g @ kf))
    dk = r(LN2 * (g.transpose(1, 2) @ qf))
    dv = r(r(P).transpose(1, 2) @ do)
    return dq, dk, dv


def slot32(n: int) -> int:
    return 8 * ((n % 16) // 4) + 4 * (n // 16) + n % 4


def transposed_tiles(x: torch.Tensor) -> torch.Tensor:
    """[H, s_pad, 128] -> rf_attention_bwd's [H, s_pad / 32, 128, 32] tiles: element (d, slot32(n % 32)) of block n / 32 = x[n][d]"""
    H, sp, d = x.shape
    n_of_slot = [0] * 32
    for n in range(32):
        n_of_slot[slot32(n)] = n
    idx = torch.tensor(n_of_slot, device=x.device)
    return x.view(H, sp // 32, 32, d)[:, :, idx, :].transpose(2, 3).contiguous()


def synthetic_operands(H: int, S: int, seed: int = 0, device="cpu"):
    """q, k, v, dout [H, S, 128] with the statistics of the GPU test's operands (unit-RMS rows, q carrying 128^-0.5 log2 e), bf16 values"""
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn(H, S, 128, generator=g) for _ in range(2))
    q = q / q.pow(2).mean(-1, keepdim=True).sqrt() * (128 ** -0.5 / LN2)
    k = k / k.pow(2).mean(-1, keepdim=True).sqrt()
    v, dout = torch.randn(H, S, 128, generator=g) * 1.5, torch.randn(H, S, 128, generator=g)
    return tuple(t.to(BF).float().to(device) for t in (q, k, v, dout))
