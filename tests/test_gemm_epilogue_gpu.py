"""The kind-specialised interior epilogue of the 16x16x32 GEMM kernels (epi16_interior, csrc/gemm_bf16.hip) must write exactly
what the generic LDS-staged epilogue writes: the 256 x 256 one-tile-per-block kernel (RF_SCHED_TILE256) and the stream-K kernel
(RF_SCHED_STREAMK) are compared bit for bit against the plain 256 loop (RF_SCHED_PLAIN256), whose 32x32 epilogue is untouched.

Covers every epilogue kind (STORE, GELU, GATE_RES with and without a residual, QKV with and without fused RMSNorm + RoPE into
q / k / V^T, QKV_GELU), interior-only grids and grids with M / N edges, two and four token groups with a tok_offset (V^T runs
that start off a multiple of 4 keep the generic path), K-segment LoRA and a cfg2-sized single-block input projection."""
import ctypes as C

import pytest
import torch

from reflectionflow_amd import _lib as L, ops
from tests.test_kernels_gpu import BF, dev, rnd   # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu

HEADS = 2


def _launch(dev, Ms, N, seg_ks, epi, schedule, seed, residual=True, rope=False, n_split=0, tok_gap=0):
    """One grouped launch with freshly allocated (zeroed) outputs; returns every tensor it writes."""
    qkv = epi in (L.RF_EPI_QKV, L.RF_EPI_QKV_GELU)
    S = sum(Ms) + tok_gap * len(Ms)
    kw = {}
    outs = []
    if qkv:
        q, k, vt, s_pad = ops.alloc_attn_operands(HEADS, S, dev)
        kw.update(q=q, k=k, vt=vt, heads=HEADS, s_pad=s_pad, n_split=n_split, q_scale=0.125)
        outs += [q, k, vt]
        if rope:
            g = torch.Generator(device="cpu").manual_seed(seed + 55)
            kw["rope"] = (torch.rand(S, 128, generator=g).to(dev), torch.rand(S, 128, generator=g).to(dev))
    if schedule == L.RF_SCHED_STREAMK:
        kw["splitk_ws"] = ops.splitk_scratch(dev)
    groups, tok = [], 0
    for gi, M in enumerate(Ms):
        tok += tok_gap
        segs = [ops.Seg(rnd(M, kk, dev=dev, seed=seed + 10 * gi + si), rnd(N, kk, dev=dev, scale=0.05, seed=seed + 100 + 10 * gi + si))
                for si, kk in enumerate(seg_ks)]
        gkw = {"bias": rnd(N, dev=dev, seed=seed + 7 + gi), "tok_offset": tok}
        if epi != L.RF_EPI_QKV:
            out = torch.zeros(M, N - n_split, dtype=BF, device=dev)
            gkw["out"] = out
            outs.append(out)
        if epi == L.RF_EPI_GATE_RES:
            gkw["gate"] = rnd(N, dev=dev, seed=seed + 9 + gi)
            if residual:
                gkw["residual"] = rnd(M, N, dev=dev, seed=seed + 8 + gi)
        if qkv:
            gkw["norm_q"] = rnd(128, dev=dev, seed=seed + 11 + gi)
            gkw["norm_k"] = rnd(128, dev=dev, seed=seed + 12 + gi)
        groups.append(ops.Group(segs, **gkw))
        tok += M
    d = ops.build_gemm_desc(groups, N, epi, schedule=schedule, **kw)
    L.check(L.load().rf_gemm_bf16(C.byref(d), ops.stream_ptr()), "rf_gemm_bf16")
    torch.cuda.synchronize()
    return outs


def _check(dev, Ms, N, seg_ks, epi, seed=0, streamk=True, **kw):
    ref = _launch(dev, Ms, N, seg_ks, epi, L.RF_SCHED_PLAIN256, seed, **kw)
    for sched in (L.RF_SCHED_TILE256,) + ((L.RF_SCHED_STREAMK,) if streamk else ()):
        got = _launch(dev, Ms, N, seg_ks, epi, sched, seed, **kw)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), f"schedule {sched}: output {i} differs in {(a != b).sum().item()} elements"


@pytest.mark.parametrize("Ms,N", [([512], 512), ([300], 392), ([512, 200], 776)])
@pytest.mark.parametrize("epi", [L.RF_EPI_STORE, L.RF_EPI_GELU])
def test_store_gelu(dev, Ms, N, epi):
    _check(dev, Ms, N, [256], epi, seed=1)


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("Ms,N", [([512], 768), ([260, 512], 520)])
def test_gate_res(dev, Ms, N, residual):
    _check(dev, Ms, N, [192], L.RF_EPI_GATE_RES, seed=2, residual=residual)


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("Ms,gap", [([512], 0), ([256, 512], 0), ([130, 512], 0), ([100, 256, 64, 300], 0), ([256, 256], 2)])
def test_qkv(dev, Ms, gap, rope):
    _check(dev, Ms, 3 * HEADS * 128, [256], L.RF_EPI_QKV, seed=3, rope=rope, tok_gap=gap)


@pytest.mark.parametrize("N", [3 * HEADS * 128 + 512, 3 * HEADS * 128 + 264])
def test_qkv_gelu(dev, N):
    _check(dev, [512], N, [256], L.RF_EPI_QKV_GELU, seed=4, rope=True, n_split=3 * HEADS * 128)


def test_lora_segments(dev):
    _check(dev, [512, 256], 512, [192, 64], L.RF_EPI_GATE_RES, seed=5)
    _check(dev, [512], 3 * HEADS * 128, [128, 64], L.RF_EPI_QKV, seed=6, rope=True)


def test_cfg2_sgl_in(dev):
    """FLUX.1-dev single-block input projection at 1024^2: 4608 x 21504 x 3072, QKV_GELU + RoPE, 24 heads."""
    global HEADS
    old, HEADS = HEADS, 24
    try:
        _check(dev, [4608], 21504, [3072], L.RF_EPI_QKV_GELU, seed=7, streamk=False, rope=True, n_split=3 * 24 * 128)
    finally:
        HEADS = old
