"""The steady-state body of the shipped bf16 GEMM loop (gemm_mainloop_pp3_m16, RF_PP3_ASM) must give exactly what the plain
256 x 256 loop gives: the MFMA sequence of every accumulator is unchanged, so any difference is a bug, not rounding.

Covers K-tile counts 1 .. 9 (odd and even, below and above the 2-tile unroll), K-segment (LoRA / concatenated input) boundaries
on every phase of the unroll, M / N edges that are not multiples of 256, two token groups, and the bias / GELU / gate-residual
epilogues."""
import ctypes as C

import pytest
import torch

from reflectionflow_amd import _lib as L, ops
from tests.test_kernels_gpu import BF, dev, rnd   # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


def _run(groups, N, epi, schedule):
    d = ops.build_gemm_desc(groups, N, epi, schedule=schedule)
    L.check(L.load().rf_gemm_bf16(C.byref(d), ops.stream_ptr()), "rf_gemm_bf16")
    torch.cuda.synchronize()


def _pair(dev, Ms, N, seg_ks, epi=L.RF_EPI_STORE, seed=0):
    """Launch the same grouped GEMM through the default loop (TILE256) and the plain loop (PLAIN256); return both outputs."""
    outs = []
    for sched in (L.RF_SCHED_TILE256, L.RF_SCHED_PLAIN256):
        groups, res = [], []
        for gi, M in enumerate(Ms):
            segs = [ops.Seg(rnd(M, k, dev=dev, seed=seed + 10 * gi + si), rnd(N, k, dev=dev, scale=0.05, seed=seed + 100 + 10 * gi + si))
                    for si, k in enumerate(seg_ks)]
            out = torch.zeros(M, N, dtype=BF, device=dev)
            kw = {"bias": rnd(N, dev=dev, seed=seed + 7 + gi), "out": out}
            if epi == L.RF_EPI_GATE_RES:
                kw["residual"] = rnd(M, N, dev=dev, seed=seed + 8 + gi)
                kw["gate"] = rnd(N, dev=dev, seed=seed + 9 + gi)
            groups.append(ops.Group(segs, **kw))
            res.append(out)
        _run(groups, N, epi, sched)
        outs.append(res)
    return outs


def _check(outs, what):
    for gi, (a, b) in enumerate(zip(*outs)):
        assert torch.isfinite(a.float()).all(), f"{what}: non-finite output (group {gi})"
        assert torch.equal(a, b), f"{what}: group {gi} differs from the plain loop in {(a != b).sum().item()} elements"


@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_k_tiles(dev, nk):
    _check(_pair(dev, [512], 512, [64 * nk]), f"nk={nk}")


@pytest.mark.parametrize("M,N", [(300, 520), (257, 255), (4608, 3072)])
def test_edges(dev, M, N):
    _check(_pair(dev, [M], N, [64 * 11]), f"M={M} N={N}")


# segment boundaries: the first segment's tile count runs over every phase of the 2-tile unroll and over steady runs of 0 .. 5 tiles
@pytest.mark.parametrize("k0", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("k1", [1, 2, 3, 6])
def test_two_segments(dev, k0, k1):
    _check(_pair(dev, [384], 640, [64 * k0, 64 * k1], seed=k0 * 7 + k1), f"segments {k0}+{k1}")


@pytest.mark.parametrize("ks", [(5, 1, 4), (2, 3, 2), (8, 2, 1), (1, 1, 1)])
def test_three_segments(dev, ks):
    _check(_pair(dev, [320], 512, [64 * k for k in ks], seed=sum(ks)), f"segments {ks}")


@pytest.mark.parametrize("epi", [L.RF_EPI_GELU, L.RF_EPI_GATE_RES])
def test_epilogues_two_groups(dev, epi):
    _check(_pair(dev, [700, 190], 768, [64 * 13, 64 * 2], epi=epi), f"epilogue {epi}")
