"""Restatement of Pillow's 8-bit bicubic resampler (what `PIL.Image.resize((w, h))` does to an RGB image with the default filter),
in plain numpy, written from Pillow's Resample.c and pinned to the installed Pillow by tests/test_handoff_cpu.py.  It is the
checker's statement of the rules the HIP resize (csrc/image_handoff.hip, tables from flux/image_hip.py) has to match exactly:

  per axis, output index i:  scale = in / out, fs = max(scale, 1), support = 2 fs, center = (i + 0.5) scale
  taps lo = max(int(center - support + 0.5), 0) .. min(int(center + support + 0.5), in)
  weight of tap j = bicubic((j - center + 0.5) / fs), a = -0.5, in double, divided by the sum over the window (added tap by tap)
  integer weight = int(k 2^22 + 0.5) for k >= 0, int(k 2^22 - 0.5) for k < 0                      (C truncation)
  a pass:  clip(((1 << 21) + sum level * coeff) >> 22, 0, 255)
  horizontal pass first, into an 8-bit image; the vertical pass reads that image; an axis whose size does not change is skipped.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22


def bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def axis_coeffs(n_in: int, n_out: int):
    """[(lo, [integer coefficients])] per output index."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        k = [bicubic((j + lo - center + 0.5) * (1.0 / fs)) for j in range(hi - lo)]
        total = 0.0
        for v in k:
            total += v
        if total != 0.0:
            k = [v / total for v in k]
        out.append((lo, [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in k]))
    return out


def max_taps(n_in: int, n_out: int) -> int:
    return 2 * int(math.ceil(2.0 * max(n_in / n_out, 1.0))) + 1


def _pass(img: np.ndarray, n_out: int, stats=None) -> np.ndarray:
    """resample axis 0 of an integer array [n_in, ...] holding 8-bit levels; stats["clipped"] counts sums the clip changed"""
    src = img.astype(np.int64)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    for i, (lo, k) in enumerate(axis_coeffs(img.shape[0], n_out)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j, c in enumerate(k):
            acc += src[lo + j] * c
        v = acc >> PRECISION_BITS
        if stats is not None:
            stats["clipped"] = stats.get("clipped", 0) + int(((v < 0) | (v > 255)).sum())
        out[i] = np.clip(v, 0, 255)
    return out


def resize(levels: np.ndarray, h: int, w: int, stats=None) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [h, w, 3], as PIL.Image.fromarray(levels).resize((w, h))."""
    x = np.asarray(levels, dtype=np.uint8)
    H, W, _ = x.shape
    if W != w:
        x = _pass(x.transpose(1, 0, 2), w, stats).transpose(1, 0, 2)
    if H != h:
        x = _pass(x, h, stats)
    return np.ascontiguousarray(x)


# the sizes the hand-off is pinned on: (H, W) -> (h, w)
SIZES = [((1024, 1024), (512, 512)), ((2048, 2048), (512, 512)), ((1024, 768), (512, 512)), ((1000, 1000), (384, 384)),
         ((256, 256), (512, 512)), ((512, 512), (512, 512))]


def synthetic_levels(seed: int, H: int, W: int) -> np.ndarray:
    """random uint8 levels [H, W, 3] whose top quarter is saturated to 0 / 255 (in 32-pixel blocks), so that the filter's
    overshoot next to saturated edges exercises the clip of both passes"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    q = H // 4
    blocks = rng.integers(0, 2, size=((q + 31) // 32, (W + 31) // 32, 3), dtype=np.uint8) * 255
    x[:q] = np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1)[:q, :W]
    return x
