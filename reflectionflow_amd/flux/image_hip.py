"""The 8-bit image steps between two rounds of the reflection search on the HIP path (csrc/image_handoff.hip).

The reference hands a selected candidate to the next round as a file (tts_reflectionflow.py:273-279): the decoded image is written
as PNG, re-opened, `resize((condition_size, condition_size))`d with PIL's default filter, and `Condition.encode` runs
`VaeImageProcessor.preprocess` + `vae.encode` on it.  Here the same values are formed on the device:

    levels_from_halo(halo)        the decoder's zero-halo NHWC output -> the PNG's uint8 levels (rf_image_levels)
    resize_levels(levels, h, w)   uint8 levels -> (the levels PIL's resize returns, the zero-halo bf16 buffer rf_vae_encode reads)
                                  (rf_pil_resize_to_vae_input)

both bit for bit what the host path gives: Pillow's 8-bit resampler is integer arithmetic over coefficient tables that
`pil_resize_tables` restates on the host (doubles, once per (in, out)), and bf16(2 (level / 255) - 1) is a 256-entry table built
with the torch expression it has to equal.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Tuple

import numpy as np
import torch

from .. import _lib as L
from ..ops import RFError, stream_ptr

BF = torch.bfloat16
PRECISION_BITS = 32 - 8 - 2          # Pillow: 8-bit samples, 2 bits of headroom for the filter's negative lobes


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Pillow's bicubic_filter, a = -0.5 (Resample.c)."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


@functools.lru_cache(maxsize=64)
def pil_resize_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis of an n_in -> n_out bicubic resize: (lo [n_out] int32,
    n [n_out] int32, coef [k][n_out] int32, tap-major, zero beyond n).  Output i reads source taps lo[i] .. lo[i] + n[i] - 1; the
    weight of tap j is bicubic((j - center + 0.5) / fs) / (sum over the window) in double, fs = max(n_in / n_out, 1), and becomes
    the integer int(k 2^22 +- 0.5) (truncation, +0.5 for k >= 0, -0.5 below).  The window sum is accumulated tap by tap, in
    Pillow's order: a pairwise sum can differ in the last bit and move a coefficient by one."""
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"pil_resize_tables({n_in}, {n_out})")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    k = 2 * int(math.ceil(support)) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int): truncation, arguments >= -1.5 here
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    assert int(n.max()) <= k and int(n.min()) >= 1
    j = np.arange(k)[None, :]
    wt = _bicubic((j + lo[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    wt = np.where(j < n[:, None], wt, 0.0)
    total = np.zeros(n_out)
    for t in range(k):
        total = total + wt[:, t]
    wt = np.where(total[:, None] != 0.0, wt / np.where(total == 0.0, 1.0, total)[:, None], wt)
    q = wt * float(1 << PRECISION_BITS)
    coef = np.where(q < 0, np.trunc(q - 0.5), np.trunc(q + 0.5)).astype(np.int32)
    return lo.astype(np.int32), n.astype(np.int32), np.ascontiguousarray(coef.T)


def vae_input_table() -> torch.Tensor:
    """bf16(2 (level / 255) - 1) for level = 0 .. 255, by VaeImageProcessor.preprocess's own operations (uint8 -> fp32, / 255,
    2 x - 1) and the `.to(bf16)` of encode_images."""
    x = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0)
    return (2.0 * x - 1.0).to(BF)


_dev_tables: Dict[tuple, tuple] = {}
_dev_lut: Dict[torch.device, torch.Tensor] = {}


def _tables_on(device, n_in: int, n_out: int):
    key = (device, n_in, n_out)
    if key not in _dev_tables:
        if len(_dev_tables) >= 64:
            _dev_tables.pop(next(iter(_dev_tables)))
        _dev_tables[key] = tuple(torch.from_numpy(t).to(device) for t in pil_resize_tables(n_in, n_out))
    return _dev_tables[key]


def _lut_on(device) -> torch.Tensor:
    if device not in _dev_lut:
        _dev_lut[device] = vae_input_table().to(device)
    return _dev_lut[device]


@torch.no_grad()
def levels_from_halo(halo: torch.Tensor, channels: int = 3) -> torch.Tensor:
    """HipVAE.decode_halo's output [(H + 2), (W + 2), C] bf16 (or a contiguous batch [B, H + 2, W + 2, C]) -> uint8 [H, W, 3]
    ([B, H, W, 3]): what VaeImageProcessor.postprocess(..., "pil") holds for that image, i.e. the PNG's levels."""
    if not halo.is_cuda or halo.dtype != BF:
        raise RFError("levels_from_halo: needs the decoder's bf16 output on the device; the HIP path has no CPU fallback")
    x = halo if halo.dim() == 4 else halo[None]
    if not x.is_contiguous() or x.shape[-1] < channels or channels != 3:
        raise RFError(f"levels_from_halo: needs a contiguous [.., H + 2, W + 2, C >= 3] buffer, got {tuple(halo.shape)}")
    B, Hp, Wp, Cc = x.shape
    out = torch.empty(B, Hp - 2, Wp - 2, 3, dtype=torch.uint8, device=x.device)
    interior = x[:, 1:, 1:]                                              # data pointer at (row 1, pixel 1, channel 0) of image 0
    L.check(L.load().rf_image_levels(interior.data_ptr(), Hp * Wp * Cc, Wp * Cc, Cc, 1, B, Hp - 2, Wp - 2, out.data_ptr(), stream_ptr()),
            "rf_image_levels")
    return out if halo.dim() == 4 else out[0]


@torch.no_grad()
def resize_levels(levels: torch.Tensor, h: int, w: int, cin_pad: int = 64) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 levels [H, W, 3] (or [B, H, W, 3]) on the device -> (levels_small uint8 [h, w, 3], vae_input_halo bf16
    [(h + 2), (w + 2), cin_pad]) (with a leading B for a batch): the image `PIL.Image.resize((w, h))` returns for an RGB image, and
    that image as `HipVAE.encode_moments_halo` takes it -- 2 (level / 255) - 1 in bf16 in channels 0..2, zero halo and pad channels,
    and behind each image the zeroed slack the encoder's first GEMM reads past the last pixel (vae_hip._padded_input)."""
    if not levels.is_cuda or levels.dtype != torch.uint8:
        raise RFError("resize_levels: needs uint8 levels on the device; the HIP path has no CPU fallback")
    x = (levels if levels.dim() == 4 else levels[None]).contiguous()
    if x.shape[-1] != 3:
        raise RFError(f"resize_levels: needs [.., H, W, 3] levels, got {tuple(levels.shape)}")
    B, H, W, _ = x.shape
    dev = x.device
    xt = _tables_on(dev, W, w) if W != w else None
    yt = _tables_on(dev, H, h) if H != h else None
    ptr = lambda t: t.data_ptr() if t is not None else None              # noqa: E731
    n = (h + 2) * (w + 2) * cin_pad
    stride = n + 64 * max(cin_pad, 64)
    flat = torch.zeros(B * stride, dtype=BF, device=dev)
    small = torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
    scratch = torch.empty(B, H, w, 3, dtype=torch.uint8, device=dev) if (xt is not None and yt is not None) else None
    lut = _lut_on(dev)
    L.check(L.load().rf_pil_resize_to_vae_input(
        x.data_ptr(), B, H, W, h, w,
        ptr(xt and xt[0]), ptr(xt and xt[1]), ptr(xt and xt[2]), xt[2].shape[0] if xt else 0,
        ptr(yt and yt[0]), ptr(yt and yt[1]), ptr(yt and yt[2]), yt[2].shape[0] if yt else 0,
        lut.data_ptr(), ptr(scratch), small.data_ptr(), flat.data_ptr(), stride, cin_pad, stream_ptr()), "rf_pil_resize_to_vae_input")
    halo = flat.view(B, stride)[:, :n].view(B, h + 2, w + 2, cin_pad)
    return (small, halo) if levels.dim() == 4 else (small[0], halo[0])
