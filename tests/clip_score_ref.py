"""fp32 restatement of the CLIP-score verifier (tts/clip_verifier.py), the checker of its HIP path.

Pinned to transformers' own `CLIPModel` + `CLIPImageProcessorPil` by tests/golden/clip_score.npz (tests/golden/make_clip_golden.py).
  * preprocess_ref: 8-bit levels -> resize the shortest edge to `size` (long edge int(size * long / short)) with torch's antialiased
    bicubic on the levels (PIL's filter, a = -0.5), horizontal pass then vertical pass, each rounded and clipped to 8 bits as PIL's
    8-bit resample does -> centre crop ((new - size) // 2) -> (v / 255 - mean) / std.  PIL uses fixed-point coefficients: this
    matches CLIPImageProcessorPil within 1 level on a minority of pixels;
  * vision_embeds: patch conv (no bias) -> [class | patches] + positions -> pre_layrnorm -> pre-LN encoder layers (quick_gelu) ->
    post_layernorm of row 0 -> visual_projection (no bias);
  * text_embeds: CLIPTextModel's pooled output (oracle/text_oracle.py) -> text_projection (no bias);
  * scores: exp(logit_scale) * cos(image, text) = the diagonal of HF's logits_per_image.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import text_oracle as TO

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
T = torch.Tensor


def resize_geometry(H: int, W: int, size: int = 224):
    """(newH, newW, top, left) of CLIPImageProcessor's shortest-edge resize + centre crop (transformers' rules)."""
    if W <= H:
        newW, newH = size, int(size * H / W)
    else:
        newH, newW = size, int(size * W / H)
    return newH, newW, (newH - size) // 2, (newW - size) // 2


def resized_levels(levels: T, size: int = 224) -> T:
    """[3, H, W] 8-bit levels -> the centre-cropped resized 8-bit levels [3, size, size] (fp32 holding integers)."""
    x = levels.float()[None]
    H, W = x.shape[-2:]
    newH, newW, top, left = resize_geometry(H, W, size)
    # two passes like PIL's 8-bit resample: horizontal first, its output rounded and clipped to 8 bits, then vertical.  (One 2-D
    # pass differs from PIL by up to 7 levels next to saturated edges, where the horizontal overshoot is clipped in PIL.)
    r = F.interpolate(x, size=(H, newW), mode="bicubic", antialias=True, align_corners=False).round().clamp(0, 255)
    r = F.interpolate(r, size=(newH, newW), mode="bicubic", antialias=True, align_corners=False)[0].round().clamp(0, 255)
    return r[:, top:top + size, left:left + size]


def normalise(levels: T) -> T:
    """(v / 255 - mean) / std in fp32, one rounding per operation (what the HIP kernel computes)."""
    v = levels.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(CLIP_STD, dtype=torch.float32)[:, None, None]
    return (v - mean) / std


def preprocess_ref(levels: T, size: int = 224) -> T:
    """[3, H, W] 8-bit levels -> pixel_values [3, size, size] fp32."""
    return normalise(resized_levels(levels, size))


def decoded_to_levels(x: T) -> T:
    """A decoded image in [-1, 1] -> the PNG's 8-bit levels: clamp(x / 2 + 0.5, 0, 1) -> rint(255 v) (VaeImageProcessor.postprocess)."""
    v = (x.float() / 2 + 0.5).clamp(0, 1)
    return (v * 255).round()


def patches_of(pixel_values: T, patch: int, k_pad: int) -> T:
    """pixel_values [B, 3, S, S] -> im2col rows [B, (S / patch)^2, k_pad], columns (c, ky, kx), zero-padded (rf_clip_preprocess layout)."""
    B, C, S, _ = pixel_values.shape
    g = S // patch
    p = pixel_values.reshape(B, C, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * patch * patch)
    return F.pad(p, (0, k_pad - C * patch * patch))


def vision_embeds(sd: Dict[str, T], pixel_values: T, num_heads: int, eps: float = 1e-5) -> T:
    """CLIPModel.get_image_features in fp32: pixel_values [B, 3, S, S] -> image_embeds [B, projection_dim]."""
    s = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v.float() for k, v in sd.items()}
    pw = s["embeddings.patch_embedding.weight"]
    D, _, P, _ = pw.shape
    x = F.conv2d(pixel_values.float(), pw, stride=P).flatten(2).transpose(1, 2)           # [B, np, D]
    B = x.shape[0]
    h = torch.cat([s["embeddings.class_embedding"].expand(B, 1, D), x], 1) + s["embeddings.position_embedding.weight"][None]
    ln = lambda t, p: F.layer_norm(t, (D,), s[p + ".weight"], s[p + ".bias"], eps)  # noqa: E731
    lin = lambda t, p: t @ s[p + ".weight"].t() + s[p + ".bias"]  # noqa: E731
    h = ln(h, "pre_layrnorm")
    S, dk = h.shape[1], D // num_heads
    L = 0
    while f"encoder.layers.{L}.layer_norm1.weight" in s:
        L += 1
    for i in range(L):
        p = f"encoder.layers.{i}."
        n = ln(h, p + "layer_norm1")
        sp = lambda t: t.reshape(B, S, num_heads, dk).transpose(1, 2)  # noqa: E731
        q, k, v = sp(lin(n, p + "self_attn.q_proj") * dk ** -0.5), sp(lin(n, p + "self_attn.k_proj")), sp(lin(n, p + "self_attn.v_proj"))
        w = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        h = h + lin((w @ v).transpose(1, 2).reshape(B, S, D), p + "self_attn.out_proj")
        n = ln(h, p + "layer_norm2")
        h = h + lin(TO.quick_gelu(lin(n, p + "mlp.fc1")), p + "mlp.fc2")
    pooled = ln(h[:, 0], "post_layernorm")
    return pooled @ s["visual_projection.weight"].t()


def text_embeds(sd: Dict[str, T], ids: T, num_heads: int, eos_token_id: int = 2) -> T:
    """CLIPModel.get_text_features in fp32: ids [B, L] -> text_embeds [B, projection_dim]."""
    text = {k: v for k, v in sd.items() if k.startswith("text_model.")}
    _, pooled = TO.clip_text_encode(text, ids, num_heads, eos_token_id=eos_token_id)
    return pooled @ sd["text_projection.weight"].float().t()


def scores(image_embeds: T, text_embed: T, logit_scale: float) -> T:
    """exp(logit_scale) * cos(image_embeds[b], text_embed) in fp32 [B]."""
    i = image_embeds.float() / image_embeds.float().norm(dim=-1, keepdim=True)
    t = text_embed.float().reshape(-1) / text_embed.float().norm()
    return math.exp(float(logit_scale)) * (i @ t)


def synthetic_levels(seed: int, H: int, W: int) -> T:
    """A smooth seeded test picture [3, H, W] uint8: low-frequency colour fields + fine noise + a hard edge (exercises the filter)."""
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(1, 3, 6, 7, generator=g), size=(H, W), mode="bilinear", align_corners=False)[0]
    noise = 0.03 * torch.randn(3, H, W, generator=g)
    yy = torch.arange(H)[:, None].float()
    xx = torch.arange(W)[None, :].float()
    edge = ((xx * 0.37 + yy * 0.61) % 41 < 9).float() * 0.35
    return ((base + noise + edge).clamp(0, 1) * 255).round().to(torch.uint8)
