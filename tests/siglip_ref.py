"""Torch restatement (fp32, CPU) of transformers' SiglipModel -- both towers, the attention-pooling head and the pairwise-sigmoid
score -- in two forms, plus the numpy restatement of rf_siglip_preprocess:
  * `vision_pooled` / `text_pooled` on the RAW state dict, operation for operation what transformers 5.15 runs with eager attention
    (tests/test_siglip_cpu.py pins them bit for bit to `SiglipModel.from_config`): the reference of the GPU tests;
  * `vision_pooled_packed` / `text_pooled_packed` on the PACKED weights the HIP towers read (flux/text_hip.py siglip_pack_*: heads
    padded to 80, q prescaled, v bias folded, intermediate size padded to 64): the proof that the packing is exact.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

BF = torch.bfloat16

# the two tiny configs of the tests: hidden 144 = 2 heads x 72 (padded to 80), inter 272 (padded to 320), 2 layers, vocab 512, 64
# positions; 224 px / 14 = 256 tokens (keys resident, no padded rows), 322 px / 14 = 529 tokens (S_pad 544: keys streamed, padded keys)
TINY_224 = dict(text=dict(vocab=512, hidden=144, heads=2, inter=272, layers=2, max_pos=64),
                vision=dict(hidden=144, heads=2, inter=272, layers=2, image_size=224, patch=14), projection_dim=144)
TINY_322 = dict(text=TINY_224["text"], vision=dict(TINY_224["vision"], image_size=322), projection_dim=144)


def bf16_round(sd):
    return {k: v.to(BF).float() for k, v in sd.items()}


def hf_siglip_model(cfg: dict, sd: dict = None):
    """transformers.SiglipModel (fp32, CPU, eval, eager attention) of a geometry table of tts/siglip_verifier.py, `sd` loaded strictly"""
    import transformers as tr
    t, v = cfg["text"], cfg["vision"]
    c = tr.SiglipConfig(
        text_config=dict(vocab_size=t["vocab"], hidden_size=t["hidden"], intermediate_size=t["inter"], num_hidden_layers=t["layers"],
                         num_attention_heads=t["heads"], max_position_embeddings=t["max_pos"], projection_size=cfg["projection_dim"],
                         bos_token_id=None, eos_token_id=None, pad_token_id=1),
        vision_config=dict(hidden_size=v["hidden"], intermediate_size=v["inter"], num_hidden_layers=v["layers"], num_attention_heads=v["heads"],
                           image_size=v["image_size"], patch_size=v["patch"]))
    c._attn_implementation = "eager"
    c.text_config._attn_implementation = "eager"
    c.vision_config._attn_implementation = "eager"
    m = tr.SiglipModel(c).eval()
    if sd is not None:
        missing, unexpected = m.load_state_dict(sd, strict=False)
        missing = [k for k in missing if not k.endswith("position_ids")]
        assert not missing and not unexpected, (missing, unexpected)
    return m


# ---- raw form: transformers' operations -------------------------------------------------------------------------------------------------
def _layers_raw(x, sd, prefix, n_layers, heads, eps):
    B, S, D = x.shape
    d = D // heads
    for i in range(n_layers):
        p = f"{prefix}encoder.layers.{i}."
        h = F.layer_norm(x, (D,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
        q = F.linear(h, sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.q_proj.bias"]).view(B, S, heads, d).transpose(1, 2)
        k = F.linear(h, sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.k_proj.bias"]).view(B, S, heads, d).transpose(1, 2)
        v = F.linear(h, sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.v_proj.bias"]).view(B, S, heads, d).transpose(1, 2)
        w = torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5
        w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        o = torch.matmul(w, v).transpose(1, 2).contiguous().reshape(B, S, D).contiguous()
        x = x + F.linear(o, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (D,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps)
        h = F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]), approximate="tanh")
        x = x + F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x


@torch.no_grad()
def vision_tokens(sd, pixel_values, cfg, eps=1e-6):
    """post_layernorm(encoder(embeddings(pixels))) [B, T, D]"""
    v, p = cfg["vision"], "vision_model."
    x = F.conv2d(pixel_values, sd[p + "embeddings.patch_embedding.weight"], sd[p + "embeddings.patch_embedding.bias"], stride=v["patch"])
    x = x.flatten(2).transpose(1, 2) + sd[p + "embeddings.position_embedding.weight"][None]
    x = _layers_raw(x, sd, p, v["layers"], v["heads"], eps)
    return F.layer_norm(x, (v["hidden"],), sd[p + "post_layernorm.weight"], sd[p + "post_layernorm.bias"], eps)


@torch.no_grad()
def pool_head(sd, x, heads, eps=1e-6, prefix="vision_model.head."):
    """SiglipMultiheadAttentionPoolingHead: torch.nn.MultiheadAttention's (slow-path) operations with the probe as the one query"""
    B, T, D = x.shape
    d = D // heads
    wi, bi = sd[prefix + "attention.in_proj_weight"], sd[prefix + "attention.in_proj_bias"]
    probe = sd[prefix + "probe"].repeat(B, 1, 1).transpose(0, 1)                       # [1, B, D] (batch_first -> time-major)
    # [T, B, D]; contiguous: with parameters that require grad torch.matmul folds the time-major input into ONE 2-D GEMM (a copy),
    # with plain tensors it would batch over T instead -- another summation blocking, other last bits
    xs = x.transpose(0, 1).contiguous()
    q = F.linear(probe, wi[:D], bi[:D])
    kv = F.linear(xs, wi[D:], bi[D:]).unflatten(-1, (2, D)).unsqueeze(0).transpose(0, -2).squeeze(-2).contiguous()
    k, vv = kv[0], kv[1]
    q = q.view(1, B * heads, d).transpose(0, 1)
    k = k.view(T, B * heads, d).transpose(0, 1)
    vv = vv.view(T, B * heads, d).transpose(0, 1)
    w = torch.bmm(q * math.sqrt(1.0 / float(d)), k.transpose(-2, -1))
    w = F.softmax(w, dim=-1)
    o = torch.bmm(w, vv).transpose(0, 1).contiguous().view(1 * B, D)
    o = F.linear(o, sd[prefix + "attention.out_proj.weight"], sd[prefix + "attention.out_proj.bias"]).view(1, B, D).transpose(1, 0)
    h = F.layer_norm(o, (D,), sd[prefix + "layernorm.weight"], sd[prefix + "layernorm.bias"], eps)
    h = F.gelu(F.linear(h, sd[prefix + "mlp.fc1.weight"], sd[prefix + "mlp.fc1.bias"]), approximate="tanh")
    return (o + F.linear(h, sd[prefix + "mlp.fc2.weight"], sd[prefix + "mlp.fc2.bias"]))[:, 0]


@torch.no_grad()
def vision_pooled(sd, pixel_values, cfg, eps=1e-6):
    return pool_head(sd, vision_tokens(sd, pixel_values, cfg, eps), cfg["vision"]["heads"], eps)


@torch.no_grad()
def text_pooled(sd, ids, cfg, eps=1e-6):
    t, p = cfg["text"], "text_model."
    S = ids.shape[1]
    x = F.embedding(ids, sd[p + "embeddings.token_embedding.weight"]) + F.embedding(torch.arange(S)[None], sd[p + "embeddings.position_embedding.weight"])
    x = _layers_raw(x, sd, p, t["layers"], t["heads"], eps)
    x = F.layer_norm(x, (t["hidden"],), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)
    return F.linear(x[:, -1, :], sd[p + "head.weight"], sd[p + "head.bias"])


@torch.no_grad()
def logits(sd, img, txt):
    """SiglipModel.forward's logits_per_image [B_img, B_txt] from the two pooled outputs"""
    img = img / img.norm(p=2, dim=-1, keepdim=True)
    txt = txt / txt.norm(p=2, dim=-1, keepdim=True)
    lpt = torch.matmul(txt, img.t()) * sd["logit_scale"].exp() + sd["logit_bias"]
    return lpt.t()


# ---- packed form: what the HIP towers compute ------------------------------------------------------------------------------------------
def _layers_packed(x, packed, heads, eps, keep=None):
    B, S, D = x.shape
    for y in packed:
        I = y["w_v"].shape[0]
        hd = I // heads
        h = F.layer_norm(x, (D,), y["ln1_w"], y["ln1_b"], eps)
        qk = F.linear(h, y["w_qk"], y["b_qk"])
        q, k = qk[..., :I].view(B, S, heads, hd).transpose(1, 2), qk[..., I:].view(B, S, heads, hd).transpose(1, 2)
        v = F.linear(h, y["w_v"]).view(B, S, heads, hd).transpose(1, 2)
        o = torch.matmul(F.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1), v).transpose(1, 2).reshape(B, S, I)
        if keep is not None:
            keep.append(o.view(B, S, heads, hd))
        x = x + F.linear(o, y["w_o"], y["b_o"])
        h = F.layer_norm(x, (D,), y["ln2_w"], y["ln2_b"], eps)
        x = x + F.linear(F.gelu(F.linear(h, y["w_fc1"], y["b_fc1"]), approximate="tanh"), y["w_fc2"], y["b_fc2"])
    return x


def _strip(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


@torch.no_grad()
def vision_pooled_packed(sd, pixel_values, cfg, eps=1e-6, keep=None):
    from reflectionflow_amd.flux import text_hip as TH
    v, s = cfg["vision"], _strip(sd, "vision_model.")
    heads, D = v["heads"], v["hidden"]
    d = D // heads
    x = F.conv2d(pixel_values, s["embeddings.patch_embedding.weight"], s["embeddings.patch_embedding.bias"], stride=v["patch"])
    x = x.flatten(2).transpose(1, 2) + s["embeddings.position_embedding.weight"][None]
    x = _layers_packed(x, TH.siglip_pack_layers(s, v["layers"], heads), heads, eps, keep)
    x = F.layer_norm(x, (D,), s["post_layernorm.weight"], s["post_layernorm.bias"], eps)
    hp = TH.siglip_pack_pool_head(s, heads)
    B, T, _ = x.shape
    kv = F.linear(x, hp["w_kv"], hp["b_kv"])
    k, vv = kv[..., :D].view(B, T, heads, d), kv[..., D:].view(B, T, heads, d)
    w = F.softmax(torch.einsum("hc,bthc->bht", hp["probe_q"].view(heads, d), k), dim=-1)
    o = torch.einsum("bht,bthc->bhc", w, vv).reshape(B, D)
    o = F.linear(o, hp["w_po"], hp["b_po"])
    h = F.layer_norm(o, (D,), hp["hln_w"], hp["hln_b"], eps)
    return o + F.linear(F.gelu(F.linear(h, hp["w_fc1"], hp["b_fc1"]), approximate="tanh"), hp["w_fc2"], hp["b_fc2"])


@torch.no_grad()
def text_pooled_packed(sd, ids, cfg, eps=1e-6, keep=None):
    from reflectionflow_amd.flux import text_hip as TH
    t, s = cfg["text"], _strip(sd, "text_model.")
    S = ids.shape[1]
    x = F.embedding(ids, s["embeddings.token_embedding.weight"]) + s["embeddings.position_embedding.weight"][None, :S]
    x = _layers_packed(x, TH.siglip_pack_layers(s, t["layers"], t["heads"]), t["heads"], eps, keep)
    x = F.layer_norm(x, (t["hidden"],), s["final_layer_norm.weight"], s["final_layer_norm.bias"], eps)
    return F.linear(x[:, -1, :], s["head.weight"], s["head.bias"])


# ---- rf_siglip_preprocess in numpy: Pillow's 8-bit resample (Resample.c), integer arithmetic on double-built coefficients -------------
def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _axis_coefs(in_size, out_size):
    """per output pixel: (lo, int64 coefficients [n]): precompute_coeffs + normalize_coeffs_8bpc (22 bits, half away from zero)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        w = [_bicubic((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for x in w:
            ww += x
        w = [x / ww if ww != 0.0 else x for x in w]
        out.append((lo, np.array([int(-0.5 + x * (1 << 22)) if x < 0 else int(0.5 + x * (1 << 22)) for x in w], np.int64)))
    return out


def _resample(rows, coefs):
    """rows [n_in, m] integer levels -> [n_out, m]: clip8(((1 << 21) + sum level * coef) >> 22)"""
    out = np.zeros((len(coefs), rows.shape[1]), np.int64)
    for i, (lo, k) in enumerate(coefs):
        ss = (1 << 21) + (rows[lo:lo + len(k)] * k[:, None]).sum(0)
        out[i] = np.clip(ss >> 22, 0, 255)
    return out


def preprocess_levels_np(levels, size):
    """[H, W, 3] uint8 levels -> [size, size, 3] uint8: horizontal pass (an 8-bit image), then the vertical pass; both always run (a
    pass over an axis that keeps its size has the coefficients 1 << 22, 0, ...: the identity)"""
    H, W, _ = levels.shape
    x = levels.astype(np.int64)
    cx, cy = _axis_coefs(W, size), _axis_coefs(H, size)
    out = np.empty((size, size, 3), np.int64)
    for c in range(3):
        hor = _resample(np.ascontiguousarray(x[:, :, c].T), cx).T
        out[:, :, c] = _resample(hor, cy)
    return out.astype(np.uint8)


def normalise_np(levels_u8):
    """(v / 255 - 0.5) / 0.5 in fp32 as the kernel forms it (v * (1 / 255)), then bf16: [S, S, 3] -> torch bf16 [3, S, S]"""
    v = levels_u8.astype(np.float32) * np.float32(1.0 / 255.0)
    return torch.from_numpy(((v - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)).permute(2, 0, 1).to(BF)


def patches_from_pixels(pixel_values, patch):
    """pixel_values [B, 3, S, S] -> im2col rows [B, (S / patch)^2, k_pad], columns (c, ky, kx), zero-padded (rf_siglip_preprocess layout)"""
    B, C, S, _ = pixel_values.shape
    g = S // patch
    k_pad = (C * patch * patch + 63) // 64 * 64
    x = pixel_values.reshape(B, C, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * patch * patch)
    out = torch.zeros(B, g * g, k_pad, dtype=pixel_values.dtype)
    out[..., : C * patch * patch] = x
    return out
