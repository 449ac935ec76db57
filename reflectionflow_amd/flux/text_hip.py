"""FLUX's two text encoders on the HIP path (librf_flux.so: rf_t5_encode / rf_clip_text_encode, csrc/text.hip).

What the reference runs for every candidate's prompt (train_flux/flux/generate.py:148-161 -> diffusers FluxPipeline.encode_prompt;
per candidate and round in tts/tts_reflectionflow.py:286-294, where the prompt changes with every reflection):
    pooled_prompt_embeds = CLIPTextModel(clip_ids [B, 77]).pooler_output
    prompt_embeds        = T5EncoderModel(t5_ids [B, 512])[0]
`HipClipVisionEncoder` (+ `clip_score`) is the image side of the CLIP-score verifier (tts/clip_verifier.py).
`HipT5Encoder` / `HipClipTextEncoder` take a Hugging Face `transformers`-layout state dict (so text_encoder_2/*.safetensors and
text_encoder/model.safetensors load unchanged, with or without the `text_model.` prefix) and token ids; `HipTextEncoders` is the
`pipe.text_encoder` callable of flux/pipeline.py (prompt -> (prompt_embeds, pooled)) once a tokenizer callable is supplied --
vocabulary files are host-side data this repo does not ship.  No CPU fallback: CPU tensors or a missing library raise.

What stays in PyTorch is plumbing only: the weight repacking done once here (q|k and wi_0|wi_1 concatenated, 1/sqrt(head_dim) folded
into CLIP's q projection, LayerNorm weights as (w - 1, b), v bias folded into the out-projection bias) and the integer work of the
attention biases (T5's relative-position buckets gathered once per sequence length; CLIP's causal mask).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, Optional, Tuple

import torch

from .. import _lib as L
from ..ops import RFError, stream_ptr

BF = torch.bfloat16


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def _tower_opts(who: str, hidden: int, num_heads: int, head_dim: int, act: str) -> "L.rf_clip_tower_opts":
    """rf_clip_tower_opts of a CLIP tower: head dim 64 (CLIP-L) or 80 (ViT-H/14 vision), activation "quick_gelu" or "gelu" (erf)."""
    if head_dim not in (64, 80):
        raise RFError(f"{who}: head dim {head_dim}: attention kernels exist for head dims 64 and 80")
    if hidden != head_dim * num_heads:
        raise RFError(f"{who}: hidden {hidden} with {num_heads} heads is not a head dim of {head_dim}")
    if act not in L.CLIP_ACTS:
        raise RFError(f"{who}: hidden_act {act!r} (one of {sorted(L.CLIP_ACTS)})")
    o = L.rf_clip_tower_opts()
    o.head_dim, o.act = head_dim, L.CLIP_ACTS[act]
    return o


def t5_relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """transformers' bidirectional bucketing of rel = key position - query position (integer plumbing for the bias table)."""
    nb = num_buckets // 2
    ret = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float().clamp(min=1) / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return ret + torch.where(n < max_exact, n, large)


class _Keep:
    def __init__(self, device):
        self.device = device
        self.keep: List[torch.Tensor] = []

    def t(self, x: torch.Tensor, dtype=BF) -> int:
        x = x.detach().to(self.device, dtype).contiguous()
        self.keep.append(x)
        return x.data_ptr()


class _Workspace:
    def __init__(self, device):
        self.device = device
        self.buf: Optional[torch.Tensor] = None

    def get(self, n: int) -> "L.rf_workspace":
        if n <= 0:
            raise RFError(f"workspace size query failed ({n})")
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.zeros(n, dtype=torch.uint8, device=self.device)
        ws = L.rf_workspace()
        ws.base, ws.bytes = self.buf.data_ptr(), self.buf.numel()
        return ws


class HipT5Encoder:
    """T5EncoderModel (T5 v1.1: gated gelu_new, no biases, RMS norms, bucketed relative-position bias shared by all layers)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, device, eps: float = 1e-6, num_buckets: int = 32,
                 max_distance: int = 128):
        device = torch.device(device)
        if device.type != "cuda":
            raise RFError(f"HipT5Encoder: device {device}; the HIP path has no CPU fallback")
        L.load()
        sd = state_dict
        emb = sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"]
        n_layers = 0
        while f"encoder.block.{n_layers}.layer.0.layer_norm.weight" in sd:
            n_layers += 1
        if n_layers == 0:
            raise RFError("HipT5Encoder: no encoder.block.* keys in the state dict")
        inner = sd["encoder.block.0.layer.0.SelfAttention.q.weight"].shape[0]
        if inner != 64 * num_heads:
            raise RFError(f"HipT5Encoder: inner dim {inner} with {num_heads} heads: the attention kernel is built for d_kv = 64")
        self.device, self.heads, self.num_buckets, self.max_distance = device, num_heads, num_buckets, max_distance
        self.d_model = emb.shape[1]
        k = self._k = _Keep(device)
        self._layers = (L.rf_t5_layer * n_layers)()
        for i in range(n_layers):
            p0, p1 = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            y = self._layers[i]
            y.ln0, y.ln1 = k.t(sd[p0 + "layer_norm.weight"]), k.t(sd[p1 + "layer_norm.weight"])
            y.w_qk = k.t(torch.cat([sd[p0 + "SelfAttention.q.weight"], sd[p0 + "SelfAttention.k.weight"]], 0))
            y.w_v, y.w_o = k.t(sd[p0 + "SelfAttention.v.weight"]), k.t(sd[p0 + "SelfAttention.o.weight"])
            y.w_wi = k.t(torch.cat([sd[p1 + "DenseReluDense.wi_0.weight"], sd[p1 + "DenseReluDense.wi_1.weight"]], 0))
            y.w_wo = k.t(sd[p1 + "DenseReluDense.wo.weight"])
        w = self._w = L.rf_t5_weights()
        w.layers, w.d_model, w.heads, w.d_kv = n_layers, self.d_model, num_heads, 64
        w.d_ff, w.vocab, w.eps = sd["encoder.block.0.layer.1.DenseReluDense.wo.weight"].shape[1], emb.shape[0], eps
        w.embed, w.final_ln = k.t(emb), k.t(sd["encoder.final_layer_norm.weight"])
        w.layer = C.cast(self._layers, C.POINTER(L.rf_t5_layer))
        self._rel = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].detach().to(device, BF).float()   # [buckets, H]
        self._bias: Dict[int, torch.Tensor] = {}
        self._ws = _Workspace(device)

    def _pos_bias(self, S: int) -> torch.Tensor:
        if S not in self._bias:
            sp = _pad32(S)
            pos = torch.arange(sp, device=self.device)
            bucket = t5_relative_position_bucket(pos[None, :] - pos[:, None], self.num_buckets, self.max_distance)
            b = self._rel[bucket].permute(2, 0, 1).contiguous()            # [H, sp, sp] fp32
            b[:, :, S:] = float("-inf")
            if len(self._bias) >= 4:
                self._bias.pop(next(iter(self._bias)))
            self._bias[S] = b
        return self._bias[S]

    @torch.no_grad()
    def encode(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [B, S] (any integer dtype, on the device) -> last hidden state [B, S, d_model] bf16."""
        if not ids.is_cuda:
            raise RFError("HipT5Encoder.encode: ids are on the CPU; the HIP path has no CPU fallback")
        B, S = ids.shape
        lib, w = L.load(), self._w
        bias = self._pos_bias(S)
        w.pos_bias, w.bias_S = bias.data_ptr(), _pad32(S)
        ids32 = ids.to(torch.int32).contiguous()
        out = torch.empty(B, S, self.d_model, dtype=BF, device=self.device)
        for b0 in range(0, B, 64):                      # (the library takes up to 64 sequences per call: one GEMM launch over all their rows)
            nb = min(64, B - b0)
            ws = self._ws.get(lib.rf_t5_workspace_bytes(C.byref(w), nb, S))
            L.check(lib.rf_t5_encode(C.byref(w), ids32[b0].data_ptr(), nb, S, out[b0].data_ptr(), self.d_model, C.byref(ws), stream_ptr()), "rf_t5_encode")
        return out


class HipClipTextEncoder:
    """CLIPTextModel (pre-LN blocks, causal mask, quick_gelu or gelu): last_hidden_state and pooler_output."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, device, eos_token_id: int = 2, eps: float = 1e-5,
                 head_dim: int = 64, act: str = "quick_gelu"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RFError(f"HipClipTextEncoder: device {device}; the HIP path has no CPU fallback")
        L.load()
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}
        n_layers = 0
        while f"encoder.layers.{n_layers}.layer_norm1.weight" in sd:
            n_layers += 1
        if n_layers == 0:
            raise RFError("HipClipTextEncoder: no encoder.layers.* keys in the state dict")
        D = sd["embeddings.token_embedding.weight"].shape[1]
        self._opts = _tower_opts("HipClipTextEncoder", D, num_heads, head_dim, act)
        self.device, self.heads, self.hidden, self.eos_token_id = device, num_heads, D, eos_token_id
        k = self._k = _Keep(device)
        f = lambda t: t.detach().float()  # noqa: E731
        self._layers = _clip_layers(k, sd, n_layers, head_dim)
        w = self._w = L.rf_clip_weights()
        w.layers, w.hidden, w.heads, w.inter = n_layers, D, num_heads, sd["encoder.layers.0.mlp.fc1.weight"].shape[0]
        w.vocab, w.max_pos, w.eps = sd["embeddings.token_embedding.weight"].shape[0], sd["embeddings.position_embedding.weight"].shape[0], eps
        w.tok_embed, w.pos_embed = k.t(sd["embeddings.token_embedding.weight"]), k.t(sd["embeddings.position_embedding.weight"])
        w.final_ln_scale, w.final_ln_shift = k.t(f(sd["final_layer_norm.weight"]) - 1.0), k.t(sd["final_layer_norm.bias"])
        w.layer = C.cast(self._layers, C.POINTER(L.rf_clip_layer))
        self._mask: Dict[int, torch.Tensor] = {}
        self._ws = _Workspace(device)

    def _causal(self, S: int) -> torch.Tensor:
        if S not in self._mask:
            sp = _pad32(S)
            m = torch.full((sp, sp), float("-inf"), device=self.device).triu(1)
            m[:, S:] = float("-inf")
            self._mask[S] = m.contiguous()
        return self._mask[S]

    def eos_positions(self, ids: torch.Tensor) -> List[int]:
        if self.eos_token_id == 2:                 # legacy config (what FLUX ships): the largest token id is EOS
            return ids.argmax(-1).tolist()
        return (ids == self.eos_token_id).int().argmax(-1).tolist()

    @torch.no_grad()
    def encode(self, ids: torch.Tensor, pool_in_library: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """ids [B, S] -> (last_hidden_state [B, S, hidden], pooler_output [B, hidden]), bf16.  pool_in_library: let rf_clip_text_encode
        copy the pooled rows itself from host-side EOS positions (costs a host sync to find them; tests)."""
        if not ids.is_cuda:
            raise RFError("HipClipTextEncoder.encode: ids are on the CPU; the HIP path has no CPU fallback")
        B, S = ids.shape
        lib, w = L.load(), self._w
        m = self._causal(S)
        w.mask, w.mask_S = m.data_ptr(), _pad32(S)
        ids32 = ids.to(torch.int32).contiguous()
        last = torch.empty(B, S, self.hidden, dtype=BF, device=self.device)
        if pool_in_library:
            eos = self.eos_positions(ids)
            pooled = torch.empty(B, self.hidden, dtype=BF, device=self.device)
        for b0 in range(0, B, 64):
            nb = min(64, B - b0)
            o = C.byref(self._opts)
            ws = self._ws.get(_ws_bytes(lib.rf_clip_text_workspace_bytes_opts(C.byref(w), o, nb, S), "rf_clip_text_workspace_bytes_opts"))
            pos_h = (C.c_int32 * nb)(*[int(e) for e in eos[b0:b0 + nb]]) if pool_in_library else None
            L.check(lib.rf_clip_text_encode_opts(C.byref(w), o, ids32[b0].data_ptr(), nb, S, pos_h, last[b0].data_ptr(),
                                                 pooled[b0].data_ptr() if pool_in_library else None, C.byref(ws), stream_ptr()),
                    "rf_clip_text_encode_opts")
        if pool_in_library:
            return last, pooled
        # pooler_output = the final-normed row at the EOS position: a device-side gather (no host sync; the C entry point takes host
        # positions for bindings that have them)
        pos = ids.argmax(-1) if self.eos_token_id == 2 else (ids == self.eos_token_id).int().argmax(-1)
        pooled = last[torch.arange(B, device=self.device), pos]
        return last, pooled


def _ws_bytes(n: int, what: str) -> int:
    """a workspace size query's answer, or the library's message for its refusal"""
    if n < 0:
        L.check(int(n), what)
    return n


def _kpad(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> [N, round_up(K, 64)], zero-padded: the GEMM walks K in 64-element tiles (a no-op for every real tower's width)."""
    K = w.shape[1]
    return w if K % 64 == 0 else torch.nn.functional.pad(w, (0, (K + 63) // 64 * 64 - K))


def _clip_layers(k: "_Keep", sd: Dict[str, torch.Tensor], n_layers: int, head_dim: int = 64) -> "C.Array":
    """rf_clip_layer records of a CLIP encoder (text or vision tower: the same pre-LN layer): q|k concatenated with 1/sqrt(head_dim)
    folded into q, LayerNorm weights as (w - 1, b), v_proj.bias folded into the out-projection bias (softmax rows sum to 1)."""
    f = lambda t: t.detach().float()  # noqa: E731
    qs = 0.125 if head_dim == 64 else head_dim ** -0.5
    layers = (L.rf_clip_layer * n_layers)()
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        y = layers[i]
        y.ln1_scale, y.ln1_shift = k.t(f(sd[p + "layer_norm1.weight"]) - 1.0), k.t(sd[p + "layer_norm1.bias"])
        y.ln2_scale, y.ln2_shift = k.t(f(sd[p + "layer_norm2.weight"]) - 1.0), k.t(sd[p + "layer_norm2.bias"])
        y.w_qk = k.t(_kpad(torch.cat([f(sd[p + "self_attn.q_proj.weight"]) * qs, f(sd[p + "self_attn.k_proj.weight"])], 0)))
        y.b_qk = k.t(torch.cat([f(sd[p + "self_attn.q_proj.bias"]) * qs, f(sd[p + "self_attn.k_proj.bias"])], 0))
        y.w_v = k.t(_kpad(sd[p + "self_attn.v_proj.weight"]))
        wo = f(sd[p + "self_attn.out_proj.weight"])
        y.w_o, y.b_o = k.t(_kpad(wo)), k.t(f(sd[p + "self_attn.out_proj.bias"]) + wo @ f(sd[p + "self_attn.v_proj.bias"]))
        y.w_fc1, y.b_fc1 = k.t(_kpad(sd[p + "mlp.fc1.weight"])), k.t(sd[p + "mlp.fc1.bias"])
        y.w_fc2, y.b_fc2 = k.t(sd[p + "mlp.fc2.weight"]), k.t(sd[p + "mlp.fc2.bias"])
    return layers


class HipClipVisionEncoder:
    """CLIPVisionModel + visual_projection of a Hugging Face `CLIPModel` state dict (`vision_model.*`, `visual_projection.weight`; the
    prefix may be absent): images -> image_embeds [B, projection_dim] bf16 (rf_clip_preprocess + rf_clip_vision_encode).
    Same weight repacking as HipClipTextEncoder; the conv patch embedding becomes a [hidden, K_pad] GEMM weight (columns (c, ky, kx),
    zero-padded to a multiple of 64).  `image_size`: the checkpoint's `vision_config.image_size` (224, 336, ...), the size the images
    are preprocessed at; it must agree with the position-embedding rows ((image_size / patch)^2 + 1).  None: taken from those rows."""

    MAX_BATCH = 64

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, device, eps: float = 1e-5, head_dim: int = 64,
                 act: str = "quick_gelu", image_size: Optional[int] = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RFError(f"HipClipVisionEncoder: device {device}; the HIP path has no CPU fallback")
        L.load()
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state_dict.items()}
        if "visual_projection.weight" not in sd:
            raise RFError("HipClipVisionEncoder: the state dict has no visual_projection.weight (a CLIPModel state dict is needed)")
        n_layers = 0
        while f"encoder.layers.{n_layers}.layer_norm1.weight" in sd:
            n_layers += 1
        if n_layers == 0:
            raise RFError("HipClipVisionEncoder: no vision_model.encoder.layers.* keys in the state dict")
        pw = sd["embeddings.patch_embedding.weight"]                     # [hidden, 3, p, p]
        D, _, P, _ = pw.shape
        self._opts = _tower_opts("HipClipVisionEncoder", D, num_heads, head_dim, act)
        T = sd["embeddings.position_embedding.weight"].shape[0]
        g = int(round(math.sqrt(T - 1)))
        if g * g + 1 != T:
            raise RFError(f"HipClipVisionEncoder: {T} positions is not a square grid + class token")
        if image_size is not None and int(image_size) != g * P:
            raise RFError(f"HipClipVisionEncoder: image_size {image_size} with patch {P} needs {(int(image_size) // P) ** 2 + 1} position rows, "
                          f"the state dict has {T} (a {g * P}-pixel tower)")
        self.device, self.heads, self.hidden, self.patch, self.image_size = device, num_heads, D, P, g * P
        self.tokens, self.s_pad, self.k_pad = T, _pad32(T), (3 * P * P + 63) // 64 * 64
        self.proj_dim = sd["visual_projection.weight"].shape[0]
        k = self._k = _Keep(device)
        f = lambda t: t.detach().float()  # noqa: E731
        self._layers = _clip_layers(k, sd, n_layers, head_dim)
        wpad = torch.zeros(D, self.k_pad)
        wpad[:, : 3 * P * P] = f(pw).reshape(D, 3 * P * P).cpu()
        mask = torch.zeros(self.s_pad, self.s_pad, device=device)
        mask[:, T:] = float("-inf")
        self._mask = mask.contiguous()
        w = self._w = L.rf_clip_vision_weights()
        w.layers, w.hidden, w.heads, w.inter = n_layers, D, num_heads, sd["encoder.layers.0.mlp.fc1.weight"].shape[0]
        w.image_size, w.patch, w.proj_dim, w.mask_S, w.eps = self.image_size, P, self.proj_dim, self.s_pad, eps
        w.patch_w, w.class_embed, w.pos_embed = k.t(wpad), k.t(sd["embeddings.class_embedding"]), k.t(sd["embeddings.position_embedding.weight"])
        w.pre_ln_scale, w.pre_ln_shift = k.t(f(sd["pre_layrnorm.weight"]) - 1.0), k.t(sd["pre_layrnorm.bias"])
        w.post_ln_scale, w.post_ln_shift = k.t(f(sd["post_layernorm.weight"]) - 1.0), k.t(sd["post_layernorm.bias"])
        w.proj, w.mask = k.t(_kpad(sd["visual_projection.weight"])), self._mask.data_ptr()
        w.layer = C.cast(self._layers, C.POINTER(L.rf_clip_layer))
        self._ws = _Workspace(device)

    def alloc_patches(self, n: int) -> torch.Tensor:
        """im2col patch rows of n images [n, (size / patch)^2, K_pad] bf16 (what preprocess writes and encode reads)."""
        g = self.image_size // self.patch
        return torch.empty(n, g * g, self.k_pad, dtype=BF, device=self.device)

    def preprocess(self, img: torch.Tensor, strides: Tuple[int, int, int, int], a: float, b: float, out: torch.Tensor, H: int, W: int,
                   n: int = 1) -> torch.Tensor:
        """rf_clip_preprocess of n images read through element strides (image, row, pixel, channel) from `img` (bf16, on the device;
        its data pointer is image 0, row 0, pixel 0, channel 0) into `out` (alloc_patches rows): level = rint(255 clamp(a v + b, 0, 1)),
        then CLIPImageProcessor's resize / crop / normalise."""
        if not (img.is_cuda and out.is_cuda) or img.dtype != BF:
            raise RFError("HipClipVisionEncoder.preprocess: needs bf16 tensors on the device")
        si, sr, sp, sc = (int(s) for s in strides)
        L.check(L.load().rf_clip_preprocess(img.data_ptr(), si, sr, sp, sc, n, H, W, a, b, self.image_size, self.patch, out.data_ptr(), stream_ptr()),
                "rf_clip_preprocess")
        return out

    def preprocess_levels(self, levels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, 3, H, W] (or [3, H, W]) 8-bit levels (any dtype holding 0 .. 255, e.g. a PNG's uint8) -> patch rows [B, np, K_pad]."""
        x = levels[None] if levels.dim() == 3 else levels
        x = x.to(self.device, BF).contiguous()                          # integers <= 256 are exact in bf16
        B, _, H, W = x.shape
        out = self.alloc_patches(B) if out is None else out
        return self.preprocess(x, (3 * H * W, W, 1, H * W), 1.0 / 255.0, 0.0, out, H, W, B)

    @torch.no_grad()
    def encode(self, patches: torch.Tensor) -> torch.Tensor:
        """patch rows [B, np, K_pad] -> image_embeds [B, projection_dim] bf16 (up to 64 images per launch sequence)."""
        if not patches.is_cuda:
            raise RFError("HipClipVisionEncoder.encode: patches are on the CPU; the HIP path has no CPU fallback")
        B = patches.shape[0]
        lib, w = L.load(), self._w
        patches = patches.contiguous()
        out = torch.empty(B, self.proj_dim, dtype=BF, device=self.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            o = C.byref(self._opts)
            ws = self._ws.get(_ws_bytes(lib.rf_clip_vision_workspace_bytes_opts(C.byref(w), o, nb), "rf_clip_vision_workspace_bytes_opts"))
            L.check(lib.rf_clip_vision_encode_opts(C.byref(w), o, patches[b0].data_ptr(), nb, out[b0].data_ptr(), C.byref(ws), stream_ptr()),
                    "rf_clip_vision_encode_opts")
        return out


def clip_score(image_embeds: torch.Tensor, text_embed: torch.Tensor, logit_scale: float) -> torch.Tensor:
    """rf_clip_score: exp(logit_scale) * cos(image_embeds[b], text_embed) -> f32 [B] on the device."""
    img = image_embeds.to(BF).contiguous()
    txt = text_embed.reshape(-1).to(BF).contiguous()
    B, P = img.shape
    if txt.numel() != P or not (img.is_cuda and txt.is_cuda):
        raise RFError(f"clip_score: image embeds {tuple(img.shape)} vs text embed {tuple(text_embed.shape)} (both on the device)")
    out = torch.empty(B, dtype=torch.float32, device=img.device)
    if B:
        L.check(L.load().rf_clip_score(img.data_ptr(), txt.data_ptr(), float(logit_scale), out.data_ptr(), B, P, stream_ptr()), "rf_clip_score")
    return out


class HipTextEncoders:
    """`pipe.text_encoder` for flux/pipeline.py, i.e. FluxPipeline.encode_prompt's two encoder calls.
    Contract of the pipeline: `te(prompt: str, max_sequence_length, dtype, device) -> (prompt_embeds [L, D_t5], pooled [D_clip])`;
    `encode_t5` / `encode_clip` run one tower only (encode_prompt gives T5 `prompt_2` and CLIP `prompt`).  A list of prompts returns
    batched tensors.  `tokenize(prompts: list[str], max_sequence_length) -> (t5_ids [B, L], clip_ids [B, 77])` is the caller's (T5's
    SentencePiece model and CLIP's BPE vocabulary are files this repo does not ship)."""

    def __init__(self, t5: HipT5Encoder, clip: HipClipTextEncoder, tokenize: Callable):
        self.t5, self.clip, self._tokenize = t5, clip, tokenize
        self._memo = None          # (prompts, L) -> ids of the last tokenize() call

    def tokenize(self, prompts, max_sequence_length: int):
        """The caller's tokenizer runs BOTH towers' vocabularies per call; encode_prompt asks for the T5 ids (L = max_sequence_length)
        and the CLIP ids (L = 77) of the same prompts one after the other -- the T5 pass is memoised per prompt list so that one
        encode_prompt costs one SentencePiece pass at the T5 length, not two passes of each tokenizer."""
        key = (tuple(prompts), int(max_sequence_length))
        if self._memo is not None and self._memo[0] == key:
            return self._memo[1]
        out = self._tokenize(list(prompts), max_sequence_length)
        self._memo = (key, out)
        return out

    def encode_t5(self, prompt, max_sequence_length: int, dtype, device):
        single = isinstance(prompt, str)
        t5_ids, _ = self.tokenize([prompt] if single else list(prompt), max_sequence_length)
        pe = self.t5.encode(t5_ids.to(device)).to(dtype)
        return pe[0] if single else pe

    def encode_clip(self, prompt, dtype, device):
        single = isinstance(prompt, str)
        prompts = [prompt] if single else list(prompt)
        # CLIP ids do not depend on the T5 length: reuse the ids of the T5 call on the same prompts when there was one
        if self._memo is not None and self._memo[0][0] == tuple(prompts):
            clip_ids = self._memo[1][1]
        else:
            clip_ids = self.tokenize(prompts, 77)[1]
        pooled = self.clip.encode(clip_ids.to(device))[1].to(dtype)
        return pooled[0] if single else pooled

    def __call__(self, prompt, max_sequence_length: int, dtype, device):
        return self.encode_t5(prompt, max_sequence_length, dtype, device), self.encode_clip(prompt, dtype, device)


# ---- SigLIP towers (csrc/siglip.hip): transformers' SiglipModel state dict -> rf_siglip_vision_weights / rf_siglip_text_weights --------
SIGLIP_HEAD = 80           # the attention kernels' head dim: every head of d <= 80 channels is zero-padded to it, which is exact


def _pad_rows_per_head(w: torch.Tensor, heads: int, d: int) -> torch.Tensor:
    """[heads * d, ...] -> [heads * 80, ...]: rows 80 h + d .. 80 h + 79 of every head zero"""
    tail = w.shape[1:]
    out = torch.zeros(heads, SIGLIP_HEAD, *tail, dtype=w.dtype)
    out[:, :d] = w.reshape(heads, d, *tail)
    return out.reshape(heads * SIGLIP_HEAD, *tail)


def _pad_rows(w: torch.Tensor, n: int) -> torch.Tensor:
    return w if w.shape[0] == n else torch.cat([w, torch.zeros(n - w.shape[0], *w.shape[1:], dtype=w.dtype)], 0)


def siglip_head_dim(who: str, hidden: int, heads: int) -> int:
    d = hidden // max(heads, 1)
    if heads <= 0 or d * heads != hidden:
        raise RFError(f"{who}: hidden {hidden} is not a multiple of {heads} heads")
    if d > SIGLIP_HEAD:
        raise RFError(f"{who}: head dim {d} > {SIGLIP_HEAD}: the attention kernels serve head dims up to {SIGLIP_HEAD} (zero-padded)")
    if d % 8:
        raise RFError(f"{who}: head dim {d} is not a multiple of 8")
    return d


def siglip_pack_mlp(fc1_w, fc1_b, fc2_w, fc2_b) -> Dict[str, torch.Tensor]:
    """intermediate_size padded to a multiple of 64 with zero fc1 rows / biases and zero fc2 columns: gelu(0) = 0 keeps it exact"""
    f = lambda t: t.detach().float().cpu()  # noqa: E731
    F = fc1_w.shape[0]
    Fp = (F + 63) // 64 * 64
    return dict(w_fc1=_pad_rows(f(fc1_w), Fp), b_fc1=_pad_rows(f(fc1_b), Fp), w_fc2=_pad_rows(f(fc2_w).t().contiguous(), Fp).t().contiguous(),
                b_fc2=f(fc2_b))


def siglip_pack_layers(sd: Dict[str, torch.Tensor], n_layers: int, heads: int) -> List[Dict[str, torch.Tensor]]:
    """The encoder layers of a SigLIP tower (`encoder.layers.N.*` keys, prefix stripped) as fp32 CPU tensors in the packed form
    include/rf_flux.h documents: heads padded d -> 80 (zero q / k / v rows and biases, zero out_proj columns), 1/sqrt(d) of the true d
    folded into q, v bias folded into the out-projection bias, intermediate size padded to a multiple of 64.  Pure repacking: the
    layer computes what the unpacked one does up to fp32 round-off (tests/test_siglip_cpu.py)."""
    f = lambda t: t.detach().float().cpu()  # noqa: E731
    out = []
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        D = sd[p + "self_attn.q_proj.weight"].shape[1]
        d = siglip_head_dim("siglip_pack_layers", D, heads)
        qs = d ** -0.5
        wq, bq = f(sd[p + "self_attn.q_proj.weight"]) * qs, f(sd[p + "self_attn.q_proj.bias"]) * qs
        wk, bk = f(sd[p + "self_attn.k_proj.weight"]), f(sd[p + "self_attn.k_proj.bias"])
        wv, bv = f(sd[p + "self_attn.v_proj.weight"]), f(sd[p + "self_attn.v_proj.bias"])
        wo, bo = f(sd[p + "self_attn.out_proj.weight"]), f(sd[p + "self_attn.out_proj.bias"])
        y = dict(ln1_w=f(sd[p + "layer_norm1.weight"]), ln1_b=f(sd[p + "layer_norm1.bias"]),
                 ln2_w=f(sd[p + "layer_norm2.weight"]), ln2_b=f(sd[p + "layer_norm2.bias"]),
                 w_qk=torch.cat([_pad_rows_per_head(wq, heads, d), _pad_rows_per_head(wk, heads, d)], 0),
                 b_qk=torch.cat([_pad_rows_per_head(bq, heads, d), _pad_rows_per_head(bk, heads, d)], 0),
                 w_v=_pad_rows_per_head(wv, heads, d),
                 w_o=_pad_rows_per_head(wo.t().contiguous(), heads, d).t().contiguous(),
                 b_o=bo + wo @ bv)
        y.update(siglip_pack_mlp(sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]))
        out.append(y)
    return out


def siglip_pack_pool_head(sd: Dict[str, torch.Tensor], heads: int) -> Dict[str, torch.Tensor]:
    """SiglipMultiheadAttentionPoolingHead (`head.*` keys): K | V projection, the probe's query (input-independent: computed here once,
    1/sqrt(d) folded in), out_proj, layernorm, the padded MLP"""
    f = lambda t: t.detach().float().cpu()  # noqa: E731
    wi, bi = f(sd["head.attention.in_proj_weight"]), f(sd["head.attention.in_proj_bias"])
    D = wi.shape[1]
    d = siglip_head_dim("siglip_pack_pool_head", D, heads)
    probe = f(sd["head.probe"]).reshape(D)
    y = dict(probe_q=(wi[:D] @ probe + bi[:D]) * d ** -0.5, w_kv=wi[D:].contiguous(), b_kv=bi[D:].contiguous(),
             w_po=f(sd["head.attention.out_proj.weight"]), b_po=f(sd["head.attention.out_proj.bias"]),
             hln_w=f(sd["head.layernorm.weight"]), hln_b=f(sd["head.layernorm.bias"]))
    y.update(siglip_pack_mlp(sd["head.mlp.fc1.weight"], sd["head.mlp.fc1.bias"], sd["head.mlp.fc2.weight"], sd["head.mlp.fc2.bias"]))
    return y


def _siglip_layer_structs(k: "_Keep", packed: List[Dict[str, torch.Tensor]]) -> "C.Array":
    layers = (L.rf_clip_layer * len(packed))()
    for y, p in zip(layers, packed):
        y.ln1_scale, y.ln1_shift = k.t(p["ln1_w"] - 1.0), k.t(p["ln1_b"])
        y.ln2_scale, y.ln2_shift = k.t(p["ln2_w"] - 1.0), k.t(p["ln2_b"])
        y.w_qk, y.b_qk, y.w_v = k.t(_kpad(p["w_qk"])), k.t(p["b_qk"]), k.t(_kpad(p["w_v"]))
        y.w_o, y.b_o = k.t(_kpad(p["w_o"])), k.t(p["b_o"])
        y.w_fc1, y.b_fc1, y.w_fc2, y.b_fc2 = k.t(_kpad(p["w_fc1"])), k.t(p["b_fc1"]), k.t(p["w_fc2"]), k.t(p["b_fc2"])
    return layers


def _count_layers(sd, who):
    n = 0
    while f"encoder.layers.{n}.layer_norm1.weight" in sd:
        n += 1
    if n == 0:
        raise RFError(f"{who}: no encoder.layers.* keys in the state dict")
    return n


class HipSiglipVisionEncoder:
    """SiglipVisionModel of a Hugging Face `SiglipModel` state dict (`vision_model.*`; the prefix may be absent): images ->
    pooler_output [B, hidden] bf16 (rf_siglip_preprocess + rf_siglip_vision_encode).  The interface of HipClipVisionEncoder."""

    MAX_BATCH = 64

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, device, eps: float = 1e-6, image_size: Optional[int] = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RFError(f"HipSiglipVisionEncoder: device {device}; the HIP path has no CPU fallback")
        L.load()
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state_dict.items()}
        n_layers = _count_layers(sd, "HipSiglipVisionEncoder")
        pw = sd["embeddings.patch_embedding.weight"]                     # [hidden, 3, p, p]
        D, _, P, _ = pw.shape
        d = siglip_head_dim("HipSiglipVisionEncoder", D, num_heads)
        T = sd["embeddings.position_embedding.weight"].shape[0]
        g = int(round(math.sqrt(T)))
        if g * g != T:
            raise RFError(f"HipSiglipVisionEncoder: {T} positions is not a square grid")
        if image_size is not None and int(image_size) // P != g:
            raise RFError(f"HipSiglipVisionEncoder: image_size {image_size} with patch {P} needs {(int(image_size) // P) ** 2} position rows, "
                          f"the state dict has {T} (a {g * P}-pixel tower)")
        # the patch convolution is "valid": so400m/14 at 384 px has 27 x 27 patches over 378 of its 384 pixels
        self.device, self.heads, self.hidden, self.patch, self.image_size = device, num_heads, D, P, int(image_size) if image_size is not None else g * P
        self.tokens, self.s_pad, self.k_pad, self.proj_dim = T, _pad32(T), (3 * P * P + 63) // 64 * 64, D
        k = self._k = _Keep(device)
        f = lambda t: t.detach().float()  # noqa: E731
        packed = siglip_pack_layers(sd, n_layers, num_heads)
        self._layers = _siglip_layer_structs(k, packed)
        hp = siglip_pack_pool_head(sd, num_heads)
        wpad = torch.zeros(D, self.k_pad)
        wpad[:, : 3 * P * P] = f(pw).reshape(D, 3 * P * P).cpu()
        w = self._w = L.rf_siglip_vision_weights()
        w.layers, w.hidden, w.heads, w.head_dim, w.inter = n_layers, D, num_heads, d, packed[0]["w_fc1"].shape[0]
        w.image_size, w.patch, w.mask_S, w.eps = self.image_size, P, self.s_pad, eps
        w.patch_w, w.patch_b = k.t(wpad), k.t(sd["embeddings.patch_embedding.bias"])
        w.pos_embed = k.t(sd["embeddings.position_embedding.weight"])
        w.post_ln_scale, w.post_ln_shift = k.t(f(sd["post_layernorm.weight"]) - 1.0), k.t(sd["post_layernorm.bias"])
        self._mask = None
        if self.s_pad != T:
            mask = torch.zeros(self.s_pad, self.s_pad, device=device)
            mask[:, T:] = float("-inf")
            self._mask = mask.contiguous()
            w.mask = self._mask.data_ptr()
        w.layer = C.cast(self._layers, C.POINTER(L.rf_clip_layer))
        if hp["w_fc1"].shape[0] != w.inter:
            raise RFError("HipSiglipVisionEncoder: the pooling head's MLP and the layers' MLP differ in width")
        w.w_kv, w.b_kv, w.probe_q = k.t(_kpad(hp["w_kv"])), k.t(hp["b_kv"]), k.t(hp["probe_q"], torch.float32)
        w.w_po, w.b_po = k.t(_kpad(hp["w_po"])), k.t(hp["b_po"])
        w.hln_scale, w.hln_shift = k.t(hp["hln_w"] - 1.0), k.t(hp["hln_b"])
        w.w_hfc1, w.b_hfc1, w.w_hfc2, w.b_hfc2 = k.t(_kpad(hp["w_fc1"])), k.t(hp["b_fc1"]), k.t(hp["w_fc2"]), k.t(hp["b_fc2"])
        self._ws = _Workspace(device)

    def alloc_patches(self, n: int) -> torch.Tensor:
        return torch.empty(n, self.tokens, self.k_pad, dtype=BF, device=self.device)

    def preprocess(self, img: torch.Tensor, strides: Tuple[int, int, int, int], a: float, b: float, out: torch.Tensor, H: int, W: int,
                   n: int = 1) -> torch.Tensor:
        """rf_siglip_preprocess of n images read through element strides (image, row, pixel, channel): level = rint(255 clamp(a v + b,
        0, 1)), then SiglipImageProcessor's resize of both axes to image_size and (v / 255 - 0.5) / 0.5."""
        if not (img.is_cuda and out.is_cuda) or img.dtype != BF:
            raise RFError("HipSiglipVisionEncoder.preprocess: needs bf16 tensors on the device")
        si, sr, sp, sc = (int(s) for s in strides)
        L.check(L.load().rf_siglip_preprocess(img.data_ptr(), si, sr, sp, sc, n, H, W, a, b, self.image_size, self.patch, out.data_ptr(), stream_ptr()),
                "rf_siglip_preprocess")
        return out

    def preprocess_levels(self, levels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, 3, H, W] (or [3, H, W]) 8-bit levels -> patch rows [B, T, K_pad]."""
        x = levels[None] if levels.dim() == 3 else levels
        x = x.to(self.device, BF).contiguous()                          # integers <= 256 are exact in bf16
        B, _, H, W = x.shape
        out = self.alloc_patches(B) if out is None else out
        return self.preprocess(x, (3 * H * W, W, 1, H * W), 1.0 / 255.0, 0.0, out, H, W, B)

    def workspace_bytes(self, nb: int) -> int:
        return _ws_bytes(L.load().rf_siglip_vision_workspace_bytes(C.byref(self._w), nb), "rf_siglip_vision_workspace_bytes")

    @torch.no_grad()
    def encode(self, patches: torch.Tensor) -> torch.Tensor:
        """patch rows [B, T, K_pad] -> pooler_output [B, hidden] bf16 (up to 64 images per launch sequence)."""
        if not patches.is_cuda:
            raise RFError("HipSiglipVisionEncoder.encode: patches are on the CPU; the HIP path has no CPU fallback")
        B = patches.shape[0]
        lib, w = L.load(), self._w
        patches = patches.contiguous()
        out = torch.empty(B, self.hidden, dtype=BF, device=self.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            ws = self._ws.get(self.workspace_bytes(nb))
            L.check(lib.rf_siglip_vision_encode(C.byref(w), patches[b0].data_ptr(), nb, out[b0].data_ptr(), C.byref(ws), stream_ptr()),
                    "rf_siglip_vision_encode")
        return out


class HipSiglipTextEncoder:
    """SiglipTextModel of a `SiglipModel` state dict (`text_model.*`): ids [B, S] -> pooler_output [B, projection_size] bf16 =
    head(final_layer_norm(x)[:, S - 1]).  No causal mask; S = 64 (max_length padding) for every published checkpoint."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int, device, eps: float = 1e-6):
        device = torch.device(device)
        if device.type != "cuda":
            raise RFError(f"HipSiglipTextEncoder: device {device}; the HIP path has no CPU fallback")
        L.load()
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}
        n_layers = _count_layers(sd, "HipSiglipTextEncoder")
        D = sd["embeddings.token_embedding.weight"].shape[1]
        d = siglip_head_dim("HipSiglipTextEncoder", D, num_heads)
        self.device, self.heads, self.hidden, self.proj_dim = device, num_heads, D, sd["head.weight"].shape[0]
        k = self._k = _Keep(device)
        f = lambda t: t.detach().float()  # noqa: E731
        packed = siglip_pack_layers(sd, n_layers, num_heads)
        self._layers = _siglip_layer_structs(k, packed)
        w = self._w = L.rf_siglip_text_weights()
        w.layers, w.hidden, w.heads, w.head_dim, w.inter = n_layers, D, num_heads, d, packed[0]["w_fc1"].shape[0]
        w.vocab, w.max_pos = sd["embeddings.token_embedding.weight"].shape[0], sd["embeddings.position_embedding.weight"].shape[0]
        w.proj_dim, w.eps = self.proj_dim, eps
        w.tok_embed, w.pos_embed = k.t(sd["embeddings.token_embedding.weight"]), k.t(sd["embeddings.position_embedding.weight"])
        w.final_ln_scale, w.final_ln_shift = k.t(f(sd["final_layer_norm.weight"]) - 1.0), k.t(sd["final_layer_norm.bias"])
        w.head_w, w.head_b = k.t(_kpad(sd["head.weight"])), k.t(sd["head.bias"])
        w.layer = C.cast(self._layers, C.POINTER(L.rf_clip_layer))
        self._mask: Dict[int, torch.Tensor] = {}
        self._ws = _Workspace(device)

    def workspace_bytes(self, nb: int, S: int) -> int:
        return _ws_bytes(L.load().rf_siglip_text_workspace_bytes(C.byref(self._w), nb, S), "rf_siglip_text_workspace_bytes")

    @torch.no_grad()
    def encode(self, ids: torch.Tensor) -> torch.Tensor:
        if not ids.is_cuda:
            raise RFError("HipSiglipTextEncoder.encode: ids are on the CPU; the HIP path has no CPU fallback")
        B, S = ids.shape
        lib, w = L.load(), self._w
        sp = _pad32(S)
        w.mask, w.mask_S = None, sp
        if sp != S:                                  # padded keys masked; never a causal mask
            if S not in self._mask:
                m = torch.zeros(sp, sp, device=self.device)
                m[:, S:] = float("-inf")
                self._mask[S] = m.contiguous()
            w.mask = self._mask[S].data_ptr()
        ids32 = ids.to(torch.int32).contiguous()
        out = torch.empty(B, self.proj_dim, dtype=BF, device=self.device)
        for b0 in range(0, B, 64):
            nb = min(64, B - b0)
            ws = self._ws.get(self.workspace_bytes(nb, S))
            L.check(lib.rf_siglip_text_encode(C.byref(w), ids32[b0].data_ptr(), nb, S, out[b0].data_ptr(), C.byref(ws), stream_ptr()),
                    "rf_siglip_text_encode")
        return out


def siglip_score(image_embeds: torch.Tensor, text_embed: torch.Tensor, logit_scale: float, logit_bias: float,
                 threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """rf_siglip_score: (sigmoid(exp(logit_scale) cos(image_embeds[b], text_embed) + logit_bias) f32 [B], labels i32 [B] = score >=
    threshold), both on the device."""
    img = image_embeds.to(BF).contiguous()
    txt = text_embed.reshape(-1).to(BF).contiguous()
    B, P = img.shape
    if txt.numel() != P or not (img.is_cuda and txt.is_cuda):
        raise RFError(f"siglip_score: image embeds {tuple(img.shape)} vs text embed {tuple(text_embed.shape)} (both on the device)")
    out = torch.empty(B, dtype=torch.float32, device=img.device)
    lab = torch.empty(B, dtype=torch.int32, device=img.device)
    if B:
        L.check(L.load().rf_siglip_score(img.data_ptr(), txt.data_ptr(), float(logit_scale), float(logit_bias), float(threshold), out.data_ptr(),
                                         lab.data_ptr(), B, P, stream_ptr()), "rf_siglip_score")
    return out, lab
