"""On-device SigLIP score verifier for the reflection search: the verifier of the CLIP family that can give a LABEL.

The reference's search sorts candidates on a yes / no label first and a score second (`nvila_sort_key`, tts/search.py).  A contrastive
cosine has no natural threshold; SigLIP's pairwise sigmoid has:

    p = sigmoid(exp(logit_scale) * cos(SiglipVisionModel(SiglipImageProcessor(png)).pooled, SiglipTextModel(prompt).pooled) + logit_bias)

is a calibrated match probability (the diagonal of HF's `sigmoid(logits_per_image)`), so `label = p >= threshold`
(`verifier_args.threshold`, default 0.5) is a principled label and the kind "siglip" sorts with `nvila_sort_key`.
google/siglip-so400m-patch14-384 (hidden 1152 = 16 heads x 72, 729 tokens) is also the vision tower inside NVILA / VILA.

`SiglipScoreVerifier` has `ClipScoreVerifier`'s surface and data path: HIP VAE decode -> rf_siglip_preprocess (reads the decoder's
zero-halo NHWC output in place) -> rf_siglip_vision_encode (one call per rank and round) -> rf_siglip_score; an `--imgpath` pool of
PNG files goes through the same kernels from its uint8 levels, so a PNG and the latents it was written from score bit-identically.
The text embedding is cached per prompt.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import torch

from ..flux.text_hip import HipSiglipTextEncoder, HipSiglipVisionEncoder, siglip_score
from ..ops import RFError

TEXT_LENGTH = 64            # max_length padding: how every published SigLIP checkpoint was trained

# google/siglip-so400m-patch14-384: 27 x 27 = 729 tokens (S_pad 736: the head-dim-80 streaming-keys attention), head dim 72
SO400M_384 = dict(text=dict(vocab=32000, hidden=1152, heads=16, inter=4304, layers=27, max_pos=64),
                  vision=dict(hidden=1152, heads=16, inter=4304, layers=27, image_size=384, patch=14), projection_dim=1152)
# google/siglip-so400m-patch14-224: 256 tokens, keys resident in the LDS
SO400M_224 = dict(text=SO400M_384["text"], vision=dict(SO400M_384["vision"], image_size=224), projection_dim=1152)
# google/siglip-base-patch16-224: head dim 64, through the same padded path
BASE_224 = dict(text=dict(vocab=32000, hidden=768, heads=12, inter=3072, layers=12, max_pos=64),
                vision=dict(hidden=768, heads=12, inter=3072, layers=12, image_size=224, patch=16), projection_dim=768)
# --synthetic --small: 2 layers per tower, 2 heads of the same head dim, an intermediate size that is no multiple of 64 where the full one is none
TINY_SO400M_384 = dict(text=dict(vocab=512, hidden=144, heads=2, inter=272, layers=2, max_pos=64),
                       vision=dict(hidden=144, heads=2, inter=272, layers=2, image_size=384, patch=14), projection_dim=144)
TINY_SO400M_224 = dict(text=TINY_SO400M_384["text"], vision=dict(TINY_SO400M_384["vision"], image_size=224), projection_dim=144)
TINY_BASE_224 = dict(text=dict(vocab=512, hidden=128, heads=2, inter=256, layers=2, max_pos=64),
                     vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=16), projection_dim=128)
GEOMETRIES = {"so400m_384": (SO400M_384, TINY_SO400M_384), "so400m_224": (SO400M_224, TINY_SO400M_224), "base_224": (BASE_224, TINY_BASE_224)}
HIDDEN_ACT = "gelu_pytorch_tanh"


def geometry_names() -> List[str]:
    return sorted(GEOMETRIES)


def geometry(name: str) -> tuple:
    """verifier_args.geometry -> (full table, its --small form)"""
    if name not in GEOMETRIES:
        raise RFError(f"verifier_args.geometry {name!r} (one of {geometry_names()})")
    return GEOMETRIES[name]


def tower_config(cfg: dict) -> dict:
    """SiglipScoreVerifier's `model_config` of a geometry table"""
    return dict(text_heads=cfg["text"]["heads"], vision_heads=cfg["vision"]["heads"], hidden_act=HIDDEN_ACT, layer_norm_eps=1e-6,
                image_size=cfg["vision"]["image_size"], patch_size=cfg["vision"]["patch"])


class SiglipScoreVerifier:
    """`score_batch(latents [n, S, 64], seeds, prompt) -> (scores f32 [n], labels i32 [n])`, `score_decoded` and `score_images(paths,
    prompt)` for runner.run_reflection_search.  `state_dict`: an HF SiglipModel state dict (`text_model.*`, `vision_model.*`,
    `logit_scale`, `logit_bias`); `tokenize(prompts) -> ids [B, 64]`; `model_config`: `read_siglip_config`'s dict (head counts, eps,
    image_size); `threshold`: labels are `score >= threshold`."""

    def __init__(self, pipe, state_dict: Dict[str, torch.Tensor], tokenize: Callable[[List[str]], torch.Tensor], height: int, width: int,
                 model_config: dict, threshold: float = 0.5):
        from ..flux.vae_hip import HipVAE
        if pipe.vae is None:
            raise RFError("SiglipScoreVerifier: the pipeline has no VAE -- the verifier scores decoded images")
        if not isinstance(pipe.vae, HipVAE):
            raise RFError("SiglipScoreVerifier: the pipeline's VAE is not the HIP VAE; call pipe.enable_hip_vae() first")
        if not 0.0 <= float(threshold) <= 1.0:
            raise RFError(f"SiglipScoreVerifier: threshold {threshold} is not a probability")
        self.pipe, self.height, self.width, self._tokenize = pipe, int(height), int(width), tokenize
        sd, dev, mc = state_dict, pipe.device, dict(model_config)
        text = {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}
        vision = {k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}
        if not text or not vision or "logit_scale" not in sd or "logit_bias" not in sd:
            raise RFError("SiglipScoreVerifier: needs a SiglipModel state dict (text_model.*, vision_model.*, logit_scale, logit_bias)")
        if mc.get("hidden_act", HIDDEN_ACT) != HIDDEN_ACT:
            raise RFError(f"SiglipScoreVerifier: hidden_act {mc['hidden_act']!r}; the SigLIP towers run {HIDDEN_ACT!r} only")
        eps = float(mc.get("layer_norm_eps", 1e-6))
        self.text = HipSiglipTextEncoder(text, int(mc["text_heads"]), dev, eps=eps)
        self.vision = HipSiglipVisionEncoder(vision, int(mc["vision_heads"]), dev, eps=eps, image_size=mc.get("image_size"))
        if self.text.proj_dim != self.vision.hidden:
            raise RFError(f"SiglipScoreVerifier: text projection_size {self.text.proj_dim} != vision hidden {self.vision.hidden}")
        self.logit_scale, self.logit_bias = float(sd["logit_scale"].float().reshape(-1)[0]), float(sd["logit_bias"].float().reshape(-1)[0])
        self.threshold = float(threshold)
        self._text_cache: Dict[str, torch.Tensor] = {}

    # ---- text side -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def text_embed(self, prompt: str) -> torch.Tensor:
        """SiglipTextModel(prompt).pooler_output [projection_size] bf16, cached per prompt."""
        if prompt not in self._text_cache:
            ids = torch.as_tensor(self._tokenize([prompt])).to(self.pipe.device)
            emb = self.text.encode(ids)[0]
            if len(self._text_cache) >= 64:
                self._text_cache.pop(next(iter(self._text_cache)))
            self._text_cache[prompt] = emb
        return self._text_cache[prompt]

    # ---- image side ----------------------------------------------------------------------------------------------------------
    def _decode_into(self, latents: torch.Tensor, patches: torch.Tensor, row: int) -> None:
        pipe = self.pipe
        z = pipe._unpack_latents(latents, self.height, self.width, pipe.vae_scale_factor)
        z = z / pipe.vae.config.scaling_factor + pipe.vae.config.shift_factor
        self._halo_into(pipe.vae.decode_halo(z)[0], patches, row)

    def _halo_into(self, out: torch.Tensor, patches: torch.Tensor, row: int) -> None:
        """the decoder's output [(H + 2), (W + 2), cout] (image at the interior, channels 0..2), read in place -> patch rows of image `row`."""
        Hp, Wp, cout = out.shape
        interior = out[1:, 1:]
        self.vision.preprocess(interior, (0, Wp * cout, cout, 1), 0.5, 0.5, patches[row:row + 1], Hp - 2, Wp - 2)

    @torch.no_grad()
    def score_batch(self, latents: torch.Tensor, seeds: Sequence[int], prompt: str, decoded=None):
        """This rank's candidates of a round: packed latents [n, S, 64] -> (scores f32 [n], labels i32 [n]) on the device; one vision
        call for all n.  `decoded`: the candidates' HipVAE.decode_halo outputs, in row order, if the caller has them."""
        if decoded is not None:
            if len(decoded) != latents.shape[0]:
                raise RFError(f"SiglipScoreVerifier.score_batch: {latents.shape[0]} candidates but {len(decoded)} decoded buffers")
            return self.score_decoded(decoded, prompt)
        n = latents.shape[0]
        patches = self.vision.alloc_patches(n)
        for b in range(n):
            self._decode_into(latents[b:b + 1], patches, b)
        return self._score(patches, prompt)

    score_batch.wants_prompt = True
    score_batch.wants_decoded = True

    @torch.no_grad()
    def score_decoded(self, halos, prompt: str):
        patches = self.vision.alloc_patches(len(halos))
        for b, out in enumerate(halos):
            if out.shape[0] - 2 != self.height or out.shape[1] - 2 != self.width:
                raise RFError(f"SiglipScoreVerifier.score_decoded: buffer {tuple(out.shape)} is not a decoded {self.height}x{self.width} image")
            self._halo_into(out, patches, b)
        return self._score(patches, prompt)

    @torch.no_grad()
    def score_images(self, paths: Sequence[str], prompt: str):
        """An `--imgpath` pool: PNG files (their uint8 levels) or the runner's `.pt` packed latents -> (f32 [n], i32 [n])."""
        patches = self.vision.alloc_patches(len(paths))
        for b, p in enumerate(paths):
            if p.endswith(".pt"):
                self._decode_into(torch.load(p).to(self.pipe.device, self.pipe.dtype), patches, b)
                continue
            import numpy as np
            from PIL import Image
            arr = np.asarray(Image.open(p).convert("RGB"))
            lv = torch.from_numpy(arr.copy()).to(self.pipe.device).permute(2, 0, 1)
            self.vision.preprocess_levels(lv, out=patches[b:b + 1])
        return self._score(patches, prompt)

    def _score(self, patches: torch.Tensor, prompt: str):
        n = patches.shape[0]
        dev = self.pipe.device
        if n == 0:
            return torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        emb = self.vision.encode(patches)
        return siglip_score(emb, self.text_embed(prompt), self.logit_scale, self.logit_bias, self.threshold)


# ---- synthetic model + tokenizer (no checkpoint offline) ------------------------------------------------------------------------
def synthetic_siglip_state(cfg: dict = SO400M_384, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A seeded random-init HF SiglipModel state dict of the given geometry (fp32, CPU), with `synthetic_clip_state`'s rules: weights
    N(0, 1/fan_in) (q / k x 2 so that attention is not uniform), LayerNorm weights 1 + N(0, 0.1^2), biases N(0, 0.1^2), embeddings and
    the probe N(0, 0.2^2); logit_scale = log 10 and logit_bias = -10, SigLIP's init."""
    t, v, P = cfg["text"], cfg["vision"], cfg["projection_dim"]
    if P != v["hidden"]:
        raise RFError(f"synthetic_siglip_state: projection_dim {P} != vision hidden {v['hidden']} (SigLIP's image embedding is the pooled hidden state)")
    Dv = v["hidden"]
    shapes = {"text_model.embeddings.token_embedding.weight": (t["vocab"], t["hidden"]),
              "text_model.embeddings.position_embedding.weight": (t["max_pos"], t["hidden"]),
              "text_model.final_layer_norm.weight": (t["hidden"],), "text_model.final_layer_norm.bias": (t["hidden"],),
              "text_model.head.weight": (P, t["hidden"]), "text_model.head.bias": (P,),
              "vision_model.embeddings.patch_embedding.weight": (Dv, 3, v["patch"], v["patch"]),
              "vision_model.embeddings.patch_embedding.bias": (Dv,),
              "vision_model.embeddings.position_embedding.weight": ((v["image_size"] // v["patch"]) ** 2, Dv),
              "vision_model.post_layernorm.weight": (Dv,), "vision_model.post_layernorm.bias": (Dv,),
              "vision_model.head.probe": (1, 1, Dv),
              "vision_model.head.attention.in_proj_weight": (3 * Dv, Dv), "vision_model.head.attention.in_proj_bias": (3 * Dv,),
              "vision_model.head.attention.out_proj.weight": (Dv, Dv), "vision_model.head.attention.out_proj.bias": (Dv,),
              "vision_model.head.layernorm.weight": (Dv,), "vision_model.head.layernorm.bias": (Dv,),
              "vision_model.head.mlp.fc1.weight": (v["inter"], Dv), "vision_model.head.mlp.fc1.bias": (v["inter"],),
              "vision_model.head.mlp.fc2.weight": (Dv, v["inter"]), "vision_model.head.mlp.fc2.bias": (Dv,)}
    for tower, c in (("text_model", t), ("vision_model", v)):
        D, F = c["hidden"], c["inter"]
        for i in range(c["layers"]):
            p = f"{tower}.encoder.layers.{i}."
            for x in ("q_proj", "k_proj", "v_proj", "out_proj"):
                shapes[p + f"self_attn.{x}.weight"] = (D, D)
                shapes[p + f"self_attn.{x}.bias"] = (D,)
            for nrm in ("layer_norm1", "layer_norm2"):
                shapes[p + nrm + ".weight"] = (D,)
                shapes[p + nrm + ".bias"] = (D,)
            shapes[p + "mlp.fc1.weight"], shapes[p + "mlp.fc1.bias"] = (F, D), (F,)
            shapes[p + "mlp.fc2.weight"], shapes[p + "mlp.fc2.bias"] = (D, F), (D,)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in sorted(shapes):
        x = torch.randn(shapes[k], generator=g)
        if "norm" in k and k.endswith(".weight"):
            x = 1.0 + 0.1 * x
        elif k.endswith("bias"):
            x = 0.1 * x
        elif "position_embedding" in k or "token_embedding" in k or k.endswith("probe"):
            x = 0.2 * x
        else:
            fan_in = math.prod(shapes[k][1:])
            x = x * fan_in ** -0.5 * (2.0 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = x
    sd["logit_scale"] = torch.tensor([math.log(10.0)])
    sd["logit_bias"] = torch.tensor([-10.0])
    return sd


def synthetic_tokenize(vocab: int, length: int = TEXT_LENGTH) -> Callable[[List[str]], torch.Tensor]:
    """Deterministic stand-in for SigLIP's SentencePiece tokenizer (its model file is not shipped): one id per UTF-8 byte
    (3 + byte % (vocab - 5)), then id 1, which is SigLIP's EOS and its pad id alike, up to `length` (padding="max_length": the model
    pools the LAST position, which is padding for every prompt shorter than `length`)."""
    def tokenize(prompts: List[str]) -> torch.Tensor:
        out = torch.full((len(prompts), length), 1, dtype=torch.int64)
        for i, p in enumerate(prompts):
            ids = [3 + b % (vocab - 5) for b in p.encode("utf-8")][: length - 1] + [1]
            out[i, : len(ids)] = torch.tensor(ids)
        return out
    return tokenize


def read_siglip_config(path: str) -> dict:
    """What the verifier needs of an HF SiglipModel directory's config.json: both towers' head counts, hidden_act (anything but
    gelu_pytorch_tanh is refused), layer_norm_eps, the vision tower's image_size and patch_size.  Keys a config leaves out take
    SiglipConfig's defaults (12 heads, 1e-6, 224, 16)."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    t, v = cfg.get("text_config") or {}, cfg.get("vision_config") or {}
    for name, c in (("text", t), ("vision", v)):
        act = c.get("hidden_act", HIDDEN_ACT)
        if act != HIDDEN_ACT:
            raise RFError(f"{path}: {name} hidden_act {act!r}; the SigLIP towers run {HIDDEN_ACT!r} only")
    t_eps, v_eps = float(t.get("layer_norm_eps", 1e-6)), float(v.get("layer_norm_eps", 1e-6))
    if t_eps != v_eps:
        raise RFError(f"{path}: text layer_norm_eps {t_eps} != vision layer_norm_eps {v_eps}")
    return dict(text_heads=int(t.get("num_attention_heads", 12)), vision_heads=int(v.get("num_attention_heads", 12)), hidden_act=HIDDEN_ACT,
                layer_norm_eps=t_eps, image_size=int(v.get("image_size", 224)), patch_size=int(v.get("patch_size", 16)))


def load_siglip_dir(path: str):
    """An HF SiglipModel directory: config.json + model.safetensors + tokenizer files -> (state dict, tokenize, model config).  The
    tokenizer is `AutoTokenizer.from_pretrained(path, local_files_only=True)` with padding="max_length" at 64 tokens.  No SigLIP
    checkpoint or SentencePiece model ships with this repository, so this loader is exercised by no test: only `read_siglip_config` is."""
    mc = read_siglip_config(path)
    from safetensors.torch import load_file
    from transformers import AutoTokenizer
    sd = load_file(os.path.join(path, "model.safetensors"))
    tok = AutoTokenizer.from_pretrained(path, local_files_only=True)

    def tokenize(prompts: List[str]) -> torch.Tensor:
        return tok(list(prompts), padding="max_length", max_length=TEXT_LENGTH, truncation=True, return_tensors="pt")["input_ids"]
    return sd, tokenize, mc


def build_from_config(config: dict, pipe, synthetic: bool = False, small: bool = False) -> SiglipScoreVerifier:
    """The verifier `verifier_args = {"name": "siglip", "siglip_model_path": DIR, "threshold": 0.5}` names: DIR is an HF SiglipModel
    directory (siglip-so400m-patch14-384, ...).  With `synthetic`: a seeded random-init SigLIP of `verifier_args.geometry`
    ("so400m_384", the default, "so400m_224" or "base_224"; their 2-layer forms with `small`) and the synthetic tokenizer.  Switches
    the pipeline's VAE to the HIP path."""
    va, pa = config.get("verifier_args", {}), config["pipeline_args"]
    if pipe.vae is None:
        raise RFError("the SigLIP verifier needs a pipeline with a VAE")
    pipe.enable_hip_vae()
    threshold = float(va.get("threshold", 0.5))
    if synthetic:
        cfg = geometry(va.get("geometry", "so400m_384"))[1 if small else 0]
        sd, tok, mc = synthetic_siglip_state(cfg, int(va.get("seed", 0))), synthetic_tokenize(cfg["text"]["vocab"]), tower_config(cfg)
    else:
        if not va.get("siglip_model_path"):
            raise RFError('verifier_args.name == "siglip" needs verifier_args.siglip_model_path (an HF SiglipModel directory)')
        sd, tok, mc = load_siglip_dir(va["siglip_model_path"])
    return SiglipScoreVerifier(pipe, sd, tok, pa["height"], pa["width"], model_config=mc, threshold=threshold)
