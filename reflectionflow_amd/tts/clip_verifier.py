"""On-device CLIP-score verifier for the reflection search.

The verifier is transformers' `CLIPModel` (clip-vit-large-patch14 layout, or the ViT-H/14 layout of PickScore / HPSv2 / LAION CLIP-H:
vision head dim 80, `hidden_act = "gelu"`) applied to what the reference's verifier reads -- the
candidate's saved 8-bit PNG -- and scored against the ORIGINAL prompt, as the reference scores every round
(tts_reflectionflow.py:157-170, 345-352):

    score = exp(logit_scale) * cos(visual_projection(ViT(CLIPImageProcessor(png))), text_projection(CLIPTextModel(prompt).pooled))

i.e. the diagonal of HF's `logits_per_image`.  A scalar metric: labels are 1 for every candidate and the kind "clip" sorts with
`search.scalar_sort_key` (descending score, index tie-break), as the reference's scalar ("openai") branch.

The image side never leaves the device: HIP VAE decode -> rf_clip_preprocess (reads the decoder's zero-halo NHWC output in place)
-> rf_clip_vision_encode (one call per rank and round) -> rf_clip_score -> the runner's {f32, i32} all-gather.  An `--imgpath`
pool (PNG files) goes through the same kernels from its uint8 levels, so a PNG and the latents it was written from score
bit-identically.  The text embedding (HIP CLIP text tower + text_projection GEMM) is cached per prompt.

The decode is shared with the runner: `score_batch` carries `wants_decoded`, so on the runner's device hand-off path it is given the
buffers `_save` already decoded (`score_decoded`) and a candidate is decoded once per rank.  Called with latents alone it decodes itself.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import torch

from .. import ops
from ..flux.text_hip import HipClipTextEncoder, HipClipVisionEncoder, clip_score
from ..ops import RFError

# openai/clip-vit-large-patch14
VIT_L14 = dict(text=dict(vocab=49408, hidden=768, heads=12, inter=3072, layers=12, max_pos=77),
               vision=dict(hidden=1024, heads=16, inter=4096, layers=24, image_size=224, patch=14), projection_dim=768)
# --synthetic --small
TINY = dict(text=dict(vocab=512, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
            vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=14), projection_dim=64)
# yuvalkirstain/PickScore_v1, HPSv2, laion/CLIP-ViT-H-14-laion2B-s32B-b79K: one CLIPModel geometry, vision head dim 80, erf GELU
VIT_H14 = dict(text=dict(vocab=49408, hidden=1024, heads=16, inter=4096, layers=24, max_pos=77),
               vision=dict(hidden=1280, heads=16, inter=5120, layers=32, image_size=224, patch=14), projection_dim=1024, act="gelu")
# --synthetic --small with geometry "vit_h14": 2 layers per tower, vision head dim 80, erf GELU
TINY_H = dict(text=dict(vocab=512, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
              vision=dict(hidden=160, heads=2, inter=320, layers=2, image_size=224, patch=14), projection_dim=64, act="gelu")
GEOMETRIES = {"vit_l14": (VIT_L14, TINY), "vit_h14": (VIT_H14, TINY_H)}        # verifier_args.geometry -> (full, --small)
# openai/clip-vit-large-patch14-336: ViT-L/14 at 336 px, 24 x 24 + 1 = 577 tokens (S_pad 608: the streaming-keys attention kernel)
VIT_L14_336 = dict(text=VIT_L14["text"], vision=dict(VIT_L14["vision"], image_size=336), projection_dim=768)
# --synthetic --small with geometry "vit_l14_336": 2 layers per tower, 577 vision tokens
TINY_336 = dict(text=TINY["text"], vision=dict(TINY["vision"], image_size=336), projection_dim=64)
# the geometries whose vision tower has more keys than the LDS holds (a table of its own: GEOMETRIES is the resident-keys set)
GEOMETRIES_STREAMED = {"vit_l14_336": (VIT_L14_336, TINY_336)}


def geometry_names() -> List[str]:
    """every value verifier_args.geometry / tools' --geometry takes"""
    return sorted({**GEOMETRIES, **GEOMETRIES_STREAMED})


def geometry(name: str) -> tuple:
    """verifier_args.geometry -> (full table, its --small form)"""
    both = {**GEOMETRIES, **GEOMETRIES_STREAMED}
    if name not in both:
        raise RFError(f"verifier_args.geometry {name!r} (one of {geometry_names()})")
    return both[name]


def tower_config(cfg: dict) -> dict:
    """ClipScoreVerifier's `model_config` of a geometry table (VIT_L14, VIT_H14, ...)."""
    return dict(text_heads=cfg["text"]["heads"], vision_heads=cfg["vision"]["heads"], hidden_act=cfg.get("act", "quick_gelu"))


class ClipScoreVerifier:
    """`score_batch(latents [n, S, 64], seeds, prompt) -> (f32 [n], i32 [n])` and `score_images(paths, prompt)` for
    runner.run_reflection_search.  `clip_state_dict`: an HF CLIPModel state dict (`text_model.*`, `vision_model.*`,
    `text_projection.weight`, `visual_projection.weight`, `logit_scale`); `tokenize(prompts) -> ids [B, L]` (CLIP BPE ids, EOS the
    largest id for the legacy eos_token_id = 2 config); height / width: the candidates' image size.  `model_config`: the head counts
    and activation of the checkpoint's config.json (`text_heads`, `vision_heads`, `hidden_act`, `image_size`; what `load_clip_dir`
    returns); None = clip-vit-large-patch14's (head dim 64 on both towers, quick_gelu).  The images are preprocessed at the
    checkpoint's `image_size` (224, or 336 for clip-vit-large-patch14-336), cross-checked against its position-embedding rows; a
    config without it takes the size those rows imply."""

    def __init__(self, pipe, clip_state_dict: Dict[str, torch.Tensor], tokenize: Callable[[List[str]], torch.Tensor], height: int, width: int,
                 eos_token_id: int = 2, eps: float = 1e-5, model_config: Optional[dict] = None):
        from ..flux.vae_hip import HipVAE
        if pipe.vae is None:
            raise RFError("ClipScoreVerifier: the pipeline has no VAE -- the verifier scores decoded images (load a pipeline with a vae/ "
                          "directory, or FluxPipeline.synthetic(..., with_vae=True))")
        if not isinstance(pipe.vae, HipVAE):
            raise RFError("ClipScoreVerifier: the pipeline's VAE is not the HIP VAE; call pipe.enable_hip_vae() first")
        self.pipe, self.height, self.width, self._tokenize = pipe, int(height), int(width), tokenize
        sd = clip_state_dict
        dev = pipe.device
        text = {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}
        vision = {k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
        if not text or not vision or "text_projection.weight" not in sd or "logit_scale" not in sd:
            raise RFError("ClipScoreVerifier: needs a CLIPModel state dict (text_model.*, vision_model.*, text/visual_projection, logit_scale)")
        t_hidden, v_hidden = text["embeddings.token_embedding.weight"].shape[1], vision["vision_model.embeddings.patch_embedding.weight"].shape[0]
        mc = dict(model_config or {})
        t_heads, v_heads, act = int(mc.get("text_heads", t_hidden // 64)), int(mc.get("vision_heads", v_hidden // 64)), mc.get("hidden_act", "quick_gelu")
        if t_heads <= 0 or v_heads <= 0 or t_hidden % t_heads or v_hidden % v_heads:
            raise RFError(f"ClipScoreVerifier: {t_heads} / {v_heads} heads do not divide the hidden widths {t_hidden} / {v_hidden}")
        self.text = HipClipTextEncoder(text, t_heads, dev, eos_token_id=eos_token_id, eps=eps, head_dim=t_hidden // t_heads, act=act)
        self.vision = HipClipVisionEncoder(vision, v_heads, dev, eps=eps, head_dim=v_hidden // v_heads, act=act, image_size=mc.get("image_size"))
        self.text_projection = sd["text_projection.weight"].detach().to(dev, torch.bfloat16).contiguous()
        self.logit_scale = float(sd["logit_scale"].float())
        self._text_cache: Dict[str, torch.Tensor] = {}

    # ---- text side -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def text_embed(self, prompt: str) -> torch.Tensor:
        """text_projection(CLIPTextModel(prompt).pooler_output) [projection_dim] bf16, cached per prompt."""
        if prompt not in self._text_cache:
            ids = torch.as_tensor(self._tokenize([prompt])).to(self.pipe.device)
            pooled = self.text.encode(ids)[1]
            emb = ops.linear(pooled.contiguous(), self.text_projection)[0]
            if len(self._text_cache) >= 64:
                self._text_cache.pop(next(iter(self._text_cache)))
            self._text_cache[prompt] = emb
        return self._text_cache[prompt]

    # ---- image side ----------------------------------------------------------------------------------------------------------
    def _decode_into(self, latents: torch.Tensor, patches: torch.Tensor, row: int) -> None:
        """packed latents [1, S, 64] -> HIP VAE decode (the runner's `_save` arithmetic) -> patch rows of image `row`."""
        pipe = self.pipe
        z = pipe._unpack_latents(latents, self.height, self.width, pipe.vae_scale_factor)
        z = z / pipe.vae.config.scaling_factor + pipe.vae.config.shift_factor
        self._halo_into(pipe.vae.decode_halo(z)[0], patches, row)

    def _halo_into(self, out: torch.Tensor, patches: torch.Tensor, row: int) -> None:
        """the decoder's output [(H + 2), (W + 2), cout] (image at the interior, channels 0..2), read in place -> patch rows of image `row`."""
        Hp, Wp, cout = out.shape
        interior = out[1:, 1:]                                              # data pointer at (row 1, pixel 1, channel 0)
        self.vision.preprocess(interior, (0, Wp * cout, cout, 1), 0.5, 0.5, patches[row:row + 1], Hp - 2, Wp - 2)

    @torch.no_grad()
    def score_batch(self, latents: torch.Tensor, seeds: Sequence[int], prompt: str, decoded=None):
        """This rank's candidates of a round: packed latents [n, S, 64] -> (scores f32 [n], labels i32 [n]) on the device; one vision
        call for all n.  `decoded`: the candidates' HipVAE.decode_halo outputs, in row order, if the caller has them (the runner's
        device hand-off): then nothing is decoded here."""
        if decoded is not None:
            if len(decoded) != latents.shape[0]:
                raise RFError(f"ClipScoreVerifier.score_batch: {latents.shape[0]} candidates but {len(decoded)} decoded buffers")
            return self.score_decoded(decoded, prompt)
        n = latents.shape[0]
        patches = self.vision.alloc_patches(n)
        for b in range(n):
            self._decode_into(latents[b:b + 1], patches, b)
        return self._score(patches, prompt)

    score_batch.wants_prompt = True           # runner.bind_prompt hands over the original prompt
    score_batch.wants_decoded = True          # ... and the runner's device hand-off the buffers it already decoded

    @torch.no_grad()
    def score_decoded(self, halos, prompt: str):
        """Candidates already decoded (HipVAE.decode_halo outputs, [(H + 2), (W + 2), cout] each) -> (scores f32 [n], labels i32 [n]):
        `score_batch` without its decode, the same kernels on the same values."""
        patches = self.vision.alloc_patches(len(halos))
        for b, out in enumerate(halos):
            if out.shape[0] - 2 != self.height or out.shape[1] - 2 != self.width:
                raise RFError(f"ClipScoreVerifier.score_decoded: buffer {tuple(out.shape)} is not a decoded {self.height}x{self.width} image")
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
            arr = np.asarray(Image.open(p).convert("RGB"))                 # [H, W, 3] uint8: the levels the PNG holds
            lv = torch.from_numpy(arr.copy()).to(self.pipe.device).permute(2, 0, 1)
            self.vision.preprocess_levels(lv, out=patches[b:b + 1])
        return self._score(patches, prompt)

    def _score(self, patches: torch.Tensor, prompt: str):
        n = patches.shape[0]
        dev = self.pipe.device
        if n == 0:
            return torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        emb = self.vision.encode(patches)
        scores = clip_score(emb, self.text_embed(prompt), self.logit_scale)
        return scores, torch.ones(n, dtype=torch.int32, device=dev)


# ---- synthetic model + tokenizer (no checkpoint offline) ------------------------------------------------------------------------
def synthetic_clip_state(cfg: dict = VIT_L14, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A seeded random-init HF CLIPModel state dict of the given geometry (fp32, CPU): weights N(0, 1/fan_in) (q / k x 2 so that
    attention is not uniform), LayerNorm weights 1 + N(0, 0.1^2), biases N(0, 0.1^2), embeddings N(0, 0.2^2) / class N(0, 0.5^2),
    logit_scale = log(1 / 0.07) (CLIP's init)."""
    t, v, P = cfg["text"], cfg["vision"], cfg["projection_dim"]
    shapes = {"text_model.embeddings.token_embedding.weight": (t["vocab"], t["hidden"]),
              "text_model.embeddings.position_embedding.weight": (t["max_pos"], t["hidden"]),
              "text_model.final_layer_norm.weight": (t["hidden"],), "text_model.final_layer_norm.bias": (t["hidden"],),
              "vision_model.embeddings.class_embedding": (v["hidden"],),
              "vision_model.embeddings.patch_embedding.weight": (v["hidden"], 3, v["patch"], v["patch"]),
              "vision_model.embeddings.position_embedding.weight": ((v["image_size"] // v["patch"]) ** 2 + 1, v["hidden"]),
              "vision_model.pre_layrnorm.weight": (v["hidden"],), "vision_model.pre_layrnorm.bias": (v["hidden"],),
              "vision_model.post_layernorm.weight": (v["hidden"],), "vision_model.post_layernorm.bias": (v["hidden"],),
              "text_projection.weight": (P, t["hidden"]), "visual_projection.weight": (P, v["hidden"])}
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
        if "norm" in k and k.endswith(".weight") or "layrnorm.weight" in k:
            x = 1.0 + 0.1 * x
        elif k.endswith(".bias"):
            x = 0.1 * x
        elif "position_embedding" in k or "token_embedding" in k:
            x = 0.2 * x
        elif k.endswith("class_embedding"):
            x = 0.5 * x
        else:
            fan_in = math.prod(shapes[k][1:])
            x = x * fan_in ** -0.5 * (2.0 if ("q_proj" in k or "k_proj" in k) else 1.0)
        sd[k] = x
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
    return sd


def synthetic_tokenize(vocab: int, length: int = 77) -> Callable[[List[str]], torch.Tensor]:
    """Deterministic stand-in for CLIP's BPE (its vocabulary files are not shipped): BOS = vocab - 2, one id per UTF-8 byte
    (3 + byte % (vocab - 5)), EOS = vocab - 1 (the largest id, where the legacy config pools), padded with EOS to `length`."""
    def tokenize(prompts: List[str]) -> torch.Tensor:
        out = torch.full((len(prompts), length), vocab - 1, dtype=torch.int64)
        for i, p in enumerate(prompts):
            ids = [vocab - 2] + [3 + b % (vocab - 5) for b in p.encode("utf-8")][: length - 2] + [vocab - 1]
            out[i, : len(ids)] = torch.tensor(ids)
        return out
    return tokenize


def read_clip_config(path: str) -> dict:
    """What the verifier needs of an HF CLIPModel directory's config.json: head counts, activation, layer_norm_eps, projection_dim,
    the vision tower's image_size (224 where the config leaves it out; 336 for clip-vit-large-patch14-336) and
    the text tower's eos_token_id (49407 in the LAION / PickScore configs: pooling at the first EOS; 2 in OpenAI's legacy configs:
    pooling at the largest id).  Keys a config leaves out take CLIPConfig's defaults."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    t, v = cfg.get("text_config") or {}, cfg.get("vision_config") or {}
    t_act, v_act = t.get("hidden_act", "quick_gelu"), v.get("hidden_act", "quick_gelu")
    if t_act != v_act:
        raise RFError(f"{path}: text hidden_act {t_act!r} != vision hidden_act {v_act!r}; the verifier runs both towers with one activation")
    t_eps, v_eps = float(t.get("layer_norm_eps", 1e-5)), float(v.get("layer_norm_eps", 1e-5))
    if t_eps != v_eps:
        raise RFError(f"{path}: text layer_norm_eps {t_eps} != vision layer_norm_eps {v_eps}")
    return dict(text_heads=int(t.get("num_attention_heads", 8)), vision_heads=int(v.get("num_attention_heads", 12)), hidden_act=t_act,
                layer_norm_eps=t_eps, projection_dim=int(cfg.get("projection_dim", 512)), eos_token_id=int(t.get("eos_token_id", 2)),
                image_size=int(v.get("image_size", 224)))


def load_clip_dir(path: str):
    """An HF CLIPModel directory: config.json + model.safetensors + tokenizer files -> (state dict, tokenize, model config); the
    model config is `read_clip_config`'s."""
    mc = read_clip_config(path)
    from safetensors.torch import load_file
    from transformers import CLIPTokenizer
    sd = load_file(os.path.join(path, "model.safetensors"))
    P = sd["text_projection.weight"].shape[0] if "text_projection.weight" in sd else mc["projection_dim"]
    if P != mc["projection_dim"]:
        raise RFError(f"{path}: text_projection has {P} rows, config.json says projection_dim = {mc['projection_dim']}")
    tok = CLIPTokenizer.from_pretrained(path, local_files_only=True)

    def tokenize(prompts: List[str]) -> torch.Tensor:
        return tok(list(prompts), padding="max_length", max_length=77, truncation=True, return_tensors="pt")["input_ids"]
    return sd, tokenize, mc


def build_from_config(config: dict, pipe, synthetic: bool = False, small: bool = False) -> ClipScoreVerifier:
    """The verifier `verifier_args = {"name": "clip" | "pickscore", "clip_model_path": DIR}` names: DIR is an HF CLIPModel directory
    (clip-vit-large-patch14, or a ViT-H/14 one: PickScore_v1, HPSv2, LAION CLIP-H); its config.json decides heads and activation.
    "pickscore" is an alias: PickScore's score IS exp(logit_scale) * cos(image, text) behind the CLIP processor, a scalar metric
    sorted with `scalar_sort_key`.  With `synthetic`: a seeded random-init CLIP of `verifier_args.geometry` ("vit_l14", the default,
    "vit_h14" or "vit_l14_336"; their 2-layer TINY / TINY_H / TINY_336 forms with `small`) and the synthetic tokenizer.  Switches the pipeline's VAE to the HIP path."""
    va, pa = config.get("verifier_args", {}), config["pipeline_args"]
    if pipe.vae is None:
        raise RFError("the CLIP verifier needs a pipeline with a VAE")
    pipe.enable_hip_vae()
    if synthetic:
        cfg = geometry(va.get("geometry", "vit_l14"))[1 if small else 0]
        seed = int(va.get("seed", 0))
        sd, tok = synthetic_clip_state(cfg, seed), synthetic_tokenize(cfg["text"]["vocab"])
        mc = dict(tower_config(cfg), eos_token_id=2, image_size=cfg["vision"]["image_size"])
    else:
        if not va.get("clip_model_path"):
            raise RFError(f'verifier_args.name == "{va.get("name", "clip")}" needs verifier_args.clip_model_path (an HF CLIPModel directory)')
        sd, tok, mc = load_clip_dir(va["clip_model_path"])
    return ClipScoreVerifier(pipe, sd, tok, pa["height"], pa["width"], eos_token_id=mc["eos_token_id"], eps=mc.get("layer_norm_eps", 1e-5),
                             model_config=mc)
