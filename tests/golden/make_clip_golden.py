"""Generates tests/golden/clip_score.npz: outputs of Hugging Face transformers' OWN `CLIPModel` and `CLIPImageProcessorPil` (the
CLIP-score verifier's definition, reflectionflow_amd/tts/clip_verifier.py) on seeded synthetic weights, pictures and prompts, in fp32.

Run here (transformers 5.15.0 is installed in this image):   python tests/golden/make_clip_golden.py
The weights and pictures are NOT stored: `clip_verifier.synthetic_clip_state(CFG, seed)` and `clip_score_ref.synthetic_levels(seed, H, W)`
rebuild them from the recorded seeds, so the fixture holds token ids, every 4th row of the processor's 8-bit crops and the model's outputs.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reflectionflow_amd.tts import clip_verifier as CV  # noqa: E402
from tests import clip_score_ref as R  # noqa: E402

import transformers  # noqa: E402
from transformers import CLIPConfig, CLIPImageProcessorPil, CLIPModel  # noqa: E402

CFG = dict(text=dict(vocab=300, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
           vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=14), projection_dim=64)
WEIGHT_SEED = 31
IMAGES = [  # (seed, H, W): what each case exercises
    (41, 256, 402),    # downscale, wide, odd leftover: new 224 x 351, left = 63
    (42, 160, 160),    # upscale, square
    (43, 300, 190),    # upscale of the short edge, tall, odd leftover: new 353 x 224, top = 64
    (44, 512, 512),    # downscale, square (2.3x: wide antialias support)
]
PROMPTS = ["a red cube left of a blue ball", "two cats on a sofa"]


def hf_model():
    t, v = CFG["text"], CFG["vision"]
    cfg = CLIPConfig(text_config=dict(vocab_size=t["vocab"], hidden_size=t["hidden"], intermediate_size=t["inter"], num_hidden_layers=t["layers"],
                                      num_attention_heads=t["heads"], max_position_embeddings=t["max_pos"], hidden_act="quick_gelu",
                                      layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0, pad_token_id=1),
                     vision_config=dict(hidden_size=v["hidden"], intermediate_size=v["inter"], num_hidden_layers=v["layers"],
                                        num_attention_heads=v["heads"], image_size=v["image_size"], patch_size=v["patch"], hidden_act="quick_gelu",
                                        layer_norm_eps=1e-5),
                     projection_dim=CFG["projection_dim"])
    m = CLIPModel(cfg).eval().float()
    sd = CV.synthetic_clip_state(CFG, WEIGHT_SEED)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m, sd


@torch.no_grad()
def main():
    m, sd = hf_model()
    proc = CLIPImageProcessorPil()
    tok = CV.synthetic_tokenize(CFG["text"]["vocab"])
    ids = tok(PROMPTS)
    imgs = [R.synthetic_levels(s, H, W) for s, H, W in IMAGES]
    pils = [Image.fromarray(x.permute(1, 2, 0).numpy()) for x in imgs]
    levels = np.stack([np.asarray(proc(p, do_rescale=False, do_normalize=False, return_tensors="np")["pixel_values"][0]) for p in pils])
    pv = torch.from_numpy(np.stack([np.asarray(proc(p, return_tensors="np")["pixel_values"][0]) for p in pils])).float()
    out = m(input_ids=ids, pixel_values=pv)
    # the restatement on the processor's own pixels, and the restatement's preprocessing
    mine_img = R.vision_embeds(sd, pv, CFG["vision"]["heads"])
    mine_txt = R.text_embeds(sd, ids, CFG["text"]["heads"])
    mine_lv = torch.stack([R.resized_levels(x) for x in imgs])
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)  # noqa: E731  (CLIPModel.forward returns L2-normalised embeddings)
    print(f"image embeds: restatement vs transformers max|d| = {float((nrm(mine_img) - out.image_embeds).abs().max()):.3e}")
    print(f"text embeds:  restatement vs transformers max|d| = {float((nrm(mine_txt) - out.text_embeds).abs().max()):.3e}")
    d = (mine_lv - torch.from_numpy(levels)).abs()
    print(f"preprocess: max level diff {float(d.max())}, fraction off {float((d > 0).float().mean()):.3f}")
    data = {"transformers_version": np.array(transformers.__version__), "weight_seed": np.array(WEIGHT_SEED),
            "images": np.array(IMAGES, dtype=np.int64), "ids": ids.numpy(), "levels_rows4": levels[:, :, ::4].astype(np.uint8),   # every 4th crop row: keeps the fixture small
            "image_embeds": m.get_image_features(pixel_values=pv).pooler_output.numpy(),     # projected, not normalised
            "text_embeds": m.get_text_features(input_ids=ids).pooler_output.numpy(),
            "logits_per_image": out.logits_per_image.numpy(), "logit_scale": np.array(float(m.logit_scale))}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_score.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
