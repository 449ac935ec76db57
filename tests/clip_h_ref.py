"""Checker of the ViT-H-style CLIP towers (head dim 80, erf GELU): transformers' own `CLIPModel`, built from a `CLIPConfig` of the test
geometry and loaded with the (bf16-rounded) synthetic state dict -- in fp32 on the CPU it is the reference, in bf16 on the device it
is the yardstick of the repo's tolerance rule (tests/test_clip_score_gpu.py).  Nothing is restated here, so nothing needs pinning:
tests/test_clip_h_cpu.py only checks that the synthetic state dict fills every parameter of the model."""
from __future__ import annotations

import torch

BF = torch.bfloat16

# the smallest tower that reaches the head-dim-80 attention: 257 tokens -> S_pad = 288 (a partial last key block, padded keys, a query
# block that ends inside the padding); hidden 160 is no multiple of the GEMM's K-tile (the K-padded weight path)
HD80 = dict(text=dict(vocab=300, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
            vision=dict(hidden=160, heads=2, inter=320, layers=2, image_size=224, patch=14), projection_dim=64, act="gelu")
# ViT-H/14's real widths, 2 layers per tower, a small vocabulary (the embedding table's height does not reach any kernel)
WIDE_H2 = dict(text=dict(vocab=1000, hidden=1024, heads=16, inter=4096, layers=2, max_pos=77),
               vision=dict(hidden=1280, heads=16, inter=5120, layers=2, image_size=224, patch=14), projection_dim=1024, act="gelu")


def bf16_round(sd):
    return {k: v.to(BF).float() for k, v in sd.items()}


def hf_clip_model(cfg: dict, sd: dict, eos_token_id: int = 2, strict: bool = True):
    """transformers.CLIPModel (fp32, CPU, eval) of a geometry table of tts/clip_verifier.py with `sd` loaded."""
    import transformers as tr
    t, v, act = cfg["text"], cfg["vision"], cfg.get("act", "quick_gelu")
    m = tr.CLIPModel(tr.CLIPConfig(
        text_config=dict(vocab_size=t["vocab"], hidden_size=t["hidden"], intermediate_size=t["inter"], num_hidden_layers=t["layers"],
                         num_attention_heads=t["heads"], max_position_embeddings=t["max_pos"], hidden_act=act, eos_token_id=eos_token_id,
                         bos_token_id=0, pad_token_id=1),
        vision_config=dict(hidden_size=v["hidden"], intermediate_size=v["inter"], num_hidden_layers=v["layers"], num_attention_heads=v["heads"],
                           image_size=v["image_size"], patch_size=v["patch"], hidden_act=act),
        projection_dim=cfg["projection_dim"])).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    if strict:
        missing = [k for k in missing if not k.endswith("position_ids")]
        assert not missing and not unexpected, (missing, unexpected)
    return m


@torch.no_grad()
def image_embeds(m, pixel_values):
    p = next(m.parameters())
    return m.get_image_features(pixel_values=pixel_values.to(p.device, p.dtype)).pooler_output.float().cpu()


@torch.no_grad()
def text_embeds(m, ids):
    p = next(m.parameters())
    return m.get_text_features(input_ids=ids.to(p.device)).pooler_output.float().cpu()
