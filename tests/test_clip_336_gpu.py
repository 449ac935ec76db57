"""GPU: the CLIP-score verifier at 336 px (openai/clip-vit-large-patch14-336's geometry: 24 x 24 + 1 = 577 tokens, S_pad 608) --
rf_clip_preprocess at size 336 (two crop columns per thread), the vision tower on attn64_stream_kernel (csrc/text.hip: more keys than
the LDS holds), and ClipScoreVerifier end to end with verifier_args.geometry = "vit_l14_336".

Checkers and rules are the 224-px tests', unchanged: tests/clip_score_ref.py's resize restatement under check_patches of
tests/test_clip_score_gpu.py (at most one 8-bit level off, on < 1 % of the values, zero K padding), and transformers' own CLIPModel
(tests/clip_h_ref.py) under rel-L2(hip, fp32) <= 2 x rel-L2(transformers bf16, fp32) + 2e-3.
"""
import pytest
import torch

from reflectionflow_amd.tts import clip_verifier as CV
from tests import clip_h_ref as H
from tests import clip_score_ref as R
from tests.test_clip_score_gpu import _small_pipe, check_patches, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tower(dev):
    from reflectionflow_amd.flux.text_hip import HipClipVisionEncoder
    cfg = CV.TINY_336
    sd = H.bf16_round(CV.synthetic_clip_state(cfg, 2))
    v = cfg["vision"]
    venc = HipClipVisionEncoder({k: x for k, x in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}, v["heads"], dev,
                                head_dim=v["hidden"] // v["heads"], image_size=v["image_size"])
    return sd, venc


@torch.no_grad()
@pytest.mark.parametrize("H_,W_", [(400, 400), (512, 704)])
def test_preprocess_at_336_vs_restatement(dev, tower, H_, W_):
    _, venc = tower
    assert (venc.image_size, venc.patch, venc.tokens, venc.s_pad) == (336, 14, 577, 608)
    lv = R.synthetic_levels(H_ * 7 + W_, H_, W_)
    got = venc.preprocess_levels(lv.to(dev))
    torch.cuda.synchronize()
    assert got.shape == (1, 576, 640)
    frac = check_patches(got[0:1], R.resized_levels(lv, 336), 640)
    print(f"  {H_}x{W_} -> 336: {100 * frac:.3f} % of values one level off the restatement")


def test_image_size_is_cross_checked_against_the_position_rows(dev):
    from reflectionflow_amd.flux.text_hip import HipClipVisionEncoder, RFError
    sd = CV.synthetic_clip_state(CV.TINY_336, 0)
    vis = {k: x for k, x in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    with pytest.raises(RFError, match="image_size 224"):
        HipClipVisionEncoder(vis, 2, dev, image_size=224)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 3])
def test_336_vision_tower_vs_transformers(dev, tower, B):
    """577 tokens in S_pad = 608 rows: four whole key chunks and a partial one with padded keys under the mask, through the tower's own
    launch site.  Both sides read the same pixel values (the checker's, as bf16 patch rows)."""
    sd, venc = tower
    imgs = [R.synthetic_levels(50 + i, 336 + 37 * i, 420 - 20 * i) for i in range(B)]
    pv = torch.stack([R.preprocess_ref(x, 336) for x in imgs])
    m = H.hf_clip_model(CV.TINY_336, sd)
    ref = H.image_embeds(m, pv)
    yard = H.image_embeds(m.to(dev, BF), pv)
    emb = venc.encode(R.patches_of(pv, 14, venc.k_pad).to(dev, BF))
    torch.cuda.synchronize()
    e, e_y = rel_l2(emb, ref), rel_l2(yard, ref)
    print(f"  B={B}: image embeds hip {e:.3e}  transformers-bf16 {e_y:.3e}")
    assert emb.shape == (B, 64) and torch.isfinite(emb.float()).all()
    assert e <= 2.0 * e_y + 2e-3, (e, e_y)


@torch.no_grad()
def test_verifier_end_to_end_with_geometry_vit_l14_336(dev):
    """build_from_config(synthetic, small) on a 256^2 pipeline: finite scores, bit-equal run to run, alone vs in a batch, and between
    score_batch (decodes itself) and score_decoded (the runner's hand-off buffers)."""
    pipe = _small_pipe(dev)
    cfg = dict(pipeline_args=dict(height=256, width=256), verifier_args=dict(name="clip", geometry="vit_l14_336", seed=4))
    v = CV.build_from_config(cfg, pipe, synthetic=True, small=True)
    assert (v.vision.image_size, v.vision.tokens, v.vision.s_pad) == (336, 577, 608)
    g = torch.Generator().manual_seed(11)
    lat = (torch.randn(3, 256, 64, generator=g) * 1.5).to(dev, BF)
    s1, l1 = v.score_batch(lat, [0, 1, 2], prompt="a red cube")
    s2, _ = v.score_batch(lat, [0, 1, 2], prompt="a red cube")
    alone = v.score_batch(lat[1:2], [1], prompt="a red cube")[0]
    halos = []
    for b in range(3):
        z = pipe._unpack_latents(lat[b:b + 1], 256, 256, pipe.vae_scale_factor)
        halos.append(pipe.vae.decode_halo(z / pipe.vae.config.scaling_factor + pipe.vae.config.shift_factor)[0])
    s3, l3 = v.score_decoded(halos, "a red cube")
    s4, _ = v.score_batch(lat, [0, 1, 2], prompt="a red cube", decoded=halos)
    torch.cuda.synchronize()
    assert torch.isfinite(s1).all() and l1.tolist() == [1, 1, 1] and l3.tolist() == [1, 1, 1]
    assert torch.equal(s1, s2) and torch.equal(s1[1:2], alone), (s1, s2, alone)
    assert torch.equal(s1, s3) and torch.equal(s1, s4), (s1, s3, s4)
    assert len(set(s1.tolist())) == 3
