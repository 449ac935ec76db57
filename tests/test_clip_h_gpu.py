"""GPU: the ViT-H/14 form of the CLIP-score verifier -- attn80_kernel (head dim 80) and clip_act_kernel<RF_CLIP_ACT_GELU> (csrc/text.hip) through the
*_opts entry points, flux/text_hip.py and tts/clip_verifier.py.

Checker: transformers' CLIPModel in fp32 on the CPU (tests/clip_h_ref.py), hidden_act "gelu", loaded with the bf16-rounded synthetic
state dict.  Tolerance, as everywhere in this repo (tests/test_clip_score_gpu.py): rel-L2(hip, fp32) <= 2 x rel-L2(transformers eager
bf16 on the device, fp32) + 2e-3, the yardstick measured in the same test and printed.  A score is exp(logit_scale) * cos(image, text):
to first order its error is at most exp(logit_scale) * (rel. error of the image embedding + rel. error of the text embedding), so the
scores are held to exp(logit_scale) * (image bound + text bound).  Batch invariance, run-to-run stability and the equality of the old
entry points with {64, quick_gelu} are checked bit for bit.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from reflectionflow_amd.tts import clip_verifier as CV
from tests import clip_h_ref as H
from tests import clip_score_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def towers(cfg, seed, dev, eos_token_id=2):
    """(bf16-rounded state dict, HIP vision encoder, HIP text encoder) of a geometry table"""
    from reflectionflow_amd.flux.text_hip import HipClipTextEncoder, HipClipVisionEncoder
    sd = H.bf16_round(CV.synthetic_clip_state(cfg, seed))
    t, v, act = cfg["text"], cfg["vision"], cfg.get("act", "quick_gelu")
    venc = HipClipVisionEncoder({k: x for k, x in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}, v["heads"], dev,
                                head_dim=v["hidden"] // v["heads"], act=act)
    tenc = HipClipTextEncoder({k: x for k, x in sd.items() if k.startswith("text_model.")}, t["heads"], dev, eos_token_id=eos_token_id,
                              head_dim=t["hidden"] // t["heads"], act=act)
    return sd, venc, tenc


# ---- 1. clip_act_kernel<RF_CLIP_ACT_GELU> (rf_gelu_erf_inplace) ----------------------------------------------------------------------------------------------------------
def _ordinal(x):
    """bf16 -> integers in value order (-0 and +0 both 0): |difference| = distance in bf16 ulps"""
    b = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b - 0x8000), b)


def _ulp_cap(got, want, what):
    d = (_ordinal(got.cpu()) - _ordinal(want.cpu())).abs()
    off = int((d > 0).sum())
    assert int(d.max()) <= 1 and off <= 0.01 * d.numel(), f"{what}: {off} of {d.numel()} elements differ, by up to {int(d.max())} bf16 ulp"
    return off


@torch.no_grad()
@pytest.mark.parametrize("n", [8, 2056, 4096 * 5])
def test_gelu_erf_kernel_equals_torch_gelu_on_bf16(dev, n):
    from reflectionflow_amd import _lib
    from reflectionflow_amd.ops import stream_ptr
    # +-0, +-10, +-1e-3 and a randn block (unit variance: |x| stays below ~4.5).  Deeper in the negative tail the comparison says nothing
    # about a kernel: 1 + erf(x / sqrt 2) cancels in fp32 (6e-7 at x = -5 against erf's own ulp of 6e-8), so two correct fp32 erf
    # implementations -- torch's on the device and torch's on the CPU -- differ there by whole binades of the bf16 result.
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[:6] = torch.tensor([0.0, -0.0, 10.0, -10.0, 1e-3, -1e-3])
    x = x.to(BF)
    cpu_ref = F.gelu(x.float()).to(BF)                       # fp32 on the CPU, rounded to bf16 once
    xd = x.to(dev)
    want = F.gelu(xd)
    got = xd.clone()
    _lib.check(_lib.load().rf_gelu_erf_inplace(got.data_ptr(), n, stream_ptr()), "rf_gelu_erf_inplace")
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    ref_off = _ulp_cap(want, cpu_ref, "torch's device gelu vs the fp32 CPU reference")      # the reference alone meets the cap
    equal = torch.equal(got.view(torch.int16), want.view(torch.int16))
    hip_off = _ulp_cap(got, cpu_ref, "clip_act_kernel<GELU> vs the fp32 CPU reference")
    print(f"  n={n}: bit-equal to torch's device gelu: {equal}; vs fp32 CPU reference: hip {hip_off}, torch device {ref_off} elements 1 ulp off")
    if not equal:                                           # torch's device erf differs from erff in the last bit: the cap above decides
        d = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        print(f"  n={n}: {d} elements differ from torch's device gelu")


# ---- 2. head dim 80 alone: the smallest tower that reaches attn80_kernel ---------------------------------------------------------------
@pytest.fixture(scope="module")
def hd80(dev):
    sd, venc, _ = towers(H.HD80, 2, dev)
    imgs = [R.synthetic_levels(50 + i, 224 + 37 * i, 300 - 20 * i) for i in range(3)]
    pv = torch.stack([R.preprocess_ref(x) for x in imgs])                      # [3, 3, 224, 224] fp32
    m = H.hf_clip_model(H.HD80, sd)
    ref = H.image_embeds(m, pv)
    yard = H.image_embeds(m.to(dev, BF), pv)
    return dict(venc=venc, pv=pv, ref=ref, yard=yard)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 3])
def test_head_dim_80_vision_tower_vs_transformers(dev, hd80, B):
    """hidden 160 = 2 heads x 80, 257 tokens in S_pad = 288 rows: a partial last key block, padded keys under the mask, a query block
    that ends inside the padding.  Both sides read the same pixel values (the checker's, as bf16 patch rows)."""
    venc, pv, ref, yard = hd80["venc"], hd80["pv"][:B], hd80["ref"][:B], hd80["yard"][:B]
    assert venc.s_pad == 288 and venc.tokens == 257 and venc.hidden == 160
    patches = R.patches_of(pv, 14, venc.k_pad).to(dev, BF)
    emb = venc.encode(patches)
    torch.cuda.synchronize()
    e, e_y = rel_l2(emb, ref), rel_l2(yard, ref)
    print(f"  B={B}: image embeds hip {e:.3e}  transformers-bf16 {e_y:.3e}")
    assert emb.shape == (B, 64) and torch.isfinite(emb.float()).all()
    assert e <= 2.0 * e_y + 2e-3, (e, e_y)


# ---- 3., 4. ViT-H/14's real widths, 2 layers per tower --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(dev):
    eos = H.WIDE_H2["text"]["vocab"] - 1                 # the LAION / PickScore form: pooled at the FIRST eos_token_id, not at the largest id
    sd, venc, tenc = towers(H.WIDE_H2, 3, dev, eos_token_id=eos)
    m = H.hf_clip_model(H.WIDE_H2, sd, eos_token_id=eos)
    ids = CV.synthetic_tokenize(H.WIDE_H2["text"]["vocab"])(["a red cube left of a blue ball"])
    t_ref = H.text_embeds(m, ids)
    return dict(sd=sd, venc=venc, tenc=tenc, m=m, ids=ids, t_ref=t_ref, ls=float(sd["logit_scale"]))


def _text_embed(w, dev):
    from reflectionflow_amd import ops
    pooled = w["tenc"].encode(w["ids"].to(dev))[1]
    return ops.linear(pooled.contiguous(), w["sd"]["text_projection.weight"].to(dev, BF).contiguous())[0]


@torch.no_grad()
@pytest.mark.parametrize("H_,W_", [(160, 160), (256, 402)])
def test_vit_h_widths_embeddings_and_scores_vs_transformers(dev, wide, H_, W_):
    """vision 1280 / 16 heads / 5120, text 1024 / 16 heads / 4096, erf GELU, projection 1024; 4 images through rf_clip_preprocess."""
    from reflectionflow_amd.flux.text_hip import clip_score
    venc, m, ls = wide["venc"], wide["m"], wide["ls"]
    imgs = [R.synthetic_levels(1000 * H_ + W_ + i, H_, W_) for i in range(4)]
    emb = venc.encode(venc.preprocess_levels(torch.stack(imgs).to(dev)))
    txt = _text_embed(wide, dev)
    sc = clip_score(emb, txt, ls)
    torch.cuda.synchronize()
    pv = torch.stack([R.preprocess_ref(x) for x in imgs])
    ref, t_ref = H.image_embeds(m, pv), wide["t_ref"]
    mb = H.hf_clip_model(H.WIDE_H2, wide["sd"], eos_token_id=H.WIDE_H2["text"]["vocab"] - 1).to(dev, BF)
    yard, t_yard = H.image_embeds(mb, pv), H.text_embeds(mb, wide["ids"])
    e, e_y, et, et_y = rel_l2(emb, ref), rel_l2(yard, ref), rel_l2(txt[None], t_ref), rel_l2(t_yard, t_ref)
    ref_sc = R.scores(ref, t_ref[0], ls)
    b_img, b_txt = 2.0 * e_y + 2e-3, 2.0 * et_y + 2e-3
    print(f"  {H_}x{W_}: image embeds hip {e:.3e}  transformers-bf16 {e_y:.3e}; text embed hip {et:.3e}  transformers-bf16 {et_y:.3e}; "
          f"scores {sc.cpu().tolist()} vs {ref_sc.tolist()}")
    assert emb.shape == (4, 1024) and txt.shape == (1024,) and torch.isfinite(emb.float()).all() and torch.isfinite(txt.float()).all()
    assert e <= b_img, (e, e_y)
    assert et <= b_txt, (et, et_y)
    assert float((sc.cpu() - ref_sc).abs().max()) <= math.exp(ls) * (b_img + b_txt)


@torch.no_grad()
def test_head_dim_80_scores_are_batch_invariant_and_stable(dev, wide):
    from reflectionflow_amd.flux.text_hip import clip_score
    venc, ls = wide["venc"], wide["ls"]
    imgs = [R.synthetic_levels(70 + i, 256, 256 + 16 * i) for i in range(8)]
    patches = torch.cat([venc.preprocess_levels(x.to(dev)) for x in imgs])
    txt = _text_embed(wide, dev)
    all8 = clip_score(venc.encode(patches), txt, ls)
    again = clip_score(venc.encode(patches), txt, ls)
    alone = torch.cat([clip_score(venc.encode(patches[i:i + 1]), txt, ls) for i in range(8)])
    torch.cuda.synchronize()
    assert torch.equal(all8, again), (all8, again)
    assert torch.equal(all8, alone), (all8, alone)
    assert len(set(all8.tolist())) == 8


# ---- 5. the v9 / v16 entry points are the new ones with {64, quick_gelu} ---------------------------------------------------------------
@torch.no_grad()
def test_old_entry_points_equal_the_opts_calls_with_64_and_quick_gelu(dev):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    lib = L.load()
    _, venc, tenc = towers(CV.TINY, 5, dev)
    assert (venc._opts.head_dim, venc._opts.act, tenc._opts.head_dim, tenc._opts.act) == (64, 0, 64, 0)
    imgs = torch.stack([R.synthetic_levels(90 + i, 200, 240) for i in range(3)])
    patches = venc.preprocess_levels(imgs.to(dev)).contiguous()
    new = venc.encode(patches)                                             # rf_clip_vision_encode_opts
    n = lib.rf_clip_vision_workspace_bytes(C.byref(venc._w), 3)
    assert n == lib.rf_clip_vision_workspace_bytes_opts(C.byref(venc._w), C.byref(venc._opts), 3) > 0
    ws = venc._ws.get(n)
    old = torch.empty_like(new)
    L.check(lib.rf_clip_vision_encode(C.byref(venc._w), patches.data_ptr(), 3, old.data_ptr(), C.byref(ws), stream_ptr()), "rf_clip_vision_encode")
    ids = CV.synthetic_tokenize(CV.TINY["text"]["vocab"])(["a red cube", "two cats on a sofa"]).to(dev)
    last_new, _ = tenc.encode(ids)                                         # rf_clip_text_encode_opts (sets the mask for S = 77)
    n = lib.rf_clip_text_workspace_bytes(C.byref(tenc._w), 2, 77)
    assert n == lib.rf_clip_text_workspace_bytes_opts(C.byref(tenc._w), C.byref(tenc._opts), 2, 77) > 0
    ws = tenc._ws.get(n)
    last_old = torch.empty_like(last_new)
    L.check(lib.rf_clip_text_encode(C.byref(tenc._w), ids.to(torch.int32).contiguous().data_ptr(), 2, 77, None, last_old.data_ptr(), None, C.byref(ws),
                                    stream_ptr()), "rf_clip_text_encode")
    torch.cuda.synchronize()
    assert torch.equal(old, new) and torch.equal(last_old, last_new)
    assert torch.isfinite(new.float()).all() and torch.isfinite(last_new.float()).all()


# ---- 6. end to end: the reflection search with the ViT-H-style verifier ----------------------------------------------------------------
def _run_h_search(name, out_dir, dev):
    from reflectionflow_amd.tts import runner, search
    from tests.test_clip_score_gpu import _search_cfg, _small_pipe
    cfg = _search_cfg()                                                    # N = 4 candidates, R = 2 rounds, 256 x 256
    cfg["verifier_args"] = {"name": name, "geometry": "vit_h14"}
    pipe = _small_pipe(dev)
    v = CV.build_from_config(cfg, pipe, synthetic=True, small=True)
    assert (v.vision._opts.head_dim, v.vision._opts.act, v.text._opts.head_dim, v.text._opts.act) == (80, 1, 64, 1)
    assert v.vision.hidden == 160 and len(v.vision._layers) == 2 and len(v.text._layers) == 2
    return runner.run_reflection_search(cfg, ["a red cube left of a blue ball"], out_dir, pipe, search.Shard(0, 1), score_batch=v.score_batch,
                                        score_images=v.score_images)


@torch.no_grad()
@pytest.mark.timeout(600)
def test_reflection_search_with_the_vit_h_verifier_and_the_pickscore_alias(dev, tmp_path):
    from tests.test_clip_score_gpu import _tree_bytes
    log = _run_h_search("clip", str(tmp_path / "clip"), dev)
    assert len(log) >= 2
    for prev, rec in zip(log, log[1:]):
        assert rec["selected"] == sorted(range(4), key=lambda i: (-prev["scores"][i][0], i))
    for rec in log:
        assert all(lab == 1 for _, lab in rec["scores"]) and all(math.isfinite(s) for s, _ in rec["scores"])
    assert len(set(s for s, _ in log[0]["scores"])) == 4
    log_p = _run_h_search("pickscore", str(tmp_path / "pickscore"), dev)
    assert [r.get("selected") for r in log_p] == [r.get("selected") for r in log] and [r["scores"] for r in log_p] == [r["scores"] for r in log]
    a, b = _tree_bytes(tmp_path / "clip"), _tree_bytes(tmp_path / "pickscore")
    assert a and a == b
