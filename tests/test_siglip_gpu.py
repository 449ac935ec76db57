"""GPU: the SigLIP score verifier on the HIP path -- rf_siglip_preprocess, the pooling head's probe attention, both towers
(csrc/siglip.hip through flux/text_hip.py), rf_siglip_score and tts/siglip_verifier.py end to end.

Reference: tests/siglip_ref.py in fp32 on the CPU, pinned bit for bit to transformers' SiglipModel by tests/test_siglip_cpu.py.
Tower tolerance, the project's rule (tests/test_clip_h_gpu.py): rel-L2(hip, fp32) <= 2 x rel-L2(transformers eager bf16 on the device,
fp32) + 2e-3, measured per tower in the test itself.  Configs: tests/siglip_ref.py TINY_224 (256 tokens: keys resident, no padded row)
and TINY_322 (529 tokens in S_pad = 544 rows: attn80_stream_kernel inside a tower, padded keys under the mask)."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from reflectionflow_amd.tts import siglip_verifier as SV
from tests import siglip_ref as R
from tests.clip_score_ref import synthetic_levels
from tests.test_kernels_gpu import assert_close
from tests.workspace_poison import POISONS, Workspace, assert_live, assert_same_bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PROMPTS = ["a red cube left of a blue ball", "two cats on a sofa"]
CFGS = {"224": R.TINY_224, "322": R.TINY_322}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


# ---- 1. rf_siglip_preprocess ---------------------------------------------------------------------------------------------------------------
PRE_CASES = [(40, 56, 28), (16, 24, 28), (28, 28, 28)]        # H, W -> size: down (non-square), up, identity; patch 14: 2 x 2 patches


@functools.lru_cache(maxsize=None)
def pre_case(H, W, size):
    from PIL import Image
    lv = np.random.default_rng(100 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(lv).resize((size, size), Image.BICUBIC))
    mine = R.preprocess_levels_np(lv, size)
    return lv, R.patches_from_pixels(R.normalise_np(pil)[None], 14), R.patches_from_pixels(R.normalise_np(mine)[None], 14)


def _preprocess(dev, img, strides, a, b, H, W, size, n=1):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    g = size // 14
    out = torch.full((n, g * g, 640), 7.0, dtype=BF, device=dev)
    L.check(L.load().rf_siglip_preprocess(img.data_ptr(), *strides, n, H, W, a, b, size, 14, out.data_ptr(), stream_ptr()), "rf_siglip_preprocess")
    torch.cuda.synchronize()
    return out.cpu()


@torch.no_grad()
@pytest.mark.parametrize("H,W,size", PRE_CASES)
def test_preprocess_equals_pil_and_the_restatement(dev, H, W, size):
    """level-exact against PIL.Image.resize((s, s), BICUBIC) (a bf16 pixel value names its level: levels are 2 / 255 apart, bf16 values
    in [-1, 1] at most 2^-8), bit-equal to the numpy restatement; fed from [3][H][W] levels and from a zero-halo NHWC buffer"""
    lv, want_pil, want_np = pre_case(H, W, size)
    chw = torch.from_numpy(lv.copy()).permute(2, 0, 1).to(dev, BF).contiguous()
    got = _preprocess(dev, chw, (3 * H * W, W, 1, H * W), 1.0 / 255.0, 0.0, H, W, size)
    assert torch.equal(got.view(torch.int16), want_np.view(torch.int16)) and torch.equal(want_np.view(torch.int16), want_pil.view(torch.int16))
    assert float(got[..., 588:].abs().max()) == 0.0                                      # the K padding is written (zero)
    # a decoded image in [-1, 1] behind a halo ring: v = the bf16 value whose level = rint(255 (0.5 v + 0.5)) is lv
    v = (torch.from_numpy(lv.astype(np.float32)) / 255.0 * 2.0 - 1.0).to(BF)
    back = torch.round((v.float() * 0.5 + 0.5).clamp(0, 1) * 255.0).to(torch.uint8)
    keep = torch.from_numpy(lv) == back                                                  # bf16 cannot name every level: use the ones it does
    lv2 = back.numpy()
    halo = torch.zeros(H + 2, W + 2, 8, dtype=BF)
    halo[1:-1, 1:-1, :3] = v
    halo = halo.to(dev)
    got2 = _preprocess(dev, halo[1:, 1:], (0, (W + 2) * 8, 8, 1), 0.5, 0.5, H, W, size)
    want2 = R.patches_from_pixels(R.normalise_np(R.preprocess_levels_np(lv2, size))[None], 14)
    assert torch.equal(got2.view(torch.int16), want2.view(torch.int16)) and int(keep.sum()) > keep.numel() // 2


@torch.no_grad()
def test_preprocess_batch_of_two_at_384_drops_the_pixels_behind_the_last_patch(dev):
    """384 = 27 x 14 + 6: the valid patch convolution sees 378 rows / columns; two images per call (NX = 2 columns per thread)"""
    imgs = torch.stack([synthetic_levels(40 + i, 300, 420) for i in range(2)])
    chw = imgs.to(dev, BF).contiguous()
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    out = torch.full((2, 729, 640), 7.0, dtype=BF, device=dev)
    L.check(L.load().rf_siglip_preprocess(chw.data_ptr(), 3 * 300 * 420, 420, 1, 300 * 420, 2, 300, 420, 1.0 / 255.0, 0.0, 384, 14, out.data_ptr(),
                                          stream_ptr()), "rf_siglip_preprocess")
    torch.cuda.synchronize()
    for i in range(2):
        full = R.normalise_np(R.preprocess_levels_np(imgs[i].permute(1, 2, 0).numpy(), 384))
        want = R.patches_from_pixels(full[None, :, :378, :378], 14)
        assert torch.equal(out[i:i + 1].cpu().view(torch.int16), want.view(torch.int16)), i


# ---- 2. the probe attention kernel -----------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("d", [72, 64])
@pytest.mark.parametrize("T", [1, 4, 256, 529])
def test_probe_attention_vs_fp64(dev, T, d):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    heads, B, rows = 2, 3, (T + 31) // 32 * 32
    D = heads * d
    g = torch.Generator().manual_seed(1000 * T + d)
    q = (torch.randn(D, generator=g) * 2.0 * d ** -0.5).float()
    kv = torch.randn(B * rows, 2 * D + 8, generator=g).to(BF)
    kv[:, 2 * D:] = float("nan")                                                          # gap columns: never read
    for b in range(B):
        kv[b * rows + T:(b + 1) * rows] = float("nan")                                    # rows >= T: never read
    out = torch.full((B, D + 8), 7.0, dtype=BF, device=dev)
    kvd, qd = kv.to(dev), q.to(dev)
    L.check(L.load().rf_siglip_probe_attention(qd.data_ptr(), kvd.data_ptr(), kvd.stride(0), kvd[:, D:].data_ptr(), kvd.stride(0), out.data_ptr(),
                                                     out.stride(0), heads, d, B, T, rows, stream_ptr()), "rf_siglip_probe_attention")
    again = torch.full_like(out, 7.0)
    L.check(L.load().rf_siglip_probe_attention(qd.data_ptr(), kvd.data_ptr(), kvd.stride(0), kvd[:, D:].data_ptr(), kvd.stride(0), again.data_ptr(),
                                                     again.stride(0), heads, d, B, T, rows, stream_ptr()), "rf_siglip_probe_attention")
    torch.cuda.synchronize()
    k = kv.view(B, rows, -1)[:, :T, :D].double().view(B, T, heads, d)
    v = kv.view(B, rows, -1)[:, :T, D:2 * D].double().view(B, T, heads, d)
    w = torch.softmax(torch.einsum("hc,bthc->bht", q.double().view(heads, d), k), dim=-1)
    ref = torch.einsum("bht,bthc->bhc", w, v).reshape(B, D)
    got = out.cpu()
    assert bool((got[:, D:].view(torch.int16) == torch.tensor(7.0, dtype=BF).view(torch.int16)).all()), "columns >= heads * d were written"
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    print(f"  PROBE T={T} d={d}: rel-L2 {rel_l2(got[:, :D], ref):.3e}")
    assert_close(got[:, :D], ref, f"probe attention T={T} d={d}")


# ---- 3. rf_siglip_score ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_score_and_labels_vs_fp32(dev):
    from reflectionflow_amd.flux.text_hip import siglip_score
    g = torch.Generator().manual_seed(3)
    txt = torch.randn(144, generator=g).to(BF)
    img = (txt.float()[None] * torch.linspace(-1, 1, 9)[:, None] + 0.7 * torch.randn(9, 144, generator=g)).to(BF)
    ls, lb, thr = math.log(10.0), -2.0, 0.3
    sc, lab = siglip_score(img.to(dev), txt.to(dev), ls, lb, thr)
    torch.cuda.synchronize()
    cos = torch.nn.functional.cosine_similarity(img.double(), txt.double()[None], dim=-1)
    p = torch.sigmoid(cos * math.exp(ls) + lb)
    assert sc.dtype == torch.float32 and lab.dtype == torch.int32
    assert float((sc.cpu().double() - p).abs().max()) < 2e-6
    far = (p - thr).abs() > 1e-5
    assert int(far.sum()) >= 8 and torch.equal(lab.cpu()[far], (p >= thr).int()[far]) and 0 < int(lab.sum()) < 9
    assert torch.equal(lab.cpu(), (sc.cpu() >= thr).int())                               # the label is the returned score's own


# ---- 4. towers ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tower_case(name):
    """state dict (bf16-rounded), 3 images' pixel values through the numpy preprocess, ids of 2 prompts and the fp32 reference"""
    cfg = CFGS[name]
    size = cfg["vision"]["image_size"]
    sd = R.bf16_round(SV.synthetic_siglip_state(cfg, 1))
    lv = [synthetic_levels(60 + i, 200, 240 + 16 * i) for i in range(3)]
    px = torch.stack([R.normalise_np(R.preprocess_levels_np(x.permute(1, 2, 0).numpy(), size)) for x in lv]).float()
    ids = SV.synthetic_tokenize(cfg["text"]["vocab"])(PROMPTS)
    img, txt = R.vision_pooled(sd, px, cfg), R.text_pooled(sd, ids, cfg)
    return cfg, sd, lv, px, ids, img, txt, R.logits(sd, img, txt)


def encoders(name, dev):
    from reflectionflow_amd.flux.text_hip import HipSiglipTextEncoder, HipSiglipVisionEncoder
    cfg, sd = tower_case(name)[:2]
    venc = HipSiglipVisionEncoder({k: v for k, v in sd.items() if k.startswith("vision_model.")}, cfg["vision"]["heads"], dev,
                                  image_size=cfg["vision"]["image_size"])
    tenc = HipSiglipTextEncoder({k: v for k, v in sd.items() if k.startswith("text_model.")}, cfg["text"]["heads"], dev)
    return venc, tenc


# thresholds in LOGIT space, chosen on the CPU from the fp32 reference alone (its logits, image-major: 224: -9.45 -9.23 | -9.05 -9.01 |
# -9.91 -9.71; 322: -11.65 -10.77 | -12.11 -11.31 | -12.06 -11.14) so that at least 3 of the 6 (image, prompt) pairs lie further from
# them than the bound exp(logit_scale) (b_img + b_txt), 0.40 / 0.37 with the bf16 yardsticks measured on the CPU (image 5.9e-3 / 4.1e-3,
# text 1.2e-2): -10.4 has all six pairs of the 224 config above it (5 of them by more than 0.6); -11.4 splits the 322 config's pairs
# three to three, with -12.11, -12.06 and -10.77 further than 0.6 from it
THRESHOLD_LOGIT = {"224": -10.4, "322": -11.4}


@torch.no_grad()
@pytest.mark.parametrize("name", ["224", "322"])
def test_towers_scores_and_labels_vs_fp32(dev, name):
    from reflectionflow_amd.flux.text_hip import siglip_score
    cfg, sd, lv, px, ids, img_ref, txt_ref, lg_ref = tower_case(name)
    venc, tenc = encoders(name, dev)
    assert (venc.tokens, venc.s_pad) == {"224": (256, 256), "322": (529, 544)}[name] and venc.hidden == 144 and venc._w.inter == 320
    patches = torch.cat([venc.preprocess_levels(x.to(dev)) for x in lv])               # rf_siglip_preprocess: three image sizes
    assert torch.equal(patches.cpu().view(torch.int16), R.patches_from_pixels(px.to(BF), 14).view(torch.int16))
    img = venc.encode(patches)
    txt = tenc.encode(ids.to(dev))
    torch.cuda.synchronize()
    mb = R.hf_siglip_model(cfg, sd).to(dev, BF)
    img_y = mb.vision_model(pixel_values=px.to(dev, BF)).pooler_output
    txt_y = mb.text_model(input_ids=ids.to(dev)).pooler_output
    e, e_y, et, et_y = rel_l2(img, img_ref), rel_l2(img_y, img_ref), rel_l2(txt, txt_ref), rel_l2(txt_y, txt_ref)
    b_img, b_txt = 2.0 * e_y + 2e-3, 2.0 * et_y + 2e-3
    print(f"  TOWERS {name}: image hip {e:.3e} transformers-bf16 {e_y:.3e}; text hip {et:.3e} transformers-bf16 {et_y:.3e}")
    assert img.shape == (3, 144) and txt.shape == (2, 144) and torch.isfinite(img.float()).all() and torch.isfinite(txt.float()).all()
    assert e <= b_img, (e, e_y)
    assert et <= b_txt, (et, et_y)
    ls, lb = float(sd["logit_scale"]), float(sd["logit_bias"])
    bound = math.exp(ls) * (b_img + b_txt)                                                # the CLIP test's logit bound
    thr_logit = THRESHOLD_LOGIT[name]
    thr = 1.0 / (1.0 + math.exp(-thr_logit))
    far = 0
    for j in range(2):
        sc, lab = siglip_score(img, txt[j], ls, lb, thr)
        p_ref = torch.sigmoid(lg_ref[:, j])
        tol = p_ref * (1.0 - p_ref) * bound                                               # the sigmoid's slope times the logit bound
        print(f"  SCORES {name} prompt {j}: {sc.cpu().tolist()} vs {p_ref.tolist()} (logits {lg_ref[:, j].tolist()}, bound {bound:.3f})")
        assert bool(((sc.cpu() - p_ref).abs() <= tol).all()), (sc.cpu(), p_ref, tol)
        decided = (lg_ref[:, j] - thr_logit).abs() > bound
        far += int(decided.sum())
        assert torch.equal(lab.cpu()[decided], (lg_ref[:, j] >= thr_logit).int()[decided])
    assert far >= 3, f"only {far} of 6 reference logits are further than {bound:.3f} from the threshold"


@torch.no_grad()
@pytest.mark.parametrize("name", ["224", "322"])
def test_towers_are_batch_invariant_and_repeatable(dev, name):
    cfg, sd, lv, px, ids = tower_case(name)[:5]
    venc, tenc = encoders(name, dev)
    patches = R.patches_from_pixels(px.to(BF), 14).to(dev)
    all3, again, alone = venc.encode(patches), venc.encode(patches), venc.encode(patches[:1])
    t2, t1 = tenc.encode(ids.to(dev)), tenc.encode(ids[:1].to(dev))
    torch.cuda.synchronize()
    assert torch.equal(all3, again) and torch.equal(all3[:1], alone)
    assert torch.equal(t2[:1], t1)


@torch.no_grad()
@pytest.mark.parametrize("name", ["vision-322", "vision-224", "text-S64", "text-S40"])
def test_tower_result_does_not_depend_on_workspace_contents(dev, name):
    """as tests/test_workspace_stale_gpu.py holds the other towers: 529 tokens in 544 rows (pad rows between the live rows of two
    images), and a 40-token prompt in 64 rows (the padded-keys mask of the text tower)"""
    from reflectionflow_amd import _lib
    kind, which = name.split("-")
    cfg, sd, lv, px, ids = tower_case("322" if which == "322" else "224")[:5]
    venc, tenc = encoders("322" if which == "322" else "224", dev)
    if kind == "vision":
        patches = R.patches_from_pixels(px[:2].to(BF), 14).to(dev)
        enc, run = venc, lambda: [venc.encode(patches)]
    else:
        idd = (ids if which == "S64" else ids[:, :40]).to(dev)
        enc, run = tenc, lambda: [tenc.encode(idd)]
    base = run()
    torch.cuda.synchronize()
    buf = enc._ws.buf
    w = Workspace(buf.numel(), _lib.text_workspace_layout(buf.numel())["sk_flags"], dev, buf=buf)
    for j, t in enumerate(base):
        assert_live(t, f"{name}[{j}]")
    for pat in POISONS:
        assert w.fill(pat, seed=4) == buf.numel() - 4096
        got = w.call(lambda ws: run())
        assert enc._ws.buf is buf
        for j, t in enumerate(got):
            assert_same_bits(t, base[j], f"{name}[{j}] on a workspace filled with '{pat}'")


@torch.no_grad()
def test_text_tower_with_a_padded_keys_mask_vs_fp32(dev):
    """S = 40 in S_pad = 64 rows: no causal mask, padded keys masked; pooled at position 39"""
    cfg, sd, lv, px, ids = tower_case("224")[:5]
    _, tenc = encoders("224", dev)
    got = tenc.encode(ids[:, :40].to(dev))
    torch.cuda.synchronize()
    ref = R.text_pooled(sd, ids[:, :40], cfg)
    e = rel_l2(got, ref)
    print(f"  TEXT S=40: hip {e:.3e}")
    assert e <= 2.0 * 2e-2 + 2e-3                                                        # the S = 64 yardstick measured on the CPU (2e-2)


# ---- 5. the verifier, end to end ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_latents_decoded_buffers_and_png_score_bit_identically(dev, tmp_path):
    from reflectionflow_amd.tts import runner
    from tests.test_clip_score_gpu import _small_pipe
    pipe = _small_pipe(dev)
    cfg = SV.TINY_SO400M_224
    v = SV.SiglipScoreVerifier(pipe, SV.synthetic_siglip_state(cfg, 4), SV.synthetic_tokenize(512), 256, 256, SV.tower_config(cfg), threshold=0.5)
    g = torch.Generator().manual_seed(11)
    lat = (torch.randn(3, 256, 64, generator=g) * 1.5).to(dev, BF)
    paths = [runner._save(str(tmp_path / f"c{i}"), lat[i:i + 1], pipe, 256, 256) for i in range(3)]
    halos = [runner.decode_halo(pipe, lat[i:i + 1], 256, 256) for i in range(3)]
    s_lat, l_lat = v.score_batch(lat, [0, 1, 2], prompt="a red cube")
    s_dec, l_dec = v.score_decoded(halos, "a red cube")
    s_dec2, _ = v.score_batch(lat, [0, 1, 2], prompt="a red cube", decoded=halos)
    s_png, l_png = v.score_images(paths, "a red cube")
    torch.cuda.synchronize()
    assert torch.equal(s_lat, s_dec) and torch.equal(s_lat, s_dec2) and torch.equal(s_lat, s_png), (s_lat, s_dec, s_png)
    assert torch.equal(l_lat, l_dec) and torch.equal(l_lat, l_png) and l_lat.dtype == torch.int32 and s_lat.dtype == torch.float32
    assert bool(((s_lat > 0) & (s_lat < 1)).all()) and len(set(s_lat.tolist())) == 3
    assert torch.equal(l_lat, (s_lat >= 0.5).int())
    assert not torch.equal(v.score_images(paths, "two cats")[0], s_png)                 # the prompt matters
    assert "a red cube" in v._text_cache and v.text_embed("a red cube") is v._text_cache["a red cube"]


@torch.no_grad()
@pytest.mark.timeout(600)
def test_reflection_search_through_the_cli_with_the_siglip_verifier(dev, tmp_path, monkeypatch):
    """verifier_args.name = "siglip", --synthetic --small (the 2-layer so400m_384 form: 729 tokens on the streaming attention): every
    round's parents are what nvila_sort_key picks from the returned (score, label) pairs; the threshold sits inside the scores' range,
    so both labels occur"""
    from reflectionflow_amd.tts import cli, search
    from tests.test_clip_score_gpu import _search_cfg
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    cfg = _search_cfg()
    cfg["verifier_args"] = {"name": "siglip", "threshold": 0.5, "seed": 2}
    cfgp, meta = tmp_path / "cfg.json", tmp_path / "meta.jsonl"
    meta.write_text(json.dumps({"prompt": "a red cube left of a blue ball"}) + "\n")

    def run(threshold, out):
        cfg["verifier_args"]["threshold"] = threshold
        cfgp.write_text(json.dumps(cfg))
        return cli.main("reflection", ["--pipeline_config_path", str(cfgp), "--meta_path", str(meta), "--output_dir", str(tmp_path / out), "--synthetic",
                                       "--small"])
    log = run(0.5, "a")
    assert len(log) >= 2
    s0 = sorted(s for s, _ in log[0]["scores"])
    assert len(set(s0)) == 4 and all(0.0 < s < 1.0 for s in s0)
    mid = 0.5 * (s0[1] + s0[2])
    log = run(mid, "b")
    assert sorted(lab for _, lab in log[0]["scores"]) == [0, 0, 1, 1]
    for prev, rec in zip(log, log[1:]):
        want = sorted(range(4), key=lambda i: search.nvila_sort_key(prev["scores"][i][0], prev["scores"][i][1], i))
        assert rec["selected"] == want
        assert [lab for _, lab in prev["scores"]] == [int(s >= mid) for s, _ in prev["scores"]]
