"""GPU: the reflection search's round boundary on the device (csrc/image_handoff.hip through flux/image_hip.py, HipVAE.encode_moments_halo,
Condition(moments=...), tts/runner.py's device hand-off).

Everything here is checked BIT FOR BIT against the host path it replaces: VaeImageProcessor.postprocess for the 8-bit levels,
PIL.Image.resize for the resize, VaeImageProcessor.preprocess + .to(bf16) for the encoder input, `candidate_condition(device=False)` for
the condition tokens, and a whole synthetic search with `device_handoff: false` for the files, scores and latents.  The decode count
pins the point of the feature: one VAE decode per generated candidate and rank, at most one VAE encode per distinct parent and round.
"""
import json
import os

import numpy as np
import pytest
import torch

from reflectionflow_amd.tts import clip_verifier as CV
from tests import pil_resize_ref as PR

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = dict(text=dict(vocab=300, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
            vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=14), projection_dim=64)
SMALL_FLUX = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, joint_attention_dim=256, pooled_projection_dim=64)
SMALL_VAE = dict(block_out_channels=(64, 64, 128, 128), norm_num_groups=32, mid_block_add_attention=False)   # 8x, HIP VAE shapes
N, R = 4, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _small_pipe(dev):
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    pipe = FluxPipeline.synthetic(SMALL_FLUX, seed=0, device=dev, with_vae=True, vae_config=SMALL_VAE)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_vae()
    return pipe


def _bits(t):
    return t.contiguous().view(torch.int16)


@torch.no_grad()
@pytest.mark.parametrize("B,H,W,C", [(1, 256, 320, 4), (2, 64, 253, 8), (1, 40, 7, 8)])
def test_image_levels_equals_postprocess(dev, B, H, W, C):
    """The decoder's zero-halo NHWC output (values beyond [-1, 1], garbage in the halo ring and the pad channels) -> exactly the uint8
    image VaeImageProcessor.postprocess(..., "pil") holds.  W % 4 != 0 takes the kernel's byte-store path."""
    from reflectionflow_amd.flux.image_hip import levels_from_halo
    from reflectionflow_amd.flux.vae import VaeImageProcessor
    g = torch.Generator().manual_seed(5 + W)
    x = (torch.rand(B, H, W, 3, generator=g) * 2.6 - 1.3).to(BF)
    x[0, 0, :6, 0] = torch.tensor([-1.0, 1.0, 0.0, 1.0 / 255.0, -3.0, 3.0]).to(BF)[: min(6, W)]
    buf = torch.full((B, H + 2, W + 2, C), 7.0, dtype=BF)
    buf[:, 1:-1, 1:-1, :3] = x
    got = levels_from_halo(buf.to(dev))
    one = levels_from_halo(buf[B - 1].to(dev))
    torch.cuda.synchronize()
    want = VaeImageProcessor(16).postprocess(x.permute(0, 3, 1, 2), output_type="pil")
    assert got.dtype == torch.uint8 and got.shape == (B, H, W, 3) and one.shape == (H, W, 3)
    for b in range(B):
        assert np.array_equal(got[b].cpu().numpy(), np.asarray(want[b])), b
    assert torch.equal(one, got[B - 1])
    assert len(np.unique(got.cpu().numpy())) > 200 or H * W < 1000


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,dst", PR.SIZES)
def test_resize_equals_pil_and_preprocess(dev, src, dst, B):
    """rf_pil_resize_to_vae_input: the uint8 output == PIL.Image.resize, and the halo output == preprocess(that PIL image).to(bf16) as
    zero-halo NHWC with zero pad channels (and the zeroed slack behind it), B images in one launch."""
    from PIL import Image
    from reflectionflow_amd.flux.image_hip import resize_levels
    from reflectionflow_amd.flux.vae import VaeImageProcessor
    (H, W), (h, w) = src, dst
    lv = np.stack([PR.synthetic_levels(H * 3 + W + h + 17 * b, H, W) for b in range(B)])
    torch.full((1 << 22,), float("nan"), device=dev)                      # recycled blocks are not clean: the kernel writes every zero
    small, halo = resize_levels(torch.from_numpy(lv).to(dev), h, w, 64)
    torch.cuda.synchronize()
    assert small.shape == (B, h, w, 3) and small.dtype == torch.uint8 and halo.shape == (B, h + 2, w + 2, 64) and halo.dtype == BF
    for b in range(B):
        pil = Image.fromarray(lv[b]).resize((w, h))
        d = np.abs(small[b].cpu().numpy().astype(np.int32) - np.asarray(pil).astype(np.int32))
        assert int(d.max()) == 0, (b, int(d.max()), float((d > 0).mean()))
        want = torch.zeros(h + 2, w + 2, 64, dtype=BF)
        want[1:-1, 1:-1, :3] = VaeImageProcessor(16).preprocess(pil).to(BF)[0].permute(1, 2, 0)
        assert torch.equal(_bits(halo[b].cpu()), _bits(want)), b
        assert halo[b].is_contiguous() and halo[b].data_ptr() % 16 == 0
    if B == 1:                                                            # the un-batched form
        s1, h1 = resize_levels(torch.from_numpy(lv[0]).to(dev), h, w, 64)
        assert torch.equal(s1, small[0]) and torch.equal(_bits(h1), _bits(halo[0]))


@torch.no_grad()
def test_encode_moments_halo_equals_encode_moments(dev):
    from reflectionflow_amd.flux.image_hip import resize_levels
    from reflectionflow_amd.flux.vae import VaeImageProcessor
    from reflectionflow_amd.ops import RFError
    pipe = _small_pipe(dev)
    lv = PR.synthetic_levels(3, 256, 256)
    small, xp = resize_levels(torch.from_numpy(lv).to(dev), 128, 128, pipe.vae.image_pad)
    from PIL import Image
    x = VaeImageProcessor(16).preprocess(Image.fromarray(small.cpu().numpy())).to(dev, BF)
    want = pipe.vae.encode_moments(x)[0]
    got = pipe.vae.encode_moments_halo(xp)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (32, 16, 16) and torch.equal(_bits(got), _bits(want))
    with pytest.raises(RFError):
        pipe.vae.encode_moments_halo(xp.cpu())
    with pytest.raises(RFError):
        pipe.vae.encode_moments_halo(xp[:, :, :8])


@torch.no_grad()
def test_condition_tokens_device_path_equal_host_path(dev, tmp_path):
    """candidate_condition / _payload_condition on the device == the host path (decode -> PIL -> resize -> preprocess -> one VAE encode
    per child), tokens and ids, for the same latents and seed -- from fresh latents, from a cached decoded buffer, and from a PNG parent."""
    from reflectionflow_amd.tts import runner
    pipe = _small_pipe(dev)
    g = torch.Generator().manual_seed(11)
    for k, (H, W, cs) in enumerate([(256, 256, 128), (256, 384, 128), (128, 128, 256)]):
        lat = (torch.randn(1, (H // 16) * (W // 16), 64, generator=g) * 1.5).to(dev, BF)
        host = runner.candidate_condition(pipe, lat, H, W, cs, device=False)
        devc = runner.candidate_condition(pipe, lat, H, W, cs)
        cached = runner.candidate_condition(pipe, lat, H, W, cs, halo=runner.decode_halo(pipe, lat, H, W))
        png = runner._save(str(tmp_path / f"p{k}"), lat, pipe, H, W)
        png_host = runner._payload_condition(pipe, png, H, W, cs, device=False)
        png_dev = runner._payload_condition(pipe, png, H, W, cs)
        assert host.condition is not None and devc.moments is not None and cached.moments is not None and png_dev.moments is not None
        for seed in (3, 4):
            enc = lambda c: c.with_generator(torch.Generator(device="cpu").manual_seed(seed)).encode(pipe)   # noqa: E731
            t0, i0, k0 = enc(host)
            for other in (devc, cached, png_host, png_dev):
                t1, i1, k1 = enc(other)
                assert t1.shape == t0.shape and torch.equal(_bits(t0), _bits(t1)) and torch.equal(i0, i1) and torch.equal(k0, k1)
        assert not torch.equal(enc(devc)[0], devc.with_generator(torch.Generator(device="cpu").manual_seed(9)).encode(pipe)[0])


@torch.no_grad()
def test_save_writes_the_same_png_on_both_paths(dev, tmp_path):
    from PIL import Image
    from reflectionflow_amd.tts import runner
    pipe = _small_pipe(dev)
    lat = (torch.randn(1, 256, 64, generator=torch.Generator().manual_seed(2)) * 1.5).to(dev, BF)
    a = runner._save(str(tmp_path / "host"), lat, pipe, 256, 256, device=False)
    b = runner._save(str(tmp_path / "dev"), lat, pipe, 256, 256)
    w = runner.PngWriter()
    c = runner._save(str(tmp_path / "thread"), lat, pipe, 256, 256, halo=runner.decode_halo(pipe, lat, 256, 256), writer=w)
    w.close()
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert np.asarray(Image.open(a)).std() > 1.0


# ---- end to end: one synthetic search per setting, with counters around the VAE ------------------------------------------------------
def _search_cfg(handoff):
    from reflectionflow_amd.tts import runner
    cfg = json.load(open(os.path.join(os.path.dirname(runner.__file__), "configs", "flux1_dev_mi355x.json")))
    cfg["pipeline_args"].update(height=256, width=256, condition_size=128, num_inference_steps=2, device_handoff=handoff)
    cfg["search_args"].update(search_branch=N, search_rounds=R)
    cfg["verifier_args"] = {"name": "clip"}
    return cfg


def _run_search(dev, out_dir, handoff):
    """-> (log, {file: bytes}, [candidate latents in generation order], decodes, encodes)"""
    from reflectionflow_amd import _lib
    from reflectionflow_amd.flux.vae_hip import HipVAE
    from reflectionflow_amd.tts import runner, search
    pipe = _small_pipe(dev)
    v = CV.ClipScoreVerifier(pipe, CV.synthetic_clip_state(TINY, 4), CV.synthetic_tokenize(300), 256, 256)
    lib = _lib.load()
    count = {"decode": 0, "encode": 0}
    latents = []
    orig_decode, orig_encode, orig_generate = HipVAE.decode_halo, lib.rf_vae_encode, runner.generate

    def decode_halo(self, z):
        count["decode"] += z.shape[0]
        return orig_decode(self, z)

    def rf_vae_encode(*a):
        count["encode"] += 1
        return orig_encode(*a)

    def generate(*a, **k):
        out = orig_generate(*a, **k)
        latents.append(out.images.detach().clone().cpu())
        return out

    HipVAE.decode_halo, lib.rf_vae_encode, runner.generate = decode_halo, rf_vae_encode, generate
    try:
        log = runner.run_reflection_search(_search_cfg(handoff), ["a red cube left of a blue ball"], out_dir, pipe, search.Shard(0, 1),
                                           score_batch=v.score_batch, score_images=v.score_images)
        torch.cuda.synchronize()
    finally:
        HipVAE.decode_halo, lib.rf_vae_encode, runner.generate = orig_decode, orig_encode, orig_generate
    files = {}
    for root, _, names in os.walk(out_dir):
        for f in names:
            p = os.path.join(root, f)
            files[os.path.relpath(p, out_dir)] = open(p, "rb").read()
    return log, files, latents, count["decode"], count["encode"]


@pytest.fixture(scope="module")
def searches(dev, tmp_path_factory):
    with torch.no_grad():
        on = _run_search(dev, str(tmp_path_factory.mktemp("handoff_on")), True)
        off = _run_search(dev, str(tmp_path_factory.mktemp("handoff_off")), False)
    return on, off


@pytest.mark.timeout(900)
def test_search_is_identical_with_and_without_device_handoff(searches):
    """N = 4, R = 2, CLIP verifier, HIP VAE: search_log.jsonl identical, every PNG the same pixels, every candidate latent bit-equal."""
    from io import BytesIO
    from PIL import Image
    (log1, files1, lat1, _, _), (log0, files0, lat0, _, _) = searches
    assert log1 == log0 and len(log1) == R + 1
    assert files1["00000/search_log.jsonl"] == files0["00000/search_log.jsonl"]
    assert sorted(files1) == sorted(files0)
    pngs = [f for f in files1 if f.endswith(".png")]
    assert len([f for f in pngs if f.startswith(("00000/samples/", "00000/midimg/"))]) == N * (R + 1)
    for f in sorted(files1):
        if f.endswith(".png"):
            a, b = np.asarray(Image.open(BytesIO(files1[f]))), np.asarray(Image.open(BytesIO(files0[f])))
            assert a.shape == (256, 256, 3) and np.array_equal(a, b), f
        assert files1[f] == files0[f], f                                  # the same pixels through the same encoder: the same bytes
    assert len(lat1) == len(lat0) == N * (R + 1)
    for k, (a, b) in enumerate(zip(lat1, lat0)):
        assert a.dtype == BF and torch.equal(_bits(a), _bits(b)), k
    assert len({bytes(_bits(a).numpy().tobytes()) for a in lat1}) == N * (R + 1)      # ... and they are not all one tensor
    for prev, rec in zip(log1, log1[1:]):                                 # the conditions matter: children follow the scores
        assert rec["selected"] == sorted(range(N), key=lambda i: (-prev["scores"][i][0], i))


@pytest.mark.timeout(900)
def test_each_candidate_is_decoded_once_and_each_parent_encoded_once(searches):
    """World 1: N (R + 1) generated candidates -> N (R + 1) VAE decodes (the host path: PNG + verifier + every parent again) and at most
    one rf_vae_encode per distinct parent and round (the host path: one per child)."""
    (log1, _, _, dec1, enc1), (log0, _, _, dec0, enc0) = searches
    parents = sum(len(set(rec["selected"])) for rec in log1[1:])
    print(f"  device hand-off: {dec1} decodes, {enc1} encodes; host path: {dec0} decodes, {enc0} encodes; distinct parents {parents}")
    assert dec1 == N * (R + 1)
    assert 1 <= enc1 <= parents
    assert dec0 == 2 * N * (R + 1) + parents and enc0 == N * R            # what the switch is compared against
