"""GPU: the CLIP-score verifier on the HIP path (csrc/clip_vision.hip through flux/text_hip.py and tts/clip_verifier.py).

Checker: tests/clip_score_ref.py (fp32), pinned to transformers 5.15's CLIPModel + CLIPImageProcessorPil by tests/test_clip_score_cpu.py.
Tolerance of the model half, as everywhere in this repo: rel-L2(hip, fp32) <= 2 x rel-L2(transformers eager bf16, fp32) + 2e-3.
Preprocessing: at most 1 level off the restatement, on a small fraction of pixels (fp32 summation order).  Batch invariance,
run-to-run stability and PNG-vs-latent scoring are checked bit for bit.
"""
import os
import socket

import numpy as np
import pytest
import torch

from reflectionflow_amd.tts import clip_verifier as CV
from tests import clip_score_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = dict(text=dict(vocab=300, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
            vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=14), projection_dim=64)
WIDE2 = dict(text=TINY["text"], vision=dict(hidden=1024, heads=16, inter=4096, layers=2, image_size=224, patch=14), projection_dim=768)
SMALL_FLUX = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, joint_attention_dim=256, pooled_projection_dim=64)
SMALL_VAE = dict(block_out_channels=(64, 64, 128, 128), norm_num_groups=32, mid_block_add_attention=False)   # 8x, HIP VAE shapes
STEP = 1.0 / (255.0 * min(R.CLIP_STD))          # one 8-bit level in normalised units


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


def bf16_round(sd):
    return {k: v.to(BF).float() for k, v in sd.items()}


def vision_encoder(cfg, seed, dev):
    from reflectionflow_amd.flux.text_hip import HipClipVisionEncoder
    sd = bf16_round(CV.synthetic_clip_state(cfg, seed))
    return sd, HipClipVisionEncoder({k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"},
                                    cfg["vision"]["hidden"] // 64, dev)


def check_patches(got, levels_ref, k_pad):
    """kernel patch rows vs the restatement's normalised levels: bit-equal but where a level differs by one."""
    want = R.patches_of(R.normalise(levels_ref)[None], 14, k_pad).to(BF).float()
    d = (got.float().cpu() - want).abs()
    frac = float((d > 0).float().mean())
    assert float(d.max()) <= STEP + 2e-2, float(d.max())
    assert frac < 0.01, frac
    assert float(got[..., 588:].float().abs().max()) == 0.0
    return frac


@torch.no_grad()
@pytest.mark.parametrize("H,W", [(256, 402), (160, 160), (300, 190), (512, 512), (1024, 1024), (768, 1360)])
def test_preprocess_from_levels_vs_restatement(dev, H, W):
    _, enc = vision_encoder(TINY, 1, dev)
    lv = R.synthetic_levels(H * 7 + W, H, W)
    got = enc.preprocess_levels(lv.to(dev))
    torch.cuda.synchronize()
    assert got.shape == (1, 256, 640)
    frac = check_patches(got[0:1], R.resized_levels(lv), 640)
    print(f"  {H}x{W}: {100 * frac:.3f} % of values one level off the restatement")


@torch.no_grad()
def test_preprocess_from_the_vae_halo_buffer(dev):
    """The decoder's zero-halo NHWC output read in place: interior at (1, 1), channels 0..2 of 4 (channel 3 is garbage)."""
    _, enc = vision_encoder(TINY, 1, dev)
    H, W = 256, 320
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(H, W, 3, generator=g) * 2.4 - 1.2)              # beyond [-1, 1]: the clamp is exercised
    buf = torch.full((H + 2, W + 2, 4), 7.0)
    buf[1:-1, 1:-1, :3] = x
    buf = buf.to(dev, BF)
    out = enc.alloc_patches(1)
    enc.preprocess(buf[1:, 1:], (0, (W + 2) * 4, 4, 1), 0.5, 0.5, out, H, W)
    torch.cuda.synchronize()
    levels = R.decoded_to_levels(buf[1:-1, 1:-1, :3].float().cpu().permute(2, 0, 1))
    check_patches(out, R.resized_levels(levels), 640)


def _yardstick_bf16(sd, cfg, pv, dev):
    """transformers' own CLIPModel in bf16 (eager, on the device): image_embeds."""
    import transformers as tr
    t, v = cfg["text"], cfg["vision"]
    m = tr.CLIPModel(tr.CLIPConfig(
        text_config=dict(vocab_size=t["vocab"], hidden_size=t["hidden"], intermediate_size=t["inter"], num_hidden_layers=t["layers"],
                         num_attention_heads=t["heads"], max_position_embeddings=t["max_pos"], hidden_act="quick_gelu", eos_token_id=2,
                         bos_token_id=0, pad_token_id=1),
        vision_config=dict(hidden_size=v["hidden"], intermediate_size=v["inter"], num_hidden_layers=v["layers"], num_attention_heads=v["heads"],
                           image_size=v["image_size"], patch_size=v["patch"], hidden_act="quick_gelu"),
        projection_dim=cfg["projection_dim"])).eval()
    m.load_state_dict(sd, strict=False)
    m = m.to(dev, BF)
    return m.get_image_features(pixel_values=pv.to(dev, BF)).pooler_output.float()


@torch.no_grad()
@pytest.mark.parametrize("which", ["tiny", "vit_l14"])
def test_vision_embeddings_and_scores_vs_restatement(dev, which):
    """Tiny config and full ViT-L/14 geometry (24 layers, width 1024, 257 tokens; synthetic weights)."""
    from reflectionflow_amd.flux.text_hip import clip_score
    cfg = TINY if which == "tiny" else CV.VIT_L14
    sd, enc = vision_encoder(cfg, 2, dev)
    imgs = [R.synthetic_levels(50 + i, 224 + 37 * i, 300 - 20 * i) for i in range(3)]
    patches = torch.cat([enc.preprocess_levels(x.to(dev)) for x in imgs])
    emb = enc.encode(patches)
    txt = torch.randn(cfg["projection_dim"], generator=torch.Generator().manual_seed(9)).to(dev, BF)
    sc = clip_score(emb, txt, float(sd["logit_scale"]))
    torch.cuda.synchronize()
    pv = torch.stack([R.preprocess_ref(x) for x in imgs])
    sdd = {k: v.to(dev) for k, v in sd.items()}
    ref = R.vision_embeds(sdd, pv.to(dev), cfg["vision"]["heads"]).cpu()
    yard = _yardstick_bf16(sd, cfg, pv, dev).cpu()
    e, e_y = rel_l2(emb, ref), rel_l2(yard, ref)
    ref_sc = R.scores(ref, txt.float().cpu(), float(sd["logit_scale"]))
    bound = 2.0 * e_y + 2e-3
    print(f"  {which}: image embeds hip {e:.3e}  transformers-bf16 {e_y:.3e}; scores {sc.cpu().tolist()} vs {ref_sc.tolist()}")
    assert emb.shape == (3, cfg["projection_dim"]) and torch.isfinite(emb.float()).all()
    assert e <= bound, (e, e_y)
    assert float((sc.cpu() - ref_sc).abs().max()) <= np.exp(float(sd["logit_scale"])) * bound


@torch.no_grad()
def test_scores_are_batch_invariant_and_stable(dev):
    """8 candidates in one call == each alone == a 3 + 5 split, bit for bit, and run to run (full width: the AUTO GEMM policy would
    pick different tilings / split-K for 1, 3, 5 and 8 images)."""
    from reflectionflow_amd.flux.text_hip import clip_score
    sd, enc = vision_encoder(WIDE2, 3, dev)
    imgs = [R.synthetic_levels(70 + i, 256, 256 + 16 * i) for i in range(8)]
    patches = torch.cat([enc.preprocess_levels(x.to(dev)) for x in imgs])
    txt = torch.randn(768, generator=torch.Generator().manual_seed(1)).to(dev, BF)
    ls = float(sd["logit_scale"])
    all8 = clip_score(enc.encode(patches), txt, ls)
    again = clip_score(enc.encode(patches), txt, ls)
    alone = torch.cat([clip_score(enc.encode(patches[i:i + 1]), txt, ls) for i in range(8)])
    split = torch.cat([clip_score(enc.encode(patches[:3]), txt, ls), clip_score(enc.encode(patches[3:]), txt, ls)])
    emb8, emb1 = enc.encode(patches), enc.encode(patches[5:6])
    torch.cuda.synchronize()
    assert torch.equal(all8, again) and torch.equal(all8, alone) and torch.equal(all8, split), (all8, alone, split)
    assert torch.equal(emb8[5:6], emb1)
    assert len(set(all8.tolist())) == 8


def _small_pipe(dev):
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    pipe = FluxPipeline.synthetic(SMALL_FLUX, seed=0, device=dev, with_vae=True, vae_config=SMALL_VAE)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_vae()
    return pipe


@torch.no_grad()
def test_png_path_equals_latent_path(dev, tmp_path):
    """score_images(saved PNG) == score_batch(latents), bit for bit: the PNG holds exactly the levels the kernel forms from the
    decoder's output, and both paths run the same kernels on the same patch rows."""
    from reflectionflow_amd.ops import RFError
    from reflectionflow_amd.tts import runner
    pipe = _small_pipe(dev)
    v = CV.ClipScoreVerifier(pipe, CV.synthetic_clip_state(TINY, 4), CV.synthetic_tokenize(300), 256, 256)
    g = torch.Generator().manual_seed(11)
    lat = (torch.randn(3, 256, 64, generator=g) * 1.5).to(dev, BF)
    paths = [runner._save(str(tmp_path / f"c{i}"), lat[i:i + 1], pipe, 256, 256) for i in range(3)]
    s_lat, l_lat = v.score_batch(lat, [0, 1, 2], prompt="a red cube")
    s_png, l_png = v.score_images(paths, "a red cube")
    s_one = v.score_images(paths[1:2], "a red cube")[0]
    torch.cuda.synchronize()
    assert torch.equal(s_lat, s_png) and torch.equal(s_png[1:2], s_one), (s_lat, s_png)
    assert l_lat.tolist() == [1, 1, 1] and l_png.tolist() == [1, 1, 1]
    assert not torch.equal(v.score_images(paths, "two cats")[0], s_png)       # the prompt matters
    with pytest.raises(RFError, match="no VAE"):
        from reflectionflow_amd.flux.pipeline import FluxPipeline
        CV.ClipScoreVerifier(FluxPipeline.synthetic(SMALL_FLUX, seed=0, device=dev), CV.synthetic_clip_state(TINY, 4),
                             CV.synthetic_tokenize(300), 256, 256)


def _search_cfg():
    import json
    from reflectionflow_amd.tts import runner
    cfg = json.load(open(os.path.join(os.path.dirname(runner.__file__), "configs", "flux1_dev_mi355x.json")))
    cfg["pipeline_args"].update(height=256, width=256, condition_size=128, num_inference_steps=2)
    cfg["search_args"].update(search_branch=4, search_rounds=2)
    cfg["verifier_args"] = {"name": "clip"}
    return cfg


def _run_clip_search(shard, out_dir, dev):
    from reflectionflow_amd.tts import runner
    pipe = _small_pipe(dev)
    v = CV.ClipScoreVerifier(pipe, CV.synthetic_clip_state(TINY, 4), CV.synthetic_tokenize(300), 256, 256)
    return runner.run_reflection_search(_search_cfg(), ["a red cube left of a blue ball"], out_dir, pipe, shard,
                                        score_batch=v.score_batch, score_images=v.score_images)


def _clip_search_worker(rank, world, port, q, out_dir):
    import torch.distributed as dist
    from reflectionflow_amd.tts import search
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    shard = search.init_distributed("gloo")
    log = _run_clip_search(shard, out_dir, torch.device("cuda:0"))
    q.put((rank, log))
    dist.barrier()
    dist.destroy_process_group()


def _tree_bytes(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


@torch.no_grad()
@pytest.mark.timeout(600)
def test_reflection_search_with_clip_world_1_and_2(dev, tmp_path):
    """run_reflection_search with the "clip" verifier: parents = descending score order; gloo world 2 (both ranks on cuda:0) picks
    the same parents and writes the same samples_best/ as world 1."""
    import torch.multiprocessing as mp
    from reflectionflow_amd.tts import search
    log1 = _run_clip_search(search.Shard(0, 1), str(tmp_path / "w1"), dev)
    for prev, rec in zip(log1, log1[1:]):
        assert rec["selected"] == sorted(range(4), key=lambda i: (-prev["scores"][i][0], i))
        assert all(lab == 1 for _, lab in rec["scores"])
    assert len(set(s for s, _ in log1[0]["scores"])) == 4
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_clip_search_worker, args=(r, 2, port, q, str(tmp_path / "w2"))) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=500) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, log in got:
        assert [r.get("selected") for r in log] == [r.get("selected") for r in log1], rank
        assert [r["scores"] for r in log] == [r["scores"] for r in log1], rank
    best1 = _tree_bytes(tmp_path / "w1" / "00000" / "samples_best")
    best2 = _tree_bytes(tmp_path / "w2" / "00000" / "samples_best")
    assert best1 and best1 == best2
