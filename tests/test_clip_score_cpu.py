"""CPU: the CLIP-score verifier's definition and plumbing (reflectionflow_amd/tts/clip_verifier.py, csrc/clip_vision.hip).

* tests/clip_score_ref.py (the fp32 restatement the GPU tests check against) vs transformers 5.15's own CLIPModel and
  CLIPImageProcessorPil (tests/golden/clip_score.npz, tests/golden/make_clip_golden.py): embeddings and logits to fp32 tolerance,
  preprocessing within 1 level on a downscale, an upscale, non-square inputs and odd crop offsets;
* "clip" sorts as a scalar verifier; the runner hands the original prompt to a prompt-aware score_batch and nothing else changes;
* the new header entry points compile as C99.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from reflectionflow_amd.tts import clip_verifier as CV
from reflectionflow_amd.tts import runner, search
from tests import clip_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "clip_score.npz")
CFG = dict(text=dict(vocab=300, hidden=128, heads=2, inter=256, layers=2, max_pos=77),
           vision=dict(hidden=128, heads=2, inter=256, layers=2, image_size=224, patch=14), projection_dim=64)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_records_what_the_generator_says(gold):
    assert str(gold["transformers_version"]) == "5.15.0"
    imgs = [tuple(int(v) for v in r) for r in gold["images"]]
    geo = [R.resize_geometry(H, W) for _, H, W in imgs]
    assert any(H > 224 and W > 224 for _, H, W in imgs) and any(min(H, W) < 224 for _, H, W in imgs)     # down- and upscale
    assert any(H != W for _, H, W in imgs)                                                              # non-square
    assert any(top % 2 == 1 or left % 2 == 1 for _, _, top, left in geo)                                # odd crop offset
    assert geo[0] == (224, 351, 0, 63) and geo[2] == (353, 224, 64, 0)


def test_preprocess_restatement_matches_clip_image_processor(gold):
    """Within 1 level of CLIPImageProcessorPil (fixed-point coefficients) on a small minority of pixels, for every case."""
    for k, (seed, H, W) in enumerate(gold["images"]):
        mine = R.resized_levels(R.synthetic_levels(int(seed), int(H), int(W)))[:, ::4]
        d = (mine - torch.from_numpy(gold["levels_rows4"][k]).float()).abs()
        assert mine.shape == d.shape and float(d.max()) <= 1.0, (k, float(d.max()))
        assert float((d > 0).float().mean()) < 0.15, (k, float((d > 0).float().mean()))


def test_embeddings_and_logits_match_transformers(gold):
    sd = CV.synthetic_clip_state(CFG, int(gold["weight_seed"]))
    ids = torch.from_numpy(gold["ids"])
    assert torch.equal(ids, CV.synthetic_tokenize(CFG["text"]["vocab"])(["a red cube left of a blue ball", "two cats on a sofa"]))
    # image side end to end: the restatement's preprocessing (<= 1 level off the processor) + model vs the fixture's embeddings; the
    # model alone on identical pixels is the next test
    txt = R.text_embeds(sd, ids, CFG["text"]["heads"])
    assert torch.allclose(txt, torch.from_numpy(gold["text_embeds"]), rtol=1e-4, atol=1e-5)
    assert abs(float(sd["logit_scale"]) - float(gold["logit_scale"])) < 1e-6
    pv = torch.stack([R.preprocess_ref(R.synthetic_levels(int(s), int(H), int(W))) for s, H, W in gold["images"]])
    img = R.vision_embeds(sd, pv, CFG["vision"]["heads"])
    ref_img = torch.from_numpy(gold["image_embeds"])
    # the restatement's pixels differ from PIL's by <= 1 level on a handful of pixels: embeddings agree to ~1e-4 relative
    assert float((img - ref_img).norm() / ref_img.norm()) < 1e-3
    logits = torch.stack([R.scores(img, t, float(sd["logit_scale"])) for t in txt], 1)          # [images, texts]
    assert torch.allclose(logits, torch.from_numpy(gold["logits_per_image"]), rtol=1e-3, atol=1e-3)


def test_vision_restatement_matches_transformers_on_identical_pixels(gold):
    """The model half alone at fp32 tolerance: the restatement and transformers' own CLIPModel on identical pixels."""
    sd = CV.synthetic_clip_state(CFG, int(gold["weight_seed"]))
    import transformers as tr
    m = tr.CLIPModel(tr.CLIPConfig(
        text_config=dict(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                         max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1),
        vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=14,
                           hidden_act="quick_gelu"), projection_dim=64)).eval().float()
    m.load_state_dict(sd, strict=False)
    pv = torch.stack([R.preprocess_ref(R.synthetic_levels(int(s), int(H), int(W))) for s, H, W in gold["images"][:2]])
    with torch.no_grad():
        ref = m.get_image_features(pixel_values=pv).pooler_output
    mine = R.vision_embeds(sd, pv, 2)
    assert torch.allclose(mine, ref, rtol=1e-4, atol=1e-5)


def test_patch_rows_layout_is_the_conv():
    """im2col columns (c, ky, kx) zero-padded to 640 against patch_embedding.weight.reshape(hidden, 588): the conv's output."""
    g = torch.Generator().manual_seed(0)
    pv = torch.randn(2, 3, 28, 28, generator=g)
    w = torch.randn(8, 3, 14, 14, generator=g)
    rows = R.patches_of(pv, 14, 640)
    assert rows.shape == (2, 4, 640) and float(rows[..., 588:].abs().max()) == 0.0
    conv = torch.nn.functional.conv2d(pv, w, stride=14).flatten(2).transpose(1, 2)
    assert torch.allclose(rows[..., :588] @ w.reshape(8, 588).t(), conv, atol=1e-4)


def test_png_levels_round_trip_through_the_affine():
    """A PNG's level l read as bf16 with (a, b) = (1/255, 0): rint(255 * clamp(a l + b)) == l in fp32 for every level -- the
    kernel's level step, so an --imgpath image and the latent it was saved from reach the resize with identical levels."""
    l = np.arange(256, dtype=np.float32)
    a = np.float32(1.0 / 255.0)
    u = np.clip(l * a + np.float32(0.0), 0, 1).astype(np.float32)
    assert np.array_equal(np.rint(u * np.float32(255.0)), l)


def test_clip_sorts_as_a_scalar_verifier():
    assert search.SORT_KEYS["clip"] is search.scalar_sort_key
    assert search.select_topk([(0.5, 1), (0.9, 1), (0.5, 1), (0.7, 1)], 3, "clip") == [1, 3, 0]
    tree = search.ReflectionTree("clip")
    assert tree.scalar
    assert runner._evaluation("a.png", (12.5, 1), tree.scalar) == {"image_name": "a.png", "overall_score": {"score": 12.5}}


def test_runner_binds_the_prompt_only_when_asked():
    seen = []

    class V:
        def score_batch(self, latents, seeds, prompt):
            seen.append(prompt)
            return torch.zeros(latents.shape[0]), torch.ones(latents.shape[0], dtype=torch.int32)
        score_batch.wants_prompt = True

    fn = runner.bind_prompt(V().score_batch, "original prompt")
    fn(torch.zeros(2, 4, 64), [1, 2])
    assert seen == ["original prompt"]
    two = lambda latents, seeds: None   # noqa: E731
    assert runner.bind_prompt(two, "p") is two
    assert runner.bind_prompt(search.stub_score_batch, "p") is search.stub_score_batch
    assert runner.bind_prompt(None, "p") is None


def test_runner_hands_the_original_prompt_to_a_prompt_aware_verifier(tmp_path, monkeypatch):
    """A whole reflection search with reflected prompts and verifier "clip": the verifier sees the ORIGINAL prompt every round and
    the parents are the previous round's candidates in descending score order (scalar sort)."""
    import json
    from tests import test_search_tree as TS
    monkeypatch.setattr(runner, "generate", TS._fake_generate)
    cfg = json.load(open(os.path.join(os.path.dirname(runner.__file__), "configs", "flux1_dev_mi355x.json")))
    cfg["pipeline_args"].update(height=64, width=64, condition_size=32, num_inference_steps=1)
    cfg["search_args"].update(search_branch=3, search_rounds=2)
    cfg["verifier_args"] = {"name": "clip"}
    seen = []

    def score_batch(latents, seeds, prompt):
        seen.append(prompt)
        return search.stub_score_batch(latents, seeds)
    score_batch.wants_prompt = True
    logs = runner.run_reflection_search(cfg, ["a red cube"], str(tmp_path), TS._FakePipe(), search.Shard(0, 1), score_batch=score_batch,
                                        reflect=lambda ctx: ["more red"] * 3, refine=lambda ctx, r: ["a redder cube"] * 3)
    assert seen == ["a red cube"] * 3                                  # rounds 0, 1, 2
    assert logs[-1]["prompts"][0] == "a redder cube [Reflexion]: more red"
    for prev, rec in zip(logs, logs[1:]):
        assert rec["selected"] == sorted(range(3), key=lambda i: (-prev["scores"][i][0], i))
        assert "labels" not in next(iter(rec["chains"].values()))      # scalar verifier: no yes / no labels


def test_header_entry_points_compile_as_c99():
    src = ('#include "rf_flux.h"\nint main(void){ rf_clip_vision_weights w = {0}; float s[1];\n'
           'int64_t n = rf_clip_vision_workspace_bytes(&w, 1);\n'
           'int r = rf_clip_preprocess((const void*)0, 0, 0, 0, 0, 1, 1, 1, 0.5f, 0.5f, 224, 14, (void*)0, (void*)0)'
           ' + rf_clip_vision_encode(&w, (const void*)0, 1, (void*)0, (const rf_workspace*)0, (void*)0)'
           ' + rf_clip_score((const void*)0, (const void*)0, 0.f, s, 1, 1, (void*)0);\nreturn (int)(n + r) & 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "c99.c")
        open(c, "w").write(src)
        r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_library_refuses_bad_vision_arguments():
    """Argument validation runs before any launch (no GPU here): NULL weights, a bad geometry, an oversized image."""
    import ctypes as C
    from reflectionflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    w = _lib.rf_clip_vision_weights()
    assert lib.rf_clip_vision_workspace_bytes(C.byref(w), 1) < 0
    assert lib.rf_clip_vision_encode(C.byref(w), None, 1, None, None, None) == -3
    assert lib.rf_clip_preprocess(None, 0, 1, 1, 1, 1, 8, 8, 1.0, 0.0, 224, 14, None, None) == -3
    assert lib.rf_clip_preprocess(16, 0, 1, 1, 1, 1, 9000, 8, 1.0, 0.0, 224, 14, 16, None) == -1
    assert lib.rf_clip_preprocess(16, 0, 1, 1, 1, 1, 64, 64, 1.0, 0.0, 224, 15, 16, None) == -1
    assert lib.rf_clip_score(16, 16, 0.0, 16, 0, 8, None) == -1
