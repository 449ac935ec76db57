"""GPU: image-guided denoising (`generate(image_guidance_scale != 1)`, reference generate.py:250-276) on the fast path --
rf_guided_euler_step, rf_flux_denoise_guided, FluxEngine.denoise_guided and the routing in generate().

  1. the guided Euler kernel is BIT-equal to the three bf16 torch element-wise ops of the per-step path followed by the
     existing Euler kernel (it rounds where they round);
  2. the fast path is BIT-equal to the per-step path (forced by a no-op callback) for every condition form, eagerly and as one
     replayed hipGraph, and leaves the condition's generator in the same state;
  3. parity with the fp32 oracle under the project's rule (tests/test_model_gpu.py `check`:
     rel-L2(hip, fp32) <= 2 x rel-L2(eager bf16, fp32) + 2e-3) on the `hd128` loop fixture, T = 4;
  4. the guided call really does not go through the per-step forward, and the fall-back conditions are intact;
  5. generate() cleans up after itself.
"""
import pytest
import torch

from oracle import flux_oracle as O
from tests.golden_util import SHAPES, T, build, load
from tests.test_model_gpu import BF, bf16_oracle, check, g, rel_l2, to_product

pytestmark = pytest.mark.gpu

GEOM, STEPS, SCALE = "hd128", 4, 1.5
CFG = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """The fixture's model as oracle (fp32), eager-bf16 oracle and product pipeline, built once for the module."""
    z = load(f"loop_{GEOM}")
    om = build(GEOM, lora=True)
    return dict(z=z, om=om, ob=bf16_oracle(om), pipe=to_product(om, dev), s=SHAPES[GEOM])


def noop_callback(pipe, i, t, kwargs):
    return {}


def run(world, dev, conds, **kw):
    from reflectionflow_amd.flux.generate import generate
    z, s = world["z"], world["s"]
    kw.setdefault("image_guidance_scale", SCALE)
    return generate(world["pipe"], conditions=conds, model_config=CFG, default_lora=True, height=s["gh"] * 16, width=s["gw"] * 16,
                    num_inference_steps=STEPS, guidance_scale=3.5, latents=g(T(z["lat"]), dev), prompt_embeds=g(T(z["pe"]), dev),
                    pooled_prompt_embeds=g(T(z["pooled"]), dev), output_type="latent", **kw).images.clone()


def token_condition(world, dev):
    from reflectionflow_amd.flux.condition import Condition
    z = world["z"]
    return Condition("cot", tokens=g(T(z["cond"]), dev), ids=T(z["cond_ids"]).to(dev))


class _VaeConfigOnly:
    """What tokens_from_posterior reads off `pipe.vae` for a moments= condition: the shift / scale constants."""

    class config:
        shift_factor, scaling_factor = 0.1159, 0.3611


def moments_condition(world, dev, seed):
    """A moments= condition (mean | logvar of a 16-channel 8 x 8 latent -> 16 tokens) sampling from its own generator."""
    from reflectionflow_amd.flux.condition import Condition
    gen = torch.Generator().manual_seed(11)
    moments = torch.cat([torch.randn(16, 8, 8, generator=gen), torch.randn(16, 8, 8, generator=gen) - 1.0]).to(dev).to(BF)
    gs = torch.Generator().manual_seed(seed)
    return Condition("cot", moments=moments, position_delta=[0, -4]).with_generator(gs), gs


# ---------------------------------------------------------------------------------------------- 1. the kernel
@torch.no_grad()
@pytest.mark.parametrize("scale", [0.0, 1.5, 7.0])
@pytest.mark.parametrize("n", [8, 2048 + 8, 2048 + 8 + 3, "fixture"])
def test_guided_euler_kernel_is_bit_equal_to_the_torch_sequence(dev, n, scale):
    """n = 8: one 16-byte vector; 2048 + 8: one full block of 256 lanes x 8 elements plus a tail vector in a second block;
    + 3: the element-wise tail behind the last whole vector; the fixture's S_img x 64.  Inputs randn * 3 so that the difference,
    the product and the sum all need rounding."""
    from reflectionflow_amd import ops
    if n == "fixture":
        n = SHAPES[GEOM]["gh"] * SHAPES[GEOM]["gw"] * 64
    gen = torch.Generator().manual_seed(n + int(scale * 10))
    x, pred, unc = ((torch.randn(n, generator=gen) * 3).to(dev).to(BF) for _ in range(3))
    dt = -0.0371
    want = x.clone()
    ops.euler_step_(want, unc + scale * (pred - unc), dt)            # the per-step path: generate.py:272 then scheduler.step
    got = x.clone()
    ops.guided_euler_step_(got, pred, unc, scale, dt)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        f"n={n} scale={scale}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} of {n} elements differ"
    if scale == 0.0:                                                   # s = 0: the step is the unconditional prediction's
        only_unc = x.clone()
        ops.euler_step_(only_unc, unc, dt)
        assert torch.equal(got, only_unc)


# ---------------------------------------------------------------------------------------------- 2. fast == per-step
def _fast_step_graph(world, dev, make_condition, monkeypatch):
    """-> (fast eager, per-step, fast as a forced hipGraph, generator states or None)."""
    from reflectionflow_amd import engine as E
    outs, states = [], []
    for kw in ({}, dict(callback_on_step_end=noop_callback)):
        cond, gen = make_condition()
        outs.append(run(world, dev, [cond], **kw))
        states.append(None if gen is None else gen.get_state())
    eng = E.engine_for(world["pipe"].transformer)
    before = set(eng._graphs)
    monkeypatch.setenv("RF_DENOISE_GRAPH", "1")
    for rep in range(2):                                               # capture on first use, replay afterwards
        cond, gen = make_condition()
        outs.append(run(world, dev, [cond]))
        states.append(None if gen is None else gen.get_state())
    new = set(eng._graphs) - before
    assert len(new) == 1 and "guided" in next(iter(new)), "the forced run did not capture a guided graph"
    return outs, states


@torch.no_grad()
def test_fast_path_equals_per_step_path_tokens(world, dev, monkeypatch):
    outs, _ = _fast_step_graph(world, dev, lambda: (token_condition(world, dev), None), monkeypatch)
    fast, step, graph0, graph1 = outs
    assert torch.isfinite(fast.float()).all()
    assert torch.equal(fast, step), f"fast path differs from the per-step path: rel-L2 {rel_l2(fast, step):.3e}"
    assert torch.equal(graph0, fast) and torch.equal(graph1, fast), "graph replay differs from the eager launches"


@torch.no_grad()
def test_fast_path_equals_per_step_path_moments(world, dev, monkeypatch):
    """T + 1 posterior samples per call (one for the conditional tokens, one per step for the unconditional pass): same draws
    in the same order from the condition's generator on both paths, and the generator ends in the same state."""
    monkeypatch.setattr(world["pipe"], "vae", _VaeConfigOnly(), raising=False)
    outs, states = _fast_step_graph(world, dev, lambda: moments_condition(world, dev, seed=5), monkeypatch)
    fast, step, graph0, graph1 = outs
    assert torch.equal(fast, step), f"fast path differs from the per-step path: rel-L2 {rel_l2(fast, step):.3e}"
    assert torch.equal(graph0, fast) and torch.equal(graph1, fast), "graph replay differs from the eager launches"
    assert all(torch.equal(states[0], s_) for s_ in states[1:]), "the paths leave the condition's generator in different states"
    untouched = torch.Generator().manual_seed(5).get_state()
    assert not torch.equal(states[0], untouched)
    # the per-step samples matter: the same call with another seed gives another result
    other = run(world, dev, [moments_condition(world, dev, seed=6)[0]])
    assert not torch.equal(other, fast)


@torch.no_grad()
def test_fast_path_equals_per_step_path_image_on_hip_vae(world, dev, monkeypatch):
    """Image-form condition through the HIP VAE (2-level synthetic VAE, 32 x 32 image -> 64 tokens): the fast path encodes the
    image once and samples its moments T times; the per-step path re-encodes it every step.  Global RNG on both paths."""
    from PIL import Image
    from reflectionflow_amd.flux import vae as V
    from reflectionflow_amd.flux.condition import Condition
    from reflectionflow_amd.flux.vae_hip import HipVAE
    vcfg = dict(block_out_channels=(64, 128), norm_num_groups=32, mid_block_add_attention=False)
    hv = HipVAE(V.init_synthetic_vae_(V.AutoencoderKL(**vcfg), seed=3).eval().to(dev).to(BF))
    calls = []
    real_encode = hv.encode
    monkeypatch.setattr(hv, "encode", lambda x, *a, **k: (calls.append(1), real_encode(x, *a, **k))[1], raising=False)
    monkeypatch.setattr(world["pipe"], "vae", hv, raising=False)
    monkeypatch.setattr(world["pipe"], "image_processor", V.VaeImageProcessor(vae_scale_factor=16), raising=False)
    px = torch.randint(0, 256, (32, 32, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).numpy()
    cond = Condition("cot", condition=Image.fromarray(px), position_delta=[0, -4])
    outs, n_enc, rng = [], [], []
    for kw in ({}, dict(callback_on_step_end=noop_callback)):
        torch.manual_seed(21)
        del calls[:]
        outs.append(run(world, dev, [cond], **kw))
        n_enc.append(len(calls))
        rng.append((torch.get_rng_state(), torch.cuda.get_rng_state(dev)))      # (the posterior noise is drawn on the device)
    assert n_enc == [2, STEPS + 1], n_enc                              # fast: the conditional tokens + ONE more for all steps
    assert torch.equal(outs[0], outs[1]), f"fast path differs from the per-step path: rel-L2 {rel_l2(outs[0], outs[1]):.3e}"
    assert all(torch.equal(a, b) for a, b in zip(rng[0], rng[1])), "the paths leave the global RNG in different states"


# ---------------------------------------------------------------------------------------------- 3. parity
@torch.no_grad()
def test_guided_fast_path_vs_fp32_oracle(world, dev):
    z, s, om, ob = world["z"], world["s"], world["om"], world["ob"]
    okw = dict(guidance_scale=3.5, condition_ids=T(z["cond_ids"]), model_config=CFG, image_hw=(s["gh"], s["gw"]))
    tb = O.denoise(ob, T(z["lat"]).to(BF), T(z["pe"]).to(BF), T(z["pooled"]).to(BF), STEPS,
                   condition_latents=T(z["cond"]).to(BF), image_guidance_scale=SCALE, **okw)
    ref = O.denoise(om, T(z["lat"]).clone(), T(z["pe"]), T(z["pooled"]), STEPS, condition_latents=T(z["cond"]),
                    conditioning_dtype=BF, image_guidance_scale=SCALE, **okw)
    plain = O.denoise(om, T(z["lat"]).clone(), T(z["pe"]), T(z["pooled"]), STEPS, condition_latents=T(z["cond"]),
                      conditioning_dtype=BF, **okw)
    assert rel_l2(ref, plain) > 1e-3, "image guidance must move the oracle's result"
    hp = run(world, dev, [token_condition(world, dev)])
    e = check(hp, ref, tb, "guided generate (fast path)")
    print(f"  guided fast path: hip {e[0]:.3e}  torch-bf16 {e[1]:.3e}")
    unguided = run(world, dev, [token_condition(world, dev)], image_guidance_scale=1.0)
    assert rel_l2(hp, unguided) > 1e-3, "image guidance must move the product's result"


# ---------------------------------------------------------------------------------------------- 4. it is the fast path
@torch.no_grad()
def test_guided_generate_does_not_take_the_per_step_forward(world, dev, monkeypatch):
    import reflectionflow_amd.flux.generate as G

    class PerStep(Exception):
        pass

    def refuse(*a, **k):
        raise PerStep("per-step tranformer_forward was called")

    want = run(world, dev, [token_condition(world, dev)])
    monkeypatch.setattr(G, "tranformer_forward", refuse)
    got = run(world, dev, [token_condition(world, dev)])               # one C call: never reaches tranformer_forward
    assert torch.equal(got, want)
    # the cases that must stay on the per-step path still do
    with pytest.raises(PerStep):
        run(world, dev, [token_condition(world, dev)], callback_on_step_end=noop_callback)
    with pytest.raises(PerStep):
        run(world, dev, [token_condition(world, dev)], joint_attention_kwargs={})


# ---------------------------------------------------------------------------------------------- 5. cleanup
@torch.no_grad()
def test_guided_generate_cleans_up(world, dev):
    """No c_factor left behind (generate.py:312-316) and the scheduler stands at step T -- also with condition_scale, which the
    guided loop carries as the same attention bias as the per-step path."""
    pipe = world["pipe"]
    fast = run(world, dev, [token_condition(world, dev)], condition_scale=1.5)
    assert not any(hasattr(m, "c_factor") for m in pipe.transformer.modules())
    assert pipe.scheduler._step_index == STEPS
    step = run(world, dev, [token_condition(world, dev)], condition_scale=1.5, callback_on_step_end=noop_callback)
    assert pipe.scheduler._step_index == STEPS
    assert torch.equal(fast, step)
    assert not torch.equal(fast, run(world, dev, [token_condition(world, dev)]))
