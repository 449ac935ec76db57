"""The training step under the other `model:` switches of the reference's config.yaml: `union_cond_attn: false` (attention mode 2),
`add_cond_attn: true` (block.py:227-228), both, and a `c_factor` on the attention modules (mode 1, block.py:115-122, which overrides
the mask).  hd128 synthetic model (2 DoubleStream + 2 SingleStream blocks, LoRA r = 4) at its smallest geometry with S_cond == S_img
(32 text + 64 image + 64 condition tokens), one sample.

LoRA gradients against the fp32 oracle's autograd (oracle/train_oracle.py, which implements all three switches), torch-bf16 as the
yardstick, by the rule of tests/test_train_gpu.py::test_training_step_flux_width_blocks_vs_fp32_oracle: rel-L2 <= 2 x torch-bf16 +
2e-3.  Recompute / kept / "auto" activations and the captured step must agree bit for bit, as they do in the shipped configuration."""
import pytest
import torch

from oracle import flux_oracle as O
from oracle import train_oracle as TO
from tests.golden_util import SHAPES, build
from tests.test_model_gpu import bf16_oracle, to_product
from tests.test_train_gpu import _compare, _oracle_grads

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHIPPED = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
# name -> (model_config, c_factor, LoRA gradients the fp32 ORACLE leaves non-zero).  With latent_lora: false the LoRA acts on the condition
# rows only, so under the mask alone nothing the loss sees depends on a LoRA factor: every reference gradient is exactly zero and the
# product's must be too (the sharpest leak test there is); add_cond_attn re-opens the path through the DoubleStream blocks (24 of
# the 50 factors); with latent_lora: true the masked attention's backward carries the image rows' own LoRA gradients.
CASES = {
    "no_union": ({"union_cond_attn": False, "add_cond_attn": False, "latent_lora": False}, None, 0),
    "no_union_latent_lora": ({"union_cond_attn": False, "add_cond_attn": False, "latent_lora": True}, None, 50),
    "add_cond": ({"union_cond_attn": True, "add_cond_attn": True, "latent_lora": False}, None, 44),
    "both": ({"union_cond_attn": False, "add_cond_attn": True, "latent_lora": False}, None, 24),
    "c_factor": (dict(SHIPPED), 0.5, 44),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(gc):
    """one sample at the hd128 geometry: 32 text + 8 x 8 image tokens, gc x gc condition tokens"""
    sh = SHAPES["hd128"]
    St, gh = sh["St"], sh["gh"]
    g = torch.Generator().manual_seed(7)
    x_0, cond = torch.randn(1, gh * gh, 64, generator=g), torch.randn(1, gc * gc, 64, generator=g)
    pe, pooled = torch.randn(1, St, 256, generator=g), torch.randn(1, 64, generator=g)
    cond_ids = O.prepare_latent_image_ids(gc, gc)
    cond_ids[:, 2] -= gc
    return dict(x_0=x_0, img_ids=O.prepare_latent_image_ids(gh, gh), pe=pe, pooled=pooled, txt_ids=torch.zeros(St, 3), cond=cond,
                cond_ids=cond_ids, t=torch.tensor([0.5]), x_1=torch.randn(1, gh * gh, 64, generator=g))


def _set_c_factor(model, cf, device=None):
    for n, m in model.named_modules():
        if n.endswith(".attn"):
            if cf is None:
                if hasattr(m, "c_factor"):
                    del m.c_factor
            else:
                m.c_factor = torch.ones(1, 1, device=device) * cf           # generate.py:86-90


def _batch(z, dev):
    d = lambda k, bf=False: z[k].to(dev).to(BF) if bf else z[k].to(dev)   # noqa: E731
    return dict(x_0=d("x_0", True), img_ids=d("img_ids"), prompt_embeds=d("pe", True), pooled_prompt_embeds=d("pooled", True), text_ids=d("txt_ids"),
                condition_latents=d("cond", True), condition_ids=d("cond_ids"), t=d("t"), x_1=d("x_1", True))


def _step(pipe, batch, cfg, ckpt="auto"):
    from reflectionflow_amd.train.step import FluxTrainer, lora_parameters
    tr = FluxTrainer(pipe.transformer, cfg, gradient_checkpointing=ckpt)
    ps = lora_parameters(pipe.transformer)
    for p in ps:
        p.grad = None
    loss = tr.step(batch)
    loss.backward()
    names = [n.replace(".lora_A.default.weight", ".lora_A").replace(".lora_B.default.weight", ".lora_B")
             for n, _ in pipe.transformer.named_parameters() if "lora_" in n]
    return loss.detach().clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in zip(names, ps)}, tr


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: loss"
    for k, v in a[1].items():
        assert (v is None and b[1][k] is None) or torch.equal(v, b[1][k]), f"{what}: {k}"


_MODEL = {}


def _model(dev):
    if not _MODEL:
        om = TO.set_trainable(build("hd128", lora=True).train())
        _MODEL.update(om=om, pipe=to_product(om, dev), z=_inputs(SHAPES["hd128"]["gh"]))
    return _MODEL["om"], _MODEL["pipe"], _MODEL["z"]


@pytest.mark.parametrize("case", list(CASES))
def test_lora_gradients_vs_fp32_oracle(dev, case):
    cfg, cf, nonzero = CASES[case]
    om, pipe, z = _model(dev)
    d = lambda k: z[k].to(dev)   # noqa: E731
    args = lambda c: (c(d("x_0")), d("img_ids"), c(d("pe")), c(d("pooled")), d("txt_ids"), c(d("cond")), d("cond_ids"), d("t"), c(d("x_1")))   # noqa: E731
    import copy
    o32 = TO.set_trainable(copy.deepcopy(om).to(dev).train())
    _set_c_factor(o32, cf, dev)
    loss32, _ = TO.training_step(o32, *args(lambda x: x), cfg, conditioning_dtype=BF)
    loss32.backward()
    ref = {k: v.cpu() for k, v in _oracle_grads(o32).items()}
    ob = TO.set_trainable(bf16_oracle(o32).train())
    for p in ob.parameters():
        p.grad = None
    _set_c_factor(ob, cf, dev)
    loss_b, _ = TO.training_step(ob, *args(lambda x: x.to(BF)), cfg, dtype=BF)
    loss_b.backward()
    tbf = {k: (None if v is None else v.cpu()) for k, v in _oracle_grads(ob).items()}
    _set_c_factor(pipe.transformer, cf)
    batch = _batch(z, dev)
    try:
        res = {ck: _step(pipe, batch, cfg, ck) for ck in (True, False, "auto")}
    finally:
        _set_c_factor(pipe.transformer, None)
    shipped = _step(pipe, batch, dict(SHIPPED, latent_lora=cfg["latent_lora"]))      # must compute something else: the switch reaches the kernels
    loss, grads, _ = res[True]
    l32 = float(loss32.detach())
    print(f"  {case}: loss hip {float(loss):.5f} torch-bf16 {float(loss_b):.5f} fp32 {l32:.5f} (shipped config: {float(shipped[0]):.5f})")
    assert abs(float(loss) - l32) <= 2 * abs(float(loss_b) - l32) + 2e-2 * l32
    n, worst, tight = _compare(case, {k: (None if v is None else v.float().cpu()) for k, v in grads.items()}, ref, tbf, add=2e-3)
    print(f"  {case}: {n} non-zero LoRA gradients within 2 x torch-bf16 + 2e-3 (worst ratio to the bound {worst:.2f})")
    assert n == nonzero, (n, nonzero)
    assert res[True][2].kept_blocks == 0 and res[False][2].kept_blocks == 4 and res["auto"][2].kept_blocks == 4
    _same(res[False], res[True], f"{case}: kept activations vs recompute")
    _same(res["auto"], res[True], f"{case}: auto vs recompute")
    assert any(v is not None and not torch.equal(v, shipped[1][k]) for k, v in grads.items()), "the switch changed nothing"


@pytest.mark.parametrize("case", ["both", "c_factor"])
def test_captured_step_is_bit_equal_to_the_eager_step(dev, case):
    from reflectionflow_amd.train.step import FluxTrainer
    cfg, cf, _ = CASES[case]
    oc = {"type": "AdamW", "params": {"lr": 2e-3, "weight_decay": 0.01}}
    z = _inputs(SHAPES["hd128"]["gh"])

    def batches(batch):
        g = torch.Generator(device=dev).manual_seed(5)
        out = []
        for i in range(2):
            b = dict(batch)
            b["x_0"] = (batch["x_0"].float() + 0.1 * i * torch.randn(batch["x_0"].shape, generator=g, device=dev)).to(BF)
            out.append(b)
        return out
    runs = []
    for captured in (False, True):
        pipe = to_product(TO.set_trainable(build("hd128", lora=True).train()), dev)
        _set_c_factor(pipe.transformer, cf)
        tr = FluxTrainer(pipe.transformer, cfg)
        opt = tr.configure_optimizers(oc)
        batch = _batch(z, dev)
        if captured:
            start = opt.bucket.param.clone()
            run = tr.capture_training_step(batch, sample_by_sample=False)
            assert torch.equal(opt.bucket.param, start), "capturing must not train"
            losses = [run(b).clone() for b in batches(batch)]
        else:
            losses = [tr.training_step(b, sample_by_sample=False).clone() for b in batches(batch)]
        torch.cuda.synchronize()
        runs.append((losses, opt.bucket.param.clone(), opt.exp_avg.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), (float(a), float(b))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_add_cond_attn_needs_equal_token_counts(dev):
    from reflectionflow_amd.ops import RFError
    from reflectionflow_amd.train.step import FluxTrainer
    _, pipe, _ = _model(dev)
    batch = _batch(_inputs(SHAPES["hd128"]["gc"]), dev)            # 64 image tokens, 16 condition tokens
    tr = FluxTrainer(pipe.transformer, CASES["add_cond"][0])
    with pytest.raises(RFError, match="S_cond == S_img"):
        tr.step(batch)
    loss = FluxTrainer(pipe.transformer, CASES["no_union"][0]).step(batch)      # the mask alone takes any S_cond
    assert torch.isfinite(loss)


def test_shipped_config_is_untouched(dev, monkeypatch):
    """union_cond_attn: true, add_cond_attn: false: the blocks receive BlockOpts with the new fields at their defaults, and the
    gradients are those of a trainer whose BlockOpts are built from (latent_lora, recompute) alone, bit for bit"""
    from reflectionflow_amd.train import blocks as B
    from reflectionflow_amd.train import step as ST
    _, pipe, z = _model(dev)
    batch = _batch(z, dev)
    seen = []

    def old_opts(latent_lora, recompute, *new):
        seen.append(new)
        return B.BlockOpts(latent_lora, recompute)
    base = _step(pipe, batch, SHIPPED)
    monkeypatch.setattr(ST, "BlockOpts", old_opts)
    other = _step(pipe, batch, SHIPPED)
    monkeypatch.undo()
    assert len(seen) == 4 and all(n == (0, 0.0, False) for n in seen), seen
    _same(other, base, "shipped config")
    assert sum(v is not None and float(v.float().abs().max()) > 0 for v in base[1].values()) >= 44
