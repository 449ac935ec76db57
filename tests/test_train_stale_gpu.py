"""The whole training step on RECYCLED memory.  Every output and scratch buffer of the training path comes from torch.empty
(train/kernels.py, train/blocks.py, the partials of train/optim.py): in a real run that memory holds what the previous step left, in
the rest of the suite it is almost always fresh zero pages.  Here the caching allocator's free lists are filled with a pattern of
tests/workspace_poison first, and loss, every LoRA gradient, every updated parameter and the optimizer state must be bit-equal to the
run whose recycled memory held zeros.

hd128 synthetic model (2 DoubleStream + 2 SingleStream blocks, LoRA r = 4).  The shipped configuration runs the batch of
test_train_gpu.py::test_training_step_hd128_against_the_reference_fixture (two samples); the variants of test_train_modes_gpu.py that
change which kernels run (no_union_latent_lora: attention mode 2 with LoRA on the image rows; add_cond: the extra gated residual;
c_factor: mode 1) run that file's one-sample batch with S_cond == S_img.  Two optimisation steps per run (forward, backward, clip at
0.5, update): the second one reads the optimizer state the first one wrote and recycles the first one's own activations.

Poisoning (`poison`): synchronise, empty_cache, drop the per-stream scratch caches of train/kernels.py and the clip partials so that
they are allocated again, then allocate every free block the live tensors' segments still hold (torch.cuda.memory_snapshot gives
their sizes), 400 blocks of 4 KiB .. 1 MiB that tile fresh small-pool segments exactly, and 32 MiB blocks that together exceed
1.5 x the step's measured peak (the large pool); fill every one with the pattern -- repeated with a period of 512 bytes, the
allocator's block granularity, so that a block handed out at ANY offset reads the same words -- free them, and go once more over
every (now merged) free block.  The pool constants (small pool: requests <= 1 MiB in 2 MiB segments, split down to 512 bytes; large
pool: a remainder <= 1 MiB is not split off; best-fit reuse) and the memory_snapshot fields are those of torch 2.10's
CUDACachingAllocator; should an upgrade change them, the read-back or the reserved-memory assertion fails, loudly.  Not vacuous:
torch.empty of three sizes reads the pattern back before the step (asserted), and torch.cuda.memory_reserved() does not grow across
the step (asserted): everything the step allocated came out of the poisoned lists.

The captured step: capture_training_step warms up on a stream of its own, calls empty_cache and captures into the graph's private
pool -- by construction none of that memory comes from the caller's free lists, so the reserved-memory assertion cannot hold there
and is not made.  What is asserted: capture and replay, both after poisoning (read-back asserted), are bit-equal to the eager run on
zeros; and a replay that follows a replay of a DIFFERENT batch (the private pool then holds that batch's activations: the
staleness a graph really sees) is bit-equal too."""
import gc

import pytest
import torch

from oracle import train_oracle as TO
from tests.golden_util import SHAPES, T, build, load
from tests.test_model_gpu import to_product
from tests.test_train_modes_gpu import CASES, SHIPPED, _batch, _inputs, _set_c_factor
from tests.workspace_poison import PATTERNS, assert_live, assert_same_bits, pattern_words

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
VARIANTS = {"shipped": (SHIPPED, None), **{k: CASES[k][:2] for k in ("no_union_latent_lora", "add_cond", "c_factor")}}
OPTIMIZERS = {
    "Prodigy": None,                                                        # the shipped config.yaml:55-61
    "AdamW": {"type": "AdamW", "params": {"lr": 2e-3, "weight_decay": 0.01}},
    "SGD": {"type": "SGD", "params": {"lr": 0.05, "momentum": 0.9, "weight_decay": 0.01}},
}
# (variant, gradient_checkpointing, optimizer, captured): every variant with recompute and with kept activations, every optimizer on
# the shipped configuration, the captured step with two optimizers
RUNS = [(v, ck, list(OPTIMIZERS)[(i + j) % 3], False) for i, v in enumerate(VARIANTS) for j, ck in enumerate((True, False))] + \
       [("shipped", True, "SGD", False), ("shipped", True, "Prodigy", True), ("c_factor", False, "AdamW", True)]
PERIOD = 256                     # 16-bit words: 512 bytes, the caching allocator's block granularity
READBACK = (1 << 10, 150 << 10, 4 << 20)      # words: a small-pool block, one near its 1 MiB limit, a large-pool block


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _drop_scratch_caches(opt):
    from reflectionflow_amd.train import kernels as K
    K._PARTIALS.clear()
    K._TN_WS.clear()
    opt._clip_ws = opt._clip_out = None


def _free_blocks():
    """(bytes, small pool?) of every free block the current stream can be served from"""
    out, stream = [], torch.cuda.current_stream().cuda_stream
    for seg in torch.cuda.memory_snapshot():
        if tuple(seg.get("segment_pool_id", (0, 0))) != (0, 0):
            continue                                                         # a captured graph's private pool: no torch.empty gets there
        if seg.get("stream", stream) != stream:
            continue                                                         # freed on another stream (a capture's warm-up): a request from this
        #                                                                      one would open a fresh, larger segment instead and leave its rest
        out += [(b["size"], seg["segment_type"] == "small") for b in seg["blocks"] if b["state"] == "inactive"]
    return out


def poison(kind, dev, peak, opt):
    """every free byte of the caching allocator's default pool <- pattern; -> the 256-word period every recycled block now reads"""
    _drop_scratch_caches(opt)
    gc.collect()                 # a tensor that only a reference cycle keeps (a dropped graph's closures) must die NOW, not after the sweep
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    period = pattern_words(kind, PERIOD, "cpu")
    tmpl = period.repeat((32 << 20) // 2 // PERIOD).to(dev)                  # 32 MiB: a segment of its own, all of it pattern
    if hasattr(opt, "partials"):                                             # Prodigy's partial sums live as long as the optimizer
        opt.partials.view(torch.int16).copy_(tmpl[:opt.partials.numel() * 2])
    T = tmpl.numel()

    def new(nbytes):
        t = torch.empty(nbytes // 2, dtype=torch.int16, device=dev)
        for o in range(0, t.numel(), T):
            t[o:o + T].copy_(tmpl[:min(T, t.numel() - o)])
        return t

    def sweep():
        """One request per free block, of the block's exact size: best fit serves it from that very block, whole.  (A smaller request
        would leave a large-pool remainder of <= 1 MiB unsplit: handed out as slack that no tensor covers.)  Only a small-pool block
        beyond 1 MiB, the pool's largest request, takes two; that pool splits down to 512 bytes."""
        got = []
        for size, small in sorted(_free_blocks(), reverse=True):
            while size > 0:
                n = min(size, 1 << 20) if small else size
                got.append(new(n))
                size -= n
        return got
    # 1. the holes the live tensors' segments keep after empty_cache
    blocks = []
    for _ in range(4):
        got = sweep()
        blocks += got
        if not got:
            break
    # 2. fresh segments.  Small pool: 2 MiB segments tiled exactly by 1 MiB + 512 KiB + ... + 4 KiB + 4 KiB; large pool: 32 MiB blocks
    for _ in range(40):
        blocks += [new(n) for n in [1 << k for k in range(20, 11, -1)] + [4 << 10]]
    total = 0
    while total < 1.5 * peak + (64 << 20):
        blocks.append(new(32 << 20))
        total += 32 << 20
    torch.cuda.synchronize()
    del blocks
    # 3. everything is free now and adjacent blocks have merged: once more over every free block, whatever 1 and 2 left out
    for _ in range(4):
        reserved = torch.cuda.memory_reserved()
        got = sweep()
        torch.cuda.synchronize()
        del got
        if torch.cuda.memory_reserved() == reserved:                         # every request came out of a block that was there
            break
    del tmpl, new
    for n in READBACK:
        t = torch.empty(n, dtype=torch.int16, device=dev)
        back = t.cpu().view(-1, PERIOD)
        assert torch.equal(back, period.expand_as(back)), f"torch.empty({2 * n} bytes) does not read back the {kind} pattern"
        del t
    return period


def _setup(dev, variant):
    cfg, cf = VARIANTS[variant]
    pipe = to_product(TO.set_trainable(build("hd128", lora=True).train()), dev)
    _set_c_factor(pipe.transformer, cf)
    if variant == "shipped":
        z = load("train_step_hd128")
        tb = lambda k: T(z[k]).to(dev)   # noqa: E731
        batch = dict(x_0=tb("x_0").to(BF), img_ids=tb("img_ids"), prompt_embeds=tb("pe").to(BF), pooled_prompt_embeds=tb("pooled").to(BF),
                     text_ids=tb("txt_ids"), condition_latents=tb("cond").to(BF), condition_ids=tb("cond_ids"), t=tb("t"), x_1=tb("x_1").to(BF))
    else:
        batch = _batch(_inputs(SHAPES["hd128"]["gh"]), dev)
    return pipe, cfg, batch


def _state(opt, losses):
    out = dict(param=opt.bucket.param.clone(), grad=opt.bucket.grad.clone())
    out.update({k: getattr(opt, k).clone() for k in opt._STATE_TENSORS})
    out.update({f"loss{i}": l.clone().reshape(1) for i, l in enumerate(losses)})
    return out


def _same_state(got, base, what):
    assert got.keys() == base.keys()
    for k, v in base.items():
        assert_same_bits(got[k], v, f"{what}: {k}")


@pytest.mark.parametrize("variant,ckpt,optimizer,captured", RUNS, ids=lambda v: str(v))
def test_step_on_recycled_memory(dev, variant, ckpt, optimizer, captured):
    from reflectionflow_amd.train.step import FluxTrainer
    pipe, cfg, batch = _setup(dev, variant)
    tr = FluxTrainer(pipe.transformer, cfg, gradient_checkpointing=ckpt, gradient_clip_val=0.5)
    opt = tr.configure_optimizers(OPTIMIZERS[optimizer])
    p0 = opt.bucket.param.clone()
    sd0 = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state_dict().items()}
    other = dict(batch, x_0=(batch["x_0"].float() * 0.5 + 0.25).to(BF))

    def restore():
        with torch.no_grad():
            opt.bucket.param.copy_(p0)
        opt.load_state_dict(sd0)

    def steps():
        return [tr.training_step(batch, sample_by_sample=None).clone() for _ in range(2)]

    # the step's peak, once, on a warm-up from the same starting point (scratch caches dropped as `poison` drops them)
    _drop_scratch_caches(opt)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    steps()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    assert tr.kept_blocks == (0 if ckpt else 4)
    base = None
    for kind in PATTERNS:
        restore()
        poison(kind, dev, peak, opt)
        reserved = torch.cuda.memory_reserved()
        losses = steps()
        torch.cuda.synchronize()
        grew = torch.cuda.memory_reserved() - reserved
        assert grew <= 0, f"[{kind}] the step reserved {grew} more bytes: not everything came from the poisoned free lists (peak {peak})"
        got = _state(opt, losses)
        if base is None:
            base = got
            for k in ("param", "grad"):
                assert_live(base[k], k)
            assert all(bool(torch.isfinite(l)) for l in losses) and float(base["grad"].float().abs().max()) > 0
            assert not torch.equal(base["param"], p0), "the step moved nothing"
        else:
            _same_state(got, base, f"{variant} ckpt={ckpt} {optimizer} [{kind}]")
    if not captured:
        return
    for kind in PATTERNS:
        restore()
        poison(kind, dev, peak, opt)
        run = tr.capture_training_step(batch, sample_by_sample=None)
        assert torch.equal(opt.bucket.param, p0), "capturing must not train"
        losses = [run(batch).clone() for _ in range(2)]
        torch.cuda.synchronize()
        _same_state(_state(opt, losses), base, f"captured {variant} [{kind}]")
        run(other)                                   # the private pool now holds another batch's activations
        restore()
        losses = [run(batch).clone() for _ in range(2)]
        torch.cuda.synchronize()
        _same_state(_state(opt, losses), base, f"captured {variant} [{kind}] after another batch")
        del run
