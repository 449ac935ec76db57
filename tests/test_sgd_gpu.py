"""rf_lora_sgd over the flat bucket against torch.optim.SGD on the same bf16 tensors (the reference's third optimizer,
train_flux/train/model.py:107-117): 6 steps per option set, each step started from torch's own state so the comparison is per step;
parameters and momentum buffer within ONE bf16 ulp (tests/test_round5_gpu.py::_ulps_bf16, as the AdamW test)."""
import pytest
import torch

from tests.test_round5_gpu import _params, _ulps_bf16

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

OPTIONS = {
    "plain": dict(lr=0.05),
    "momentum": dict(lr=0.05, momentum=0.9),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True),
    "dampening": dict(lr=0.05, momentum=0.9, dampening=0.1),
    "weight_decay": dict(lr=0.05, momentum=0.9, weight_decay=0.01),
    "maximize": dict(lr=0.05, momentum=0.9, maximize=True),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _grads(ps, g, dev):
    return [(torch.randn(p.shape, generator=g, device=dev) * 0.1).to(BF) for p in ps]


@pytest.mark.parametrize("name", list(OPTIONS))
def test_lora_sgd_kernel_against_torch_sgd(dev, name):
    from reflectionflow_amd.train.optim import FlatLoraBucket, LoraSGD
    kw = OPTIONS[name]
    ps_t, g = _params(dev)
    with torch.no_grad():
        for p in ps_t:
            if float(p.abs().max()) == 0.0:
                p.copy_((torch.randn(p.shape, generator=g, device=dev) * 0.02).to(BF))     # weight decay needs something to decay
    ps_h = [torch.nn.Parameter(p.detach().clone()) for p in ps_t]
    opt_t = torch.optim.SGD(ps_t, **kw)
    opt_h = LoraSGD(FlatLoraBucket(ps_h), **kw)
    bucket = opt_h.bucket
    has_buf = kw.get("momentum", 0.0) != 0.0
    worst = 0.0
    for step in range(1, 7):
        grads = _grads(ps_t, g, dev)
        with torch.no_grad():                                   # start the HIP step from torch's state
            for ph, pt, o in zip(ps_h, ps_t, bucket.offsets):
                ph.copy_(pt)
                if step > 1 and has_buf:
                    opt_h.momentum_buffer[o:o + pt.numel()].copy_(opt_t.state[pt]["momentum_buffer"].reshape(-1))
        for pt, ph, gr in zip(ps_t, ps_h, grads):
            pt.grad = gr.clone()
            ph.grad.copy_(gr)
        before = [p.detach().clone() for p in ps_t]
        opt_t.step()
        opt_h.step()
        for pt, ph, o, b in zip(ps_t, ps_h, bucket.offsets, before):
            n = pt.numel()
            assert not torch.equal(pt.detach(), b), "torch's step moved nothing: the comparison would be empty"
            u = _ulps_bf16(ph.detach(), pt.detach())
            if has_buf:
                u = max(u, _ulps_bf16(opt_h.momentum_buffer[o:o + n].view_as(pt), opt_t.state[pt]["momentum_buffer"]))
            worst = max(worst, u)
    print(f"  rf_lora_sgd[{name}] vs torch.optim.SGD, bf16 state, 6 steps x 6 tensors: worst distance {worst:.2f} bf16 ulp")
    assert worst <= 1.0
    if not has_buf:
        assert float(opt_h.momentum_buffer.float().abs().max()) == 0.0, "momentum = 0 must not touch the buffer"


def test_lora_sgd_fp32_buffer_zero_gradient_and_grad_scale(dev):
    from reflectionflow_amd.train.optim import LoraSGD
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01)
    # fp32 momentum buffer against the formula in fp32, stepping from the HIP path's own bf16 parameters
    ps, g = _params(dev, seed=3)
    opt = LoraSGD(ps, state_dtype=torch.float32, **kw)
    bufs = [None] * len(ps)
    for step in range(1, 7):
        grads = _grads(ps, g, dev)
        for p, gr in zip(ps, grads):
            p.grad.copy_(gr)
        ref = [p.detach().float().clone() for p in ps]
        opt.step()
        for i, (p, r, gr, o) in enumerate(zip(ps, ref, grads, opt.bucket.offsets)):
            gg = (gr.float() + 0.01 * r).to(BF).float()                          # torch rounds the decayed gradient to the tensors' dtype
            bufs[i] = gg.clone() if step == 1 else bufs[i] * 0.9 + 0.9 * gg
            assert _ulps_bf16(p.detach(), (r - 0.05 * bufs[i]).to(BF)) <= 1.0
            m = opt.momentum_buffer[o:o + p.numel()].view_as(p)
            assert float((m - bufs[i]).abs().max()) <= 2e-6 * float(bufs[i].abs().max())
    # an all-zero gradient without weight decay moves nothing, with or without momentum
    for kw0 in (dict(lr=0.05), dict(lr=0.05, momentum=0.9), dict(lr=0.05, momentum=0.9, nesterov=True)):
        pz, _ = _params(dev, seed=4)
        oz = LoraSGD(pz, **kw0)
        start = oz.bucket.param.clone()
        for _ in range(3):
            oz.step()
        assert torch.equal(oz.bucket.param, start) and float(oz.momentum_buffer.float().abs().max()) == 0.0
    # grad_scale = the all-reduce's averaging: a SUM of 4 identical ranks with grad_scale 1/4 is the single-rank step
    pa, ga = _params(dev, seed=5)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa, ob = LoraSGD(pa, **kw), LoraSGD(pb, **kw)
    ob.grad_scale = 0.25
    for _ in range(2):
        for p, q in zip(pa, pb):
            gr = (torch.randn(p.shape, generator=ga, device=dev) * 0.1).to(BF)
            p.grad.copy_(gr)
            q.grad.copy_(gr * 4)
        oa.step(), ob.step()
    assert torch.equal(oa.bucket.param, ob.bucket.param)


def test_lora_sgd_state_dict_round_trip_resumes_bit_exactly(dev):
    from reflectionflow_amd.train.optim import LoraSGD, build_optimizer
    oc = {"type": "SGD", "params": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01)}
    pa, g = _params(dev, seed=6)
    oa = build_optimizer(pa, oc)
    assert isinstance(oa, LoraSGD) and oa.param_groups[0]["momentum"] == 0.9
    gs = [_grads(pa, g, dev) for _ in range(6)]

    def run(opt, ps, steps):
        for grads in steps:
            for p, gr in zip(ps, grads):
                p.grad.copy_(gr)
            opt.step()
    run(oa, pa, gs[:3])
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in oa.state_dict().items()}
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    run(oa, pa, gs[3:])
    ob = build_optimizer(pb, {"type": "SGD", "params": dict(lr=1.0)})
    ob.load_state_dict(sd)
    assert ob.step_count == 3 and ob.defaults["lr"] == 0.05 and ob.defaults["nesterov"] is True
    run(ob, pb, gs[3:])
    assert torch.equal(oa.bucket.param, ob.bucket.param) and torch.equal(oa.momentum_buffer, ob.momentum_buffer)
    assert float(oa.momentum_buffer.float().abs().max()) > 0.0
