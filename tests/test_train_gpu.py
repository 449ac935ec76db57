"""SURVEY 8f row 4 on the GPU: the backward kernels against torch fp32 autograd of the same maps, then gradient parity of the
whole training step (train_flux/train/model.py:164-238) against

  * the fixture tests/golden/train_step_hd128.npz -- loss and all 50 LoRA gradients RECORDED FROM THE REFERENCE's own step, fp32;
  * the fp32 oracle on the fly at FLUX width (one DoubleStream + one SingleStream block, D = 3072, r = 32).

Tolerance (stated): the HIP path computes in bf16 with fp32 accumulation and hands bf16 gradients between kernels, exactly where
torch's bf16 autograd rounds.  A gradient g is accepted when  rel-L2(g_hip, g_fp32) <= 2 x rel-L2(g_torch_bf16, g_fp32) + 1e-2,
torch_bf16 = the oracle itself run in bf16 on the same GPU; single kernels against fp32 math: rel-L2 <= 1e-2 (bf16 outputs)."""
import math

import numpy as np
import pytest
import torch

from oracle import flux_oracle as O
from oracle import train_oracle as TO
from tests.golden_util import GEOMS, SHAPES, T, build, load
from tests.test_model_gpu import bf16_oracle, rel_l2, to_product

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rnd(dev, *shape, seed=0, sc=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * sc).to(BF)


# ------------------------------------------------------------------------------------------------- row kernels
def test_transpose_gelu_gate(dev):
    from reflectionflow_amd.train import kernels as K
    x = rnd(dev, 100, 328, seed=1)
    xt = K.transpose(x)
    assert xt.shape == (328, 128) and torch.equal(xt[:, :100], x.t()) and float(xt[:, 100:].abs().max()) == 0.0
    assert torch.equal(K.transpose(x[:, 8:72], rows_pad=100), x[:, 8:72].t().contiguous())
    z = rnd(dev, 77, 512, seed=2, sc=2.0)
    zf = z.float().requires_grad_(True)
    h = torch.nn.functional.gelu(zf, approximate="tanh")
    dh = rnd(dev, 77, 512, seed=3)
    h.backward(dh.float())
    assert rel_l2(K.gelu(z), h.detach()) < 4e-3
    assert rel_l2(K.gelu_bwd(z, dh), zf.grad) < 6e-3
    big = z[:, :256]                                                   # a column slice (the single block's mlp half)
    assert torch.equal(K.gelu(big), K.gelu(big.contiguous()))
    f, gate, res, dy = rnd(dev, 300, 256, seed=4), rnd(dev, 256, seed=5), rnd(dev, 300, 256, seed=6), rnd(dev, 300, 256, seed=7)
    y = K.gate_residual(f, gate, res)
    assert rel_l2(y, res.float() + gate.float() * f.float()) < 4e-3
    df, dg = K.gate_bwd(dy, f, gate)
    assert rel_l2(df, dy.float() * gate.float()) < 4e-3
    assert rel_l2(dg, (dy.float() * f.float()).sum(0)) < 1e-5 and dg.dtype == torch.float32
    df2, dg2 = K.gate_bwd(dy, f, gate)
    assert torch.equal(dg, dg2), "column sums must be bit-reproducible"


@pytest.mark.parametrize("rows,D", [(50, 256), (777, 3072), (4608, 3072)])
def test_layernorm_modulate_bwd(dev, rows, D):
    from reflectionflow_amd import ops
    from reflectionflow_amd.train import kernels as K
    x, dy, dres = rnd(dev, rows, D, seed=1, sc=2.0), rnd(dev, rows, D, seed=2), rnd(dev, rows, D, seed=3)
    sc, sh = rnd(dev, D, seed=4, sc=0.5), rnd(dev, D, seed=5)
    xf, scf, shf = x.float().requires_grad_(True), sc.float().requires_grad_(True), sh.float().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xf, (D,), eps=1e-6) * (1 + scf) + shf
    assert rel_l2(ops.layernorm_modulate(x, sc, sh), y.detach()) < 4e-3
    y.backward(dy.float())
    dx, dsc, dsh = K.layernorm_modulate_bwd(x, dy, sc, dres=dres)
    assert rel_l2(dx, xf.grad + dres.float()) < 5e-3
    assert rel_l2(dsc, scf.grad) < 1e-4 and rel_l2(dsh, shf.grad) < 1e-4
    dx0, _, _ = K.layernorm_modulate_bwd(x, dy, sc)
    assert rel_l2(dx0, xf.grad) < 5e-3
    assert torch.equal(K.layernorm_modulate_bwd(x, dy, sc, dres=dres)[1], dsc)


def _ref_norm_rope(x, w, cos, sin, eps, scale):
    """x [S, H, 128] fp32 -> RoPE(RMSNorm(x) * w) * scale (block.py:38-41,60-67 + apply_rotary_emb)"""
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    a, b = y[..., 0::2], y[..., 1::2]
    c0, c1, s0, s1 = cos[:, None, 0::2], cos[:, None, 1::2], sin[:, None, 0::2], sin[:, None, 1::2]
    return torch.stack([a * c0 - b * s0, b * c1 + a * s1], -1).flatten(-2) * scale


@pytest.mark.parametrize("H,S,n_added,extra", [(2, 112, 32, 0), (3, 300, 0, 512)])
def test_qkv_train_fwd_bwd(dev, H, S, n_added, extra):
    from reflectionflow_amd import ops
    from reflectionflow_amd.train import kernels as K
    D = H * 128
    raw = rnd(dev, S, 3 * D + extra, seed=1)
    norms = tuple((1 + 0.1 * rnd(dev, 128, seed=10 + i).float()).to(BF) for i in range(4))
    ids = torch.stack([torch.zeros(S), torch.arange(S) // 8, torch.arange(S) % 8], 1).to(dev)
    cos, sin = (t.contiguous() for t in O.FluxPosEmbed(10000, (16, 56, 56))(ids))
    a = K.qkv_train_fwd(raw, H, n_added, norms if n_added else (norms[0], norms[1], None, None), cos, sin)
    # the no-grad pass of a checkpointed block writes the forward's operands only -- the same bits
    a0 = K.qkv_train_fwd(raw, H, n_added, norms if n_added else (norms[0], norms[1], None, None), cos, sin, backward_operands=False)
    assert a0.v is None and a0.qt is None and a0.kt is None
    assert torch.equal(a0.q, a.q) and torch.equal(a0.k, a.k) and torch.equal(a0.vt, a.vt)
    rf = raw.float().requires_grad_(True)
    tok = torch.arange(S, device=dev)[:, None, None]
    wq = torch.where(tok < n_added, norms[2].float(), norms[0].float())
    wk = torch.where(tok < n_added, norms[3].float(), norms[1].float())
    q = _ref_norm_rope(rf[:, :D].view(S, H, 128), wq, cos, sin, 1e-6, ops.QK_PRESCALE)
    k = _ref_norm_rope(rf[:, D:2 * D].view(S, H, 128), wk, cos, sin, 1e-6, 1.0)
    v = rf[:, 2 * D:3 * D].view(S, H, 128)
    for got, want in ((a.q, q), (a.k, k), (a.v, v)):
        assert rel_l2(got[:, :S], want.detach().permute(1, 0, 2)) < 4e-3
        assert float(got[:, S:].abs().max() if a.s_pad > S else 0.0) == 0.0
    # transposed tiles: element (d, slot(n)) of block n // 32 = x[n][d]
    n = torch.arange(a.s_pad, device=dev)
    slot = 8 * ((n % 16) // 4) + 4 * ((n % 32) // 16) + n % 4
    for tiles, rows in ((a.qt, a.q), (a.kt, a.k)):
        back = tiles[:, n // 32, :, slot]                              # advanced indices split by a slice: result is [s_pad, H, 128]
        assert torch.equal(back.permute(1, 0, 2), rows)
    # vt must be what the forward attention kernel expects: compare attention on it with fp32 softmax
    out = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True)
    qf, kf, vf = (t[:, :S].float() for t in (a.q, a.k, a.v))
    ref = torch.softmax(qf @ kf.transpose(1, 2) * LN2, -1) @ vf
    assert rel_l2(out, ref.permute(1, 0, 2).reshape(S, D)) < 1e-2
    # backward
    dq, dk, dv = rnd(dev, H, a.s_pad, 128, seed=21), rnd(dev, H, a.s_pad, 128, seed=22), rnd(dev, H, a.s_pad, 128, seed=23)
    (q * dq[:, :S].float().permute(1, 0, 2)).sum().backward(retain_graph=True)
    (k * dk[:, :S].float().permute(1, 0, 2)).sum().backward(retain_graph=True)
    (v * dv[:, :S].float().permute(1, 0, 2)).sum().backward()
    d_raw = torch.zeros_like(raw)
    K.qkv_train_bwd(raw, H, n_added, norms if n_added else (norms[0], norms[1], None, None), cos, sin, dq, dk, dv, d_raw)
    assert rel_l2(d_raw[:, :3 * D], rf.grad[:, :3 * D]) < 6e-3
    assert float(d_raw[:, 3 * D:].abs().max() if extra else 0.0) == 0.0


@pytest.mark.parametrize("S,N,R", [(1024, 3072, 32), (1000, 3080, 64), (70, 136, 16), (129, 128, 32), (31, 8, 64), (2560, 12288, 64), (1024, 21504, 128), (300, 512, 208)])
def test_gemm_tn_skinny(dev, S, N, R):
    """out[n, j] = sum_s big[s, n] skinny[s, j] (the LoRA factor gradients) against fp64, both output orientations, operands that
    are column windows of wider buffers, and bit-reproducibility."""
    from reflectionflow_amd.train import kernels as K
    wide, sk_wide = rnd(dev, S, N + 24, seed=5), rnd(dev, S, R + 8, seed=6)
    big, sk = wide[:, 8:8 + N], sk_wide[:, 8:8 + R]
    ref = big.double().t() @ sk.double()
    out = K.gemm_tn(big, sk)
    assert out.shape == (N, R)
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err < 6e-3, err
    outT = torch.zeros(R, N + 16, dtype=BF, device=dev)
    K.gemm_tn(big, sk, transposed=True, out=outT[:, 16:])
    assert torch.equal(outT[:, 16:].t().contiguous(), out) and float(outT[:, :16].abs().max()) == 0.0
    assert torch.equal(K.gemm_tn(big, sk), out)


@pytest.mark.parametrize("H,S", [(2, 112), (3, 256), (2, 1000), (24, 1024), (4, 4608), (8, 2304)])   # (8, 2304): the split-key launches qualify
def test_attention_bwd_vs_fp32_autograd(dev, H, S):
    from reflectionflow_amd import ops
    from reflectionflow_amd.train import kernels as K
    D = H * 128
    raw = rnd(dev, S, 3 * D, seed=3, sc=1.5)
    w = (torch.ones(128, device=dev) * 1.0).to(BF)
    ids = torch.stack([torch.zeros(S), torch.arange(S) // 32, torch.arange(S) % 32], 1).to(dev)
    cos, sin = (t.contiguous() for t in O.FluxPosEmbed(10000, (16, 56, 56))(ids))
    a = K.qkv_train_fwd(raw, H, 0, (w, w, None, None), cos, sin)
    out = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True)
    dout = rnd(dev, S, D, seed=4)
    dq, dk, dv = K.attention_bwd(a, out, dout)
    qf, kf, vf = (t[:, :S].float().detach().requires_grad_(True) for t in (a.q, a.k, a.v))
    ref = torch.softmax(qf @ kf.transpose(1, 2) * LN2, -1) @ vf                  # [H, S, 128]
    assert rel_l2(out, ref.detach().permute(1, 0, 2).reshape(S, D)) < 1e-2
    ref.backward(dout.float().view(S, H, 128).permute(1, 0, 2))
    e = [rel_l2(dq[:, :S], qf.grad), rel_l2(dk[:, :S], kf.grad), rel_l2(dv[:, :S], vf.grad)]
    print(f"  attention bwd H={H} S={S}: rel-L2 dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < 1.2e-2
    if a.s_pad > S:
        assert float(dq[:, S:].abs().max()) == 0.0 and float(dk[:, S:].abs().max()) == 0.0 and float(dv[:, S:].abs().max()) == 0.0
    again = K.attention_bwd(a, out, dout)
    assert all(torch.equal(x, y) for x, y in zip((dq, dk, dv), again)), "the backward must be bit-reproducible (no atomics)"
    # the forward's own row statistics (rf_attn_desc.lse) replace the dq kernel's statistics pass: every forward kernel the library
    # may pick must write log2-sum-exp2 of the scaled score rows, and the gradients must meet the same bound
    s2 = qf.detach().double() @ kf.detach().double().transpose(1, 2)
    lse_ref = torch.logsumexp(s2 * LN2, -1) / LN2                                  # log2 sum_k 2^s2
    # (|s2| <= 128 * 0.128 here: the bounded kernels may run with score_bound = 100)
    # every form must run exactly where its precondition holds (tests/attn_fwd_cases.form_runs) and fail loudly elsewhere
    from tests import attn_fwd_cases as AF
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kernels = [(None, 0.0, True)] + [(f.kernel, 100.0 if f.bounded else 0.0, AF.form_runs(f, H, S, cus)) for f in AF.FORMS + AF.SPLIT_FORMS]
    ran = 0
    for kern, bound, runs in kernels:
        lse = torch.full((H, a.s_pad), float("nan"), dtype=torch.float32, device=dev)
        if not runs:
            with pytest.raises(ops.RFError):                                        # this kernel cannot run this shape
                ops.attention(a.q, a.k, a.vt, S, q_prescaled=True, lse=lse, kernel=kern, score_bound=bound)
            continue
        out2 = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True, lse=lse, kernel=kern, score_bound=bound)
        ran += 1
        assert torch.equal(out2, out) or rel_l2(out2, out) < 2e-2
        err = float((lse[:, :S].double() - lse_ref).abs().max())
        print(f"  forward lse (kernel {kern}) H={H} S={S}: max |lse - ref| = {err:.2e} (log2 units)")
        assert err < 2e-2
        g2 = K.attention_bwd(a, out2, dout, lse=lse)
        e2 = [rel_l2(g2[0][:, :S], qf.grad), rel_l2(g2[1][:, :S], kf.grad), rel_l2(g2[2][:, :S], vf.grad)]
        assert max(e2) < 1.2e-2, e2
        if a.s_pad > S:
            assert all(float(t[:, S:].abs().max()) == 0.0 for t in g2)
            assert bool((lse[:, S:] == 1e30).all()), "padded rows must be closed by the backward"
    assert ran >= 2


_ATTN_CASES = {}


def _attn_bwd_case(dev, H, S):
    """operands, the product forward (+ lse) and the fp32-autograd reference of one (heads, S) -- built once per module"""
    if (H, S) in _ATTN_CASES:
        return _ATTN_CASES[(H, S)]
    from reflectionflow_amd import ops
    from reflectionflow_amd.train import kernels as K
    D = H * 128
    raw = rnd(dev, S, 3 * D, seed=3, sc=1.5)
    w = torch.ones(128, device=dev).to(BF)
    ids = torch.stack([torch.zeros(S), torch.arange(S) // 64, torch.arange(S) % 64], 1).to(dev)
    cos, sin = (t.contiguous() for t in O.FluxPosEmbed(10000, (16, 56, 56))(ids))
    a = K.qkv_train_fwd(raw, H, 0, (w, w, None, None), cos, sin)
    lse = torch.full((H, a.s_pad), float("nan"), dtype=torch.float32, device=dev)
    out = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True, lse=lse)
    dout = rnd(dev, S, D, seed=4)
    gq, gk, gv, lse_ref = [], [], [], []
    for h0 in range(0, H, 4):                                            # fp32 autograd, four heads at a time (S^2 fp32 each)
        qf, kf, vf = (t[h0:h0 + 4, :S].float().detach().requires_grad_(True) for t in (a.q, a.k, a.v))
        s2 = qf @ kf.transpose(1, 2)
        ref = torch.softmax(s2 * LN2, -1) @ vf
        ref.backward(dout.float().view(S, H, 128).permute(1, 0, 2)[h0:h0 + 4])
        assert rel_l2(out.view(S, H, 128)[:, h0:h0 + 4], ref.detach().permute(1, 0, 2)) < 1e-2
        lse_ref.append((torch.logsumexp(s2.detach().double() * LN2, -1) / LN2))
        gq.append(qf.grad), gk.append(kf.grad), gv.append(vf.grad)
        del s2, ref
    case = dict(a=a, out=out, dout=dout, lse=lse, lse_ref=torch.cat(lse_ref), g=(torch.cat(gq), torch.cat(gk), torch.cat(gv)))
    _ATTN_CASES.clear()                                                   # one case resident at a time (24 x 5632 is ~2 GB)
    _ATTN_CASES[(H, S)] = case
    return case


def _bwd_forms():
    from reflectionflow_amd import _lib as L
    dq = [("dq256", L.RF_ATTN_BWD_DQ_256), ("dq128", L.RF_ATTN_BWD_DQ_128), ("dq192", L.RF_ATTN_BWD_DQ_192)]
    dkv = [("dkv128", L.RF_ATTN_BWD_DKV_128), ("dkv192", L.RF_ATTN_BWD_DKV_192), ("dkv128x2", L.RF_ATTN_BWD_DKV_128X2)]
    return dq, dkv


@pytest.mark.parametrize("H,S", [(3, 1000), (5, 448), (24, 2560), (24, 5632), (6, 4608)])
def test_attention_bwd_every_kernel_form(dev, H, S):
    """rf_attention_bwd sizes its two launches by CU rounds, so on a 256-CU part the small test shapes only ever
    reached dq<2,4 waves> + dkv<2>.  Here every dq form {256, 128, 192 queries per workgroup} x every dK / dV form {128, 192, 128 keys
    two-per-CU} is FORCED through rf_attn_bwd_desc.kernel on every shape -- ragged (1000), short (448), the two training shapes
    24 x 2560 (target 512 + condition 512 + text) and 24 x 5632 (target 1024 + condition 512 + text, config.yaml:39-40) and the cfg2
    token count -- with and without the forward's row statistics: dq / dk / dv against fp32 autograd of
    F.scaled_dot_product_attention (block.py:123-125), padded rows exactly zero, the forward's lse against fp64, bit-reproducible, and
    what AUTO picks is one of the forms just checked (rf_debug_last_attn_bwd_path)."""
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.train import kernels as K
    c = _attn_bwd_case(dev, H, S)
    a, out, dout, ref = c["a"], c["out"], c["dout"], c["g"]
    err_lse = float((c["lse"][:, :S].double() - c["lse_ref"]).abs().max())
    print(f"  forward lse H={H} S={S}: max |lse - fp64| = {err_lse:.2e} (log2 units)")
    assert err_lse < 2e-2
    dq_forms, dkv_forms = _bwd_forms()
    worst, results = 0.0, {}
    for given in (True, False):
        for qn, qf_ in dq_forms:
            for kn, kf_ in dkv_forms:
                lse = c["lse"].clone() if given else None
                g = K.attention_bwd(a, out, dout, lse=lse, kernel=qf_ | kf_)
                assert L.load().rf_debug_last_attn_bwd_path() == (qf_ | kf_)
                e = [rel_l2(x[:, :S], r) for x, r in zip(g, ref)]
                worst = max(worst, max(e))
                assert max(e) < 1.2e-2, (qn, kn, given, e)
                if a.s_pad > S:
                    assert all(float(x[:, S:].abs().max()) == 0.0 for x in g), (qn, kn, "padded rows must be zero")
                    if given:
                        assert bool((lse[:, S:] == 1e30).all())
                results[(given, qn, kn)] = g
    print(f"  attention bwd H={H} S={S}: 18 forced form pairs, worst rel-L2 vs fp32 autograd {worst:.2e}")
    # dq depends only on the dq form; dk / dv only on the dK / dV form when the row statistics are the forward's (without them the dq
    # launch computes them for the dK / dV launch, and its forms may round the statistics differently)
    for given in (True, False):
        for qn, _ in dq_forms:
            assert all(torch.equal(results[(given, qn, "dkv128")][0], results[(given, qn, kn)][0]) for kn, _ in dkv_forms)
    for kn, _ in dkv_forms:
        assert all(torch.equal(results[(True, "dq256", kn)][i], results[(True, qn, kn)][i]) for qn, _ in dq_forms for i in (1, 2))
    # AUTO: one of the forms above, reproducibly
    g_auto = K.attention_bwd(a, out, dout, lse=c["lse"].clone())
    path = L.load().rf_debug_last_attn_bwd_path()
    names = {f: n for n, f in dq_forms + dkv_forms}
    qn, kn = names[path & 0xff], names[path & 0xff00]
    print(f"  AUTO at H={H} S={S}: {qn} + {kn}")
    assert all(torch.equal(x, y) for x, y in zip(g_auto, results[(True, qn, kn)]))
    assert all(torch.equal(x, y) for x, y in zip(K.attention_bwd(a, out, dout, lse=c["lse"].clone()), g_auto)), "not bit-reproducible"
    with pytest.raises(Exception):
        K.attention_bwd(a, out, dout, kernel=7)


def test_fused_lora_node_equals_the_torch_op_construction(dev):
    """train.blocks.fused_lora builds (A_pad, Bs_pad) of sibling linears with ONE launch (rf_lora_fuse) and its backward adds the
    gradients into every lora_A / lora_B `.grad` with one more (rf_lora_unfuse_grads): values and gradients bit-equal to the cat /
    scaling / block_diag / pad construction in torch ops on the same bf16 tensors (a plain linear among the siblings contributes output
    rows and no rank; ranks that are not multiples of 8; a second backward accumulates)."""
    import torch.nn as nn
    from reflectionflow_amd.flux import modules as M
    from reflectionflow_amd.train.blocks import fused_lora

    def lin(i, o, r=None):
        base = nn.Linear(i, o)
        if r is None:
            return base.to(dev, BF)
        l = M.LoraLinear(base, r, 2 * r)
        for p in (l.lora_A["default"].weight, l.lora_B["default"].weight):
            nn.init.normal_(p)
        return l.to(dev, BF)

    def reference(linears):
        As, Bs = [], []
        for l in linears:
            if isinstance(l, M.LoraLinear):
                As.append(torch.cat([l.lora_A[a].weight for a in l.active_adapters], 0))
                Bs.append(torch.cat([l.lora_B[a].weight * l.scaling[a] for a in l.active_adapters], 1))
            else:
                As.append(torch.zeros(0, l.in_features, device=dev, dtype=BF))
                Bs.append(torch.zeros(l.out_features, 0, device=dev, dtype=BF))
        A, B = torch.cat(As, 0), torch.block_diag(*Bs)
        r = A.shape[0]
        rp = (r + 63) // 64 * 64
        return torch.nn.functional.pad(A, (0, 0, 0, rp - r)), torch.nn.functional.pad(B, (0, rp - r))

    torch.manual_seed(0)
    for linears in ([lin(48, 32, 8), lin(48, 16), lin(48, 40, 4)], [lin(64, 24, 32)], [lin(32, 8, 40), lin(32, 8, 40)],
                    [lin(3072, 3072, 32), lin(3072, 3072, 32), lin(3072, 3072, 32), lin(3072, 12288, 32)]):
        A, B = fused_lora(linears)
        A0, B0 = reference(linears)
        assert torch.equal(A, A0) and torch.equal(B, B0)
        ps = [p for l in linears if isinstance(l, M.LoraLinear) for p in (l.lora_A["default"].weight, l.lora_B["default"].weight)]
        gA, gB = torch.randn_like(A), torch.randn_like(B)
        want = torch.autograd.grad([A0, B0], ps, [gA, gB])
        for p in ps:
            p.grad = None
        torch.autograd.backward([A, B], [gA, gB], retain_graph=True)
        for p, y in zip(ps, want):
            assert torch.equal(p.grad, y)
        torch.autograd.backward([A, B], [gA, gB])                      # accumulates: bf16(g + g) = 2 g exactly
        for p, y in zip(ps, want):
            assert torch.equal(p.grad, 2 * y)
    assert fused_lora([lin(8, 8)]) == (None, None)


# ------------------------------------------------------------------------------------------------- the whole step
def _product_step(pipe, batch, cfg):
    from reflectionflow_amd.train.step import FluxTrainer, lora_parameters
    tr = FluxTrainer(pipe.transformer, cfg)
    for p in lora_parameters(pipe.transformer):
        p.grad = None
    loss = tr.step(batch)
    loss.backward()
    grads = {}
    for n, p in pipe.transformer.named_parameters():
        if "lora_" in n:
            grads[n.replace(".lora_A.default.weight", ".lora_A").replace(".lora_B.default.weight", ".lora_B")] = \
                None if p.grad is None else p.grad.float().clone()
    return loss.detach().float(), grads


def _oracle_grads(m, key=lambda n: n.replace(".lora_A.default.weight", ".lora_A").replace(".lora_B.default.weight", ".lora_B")):
    return {key(n): (None if p.grad is None else p.grad.float().clone()) for n, p in TO.lora_parameters(m).items()}


ADD_TOL = 1e-2          # additive term of the gradient rule (module docstring); the ratio to the inference rule's 2e-3 is printed


def _compare(name, hip, ref32, tbf, add=ADD_TOL):
    """every non-zero reference gradient: rel-L2(hip, fp32) <= 2 rel-L2(torch-bf16, fp32) + add.  Returns (#checked, worst ratio to
    that bound, worst ratio to the bound with the inference rule's additive term 2e-3)."""
    worst, worst_tight, checked = 0.0, 0.0, 0
    for n, g32 in ref32.items():
        gh, gb = hip[n], tbf[n]
        if float(g32.abs().max()) == 0.0:
            assert gh is None or float(gh.abs().max()) == 0.0, f"{n}: the reference gradient is exactly zero"
            continue
        assert gh is not None, f"{n}: no gradient"
        e_h, e_b = rel_l2(gh, g32), rel_l2(gb, g32)
        worst, worst_tight = max(worst, e_h / (2 * e_b + add)), max(worst_tight, e_h / (2 * e_b + 2e-3))
        assert e_h <= 2 * e_b + add, f"{name} {n}: rel-L2 hip {e_h:.3e} vs torch-bf16 {e_b:.3e} (+{add:g})"
        checked += 1
    return checked, worst, worst_tight


def test_training_step_hd128_against_the_reference_fixture(dev):
    """2 double + 2 single blocks, LoRA r = 4 on the FLUX-Corrector target list, batch of 2, condition tokens: the loss and all 50
    LoRA gradients of the HIP path vs the gradients the REFERENCE's own step produced (fp32 fixture)."""
    z = load("train_step_hd128")
    om = TO.set_trainable(build("hd128", lora=True).train())
    cfg = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
    ref = {k[5:].replace(".lora_A.default.weight", ".lora_A").replace(".lora_B.default.weight", ".lora_B"): T(z[k]) for k in z if k.startswith("grad/")}
    # torch-bf16 yardstick: the oracle in bf16 on this GPU
    ob = TO.set_trainable(bf16_oracle(om).to(dev).train())
    tb = lambda k: T(z[k]).to(dev)   # noqa: E731
    loss_b, _ = TO.training_step(ob, tb("x_0").to(BF), tb("img_ids"), tb("pe").to(BF), tb("pooled").to(BF), tb("txt_ids"), tb("cond").to(BF),
                                 tb("cond_ids"), tb("t"), tb("x_1").to(BF), cfg, dtype=BF)
    loss_b.backward()
    tbf = {k: (None if v is None else v.cpu()) for k, v in _oracle_grads(ob).items()}
    pipe = to_product(om, dev)
    batch = dict(x_0=tb("x_0").to(BF), img_ids=tb("img_ids"), prompt_embeds=tb("pe").to(BF), pooled_prompt_embeds=tb("pooled").to(BF),
                 text_ids=tb("txt_ids"), condition_latents=tb("cond").to(BF), condition_ids=tb("cond_ids"), t=tb("t"), x_1=tb("x_1").to(BF))
    loss, grads = _product_step(pipe, batch, cfg)
    grads = {k: (None if v is None else v.cpu()) for k, v in grads.items()}
    l32 = float(T(z["loss"]))
    print(f"  loss: hip {float(loss):.5f} torch-bf16 {float(loss_b):.5f} reference fp32 {l32:.5f}")
    assert abs(float(loss) - l32) <= 2 * abs(float(loss_b) - l32) + 2e-2 * l32
    n, worst, tight = _compare("hd128", grads, ref, tbf)
    print(f"  {n} non-zero LoRA gradients within tolerance (worst ratio to the bound {worst:.2f}; to 2 x bf16 + 2e-3: {tight:.2f})")
    assert n == 44
    # bit-reproducible: the same step again
    loss2, grads2 = _product_step(pipe, batch, cfg)
    assert torch.equal(loss, loss2)
    for k, v in grads.items():
        assert (v is None and grads2[k] is None) or torch.equal(v, grads2[k].cpu()), k


def test_kept_activations_give_the_gradients_of_gradient_checkpointing(dev):
    """FluxTrainer(gradient_checkpointing=True | False | "auto"): True is the reference's flag (every block re-runs its forward in the
    backward, transformer.py:139-157), False keeps every block's intermediates, "auto" keeps what fits the free HBM.  The backward runs
    the same kernels on the same operands in all three: loss and every LoRA gradient bit-equal."""
    from reflectionflow_amd.train.step import FluxTrainer, lora_parameters
    z = load("train_step_hd128")
    om = TO.set_trainable(build("hd128", lora=True).train())
    cfg = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
    tb = lambda k: T(z[k]).to(dev)   # noqa: E731
    pipe = to_product(om, dev)
    batch = dict(x_0=tb("x_0").to(BF), img_ids=tb("img_ids"), prompt_embeds=tb("pe").to(BF), pooled_prompt_embeds=tb("pooled").to(BF),
                 text_ids=tb("txt_ids"), condition_latents=tb("cond").to(BF), condition_ids=tb("cond_ids"), t=tb("t"), x_1=tb("x_1").to(BF))
    ps = lora_parameters(pipe.transformer)
    res = {}
    for mode, want_kept in ((True, 0), (False, 8), ("auto", 8)):      # 2 + 2 blocks x batch of 2
        tr = FluxTrainer(pipe.transformer, cfg, gradient_checkpointing=mode)
        for p in ps:
            p.grad = None
        loss = tr.step(batch)
        assert tr.kept_blocks == want_kept, (mode, tr.kept_blocks)
        loss.backward()
        res[mode] = (loss.detach().clone(), [None if p.grad is None else p.grad.clone() for p in ps])
        del loss
    assert sum(g is not None and float(g.float().abs().max()) > 0 for g in res[True][1]) >= 44
    for mode in (False, "auto"):
        assert torch.equal(res[mode][0], res[True][0])
        for a, b in zip(res[mode][1], res[True][1]):
            assert (a is None and b is None) or torch.equal(a, b), mode
    with pytest.raises(Exception):
        FluxTrainer(pipe.transformer, cfg, gradient_checkpointing="sometimes")
    # training_step over the batch of 2: one sample at a time with half the loss each == the batched step up to the accumulation order
    tr = FluxTrainer(pipe.transformer, cfg)
    opt = tr.configure_optimizers({"type": "AdamW", "params": {"lr": 0.0, "weight_decay": 0.0}})
    l_b = tr.training_step(batch, sample_by_sample=False).clone()
    g_b = opt.bucket.grad.float().clone()
    l_s = tr.training_step(batch).clone()                    # default for B > 1 with kept activations
    g_s = opt.bucket.grad.float()
    assert tr.kept_blocks == 4                               # the blocks of ONE sample
    assert abs(float(l_s) - float(l_b)) <= 1.2e-2 * abs(float(l_b)), (float(l_s), float(l_b))      # bf16 losses: three ulps
    assert rel_l2(g_s, g_b) < 5e-3, rel_l2(g_s, g_b)
    print(f"  sample-by-sample vs batched: loss {float(l_s):.5f} / {float(l_b):.5f}, gradient rel-L2 {rel_l2(g_s, g_b):.2e}")


@pytest.mark.parametrize("nd,ns,gh,gc,add", [(1, 1, 32, 16, 2e-3), (2, 2, 64, 32, 2e-3)], ids=["1+1_S1792", "2+2_S5632_cfg4_training_shape"])
def test_training_step_flux_width_blocks_vs_fp32_oracle(dev, nd, ns, gh, gc, add):
    """DoubleStream + SingleStream blocks at FLUX.1-dev width (D = 3072, 24 heads, mlp 12288, LoRA r = 32): loss and LoRA gradients vs
    the fp32 oracle (run on the GPU), torch-bf16 as the yardstick.
      1+1 blocks, 512 text + 1024 image + 256 condition tokens (S = 1792)
      2+2 blocks, 512 text + 4096 image + 1024 condition = S = 5632: the sizes the reference trains at (config.yaml:39-40,
          target_size 1024 / condition_size 512) -- at 24 x 5632 the attention backward runs the forms AUTO picks there
          (test_attention_bwd_every_kernel_form prints them) and the GEMMs their 256^2 / stream-K schedules.
    The additive term of the rule is the inference rule's 2e-3 here (round 4: 1e-2)."""
    torch.manual_seed(0)
    om = O.FluxTransformer2DModel(num_layers=nd, num_single_layers=ns).float()
    O.inject_lora(om, r=32, alpha=32.0)
    O.init_synthetic_(om, seed=3, std=0.02)
    TO.set_trainable(om.train())
    St = 512
    Si, Sc = gh * gh, gc * gc
    g = torch.Generator().manual_seed(5)
    x_0, cond = torch.randn(1, Si, 64, generator=g), torch.randn(1, Sc, 64, generator=g)
    pe, pooled = torch.randn(1, St, 4096, generator=g), torch.randn(1, 768, generator=g)
    txt_ids, img_ids = torch.zeros(St, 3), O.prepare_latent_image_ids(gh, gh)
    cond_ids = O.prepare_latent_image_ids(gc, gc)
    cond_ids[:, 2] -= gc
    t, x_1 = torch.tensor([0.5]), torch.randn(1, Si, 64, generator=g)                    # t * 1000 exact in bf16
    cfg = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
    pipe = to_product(om, dev)
    o32 = om.to(dev)
    d = lambda x: x.to(dev)   # noqa: E731
    loss32, _ = TO.training_step(o32, d(x_0), d(img_ids), d(pe), d(pooled), d(txt_ids), d(cond), d(cond_ids), d(t), d(x_1), cfg,
                                 conditioning_dtype=BF)
    loss32.backward()
    ref = {k: v.cpu() for k, v in _oracle_grads(o32).items()}
    ob = TO.set_trainable(bf16_oracle(o32).train())
    for p in ob.parameters():
        p.grad = None
    loss_b, _ = TO.training_step(ob, d(x_0).to(BF), d(img_ids), d(pe).to(BF), d(pooled).to(BF), d(txt_ids), d(cond).to(BF), d(cond_ids), d(t),
                                 d(x_1).to(BF), cfg, dtype=BF)
    loss_b.backward()
    tbf = {k: (None if v is None else v.cpu()) for k, v in _oracle_grads(ob).items()}
    del o32, ob
    torch.cuda.empty_cache()
    batch = dict(x_0=d(x_0).to(BF), img_ids=d(img_ids), prompt_embeds=d(pe).to(BF), pooled_prompt_embeds=d(pooled).to(BF), text_ids=d(txt_ids),
                 condition_latents=d(cond).to(BF), condition_ids=d(cond_ids), t=d(t), x_1=d(x_1).to(BF))
    loss, grads = _product_step(pipe, batch, cfg)
    grads = {k: (None if v is None else v.cpu()) for k, v in grads.items()}
    l32 = float(loss32)
    print(f"  FLUX-width {nd}+{ns} S={St + Si + Sc}: loss hip {float(loss):.5f} torch-bf16 {float(loss_b):.5f} fp32 {l32:.5f}")
    assert abs(float(loss) - l32) <= 2 * abs(float(loss_b) - l32) + 2e-2 * l32
    n, worst, tight = _compare(f"flux-width {nd}+{ns}", grads, ref, tbf, add=add)
    print(f"  {n} non-zero LoRA gradients within 2 x torch-bf16 + {add:g} (worst ratio to the bound {worst:.2f}; to 2 x bf16 + 2e-3: {tight:.2f})")
    assert n >= 20 * nd
    loss2, grads2 = _product_step(pipe, batch, cfg)                                   # bit-reproducible at the full shape too
    assert torch.equal(loss, loss2)
    assert all((v is None and grads2[k] is None) or torch.equal(v, grads2[k].cpu()) for k, v in grads.items())
