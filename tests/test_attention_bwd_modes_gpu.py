"""rf_attention_bwd in the condition modes of the forward: mode 2 (the main <-> condition blocks masked, `union_cond_attn:
false`) and mode 1 (log(c_factor) added to them), against fp32 autograd through softmax(q k^T ln2 + mask) on the kernels' own bf16
operands (tests/attn_bwd_modes_ref.py, mask built as train_flux/flux/block.py:106-122 builds it).

Shapes: the smallest at which the per-element region test of the kernels can fail (attn_bwd_modes_ref.SHAPES).  Every dq form x
dK / dV form and AUTO, with the kernel's own statistics pass and with the forward's lse of the same mode.  Bound: rel-L2 < 1.2e-2 per
gradient, the number of tests/test_train_gpu.py::test_attention_bwd_vs_fp32_autograd (the fp32 yardstick with the kernels' rounding
points sits at 2.6e-3, tests/test_attention_bwd_modes_cpu.py).  The exactness checks catch what a tolerance cannot: a mask that
leaks."""
import ctypes as C

import pytest
import torch

from oracle import flux_oracle as O
from tests import attn_bwd_modes_ref as R
from tests import workspace_poison as WP

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


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


def _forms(mode):
    from reflectionflow_amd import _lib as L
    dkv = [L.RF_ATTN_BWD_DKV_128, L.RF_ATTN_BWD_DKV_192] + ([L.RF_ATTN_BWD_DKV_128X2] if mode == 0 else [])
    return [0] + [a | b for a in (L.RF_ATTN_BWD_DQ_256, L.RF_ATTN_BWD_DQ_128, L.RF_ATTN_BWD_DQ_192) for b in dkv]


_OPERANDS = {}
_CASES = {}


def _operands(dev, H, S):
    """q, k, v, ... of one (heads, S) from rf_qkv_train_fwd, as tests/test_train_gpu.py::test_attention_bwd_vs_fp32_autograd builds them"""
    if (H, S) not in _OPERANDS:
        from reflectionflow_amd.train import kernels as K
        D = H * 128
        raw = rnd(dev, S, 3 * D, seed=3, sc=1.5)
        w = (torch.ones(128, device=dev) * 1.0).to(BF)
        ids = torch.stack([torch.zeros(S), torch.arange(S) // 32, torch.arange(S) % 32], 1).to(dev)
        cos, sin = (t.contiguous() for t in O.FluxPosEmbed(10000, (16, 56, 56))(ids))
        a = K.qkv_train_fwd(raw, H, 0, (w, w, None, None), cos, sin)
        _OPERANDS[(H, S)] = (a, rnd(dev, S, D, seed=4))
    return _OPERANDS[(H, S)]


def _hm(x, H):
    """token-major [S, H * 128] -> head-major [H, S, 128]"""
    return x.view(x.shape[0], H, 128).permute(1, 0, 2)


def _case(dev, H, S, n_main, mode, bias):
    """operands, the product forward (+ its lse) and the fp32 reference of one (shape, mode): built once, never modified"""
    key = (H, S, n_main, mode, bias)
    if key not in _CASES:
        from reflectionflow_amd import ops
        a, dout = _operands(dev, H, S)
        lse = torch.full((H, a.s_pad), float("nan"), dtype=torch.float32, device=dev)
        out = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True, mode=mode, n_main=n_main, cross_bias=bias, lse=lse)
        ref = R.reference(a.q[:, :S], a.k[:, :S], a.v[:, :S], _hm(dout, H), mode, n_main, bias)
        _CASES[key] = (a, dout, out, lse, ref)
    return _CASES[key]


def _check_grads(got, ref, S, what):
    dq, dk, dv = got
    e = [R.rel_l2(dq[:, :S], ref[1]), R.rel_l2(dk[:, :S], ref[2]), R.rel_l2(dv[:, :S], ref[3])]
    print(f"  {what}: rel-L2 dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < R.BOUND, (what, e)
    for t in got:
        assert t.shape[1] == S or float(t[:, S:].abs().max()) == 0.0, f"{what}: pad rows must be exactly zero"


@pytest.mark.parametrize("name,mode,bias", R.MODES)
@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_modes_vs_fp32_autograd_every_form(dev, H, S, n_main, name, mode, bias):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.train import kernels as K
    a, dout, out, lse, ref = _case(dev, H, S, n_main, mode, bias)
    assert R.rel_l2(_hm(out, H), ref[0]) < 1e-2
    err = float((lse[:, :S].double() - ref[4]).abs().max())
    print(f"  forward lse {name} H={H} S={S} n_main={n_main}: max |lse - fp64| = {err:.2e} (log2 units)")
    assert err < R.LSE_BOUND
    picked = set()
    for kern in _forms(mode):
        for given in (False, True):
            got = K.attention_bwd(a, out, dout, lse=lse.clone() if given else None, kernel=kern, mode=mode, n_main=n_main, cross_bias=bias)
            _check_grads(got, ref, S, f"{name} H={H} S={S} n_main={n_main} kernel=0x{kern:x} lse_given={int(given)}")
            if kern == 0:
                picked.add(L.load().rf_debug_last_attn_bwd_path())
            again = K.attention_bwd(a, out, dout, lse=lse.clone() if given else None, kernel=kern, mode=mode, n_main=n_main, cross_bias=bias)
            assert all(torch.equal(x, y) for x, y in zip(got, again)), "the backward must be bit-reproducible (no atomics)"
    assert all((p & 0xff00) != L.RF_ATTN_BWD_DKV_128X2 for p in picked), "AUTO must not pick the two-per-CU dK / dV form outside mode 0"
    with pytest.raises(L.RFError):
        K.attention_bwd(a, out, dout, kernel=L.RF_ATTN_BWD_DQ_128 | L.RF_ATTN_BWD_DKV_128X2, mode=mode, n_main=n_main, cross_bias=bias)


@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_mask_blocks_exactly(dev, H, S, n_main):
    """mode 2 with dout = 0 on one region: nothing may reach that region's dq rows and dk / dv keys, exactly, in every form"""
    from reflectionflow_amd.train import kernels as K
    a, dout, out, lse, _ = _case(dev, H, S, n_main, 2, 0.0)
    for lo, hi in ((n_main, S), (0, n_main)):
        d0 = dout.clone()
        d0[lo:hi] = 0
        for kern in _forms(2):
            for given in (False, True):
                got = K.attention_bwd(a, out, d0, lse=lse.clone() if given else None, kernel=kern, mode=2, n_main=n_main)
                for t, nm in zip(got, ("dq", "dk", "dv")):
                    assert float(t[:, lo:hi].abs().max()) == 0.0, f"{nm} rows {lo}:{hi} must be exactly zero (kernel 0x{kern:x}, lse_given {given})"
                    assert float(t[:, :S].abs().max()) > 0.0


@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_mask_hides_condition_values_bit_for_bit(dev, H, S, n_main):
    """mode 2: replacing q, k, v of the condition rows by other finite values, magnitudes of 1e4 among them, leaves dq, dk, dv of the
    main rows bit-identical (the main rows of o, dout and -- when given -- lse are the same in both runs, as they are in a real step:
    a main row's forward does not see the condition rows either)"""
    from reflectionflow_amd.train import kernels as K
    a, dout, out, lse, _ = _case(dev, H, S, n_main, 2, 0.0)
    assert torch.equal(R.transposed_tiles(a.q), a.qt) and torch.equal(R.transposed_tiles(a.k), a.kt), "the helper's tiles are rf_qkv_train_fwd's"
    g = torch.Generator(device=dev).manual_seed(11)
    q2, k2, v2 = a.q.clone(), a.k.clone(), a.v.clone()
    for t, sc in ((q2, 0.3), (k2, 2.0), (v2, 3.0)):
        new = torch.randn(H, S - n_main, 128, generator=g, device=dev) * sc
        new[:, :, ::7] = 1e4
        new[:, ::2, 3::11] = -1e4
        t[:, n_main:S] = new.to(BF)
    b = K.AttnOperands(q2, k2, v2, None, R.transposed_tiles(q2), R.transposed_tiles(k2), S, a.s_pad)
    # the condition rows' own forward output and statistics for the new values (fp32 torch; finite: 128 * 1e4 * 1e4 < fp32 max)
    ref_o, _, _, _, ref_lse = R.reference(q2[:, :S], k2[:, :S], v2[:, :S], _hm(dout, H), 2, n_main, 0.0)
    out2, lse2 = out.clone(), lse.clone()
    out2[n_main:] = ref_o.permute(1, 0, 2).reshape(S, H * 128)[n_main:].to(BF)
    lse2[:, n_main:S] = ref_lse[:, n_main:].float()
    assert torch.isfinite(out2.float()).all() and torch.isfinite(lse2[:, :S]).all()
    for kern in _forms(2):
        for given in (False, True):
            base = K.attention_bwd(a, out, dout, lse=lse.clone() if given else None, kernel=kern, mode=2, n_main=n_main)
            got = K.attention_bwd(b, out2, dout, lse=lse2.clone() if given else None, kernel=kern, mode=2, n_main=n_main)
            for x, y, nm in zip(base, got, ("dq", "dk", "dv")):
                WP.assert_live(x[:, :n_main], nm)
                WP.assert_same_bits(y[:, :n_main], x[:, :n_main], f"{nm} of the main rows (kernel 0x{kern:x}, lse_given {given})")


@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_zero_bias_is_mode_0_bit_for_bit(dev, H, S, n_main):
    """mode 1 with cross_bias = 0 adds 0.0f to every score: the same bits as mode 0, form by form (one lse for both)"""
    from reflectionflow_amd import ops
    from reflectionflow_amd.train import kernels as K
    a, dout = _operands(dev, H, S)
    lse = torch.empty(H, a.s_pad, dtype=torch.float32, device=dev)
    out = ops.attention(a.q, a.k, a.vt, S, q_prescaled=True, lse=lse)
    for kern in _forms(1):
        for given in (False, True):
            base = K.attention_bwd(a, out, dout, lse=lse.clone() if given else None, kernel=kern)
            got = K.attention_bwd(a, out, dout, lse=lse.clone() if given else None, kernel=kern, mode=1, n_main=n_main, cross_bias=0.0)
            WP.assert_live(base[0][:, :S], "dq")
            for x, y, nm in zip(base, got, ("dq", "dk", "dv")):
                WP.assert_same_bits(y, x, f"{nm} (kernel 0x{kern:x}, lse_given {given})")


def _bwd_on_scratch(a, o, dout, mode, n_main, bias, kern, lse_given, dot, lse, dsum):
    """rf_attention_bwd on caller-provided scratch (K.attention_bwd allocates its own)"""
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    dq, dk, dv = torch.empty_like(a.q), torch.empty_like(a.q), torch.empty_like(a.q)
    d = L.rf_attn_bwd_desc()
    d.q, d.k, d.v, d.qt, d.kt = a.q.data_ptr(), a.k.data_ptr(), a.v.data_ptr(), a.qt.data_ptr(), a.kt.data_ptr()
    d.o, d.dout, d.ldo, d.lddo = o.data_ptr(), dout.data_ptr(), o.stride(0), dout.stride(0)
    d.dq, d.dk, d.dv, d.dot, d.lse, d.dsum = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dot.data_ptr(), lse.data_ptr(), dsum.data_ptr()
    d.heads, d.S, d.s_pad, d.mode, d.lse_given, d.kernel = a.q.shape[0], a.S, a.s_pad, mode, int(lse_given), kern
    d.n_main, d.cross_bias = n_main, bias
    L.check(L.load().rf_attention_bwd(C.byref(d), stream_ptr()), "rf_attention_bwd")
    return dq, dk, dv


@pytest.mark.parametrize("name,mode,bias", R.MODES)
@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_scratch_content_does_not_matter(dev, H, S, n_main, name, mode, bias):
    """dot, dsum and -- when the kernel makes its own statistics -- lse are scratch: filled with 0xFF bytes (NaN as bf16 and fp32)
    before the call, the gradients are those of the zero-filled run, bit for bit"""
    a, dout, out, lse, _ = _case(dev, H, S, n_main, mode, bias)

    def scratch(kind):
        dot = WP.pattern_words(kind, a.qt.numel(), dev).view(BF).view(a.qt.shape)
        st = [WP.pattern_words(kind, 2 * H * a.s_pad, dev).view(torch.float32).view(H, a.s_pad) for _ in range(2)]
        return dot, st[0], st[1]
    for kern in _forms(mode):
        for given in (False, True):
            res = {}
            for kind in ("zero", "nan"):
                dot, l, dsum = scratch(kind)
                if given:
                    l = lse.clone()
                res[kind] = _bwd_on_scratch(a, out, dout, mode, n_main, bias, kern, given, dot, l, dsum)
            WP.assert_live(res["zero"][0][:, :S], "dq")
            for x, y, nm in zip(res["zero"], res["nan"], ("dq", "dk", "dv")):
                WP.assert_same_bits(y, x, f"{nm} {name} (kernel 0x{kern:x}, lse_given {given})")
