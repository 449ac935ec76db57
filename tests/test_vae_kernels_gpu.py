"""GPU: the VAE kernels of csrc/vae.hip ONE OP AT A TIME, through rf_debug_vae_op -- the host functions rf_vae_decode / rf_vae_encode run
(group_norm, conv3x3, upsample2x, downsample, attention_core, attention), so grids, instantiations and the fold decision are the product's.

Reference: fp64 on the CPU from the same bf16 operands with plain torch (tests/vae_kernel_cases.py).  Bound: tests/test_kernels_gpu.py's
assert_close as it stands (elementwise 1.2e-2 |ref| + 1.2e-2 mean|ref|, rel-L2 < 4e-3) on interior pixels; "exact" = torch.equal.
tests/test_vae_kernels_cpu.py holds fp32 yardsticks with the kernels' roundings to the same bound on the same inputs.
Weights go through the production packer (vae_hip._Packer.conv3 / .norm / .attn).  Every output is prefilled with a NaN bit pattern and
followed by a guard of sentinels that must survive; inputs whose halo an op must not read carry NaN there (GroupNorm, upsample,
downsample, the attention block), the convolution's input has the clean zero halo and the zeroed tail its contract names, and NaN behind.
The workspace holds NaN in every word on entry.
"""
import ctypes as C

import pytest
import torch

from tests import vae_kernel_cases as K
from tests.test_kernels_gpu import assert_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PRE = 0x7FC1                    # prefill: a NaN with a payload -- "untouched" is a bit-pattern check
SENT = 0x7B7B
GUARD, PAD = 8192, 65536        # elements: sentinels behind a buffer, then NaN (what a stray read would pick up)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Buf:
    """n bf16 elements on the device (prefilled with PRE), a guard of sentinels and NaN padding behind them"""

    def __init__(self, dev, n, content=None):
        self.n = n
        self.full = torch.empty(n + GUARD + PAD, dtype=BF, device=dev)
        bits = self.full.view(torch.int16)
        bits.fill_(PRE)
        bits[n:n + GUARD] = SENT
        self.t = self.full[:n]
        if content is not None:
            self.t.copy_(content.reshape(-1).to(dev))

    ptr = property(lambda self: self.full.data_ptr())

    def bits(self):
        return self.t.view(torch.int16).cpu()

    def assert_guard(self, what):
        tail = self.full.view(torch.int16)[self.n:].cpu()
        assert bool((tail[:GUARD] == SENT).all()) and bool((tail[GUARD:] == PRE).all()), f"{what}: wrote behind its output"


def pre_like(*shape):
    return torch.full(shape, PRE, dtype=torch.int16).view(BF)


def padded(x, halo, tail=None):
    """interior [H][W][C] -> flat zero-/NaN-halo image [(H+2)(W+2)][C] (+ `tail` value over the RF_VAE_TAIL_PIXELS behind it)"""
    H, W, Cc = x.shape
    img = torch.full((H + 2, W + 2, Cc), halo, dtype=BF)
    img[1:-1, 1:-1] = x
    flat = img.reshape(-1)
    return flat if tail is None else torch.cat([flat, torch.full((K.TAIL * Cc,), tail, dtype=BF)])


def run_op(dev, op, H, W, Cc=0, inp=None, out=None, residual=None, norm=None, conv=None, attn=None, silu=0, compact=0, groups=K.GN_GROUPS):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.ops import stream_ptr
    lib = L.load()
    d = L.rf_vae_op_desc()
    d.op, d.H, d.W, d.C, d.groups, d.silu, d.compact = op, H, W, Cc, groups, silu, compact
    if norm is not None:
        d.norm = C.pointer(norm)
    if conv is not None:
        d.conv = C.pointer(conv)
    if attn is not None:
        d.attn = C.pointer(attn)
    d.input, d.out, d.residual = inp, out, residual
    n = lib.rf_debug_vae_op(C.byref(d), None)
    assert n > 0, (n, lib.rf_last_error())
    wst = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)         # every bf16 / fp32 word a NaN
    ws = L.rf_workspace()
    ws.base, ws.bytes = wst.data_ptr(), n
    d.ws = C.pointer(ws)
    L.check(lib.rf_debug_vae_op(C.byref(d), stream_ptr()), "rf_debug_vae_op")
    torch.cuda.synchronize()


# ---- ATTN_CORE ------------------------------------------------------------------------------------------------------------------
def attn_core(dev, q, k, v):
    from reflectionflow_amd import _lib as L
    S = q.shape[0]
    qk = Buf(dev, S * 1024, torch.cat([q, k], 1))
    vt = Buf(dev, 512 * S, v.T.contiguous())
    out = Buf(dev, S * 512)
    run_op(dev, L.RF_VAE_OP_ATTN_CORE, 1, S, 512, inp=qk.ptr, residual=vt.ptr, out=out.ptr)
    out.assert_guard(f"attention core S={S}")
    return out.t.cpu().view(S, 512)


@pytest.mark.parametrize("form", K.ATTN_FORMS)
@pytest.mark.parametrize("S", K.ATTN_S)
def test_attn_core_vs_fp64(dev, S, form):
    q, k, v = K.attn_inputs(form, S)
    got = attn_core(dev, q, k, v)
    r = assert_close(got, K.attn_ref64(q, k, v), f"vae_attn_kernel {form} S={S}")
    ry = float((K.attn_yardstick(q, k, v).double() - K.attn_ref64(q, k, v)).norm() / K.attn_ref64(q, k, v).norm())
    print(f"  attn core {form} S={S}: rel-L2 {r:.2e} (yardstick {ry:.2e})")
    assert torch.equal(got, attn_core(dev, q, k, v)), "two launches differ"


@pytest.mark.parametrize("S", K.ATTN_S)
def test_attn_core_routing_is_bit_exact(dev, S):
    """one key per query carries all the weight: a wrong key order between P and V, a wrong K / V^T swizzle or a tile landing in the
    wrong buffer moves a row of v somewhere else -- nothing averages away"""
    q, k, v, pi = K.routing_inputs(S)
    got = attn_core(dev, q, k, v)
    want = v[pi]
    if not torch.equal(got, want):
        bad = (got.view(torch.int16) != want.view(torch.int16))
        rows = torch.nonzero(bad.any(1)).flatten()[:8].tolist()
        cols = torch.nonzero(bad.any(0)).flatten()[:16].tolist()
        raise AssertionError(f"routing S={S}: {int(bad.sum())} elements differ; first rows {rows}, first channels {cols}")


def test_attn_core_workgroup_invariance(dev):
    """S = 192 (three workgroups): the rows of workgroup b do not depend on what the other workgroups' queries hold.  (The entry point has
    one S for queries and keys, so "a launch whose q holds only that block" is a launch with the other blocks' q zeroed.)"""
    q, k, v = K.attn_inputs("plain", 192)
    full = attn_core(dev, q, k, v)
    for b in range(3):
        qb = torch.zeros_like(q)
        qb[64 * b:64 * b + 64] = q[64 * b:64 * b + 64]
        assert torch.equal(attn_core(dev, qb, k, v)[64 * b:64 * b + 64], full[64 * b:64 * b + 64]), f"workgroup {b}"


# ---- GROUP_NORM -----------------------------------------------------------------------------------------------------------------
def pack_norm(dev, gamma, beta):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.flux.vae_hip import _Packer
    m = torch.nn.GroupNorm(K.GN_GROUPS, gamma.numel(), eps=1e-6)
    with torch.no_grad():
        m.weight.copy_(gamma.float())
        m.bias.copy_(beta.float())
    p, n = _Packer(dev), L.rf_vae_norm()
    p.norm(n, m)
    return n, p


def check_group_norm(dev, form, H, W, Cc, variants):
    from reflectionflow_amd import _lib as L
    x, gamma, beta = K.gn_inputs(form, H, W, Cc)
    norm, keep = pack_norm(dev, gamma, beta)
    xin = Buf(dev, (H + 2) * (W + 2) * Cc, padded(x, float("nan")))
    for silu, compact in variants:
        what = f"GroupNorm {form} {H}x{W}x{Cc} silu={silu} compact={compact}"
        ref = K.gn_ref64(x, gamma, beta, silu)
        out = Buf(dev, H * W * Cc if compact else ((H + 2) * (W + 2) + K.TAIL) * Cc)
        run_op(dev, L.RF_VAE_OP_GROUP_NORM, H, W, Cc, inp=xin.ptr, out=out.ptr, norm=norm, silu=int(silu), compact=int(compact))
        out.assert_guard(what)
        if compact:
            got = out.t.cpu().view(H, W, Cc)                       # exactly H W rows: all written (finite), nothing behind them
        else:
            img = out.t.cpu()[:(H + 2) * (W + 2) * Cc].view(H + 2, W + 2, Cc)
            got = img[1:-1, 1:-1]
            ring = img.clone().view(torch.int16)
            ring[1:-1, 1:-1] = 0
            assert not ring.any(), f"{what}: halo ring not exactly zero"
            assert not out.bits()[(H + 2) * (W + 2) * Cc:].any(), f"{what}: tail behind the image not exactly zero"
        r = assert_close(got, ref, what)
        ry = float((K.gn_yardstick(x, gamma, beta, silu).double() - ref).norm() / ref.norm())
        print(f"  {what}: rel-L2 {r:.2e} (yardstick {ry:.2e})")


@pytest.mark.parametrize("form", K.GN_FORMS)
@pytest.mark.parametrize("H,W", K.GN_HW)
@pytest.mark.parametrize("Cc", K.GN_C)
def test_group_norm(dev, Cc, H, W, form):
    check_group_norm(dev, form, H, W, Cc, [(s, c) for s in (False, True) for c in (False, True)])


@pytest.mark.parametrize("form", ("normal", "channel_offset"))
def test_group_norm_capped_grid(dev, form):
    """npix >= GN_BLOCKS * 64: 2048 blocks of 65 padded pixels"""
    H, W, Cc = K.GN_CAPPED
    assert (H + 2) * (W + 2) >= 2048 * 64 and -(-(H + 2) * (W + 2) // 2048) == 65
    check_group_norm(dev, form, H, W, Cc, [(True, False), (False, True)])


# ---- CONV3X3 --------------------------------------------------------------------------------------------------------------------
def pack_conv(dev, m):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.flux.vae_hip import _Packer
    p, cv = _Packer(dev), L.rf_vae_conv()
    p.conv3(cv, m)
    return cv, p


def run_conv(dev, cv, m, x, residual, alias, what):
    """-> interior [H][W][cout]; checks every write outside it"""
    from reflectionflow_amd import _lib as L
    H, W, Ci = x.shape
    Co, Wp = cv.cout, W + 2
    g = cv.fold if (cv.fold > 1 and cv.fold <= W + 3) else 1
    xin = Buf(dev, ((H + 2) * Wp + K.TAIL) * Ci, padded(x, 0.0, tail=0.0))
    first, last = Wp + 1, H * Wp + W                                  # first / last interior pixel
    res_img = None if residual is None else padded(residual, 0.0).view(-1, Co)
    if alias:
        start = res_img.clone()
        start[:first] = pre_like(first, Co)
        start[last + 1:] = pre_like(start.shape[0] - last - 1, Co)
        out = Buf(dev, (H + 2) * Wp * Co, start)
        res_ptr = out.ptr
    else:
        out = Buf(dev, (H + 2) * Wp * Co)
        rb = None if residual is None else Buf(dev, ((H + 2) * Wp + K.TAIL) * Co, torch.cat([res_img.reshape(-1), torch.zeros(K.TAIL * Co, dtype=BF)]))
        res_ptr = None if rb is None else rb.ptr
    run_op(dev, L.RF_VAE_OP_CONV3X3, H, W, inp=xin.ptr, out=out.ptr, residual=res_ptr, conv=cv)
    out.assert_guard(what)
    bits = out.bits().view(-1, Co)
    assert bool((bits[:first] == PRE).all()), f"{what}: wrote above the first interior pixel (top halo row)"
    free = last + 1 + (g - 1)                                         # unfolded: nothing behind the last interior pixel; folded: g - 1 pixels
    assert bool((bits[free:] == PRE).all()), f"{what}: wrote more than {g - 1} pixels behind the last interior pixel (fold {g})"
    return out.t.cpu().view(H + 2, Wp, Co)[1:-1, 1:-1], g


CONV_CASES = [(ci, co, H, W) for (ci, co) in K.CONV_SHAPES for (H, W) in K.CONV_HW] + [K.CONV_NARROW + hw for hw in K.CONV_NARROW_HW]
FOLDS = {(64, 128): 2, (128, 256): 0, (64, 32): 8, (128, 8): 32}


@pytest.mark.parametrize("ci,co,H,W", CONV_CASES)
def test_conv3x3_vs_fp64(dev, ci, co, H, W):
    m = K.conv_module(ci, co)
    cv, keep = pack_conv(dev, m)
    assert cv.fold == FOLDS[(ci, co)]
    x, res = K.conv_inputs(H, W, ci, co)
    for mode in ("plain", "residual", "aliased"):
        what = f"conv3x3 {ci}->{co} {H}x{W} {mode}"
        got, g = run_conv(dev, cv, m, x, None if mode == "plain" else res, mode == "aliased", what)
        assert g == (cv.fold if 1 < cv.fold <= W + 3 else 1)
        r = assert_close(got, K.conv_ref64(m, x, None if mode == "plain" else res), what)
        print(f"  {what} (fold {g}): rel-L2 {r:.2e}")


@pytest.mark.parametrize("ci,co,H,W", [(64, 128, 5, 29), (128, 256, 5, 29), (64, 32, 7, 40), (128, 8, 5, 28), (128, 8, 5, 29), (128, 8, 5, 40)])
def test_conv3x3_impulse_is_exact(dev, ci, co, H, W):
    """x = a single 1.0, bias 0: the interior is the bf16 weight's taps around that pixel, exactly, and exactly 0 elsewhere"""
    m = K.conv_module(ci, co, zero_bias=True)
    cv, keep = pack_conv(dev, m)
    for n, (py, px) in enumerate(K.impulse_positions(H, W)):
        x = torch.zeros(H, W, ci, dtype=BF)
        x[py, px, (37 * n + 5) % ci] = 1.0
        got, g = run_conv(dev, cv, m, x, None, False, f"conv3x3 impulse {ci}->{co} at {py},{px}")
        want = K.conv_ref64(m, x).to(BF)
        assert torch.equal(want.double(), K.conv_ref64(m, x))        # one product per output: the reference itself is exact
        assert torch.equal(got, want), f"impulse {ci}->{co} {H}x{W} at ({py},{px}) fold {g}: {int((got != want).sum())} elements differ"


# ---- UPSAMPLE2X -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", (64, 512))
@pytest.mark.parametrize("h,w", ((1, 1), (3, 5), (8, 8)))
def test_upsample2x_is_exact(dev, h, w, Cc):
    from reflectionflow_amd import _lib as L
    x = torch.randn(h, w, Cc, generator=K.gen(51, h, w, Cc)).to(BF)
    xin = Buf(dev, (h + 2) * (w + 2) * Cc, padded(x, float("nan")))
    n_img = (2 * h + 2) * (2 * w + 2) * Cc
    out = Buf(dev, n_img + K.TAIL * Cc)
    run_op(dev, L.RF_VAE_OP_UPSAMPLE2X, h, w, Cc, inp=xin.ptr, out=out.ptr)
    out.assert_guard("upsample2x")
    want = padded(x.repeat_interleave(2, 0).repeat_interleave(2, 1), 0.0, tail=0.0)
    assert torch.equal(out.t.cpu().view(torch.int16), want.view(torch.int16)), "upsample2x: interior, zero halo or zero tail differ"


# ---- DOWNSAMPLE -----------------------------------------------------------------------------------------------------------------
def run_down(dev, cv, x, what):
    from reflectionflow_amd import _lib as L
    H, W, Ci = x.shape
    Ho, Wo, Co = H // 2, W // 2, cv.cout
    xin = Buf(dev, (H + 2) * (W + 2) * Ci, padded(x, float("nan")))
    out = Buf(dev, (Ho + 2) * (Wo + 2) * Co)
    run_op(dev, L.RF_VAE_OP_DOWNSAMPLE, H, W, inp=xin.ptr, out=out.ptr, conv=cv)
    out.assert_guard(what)
    bits = out.bits().view(-1, Co)
    assert bool((bits[:Wo + 3] == PRE).all()) and bool((bits[Ho * (Wo + 2) + Wo + 1:] == PRE).all()), f"{what}: wrote outside rows first..last interior"
    return out.t.cpu().view(Ho + 2, Wo + 2, Co)[1:-1, 1:-1]


@pytest.mark.parametrize("Cc", (64, 128))
@pytest.mark.parametrize("H,W", ((2, 2), (4, 6), (16, 10)))
def test_downsample_vs_fp64(dev, H, W, Cc):
    m = K.conv_module(Cc, Cc, stride=2)
    cv, keep = pack_conv(dev, m)
    x, _ = K.conv_inputs(H, W, Cc, Cc)
    what = f"downsample {Cc} {H}x{W}"
    r = assert_close(run_down(dev, cv, x, what), K.conv_ref64(m, x), what)
    print(f"  {what}: rel-L2 {r:.2e}")


@pytest.mark.parametrize("Cc", (64, 128))
def test_downsample_impulse_is_exact(dev, Cc):
    """the pad (0, 1, 0, 1) taps are zero by construction, not read from the (NaN) halo: impulses at the bottom-right pixel, at a pixel
    of the last column and of the last row"""
    H, W = 4, 6
    m = K.conv_module(Cc, Cc, stride=2, zero_bias=True)
    cv, keep = pack_conv(dev, m)
    for n, (py, px) in enumerate(((H - 1, W - 1), (1, W - 1), (H - 1, 2), (2, 3))):
        x = torch.zeros(H, W, Cc, dtype=BF)
        x[py, px, (29 * n + 3) % Cc] = 1.0
        want = K.conv_ref64(m, x).to(BF)
        assert float(want.abs().sum()) > 0
        assert torch.equal(run_down(dev, cv, x, f"downsample impulse {py},{px}"), want), f"downsample impulse at ({py},{px})"


# ---- ATTN_BLOCK -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", K.BLOCK_HW)
def test_attn_block_vs_fp64(dev, H, W):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.flux.vae_hip import _Packer
    m, x = K.block_module(), K.block_input(H, W)
    p, a = _Packer(dev), L.rf_vae_attn()
    p.attn(a, m)
    start = padded(x, float("nan")).view(torch.int16).clone()
    img = start.view(H + 2, W + 2, 512)
    ring = torch.ones(H + 2, W + 2, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    img[ring] = PRE
    buf = Buf(dev, start.numel(), start.view(BF))
    run_op(dev, L.RF_VAE_OP_ATTN_BLOCK, H, W, 512, out=buf.ptr, attn=a)
    what = f"attention block {H}x{W}"
    buf.assert_guard(what)
    got = buf.t.cpu().view(H + 2, W + 2, 512)
    assert bool((got.view(torch.int16)[ring] == PRE).all()), f"{what}: the halo of the in-place image changed"
    ref = K.block_ref64(m, x)
    r = assert_close(got[1:-1, 1:-1], ref, what)
    ry = float((K.block_yardstick(m.float(), x).double() - ref).norm() / ref.norm())
    print(f"  {what}: rel-L2 {r:.2e} (yardstick {ry:.2e})")
