"""No GPU: (1) rf_debug_vae_op refuses what the VAE kernels of csrc/vae.hip cannot run, before any HIP call -- each refusal returns its
RF_ERR_* code and leaves the product path's message in rf_last_error(); (2) the yardsticks: fp32 restatements of the attention kernel,
the three GroupNorm passes and the attention block that round where the kernels round, held against fp64 under the bound
tests/test_vae_kernels_gpu.py applies to the kernels (tests/test_kernels_gpu.py::assert_close), on every GPU case's inputs -- so a correct
kernel can meet that bound.  The figures are recorded in profiles/vae_kernels.md."""
import ctypes as C

import pytest
import torch

from reflectionflow_amd import _lib as L
from tests import vae_kernel_cases as K
from tests.test_kernels_gpu import assert_close

RF_ERR_SHAPE, RF_ERR_ALIGN, RF_ERR_NULL, RF_ERR_UNSUPPORTED, RF_ERR_WORKSPACE = -1, -2, -3, -5, -6
ADDR = 1 << 20                   # a 16-byte-aligned address: a refused call never touches it


def call(op, H=8, W=8, Cc=512, groups=32, norm="ok", conv=None, attn="ok", inp=ADDR, out=ADDR, residual=None, ws_bytes=1 << 40, ws_base=ADDR,
         desc=True):
    """One call with valid arguments except for what the keywords change"""
    lib = L.load()
    d = L.rf_vae_op_desc()
    d.op, d.H, d.W, d.C, d.groups = op, H, W, Cc, groups
    n = L.rf_vae_norm()
    n.gamma = n.beta = ADDR
    if norm == "nogamma":
        n.gamma = None
    cv = L.rf_vae_conv()
    cv.w = cv.b = ADDR
    cv.cin, cv.cout = conv or (64, 64)
    a = L.rf_vae_attn()
    a.norm.gamma = a.norm.beta = a.w_qk = a.b_qk = a.w_v = a.w_out = a.b_out = ADDR
    a.C = Cc
    if attn == "noweights":
        a.w_v = None
    if norm is not None:
        d.norm = C.pointer(n)
    d.conv = C.pointer(cv)
    if attn is not None:
        d.attn = C.pointer(a)
    d.input, d.out, d.residual = inp, out, residual
    ws = L.rf_workspace()
    ws.base, ws.bytes = ws_base, ws_bytes
    if ws_base is not None:
        d.ws = C.pointer(ws)
    rc = lib.rf_debug_vae_op(C.byref(d) if desc else None, None)
    return rc, lib.rf_last_error().decode(errors="replace")


GN, CONV, UP, DOWN, CORE, BLOCK = range(6)


@pytest.mark.parametrize("kw,code,word", [
    (dict(op=CORE, H=6, W=8, residual=ADDR), RF_ERR_SHAPE, "attention over 48 tokens"),            # tokens not a multiple of 64
    (dict(op=BLOCK, H=6, W=8), RF_ERR_SHAPE, "attention over 48 tokens"),
    (dict(op=CORE, Cc=256, residual=ADDR), RF_ERR_UNSUPPORTED, "built for 512 channels (got 256)"),
    (dict(op=BLOCK, Cc=256), RF_ERR_UNSUPPORTED, "built for 512 channels (got 256)"),
    (dict(op=BLOCK, attn="noweights"), RF_ERR_NULL, "attention weights NULL"),
    (dict(op=BLOCK, attn=None), RF_ERR_NULL, "ATTN_BLOCK without attn"),
    (dict(op=BLOCK, groups=16), RF_ERR_SHAPE, "GroupNorm over C=512 channels, 16 groups"),       # the block's own GroupNorm: 32 per group
    (dict(op=CORE), RF_ERR_NULL, "without vt"),
    (dict(op=GN, Cc=96), RF_ERR_SHAPE, "GroupNorm over C=96 channels, 32 groups"),
    (dict(op=GN, Cc=64, groups=64), RF_ERR_SHAPE, "GroupNorm over C=64 channels, 64 groups"),    # 1 channel per group
    (dict(op=GN, Cc=512, groups=16), RF_ERR_SHAPE, "GroupNorm over C=512 channels, 16 groups"),  # 32 channels per group
    (dict(op=GN, Cc=0), RF_ERR_SHAPE, "GroupNorm over C=0"),
    (dict(op=GN, Cc=64, groups=0), RF_ERR_SHAPE, "0 groups"),
    (dict(op=GN, Cc=64, norm="nogamma"), RF_ERR_NULL, "GroupNorm weights NULL"),
    (dict(op=GN, Cc=64, norm=None), RF_ERR_NULL, "GROUP_NORM without norm"),
    (dict(op=CONV, conv=(96, 64)), RF_ERR_SHAPE, "conv3x3 96 -> 64"),                              # cin % 64
    (dict(op=CONV, conv=(64, 12)), RF_ERR_SHAPE, "conv3x3 64 -> 12"),                              # cout % 8
    (dict(op=DOWN, conv=(96, 96)), RF_ERR_SHAPE, "downsample of 8x8x96"),
    (dict(op=DOWN, H=7), RF_ERR_SHAPE, "downsample of 7x8x64"),                                    # odd side
    (dict(op=UP, Cc=60), RF_ERR_SHAPE, "UPSAMPLE2X over C=60"),
    (dict(op=9), RF_ERR_UNSUPPORTED, "op=9"),
    (dict(op=GN, Cc=64, H=0), RF_ERR_SHAPE, "H=0"),
    (dict(op=GN, Cc=64, out=None), RF_ERR_NULL, "NULL tensor"),
    (dict(op=CONV, inp=None), RF_ERR_NULL, "NULL tensor"),
    (dict(op=GN, Cc=64, inp=ADDR + 2), RF_ERR_ALIGN, "16-byte"),
    (dict(op=UP, Cc=64, out=ADDR + 8), RF_ERR_ALIGN, "16-byte"),
    (dict(op=CONV, residual=ADDR + 4), RF_ERR_ALIGN, "16-byte"),
    (dict(op=GN, Cc=64, ws_base=ADDR + 4), RF_ERR_WORKSPACE, "workspace"),
    (dict(op=GN, Cc=64, ws_bytes=4096), RF_ERR_WORKSPACE, "workspace 4096 <"),
    (dict(op=GN, desc=False), RF_ERR_NULL, "descriptor NULL"),
])
def test_refusals(kw, code, word):
    rc, msg = call(**kw)
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_workspace_query():
    """ws == NULL: the bytes the op needs; an op with buffers of its own needs more than one without"""
    base, _ = call(op=GN, Cc=64, ws_base=None)
    down, _ = call(op=DOWN, H=16, W=10, conv=(128, 128), ws_base=None)
    block, _ = call(op=BLOCK, H=8, W=16, ws_base=None)
    assert base > (64 << 20) and down >= base + 8 * 7 * 9 * 128 * 2 and block >= base + 128 * 512 * 2 * 6
    assert call(op=GN, Cc=96, ws_base=None)[0] == RF_ERR_SHAPE           # a refusal stays a refusal


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", K.ATTN_FORMS)
@pytest.mark.parametrize("S", K.ATTN_S + (576,))
def test_attention_yardstick(form, S):
    q, k, v = K.attn_inputs(form, S)
    r = assert_close(K.attn_yardstick(q, k, v), K.attn_ref64(q, k, v), f"attention yardstick {form} S={S}")
    print(f"  attention yardstick {form} S={S}: rel-L2 {r:.2e}")
    n = K.attn_rescale_counts(q, k)
    if form == "rising":
        assert int(n.min()) == S // 32 - 1, "the running max must rise on every tile, for every query"
    if form == "falling":
        assert int(n.max()) == 0, "the running max must never rise after the first tile"


@pytest.mark.parametrize("S", K.ATTN_S)
def test_routing_is_exact_in_fp32(S):
    q, k, v, pi = K.routing_inputs(S)
    assert torch.equal(K.attn_yardstick(q, k, v), v[pi])
    assert float(v.float().abs().min()) >= 2.0 ** -6


def gn_shapes():
    return [(H, W, Cc) for Cc in K.GN_C for (H, W) in K.GN_HW] + [K.GN_CAPPED]


def bound_fraction(got, ref):
    got, ref = got.double(), ref.double()
    atol = 1.2e-2 * float(ref.abs().mean()) + 1e-6
    return float(((got - ref).abs() / (atol + 1.2e-2 * ref.abs())).max())


@pytest.mark.parametrize("form", K.GN_FORMS)
@pytest.mark.parametrize("H,W,Cc", gn_shapes())
def test_group_norm_yardstick(form, H, W, Cc):
    x, gamma, beta = K.gn_inputs(form, H, W, Cc)
    for silu in (False, True):
        assert_close(K.gn_yardstick(x, gamma, beta, silu), K.gn_ref64(x, gamma, beta, silu), f"GroupNorm yardstick {form} {H}x{W}x{Cc} silu={silu}")


def test_group_norm_outlier_exponent_is_the_largest():
    """the first-pixel outlier is 2^k for the largest k at which the yardstick stays under HALF the bound on every shape"""
    def worst(k):
        w = 0.0
        for (H, W, Cc) in gn_shapes():
            x, gamma, beta = K.gn_inputs("outlier", H, W, Cc, outlier_log2=k)
            for silu in (False, True):
                w = max(w, bound_fraction(K.gn_yardstick(x, gamma, beta, silu), K.gn_ref64(x, gamma, beta, silu)))
        return w
    lo, hi = worst(K.GN_OUTLIER_LOG2), worst(K.GN_OUTLIER_LOG2 + 1)
    print(f"  outlier 2^{K.GN_OUTLIER_LOG2}: {lo:.2f} of the bound; 2^{K.GN_OUTLIER_LOG2 + 1}: {hi:.2f}")
    assert lo < 0.5 <= hi, (lo, hi)


@pytest.mark.parametrize("H,W", K.BLOCK_HW)
def test_attention_block_yardstick(H, W):
    m, x = K.block_module(), K.block_input(H, W)
    ref = K.block_ref64(m, x)
    got = K.block_yardstick(m.float(), x)
    assert_close(got, ref, f"attention block yardstick {H}x{W}")
    assert bound_fraction(got, ref) < 0.5
