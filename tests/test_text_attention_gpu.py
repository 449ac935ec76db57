"""GPU: attn64_kernel / attn80_kernel (csrc/text.hip) one launch at a time, through rf_debug_text_attention -- the launch code the T5,
CLIP text and CLIP vision towers use, on caller buffers.

Reference: fp64 on the CPU from the same bf16 operands, softmax(scale * q.k^T + bias) @ v over the S real keys.
Bound: assert_close of tests/test_kernels_gpu.py as it stands (elementwise 1.2e-2 |ref| + 1.2e-2 mean|ref|, rel-L2 < 4e-3).
Yardstick: `yardstick()` below, an fp32 restatement that rounds where the kernel rounds (P to bf16 before PV, the row sum from the
unrounded P, one rounding of the output).  It is held to the same bound and its rel-L2 is printed next to the kernel's: pure rounding
reaches about half the bound, a routing or channel error is orders of magnitude above it.

Every case: heads = 3 (odd head offsets), B = 2, row pitches 64 elements wider than heads * head_dim, ldvt = B * S_pad + 64, 8 extra
rows of V^T.  Gap columns / rows of q, k, vt are NaN (a load outside a head's columns poisons the result), `out` is prefilled with 7.0,
and the pad rows of q / k and pad key columns of V^T (>= S) hold +-1e4: finite, as the towers guarantee by memset (0 x NaN is NaN inside
the MFMA), but large enough that a masked key which contributes anything at all is seen.
"""
import functools
import math
import zlib

import pytest
import torch

from tests.test_kernels_gpu import assert_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HEADS, NB, GAP, FILL, PAD = 3, 2, 64, 7.0, 1.0e4
NINF = float("-inf")

# (head_dim, S, S_pad): m = S_pad / 32 even takes the padded V^T pitch of attn80_kernel; 480 / 512 keys are the LDS limits
SHAPES80 = [(80, 1, 32), (80, 32, 32), (80, 33, 64), (80, 96, 96), (80, 100, 128), (80, 257, 288), (80, 449, 480), (80, 480, 480)]
SHAPES64 = [(64, 7, 32), (64, 77, 96), (64, 257, 288), (64, 500, 512), (64, 512, 512)]
SHAPES = SHAPES80 + SHAPES64
FORMS = ("folded", "scaled", "peaked")


def parity_variants(S, S_pad):
    """(input form, bias form) of test (a).  The causal mask goes with the peaked form at every shape, and with the folded form (CLIP
    text's own) up to 128 keys.  Why not everywhere: under a causal mask the first rows are sums of a few O(1) terms whose P is rounded
    to bf16, an error of up to 2^-9 sum_j p_j |v_j| ~ 2e-3 that no kernel of this design avoids, while the elementwise floor of the
    bound, 1.2e-2 mean|ref|, falls with S because the late rows average many keys (mean|ref| = 0.15 at 449+ keys: floor 1.8e-3).  At
    S >= 257 the yardstick -- pure rounding -- itself reaches 0.95 .. 1.08 of the bound in its worst element of ~2e5; with peaked
    scores mean|ref| stays near 0.6 at every S and the yardstick stays below 0.5 of it, as it does for folded + causal up to 128 keys
    (<= 0.63)."""
    for form in FORMS:
        for kind in ("shared", "per_head") + (("none",) if S == S_pad else ()):
            yield form, kind
    yield "peaked", "causal"
    if S_pad <= 128:
        yield "folded", "causal"


def shape_id(s):
    return f"hd{s[0]}-S{s[1]}of{s[2]}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- operands (CPU, built once per case and never modified) ------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _pad_values(shape, g):
    return (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * PAD


def make_operands(hd, S, S_pad, q_std, seed, chan=None, heads=HEADS, nb=NB):
    """q, k [nb * S_pad (+ 1 guard row for out)][inner + GAP], vt [inner + 8][nb * S_pad + GAP] as bf16 with NaN gaps and +-1e4 padding.
    chan = (lo, hi): q and k are zero outside those channels of every head."""
    g = _gen("ops", hd, S, S_pad, seed)
    inner, R = heads * hd, nb * S_pad
    real = (torch.arange(R) % S_pad) < S
    def rows(std):
        x = torch.where(real[:, None], torch.randn(R, inner, generator=g) * std, _pad_values((R, inner), g))
        if chan is not None:
            c = torch.arange(inner) % hd
            x = x * ((c >= chan[0]) & (c < chan[1])).float()
        full = torch.full((R, inner + GAP), float("nan"))
        full[:, :inner] = x
        return full.to(BF)
    q, k = rows(q_std), rows(1.0)
    v = torch.where(real[None, :], torch.randn(inner, R, generator=g), _pad_values((inner, R), g))
    vt = torch.full((inner + 8, R + GAP), float("nan"))
    vt[:inner, :R] = v
    return q, k, vt.to(BF)


def make_bias(kind, S, S_pad, seed, heads=HEADS):
    """[heads or 1][S_pad][S_pad] fp32: N(0, 1), -inf in the key columns >= S (+ the causal mask); None for kind 'none'"""
    if kind == "none":
        assert S == S_pad
        return None
    g = _gen("bias", kind, S, S_pad, seed)
    b = torch.randn(heads if kind == "per_head" else 1, S_pad, S_pad, generator=g)
    b[:, :, S:] = NINF
    if kind == "causal":
        b = b.masked_fill(torch.ones(S_pad, S_pad, dtype=torch.bool).triu(1), NINF)
    return b.contiguous()


def _per_head(q, k, vt, bias, hd, S, S_pad, heads, nb):
    """(z, h, q [S][hd], k [S][hd], v [S][hd], bias [S][S] or None) of every sequence and head, real rows / keys only"""
    for z in range(nb):
        r0 = z * S_pad
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            b = None if bias is None else bias[h if bias.shape[0] > 1 else 0, :S, :S]
            yield z, h, q[r0:r0 + S, c], k[r0:r0 + S, c], vt[c, r0:r0 + S].t(), b


def reference(q, k, vt, bias, hd, S, S_pad, scale, heads=HEADS, nb=NB):
    """fp64: [nb][S][heads * hd]"""
    out = torch.zeros(nb, S, heads * hd, dtype=torch.float64)
    for z, h, qh, kh, vh, b in _per_head(q, k, vt, bias, hd, S, S_pad, heads, nb):
        s = scale * (qh.double() @ kh.double().t())
        if b is not None:
            s = s + b.double()
        out[z, :, h * hd:(h + 1) * hd] = torch.softmax(s, dim=-1) @ vh.double()
    return out


def yardstick(q, k, vt, bias, hd, S, S_pad, scale, heads=HEADS, nb=NB):
    """The kernel's arithmetic in fp32 with its roundings: scores and softmax in fp32, P rounded to bf16 for the PV product, the row sum
    taken from the unrounded P, one division and one rounding to bf16 at the end."""
    out = torch.zeros(nb, S, heads * hd, dtype=BF)
    for z, h, qh, kh, vh, b in _per_head(q, k, vt, bias, hd, S, S_pad, heads, nb):
        s = (qh.float() @ kh.float().t()) * scale
        if b is not None:
            s = s + b
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o = (p.to(BF).float() @ vh.float()) / p.sum(dim=-1, keepdim=True)
        out[z, :, h * hd:(h + 1) * hd] = o.to(BF)
    return out


def figures(got, ref):
    """for the printed record only (assert_close judges): rel-L2 and the worst element's error as a fraction of assert_close's
    elementwise allowance 1.2e-2 |ref| + 1.2e-2 mean|ref|"""
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    return f"rel-L2 {float(err.norm() / ref.norm()):.3e} worst/allowed {float((err / (1.2e-2 * ref.abs() + 1.2e-2 * ref.abs().mean() + 1e-6)).max()):.2f}"


@functools.lru_cache(maxsize=None)
def parity_case(hd, S, S_pad, form, kind):
    """operands, bias, scale, fp64 reference and the yardstick's rel-L2 of one case of test (a); shared by qi = 1 and qi = 4"""
    q_std = {"folded": hd ** -0.5, "scaled": 1.0, "peaked": 6.0 * hd ** -0.5}[form]
    scale = hd ** -0.5 if form == "scaled" else 1.0
    q, k, vt = make_operands(hd, S, S_pad, q_std, FORMS.index(form))
    bias = make_bias(kind, S, S_pad, FORMS.index(form))
    ref = reference(q, k, vt, bias, hd, S, S_pad, scale)
    what = f"{shape_id((hd, S, S_pad))} {form} {kind}"
    yard = yardstick(q, k, vt, bias, hd, S, S_pad, scale)
    assert_close(yard, ref, f"yardstick {what}")
    return q, k, vt, bias, scale, ref, figures(yard, ref)


@functools.lru_cache(maxsize=None)
def channel_case(hd, S, S_pad, lo, hi):
    q, k, vt = make_operands(hd, S, S_pad, 2.0 * (hi - lo) ** -0.5, 10 + lo, chan=(lo, hi))   # scores ~ N(0, 4): far from uniform
    bias = make_bias("shared", S, S_pad, 10 + lo)
    ref = reference(q, k, vt, bias, hd, S, S_pad, 1.0)
    yard = yardstick(q, k, vt, bias, hd, S, S_pad, 1.0)
    assert_close(yard, ref, f"yardstick {shape_id((hd, S, S_pad))} channels [{lo},{hi})")
    return q, k, vt, bias, ref, figures(yard, ref)


# ---- one launch ------------------------------------------------------------------------------------------------------------------------
def launch(dev, hd, qi, q, k, vt, bias, S, S_pad, scale, heads=HEADS, nb=NB, bias_hs=None):
    """q, k, vt, bias: device tensors.  Returns out [nb * S_pad + 1][q.shape[1]] (prefilled with 7.0; the last row is a guard row)."""
    from reflectionflow_amd import _lib
    from reflectionflow_amd.ops import stream_ptr
    out = torch.full((nb * S_pad + 1, q.shape[1]), FILL, dtype=BF, device=dev)
    if bias_hs is None:
        bias_hs = S_pad * S_pad if bias is not None and bias.shape[0] > 1 else 0
    rc = _lib.load().rf_debug_text_attention(hd, qi, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), vt.stride(0),
                                             None if bias is None else bias.data_ptr(), bias_hs, out.data_ptr(), out.stride(0), heads, nb, S, S_pad,
                                             scale, stream_ptr())
    _lib.check(rc, "rf_debug_text_attention")
    return out


def to_dev(dev, *xs):
    return [None if x is None else x.to(dev) for x in xs]


def real_rows(out, hd, S, S_pad, heads=HEADS, nb=NB):
    """[nb][S][heads * hd] of a launch's `out`, on the CPU"""
    return out[:nb * S_pad].view(nb, S_pad, -1)[:, :S, :heads * hd].cpu()


def assert_untouched(out, hd, S, S_pad, what, heads=HEADS, nb=NB):
    """(d): pad rows, the gap columns and the guard row still hold 7.0 bit for bit"""
    fill = torch.tensor(FILL, dtype=BF).view(torch.int16)
    bits = out.cpu().view(torch.int16)
    assert bool((bits[nb * S_pad] == fill).all()), f"{what}: the guard row behind the last sequence was written"
    assert bool((bits[:, heads * hd:] == fill).all()), f"{what}: columns >= heads * head_dim of out were written"
    body = bits[:nb * S_pad].view(nb, S_pad, -1)
    assert bool((body[:, S:] == fill).all()), f"{what}: rows >= S of out were written"
    assert bool(torch.isfinite(real_rows(out, hd, S, S_pad, heads, nb).float()).all()), f"{what}: non-finite output in a real row"


# ---- (a) parity vs fp64, (d) writes stay in bounds ------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_vs_fp64_and_writes_stay_in_bounds(dev, shape, qi):
    hd, S, S_pad = shape
    for form, kind in parity_variants(S, S_pad):
        q, k, vt, bias, scale, ref, y = parity_case(hd, S, S_pad, form, kind)
        what = f"{shape_id(shape)} qi={qi} {form} {kind}"
        out = launch(dev, hd, qi, *to_dev(dev, q, k, vt, bias), S, S_pad, scale)
        torch.cuda.synchronize()
        assert_untouched(out, hd, S, S_pad, what)
        got = real_rows(out, hd, S, S_pad)
        print(f"  PARITY {shape_id(shape)} qi={qi} {form:6s} {kind:8s} kernel {figures(got, ref)} | yardstick {y}")
        assert_close(got, ref, what)


# ---- (b) exact key routing -------------------------------------------------------------------------------------------------------------------
def routing_perms(S, heads=HEADS):
    """pi_h(i) = (a_h i + c_h) mod S with a_h coprime to S, different per head"""
    a, perms = 4, []
    for h in range(heads):
        a += 1
        while math.gcd(a, S) != 1:
            a += 1
        perms.append((a * torch.arange(S) + 7 * h + 3) % S)
    return perms


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_exact_key_routing(dev, shape, qi):
    """One key per query row has bias 0, every other -inf: p = 1 there and 0 elsewhere, l = 1, every other term of the PV sum is
    0 x finite, so out[z][i][h] must be v[z][pi_h(i)][h] bit for bit: key-slot permutation of the PV operand, V^T chunk swizzle, bias
    indexing and the head / sequence / row offsets of `out`, with no tolerance."""
    hd, S, S_pad = shape
    q, k, vt = make_operands(hd, S, S_pad, hd ** -0.5, 20)
    perms = routing_perms(S)
    bias = torch.full((HEADS, S_pad, S_pad), NINF)
    for h, pi in enumerate(perms):
        bias[h, torch.arange(S), pi] = 0.0
    out = launch(dev, hd, qi, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    assert_untouched(out, hd, S, S_pad, f"routing {shape_id(shape)} qi={qi}")
    got = real_rows(out, hd, S, S_pad).view(NB, S, HEADS, hd)
    want = torch.empty_like(got)
    for z in range(NB):
        for h, pi in enumerate(perms):
            want[z, :, h] = vt[h * hd:(h + 1) * hd, z * S_pad + pi].t()
    bad = got.view(torch.int16) != want.view(torch.int16)
    if bad.any():
        idx = torch.nonzero(bad)
        first = [(z, i, h, c, int(perms[h][i]), float(got[z, i, h, c]), float(want[z, i, h, c])) for z, i, h, c in idx[:8].tolist()]
        raise AssertionError(f"routing {shape_id(shape)} qi={qi}: {int(bad.sum())}/{bad.numel()} elements differ; heads {sorted(set(idx[:, 2].tolist()))}, "
                             f"channels {sorted(set(idx[:, 3].tolist()))[:16]}, {len(set(idx[:, 1].tolist()))} rows; "
                             f"first (seq, row, head, channel, key, got, want): {first}")


# ---- (c) channel ranges of QK^T ------------------------------------------------------------------------------------------------------------
CHANNEL_CASES = [(s, 64, 80) for s in SHAPES80] + [(s, lo, lo + 32) for s in SHAPES for lo in (0, 32)]


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("shape,lo,hi", CHANNEL_CASES, ids=lambda x: shape_id(x) if isinstance(x, tuple) else str(x))
def test_qk_channel_ranges(dev, shape, lo, hi, qi):
    """q and k are nonzero in channels [lo, hi) of every head only: [64, 80) is the half-empty third MFMA of attn80_kernel on its own,
    [0, 32) and [32, 64) the two whole k-steps.  A k-step that is dropped or mispaired leaves uniform or unrelated scores."""
    hd, S, S_pad = shape
    q, k, vt, bias, ref, y = channel_case(hd, S, S_pad, lo, hi)
    out = launch(dev, hd, qi, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    what = f"{shape_id(shape)} qi={qi} channels [{lo},{hi})"
    assert_untouched(out, hd, S, S_pad, what)
    got = real_rows(out, hd, S, S_pad)
    print(f"  CHANNELS {shape_id(shape)} qi={qi} [{lo},{hi}) kernel {figures(got, ref)} | yardstick {y}")
    assert_close(got, ref, what)


# ---- (e) form and batch invariance, bit for bit ----------------------------------------------------------------------------------------
def wide_rule(heads, nb, S_pad):
    """text.hip, text_attention_launch: 256 queries per workgroup once (head, sequence) pairs x query blocks fill the CUs"""
    return 4 if heads * nb * ((S_pad + 255) // 256) >= 256 else 1


@torch.no_grad()
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_form_and_batch_invariance(dev, shape):
    hd, S, S_pad = shape
    q, k, vt, bias, scale, _, _ = parity_case(hd, S, S_pad, "folded", "per_head")
    qd, kd, vd, bd = to_dev(dev, q, k, vt, bias)
    one = launch(dev, hd, 1, qd, kd, vd, bd, S, S_pad, scale)
    four = launch(dev, hd, 4, qd, kd, vd, bd, S, S_pad, scale)
    again = launch(dev, hd, 1, qd, kd, vd, bd, S, S_pad, scale)
    auto = launch(dev, hd, 0, qd, kd, vd, bd, S, S_pad, scale)
    alone = []
    for z in range(NB):   # the same buffers, one sequence at a time: same pitches, pointers moved to sequence z
        o = launch(dev, hd, 1, qd[z * S_pad:], kd[z * S_pad:], vd[:, z * S_pad:], bd, S, S_pad, scale, nb=1)
        alone.append(o[:S_pad])
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int16)
    assert torch.equal(bits(four), bits(one)), "qi = 4 differs from qi = 1"
    assert torch.equal(bits(again), bits(one)), "a repeated launch differs"
    assert wide_rule(HEADS, NB, S_pad) == 1
    assert torch.equal(bits(auto), bits(one)), "qi = 0 differs from the instantiation the rule names"
    assert torch.equal(bits(torch.cat(alone)), bits(one[:NB * S_pad])), "two B = 1 launches differ from the B = 2 launch"


@torch.no_grad()
@pytest.mark.parametrize("hd,heads,nb", [(80, 32, 8), (64, 64, 4)])
def test_auto_form_is_the_wide_one_when_the_rule_says_so(dev, hd, heads, nb):
    """heads * B * ceil(S_pad / 256) >= 256: qi = 0 must be the 256-query form, and equal the 64-query form like everywhere else"""
    S, S_pad = 20, 32
    assert wide_rule(heads, nb, S_pad) == 4
    q, k, vt = make_operands(hd, S, S_pad, hd ** -0.5, 30, heads=heads, nb=nb)
    bias = make_bias("shared", S, S_pad, 30)
    ref = reference(q, k, vt, bias, hd, S, S_pad, 1.0, heads=heads, nb=nb)
    qd, kd, vd, bd = to_dev(dev, q, k, vt, bias)
    outs = [launch(dev, hd, qi, qd, kd, vd, bd, S, S_pad, 1.0, heads=heads, nb=nb) for qi in (0, 4, 1)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "qi = 0 differs from qi = 4"
    assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16)), "qi = 4 differs from qi = 1"
    assert_untouched(outs[0], hd, S, S_pad, f"hd{hd} heads={heads} B={nb}", heads=heads, nb=nb)
    assert_close(real_rows(outs[0], hd, S, S_pad, heads=heads, nb=nb), ref, f"hd{hd} heads={heads} B={nb} qi=0")
