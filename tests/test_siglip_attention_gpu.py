"""GPU: attn80_stream_kernel (csrc/text.hip), the head-dim-80 attention that streams K / V^T through the LDS in chunks of 96 keys with an
online softmax, one launch at a time through rf_text_attention80.  stream_keys = 1 runs it at shapes where the resident attn80_kernel also
runs; beyond 480 keys (SigLIP so400m/14 at 384 px: 729 tokens, S_pad 736) it is what stream_keys = 0 launches.

Reference, operands, bound and helpers: tests/test_text_attention_gpu.py (fp64 from the same bf16 operands; assert_close: elementwise
1.2e-2 |ref| + 1.2e-2 mean|ref|, rel-L2 < 4e-3; NaN gaps, +-1e4 padding, `out` prefilled with 7.0).  Every case: heads = 2, B = 2.
Yardstick: `yardstick_online()` below, tests/test_text_attention_stream_gpu.py's with the chunk and head dim as arguments: the kernel's
arithmetic in fp32 torch with its roundings in the ONLINE form, held to the same bound in every case before the kernel is
(profiles/siglip.md has its table).  The causal mask goes with peaked scores at every shape and with folded scores up to 128 keys only
(parity_variants' docstring in tests/test_text_attention_gpu.py says why).

Shapes (S, S_pad) against the 96-key chunk, stream_keys = 1: (1, 32) = one partial chunk; (90, 96) = exactly one chunk; (100, 128) = one
whole + 32; (200, 224) = two whole + a partial tail of 32; (449, 480) = five whole, the resident kernel's limit.  Natural route,
stream_keys = 0: (481, 512) = five whole + 32; (577, 608) = six whole + 32; (729, 736) = seven whole + 64.
"""
import functools

import pytest
import torch

from tests.test_text_attention_gpu import (BF, FILL, FORMS, NINF, assert_close, assert_untouched, figures, launch, make_bias, make_operands,
                                           real_rows, reference, to_dev, wide_rule, _per_head)

pytestmark = pytest.mark.gpu
HEADS, NB, HD, CK = 2, 2, 80, 96
LOG2E = 1.4426950408889634
FORCED = [(1, 32), (90, 96), (100, 128), (200, 224), (449, 480)]
NATURAL = [(481, 512), (577, 608), (729, 736)]
CASES = [(s, 1) for s in FORCED] + [(s, 0) for s in NATURAL]          # (shape, stream_keys)


def sid(x):
    return f"S{x[0]}of{x[1]}" if isinstance(x, tuple) else str(x)


def case_id(c):
    return f"{sid(c[0])}-{'forced' if c[1] else 'natural'}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def variants(S, S_pad):
    for form in FORMS:
        for kind in ("shared", "per_head") + (("none",) if S == S_pad else ()):
            yield form, kind
    yield "peaked", "causal"
    if S_pad <= 128:
        yield "folded", "causal"


def yardstick_online(q, k, vt, bias, S, S_pad, scale, hd=HD, ck=CK):
    """a streaming kernel's arithmetic in fp32 with its roundings (module docstring); chunks of ck keys from key 0, real keys only (a
    padded key's -inf bias gives P = 0 and leaves every sum as it is)"""
    out = torch.zeros(NB, S, HEADS * hd, dtype=BF)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    for z, h, qh, kh, vh, b in _per_head(q, k, vt, bias, hd, S, S_pad, HEADS, NB):
        s = (qh.float() @ kh.float().t()) * sl2
        if b is not None:
            s = s + b * torch.tensor(LOG2E, dtype=torch.float32)
        m = torch.full((S, 1), NINF)
        l = torch.zeros(S, 1)
        o = torch.zeros(S, hd)
        for c0 in range(0, S, ck):
            sc = s[:, c0:c0 + ck]
            mnew = torch.maximum(m, sc.max(dim=-1, keepdim=True).values)
            msub = torch.where(mnew > NINF, mnew, torch.zeros_like(mnew))
            alpha = torch.exp2(m - msub)
            p = torch.exp2(sc - msub)
            o = o * alpha + p.to(BF).float() @ vh[c0:c0 + ck].float()
            l = l * alpha + p.sum(dim=-1, keepdim=True)
            m = mnew
        out[z, :, h * hd:(h + 1) * hd] = (o / l).to(BF)
    return out


@functools.lru_cache(maxsize=None)
def case(S, S_pad, form, kind):
    """operands, bias, scale, fp64 reference and the online yardstick's figures; built once, shared by every test and never modified"""
    q_std = {"folded": HD ** -0.5, "scaled": 1.0, "peaked": 6.0 * HD ** -0.5}[form]
    scale = HD ** -0.5 if form == "scaled" else 1.0
    q, k, vt = make_operands(HD, S, S_pad, q_std, FORMS.index(form), heads=HEADS, nb=NB)
    bias = make_bias(kind, S, S_pad, FORMS.index(form), heads=HEADS)
    ref = reference(q, k, vt, bias, HD, S, S_pad, scale, heads=HEADS, nb=NB)
    yard = yardstick_online(q, k, vt, bias, S, S_pad, scale)
    assert_close(yard, ref, f"online yardstick {sid((S, S_pad))} {form} {kind}")
    return q, k, vt, bias, scale, ref, figures(yard, ref)


def launch_s(dev, qi, stream_keys, q, k, vt, bias, S, S_pad, scale, nb=NB, bias_hs=None):
    """rf_text_attention80 on device tensors; out [nb * S_pad + 1][q.shape[1]] prefilled with 7.0 (the last row is a guard row)"""
    from reflectionflow_amd import _lib
    from reflectionflow_amd.ops import stream_ptr
    out = torch.full((nb * S_pad + 1, q.shape[1]), FILL, dtype=BF, device=dev)
    if bias_hs is None:
        bias_hs = S_pad * S_pad if bias is not None and bias.shape[0] > 1 else 0
    rc = _lib.load().rf_text_attention80(qi, stream_keys, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), vt.stride(0),
                                         None if bias is None else bias.data_ptr(), bias_hs, out.data_ptr(), out.stride(0), HEADS, nb, S, S_pad, scale,
                                         stream_ptr())
    _lib.check(rc, "rf_text_attention80")
    return out


def rows(out, S, S_pad):
    return real_rows(out, HD, S, S_pad, heads=HEADS, nb=NB)


def untouched(out, S, S_pad, what):
    assert_untouched(out, HD, S, S_pad, what, heads=HEADS, nb=NB)


def bits(x):
    return x.view(torch.int16)


# ---- parity vs fp64 in every bias form; stray writes ------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_parity_vs_fp64_and_writes_stay_in_bounds(dev, c, qi):
    (S, S_pad), sk = c
    for form, kind in variants(S, S_pad):
        q, k, vt, bias, scale, ref, y = case(S, S_pad, form, kind)
        what = f"{case_id(c)} qi={qi} {form} {kind}"
        out = launch_s(dev, qi, sk, *to_dev(dev, q, k, vt, bias), S, S_pad, scale)
        torch.cuda.synchronize()
        untouched(out, S, S_pad, what)
        got = rows(out, S, S_pad)
        print(f"  STREAM80 {case_id(c)} qi={qi} {form:6s} {kind:8s} kernel {figures(got, ref)} | yardstick {y}")
        assert_close(got, ref, what)


# ---- masks that empty whole chunks ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(which):
    """S = 288 of S_pad = 320: the partial last chunk [288, 320) holds padded keys only (a chunk of -inf at the end) in every variant.
    'middle': keys [96, 192) are -inf for every row as well.  'first': rows i % 3 == 0 see -inf in all of [0, 96), i.e. their state is
    still empty when the second chunk arrives; rows i % 3 == 1 see -inf everywhere but in the LAST real chunk."""
    S, S_pad = 288, 320
    q, k, vt = make_operands(HD, S, S_pad, HD ** -0.5, 40, heads=HEADS, nb=NB)
    bias = make_bias("per_head", S, S_pad, 40, heads=HEADS).clone()
    i = torch.arange(S_pad)
    if which == "middle":
        bias[:, :, 96:192] = NINF
    else:
        bias[:, i % 3 == 0, 0:96] = NINF
        bias[:, i % 3 == 1, 0:192] = NINF
    bias = bias.contiguous()
    ref = reference(q, k, vt, bias, HD, S, S_pad, 1.0, heads=HEADS, nb=NB)
    yard = yardstick_online(q, k, vt, bias, S, S_pad, 1.0)
    assert_close(yard, ref, f"online yardstick mask {which}")
    return S, S_pad, q, k, vt, bias, ref, figures(yard, ref)


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("which", ["middle", "first"])
def test_chunks_of_minus_infinity(dev, which, qi):
    S, S_pad, q, k, vt, bias, ref, y = mask_case(which)
    out = launch_s(dev, qi, 1, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    what = f"mask {which} qi={qi}"
    untouched(out, S, S_pad, what)          # includes: every real row is finite
    got = rows(out, S, S_pad)
    print(f"  STREAM80 mask {which:6s} qi={qi} kernel {figures(got, ref)} | yardstick {y}")
    assert_close(got, ref, what)


# ---- exact key routing, one chunk position at a time ------------------------------------------------------------------------------------------
ROUTES = [((200, 224), 1, (0, 96)), ((200, 224), 1, (96, 192)), ((200, 224), 1, (192, 200)),
          ((729, 736), 0, (0, 96)), ((729, 736), 0, (384, 480)), ((729, 736), 0, (672, 729))]


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("shape,sk,keys", ROUTES, ids=[f"{sid(r[0])}-keys{r[2][0]}to{r[2][1]}" for r in ROUTES])
def test_exact_key_routing_per_chunk_position(dev, shape, sk, keys, qi):
    """One key per query row has bias 0, every other -inf, and all selected keys lie in ONE chunk (first, a middle one, the partial
    last): p = 1 there and 0 elsewhere, every other chunk leaves the state as it is, l = 1: out[z][i][h] is v[z][key_h(i)][h] bit for
    bit -- chunk addressing of K / V^T / bias, the slot permutation and chunk swizzle inside the buffer, the rescale by exactly 0 or 1."""
    S, S_pad = shape
    lo, hi = keys
    q, k, vt = make_operands(HD, S, S_pad, HD ** -0.5, 50, heads=HEADS, nb=NB)
    sel = [lo + (5 * torch.arange(S) + 7 * h + 3) % (hi - lo) for h in range(HEADS)]
    bias = torch.full((HEADS, S_pad, S_pad), NINF)
    for h, key in enumerate(sel):
        bias[h, torch.arange(S), key] = 0.0
    out = launch_s(dev, qi, sk, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    untouched(out, S, S_pad, f"routing {sid(shape)} keys {keys} qi={qi}")
    got = rows(out, S, S_pad).view(NB, S, HEADS, HD)
    want = torch.empty_like(got)
    for z in range(NB):
        for h, key in enumerate(sel):
            want[z, :, h] = vt[h * HD:(h + 1) * HD, z * S_pad + key].t()
    bad = bits(got) != bits(want)
    assert not bad.any(), (f"routing {sid(shape)} keys {keys} qi={qi}: {int(bad.sum())}/{bad.numel()} elements differ; first (seq, row, head, channel): "
                           f"{torch.nonzero(bad)[:8].tolist()}")


# ---- channel ranges ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def channel_case(S, S_pad, lo, hi, zero_v_from=None):
    """q and k nonzero in channels [lo, hi) of every head only; zero_v_from: v is zero in channels >= that of every head as well"""
    q, k, vt = make_operands(HD, S, S_pad, 2.0 * (hi - lo) ** -0.5, 10 + lo, chan=(lo, hi), heads=HEADS, nb=NB)   # scores ~ N(0, 4)
    if zero_v_from is not None:
        vt = vt.clone()
        for h in range(HEADS):
            vt[h * HD + zero_v_from:(h + 1) * HD, :NB * S_pad] = 0.0
    bias = make_bias("shared", S, S_pad, 10 + lo, heads=HEADS)
    ref = reference(q, k, vt, bias, HD, S, S_pad, 1.0, heads=HEADS, nb=NB)
    yard = yardstick_online(q, k, vt, bias, S, S_pad, 1.0)
    assert_close(yard, ref, f"online yardstick {sid((S, S_pad))} channels [{lo},{hi})")
    return q, k, vt, bias, ref, figures(yard, ref)


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_qk_channels_64_to_80_alone(dev, c, qi):
    """CHANNEL_CASES' [64, 80) of tests/test_text_attention_gpu.py: the half-empty third MFMA of every score tile on its own"""
    (S, S_pad), sk = c
    q, k, vt, bias, ref, y = channel_case(S, S_pad, 64, 80)
    out = launch_s(dev, qi, sk, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    what = f"{case_id(c)} qi={qi} channels [64,80)"
    untouched(out, S, S_pad, what)
    got = rows(out, S, S_pad)
    print(f"  STREAM80 CHANNELS {case_id(c)} qi={qi} kernel {figures(got, ref)} | yardstick {y}")
    assert_close(got, ref, what)


@torch.no_grad()
@pytest.mark.parametrize("c", [((200, 224), 1), ((449, 480), 0), ((729, 736), 0)], ids=case_id)
def test_heads_of_72_zero_padded_to_80_are_exact(dev, c):
    """the packing of a head-dim-72 tower: channels [72, 80) of q, k and v of every head are zero.  The scores are those of the 72 real
    channels, and output channels [72, 80) are exactly 0 (sums of P x 0), in the resident kernel as in the streaming one."""
    (S, S_pad), sk = c
    q, k, vt, bias, ref, _ = channel_case(S, S_pad, 0, 72, zero_v_from=72)
    out = launch_s(dev, 0, sk, *to_dev(dev, q, k, vt, bias), S, S_pad, 1.0)
    torch.cuda.synchronize()
    untouched(out, S, S_pad, f"{case_id(c)} zero-padded heads")
    got = rows(out, S, S_pad)
    assert_close(got, ref, f"{case_id(c)} zero-padded heads")
    pad = got.view(NB, S, HEADS, HD)[..., 72:]
    assert bool((pad == 0).all()), f"{case_id(c)}: {int((pad != 0).sum())} nonzero values in the padded output channels"


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("c", [((200, 224), 1), ((729, 736), 0)], ids=case_id)
def test_repeatable_batch_invariant_and_independent_of_qi(dev, c):
    (S, S_pad), sk = c
    q, k, vt, bias, scale, _, _ = case(S, S_pad, "folded", "per_head")
    qd, kd, vd, bd = to_dev(dev, q, k, vt, bias)
    one = launch_s(dev, 1, sk, qd, kd, vd, bd, S, S_pad, scale)
    four = launch_s(dev, 4, sk, qd, kd, vd, bd, S, S_pad, scale)
    again = launch_s(dev, 1, sk, qd, kd, vd, bd, S, S_pad, scale)
    auto = launch_s(dev, 0, sk, qd, kd, vd, bd, S, S_pad, scale)
    alone = []
    for z in range(NB):   # the same buffers, one sequence at a time: same pitches, pointers moved to sequence z
        o = launch_s(dev, 1, sk, qd[z * S_pad:], kd[z * S_pad:], vd[:, z * S_pad:], bd, S, S_pad, scale, nb=1)
        alone.append(o[:S_pad])
    torch.cuda.synchronize()
    assert torch.equal(bits(four), bits(one)), "qi = 4 differs from qi = 1"
    assert torch.equal(bits(again), bits(one)), "a repeated launch differs"
    assert wide_rule(HEADS, NB, S_pad) == 1
    assert torch.equal(bits(auto), bits(one)), "qi = 0 differs from the instantiation the rule names"
    assert torch.equal(bits(torch.cat(alone)), bits(one[:NB * S_pad])), "two B = 1 launches differ from the B = 2 launch"


@torch.no_grad()
@pytest.mark.parametrize("shape", [(100, 128), (449, 480)], ids=sid)
def test_the_natural_route_keeps_the_resident_kernel_up_to_480_keys(dev, shape):
    """stream_keys = 0 at S_pad <= 480 is the launch rf_debug_text_attention(80, qi = 0) makes, bit for bit; the forced streaming launch
    is another kernel with another summation order: not bit-equal, and within the same bound of the fp64 reference"""
    S, S_pad = shape
    q, k, vt, bias, scale, ref, _ = case(S, S_pad, "scaled", "per_head")
    qd, kd, vd, bd = to_dev(dev, q, k, vt, bias)
    product = launch_s(dev, 0, 0, qd, kd, vd, bd, S, S_pad, scale)
    debug = launch(dev, HD, 0, qd, kd, vd, bd, S, S_pad, scale, heads=HEADS, nb=NB)
    forced = launch_s(dev, 0, 1, qd, kd, vd, bd, S, S_pad, scale)
    torch.cuda.synchronize()
    assert torch.equal(bits(product), bits(debug))
    assert_close(rows(product, S, S_pad), ref, f"resident {sid(shape)}")
    assert_close(rows(forced, S, S_pad), ref, f"forced {sid(shape)}")
