"""GPU: attn64_stream_kernel (csrc/text.hip), the head-dim-64 attention that streams K / V^T through the LDS in chunks of 128 keys with an
online softmax, one launch at a time through rf_text_attention -- the launch site the towers use.  stream_keys = 1 runs it at shapes
where the resident kernel also runs; beyond 512 keys (ViT-L/14 at 336 px: 577 tokens, S_pad 608) it is what stream_keys = 0 launches.

Reference, operands, bound and helpers: tests/test_text_attention_gpu.py (fp64 from the same bf16 operands; assert_close: elementwise
1.2e-2 |ref| + 1.2e-2 mean|ref|, rel-L2 < 4e-3; NaN gaps, +-1e4 padding, `out` prefilled with 7.0).  Every case: heads = 2, B = 2.
Yardstick: `yardstick_online()` below, the kernel's arithmetic in fp32 torch with its roundings, in the ONLINE form: per 128-key chunk
the chunk maximum, m' = max(m, chunk), O and l rescaled by exp2(m - m'), P = exp2(s - m') rounded to bf16 for the PV product, l from the
unrounded P, one division and one rounding at the end.  It is held to the same bound in every case before the kernel is
(profiles/text_attention_stream.md has its table).  As in the resident tests the causal mask goes with peaked scores at every shape
and with folded scores up to 128 keys only (parity_variants' docstring in tests/test_text_attention_gpu.py says why).

Shapes (S, S_pad) against the 128-key chunk: 32, 64 = one partial chunk; 128 = one whole chunk; 160 = whole + partial; 256, 512 = whole
chunks only; 288 = two whole + a partial tail; natural route: 544 = 4 whole + 32 keys, 608 = 4 whole + 96, 1056 = 8 whole + 32.
"""
import functools

import pytest
import torch

from tests.test_text_attention_gpu import (BF, FILL, FORMS, NINF, assert_close, assert_untouched, figures, launch, make_bias, make_operands,
                                           real_rows, reference, to_dev, wide_rule, _per_head)

pytestmark = pytest.mark.gpu
HEADS, NB, HD, CK = 2, 2, 64, 128
LOG2E = 1.4426950408889634
FORCED = [(1, 32), (33, 64), (100, 128), (130, 160), (256, 256), (257, 288), (500, 512)]
NATURAL = [(530, 544), (577, 608), (1025, 1056)]
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


def yardstick_online(q, k, vt, bias, S, S_pad, scale):
    """attn64_stream_kernel's arithmetic in fp32 with its roundings (module docstring); chunks of CK keys from key 0, real keys only (a
    padded key's -inf bias gives P = 0 and leaves every sum as it is)"""
    out = torch.zeros(NB, S, HEADS * HD, dtype=BF)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    for z, h, qh, kh, vh, b in _per_head(q, k, vt, bias, HD, S, S_pad, HEADS, NB):
        s = (qh.float() @ kh.float().t()) * sl2
        if b is not None:
            s = s + b * torch.tensor(LOG2E, dtype=torch.float32)
        m = torch.full((S, 1), NINF)
        l = torch.zeros(S, 1)
        o = torch.zeros(S, HD)
        for c0 in range(0, S, CK):
            sc = s[:, c0:c0 + CK]
            mnew = torch.maximum(m, sc.max(dim=-1, keepdim=True).values)
            msub = torch.where(mnew > NINF, mnew, torch.zeros_like(mnew))
            alpha = torch.exp2(m - msub)
            p = torch.exp2(sc - msub)
            o = o * alpha + p.to(BF).float() @ vh[c0:c0 + CK].float()
            l = l * alpha + p.sum(dim=-1, keepdim=True)
            m = mnew
        out[z, :, h * HD:(h + 1) * HD] = (o / l).to(BF)
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
    """rf_text_attention on device tensors; out [nb * S_pad + 1][q.shape[1]] prefilled with 7.0 (the last row is a guard row)"""
    from reflectionflow_amd import _lib
    from reflectionflow_amd.ops import stream_ptr
    out = torch.full((nb * S_pad + 1, q.shape[1]), FILL, dtype=BF, device=dev)
    if bias_hs is None:
        bias_hs = S_pad * S_pad if bias is not None and bias.shape[0] > 1 else 0
    rc = _lib.load().rf_text_attention(HD, qi, stream_keys, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), vt.stride(0),
                                       None if bias is None else bias.data_ptr(), bias_hs, out.data_ptr(), out.stride(0), HEADS, nb, S, S_pad, scale,
                                       stream_ptr())
    _lib.check(rc, "rf_text_attention")
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
        print(f"  STREAM {case_id(c)} qi={qi} {form:6s} {kind:8s} kernel {figures(got, ref)} | yardstick {y}")
        assert_close(got, ref, what)


# ---- masks that empty whole chunks ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(which):
    """S = 384 of S_pad = 416: the partial last chunk [384, 416) holds padded keys only (a chunk of -inf at the end) in every variant.
    'middle': keys [128, 256) are -inf for every row as well.  'first': rows i % 3 == 0 see -inf in all of [0, 128), i.e. their state
    is still empty when the second chunk arrives; rows i % 3 == 1 see -inf everywhere but in the LAST real chunk."""
    S, S_pad = 384, 416
    q, k, vt = make_operands(HD, S, S_pad, HD ** -0.5, 40, heads=HEADS, nb=NB)
    bias = make_bias("per_head", S, S_pad, 40, heads=HEADS).clone()
    i = torch.arange(S_pad)
    if which == "middle":
        bias[:, :, 128:256] = NINF
    else:
        bias[:, i % 3 == 0, 0:128] = NINF
        bias[:, i % 3 == 1, 0:256] = NINF
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
    print(f"  STREAM mask {which:6s} qi={qi} kernel {figures(got, ref)} | yardstick {y}")
    assert_close(got, ref, what)


# ---- exact key routing, one chunk position at a time ------------------------------------------------------------------------------------------
ROUTES = [((280, 288), 1, (0, 128)), ((280, 288), 1, (128, 256)), ((280, 288), 1, (256, 280)),
          ((577, 608), 0, (0, 128)), ((577, 608), 0, (256, 384)), ((577, 608), 0, (512, 577))]


@torch.no_grad()
@pytest.mark.parametrize("qi", [1, 4])
@pytest.mark.parametrize("shape,sk,keys", ROUTES, ids=[f"{sid(r[0])}-keys{r[2][0]}to{r[2][1]}" for r in ROUTES])
def test_exact_key_routing_per_chunk_position(dev, shape, sk, keys, qi):
    """One key per query row has bias 0, every other -inf, and all selected keys lie in ONE chunk (first, a middle one, the partial
    last): p = 1 there and 0 elsewhere, every other chunk leaves the state as it is, l = 1: out[z][i][h] is v[z][key_h(i)][h] bit for
    bit -- chunk addressing of K / V^T / bias, the slot permutation inside the chunk, and the rescale by exactly 0 or 1."""
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


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("c", [((257, 288), 1), ((577, 608), 0)], ids=case_id)
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
@pytest.mark.parametrize("shape", [(100, 128), (500, 512)], ids=sid)
def test_the_products_rule_keeps_the_resident_kernel_up_to_512_keys(dev, shape):
    """stream_keys = 0 at S_pad <= 512 is the launch rf_debug_text_attention(qi = 0) makes, bit for bit; the forced streaming launch is
    another kernel with another rounding order and is merely close"""
    S, S_pad = shape
    q, k, vt, bias, scale, ref, _ = case(S, S_pad, "scaled", "per_head")
    qd, kd, vd, bd = to_dev(dev, q, k, vt, bias)
    product = launch_s(dev, 0, 0, qd, kd, vd, bd, S, S_pad, scale)
    debug = launch(dev, HD, 0, qd, kd, vd, bd, S, S_pad, scale, heads=HEADS, nb=NB)
    forced = launch_s(dev, 0, 1, qd, kd, vd, bd, S, S_pad, scale)
    torch.cuda.synchronize()
    assert torch.equal(bits(product), bits(debug))
    assert_close(rows(forced, S, S_pad), ref, f"forced {sid(shape)}")
