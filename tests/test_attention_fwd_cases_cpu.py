"""The forward-attention cases are what they claim to be, and their checkers have teeth -- all without a GPU.

  * selector: pi_h is a permutation, the matching score leads every other by >= 24 + log2 S (so the other S - 1 keys together weigh
    < 2^-24), and the fp64 softmax output is within 2^-12 of v[pi]: "the output row IS the value row" is a condition, not a tolerance.
  * census: the fp64 output is 64 (h + 1) / S everywhere.
  * the V^T builder round-trips through vt_unpermute (also with s_pad > S) and equals make_qkv's layout.
  * the mixed-size plans add up; the split shapes qualify on a 256-CU part.
  * teeth: outputs of emulated kernel defects (built in torch, rounded to bf16 as a kernel would) fail the checkers, and the failure
    message names the defect.
"""
import math
import re

import pytest
import torch

from tests import attn_fwd_cases as A

BF = torch.bfloat16
SELECTOR_CASES = [(A.SWEEP_H, S) for S in A.RING_SWEEP] + list(A.SPLIT_SHAPES)


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("H,S", SELECTOR_CASES)
def test_selector_case_is_exact(H, S):
    c = A.build_selector(H, S, "cpu")
    v = A.selector_values(H, S)
    assert torch.equal(c.vf, v) and torch.equal(v.float(), v.float().round()) and 1 <= int(v.float().min()) and int(v.float().max()) <= 251
    assert torch.equal(A.vt_unpermute(c.vt, S), c.vf)
    worst = 1e9
    for h in range(H):
        pi = A.selector_pi(h, S)
        assert torch.equal(pi.sort().values, torch.arange(S)), f"pi_{h} is not a permutation at S = {S}"
        s = c.qp[h].double() @ c.kf[h].double().T                                           # exact: sums of 128 values +-0.75
        assert float(s.abs().max()) <= 96.0 < A.SELECTOR_BOUND
        match = s[torch.arange(S), pi]
        assert torch.equal(match, torch.full((S,), 96.0, dtype=torch.float64))
        other = s.clone()
        other[torch.arange(S), pi] = -1e9
        margin = float((match - other.amax(-1)).min())
        worst = min(worst, margin)
        assert margin >= 24 + math.log2(S), f"H={H} S={S} head {h}: margin {margin} < {24 + math.log2(S):.1f}: change the seed"
        ref = A.softmax_ref64(c.qp[h:h + 1], c.kf[h:h + 1], c.vf[h:h + 1]).double()
        assert float((ref - v[h, pi].double()).abs().max()) < 2.0 ** -12
    print(f"  selector H={H} S={S}: smallest margin {worst} (needs {24 + math.log2(S):.1f})")
    # the expected tensor is that reference, rounded
    A.check_selector(A.selector_expected(H, S).to(BF), H, S, "expected")


@pytest.mark.parametrize("H,S", SELECTOR_CASES)
def test_census_reference(H, S):
    c = A.build_census(H, S, "cpu")
    assert float(c.qp.float().abs().max()) == 0.0 and S // 64 <= 128
    exp = A.census_expected(H, S)
    for h in range(0, H, 8):
        ref = A.softmax_ref64(c.qp[h:h + 8], c.kf[h:h + 8], c.vf[h:h + 8])
        assert torch.equal(ref, exp[:, h * 128:(h + 8) * 128]), "the fp64 census output is not 64 (h + 1) / S"
    want = torch.tensor([64.0 * (h + 1) / S for h in range(H)], dtype=torch.float64).float()
    assert torch.equal(exp.view(S, H, 128), want[None, :, None].expand(S, H, 128))
    A.check_census(exp.to(BF), H, S, "expected")                                            # one rounding: inside one bf16 ulp


@pytest.mark.parametrize("S,s_pad", [(256, 256), (256, 320), (768, 960), (333, 384), (333, 512), (64, 64)])
def test_vt_builder_round_trips(S, s_pad):
    vf = A.rnd(3, S, 128, dev="cpu", seed=S)
    vt = A.vt_pack(vf, s_pad, pad_fill=float("nan"))
    assert vt.shape == (3, s_pad // 64, 128, 64) and vt.is_contiguous()
    assert torch.equal(A.vt_unpermute(vt, S), vf)
    full = (S + 63) // 64
    assert torch.isnan(vt[:, full:].float()).all(), "whole pad tiles hold the fill"
    assert float(vt[:, :full].float().nan_to_num(nan=1e9).abs().max()) < 1e9, "the pad columns of the partial tile are finite"
    if S % 64:
        assert float(A.vt_unpermute(vt, full * 64)[:, S:].float().abs().max()) == 0.0
    # bits 2 and 3 of the key index inside its tile are swapped: key 4 sits at position 8, key 8 at position 4
    assert torch.equal(vt[:, 0, :, 8], vf[:, 4]) and torch.equal(vt[:, 0, :, 4], vf[:, 8]) and torch.equal(vt[:, 0, :, 12], vf[:, 12])
    # the builders at s_pad > S hold the same operands as at s_pad == S
    for build in (A.build_random, A.build_selector, A.build_census):
        if S % 64 == 0 and s_pad > S:
            a, b = build(3, S, "cpu", 5), build(3, S, "cpu", 5, s_pad=s_pad, pad_fill=float("nan"))
            assert b.q.shape == (3, s_pad, 128) and b.s_pad == s_pad and a.s_pad == S
            assert torch.equal(a.q, b.q[:, :S]) and torch.equal(a.k, b.k[:, :S]) and torch.equal(a.vt, b.vt[:, :S // 64])
            assert torch.isnan(b.q[:, S:].float()).all() and torch.isnan(b.k[:, S:].float()).all() and torch.isnan(b.vt[:, S // 64:].float()).all()
            assert all(torch.equal(x, y) for x, y in zip(a[3:6], b[3:6]))


def test_random_builder_is_prescaled():
    from reflectionflow_amd import ops
    q, k, vt, qp, kf, vf = A.prescaled(3, 256, "cpu", seed=256)
    c = A.build_random(3, 256, "cpu", 256)
    assert all(torch.equal(x, y) for x, y in zip(c[:6], (q, k, vt, qp, kf, vf)))
    qf = A.make_qkv(3, 256, "cpu", seed=256)[3]
    assert torch.equal(qp, (qf.float() * ops.QK_PRESCALE).to(BF))


def test_case_lists():
    assert tuple(f.name for f in A.FORMS) == ("ONLINE128", "ONLINE256", "BOUNDED32", "BOUNDED16", "LAGGED16", "BOUNDED16_MIX", "LAGGED16_MIX")
    assert [f.path for f in A.FORMS + A.SPLIT_FORMS] == [1, 2, 4, 5, 8, 10, 11, 6, 9]
    assert A.RING_SWEEP == tuple(range(256, 2305, 256)) and A.SWEEP_H % 8 != 0
    assert all(math.gcd(73, S) == 1 for S in A.RING_SWEEP)
    seen = set()
    for S in A.RING_SWEEP:
        plans = A.mix_plans(S)
        assert plans[0] == 0 and plans == tuple(b for b in range(0, S, 4) if 12 * b <= S // 16)
        for b in plans:
            a, b2 = A.mix_sizes(S, b)
            assert b2 == b and a >= 0 and 256 * a + 192 * b == S, (S, b)
            if a == 0:
                seen.add((S, b))
    assert seen == {(768, 4), (1536, 8), (2304, 12)} == set(A.ALL_SMALL.items())
    labels = [x[0] for x in A.launches(A.FORMS, 2304)]
    assert len(labels) == len(set(labels)) == 5 + 2 * 4
    for H, S in A.SPLIT_SHAPES:
        assert A.split_qualifies(H, S, 256), (H, S)
        assert all(A.form_runs(f, H, S, 256) for f in A.FORMS + A.SPLIT_FORMS)
    for S in A.RING_SWEEP:
        assert not A.split_qualifies(A.SWEEP_H, S, 256)
        assert all(A.form_runs(f, A.SWEEP_H, S, 256) for f in A.FORMS) and not any(A.form_runs(f, A.SWEEP_H, S, 256) for f in A.SPLIT_FORMS)
    # the predicate follows the CU count (the library rounds it down to whole XCD rows) and the ring precondition
    assert A.split_qualifies(8, 2048, 256) and not A.split_qualifies(8, 1792, 256) and A.split_qualifies(8, 1792, 199)
    assert not A.split_qualifies(8, 2304, 328) and not A.form_runs(A.BOUNDED16, 3, 320, 256) and A.form_runs(A.ONLINE256, 3, 333, 256)


# ------------------------------------------------------------------------------------------------------------ the teeth
def emulate(c, drop=None, twice=None, v_of_key=None, swap_rows=None, swap_dtiles=None, head_shift=0):
    """fp64 attention over the operands of a case with one defect of a kernel, rounded to bf16: [S, H*128]
       drop / twice   key tile whose P is counted 0 / 2 times (in O and in l)
       v_of_key       index tensor [S]: key j's P multiplies v[v_of_key[j]] instead of v[j]
       swap_rows / swap_dtiles / head_shift: the output's query rows / 16-column d tiles / head slots moved"""
    H, S = c.qp.shape[0], c.S
    s = torch.einsum("hqd,hkd->hqk", c.qp.double(), c.kf.double())
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    if drop is not None:
        p[:, :, 64 * drop:64 * drop + 64] = 0
    if twice is not None:
        p[:, :, 64 * twice:64 * twice + 64] *= 2
    v = c.vf.double() if v_of_key is None else c.vf.double()[:, v_of_key]
    o = torch.einsum("hqk,hkd->hqd", p / p.sum(-1, keepdim=True), v)                        # [H, S, 128]
    if swap_rows is not None:
        a, b = swap_rows
        o[:, [a, b]] = o[:, [b, a]]
    if swap_dtiles is not None:
        a, b = swap_dtiles
        o = o.view(H, S, 8, 16)
        o[:, :, [a, b]] = o[:, :, [b, a]]
        o = o.reshape(H, S, 128)
    o = torch.roll(o, head_shift, 0)
    return o.permute(1, 0, 2).reshape(S, H * 128).to(BF)


@pytest.fixture(scope="module")
def teeth_cases():
    H, S = 3, 512
    return H, S, A.build_selector(H, S, "cpu"), A.build_census(H, S, "cpu")


def test_checkers_accept_the_correct_output(teeth_cases):
    H, S, sel, cen = teeth_cases
    A.check_selector(emulate(sel), H, S, "selector")
    A.check_census(emulate(cen), H, S, "census")


def _fails(check, out, H, S, pattern):
    with pytest.raises(AssertionError) as e:
        check(out, H, S, "emulated")
    msg = str(e.value)
    assert re.search(pattern, msg), f"the message does not name the defect ({pattern!r}): {msg}"
    assert re.search(r"first bad \(row \d+, head \d+, column \d+\)", msg), msg
    return msg


def test_teeth_a_dropped_key_tile(teeth_cases):
    H, S, sel, cen = teeth_cases
    _fails(A.check_census, emulate(cen, drop=5), H, S, r"key tile 5 counted 0\.00x")
    msg = _fails(A.check_selector, emulate(sel, drop=5), H, S, r"carries no key's code \(expected key (\d+)")
    assert int(re.search(r"expected key (\d+)", msg).group(1)) // 64 == 5            # the first bad row is one whose key was in the tile


def test_teeth_a_key_tile_counted_twice(teeth_cases):
    H, S, sel, cen = teeth_cases
    _fails(A.check_census, emulate(cen, twice=2), H, S, r"key tile 2 counted 2\.00x")
    # (one-hot rows cannot see this: twice the only key that matters is still all of the row)
    A.check_selector(emulate(sel, twice=2), H, S, "selector")


def test_teeth_k_tile_paired_with_the_next_vt_tile(teeth_cases):
    H, S, sel, cen = teeth_cases
    nxt = (torch.arange(S) + 64) % S
    msg = _fails(A.check_selector, emulate(sel, v_of_key=nxt), H, S, r"K tile (\d+) was paired with V\^T tile (\d+)")
    t, t2 = (int(x) for x in re.search(r"K tile (\d+) was paired with V\^T tile (\d+)", msg).groups())
    assert t2 == (t + 1) % (S // 64)


def test_teeth_vt_key_permutation_missing(teeth_cases):
    H, S, sel, cen = teeth_cases
    msg = _fails(A.check_selector, emulate(sel, v_of_key=A.vt_position(torch.arange(S))), H, S, r"bits 2 and 3 of the key index are swapped")
    got, want = (int(x) for x in re.search(r"carries key (\d+) \(expected key (\d+)", msg).groups())
    assert got != want and got == int(A.vt_position(torch.tensor(want)))


def test_teeth_two_query_rows_of_a_q_tile_exchanged(teeth_cases):
    H, S, sel, cen = teeth_cases
    msg = _fails(A.check_selector, emulate(sel, swap_rows=(16 * 7 + 3, 16 * 7 + 12)), H, S, r"query rows exchanged")
    assert "first bad (row 115, head 0" in msg and "key of query row 124" in msg


def test_teeth_two_d_tiles_exchanged(teeth_cases):
    H, S, sel, cen = teeth_cases
    msg = _fails(A.check_selector, emulate(sel, swap_dtiles=(2, 5)), H, S, r"d tile 2 holds d tile 5, d tile 5 holds d tile 2")
    assert "column 32)" in msg


def test_teeth_head_written_at_the_next_head(teeth_cases):
    H, S, sel, cen = teeth_cases
    msg = _fails(A.check_selector, emulate(sel, head_shift=1), H, S, r"head offset")
    assert "head 2's own row written at head 0" in msg
    _fails(A.check_census, emulate(cen, head_shift=1), H, S, r"head 1: every key tile off by the factor 0\.5000: that is the value of head 0")


def test_teeth_non_finite_and_lse():
    H, S = 3, 256
    out = A.census_expected(H, S).to(BF)
    out[17, 130] = float("nan")
    with pytest.raises(AssertionError, match=r"first bad \(row 17, head 1, column 2\)"):
        A.check_census(out, H, S, "nan")
    out = A.selector_expected(H, S).to(BF)
    out[200, 5] = float("inf")
    with pytest.raises(AssertionError, match=r"first bad \(row 200, head 0, column 5\)"):
        A.check_selector(out, H, S, "inf")
    c = A.build_random(H, S, "cpu", 7)
    ref = A.lse_ref64(c.qp, c.kf)
    assert torch.allclose(ref, torch.logsumexp(torch.einsum("hqd,hkd->hqk", c.qp.double(), c.kf.double()) * math.log(2), -1) / math.log(2),
                          rtol=0, atol=1e-12)
    lse = torch.full((H, 320), 1e30)
    lse[:, :S] = ref.float()
    A.check_lse(lse, ref, S, "exact")
    assert abs(A.LSE_BOUND - 6.6e-3) < 1e-4
    lse[1, 100] += 8e-3                                  # a row sum off by 0.55 %
    with pytest.raises(AssertionError, match="lse off by"):
        A.check_lse(lse, ref, S, "off")
