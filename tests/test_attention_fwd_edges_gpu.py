"""Forward attention at the small shapes and edges where a re-scheduled kernel goes wrong: every ring depth 1..9, every legal
mixed-size plan (the all-small ones included), the split launch at its smallest shapes with more than 8 heads, padded operands,
pitched outputs, the row statistic of every form, and inputs that tell WHICH key / tile / row / column an output used
(tests/attn_fwd_cases.py; the checkers' teeth are proven on the CPU in test_attention_fwd_cases_cpu.py).

Every form is requested explicitly and must run exactly where attn_fwd_cases.form_runs says so (an RFError there is a failure; where
it says no, the request must raise), and rf_debug_last_attn_path() must name the kernel asked for.
"""
import math

import pytest
import torch

from tests import attn_fwd_cases as A

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
RANDOM_BOUND = 60.0                 # i.i.d. N(0, 1) rows and a prescaled q: the scores have sigma 1.44, |s| < 12 at these sizes
ALL_FORMS = A.FORMS + A.SPLIT_FORMS
SWEEP_CASES = [(A.SWEEP_H, S) for S in A.RING_SWEEP]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(form, c, bound, cus, mix_small=0, **kw):
    """one explicit request: the output where the form must run, None after asserting that it raises where it must not"""
    from reflectionflow_amd import _lib as L, ops
    H = c.q.shape[0]

    def call():
        return ops.attention(c.q, c.k, c.vt, c.S, q_prescaled=True, score_bound=bound, kernel=form.kernel, mix_small=mix_small, **kw)
    if not A.form_runs(form, H, c.S, cus):
        with pytest.raises(ops.RFError):
            call()
        return None
    out = call()
    assert L.load().rf_debug_last_attn_path() == form.path, (form.name, L.load().rf_debug_last_attn_path())
    return out


def run_all(c, bound, cus, forms, what):
    """{label: output} of every launch of a case that runs here (each asserted to take its own path)"""
    outs = {}
    for label, form, b in A.launches(forms, c.S):
        o = launch(form, c, bound, cus, mix_small=b)
        if o is not None:
            outs[label] = o
    print(f"  {what} H={c.q.shape[0]} S={c.S} on {cus} CUs ran: {' '.join(outs)}")
    return outs


def forms_of_case(H):
    """the sweep (H = 3) asks for every form (the split requests must raise there); the split shapes run the two split forms"""
    return ALL_FORMS if H == A.SWEEP_H else A.SPLIT_FORMS


@pytest.mark.parametrize("S", A.RING_SWEEP)
def test_ring_rounds_vs_fp64(dev, cus, S):
    """Ring depths 1..9 of the 4-slot K / V^T rings (the prologue's nt > 1 / nt > 2 guards, the counted drain), at three heads."""
    H = A.SWEEP_H
    c = A.build_random(H, S, dev, seed=S)
    ref = A.ref64_chunked(c.qp, c.kf, c.vf)
    outs = run_all(c, RANDOM_BOUND, cus, ALL_FORMS, "ring")
    assert set(outs) == {lab for lab, _, _ in A.launches(A.FORMS, S)}               # S % 256 == 0, H = 3: all but the split launch
    for label, form, b in A.launches(A.FORMS, S):
        again = launch(form, c, RANDOM_BOUND, cus, mix_small=b)
        assert torch.equal(again, outs[label]), f"{label} S={S}: not bit-stable"
    e = {}
    for label, o in outs.items():
        A.assert_close(o, ref, f"attention {label} S={S}", atol=2e-3)
        e[label] = A.rel_l2(o, ref)
    print(f"  S={S}: rel-L2 vs fp64: " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    assert all(v <= 1.3 * e["ONLINE256"] + 1e-4 for n, v in e.items() if n.startswith("LAGGED")), e
    for label, form, b in A.launches(A.FORMS, S):
        if form.mix:                                                                    # "bit-identical rows", also with no big workgroup
            a = A.mix_sizes(S, b)[0]
            assert torch.equal(outs[label], outs[A.PLAIN_OF[form.name]]), \
                f"S={S}: mixed-size launch {label} ({a} x 256 + {b} x 192 queries per head) differs from the plain launch"


@pytest.mark.parametrize("H,S", SWEEP_CASES + list(A.SPLIT_SHAPES))
def test_selector_identifies_the_key_every_row_used(dev, cus, H, S):
    """One-hot rows whose value row is a code of (head, key): the output must BE v[pi(row)].  (In the lagged forms the matching key
    mostly lies outside the first tile: the row is re-centred at a tile chosen by pi.)"""
    c = A.build_selector(H, S, dev)
    outs = run_all(c, A.SELECTOR_BOUND, cus, forms_of_case(H), "selector")
    assert outs
    for label, o in outs.items():
        A.check_selector(o, H, S, f"selector {label} H={H} S={S}")


@pytest.mark.parametrize("H,S", SWEEP_CASES + list(A.SPLIT_SHAPES))
def test_census_counts_every_key_tile_once(dev, cus, H, S):
    """q = 0: every P is 1 and every key tile reports its multiplicity in its own columns."""
    c = A.build_census(H, S, dev, seed=S)
    outs = run_all(c, RANDOM_BOUND, cus, forms_of_case(H), "census")
    assert outs
    for label, o in outs.items():
        A.check_census(o, H, S, f"census {label} H={H} S={S}")


@pytest.mark.parametrize("H,S", A.SPLIT_SHAPES)
def test_split_launch_small_shapes_vs_fp64(dev, cus, H, S):
    """The share arithmetic of the split launch (heads / 8 > 1, blocks spread over 2-3 workgroups, pieces with t0 != 0) with a scratch
    full of NaN: every slot that is read was written by this launch."""
    from reflectionflow_amd import _lib as L, ops
    c = A.build_random(H, S, dev, seed=H + S)
    ref = A.ref64_chunked(c.qp, c.kf, c.vf)
    ws = ops.attn_scratch(dev)
    ran = []
    for form in A.SPLIT_FORMS:
        o = []
        for _ in range(2):
            ws.view(torch.uint8).fill_(0xFF)
            o.append(launch(form, c, RANDOM_BOUND, cus))
        if o[0] is None:
            continue
        ran.append(form.name)
        e = A.assert_close(o[0], ref, f"{form.name} H={H} S={S}", atol=2e-3)
        print(f"  split H={H} S={S}: {form.name} rel-L2 vs fp64 {e:.2e}")
        assert torch.equal(o[0], o[1]), f"{form.name} H={H} S={S}: not bit-stable"
    assert ran == [f.name for f in A.SPLIT_FORMS if A.form_runs(f, H, S, cus)]
    for bound in (RANDOM_BOUND, 0.0):                                                   # what the dispatch itself picks, scratch attached
        ws.view(torch.uint8).fill_(0xFF)
        o = ops.attention(c.q, c.k, c.vt, S, q_prescaled=True, score_bound=bound)
        path = L.load().rf_debug_last_attn_path()
        e = A.assert_close(o, ref, f"AUTO (bound {bound}) H={H} S={S}", atol=2e-3)
        print(f"  split H={H} S={S} on {cus} CUs: AUTO with bound {bound} took path {path}, rel-L2 vs fp64 {e:.2e}; split forms ran: {ran}")


OUT_SENTINEL, LSE_SENTINEL = -32768.0, -1.0e30


@pytest.mark.parametrize("S", [256, 768])
def test_layout_edges(dev, cus, S):
    """s_pad > S (another head stride of q / k, more V^T tiles per head) with NaN in everything the contract says is never read, an
    `out` of a wider pitch (16-byte and 8-byte aligned rows: both store paths of the epilogues) and a pre-filled lse: the same bits as
    from tight operands, and nothing else touched."""
    H = A.SWEEP_H
    tight = A.build_random(H, S, dev, seed=S + 1)
    cases = [(f.name, f, A.ALL_SMALL.get(S, 0) if f.mix else 0) for f in A.FORMS]          # MIX: the all-small plan where S has one
    ref = {}
    for label, form, b in cases:
        lse = torch.full((H, S), LSE_SENTINEL, dtype=torch.float32, device=dev)
        ref[label] = (launch(form, tight, RANDOM_BOUND, cus, mix_small=b, lse=lse), lse)
        assert torch.isfinite(lse).all() and bool((lse != LSE_SENTINEL).all())
    for s_pad in (S + 64, S + 192):
        c = A.build_random(H, S, dev, seed=S + 1, s_pad=s_pad, pad_fill=float("nan"))
        assert c.q.shape[1] == s_pad and c.vt.shape[1] == s_pad // 64 and torch.isnan(c.vt[:, S // 64:].float()).all()
        for pitch in (H * 128 + 8, H * 128 + 4):
            for label, form, b in cases:
                buf = torch.full((S, pitch), OUT_SENTINEL, dtype=BF, device=dev)
                out = buf[:, :H * 128]
                assert out.data_ptr() % 16 == 0 and out.stride(0) == pitch
                lse = torch.full((H, s_pad), LSE_SENTINEL, dtype=torch.float32, device=dev)
                got = launch(form, c, RANDOM_BOUND, cus, mix_small=b, out=out, lse=lse)
                what = f"{label} S={S} s_pad={s_pad} pitch={pitch}"
                assert got.data_ptr() == out.data_ptr()
                assert torch.equal(out, ref[label][0]), f"{what}: output differs from the tight operands' " \
                    f"({int((out != ref[label][0]).sum())} elements, non-finite: {int((~torch.isfinite(out.float())).sum())})"
                assert bool((buf[:, H * 128:] == OUT_SENTINEL).all()), f"{what}: wrote outside its {H * 128} columns"
                assert torch.equal(lse[:, :S], ref[label][1]), f"{what}: lse differs"
                assert bool((lse[:, S:] == LSE_SENTINEL).all()), f"{what}: lse rows >= S written"


@pytest.mark.parametrize("H,S", [(A.SWEEP_H, 256), (A.SWEEP_H, 1280), (16, 1536)])
def test_lse_every_form(dev, cus, H, S):
    """rf_attn_desc.lse of every form against the fp64 log2-sum-exp2, at a bound derived from the number formats (attn_fwd_cases.LSE_BOUND);
    producing it must not change the output."""
    c = A.build_random(H, S, dev, seed=3 * S + H)
    ref = A.lse_ref64(c.qp, c.kf)
    worst = {}
    for label, form, b in A.launches(ALL_FORMS, S):
        plain = launch(form, c, RANDOM_BOUND, cus, mix_small=b)
        if plain is None:
            continue
        lse = torch.full((H, c.s_pad), float("nan"), dtype=torch.float32, device=dev)
        with_lse = launch(form, c, RANDOM_BOUND, cus, mix_small=b, lse=lse)
        assert torch.equal(plain, with_lse), f"{label} H={H} S={S}: the output changes when lse is produced"
        worst[label] = A.check_lse(lse, ref, S, f"{label} H={H} S={S}")
    assert set(worst) == {lab for lab, f, _ in A.launches(ALL_FORMS, S) if A.form_runs(f, H, S, cus)}
    print(f"  lse H={H} S={S}: " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))


@pytest.mark.parametrize("H,S,mode,pre,bound", [(8, 512, 0, 1, 60.0), (8, 512, 0, 1, 0.0), (3, 333, 1, 0, 0.0)])
def test_plain_entry_points_equal_the_descriptor_call(dev, H, S, mode, pre, bound):
    """rf_attention_fwd / rf_attention_fwd_ws fill a descriptor with kernel = AUTO: the same bits and the same path as rf_attention."""
    from reflectionflow_amd import _lib as L, ops
    lib = L.load()
    c = A.build_random(H, S, dev, seed=S)
    n_main, bias, scale = (200, 0.7, 1.0 / math.sqrt(128.0)) if mode else (S, 0.0, 1.0 / math.sqrt(128.0))
    ws = ops.attn_scratch(dev)
    for with_ws in (False, True):
        want = ops.attention(c.q, c.k, c.vt, S, n_main=n_main, mode=mode, cross_bias=bias, scale=scale, q_prescaled=bool(pre),
                             score_bound=bound, scratch=with_ws, kernel=L.RF_ATTN_AUTO)
        path = lib.rf_debug_last_attn_path()
        out = torch.full_like(want, OUT_SENTINEL)
        args = [c.q.data_ptr(), c.k.data_ptr(), c.vt.data_ptr(), out.data_ptr(), H, S, c.s_pad, out.stride(0), n_main, mode, bias, scale,
                pre, bound]
        if with_ws:
            rc = lib.rf_attention_fwd_ws(*args, ws.data_ptr(), ws.numel() * 4, ops.stream_ptr())
        else:
            rc = lib.rf_attention_fwd(*args, ops.stream_ptr())
        L.check(rc, "rf_attention_fwd")
        name = "rf_attention_fwd_ws" if with_ws else "rf_attention_fwd"
        assert lib.rf_debug_last_attn_path() == path, (name, lib.rf_debug_last_attn_path(), path)
        assert torch.isfinite(out.float()).all() and torch.equal(out, want), f"{name} H={H} S={S} mode {mode}: differs from rf_attention"
        print(f"  {name} H={H} S={S} mode {mode} bound {bound}: path {path}")
