"""Cases, inputs and checkers of the forward-attention parity tests (importable without a GPU).

Three kinds of input for the same launches:
  random    i.i.d. Gaussian q, k, v: the numbers against an fp64 softmax.
  selector  every query row attends to exactly ONE key (score 96 against <= 45 elsewhere) whose value row is an integer code of
            (head, key): the output row must BE that code, so a wrong row says which key, which head or which column it took.
  census    q = 0: every P is exactly 1, and key tile t's value rows are (head + 1) in the columns d % (S / 64) == t and 0 elsewhere:
            every output element is 64 (head + 1) / S, and a tile that was dropped or counted twice moves its own columns.
Every launch uses a prescaled q, so each kernel form sees the same operands.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from reflectionflow_amd import _lib as L

BF = torch.bfloat16


# ------------------------------------------------------------------------ shared with test_kernels_gpu / test_round3_gpu
def rnd(*shape, dev, scale=1.0, seed=None):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed if seed is not None else (hash(shape) % 100000))
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(BF)


def assert_close(got, ref, what, rtol=1.2e-2, atol=None):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    if atol is None:
        atol = 1.2e-2 * float(ref.abs().mean()) + 1e-6
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    rel_l2 = float((got - ref).norm() / (ref.norm() + 1e-12))
    if bad.any():
        idx = torch.nonzero(bad)[:8].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements off, max err {float(err.max()):.4g}, "
                             f"rel-L2 {rel_l2:.3e}, first bad idx {idx}, got {got[bad][:4].tolist()} ref {ref[bad][:4].tolist()}")
    assert rel_l2 < 4e-3, f"{what}: rel-L2 {rel_l2:.3e}"
    return rel_l2


def vt_position(kv):
    """where key kv of a head is stored in V^T: bits 2 and 3 of the index inside its 64-key tile are swapped"""
    return (kv & ~63) | (kv & 51) | ((kv & 4) << 1) | ((kv & 8) >> 1)


def vt_pack(vf, s_pad, pad_fill=0.0):
    """plain v [H, S, 128] -> key-permuted V^T tiles [H, s_pad/64, 128, 64].  The pad key columns of a partial last tile are zero
    (the kernels read them); whole tiles behind it hold `pad_fill`."""
    H, S = vf.shape[0], vf.shape[1]
    vpad = torch.full((H, s_pad, 128), pad_fill, device=vf.device, dtype=BF)
    vpad[:, :(S + 63) // 64 * 64] = 0
    vpad[:, :S] = vf
    vperm = torch.empty_like(vpad)
    vperm[:, vt_position(torch.arange(s_pad, device=vf.device))] = vpad      # permuted position <- key
    return vperm.reshape(H, s_pad // 64, 64, 128).permute(0, 1, 3, 2).contiguous()


def vt_unpermute(vt, S):
    """[H, S_pad/64, 128, 64] key-permuted V^T tiles -> [H, S, 128]."""
    H, nt = vt.shape[0], vt.shape[1]
    kv = torch.arange(64, device=vt.device)
    pos = (kv & 51) | ((kv & 4) << 1) | ((kv & 8) >> 1)
    v = vt[:, :, :, pos]                      # [H, nt, 128, 64(kv)]
    return v.permute(0, 1, 3, 2).reshape(H, nt * 64, 128)[:, :S]


def make_qkv(H, S, dev, seed=0, qscale=1.0):
    from reflectionflow_amd import ops
    q, k, vt, s_pad = ops.alloc_attn_operands(H, S, dev)
    qf = rnd(H, S, 128, dev=dev, seed=seed + 1, scale=qscale)
    kf = rnd(H, S, 128, dev=dev, seed=seed + 2)
    vf = rnd(H, S, 128, dev=dev, seed=seed + 3)
    q[:, :S], k[:, :S] = qf, kf
    vt.copy_(vt_pack(vf, s_pad))
    return q, k, vt, qf, kf, vf


def softmax_ref64(qp, kf, vf):
    """fp64 softmax(q k^T) v in the exp2 domain (q already carries scale * log2 e): [H,S,128] x3 -> [S, H*128] fp32."""
    s = torch.einsum("hqd,hkd->hqk", qp.double(), kf.double())
    s = s - s.amax(dim=-1, keepdim=True)
    p = torch.exp2(s)
    o = torch.einsum("hqk,hkd->hqd", p / p.sum(-1, keepdim=True), vf.double())
    return o.permute(1, 0, 2).reshape(qp.shape[1], -1).float()


def prescaled(H, S, dev, seed, qscale=1.0):
    from reflectionflow_amd import ops
    q, k, vt, qf, kf, vf = make_qkv(H, S, dev, seed=seed, qscale=qscale)
    qp = (qf.float() * ops.QK_PRESCALE).to(BF)
    q[:, :S] = qp
    return q, k, vt, qp, kf, vf


def ref64_chunked(qp, kf, vf, chunk=8):
    """softmax_ref64, `chunk` heads at a time (the fp64 score block of 64 heads does not have to exist at once)"""
    H = qp.shape[0]
    return torch.cat([softmax_ref64(qp[h:h + chunk], kf[h:h + chunk], vf[h:h + chunk]) for h in range(0, H, chunk)], dim=1)


def lse_ref64(qp, kf, chunk=8):
    """fp64 log2 sum_k exp2(q . k) of every query row: [H, S]"""
    out = []
    for h in range(0, qp.shape[0], chunk):
        s = torch.einsum("hqd,hkd->hqk", qp[h:h + chunk].double(), kf[h:h + chunk].double())
        m = s.amax(-1)
        out.append(m + torch.log2(torch.exp2(s - m[..., None]).sum(-1)))
    return torch.cat(out)


def rel_l2(got, ref):
    return float((got.float() - ref.float()).norm() / (ref.float().norm() + 1e-12))


# ------------------------------------------------------------------------------------------------------------ the forms
Form = namedtuple("Form", "name kernel path bounded lagged mix split")


def _F(name, path, **kw):
    return Form(name, getattr(L, "RF_ATTN_" + name), path, *(kw.get(f, False) for f in ("bounded", "lagged", "mix", "split")))


ONLINE128, ONLINE256 = _F("ONLINE128", 1), _F("ONLINE256", 2)
BOUNDED32, BOUNDED16 = _F("BOUNDED32", 4, bounded=True), _F("BOUNDED16", 5, bounded=True)
LAGGED16 = _F("LAGGED16", 8, lagged=True)
BOUNDED16_MIX, LAGGED16_MIX = _F("BOUNDED16_MIX", 10, bounded=True, mix=True), _F("LAGGED16_MIX", 11, lagged=True, mix=True)
BOUNDED16_SPLIT = _F("BOUNDED16_SPLIT", 6, bounded=True, split=True)
LAGGED16_SPLIT = _F("LAGGED16_SPLIT", 9, lagged=True, split=True)
FORMS = (ONLINE128, ONLINE256, BOUNDED32, BOUNDED16, LAGGED16, BOUNDED16_MIX, LAGGED16_MIX)
SPLIT_FORMS = (BOUNDED16_SPLIT, LAGGED16_SPLIT)
# the plain launch whose rows a mixed-size or split launch recomputes
PLAIN_OF = {"BOUNDED16_MIX": "BOUNDED16", "LAGGED16_MIX": "LAGGED16", "BOUNDED16_SPLIT": "BOUNDED16", "LAGGED16_SPLIT": "LAGGED16"}


def split_qualifies(heads, S, cus):
    """the split launch's own precondition: at least two key quads per persistent workgroup of an XCD (P = CUs in whole XCD rows)"""
    P = cus // 8 * 8
    return S % 256 == 0 and heads % 8 == 0 and P >= 8 and (heads // 8) * (S // 256) ** 2 >= 2 * (P // 8)


def form_runs(form, heads, S, cus):
    """whether an explicit request for `form` (mode 0, prescaled q, a proven bound where the form needs one, scratch attached
    where heads % 8 == 0) must run at (heads, S) on a part with `cus` CUs.  True: an RFError is a failure.  False: it must raise."""
    if form.split:
        return split_qualifies(heads, S, cus)
    if form.bounded or form.lagged:
        return S % 256 == 0                      # whole rounds of the 4-slot ring
    return True


# ------------------------------------------------------------------------------------------------------------ case lists
SWEEP_H = 3                                      # not a multiple of 8: head = block % heads is exercised
RING_SWEEP = (256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304)          # ring rounds 1 .. 9
SPLIT_SHAPES = ((8, 2048), (16, 1536), (24, 1280), (32, 1024), (64, 768), (8, 2304))
ALL_SMALL = {768: 4, 1536: 8, 2304: 12}          # plans with no 256-query workgroup at all


def mix_plans(S):
    """every legal rf_attn_desc.mix_small at S: b in {0, 4, 8, ...} with 12 b <= S / 16 (0 = the library's own plan)"""
    return tuple(range(0, (S // 16) // 12 + 1, 4))


def mix_sizes(S, b):
    """(256-query, 192-query) workgroups per head of the forced plan b"""
    return (S // 16 - 12 * b) // 16, b


def launches(forms, S):
    """(label, form, mix_small) of every launch of a case: the MIX forms once per legal plan"""
    out = []
    for f in forms:
        if f.mix:
            out += [(f"{f.name}[{b}]", f, b) for b in mix_plans(S)]
        else:
            out.append((f.name, f, 0))
    return out


# -------------------------------------------------------------------------------------------------------- input builders
Operands = namedtuple("Operands", "q k vt qp kf vf S s_pad")


def pack_operands(qp, kf, vf, s_pad=None, pad_fill=0.0):
    """plain [H, S, 128] q / k / v -> the product layout at s_pad >= S rows per head; q / k rows >= S and the V^T tiles behind
    the last (partial) one hold `pad_fill`"""
    H, S = qp.shape[0], qp.shape[1]
    s_pad = (S + 63) // 64 * 64 if s_pad is None else s_pad
    assert s_pad >= S and s_pad % 64 == 0
    q = torch.full((H, s_pad, 128), pad_fill, device=qp.device, dtype=BF)
    k = torch.full((H, s_pad, 128), pad_fill, device=qp.device, dtype=BF)
    q[:, :S], k[:, :S] = qp, kf
    return Operands(q, k, vt_pack(vf, s_pad, pad_fill), qp, kf, vf, S, s_pad)


def build_random(H, S, dev, seed, s_pad=None, pad_fill=0.0):
    """what prescaled() builds, at any s_pad"""
    q, k, vt, qp, kf, vf = prescaled(H, S, dev, seed)
    if s_pad in (None, q.shape[1]) and pad_fill == 0.0:
        return Operands(q, k, vt, qp, kf, vf, S, q.shape[1])
    return pack_operands(qp, kf, vf, s_pad, pad_fill)


SELECTOR_BOUND = 100.0                            # |s| <= 0.75 * 128 = 96: proven


def selector_pi(h, S):
    """the key query row i of head h attends to: a permutation of the keys (73 is coprime to every S used)"""
    return (73 * torch.arange(S) + 131 * (h + 1)) % S


def selector_values(H, S):
    """v[h, j, d] = ((j (d + 1) + h) % 251) + 1: integers in [1, 251], exact in bf16; rows differ unless j = j' (mod 251), h = h'"""
    h = torch.arange(H)[:, None, None]
    j = torch.arange(S)[None, :, None]
    d = torch.arange(128)[None, None, :]
    return (((j * (d + 1) + h) % 251) + 1).to(BF)


def selector_seed(H, S):
    return 1000 * H + S


def build_selector(H, S, dev, seed=None, s_pad=None, pad_fill=0.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(selector_seed(H, S) if seed is None else seed)
    kf = (torch.randint(0, 2, (H, S, 128), generator=g) * 2 - 1).to(BF)       # +-1
    qp = torch.stack([0.75 * kf[h, selector_pi(h, S)] for h in range(H)])      # exact: the matching score is 0.75 * 128 = 96
    return pack_operands(qp.to(dev), kf.to(dev), selector_values(H, S).to(dev), s_pad, pad_fill)


def selector_expected(H, S, dev="cpu"):
    """[S, H*128]: row i of head h is v[h, pi_h(i)]"""
    v = selector_values(H, S)
    return torch.stack([v[h, selector_pi(h, S)] for h in range(H)], 1).reshape(S, H * 128).float().to(dev)


def census_values(H, S):
    nt = S // 64
    j = torch.arange(S)[None, :, None]
    d = torch.arange(128)[None, None, :]
    return ((j // 64 == d % nt) * (torch.arange(H)[:, None, None] + 1)).to(BF)


def build_census(H, S, dev, seed=0, s_pad=None, pad_fill=0.0):
    assert S % 64 == 0 and S // 64 <= 128
    kf = rnd(H, S, 128, dev="cpu", seed=seed + 2)
    qp = torch.zeros(H, S, 128, dtype=BF)
    return pack_operands(qp.to(dev), kf.to(dev), census_values(H, S).to(dev), s_pad, pad_fill)


def census_expected(H, S, dev="cpu"):
    """[S, H*128] fp32: every element of head h is 64 (h + 1) / S"""
    return ((torch.arange(H, dtype=torch.float64) + 1) * 64 / S).float().repeat_interleave(128)[None].expand(S, -1).to(dev)


# -------------------------------------------------------------------------------------------------------------- checkers
SELECTOR_TOL = 1.0 / 64
CENSUS_RTOL = 2.0 ** -7                          # one bf16 ulp: the kernels compute O * (1 / l) in fp32 and round once
LSE_BOUND = math.log2(1.0 + 2.0 ** -8) + 1e-3    # bf16-rounded P summed on the matrix pipe + the fp32 score chains and v_log_f32


def _selector_diagnosis(row, i, h, H, S):
    """what the 128 values of output row i, head slot h, are instead of v[h, pi_h(i)]"""
    v = selector_values(H, S).float()
    want = int(selector_pi(h, S)[i])
    hit = [(int(a), int(b)) for a, b in ((v - row[None, None, :]).abs().amax(-1) < SELECTOR_TOL).nonzero()]
    if hit:
        pi = selector_pi(h, S)
        same = [j for h2, j in hit if h2 == h]               # (keys j and j + 251 of a head carry the same code)
        if not same:
            h2, j = hit[0]
            msg = f"the row carries key {j} of head {h2} (expected key {want} of head {h})"
            if any(j2 == int(selector_pi(h2, S)[i]) for hh, j2 in hit if hh == h2):
                msg += f": this is head {h2}'s own row written at head {h} (head offset)"
            return msg
        swapped = int(vt_position(torch.tensor(want)))
        if swapped in same:
            return f"the row carries key {swapped} (expected key {want} of head {h}): bits 2 and 3 of the key index are swapped (V^T key permutation)"
        tiled = [j for j in same if (j - want) % 64 == 0]
        if tiled:
            return (f"the row carries key {tiled[0]} (expected key {want} of head {h}): K tile {want // 64} was paired with "
                    f"V^T tile {tiled[0] // 64}")
        rows = [i2 for i2 in range(i // 16 * 16, i // 16 * 16 + 16) if int(pi[i2]) in same]
        if rows:
            return (f"the row carries key {int(pi[rows[0]])} (expected key {want} of head {h}): that is the key of query row {rows[0]} "
                    "of the same 16-row q-tile (query rows exchanged)")
        return f"the row carries key {same[0]} (expected key {want} of head {h})"
    # the right row with its 16-column d tiles in another order?
    rt, wt = row.view(8, 16), v[h, want].view(8, 16)
    src = [next((b for b in range(8) if (rt[a] - wt[b]).abs().max() < SELECTOR_TOL), None) for a in range(8)]
    if all(s is not None for s in src):
        moved = [(a, s) for a, s in enumerate(src) if s != a]
        return "the row is the expected one with d tiles moved: " + ", ".join(f"d tile {a} holds d tile {s}" for a, s in moved)
    return f"the row carries no key's code (expected key {want} of head {h})"


def check_selector(out, H, S, what):
    """max |out - v[pi]| < 1/64 (a condition: the fp64 output is within 2^-12 of an integer in [1, 251], which bf16 holds exactly)"""
    got = out.float()
    exp = selector_expected(H, S, got.device)
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)}"
    bad = ~((got - exp).abs() < SELECTOR_TOL)                                   # (NaN is bad)
    if bad.any():
        i, c = (int(x) for x in bad.nonzero()[0])
        h, d = c // 128, c % 128
        row = got[i, h * 128:(h + 1) * 128].cpu()
        raise AssertionError(f"{what}: {int(bad.sum())} elements off; first bad (row {i}, head {h}, column {d}): got {float(got[i, c])} "
                             f"expected {float(exp[i, c])}; " + _selector_diagnosis(row, i, h, H, S))


def check_census(out, H, S, what):
    """|out - 64 (h + 1) / S| <= 2^-7 of it, everywhere"""
    got = out.float()
    exp = census_expected(H, S, got.device)
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)}"
    bad = ~((got - exp).abs() <= CENSUS_RTOL * exp)
    if not bad.any():
        return
    nt = S // 64
    i, c = (int(x) for x in bad.nonzero()[0])
    lines = []
    for h in range(H):
        if not bad[:, h * 128:(h + 1) * 128].any():
            continue
        ratio = (got[:, h * 128:(h + 1) * 128] / exp[:, h * 128:(h + 1) * 128]).cpu()       # [S, 128]: c_t * S / l in tile t's columns
        tile_of = torch.arange(128) % nt
        rows = bad[:, h * 128:(h + 1) * 128].any(1).cpu()
        f = torch.stack([ratio[rows][:, tile_of == t].median() for t in range(nt)])         # factor of every tile, over the bad rows
        if not torch.isfinite(f).all():
            lines.append(f"head {h}: non-finite output")
            continue
        base = float(f.median())
        off = [t for t in range(nt) if not abs(float(f[t]) - base) <= 2 * CENSUS_RTOL * abs(base)]
        if off and base > 0:
            lines.append(f"head {h}, query rows {int(rows.nonzero()[0])}..{int(rows.nonzero()[-1])}: " + ", ".join(
                f"key tile {t} counted {float(f[t]) / base:.2f}x (its columns are off by the factor {float(f[t]):.4f})" for t in off[:8]))
        else:
            hint = ""
            hv = base * (h + 1)
            if abs(hv - round(hv)) < 0.02 and round(hv) != h + 1 and 1 <= round(hv) <= H:
                hint = f": that is the value of head {round(hv) - 1}"
            lines.append(f"head {h}: every key tile off by the factor {base:.4f}" + hint)
        if len(lines) == 4:
            break
    raise AssertionError(f"{what}: {int(bad.sum())} elements off; first bad (row {i}, head {c // 128}, column {c % 128}): got "
                         f"{float(got[i, c])} expected {float(exp[i, c])}; " + "; ".join(lines))


def check_lse(lse, ref, S, what):
    """lse [H, s_pad] fp32 of a launch against the fp64 log2-sum-exp2 [H, S]; returns the observed maximum"""
    err = float((lse[:, :S].double() - ref).abs().max())
    print(f"  lse {what}: max |lse - fp64| = {err:.3e} log2 units (bound {LSE_BOUND:.3e})")
    assert err <= LSE_BOUND, f"{what}: lse off by {err:.3e} log2 units > {LSE_BOUND:.3e}"
    return err
