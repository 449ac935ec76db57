"""The training kernels at the shapes where their dispatch branches, through the C ABI (include/rf_flux.h, "TRAINING path"; the ctypes
signatures of reflectionflow_amd/_lib.py), on caller memory that holds whatever the previous step left.

Window harness (`Win`, `Ctx`): every operand, output and scratch buffer is a window inside a larger parent of 16-bit words filled
with a pattern of tests/workspace_poison (zero / stale / extreme / nan); inputs then receive their data.  A 2-D window starts 64 rows
and 128 words into its parent and its row pitch is the parent's width (>= window + 256 words: always wider than the row); a buffer
the ABI takes without a pitch (q, k, v, the tiles, partials, ws, the flat optimizer tensors) is a contiguous window with 8192 words of
guard on either side.  Window starts stay 16-byte aligned.  Per kernel, case and pattern:
  (a) the window matches the fp64 reference of tests/train_kernel_cases.py within the bound stated there (test_train_kernels_cpu.py
      proves each bound reachable);  (b) it is bit-equal to the zero-pattern run;  (c) every word of every parent outside the
  windows the call may write is unchanged -- a row or column too far lands in allocated memory and is SEEN, nothing here depends on a
  fault -- and no input parent changed at all;  (d) the baseline is finite and not constant (windows of more than one element).
Promised zeros (rows >= S of q, k, v; the pad slots of vt, qt, kt; rows <= r < rows_pad of the transpose; the unowned parts of A_out /
Bs_out) are part of the bit-exact comparisons: all-zero bits under every pattern.

Which case reaches which branch (csrc/train_rowops.hip):
  ln_mod_bwd_kernel<1>   D 8 (one lane live), 264, 512          <2>  D 520 (last chunk 8 columns), 1024
  ln_mod_bwd_kernel<4>   D 1032 (nch 3: chunk 3 empty), 1536 (nch 3), 2048, and <6>: D 2056, 2560 (nch 5: chunk 5 empty), 3064, 3072
  ... its grid-stride loop: r2049_D1032, r2051_D1032 (512-block cap), r1025_D3072, r2051_D3072 (256-block cap); fewer rows than
  waves: r1 / r3 / r5; the prefetch of a row that does not exist: every rows % 4 != 0
  gate_bwd_kernel<1,2,4,6>: the same D set; its grid-stride loop: r2049_*, r4099_* (rows > 2048)
  colsum_reduce_kernel   nw < 4: rows 1 .. 13; the 16-way unrolled body (w + 12 < nw per row group j) in some groups and the tail loop
                         alone in the others: rows 49 / 53 / 61 / 64 (nw 13 .. 16); one turn of it everywhere: rows 65 (nw 17); nw 256 / 512;
                         out1 == out0 (gate), split (LayerNorm); not launched at all: d_scale / d_gate NULL (partials still written)
  gelu_kernel<false / true>, gate_res_kernel grid-stride loops: (1030, 8192), one block's worth of items past 4096 blocks
  transpose_vec_kernel / transpose_kernel: TRANSPOSE_CASES, every one with ld_dst > rows_pad (the harness has no other pitch)
  tn_skinny_kernel<1,2,4,8> x {plain, transposed} and every slice sequence of the 128 / 64 / 32 / 16 split: TN_R; partial 32-token
                         steps and chunk counts 1 .. 3: TN_S; a column tile that ends inside / at / past 128: TN_N
  lora_fuse_kernel / lora_unfuse_kernel: lora_cases() -- two entries in one 8-column group, r_pad > sum r, unowned N rows, two
                         adapters of one linear, 8 entries, NULL dA / dB, accumulate 0 / 1
  optimizer kernels      n = 8 (one access), 8184 / 8192 / 8200 / 24584: the last access of a block in, out, and the next block's first

rf_gate_residual with out aliasing res: the header does not say it may, and the kernel declares both __restrict__ -- so it is NOT part
of the contract and is not tested here (train/blocks.py never aliases them either)."""
import pytest
import torch

from tests import train_kernel_cases as TC
from tests.test_round5_gpu import _ulps_bf16
from tests.workspace_poison import PATTERNS, POISONS, assert_live, assert_same_bits, pattern_words

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GR, GC, GFLAT = 64, 128, 8192
RF_ERR_WORKSPACE = -6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Win:
    """rows x cols elements of `dtype` (bf16 or fp32) inside a pattern-filled parent of int16 words"""

    def __init__(self, dev, rows, cols, pad, kind, dtype=BF, flat=False, seed=0):
        self.w = 2 if dtype == F32 else 1
        gr, gc = (0, GFLAT) if flat else (GR, GC)
        assert not flat or rows == 1
        width = 2 * gc + (cols + pad) * self.w
        self.parent = pattern_words(kind, (rows + 2 * gr) * width, dev, seed).view(rows + 2 * gr, width)
        self.ld = width // self.w
        self.sl = (slice(gr, gr + rows), slice(gc // self.w, gc // self.w + cols))
        self.win = self.parent.view(dtype)[self.sl]
        self.ptr = self.win.data_ptr()
        self.before = None

    def put(self, data):
        self.win.copy_(data.reshape(self.win.shape).to(self.win.device))
        return self

    def arm(self):
        self.before = self.parent.clone()

    def get(self, shape=None):
        t = self.win.clone()
        return t if shape is None else t.reshape(shape)

    def check(self, what, written):
        """written: the call may have changed the window; everything else must be as armed"""
        cur = self.parent
        if written:
            cur = self.parent.clone()
            cur.view(self.win.dtype)[self.sl] = self.before.view(self.win.dtype)[self.sl]
        bad = int((cur != self.before).sum())
        assert bad == 0, f"{what}: {bad} words outside the window changed" if written else f"{what}: {bad} words of an input changed"


class Ctx:
    """the windows of one call under one pattern"""

    def __init__(self, dev, kind):
        self.dev, self.kind, self.wins = dev, kind, []

    def _new(self, written, name, *a, **kw):
        w = Win(self.dev, *a, kind=self.kind, seed=len(self.wins), **kw)
        self.wins.append((name, w, written))
        return w

    def inp(self, name, data, pad=8, flat=False):
        """an input window holding `data`"""
        dt = F32 if data.dtype == F32 else BF
        if flat:
            w = self._new(False, name, 1, data.numel(), pad, dtype=dt, flat=True)
        else:
            w = self._new(False, name, data.shape[0], data.shape[1], pad, dtype=dt)
        return w.put(data)

    def out(self, name, rows, cols, pad=8, dtype=BF, flat=False, init=None):
        w = self._new(True, name, rows, cols, pad, dtype=dtype, flat=flat)
        if init is not None:
            w.put(init)
        return w

    def arm(self):
        for _, w, _ in self.wins:
            w.arm()

    def done(self):
        torch.cuda.synchronize()
        for name, w, written in self.wins:
            w.check(f"{name} [{self.kind}]", written)


def _stream():
    from reflectionflow_amd import ops
    return ops.stream_ptr()


def _ok(rc, what):
    from reflectionflow_amd import _lib
    _lib.check(rc, what)


def run_patterns(make, live=()):
    """make(kind) -> {name: tensor}.  Every poisoned run bit-equal to the zero run, which is returned (on the CPU)."""
    outs = {kind: make(kind) for kind in PATTERNS}
    base = outs["zero"]
    for kind in POISONS:
        assert outs[kind].keys() == base.keys()
        for name, t in base.items():
            assert_same_bits(outs[kind][name], t, f"{name} [{kind}]")
    for name in live:
        if base[name].numel() > 1:
            assert_live(base[name], name)
    return {k: v.cpu() for k, v in base.items()}


def inside(got, ref, bound, what):
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: not finite"
    over = (g - ref).abs() - bound
    worst = float(((g - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"  {what}: worst |err| / bound {worst:.3f}")
    assert float(over.max()) <= 0.0, f"{what}: {int((over > 0).sum())} of {over.numel()} elements outside the bound (worst ratio {worst:.3f})"


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.dtype == BF:
        got, want = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} elements differ in bits"


# ------------------------------------------------------------------------------------------------------- LayerNorm-modulate backward
@pytest.mark.parametrize("case", TC.ln_cases(), ids=lambda c: c[0])
def test_layernorm_modulate_bwd(dev, case):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    _, rows, D, has_dres, dmod, pads, offset = case
    blocks = min((rows + 3) // 4, 256 if D > 2048 else 512)
    assert blocks * 2 * D * 4 <= lib.rf_train_partials_bytes(D)
    for exact in (False, True):
        x, dy, scale, dres = TC.ln_inputs(rows, D, offset, exact)
        dres = dres if has_dres else None
        ref = TC.ln_bwd_ref(x, dy, scale, dres)

        def run(kind):
            c = Ctx(dev, kind)
            wx, wdy, wsc = c.inp("x", x, pads[0]), c.inp("dy", dy, pads[1]), c.inp("scale", scale[None], 8)
            wdr = c.inp("dres", dres, pads[2]) if has_dres else None
            wdx = c.out("dx", rows, D, pads[3])
            wds, wdh = (c.out("d_scale", 1, D, 8, F32), c.out("d_shift", 1, D, 24, F32)) if dmod else (None, None)
            part = c.out("partials", 1, blocks * 2 * D, 0, F32, flat=True)
            c.arm()
            _ok(lib.rf_layernorm_modulate_bwd(wx.ptr, wx.ld, wdy.ptr, wdy.ld, wdr.ptr if wdr else None, wdr.ld if wdr else 0, wdx.ptr, wdx.ld,
                                              rows, D, wsc.ptr, TC.EPS, wds.ptr if dmod else None, wdh.ptr if dmod else None, part.ptr,
                                              blocks * 2 * D * 4, _stream()), "rf_layernorm_modulate_bwd")
            c.done()
            o = dict(dx=wdx.get())
            if dmod:
                o.update(d_scale=wds.get(), d_shift=wdh.get())
            return o
        base = run_patterns(run, live=("dx", "d_scale", "d_shift") if dmod else ("dx",))
        tag = f"{case[0]}{' exact' if exact else ''}"
        inside(base["dx"], ref["dx"], TC.bound_ln_dx(ref, D), f"dx {tag}")
        if dmod:
            inside(base["d_scale"][0], ref["d_scale"], TC.bound_colsum(rows, ref["scale_abs"]), f"d_scale {tag}")
            if exact:
                same(base["d_shift"][0].double(), ref["d_shift"], f"d_shift {tag} (integer sum)")
            else:
                inside(base["d_shift"][0], ref["d_shift"], TC.bound_colsum(rows, ref["shift_abs"]), f"d_shift {tag}")


# ------------------------------------------------------------------------------------------------------------------- gate backward
@pytest.mark.parametrize("case", TC.gate_cases(), ids=lambda c: c[0])
def test_gate_bwd(dev, case):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    _, rows, D, want, pads = case
    blocks = min((rows + 3) // 4, 512)
    need = blocks * D * 4
    for exact in (False, True):
        dy, f, gate = TC.gate_inputs(rows, D, exact)
        ref = TC.gate_bwd_ref(dy, f, gate)

        def run(kind):
            c = Ctx(dev, kind)
            wdy, wf, wg = c.inp("dy", dy, pads[0]), c.inp("f", f, pads[1]), c.inp("gate", gate[None], 8)
            wdf = c.out("df", rows, D, pads[2])
            wdg = c.out("d_gate", 1, D, 8, F32) if want else None
            part = c.out("partials", 1, blocks * D, 0, F32, flat=True)
            c.arm()
            args = (wdy.ptr, wdy.ld, wf.ptr, wf.ld, wg.ptr, wdf.ptr, wdf.ld, rows, D, wdg.ptr if want else None, part.ptr)
            assert lib.rf_gate_bwd(*args, need - 1, _stream()) == RF_ERR_WORKSPACE, "partials one byte short must be refused"
            _ok(lib.rf_gate_bwd(*args, need, _stream()), "rf_gate_bwd")
            c.done()
            o = dict(df=wdf.get())
            if want:
                o["d_gate"] = wdg.get()
            return o
        base = run_patterns(run, live=("df", "d_gate") if want else ("df",))
        tag = f"{case[0]}{' exact' if exact else ''}"
        inside(base["df"], ref["df"], TC.bound_elementwise(ref["df"]), f"df {tag}")
        if want:
            if exact:
                same(base["d_gate"][0].double(), ref["d_gate"], f"d_gate {tag} (integer sum)")
            else:
                inside(base["d_gate"][0], ref["d_gate"], TC.bound_colsum(rows, ref["gate_abs"]), f"d_gate {tag}")


# ------------------------------------------------------------------------------------------- GELU, GELU', gated residual (elementwise)
@pytest.mark.parametrize("rows,cols", TC.EW_SHAPES)
def test_gelu_gelu_bwd_gate_residual(dev, rows, cols):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    z, dh = TC.gelu_inputs(rows, cols)
    res, f, gate = TC.gate_inputs(rows, cols)
    ref = dict(h=TC.gelu(z.double()), dz=dh.double() * TC.gelu_grad(z.double()), y=TC.gate_fwd(f.double(), gate.double(), res.double()))

    def run(kind):
        c = Ctx(dev, kind)
        wz, wdh = c.inp("z", z, 24), c.inp("dh", dh, 64)
        wf, wg, wr = c.inp("f", f, 200), c.inp("gate", gate[None], 8), c.inp("res", res, 8)
        wh, wdz, wy = c.out("h", rows, cols, 64), c.out("dz", rows, cols, 8), c.out("y", rows, cols, 24)
        c.arm()
        _ok(lib.rf_gelu(wz.ptr, wz.ld, wh.ptr, wh.ld, rows, cols, _stream()), "rf_gelu")
        _ok(lib.rf_gelu_bwd(wz.ptr, wz.ld, wdh.ptr, wdh.ld, wdz.ptr, wdz.ld, rows, cols, _stream()), "rf_gelu_bwd")
        _ok(lib.rf_gate_residual(wf.ptr, wf.ld, wg.ptr, wr.ptr, wr.ld, wy.ptr, wy.ld, rows, cols, _stream()), "rf_gate_residual")
        c.done()
        return dict(h=wh.get(), dz=wdz.get(), y=wy.get())
    base = run_patterns(run, live=("h", "dz", "y"))
    for name in ("h", "dz", "y"):
        inside(base[name], ref[name], TC.bound_elementwise(ref[name]), f"{name} {rows}x{cols}")


# ----------------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("case", TC.TRANSPOSE_CASES, ids=lambda c: "{}_{}x{}_pad{}".format(*c[:4]))
def test_transpose(dev, case):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    path, rows, cols, rows_pad, extra, src_pad = case
    src = TC.rnd(TC.gen(91, rows, cols), rows, cols)
    ref = TC.transpose_ref(src, rows_pad)

    def run(kind):
        c = Ctx(dev, kind)
        ws, wd = c.inp("src", src, src_pad), c.out("dst", cols, rows_pad, extra)
        vec = ws.ptr % 16 == 0 and wd.ptr % 16 == 0 and ws.ld % 8 == 0 and wd.ld % 8 == 0 and cols % 8 == 0 and rows_pad % 8 == 0
        assert vec == (path == "vec") and wd.ld > rows_pad, (path, ws.ld, wd.ld)
        c.arm()
        _ok(lib.rf_transpose_bf16(ws.ptr, ws.ld, rows, cols, wd.ptr, wd.ld, rows_pad, _stream()), "rf_transpose_bf16")
        c.done()
        return dict(dst=wd.get())
    base = run_patterns(run, live=("dst",) if rows * cols > 1 else ())
    same(base["dst"], ref, "dst")


# ----------------------------------------------------------------------------------------------------------- token-axis skinny GEMM
@pytest.mark.parametrize("S,N,R", TC.tn_cases())
def test_gemm_tn_skinny(dev, S, N, R):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    need = int(lib.rf_gemm_tn_skinny_ws_bytes(S, N, R))
    assert need == (S + 127) // 128 * N * R * 4
    for exact in (False, True):
        big, sk = TC.tn_inputs(S, N, R, exact)
        ref = TC.tn_ref(big, sk)

        def run(kind):
            c = Ctx(dev, kind)
            wb, wk = c.inp("big", big, 24), c.inp("skinny", sk, 8)
            wo, wt = c.out("out", N, R, 8), c.out("out_t", R, N, 64)
            ws = c.out("ws", 1, need // 4, 0, F32, flat=True)
            c.arm()
            assert lib.rf_gemm_tn_skinny(wb.ptr, wb.ld, wk.ptr, wk.ld, wo.ptr, wo.ld, S, N, R, 0, ws.ptr, need - 1, _stream()) == RF_ERR_WORKSPACE
            _ok(lib.rf_gemm_tn_skinny(wb.ptr, wb.ld, wk.ptr, wk.ld, wo.ptr, wo.ld, S, N, R, 0, ws.ptr, need, _stream()), "rf_gemm_tn_skinny")
            _ok(lib.rf_gemm_tn_skinny(wb.ptr, wb.ld, wk.ptr, wk.ld, wt.ptr, wt.ld, S, N, R, 1, ws.ptr, need, _stream()), "rf_gemm_tn_skinny^T")
            c.done()
            return dict(out=wo.get(), out_t=wt.get())
        base = run_patterns(run, live=("out", "out_t"))
        same(base["out_t"].T.contiguous(), base["out"], "the two orientations")
        if exact:
            same(base["out"], ref["out"].to(BF), "out == bf16(exact integer sum)")
        else:
            inside(base["out"], ref["out"], TC.bound_tn(S, ref["out"], ref["abs"]), f"out S={S} N={N} R={R}")


# ------------------------------------------------------------------------------------------------- q|k|v -> attention operands, back
@pytest.mark.parametrize("case", TC.qkv_cases(), ids=lambda c: "h{}_S{}_a{}_p{}_l{}_b{}".format(*[int(v) for v in c]))
def test_qkv_train_fwd_bwd(dev, case):
    from reflectionflow_amd import _lib, ops
    lib = _lib.load()
    heads, S, n_added, sp_extra, ld_extra, bwd_ops = case
    D, s_pad, qs = heads * 128, (S + 63) // 64 * 64 + sp_extra, ops.QK_PRESCALE
    raw, w, cos, sin, (dq, dk, dv) = TC.qkv_inputs(heads, S)
    ref = TC.qkv_fwd_ref(raw, heads, n_added, w, cos, sin, qs)
    rb = TC.qkv_bwd_ref(raw, heads, n_added, w, cos, sin, qs, dq, dk, dv)
    hn = heads * s_pad * 128
    wn = w if n_added else (w[0], w[1], None, None)

    def run(kind):
        c = Ctx(dev, kind)
        # ld_raw == 3 D exactly is a contiguous buffer (no pitch to be wider); + 512 is a window of pitch 3 D + 512
        wraw = c.inp("raw", raw, ld_extra - 2 * GC) if ld_extra else c.inp("raw", raw, 0, flat=True)
        ld_raw = wraw.ld if ld_extra else 3 * D
        assert ld_raw == 3 * D + ld_extra
        ww = [c.inp(f"w{i}", t[None], 8) if t is not None else None for i, t in enumerate(wn)]
        wc, wsn = c.inp("cos", cos, 0, flat=True), c.inp("sin", sin, 0, flat=True)
        o = {n: c.out(n, 1, hn, 0, flat=True) for n in (("q", "k", "v", "vt", "qt", "kt") if bwd_ops else ("q", "k", "vt"))}
        # the gradients: rows >= S of dq / dk / dv keep the pattern -- the backward must not read them
        g = {}
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            g[n] = c.out(n, 1, hn, 0, flat=True)
            g[n].win.view(heads, s_pad, 128)[:, :S] = t.to(dev)
        wd = c.out("d_raw", S, 3 * D, 8 + ld_extra)
        c.arm()
        p = lambda x: x.ptr if x is not None else None   # noqa: E731
        common = (heads, S, s_pad, n_added, p(ww[0]), p(ww[1]), p(ww[2]), p(ww[3]), wc.ptr, wsn.ptr, TC.EPS, qs)
        _ok(lib.rf_qkv_train_fwd(wraw.ptr, ld_raw, *common, o["q"].ptr, o["k"].ptr, p(o.get("v")), o["vt"].ptr, p(o.get("qt")), p(o.get("kt")),
                                 _stream()), "rf_qkv_train_fwd")
        _ok(lib.rf_qkv_train_bwd(wraw.ptr, ld_raw, *common, g["dq"].ptr, g["dk"].ptr, g["dv"].ptr, wd.ptr, wd.ld, _stream()), "rf_qkv_train_bwd")
        torch.cuda.synchronize()
        for n in g:                               # (inputs held in writable windows: nothing of them may change)
            assert torch.equal(g[n].parent, g[n].before), f"{n} was written"
        c.done()
        out = {n: x.get((heads, s_pad, 128)) for n, x in o.items() if n in ("q", "k", "v")}
        out.update(vt=o["vt"].get((heads, s_pad // 64, 128, 64)), d_raw=wd.get())
        if bwd_ops:
            out.update(qt=o["qt"].get((heads, s_pad // 32, 128, 32)), kt=o["kt"].get((heads, s_pad // 32, 128, 32)))
        return out
    base = run_patterns(run, live=("q", "k", "d_raw"))
    for n in ("q", "k"):
        inside(base[n][:, :S], ref[n], TC.bound_qkv_fwd(ref[n], ref[n + "_mag"]), n)
        assert not base[n][:, S:].view(torch.int16).any(), f"{n}: rows >= S must be all-zero bits"
    v_full = TC.pad_rows(raw[:, 2 * D:].reshape(S, heads, 128).permute(1, 0, 2), s_pad)
    same(base["vt"], TC.vt_tiles(v_full), "vt (pad key columns zero)")
    if bwd_ops:
        same(base["v"], v_full, "v (rows >= S zero)")
        same(base["qt"], TC.t_tiles(base["q"]), "qt == the tiles of q (pad slots zero)")
        same(base["kt"], TC.t_tiles(base["k"]), "kt == the tiles of k (pad slots zero)")
    inside(base["d_raw"][:, :2 * D], rb["d_raw"][:, :2 * D], TC.bound_qkv_bwd(rb)[:, :2 * D], "d_raw q | k")
    same(base["d_raw"][:, 2 * D:], dv.permute(1, 0, 2).reshape(S, D), "d_raw v columns == dv")


# ------------------------------------------------------------------------------------------------------------ fused LoRA operands
def _lora_table(entries, A, B, dA, dB):
    from reflectionflow_amd import _lib
    tab = (_lib.rf_lora_fuse_entry * len(entries))()
    for i, (n0, n, r0, r, sc, wa, wb) in enumerate(entries):
        e = tab[i]
        e.A, e.B = (A[i].ptr if A else None), (B[i].ptr if B else None)
        e.dA, e.dB = (dA[i].ptr if dA and wa else None), (dB[i].ptr if dB and wb else None)
        e.n0, e.n, e.r0, e.r, e.scaling = n0, n, r0, r, sc
    return tab


@pytest.mark.parametrize("name", list(TC.lora_cases()))
def test_lora_fuse_unfuse(dev, name):
    from reflectionflow_amd import _lib
    lib = _lib.load()
    K, N, r_pad, entries = TC.lora_cases()[name]
    fac, g0, dA, dBs = TC.lora_inputs(name)
    A_ref, B_ref = TC.lora_fuse_ref(name, fac)

    def fuse(kind):
        c = Ctx(dev, kind)
        wa = [c.inp(f"A{i}", a, 0, flat=True) for i, (a, _) in enumerate(fac)]
        wb = [c.inp(f"B{i}", b, 0, flat=True) for i, (_, b) in enumerate(fac)]
        oa, ob = c.out("A_out", 1, r_pad * K, 0, flat=True), c.out("Bs_out", 1, N * r_pad, 0, flat=True)
        c.arm()
        _ok(lib.rf_lora_fuse(_lora_table(entries, wa, wb, None, None), len(entries), K, N, r_pad, oa.ptr, ob.ptr, _stream()), "rf_lora_fuse")
        c.done()
        return dict(A=oa.get((r_pad, K)), Bs=ob.get((N, r_pad)))
    base = run_patterns(fuse, live=("A", "Bs"))
    same(base["A"], A_ref, "A_out (unowned rows zero)")
    same(base["Bs"], B_ref, "Bs_out == bf16(scaling * B), zero elsewhere")
    for acc in (0, 1):
        want = TC.lora_unfuse_ref(name, g0, dA, dBs, acc)

        def unfuse(kind):
            c = Ctx(dev, kind)
            wda, wdb = c.inp("dA", dA, 0, flat=True), c.inp("dBs", dBs, 0, flat=True)
            # accumulate = 1 adds into what the factor gradients hold; accumulate = 0 must not depend on it: they keep the pattern
            oa = [c.out(f"dA{i}", 1, a.numel(), 0, flat=True, init=a if acc else None) for i, (a, _) in enumerate(g0)]
            ob = [c.out(f"dB{i}", 1, b.numel(), 0, flat=True, init=b if acc else None) for i, (_, b) in enumerate(g0)]
            c.arm()
            _ok(lib.rf_lora_unfuse_grads(_lora_table(entries, None, None, oa, ob), len(entries), K, N, r_pad, wda.ptr, wdb.ptr, acc, _stream()),
                "rf_lora_unfuse_grads")
            c.done()
            out = {}
            for i, (n0, n, r0, r, sc, wa_, wb_) in enumerate(entries):
                if wa_:
                    out[f"dA{i}"] = oa[i].get((r, K))
                if wb_:
                    out[f"dB{i}"] = ob[i].get((n, r))
            return out
        got = run_patterns(unfuse, live=[f"dA{i}" for i, e in enumerate(entries) if e[5]])
        for i, (n0, n, r0, r, sc, wa_, wb_) in enumerate(entries):
            if wa_:
                same(got[f"dA{i}"], want[i][0], f"dA{i} accumulate={acc}")
            if wb_:
                same(got[f"dB{i}"], want[i][1], f"dB{i} accumulate={acc}")


# ------------------------------------------------------------------------------------------------------------------- the optimizers
def _state(c, name, t, fp32):
    return c.out(name, 1, t.numel(), 0, F32 if fp32 else BF, flat=True, init=t.float() if fp32 else t)


def _state_close(got, want, fp32, what):
    """the existing criteria: bf16 state within one bf16 ulp of the fp32 oracle's, fp32 state to 2e-6 of its largest magnitude"""
    if fp32:
        assert float((got[0] - want).abs().max()) <= 2e-6 * float(want.abs().max()), what
    else:
        assert _ulps_bf16(got[0], want.to(BF)) <= 1.0, what


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16_state", "fp32_state"])
@pytest.mark.parametrize("n", TC.OPT_N)
def test_adamw_and_sgd(dev, n, fp32):
    from oracle import optim_oracle as OO
    from reflectionflow_amd import _lib
    lib = _lib.load()
    p, g, m, v, _ = TC.opt_inputs(n)
    kw = dict(lr=2e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.05)
    rp, rm, rv = p.float().clone(), m.float().clone(), v.float().clone()
    OO.adamw_step(rp, g.float(), rm, rv, 3, **kw)
    sg = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01)
    # rf_lora_sgd's criteria are those of tests/test_sgd_gpu.py: bf16 state against torch.optim.SGD itself on the same tensors (its
    # single-tensor form, started from a momentum buffer so that the step is not the first), fp32 state against the formula in fp32
    if fp32:
        r, gd = p.to(dev).float(), g.to(dev).float()
        gg = (gd + sg["weight_decay"] * r).to(BF).float()                  # torch rounds the decayed gradient to the tensors' dtype
        sbuf = m.to(dev).float() * sg["momentum"] + (1 - sg["dampening"]) * gg
        sp, sbuf = (r - sg["lr"] * sbuf).to(BF).cpu(), sbuf.cpu()
    else:
        pt = torch.nn.Parameter(p.to(dev))
        pt.grad = g.to(dev)
        topt = torch.optim.SGD([pt], foreach=False, **sg)
        topt.state[pt]["momentum_buffer"] = m.to(dev).clone()
        topt.step()
        sp, sbuf = pt.detach().cpu(), topt.state[pt]["momentum_buffer"].cpu()

    def run(kind):
        c = Ctx(dev, kind)
        wg = c.inp("grad", g, 0, flat=True)
        wp, wm, wv = c.out("param", 1, n, 0, flat=True, init=p), _state(c, "exp_avg", m, fp32), _state(c, "exp_avg_sq", v, fp32)
        wp2, wb = c.out("param_sgd", 1, n, 0, flat=True, init=p), _state(c, "momentum_buffer", m, fp32)
        c.arm()
        _ok(lib.rf_lora_adamw(wp.ptr, wg.ptr, wm.ptr, wv.ptr, n, int(fp32), 3, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], kw["weight_decay"],
                              1.0, _stream()), "rf_lora_adamw")
        _ok(lib.rf_lora_sgd(wp2.ptr, wg.ptr, wb.ptr, n, int(fp32), 2, sg["lr"], sg["momentum"], sg["dampening"], sg["weight_decay"], 0, 0, 1.0,
                            _stream()), "rf_lora_sgd")
        c.done()
        return dict(p=wp.get(), m=wm.get(), v=wv.get(), p_sgd=wp2.get(), buf=wb.get())
    base = run_patterns(run, live=("p", "m", "v", "p_sgd", "buf"))
    assert _ulps_bf16(base["p"][0], rp.to(BF)) <= 1.0
    _state_close(base["m"], rm, fp32, "exp_avg")
    _state_close(base["v"], rv, fp32, "exp_avg_sq")
    print(f"  rf_lora_sgd n={n} fp32={fp32}: {_ulps_bf16(base['p_sgd'][0], sp):.2f} bf16 ulp")
    assert _ulps_bf16(base["p_sgd"][0], sp) <= 1.0
    _state_close(base["buf"], sbuf.float(), fp32, "momentum_buffer")


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16_state", "fp32_state"])
@pytest.mark.parametrize("n", TC.OPT_N)
def test_prodigy_and_clip(dev, n, fp32):
    from oracle import optim_oracle as OO
    from reflectionflow_amd import _lib
    lib = _lib.load()
    p, g, m, v, s = TC.opt_inputs(n, seed=1)
    p0 = (p.float() + TC.rnd(TC.gen(82, n), n, sc=0.02).float()).to(BF)
    kw = dict(lr=1.0, use_bias_correction=True, safeguard_warmup=True, weight_decay=0.01)
    d0, d = 1e-6, 1e-4
    x = p.float().clone()
    st = dict(m=m.float().clone(), v=v.float().clone(), s=s.float().clone(), p0=p0.float(), d=d, d0=d0, d_max=d, d_numerator=1e-7, d_denom=0.0,
              d_hat=d, k=3)
    OO.prodigy_step(x, g.float(), st, **kw)
    pb = int(lib.rf_lora_prodigy_partials_bytes(n))
    blocks = (n + 8191) // 8192
    assert pb == blocks * 8
    # clipping: total_norm = || grad_scale * grad ||, coef = min(1, max_norm / (total_norm + 1e-6))
    gs, mx = 0.5, 0.5 * float((g.double() * 0.5).norm())           # the limit at half the norm: the gradients are scaled
    norm64 = float((g.double() * gs).norm())
    coef = min(1.0, mx / (norm64 + 1e-6))

    def run(kind):
        c = Ctx(dev, kind)
        wg, w0 = c.inp("grad", g, 0, flat=True), c.inp("p0", p0, 0, flat=True)
        wp = c.out("param", 1, n, 0, flat=True, init=p)
        wm, wv, ws = _state(c, "exp_avg", m, fp32), _state(c, "exp_avg_sq", v, fp32), _state(c, "s", s, fp32)
        part = c.out("partials", 1, pb // 4, 0, F32, flat=True)
        wcg = c.out("clip_grad", 1, n, 0, flat=True, init=g)
        cpart = c.out("clip_partials", 1, blocks, 0, F32, flat=True)
        cout = c.out("clip_out", 1, 2, 2, F32, flat=True)
        dstate = torch.tensor([d, d, 1e-7, 0.0, d, 3.0, 0.0, d0], dtype=F64, device=dev)
        c.arm()
        _ok(lib.rf_lora_prodigy(wp.ptr, wg.ptr, wm.ptr, wv.ptr, ws.ptr, w0.ptr, n, int(fp32), dstate.data_ptr(), 1.0, 0.9, 0.999, 0.0, 1e-8, 0.01, 1,
                                1, 1, 1.0, 3.0e38, 1.0, part.ptr, pb, _stream()), "rf_lora_prodigy")
        assert lib.rf_lora_clip_grad_norm(wcg.ptr, n, mx, gs, cpart.ptr, blocks * 4 - 1, cout.ptr, _stream()) == RF_ERR_WORKSPACE
        _ok(lib.rf_lora_clip_grad_norm(wcg.ptr, n, mx, gs, cpart.ptr, blocks * 4, cout.ptr, _stream()), "rf_lora_clip_grad_norm")
        c.done()
        return dict(p=wp.get(), m=wm.get(), v=wv.get(), s=ws.get(), dstate=dstate.float(), clip=wcg.get(), clip_out=cout.get(), dstate64=dstate.clone().view(torch.int16))
    base = run_patterns(run, live=("p", "m", "v", "s", "clip"))
    ds = base["dstate64"].view(F64).tolist()
    got = dict(d=ds[0], d_max=ds[1], d_numerator=ds[2], d_denom=ds[3], d_hat=ds[4], k=int(ds[5]))
    for key, tol in (("d_denom", 1e-5), ("d_numerator", 1e-4), ("d_hat", 1e-4), ("d", 1e-4)):
        assert abs(got[key] - st[key]) <= tol * abs(st[key]) + 1e-30, (key, got[key], st[key])
    assert got["k"] == st["k"] == 4
    assert _ulps_bf16(base["p"][0], x.to(BF)) <= 1.0
    _state_close(base["m"], st["m"], fp32, "exp_avg")
    _state_close(base["v"], st["v"], fp32, "exp_avg_sq")
    _state_close(base["s"], st["s"], fp32, "s")
    assert abs(float(base["clip_out"][0, 0]) - norm64) <= 1e-6 * norm64 and abs(float(base["clip_out"][0, 1]) - coef) <= 2e-6 * coef
    assert coef < 1.0 and _ulps_bf16(base["clip"][0], (g.float() * coef).to(BF)) <= 1.0
