"""The yardsticks of tests/test_train_kernels_edges_gpu.py, proved before any kernel is judged by them (no GPU):

  reference vs autograd   the hand-written fp64 backward formulas of tests/train_kernel_cases.py equal fp64 torch autograd of the same
                          map to 1e-12 relative (LayerNorm-modulate, gate, GELU and GELU', q|k|v -> operands and back);
  reference alone         for EVERY case of the GPU file, the same formula in fp32 with the kernels' one bf16 rounding stays inside
                          the acceptance bound against fp64: a correct kernel can reach the bound.  No case needed other inputs or
                          a further term.  One restatement had to change its FORM: GELU' written with tanh misses the
                          elementwise bound in fp32 for z << 0 (1 + t and 1 - t^2 cancel), so the fp32 side evaluates the
                          identical sigmoid form the kernel uses (train_kernel_cases.gelu_sig); the fp64 reference and every
                          bound stay as stated.  q / k and d_raw, whose bound is left open, get u |ref| + 4 gamma(128) A with
                          A the magnitudes of the terms of the last sum, as dx does;
  exact arithmetic        the integer cases: every partial sum is below 2^24, so an fp32 sum in any order is exact and the expected
                          value is the integer (d_shift, d_gate) or one bf16 rounding of it (rf_gemm_tn_skinny);
  index maps              the tile packers against a direct loop over the header's slot formulas."""
import pytest
import torch

from tests import train_kernel_cases as TC

BF, F64, F32 = TC.BF, TC.F64, TC.F32


def _close(a, b, what, tol=1e-12):
    err = float((a - b).abs().max())
    assert err <= tol * max(float(b.abs().max()), 1e-300), f"{what}: {err:.3e} vs max {float(b.abs().max()):.3e}"


def _inside(got, ref, bound, what):
    over = (got.double() - ref).abs() - bound
    assert float(over.max()) <= 0.0, f"{what}: fp32 restatement exceeds the bound by {float(over.max()):.3e} ({int((over > 0).sum())} elements)"


# ---------------------------------------------------------------------------------------------------------- reference vs fp64 autograd
@pytest.mark.parametrize("rows,D,offset", [(5, 8, 0.0), (13, 264, 0.0), (4, 1032, 0.0), (17, 520, 8.0)])
def test_ln_bwd_reference_equals_autograd(rows, D, offset):
    x, dy, scale, dres = TC.ln_inputs(rows, D, offset)
    x64, sc64 = x.double().requires_grad_(True), scale.double().requires_grad_(True)
    sh64 = torch.zeros(D, dtype=F64, requires_grad=True)
    (TC.ln_fwd(x64, sc64, sh64) * dy.double()).sum().backward()
    ref = TC.ln_bwd_ref(x, dy, scale, dres)
    _close(ref["dx"], x64.grad + dres.double(), "dx")
    _close(ref["d_scale"], sc64.grad, "d_scale")
    _close(ref["d_shift"], sh64.grad, "d_shift")
    _close(TC.ln_bwd_ref(x, dy, scale, None)["dx"], x64.grad, "dx without dres")


def test_gate_and_gelu_references_equal_autograd():
    dy, f, gate = TC.gate_inputs(13, 264)
    f64, g64 = f.double().requires_grad_(True), gate.double().requires_grad_(True)
    (TC.gate_fwd(f64, g64, torch.zeros(13, 264, dtype=F64)) * dy.double()).sum().backward()
    ref = TC.gate_bwd_ref(dy, f, gate)
    _close(ref["df"], f64.grad, "df")
    _close(ref["d_gate"], g64.grad, "d_gate")
    z, _ = TC.gelu_inputs(77, 512)
    z64 = z.double().requires_grad_(True)
    h = TC.gelu(z64)
    _close(h.detach(), torch.nn.functional.gelu(z.double(), approximate="tanh"), "gelu vs torch's gelu_tanh")
    h.sum().backward()
    _close(TC.gelu_grad(z.double()), z64.grad, "gelu'")
    gz = TC.gelu_grad(z.double())
    _close(TC.gelu_sig(z.double()), h.detach(), "gelu, sigmoid form")
    _close(TC.gelu_grad_sig(z.double()), gz, "gelu', sigmoid form")
    assert bool((gz < 0).any()) and bool((gz > 0).any()) and bool((z == 30).any()) and bool((z == -30).any()) and bool((z == 0).any())


@pytest.mark.parametrize("heads,S,n_added", [(1, 1, 1), (3, 33, 0), (3, 65, 1), (1, 64, 64)])
def test_qkv_references_equal_autograd(heads, S, n_added):
    raw, w, cos, sin, (dq, dk, dv) = TC.qkv_inputs(heads, S)
    r64 = raw.double().requires_grad_(True)
    f = TC.qkv_fwd_ref(r64, heads, n_added, w, cos, sin, 0.1275)
    (f["q"] * dq.double()).sum().backward(retain_graph=True)
    (f["k"] * dk.double()).sum().backward(retain_graph=True)
    (f["v"] * dv.double()).sum().backward()
    b = TC.qkv_bwd_ref(raw, heads, n_added, w, cos, sin, 0.1275, dq, dk, dv)
    _close(b["d_raw"], r64.grad, "d_raw")


def test_tile_packers_against_the_header_formulas():
    g = TC.gen(1)
    x = TC.rnd(g, 2, 128, 128)
    qt, vt = TC.t_tiles(x), TC.vt_tiles(x)
    for n in (0, 1, 3, 4, 5, 12, 15, 16, 17, 31, 32, 47, 63, 64, 100, 127):
        slot = 8 * ((n % 16) // 4) + 4 * ((n % 32) // 16) + n % 4
        assert torch.equal(qt[:, n // 32, :, slot], x[:, n]), n
        kv = n % 64
        p = (kv & ~12) | ((kv & 4) << 1) | ((kv & 8) >> 1)
        assert torch.equal(vt[:, n // 64, :, p], x[:, n]), n
    assert sorted(TC.slot32(torch.arange(32)).tolist()) == list(range(32))


# ---------------------------------------------------------------------------------------------- the reference alone inside the bound
@pytest.mark.parametrize("case", TC.ln_cases(), ids=lambda c: c[0])
def test_ln_fp32_restatement_inside_the_bound(case):
    _, rows, D, dres, dmod, _, offset = case
    for exact in (False, True):
        x, dy, scale, dr = TC.ln_inputs(rows, D, offset, exact)
        dr = dr if dres else None
        ref, y = TC.ln_bwd_ref(x, dy, scale, dr), TC.ln_bwd_ref(x, dy, scale, dr, dt=F32)
        _inside(y["dx"].to(BF), ref["dx"], TC.bound_ln_dx(ref, D), "dx")
        _inside(y["d_scale"], ref["d_scale"], TC.bound_colsum(rows, ref["scale_abs"]), "d_scale")
        if exact:
            assert float(ref["shift_abs"].max()) < 2 ** 24
            assert torch.equal(y["d_shift"].double(), ref["d_shift"]) and torch.equal(ref["d_shift"], ref["d_shift"].round())


@pytest.mark.parametrize("case", TC.gate_cases(), ids=lambda c: c[0])
def test_gate_fp32_restatement_inside_the_bound(case):
    _, rows, D, _, _ = case
    dy, f, gate = TC.gate_inputs(rows, D)
    ref, y = TC.gate_bwd_ref(dy, f, gate), TC.gate_bwd_ref(dy, f, gate, dt=F32)
    _inside(y["df"].to(BF), ref["df"], TC.bound_elementwise(ref["df"]), "df")
    dy, f, gate = TC.gate_inputs(rows, D, exact=True)
    ref, y = TC.gate_bwd_ref(dy, f, gate), TC.gate_bwd_ref(dy, f, gate, dt=F32)
    assert float(ref["gate_abs"].max()) < 2 ** 24 and torch.equal(ref["d_gate"], ref["d_gate"].round())
    assert torch.equal(y["d_gate"].double(), ref["d_gate"])
    _inside(y["df"].to(BF), ref["df"], TC.bound_elementwise(ref["df"]), "df (integer dy)")


@pytest.mark.parametrize("rows,cols", TC.EW_SHAPES)
def test_elementwise_fp32_restatements_inside_the_bound(rows, cols):
    z, dh = TC.gelu_inputs(rows, cols)
    h = TC.gelu(z.double())
    _inside(TC.gelu_sig(z.float()).to(BF), h, TC.bound_elementwise(h), "gelu")
    dz = dh.double() * TC.gelu_grad(z.double())
    _inside((dh.float() * TC.gelu_grad_sig(z.float())).to(BF), dz, TC.bound_elementwise(dz), "gelu'")
    dy, f, gate = TC.gate_inputs(rows, cols)
    out = TC.gate_fwd(f.double(), gate.double(), dy.double())
    _inside(TC.gate_fwd(f.float(), gate.float(), dy.float()).to(BF), out, TC.bound_elementwise(out), "gated residual")


@pytest.mark.parametrize("S,N,R", TC.tn_cases())
def test_tn_fp32_restatement_and_exact_cases(S, N, R):
    big, sk = TC.tn_inputs(S, N, R)
    ref = TC.tn_ref(big, sk)
    _inside(TC.tn_ref(big, sk, dt=F32)["out"].to(BF), ref["out"], TC.bound_tn(S, ref["out"], ref["abs"]), "out")
    big, sk = TC.tn_inputs(S, N, R, exact=True)
    ref = TC.tn_ref(big, sk)
    assert float(ref["abs"].max()) < 2 ** 24 and torch.equal(ref["out"], ref["out"].round())
    assert float(big.float().abs().max()) <= 8 and float(sk.float().abs().max()) <= 8
    assert torch.equal(TC.tn_ref(big, sk, dt=F32)["out"].double(), ref["out"])


@pytest.mark.parametrize("case", TC.qkv_cases(), ids=lambda c: "h{}_S{}_a{}_p{}_l{}_b{}".format(*[int(v) for v in c]))
def test_qkv_fp32_restatement_inside_the_bound(case):
    heads, S, n_added, _, _, _ = case
    raw, w, cos, sin, (dq, dk, dv) = TC.qkv_inputs(heads, S)
    ref, y = (TC.qkv_fwd_ref(raw, heads, n_added, w, cos, sin, 0.1275, dt=dt) for dt in (F64, F32))
    for nm in ("q", "k"):
        _inside(y[nm].to(BF), ref[nm], TC.bound_qkv_fwd(ref[nm], ref[nm + "_mag"]), nm)
    assert torch.equal(y["v"].to(BF), raw[:, 2 * heads * 128:].view(S, heads, 128).permute(1, 0, 2))
    rb, yb = (TC.qkv_bwd_ref(raw, heads, n_added, w, cos, sin, 0.1275, dq, dk, dv, dt=dt) for dt in (F64, F32))
    _inside(yb["d_raw"].to(BF), rb["d_raw"], TC.bound_qkv_bwd(rb), "d_raw")


def test_lora_references_are_consistent():
    """The unowned parts of the fused operands are zero; with every scaling at 1, fuse followed by unfuse (accumulate = 0) hands
    every wanted factor back bit for bit and leaves an unwanted one (NULL pointer) what it held; accumulating adds the same blocks
    to what the gradients held, with one more bf16 rounding."""
    for name, (K, N, r_pad, entries) in TC.lora_cases().items():
        fac, g0, dA, dBs = TC.lora_inputs(name)
        A, Bs = TC.lora_fuse_ref(name, fac)
        own_a, own_b = torch.zeros(r_pad, dtype=torch.bool), torch.zeros(N, r_pad, dtype=torch.bool)
        for (n0, n, r0, r, sc, _, _), (a, b) in zip(entries, fac):
            assert not own_a[r0:r0 + r].any(), "entries share rank rows"
            own_a[r0:r0 + r] = True
            own_b[n0:n0 + n, r0:r0 + r] = True
            assert torch.equal(A[r0:r0 + r], a)
        assert float(A[~own_a].abs().max() if (~own_a).any() else 0) == 0 and float(Bs[~own_b].abs().max()) == 0
        A1, B1 = TC.lora_fuse_ref(name, fac, scaling=1.0)
        back = TC.lora_unfuse_ref(name, g0, A1, B1, 0, scaling=1.0)
        acc = TC.lora_unfuse_ref(name, g0, A1, B1, 1, scaling=1.0)
        for (n0, n, r0, r, sc, wa, wb), (ga, gb), (ha, hb), (a, b), (a0, b0) in zip(entries, back, acc, fac, g0):
            assert torch.equal(ga, a if wa else a0) and torch.equal(gb, b if wb else b0), name
            assert torch.equal(ha, (a0.float() + a.float()).to(BF) if wa else a0), name
            assert torch.equal(hb, (b0.float() + b.float()).to(BF) if wb else b0), name
    assert len(TC.lora_cases()["eight"][3]) == 8
