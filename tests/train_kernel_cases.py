"""Case lists, inputs, fp64 references and acceptance bounds of the training-kernel edge tests (csrc/train_rowops.hip, csrc/optim.hip
through the C ABI of include/rf_flux.h, "TRAINING path").  Shared by tests/test_train_kernels_edges_gpu.py (the kernels against fp64)
and tests/test_train_kernels_cpu.py (the references against fp64 autograd, the exactness of the integer cases, and an fp32 restatement
of every formula against the same fp64 under the same bound on the same inputs: the bound is reachable by a correct kernel).
Plain torch on the CPU, deterministic.

Every reference takes `dt`: torch.float64 is the reference, torch.float32 the restatement (same formula, fp32 arithmetic, and the one
bf16 rounding on the way out that the kernels make).

Bounds (derived, not tuned).  u = 2^-8 is one bf16 rounding, relative (round-to-nearest needs half of it: the other half is the
room an fp32 result a few ulp off the reference needs to land on the neighbouring bf16 value); gamma(n) = (n + 16) 2^-24 bounds
an fp32 sum of n terms in ANY order, relative to the sum of the terms' magnitudes (the 16 are the multiplications, the rsqrt /
exp2 / rcp approximations and the second stage of a two-stage sum)."""
import math

import torch

BF = torch.bfloat16
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -8
EPS = 1e-6
PATTERN_PADS = (8, 24, 64, 200)          # the four row-pitch paddings (elements beyond the window's width; multiples of 8)


def gamma(n: int) -> float:
    return (n + 16) * 2.0 ** -24


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def rnd(g, *shape, sc=1.0):
    return (torch.randn(*shape, generator=g) * sc).to(BF)


def ints(g, *shape, lim=8):
    """small integers |v| <= lim: exactly representable in bf16, products and short sums exact in fp32"""
    return torch.randint(-lim, lim + 1, shape, generator=g).to(BF)


def bound_elementwise(ref):
    """GELU, GELU', gated residual, df: one bf16 rounding of an fp32 result within a few ulp"""
    return U * ref.abs() + 2.0 ** -20


def bound_colsum(rows, abs_sum):
    """fp32 column sums over `rows` terms, two-stage"""
    return 2 * gamma(rows) * abs_sum


def bound_tn(S, ref, abs_sum):
    return U * ref.abs() + gamma(S) * abs_sum


# ---- LayerNorm-modulate backward --------------------------------------------------------------------------------------------------
D_SET = (8, 264, 512, 520, 1024, 1032, 1536, 2048, 2056, 2560, 3064, 3072)      # NCH 1, 2, 4, 6 with an empty or partial last chunk


def ln_cases():
    """(id, rows, D, dres, dmod, pads (x, dy, dres, dx), offset).  offset != 0: every row has a mean of `offset` standard deviations."""
    out, k = [], 0

    def add(rows, D, offset=0.0):
        nonlocal k
        pads = tuple(PATTERN_PADS[(k + j) % 4] for j in range(4))
        # dres and d_scale / d_shift cycle through (given, given), (NULL, given), (given, NULL), (NULL, NULL)
        out.append((f"r{rows}_D{D}" + ("_mean8" if offset else ""), rows, D, k % 2 == 0, (k // 2) % 2 == 0, pads, offset))
        k += 1
    for D in D_SET:
        add(5, D)
    for rows in (1, 3, 4, 5, 13, 17, 65):
        for D in (8, 264, 1032):
            add(rows, D)
    for rows, D in ((2049, 1032), (2051, 1032), (1025, 3072), (2051, 3072)):      # past the 512- / 256-block cap: the grid-stride loop
        add(rows, D)
    add(2051, 1032)                                                               # ... once more with the other NULL combination
    add(17, 520, offset=8.0)
    for rows in (49, 53, 61, 64):               # 13 .. 16 partial rows: colsum_reduce's 16-way unrolled body runs in some of its four
        add(rows, 264)                          # row groups and only the tail loop in the others (w + 12 < nw per group)
    return out


def ln_inputs(rows, D, offset=0.0, exact=False, seed=0):
    g = gen(21, rows, D, seed, int(exact))
    x = (torch.randn(rows, D, generator=g) + offset).to(BF)
    scale = rnd(g, D, sc=0.3)
    if exact:
        return x, ints(g, rows, D), scale, ints(g, rows, D)
    return x, rnd(g, rows, D), scale, rnd(g, rows, D)


def ln_fwd(x, scale, shift, eps=EPS):
    """y = LayerNorm(x) (1 + scale) + shift, in x's dtype (for autograd)"""
    xc = x - x.mean(-1, keepdim=True)
    return xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps) * (1 + scale) + shift


def ln_bwd_ref(x, dy, scale, dres=None, eps=EPS, dt=F64):
    """dx, d_scale, d_shift of rf_layernorm_modulate_bwd and the magnitudes the bounds are made of"""
    x, dy, scale = x.to(dt), dy.to(dt), scale.to(dt)
    xc = x - x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    gy = dy * (1 + scale)
    m1, m2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - m1 - xh * m2)
    A = rstd * (gy.abs() + m1.abs() + (xh * m2).abs())
    if dres is not None:
        dx, A = dx + dres.to(dt), A + dres.to(dt).abs()
    return dict(dx=dx, d_scale=(dy * xh).sum(0), d_shift=dy.sum(0), A=A, scale_abs=(dy * xh).abs().sum(0), shift_abs=dy.abs().sum(0))


def bound_ln_dx(ref, D):
    return U * ref["dx"].abs() + 4 * gamma(D) * ref["A"]


# ---- gate backward / gated residual / GELU ----------------------------------------------------------------------------------------
def gate_cases():
    """(id, rows, D, d_gate wanted, pads (dy, f, df))"""
    out, k = [], 0

    def add(rows, D):
        nonlocal k
        out.append((f"r{rows}_D{D}", rows, D, k % 3 != 1, tuple(PATTERN_PADS[(k + j) % 4] for j in range(3))))
        k += 1
    for i, D in enumerate(D_SET):
        add((5, 13)[i % 2], D)
    for rows in (1, 3, 5, 13, 65):
        for D in (264, 1032):
            add(rows, D)
    for rows, D in ((2049, 520), (4099, 520), (2049, 1032), (4099, 1032), (2049, 3072)):      # rows > 2048: the grid-stride loop
        add(rows, D)
    for rows in (49, 53, 61, 64):               # 13 .. 16 partial rows: the boundary of colsum_reduce's 16-way unroll (see ln_cases)
        add(rows, 264)
    return out


def gate_inputs(rows, D, exact=False):
    g = gen(31, rows, D, int(exact))
    gate = rnd(g, D)
    if exact:
        return ints(g, rows, D), ints(g, rows, D), gate
    return rnd(g, rows, D), rnd(g, rows, D), gate


def gate_bwd_ref(dy, f, gate, dt=F64):
    dy, f, gate = dy.to(dt), f.to(dt), gate.to(dt)
    return dict(df=gate * dy, d_gate=(dy * f).sum(0), gate_abs=(dy * f).abs().sum(0))


def gate_fwd(f, gate, res):
    return res + gate * f


EW_SHAPES = ((1, 8), (77, 512), (3, 3064), (1030, 8192))      # the last: 1 054 720 eight-element items, one block past the 4096-block grid
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu(z):
    """gelu_tanh in z's dtype"""
    return 0.5 * z * (1 + torch.tanh(K0 * (z + K1 * z * z * z)))


def gelu_grad(z):
    """d gelu_tanh / dz, written out"""
    t = torch.tanh(K0 * (z + K1 * z * z * z))
    return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * K0 * (1 + 3 * K1 * z * z)


def gelu_sig(z):
    """the same functions in the form the kernels evaluate: gelu = z s, gelu' = s + z s (1 - s) 2u', s = sigmoid(2u).  Identical in
    exact arithmetic; in fp32 the tanh form loses gelu' for z << 0 to the cancellations 1 + t and 1 - t^2 (absolute error 1e-7 times
    0.5 |z| u' ~ 10, against a result that tends to 0), the sigmoid form does not -- so THIS is the fp32 restatement the bound is
    proved reachable with, and the fp64 reference stays the tanh form that is checked against autograd."""
    return z * torch.sigmoid(2 * K0 * (z + K1 * z * z * z))


def gelu_grad_sig(z):
    s = torch.sigmoid(2 * K0 * (z + K1 * z * z * z))
    return s + z * s * (1 - s) * 2 * K0 * (1 + 3 * K1 * z * z)


def gelu_inputs(rows, cols):
    """z with +-0, +-30 and a grid around -0.75 where GELU' changes sign; dh"""
    g = gen(41, rows, cols)
    z = (torch.randn(rows, cols, generator=g) * 2.0).flatten()
    special = torch.cat([torch.tensor([0.0, -0.0, 30.0, -30.0]), -1.0 + torch.arange(64) / 128.0])      # -1 .. -0.5 in bf16 steps
    n = min(z.numel(), special.numel())
    z[:n] = special[:n]
    if z.numel() > 4 * special.numel():
        z[-special.numel():] = special                   # ... and in the last items of the tensor (the grid-stride tail)
    return z.view(rows, cols).to(BF), rnd(g, rows, cols)


# ---- transpose --------------------------------------------------------------------------------------------------------------------
# (rows, cols, rows_pad, extra ld_dst, src pad): vector path = everything a multiple of 8; any odd number sends it to the scalar kernel
TRANSPOSE_CASES = (
    ("vec", 1, 8, 8, 0, 8), ("vec", 63, 64, 64, 8, 8), ("vec", 65, 72, 128, 0, 24), ("vec", 100, 328, 128, 64, 8),
    ("scalar", 1, 1, 1, 0, 3), ("scalar", 65, 3, 70, 5, 1), ("scalar", 100, 64, 100, 0, 8), ("scalar", 64, 65, 64, 8, 7),
)


def transpose_ref(src, rows_pad):
    out = torch.zeros(src.shape[1], rows_pad, dtype=src.dtype)
    out[:, :src.shape[0]] = src.T
    return out


# ---- token-axis skinny GEMM -------------------------------------------------------------------------------------------------------
TN_S = (1, 31, 32, 33, 127, 128, 129, 257)
TN_N = (8, 120, 128, 136)
TN_R = (16, 48, 80, 112, 128, 144, 208)       # slices 16 | 32+16 | 64+16 | 64+32+16 | 128 | 128+16 | 128+64+16


def tn_cases():
    """every S, every N and every R at least once (the three lists walked together)"""
    return [(TN_S[i % 8], TN_N[i % 4], TN_R[i % 7]) for i in range(8)] + [(257, 136, 208), (129, 120, 128)]


def tn_inputs(S, N, R, exact=False):
    g = gen(51, S, N, R, int(exact))
    return (ints(g, S, N), ints(g, S, R)) if exact else (rnd(g, S, N), rnd(g, S, R))


def tn_ref(big, sk, dt=F64):
    return dict(out=big.to(dt).T @ sk.to(dt), abs=big.to(dt).abs().T @ sk.to(dt).abs())


# ---- q|k|v -> attention operands and back ---------------------------------------------------------------------------------------
def qkv_cases():
    """(heads, S, n_added, extra s_pad, extra ld_raw, backward operands)"""
    out = []
    for i, S in enumerate((1, 31, 33, 63, 64, 65, 112)):
        heads = (1, 3)[i % 2]
        n_added = (0, 1, S)[i % 3]
        out.append((heads, S, n_added, 64 * (i % 2), 512 * ((i // 2) % 2), i % 4 != 3))
    out += [(3, 65, 65, 0, 0, True), (1, 112, 1, 64, 512, False), (3, 33, 0, 64, 512, True)]
    return out


def qkv_inputs(heads, S):
    """raw [S][3 D]; four norm weights; cos / sin as ARBITRARY fp32 tables in [-1, 1] (the map is linear in them: a swapped index
    shows, which a true rotation with cos[2i] == cos[2i+1] would hide); dq, dk, dv [heads][S][128]"""
    g = gen(61, heads, S)
    D = heads * 128
    raw = rnd(g, S, 3 * D)
    w = [(1 + 0.1 * torch.randn(128, generator=g)).to(BF) for _ in range(4)]
    cos, sin = (torch.rand(S, 128, generator=g) * 2 - 1 for _ in range(2))
    d = [rnd(g, heads, S, 128) for _ in range(3)]
    return raw, w, cos, sin, d


def _tok_w(S, n_added, w_main, w_added, dt):
    tok = torch.arange(S)[:, None, None]
    return torch.where(tok < n_added, w_added.to(dt), w_main.to(dt)) if n_added else w_main.to(dt).expand(S, 1, 128)


def _norm_rope(x, w, cos, sin, eps, sc):
    """x [S, H, 128]: per-head RMSNorm, weight, RoPE on (even, odd) pairs with the tables' own even / odd entries, scale"""
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w
    a, b = y[..., 0::2], y[..., 1::2]
    c0, c1, s0, s1 = cos[:, None, 0::2], cos[:, None, 1::2], sin[:, None, 0::2], sin[:, None, 1::2]
    o = torch.stack([a * c0 - b * s0, b * c1 + a * s1], -1).flatten(-2) * sc
    mag = torch.stack([(a * c0).abs() + (b * s0).abs(), (b * c1).abs() + (a * s1).abs()], -1).flatten(-2) * abs(sc)
    return o, mag


def qkv_fwd_ref(raw, heads, n_added, w, cos, sin, q_scale, eps=EPS, dt=F64):
    """-> q, k, v [heads][S][128] (and the magnitudes of the q / k bound).  raw may require grad (dt must then be its dtype)."""
    S, D = raw.shape[0], heads * 128
    r = raw.to(dt)
    cos, sin = cos.to(dt), sin.to(dt)
    x = [r[:, a * D:(a + 1) * D].reshape(S, heads, 128) for a in range(3)]
    q, qm = _norm_rope(x[0], _tok_w(S, n_added, w[0], w[2], dt), cos, sin, eps, q_scale)
    k, km = _norm_rope(x[1], _tok_w(S, n_added, w[1], w[3], dt), cos, sin, eps, 1.0)
    p = lambda t: t.permute(1, 0, 2)   # noqa: E731
    return dict(q=p(q), k=p(k), v=p(x[2]), q_mag=p(qm), k_mag=p(km))


def bound_qkv_fwd(ref, mag):
    return U * ref.abs() + 4 * gamma(128) * mag


def qkv_bwd_ref(raw, heads, n_added, w, cos, sin, q_scale, dq, dk, dv, eps=EPS, dt=F64):
    """d_raw [S][3 D] written out by hand (RoPE^T, weight, RMSNorm backward) and the magnitude A of its bound"""
    S, D = raw.shape[0], heads * 128
    r = raw.to(dt)
    cos, sin = cos.to(dt), sin.to(dt)
    c0, c1, s0, s1 = cos[:, None, 0::2], cos[:, None, 1::2], sin[:, None, 0::2], sin[:, None, 1::2]
    outs, mags = [], []
    for a, (go, sc, wm, wa) in enumerate(((dq, q_scale, w[0], w[2]), (dk, 1.0, w[1], w[3]))):
        x = r[:, a * D:(a + 1) * D].reshape(S, heads, 128)
        wt = _tok_w(S, n_added, wm, wa, dt)
        rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
        n = x * rs
        g = go.to(dt).permute(1, 0, 2) * sc
        ga, gb = g[..., 0::2], g[..., 1::2]
        dy = torch.stack([ga * c0 + gb * s1, gb * c1 - ga * s0], -1).flatten(-2)
        dy_mag = torch.stack([(ga * c0).abs() + (gb * s1).abs(), (gb * c1).abs() + (ga * s0).abs()], -1).flatten(-2)
        dn = dy * wt
        outs.append(rs * (dn - n * (dn * n).mean(-1, keepdim=True)))
        mags.append(rs * (dy_mag * wt.abs() + n.abs() * (dy_mag * wt.abs() * n.abs()).mean(-1, keepdim=True)))
    outs.append(dv.to(dt).permute(1, 0, 2))
    mags.append(torch.zeros_like(outs[-1]))
    return dict(d_raw=torch.cat([o.reshape(S, D) for o in outs], 1), A=torch.cat([m.reshape(S, D) for m in mags], 1))


def bound_qkv_bwd(ref):
    return U * ref["d_raw"].abs() + 4 * gamma(128) * ref["A"]


def slot32(n):
    """rf_flux.h: slot(n) = 8 ((n%16)/4) + 4 ((n%32)/16) + n%4"""
    return 8 * ((n % 16) // 4) + 4 * ((n % 32) // 16) + n % 4


def t_tiles(x):
    """[heads][s_pad][128] -> the transposed tiles [heads][s_pad/32][128][32]: element (d, slot(n)) of block n/32 = x[n][d]"""
    H, sp, _ = x.shape
    n = torch.arange(sp)
    out = torch.zeros(H, sp // 32, 128, 32, dtype=x.dtype)
    out[:, n // 32, :, slot32(n)] = x.permute(1, 0, 2)
    return out


def vt_tiles(v):
    """[heads][s_pad][128] -> rf_attention's V^T tiles [heads][s_pad/64][128][64]: key kv of a tile at p(kv) = bits 2 and 3 swapped"""
    H, sp, _ = v.shape
    n = torch.arange(sp)
    kv = n % 64
    p = (kv & ~12) | ((kv & 4) << 1) | ((kv & 8) >> 1)
    out = torch.zeros(H, sp // 64, 128, 64, dtype=v.dtype)
    out[:, n // 64, :, p] = v.permute(1, 0, 2)
    return out


def pad_rows(x, s_pad):
    out = torch.zeros(x.shape[0], s_pad, x.shape[2], dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


# ---- fused LoRA operands ----------------------------------------------------------------------------------------------------------
def lora_cases():
    """id -> (K, N, r_pad, entries [(n0, n, r0, r, scaling, dA wanted, dB wanted)])"""
    return {
        "one_r4": (64, 24, 8, [(0, 24, 0, 4, 2.0, True, True)]),                                            # r_pad > sum r
        "shared_group": (72, 40, 8, [(0, 16, 0, 4, 0.75, True, True), (16, 24, 4, 4, 1.5, True, True)]),      # two entries in one 8-column group
        "three_gaps": (136, 100, 64, [(8, 24, 0, 8, 1.0, True, False), (40, 16, 8, 16, 0.5, False, True),      # rows 0-7, 32-39, 56-99 unowned;
                                      (40, 16, 24, 4, 3.0, True, True)]),                                      # two adapters of ONE linear; NULL dA / dB
        "eight": (64, 8 * 12, 128, [(12 * i, 12, r0, r, 0.25 * (i + 1), i != 3, i != 5) for i, (r0, r) in
                                    enumerate(((0, 4), (4, 4), (8, 8), (16, 16), (32, 32), (64, 4), (72, 8), (80, 32)))]),
        "r32": (264, 33, 64, [(1, 32, 16, 32, 0.5, True, True)]),
    }


def lora_inputs(name):
    K, N, r_pad, entries = lora_cases()[name]
    g = gen(71, len(name), K, N)
    fac = [(rnd(g, r, K), rnd(g, n, r)) for (_, n, _, r, _, _, _) in entries]
    grads0 = [(rnd(g, r, K), rnd(g, n, r)) for (_, n, _, r, _, _, _) in entries]      # what dA_i / dB_i hold before an accumulating call
    return fac, grads0, rnd(g, r_pad, K), rnd(g, N, r_pad)


def lora_fuse_ref(name, fac, scaling=None):
    """scaling: replaces every entry's own (the CPU test's round trip uses 1)"""
    K, N, r_pad, entries = lora_cases()[name]
    A, Bs = torch.zeros(r_pad, K, dtype=BF), torch.zeros(N, r_pad, dtype=BF)
    for (n0, n, r0, r, sc, _, _), (a, b) in zip(entries, fac):
        sc = sc if scaling is None else scaling
        A[r0:r0 + r] = a
        Bs[n0:n0 + n, r0:r0 + r] = (b.float() * sc).to(BF)          # bf16(scaling * B): one fp32 product, one rounding
    return A, Bs


def lora_unfuse_ref(name, grads0, dA, dBs, accumulate, scaling=None):
    """-> [(dA_i, dB_i)] with the header's roundings: dA rows copied (or bf16(dA_i + rows)); bf16(scaling * dBs) (or
    bf16(bf16(scaling * dBs) + dB_i)).  Entries whose pointer is NULL keep what they held."""
    K, N, r_pad, entries = lora_cases()[name]
    out = []
    for (n0, n, r0, r, sc, wa, wb), (a0, b0) in zip(entries, grads0):
        sc = sc if scaling is None else scaling
        ga, gb = dA[r0:r0 + r], (dBs[n0:n0 + n, r0:r0 + r].float() * sc).to(BF)
        if accumulate:
            ga, gb = (a0.float() + ga.float()).to(BF), (b0.float() + gb.float()).to(BF)
        out.append((ga if wa else a0, gb if wb else b0))
    return out


# ---- optimizers -------------------------------------------------------------------------------------------------------------------
OPT_N = (8, 8184, 8192, 8200, 24584)       # the tails of the 8192-element block


def opt_inputs(n, seed=0):
    """param, grad, exp_avg, exp_avg_sq (>= 1e-4: an update stays a few bf16 spacings of the parameter, so the rounding of a bf16
    state between Prodigy's launches cannot move it by a spacing), s"""
    g = gen(81, n, seed)
    p = rnd(g, n, sc=0.05)
    return p, rnd(g, n, sc=0.1), rnd(g, n, sc=0.01), ((torch.randn(n, generator=g) * 0.01).square() + 1e-4).to(BF), rnd(g, n, sc=0.05)
