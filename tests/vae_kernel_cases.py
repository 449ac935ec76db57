"""Inputs, fp64 references and fp32 yardsticks of the VAE op tests (csrc/vae.hip through rf_debug_vae_op).  Shared by
tests/test_vae_kernels_gpu.py (the kernels against fp64) and tests/test_vae_kernels_cpu.py (the yardsticks -- fp32 restatements that round
where the kernels round -- against the same fp64 under the same bound, on the same inputs: the bound is reachable by a correct kernel).
Everything here is plain torch on the CPU and deterministic."""
import math

import torch
import torch.nn.functional as F

BF = torch.bfloat16
VA_C = 512
TAIL = 64                       # RF_VAE_TAIL_PIXELS


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


# ---- attention core ---------------------------------------------------------------------------------------------------------
ATTN_S = (64, 128, 192, 320)
ATTN_FORMS = ("plain", "peaked", "rising", "falling")
ATTN_SLOPE = 0.25               # score per key index of the rising / falling forms: 8 per 32-key tile against unit-variance noise


def attn_inputs(form, S):
    """q, k, v bf16 [S][512], every row distinct.  rising / falling add a shared unit direction u: q += 8 u, k_j += b_j u with b_j
    growing / shrinking linearly in the key index j, so the scaled score carries ATTN_SLOPE * j (or * (S-1-j)) on top of N(0,1) noise:
    the running max rises on every 32-key tile (the alpha != 1 rescale fires on every tile) / never after the first (it never fires)."""
    g = gen(11, ATTN_FORMS.index(form), S)
    q, k, v = (torch.randn(S, VA_C, generator=g) for _ in range(3))
    if form == "peaked":
        q = q * 6
    if form in ("rising", "falling"):
        u = torch.randn(VA_C, generator=g)
        u = u / u.norm()
        j = torch.arange(S, dtype=torch.float32)
        if form == "falling":
            j = (S - 1) - j
        beta = ATTN_SLOPE * math.sqrt(VA_C) / 8.0
        q = q + 8.0 * u
        k = k + (beta * j)[:, None] * u
    return q.to(BF), k.to(BF), v.to(BF)


def attn_ref64(q, k, v):
    s = (q.double() @ k.double().T) / math.sqrt(q.shape[1])
    return torch.softmax(s, -1) @ v.double()


def attn_yardstick(q, k, v, tile=32):
    """vae_attn_kernel's arithmetic in fp32: online softmax over 32-key tiles in the exp2 domain, P rounded to bf16 before PV, the row sum
    from the unrounded P, one output rounding."""
    S, C = q.shape
    sl2 = 1.4426950408889634 / math.sqrt(C)
    qf, kf, vf = q.float(), k.float(), v.float()
    m = torch.full((S,), -1e30)
    l = torch.zeros(S)
    o = torch.zeros(S, C)
    for t in range(0, S, tile):
        sc = (qf @ kf[t:t + tile].T) * sl2
        m_new = torch.maximum(m, sc.max(1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(sc - m_new[:, None])
        l = l * alpha + p.sum(1)
        o = o * alpha[:, None] + p.to(BF).float() @ vf[t:t + tile]
        m = m_new
    return (o * (1.0 / l)[:, None]).to(BF)


def attn_rescale_counts(q, k, tile=32):
    """per query: on how many tiles AFTER the first the running max rises (alpha != 1)"""
    sc = (q.float() @ k.float().T)
    tm = sc.view(sc.shape[0], -1, tile).max(2).values
    run = torch.cummax(tm, 1).values
    return (run[:, 1:] > run[:, :-1]).sum(1)


def routing_inputs(S):
    """k_j = 32 e_c(j), q_i = 32 e_c(pi(i)): the hit scores 1024 / sqrt(512) = 45.3, every other key 0, so every other key weighs e^-45
    -- below half an ulp of any |v| >= 2^-6 in fp32 even summed over 320 keys: out[i] must be BIT-EQUAL to v[pi(i)].
    c(j) = 8 ((37 j) mod 64) + ((j div 64 + j) mod 8) is injective for S <= 512 and touches every 16-byte chunk 0..63 of a K row (both
    channel halves) already with 64 keys; pi(i) = (7 i + 3) mod S."""
    j = torch.arange(S)
    c = 8 * ((37 * j) % 64) + ((j // 64 + j) % 8)
    assert len(set(c.tolist())) == S and set((c // 8).tolist()) == set(range(64))
    pi = (7 * j + 3) % S
    assert sorted(pi.tolist()) == list(range(S)) and not torch.equal(pi, j)
    k = torch.zeros(S, VA_C)
    k[j, c] = 32.0
    q = torch.zeros(S, VA_C)
    q[j, c[pi]] = 32.0
    g = gen(12, S)
    v = torch.randn(S, VA_C, generator=g)
    v = torch.sign(v) * (v.abs() + 2.0 ** -6)
    return q.to(BF), k.to(BF), v.to(BF), pi


# ---- GroupNorm --------------------------------------------------------------------------------------------------------------
GN_C = (64, 128, 256, 512)
GN_HW = ((1, 1), (3, 5), (8, 8), (17, 23))
GN_CAPPED = (363, 361, 64)      # npix = 365 * 363 = 132 495 >= 2048 * 64: nblk = 2048, pix_per_block = 65
GN_GROUPS = 32
GN_BLOCKS = 2048
# first-pixel outlier: 2^k with the largest k for which the yardstick stays under HALF the bound on every GN shape
# (tests/test_vae_kernels_cpu.py::test_group_norm_outlier_exponent_is_the_largest holds k and k + 1 to that)
GN_OUTLIER_LOG2 = 5
GN_FORMS = ("normal", "group_offset", "channel_offset", "outlier")


def gn_inputs(form, H, W, C, outlier_log2=None):
    """x bf16 [H][W][C] (interior), gamma, beta bf16 [C]"""
    g = gen(21, GN_FORMS.index(form), H, W, C)
    x = torch.randn(H, W, C, generator=g)
    if form == "group_offset":
        x = x + 200.0
    elif form == "channel_offset":
        x = x + (torch.rand(C, generator=g) * 400.0 - 200.0)
    elif form == "outlier":
        x[0, 0, :] = 2.0 ** (GN_OUTLIER_LOG2 if outlier_log2 is None else outlier_log2)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    return x.to(BF), gamma.to(BF), beta.to(BF)


def silu64(t):
    return t * torch.sigmoid(t)


def gn_ref64(x, gamma, beta, silu, groups=GN_GROUPS):
    y = F.group_norm(x.double().permute(2, 0, 1)[None], groups, gamma.double(), beta.double(), eps=1e-6)[0].permute(1, 2, 0)
    return silu64(y) if silu else y


def gn_yardstick(x, gamma, beta, silu, groups=GN_GROUPS):
    """The three passes in the kernels' precision: per block of pix_per_block PADDED pixels fp32 sums of (x - s) and (x - s)^2 with
    s = the channel's first interior pixel; fp64 over the blocks, un-shift, mean / rstd; the affine a, b rounded to fp32; y = x a + b
    (+ SiLU) in fp32, one rounding to bf16."""
    H, W, C = x.shape
    Wp = W + 2
    npix = (H + 2) * Wp
    nblk = -(-npix // 64) if npix < GN_BLOCKS * 64 else GN_BLOCKS
    ppb = -(-npix // nblk)
    xp = torch.zeros(nblk * ppb, C)
    inside = torch.zeros(nblk * ppb, dtype=torch.bool)
    idx = ((torch.arange(H) + 1)[:, None] * Wp + torch.arange(W)[None] + 1).reshape(-1)
    xp[idx] = x.float().reshape(-1, C)
    inside[idx] = True
    sh = x[0, 0].float()
    d = torch.where(inside[:, None], xp - sh, torch.zeros(()))
    a = d.view(nblk, ppb, C).sum(1)                       # fp32 per block
    b = (d * d).view(nblk, ppb, C).sum(1)
    a, b, s = a.double().sum(0), b.double().sum(0), sh.double()
    n = float(H * W)
    cpg = C // groups
    t1 = (a + n * s).view(groups, cpg).sum(1)
    t2 = (b + 2.0 * s * a + n * s * s).view(groups, cpg).sum(1)
    count = n * cpg
    mean = t1 / count
    var = (t2 / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    mean, rstd = mean.repeat_interleave(cpg), rstd.repeat_interleave(cpg)
    A = (rstd * gamma.double()).float()
    B = (beta.double() - mean * rstd * gamma.double()).float()
    y = x.float() * A + B
    if silu:
        y = y * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * y)))
    return y.to(BF)


# ---- convolutions -----------------------------------------------------------------------------------------------------------
CONV_SHAPES = ((64, 128), (128, 256), (64, 32))
CONV_HW = ((1, 1), (2, 3), (5, 29), (7, 40))
CONV_NARROW = (128, 8)
CONV_NARROW_HW = ((5, 28), (5, 29), (5, 40))          # fold 32: unfolded (32 > W + 3), the boundary fold == W + 3, folded


def conv_module(cin, cout, stride=1, zero_bias=False):
    """a torch Conv2d whose weights are bf16 values (so the packer's rounding changes nothing), unit-variance outputs"""
    g = gen(31, cin, cout, stride)
    m = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1 if stride == 1 else 0)
    with torch.no_grad():
        m.weight.copy_((torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(BF).float())
        m.bias.copy_(torch.zeros(cout) if zero_bias else torch.randn(cout, generator=g).to(BF).float())
    return m


def conv_inputs(H, W, cin, cout):
    g = gen(32, H, W, cin, cout)
    return torch.randn(H, W, cin, generator=g).to(BF), torch.randn(H, W, cout, generator=g).to(BF)      # x, residual


@torch.no_grad()
def conv_ref64(m, x, residual=None):
    """x [H][W][cin] -> [H][W][cout] fp64: F.conv2d(padding=1), or the stride-2 form over F.pad(x, (0, 1, 0, 1))"""
    xi = x.double().permute(2, 0, 1)[None]
    if m.stride[0] == 2:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), m.weight.double(), m.bias.double(), stride=2)
    else:
        y = F.conv2d(xi, m.weight.double(), m.bias.double(), padding=1)
    y = y[0].permute(1, 2, 0)
    return y if residual is None else y + residual.double()


def impulse_positions(H, W):
    """the four corners, one pixel of each edge, the centre (distinct ones)"""
    ps = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]
    return sorted(set(ps))


# ---- attention block --------------------------------------------------------------------------------------------------------
BLOCK_HW = ((8, 8), (8, 16))
# to_q, to_k weights and biases x this: scores of std 1.6, the largest row weight 13 .. 18 x the uniform 1 / S.  The largest gain on a grid
# of 0.5 for which block_yardstick stays under half the bound (q and k are rounded to bf16 between the launches, so the score error, and
# with it the distance of ANY bf16 pipeline from fp64, grows with the gain: 2.5 -> 0.72 of the bound, 3.5 -> 1.27)
BLOCK_QK_GAIN = 2.0


def block_module():
    from reflectionflow_amd.flux.vae import VaeAttention
    torch.manual_seed(41)
    m = VaeAttention(VA_C, GN_GROUPS)
    with torch.no_grad():
        for lin in (m.to_q, m.to_k):
            lin.weight.mul_(BLOCK_QK_GAIN)
            lin.bias.mul_(BLOCK_QK_GAIN)
        m.group_norm.weight.copy_(1.0 + 0.3 * torch.randn(VA_C))
        m.group_norm.bias.copy_(0.3 * torch.randn(VA_C))
        for p in m.parameters():
            p.copy_(p.to(BF).float())
    return m.eval()


def block_input(H, W):
    return (torch.randn(H, W, VA_C, generator=gen(42, H, W)) + 0.5).to(BF)


@torch.no_grad()
def block_ref64(m, x):
    return m.double()(x.double().permute(2, 0, 1)[None])[0].permute(1, 2, 0)


@torch.no_grad()
def block_yardstick(m, x):
    """attention() of csrc/vae.hip with its roundings: bf16 between every launch, the V bias folded into the out-projection bias"""
    H, W, C = x.shape
    gn = m.group_norm
    xn = gn_yardstick(x, gn.weight.to(BF), gn.bias.to(BF), False).reshape(H * W, C)
    lin = lambda t, w, b: (t.float() @ w.to(BF).float().T + (0 if b is None else b.float())).to(BF)
    q, k = lin(xn, m.to_q.weight, m.to_q.bias.to(BF)), lin(xn, m.to_k.weight, m.to_k.bias.to(BF))
    v = lin(xn, m.to_v.weight, None)
    ao = attn_yardstick(q, k, v)
    wo = m.to_out[0].weight.float()
    bo = (m.to_out[0].bias.float() + wo @ m.to_v.bias.float()).to(BF)
    o = lin(ao, wo, bo)
    return (x.float() + o.float().reshape(H, W, C)).to(BF)
