"""Stale-content invariance of every scratch buffer the library runs out of: the engine workspace (rf_double_block_fwd,
rf_single_block_fwd, rf_flux_forward, rf_flux_denoise, rf_flux_denoise_guided), the pad rows and the split-launch scratch of the
attention forward, the stream-K partials of the GEMMs, and the workspaces of the text / CLIP / vision towers.

The contract (include/rf_flux.h, rf_workspace): zero-fill a workspace once -- for the 4 KiB stream-K flag page inside -- and after
that the library depends on no byte of it between calls.  Every other test of the suite runs on a zero-filled buffer that is then
reused with identical inputs, where a read-before-write sees either zeros or the right value: these tests fill the buffer with what a
previous, different call (or nobody) left there -- the patterns of tests/workspace_poison.py -- and demand the result of the
zero-filled run BIT FOR BIT.  No tolerance anywhere; the zero-filled run itself must be finite and not constant.

Safety: the flag page is never written and a workspace is never shared between two geometries (tests/workspace_poison.py,
`Workspace`); a non-zero flag could make a stream-K launch wait forever.
"""
import ctypes as C
import math

import pytest
import torch

from tests.golden_util import build
from tests.workspace_poison import PATTERNS, POISONS, Workspace, assert_live, assert_same_bits, bits, fill_bytes, pattern_words

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rnd(*shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(BF)


# =====================================================================================================================
# a. engine entry points
# =====================================================================================================================
# (S_txt, S_img, S_cond): S = 83 (45 pad keys) | S = 147 with a condition | S = 256 (no pad: the shift-free kernels) | one text token
GEOMS = {"s83": (19, 64, 0), "s147": (19, 64, 64), "s256": (64, 192, 0), "s65": (1, 64, 0)}
# variant -> (geometry, model_config, c_factor, fp8)
VARIANTS = {
    "s83": ("s83", {}, None, False),
    "s83-lora_main": ("s83", {"latent_lora": True}, None, False),
    "s83-fp8": ("s83", {}, None, True),
    "s147-bias": ("s147", {}, 1.5, False),                                  # attn_mode 1, cross_bias = log 1.5
    "s147-mask": ("s147", {"union_cond_attn": False}, None, False),         # attn_mode 2
    "s147-bias-lora_main": ("s147", {"latent_lora": True}, 1.5, False),
    "s147-mask-fp8": ("s147", {"union_cond_attn": False}, None, True),
    "s147-bias-add_cond": ("s147", {"add_cond_attn": True}, 1.5, False),
    "s256": ("s256", {}, None, False),
    "s256-fp8": ("s256", {}, None, True),
    "s65": ("s65", {}, None, False),
    "s65-lora_main": ("s65", {"latent_lora": True}, None, False),
}
CALLS = ("double", "single", "forward", "denoise", "guided")


@pytest.fixture(scope="module")
def engines(dev):
    """{fp8: FluxEngine} over the small hd128 model (D 256, 2 heads, 2 + 2 blocks) with rank-4 LoRA: the fused q|k|v factors have
    rank 12, r_pad 64, so columns 64 .. 255 of the LT rows are never written."""
    from reflectionflow_amd.engine import FluxEngine
    from tests.test_model_gpu import to_product
    out = {}
    with torch.no_grad():
        for fp8 in (False, True):
            tr = to_product(build("hd128", lora=True), dev).transformer
            object.__setattr__(tr, "_rf_fp8", fp8)
            out[fp8] = FluxEngine(tr)
            assert out[fp8].fp8 == fp8 and out[fp8]._dbl[0].lora_qkv.r_pad == 64
    return out


class EngineCase:
    """One (geometry, variant): its dims, its inputs (seeded, `scale` x the usual activation scale) and the five calls."""

    def __init__(self, eng, variant, dev):
        from reflectionflow_amd import _lib
        geom, mc, cf, fp8 = VARIANTS[variant]
        self.eng, self.dev, self.variant, self.mc, self.cf = eng, dev, variant, mc, cf
        self.St, self.Si, self.Sc = GEOMS[geom]
        self.d = eng.dims(self.St, self.Si, self.Sc, mc, cf)
        assert self.d.fp8 == int(fp8)
        self.lib = _lib.load()
        self.total = int(self.lib.rf_workspace_bytes(C.byref(self.d)))
        self.layout = _lib.workspace_layout(self.d)
        S = self.St + self.Si + self.Sc
        th = torch.rand(S, 128, generator=torch.Generator().manual_seed(5)) * 6.28
        self.cos, self.sin = th.cos().to(dev).contiguous(), th.sin().to(dev).contiguous()

    def workspace(self):
        return Workspace(self.total, self.layout["sk_flags"], self.dev)

    def inputs(self, seed, scale=1.0):
        e, dev, D = self.eng, self.dev, self.eng.D
        r = lambda *s, k, sc=1.0: rnd(*s, dev=dev, seed=seed * 100 + k, scale=sc * scale)  # noqa: E731
        i = dict(x_txt=r(self.St, D, k=1), x_img=r(self.Si, D, k=2), x_cond=r(max(self.Sc, 1), D, k=3),
                 lat=r(self.Si, e.in_ch, k=4), ctx=r(self.St, e.model.joint_dim, k=5), cond=r(max(self.Sc, 1), e.in_ch, k=6),
                 unc=r(2, max(self.Sc, 1), e.in_ch, k=7),
                 # modulation rows: scales / shifts / gates of size 0.3 keep three denoise steps of the synthetic model finite
                 mod6=[r(6 * D, k=8 + j, sc=0.3) for j in range(3)], mod3=[r(3 * D, k=11 + j, sc=0.3) for j in range(2)],
                 mod_steps=r(3, e.mod_cols, k=13, sc=0.3), mod_unc=r(3, e.mod_cols, k=14, sc=0.3), mod_cond=r(e.mod_cols, k=15, sc=0.3))
        return i

    def applies(self, call):
        return call != "guided" or self.Sc > 0

    def run(self, call, i, ws):
        """one library call on the rf_workspace `ws`; returns the tensor(s) it produced, concatenated"""
        from reflectionflow_amd import _lib, ops
        e, d, lib, Sc = self.eng, self.d, self.lib, self.Sc
        cond = lambda t: t if Sc > 0 else None  # noqa: E731
        if call == "double":
            xt, xi, xc = i["x_txt"].clone(), i["x_img"].clone(), i["x_cond"].clone()
            _lib.check(lib.rf_double_block_fwd(C.byref(d), C.byref(e._dbl[0]), xt.data_ptr(), xi.data_ptr(), ops.ptr(cond(xc)), e.D,
                                               i["mod6"][0].data_ptr(), i["mod6"][1].data_ptr(), ops.ptr(cond(i["mod6"][2])),
                                               self.cos.data_ptr(), self.sin.data_ptr(), C.byref(ws), ops.stream_ptr()), "rf_double_block_fwd")
            return torch.cat([xt, xi] + ([xc] if Sc > 0 else []))
        if call == "single":
            xm, xc = torch.cat([i["x_txt"], i["x_img"]]).contiguous(), i["x_cond"].clone()
            _lib.check(lib.rf_single_block_fwd(C.byref(d), C.byref(e._sgl[0]), xm.data_ptr(), ops.ptr(cond(xc)), e.D, i["mod3"][0].data_ptr(),
                                               ops.ptr(cond(i["mod3"][1])), self.cos.data_ptr(), self.sin.data_ptr(), C.byref(ws),
                                               ops.stream_ptr()), "rf_single_block_fwd")
            return torch.cat([xm] + ([xc] if Sc > 0 else []))
        kw = dict(cond_latents=cond(i["cond"]), mod_cond=cond(i["mod_cond"]), model_config=self.mc, c_factor=self.cf, ws=ws)
        if call == "forward":
            return e.forward(i["lat"], i["ctx"], i["mod_steps"][0], self.cos, self.sin, **kw)
        if call == "denoise":
            return e.denoise(i["lat"].clone(), i["ctx"], i["mod_steps"], [-0.3, -0.3, -0.4], self.cos, self.sin, use_graph=False, **kw)
        assert call == "guided"
        kw.pop("cond_latents"), kw.pop("mod_cond")
        return e.denoise_guided(i["lat"].clone(), i["ctx"], i["mod_steps"][:2].contiguous(), i["mod_unc"][:2].contiguous(), [-0.5, -0.5],
                                self.cos, self.sin, i["cond"], i["unc"], i["mod_cond"], 1.5, use_graph=False, **kw)


# (image guidance needs a condition: "guided" is a case of the conditioned geometry only)
ENGINE_CASES = [(v, c) for v in VARIANTS for c in CALLS if c != "guided" or GEOMS[VARIANTS[v][0]][2] > 0]


@torch.no_grad()
@pytest.mark.parametrize("variant,call", ENGINE_CASES, ids=[f"{v}-{c}" for v, c in ENGINE_CASES])
def test_engine_result_does_not_depend_on_workspace_contents(dev, engines, variant, call):
    from reflectionflow_amd import _lib
    case = EngineCase(engines[VARIANTS[variant][3]], variant, dev)
    assert case.applies(call)
    i = case.inputs(seed=1)
    outs = {}
    for kind in PATTERNS:
        w = case.workspace()                                     # a fresh buffer per run: nothing but the pattern is in it
        assert w.fill(kind, seed=3) == case.total - 4096
        outs[kind] = w.call(lambda ws: case.run(call, i, ws))
        if variant.startswith("s256") and call in ("double", "single"):
            path = _lib.load().rf_debug_last_attn_path()
            assert path not in (1, 2), f"S = 256 with the engine's score bound should run a shift-free kernel, ran path {path}"
    assert_live(outs["zero"], f"{call}[{variant}]")
    for kind in POISONS:
        assert_same_bits(outs[kind], outs["zero"], f"{call}[{variant}] on a workspace filled with '{kind}'")


@torch.no_grad()
@pytest.mark.parametrize("variant", ["s83", "s147-bias", "s256", "s65"])
def test_engine_sequence_on_one_workspace(dev, engines, variant):
    """The production pattern across denoise steps and search rounds: ONE workspace, inputs A (8 x the activation scale) and then
    inputs B.  B must come out as on a fresh zero workspace, whatever A left behind."""
    case = EngineCase(engines[False], variant, dev)
    a, b = case.inputs(seed=2, scale=8.0), case.inputs(seed=1)
    for call in CALLS:
        if not case.applies(call):
            continue
        fresh, used = case.workspace(), case.workspace()
        want = fresh.call(lambda ws: case.run(call, b, ws))
        used.call(lambda ws: case.run(call, a, ws))
        got = used.call(lambda ws: case.run(call, b, ws))
        assert_live(want, f"{call}[{variant}]")
        assert_same_bits(got, want, f"{call}[{variant}] after a call with other, larger inputs on the same workspace")


# =====================================================================================================================
# b. attention forward, kernel level
# =====================================================================================================================
SENTINEL = -12345.0


def poison_pad_rows(q, k, vt, S, kind, seed):
    """rows S .. s_pad of q and k and the pad key columns of the V^T tiles <- pattern (the live rows / columns stay)"""
    H, s_pad = q.shape[0], q.shape[1]
    n = s_pad - S
    if n == 0:
        return
    for t, sd in ((q, 1), (k, 2)):
        t[:, S:] = pattern_words(kind, H * n * 128, q.device, seed + sd).view(BF).reshape(H, n, 128)
    kv = torch.arange(S, s_pad, device=q.device)
    pos = (kv & ~63) | (kv & 51) | ((kv & 4) << 1) | ((kv & 8) >> 1)          # the V^T tiles' key permutation (make_qkv)
    # (two index tensors around a slice: the indexed view is [n][H][128])
    vt[:, pos // 64, :, pos % 64] = pattern_words(kind, H * n * 128, q.device, seed + 3).view(BF).reshape(n, H, 128)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("S", [65, 100, 127, 191])
@pytest.mark.parametrize("kernel", ["RF_ATTN_ONLINE128", "RF_ATTN_ONLINE256"])
def test_attention_pad_rows_do_not_reach_the_output(dev, kernel, S, mode):
    """rf_attention's contract for rows / keys >= S is "finite": both finite patterns must give the zero-pad result, write nothing
    outside [S][heads * 128] of an out with a wider pitch, and leave the lse rows >= S alone."""
    from reflectionflow_amd import _lib, ops
    from tests.test_kernels_gpu import make_qkv
    H = 2
    n_main = S - S // 3
    res = {}
    for kind in ("zero", "stale", "extreme"):
        q, k, vt, _, _, _ = make_qkv(H, S, dev, seed=S + mode)
        poison_pad_rows(q, k, vt, S, kind, seed=7)
        for want_lse in (True, False):
            buf = torch.full((S, H * 128 + 8), 7.0, dtype=BF, device=dev)          # ldo = heads * 128 + 8
            lse = torch.full((H, q.shape[1]), SENTINEL, device=dev) if want_lse else None
            with ops.attn_kernel(getattr(_lib, kernel)):
                ops.attention(q, k, vt, S, out=buf[:, :H * 128], n_main=n_main, mode=mode, cross_bias=math.log(1.5), lse=lse)
            torch.cuda.synchronize()
            assert _lib.load().rf_debug_last_attn_path() == (1 if kernel == "RF_ATTN_ONLINE128" else 2)
            assert (buf[:, H * 128:] == 7.0).all(), f"'{kind}': the gap columns of out were written"
            if want_lse:
                assert (lse[:, S:] == SENTINEL).all(), f"'{kind}': lse rows >= S were written"
                res[kind] = (buf[:, :H * 128].clone(), lse[:, :S].clone())
            else:
                assert torch.equal(bits(buf[:, :H * 128]), bits(res[kind][0])), f"'{kind}': out differs with and without lse"
    assert_live(res["zero"][0], "attention out")
    assert_live(res["zero"][1], "attention lse")
    for kind in ("stale", "extreme"):
        assert_same_bits(res[kind][0], res["zero"][0], f"{kernel} S={S} mode {mode}: out with '{kind}' pad rows")
        assert torch.equal(res[kind][1].view(torch.int32), res["zero"][1].view(torch.int32)), f"{kernel} S={S} mode {mode}: lse with '{kind}' pad rows"


@pytest.mark.parametrize("kernel", ["RF_ATTN_BOUNDED16_SPLIT", "RF_ATTN_LAGGED16_SPLIT"])
def test_attention_split_launch_does_not_depend_on_its_scratch(dev, kernel):
    from reflectionflow_amd import _lib, ops
    from tests.test_kernels_gpu import make_qkv
    # the smallest shape the split launch accepts: heads % 8 == 0 and (heads / 8) (S / 256)^2 >= 2 (CUs / 8)
    P = torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8
    H, nq = 8, 1
    while nq * nq < 2 * (P // 8):
        nq += 1
    S = 256 * nq                                                              # 2048 on a 256-CU part
    q, k, vt, qf, kf, _ = make_qkv(H, S, dev, seed=11, qscale=0.1)           # q "prescaled": the scores are q . k as they are
    bound = 1.02 * float(torch.matmul(qf.float(), kf.float().transpose(1, 2)).abs().max())
    assert 0 < bound <= 100.0                                                 # what the bounded kernel needs proven
    scratch = ops.attn_scratch(dev)
    raw = scratch.view(torch.uint8)
    outs = {}
    for kind in PATTERNS:
        fill_bytes(raw, 0, raw.numel(), kind, seed=5)                         # attention scratch has no flag page: all of it
        with ops.attn_kernel(getattr(_lib, kernel)):
            outs[kind] = ops.attention(q, k, vt, S, q_prescaled=True, score_bound=bound)
        torch.cuda.synchronize()
        assert _lib.load().rf_debug_last_attn_path() == (6 if kernel == "RF_ATTN_BOUNDED16_SPLIT" else 9)
    assert_live(outs["zero"], kernel)
    for kind in POISONS:
        assert_same_bits(outs[kind], outs["zero"], f"{kernel} S={S} on scratch filled with '{kind}'")


# =====================================================================================================================
# c. GEMM scratch: the partial tiles of a forced stream-K launch
# =====================================================================================================================
@pytest.fixture
def force_sk(dev):
    from tests.pins import pins
    pins.tile(256)
    pins.sk(1)
    yield pins
    pins.reset()


def _run_on_partials(dev, pins, launch, what):
    """launch(splitk_ws) -> tensors, on a scratch whose partial region (bytes 4096 .. end) holds each pattern"""
    ws = torch.zeros(1024 + (16 << 20), dtype=torch.float32, device=dev)
    raw = ws.view(torch.uint8)
    outs = {}
    for kind in PATTERNS:
        fill_bytes(raw, 4096, raw.numel(), kind, seed=9)
        torch.cuda.synchronize()
        assert not bool(ws[:1024].any()), "flag page not zero before the launch"
        outs[kind] = [t.clone() for t in launch(ws)]
        torch.cuda.synchronize()
        assert pins.last_path() == 2, "the launch did not take the stream-K schedule"
        assert not bool(ws[:1024].any()), "the launch left the flag page non-zero"
    for j, base in enumerate(outs["zero"]):
        assert_live(base, f"{what}[{j}]")
        for kind in POISONS:
            assert_same_bits(outs[kind][j], base, f"{what}[{j}] with '{kind}' partial tiles")


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8a8"])
def test_stream_k_gate_res_does_not_depend_on_its_partials(dev, force_sk, w8):
    """the smallest case of test_gemm_stream_k_gate_res: 48 tiles, every tile cut in ~5 pieces.  fp8 K-tiles are 128 elements wide, and
    the plan declines a launch with < 4 K-tiles per worker (48 tiles x 16 K-tiles over 256 workers = 3): the fp8 launch takes the same
    M and N with K = 8192 (64 K-tiles per tile, 12 per worker)."""
    from reflectionflow_amd import ops
    M, N, K = 1500, 2048, (8192 if w8 else 2048)
    x, W = rnd(M, K, dev=dev, seed=1), rnd(N, K, dev=dev, seed=2, scale=0.05)
    b, gate, res = rnd(N, dev=dev, seed=3), rnd(N, dev=dev, seed=4), rnd(M, N, dev=dev, seed=5)
    if w8:
        (A8, sa), (W8, sw) = ops.quant_rows_fp8(x), ops.quantize_weight_fp8(W)

    def launch(ws):
        out = torch.empty(M, N, dtype=BF, device=dev)
        if w8:
            ops.gemm_w8a8([ops.Group([ops.Seg(A8, W8)], bias=b, out=out, residual=res, gate=gate, a_scale=sa, w_scale=sw)], N,
                          ops.RF_EPI_GATE_RES, splitk_ws=ws)
        else:
            ops.gemm([ops.Group([ops.Seg(x, W)], bias=b, out=out, residual=res, gate=gate)], N, ops.RF_EPI_GATE_RES, splitk_ws=ws)
        return [out]

    _run_on_partials(dev, force_sk, launch, "stream-K gate_res " + ("w8a8" if w8 else "bf16"))


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8a8"])
def test_stream_k_qkv_fused_does_not_depend_on_its_partials(dev, force_sk, w8):
    """the shape of test_gemm_stream_k_qkv_fused: text / image / condition groups under the fused QKV + RMSNorm + RoPE epilogue
    (fp8: K = 6144 instead of 3072, for the same reason as above: 42 tiles x 24 K-tiles of 128 leave 3.9 per worker)"""
    from reflectionflow_amd import ops
    H, St, Si, Sc, K = 4, 512, 1024, 256, (6144 if w8 else 3072)
    D, S = H * 128, St + Si + Sc
    g = torch.Generator().manual_seed(6)
    cos, sin = torch.rand(S, 128, generator=g).to(dev), torch.rand(S, 128, generator=g).to(dev)
    groups = []
    for gi, (M, off) in enumerate([(St, 0), (Si, St), (Sc, St + Si)]):
        x, W, b = rnd(M, K, dev=dev, seed=gi), rnd(3 * D, K, dev=dev, scale=0.05, seed=10 + gi), rnd(3 * D, dev=dev, seed=20 + gi)
        nq, nk = rnd(128, dev=dev, seed=30 + gi) + 1.0, rnd(128, dev=dev, seed=40 + gi) + 1.0
        kw = dict(bias=b, tok_offset=off, norm_q=nq, norm_k=nk)
        if w8:
            (A8, sa), (W8, sw) = ops.quant_rows_fp8(x), ops.quantize_weight_fp8(W)
            groups.append(ops.Group([ops.Seg(A8, W8)], a_scale=sa, w_scale=sw, **kw))
        else:
            groups.append(ops.Group([ops.Seg(x, W)], **kw))

    def launch(ws):
        q, k, vt, s_pad = ops.alloc_attn_operands(H, S, dev)
        (ops.gemm_w8a8 if w8 else ops.gemm)(groups, 3 * D, ops.RF_EPI_QKV, q=q, k=k, vt=vt, heads=H, s_pad=s_pad, rope=(cos, sin),
                                            q_scale=ops.QK_PRESCALE, splitk_ws=ws)
        return [q, k, vt]

    _run_on_partials(dev, force_sk, launch, "stream-K fused QKV " + ("w8a8" if w8 else "bf16"))


# =====================================================================================================================
# d. text, CLIP and vision towers
# =====================================================================================================================
def _t5(dev):
    from oracle import text_oracle as TO
    from reflectionflow_amd.flux.text_hip import HipT5Encoder
    from tests.test_text_gpu import bf16_round
    enc = HipT5Encoder(bf16_round(TO.synthetic_t5_state(128, 256, 64, 4, 512, 2, 11)), 4, dev)
    ids = torch.randint(0, 128, (2, 77), generator=torch.Generator().manual_seed(1)).to(dev)
    return enc, lambda: [enc.encode(ids)]


def _clip_text(dev, hidden, heads, head_dim, act):
    from oracle import text_oracle as TO
    from reflectionflow_amd.flux.text_hip import HipClipTextEncoder
    from tests.test_text_gpu import bf16_round
    sd = bf16_round(TO.synthetic_clip_state(128, hidden, heads, 2 * hidden, 2, 77, 21))
    enc = HipClipTextEncoder({"text_model." + k: v for k, v in sd.items()}, heads, dev, head_dim=head_dim, act=act)
    ids = torch.randint(3, 126, (2, 77), generator=torch.Generator().manual_seed(2))
    ids[0, 25:], ids[1, 76:] = 127, 127
    ids = ids.to(dev)
    return enc, lambda: list(enc.encode(ids, pool_in_library=True))


def _vision(dev, cfg, seed):
    from reflectionflow_amd.flux.text_hip import HipClipVisionEncoder
    from reflectionflow_amd.tts import clip_verifier as CV
    from tests import clip_h_ref as HR
    sd, v = HR.bf16_round(CV.synthetic_clip_state(cfg, seed)), cfg["vision"]
    enc = HipClipVisionEncoder({k: x for k, x in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}, v["heads"], dev,
                               head_dim=v["hidden"] // v["heads"], act=cfg.get("act", "quick_gelu"), image_size=v["image_size"])
    patches = enc.alloc_patches(2)
    patches.copy_(rnd(*patches.shape, dev=dev, seed=3))
    return enc, lambda: [enc.encode(patches)]


def _tower(name, dev):
    from reflectionflow_amd.tts import clip_verifier as CV
    from tests import clip_h_ref as HR
    if name == "t5-hd64":
        return _t5(dev)
    if name == "clip_text-hd64":
        return _clip_text(dev, 256, 4, 64, "quick_gelu")
    if name == "clip_text-hd80":
        return _clip_text(dev, 160, 2, 80, "gelu")
    cfg = {"vision-hd64": CV.TINY, "vision-hd80": HR.HD80, "vision-hd64-streamed": CV.TINY_336}[name]
    return _vision(dev, cfg, 2)


@torch.no_grad()
@pytest.mark.parametrize("name", ["t5-hd64", "clip_text-hd64", "clip_text-hd80", "vision-hd64", "vision-hd80", "vision-hd64-streamed"])
def test_tower_result_does_not_depend_on_workspace_contents(dev, name):
    """B = 2 sequences whose token count is no multiple of 32 (77 in 96 rows, 257 in 288, 577 in 608): sequence 0's pad rows lie
    between live rows.  The tower owns those rows, so it must make them harmless by itself."""
    from reflectionflow_amd import _lib
    enc, run = _tower(name, dev)
    if name.startswith("vision"):
        assert enc.tokens < enc.s_pad and (enc.s_pad > 512) == name.endswith("streamed")
    base = run()                                                  # allocates the tower's zero-filled workspace: the baseline
    torch.cuda.synchronize()
    buf = enc._ws.buf
    w = Workspace(buf.numel(), _lib.text_workspace_layout(buf.numel())["sk_flags"], dev, buf=buf)
    for j, t in enumerate(base):
        assert_live(t, f"{name}[{j}]")
    for kind in POISONS:
        assert w.fill(kind, seed=4) == buf.numel() - 4096
        got = w.call(lambda ws: run())
        assert enc._ws.buf is buf, "the tower changed its workspace between two calls of one geometry"
        for j, t in enumerate(got):
            assert_same_bits(t, base[j], f"{name}[{j}] on a workspace filled with '{kind}'")
