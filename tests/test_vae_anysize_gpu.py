"""GPU: the VAE at geometries whose bottleneck holds a token count that is no multiple of 64 -- vae_attn_kernel<true> of csrc/vae.hip (the
key tail masked in the last 32-key tile) alone (RF_VAE_OP_ATTN_CORE_RAGGED), inside the mid-block attention (RF_VAE_OP_ATTN_BLOCK_RAGGED),
inside whole decoders / encoders (rf_vae_decode / rf_vae_encode through HipVAE) and at the pipeline's call sites.

References and bounds are the existing ones, as they stand: fp64 on the CPU from the same bf16 operands under
tests/test_kernels_gpu.py::assert_close (elementwise 1.2e-2 |ref| + 1.2e-2 mean|ref|, rel-L2 < 4e-3) for the ops
(tests/test_vae_anysize_cpu.py holds the fp32 yardsticks to the same bound on the same inputs); oracle/vae_oracle.py under
rel-L2(hip) <= 2 rel-L2(torch bf16 on the CPU) + 2e-3 for whole VAEs (tests/test_vae_gpu.py); "exact" = torch.equal.
qk has S_pad = round_up(S, 64) rows and vt a row pitch of S_pad: the rows / columns from S on are PAD, and no result may depend on what
they hold -- every core case runs with the pad zero, filled with byte 0x7F (3.4e38) and filled with byte 0xFF (NaN), the three outputs
bit-equal.  Outputs are prefilled with a NaN pattern and followed by sentinels (the guard starts right behind row S - 1); inputs are
compared byte for byte after every call, their own guard included."""
import pytest
import torch

from tests import vae_anysize_cases as A
from tests import vae_kernel_cases as K
from tests.test_kernels_gpu import assert_close
from tests.test_vae_gpu import MID, bf16_state, make_vae, rel_l2
from tests.test_vae_kernels_gpu import PRE, Buf, padded, run_op

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PADS = (0x00, 0x7F, 0xFF)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reflectionflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def pad_words(byte, *shape):
    return torch.full(shape, byte * 0x0101 - (0x10000 if byte >= 0x80 else 0), dtype=torch.int16).view(BF)


def ragged_core(dev, q, k, v, pad=0x00, k_pad=None, v_pad=None):
    """RF_VAE_OP_ATTN_CORE_RAGGED on q, k, v [S][512] -> out [S][512] (CPU).  Pad rows of qk / pad columns of vt: every byte `pad`, or the K
    row `k_pad` / the V value `v_pad`."""
    from reflectionflow_amd import _lib as L
    S, Sp = q.shape[0], A.s_pad(q.shape[0])
    qk = pad_words(pad, Sp, 1024)
    qk[:S, :512], qk[:S, 512:] = q, k
    vt = pad_words(pad, 512, Sp)
    vt[:, :S] = v.T
    if k_pad is not None:
        qk[S:, 512:] = k_pad
    if v_pad is not None:
        vt[:, S:] = v_pad
    bq, bv, out = Buf(dev, Sp * 1024, qk), Buf(dev, 512 * Sp, vt), Buf(dev, S * 512)
    before = bq.full.view(torch.int16).clone(), bv.full.view(torch.int16).clone()
    run_op(dev, L.RF_VAE_OP_ATTN_CORE_RAGGED, 1, S, 512, inp=bq.ptr, residual=bv.ptr, out=out.ptr)
    what = f"ragged attention core S={S} pad={pad:#x}"
    out.assert_guard(what)
    assert torch.equal(bq.full.view(torch.int16), before[0]), f"{what}: qk changed"
    assert torch.equal(bv.full.view(torch.int16), before[1]), f"{what}: vt changed"
    return out.t.cpu().view(S, 512)


def assert_bits(got, want, what):
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = got.view(torch.int16) != want.view(torch.int16)
        rows = torch.nonzero(bad.any(1)).flatten()[:8].tolist()
        cols = torch.nonzero(bad.any(0)).flatten()[:16].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ ({int(torch.isnan(got.float()).sum())} NaN); first rows {rows}, "
                             f"first channels {cols}")


# ---- 1. core vs fp64, pad contents ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", K.ATTN_FORMS)
@pytest.mark.parametrize("S", A.CORE_S)
def test_ragged_core_vs_fp64(dev, S, form):
    q, k, v = K.attn_inputs(form, S)
    ref = K.attn_ref64(q, k, v)
    got = ragged_core(dev, q, k, v, PADS[0])
    r = assert_close(got, ref, f"vae_attn_kernel<true> {form} S={S}")
    ry = float((K.attn_yardstick(q, k, v).double() - ref).norm() / ref.norm())
    print(f"  ragged attn core {form} S={S}: rel-L2 {r:.2e} (yardstick {ry:.2e})")
    for pad in PADS[1:]:
        assert_bits(ragged_core(dev, q, k, v, pad), got, f"{form} S={S}: pad bytes {pad:#x} change the result")


# ---- 2. routing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", A.CORE_S)
def test_ragged_core_routing_is_bit_exact(dev, S):
    """one key per query carries all the weight, query 0 picks the last real key: a tail key dropped with the pad, a mask shifted by one
    lane group or a V^T column read at the pitch S moves a row of v somewhere else -- nothing averages away"""
    q, k, v, pi, c = A.ragged_routing_inputs(S)
    assert_bits(ragged_core(dev, q, k, v, 0xFF), v[pi], f"routing S={S}")


# ---- 3. pad keys that would win ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", A.CORE_S)
def test_ragged_core_masks_pad_keys_that_would_win(dev, S):
    """every pad K row scores as high as the query's one hit, every pad V is 1000: a pad key that reaches the softmax takes half a row or
    more (tests/test_vae_anysize_cpu.py::test_ragged_routing_is_exact_in_fp32 shows it on the yardstick)"""
    q, k, v, pi, c = A.ragged_routing_inputs(S)
    assert_bits(ragged_core(dev, q, k, v, 0x00, k_pad=A.winning_pad_key(c), v_pad=1000.0), v[pi], f"winning pad keys S={S}")


# ---- 4. workgroups -----------------------------------------------------------------------------------------------------------------------
def test_ragged_core_workgroup_invariance(dev):
    """S = 129: workgroups of 64, 64 and ONE query; the rows of workgroup b do not depend on what the other workgroups' queries hold"""
    S = 129
    q, k, v = K.attn_inputs("plain", S)
    full = ragged_core(dev, q, k, v, 0xFF)
    assert_close(full, K.attn_ref64(q, k, v), "S=129")
    for b in range(3):
        rows = slice(64 * b, min(64 * b + 64, S))
        qb = torch.zeros_like(q)
        qb[rows] = q[rows]
        assert_bits(ragged_core(dev, qb, k, v, 0xFF)[rows], full[rows], f"workgroup {b}")


# ---- 5. the attention block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", A.BLOCK_HW)
def test_ragged_attn_block_vs_fp64(dev, H, W):
    from reflectionflow_amd import _lib as L
    from reflectionflow_amd.flux.vae_hip import _Packer
    m, x = K.block_module(), K.block_input(H, W)
    p, a = _Packer(dev), L.rf_vae_attn()
    p.attn(a, m)
    start = padded(x, float("nan")).view(torch.int16).clone()
    img = start.view(H + 2, W + 2, 512)
    ring = torch.ones(H + 2, W + 2, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    img[ring] = PRE
    buf = Buf(dev, start.numel(), start.view(BF))
    run_op(dev, L.RF_VAE_OP_ATTN_BLOCK_RAGGED, H, W, 512, out=buf.ptr, attn=a)          # (run_op: every workspace word a NaN)
    what = f"ragged attention block {H}x{W}"
    buf.assert_guard(what)
    got = buf.t.cpu().view(H + 2, W + 2, 512)
    assert bool((got.view(torch.int16)[ring] == PRE).all()), f"{what}: the halo of the in-place image changed"
    ref = K.block_ref64(m, x)
    r = assert_close(got[1:-1, 1:-1], ref, what)
    ry = float((K.block_yardstick(m.float(), x).double() - ref).norm() / ref.norm())
    print(f"  {what}: rel-L2 {r:.2e} (yardstick {ry:.2e})")


def test_ragged_ops_run_the_whole_tile_kernel_at_multiples_of_64(dev):
    """S % 64 == 0 through op 6 is op 4's launch: bit-equal"""
    from reflectionflow_amd import _lib as L
    q, k, v = K.attn_inputs("plain", 128)
    outs = []
    for op in (L.RF_VAE_OP_ATTN_CORE, L.RF_VAE_OP_ATTN_CORE_RAGGED):
        bq, bv, out = Buf(dev, 128 * 1024, torch.cat([q, k], 1)), Buf(dev, 512 * 128, v.T.contiguous()), Buf(dev, 128 * 512)
        run_op(dev, op, 2, 64, 512, inp=bq.ptr, residual=bv.ptr, out=out.ptr)
        out.assert_guard("S=128")
        outs.append(out.t.cpu())
    assert_bits(outs[1].view(128, 512), outs[0].view(128, 512), "op 6 vs op 4 at S=128")


# ---- 6. whole VAEs -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid_dec(dev):
    """fp32 weights as the bf16 modules hold them (the oracle's), the eager bf16 module on the CPU (the yardstick), the HIP VAE"""
    from reflectionflow_amd.flux.vae_hip import HipVAE
    return bf16_state(make_vae(MID, seed=3)), make_vae(MID, seed=3).to(BF), HipVAE(make_vae(MID, seed=3).to(dev).to(BF))


@pytest.fixture(scope="module")
def mid_enc(dev):
    from reflectionflow_amd.flux.vae_hip import HipVAE
    return bf16_state(make_vae(MID, seed=4)), make_vae(MID, seed=4).to(BF), HipVAE(make_vae(MID, seed=4).to(dev).to(BF))


@torch.no_grad()
@pytest.mark.parametrize("h,w", [(5, 7), (9, 9), (3, 43)])
def test_decode_vs_oracle_ragged(dev, mid_dec, h, w):
    from oracle import vae_oracle as VO
    sd, mb, hv = mid_dec
    z = torch.randn(1, 16, h, w, generator=torch.Generator().manual_seed(h * 100 + w))
    ref = VO.vae_decode(sd, z.to(BF).float(), groups=MID["norm_num_groups"])
    tb = mb.decode(z.to(BF)).sample
    out = hv.decode(z.to(dev).to(BF)).sample
    out2 = hv.decode(z.to(dev).to(BF)).sample
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 4 * h, 4 * w) and torch.isfinite(out.float()).all()
    assert torch.equal(out, out2), "decode is not bit-stable run to run"
    e_hip, e_t = rel_l2(out, ref), rel_l2(tb, ref)
    print(f"  decode mid {h}x{w}: hip {e_hip:.3e}  torch-bf16 {e_t:.3e}")
    assert e_hip <= 2.0 * e_t + 2e-3, (e_hip, e_t)


@torch.no_grad()
@pytest.mark.parametrize("H,W", [(20, 28), (36, 36), (12, 172)])
def test_encode_vs_oracle_ragged(dev, mid_enc, H, W):
    from oracle import vae_oracle as VO
    sd, mb, hv = mid_enc
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H + W)) * 2 - 1
    ref = VO.vae_encode_moments(sd, x.to(BF).float(), groups=MID["norm_num_groups"])
    tb = mb.encoder(x.to(BF))
    mo = hv.encode_moments(x.to(dev).to(BF))
    mo2 = hv.encode_moments(x.to(dev).to(BF))
    torch.cuda.synchronize()
    assert mo.shape == ref.shape == (1, 32, H // 4, W // 4) and torch.isfinite(mo.float()).all()
    assert torch.equal(mo, mo2), "encode is not bit-stable run to run"
    e_hip, e_t = rel_l2(mo, ref), rel_l2(tb, ref)
    print(f"  encode mid {H}x{W}: hip {e_hip:.3e}  torch-bf16 {e_t:.3e}")
    assert e_hip <= 2.0 * e_t + 2e-3, (e_hip, e_t)


@torch.no_grad()
@pytest.mark.parametrize("what,h,w", [("decode", 5, 7), ("encode", 36, 36)])
def test_ragged_result_does_not_depend_on_workspace_contents(dev, what, h, w):
    """the pad rows of q | k and the pad columns of V^T live in the caller's workspace and are never written: a zeroed workspace, one of
    3.4e38 (byte 0x7F) and one of NaN (byte 0xFF) give bit-equal results"""
    from reflectionflow_amd.flux.vae_hip import HipVAE
    hv = HipVAE(make_vae(MID, seed=6).to(dev).to(BF))
    g = torch.Generator().manual_seed(h * 7 + w)
    if what == "decode":
        x = torch.randn(1, 16, h, w, generator=g).to(dev).to(BF)
        run = lambda: hv.decode(x).sample.clone()
    else:
        x = (torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(dev).to(BF)
        run = lambda: hv.encode_moments(x).clone()
    base = run()
    assert len(hv._ws) == 1 and torch.isfinite(base.float()).all()
    (ws,) = hv._ws.values()
    for byte in (0x7F, 0xFF):
        ws.fill_(byte)
        got = run()
        torch.cuda.synchronize()
        assert torch.equal(got, base), (f"{what} {h}x{w}: workspace filled with byte {byte:#x} changes the result "
                                        f"({int(torch.isnan(got.float()).sum())} NaN, {int((got != base).sum())} of {got.numel()} elements differ)")


@torch.no_grad()
def test_flux_vae_decode_88x104(dev):
    """the FLUX.1-dev VAE shape at a latent of 11 x 13 = 143 tokens -> 88 x 104 pixels"""
    from oracle import vae_oracle as VO
    from reflectionflow_amd.flux.vae_hip import HipVAE
    m = make_vae({}, seed=5)
    sd = bf16_state(m)
    hv = HipVAE(make_vae({}, seed=5).to(dev).to(BF))
    hv.check_geometry(88, 104)
    z = torch.randn(1, 16, 11, 13, generator=torch.Generator().manual_seed(1))
    ref = VO.vae_decode(sd, z.to(BF).float())
    tb = m.to(BF).decode(z.to(BF)).sample
    out = hv.decode(z.to(dev).to(BF)).sample
    assert out.shape == (1, 3, 88, 104) and torch.isfinite(out.float()).all()
    e_hip, e_t = rel_l2(out, ref), rel_l2(tb, ref)
    print(f"  FLUX VAE decode 88x104: hip {e_hip:.3e}  torch-bf16 {e_t:.3e}")
    assert e_hip <= 2.0 * e_t + 2e-3, (e_hip, e_t)


# ---- 7. call sites -----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_call_sites_take_any_multiple_of_the_scale(dev):
    from reflectionflow_amd.flux.generate import generate
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    from reflectionflow_amd.flux.vae_hip import HipVAE
    from reflectionflow_amd.ops import RFError
    from reflectionflow_amd.tts import runner
    cfgt = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, joint_attention_dim=256, pooled_projection_dim=64)
    pipe = FluxPipeline.synthetic(cfgt, seed=0, torch_dtype=BF, device=dev, with_vae=True, vae_config=MID)
    pipe.set_progress_bar_config(disable=True)
    torch_vae = pipe.vae
    lat = torch.randn(1, 16, 6, 10, generator=torch.Generator().manual_seed(3)).to(dev).to(BF)      # 60 tokens
    ref_img = torch_vae.decode(lat, return_dict=False)[0]
    pipe.enable_hip_vae()
    assert isinstance(pipe.vae, HipVAE)
    pipe.vae.check_geometry(88, 104)
    pipe.vae.check_geometry(1000, 1000)
    with pytest.raises(RFError, match="multiples of"):
        pipe.vae.check_geometry(90, 104)
    img = pipe.vae.decode(lat, return_dict=False)[0]
    assert img.shape == (1, 3, 24, 40) and rel_l2(img, ref_img) < 3e-2
    # a round's candidates (height / width name the FLUX geometry: 48 / 8 x 80 / 8 = 6 x 10 latents; the 3-level test VAE scales by 4)
    packed = pipe._pack_latents(torch.cat([lat, lat * 0.5]), 2, 16, 6, 10)
    batch = runner.decode_candidates(pipe, packed, 48, 80)
    assert batch.shape == (2, 3, 24, 40) and batch.is_cuda and float(batch.min()) >= 0.0 and float(batch.max()) <= 1.0
    # generate(): 96 x 160 -> 12 x 20 = 240 latent pixels, refused before this change
    g = torch.Generator().manual_seed(2)
    kw = dict(model_config={}, height=96, width=160, num_inference_steps=2, guidance_scale=3.5,
              prompt_embeds=torch.randn(1, 16, 256, generator=g).to(dev).to(BF), pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(dev).to(BF))
    out_lat = generate(pipe, output_type="latent", generator=torch.Generator().manual_seed(4), **kw).images
    got = generate(pipe, output_type="pt", generator=torch.Generator().manual_seed(4), **kw).images
    z = pipe._unpack_latents(out_lat, 96, 160, pipe.vae_scale_factor) / pipe.vae.config.scaling_factor + pipe.vae.config.shift_factor
    want = pipe.image_processor.postprocess(torch_vae.decode(z.to(BF), return_dict=False)[0], output_type="pt")
    assert got.shape == want.shape == (1, 3, 48, 80)
    assert rel_l2(got, want) < 3e-2
