"""CPU: the host-side statements the on-device round hand-off of the reflection search rests on (csrc/image_handoff.hip,
flux/image_hip.py, Condition(moments=...)).

  * tests/pil_resize_ref.py (integer restatement of Pillow's 8-bit bicubic resampler) == PIL.Image.resize, exactly, saturated regions
    included; the product's coefficient tables (flux/image_hip.py pil_resize_tables, what the kernel reads) are those of the restatement;
  * the 256-entry encoder-input table == VaeImageProcessor.preprocess(...).to(bf16);
  * Condition(moments=...).encode == encode_images on a pipeline whose vae.encode returns those moments, same generator seed, bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import pil_resize_ref as PR

BF = torch.bfloat16


@pytest.mark.parametrize("src,dst", PR.SIZES)
def test_restatement_equals_pil_resize(src, dst):
    from PIL import Image
    (H, W), (h, w) = src, dst
    lv = PR.synthetic_levels(H * 3 + W + h, H, W)
    want = np.asarray(Image.fromarray(lv).resize((w, h)))
    stats = {}
    got = PR.resize(lv, h, w, stats)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"  {H}x{W} -> {h}x{w}: max |d| = {int(d.max())}, sums changed by the clip: {stats.get('clipped', 0)}")
    assert got.shape == want.shape == (h, w, 3)
    assert int(d.max()) == 0
    assert (src == dst) or stats["clipped"] > 0                                                 # the clip is exercised


@pytest.mark.parametrize("n_in,n_out", [(1024, 512), (2048, 512), (768, 512), (1000, 384), (256, 512), (1360, 512), (37, 64), (4096, 224)])
def test_product_tables_are_the_restatements(n_in, n_out):
    from reflectionflow_amd.flux.image_hip import pil_resize_tables
    lo, n, coef = pil_resize_tables(n_in, n_out)
    ref = PR.axis_coeffs(n_in, n_out)
    assert lo.dtype == n.dtype == coef.dtype == np.int32
    assert coef.shape == (PR.max_taps(n_in, n_out), n_out) and coef.flags["C_CONTIGUOUS"]         # tap-major, Pillow's ksize
    assert lo.tolist() == [r[0] for r in ref] and n.tolist() == [len(r[1]) for r in ref]
    for i, (_, k) in enumerate(ref):
        assert coef[: len(k), i].tolist() == k and not coef[len(k):, i].any(), i
    assert int((lo + n).max()) <= n_in and int(lo.min()) >= 0 and int(n.min()) >= 1
    assert pil_resize_tables(n_in, n_out)[2] is coef                                            # cached per (in, out)


def test_vae_input_table_equals_preprocess():
    from PIL import Image
    from reflectionflow_amd.flux.image_hip import vae_input_table
    from reflectionflow_amd.flux.vae import VaeImageProcessor
    lv = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)                      # every level once, 16 x 16 RGB
    want = VaeImageProcessor(16).preprocess(Image.fromarray(lv)).to(BF)[0, 0].reshape(-1)
    got = vae_input_table()
    assert got.dtype == BF and got.shape == (256,)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert float(got[0]) == -1.0 and float(got[255]) == 1.0


class _StubVae:
    """vae.encode(x) returns fixed moments, as HipVAE.encode does (DiagonalGaussianDistribution of encode_moments)."""

    class config:
        shift_factor, scaling_factor = 0.1159, 0.3611

    def __init__(self, moments):
        self.moments, self.calls = moments, 0

    def encode(self, x):
        from reflectionflow_amd.flux.vae import AutoencoderKLOutput, DiagonalGaussianDistribution
        self.calls += 1
        return AutoencoderKLOutput(DiagonalGaussianDistribution(self.moments[None]))


def _stub_pipe(moments):
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    from reflectionflow_amd.flux.vae import VaeImageProcessor

    class P:
        device, dtype = torch.device("cpu"), BF
        image_processor = VaeImageProcessor(16)
        _pack_latents = staticmethod(FluxPipeline._pack_latents)
        _prepare_latent_image_ids = staticmethod(FluxPipeline._prepare_latent_image_ids)
    p = P()
    p.vae = _StubVae(moments)
    return p


def test_condition_from_moments_equals_encode_images():
    from PIL import Image
    from reflectionflow_amd.flux.condition import Condition
    g = torch.Generator().manual_seed(3)
    moments = torch.cat([torch.randn(16, 8, 8, generator=g), torch.randn(16, 8, 8, generator=g) * 3.0 - 2.0]).to(BF)   # mean | logvar
    moments[16, 0, 0], moments[17, 0, 0] = 40.0, -50.0                                          # beyond the clamp [-30, 20]
    pipe = _stub_pipe(moments)
    img = Image.fromarray(PR.synthetic_levels(1, 64, 64))
    for seed in (0, 7):
        host = Condition("cot", condition=img, position_delta=[0, -4]).with_generator(torch.Generator().manual_seed(seed))
        devc = Condition("cot", moments=moments, position_delta=[0, -4]).with_generator(torch.Generator().manual_seed(seed))
        calls = pipe.vae.calls
        t0, i0, k0 = host.encode(pipe)
        assert pipe.vae.calls == calls + 1
        t1, i1, k1 = devc.encode(pipe)
        assert pipe.vae.calls == calls + 1                                                      # moments=: no encoder call
        assert t1.shape == t0.shape == (1, 16, 64) and t1.dtype == t0.dtype == BF
        assert torch.equal(t0.view(torch.int16), t1.view(torch.int16)) and torch.equal(i0, i1) and torch.equal(k0, k1)
    a = Condition("cot", moments=moments).with_generator(torch.Generator().manual_seed(0)).encode(pipe)[0]
    b = Condition("cot", moments=moments).with_generator(torch.Generator().manual_seed(7)).encode(pipe)[0]
    assert not torch.equal(a, b)                                                                # the posterior IS sampled per child
    with pytest.raises(AssertionError):
        Condition("cot", moments=moments, tokens=a, ids=torch.zeros(16, 3))


def test_binding_declares_the_handoff_entry_points():
    from reflectionflow_amd import _lib
    from tests.test_abi_cpu import header_functions
    for name in ("rf_image_levels", "rf_pil_resize_to_vae_input"):
        assert name in _lib.declared_symbols() and name in header_functions()
    assert _lib.ABI_VERSION == 17


def test_handoff_entry_points_validate_arguments():
    import ctypes as C
    import os
    from reflectionflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.rf_abi_version() == 17
    assert lib.rf_image_levels(None, 0, 1, 1, 1, 1, 8, 8, None, None) == -3
    assert lib.rf_image_levels(256, 0, 80, 8, 1, 1, 8, 9000, 256, None) == -1 and b"W=9000" in lib.rf_last_error()
    assert lib.rf_image_levels(256, 0, 80, 8, 1, 1, 8, 8, 258, None) == -2
    n = C.c_void_p(256)
    args = lambda **k: [k.get("levels", 256), 1, 16, 16, 8, 8, k.get("xlo", n), n, n, k.get("kx", 9), n, n, n, 9, 256, k.get("scratch", 256), 256, 256,  # noqa: E731
                        k.get("s_halo", 100 * 64), k.get("cpad", 64), None]
    assert lib.rf_pil_resize_to_vae_input(*args(levels=None)) == -3
    assert lib.rf_pil_resize_to_vae_input(*args(xlo=None)) == -3 and b"x tables" in lib.rf_last_error()
    assert lib.rf_pil_resize_to_vae_input(*args(kx=10)) == -1 and b"kx=10" in lib.rf_last_error()
    assert lib.rf_pil_resize_to_vae_input(*args(scratch=None)) == -3 and b"scratch" in lib.rf_last_error()
    assert lib.rf_pil_resize_to_vae_input(*args(s_halo=99 * 64)) == -1                            # smaller than one halo image
    assert lib.rf_pil_resize_to_vae_input(*args(cpad=12)) == -1
