"""CPU: the image-guided denoise entry points (rf_guided_euler_step, rf_flux_denoise_guided) are declared in
include/rf_flux.h, bound by the ctypes binding, exported by the library, and validate their arguments loudly.  No kernel is
launched: every call below is refused before it reaches a launch."""
import ctypes as C
import os

import pytest

NEW = ("rf_guided_euler_step", "rf_flux_denoise_guided")


@pytest.fixture(scope="module")
def lib():
    from reflectionflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_and_binding_declare_the_guided_entry_points():
    from reflectionflow_amd import _lib
    from tests.test_abi_cpu import header_functions
    for name in NEW:
        assert name in header_functions(), f"{name} is not declared in include/rf_flux.h"
        assert name in _lib.declared_symbols(), f"{name} is not in the ctypes binding"
    assert _lib.ABI_VERSION == 17                    # additive entry points: no struct or signature changed


def test_library_exports_the_guided_entry_points(lib):
    from reflectionflow_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name)


def test_guided_euler_step_validates_arguments(lib):
    ok = 256                                          # a 16-byte aligned (never dereferenced) address
    assert lib.rf_guided_euler_step(None, ok, ok, 64, 1.5, -0.1, None) == -3
    assert lib.rf_guided_euler_step(ok, None, ok, 64, 1.5, -0.1, None) == -3
    assert lib.rf_guided_euler_step(ok, ok, None, 64, 1.5, -0.1, None) == -3
    assert b"rf_guided_euler_step" in lib.rf_last_error()
    for args in ((ok + 2, ok, ok), (ok, ok + 8, ok), (ok, ok, ok + 4)):
        assert lib.rf_guided_euler_step(*args, 64, 1.5, -0.1, None) == -2
    assert b"16-byte" in lib.rf_last_error()
    assert lib.rf_guided_euler_step(None, None, None, 0, 1.5, -0.1, None) == 0       # nothing to do, as rf_euler_step


def _guided_args(lib, **k):
    """A full rf_flux_denoise_guided argument list over placeholder addresses; keyword overrides by name."""
    from reflectionflow_amd import _lib
    dims = _lib.rf_flux_dims()
    dims.D, dims.heads, dims.mlp, dims.S_txt, dims.S_img = 256, 2, 1024, 32, 64
    dims.S_cond = k.pop("S_cond", 16)
    model = _lib.rf_flux_model()
    model.in_ch, model.joint_dim = 64, 256
    ws = _lib.rf_workspace()
    ws.base, ws.bytes = 256, 1 << 30
    dts = (C.c_float * 4)(-0.1, -0.1, -0.1, -0.1)
    p = 256
    a = dict(dims=C.byref(dims), m=C.byref(model), latents=p, cond=p, unc=p, unc_stride=0, ctx=p, mod_main=p, mod_unc=p,
             mod_stride=1024, mod_cond=p, cos=p, sin=p, dts=dts, T=4, scale=1.5, vel=p, unc_scratch=p, ws=C.byref(ws), stream=None)
    assert set(k) <= set(a), set(k) - set(a)
    a.update(k)
    keep = (dims, model, ws, dts)
    return list(a.values()), keep


def test_flux_denoise_guided_validates_arguments(lib):
    for name in ("mod_main", "mod_unc", "mod_cond", "dts", "latents", "vel", "unc_scratch", "cond", "unc", "m", "dims"):
        args, keep = _guided_args(lib, **{name: None})
        assert lib.rf_flux_denoise_guided(*args) == -3, name
        assert b"rf_flux_denoise_guided" in lib.rf_last_error()
    args, keep = _guided_args(lib, T=0)
    assert lib.rf_flux_denoise_guided(*args) == -1 and b"T=0" in lib.rf_last_error()
    args, keep = _guided_args(lib, T=-3)
    assert lib.rf_flux_denoise_guided(*args) == -1
    args, keep = _guided_args(lib, S_cond=0)
    assert lib.rf_flux_denoise_guided(*args) == -1 and b"S_cond=0" in lib.rf_last_error()
