"""rf_attention_bwd in the condition modes, the parts that need no device: the refusals of the entry point (validation runs
before any HIP call, so the host alone can see them), the descriptor's layout in C against its ctypes mirror, the SGD branch of
build_optimizer, and the yardstick of tests/attn_bwd_modes_ref.py held to the GPU test's bound at every GPU test shape (the bound
must be attainable by an implementation with the kernels' rounding points before it is asked of the kernels)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest
import torch

from tests import attn_bwd_modes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from reflectionflow_amd import _lib
    return _lib.load()


def _desc(S=200, s_pad=256, heads=2, mode=0, n_main=0, cross_bias=0.0, kernel=0):
    """a descriptor whose pointers are non-NULL and 16-byte aligned but never dereferenced: every call below must fail in validation"""
    from reflectionflow_amd import _lib as L
    buf = C.create_string_buffer(64)
    p = (C.addressof(buf) + 15) // 16 * 16
    d = L.rf_attn_bwd_desc()
    for name in ("q", "k", "v", "qt", "kt", "o", "dout", "dq", "dk", "dv", "dot", "lse", "dsum"):
        setattr(d, name, p)
    d.ldo = d.lddo = heads * 128
    d.heads, d.S, d.s_pad, d.mode, d.lse_given, d.kernel = heads, S, s_pad, mode, 0, kernel
    d.n_main, d.cross_bias = n_main, cross_bias
    d._keep = buf
    return d


def _call(lib, d):
    rc = lib.rf_attention_bwd(C.byref(d), None)
    return rc, lib.rf_last_error().decode()


RF_ERR_SHAPE, RF_ERR_UNSUPPORTED = -1, -5


@pytest.mark.parametrize("mode", [-1, 3, 7])
def test_unknown_mode_is_refused_by_name(lib, mode):
    rc, msg = _call(lib, _desc(mode=mode, n_main=100))
    assert rc == RF_ERR_UNSUPPORTED and f"mode={mode}" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n_main", [0, -5, 200, 4096])
def test_modes_need_both_regions(lib, mode, n_main):
    """0 < n_main < S: every row keeps at least one unmasked key"""
    rc, msg = _call(lib, _desc(mode=mode, n_main=n_main))
    assert rc == RF_ERR_SHAPE and "n_main" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("bias", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_cross_bias_is_refused(lib, mode, bias):
    rc, msg = _call(lib, _desc(mode=mode, n_main=100, cross_bias=bias))
    assert rc == RF_ERR_SHAPE and "cross_bias" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [1, 2])
def test_two_per_cu_dkv_form_is_mode_0_only(lib, mode):
    from reflectionflow_amd import _lib as L
    rc, msg = _call(lib, _desc(mode=mode, n_main=100, kernel=L.RF_ATTN_BWD_DQ_128 | L.RF_ATTN_BWD_DKV_128X2))
    assert rc == RF_ERR_UNSUPPORTED and "128X2" in msg, (rc, msg)


def test_mode_0_ignores_the_new_fields(lib):
    """mode 0 with garbage in n_main / cross_bias passes the mode checks (it fails later, on a deliberately bad kernel request)"""
    rc, msg = _call(lib, _desc(mode=0, n_main=-7, cross_bias=float("nan"), kernel=0x10000))
    assert rc == RF_ERR_UNSUPPORTED and "kernel=0x10000" in msg, (rc, msg)


def test_python_wrapper_signature():
    import inspect
    from reflectionflow_amd.train import kernels as K
    from reflectionflow_amd.train.blocks import BlockOpts
    sig = inspect.signature(K.attention_bwd).parameters
    assert sig["mode"].default == 0 and sig["n_main"].default is None and sig["cross_bias"].default == 0.0
    o = BlockOpts()
    assert (o.latent_lora, o.recompute, o.attn_mode, o.cross_bias, o.add_cond_attn) == (False, True, 0, 0.0, False)


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof(rf_attn_bwd_desc) and the offsets of the two appended fields, as a C compiler sees include/rf_flux.h"""
    from reflectionflow_amd import _lib as L
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else None
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rf_flux.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(rf_attn_bwd_desc), offsetof(rf_attn_bwd_desc, kernel), '
                   'offsetof(rf_attn_bwd_desc, n_main), offsetof(rf_attn_bwd_desc, cross_bias), offsetof(rf_attn_bwd_desc, mode)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_kernel, off_n_main, off_bias, off_mode = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    D = L.rf_attn_bwd_desc
    assert size == C.sizeof(D) == 152
    assert (off_mode, off_kernel) == (D.mode.offset, D.kernel.offset) == (132, 140), "the v17 offsets must not move"
    assert (off_n_main, off_bias) == (D.n_main.offset, D.cross_bias.offset) == (144, 148)
    # additive: fields appended behind everything a v17 caller fills, read only in the modes v17 refused -- the version stays
    assert L.ABI_VERSION == L.load().rf_abi_version() == 17


def test_build_optimizer_knows_sgd():
    """`"SGD"` is the third optimizer of the reference's configure_optimizers (train/model.py:107-117): no "use torch.optim.SGD" error
    any more; on CPU tensors the refusal is the one every flat optimizer gives"""
    from reflectionflow_amd.ops import RFError
    from reflectionflow_amd.train.optim import build_optimizer

    def params():
        return [torch.nn.Parameter(torch.zeros(4, 8, dtype=torch.bfloat16))]
    with pytest.raises(RFError) as e_adamw:
        build_optimizer(params(), {"type": "AdamW"})
    with pytest.raises(RFError) as e_sgd:
        build_optimizer(params(), {"type": "SGD", "params": {"lr": 0.1, "momentum": 0.9}})
    assert "torch.optim.SGD" not in str(e_sgd.value)
    assert str(e_sgd.value) == str(e_adamw.value) and "GPU only" in str(e_sgd.value)
    with pytest.raises(RFError, match="nesterov"):
        build_optimizer(params(), {"type": "SGD", "params": {"nesterov": True}})


def test_trainer_no_longer_refuses_the_switches():
    """FluxTrainer.__init__ carried the refusal; the source must not (constructing a trainer needs a device)"""
    src = open(os.path.join(ROOT, "reflectionflow_amd", "train", "step.py")).read()
    assert "the training path covers the shipped training config" not in src


def test_mask_is_the_reference_blocks():
    m = R.attn_mask(6, 4, 2, 0.0)
    assert torch.isinf(m[:4, 4:]).all() and torch.isinf(m[4:, :4]).all() and (m[:4, :4] == 0).all() and (m[4:, 4:] == 0).all()
    b = R.attn_mask(6, 4, 1, math.log(3.0))
    assert torch.allclose(b[:4, 4:], torch.full((4, 2), math.log(3.0))) and (b[4:, 4:] == 0).all() and (b[:4, :4] == 0).all()
    assert (R.attn_mask(6, 4, 0, 1.0) == 0).all()


def test_transposed_tiles_follow_slot32():
    x = torch.arange(2 * 64 * 128, dtype=torch.float32).view(2, 64, 128)
    t = R.transposed_tiles(x)
    assert t.shape == (2, 2, 128, 32)
    for n in (0, 1, 5, 16, 21, 31, 37, 63):
        assert torch.equal(t[1, n // 32, :, R.slot32(n % 32)], x[1, n])


@pytest.mark.parametrize("name,mode,bias", R.MODES)
@pytest.mark.parametrize("H,S,n_main", R.SHAPES)
def test_yardstick_meets_the_gpu_bound(H, S, n_main, name, mode, bias):
    """fp32 arithmetic with the kernels' rounding points (bf16 P, bf16 g, bf16 outputs) against fp32 autograd: rel-L2 < 1.2e-2 per
    gradient at every shape the GPU test uses.  Measured here: <= 2.6e-3 (printed)."""
    q, k, v, dout = R.synthetic_operands(H, S, seed=S + n_main)
    _, dq, dk, dv, _ = R.reference(q, k, v, dout, mode, n_main, bias)
    yq, yk, yv = R.yardstick(q, k, v, dout, mode, n_main, bias)
    e = [R.rel_l2(yq, dq), R.rel_l2(yk, dk), R.rel_l2(yv, dv)]
    print(f"  yardstick {name} H={H} S={S} n_main={n_main}: rel-L2 dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < R.BOUND, e
    if mode == 2:        # the mask leaks nothing: a main row's gradient is blind to the condition rows' values
        q2, k2, v2 = (t.clone() for t in (q, k, v))
        for t in (q2, k2, v2):
            t[:, n_main:] = 3.0 * t[:, n_main:].flip(1) + 1.0
        _, dq2, dk2, dv2, _ = R.reference(q2, k2, v2, dout, mode, n_main, bias)
        for a, b in ((dq, dq2), (dk, dk2), (dv, dv2)):
            assert torch.allclose(a[:, :n_main], b[:, :n_main], rtol=1e-5, atol=1e-7)
