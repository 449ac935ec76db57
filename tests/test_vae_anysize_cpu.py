"""No GPU: the any-size attention of the VAE (token counts that are no multiple of 64).  (1) The yardsticks of tests/vae_kernel_cases.py
-- fp32 restatements that round where the kernels round; attn_yardstick's 32-key loop already slices a ragged last tile -- against fp64
under the bound tests/test_vae_anysize_gpu.py applies to the kernels (tests/test_kernels_gpu.py::assert_close), on every GPU case's
inputs: a correct kernel can meet that bound.  (2) What RF_VAE_OP_ATTN_CORE_RAGGED / RF_VAE_OP_ATTN_BLOCK_RAGGED refuse and answer
before any HIP call.  The figures are recorded in profiles/vae_anysize.md."""
import pytest
import torch

from tests import vae_anysize_cases as A
from tests import vae_kernel_cases as K
from tests.test_kernels_gpu import assert_close
from tests.test_vae_kernels_cpu import ADDR, RF_ERR_NULL, RF_ERR_SHAPE, RF_ERR_UNSUPPORTED, call

CORE_RAGGED, BLOCK_RAGGED = 6, 7


def test_op_numbers():
    from reflectionflow_amd import _lib as L
    assert (L.RF_VAE_OP_ATTN_CORE_RAGGED, L.RF_VAE_OP_ATTN_BLOCK_RAGGED) == (CORE_RAGGED, BLOCK_RAGGED)


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", K.ATTN_FORMS)
@pytest.mark.parametrize("S", A.CORE_S)
def test_attention_yardstick(form, S):
    q, k, v = K.attn_inputs(form, S)
    r = assert_close(K.attn_yardstick(q, k, v), K.attn_ref64(q, k, v), f"attention yardstick {form} S={S}")
    print(f"  attention yardstick {form} S={S}: rel-L2 {r:.2e}")


@pytest.mark.parametrize("S", A.CORE_S)
def test_ragged_routing_is_exact_in_fp32(S):
    q, k, v, pi, c = A.ragged_routing_inputs(S)
    assert torch.equal(K.attn_yardstick(q, k, v), v[pi])
    assert float(v.float().abs().min()) >= 2.0 ** -6
    # ... and a pad key that is NOT masked moves every row: the GPU test's pad rows have teeth
    n = A.s_pad(S) - S
    kp = torch.cat([k, A.winning_pad_key(c)[None].expand(n, -1)])
    vp = torch.cat([v, torch.full((n, K.VA_C), 1000.0, dtype=A.BF)])
    qp = torch.cat([q, torch.zeros(n, K.VA_C, dtype=A.BF)])
    leaked = K.attn_yardstick(qp, kp, vp)[:S]
    assert bool((leaked != v[pi]).any(1).all())


@pytest.mark.parametrize("H,W", A.BLOCK_HW)
def test_attention_block_yardstick(H, W):
    m, x = K.block_module(), K.block_input(H, W)
    r = assert_close(K.block_yardstick(m.float(), x), K.block_ref64(m, x), f"attention block yardstick {H}x{W}")
    print(f"  attention block yardstick {H}x{W}: rel-L2 {r:.2e}")


# ---- refusals and queries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,code,word", [
    (dict(op=CORE_RAGGED, Cc=256, residual=ADDR), RF_ERR_UNSUPPORTED, "built for 512 channels (got 256)"),
    (dict(op=BLOCK_RAGGED, Cc=256), RF_ERR_UNSUPPORTED, "built for 512 channels (got 256)"),
    (dict(op=CORE_RAGGED, H=6, W=8), RF_ERR_NULL, "without vt"),
    (dict(op=BLOCK_RAGGED, H=6, W=8, attn=None), RF_ERR_NULL, "ATTN_BLOCK without attn"),
    (dict(op=BLOCK_RAGGED, H=6, W=8, attn="noweights"), RF_ERR_NULL, "attention weights NULL"),
    (dict(op=BLOCK_RAGGED, H=6, W=8, groups=16), RF_ERR_SHAPE, "GroupNorm over C=512 channels, 16 groups"),
    (dict(op=CORE_RAGGED, H=0, residual=ADDR), RF_ERR_SHAPE, "H=0"),
    (dict(op=BLOCK_RAGGED, H=0), RF_ERR_SHAPE, "H=0"),
    (dict(op=CORE_RAGGED, H=6, W=8, residual=ADDR, out=None), RF_ERR_NULL, "NULL tensor"),
    (dict(op=CORE_RAGGED, H=6, W=8, residual=ADDR + 4), -2, "16-byte"),
    (dict(op=8), RF_ERR_UNSUPPORTED, "op=8"),
])
def test_refusals(kw, code, word):
    rc, msg = call(**kw)
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_whole_tile_ops_still_refuse_a_tail():
    """ops 4 and 5 keep their contract (tests/test_vae_kernels_cpu.py pins the message); 6 and 7 pass the same geometry's validation"""
    for op in (4, 5):
        rc, msg = call(op=op, H=6, W=8, residual=ADDR)
        assert rc == RF_ERR_SHAPE and "attention over 48 tokens (need a multiple of 64)" in msg, (rc, msg)
    for op in (CORE_RAGGED, BLOCK_RAGGED):
        assert call(op=op, H=6, W=8, residual=ADDR, ws_base=None)[0] > 0


def test_workspace_query():
    """ws == NULL: the bytes the op needs.  The ragged block carves q | k and V^T over S_pad = 64 rows / columns at 6 x 8 = 48 tokens: what
    the whole-tile block needs at 64 tokens, less the 16 rows each of its three [S][512] buffers; equal at S % 64 == 0."""
    base, _ = call(op=0, Cc=64, ws_base=None)
    core, _ = call(op=CORE_RAGGED, H=6, W=8, residual=ADDR, ws_base=None)
    b48, _ = call(op=BLOCK_RAGGED, H=6, W=8, ws_base=None)
    b64, _ = call(op=BLOCK_RAGGED, H=8, W=8, ws_base=None)
    old64, _ = call(op=5, H=8, W=8, ws_base=None)
    assert core == base > (64 << 20)
    assert b64 == old64 and b48 == b64 - 3 * 16 * 512 * 2
    assert b48 >= base + 48 * 512 * 2 * 3 + 64 * 512 * 2 * 3
    one, _ = call(op=BLOCK_RAGGED, H=1, W=1, ws_base=None)
    assert one == base + 3 * 1024 + 64 * 512 * 2 * 3
