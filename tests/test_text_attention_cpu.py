"""rf_debug_text_attention refuses what the attention kernels of csrc/text.hip cannot run, before any HIP call (no GPU needed): each
refusal returns its RF_ERR_* code and leaves a message in rf_last_error()."""
import ctypes as C

import pytest

from reflectionflow_amd import _lib as L

RF_ERR_SHAPE, RF_ERR_ALIGN, RF_ERR_NULL, RF_ERR_UNSUPPORTED = -1, -2, -3, -5
HEADS, NB = 3, 2


@pytest.fixture(scope="module")
def buf():
    """16-byte-aligned host memory: a refused call never touches it"""
    raw = C.create_string_buffer(4096 + 16)
    addr = (C.addressof(raw) + 15) & ~15
    return raw, addr


def call(addr, head_dim=80, qi=1, S=257, S_pad=288, bias=True, heads=HEADS, B=NB, q_off=0, ldq=None, ldo=None, ldvt=None, bias_hs=0):
    """One call with valid arguments except for what the keywords change; q_off: bytes added to q, None = a NULL q"""
    inner = heads * head_dim
    ldq = inner + 64 if ldq is None else ldq
    ldo = inner + 64 if ldo is None else ldo
    ldvt = B * S_pad + 64 if ldvt is None else ldvt
    lib = L.load()
    rc = lib.rf_debug_text_attention(head_dim, qi, None if q_off is None else addr + q_off, ldq, addr, ldq, addr, ldvt, addr if bias else None, bias_hs,
                                     addr, ldo, heads, B, S, S_pad, 1.0, None)
    return rc, lib.rf_last_error().decode(errors="replace")


@pytest.mark.parametrize("kw,code,word", [
    (dict(head_dim=80, S=500, S_pad=512), RF_ERR_SHAPE, "S_pad=512"),          # 512 keys fit the LDS at head dim 64 only
    (dict(head_dim=64, S=500, S_pad=544), RF_ERR_SHAPE, "S_pad=544"),
    (dict(S=40, S_pad=48), RF_ERR_SHAPE, "S_pad=48"),                          # S_pad % 32 != 0
    (dict(S=289, S_pad=288), RF_ERR_SHAPE, "S=289"),                           # S > S_pad
    (dict(S=0, S_pad=32), RF_ERR_SHAPE, "S=0"),
    (dict(bias=False), RF_ERR_NULL, "bias NULL"),                              # padded keys would go unmasked
    (dict(head_dim=96), RF_ERR_UNSUPPORTED, "head_dim=96"),
    (dict(qi=2), RF_ERR_UNSUPPORTED, "qi=2"),
    (dict(q_off=2), RF_ERR_ALIGN, "16-byte"),                                  # a misaligned pointer
    (dict(q_off=None), RF_ERR_NULL, "NULL"),
    (dict(ldo=HEADS * 80 - 8), RF_ERR_SHAPE, "ldo=232"),                       # ldo < heads * head_dim
    (dict(ldq=HEADS * 80 + 4), RF_ERR_ALIGN, "ldq=244"),                       # a pitch that is no multiple of 8 elements
    (dict(ldvt=NB * 288 - 8), RF_ERR_SHAPE, "ldvt=568"),                       # ldvt < B * S_pad
    (dict(B=65), RF_ERR_SHAPE, "B=65"),
    (dict(head_dim=80, heads=52), RF_ERR_SHAPE, "heads=52"),                   # heads * head_dim > 4096
    (dict(bias_hs=288), RF_ERR_SHAPE, "bias_hs=288"),                          # a head stride shorter than one [S_pad][S_pad] plane
])
def test_refusals(buf, kw, code, word):
    rc, msg = call(buf[1], **kw)
    assert rc == code, (rc, msg)
    assert "rf_debug_text_attention" in msg and word in msg, msg
