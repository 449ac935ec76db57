"""CPU: the streaming-keys attention of csrc/text.hip (attn64_stream_kernel) and what it opens up -- rf_text_attention (include/rf_flux.h)
refuses what it cannot run before any HIP call (no GPU needed), the vision tower's size query takes the 577 tokens of ViT-L/14 at 336 px
at head dim 64 and still refuses them at head dim 80, rf_clip_preprocess takes size 336, the verifier's config plumbing carries the
image size, and the kernel's LDS image (a 128-key chunk in attn64_kernel's layout) against the bank model of tests/test_lds_layouts_cpu.py."""
import ctypes as C
import json
import os
import re

import pytest

from reflectionflow_amd import _lib as L
from reflectionflow_amd.tts import clip_verifier as CV
from tests.test_clip_h_cpu import _opts, _vision_weights
from tests.test_lds_layouts_cpu import ways

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_ERR_SHAPE, RF_ERR_ALIGN, RF_ERR_NULL, RF_ERR_UNSUPPORTED = -1, -2, -3, -5
HEADS, NB = 3, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def buf():
    """16-byte-aligned host memory: a refused call never touches it"""
    raw = C.create_string_buffer(4096 + 16)
    return raw, (C.addressof(raw) + 15) & ~15


def call(lib, addr, head_dim=64, qi=1, stream_keys=0, S=257, S_pad=288, bias=True, heads=HEADS, B=NB, q_off=0, ldq=None, ldo=None, ldvt=None, bias_hs=0):
    """One call with valid arguments except for what the keywords change; q_off: bytes added to q, None = a NULL q"""
    inner = heads * head_dim
    ldq = inner + 64 if ldq is None else ldq
    ldo = inner + 64 if ldo is None else ldo
    ldvt = B * S_pad + 64 if ldvt is None else ldvt
    rc = lib.rf_text_attention(head_dim, qi, stream_keys, None if q_off is None else addr + q_off, ldq, addr, ldq, addr, ldvt, addr if bias else None,
                               bias_hs, addr, ldo, heads, B, S, S_pad, 1.0, None)
    return rc, lib.rf_last_error().decode(errors="replace")


def test_entry_point_is_declared_bound_and_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rf_flux.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+rf_text_attention\s*\(([^)]*)\)\s*;", txt)
    assert m, "rf_text_attention is not declared in include/rf_flux.h"
    res, args = L._SIGS["rf_text_attention"]
    params = [p.strip() for p in m.group(1).split(",")]
    assert res is C.c_int and len(params) == len(args) == 19
    assert params[2] == "int32_t stream_keys" and args[:3] == [C.c_int32] * 3
    dbg = L._EXTRA_SIGS["rf_debug_text_attention"][1]
    assert args[:2] + args[3:] == dbg                     # the debug entry's arguments plus stream_keys
    assert hasattr(C.CDLL(L.LIB_PATH), "rf_text_attention")
    assert "rf_text_attention" in L.declared_symbols() and "rf_text_attention" not in L.debug_symbols()
    assert L.ABI_VERSION == 17 and lib.rf_abi_version() == 17


# tests/test_text_attention_cpu.py's table at head dim 64 (this entry point's only one), every row with the debug entry's code
@pytest.mark.parametrize("kw,code,word", [
    (dict(S=2000, S_pad=2080), RF_ERR_SHAPE, "S_pad=2080"),                    # beyond the streaming limit; the message names it
    (dict(S=40, S_pad=48), RF_ERR_SHAPE, "S_pad=48"),                          # S_pad % 32 != 0
    (dict(S=289, S_pad=288), RF_ERR_SHAPE, "S=289"),                           # S > S_pad
    (dict(S=0, S_pad=32), RF_ERR_SHAPE, "S=0"),
    (dict(bias=False), RF_ERR_NULL, "bias NULL"),                              # padded keys would go unmasked
    (dict(head_dim=96), RF_ERR_UNSUPPORTED, "head_dim=96"),
    (dict(head_dim=80), RF_ERR_UNSUPPORTED, "head_dim=80"),                    # head dim 80 has no streaming kernel: not served here at all
    (dict(head_dim=80, S=500, S_pad=512), RF_ERR_UNSUPPORTED, "head_dim=80"),
    (dict(qi=2), RF_ERR_UNSUPPORTED, "qi=2"),
    (dict(stream_keys=2), RF_ERR_UNSUPPORTED, "stream_keys=2"),
    (dict(stream_keys=-1), RF_ERR_UNSUPPORTED, "stream_keys=-1"),
    (dict(q_off=2), RF_ERR_ALIGN, "16-byte"),                                  # a misaligned pointer
    (dict(q_off=None), RF_ERR_NULL, "NULL"),
    (dict(ldo=HEADS * 64 - 8), RF_ERR_SHAPE, "ldo=184"),                       # ldo < heads * head_dim
    (dict(ldq=HEADS * 64 + 4), RF_ERR_ALIGN, "ldq=196"),                       # a pitch that is no multiple of 8 elements
    (dict(ldvt=NB * 288 - 8), RF_ERR_SHAPE, "ldvt=568"),                       # ldvt < B * S_pad
    (dict(B=65), RF_ERR_SHAPE, "B=65"),
    (dict(heads=65), RF_ERR_SHAPE, "heads=65"),                                # heads * head_dim > 4096
    (dict(bias_hs=288), RF_ERR_SHAPE, "bias_hs=288"),                          # a head stride shorter than one [S_pad][S_pad] plane
    (dict(stream_keys=1, S=2000, S_pad=2080), RF_ERR_SHAPE, "2048"),
])
def test_refusals(lib, buf, kw, code, word):
    rc, msg = call(lib, buf[1], **kw)
    assert rc == code, (rc, msg)
    assert "rf_text_attention" in msg and word in msg, msg


def test_the_streaming_limit_is_named_and_the_debug_entry_keeps_its_own(lib, buf):
    rc, msg = call(lib, buf[1], S=2000, S_pad=2080)
    assert rc == RF_ERR_SHAPE and "2048" in msg
    a = buf[1]
    rc = lib.rf_debug_text_attention(64, 1, a, 256, a, 256, a, 2 * 544 + 64, a, 0, a, 256, HEADS, NB, 500, 544, 1.0, None)
    assert rc == RF_ERR_SHAPE and b"S_pad=544" in lib.rf_last_error() and b"512" in lib.rf_last_error()


def test_vision_size_query_takes_577_tokens_at_head_dim_64_only(lib):
    q = lib.rf_clip_vision_workspace_bytes_opts
    w64, k64 = _vision_weights(128, 2, image_size=336)
    assert w64.mask_S == 608
    n = q(C.byref(w64), C.byref(_opts(64, 0)), 2)
    assert n > 0 and lib.rf_clip_vision_workspace_bytes(C.byref(w64), 2) == n
    w80, k80 = _vision_weights(160, 2, image_size=336)
    assert q(C.byref(w80), C.byref(_opts(80)), 2) == -1                        # head dim 80 keeps its resident keys: <= 480
    # 448 px / 14: 1025 tokens, S_pad 1056; and the limit itself, S_pad 2048 (630 / 14 = 45: 2026 tokens), and one patch row more
    w448, k448 = _vision_weights(128, 2, image_size=448)
    assert w448.mask_S == 1056 and q(C.byref(w448), C.byref(_opts(64, 0)), 1) > 0
    w630, k630 = _vision_weights(128, 2, image_size=630)
    assert w630.mask_S == 2048 and q(C.byref(w630), C.byref(_opts(64, 0)), 1) > 0
    w644, k644 = _vision_weights(128, 2, image_size=644)
    assert q(C.byref(w644), C.byref(_opts(64, 0)), 1) == -1 and b"2048" in lib.rf_last_error()
    assert lib.rf_clip_vision_encode_opts(C.byref(w644), C.byref(_opts(64, 0)), 256, 1, 256, None, None) == -1


def test_preprocess_validation_accepts_336_and_448(lib):
    # a NULL image is the check AFTER the size's in no case; so: size accepted <=> the call gets as far as the stride check
    bad_stride = lambda size, patch: lib.rf_clip_preprocess(16, 0, 0, 1, 1, 1, 64, 64, 1.0, 0.0, size, patch, 16, None)  # noqa: E731
    for size in (224, 336, 448, 512):
        assert bad_stride(size, 14 if size % 14 == 0 else 16) == -1 and b"strides" in lib.rf_last_error(), size
    assert bad_stride(518, 14) == -1 and b"size=518" in lib.rf_last_error() and b"512" in lib.rf_last_error()
    assert bad_stride(336, 15) == -1 and b"size=336" in lib.rf_last_error()


def test_config_plumbing_carries_the_image_size(tmp_path):
    d = str(tmp_path)
    json.dump({"text_config": {"num_attention_heads": 12}, "vision_config": {"num_attention_heads": 16, "image_size": 336, "patch_size": 14},
               "projection_dim": 768}, open(os.path.join(d, "config.json"), "w"))
    mc = CV.read_clip_config(d)
    assert mc["image_size"] == 336 and (mc["text_heads"], mc["vision_heads"], mc["hidden_act"]) == (12, 16, "quick_gelu")
    json.dump({"text_config": {}, "vision_config": {}}, open(os.path.join(d, "config.json"), "w"))
    assert CV.read_clip_config(d)["image_size"] == 224


def test_geometry_tables_of_the_336_tower():
    L336, T336 = CV.VIT_L14_336, CV.TINY_336
    assert L336["vision"] == dict(hidden=1024, heads=16, inter=4096, layers=24, image_size=336, patch=14) and L336["text"] == CV.VIT_L14["text"]
    assert L336["projection_dim"] == 768 and "act" not in L336
    assert T336["vision"]["image_size"] == 336 and T336["vision"]["layers"] == T336["text"]["layers"] == 2
    assert T336["vision"]["hidden"] // T336["vision"]["heads"] == 64
    assert CV.geometry("vit_l14_336") == (L336, T336) and CV.geometry("vit_l14") == (CV.VIT_L14, CV.TINY)
    assert CV.geometry_names() == ["vit_h14", "vit_l14", "vit_l14_336"]
    with pytest.raises(CV.RFError, match="vit_l14_336"):
        CV.geometry("vit_b32")
    sd = CV.synthetic_clip_state(T336, 0)
    assert sd["vision_model.embeddings.position_embedding.weight"].shape == (577, 128)
    tool = open(os.path.join(ROOT, "tools", "kb_clip_score.py")).read()
    assert '"vit_l14_336"' in tool


# ---- LDS image of a chunk (csrc/text.hip, attn64_stream_kernel): attn64_kernel's formulas at S_pad = 128, lane = 16 g + l15 -------------
CK, VP, KB = 128, 2 * 128 + 16, 128 * 128


def test_lds_budget_is_independent_of_s_pad_and_fits_two_workgroups():
    buf_bytes = KB + 64 * VP
    assert buf_bytes == 33792 and 2 * buf_bytes == 67584
    assert (160 * 1024) // (2 * buf_bytes) == 2
    assert 2 * (256 * 128 + 64 * (2 * 256 + 16)) == 133120 and (160 * 1024) // 133120 == 1      # 256-key chunks: one workgroup per CU


def test_chunk_k_fragment_reads_are_conflict_free_in_both_buffers():
    # kl + r * 128 + (((4 ds + g) ^ (r & 7)) << 4), r = 16 t + l15, kl = buffer base
    for base in (0, KB + 64 * VP):
        for t in range(CK // 16):
            for ds in range(2):
                assert ways(lambda l: base + (16 * t + (l & 15)) * 128 + (((4 * ds + (l >> 4)) ^ ((16 * t + (l & 15)) & 7)) << 4)) == 1


def test_chunk_vt_fragment_reads_are_two_way_as_in_the_resident_kernel():
    # vl + (16 dt + l15) * VP + b * 64 + g * 16: the resident kernel's pitch formula (2 keys + 16 B) at 128 keys; 2-way under the model,
    # the figure tests/test_clip_h_cpu.py records for attn64_kernel at 288 keys
    for base in (KB, KB + 64 * VP + KB):
        for dt in range(4):
            for b in range(CK // 32):
                assert ways(lambda l: base + (16 * dt + (l & 15)) * VP + b * 64 + ((l >> 4) << 4)) == 2
    assert ways(lambda l: (l & 15) * (2 * 288 + 16) + ((l >> 4) << 4)) == 2


def test_chunk_staging_fills_the_images_without_overlap():
    """thread tid, piece i: idx = tid + 256 i -> K row idx >> 3, chunk idx & 7; V^T channel idx >> 4, 8 keys from (idx & 15) * 8"""
    for nk in (32, 96, 128):
        k_seen, v_seen = set(), set()
        for idx in range(1024):
            r, c = idx >> 3, idx & 7
            if r < nk:
                a = r * 128 + ((c ^ (r & 7)) << 4)
                assert 0 <= a and a + 16 <= KB
                k_seen.add(a)
            d, m = idx >> 4, idx & 15
            if m * 8 < nk:
                blk, kap = (m * 8) >> 5, (m * 8) & 31
                tile, g0 = kap >> 4, (kap & 15) >> 2
                for part in (8 * g0 + 4 * tile, 8 * (g0 + 1) + 4 * tile):
                    a = KB + d * VP + blk * 64 + part * 2
                    assert KB <= a and a + 8 <= KB + 64 * VP
                    v_seen.add(a)
        assert len(k_seen) == nk * 8 and len(v_seen) == 2 * 64 * (nk // 8)
        # slot(key) = 8 (key%16 / 4) + 4 (key / 16) + key % 4 is a permutation of a 32-key block, and staging realises it
        slot = lambda key: 8 * ((key % 16) // 4) + 4 * (key // 16) + key % 4  # noqa: E731
        assert sorted(slot(key) for key in range(32)) == list(range(32))
        for m in range(4):
            kap = m * 8
            tile, g0 = kap >> 4, (kap & 15) >> 2
            assert [8 * g0 + 4 * tile + j for j in range(4)] == [slot(kap + j) for j in range(4)]
            assert [8 * (g0 + 1) + 4 * tile + j for j in range(4)] == [slot(kap + 4 + j) for j in range(4)]
