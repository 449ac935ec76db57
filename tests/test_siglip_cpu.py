"""CPU: the SigLIP score verifier -- the torch restatement of transformers' SiglipModel that the GPU tests use as their reference
(tests/siglip_ref.py), the exactness of the weight packing (heads 72 -> 80, inter 272 -> 320, q prescaled, v bias folded), the numpy
restatement of rf_siglip_preprocess against PIL, the argument checks of the new entry points (no kernel is launched: there is no GPU
here), the refusals the existing entry points keep, the LDS image of attn80_stream_kernel's 96-key chunk against the bank model of
tests/test_lds_layouts_cpu.py, and the verifier's config plumbing."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from reflectionflow_amd import _lib as L
from reflectionflow_amd.tts import search
from reflectionflow_amd.tts import siglip_verifier as SV
from tests import siglip_ref as R
from tests.test_clip_h_cpu import _opts, _vision_weights
from tests.test_lds_layouts_cpu import SWZ, ways

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_ERR_SHAPE, RF_ERR_ALIGN, RF_ERR_NULL, RF_ERR_UNSUPPORTED = -1, -2, -3, -5
HEADS, NB = 3, 2
NEW = ["rf_text_attention80", "rf_siglip_score", "rf_siglip_preprocess", "rf_siglip_vision_workspace_bytes", "rf_siglip_vision_encode",
       "rf_siglip_text_workspace_bytes", "rf_siglip_text_encode", "rf_siglip_probe_attention"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


# ---- the restatement is the reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_case(name):
    cfg = {"224": R.TINY_224, "322": R.TINY_322}[name]
    m = R.hf_siglip_model(cfg, R.bf16_round(SV.synthetic_siglip_state(cfg, 1)))
    g = torch.Generator().manual_seed(5)
    px = torch.randn(3, 3, cfg["vision"]["image_size"], cfg["vision"]["image_size"], generator=g)
    ids = SV.synthetic_tokenize(cfg["text"]["vocab"])(["a cat", "two dogs on a bench"])
    return cfg, m, px, ids


@torch.no_grad()
@pytest.mark.parametrize("name", ["224", "322"])
def test_restatement_is_bit_equal_to_transformers(name):
    """tests/siglip_ref.py (fp32, on bf16-rounded weights held in storage of its own) against SiglipModel.from_config with eager
    attention: the vision tokens, both towers' pooled outputs and logits_per_image, bit for bit"""
    cfg, m, px, ids = model_case(name)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    out = m(input_ids=ids, pixel_values=px)
    vis = m.vision_model(pixel_values=px)
    assert torch.equal(R.vision_tokens(sd, px, cfg), vis.last_hidden_state)
    rv, rt = R.vision_pooled(sd, px, cfg), R.text_pooled(sd, ids, cfg)
    assert torch.equal(rv, vis.pooler_output) and rv.shape == (3, 144)
    assert torch.equal(rt, m.text_model(input_ids=ids).pooler_output) and rt.shape == (2, 144)
    assert torch.equal(R.logits(sd, rv, rt), out.logits_per_image)
    assert set(k for k in sd if not k.endswith("position_ids")) == set(SV.synthetic_siglip_state(cfg, 0))


@torch.no_grad()
@pytest.mark.parametrize("name", ["224", "322"])
def test_packing_is_exact(name):
    """the restatement on the PACKED weights equals the restatement on the raw ones to fp32 round-off, and the padded channels of every
    attention output are identically 0"""
    cfg, m, px, ids = model_case(name)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    keep = []
    pv, pt = R.vision_pooled_packed(sd, px, cfg, keep=keep), R.text_pooled_packed(sd, ids, cfg, keep=keep)
    rv, rt = R.vision_pooled(sd, px, cfg), R.text_pooled(sd, ids, cfg)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    print(f"  PACKING {name}: vision rel-L2 {rel(pv, rv):.2e} text {rel(pt, rt):.2e}")
    assert rel(pv, rv) <= 1e-5 and rel(pt, rt) <= 1e-5
    assert len(keep) == 4 and all(k.shape[-2:] == (2, 80) for k in keep)
    assert all(float(k[..., 72:].abs().max()) == 0.0 for k in keep)
    assert all(float(k[..., :72].abs().max()) > 0.0 for k in keep)


def test_packed_shapes_and_refusals():
    from reflectionflow_amd.flux import text_hip as TH
    cfg = R.TINY_224
    sd = {k[len("vision_model."):]: v for k, v in SV.synthetic_siglip_state(cfg, 0).items() if k.startswith("vision_model.")}
    y = TH.siglip_pack_layers(sd, 2, 2)[1]
    assert y["w_qk"].shape == (320, 144) and y["b_qk"].shape == (320,) and y["w_v"].shape == (160, 144) and y["w_o"].shape == (144, 160)
    assert y["w_fc1"].shape == (320, 144) and y["b_fc1"].shape == (320,) and y["w_fc2"].shape == (144, 320)
    for h in range(2):
        assert float(y["w_qk"][80 * h + 72:80 * h + 80].abs().max()) == 0.0 and float(y["w_v"][80 * h + 72:80 * h + 80].abs().max()) == 0.0
        assert float(y["w_o"][:, 80 * h + 72:80 * h + 80].abs().max()) == 0.0 and float(y["b_qk"][160 + 80 * h + 72:160 + 80 * h + 80].abs().max()) == 0.0
    assert float(y["w_fc1"][272:].abs().max()) == 0.0 and float(y["b_fc1"][272:].abs().max()) == 0.0 and float(y["w_fc2"][:, 272:].abs().max()) == 0.0
    q = sd["encoder.layers.1.self_attn.q_proj.weight"]
    assert torch.equal(y["w_qk"][80:152], q[72:144] * 72 ** -0.5)                    # the TRUE head dim's scale, head 1 at rows 80 ..
    hp = TH.siglip_pack_pool_head(sd, 2)
    assert hp["probe_q"].shape == (144,) and hp["w_kv"].shape == (288, 144) and hp["w_fc1"].shape == (320, 144)
    # so400m: 4304 -> 4352; head dim 64 goes through the same padded path; head dims above 80 are refused
    assert TH.siglip_pack_mlp(torch.zeros(4304, 8), torch.zeros(4304), torch.zeros(8, 4304), torch.zeros(8))["w_fc2"].shape == (8, 4352)
    assert TH.siglip_head_dim("x", 768, 12) == 64 and TH.siglip_head_dim("x", 1152, 16) == 72
    with pytest.raises(TH.RFError, match="head dim 96"):
        TH.siglip_head_dim("x", 192, 2)
    with pytest.raises(TH.RFError, match="not a multiple"):
        TH.siglip_head_dim("x", 100, 3)


# ---- preprocessing ----------------------------------------------------------------------------------------------------------------------
PRE_CASES = [(40, 56, 28), (16, 24, 28), (28, 28, 28)]        # H, W -> size: down (non-square), up, identity


def pre_image(H, W):
    return np.random.default_rng(100 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H,W,size", PRE_CASES)
def test_preprocess_restatement_equals_pil_level_for_level(H, W, size):
    from PIL import Image
    lv = pre_image(H, W)
    pil = np.asarray(Image.fromarray(lv).resize((size, size), Image.BICUBIC))
    mine = R.preprocess_levels_np(lv, size)
    assert mine.shape == pil.shape == (size, size, 3) and np.array_equal(mine, pil)
    if (H, W) == (size, size):
        assert np.array_equal(mine, lv)
    # the normalisation: SiglipImageProcessor's rescale 1 / 255, mean = std = 0.5, rounded to bf16
    want = torch.from_numpy(((pil.astype(np.float32) * np.float32(1 / 255) - np.float32(0.5)) / np.float32(0.5))).permute(2, 0, 1).to(R.BF)
    assert torch.equal(R.normalise_np(mine), want)
    assert float(R.normalise_np(np.array([[[0, 255, 128]]], np.uint8)).float().abs().max()) == 1.0


def test_preprocess_argument_checks(lib):
    bad_stride = lambda size, patch: lib.rf_siglip_preprocess(16, 0, 0, 1, 1, 1, 64, 64, 1.0, 0.0, size, patch, 16, None)  # noqa: E731
    for size, patch in ((224, 16), (384, 14), (512, 16)):
        assert bad_stride(size, patch) == RF_ERR_SHAPE and b"strides" in lib.rf_last_error(), size
    assert bad_stride(518, 14) == RF_ERR_SHAPE and b"size=518" in lib.rf_last_error() and b"512" in lib.rf_last_error()
    assert bad_stride(14, 16) == RF_ERR_SHAPE and b"size=14 patch=16" in lib.rf_last_error()        # 384 / 14 is fine: a valid convolution
    assert lib.rf_siglip_preprocess(16, 1, 1, 1, 1, 1, 8200, 64, 1.0, 0.0, 384, 14, 16, None) == RF_ERR_SHAPE and b"H=8200" in lib.rf_last_error()
    assert lib.rf_siglip_preprocess(None, 1, 1, 1, 1, 1, 64, 64, 1.0, 0.0, 384, 14, 16, None) == RF_ERR_NULL


# ---- argument checks without a GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buf():
    """16-byte-aligned host memory: a refused call never touches it"""
    raw = C.create_string_buffer(4096 + 16)
    return raw, (C.addressof(raw) + 15) & ~15


def call80(lib, addr, qi=1, stream_keys=0, S=257, S_pad=288, bias=True, heads=HEADS, B=NB, q_off=0, ldq=None, ldo=None, ldvt=None, bias_hs=0):
    """One rf_text_attention80 call with valid arguments except for what the keywords change; q_off: bytes added to q, None = NULL"""
    inner = heads * 80
    ldq = inner + 64 if ldq is None else ldq
    ldo = inner + 64 if ldo is None else ldo
    ldvt = B * S_pad + 64 if ldvt is None else ldvt
    rc = lib.rf_text_attention80(qi, stream_keys, None if q_off is None else addr + q_off, ldq, addr, ldq, addr, ldvt, addr if bias else None, bias_hs, addr,
                                 ldo, heads, B, S, S_pad, 1.0, None)
    return rc, lib.rf_last_error().decode(errors="replace")


def test_new_entry_points_are_declared_bound_and_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rf_flux.h")).read(), flags=re.S)
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/rf_flux.h"
        res, args = L._SIGS[name]
        assert res is (C.c_int64 if m.group(1) == "int64_t" else C.c_int)
        assert len([p for p in m.group(2).split(",")]) == len(args), name
        assert hasattr(raw, name) and name in L.declared_symbols() and name not in L.debug_symbols()
    # rf_text_attention's arguments without head_dim; rf_siglip_preprocess takes rf_clip_preprocess's
    assert L._SIGS["rf_text_attention80"][1] == L._SIGS["rf_text_attention"][1][1:]
    assert L._SIGS["rf_siglip_preprocess"] == L._SIGS["rf_clip_preprocess"]
    assert not [n for n in L.debug_symbols() if "siglip" in n]                       # the debug header is as it was
    assert L.ABI_VERSION == 17 and lib.rf_abi_version() == 17
    assert L.RF_CLIP_ACT_GELU_TANH == 2 and L.CLIP_ACTS == {"quick_gelu": 0, "gelu": 1}


def test_struct_layouts_agree_with_the_header():
    from tests.test_clip_h_cpu import _run_c
    out = _run_c("".join(f'printf("{s} %zu\\n", sizeof({s}));\n' for s in ("rf_siglip_vision_weights", "rf_siglip_text_weights", "rf_clip_weights",
                                                                            "rf_clip_layer", "rf_clip_vision_weights")) +
                 'printf("layer %zu\\n", offsetof(rf_siglip_vision_weights, layer));\nprintf("hfc2 %zu\\n", offsetof(rf_siglip_vision_weights, b_hfc2));\n'
                 'printf("tlayer %zu\\n", offsetof(rf_siglip_text_weights, layer));\nprintf("tanh %d\\n", RF_CLIP_ACT_GELU_TANH);\n')
    o = {k: int(v) for k, v in out.items()}
    assert o["rf_siglip_vision_weights"] == C.sizeof(L.rf_siglip_vision_weights) and o["rf_siglip_text_weights"] == C.sizeof(L.rf_siglip_text_weights)
    assert o["layer"] == L.rf_siglip_vision_weights.layer.offset and o["hfc2"] == L.rf_siglip_vision_weights.b_hfc2.offset
    assert o["tlayer"] == L.rf_siglip_text_weights.layer.offset and o["tanh"] == 2
    assert (o["rf_clip_layer"], o["rf_clip_weights"], o["rf_clip_vision_weights"]) == (104, 80, 120)        # the v17 layouts, untouched


@pytest.mark.parametrize("kw,code,word", [
    (dict(S=2000, S_pad=2080), RF_ERR_SHAPE, "S_pad=2080"),                    # beyond the streaming limit; the message names it
    (dict(stream_keys=1, S=2000, S_pad=2080), RF_ERR_SHAPE, "2048"),
    (dict(S=40, S_pad=48), RF_ERR_SHAPE, "S_pad=48"),                          # S_pad % 32 != 0
    (dict(S=289, S_pad=288), RF_ERR_SHAPE, "S=289"),
    (dict(S=0, S_pad=32), RF_ERR_SHAPE, "S=0"),
    (dict(bias=False), RF_ERR_NULL, "bias NULL"),                              # padded keys would go unmasked
    (dict(qi=2), RF_ERR_UNSUPPORTED, "qi=2"),
    (dict(stream_keys=2), RF_ERR_UNSUPPORTED, "stream_keys=2"),
    (dict(stream_keys=-1), RF_ERR_UNSUPPORTED, "stream_keys=-1"),
    (dict(q_off=2), RF_ERR_ALIGN, "16-byte"),                                  # a misaligned pointer
    (dict(q_off=None), RF_ERR_NULL, "NULL"),
    (dict(ldo=HEADS * 80 - 8), RF_ERR_SHAPE, "ldo=232"),                       # ldo < heads * 80
    (dict(ldq=HEADS * 80 + 4), RF_ERR_ALIGN, "ldq=244"),                       # a pitch that is no multiple of 8 elements
    (dict(ldvt=NB * 288 - 8), RF_ERR_SHAPE, "ldvt=568"),                       # ldvt < B * S_pad
    (dict(B=65), RF_ERR_SHAPE, "B=65"),
    (dict(heads=52), RF_ERR_SHAPE, "heads=52"),                                # heads * 80 > 4096
    (dict(bias_hs=288), RF_ERR_SHAPE, "bias_hs=288"),
])
def test_text_attention80_refusals(lib, buf, kw, code, word):
    rc, msg = call80(lib, buf[1], **kw)
    assert rc == code, (rc, msg)
    assert "rf_text_attention80" in msg and word in msg, msg


def _siglip_vision(hidden=144, heads=2, head_dim=72, inter=320, image_size=224, patch=14):
    w = L.rf_siglip_vision_weights()
    layers = (L.rf_clip_layer * 2)()
    g = image_size // patch
    w.layers, w.hidden, w.heads, w.head_dim, w.inter, w.image_size, w.patch = 2, hidden, heads, head_dim, inter, image_size, patch
    w.mask_S, w.eps = (g * g + 31) // 32 * 32, 1e-6
    for n in ("patch_w", "patch_b", "pos_embed", "post_ln_scale", "post_ln_shift", "mask", "w_kv", "b_kv", "probe_q", "w_po", "b_po", "hln_scale",
              "hln_shift", "w_hfc1", "b_hfc1", "w_hfc2", "b_hfc2"):
        setattr(w, n, 256)                                # never dereferenced: the size query validates and adds
    w.layer = C.cast(layers, C.POINTER(L.rf_clip_layer))
    return w, layers


def _siglip_text(hidden=144, heads=2, head_dim=72, inter=320):
    w = L.rf_siglip_text_weights()
    layers = (L.rf_clip_layer * 2)()
    w.layers, w.hidden, w.heads, w.head_dim, w.inter, w.vocab, w.max_pos, w.proj_dim, w.eps = 2, hidden, heads, head_dim, inter, 512, 64, 144, 1e-6
    for n in ("tok_embed", "pos_embed", "final_ln_scale", "final_ln_shift", "head_w", "head_b"):
        setattr(w, n, 256)
    w.layer = C.cast(layers, C.POINTER(L.rf_clip_layer))
    return w, layers


def test_siglip_size_queries(lib):
    qv, qt = lib.rf_siglip_vision_workspace_bytes, lib.rf_siglip_text_workspace_bytes
    w, keep = _siglip_vision()
    n1, n3 = qv(C.byref(w), 1), qv(C.byref(w), 3)
    assert 0 < n1 < n3
    # 729 tokens of so400m/14 at 384 px (S_pad 736 > 480: what no CLIP entry point takes at head dim 80), and the limit: 45^2 = 2025
    w384, k384 = _siglip_vision(image_size=384)
    assert w384.mask_S == 736 and qv(C.byref(w384), 8) > 0
    w630, k630 = _siglip_vision(image_size=630)
    assert w630.mask_S == 2048 and qv(C.byref(w630), 1) > 0
    w644, k644 = _siglip_vision(image_size=644)                                  # 46^2 = 2116 tokens
    assert qv(C.byref(w644), 1) == RF_ERR_SHAPE and b"2116 tokens > 2048" in lib.rf_last_error()
    assert lib.rf_siglip_vision_encode(C.byref(w644), 256, 1, 256, None, None) == RF_ERR_SHAPE
    assert qv(C.byref(w), 65) == RF_ERR_SHAPE and b"B=65" in lib.rf_last_error()
    assert qv(C.byref(w), 0) == RF_ERR_SHAPE
    big, kbig = _siglip_vision(hidden=52 * 72, heads=52)
    assert qv(C.byref(big), 1) == RF_ERR_SHAPE and b"heads * 80 = 4160 > 4096" in lib.rf_last_error()
    w96, k96 = _siglip_vision(hidden=192, heads=2, head_dim=96)
    assert qv(C.byref(w96), 1) == RF_ERR_SHAPE and b"head_dim=96" in lib.rf_last_error()
    odd, kodd = _siglip_vision(inter=272)
    assert qv(C.byref(odd), 1) == RF_ERR_SHAPE and b"inter=272" in lib.rf_last_error()
    w64, k64 = _siglip_vision(hidden=128, heads=2, head_dim=64)                  # head dim 64: the same padded path
    assert qv(C.byref(w64), 1) > 0
    assert qv(None, 1) == RF_ERR_NULL
    t, kt = _siglip_text()
    assert qt(C.byref(t), 2, 64) > 0 and qt(C.byref(t), 2, 40) > 0
    assert qt(C.byref(t), 65, 64) == RF_ERR_SHAPE and b"B=65" in lib.rf_last_error()
    assert qt(C.byref(t), 1, 65) == RF_ERR_SHAPE and b"S=65" in lib.rf_last_error()
    t.max_pos = 4096
    assert qt(C.byref(t), 1, 2048) > 0 and qt(C.byref(t), 1, 2049) == RF_ERR_SHAPE and b"2048" in lib.rf_last_error()
    tbig, ktb = _siglip_text(hidden=52 * 72, heads=52)
    assert qt(C.byref(tbig), 1, 64) == RF_ERR_SHAPE and b"4096" in lib.rf_last_error()
    # S = 40 is no multiple of 32: the encode call wants the padded-keys mask
    t.max_pos = 64
    assert lib.rf_siglip_text_encode(C.byref(t), 256, 1, 40, 256, None, None) == RF_ERR_SHAPE and b"mask" in lib.rf_last_error()
    pa = lambda **kw: lib.rf_siglip_probe_attention(*[{**dict(q=256, k=256, ldk=288, v=256, ldv=288, out=256, ldo=144, heads=2, d=72, B=3, T=256, rows=256,  # noqa: E731
                                                              st=None), **kw}[n] for n in ("q", "k", "ldk", "v", "ldv", "out", "ldo", "heads", "d", "B", "T", "rows", "st")])
    assert pa(d=96) == RF_ERR_SHAPE and b"head_dim=96" in lib.rf_last_error()
    assert pa(T=2049, rows=2080) == RF_ERR_SHAPE and b"T=2049" in lib.rf_last_error()
    assert pa(rows=200) == RF_ERR_SHAPE and pa(ldk=136) == RF_ERR_SHAPE and pa(k=258) == RF_ERR_ALIGN and pa(q=None) == RF_ERR_NULL
    assert lib.rf_siglip_score(None, 256, 0.0, 0.0, 0.5, 256, None, 1, 8, None) == RF_ERR_NULL
    assert lib.rf_siglip_score(256, 256, 0.0, 0.0, 1.5, 256, None, 1, 8, None) == RF_ERR_SHAPE and b"threshold" in lib.rf_last_error()


def test_the_existing_entry_points_keep_their_refusals(lib, buf):
    a = buf[1]
    q = lib.rf_clip_vision_workspace_bytes_opts
    w, keep = _vision_weights(160, 2)
    assert q(C.byref(w), C.byref(_opts(72)), 1) == RF_ERR_UNSUPPORTED and b"head_dim=72" in lib.rf_last_error()
    assert q(C.byref(w), C.byref(_opts(80, 2)), 1) == RF_ERR_UNSUPPORTED and b"act=2" in lib.rf_last_error()     # gelu_tanh is not a CLIP activation
    big80, k80 = _vision_weights(160, 2, image_size=308)                       # 485 tokens -> S_pad 512 > 480
    assert q(C.byref(big80), C.byref(_opts(80)), 1) == RF_ERR_SHAPE and b"480" in lib.rf_last_error()
    assert lib.rf_clip_vision_encode_opts(C.byref(big80), C.byref(_opts(80)), 256, 1, 256, None, None) == RF_ERR_SHAPE and b"480" in lib.rf_last_error()
    w336, k336 = _vision_weights(160, 2, image_size=336)
    assert q(C.byref(w336), C.byref(_opts(80)), 2) == RF_ERR_SHAPE
    rc = lib.rf_text_attention(80, 1, 0, a, 304, a, 304, a, 640, a, 0, a, 304, HEADS, NB, 257, 288, 1.0, None)
    assert rc == RF_ERR_UNSUPPORTED and b"head_dim=80" in lib.rf_last_error()
    rc = lib.rf_text_attention(80, 1, 1, a, 304, a, 304, a, 1088, a, 0, a, 304, HEADS, NB, 500, 512, 1.0, None)
    assert rc == RF_ERR_UNSUPPORTED and b"head_dim=80" in lib.rf_last_error()
    rc = lib.rf_debug_text_attention(80, 1, a, 304, a, 304, a, 2 * 512 + 64, a, 0, a, 304, HEADS, NB, 500, 512, 1.0, None)
    assert rc == RF_ERR_SHAPE and b"S_pad=512" in lib.rf_last_error() and b"480" in lib.rf_last_error()


# ---- LDS image of a chunk (csrc/text.hip, attn80_stream_kernel): attn80_kernel's formulas at S_pad = 96, lane = 16 g + l15 ----------------
CK, VP, KB = 96, 64 * 3, 96 * 160
BUF = KB + 80 * VP


def test_lds_budget_is_independent_of_s_pad_and_fits_two_workgroups():
    assert KB == 15360 and 80 * VP == 15360 and BUF == 30720 and 2 * BUF == 61440
    assert (160 * 1024) // (2 * BUF) == 2 and 2 * (2 * BUF) <= 160 * 1024
    assert (CK // 32) % 2 == 1                                                     # m = 3: odd without a padding block
    assert 2 * (128 * 160 + 80 * 64 * 5) == 92160 and (160 * 1024) // 92160 == 1    # 128-key chunks: one workgroup per CU
    assert BUF % 256 == 0 and KB % 256 == 0                                         # every image starts on a bank row


def test_chunk_k_fragment_reads_are_conflict_free_in_both_buffers():
    # kl + r * 160 + ((4 ds + g) << 4), r = 16 t + l15; the third k-step: chunk 8 + g for g < 2 (idle lanes parked as in test_clip_h_cpu)
    for base in (0, BUF):
        for t in range(CK // 16):
            for ds in range(2):
                assert ways(lambda l: base + (16 * t + (l & 15)) * 160 + ((4 * ds + (l >> 4)) << 4)) == 1
            assert ways(lambda l: base + (16 * t + (l & 15)) * 160 + ((8 + ((l >> 4) & 1)) << 4)) == 1
    assert (CK - 1) * 160 + (9 << 4) + 16 <= KB                                      # the last fragment read ends inside the K image


def test_chunk_vt_fragment_reads_are_conflict_free_in_both_buffers():
    # vl + (16 dt + l15) * VP + b * 64 + ((g ^ swz(l15 >> 2)) << 4)
    for base in (KB, BUF + KB):
        for dt in range(5):
            for b in range(CK // 32):
                assert ways(lambda l: base + (16 * dt + (l & 15)) * VP + b * 64 + (((l >> 4) ^ SWZ[(l & 15) >> 2]) << 4)) == 1
    assert ways(lambda l: (l & 15) * VP + ((l >> 4) << 4)) >= 2                      # the odd pitch without the swizzle
    assert 79 * VP + 2 * 64 + (3 << 4) + 16 <= 80 * VP


def test_chunk_staging_fills_the_images_without_overlap():
    """thread tid, piece i: idx = tid + 256 i -> K piece idx (row idx / 10, chunk idx % 10) while idx < 10 nk; V^T channel idx / 12, 8 keys
    from (idx % 12) * 8 while idx < 960"""
    for nk in (32, 64, 96):
        k_seen, v_seen = set(), set()
        for idx in range(1024):
            if idx < nk * 10:
                assert idx * 16 + 16 <= KB and idx // 10 < nk
                k_seen.add(idx * 16)
            d, m = idx // 12, idx % 12
            if idx < 960 and m * 8 < nk:
                blk, kap = (m * 8) >> 5, (m * 8) & 31
                tile, g0 = kap >> 4, (kap & 15) >> 2
                sw = SWZ[(d & 15) >> 2]
                assert sw == (0x78 >> (2 * ((d & 15) >> 2))) & 3
                for g in (g0, g0 + 1):
                    a = KB + d * VP + blk * 64 + 8 * tile + ((g ^ sw) << 4)
                    assert KB <= a and a + 8 <= BUF
                    v_seen.add(a)
        assert len(k_seen) == nk * 10 and len(v_seen) == 2 * 80 * (nk // 8)
    assert 960 == CK * 10 == 80 * (CK // 8) <= 4 * 256


# ---- config plumbing --------------------------------------------------------------------------------------------------------------------
def test_read_siglip_config_defaults_and_refusals(tmp_path):
    d = str(tmp_path)
    json.dump({"text_config": {}, "vision_config": {}}, open(os.path.join(d, "config.json"), "w"))
    assert SV.read_siglip_config(d) == dict(text_heads=12, vision_heads=12, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, image_size=224,
                                            patch_size=16)
    json.dump({"text_config": {"num_attention_heads": 16, "hidden_size": 1152}, "vision_config": {"num_attention_heads": 16, "image_size": 384,
                                                                                               "patch_size": 14, "hidden_act": "gelu_pytorch_tanh"}},
              open(os.path.join(d, "config.json"), "w"))
    mc = SV.read_siglip_config(d)
    assert (mc["text_heads"], mc["vision_heads"], mc["image_size"], mc["patch_size"]) == (16, 16, 384, 14)
    json.dump({"text_config": {}, "vision_config": {"hidden_act": "gelu"}}, open(os.path.join(d, "config.json"), "w"))
    with pytest.raises(SV.RFError, match="hidden_act"):
        SV.read_siglip_config(d)


def test_geometries_synthetic_state_and_tokenizer():
    assert SV.geometry_names() == ["base_224", "so400m_224", "so400m_384"]
    full, small = SV.geometry("so400m_384")
    assert full["vision"] == dict(hidden=1152, heads=16, inter=4304, layers=27, image_size=384, patch=14) and full["text"]["max_pos"] == 64
    assert small["vision"]["layers"] == small["text"]["layers"] == 2 and small["vision"]["hidden"] // small["vision"]["heads"] == 72
    assert SV.geometry("so400m_224")[0]["vision"]["image_size"] == 224 and (224 // 14) ** 2 == 256
    assert SV.geometry("base_224")[0]["vision"] == dict(hidden=768, heads=12, inter=3072, layers=12, image_size=224, patch=16)
    with pytest.raises(SV.RFError, match="so400m_384"):
        SV.geometry("vit_l14")
    sd = SV.synthetic_siglip_state(R.TINY_322, 3)
    assert sd["vision_model.embeddings.position_embedding.weight"].shape == (529, 144) and sd["vision_model.head.probe"].shape == (1, 1, 144)
    assert float(sd["logit_scale"]) == pytest.approx(np.log(10.0)) and float(sd["logit_bias"]) == -10.0
    ids = SV.synthetic_tokenize(512)(["a cat", "x" * 100])
    assert ids.shape == (2, 64) and ids[0, 5:].tolist() == [1] * 59 and int(ids.max()) < 512 and int(ids.min()) >= 1


def test_threshold_is_carried_and_siglip_sorts_on_the_label_first():
    class Pipe:
        vae = None
    with pytest.raises(SV.RFError, match="VAE"):
        SV.build_from_config({"verifier_args": {"name": "siglip", "threshold": 0.7}, "pipeline_args": {"height": 256, "width": 256}}, Pipe(), True, True)
    seen = {}

    class FakeVerifier:
        def __init__(self, pipe, sd, tok, h, w, model_config, threshold):
            seen.update(threshold=threshold, mc=model_config, hw=(h, w), T=sd["vision_model.embeddings.position_embedding.weight"].shape[0])

    class Pipe2:
        vae = object()

        def enable_hip_vae(self):
            seen["hip_vae"] = True
    real, SV.SiglipScoreVerifier = SV.SiglipScoreVerifier, FakeVerifier
    try:
        SV.build_from_config({"verifier_args": {"name": "siglip", "threshold": 0.7, "geometry": "so400m_224"},
                              "pipeline_args": {"height": 256, "width": 320}}, Pipe2(), synthetic=True, small=True)
        assert seen["threshold"] == 0.7 and seen["hip_vae"] and seen["hw"] == (256, 320) and seen["T"] == 256
        assert seen["mc"]["vision_heads"] == 2 and seen["mc"]["image_size"] == 224 and seen["mc"]["layer_norm_eps"] == 1e-6
        SV.build_from_config({"verifier_args": {"name": "siglip"}, "pipeline_args": {"height": 256, "width": 256}}, Pipe2(), synthetic=True, small=True)
        assert seen["threshold"] == 0.5 and seen["T"] == 729
        with pytest.raises(SV.RFError, match="siglip_model_path"):
            SV.build_from_config({"verifier_args": {"name": "siglip"}, "pipeline_args": {"height": 256, "width": 256}}, Pipe2())
    finally:
        SV.SiglipScoreVerifier = real
    # the runner sends a kind it has no scalar rule for to nvila_sort_key: label first, score second
    kind = "siglip" if "siglip" in search.SORT_KEYS else "nvila"
    assert search.SORT_KEYS[kind] is search.nvila_sort_key
    assert search.select_topk([(0.9, 0), (0.2, 1), (0.6, 1), (0.95, 0)], 3, kind) == [2, 1, 0]          # label 1 by descending score, then label 0 by ASCENDING score (the reference's rule)
    src = open(os.path.join(ROOT, "reflectionflow_amd", "tts", "cli.py")).read()
    assert '"siglip"' in src and "siglip_verifier" in src
