"""CPU: the ViT-H/14 form of the CLIP-score verifier (head dim 80, erf GELU; PickScore / HPSv2 / LAION CLIP-H) -- the additive C ABI
(include/rf_flux.h: rf_clip_tower_opts + the *_opts entry points), its host-side validation (no kernel is launched: there is no GPU
here), the config plumbing of tts/clip_verifier.py and the LDS layout of attn80_kernel (csrc/text.hip) against the bank model of
tests/test_lds_layouts_cpu.py."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import pytest
import torch

from reflectionflow_amd.tts import clip_verifier as CV
from tests import clip_h_ref as H
from tests.test_lds_layouts_cpu import SWZ, ways

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rf_flux.h")
NEW = ["rf_clip_text_workspace_bytes_opts", "rf_clip_text_encode_opts", "rf_clip_vision_workspace_bytes_opts", "rf_clip_vision_encode_opts",
       "rf_gelu_erf_inplace"]


@pytest.fixture(scope="module")
def lib():
    from reflectionflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _run_c(body: str) -> dict:
    src = '#include "rf_flux.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        return dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())


def test_abi_version_and_existing_clip_structs_are_unchanged(lib):
    from reflectionflow_amd import _lib
    assert _lib.ABI_VERSION == 17 and lib.rf_abi_version() == 17
    out = _run_c("".join(f'printf("{s} %zu\\n", sizeof({s}));\n' for s in ("rf_clip_layer", "rf_clip_weights", "rf_clip_vision_weights")))
    # 13 pointers; 8 x int32 + 6 pointers; 10 x int32 + 10 pointers: the v16 / v17 layouts
    assert {k: int(v) for k, v in out.items()} == {"rf_clip_layer": 104, "rf_clip_weights": 80, "rf_clip_vision_weights": 120}
    for s in out:
        assert int(out[s]) == C.sizeof(getattr(_lib, s)), s


def test_header_and_binding_agree_on_the_new_struct_and_prototypes(lib):
    from reflectionflow_amd import _lib
    out = _run_c('printf("size %zu\\n", sizeof(rf_clip_tower_opts));\nprintf("head_dim %zu\\n", offsetof(rf_clip_tower_opts, head_dim));\n'
                 'printf("act %zu\\n", offsetof(rf_clip_tower_opts, act));\nprintf("quick %d\\n", RF_CLIP_ACT_QUICK_GELU);\n'
                 'printf("gelu %d\\n", RF_CLIP_ACT_GELU);\n')
    o = _lib.rf_clip_tower_opts
    assert int(out["size"]) == C.sizeof(o) == 8
    assert int(out["head_dim"]) == o.head_dim.offset == 0 and int(out["act"]) == o.act.offset == 4
    assert (int(out["quick"]), int(out["gelu"])) == (_lib.RF_CLIP_ACT_QUICK_GELU, _lib.RF_CLIP_ACT_GELU) == (0, 1)
    assert _lib.CLIP_ACTS == {"quick_gelu": 0, "gelu": 1}
    # every new prototype: declared, bound, exported, and the binding passes as many arguments of the same kind as the header names
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/rf_flux.h"
        res, args = _lib._SIGS[name]
        assert res is (C.c_int64 if m.group(1) == "int64_t" else C.c_int)
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
                if "rf_clip_tower_opts" in p:
                    assert a is C.POINTER(_lib.rf_clip_tower_opts)
            else:
                assert a is {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]], (name, p, a)
        assert hasattr(raw, name)
    # ... and the old entry points keep their prototypes (argument lists without the opts pointer)
    for old in ("rf_clip_text_workspace_bytes", "rf_clip_text_encode", "rf_clip_vision_workspace_bytes", "rf_clip_vision_encode"):
        new_args = list(_lib._SIGS[old + "_opts"][1])
        assert new_args.pop(1) is C.POINTER(_lib.rf_clip_tower_opts) and new_args == list(_lib._SIGS[old][1])


def _vision_weights(hidden, heads, inter=320, image_size=224, patch=14):
    from reflectionflow_amd import _lib
    w = _lib.rf_clip_vision_weights()
    layers = (_lib.rf_clip_layer * 2)()
    g = image_size // patch
    w.layers, w.hidden, w.heads, w.inter, w.image_size, w.patch, w.proj_dim = 2, hidden, heads, inter, image_size, patch, 64
    w.mask_S, w.eps = (g * g + 1 + 31) // 32 * 32, 1e-5
    for n in ("patch_w", "class_embed", "pos_embed", "pre_ln_scale", "pre_ln_shift", "post_ln_scale", "post_ln_shift", "proj", "mask"):
        setattr(w, n, 256)                                # never dereferenced: the size query validates and adds
    w.layer = C.cast(layers, C.POINTER(_lib.rf_clip_layer))
    return w, layers


def _opts(head_dim, act=1):
    from reflectionflow_amd import _lib
    o = _lib.rf_clip_tower_opts()
    o.head_dim, o.act = head_dim, act
    return o


def test_vision_workspace_query_validates_head_dim_geometry_and_the_lds_limit(lib):
    q = lib.rf_clip_vision_workspace_bytes_opts
    w, keep = _vision_weights(160, 2)
    n = q(C.byref(w), C.byref(_opts(80)), 3)
    assert n > 0
    assert lib.rf_clip_vision_workspace_bytes(C.byref(w), 3) == -1          # the v16 entry point is {64, quick_gelu}: 160 != 2 * 64
    # the operands whose K axis is the hidden width are pitched to the GEMM's 64-element K-tile: the workspace of hidden 160 is hidden 192's
    w192, keep192 = _vision_weights(192, 3)
    assert n == q(C.byref(w192), C.byref(_opts(64, 0)), 3) == lib.rf_clip_vision_workspace_bytes(C.byref(w192), 3)
    assert q(C.byref(w), C.byref(_opts(72)), 1) == -5 and b"head_dim=72" in lib.rf_last_error()
    assert q(C.byref(w), C.byref(_opts(80, 2)), 1) == -5 and b"act=2" in lib.rf_last_error()
    w168, keep168 = _vision_weights(168, 2)
    assert q(C.byref(w168), C.byref(_opts(80)), 1) == -1 and b"heads * head_dim" in lib.rf_last_error()
    assert q(C.byref(w), C.byref(_opts(64)), 1) == -1                       # 160 = 2 x 80, not 2 x 64
    assert q(C.byref(w), None, 1) == -3
    # 308 / 14 = 22: 485 tokens -> S_pad 512 keys.  Head dim 64 holds them in the LDS, head dim 80 does not (limit 480)
    big64, k64 = _vision_weights(128, 2, image_size=308)
    assert big64.mask_S == 512 and q(C.byref(big64), C.byref(_opts(64, 0)), 1) > 0
    big80, k80 = _vision_weights(160, 2, image_size=308)
    assert q(C.byref(big80), C.byref(_opts(80)), 1) == -1
    msg = lib.rf_last_error()
    assert b"S_pad=512" in msg and b"480" in msg and b"LDS" in msg, msg
    assert lib.rf_clip_vision_encode_opts(C.byref(big80), C.byref(_opts(80)), 256, 1, 256, None, None) == -1 and b"480" in lib.rf_last_error()
    # 294 / 14 = 21: 442 tokens -> S_pad 448 <= 480 fits
    ok80, kok = _vision_weights(160, 2, image_size=294)
    assert ok80.mask_S == 448 and q(C.byref(ok80), C.byref(_opts(80)), 1) > 0


def test_text_workspace_query_takes_the_same_opts(lib):
    from reflectionflow_amd import _lib
    w = _lib.rf_clip_weights()
    layers = (_lib.rf_clip_layer * 2)()
    w.layers, w.hidden, w.heads, w.inter, w.vocab, w.max_pos, w.eps = 2, 160, 2, 320, 300, 77, 1e-5
    for n in ("tok_embed", "pos_embed", "final_ln_scale", "final_ln_shift"):
        setattr(w, n, 256)
    w.layer = C.cast(layers, C.POINTER(_lib.rf_clip_layer))
    q = lib.rf_clip_text_workspace_bytes_opts
    assert q(C.byref(w), C.byref(_opts(80)), 2, 77) > 0
    assert q(C.byref(w), C.byref(_opts(72)), 2, 77) == -5
    assert q(C.byref(w), C.byref(_opts(64)), 2, 77) == -1 and lib.rf_clip_text_workspace_bytes(C.byref(w), 2, 77) == -1
    w.hidden = 128
    assert q(C.byref(w), C.byref(_opts(64, 1)), 2, 77) == lib.rf_clip_text_workspace_bytes(C.byref(w), 2, 77) > 0
    w.hidden, w.max_pos = 160, 512
    assert q(C.byref(w), C.byref(_opts(80)), 1, 480) > 0
    assert q(C.byref(w), C.byref(_opts(80)), 1, 481) == -1 and b"480" in lib.rf_last_error()
    assert lib.rf_gelu_erf_inplace(None, 8, None) == -3 and lib.rf_gelu_erf_inplace(256, 12, None) == -1


VIT_H_CONFIG = {   # the fields of laion/CLIP-ViT-H-14-laion2B-s32B-b79K's (= PickScore_v1's) config.json the verifier reads
    "model_type": "clip", "projection_dim": 1024, "logit_scale_init_value": 2.6592,
    "text_config": {"hidden_size": 1024, "intermediate_size": 4096, "num_attention_heads": 16, "num_hidden_layers": 24, "hidden_act": "gelu",
                    "layer_norm_eps": 1e-5, "max_position_embeddings": 77, "vocab_size": 49408, "eos_token_id": 49407, "bos_token_id": 49406,
                    "pad_token_id": 1},
    "vision_config": {"hidden_size": 1280, "intermediate_size": 5120, "num_attention_heads": 16, "num_hidden_layers": 32, "hidden_act": "gelu",
                      "layer_norm_eps": 1e-5, "image_size": 224, "patch_size": 14}}


def test_load_clip_dir_reads_heads_activation_and_eos_from_config_json(tmp_path):
    from safetensors.torch import save_file
    from reflectionflow_amd.ops import RFError
    d = str(tmp_path)
    json.dump(VIT_H_CONFIG, open(os.path.join(d, "config.json"), "w"))
    save_file({"text_projection.weight": torch.zeros(1024, 8), "logit_scale": torch.tensor(2.6592)}, os.path.join(d, "model.safetensors"))
    # the smallest CLIP BPE vocabulary: the two specials and one word
    json.dump({"<|startoftext|>": 0, "<|endoftext|>": 1, "a</w>": 2}, open(os.path.join(d, "vocab.json"), "w"))
    open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\n")
    sd, tokenize, mc = CV.load_clip_dir(d)
    assert (mc["text_heads"], mc["vision_heads"], mc["hidden_act"], mc["eos_token_id"]) == (16, 16, "gelu", 49407)
    assert mc["layer_norm_eps"] == 1e-5 and mc["projection_dim"] == 1024
    assert set(sd) == {"text_projection.weight", "logit_scale"}
    ids = tokenize(["a"])
    assert ids.shape == (1, 77) and ids[0, :3].tolist() == [0, 2, 1]
    assert mc == CV.read_clip_config(d)
    # head dims that follow: 64 on the text tower, 80 on the vision tower
    assert 1024 // mc["text_heads"] == 64 and 1280 // mc["vision_heads"] == 80
    # a config without the keys is OpenAI's legacy form; towers with two activations are refused
    json.dump({"text_config": {"num_attention_heads": 12}, "vision_config": {"num_attention_heads": 16}, "projection_dim": 768},
              open(os.path.join(d, "config.json"), "w"))
    mc = CV.read_clip_config(d)
    assert (mc["text_heads"], mc["vision_heads"], mc["hidden_act"], mc["eos_token_id"]) == (12, 16, "quick_gelu", 2)
    json.dump({"text_config": {"hidden_act": "gelu"}, "vision_config": {"hidden_act": "quick_gelu"}}, open(os.path.join(d, "config.json"), "w"))
    with pytest.raises(RFError, match="hidden_act"):
        CV.read_clip_config(d)


def test_geometry_tables_and_the_pickscore_alias():
    from reflectionflow_amd.tts import search
    h = CV.VIT_H14
    assert h["text"] == dict(vocab=49408, hidden=1024, heads=16, inter=4096, layers=24, max_pos=77)
    assert h["vision"] == dict(hidden=1280, heads=16, inter=5120, layers=32, image_size=224, patch=14)
    assert h["projection_dim"] == 1024 and h["act"] == "gelu"
    assert CV.GEOMETRIES == {"vit_l14": (CV.VIT_L14, CV.TINY), "vit_h14": (CV.VIT_H14, CV.TINY_H)}
    th = CV.TINY_H
    assert th["vision"]["hidden"] // th["vision"]["heads"] == 80 and th["vision"]["layers"] == th["text"]["layers"] == 2 and th["act"] == "gelu"
    assert CV.tower_config(h) == dict(text_heads=16, vision_heads=16, hidden_act="gelu")
    assert CV.tower_config(CV.VIT_L14) == dict(text_heads=12, vision_heads=16, hidden_act="quick_gelu")
    # the synthetic state dict is driven by shapes only: it fills every parameter of transformers' CLIPModel of the geometry
    sd = CV.synthetic_clip_state(th, 0)
    assert sd["vision_model.encoder.layers.1.mlp.fc1.weight"].shape == (320, 160)
    H.hf_clip_model(th, sd)                                # strict: asserts no missing / unexpected key
    shapes = {k: tuple(v.shape) for k, v in CV.synthetic_clip_state(dict(h, text=dict(h["text"], layers=1, vocab=8),
                                                                          vision=dict(h["vision"], layers=1)), 0).items()}
    assert shapes["vision_model.encoder.layers.0.self_attn.q_proj.weight"] == (1280, 1280)
    assert shapes["text_projection.weight"] == (1024, 1024) and shapes["visual_projection.weight"] == (1024, 1280)
    assert search.SORT_KEYS["pickscore"] is search.scalar_sort_key
    assert search.select_topk([(0.5, 1), (0.9, 1), (0.5, 1), (0.7, 1)], 3, "pickscore") == [1, 3, 0]


def test_weight_packing_folds_the_head_dim_scale_and_pads_k():
    from reflectionflow_amd.flux import text_hip as TH
    w = torch.arange(6.0).reshape(2, 3)
    p = TH._kpad(w)
    assert p.shape == (2, 64) and torch.equal(p[:, :3], w) and float(p[:, 3:].abs().max()) == 0.0
    w64 = torch.ones(2, 128)
    assert TH._kpad(w64) is w64
    with pytest.raises(TH.RFError, match="head dim"):
        TH._tower_opts("x", 144, 2, 72, "gelu")
    with pytest.raises(TH.RFError, match="not a head dim"):
        TH._tower_opts("x", 168, 2, 80, "gelu")
    with pytest.raises(TH.RFError, match="hidden_act"):
        TH._tower_opts("x", 160, 2, 80, "relu")
    o = TH._tower_opts("x", 1280, 16, 80, "gelu")
    assert (o.head_dim, o.act) == (80, 1)


# ---- LDS layout of attn80_kernel (csrc/text.hip), lane = 16 g + l15 ---------------------------------------------------------------
S_PADS = (32, 96, 288, 320, 448, 480)


def vpitch(s_pad):
    return 64 * ((s_pad >> 5) | 1)


def test_attn80_lds_budget():
    lds = lambda s: s * 160 + 80 * vpitch(s)  # noqa: E731
    assert lds(288) == 92160 and lds(480) == 153600 <= 160 * 1024 < lds(512)
    assert all(vpitch(s) >= 2 * s and (vpitch(s) // 64) % 2 == 1 for s in range(32, 513, 32))


def test_attn80_k_fragment_reads_are_conflict_free():
    # kl + r * 160 + ((4 ds + g) << 4) for the whole k-steps ds = 0, 1 (channels 0 .. 63), r = 16 t + l15: the row as it lies in memory
    for t in range(30):
        for ds in range(2):
            assert ways(lambda l: (16 * t + (l & 15)) * 160 + ((4 * ds + (l >> 4)) << 4)) == 1
    # channels 64 .. 79: kl + r * 160 + ((8 + g) << 4), read by the lanes with g < 2 only (the others hold zeros and issue no load);
    # parking the idle lanes of the other two lane groups on chunk 8 + (g & 1) of their row models a read of the same shape
    for t in range(30):
        assert ways(lambda l: (16 * t + (l & 15)) * 160 + ((8 + ((l >> 4) & 1)) << 4)) == 1
    # no fragment read reaches past the row's 10 chunks
    assert max(4 * ds + g for ds in range(2) for g in range(4)) == 7 and max(8 + g for g in range(2)) == 9
    # what does not work: attn64_kernel's 8-chunk xor on 160-byte rows, and an odd pitch of 11 chunks
    assert max(ways(lambda l: (l & 15) * 160 + (((4 * ds + (l >> 4)) ^ ((l & 15) & 7)) << 4)) for ds in range(2)) >= 2
    assert max(ways(lambda l: (l & 15) * 176 + ((4 * ds + (l >> 4)) << 4)) for ds in range(2)) >= 2


def test_attn80_vt_fragment_reads_are_conflict_free_only_with_odd_pitch_and_swizzle():
    # vl + (16 dt + l15) * vpitch + b * 64 + ((g ^ swz(l15 >> 2)) << 4), swz = (0x78 >> 2 h) & 3
    for s_pad in S_PADS:
        vp, base = vpitch(s_pad), s_pad * 160
        for dt in range(5):
            for b in range(s_pad // 32):
                assert ways(lambda l: base + (16 * dt + (l & 15)) * vp + b * 64 + (((l >> 4) ^ SWZ[(l & 15) >> 2]) << 4)) == 1
    assert ways(lambda l: (l & 15) * vpitch(288) + ((l >> 4) << 4)) >= 2                            # odd pitch without the swizzle
    assert ways(lambda l: (l & 15) * 640 + (((l >> 4) ^ SWZ[(l & 15) >> 2]) << 4)) >= 2             # the swizzle on an even pitch (S_pad 320 unpadded)
    assert ways(lambda l: (l & 15) * (2 * 288 + 16) + ((l >> 4) << 4)) == 2                         # attn64_kernel's pitch, for the record
    # staging writes chunk c of a key block at c ^ swz(row): the read side's g ^ swz is its inverse, and the 80 x S_pad / 8 chunks land on
    # distinct addresses inside the V^T array
    for s_pad in (96, 288):
        vp, seen = vpitch(s_pad), set()
        for d in range(80):
            sw = SWZ[(d & 15) >> 2]
            for blk in range(s_pad // 32):
                for c in range(4):
                    a = d * vp + blk * 64 + ((c ^ sw) << 4)
                    assert 0 <= a and a + 16 <= 80 * vp
                    seen.add(a)
                    assert ((c ^ sw) ^ sw) == c
        assert len(seen) == 80 * (s_pad // 8)
