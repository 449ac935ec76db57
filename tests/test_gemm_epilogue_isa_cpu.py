"""Guard the kind-specialised interior epilogue of the shipped bf16 GEMM (epi16_interior in gemm_bf16_pp16e_kernel) against the
compiler: disassemble the kernel from the built librf_flux.so and check the code after the last MFMA.

Every interior body (STORE, GELU, GATE_RES with / without residual, Q and K with / without RMSNorm + RoPE, V^T) must be ONE
straight-line basic block holding all of its buffer stores: no per-row exec mask, no kind test, no 64-bit address arithmetic in
the row loops, and no waterfall loop (readfirstlane + exec mask) around a buffer resource.  The kernel keeps 0 scratch and at most
256 VGPRs.  (The generic gemm_epilogue_lds_v stays in the kernel as the edge-tile path; it is not checked here.)"""
import collections
import re
import subprocess

import pytest

from tests.test_gemm_isa_cpu import KERNEL, _blocks, _tool, code_object, kernel_asm   # noqa: F401  (fixtures)

STORES = ("buffer_store_dwordx4", "buffer_store_dwordx2")


def _tail_blocks(lines):
    last = max(i for i, l in enumerate(lines) if l.startswith("v_mfma"))
    return _blocks(lines[last + 1:])


def test_interior_bodies_are_straight_line(kernel_asm):
    bodies = [b for _, b in _tail_blocks(kernel_asm) if any(l.startswith(STORES) for l in b)]
    # STORE, GELU, GATE_RES x2, Q x2, K x2, V^T
    assert len(bodies) == 9, [len(b) for b in bodies]
    for b in bodies:
        c = collections.Counter(l.split()[0] for l in b)
        n16, n8 = c["buffer_store_dwordx4"], c["buffer_store_dwordx2"]
        assert (n16, n8) in ((16, 0), (0, 32)), (n16, n8)      # every store of the wave's 64 x 128 sub-tile in one block
        assert c["s_and_saveexec_b64"] == 0 and c["s_or_b64"] == 0, "per-row exec masks in an interior body"
        assert c["v_lshl_add_u64"] <= 1 and c["v_lshlrev_b64"] == 0, "64-bit address arithmetic in an interior body"
        assert c["v_readfirstlane_b32"] == 0, "waterfall loop around a buffer resource"
        assert not any(k.startswith("global_store") for k in c), "an interior body falls back to 64-bit stores"


def test_epilogue_tail_size(kernel_asm):
    """Counts after the last MFMA: the interior bodies add code but no exec-mask or 64-bit-address work (HEAD before the interior
    bodies: 242 s_and_saveexec_b64, 555 v_lshl_add_u64, 192 v_lshlrev_b64 -- all of it now in the edge-tile path only)."""
    tail = [l for _, b in _tail_blocks(kernel_asm) for l in b]
    c = collections.Counter(l.split()[0] for l in tail)
    assert c["s_and_saveexec_b64"] <= 260
    assert c["v_lshl_add_u64"] <= 600
    assert c["buffer_store_dwordx4"] == 128 and c["buffer_store_dwordx2"] == 32


def test_no_scratch_and_vgpr_budget(code_object):
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", code_object], check=True, capture_output=True, text=True).stdout
    i = notes.index(f".name:           {KERNEL}")
    j = notes.find(".name:", i + 10)
    # the metadata of one kernel: the fields before and after its .name
    start = notes.rfind("- .agpr_count", 0, i)
    block = notes[start:j if j > 0 else len(notes)]
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert scratch == 0
    assert vgpr <= 256
