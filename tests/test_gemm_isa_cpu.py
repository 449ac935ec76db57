"""Guard the steady-state body of the shipped bf16 GEMM loop (gemm_bf16_pp16e_kernel, RF_PP3_ASM) against the compiler: disassemble
the kernel from the built librf_flux.so and check the loop the hand-placed LDS-DMA pieces sit in.

The steady-state loop is the basic block that holds the asm pieces (`s_add_u32 m0, m0, ...` behind each one) and branches back to
itself.  Per K-tile it must hold the schedule of tile(): 64 MFMAs, 24 ds_read_b128, 8 LDS-DMA pieces, 8 barriers -- and none of the
per-tile overhead the body exists to remove: no s_load, no M0 re-load or s_nop in front of a piece, no conditional branch but the
back-edge."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "reflectionflow_amd", "librf_flux.so")
LLVM = "/opt/rocm/llvm/bin"
KERNEL = "_ZN2rf22gemm_bf16_pp16e_kernelENS_10GemmParamsE"


def _tool(name):
    p = os.path.join(LLVM, name)
    if not os.path.exists(p):
        pytest.skip(f"{name} is not installed")
    return p


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("librf_flux.so is not built")
    d = tmp_path_factory.mktemp("isa")
    fat, co = str(d / "fat.bin"), str(d / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


@pytest.fixture(scope="module")
def kernel_asm(code_object):
    out = subprocess.run([_tool("llvm-objdump"), "-d", "--symbolize-operands", code_object], check=True, capture_output=True, text=True).stdout
    i = out.index(f"<{KERNEL}>:")
    m = re.compile(r"^[0-9a-f]{16} <[^L]", re.M).search(out, i + len(KERNEL))   # the next symbol that is not a local label
    j = m.start() if m else len(out)
    lines = [re.sub(r"\s*//.*$", "", l).strip() for l in out[i:j].splitlines()[1:]]
    return [l for l in lines if l]


def _blocks(lines):
    """Basic blocks as (label, [instructions]); a block ends at a label or after a branch."""
    blocks, label, cur = [], None, []
    for l in lines:
        m = re.match(r"^[0-9a-f]+ <(L\d+)>:$", l)
        if m:
            if cur or label:
                blocks.append((label, cur))
            label, cur = m.group(1), []
            continue
        cur.append(l)
        if l.startswith(("s_branch", "s_cbranch")):
            blocks.append((label, cur))
            label, cur = None, []
    if cur:
        blocks.append((label, cur))
    return blocks


def _steady_loop(lines):
    """(label, instructions) of the steady-state loop, or (None, None)."""
    for label, ins in _blocks(lines):
        if label and any(l.startswith("s_add_u32 m0, m0") for l in ins) and ins[-1].startswith("s_cbranch") and ins[-1].endswith(" " + label):
            return label, ins
    return None, None


def test_steady_loop_schedule(kernel_asm):
    _, ins = _steady_loop(kernel_asm)
    assert ins is not None, "no self-looping block with hand-placed LDS-DMA in gemm_bf16_pp16e_kernel (built with RF_PP3_ASM=0?)"
    ops = [l.split()[0] for l in ins]
    tiles = 2   # one trip of the loop = one pair of K-tiles
    assert ops.count("v_mfma_f32_16x16x32_bf16") == 64 * tiles
    assert ops.count("ds_read_b128") == 24 * tiles
    dma = [k for k, l in enumerate(ins) if l.startswith("buffer_load_dwordx4") and l.endswith("offen lds")]
    assert len(dma) == 8 * tiles
    assert ops.count("s_barrier") == 8 * tiles
    # the only wait on global memory: vmcnt(8) in phases p0 and p2, as tile() has it
    assert [l for l in ins if "vmcnt" in l] == ["s_waitcnt vmcnt(8)"] * (2 * tiles)
    assert not [o for o in ops if o.startswith("s_load")], "scalar loads inside the steady-state loop"
    assert ops.count("s_cbranch_scc0") + ops.count("s_cbranch_scc1") + ops.count("s_cbranch_vccz") + ops.count("s_cbranch_vccnz") + \
        ops.count("s_cbranch_execz") + ops.count("s_cbranch_execnz") == 1 and ops.count("s_branch") == 0
    for k in dma:
        # M0 is advanced behind the previous piece; nothing re-loads it in front of this one, and no s_nop sits right before it
        # except the single wait state between the two pieces of one stage (SALU write of M0 -> LDS-DMA)
        prev = ins[k - 1]
        assert not prev.startswith("s_mov_b32 m0"), f"M0 re-loaded in front of a piece: {prev}"
        if prev.startswith("s_nop"):
            assert ins[k - 2].startswith("s_add_u32 m0, m0, 0x2000") and ins[k - 3] == ins[k].replace(ins[k].split()[1], ins[k - 3].split()[1]), \
                "s_nop in front of a piece that does not follow its stage's first piece"
    writes_m0 = [l for l in ins if re.match(r"^s_\w+ m0,", l)]
    assert all(l.startswith("s_add_u32 m0, m0, ") for l in writes_m0) and len(writes_m0) == len(dma)


def test_compiler_dma_sets_m0(kernel_asm):
    """Every LDS-DMA piece the COMPILER emitted (outside the hand-placed loop) finds its M0 written earlier in its own basic block:
    none relies on an M0 value from before an asm statement."""
    steady, _ = _steady_loop(kernel_asm)
    assert steady is not None
    for label, ins in _blocks(kernel_asm):
        if label == steady:
            continue
        for k, l in enumerate(ins):
            if l.startswith("buffer_load_dword") and l.endswith(" lds"):
                assert any(re.match(r"^s_\w+ m0,", p) for p in ins[:k]), f"compiler LDS-DMA without an M0 write in its block {label}: {l}"


def test_registers_and_scratch(code_object):
    out = subprocess.run([_tool("llvm-readelf"), "--notes", code_object], check=True, capture_output=True, text=True).stdout
    meta = None
    for b in re.split(r"\n\s*- \.(?=agpr_count|args)", out):
        if re.search(r"\.name:\s+" + re.escape(KERNEL) + r"\s", b):
            meta = b
    assert meta is not None
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", "." + meta).group(1))   # noqa: E731
    assert get("vgpr_count") + get("agpr_count") <= 256
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0
    assert get("private_segment_fixed_size") == 0
