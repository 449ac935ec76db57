"""CPU: rf_debug_workspace_layout / rf_debug_text_workspace_layout are pure arithmetic, and the fill helper of the stale-workspace
tests (tests/workspace_poison.py) covers every region of the engine workspace except the stream-K flag page."""
import ctypes as C

import pytest

from tests.workspace_poison import fill_ranges


@pytest.fixture(scope="module")
def L():
    from reflectionflow_amd import _lib
    _lib.load()
    return _lib


def dims(L, St, Si, Sc, fp8, D=256, heads=2, mlp=1024):
    d = L.rf_flux_dims()
    d.D, d.heads, d.mlp, d.S_txt, d.S_img, d.S_cond, d.fp8 = D, heads, mlp, St, Si, Sc, fp8
    return d


@pytest.mark.parametrize("St,Si,Sc", [(19, 64, 0), (19, 64, 64), (64, 192, 0), (1, 64, 0), (512, 4096, 1024)])
@pytest.mark.parametrize("fp8", [0, 1])
def test_engine_layout_tiles_the_workspace_and_the_fill_covers_it(L, St, Si, Sc, fp8):
    big = St == 512
    d = dims(L, St, Si, Sc, fp8, *((3072, 24, 12288) if big else ()))
    total = int(L.load().rf_workspace_bytes(C.byref(d)))
    lay = L.workspace_layout(d)
    assert list(lay) == list(L.WS_REGIONS)
    S = St + Si + Sc
    s_pad = (S + 63) // 64 * 64
    assert lay["q"][1] == lay["k"][1] == lay["vt"][1] == d.heads * s_pad * 128 * 2          # pad rows / key columns included
    assert lay["xn"][1] == lay["att"][1] == lay["x"][1] == S * d.D * 2 and lay["lt"][1] == S * 256 * 2 and lay["hid"][1] == S * d.mlp * 2
    assert lay["sk_flags"][1] == 4096 and lay["sk_partials"][0] == lay["sk_flags"][0] + 4096
    f8 = [lay[n] for n in ("xn8", "a8", "s_xn", "s_a")]
    assert [n for _, n in f8] == ([S * d.D, S * (d.D + d.mlp), S * 4, S * 4] if fp8 else [0, 0, 0, 0])
    # the regions follow one another on 256-byte boundaries with less than 256 bytes between them, and end at rf_workspace_bytes
    end = 0
    for name, (off, n) in lay.items():
        if n == 0:
            continue
        assert off % 256 == 0 and 0 <= off - end < 256, (name, off, end)
        end = off + n
    assert 0 <= total - end < 256
    # the fill: everything but the flag page, so every other region lies inside it
    ranges = fill_ranges(total, lay["sk_flags"])
    assert sum(hi - lo for lo, hi in ranges) == total - 4096
    for name, (off, n) in lay.items():
        if name != "sk_flags" and n:
            assert any(lo <= off and off + n <= hi for lo, hi in ranges), name
    out = (C.c_int64 * 28)()
    assert L.load().rf_debug_workspace_layout(C.byref(d), out, 13) == -1 and L.load().rf_debug_workspace_layout(None, out, 14) == -3


def test_tower_layout_puts_the_gemm_scratch_last(L):
    total = 5 * (1 << 20) + 4096 + (64 << 20)
    lay = L.text_workspace_layout(total)
    assert lay["sk_flags"] == (5 * (1 << 20), 4096) and lay["sk_partials"] == (5 * (1 << 20) + 4096, 64 << 20)
    assert sum(hi - lo for lo, hi in fill_ranges(total, lay["sk_flags"])) == total - 4096
    out = (C.c_int64 * 4)()
    assert L.load().rf_debug_text_workspace_layout(4096, out, 2) == -1
