"""Test helper: fill patterns for scratch memory and the ONE way the stale-workspace tests touch a workspace.

A workspace is an rf_workspace over a byte tensor with one region that is off limits: the 4 KiB stream-K flag page (a non-zero flag
can make a stream-K launch wait for a partner that never comes).  `Workspace.fill` writes every byte EXCEPT that page, and
`Workspace.call` checks the page is all zero before and after every library call it wraps.  A Workspace is made for one geometry
and never handed to another.

Patterns (every region is filled from its first byte to its last, whatever type the library keeps there):
  zero     what engine.get_workspace / text_hip._Workspace hand out today: the baseline every other run must equal bit for bit
  stale    N(0, 1) values rounded to bf16, reinterpreted as raw bytes: "what the previous call left".  As bf16 finite; as fp32 (two
           words, the high one a finite bf16) finite.  As e4m3fn bytes: the high byte of a bf16 (sign + the upper 7 exponent bits) is
           0x38 .. 0x41 for magnitudes 2^-14 .. 2^4, i.e. +-1.0 .. +-2.25, and stays below 0x7F for every finite bf16: always
           finite; the low byte (one exponent bit + the mantissa) is uniform over 0 .. 255, so 2 bytes in 256 are 0x7F / 0xFF = NaN
           and the rest any finite e4m3fn value
  extreme  every 16-bit word 0x7F7F: bf16 3.39e38 and fp32 (0x7F7F7F7F) 3.39e38, both finite -- any arithmetic on them overflows;
           the e4m3fn byte 0x7F is NaN on purpose (an fp8 region must be fully written before it is read)
  nan      every byte 0xFF: NaN as bf16, fp32 and e4m3fn.  Where the library states that it depends on no byte of a buffer, this
           is the pattern that holds it to that (0 * NaN is not 0, 0 * 3.39e38 is)
"""
import torch

PATTERNS = ("zero", "stale", "extreme", "nan")
POISONS = PATTERNS[1:]


def pattern_words(kind: str, n: int, device, seed: int = 0) -> torch.Tensor:
    """n 16-bit words of a pattern as an int16 tensor"""
    if kind == "zero":
        return torch.zeros(n, dtype=torch.int16, device=device)
    if kind == "stale":
        g = torch.Generator(device=device).manual_seed(1000 + seed)
        return torch.randn(n, generator=g, device=device).to(torch.bfloat16).view(torch.int16)
    if kind == "extreme":
        return torch.full((n,), 0x7F7F, dtype=torch.int16, device=device)
    if kind == "nan":
        return torch.full((n,), -1, dtype=torch.int16, device=device)
    raise ValueError(kind)


def fill_bytes(buf: torch.Tensor, lo: int, hi: int, kind: str, seed: int = 0) -> int:
    """bytes [lo, hi) of the uint8 tensor `buf` <- pattern; returns the bytes written"""
    assert buf.dtype == torch.uint8 and buf.is_contiguous() and 0 <= lo <= hi <= buf.numel()
    n = hi - lo
    if n:
        buf[lo:hi] = pattern_words(kind, (n + 1) // 2, buf.device, seed + lo % 9973).view(torch.uint8)[:n]
    return n


def fill_ranges(total: int, flags: tuple) -> list:
    """the byte ranges of a workspace of `total` bytes a fill writes: everything but the flag page (offset, length)"""
    off, n = flags
    assert 0 <= off and off + n <= total and n == 4096 and off % 256 == 0, (flags, total)
    return [(0, off), (off + n, total)]


class Workspace:
    """An rf_workspace of `total` bytes whose flag page (offset, length) is never written by a test."""

    def __init__(self, total: int, flags: tuple, device, buf: torch.Tensor = None):
        from reflectionflow_amd import _lib
        self.total, self.flags = int(total), (int(flags[0]), int(flags[1]))
        self.ranges = fill_ranges(self.total, self.flags)
        self.buf = torch.zeros(self.total, dtype=torch.uint8, device=device) if buf is None else buf
        assert self.buf.dtype == torch.uint8 and self.buf.numel() == self.total
        self.ws = _lib.rf_workspace()
        self.ws.base, self.ws.bytes = self.buf.data_ptr(), self.total

    def flags_are_zero(self) -> bool:
        off, n = self.flags
        return not bool(self.buf[off:off + n].any())

    def fill(self, kind: str, seed: int = 0) -> int:
        """every byte outside the flag page <- pattern; returns the bytes written (== total - 4096)"""
        n = sum(fill_bytes(self.buf, lo, hi, kind, seed) for lo, hi in self.ranges)
        assert n == self.total - 4096
        assert self.flags_are_zero(), "the fill touched the flag page"
        return n

    def call(self, fn):
        """fn(rf_workspace) with the flag page checked on both sides"""
        torch.cuda.synchronize()
        assert self.flags_are_zero(), "flag page not zero before the call"
        r = fn(self.ws)
        torch.cuda.synchronize()
        assert self.flags_are_zero(), "the library left the flag page non-zero"
        return r


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def assert_live(t: torch.Tensor, what: str):
    """the baseline itself must be a real result: finite and not constant (an all-NaN or all-zero pair would compare equal)"""
    f = t.float()
    assert torch.isfinite(f).all(), f"{what}: the zero-workspace baseline is not finite"
    assert float(f.max()) > float(f.min()), f"{what}: the zero-workspace baseline is constant"


def assert_same_bits(got: torch.Tensor, base: torch.Tensor, what: str):
    assert got.shape == base.shape and got.dtype == base.dtype
    if not torch.equal(bits(got), bits(base)):
        ne = bits(got) != bits(base)
        bad = int(ne.sum())
        nonfinite = int((~torch.isfinite(got.float())).sum())
        raise AssertionError(f"{what}: {bad} of {ne.numel()} 16-bit words differ from the zero-workspace run ({nonfinite} values not finite)")
