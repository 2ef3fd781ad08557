"""Large device buffers for the large-offset tests (tests/test_gpu_large_offsets.py): tensors whose used region reaches past
2^31 bytes, 2^32 bytes and 2^31 elements from the base pointer.

tests/guarded.py fills its whole arena with a pattern and compares all of it; at 4-14 GiB per operand that is not affordable.
The helpers here allocate with torch.empty and touch only what a test uses:
  - `Big` (one per test, the `big` fixture of the test module): allocations that are counted against a hard cap of 24 GiB held
    at once and freed when the test ends; an allocation the device has no room for skips the test, with the numbers;
  - strided row views: rows [M, K] written at a row stride `ld` into such a buffer, [M, N] read back - only the rows' bytes;
  - `periodic_fill` / `assert_periodic`: a dense [rows, C] tensor holding a block of P rows over and over (P prime, so a
    wrap of an offset by 2^31 or 2^32 lands on another phase of the period and shows), filled and compared on the device;
  - `tail_slice`: the same memory seen from a pointer advanced to a row or image boundary past a threshold.
Nothing here loops over elements from Python or copies a large tensor to the host.
"""
from __future__ import annotations

import contextlib
import math
from typing import List

import torch

GIB = 1 << 30
CAP_BYTES = 24 * GIB        # no test may hold more device memory than this through these helpers
HEADROOM_BYTES = 2 * GIB    # free memory required beyond an allocation
PERIOD = 4099               # prime: rows (or images) per period of the periodic fills
T31, T32 = 1 << 31, 1 << 32
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def element_size(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


class Big:
    """The large allocations of ONE test: counted, capped, freed together by close()."""

    def __init__(self, device="cuda", cap: int = CAP_BYTES, mem_get_info=None):
        self.device = device
        self.cap = int(cap)
        self.held = 0
        self.peak = 0
        self._bufs: List[torch.Tensor] = []
        self._mem_get_info = mem_get_info if mem_get_info is not None else (lambda: torch.cuda.mem_get_info())

    def charge(self, nbytes: int) -> None:
        """count `nbytes` more against the cap (also for tensors a kernel wrapper allocates itself)"""
        self.held += int(nbytes)
        self.peak = max(self.peak, self.held)
        assert self.held <= self.cap, f"this test would hold {self.held / GIB:.2f} GiB at once, the cap is {self.cap / GIB:.0f} GiB"

    def reserve(self, nbytes: int) -> int:
        """count `nbytes` against the cap and make sure the device has room for them (+ headroom), else skip the test with the
        numbers.  For tensors the code under test allocates itself (outputs and scratch of the rajni_amd.ops wrappers)."""
        import pytest
        need = int(nbytes)
        self.charge(need)
        free, _total = self._mem_get_info()
        if free < need + HEADROOM_BYTES:
            self.held -= need
            pytest.skip(f"needs {need / GIB:.2f} GiB of device memory (+ {HEADROOM_BYTES / GIB:.0f} GiB headroom), "
                        f"{free / GIB:.2f} GiB are free")
        return need

    def empty(self, nbytes: int, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
        """flat torch.empty tensor of `dtype` covering `nbytes` bytes (rounded up to whole elements); nothing is written"""
        es = element_size(dtype)
        n = (int(nbytes) + es - 1) // es
        self.reserve(n * es)
        t = torch.empty(n, dtype=dtype, device=self.device)
        self._bufs.append(t)
        return t

    def dense(self, shape, dtype) -> torch.Tensor:
        """contiguous tensor of `shape`"""
        return self.empty(math.prod(shape) * element_size(dtype), dtype)[:math.prod(shape)].view(*shape)

    def rows(self, M: int, cols: int, ld: int, dtype) -> torch.Tensor:
        """[M, cols] view whose rows are `ld` elements apart; the buffer ends with the last row (no tail)"""
        assert ld >= cols
        n = (M - 1) * ld + cols
        return self.empty(n * element_size(dtype), dtype).as_strided((M, cols), (ld, 1))

    def close(self) -> None:
        self._bufs.clear()
        self.held = 0
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


@contextlib.contextmanager
def big_empty(nbytes: int, dtype: torch.dtype = torch.uint8, device="cuda", **kw):
    """one large torch.empty allocation on its own: `with big_empty(n, dtype) as t:` - skipped with the numbers when the device
    has no room, counted against the cap, freed (and the allocator's cache emptied) on exit"""
    b = Big(device, **kw)
    try:
        yield b.empty(nbytes, dtype)
    finally:
        b.close()


def row_offset_bytes(t: torch.Tensor, row: int) -> int:
    """byte offset of row `row` of a 2-D (strided) view from its own base pointer"""
    return row * t.stride(0) * t.element_size()


def first_row_past(ld: int, threshold_elems: int) -> int:
    """smallest row index whose start lies at or beyond `threshold_elems` elements at row stride `ld`"""
    return -(-threshold_elems // ld)


def crossings(used_elems: int, esize: int) -> dict:
    """which of the three thresholds a used region of `used_elems` elements of `esize` bytes reaches beyond"""
    return {"2^31 bytes": used_elems * esize > T31, "2^32 bytes": used_elems * esize > T32, "2^31 elements": used_elems > T31}


def assert_crosses_all(used_elems: int, esize: int, what: str) -> None:
    c = crossings(used_elems, esize)
    assert all(c.values()), f"{what}: the used region ({used_elems} elements of {esize} B) does not cross {[k for k, v in c.items() if not v]}"


def bits(t: torch.Tensor) -> torch.Tensor:
    """the same memory as integers of the element's width (bit-for-bit comparisons: NaN == NaN, -0 != +0)"""
    return t.view(_INT_VIEW[t.element_size()])


def periodic_fill(buf_rows: torch.Tensor, block: torch.Tensor) -> None:
    """buf_rows [rows, C] (dense): row r := block[r mod P], block [P, C] on any device.  Doubling copies on the device:
    about log2(rows / P) launches, each row written once."""
    rows, P = buf_rows.shape[0], block.shape[0]
    assert buf_rows.is_contiguous() and buf_rows.shape[1:] == block.shape[1:]
    n = min(P, rows)
    buf_rows[:n].copy_(block[:n].to(buf_rows.device, buf_rows.dtype))
    while n < rows:
        m = min(n, rows - n)
        buf_rows[n:n + m].copy_(buf_rows[:m])       # n is a multiple of P: the phases line up
        n += m


def assert_periodic(out_rows: torch.Tensor, P: int, what: str = "", periods_per_chunk: int = 16) -> None:
    """every row r of out_rows [rows, ...] (dense) is bit-equal to row r mod P; compared on the device in chunks of
    `periods_per_chunk` periods, one host synchronisation at the end.  On failure names the first differing row."""
    rows = out_rows.shape[0]
    if rows <= P:
        return
    flat = bits(out_rows.reshape(rows, -1))
    first = flat[:P]
    step = P * periods_per_chunk
    bad_at = torch.full((1,), rows, dtype=torch.int64, device=out_rows.device)
    for r0 in range(P, rows, step):
        r1 = min(rows, r0 + step)
        full = (r1 - r0) // P
        if full:
            ne = (flat[r0:r0 + full * P].view(full, P, -1) != first).any(dim=-1).view(-1)
            _note_first(ne, r0, bad_at)
        rem = r1 - (r0 + full * P)
        if rem:
            ne = (flat[r0 + full * P:r1] != first[:rem]).any(dim=-1)
            _note_first(ne, r0 + full * P, bad_at)
    b = int(bad_at.item())
    assert b == rows, (f"{what}: row {b} differs from row {b % P} (= {b} mod {P}); row {b} starts "
                       f"{b * flat.shape[1] * flat.element_size()} bytes from the base")


def _note_first(ne: torch.Tensor, r0: int, bad_at: torch.Tensor) -> None:
    idx = torch.where(ne, torch.arange(ne.numel(), device=ne.device) + r0, torch.full_like(bad_at, 1 << 62))
    torch.minimum(bad_at, idx.min().view(1), out=bad_at)


def tail_slice(t: torch.Tensor, start: int) -> torch.Tensor:
    """t[start:] - the same memory from a base pointer advanced to row / image `start` (its offsets start at 0 again)"""
    s = t[start:]
    assert s.data_ptr() == t.data_ptr() + start * t.stride(0) * t.element_size()
    return s


def assert_bit_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got.contiguous()) != bits(want.contiguous())
    n = int(ne.sum())
    if n:
        first = [int(v) for v in ne.nonzero()[0]]
        raise AssertionError(f"{what}: {n} of {ne.numel()} elements differ bit for bit, first at {first}")
