"""Guarded buffers for bounds tests of the kernels: a tensor view carved out of a byte arena that is prefilled with a
poison pattern, with a guard zone before and after it.

The default pattern is the byte 0xFF.  It is NaN in bf16, fp32 and e4m3fn and -1 in int32, and no kernel produces it
from finite inputs (the e4m3 conversions saturate), so one pattern serves three checks:
  - the guard zones are intact, byte for byte (nothing was written outside the view);
  - every element of an output view was written (no element still has all its bytes 0xFF);
  - padding an input view leaves unwritten (row-stride gaps, tails) reaches a result only as NaN.
Index arrays are the exception: their arena holds a VALID index (`fill_int32`) of a row that is itself poisoned, so an
over-read yields NaN data and never an out-of-range address.

The guard before the view is 4 KiB; the guard after it covers at least one full row tile (256 rows x the row stride) and
never less than 64 KiB, so a ragged tile that stores past the last row lands in the guard and not past it.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

POISON = 0xFF
ALIGN = 256
GUARD_BEFORE = 4096
ROW_TILE = 256
MIN_GUARD_AFTER = 64 * 1024


def element_size(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def assert_aligned(t: torch.Tensor, align: int = ALIGN, what: str = "view") -> None:
    off = t.data_ptr() % align
    assert off == 0, f"{what}: data pointer is {off} bytes past a {align}-byte boundary"


class Guarded:
    """`shape` [..., cols] of `dtype` inside a poisoned arena on `device`.  Rows (every leading index, flattened) are
    `row_stride` elements apart (default: cols).  `fill_int32` replaces the 0xFF pattern by an int32 value (index
    arrays).  `after_rows` widens the guard after the view to that many rows (an input whose over-reads may reach
    further than one row tile, like gathered residual rows).  `misalign` starts the view that many bytes past a 256-byte
    boundary and `align` is what the view's pointer must then be a multiple of: the default 256 refuses every `misalign`
    (the self-test sees that), the placement tests ask for `align=16, misalign=16` and the like."""

    def __init__(self, shape: Sequence[int], dtype: torch.dtype, device="cpu", row_stride: Optional[int] = None,
                 fill_int32: Optional[int] = None, after_rows: int = ROW_TILE, misalign: int = 0, align: int = ALIGN):
        self.align = int(align)
        assert self.align > 0 and ALIGN % self.align == 0, f"align must divide {ALIGN} ({align})"
        self.shape = tuple(int(s) for s in shape)
        self.dtype = dtype
        self.esize = element_size(dtype)
        self.cols = self.shape[-1] if self.shape else 1
        self.rows = math.prod(self.shape[:-1]) if len(self.shape) > 1 else 1
        self.ld = self.cols if row_stride is None else int(row_stride)
        assert self.ld >= self.cols, (self.ld, self.cols)
        self.region = self.rows * self.ld * self.esize          # bytes of the view, row gaps included
        after = max(MIN_GUARD_AFTER, max(ROW_TILE, after_rows) * self.ld * self.esize)
        after = (after + ALIGN - 1) // ALIGN * ALIGN
        total = GUARD_BEFORE + 2 * ALIGN + (self.region + ALIGN - 1) // ALIGN * ALIGN + after
        self.arena = torch.empty(total, dtype=torch.uint8, device=device)
        if fill_int32 is None:
            self.pattern = torch.tensor([POISON] * 4, dtype=torch.uint8)
        else:
            self.pattern = torch.tensor([int(fill_int32)], dtype=torch.int32).view(torch.uint8)
        self.arena.view(torch.int32).copy_(self.pattern.view(torch.int32).expand(total // 4))
        base = self.arena.data_ptr()
        self.offset = GUARD_BEFORE + (-(base + GUARD_BEFORE)) % ALIGN + misalign
        self.end = self.offset + self.region
        strides = [1] * len(self.shape)
        if len(self.shape) >= 2:
            strides[-2] = self.ld
            for i in range(len(self.shape) - 3, -1, -1):
                strides[i] = strides[i + 1] * self.shape[i + 1]
        if misalign % self.esize:
            raise ValueError("misalign must be a multiple of the element size")
        flat = self.arena[self.offset:self.offset + max(self.region, self.esize)]
        self.t = flat.view(dtype).as_strided(self.shape, strides)
        assert_aligned(self.t, self.align, what=f"guarded {dtype} {self.shape}")

    # ---- pointers ------------------------------------------------------------------------------
    def ptr(self) -> int:
        return self.t.data_ptr()

    def fill_(self, value: torch.Tensor) -> "Guarded":
        """Copy `value` (any device, the view's shape) into the view; gaps and tails keep the pattern."""
        self.t.copy_(value.reshape(self.shape).to(self.dtype))
        return self

    # ---- checks --------------------------------------------------------------------------------
    def _pattern_at(self, n: int, start: int) -> torch.Tensor:
        p = self.pattern.to(self.arena.device)
        idx = (torch.arange(n, device=self.arena.device) + start) % 4
        return p[idx]

    def _first_bad(self, lo: int, hi: int) -> Optional[int]:
        if hi <= lo:
            return None
        bad = self.arena[lo:hi] != self._pattern_at(hi - lo, lo)
        if not bool(bad.any()):
            return None
        return lo + int(bad.nonzero()[0, 0])

    def guard_damage(self) -> Optional[str]:
        """None when both guard zones hold the pattern, else where the first changed byte is."""
        b = self._first_bad(0, self.offset)
        if b is not None:
            return f"guard BEFORE the view changed at byte {b - self.offset} (relative to the view)"
        a = self._first_bad(self.end, self.arena.numel())
        if a is not None:
            row, col = divmod(a - self.offset, self.ld * self.esize)
            return (f"guard AFTER the view changed at byte {a - self.end} past its end "
                    f"(row {row} col {col // self.esize} at the view's row stride)")
        return None

    def gap_damage(self) -> Optional[str]:
        """None when the row gaps [cols, row_stride) of every row hold the pattern."""
        if self.ld == self.cols:
            return None
        v = self.arena[self.offset:self.end].view(self.rows, self.ld * self.esize)[:, self.cols * self.esize:]
        want = self._pattern_at(self.region, self.offset).view(self.rows, self.ld * self.esize)[:, self.cols * self.esize:]
        bad = (v != want).nonzero()
        if bad.numel() == 0:
            return None
        r, c = int(bad[0, 0]), int(bad[0, 1])
        return f"row gap written: row {r} element {self.cols + c // self.esize} (row width {self.cols}, stride {self.ld})"

    def unwritten(self) -> int:
        """Number of elements of the view whose bytes all still equal 0xFF."""
        v = self.arena[self.offset:self.end].view(self.rows, self.ld * self.esize)[:, :self.cols * self.esize]
        return int((v.view(self.rows, self.cols, self.esize) == POISON).all(dim=-1).sum())

    def check(self, what: str = "", written: bool = True, gaps: bool = True) -> None:
        """Assert the view is aligned as asked (256 bytes by default), both guards are intact, the row gaps are untouched (`gaps`) and every
        element was written (`written`: outputs)."""
        assert_aligned(self.t, self.align, what=what)
        d = self.guard_damage()
        assert d is None, f"{what}: {d}"
        if gaps:
            d = self.gap_damage()
            assert d is None, f"{what}: {d}"
        if written:
            n = self.unwritten()
            assert n == 0, f"{what}: {n} of {self.rows * self.cols} output elements were never written"

