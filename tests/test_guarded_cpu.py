"""The guarded-buffer helper (tests/guarded.py) on CPU tensors: it must see a single byte written into either guard, a
byte written into a row gap, an output element that was never written, and a view off its 256-byte boundary.  No GPU."""
import pytest
import torch

from guarded import ALIGN, GUARD_BEFORE, MIN_GUARD_AFTER, ROW_TILE, Guarded


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8, torch.int32])
def test_fully_written_view_passes(dtype):
    g = Guarded((3, 5, 40), dtype, row_stride=48)
    assert g.ptr() % ALIGN == 0 and g.t.stride() == (5 * 48, 48, 1)
    g.t.copy_(torch.ones(3, 5, 40).to(dtype))
    g.check("dense write")


def test_guard_sizes():
    g = Guarded((7, 8), torch.float32, row_stride=16)
    assert g.offset >= GUARD_BEFORE
    assert g.arena.numel() - g.end >= max(MIN_GUARD_AFTER, ROW_TILE * 16 * 4)
    big = Guarded((3, 1000), torch.float32, row_stride=1024)
    assert big.arena.numel() - big.end >= ROW_TILE * 1024 * 4


def test_poison_is_nan_and_minus_one():
    g = Guarded((4, 16), torch.uint8)
    assert torch.isnan(g.arena.view(torch.bfloat16)).all() and torch.isnan(g.arena.view(torch.float32)).all()
    assert torch.isnan(g.arena.view(torch.float8_e4m3fn).float()).all()
    assert (g.arena.view(torch.int32) == -1).all()


@pytest.mark.parametrize("where", [-1, -GUARD_BEFORE, 0, 1, MIN_GUARD_AFTER - 1])
def test_single_byte_in_a_guard_is_seen(where):
    g = Guarded((10, 24), torch.bfloat16)
    g.t.zero_()
    pos = g.offset + where if where < 0 else g.end + where
    g.arena[pos] = 0x00
    with pytest.raises(AssertionError, match="guard (BEFORE|AFTER)"):
        g.check("guard")


def test_byte_in_a_row_gap_is_seen():
    g = Guarded((6, 20), torch.float32, row_stride=24)
    g.t.zero_()
    g.check("clean")
    g.arena[g.offset + (3 * 24 + 22) * 4 + 1] = 0x12
    with pytest.raises(AssertionError, match="row gap"):
        g.check("gap")
    g.check("gap ignored", gaps=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
def test_unwritten_element_is_seen(dtype):
    g = Guarded((2, 9, 32), dtype, row_stride=40)
    g.t.fill_(3)
    e = (1 * 9 + 8) * 40 + 31                      # element [1, 8, 31]: the last one of the view
    g.arena[g.offset + e * g.esize:g.offset + (e + 1) * g.esize] = 0xFF
    assert g.unwritten() == 1
    with pytest.raises(AssertionError, match="1 of 576 output elements were never written"):
        g.check("unwritten")


def test_a_written_nan_is_not_counted_as_unwritten():
    g = Guarded((4, 8), torch.float32)
    g.t.fill_(float("nan"))       # the canonical NaN 0x7FC00000, not the poison bytes
    assert g.unwritten() == 0


def test_misaligned_view_is_refused():
    with pytest.raises(AssertionError, match="256-byte boundary"):
        Guarded((4, 8), torch.float32, misalign=16)
    g = Guarded((4, 8), torch.float32)
    g.t = g.arena[g.offset + 64:g.offset + 64 + 128].view(torch.float32).view(4, 8)
    with pytest.raises(AssertionError, match="256-byte boundary"):
        g.check("shifted")


def test_view_at_a_chosen_placement_is_accepted_and_still_guarded():
    g = Guarded((4, 8), torch.float32, row_stride=16, align=16, misalign=16)
    assert g.ptr() % ALIGN == 16 and g.ptr() % 16 == 0
    g.t.zero_()
    g.check("placed")
    for before in (True, False):                      # one byte before the view, one byte after it
        h = Guarded((4, 8), torch.float32, row_stride=16, align=16, misalign=16)
        h.t.zero_()
        h.arena[h.offset - 1 if before else h.end] = 0x00
        with pytest.raises(AssertionError, match="guard (BEFORE|AFTER)"):
            h.check("placed")
    g.arena[g.offset + (2 * 16 + 9) * 4] = 0x12
    with pytest.raises(AssertionError, match="row gap"):
        g.check("placed gap")
    i = Guarded((3, 5), torch.int32, fill_int32=7, align=4, misalign=4)
    assert i.ptr() % ALIGN == 4 and (i.arena.view(torch.int32) == 7).all()
    i.t.copy_(torch.arange(15, dtype=torch.int32).view(3, 5))
    i.check("index", written=False)


def test_placement_below_the_asked_alignment_is_refused():
    with pytest.raises(AssertionError, match="8 bytes past a 16-byte boundary"):
        Guarded((4, 8), torch.float32, align=16, misalign=8)


def test_index_arena_holds_a_valid_index():
    g = Guarded((3, 5), torch.int32, fill_int32=7)
    assert (g.arena.view(torch.int32) == 7).all()
    g.t.copy_(torch.arange(15, dtype=torch.int32).view(3, 5))
    g.check("index", written=False)
    g.arena[g.end + 5] = 0x55
    with pytest.raises(AssertionError, match="guard AFTER"):
        g.check("index", written=False)
