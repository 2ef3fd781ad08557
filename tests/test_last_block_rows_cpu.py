"""Which plans compute their last block for the CLS rows only: the host-side eligibility test of vit_forward through
rajni_debug_last_block_cls_rows (include/rajni_hip_debug.h).  No GPU: nothing is launched, no device pointer is followed."""
import ctypes as C

import pytest

from rajni_amd import _native as nat


def _plan(depth=4, keeps=(0, 6, 0, 0), img=64, patch=16):
    blocks = (nat.Block * depth)()
    for i, k in enumerate(keeps):
        blocks[i].keep = k
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, img, patch
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = 128, 2, 64, depth, 512, 10
    p.blocks = blocks
    return p, blocks      # (the caller keeps `blocks` alive)


def _eligible(p, ext=None, prefix=None):
    return nat.lib().rajni_debug_last_block_cls_rows(C.byref(p), C.byref(ext) if ext is not None else None,
                                                     C.byref(prefix) if prefix is not None else None)


def test_the_default_plan_is_eligible_and_each_exclusion_is_honoured():
    lib = nat.lib()
    p, keep_alive = _plan()
    assert _eligible(p) == 1
    assert _eligible(p, nat.VitExt()) == 1                       # an all-zero ext record: token pooling
    ext = nat.VitExt()
    ext.pool = nat.POOL_AVG                                      # every row of the last block is averaged
    assert _eligible(p, ext) == 0
    for field in ("act_fp8", "cls_only_last_block"):             # they keep the opt-in's own branch
        setattr(p, field, 1)
        assert _eligible(p) == 0
        setattr(p, field, 0)
    pruning, keep_alive2 = _plan(keeps=(0, 6, 0, 3))             # the last block is a pruning stage
    assert _eligible(pruning) == 0
    try:
        lib.rajni_debug_set_last_block_all_rows(1)
        assert _eligible(p) == 0
    finally:
        lib.rajni_debug_set_last_block_all_rows(0)
    assert _eligible(p) == 1
    del keep_alive, keep_alive2


def test_token_count_entering_the_last_block():
    # one patch (16 x 16 image) and the class token: N = 2 is eligible ...
    p, keep_alive = _plan(depth=2, keeps=(0, 0), img=16)
    assert _eligible(p) == 1
    # ... registers count as tokens (1 patch + CLS + 4 registers) ...
    pre = nat.VitPrefix()
    pre.num_prefix = 5
    pre.reg_token = 0x1000
    assert _eligible(p, None, pre) == 1
    # ... and a stream that is one row per image already has nothing to skip
    p.img_size = 8
    assert _eligible(p) == 0
    del keep_alive


@pytest.mark.parametrize("bad", ["null", "no_blocks"])
def test_malformed_plans_are_not_eligible(bad):
    if bad == "null":
        assert nat.lib().rajni_debug_last_block_cls_rows(None, None, None) == 0
    else:
        p, _ = _plan()
        p.blocks = C.POINTER(nat.Block)()
        assert _eligible(p) == 0
