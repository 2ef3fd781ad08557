"""The whole forward refuses a bad pruning schedule or logits stride before its first launch: the keep range, the keep
buffers and the logits row stride depend on the plan alone (token counts are data independent), so they are checked behind
check_plan / check_ext and in front of the workspace-size refusal.  No GPU: every plan here has workspace = NULL, so
whichever way a check goes nothing is launched, and the weight / image / logits addresses are fakes nobody follows."""
import ctypes as C

import pytest

from rajni_amd import _native as nat

FAKE = 0x10000          # 16-byte aligned, never dereferenced
ERR_INVALID = 1         # RAJNI_ERR_INVALID
IMAGES, LOGITS = FAKE + 0x100, FAKE + 0x200


def _plan(keeps=(0, 0, 0, 0), buffers=(), logits_ld=0):
    """img 64 / patch 16 (16 patch tokens), depth 4, C 128 = 2 x 64, hidden 512, 16 classes, bf16; blocks listed in `buffers`
    get keep_idx and next_scores"""
    depth = len(keeps)
    blocks = (nat.Block * depth)()
    for i, k in enumerate(keeps):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, FAKE)
        blocks[i].keep = k
        if i in buffers:
            blocks[i].keep_idx = blocks[i].next_scores = FAKE
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = 128, 2, 64, depth, 512, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-6, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, FAKE)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.logits_ld = logits_ld
    return p, blocks      # (the caller keeps `blocks` alive)


def _forward(p, prefix=None):
    lib = nat.lib()
    if prefix is None:
        rc = lib.rajni_vit_forward(C.byref(p), IMAGES, LOGITS, None)
    else:
        rc = lib.rajni_vit_forward_ext_prefix(C.byref(p), None, C.byref(prefix), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _control(prefix=None):
    """the same plan with a valid schedule and buffers passes every check up front and stops at the missing workspace:
    each refusal below is the defect's, and nothing was launched on the way to it"""
    p, keep_alive = _plan(keeps=(0, 8, 6, 0), buffers=(1, 2))
    rc, msg = _forward(p, prefix)
    assert rc == ERR_INVALID and "workspace too small" in msg, msg
    del keep_alive


@pytest.mark.parametrize("keeps, buffers, message", [
    ((0, 17, 0, 0), (1,), "block 1: keep=17 but only 16 patch tokens"),
    ((0, 8, 9, 0), (1,), "block 2: keep=9 but only 8 patch tokens"),        # the walk follows the pruning
    ((0, 17, 0, 0), (), "block 1: keep=17 but only 16 patch tokens"),         # range before buffers
])
def test_keep_beyond_the_patch_tokens_entering_the_block(keeps, buffers, message):
    _control()
    p, keep_alive = _plan(keeps=keeps, buffers=buffers)
    rc, msg = _forward(p)
    assert rc == ERR_INVALID and msg == message, msg
    del keep_alive


def test_prefix_tokens_do_not_count_as_patch_tokens():
    p, keep_alive = _plan(keeps=(0, 17, 0, 0), buffers=(1,))
    pre = nat.VitPrefix()
    pre.num_prefix, pre.reg_token = 5, FAKE
    _control(pre)
    rc, msg = _forward(p, pre)
    assert rc == ERR_INVALID and msg == "block 1: keep=17 but only 16 patch tokens", msg
    del keep_alive


@pytest.mark.parametrize("missing", ["keep_idx", "next_scores"])
def test_a_scheduled_block_without_its_buffers(missing):
    _control()
    p, blocks = _plan(keeps=(0, 8, 0, 0), buffers=(1,))
    setattr(blocks[1], missing, None)
    rc, msg = _forward(p)
    assert rc == ERR_INVALID and msg == "block 1: keep_idx/next_scores buffers missing", msg


@pytest.mark.parametrize("ld", [12, 8])     # not a multiple of 8; smaller than the 16 classes
def test_logits_row_stride(ld):
    _control()
    p, keep_alive = _plan(logits_ld=ld)
    rc, msg = _forward(p)
    assert rc == ERR_INVALID, msg
    assert msg == f"rajni_vit_forward: logits row stride must be a multiple of 8 and >= num_classes ({ld})", msg
    del keep_alive
