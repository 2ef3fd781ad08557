"""`forward_features(x, dense=True, fill="last")` / RAJNI_POOL_DENSE_LAST without a device: the value's pin, its refusals before
the first launch (the fake-pointer plans of tests/test_features_cpu.py: workspace = NULL, so "workspace too small" means every
check in front of it passed), what the wrapper refuses, the wrapper's exit_block composition against tests/numerics_last.py, and
that the fixture of the device test can tell the two ways to get the tensor wrong."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import numerics_features as nf
import numerics_last as nl
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import compose_exit_block
from test_features_cpu import ERR_INVALID, ERR_UNSUPPORTED, FAKE, FIX, SCHED, _ext, _forward, _plan, _reaches_the_workspace_check, images_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "RAJNI_POOL_DENSE_LAST"


def test_the_value_is_five_and_four_stays_unknown():
    assert nat.POOL_DENSE_LAST == 5
    header = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"RAJNI_POOL_DENSE_LAST\s*=\s*5\b", header)
    for headless in (True, False):
        p, keep_alive = _plan(headless=headless)
        rc, msg = _forward(p, _ext(4))
        assert rc == ERR_UNSUPPORTED and msg == "rajni_vit_forward_ext: pool must be RAJNI_POOL_TOKEN or RAJNI_POOL_AVG (4)", msg
        del keep_alive


def test_a_clean_headless_plan_passes_every_check():
    for keeps, buffers in (((0, 8, 6, 0), (1, 2)), ((0, 0, 0, 0), ()), ((8, 6, 4, 2), (0, 1, 2, 3))):
        p, keep_alive = _plan(keeps, buffers)
        _reaches_the_workspace_check(p, _ext(nat.POOL_DENSE_LAST))
        _reaches_the_workspace_check(p, _ext(nat.POOL_DENSE_LAST, mlp_act=nat.MLP_QUICK_GELU), nat.VitPrefix(5, FAKE))
        p.logits_ld = 128
        _reaches_the_workspace_check(p, _ext(nat.POOL_DENSE_LAST))
        del keep_alive


def test_every_refusal_of_the_dense_output_under_the_new_name():
    headed, k1 = _plan(headless=False)
    rc, msg = _forward(headed, _ext(nat.POOL_DENSE_LAST))
    assert rc == ERR_UNSUPPORTED and NAME in msg and "headless" in msg and "per-token classification" in msg, msg
    p, k2 = _plan()
    for fields in (dict(fc_norm_w=FAKE), dict(norm_absent=1)):
        rc, msg = _forward(p, _ext(nat.POOL_DENSE_LAST, **fields))
        assert rc == ERR_UNSUPPORTED and NAME in msg and "no cast-only row kernel" in msg, msg
    p.cls_only_last_block = 1
    rc, msg = _forward(p, _ext(nat.POOL_DENSE_LAST))
    assert rc == ERR_INVALID and NAME in msg and "cls_only_last_block" in msg, msg
    p.cls_only_last_block = 0
    p.act_fp8 = 1
    rc, msg = _forward(p, _ext(nat.POOL_DENSE_LAST))
    assert rc == ERR_UNSUPPORTED and NAME in msg and "act_fp8" in msg, msg
    p.act_fp8 = 0
    rc, msg = _forward(p, _ext(nat.POOL_DENSE_LAST), nat.VitPrefix(2, FAKE, head_rows=2))
    assert rc == ERR_UNSUPPORTED and NAME in msg and "head_rows=2" in msg, msg
    # the output is dense: the codes of the headless plan's stride refusals
    for ld, code, what in ((64, ERR_INVALID, ">= C"), (132, ERR_INVALID, "multiple of 8"), (256, ERR_UNSUPPORTED, "0 or C")):
        p.logits_ld = ld
        rc, msg = _forward(p, _ext(nat.POOL_DENSE_LAST))
        assert rc == code and NAME in msg and "logits row stride" in msg and what in msg, (ld, rc, msg)
    del k1, k2


def test_the_last_block_runs_all_rows():
    p, keep_alive = _plan()
    e = _ext(nat.POOL_DENSE_LAST)
    assert nat.lib().rajni_debug_last_block_cls_rows(C.byref(p), C.byref(e), None) == 0
    pre = nat.VitPrefix(5, FAKE)
    assert nat.lib().rajni_debug_last_block_cls_rows(C.byref(p), C.byref(e), C.byref(pre)) == 0
    assert nat.lib().rajni_debug_last_block_cls_rows(C.byref(p), None, None) == 1
    del keep_alive


# ---- wrapper ----------------------------------------------------------------------------------------------------------------

def test_fill_takes_zero_or_last_and_last_needs_dense():
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), SCHED)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match='fill="last"'):
        w.forward_features(x, fill="last")
    with pytest.raises(ValueError, match='fill="last"'):
        w.forward_features(x, dense=False, fill="last")
    for bad in ("first", "", None, 0):
        with pytest.raises(ValueError, match='"zero" or "last"'):
            w.forward_features(x, dense=True, fill=bad)
    with pytest.raises(nat.NativeError):            # a legal call: no CPU fallback, as ever
        w.forward_features(x, dense=True, fill="last")
    with pytest.raises(nat.NativeError):
        w.forward_features(x, dense=True, fill="zero")


def test_the_feature_refusals_apply_unchanged():
    """`_check_features` is what every feature plan passes first (the device check sits in front of it in the public call, so
    the helper is called directly, as tests/test_features_cpu.py does); the plan mode exists"""
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro512_patch16_64"), {}).set_weight_format("fp8_mfma")
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w._check_features(w.check_supported())
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), {}).set_last_block_cls_only(True)
    with pytest.raises(ValueError, match="set_last_block_cls_only"):
        w._check_features(w.check_supported())
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_fcnorm_patch16_64"), {})
    with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
        w._check_features(w.check_supported())


def _random_selections(P, n, keeps, B, seed):
    rng, N, out = np.random.default_rng(seed), P + n, {}
    for i, keep in keeps.items():
        out[i] = np.stack([np.concatenate([np.arange(P), P + np.sort(rng.choice(N - P, keep, replace=False))]) for _ in range(B)])
        N = P + keep
    return out


@pytest.mark.parametrize("P, keeps", [(1, {1: 11, 2: 5}), (5, {0: 16, 1: 9, 2: 9, 3: 1}), (1, {}), (2, {3: 1})])
def test_exit_block_composition(P, keeps):
    B, n, depth = 3, 16, 4
    sel = _random_selections(P, n, keeps, B, seed=3)
    got = compose_exit_block({i: torch.from_numpy(v).to(torch.int32) for i, v in sel.items()}, B, P + n, depth, "cpu")
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, P + n)
    dropped, want = nl.dropped_positions(sel, B, P + n)
    want[want < 0] = depth
    np.testing.assert_array_equal(got.numpy(), want)
    assert (got[:, :P] == depth).all()                       # prefix tokens never leave
    src = nf.compose_source_idx(sel, B, P + n)
    for b in range(B):
        assert (got[b, src[b]] == depth).all() and int((got[b] == depth).sum()) == src.shape[1]
        for i, keep in keeps.items():
            assert int((got[b] == i).sum()) == len(dropped[i][b])


# ---- the restatement, and what the fixture can tell ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_the_restatement_fills_every_row_and_the_fixture_can_tell(name):
    """every pruned position holds the row of the cut-off graph, every other row is `dense`'s; and the two ways to get the tensor
    wrong - zero fill, and dropped rows placed by the current block's indices alone (without composing the earlier maps) - each
    move it by at least 5x the acceptance bar of the 16-bit device test (1e-2 of max|want|)"""
    cfg = ts.config_of(name)
    P = cfg.num_prefix_tokens
    sd = ts.state_dict_numpy(ts.create_model(name, round_bf16=True, **FIX))
    imgs = images_of(cfg, 3, seed=5)
    r = nl.features_last_restated(sd, imgs, SCHED, cfg)
    want, dense, ex, src = r["dense_last"], r["dense"], r["exit_block"], r["source_idx"]
    n0 = cfg.num_patches + P
    assert want.shape == dense.shape == (3, n0, cfg.embed_dim) and ex.shape == (3, n0) and ex.dtype == np.int32
    assert sorted(np.unique(ex)) == [1, 2, cfg.depth] and (ex[:, :P] == cfg.depth).all()
    assert (np.abs(want).max(axis=-1) > 0.1).all(), "no row is zero"
    sel = {i: t["keep_idx"] for i, t in r["trace"].items()}
    for b in range(3):
        assert np.array_equal(np.flatnonzero(ex[b] == cfg.depth), src[b])
        assert np.array_equal(want[b, src[b]], dense[b, src[b]])
        for i in (1, 2):
            rows = np.flatnonzero(ex[b] == i)
            assert len(rows) == r["counts"][i] - sel[i].shape[1]
            assert np.array_equal(want[b, rows], r["entry"][i][b, rows]) and not dense[b, rows].any()
    # block 1 is the first scheduled one: its entry is the unpruned stream behind block 0, every row present
    assert (np.abs(r["entry"][1]).max(axis=-1) > 0.1).all()
    # the second wrong form: block 2's dropped rows land at their index in the stream that ENTERED block 2
    wrong = want.copy()
    for b in range(3):
        j = np.setdiff1d(np.arange(r["counts"][2]), sel[2][b])            # stream indices block 2 drops
        s = sel[1][b, j]                                                   # where they belong
        wrong[b, s] = 0.0
        wrong[b, j] = want[b, s]
    need = 5 * 1e-2 * float(np.abs(want).max())
    for what, bad in (("zero fill", dense), ("current block's indices alone", wrong)):
        moved = float(np.abs(bad - want).max())
        print(f"[features-last] {name}: {what} moves the tensor by {moved:.4g} = {moved / need:.3g} x (5 x bar = {need:.4g})")
        assert moved >= need, (what, moved, need)
    # depth = 0 is the embedded stream: with block 0 scheduled the dropped rows are norm(embed)
    r0 = nl.features_last_restated(sd, imgs, {0: {"keep_ratio": 0.5}}, cfg)
    x0 = nf.features_restated(sd, imgs, {}, dataclasses.replace(cfg, depth=0))["tokens"]
    assert np.array_equal(r0["entry"][0], x0)
    rows = r0["exit_block"] == 0
    assert rows.sum() == 3 * (cfg.num_patches - cfg.num_patches // 2) and np.array_equal(r0["dense_last"][rows], x0[rows])
