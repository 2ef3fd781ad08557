"""Feature outputs without a device: the pins the design rests on (no new entry point, no record or workspace change), the
refusals of the headless plan and of RAJNI_POOL_NONE / RAJNI_POOL_DENSE before the first launch, what the wrapper recognises
and refuses, and the restated graph of tests/numerics_features.py against the base model's own forward_features.

The refusal tests use the fake-pointer plans of tests/test_forward_refusals_cpu.py: workspace = NULL, so "workspace too small"
means every check in front of it passed, and nothing is launched either way."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_features as nf
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
IMAGES, LOGITS = FAKE + 0x100, FAKE + 0x200

# the exported symbols as they stand: a new entry point fails this file
SYMBOLS = """rajni_abi_version rajni_last_error rajni_device_check rajni_importance rajni_select_topk rajni_score_select
rajni_gather_rows rajni_attention rajni_attention_fp8 rajni_layernorm rajni_layernorm_fp8 rajni_linear rajni_qk_norm
rajni_layernorm_stream rajni_pool_norm rajni_debug_force_gemm_tiling rajni_debug_force_f8_tiling rajni_debug_set_resid_stagger
rajni_debug_set_gemm_nblock_bytes rajni_debug_set_persistent_workgroups rajni_debug_linear_plan rajni_debug_force_attention
rajni_debug_attention_rows rajni_debug_set_last_block_all_rows rajni_debug_last_block_cls_rows rajni_debug_force_score_two_pass
rajni_debug_force_score_tiled rajni_debug_set_gemm_stamps rajni_patch_embed_workspace_bytes rajni_patch_embed
rajni_vit_workspace_bytes rajni_vit_forward rajni_vit_forward_ext rajni_select_topk_prefix rajni_score_select_prefix
rajni_score_select_workspace_bytes rajni_score_select_ws rajni_patch_embed_prefix rajni_pool_norm_prefix
rajni_vit_workspace_bytes_prefix rajni_vit_forward_ext_prefix rajni_profile_enable rajni_profile_class_name
rajni_profile_collect rajni_profile_reset""".split()


# ---- pins -------------------------------------------------------------------------------------------------------------------

def test_abi_records_and_symbols_are_what_they_were():
    assert nat.lib().rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.VitPrefix) == 16
    assert (nat.POOL_TOKEN, nat.POOL_AVG, nat.POOL_NONE, nat.POOL_DENSE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"RAJNI_POOL_NONE\s*=\s*2\b", header) and re.search(r"RAJNI_POOL_DENSE\s*=\s*3\b", header)
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", header) and re.search(r"RAJNI_NUM_KCLASS\s*=\s*17\b", header)
    header += open(os.path.join(ROOT, "include", "rajni_hip_debug.h")).read()
    declared = set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", header)) - {"rajni_stream_t"}
    assert set(nat.EXPORTED_SYMBOLS) == declared == set(SYMBOLS)
    assert len(nat.EXPORTED_SYMBOLS) == len(SYMBOLS) == 45


def _plan(keeps=(0, 8, 6, 0), buffers=(1, 2), headless=True, logits_ld=0):
    """the plan of tests/test_forward_refusals_cpu.py (16 patch tokens, depth 4, C 128, bf16), with or without its head"""
    depth = len(keeps)
    blocks = (nat.Block * depth)()
    for i, k in enumerate(keeps):
        for name, _ in nat.Block._fields_[:14]:
            setattr(blocks[i], name, FAKE)
        blocks[i].keep = k
        if i in buffers:
            blocks[i].keep_idx = blocks[i].next_scores = FAKE
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = 128, 2, 64, depth, 512, 0 if headless else 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-6, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b"):
        setattr(p, name, FAKE)
    if not headless:
        p.head_w = p.head_b = FAKE
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.logits_ld = logits_ld
    return p, blocks


def _ext(pool=nat.POOL_TOKEN, **fields):
    e = nat.VitExt()
    e.pool = pool
    for k, v in fields.items():
        setattr(e, k, v)
    return e


def _forward(p, ext=None, prefix=None):
    lib = nat.lib()
    rc = lib.rajni_vit_forward_ext_prefix(C.byref(p), C.byref(ext) if ext is not None else None,
                                          C.byref(prefix) if prefix is not None else None, IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _reaches_the_workspace_check(p, ext=None, prefix=None):
    rc, msg = _forward(p, ext, prefix)
    assert rc == ERR_INVALID and "workspace too small" in msg, (rc, msg)


def test_the_workspace_of_a_headless_plan_is_that_of_the_plan_with_a_head():
    lib = nat.lib()
    with_head, k1 = _plan(headless=False)
    without, k2 = _plan(headless=True)
    assert lib.rajni_vit_workspace_bytes(C.byref(without)) == lib.rajni_vit_workspace_bytes(C.byref(with_head)) > 0
    pre = nat.VitPrefix(5, FAKE)
    assert (lib.rajni_vit_workspace_bytes_prefix(C.byref(without), C.byref(pre))
            == lib.rajni_vit_workspace_bytes_prefix(C.byref(with_head), C.byref(pre)) > 0)
    del k1, k2


# ---- what is accepted: fails on a build without the feature ("null weight pointer" / "pool must be") ------------------------

@pytest.mark.parametrize("ld", [0, 128])
def test_a_headless_plan_passes_every_check(ld):
    p, keep_alive = _plan(logits_ld=ld)
    rc = nat.lib().rajni_vit_forward(C.byref(p), IMAGES, LOGITS, None)
    assert rc == ERR_INVALID and "workspace too small" in nat.lib().rajni_last_error().decode()
    _reaches_the_workspace_check(p)
    _reaches_the_workspace_check(p, _ext())
    _reaches_the_workspace_check(p, _ext(nat.POOL_AVG, fc_norm_w=FAKE))           # gap + fc_norm, no final norm needed ...
    _reaches_the_workspace_check(p, _ext(nat.POOL_AVG, fc_norm_w=FAKE, norm_absent=1))
    _reaches_the_workspace_check(p, _ext(mlp_act=nat.MLP_SWIGLU, norm_pre_w=FAKE), nat.VitPrefix(5, FAKE))
    del keep_alive


@pytest.mark.parametrize("pool", [nat.POOL_NONE, nat.POOL_DENSE])
def test_the_token_outputs_pass_every_check(pool):
    for keeps, buffers in (((0, 8, 6, 0), (1, 2)), ((0, 0, 0, 0), ()), ((8, 6, 4, 2), (0, 1, 2, 3))):
        p, keep_alive = _plan(keeps, buffers)
        _reaches_the_workspace_check(p, _ext(pool))
        _reaches_the_workspace_check(p, _ext(pool, mlp_act=nat.MLP_QUICK_GELU), nat.VitPrefix(5, FAKE))
        p.logits_ld = 128
        _reaches_the_workspace_check(p, _ext(pool))
        del keep_alive


# ---- what is refused, each with its code and its cause ----------------------------------------------------------------------

def test_half_a_headless_plan_is_a_null_weight_pointer():
    p, keep_alive = _plan(headless=True)
    p.num_classes = 16                              # no head_w, but classes
    rc, msg = _forward(p)
    assert rc == ERR_INVALID and "null weight pointer" in msg, msg
    p, keep_alive = _plan(headless=False)
    p.num_classes = 0                               # a head_w, but no classes
    rc, msg = _forward(p)
    assert rc == ERR_INVALID and "null weight pointer" in msg, msg
    del keep_alive


def test_headless_refusals():
    p, keep_alive = _plan()
    rc, msg = _forward(p, None, nat.VitPrefix(2, FAKE, head_rows=2))
    assert rc == ERR_UNSUPPORTED and "head_rows=2" in msg and "headless" in msg, msg
    p.act_fp8 = 1
    rc, msg = _forward(p)
    assert rc == ERR_UNSUPPORTED and "headless" in msg and "act_fp8" in msg, msg
    p.act_fp8 = 0
    for ld, code, what in ((64, ERR_INVALID, ">= C"), (132, ERR_INVALID, "multiple of 8"), (256, ERR_UNSUPPORTED, "0 or C")):
        p.logits_ld = ld
        rc, msg = _forward(p)
        assert rc == code and "logits row stride" in msg and what in msg, (ld, rc, msg)
    del keep_alive


@pytest.mark.parametrize("pool, name", [(nat.POOL_NONE, "RAJNI_POOL_NONE"), (nat.POOL_DENSE, "RAJNI_POOL_DENSE")])
def test_token_output_refusals(pool, name):
    headed, k1 = _plan(headless=False)
    rc, msg = _forward(headed, _ext(pool))
    assert rc == ERR_UNSUPPORTED and name in msg and "headless" in msg and "per-token classification" in msg, msg
    p, k2 = _plan()
    for fields in (dict(fc_norm_w=FAKE), dict(norm_absent=1)):
        rc, msg = _forward(p, _ext(pool, **fields))
        assert rc == ERR_UNSUPPORTED and name in msg and "no cast-only row kernel" in msg, msg
    p.cls_only_last_block = 1
    rc, msg = _forward(p, _ext(pool))
    assert rc == ERR_INVALID and name in msg and "cls_only_last_block" in msg, msg
    p.cls_only_last_block = 0
    p.act_fp8 = 1
    rc, msg = _forward(p, _ext(pool))
    assert rc == ERR_UNSUPPORTED and "act_fp8" in msg, msg
    p.act_fp8 = 0
    rc, msg = _forward(p, _ext(pool), nat.VitPrefix(2, FAKE, head_rows=2))
    assert rc == ERR_UNSUPPORTED and "head_rows=2" in msg, msg
    p.logits_ld = 256                                # the token outputs are dense
    rc, msg = _forward(p, _ext(pool))
    assert rc == ERR_UNSUPPORTED and "logits row stride" in msg, msg
    del k1, k2


def test_an_unknown_pool_keeps_its_refusal():
    for headless in (True, False):
        p, keep_alive = _plan(headless=headless)
        for bad in (4, -1):
            rc, msg = _forward(p, _ext(bad))
            assert rc == ERR_UNSUPPORTED, msg
            assert msg == f"rajni_vit_forward_ext: pool must be RAJNI_POOL_TOKEN or RAJNI_POOL_AVG ({bad})", msg
        del keep_alive


def test_last_block_cls_rows_eligibility():
    lib = nat.lib()
    p, keep_alive = _plan()
    elig = lambda e: lib.rajni_debug_last_block_cls_rows(C.byref(p), C.byref(e) if e is not None else None, None)
    assert elig(None) == 1 and elig(_ext()) == 1                 # a headless token plan: the head's row is still row 0
    assert elig(_ext(nat.POOL_NONE)) == 0 and elig(_ext(nat.POOL_DENSE)) == 0
    del keep_alive


# ---- wrapper ----------------------------------------------------------------------------------------------------------------

FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.7}, 2: {"keep_ratio": 0.5}}


def headless_model(name, **fix):
    m = ts.create_model(name, round_bf16=True, **(fix or FIX))
    m.head = nn.Identity()
    return m


@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64", "vit_micro_reg4_patch16_64",
                                  "vit_micro_qknorm_patch16_64", "vit_micro_swiglu_patch16_64", "vit_micro_quickgelu_patch16_64"])
def test_headless_models_are_supported(name):
    d = rajni_amd.RAJNIViTWrapper(headless_model(name), SCHED).check_supported()
    assert d["headless"] is True and d["num_classes"] == 0 and d["head_rows"] == 1
    # the entry point does not depend on the head: a plain token model still needs no ext record
    with_head = rajni_amd.RAJNIViTWrapper(ts.create_model(name, round_bf16=True, **FIX), SCHED).check_supported()
    assert with_head["headless"] is False and d["ext"] == with_head["ext"] and with_head["num_classes"] == 10
    assert d["ext"] == (name != "vit_micro_patch16_64" and name != "vit_micro_reg4_patch16_64")


def test_other_heads_stay_refused():
    m = ts.create_model("vit_micro_patch16_64")
    m.head = nn.Sequential()
    with pytest.raises(NotImplementedError, match="must be nn.Linear or nn.Identity"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = ts.create_model("vit_micro_distilled_patch16_64")
    m.head, m.head_dist = nn.Identity(), nn.Identity()
    with pytest.raises(NotImplementedError, match="distillation"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # a pooling the wrapper does not compute stays refused on a headless model too
    m = headless_model("vit_micro_patch16_64")
    m.global_pool = ""
    with pytest.raises(NotImplementedError, match="global_pool"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()


def test_fp8_mfma_on_a_headless_model_is_refused():
    w = rajni_amd.RAJNIViTWrapper(headless_model("vit_micro512_patch16_64"), {})
    with pytest.raises(NotImplementedError, match="headless"):
        w.set_weight_format("fp8_mfma")
    w.set_weight_format("fp8")
    assert w.check_supported()["headless"]
    # the head swapped behind the setter's back: the description refuses it
    w2 = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro512_patch16_64"), {}).set_weight_format("fp8_mfma")
    w2.m.head = nn.Identity()
    with pytest.raises(NotImplementedError, match="headless"):
        w2.check_supported()


def test_forward_features_refusals_need_no_device():
    """they come from the description and the options, in front of anything native (the device check itself comes first, so
    the helper is called directly)"""
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_fcnorm_patch16_64"), {})
    with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
        w._check_features(w.check_supported())
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro512_patch16_64"), {}).set_weight_format("fp8_mfma")
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w._check_features(w.check_supported())
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), {}).set_last_block_cls_only(True)
    with pytest.raises(ValueError, match="set_last_block_cls_only"):
        w._check_features(w.check_supported())
    with pytest.raises(nat.NativeError):            # and the public call still has no CPU fallback
        w.forward_features(torch.zeros(1, 3, 64, 64))


# ---- the restated graph -----------------------------------------------------------------------------------------------------

def images_of(cfg, B, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64", "deit3_micro_reg4_patch16_64",
                                  "vit_micro_all_patch16_64", "vit_micro_swiglu_patch16_64", "vit_micro_swiglu_split_patch16_64",
                                  "vit_micro_clip_quickgelu_patch16_64", "vit_micro_distilled_patch16_64"])
def test_unpruned_restatement_is_the_base_models_forward_features(name):
    cfg = ts.config_of(name)
    model = ts.create_model(name, round_bf16=True, **FIX).double()
    sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    imgs = images_of(cfg, 3)
    r = nf.features_restated(sd, imgs, {}, cfg)
    with torch.no_grad():
        want = model.forward_features(torch.from_numpy(imgs).double()).numpy()
    assert r["tokens"].shape == want.shape == (3, cfg.num_patches + cfg.num_prefix_tokens, cfg.embed_dim)
    assert np.abs(r["tokens"] - want).max() <= 1e-10 and np.abs(r["dense"] - want).max() <= 1e-10
    assert (r["source_idx"] == np.arange(want.shape[1])).all()
    if not cfg.distilled:
        model.head = nn.Identity()
        with torch.no_grad():
            pooled = model(torch.from_numpy(imgs).double()).numpy()
        assert pooled.shape == (3, cfg.embed_dim) and np.abs(r["pooled"] - pooled).max() <= 1e-10


@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_pruned_restatement_scatters_and_the_fixture_can_tell(name):
    """dense[b, source_idx[b]] == tokens[b], every other row zero; and the two ways to get the dense tensor wrong - the
    left-packed tokens read as if dense, and a scatter by the FIRST stage's map only - each move it by at least 5x the
    acceptance bar of the 16-bit device test (1e-2 of max|tokens|)"""
    cfg = ts.config_of(name)
    P = cfg.num_prefix_tokens
    sd = ts.state_dict_numpy(ts.create_model(name, round_bf16=True, **FIX))
    imgs = images_of(cfg, 3, seed=5)
    r = nf.features_restated(sd, imgs, SCHED, cfg)
    tokens, dense, src = r["tokens"], r["dense"], r["source_idx"]
    n0, Nf = cfg.num_patches + P, tokens.shape[1]
    assert r["counts"][-1] == Nf < n0 and dense.shape == (3, n0, cfg.embed_dim) and src.shape == (3, Nf)
    assert (src[:, :P] == np.arange(P)).all() and (np.diff(src, axis=1) > 0).all() and src.max() < n0
    assert len({tuple(s) for s in src}) > 1, "the maps must differ between the images"
    first, second = r["trace"][1]["keep_idx"], r["trace"][2]["keep_idx"]
    np.testing.assert_array_equal(src, np.take_along_axis(first, second, axis=1))
    for b in range(3):
        assert np.array_equal(dense[b, src[b]], tokens[b])
        rest = np.setdiff1d(np.arange(n0), src[b])
        assert len(rest) == n0 - Nf and not dense[b, rest].any()
    need = 5 * 1e-2 * float(np.abs(tokens).max())
    packed = np.zeros_like(dense)
    packed[:, :Nf] = tokens
    first_only = nf.scatter_dense(tokens, first[:, :Nf], n0)
    for what, wrong in (("left-packed tokens", packed), ("first stage's map only", first_only)):
        moved = float(np.abs(wrong - dense).max())
        print(f"[features] {name}: {what} moves the dense tensor by {moved:.4g}; 5 x bar = {need:.4g}")
        assert moved >= need, (what, moved, need)
    # the restatement in the model's 16-bit dtype runs and stays near (its distance is what the device bar is derived from)
    r16 = nf.features_restated(sd, imgs, SCHED, cfg, forced_keep={i: t["keep_idx"] for i, t in r["trace"].items()},
                               dtype=torch.bfloat16)
    assert np.array_equal(r16["source_idx"], src)
    assert np.abs(r16["tokens"] - tokens).max() <= 0.1 * np.abs(tokens).max()
