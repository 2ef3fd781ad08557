"""Models without a class token and the mean importance query (include/rajni_hip_query.h) without a GPU: the restated rule
against the fixture recorded from the reference, the ABI additions and their refusals, the timm-shaped no-class models, the
wrapper's classification of such models and what it still refuses, and the seeds of the GPU forward tests."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics as nm
import numerics_noclass as nq
import numerics_prefix as npx
import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import compute_importance
from rajni_amd.wrapper.importance import compute_importance_query
from rajni_amd.wrapper.model import model_num_prefix, plan_token_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = ["vit_micro_nocls_gap_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64", "vit_micro_reg1_nocls_gap_d80_patch16_64"]
QUERY_SYMBOLS = ("rajni_score_select_query_workspace_bytes", "rajni_score_select_query", "rajni_select_topk_query",
                 "rajni_patch_embed_query", "rajni_vit_workspace_bytes_query", "rajni_vit_forward_query")


# ---- the rule --------------------------------------------------------------------------------------------------------------

def test_the_restatement_reproduces_the_reference_where_the_two_rules_coincide():
    """identical query rows: the mean query is the reference's q[:, :, 0]; the bar is the one tests/test_oracle_golden.py
    holds the oracle's importance to"""
    cases = nq.load_fixture()
    assert [(c["B"], c["N"], c["H"], c["D"]) for c, _, _ in cases] == [(2, 64, 2, 16), (2, 256, 3, 64), (1, 64, 2, 80)]
    for c, qkv, ref in cases:
        q = qkv.reshape(c["B"], c["N"], 3, c["H"] * c["D"])[:, :, 0]
        assert (q == q[:, :1]).all() and (q * 64 == np.round(q * 64)).all() and np.abs(q).max() <= 4
        assert np.array_equal(q.mean(axis=1, dtype=np.float32), q[:, 0])           # exact in fp32 too
        got = nq.importance_scores(qkv, c["H"], query="mean")
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-8)
        np.testing.assert_array_equal(got, orc.importance_scores(qkv, c["H"]))     # and so the oracle's, to the bit


@pytest.mark.parametrize("kind", nm.IMP_KINDS + nq.QUERY_KINDS)
def test_the_cls_query_of_the_restatement_is_the_oracle(kind):
    make = nq.query_qkv if kind in nq.QUERY_KINDS else nm.importance_qkv
    qkv = make(kind, 2, 33, 2, 64, "bf16")
    for dt in (np.float64, np.float32):
        np.testing.assert_array_equal(nq.importance_scores(qkv, 2, dtype=dt, query="cls"), orc.importance_scores(qkv, 2, dtype=dt))
    mean = nq.importance_scores(qkv, 2, query="mean")
    assert mean.shape == (2, 33) and np.isfinite(mean).all() and not np.allclose(mean, orc.importance_scores(qkv, 2), rtol=1e-3)
    with pytest.raises(ValueError):
        nq.importance_scores(qkv, 2, query="max")


def test_the_budget_is_the_importance_budget_plus_the_derived_mean_term():
    qkv = nm.importance_qkv("voffset", 2, 33, 2, 64, "bf16")
    want, bud, e32 = nq.importance_budget(qkv, 2, "bf16", query="cls")
    w0, b0, e0 = nm.importance_budget(qkv, 2, "bf16")
    assert np.array_equal(want, w0) and np.array_equal(bud, b0) and e32 == e0
    for kind in nq.QUERY_KINDS:
        qkv = nq.query_qkv(kind, 2, 65, 2, 64, "fp32")
        want, bud, e32 = nq.importance_budget(qkv, 2, "fp32")
        base = (nm.UNIT["fp32"] + 4 * e32) * np.abs(want) + nm.FLOOR["fp32"]
        assert (bud >= base).all() and (bud > base).any()
        # a sequential fp32 sum (one legitimate order) stays inside, and so does the pairwise one
        t = qkv.reshape(2, 65, 3, 128).astype(np.float32).copy()
        acc = np.zeros((2, 128), np.float32)
        for n in range(65):
            acc = acc + t[:, n, 0]
        t[:, :, 0] = (acc * np.float32(1.0 / 65))[:, None]
        got = orc.importance_scores(t.reshape(2, 65, 384), 2, dtype=np.float32)
        assert nm.worst_ratio(got, want, bud)[0] <= 1.0


def test_keep_counts_without_prefix_tokens():
    assert ops.keep_count(0.75, 16, 0) == npx.keep_count(0.75, 16, 0) == 12
    assert ops.keep_count(0.01, 16, 0) == 1 and ops.keep_count(1.0, 16, 0) == 16
    assert plan_token_counts(16, 4, nq.SCHED, 0) == npx.token_counts(16, 4, nq.SCHED, 0) == [16, 16, 12, 7]
    assert plan_token_counts(20, 4, nq.SCHED, 4) == [20, 20, 16, 11]
    s = np.array([[3.0, 1, 2, 2, 5, 0]])
    np.testing.assert_array_equal(npx.select_tokens(s, 3, 0), [[0, 2, 4]])


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_the_query_header_is_additive_and_nothing_else_moves():
    assert nat.QUERY_SYMBOLS == QUERY_SYMBOLS
    header = open(os.path.join(ROOT, "include", "rajni_hip_query.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", code)) == set(QUERY_SYMBOLS)
    assert '#include "rajni_hip_image.h"' in header
    lib = nat.lib()
    for s in QUERY_SYMBOLS:
        assert getattr(lib, s) is not None
    assert C.sizeof(nat.VitQuery) == 8 and [f[0] for f in nat.VitQuery._fields_] == ["class_token", "query"]
    assert re.search(r"typedef struct \{\s*int class_token;[^}]*int query;[^}]*\} rajni_vit_query;", header)
    assert re.search(r"enum \{ RAJNI_QUERY_CLS = 0, RAJNI_QUERY_MEAN = 1 \};", header) and (nat.QUERY_CLS, nat.QUERY_MEAN) == (0, 1)
    assert "own extension" in header.lower() and "nobody has measured" in header.lower()
    # the old counts, sizes and versions
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert len(nat.EXPORTED_SYMBOLS) == 45 and len(nat.IMAGE_SYMBOLS) == 5
    assert not set(QUERY_SYMBOLS) & (set(nat.EXPORTED_SYMBOLS) | set(nat.LAYERS_SYMBOLS) | set(nat.IMAGE_SYMBOLS))
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.VitPrefix) == 16 and C.sizeof(nat.VitLayers) == 40 and C.sizeof(nat.VitImage) == 8
    for h in ("rajni_hip.h", "rajni_hip_debug.h", "rajni_hip_layers.h", "rajni_hip_image.h"):
        assert "rajni_vit_query" not in open(os.path.join(ROOT, "include", h)).read()


def test_the_scratch_grows_by_the_mean_query_row_only_where_tiles_run():
    lib = nat.lib()
    for dt in (nat.RAJNI_BF16, nat.RAJNI_F16, nat.RAJNI_F32):
        for (B, N, H, D) in ((3, 197, 12, 64), (2, 700, 2, 64), (2, 1374, 6, 64), (1, 5, 1, 8)):
            old = lib.rajni_score_select_workspace_bytes(B, N, H, D, dt)
            assert lib.rajni_score_select_query_workspace_bytes(B, N, H, D, dt, nat.QUERY_CLS) == old
            new = lib.rajni_score_select_query_workspace_bytes(B, N, H, D, dt, nat.QUERY_MEAN)
            assert new == (old + (B * H * D * 4 + 255) // 256 * 256 if old else 0), (B, N, H, D)
        assert lib.rajni_score_select_query_workspace_bytes(2, 700, 2, 64, dt, 2) == 0
    lib.rajni_debug_force_score_tiled(1)
    try:
        old = lib.rajni_score_select_workspace_bytes(3, 33, 2, 64, nat.RAJNI_BF16)
        assert old > 0 and lib.rajni_score_select_query_workspace_bytes(3, 33, 2, 64, nat.RAJNI_BF16, nat.QUERY_MEAN) == old + 3 * 128 * 4
    finally:
        lib.rajni_debug_force_score_tiled(0)


def _err(lib):
    return lib.rajni_last_error().decode()


def test_argument_checks_run_without_a_device():
    lib = nat.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    BF = nat.RAJNI_BF16
    # rajni_score_select_query(qkv, B, N, H, D, eps, num_prefix, keep, query, scores_out, keep_idx, next_scores, dtype, ws, bytes, stream)
    for args, word in (((None, 1, 8, 1, 8, 1e-6, 0, 1, 1, None, p, None, BF, None, 0), "qkv"),
                       ((p, 1, 8, 1, 8, 1e-6, 0, 1, 2, None, p, None, BF, None, 0), "query"),
                       ((p, 1, 8, 1, 8, 1e-6, -1, 1, 1, None, p, None, BF, None, 0), "num_prefix"),
                       ((p, 1, 8, 1, 8, 1e-6, 33, 1, 1, None, p, None, BF, None, 0), "num_prefix"),
                       ((p, 1, 1, 1, 8, 1e-6, 0, 1, 1, None, p, None, BF, None, 0), "N >= 2"),
                       ((p, 1, 8, 1, 8, 1e-6, 0, 9, 1, None, p, None, BF, None, 0), "keep"),
                       ((p, 1, 8, 1, 8, 1e-6, 0, 1, 1, None, None, None, BF, None, 0), "keep_idx"),
                       ((p, 1, 8, 1, 8, 1e-6, 0, 0, 1, None, None, None, BF, None, 0), "scores_out"),
                       ((p, 1, 8, 1, 8, 1e-6, 0, 1, 1, None, p, None, 7, None, 0), "dtype"),
                       ((p + 2, 1, 8, 1, 8, 1e-6, 0, 1, 1, None, p, None, BF, None, 0), "qkv must be 16-byte aligned")):
        assert lib.rajni_score_select_query(*args, None) == 1, args
        assert "rajni_score_select_query" in _err(lib) and word in _err(lib), (_err(lib), word)
    # (the class query with a prefix token is rajni_score_select_ws, refusals included)
    assert lib.rajni_score_select_query(None, 1, 8, 1, 8, 1e-6, 1, 1, 0, None, p, None, BF, None, 0, None) == 1
    assert "rajni_score_select_ws" in _err(lib)
    # rajni_select_topk_query(scores, B, N, num_prefix, keep, keep_idx, next_scores, dtype, stream)
    for args in ((None, 1, 8, 0, 1, p, None, BF), (p, 1, 8, -1, 1, p, None, BF), (p, 1, 1, 0, 1, p, None, BF), (p, 1, 8, 0, 9, p, None, BF)):
        assert lib.rajni_select_topk_query(*args, None) == 1 and "rajni_select_topk_query" in _err(lib), args
    # rajni_patch_embed_query(images, w, bias, reg, num_reg, pos, pos_has_cls, x, x_f32, B, Cin, H, W, P, C, dtype, ws, bytes, stream)
    ok = [p, p, p, p, 4, p, 1, p, 0, 1, 3, 64, 64, 16, 128, BF, None, 0]
    for pos, val, word in ((0, None, "null"), (3, None, "reg"), (4, 0, "reg"), (4, 33, "num_reg"), (5, None, "null"), (15, 7, "dtype"),
                           (3, p + 2, "reg must be")):
        args = list(ok)
        args[pos] = val
        assert lib.rajni_patch_embed_query(*args, None) == 1, (pos, val)
        assert "rajni_patch_embed_query" in _err(lib) and word in _err(lib), (_err(lib), word)


def _plan():
    plan = nat.VitPlan()
    plan.dtype, plan.B, plan.in_chans, plan.img_size, plan.patch_size = nat.RAJNI_BF16, 3, 3, 64, 16
    plan.C, plan.H, plan.D, plan.depth, plan.hidden, plan.num_classes = 128, 2, 64, 4, 512, 10
    return plan


def test_the_forward_names_the_field_it_refuses():
    lib = nat.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    plan, ext = _plan(), nat.VitExt()
    ext.pool = nat.POOL_AVG
    fwd = lambda e, pre, q: lib.rajni_vit_forward_query(C.byref(plan), C.byref(e) if e is not None else None,
                                                        C.byref(pre) if pre is not None else None, None, None, C.byref(q), p, p, None)
    for q, e, word in ((nat.VitQuery(2, 1), ext, "query.class_token"), (nat.VitQuery(1, 2), ext, "query.query"),
                       (nat.VitQuery(0, 0), ext, "query.query must be RAJNI_QUERY_MEAN"), (nat.VitQuery(0, 1), None, "ext.pool"),
                       (nat.VitQuery(0, 1), nat.VitExt(), "ext.pool")):
        assert fwd(e, None, q) == 1 and word in _err(lib), (_err(lib), word)
        assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, C.byref(q)) == 0 or word == "ext.pool"
    plan.cls_only_last_block = 1
    assert fwd(ext, None, nat.VitQuery(0, 1)) == 1 and "plan.cls_only_last_block" in _err(lib)
    plan.cls_only_last_block, plan.act_fp8 = 0, 1
    assert fwd(ext, None, nat.VitQuery(0, 1)) == 2 and "plan.act_fp8" in _err(lib)
    plan.act_fp8 = 0
    # the prefix record counts the registers alone
    for num, reg, rows, word in ((2, p, 2, "head_rows"), (3, None, 0, "reg_token"), (0, p, 0, "reg_token"), (33, p, 0, "num_prefix")):
        pre = nat.VitPrefix(num, reg, rows)
        assert fwd(ext, pre, nat.VitQuery(0, 1)) == 1 and word in _err(lib), (_err(lib), word)
        assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), C.byref(pre), None, C.byref(nat.VitQuery(0, 1))) == 0
    # what passes the records reaches the plan's own checks (this plan has no blocks)
    assert fwd(ext, nat.VitPrefix(1, p), nat.VitQuery(0, 1)) == 1 and _err(lib) == "rajni_vit_forward: bad plan"


def test_the_workspace_query_takes_the_query_record():
    lib = nat.lib()
    plan = _plan()
    base = lib.rajni_vit_workspace_bytes(C.byref(plan))
    buf = (C.c_char * 64)()
    for q in (None, nat.VitQuery(1, 0)):
        assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, C.byref(q) if q else None) == base
    assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, C.byref(nat.VitQuery(1, 1))) == base      # one workgroup scores 17 tokens
    sizes = [lib.rajni_vit_workspace_bytes_query(C.byref(plan), C.byref(nat.VitPrefix(R, C.addressof(buf) if R else None)), None,
                                                 C.byref(nat.VitQuery(0, 1))) for R in (0, 1, 4)]
    assert 0 < sizes[0] < base == sizes[1] < sizes[2]
    # a grid the tiles score: the mean query's B * C * 4 bytes more than the class query's plan
    plan.img_size = 400
    img = nat.VitImage(400, 400)
    cls = lib.rajni_vit_workspace_bytes_image(C.byref(plan), None, C.byref(img))
    assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, C.byref(img), C.byref(nat.VitQuery(1, 1))) == cls + 3 * 128 * 4


# ---- timm_shaped -------------------------------------------------------------------------------------------------------------

def test_vitconfig_rules_and_field_order():
    fields = [f.name for f in dataclasses.fields(ts.ViTConfig)]
    assert fields[-5:] == ["class_token", "mlp", "distilled", "act", "reg_tokens"] and ts.ViTConfig().class_token is True
    assert fields[:15] == ["img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_ratio", "num_classes",
                           "layer_scale", "no_embed_class", "ln_eps", "qk_norm", "pre_norm", "global_pool", "fc_norm"] and len(fields) == 20
    # every config that existed: rebuilt from its values in field order with class_token left out, it is itself
    for name, cfg in {**ts.CONFIGS, **ts.SWIGLU_CONFIGS}.items():
        vals = [getattr(cfg, f) for f in fields]
        assert cfg.class_token is True and ts.ViTConfig(*vals[:15], True, *vals[16:]) == cfg, name
        assert cfg.num_prefix_tokens == 1 + cfg.reg_tokens + int(cfg.distilled)
    with pytest.raises(ValueError, match="global_pool"):
        ts.ViTConfig(class_token=False)
    with pytest.raises(ValueError, match="global_pool"):
        ts.ViTConfig(class_token=False, global_pool="token", reg_tokens=4)
    with pytest.raises(ValueError, match="distilled"):
        ts.ViTConfig(class_token=False, global_pool="avg", distilled=True)
    assert set(MICRO) < set(ts.NOCLASS_CONFIGS) and not set(ts.NOCLASS_CONFIGS) & (set(ts.CONFIGS) | set(ts.SWIGLU_CONFIGS))
    for name, R, D, rows in zip(MICRO, (0, 4, 1), (64, 64, 80), (16, 16, 17)):
        cfg = ts.config_of(name)
        assert (cfg.class_token, cfg.reg_tokens, cfg.num_prefix_tokens, cfg.head_dim, cfg.global_pool) == (False, R, R, D, "avg")
        m = ts.create_model(name)
        assert m.cls_token is None and "cls_token" not in m.state_dict() and m.pos_embed.shape[1] == rows and m.num_prefix_tokens == R
    assert ts.config_of("vit_micro_reg4_nocls_gap_patch16_64").layer_scale and not ts.config_of("vit_micro_reg4_nocls_gap_patch16_64").use_fc_norm
    for name in ("vit_medium_patch16_gap_256", "vit_betwixt_patch16_reg4_gap_256"):      # (dims from memory: only their form is held)
        cfg = ts.config_of(name)
        assert not cfg.class_token and cfg.global_pool == "avg" and cfg.img_size == 256 and cfg.embed_dim % cfg.num_heads == 0


def test_synthetic_weights_of_existing_configs_are_what_they_were():
    """the class-token twin of a no-class config draws the same stream, with cls_token in front; a no-class config draws
    nothing in its place"""
    cfg = ts.config_of("vit_micro_reg4_nocls_gap_patch16_64")
    twin = dataclasses.replace(cfg, class_token=True)
    a, b = ts.synth_state_dict(cfg, seed=3, std=0.05, bias_std=0.1), ts.synth_state_dict(twin, seed=3, std=0.05, bias_std=0.1)
    assert set(b) - set(a) == {"cls_token"} and list(b)[0] == "cls_token"
    rng = np.random.default_rng(3)
    first = (rng.standard_normal((1, 1, 128), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    np.testing.assert_array_equal(b["cls_token"], first)
    np.testing.assert_array_equal(ts.synth_state_dict(ts.CONFIGS["vit_micro_patch16_64"], seed=3, std=0.05)["cls_token"], first)


@pytest.mark.parametrize("name", MICRO)
def test_the_stock_forward_is_the_restatement_with_an_empty_schedule(name):
    cfg = ts.config_of(name)
    model = ts.create_model(cfg, seed=5, round_bf16=True, **nq.FIX_BASE)
    sd = ts.state_dict_numpy(model)
    imgs = nq.images_of(cfg, 2, 3)
    with torch.no_grad():
        stock = model(torch.from_numpy(imgs)).numpy()
        feats = model.forward_features(torch.from_numpy(imgs)).numpy()
    want, counts, tr = nq.vit_forward_restated(sd, imgs, {}, cfg)
    assert counts == [cfg.num_patches + cfg.reg_tokens] * cfg.depth and tr == {} and feats.shape[1] == counts[0]
    assert np.abs(stock - want).max() <= 1e-4 * np.abs(want).max()
    tok, _, _ = nq.vit_forward_restated(sd, imgs, {}, cfg, features="tokens")
    assert np.abs(feats - tok).max() <= 1e-4 * np.abs(tok).max()
    # and with a schedule the registers stay and the counts are the rule's
    _, counts, tr = nq.vit_forward_restated(sd, imgs, nq.SCHED, cfg)
    P = cfg.reg_tokens
    assert counts == npx.token_counts(16 + P, 4, nq.SCHED, P)
    for t in tr.values():
        assert (t["keep_idx"][:, :P] == np.arange(P)).all() and (np.diff(t["keep_idx"], axis=1) > 0).all()


# ---- the wrapper -------------------------------------------------------------------------------------------------------------

def _refused(model, match):
    w = rajni_amd.RAJNIViTWrapper(model, nq.SCHED)
    with pytest.raises(NotImplementedError, match=match):
        w.check_supported()


@pytest.mark.parametrize("name", MICRO)
def test_consistent_models_without_a_class_token_are_accepted(name):
    cfg = ts.config_of(name)
    m = ts.create_model(name)
    assert model_num_prefix(m) == cfg.reg_tokens
    w = rajni_amd.RAJNIViTWrapper(m, nq.SCHED)
    d = w.check_supported()
    assert d["num_prefix"] == cfg.reg_tokens and d["class_token"] is False and d["pool"] == "avg" and d["head_rows"] == 1
    assert w.importance_query == "mean"
    for i in nq.SCHED:
        assert w.blocks[i].attn.num_prefix_tokens == cfg.reg_tokens and w.blocks[i].attn.importance_query == "mean"
    # headless is fine too, any pool attribute
    m = ts.create_model(name)
    m.head, m.global_pool = nn.Identity(), "avg"
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["headless"]


def test_half_formed_models_stay_refused_with_the_class_token_named():
    C_ = 128
    m = ts.create_model("vit_micro_reg4_patch16_64")                      # declares 5 prefix tokens, 21 pos rows
    m.cls_token = None
    _refused(m, "cls_token.*declares 5 prefix tokens")
    m = ts.create_model("vit_micro_reg4_nocls_gap_patch16_64")
    m.num_prefix_tokens = 5
    _refused(m, "cls_token.*declares 5 prefix tokens")
    for rows in (15, 17, 21):                                              # 16 patches, R = 4: 16 or 20 rows
        m = ts.create_model("vit_micro_reg4_nocls_gap_patch16_64")
        m.pos_embed = nn.Parameter(torch.zeros(1, rows, C_))
        _refused(m, "cls_token.*pos_embed")
    m = ts.create_model("vit_micro_reg4_nocls_gap_patch16_64")
    m.pos_embed = nn.Parameter(torch.zeros(1, 20, C_))                     # (a row for every register is fine)
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["num_prefix"] == 4
    m = ts.create_model("vit_micro_nocls_gap_patch16_64")
    m.global_pool = "token"
    _refused(m, "cls_token.*global_pool")
    m = ts.create_model("vit_micro_nocls_gap_patch16_64")
    m.dist_token = nn.Parameter(torch.zeros(1, 1, C_))
    _refused(m, "cls_token.*distillation")
    m = ts.create_model("vit_micro_nocls_gap_patch16_64")
    m.head_dist = nn.Linear(C_, 10)
    _refused(m, "cls_token.*distillation")
    for shape in ((4, C_), (1, 4, C_ + 8), (2, 4, C_), (1, 0, C_)):
        m = ts.create_model("vit_micro_reg4_nocls_gap_patch16_64")
        m.reg_token = nn.Parameter(torch.zeros(*shape))
        _refused(m, "cls_token.*reg_token must be")
    m = ts.create_model("vit_micro_nocls_gap_patch16_64")
    m.reg_token, m.num_prefix_tokens = nn.Parameter(torch.zeros(1, 33, C_)), 33
    _refused(m, "cls_token.*33 prefix tokens")


def test_the_importance_query_setter():
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_nocls_gap_patch16_64"), nq.SCHED)
    with pytest.raises(ValueError, match="no class token"):
        w.set_importance_query("cls")
    with pytest.raises(ValueError, match="query must be"):
        w.set_importance_query("max")
    assert w.set_importance_query("mean") is w and w.importance_query == "mean"
    with pytest.raises(ValueError, match="no class token"):
        w.set_last_block_cls_only(True)
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.set_weight_format("fp8_mfma").check_supported()
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_gap_patch16_64"), nq.SCHED)
    assert w.importance_query == "cls" and w.blocks[1].attn.importance_query == "cls"
    assert w.set_importance_query("mean").importance_query == "mean" and w.blocks[1].attn.importance_query == "mean"
    assert w.set_importance_query("cls").importance_query == "cls" and w.blocks[2].attn.importance_query == "cls"
    with pytest.raises(ValueError, match="query must be"):
        ops.query_code("row0")
    import inspect
    for fn in (ops.score_select, ops.importance, compute_importance_query):
        assert inspect.signature(fn).parameters["query"].default == "cls"
    assert list(inspect.signature(compute_importance).parameters) == ["qkv", "num_heads", "eps"]      # the reference's, as it was
    from rajni_amd import run
    assert run.get_args(["--importance_query", "mean"]).importance_query == "mean" and run.get_args([]).importance_query is None


# ---- the seeds of tests/test_gpu_noclass_forward.py ----------------------------------------------------------------------------

def _fixture(name, seed):
    cfg = ts.config_of(name)
    return cfg, ts.state_dict_numpy(ts.create_model(cfg, seed=seed, round_bf16=True, **nq.FIX_BASE))


def search_seeds(name, query="mean", seeds=range(1, 81)):
    """(weight seed, image seed = weight seed + 4) with the LARGEST smallest boundary gap, in units of the bf16 score budget,
    among the given weight seeds at B = 3 - how numerics_noclass.SEEDS was filled (the test below holds each entry to
    GAP_FACTOR); not run by the suite"""
    best = (0.0, None)
    for seed in seeds:
        cfg, sd = _fixture(name, seed)
        best = max(best, (nq.boundary_gap_ratios(sd, nq.images_of(cfg, 3, seed + 4), nq.SCHED, cfg, "bf16", query), seed))
    return best[1], best[1] + 4


@pytest.mark.parametrize("name", sorted(nq.SEEDS))
def test_no_committed_seed_hinges_on_a_near_tie(name):
    wseed, iseed = nq.SEEDS[name]
    cfg, sd = _fixture(name, wseed)
    query = "mean"
    for B in (3, 1):
        r = nq.boundary_gap_ratios(sd, nq.images_of(cfg, B, iseed), nq.SCHED, cfg, "bf16", query)
        print(f"[noclass] {name} B={B}: smallest boundary gap / bf16 score budget = {r:.3g}")
        assert r >= nq.GAP_FACTOR
