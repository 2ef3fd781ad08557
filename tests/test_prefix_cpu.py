"""Register tokens (prefix tokens beyond CLS; timm `reg_tokens=R`) without a GPU: the ABI additions and their argument checks,
the timm-shaped register model against a hand restatement, the wrapper's host logic and what it still refuses, and the
restated selection rule of tests/numerics_prefix.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_prefix as npx
import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import RAJNIAttention
from rajni_amd.wrapper.model import plan_token_counts

REG_CONFIGS = ["vit_micro_reg4_patch16_64", "deit3_micro_reg4_patch16_64", "vit_micro_reg1_gap_patch14_56",
               "vit_micro512_reg4_patch16_64", "vit_small_patch14_reg4_dinov2"]
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
NEW_SYMBOLS = ("rajni_select_topk_prefix", "rajni_score_select_prefix", "rajni_patch_embed_prefix", "rajni_pool_norm_prefix",
               "rajni_vit_workspace_bytes_prefix", "rajni_vit_forward_ext_prefix")


def _images(cfg, B=2, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_the_pins_hold():
    lib = nat.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in nat.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert lib.rajni_profile_class_name(16) and not lib.rajni_profile_class_name(17)
    # the records beside the plan: the ext record as it was, the prefix record as the header declares it (LP64: int, pointer)
    assert C.sizeof(nat.VitExt) == 72
    assert C.sizeof(nat.VitPrefix) == 16 and nat.VitPrefix.num_prefix.offset == 0 and nat.VitPrefix.reg_token.offset == 8
    assert nat.MAX_PREFIX == 32


def test_exported_symbols_are_the_headers_prototypes():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for h in ("rajni_hip.h", "rajni_hip_debug.h"):
        with open(os.path.join(root, "include", h)) as f:
            names |= set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)))
    assert names == set(nat.EXPORTED_SYMBOLS)


def _err(lib):
    return lib.rajni_last_error().decode()


def test_argument_checks_run_without_a_device():
    lib = nat.load_library()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)                                 # a non-null pointer no check dereferences
    BF = nat.RAJNI_BF16
    # rajni_select_topk_prefix(scores, B, N, num_prefix, keep, keep_idx, next_scores, dtype, stream)
    for args in ((None, 1, 8, 2, 1, p, None, BF), (p, 1, 8, 2, 1, None, None, BF), (p, 1, 8, 0, 1, p, None, BF),
                 (p, 1, 8, 33, 1, p, None, BF), (p, 1, 2, 2, 1, p, None, BF), (p, 1, 8, 2, 0, p, None, BF),
                 (p, 1, 8, 2, 7, p, None, BF), (p, 0, 8, 2, 1, p, None, BF), (p, 1, 8, 2, 1, p, None, 9)):
        assert lib.rajni_select_topk_prefix(*args, None) == 1, args
        assert "rajni_select_topk_prefix" in _err(lib)
    # rajni_score_select_prefix(qkv, B, N, H, D, eps, num_prefix, keep, scores_out, keep_idx, next_scores, dtype, stream)
    for args in ((None, 1, 8, 1, 8, 1e-6, 2, 1, None, p, None, BF), (p, 1, 8, 1, 8, 1e-6, 2, 1, None, None, None, BF),
                 (p, 1, 8, 1, 8, 1e-6, 0, 1, None, p, None, BF), (p, 1, 8, 1, 8, 1e-6, 33, 1, None, p, None, BF),
                 (p, 1, 5, 1, 8, 1e-6, 5, 1, None, p, None, BF), (p, 1, 8, 1, 8, 1e-6, 2, 7, None, p, None, BF),
                 (p, 1, 8, 1, 8, 1e-6, 2, 0, None, p, None, BF), (p, 1, 8, 1, 8, 1e-6, 2, 1, None, p, None, 5)):
        assert lib.rajni_score_select_prefix(*args, None) == 1, args
        assert "rajni_score_select_prefix" in _err(lib)
    # rajni_patch_embed_prefix(images, w, bias, cls, reg, num_prefix, pos, pos_has_cls, x, x_f32, B, Cin, S, P, C, dtype, ws, bytes, stream)
    ok = [p, p, p, p, p, 5, p, 1, p, 0, 1, 3, 64, 16, 128, BF, None, 0]
    for pos, val in ((0, None), (3, None), (4, None), (5, 0), (5, 33), (6, None), (8, None), (15, 7), (3, p + 2)):
        args = list(ok)
        args[pos] = val
        assert lib.rajni_patch_embed_prefix(*args, None) == 1, (pos, val)
        assert "rajni_patch_embed_prefix" in _err(lib)
    # rajni_pool_norm_prefix(x, B, N, num_prefix, C, pool, nw, nb, neps, fw, fb, feps, out, dtype, x_f32, stream)
    for args in ((None, 1, 8, 2, 64, 1, None, None, 0.0, None, None, 0.0, p, BF, 0), (p, 1, 8, 2, 64, 1, None, None, 0.0, None, None, 0.0, None, BF, 0),
                 (p, 1, 8, 0, 64, 1, None, None, 0.0, None, None, 0.0, p, BF, 0), (p, 1, 8, 33, 64, 1, None, None, 0.0, None, None, 0.0, p, BF, 0),
                 (p, 1, 2, 2, 64, 1, None, None, 0.0, None, None, 0.0, p, BF, 0), (p, 1, 8, 2, 64, 1, None, None, 0.0, None, None, 0.0, p, 7, 0)):
        assert lib.rajni_pool_norm_prefix(*args, None) == 1, args
        assert "rajni_pool_norm_prefix" in _err(lib)
    # the whole forward and the workspace query
    plan, ext = nat.VitPlan(), nat.VitExt()
    for num, reg in ((40, p), (-1, None), (3, None), (1, p), (0, p)):
        pre = nat.VitPrefix()
        pre.num_prefix, pre.reg_token = num, reg
        assert lib.rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext), C.byref(pre), p, p, None) == 1, (num, reg)
        assert "rajni_vit_forward_ext_prefix" in _err(lib)
        plan.patch_size, plan.img_size = 16, 64
        assert lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), C.byref(pre)) == 0
        plan.patch_size = plan.img_size = 0
    pre = nat.VitPrefix()
    pre.num_prefix, pre.reg_token = 5, p
    assert lib.rajni_vit_forward_ext_prefix(None, None, C.byref(pre), p, p, None) == 1
    assert lib.rajni_vit_forward_ext_prefix(C.byref(plan), None, None, None, None, None) == 1


def test_workspace_query_takes_the_prefix_record():
    lib = nat.load_library()
    plan = nat.VitPlan()
    plan.dtype, plan.B, plan.in_chans, plan.img_size, plan.patch_size = nat.RAJNI_BF16, 3, 3, 64, 16
    plan.C, plan.H, plan.D, plan.depth, plan.hidden, plan.num_classes = 128, 2, 64, 4, 512, 10
    base = lib.rajni_vit_workspace_bytes(C.byref(plan))
    assert base > 0 and lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), None) == base
    buf = (C.c_char * 64)()
    sizes = []
    for P in (0, 1, 2, 5):
        pre = nat.VitPrefix()
        pre.num_prefix, pre.reg_token = P, (C.addressof(buf) if P > 1 else None)
        sizes.append(lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), C.byref(pre)))
    assert sizes[0] == sizes[1] == base and base < sizes[2] < sizes[3]
    # every buffer is rows x width with rows = B * (n + P): 4 more rows per image can only add, and by less than (n+5)/(n+1)
    assert sizes[3] <= base * 21 // 17 + 16 * 256


# ---------------------------------------------------------------------------------------------------------------
# timm_shaped
# ---------------------------------------------------------------------------------------------------------------

# sha256 (16 hex digits) over names and bytes of synth_state_dict in draw order, computed on the parent commit (before
# reg_tokens existed):  name: (seed 0 defaults, seed 3 std 0.08 bias_std 0.02)
PARENT = {"vit_micro_patch16_64": ("0589783db7044cd4", "0b25e3a4f0eed014"),
          "deit3_micro_patch16_64": ("c073c6a6b084ab96", "c2a3ade870131ac1"),
          "vit_micro_all_patch16_64": ("750dcf7fd98607a4", "72a7b0e3144ff4ff")}


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("name", sorted(PARENT))
def test_existing_configs_keep_their_weight_stream(name):
    cfg = ts.CONFIGS[name]
    assert cfg.reg_tokens == 0 and cfg.num_prefix_tokens == 1
    assert sd_hash(ts.synth_state_dict(cfg, seed=0)) == PARENT[name][0]
    assert sd_hash(ts.synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02)) == PARENT[name][1]
    m = ts.create_model(cfg)
    assert m.reg_token is None and m.num_prefix_tokens == 1 and "reg_token" not in m.state_dict()


def test_register_configs_are_shaped_like_timm_and_draw_reg_token_last():
    assert list(ts.ViTConfig.__dataclass_fields__)[-1] == "reg_tokens"
    for name in REG_CONFIGS:
        cfg = ts.CONFIGS[name]
        R = cfg.reg_tokens
        assert R >= 1
        sd = ts.synth_state_dict(cfg, seed=4, std=0.05, bias_std=0.02)
        assert list(sd)[-1] == "reg_token" and sd["reg_token"].shape == (1, R, cfg.embed_dim)
        assert sd["pos_embed"].shape[1] == cfg.num_patches + (0 if cfg.no_embed_class else 1 + R)
        if name != "vit_small_patch14_reg4_dinov2":
            m = ts.create_model(cfg)
            assert m.num_prefix_tokens == 1 + R and tuple(m.reg_token.shape) == (1, R, cfg.embed_dim)
    d = ts.CONFIGS["vit_small_patch14_reg4_dinov2"]
    assert (d.embed_dim, d.depth, d.num_heads, d.patch_size, d.reg_tokens, d.no_embed_class) == (384, 12, 6, 14, 4, True)
    assert d.layer_scale and d.num_patches + 5 == 261
    # no_embed_class: the register config's every other tensor is the register-free config's, bit for bit
    plain = ts.synth_state_dict(ts.CONFIGS["deit3_micro_patch16_64"], seed=4, std=0.05, bias_std=0.02)
    reg = ts.synth_state_dict(ts.CONFIGS["deit3_micro_reg4_patch16_64"], seed=4, std=0.05, bias_std=0.02)
    assert list(reg)[:-1] == list(plain) and all(np.array_equal(reg[k], plain[k]) for k in plain)


@pytest.mark.parametrize("name", REG_CONFIGS[:4])
def test_stock_forward_equals_the_hand_restatement(name):
    """_pos_embed + blocks + pool of the timm-shaped model, in fp64, against tests/numerics_prefix.py to 1e-6: both pos-embed
    layouts (with prefix rows, no_embed_class) and both pools ('token', 'avg' over rows P..)"""
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **FIX)
    sd = ts.state_dict_numpy(model)
    imgs = _images(cfg, 3)
    with torch.no_grad():
        stock = model.double()(torch.from_numpy(imgs).double()).numpy()
    want, counts, _ = npx.vit_forward_restated(sd, imgs, {}, cfg)
    assert counts == [cfg.num_patches + 1 + cfg.reg_tokens] * cfg.depth
    assert np.abs(stock - want).max() <= 1e-6 * np.abs(want).max()
    # and _pos_embed row by row
    with torch.no_grad():
        x = model._pos_embed(model.patch_embed(torch.from_numpy(imgs).double())).numpy()
    P, n = 1 + cfg.reg_tokens, cfg.num_patches
    pos = sd["pos_embed"][0].astype(np.float64)
    pre = np.concatenate([sd["cls_token"][0], sd["reg_token"][0]]).astype(np.float64)
    assert x.shape == (3, P + n, cfg.embed_dim)
    np.testing.assert_allclose(x[0, :P], pre if cfg.no_embed_class else pre + pos[:P], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(x[0, :P], x[2, :P])


@pytest.mark.parametrize("name", ["deit3_micro_reg4_patch16_64", "vit_micro_reg4_patch16_64", "vit_micro_reg1_gap_patch14_56"])
def test_fixtures_can_tell_whether_the_registers_are_there(name):
    """ignoring the registers (the same patch selections, register rows removed) moves the fp32 logits by >= 5x the 1e-2 bar"""
    cfg = ts.CONFIGS[name]
    # (one register in front of an 'avg' pool is a weak signal at the project's seed: tests/test_gpu_prefix_forward.py::FIX_OF)
    fix = dict(seed=12, std=0.08, bias_std=0.1) if name == "vit_micro_reg1_gap_patch14_56" else FIX
    sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, **fix))
    for sched in ({}, SCHED):
        for B in (3, 1):
            moved, need = npx.registers_matter(sd, _images(cfg, B), sched, cfg, 1e-2)
            assert moved >= need


# ---------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------

def test_keep_count_with_prefix_tokens_is_pythons():
    for P in (1, 2, 5, 32):
        for N in list(range(P + 1, P + 40)) + [197 + P - 1, 257 + P - 1, 577 + P - 1]:
            for r in (0.0, 0.01, 0.1, 0.29, 0.3, 0.5, 0.58, 0.6, 0.7, 0.72, 0.75, 0.8, 0.88, 0.9, 0.99, 1.0):
                want = max(1, int(r * (N - P)))
                assert ops.keep_count(r, N, P) == want == npx.keep_count(r, N, P)
                if P == 1:
                    assert ops.keep_count(r, N) == orc.keep_count(r, N) == want
    assert plan_token_counts(21, 4, orc.normalise_schedule(SCHED), 5) == npx.token_counts(21, 4, SCHED, 5) == [21, 21, 17, 12]
    assert plan_token_counts(17, 4, orc.normalise_schedule(SCHED)) == orc.token_counts(17, 4, orc.normalise_schedule(SCHED))


def test_restated_selection_rule():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((4, 23))
    np.testing.assert_array_equal(npx.select_tokens(s, 9, 1), orc.select_tokens(s, 9))
    # registers never take a rank slot, whatever they hold; ties: lower index first; NaN = +inf; -0 = +0
    row = np.array([[0.1, np.inf, np.nan, 0.5, 0.5, -0.0, 0.0, np.nan, 0.5, -1.0]])
    np.testing.assert_array_equal(npx.select_tokens(row, 3, 3), [[0, 1, 2, 3, 4, 7]])
    np.testing.assert_array_equal(npx.select_tokens(row, 5, 3), [[0, 1, 2, 3, 4, 5, 7, 8]])
    np.testing.assert_array_equal(npx.select_tokens(row, 1, 5), [[0, 1, 2, 3, 4, 7]])
    np.testing.assert_array_equal(npx.select_tokens(row, 7, 3), [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9]])


# ---------------------------------------------------------------------------------------------------------------
# wrapper host logic
# ---------------------------------------------------------------------------------------------------------------

def test_wrapper_accepts_a_register_model():
    """fails without the feature: the parent raises NotImplementedError('... prefix tokens (register / distillation ...')"""
    m = ts.create_model("vit_micro_reg4_patch16_64")
    d = rajni_amd.RAJNIViTWrapper(m, SCHED).check_supported()
    assert d["num_prefix"] == 5


@pytest.mark.parametrize("name", REG_CONFIGS)
def test_wrapper_accepts_the_register_configs(name):
    cfg = ts.CONFIGS[name]
    if name == "vit_small_patch14_reg4_dinov2":
        cfg = ts.ViTConfig(**{**cfg.to_dict(), "depth": 2})             # (the full depth only costs time here)
    m = ts.create_model(cfg)
    before = {k for k, _ in m.named_parameters()}
    w = rajni_amd.RAJNIViTWrapper(m, SCHED if cfg.depth > 2 else {1: {"keep_ratio": 0.5}})
    d = w.check_supported()
    assert d["num_prefix"] == 1 + cfg.reg_tokens and d["pool"] == cfg.global_pool
    assert d["ext"] == (cfg.global_pool == "avg")
    assert {k for k, _ in m.named_parameters()} == before
    att = m.blocks[1].attn
    assert isinstance(att, RAJNIAttention) and att.num_prefix_tokens == 1 + cfg.reg_tokens
    assert rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), SCHED).check_supported()["num_prefix"] == 1
    assert ts.create_model("vit_micro_patch16_64").blocks[1].attn is not None
    a = RAJNIAttention(ts.create_model("vit_micro_patch16_64").blocks[0].attn, 0.5, True)
    assert a.num_prefix_tokens == 1


def _refused(model, match):
    with pytest.raises(NotImplementedError, match=match):
        rajni_amd.RAJNIViTWrapper(model, {}).check_supported()


def test_what_is_still_refused():
    C_ = 128
    m = ts.create_model("vit_micro_reg4_patch16_64")
    m.cls_token = None                                                     # class_token=False
    _refused(m, "cls_token")
    m = ts.create_model("vit_micro_reg4_patch16_64")
    m.dist_token = nn.Parameter(torch.zeros(1, 1, C_))                     # DeiT distilled
    _refused(m, "[Dd]istillation")
    m = ts.create_model("vit_micro_patch16_64")
    m.head_dist = nn.Linear(C_, 10)
    _refused(m, "[Dd]istillation")
    m = ts.create_model("vit_micro_patch16_64")                            # P = 33
    m.reg_token, m.num_prefix_tokens = nn.Parameter(torch.zeros(1, 32, C_)), 33
    _refused(m, "33 prefix tokens")
    m.reg_token, m.num_prefix_tokens = nn.Parameter(torch.zeros(1, 31, C_)), 32     # P = 32 passes the count check ...
    _refused(m, "pos_embed")                                                          # ... and stops at its 17-row pos-embed
    for shape in ((4, C_), (1, 4, C_ + 8), (2, 4, C_), (1, 0, C_), (1, 4, 1, C_)):
        m = ts.create_model("vit_micro_reg4_patch16_64")
        m.reg_token = nn.Parameter(torch.zeros(*shape))
        _refused(m, "reg_token must be")
    for rows in (17, 20, 22):                                              # 16 patches, P = 5: 16 or 21 rows
        m = ts.create_model("vit_micro_reg4_patch16_64")
        m.pos_embed = nn.Parameter(torch.zeros(1, rows, C_))
        _refused(m, "pos_embed")
    m = ts.create_model("vit_micro_reg4_patch16_64")
    m.pos_embed = nn.Parameter(torch.zeros(1, 16, C_))                     # (the no_embed_class layout is fine)
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["num_prefix"] == 5
    # declared prefix count against what the parameters supply
    m = ts.create_model("vit_micro_patch16_64")
    m.num_prefix_tokens = 2
    _refused(m, "2 prefix tokens")
    m = ts.create_model("vit_micro_reg4_patch16_64")
    m.num_prefix_tokens = 1
    _refused(m, "1 prefix tokens")
    m = ts.create_model("vit_micro_reg4_patch16_64")
    m.num_prefix_tokens = 6
    _refused(m, "6 prefix tokens")
    # construction itself never raises for these: the check reports them
    m = ts.create_model("vit_micro_patch16_64")
    m.num_prefix_tokens = 2
    assert rajni_amd.RAJNIViTWrapper(m, SCHED).blocks[1].attn.num_prefix_tokens == 1
