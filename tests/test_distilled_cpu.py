"""DeiT's distilled models (timm `VisionTransformerDistilled`: a dist token behind the class token, two averaged heads) without a
GPU: the timm-shaped model, the unchanged weight streams of every older config, what the wrapper accepts and refuses, the
`head_rows` field of rajni_vit_prefix and its refusals through the library (fake pointers and a NULL workspace: nothing is
launched whichever way a check goes), the fused head on numpy, and the validity of the fixtures the GPU tests run."""
import ctypes as C
import dataclasses
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_distilled as nd
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import RAJNIAttention

DEIT = ["deit_tiny_distilled_patch16_224", "deit_small_distilled_patch16_224", "deit_base_distilled_patch16_224",
        "deit_base_distilled_patch16_384"]
OK, INVALID, UNSUPPORTED = 0, 1, 2
FAKE = 0x10000          # 16-byte aligned, never dereferenced


# ---------------------------------------------------------------------------------------------------------------
# timm_shaped
# ---------------------------------------------------------------------------------------------------------------

# sha256 (16 hex digits) over names and bytes of synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02) in draw order, computed on
# the parent commit (before `distilled` existed), for EVERY config that commit had
PARENT = {
    "vit_tiny_patch16_224": "a4f955f0c9977d03",
    "vit_small_patch16_224": "2cf2fd17aaf8e678",
    "vit_base_patch16_224": "75e15e0f1cee5f28",
    "vit_large_patch16_224": "dde976e1fb237d21",
    "vit_large_patch16_384": "fec2a7d4f97895d2",
    "deit3_base_patch16_224": "3c2f272ff90e580f",
    "vit_huge_patch14_224": "807ab7f93141d86a",
    "vit_micro_patch16_64": "0b25e3a4f0eed014",
    "deit3_micro_patch16_64": "c2a3ade870131ac1",
    "vit_micro512_patch16_64": "76d51cf3475f0560",
    "vit_micro_patch14_56": "fdb7bc9ccf0a1882",
    "vit_micro_d80_patch16_64": "84b42027dc237f6e",
    "vit_base_patch16_clip_224": "386edb674a0d1313",
    "vit_base_patch16_qknorm_224": "71fe309bc5363cba",
    "vit_micro_qknorm_patch16_64": "abc4c3af0448ab5f",
    "vit_micro_prenorm_patch16_64": "c32de75e3cca9410",
    "vit_micro_gap_patch16_64": "48516a1362d0fc4c",
    "vit_micro_fcnorm_patch16_64": "48516a1362d0fc4c",
    "vit_micro_all_patch16_64": "72a7b0e3144ff4ff",
    "vit_micro512_qknorm_patch16_64": "b3cca53cd33aea80",
    "vit_micro_d80_qknorm_patch16_64": "c9caaa8122056269",
    "vit_micro_reg4_patch16_64": "094ee1c5866ac488",
    "deit3_micro_reg4_patch16_64": "4f600a2150cd962c",
    "vit_micro_reg1_gap_patch14_56": "3d481281f0f5e16d",
    "vit_micro512_reg4_patch16_64": "96f85af0065b443a",
    "vit_small_patch14_reg4_dinov2": "f677e4ad0825ea0c",
    "vit_small_patch14_reg4_dinov2_518": "ded8a733c35d87eb",
    "vit_micro_patch16_400": "f1f2e604265d268c",
    "vit_micro_reg4_patch16_400": "c5f5c2d5f35ab936",
    "vit_base_patch16_clip_quickgelu_224": "386edb674a0d1313",
    "vit_base_patch32_clip_quickgelu_224": "06ed4f6cec2776e2",
    "vit_large_patch14_clip_quickgelu_224": "aab0cac0f767537b",
    "vit_micro_quickgelu_patch16_64": "0b25e3a4f0eed014",
    "vit_micro_clip_quickgelu_patch16_64": "c32de75e3cca9410",
    "vit_micro512_quickgelu_patch16_64": "76d51cf3475f0560",
    "vit_micro_quickgelu_h344_patch16_64": "9dded809342dd903",
}
NEW = DEIT + nd.MICRO


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def test_the_config_table_is_the_parents_plus_the_six_distilled_ones():
    assert list(ts.CONFIGS) == list(PARENT) + NEW
    assert all(ts.CONFIGS[n].distilled and ts.CONFIGS[n].num_prefix_tokens == 2 and ts.CONFIGS[n].reg_tokens == 0 for n in NEW)


@pytest.mark.parametrize("name", list(PARENT))
def test_existing_configs_keep_their_weight_stream(name):
    cfg = ts.CONFIGS[name]
    assert not cfg.distilled and cfg.num_prefix_tokens == 1 + cfg.reg_tokens
    sd = ts.synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02)
    assert sd_hash(sd) == PARENT[name]
    assert not any(k.startswith(("dist_token", "head_dist")) for k in sd)


def test_a_plain_model_has_no_distillation_attributes():
    m = ts.create_model("vit_micro_patch16_64")
    assert not hasattr(m, "dist_token") and not hasattr(m, "head_dist") and not hasattr(m, "distilled_training")


def test_the_config_field_and_the_new_configs():
    fields = list(ts.ViTConfig.__dataclass_fields__)
    # before reg_tokens - and before `act`: tests/test_activations_cpu.py holds those two to be the last fields
    assert fields[-1] == "reg_tokens" and fields.index("distilled") == len(fields) - 3 and ts.ViTConfig().distilled is False
    with pytest.raises(ValueError, match="distilled"):
        ts.ViTConfig(distilled=True, reg_tokens=4)
    dims = {"deit_tiny_distilled_patch16_224": (224, 192, 12, 3), "deit_small_distilled_patch16_224": (224, 384, 12, 6),
            "deit_base_distilled_patch16_224": (224, 768, 12, 12), "deit_base_distilled_patch16_384": (384, 768, 12, 12),
            "vit_micro_distilled_patch16_64": (64, 128, 4, 2), "vit_micro512_distilled_patch16_64": (64, 512, 4, 8)}
    for name, want in dims.items():
        c = ts.CONFIGS[name]
        assert (c.img_size, c.embed_dim, c.depth, c.num_heads) == want and c.patch_size == 16 and c.global_pool == "token"
        assert c.num_classes == (10 if "micro" in name else 1000)
    assert ts.CONFIGS["deit_tiny_distilled_patch16_224"].num_patches + 2 == 198
    for name in nd.MICRO + DEIT[:1]:
        cfg = ts.CONFIGS[name]
        sd = ts.synth_state_dict(cfg, seed=4, std=0.05, bias_std=0.02)
        # drawn after every other tensor
        assert list(sd)[-3:] == ["dist_token", "head_dist.weight", "head_dist.bias"]
        assert sd["dist_token"].shape == (1, 1, cfg.embed_dim) and sd["head_dist.weight"].shape == sd["head.weight"].shape
        assert sd["pos_embed"].shape[1] == cfg.num_patches + 2
        m = ts.create_model(cfg)
        assert m.num_prefix_tokens == 2 and tuple(m.dist_token.shape) == (1, 1, cfg.embed_dim) and m.distilled_training is False
        assert isinstance(m.head_dist, nn.Linear) and m.head_dist.out_features == m.head.out_features


@pytest.mark.parametrize("name", nd.MICRO)
def test_stock_forward_equals_the_hand_restatement(name):
    """token order [cls, dist, patches], pos-embed on every row, the two heads averaged: the timm-shaped model in fp64 against
    tests/numerics_distilled.py to 1e-6, and timm's training-mode pair"""
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **nd.FIX[name])
    sd = ts.state_dict_numpy(model)
    imgs = nd.images_of(cfg, 3)
    with torch.no_grad():
        stock = model.double()(torch.from_numpy(imgs).double()).numpy()
        x = model._pos_embed(model.patch_embed(torch.from_numpy(imgs).double())).numpy()
        feats = model.forward_features(torch.from_numpy(imgs).double())
    want, counts, _ = nd.vit_forward_restated(sd, imgs, {}, cfg)
    assert counts == [cfg.num_patches + 2] * cfg.depth
    assert np.abs(stock - want).max() <= 1e-6 * np.abs(want).max()
    pos = sd["pos_embed"][0].astype(np.float64)
    assert x.shape == (3, cfg.num_patches + 2, cfg.embed_dim)
    np.testing.assert_allclose(x[1, 0], sd["cls_token"][0, 0].astype(np.float64) + pos[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(x[1, 1], sd["dist_token"][0, 0].astype(np.float64) + pos[1], rtol=0, atol=1e-12)
    # by hand, without the restatement's helper
    t = lambda n: torch.from_numpy(sd[n]).double()
    by_hand = ((feats[:, 0] @ t("head.weight").T + t("head.bias")) + (feats[:, 1] @ t("head_dist.weight").T + t("head_dist.bias"))) / 2
    assert np.abs(stock - by_hand.numpy()).max() <= 1e-12
    model.distilled_training = True
    with torch.no_grad():
        assert torch.equal(model(torch.from_numpy(imgs).double()), torch.from_numpy(stock))      # eval mode: still the average
        pair = model.train()(torch.from_numpy(imgs).double())
    assert isinstance(pair, tuple) and len(pair) == 2 and np.abs((pair[0] + pair[1]).numpy() / 2 - stock).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
# the wrapper
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", nd.MICRO[:1] + DEIT)
def test_the_wrapper_accepts_distilled_models(name):
    cfg = ts.CONFIGS[name] if "micro" in name else dataclasses.replace(ts.CONFIGS[name], depth=2)
    base = ts.create_model(cfg)
    names = [n for n, _ in base.named_parameters()]
    w = rajni_amd.RAJNIViTWrapper(base, {1: {"keep_ratio": 0.5}})
    d = w.check_supported()
    assert d["num_prefix"] == 2 and d["head_rows"] == 2 and d["pool"] == "token" and not d["fc_norm"] and not d["ext"]
    assert [n for n, _ in w.named_parameters()] == ["m." + n for n in names]           # the fused head is no parameter
    assert isinstance(w.blocks[1].attn, RAJNIAttention) and w.blocks[1].attn.num_prefix_tokens == 2
    assert rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), {}).check_supported()["head_rows"] == 1
    assert rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_reg4_patch16_64"), {}).check_supported()["head_rows"] == 1
    # the no_embed_class layout (a pos-embed of n rows) passes like the register models'
    base.pos_embed = nn.Parameter(torch.zeros(1, cfg.num_patches, cfg.embed_dim))
    assert rajni_amd.RAJNIViTWrapper(base, {}).check_supported()["num_prefix"] == 2


def _refused(model, match="[Dd]istillation", exc=NotImplementedError):
    with pytest.raises(exc, match=match):
        rajni_amd.RAJNIViTWrapper(model, {}).check_supported()


def test_what_the_wrapper_refuses():
    name, C_ = "vit_micro_distilled_patch16_64", 128
    m = ts.create_model(name)
    m.head_dist = None                                                      # one of the pair without the other
    _refused(m)
    m = ts.create_model(name)
    m.dist_token = None
    _refused(m)
    m = ts.create_model(name)
    m.reg_token = nn.Parameter(torch.zeros(1, 4, C_))                        # together with registers
    _refused(m)
    for shape in ((1, 2, C_), (1, C_), (1, 1, C_ + 8)):
        m = ts.create_model(name)
        m.dist_token = nn.Parameter(torch.zeros(*shape))
        _refused(m)
    for bad in (nn.Linear(C_, 11), nn.Linear(C_ + 8, 10), nn.Identity()):    # a head_dist that is not shaped like head
        m = ts.create_model(name)
        m.head_dist = bad
        _refused(m)
    m = ts.create_model(name)
    m.global_pool = "avg"
    _refused(m)
    m = ts.create_model(name)
    m.fc_norm = nn.LayerNorm(C_)
    _refused(m)
    m = ts.create_model(name)
    m.num_prefix_tokens = 3
    _refused(m)
    m = ts.create_model(name)
    m.distilled_training = True
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["head_rows"] == 2      # eval mode: the average, as timm
    m.train()
    _refused(m)
    # the opt-ins that do not serve two head rows
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(name), {})
    with pytest.raises(ValueError, match="[Dd]istillation"):
        w.set_last_block_cls_only(True)
    with pytest.raises(NotImplementedError, match="[Dd]istillation"):
        w.set_weight_format("fp8_mfma")
    w.set_weight_format("fp8").set_last_block_cls_only(False)                        # these are fine
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), {}).set_last_block_cls_only(True)
    w.m.dist_token, w.m.head_dist = nn.Parameter(torch.zeros(1, 1, C_)), nn.Linear(C_, 10)      # (swapped in after the setter)
    w.m.pos_embed, w.m.num_prefix_tokens = nn.Parameter(torch.zeros(1, 18, C_)), 2
    with pytest.raises(ValueError, match="[Dd]istillation"):
        w.check_supported()


# ---------------------------------------------------------------------------------------------------------------
# the C ABI: the record and its refusals
# ---------------------------------------------------------------------------------------------------------------

def test_record_layout_and_abi_version():
    assert C.sizeof(nat.VitPrefix) == 16
    assert (nat.VitPrefix.num_prefix.offset, nat.VitPrefix.head_rows.offset, nat.VitPrefix.reg_token.offset) == (0, 4, 8)
    assert nat.lib().rajni_abi_version() == nat.ABI_VERSION == 8
    pre = nat.VitPrefix(5, FAKE)                       # positional construction is (num_prefix, reg_token), as before
    assert (pre.num_prefix, pre.head_rows, pre.reg_token) == (5, 0, FAKE)
    assert bytes(nat.VitPrefix()) == bytes(16)
    # the sizes of the other records hold
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.QkAffine) == 32


def _plan(keeps=(0, 8, 6, 0), buffers=(1, 2)):
    """img 64 / patch 16 (16 patch tokens), depth 4, C 128 = 2 x 64, hidden 512, 16 classes, bf16 - the plan of
    tests/test_forward_refusals_cpu.py: fake weight addresses, a NULL workspace"""
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
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = 128, 2, 64, depth, 512, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-6, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, FAKE)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    return p, blocks


def _prefix(num_prefix=2, head_rows=2, reg=FAKE):
    pre = nat.VitPrefix()
    pre.num_prefix, pre.head_rows, pre.reg_token = num_prefix, head_rows, reg
    return pre


def _forward(p, pre, ext=None):
    lib = nat.lib()
    rc = lib.rajni_vit_forward_ext_prefix(C.byref(p), C.byref(ext) if ext is not None else None,
                                          C.byref(pre) if pre is not None else None, FAKE + 0x100, FAKE + 0x200, None)
    return rc, lib.rajni_last_error().decode()


def _passes_every_check(p, pre, ext=None):
    """stops at the missing workspace: every check up front went through and nothing was launched"""
    rc, msg = _forward(p, pre, ext)
    assert rc == INVALID and "workspace too small" in msg, (rc, msg)


def test_a_valid_distilled_record_passes_every_check_up_front():
    p, keep_alive = _plan()
    _passes_every_check(p, _prefix())
    _passes_every_check(p, _prefix(), nat.VitExt())                          # an all-zero ext record
    for hr in (0, 1):                                                        # the forward as it was
        _passes_every_check(p, _prefix(5, hr))
        _passes_every_check(p, _prefix(1, hr, None))
        _passes_every_check(p, _prefix(0, hr, None))
    _passes_every_check(p, None)
    del keep_alive


@pytest.mark.parametrize("head_rows", [-1, 3, 2 ** 20])
def test_head_rows_outside_0_to_2(head_rows):
    p, keep_alive = _plan()
    rc, msg = _forward(p, _prefix(2, head_rows))
    assert rc == INVALID and "head_rows must be 0..2" in msg, (rc, msg)
    assert nat.lib().rajni_vit_workspace_bytes_prefix(C.byref(p), C.byref(_prefix(2, head_rows))) == 0
    del keep_alive


@pytest.mark.parametrize("num_prefix, reg", [(0, None), (1, None), (3, FAKE), (5, FAKE)])
def test_two_head_rows_need_exactly_two_prefix_tokens(num_prefix, reg):
    p, keep_alive = _plan()
    rc, msg = _forward(p, _prefix(num_prefix, 2, reg))
    assert rc == INVALID and "needs num_prefix == 2" in msg, (rc, msg)
    del keep_alive


def test_two_head_rows_need_a_token_head_behind_the_final_norm():
    p, keep_alive = _plan()
    for field, value in (("pool", nat.POOL_AVG), ("fc_norm_w", FAKE), ("norm_absent", 1)):
        ext = nat.VitExt()
        setattr(ext, field, value)
        if field == "norm_absent":
            ext.fc_norm_w = FAKE        # (a plan without a final norm is only legal with an fc_norm; either refuses)
        _passes_every_check(p, _prefix(5, 0), ext)                           # control: legal without the distilled head
        rc, msg = _forward(p, _prefix(), ext)
        assert rc == UNSUPPORTED and "head_rows=2 needs a token head" in msg, (field, rc, msg)
    del keep_alive


def test_two_head_rows_with_the_cls_only_last_block_or_fp8_activations():
    p, keep_alive = _plan()
    p.cls_only_last_block = 1
    _passes_every_check(p, _prefix(5, 0))
    rc, msg = _forward(p, _prefix())
    assert rc == INVALID and "cls_only_last_block" in msg and "head_rows=2" in msg, (rc, msg)
    p.cls_only_last_block = 0
    # act_fp8 needs C >= 512, multiples of 256 and e4m3 weights with scales: a plan that is legal without the distilled head
    p.C, p.H, p.hidden, p.act_fp8 = 512, 8, 2048, 1
    for blk in keep_alive:
        blk.qkv_s = blk.proj_s = blk.fc1_s = blk.fc2_s = FAKE
    _passes_every_check(p, _prefix(5, 0))
    rc, msg = _forward(p, _prefix())
    assert rc == UNSUPPORTED and "head_rows=2 is unsupported with act_fp8" in msg, (rc, msg)
    del keep_alive


def test_workspace_and_last_block_eligibility():
    lib = nat.lib()
    p, keep_alive = _plan()
    size = lambda pre: lib.rajni_vit_workspace_bytes_prefix(C.byref(p), C.byref(pre))
    # head_rows 0 and 1 ask for exactly what the record asked for before; 2 adds the second query row and the {0, 1} selection
    assert size(_prefix(2, 0)) == size(_prefix(2, 1)) > 0
    extra = size(_prefix(2, 2)) - size(_prefix(2, 0))
    assert 0 < extra <= 2 * 256 + p.B * p.C * 2 + p.B * 8
    eligible = lambda plan, pre: lib.rajni_debug_last_block_cls_rows(C.byref(plan), None, C.byref(pre))
    assert eligible(p, _prefix()) == 1                                        # the last block does not prune
    pruning, keep_alive2 = _plan(keeps=(0, 8, 0, 4), buffers=(1, 3))
    assert eligible(pruning, _prefix()) == 0
    try:
        lib.rajni_debug_set_last_block_all_rows(1)
        assert eligible(p, _prefix()) == 0
    finally:
        lib.rajni_debug_set_last_block_all_rows(0)
    del keep_alive, keep_alive2


# ---------------------------------------------------------------------------------------------------------------
# the fused head and the fixtures
# ---------------------------------------------------------------------------------------------------------------

def test_fused_head_on_numpy():
    """[W / 2 | W_dist / 2] against [n0 | n1] plus (b + b_dist) / 2 is the average of the two heads: exactly in fp64 on fp32 data
    (halving is exact), and to fp32 rounding when both are evaluated in fp32"""
    cfg = ts.CONFIGS["vit_micro_distilled_patch16_64"]
    sd = ts.synth_state_dict(cfg, **nd.FIX["vit_micro_distilled_patch16_64"])
    rng = np.random.default_rng(5)
    n = rng.standard_normal((7, 2, cfg.embed_dim)).astype(np.float32)
    w, b = nd.fused_head(sd)
    assert w.shape == (cfg.num_classes, 2 * cfg.embed_dim) and b.shape == (cfg.num_classes,) and w.dtype == b.dtype == np.float32
    np.testing.assert_array_equal(2 * w[:, :cfg.embed_dim], sd["head.weight"])
    np.testing.assert_array_equal(2 * w[:, cfg.embed_dim:], sd["head_dist.weight"])
    want = nd.averaged_heads(torch.from_numpy(n[:, 0]).double(), torch.from_numpy(n[:, 1]).double(), sd).numpy()
    fused64 = n.reshape(7, -1).astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    # only the fp32 rounding of (b + b_dist) / 2 separates the two
    assert np.abs(fused64 - want).max() <= 2.0 ** -24 * np.abs(sd["head.bias"] + sd["head_dist.bias"]).max()
    fused32 = n.reshape(7, -1) @ w.T + b
    eps32 = 2.0 ** -24
    budget = (2 * cfg.embed_dim + 2) * eps32 * (np.abs(n.reshape(7, -1)) @ np.abs(w).T + np.abs(b))      # fp32 dot product of length 2C
    assert (np.abs(fused32 - want) <= budget).all()
    print(f"[distilled] fused head vs the averaged heads: fp64 {np.abs(fused64 - want).max():.3g}, fp32 {np.abs(fused32 - want).max():.3g}")


@pytest.mark.parametrize("name", nd.MICRO)
def test_fixtures_can_tell_whether_the_feature_is_there_and_fit_the_format(name):
    """every forward fixture of tests/test_gpu_distilled.py: `head` on the class row alone, and the dist row dropped from the
    stream, each move the fp32 logits by at least 5x the loosest bar (1e-2 of the logit scale), and the bf16 format's own cost
    (an ideal bf16 forward on the CPU) leaves a quarter of that bar free - the rule FIX's seeds were chosen by"""
    cfg = ts.CONFIGS[name]
    sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, **nd.FIX[name]))
    for sched, B, seed in nd.FORWARD_CASES + [("carried", 1, 2)]:
        imgs = nd.images_of(cfg, B, seed)
        a, b, need = nd.feature_matters(sd, imgs, nd.SCHEDULES[sched], cfg, max(nd.BAR.values()))
        assert a >= need and b >= need, (sched, B, seed, a, b, need)
        if (sched, B, seed) in nd.FORWARD_CASES:
            cost = nd.format_cost(sd, imgs, nd.SCHEDULES[sched], cfg)
            print(f"[distilled] {name} {sched} B={B} images {seed}: an ideal bf16 forward costs {cost / 1e-2:.2f} x the 1e-2 bar")
            assert cost <= nd.FORMAT_HEADROOM * 1e-2, (sched, B, seed, cost)


def test_token_counts_of_the_schedules():
    assert nd.token_counts(18, 4, nd.SCHEDULES["carried"], 2) == [18, 18, 10, 6]
    assert nd.token_counts(18, 4, nd.SCHEDULES["last"], 2) == [18, 18, 14, 14]
    from rajni_amd.wrapper.model import plan_token_counts, normalise_schedule
    for s in nd.SCHEDULES.values():
        assert plan_token_counts(18, 4, normalise_schedule(s), 2) == nd.token_counts(18, 4, s, 2)
