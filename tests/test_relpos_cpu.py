"""A relative position bias on the attention logits (include/rajni_hip_relpos.h) without a GPU: the record's layout against the
header and the ABI the feature must not move, the refusals of the forward and of the two kernel entries (before any launch:
every plan here has workspace = NULL and fake addresses nobody follows, the pattern of tests/test_activations_cpu.py), the
wrapper's recognition and decomposition of a bias, its refusals, and the validity of the forward fixtures of
tests/numerics_relpos.py."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_eva as ne
import numerics_relpos as nrp
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import RAJNIViTWrapper
from rajni_amd.wrapper import model as wm

OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
IMAGES, LOGITS = PTR + 0x100, PTR + 0x200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rajni_hip_relpos.h")).read()
SCHED = {1: {"keep_ratio": 0.5, "update": True}}


# ---- the record and the ABI ------------------------------------------------------------------------------------------------

def test_record_layout_and_placement_lines_match_the_header():
    body = re.search(r"typedef struct \{(.*?)\} rajni_vit_relpos;", HEADER, re.S).group(1)
    names = re.findall(r"(\w+)[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in nat.VitRelPos._fields_] == ["table", "prefix_q", "prefix_k", "prefix_qk", "block_stride", "gh", "gw"]
    assert C.sizeof(nat.VitRelPos) == 48
    assert [getattr(nat.VitRelPos, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44]
    assert re.search(r"#define RAJNI_RELPOS_MAX_GRID 32\b", HEADER) and nat.RELPOS_MAX_GRID == 32
    assert '#include "rajni_hip_mlpnorm.h"' in HEADER
    table = HEADER[HEADER.index("---- placement"):HEADER.index("(end of the placement table)")]
    rows = dict(re.findall(r"^ \*   (rajni_\w+): (.+)$", table, re.M))
    assert rows == {
        "rajni_attention_relpos": "qkv 16, keep_idx 4, out 16, table 4, prefix_q 4, prefix_k 4, prefix_qk 4, pos 4",
        "rajni_score_select_relpos": "qkv 16, scores_out 2, keep_idx 4, next_scores 2, workspace 256, prefix_q 4, prefix_qk 4",
        "rajni_vit_forward_relpos": "images 16, logits 16",
        "rajni_vit_relpos": "table 4, prefix_q 4, prefix_k 4, prefix_qk 4"}


# sha256 (16 hex digits) of every header that existed at the parent commit: none of them changes
OTHER_HEADERS = {
    "rajni_hip.h": "7bed3c892bcac57d",
    "rajni_hip_debug.h": "78c74124628c1507",
    "rajni_hip_layers.h": "4e37c1412b992f9e",
    "rajni_hip_image.h": "2ddb44aec4aed464",
    "rajni_hip_query.h": "a8db4b5756c10a27",
    "rajni_hip_attnpool.h": "3a143ac1f45ec423",
    "rajni_hip_norm.h": "aca2b19cf1ed37f9",
    "rajni_hip_rope.h": "7b5fc09b2877c592",
    "rajni_hip_mlpnorm.h": "8a60485db8f40c79",
}


def test_the_header_is_additive():
    lib = nat.lib()
    assert nat.RELPOS_SYMBOLS == ("rajni_attention_relpos", "rajni_score_select_relpos", "rajni_vit_workspace_bytes_relpos",
                                  "rajni_vit_forward_relpos")
    for sym in nat.RELPOS_SYMBOLS:
        assert getattr(lib, sym).argtypes is not None
    assert nat.ABI_VERSION == 8 and lib.rajni_abi_version() == 8 and nat.NUM_KCLASS == 17
    assert not set(nat.RELPOS_SYMBOLS) & set(nat.EXPORTED_SYMBOLS)
    inc = os.path.join(ROOT, "include")
    digest = lambda h: hashlib.sha256(open(os.path.join(inc, h), "rb").read()).hexdigest()[:16]
    assert {h: digest(h) for h in OTHER_HEADERS} == OTHER_HEADERS
    others = "".join(open(os.path.join(inc, h)).read() for h in sorted(OTHER_HEADERS))
    assert not set(nat.RELPOS_SYMBOLS) & set(re.findall(r"\b(rajni_\w+)\s*\(", others)) and "relpos" not in others
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", others)
    # every record that existed keeps its size
    sizes = {nat.VitExt: 72, nat.VitPrefix: 16, nat.VitImage: 8, nat.VitQuery: 8, nat.VitNorm: 24, nat.VitLayers: 40, nat.VitRope: 40}
    assert {k.__name__: C.sizeof(k) for k in sizes} == {k.__name__: v for k, v in sizes.items()}
    assert C.sizeof(nat.VitPlan) == 168 and C.sizeof(nat.Block) == 200 and C.sizeof(nat.VitAttnPool) == 112 and C.sizeof(nat.LinearArgs) == 144


# ---- the forward's refusals, before any launch ---------------------------------------------------------------------------

def _plan(act_fp8=0, C_=128, hidden=512, H=2, D=64):
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, PTR)
        if act_fp8:
            blocks[i].qkv_s = blocks[i].proj_s = blocks[i].fc1_s = blocks[i].fc2_s = PTR
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = C_, H, D, depth, hidden, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-5, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, PTR)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.act_fp8 = act_fp8
    return p, blocks


def _rel(gh=4, gw=4, H=2, per_block=False):
    r = nat.VitRelPos()
    r.table, r.prefix_q, r.prefix_k, r.prefix_qk = PTR, PTR + 0x1000, PTR + 0x2000, PTR + 0x3000
    r.gh, r.gw = gh, gw
    r.block_stride = H * (2 * gh - 1) * (2 * gw - 1) if per_block else 0
    return r


def _forward(p, rel, pre=None, img=None, qry=None, rope=None):
    lib = nat.lib()
    ref = lambda r: C.byref(r) if r is not None else None
    ext = nat.VitExt(pool=nat.POOL_AVG) if qry is not None and qry.class_token == 0 else None
    rc = lib.rajni_vit_forward_relpos(C.byref(p), ref(ext), ref(pre), None, ref(img), ref(qry), None, None, ref(rope), None, ref(rel),
                                      IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _size(p, rel, pre=None, img=None):
    ref = lambda r: C.byref(r) if r is not None else None
    return nat.lib().rajni_vit_workspace_bytes_relpos(C.byref(p), ref(pre), ref(img), None, None, None, None, None, ref(rel))


def test_a_valid_plan_stops_at_the_workspace_and_the_map_is_all_the_record_adds():
    base = nat.lib().rajni_vit_workspace_bytes(C.byref(_plan()[0]))
    for kw in (dict(), dict(per_block=True)):
        p, keep = _plan()
        rc, msg = _forward(p, _rel(**kw))
        assert rc == INVALID and "workspace too small" in msg, msg
        assert _size(p, _rel(**kw)) == base + (4 * 17 * 4 + 255) // 256 * 256          # B * n0 * 4 bytes, whole 256-byte units
    # NULL and the all-zero record: the dry run of rajni_vit_forward_mlpnorm, and its size
    p, keep = _plan()
    assert _size(p, None) == _size(p, nat.VitRelPos()) == base
    for rec in (None, nat.VitRelPos()):
        rc, msg = _forward(p, rec)
        assert rc == INVALID and msg.startswith("rajni_vit_forward: workspace too small"), msg
    # a rectangular fixed grid
    p, keep = _plan()
    p.img_size = 48
    rc, msg = _forward(p, _rel(3, 6), img=nat.VitImage(48, 96))
    assert rc == INVALID and "workspace too small" in msg, msg


def test_every_refusal_of_the_forward_names_the_combination():
    who = "rajni_vit_forward_relpos"
    def refused(code, text, p=None, **kw):
        p = p or _plan()[0]
        rel = kw.pop("rel", None) or _rel()
        rc, msg = _forward(p, rel, **kw)
        assert rc == code and msg.startswith(who) and text in msg, (rc, msg)
        if "img" not in kw and "qry" not in kw and "rope" not in kw:
            assert _size(p, rel) == 0 and text in nat.lib().rajni_last_error().decode()
    for name in ("table", "prefix_q", "prefix_k", "prefix_qk"):
        r = _rel()
        setattr(r, name, None)
        refused(INVALID, f"null pointer (relpos.{name})", rel=r)
    refused(INVALID, "must equal the forward's patch grid, 4 x 4 (3 x 6)", rel=_rel(3, 6))
    r = _rel()
    r.block_stride = 7
    refused(INVALID, "relpos.block_stride must be 0 (one table for all blocks) or H * (2 gh - 1) * (2 gw - 1) = 98 (7)", rel=r)
    # the cap: 33 x 33 patches
    p = _plan()[0]
    p.img_size = 33 * 16
    refused(UNSUPPORTED, "on a 33 x 33 grid - the cap is 32 x 32 patches", p=p, rel=_rel(33, 33))
    p = _plan()[0]
    p.img_size = 32 * 16
    assert "workspace too small" in _forward(p, _rel(32, 32))[1]
    # head dims other than 64
    refused(UNSUPPORTED, "with head dim 32 - the bias kernels are head dim 64 only", p=_plan(H=4, D=32)[0], rel=_rel(H=4))
    # fp8_mfma
    refused(UNSUPPORTED, "unsupported with plan.act_fp8", p=_plan(act_fp8=1, C_=512, hidden=2048, H=8)[0], rel=_rel(H=8))
    # the mean importance query, and a sequence without a class token
    refused(UNSUPPORTED, "with the mean importance query (RAJNI_QUERY_MEAN)", qry=nat.VitQuery(1, nat.QUERY_MEAN))
    refused(UNSUPPORTED, "with query.class_token = 0", qry=nat.VitQuery(0, nat.QUERY_MEAN))
    # RoPE together with a bias
    rope = nat.VitRope()
    rope.cos, rope.sin, rope.rows = PTR, PTR + 0x1000, 16
    refused(UNSUPPORTED, "together with RoPE (a rope record)", rope=rope)
    # the CLS-only last block
    p = _plan()[0]
    p.cls_only_last_block = 1
    refused(UNSUPPORTED, "with plan.cls_only_last_block", p=p)
    # placement
    r = _rel()
    r.table = PTR + 2
    rc, msg = _forward(_plan()[0], r)
    assert rc == INVALID and "table" in msg and "rajni_vit_forward_relpos: relpos" in msg, msg


def test_the_kernel_entries_refuse_before_any_launch():
    lib = nat.lib()
    att = lambda D=64, gh=4, gw=4, table=PTR, scale=0.125: lib.rajni_attention_relpos(
        PTR, None, PTR + 0x10000, 1, 17, 17, 2, D, scale, nat.RAJNI_BF16, table, PTR, PTR, PTR, gh, gw, 1, None, None)
    err = lambda: lib.rajni_last_error().decode()
    assert att(D=32) == UNSUPPORTED and "head dim 32 - head dim 64 only" in err()
    assert att(gh=33) == UNSUPPORTED and "takes at most 32 x 32 patches" in err()
    assert att(gh=0) == INVALID and "bad grid" in err()
    assert att(table=None) == INVALID and "null pointer" in err()
    assert att(table=PTR + 2) == INVALID and "table" in err()
    assert att(scale=0.0) == INVALID and "scale must be positive" in err()
    sel = lambda pq=PTR, pqk=PTR, P=1: lib.rajni_score_select_relpos(PTR, 2, 17, 2, 64, 1e-6, P, 4, PTR, PTR, PTR, nat.RAJNI_BF16, None, 0,
                                                                    pq, pqk, None)
    assert sel(pq=None) == INVALID and "null pointer" in err()
    assert sel(pqk=PTR + 2) == INVALID and "prefix_qk" in err()
    assert sel(P=0) == INVALID and "num_prefix must be 1.." in err()


# ---- the wrapper: recognition, decomposition, refusals -------------------------------------------------------------------

@pytest.mark.parametrize("name", nrp.MICRO)
def test_decomposition_round_trips_the_dense_bias_exactly(name):
    m = nrp.build_model(name)
    cfg = m.cfg
    w = RAJNIViTWrapper(m, SCHED)
    d = w.check_supported()
    assert d["rel_pos"] == ("shared" if cfg.rel_pos in ("beit_shared", "srelpos") else "block") and d["rel_pos_grid"] == cfg.grid
    per, shared = wm.rel_pos_sources(m, w.blocks)
    tabs = nrp.native_tables(ts.state_dict_numpy(m), cfg)             # the contract's inputs, read from the state dict
    gh, gw = cfg.grid
    n0 = gh * gw + 1
    for i in range(cfg.depth if per else 1):
        dense = wm.dense_rel_pos_bias(per[i] if per else shared, cfg.num_heads, "test")
        assert tuple(dense.shape) == (cfg.num_heads, n0, n0)
        got = wm.decompose_rel_pos_bias(dense, gh, gw, 1)
        for g, want in zip(got, tabs):
            np.testing.assert_array_equal(g.numpy().astype(np.float64), want[i])
        back = nrp.dense_bias(*(g.numpy() for g in got), gh, gw, 1, np.arange(n0), np.arange(n0))
        np.testing.assert_array_equal(back, dense.numpy().astype(np.float64))


def test_a_block_bias_beside_a_shared_one_is_summed_and_disagreeing_blocks_are_refused():
    m = nrp.build_model("beit_micro_patch16_64")
    m.rel_pos_bias = ts.RelativePositionBias(m.cfg.grid, m.cfg.num_heads)
    with torch.no_grad():
        m.rel_pos_bias.relative_position_bias_table.copy_(torch.arange(52 * 2, dtype=torch.float32).reshape(52, 2) / 8)
    w = RAJNIViTWrapper(m, SCHED)
    assert w.check_supported()["rel_pos"] == "block"
    per, shared = wm.rel_pos_sources(m, w.blocks)
    both = wm.dense_rel_pos_bias(per[2], 2, "t") + wm.dense_rel_pos_bias(shared, 2, "t")
    table = wm.decompose_rel_pos_bias(both, 4, 4, 1)[0]
    own = m.blocks[2].attn.relative_position_bias_table.detach()[:49].t() + m.rel_pos_bias.relative_position_bias_table.detach()[:49].t()
    assert torch.equal(table, own)
    m.rel_pos_bias = None
    m.blocks[3].attn.relative_position_bias_table = None
    with pytest.raises(NotImplementedError, match="block 0 has a relative position bias and block 3 has none"):
        RAJNIViTWrapper(m, SCHED).check_supported()


def test_a_perturbed_bias_is_refused_naming_the_block_and_the_element():
    m = nrp.build_model("beit_micro_patch16_64")
    w = RAJNIViTWrapper(m, SCHED)
    dense = wm.dense_rel_pos_bias(wm.rel_pos_sources(m, w.blocks)[0][1], 2, "t")
    for (h, q, k), what in (((1, 3, 5), "another pair of the same offset"), ((0, 0, 7), "the first prefix-query / patch-key pair"),
                            ((1, 9, 0), "the first patch-query / prefix-key pair")):
        bad = dense.clone()
        bad[h, q, k] = torch.nextafter(bad[h, q, k], torch.tensor(9.0))             # one ulp
        with pytest.raises(NotImplementedError, match=re.escape(f"block 1: relative position bias: not a function of the relative "
                                                                 f"offset: element [head {h}, query {q}, key {k}]") + ".*" + what):
            wm.decompose_rel_pos_bias(bad, 4, 4, 1, "block 1: relative position bias")
    # ... and through the wrapper, at pack time (host only: the refusal precedes every device call)
    class Bent(nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner
            self.window_size = inner.window_size

        def get_bias(self):
            b = self.inner.get_bias().clone()
            b[0, 1, 4, 9] += 0.5
            return b
    m = nrp.build_model("vit_micro_relpos_patch16_64")
    m.blocks[2].attn.rel_pos = Bent(m.blocks[2].attn.rel_pos)
    w = RAJNIViTWrapper(m, SCHED)
    with pytest.raises(NotImplementedError, match=r"block 2: relative position bias: not a function of the relative offset: element "
                                                  r"\[head 1, query 4, key 9\]"):
        w._pack_weights(torch.device("cpu"), torch.float32)


def test_models_outside_the_contract_are_refused_not_run_without_the_bias():
    def refused(mutate, text, name="beit_micro_patch16_64"):
        m = nrp.build_model(name)
        mutate(m)
        with pytest.raises(NotImplementedError, match=text):
            RAJNIViTWrapper(m, SCHED).check_supported()
    def no_getter(m):
        for blk in m.blocks:
            blk.attn._get_rel_pos_bias = None
    refused(no_getter, "relative_position_bias_table without a callable attn._get_rel_pos_bias")
    refused(lambda m: setattr(m.blocks[0].attn, "rel_pos", nn.Identity()), "attn.relative_position_bias_table together with attn.rel_pos")
    refused(lambda m: [setattr(b.attn, "rel_pos", nn.Identity()) for b in m.blocks], r"attn.rel_pos \(Identity\) has no get_bias",
            name="vit_micro_relpos_patch16_64")
    refused(lambda m: setattr(m, "rel_pos_bias", nn.Identity()), r"reading the bias failed \(TypeError", name="beit_micro_shared_patch16_64")
    refused(lambda m: setattr(m, "shared_rel_pos", nn.Identity()), r"base_model.shared_rel_pos \(Identity\) has no get_bias")
    class Wrong(nn.Module):
        def forward(self):
            return torch.zeros(2, 7, 7)
    refused(lambda m: setattr(m, "rel_pos_bias", Wrong()), "cannot tell the grid of a relative position bias over 6 patches",
            name="beit_micro_shared_patch16_64")
    # the parent commit ran such a model without its bias: the description now says it has one
    assert RAJNIViTWrapper(nrp.build_model("beit_micro_patch16_64"), SCHED).check_supported()["rel_pos"] == "block"
    assert RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), SCHED).check_supported()["rel_pos"] is None


def test_the_wrapper_refuses_what_section_three_lists():
    new = lambda name="beit_micro_patch16_64": RAJNIViTWrapper(nrp.build_model(name), SCHED)
    with pytest.raises(NotImplementedError, match="set_last_block_cls_only: not supported on a model with a relative position bias"):
        new("vit_micro_relpos_patch16_64").set_last_block_cls_only(True)
    with pytest.raises(NotImplementedError, match=r'set_weight_format\("fp8_mfma"\): not supported on a model with a relative position bias'):
        new().set_weight_format("fp8_mfma")
    new().set_weight_format("fp8")
    with pytest.raises(NotImplementedError, match=r"set_dynamic_img_size\(True\): not supported on a model with a relative position bias"):
        new().set_dynamic_img_size(True)
    with pytest.raises(NotImplementedError, match=r'set_importance_query\("mean"\): not supported on a model with a relative position bias'):
        new().set_importance_query("mean")
    # attached after the setters: the description refuses
    w = RAJNIViTWrapper(ts.create_model("vit_micro_rope_patch16_64"), SCHED)
    w.m.rel_pos_bias = ts.RelativePositionBias((4, 4), 2)
    with pytest.raises(NotImplementedError, match="also has rotary position embeddings"):
        w.check_supported()
    m = ts.create_model(ts.RelPosViTConfig(img_size=64, embed_dim=128, depth=2, num_heads=4, num_classes=10, abs_pos=False, rel_pos="relpos"))
    with pytest.raises(NotImplementedError, match="head dim 32: the bias kernels are head dim 64 only"):
        RAJNIViTWrapper(m, SCHED).check_supported()
    m = ts.create_model(ts.RelPosViTConfig(img_size=16 * 33, embed_dim=64, depth=1, num_heads=1, num_classes=10, abs_pos=False,
                                           rel_pos="srelpos"))
    with pytest.raises(NotImplementedError, match="on a 33 x 33 grid: the cap is 32 x 32 patches"):
        RAJNIViTWrapper(m, {}).check_supported()
    # the module's own forward takes no table and does not run without it
    w = new()
    with pytest.raises(NotImplementedError, match="RAJNIAttention: this attention has a relative position bias"):
        w.blocks[1].attn.forward(torch.zeros(1, 17, 128, device="meta"))


# ---- the timm-shaped models ----------------------------------------------------------------------------------------------------

def test_configs_keep_the_other_tables_and_name_the_real_checkpoints():
    assert len(ts.ViTConfig.__dataclass_fields__) == 20
    for name in ("beit_base_patch16_224", "beit_large_patch16_224", "beitv2_base_patch16_224", "vit_relpos_base_patch16_clsgap_224"):
        cfg = ts.config_of(name)
        assert cfg.head_dim == 64 and cfg.grid == (14, 14) and not cfg.abs_pos and cfg.rel_pos in ("beit", "relpos")
    cfg = ts.config_of("beit_micro_patch16_48x96")
    assert cfg.grid == (3, 6) and cfg.num_patches == 18
    sd = ts.synth_state_dict(ts.config_of("beit_micro_patch16_64"), seed=3, std=0.08, bias_std=0.1)
    t = sd["blocks.2.attn.relative_position_bias_table"]
    assert t.shape == (52, 2) and 0.7 < t.std() < 1.3                    # the fixture choice: tables of order one
    assert "pos_embed" not in sd and "blocks.0.attn.q_bias" in sd and "blocks.0.gamma_1" in sd and "fc_norm.weight" in sd


def test_relative_position_index_is_timms():
    idx = ts.relative_position_index(2, 3, True)
    assert idx.shape == (7, 7) and int(idx[0, 3]) == 15 and int(idx[4, 0]) == 16 and int(idx[0, 0]) == 17
    # query patch (1, 2) against key patch (0, 0): dy = 1, dx = 2 -> (1 + 1) * 5 + (2 + 2)
    assert int(idx[1 + 5, 1 + 0]) == 14 and int(idx[1 + 0, 1 + 5]) == 0


# ---- the forward fixtures ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", nrp.MICRO)
def test_restatement_is_the_stock_forward_and_with_zero_tables_the_existing_graph(name):
    cfg, sd, iseed = nrp.fixture(name)
    imgs = nrp.images_of(cfg, 2, iseed)
    with torch.no_grad():
        stock = nrp.build_model(name)(torch.from_numpy(imgs)).numpy()
    got, counts, _ = nrp.vit_forward_restated(sd, imgs, {}, cfg)
    assert np.abs(got - stock).max() <= 1e-5 * np.abs(stock).max() and counts == [cfg.num_patches + 1] * cfg.depth
    zero = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, zero_tables=True)
    old = ne.vit_forward_restated(sd, imgs, nrp.SCHED, cfg)
    np.testing.assert_array_equal(zero[0], old[0])
    assert all(np.array_equal(zero[2][i]["keep_idx"], old[2][i]["keep_idx"]) for i in old[2])


@pytest.mark.parametrize("sched", ["SCHED", "CARRIED"])
@pytest.mark.parametrize("name", nrp.MICRO)
def test_committed_seeds_clear_every_criterion(name, sched):
    cfg = nrp.fixture(name)[0]
    sep = nrp.mutant_separations(name, sched)
    print(name, sched, {k: round(v, 4) for k, v in sep.items()})
    for mut, v in sep.items():
        if nrp.vacuous(cfg, mut):
            assert v == 0.0, (mut, v)
        else:
            assert v >= nrp.MUTANT_FACTOR * nrp.BAR["bf16"], (mut, v)
    assert nrp.boundary_gap_ratios(name, sched) >= nrp.GAP_FACTOR
    assert nrp.selections_agree(name, sched)          # no image is left out of a free-running comparison


@pytest.mark.parametrize("name", nrp.MICRO)
def test_committed_seeds_are_within_the_format_headroom(name):
    wseed = nrp.SEEDS[name][0]
    assert nrp.SEEDS[name][1] == wseed + 4
    assert max(nrp.format_cost(name, wseed, B) for B in (1, nrp.BATCH)) <= nrp.FORMAT_HEADROOM * nrp.BAR["bf16"]


def test_axes_swapped_is_live_on_the_rectangular_fixture_and_packed_positions_needs_pruning():
    # exchanging dy and dx moves every fixture (a learned table is not symmetric), the 3 x 6 one included - the one on which a
    # kernel that decodes a place with the wrong grid width also reads outside the rows it should
    assert nrp.mutant_separations("beit_micro_patch16_48x96")["axes_swapped"] >= nrp.MUTANT_FACTOR * nrp.BAR["bf16"]
    cfg, sd, iseed = nrp.fixture("beit_micro_patch16_64")
    imgs = nrp.images_of(cfg, 2, iseed)
    a = nrp.vit_forward_restated(sd, imgs, {}, cfg)[0]
    b = nrp.vit_forward_restated(sd, imgs, {}, cfg, mutant="packed_positions")[0]
    np.testing.assert_array_equal(a, b)               # without pruning the packed row IS the place
