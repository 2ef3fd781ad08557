"""The norm inside the MLP and timm Eva's block layout (include/rajni_hip_mlpnorm.h) without a GPU: the record's layout against
the header and the ABI the feature must not move, the refusals of the forward and of rajni_hidden_norm (before any launch: every
plan here has workspace = NULL and fake addresses nobody follows, the pattern of tests/test_rope_cpu.py), the wrapper's
recognition of every spelling and its refusals, the packed q / k / v projection, the restated forward against the timm-shaped
module, the kernel's restatement and derived budget, and the validity of the forward fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics as nm
import numerics_eva as ne
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.attention import packed_qkv, qkv_form
from rajni_amd.wrapper.model import block_layer_scales, gated_mlp_form, mlp_norm_module

OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
IMAGES, LOGITS = PTR + 0x100, PTR + 0x200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rajni_hip_mlpnorm.h")).read()
SCHED = ne.SCHED


def _wrapped(name="vit_micro_eva_patch16_64", sched=SCHED, **kw):
    return rajni_amd.RAJNIViTWrapper(ts.create_model(name, seed=1, **kw), sched)


# ---- the record and the ABI ------------------------------------------------------------------------------------------------

def test_record_layout_matches_the_header():
    body = re.search(r"typedef struct \{(.*?)\} rajni_vit_mlp_norm;", HEADER, re.S).group(1)
    names = re.findall(r"(?:int|float|const float\* const\*)\s+(\w+);", body)
    assert names == [n for n, _ in nat.VitMlpNorm._fields_] == ["w", "b", "eps", "n"]
    assert C.sizeof(nat.VitMlpNorm) == 24 and [getattr(nat.VitMlpNorm, n).offset for n in names] == [0, 8, 16, 20]
    assert int(re.search(r"#define RAJNI_HIDDEN_NORM_MAX (\d+)", HEADER).group(1)) == nat.HIDDEN_NORM_MAX == ne.CAP >= 4096
    assert '#include "rajni_hip_rope.h"' in HEADER
    table = HEADER[HEADER.index("---- placement"):HEADER.index("(end of the placement table)")]
    rows = dict(re.findall(r"^ \*   (rajni_\w+): (.+)$", table, re.M))
    assert rows["rajni_hidden_norm"] == "x 16, w 16, b 16" and rows["rajni_vit_mlp_norm"] == "w 16, b 16"


def test_symbols_resolve_and_the_abi_stays_where_it_is():
    lib = nat.lib()
    assert nat.MLPNORM_SYMBOLS == ("rajni_hidden_norm", "rajni_vit_workspace_bytes_mlpnorm", "rajni_vit_forward_mlpnorm")
    for sym in nat.MLPNORM_SYMBOLS:
        assert getattr(lib, sym).argtypes is not None
    assert nat.ABI_VERSION == 8 and lib.rajni_abi_version() == 8 and nat.NUM_KCLASS == 17
    assert not set(nat.MLPNORM_SYMBOLS) & set(nat.EXPORTED_SYMBOLS + nat.ROPE_SYMBOLS + nat.NORM_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", main)
    sizes = {nat.VitExt: 72, nat.VitPrefix: 16, nat.VitImage: 8, nat.VitQuery: 8, nat.VitNorm: 24, nat.VitLayers: 40, nat.VitRope: 40}
    assert {k.__name__: C.sizeof(k) for k in sizes} == {k.__name__: v for k, v in sizes.items()}
    assert C.sizeof(nat.VitPlan) == 168 and C.sizeof(nat.Block) == 200 and C.sizeof(nat.LinearArgs) == 144


# ---- the forward's refusals, before any launch ---------------------------------------------------------------------------

def _plan(act_fp8=0, C_=128, hidden=384, H=2):
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, PTR)
        if act_fp8:
            blocks[i].qkv_s = blocks[i].proj_s = blocks[i].fc1_s = blocks[i].fc2_s = PTR
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = C_, H, 64, depth, hidden, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-5, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, PTR)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.act_fp8 = act_fp8
    return p, blocks


def _record(n=344, depth=4, b=True, hole=None, w_at=PTR):
    r = nat.VitMlpNorm()
    w = (C.c_void_p * depth)(*[None if i == hole else w_at + 0x1000 * i for i in range(depth)])
    bb = (C.c_void_p * depth)(*[PTR + 0x100000 + 0x1000 * i for i in range(depth)])
    r.w, r.eps, r.n = w, 1e-6, n
    if b:
        r.b = bb
    return r, (w, bb)


def _forward(p, rec, rope=None):
    lib = nat.lib()
    ref = lambda r: C.byref(r) if r is not None else None
    rc = lib.rajni_vit_forward_mlpnorm(C.byref(p), None, None, None, None, None, None, None, ref(rope), ref(rec), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _size(p, rec):
    return nat.lib().rajni_vit_workspace_bytes_mlpnorm(C.byref(p), None, None, None, None, None, None, C.byref(rec) if rec is not None else None)


def test_a_valid_plan_stops_at_the_workspace_and_the_record_adds_nothing():
    base = nat.lib().rajni_vit_workspace_bytes(C.byref(_plan()[0]))
    for kw in (dict(), dict(b=False), dict(n=384), dict(n=1)):
        p, keep = _plan()
        rec, arrays = _record(**kw)
        rc, msg = _forward(p, rec)
        assert rc == INVALID and "workspace too small" in msg, msg
        assert _size(p, rec) == base
    p, keep = _plan()
    assert _size(p, None) == _size(p, nat.VitMlpNorm()) == base
    # NULL and all zero are rajni_vit_forward_rope's call, by name too
    p.patch_size = 0
    for rec in (None, nat.VitMlpNorm()):
        rc, msg = _forward(p, rec)
        assert rc != OK and not msg.startswith("rajni_vit_forward_mlpnorm"), msg


def test_refused_records_name_themselves():
    who = "rajni_vit_forward_mlpnorm: "
    for n in (0, -3, 385, 4097):
        p, keep = _plan()
        rec, arrays = _record(n=n)
        rc, msg = _forward(p, rec)
        assert rc == INVALID and msg.startswith(who + "mlp_norm.n must be the MLP width, 1..plan.hidden = 384") and f"({n})" in msg, msg
        assert _size(p, rec) == 0 and "mlp_norm.n" in nat.lib().rajni_last_error().decode()
    # over the cap, on a plan wide enough to hold it
    p, keep = _plan(hidden=8192)
    rec, arrays = _record(n=4104)
    rc, msg = _forward(p, rec)
    assert rc == UNSUPPORTED and msg == who + "mlp_norm.n = 4104 is over rajni_hidden_norm's cap of 4096 columns", msg
    # a NULL w, a NULL w[i]
    p, keep = _plan()
    rec, arrays = _record()
    rec.w = None
    rc, msg = _forward(p, rec)
    assert rc == INVALID and msg == who + "null pointer (mlp_norm.w) with a non-zero mlp_norm record", msg
    rec, arrays = _record(hole=2)
    rc, msg = _forward(p, rec)
    assert rc == INVALID and msg == who + "null pointer (mlp_norm.w[2]) with a non-zero mlp_norm record", msg
    # placement
    rec, arrays = _record(w_at=PTR + 8)
    rc, msg = _forward(p, rec)
    assert rc == INVALID and "mlp_norm block 0" in msg and "w" in msg, msg
    # act_fp8
    p, keep = _plan(act_fp8=1, C_=512, hidden=2048, H=8)
    rec, arrays = _record(n=2048)
    rc, msg = _forward(p, rec)
    assert rc == UNSUPPORTED and msg.startswith(who + "a norm inside the MLP (an mlp_norm record) is unsupported with plan.act_fp8"), msg


def test_hidden_norm_refusals():
    lib = nat.lib()

    def call(kind=0, x=PTR, ld=384, w=PTR, b=PTR, rows=4, n=344, dtype=nat.RAJNI_BF16):
        rc = lib.rajni_hidden_norm(kind, x, ld, w, b, rows, n, 1e-6, dtype, 0, None)
        return rc, lib.rajni_last_error().decode()

    rc, msg = call(n=ne.CAP + 8, ld=ne.CAP + 64)
    assert rc == UNSUPPORTED and msg == f"rajni_hidden_norm: a width of {ne.CAP + 8} is over the cap of {ne.CAP} columns " \
                                       "(one wave holds the row in registers)", msg
    for kw, text in ((dict(kind=2), "kind must be"), (dict(n=0), "bad shape"), (dict(rows=0), "bad shape"),
                     (dict(ld=340), "ld must be at least n"), (dict(ld=388), "multiple of 8"), (dict(dtype=9), "bad dtype"),
                     (dict(x=None), "null pointer (x)"), (dict(w=None), "null pointer (w)")):
        rc, msg = call(**kw)
        assert rc != OK and text in msg, (kw, msg)
    for name in ("x", "w", "b"):
        rc, msg = call(**{name: PTR + 8})
        assert rc == INVALID and name in msg and "16" in msg, msg


# ---- timm_shaped ---------------------------------------------------------------------------------------------------------------

def test_configs():
    assert issubclass(ts.EvaViTConfig, ts.RopeViTConfig) and ts.ViTConfig().mlp_norm is False and ts.ViTConfig().eva_block is False
    want = {"eva02_tiny_patch14_224": (192, 12, 3, 512, "swiglu_packed", False),
            "eva02_small_patch14_224": (384, 12, 6, 1024, "swiglu_packed", False),
            "eva02_base_patch14_224": (768, 12, 12, 2048, "swiglu", True),
            "eva02_large_patch14_224": (1024, 24, 16, 2730, "swiglu", True)}
    for name, dims in want.items():
        c = ts.config_of(name)
        assert (c.embed_dim, c.depth, c.num_heads, c.hidden_dim, c.mlp, c.mlp_norm) == dims
        assert c.eva_block and c.rope == "axial" and c.patch_size == 14 and c.head_dim == 64
    assert [ts.config_of(n).hidden_dim for n in ne.MICRO] == [344, 342, 344, 344, 640]
    assert set(ne.MICRO) <= set(ts.EVA_CONFIGS) and ts.EVA_CONFIGS in ts.ALL_CONFIG_TABLES
    c = ts.config_of("vit_micro_eva_rms_gap_patch16_64")
    assert c.norm == "rms" and not c.class_token and ts.config_of("vit_micro_eva_h342_patch16_64").qkv_split
    c = ts.config_of("vit_micro_mlpnorm_patch16_64")
    assert c.mlp == "mlp" and c.rope == "none" and not c.eva_block and c.mlp_norm
    assert ts.config_of("vit_micro_eva_d40_patch14_56").head_dim == 40


def test_modules_have_eva_spellings_and_older_configs_keep_their_weights():
    m = ts.create_model("vit_micro_eva_patch16_64", seed=3)
    blk = m.blocks[0]
    assert not hasattr(blk, "ls1") and blk.gamma_1.shape == (128,) and blk.attn.qkv.bias is None and blk.attn.q_bias.shape == (128,)
    assert isinstance(blk.attn.norm, nn.Identity) and isinstance(blk.mlp.norm, nn.LayerNorm) and blk.mlp.norm.normalized_shape == (344,)
    m = ts.create_model("vit_micro_eva_h342_patch16_64", seed=3)
    a = m.blocks[0].attn
    assert a.qkv is None and a.k_proj.bias is None and a.q_proj.bias is not None and m.blocks[0].gamma_1 is None
    assert isinstance(ts.create_model("vit_micro_eva_rms_gap_patch16_64").blocks[1].mlp.norm, ts.RmsNorm)
    # the same draws under either spelling
    plain = ts.synth_state_dict(ts.RopeViTConfig(**ts._MICRO, mlp_ratio=2.6875, mlp="swiglu", rope="axial"), seed=5, bias_std=0.02)
    eva = ts.synth_state_dict(ts.EvaViTConfig(**ts._MICRO, mlp_ratio=2.6875, mlp="swiglu", rope="axial", eva_block=True, qkv_split=True),
                              seed=5, bias_std=0.02)
    w = plain["blocks.2.attn.qkv.weight"]
    assert np.array_equal(np.concatenate([eva[f"blocks.2.attn.{n}.weight"] for n in ("q_proj", "k_proj", "v_proj")]), w)
    assert np.array_equal(eva["blocks.2.attn.v_proj.bias"], plain["blocks.2.attn.qkv.bias"][256:])
    assert np.array_equal(eva["head.weight"], plain["head.weight"])


# ---- the wrapper: recognition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ne.MICRO + ["eva02_tiny_patch14_224"])
def test_eva_configs_are_accepted(name):
    cfg = ts.config_of(name)
    d = _wrapped(name).check_supported()
    assert d["mlp_norm"] == cfg.mlp_norm and d["hidden"] == cfg.hidden_dim and d["hidden_pad"] == (cfg.hidden_dim + 63) // 64 * 64
    assert d["norm_kind"] == cfg.norm and d["mlp_act"] == ("gelu" if cfg.mlp == "mlp" else "swiglu")
    if cfg.mlp_norm:
        assert d["mlp_norm_eps"] == cfg.ln_eps


def test_mlp_norm_recognition_and_refusals():
    w = _wrapped()
    assert gated_mlp_form(w.blocks[0].mlp) == "split" and isinstance(mlp_norm_module(w.blocks[0].mlp), nn.LayerNorm)
    assert mlp_norm_module(ts.Mlp(128, 256)) is None and mlp_norm_module(nn.Linear(4, 4)) is None
    packed = ts.GluMlp(128, 344)
    packed.norm = nn.LayerNorm(344)
    assert gated_mlp_form(packed) == "packed" and mlp_norm_module(packed) is packed.norm
    # None stays "no norm"
    w = _wrapped("vit_micro_swiglu_patch16_64")
    for blk in w.blocks:
        blk.mlp.norm = None
    assert w.check_supported()["mlp_norm"] is False
    # a norm in one block only
    w = _wrapped()
    w.blocks[2].mlp.norm = nn.Identity()
    with pytest.raises(NotImplementedError, match=r"block 2: SwiGLU: no mlp.norm where block 0 has one"):
        w.check_supported()
    # another kind than the model's, on a gated and on a plain MLP
    for name in ("vit_micro_eva_patch16_64", "vit_micro_mlpnorm_patch16_64"):
        w = _wrapped(name)
        w.blocks[1].mlp.norm = ts.RmsNorm(344)
        with pytest.raises(NotImplementedError, match=r"blocks.1.mlp.norm is rms but blocks.0.norm1 is layernorm: mixed norm kinds"):
            w.check_supported()
    w = _wrapped("vit_micro_eva_rms_gap_patch16_64")
    w.blocks[0].mlp.norm = nn.LayerNorm(344)
    with pytest.raises(NotImplementedError, match=r"blocks.0.mlp.norm is layernorm but blocks.0.norm1 is rms"):
        w.check_supported()
    # a norm over another width, something that is no norm, another eps
    w = _wrapped()
    w.blocks[3].mlp.norm = nn.LayerNorm(343)
    with pytest.raises(NotImplementedError, match=r"blocks.3.mlp.norm: LayerNorm must be affine .* over the 344 channels"):
        w.check_supported()
    w = _wrapped()
    w.blocks[3].mlp.norm = nn.Tanh()
    with pytest.raises(NotImplementedError, match=r"blocks.3.mlp.norm: .*Tanh computes neither"):
        w.check_supported()
    w = _wrapped()
    w.blocks[3].mlp.norm = nn.LayerNorm(344, eps=1e-5)
    with pytest.raises(NotImplementedError, match=r"blocks.3.mlp.norm has eps 1e-05"):
        w.check_supported()
    # wider than the kernel's cap
    big = ts.VisionTransformer(ts.EvaViTConfig(img_size=32, embed_dim=128, depth=1, num_heads=2, mlp_ratio=40.0, mlp_norm=True))
    with pytest.raises(NotImplementedError, match=r"mlp.norm over an MLP width of 5120.*up to 4096 columns"):
        rajni_amd.RAJNIViTWrapper(big, {}).check_supported()


def test_fp8_mfma_is_refused_at_the_setter_and_at_build_and_fp8_is_not():
    w = _wrapped("vit_micro_mlpnorm_patch16_64")
    with pytest.raises(NotImplementedError, match=r"norm inside the MLP \(mlp.norm\)"):
        w.set_weight_format("fp8_mfma")
    assert w.set_weight_format("fp8")._weight_format == "fp8"
    w = _wrapped("vit_micro512_patch16_64").set_weight_format("fp8_mfma")      # the norm attached after the setter
    for blk in w.blocks:
        blk.mlp.norm = nn.LayerNorm(2048, eps=1e-6)
    with pytest.raises(NotImplementedError, match=r'"fp8_mfma" on a model with a norm inside the MLP'):
        w.check_supported()


def test_layer_scale_spellings():
    w = _wrapped()
    g1, g2 = block_layer_scales(w.blocks[0], "block 0")
    assert g1 is w.blocks[0].gamma_1 and g2 is w.blocks[0].gamma_2
    assert block_layer_scales(_wrapped("vit_micro_eva_h342_patch16_64").blocks[0], "b") == (None, None)
    old = _wrapped("vit_micro_rope_half_reg4_patch16_64").blocks[1]
    assert block_layer_scales(old, "b")[0] is old.ls1.gamma
    assert block_layer_scales(_wrapped("vit_micro_patch16_64").blocks[1], "b") == (None, None)
    w.blocks[1].ls1 = ts.LayerScale(128, 0.1)
    with pytest.raises(NotImplementedError, match=r"block 1: both ls1 and gamma_1"):
        w.check_supported()
    w = _wrapped()
    w.blocks[1].gamma_2 = nn.Parameter(torch.ones(1, 128))
    with pytest.raises(NotImplementedError, match=r"block 1: gamma_2 must be a \[C\] parameter or None"):
        w.check_supported()


def test_qkv_spellings_and_the_packed_projection():
    torch.manual_seed(0)
    # cat(q_bias, 0, v_bias)
    a = _wrapped(bias_std=0.05).blocks[0].attn
    assert qkv_form(a) == "fused_qv_bias"
    wt, b = packed_qkv(a)
    assert wt.data_ptr() == a.qkv.weight.data_ptr()
    assert torch.equal(b, torch.cat([a.q_bias, torch.zeros(128), a.v_bias])) and float(a.q_bias.abs().max()) > 0
    # the scheduled block's RAJNIAttention keeps the spelling (block 1 is scheduled)
    wr = _wrapped(bias_std=0.05)
    assert type(wr.blocks[1].attn).__name__ == "RAJNIAttention" and qkv_form(wr.blocks[1].attn) == "fused_qv_bias"
    # q_proj / k_proj / v_proj: the three linears to the last bit
    wr = _wrapped("vit_micro_eva_h342_patch16_64", bias_std=0.05)
    for blk in wr.blocks:
        a = blk.attn
        assert qkv_form(a) == "split"
        wt, b = packed_qkv(a)
        assert wt.shape == (384, 128) and b.shape == (384,)
        x = torch.randn(7, 128)
        got = torch.stack([x @ wt[i * 128:(i + 1) * 128].T + b[i * 128:(i + 1) * 128] for i in range(3)])
        want = torch.stack([a.q_proj(x), a.k_proj(x), a.v_proj(x)])
        assert torch.equal(got, want)
        assert torch.equal(wt, torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]))
        assert torch.equal(b[128:256], torch.zeros(128)) and torch.equal(b[:128], a.q_proj.bias)
    a = ts.Attention(128, 2, bias=False, eva=True, qkv_split=True)
    assert packed_qkv(a)[1] is None
    assert qkv_form(ts.Attention(128, 2)) == "fused" and packed_qkv(ts.Attention(128, 2))[1] is not None
    # half-formed spellings
    a = _wrapped(bias_std=0.05).blocks[0].attn
    a.v_bias = None
    with pytest.raises(NotImplementedError, match=r"q_bias and attn.v_bias come together.*only q_bias"):
        qkv_form(a)
    w = _wrapped()
    w.blocks[2].attn.q_bias = None
    with pytest.raises(NotImplementedError, match=r"block 2: attn.q_bias and attn.v_bias come together.*only v_bias"):
        w.check_supported()
    w = _wrapped()
    w.blocks[0].attn.qkv.bias = nn.Parameter(torch.zeros(384))
    with pytest.raises(NotImplementedError, match=r"block 0: attn.q_bias / attn.v_bias must be \[128\] beside a bias-free attn.qkv"):
        w.check_supported()
    w = _wrapped("vit_micro_eva_h342_patch16_64")
    w.blocks[3].attn.k_proj = None
    with pytest.raises(NotImplementedError, match=r"block 3: attn.qkv is absent, so q_proj, k_proj and v_proj must be three nn.Linear"):
        w.check_supported()
    w = _wrapped("vit_micro_eva_h342_patch16_64")
    w.blocks[0].attn.qkv = nn.Linear(128, 384)
    with pytest.raises(NotImplementedError, match=r"block 0: attn.qkv together with q_proj"):
        w.check_supported()
    # Eva's inner attention norm
    for sched in (SCHED, {}):
        w = _wrapped(sched=sched)
        w.blocks[1].attn.norm = nn.LayerNorm(128)
        with pytest.raises(NotImplementedError, match=r"block 1: attn.norm \(LayerNorm\), a norm between attention and proj"):
            w.check_supported()


# ---- the restated forward ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ne.MICRO)
def test_restated_forward_is_the_modules_forward_when_nothing_is_pruned(name):
    cfg, sd, iseed, tables = ne.fixture(name)
    imgs = ne.images_of(cfg, 2, iseed)
    got, counts, trace = ne.vit_forward_restated(sd, imgs, {}, cfg, tables)
    with torch.no_grad():
        want = ne.build_model(name).double()(torch.from_numpy(imgs).double()).numpy()
    assert counts == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth and not trace
    # (the module rotates q and k in fp32 whatever its dtype - timm's apply_rot_embed_cat - so a rope model's "fp64" forward
    # carries one fp32 rounding per rotated element)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"[eva] {name}: restated vs the module's fp64 forward {err:.3g}")
    assert err <= (1e-5 if cfg.rope != "none" else 1e-9)


# ---- the kernel's restatement and its budget -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["layernorm", "rms"])
@pytest.mark.parametrize("n", [8, 342, 344, 2730])
def test_the_emulated_kernel_meets_the_derived_budget_and_the_mutants_do_not(n, kind):
    ld = (n + 63) // 64 * 64
    for dt in ("bf16", "fp32"):
        x, names, w, b = ne.kernel_rows(10, n, ld, dt, seed=1)
        want, bud = ne.hidden_norm_budget(x, w, b, 1e-6, n, kind, "fp32")
        got = ne.emul_hidden_norm(x, w, b, 1e-6, n, kind)
        assert np.all(got[:, n:] == 0) and np.all(want[:, n:] == 0) and np.all(bud[:, n:] == 0)
        assert ne.worst(got, want, bud, n) <= 1.0, (dt, ne.worst(got, want, bud, n))
        if ld != n and n > 8:
            other = ne.emul_hidden_norm(x, w, b, 1e-6, n, kind, mutant="divisor_ld")
            assert ne.worst(other, want, bud, n) > 1.0
    if kind == "layernorm":      # what the two passes are for: the fp32 row of mean 1000 and spread 0.05
        x, names, w, b = ne.kernel_rows(10, n, ld, "fp32", seed=1)
        rows = names == "big_mean"
        want, bud = ne.hidden_norm_budget(x[rows], w, b, 1e-6, n, kind, "fp32")
        assert ne.worst(ne.emul_hidden_norm(x[rows], w, b, 1e-6, n, kind), want, bud, n) <= 1.0
        if n > 8:
            assert ne.worst(ne.emul_hidden_norm(x[rows], w, b, 1e-6, n, kind, mutant="one_pass"), want, bud, n) > 1.0
        # a row of one repeated value: zero variance, eps alone under the root, b comes out
        x = np.zeros((1, ld), np.float32)
        x[:, :n] = 3.25
        assert np.array_equal(ne.emul_hidden_norm(x, w, b, 1e-6, n, kind)[0, :n], b)


def test_chain_length():
    assert [ne.chain_length(n) for n in (8, 512, 513, 2730, 4096)] == [14, 14, 22, 54, 70]


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------

def _cases(name):
    return ne.CASES + ne.EXTRA.get(name, [])


@pytest.mark.parametrize("name", ne.MICRO)
def test_fixture_seeds_hold_their_conditions(name):
    assert ne.MAX_SKIPPED == 0 and set(ne.SEEDS) == set(ne.MICRO)
    wseed, iseed = ne.SEEDS[name]
    assert iseed == wseed + 4 and wseed >= 1
    cfg, sd = ne.fixture(name)[:2]
    assert max(ne.format_cost(name, wseed, B) for B in (1, ne.BATCH)) <= ne.FORMAT_HEADROOM * ne.BAR["bf16"]
    for earlier in range(1, min(wseed, 4)):      # (the search's order, spot-checked on the first seeds)
        assert not ne.holds(name, earlier)
    live = 0
    for sched, size in _cases(name):
        assert ne.boundary_gap_ratios(name, sched, size) >= ne.GAP_FACTOR, (sched, size)
        for mut, sep in ne.mutant_separations(name, sched, size).items():
            if ne.vacuous(cfg, sd, mut):
                continue
            live += 1
            assert sep >= ne.mutant_bar(mut), (mut, sched, size, sep)
    assert live >= 4 * len(_cases(name))
    assert ne.mutant_bar("no_mlp_norm") == 4e-2 and ne.mutant_bar("k_bias_nonzero") == ne.mutant_bar("divisor_ld") == 4e-3


def test_every_mutant_is_live_on_some_fixture():
    live = {m for name in ne.MICRO for m in ne.MUTANTS if not ne.vacuous(*ne.fixture(name)[:2], m)}
    assert live == set(ne.MUTANTS)
