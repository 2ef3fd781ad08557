"""RMSNorm trunks and the patch-embedding norm (include/rajni_hip_norm.h; the AIMv2 ViTs) without a GPU: the record's layout
against the header and the ABI the feature must not move, the forward's refusals (before any launch: every plan here has
workspace = NULL and fake addresses nobody follows, the pattern of tests/test_activations_cpu.py), the wrapper's recognition of a
norm by what it computes, the synthetic weights, the RMSNorm error budget with its measured constant and three mutants, and the
validity of the forward fixtures (an RMS graph and the same graph with LayerNorm substituted, an embedding norm present and
absent, must differ by 10 x the GPU tests' bar)."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics as nm
import numerics_rmsnorm as nr
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import classify_norm

OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
IMAGES, LOGITS = PTR + 0x100, PTR + 0x200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rajni_hip_norm.h")).read()


# ---- the record and the ABI ------------------------------------------------------------------------------------------------

def test_record_layout_matches_the_header():
    body = re.search(r"typedef struct \{(.*?)\} rajni_vit_norm;", HEADER, re.S).group(1)
    names = re.findall(r"(?:int|float|const float\*)\s+(\w+);", body)
    assert names == [n for n, _ in nat.VitNorm._fields_] == ["kind", "embed_norm_eps", "embed_norm_w", "embed_norm_b"]
    assert C.sizeof(nat.VitNorm) == 24
    assert [getattr(nat.VitNorm, n).offset for n in names] == [0, 4, 8, 16]
    assert re.search(r"RAJNI_NORM_LAYERNORM\s*=\s*0\s*,\s*RAJNI_NORM_RMS\s*=\s*1\b", HEADER)
    assert (nat.NORM_LAYERNORM, nat.NORM_RMS) == (0, 1)
    assert '#include "rajni_hip_attnpool.h"' in HEADER and "(end of the placement table)" in HEADER
    table = HEADER[HEADER.index("---- placement"):HEADER.index("(end of the placement table)")]
    rows = dict(re.findall(r"^ \*   (rajni_\w+): (.+)$", table, re.M))
    assert rows["rajni_norm_rows"] == "x 16, w 16, b 16, y 16" and rows["rajni_embed_norm"] == "x 16, w 16, b 16, pos 16"
    assert "unverified against an installed timm" in HEADER


def test_symbols_resolve_and_the_abi_stays_where_it_is():
    lib = nat.lib()
    assert nat.NORM_SYMBOLS == ("rajni_norm_rows", "rajni_embed_norm", "rajni_vit_workspace_bytes_norm", "rajni_vit_forward_norm")
    for sym in nat.NORM_SYMBOLS:
        assert getattr(lib, sym).argtypes is not None
    assert nat.ABI_VERSION == 8 and lib.rajni_abi_version() == 8 and nat.NUM_KCLASS == 17
    assert not set(nat.NORM_SYMBOLS) & set(nat.EXPORTED_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "rajni_hip.h")).read() + open(os.path.join(ROOT, "include", "rajni_hip_debug.h")).read()
    declared = set(re.findall(r"\b(rajni_\w+)\s*\(", main))
    assert set(nat.EXPORTED_SYMBOLS) <= declared and not set(nat.NORM_SYMBOLS) & declared
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", main)


# ---- the forward's refusals, before any launch ---------------------------------------------------------------------------

def _plan(act_fp8=0, C_=128, hidden=512, H=2, null_b=True):
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, PTR)
        if null_b:
            blocks[i].norm1_b = blocks[i].norm2_b = None
        if act_fp8:
            blocks[i].qkv_s = blocks[i].proj_s = blocks[i].fc1_s = blocks[i].fc2_s = PTR
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = C_, H, 64, depth, hidden, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-5, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, PTR)
    if null_b:
        p.norm_b = None
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.act_fp8 = act_fp8
    return p, blocks


def _forward(p, nrm, ext=None, lay=None, pool=None):
    lib = nat.lib()
    ref = lambda r: C.byref(r) if r is not None else None
    rc = lib.rajni_vit_forward_norm(C.byref(p), ref(ext), None, ref(lay), None, None, ref(pool), ref(nrm), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _norm(kind=nat.NORM_RMS, embed=False):
    n = nat.VitNorm()
    n.kind = kind
    if embed:
        n.embed_norm_w, n.embed_norm_eps = PTR, 1e-5
    return n


def test_a_valid_rms_plan_with_null_biases_stops_at_the_workspace():
    # the control: every check passes with every *_b norm pointer NULL, and nothing was launched on the way
    for embed in (False, True):
        p, keep = _plan()
        ext = nat.VitExt()
        ext.norm_pre_w, ext.fc_norm_w, ext.pool = PTR, PTR, nat.POOL_AVG      # norm_pre_b and fc_norm_b stay NULL
        rc, msg = _forward(p, _norm(embed=embed), ext)
        assert rc == INVALID and "workspace too small" in msg, msg
        assert nat.lib().rajni_vit_workspace_bytes_norm(C.byref(p), None, None, None, None, C.byref(_norm(embed=embed))) == \
            nat.lib().rajni_vit_workspace_bytes(C.byref(p)) > 0
    # the same plan as a LayerNorm plan misses its bias vectors
    p, keep = _plan()
    rc, msg = _forward(p, None)
    assert rc == INVALID and "null weight pointer" in msg, msg
    # ... and a LayerNorm plan with an embedding norm (its bias NULL = 0) is served
    p, keep = _plan(null_b=False)
    rc, msg = _forward(p, _norm(nat.NORM_LAYERNORM, embed=True))
    assert rc == INVALID and "workspace too small" in msg, msg


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_an_unknown_kind_is_invalid(bad):
    p, keep = _plan()
    rc, msg = _forward(p, _norm(bad))
    assert rc == INVALID and msg == f"rajni_vit_forward_norm: norm.kind must be RAJNI_NORM_LAYERNORM or RAJNI_NORM_RMS ({bad})", msg
    assert nat.lib().rajni_vit_workspace_bytes_norm(C.byref(p), None, None, None, None, C.byref(_norm(bad))) == 0
    assert "norm.kind" in nat.lib().rajni_last_error().decode()
    lib = nat.lib()
    assert lib.rajni_norm_rows(bad, PTR, 128, PTR, None, PTR, 4, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert "kind" in lib.rajni_last_error().decode()
    assert lib.rajni_embed_norm(bad, PTR, PTR, None, PTR, 0, 1, 4, 0, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert "kind" in lib.rajni_last_error().decode()


def test_refused_combinations_name_themselves():
    big = dict(act_fp8=1, C_=512, hidden=2048, H=8)
    # RMS with act_fp8, an embedding norm with act_fp8
    p, keep = _plan(**big)
    rc, msg = _forward(p, _norm())
    assert rc == UNSUPPORTED and "RMSNorm" in msg and "act_fp8" in msg, msg
    p, keep = _plan(null_b=False, **big)
    rc, msg = _forward(p, _norm(nat.NORM_LAYERNORM, embed=True))
    assert rc == UNSUPPORTED and "patch-embedding norm" in msg and "act_fp8" in msg, msg
    p, keep = _plan(null_b=False, **big)          # (the control: the same plan without the record is served)
    rc, msg = _forward(p, None)
    assert rc == INVALID and "workspace too small" in msg, msg
    # RMS with a pool record
    p, keep = _plan()
    ext = nat.VitExt()
    ext.pool = nat.POOL_MAP
    pool = nat.VitAttnPool()
    for name in ("q", "kv_w", "kv_b", "proj_w", "proj_b", "norm_w", "norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
        setattr(pool, name, PTR)
    pool.hidden, pool.heads, pool.norm_eps = 512, 2, 1e-5
    rc, msg = _forward(p, _norm(), ext, pool=pool)
    assert rc == UNSUPPORTED and "RMSNorm" in msg and "attention-pool" in msg, msg
    # RMS with layers.norm = 1; norm = 0 is served
    for lnorm, want in ((1, UNSUPPORTED), (0, INVALID)):
        p, keep = _plan()
        p.num_classes, p.head_w, p.head_b = 0, None, None
        lay = nat.VitLayers()
        caps = (C.c_int * 2)(1, 3)
        lay.n, lay.blocks, lay.norm, lay.fill, lay.out = 2, caps, lnorm, 0, PTR
        rc, msg = _forward(p, _norm(), lay=lay)
        assert rc == want, msg
        assert ("layers.norm = 1" in msg and "RMSNorm" in msg) if lnorm else "workspace too small" in msg, msg
    # placement of the record's own pointers
    p, keep = _plan()
    n = _norm(embed=True)
    n.embed_norm_w = PTR + 4
    rc, msg = _forward(p, n)
    assert rc == INVALID and "embed_norm_w must be 16-byte aligned" in msg, msg


def test_row_entry_points_refuse_before_any_launch():
    lib = nat.lib()
    # C beyond one wave's registers, C not a multiple of 8, and a NULL b under LAYERNORM
    assert lib.rajni_norm_rows(nat.NORM_RMS, PTR, 4096, PTR, None, PTR, 4, 4096, 1e-5, nat.RAJNI_BF16, 0, None) == UNSUPPORTED
    assert "C <= 2048" in lib.rajni_last_error().decode()
    assert lib.rajni_norm_rows(nat.NORM_LAYERNORM, PTR, 128, PTR, None, PTR, 4, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert "null pointer" in lib.rajni_last_error().decode()
    assert lib.rajni_norm_rows(nat.NORM_RMS, PTR + 2, 128, PTR, None, PTR, 4, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert "x must be 16-byte aligned" in lib.rajni_last_error().decode()
    assert lib.rajni_embed_norm(nat.NORM_RMS, PTR, PTR, None, PTR, 0, 2, 17, 1, 132, 1e-5, nat.RAJNI_BF16, 0, None) == UNSUPPORTED
    assert lib.rajni_embed_norm(nat.NORM_RMS, PTR, PTR, None, PTR, 0, 2, 5, 5, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert lib.rajni_embed_norm(nat.NORM_RMS, PTR, PTR, None, PTR + 8, 0, 2, 17, 1, 128, 1e-5, nat.RAJNI_BF16, 0, None) == INVALID
    assert "pos must be 16-byte aligned" in lib.rajni_last_error().decode()


# ---- the wrapper recognises a norm by what it computes --------------------------------------------------------------------

class RMSNorm(nn.Module):                   # the name, computing something else: the mean is subtracted
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        x = x - x.mean(-1, keepdim=True)
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


class ScaleNorm(nn.Module):                 # another name, computing RMSNorm
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


def test_classify_norm():
    dim = 128
    assert classify_norm(nn.LayerNorm(dim), dim) == "layernorm"
    assert classify_norm(ts.RmsNorm(dim, eps=1e-5), dim) == "rms"
    assert classify_norm(ScaleNorm(dim), dim) == "rms"
    assert classify_norm(nn.RMSNorm(dim, eps=1e-6), dim) == "rms"
    assert classify_norm(ts.RmsNorm(dim).to(torch.bfloat16), dim) == "rms"       # probed on an fp32 copy
    m = ts.RmsNorm(dim)
    with torch.no_grad():
        m.weight.copy_(1 + 0.1 * torch.randn(dim))
    assert classify_norm(m, dim) == "rms"
    with pytest.raises(NotImplementedError, match="RMSNorm computes neither"):
        classify_norm(RMSNorm(dim), dim)
    with pytest.raises(NotImplementedError, match="eps=None"):
        classify_norm(nn.RMSNorm(dim), dim)
    with pytest.raises(NotImplementedError, match="affine"):
        classify_norm(nn.LayerNorm(dim, elementwise_affine=False), dim)
    with pytest.raises(NotImplementedError, match="affine"):
        classify_norm(nn.LayerNorm(64), dim)
    with pytest.raises(NotImplementedError, match="GELU computes neither"):
        classify_norm(nn.GELU(), dim)
    with pytest.raises(NotImplementedError, match="RmsNorm computes neither"):
        classify_norm(ts.RmsNorm(64), dim)


def _wrap(name, **kw):
    return rajni_amd.RAJNIViTWrapper(ts.create_model(name, std=0.08, bias_std=0.02, **kw), nr.SCHED)


def test_describe_reports_the_kind_and_the_record():
    for name, kind, embed in (("vit_micro_rms_patch16_64", "rms", False), ("vit_micro_aimv2_patch16_64", "rms", True),
                              ("vit_micro_aimv2_d128_patch14_56", "rms", True),
                              ("vit_micro_reg4_embednorm_patch16_64", "layernorm", True), ("vit_micro_patch16_64", "layernorm", False)):
        d = _wrap(name).check_supported()
        assert (d["norm_kind"], d["embed_norm"], d["norm_record"]) == (kind, embed, kind == "rms" or embed), name
    d = _wrap("vit_micro_aimv2_patch16_64").check_supported()
    assert d["mlp_act"] == "swiglu" and not d["class_token"] and d["headless"] and d["pool"] == "avg" and not d["fc_norm"]
    assert d["ln_eps"] == d["embed_norm_eps"] == 1e-5


def test_wrapper_refusals_name_the_module():
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.blocks[2].norm2 = nn.LayerNorm(128, eps=1e-6)
    with pytest.raises(NotImplementedError, match=r"blocks\.2\.norm2 is layernorm but blocks\.0\.norm1 is rms"):
        w.check_supported()
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.norm = nn.LayerNorm(128, eps=1e-6)
    with pytest.raises(NotImplementedError, match=r"RAJNIViTWrapper: norm is layernorm but"):
        w.check_supported()
    w = _wrap("vit_micro_patch16_64")
    w.m.patch_embed.norm = ts.RmsNorm(128)
    with pytest.raises(NotImplementedError, match=r"patch_embed\.norm is rms but blocks\.0\.norm1 is layernorm"):
        w.check_supported()
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.blocks[1].norm1 = ts.RmsNorm(128, eps=1e-5)
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.norm1 has eps 1e-05 but blocks\.0\.norm1 has 1e-06"):
        w.check_supported()
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.norm = ts.RmsNorm(128, eps=1e-5)
    with pytest.raises(NotImplementedError, match=r"base_model\.norm has eps 1e-05"):
        w.check_supported()
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.blocks[3].norm1 = RMSNorm(128, eps=1e-6)
    with pytest.raises(NotImplementedError, match=r"blocks\.3\.norm1: .*RMSNorm computes neither"):
        w.check_supported()
    w = _wrap("vit_micro_rms_patch16_64")
    w.m.blocks[0].norm1 = nn.RMSNorm(128)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.norm1: RMSNorm has eps=None"):
        w.check_supported()


def test_aimv2_3b_is_refused_with_the_cap():
    cfg = dataclasses.replace(ts.NORM_CONFIGS["aimv2_3b_patch14_224"], depth=1)
    assert cfg.embed_dim == 3072
    w = rajni_amd.RAJNIViTWrapper(ts.VisionTransformer(cfg), {})
    with pytest.raises(NotImplementedError, match=r"embed dim of 3072.*C <= 2048"):
        w.check_supported()
    for name in ("aimv2_large_patch14_224", "aimv2_huge_patch14_224", "aimv2_1b_patch14_224"):
        c = dataclasses.replace(ts.NORM_CONFIGS[name], depth=1)
        d = rajni_amd.RAJNIViTWrapper(ts.VisionTransformer(c), {}).check_supported()
        assert d["norm_kind"] == "rms" and d["embed_norm"] and d["D"] == 128 and d["patch"] == 14 and d["hidden"] % 64 == 0


def test_unsupported_options_name_the_feature():
    w = _wrap("vit_micro_rms_patch16_64")
    with pytest.raises(NotImplementedError, match="RMSNorm"):
        w.set_weight_format("fp8_mfma")
    w = _wrap("vit_micro_reg4_embednorm_patch16_64")
    with pytest.raises(NotImplementedError, match=r"patch_embed\.norm"):
        w.set_weight_format("fp8_mfma")
    assert _wrap("vit_micro_rms_patch16_64").set_weight_format("fp8") is not None
    # a 'map' head
    cfg = ts.NormViTConfig(img_size=64, embed_dim=128, depth=2, num_heads=2, num_classes=10, global_pool="map", class_token=False,
                           norm="rms")
    m = ts.VisionTransformer(cfg)
    m.attn_pool.norm = nn.LayerNorm(128)          # (the pool's own norm is held to LayerNorm by attn_pool_module)
    with pytest.raises(NotImplementedError, match=r"global_pool='map' on a model with RMSNorm"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # q/k-norm stays LayerNorm only
    cfg = ts.NormViTConfig(img_size=64, embed_dim=128, depth=2, num_heads=2, num_classes=10, qk_norm=True, norm="rms")
    m = ts.VisionTransformer(cfg)
    assert isinstance(m.blocks[0].attn.q_norm, nn.LayerNorm) and rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["qk_norm"]
    m.blocks[0].attn.q_norm = ts.RmsNorm(64)
    with pytest.raises(NotImplementedError):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()


# ---- timm_shaped -----------------------------------------------------------------------------------------------------------

def test_configs_and_synthetic_weights():
    assert len(dataclasses.fields(ts.ViTConfig)) == 20          # (what existing tests count)
    fields = [f.name for f in dataclasses.fields(ts.NormViTConfig)]
    assert fields[-3:] == ["norm", "embed_norm", "bias"] and fields[:20] == [f.name for f in dataclasses.fields(ts.ViTConfig)]
    c = ts.ViTConfig()
    assert (c.norm, c.embed_norm, c.bias) == ("layernorm", False, True)
    with pytest.raises(ValueError, match="norm"):
        ts.NormViTConfig(norm="batch")
    assert list(ts.NORM_CONFIGS) == ["aimv2_large_patch14_224", "aimv2_huge_patch14_224", "aimv2_1b_patch14_224",
                                     "aimv2_3b_patch14_224"] + nr.MICRO
    assert not set(ts.NORM_CONFIGS) & (set(ts.CONFIGS) | set(ts.SWIGLU_CONFIGS) | set(ts.NOCLASS_CONFIGS) | set(ts.MAP_CONFIGS))
    for name, (C_, H, hid) in {"aimv2_large_patch14_224": (1024, 8, 2816), "aimv2_huge_patch14_224": (1536, 12, 4096),
                               "aimv2_1b_patch14_224": (2048, 16, 5632)}.items():
        c = ts.config_of(name)
        assert (c.embed_dim, c.num_heads, c.hidden_dim, c.depth, c.patch_size, c.ln_eps) == (C_, H, hid, 24, 14, 1e-5)
        assert (c.mlp, c.class_token, c.global_pool, c.use_fc_norm, c.num_classes, c.norm, c.embed_norm, c.bias) == \
            ("swiglu", False, "avg", False, 0, "rms", True, False)
    # a config that says what ViTConfig's defaults say draws the stream it always drew
    for name in ("vit_micro_patch16_64", "vit_micro_swiglu_split_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64"):
        base = ts.config_of(name)
        twin = ts.NormViTConfig(**base.to_dict())
        a, b = ts.synth_state_dict(base, seed=3, std=0.08, bias_std=0.02), ts.synth_state_dict(twin, seed=3, std=0.08, bias_std=0.02)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # the RMS model has no norm bias, the bias-free model no linear bias, the headless model no head
    sd = ts.synth_state_dict(ts.config_of("vit_micro_aimv2_patch16_64"), seed=1, std=0.08, bias_std=0.02)
    assert not [k for k in sd if k.endswith(".bias") and k != "patch_embed.proj.bias"] and "head.weight" not in sd
    assert "patch_embed.norm.weight" in sd and list(sd)[-1] == "patch_embed.norm.weight"
    m = ts.create_model("vit_micro_aimv2_patch16_64", seed=1)
    assert isinstance(m.head, nn.Identity) and isinstance(m.patch_embed.norm, ts.RmsNorm) and m.blocks[0].attn.qkv.bias is None
    sd = ts.synth_state_dict(ts.config_of("vit_micro_reg4_embednorm_patch16_64"), seed=1)
    assert list(sd)[-2:] == ["patch_embed.norm.weight", "patch_embed.norm.bias"]
    # the module against the formula
    x = torch.randn(5, 128) + 0.7
    r = ts.RmsNorm(128, eps=1e-5)
    _, want = nr.rms64(x.numpy(), r.weight.detach().numpy(), 1e-5)
    assert np.abs(r(x).detach().numpy() - want).max() <= 1e-6


@pytest.mark.parametrize("name", nr.MICRO)
def test_restatement_is_the_stock_forward_on_the_empty_schedule(name):
    cfg, sd, iseed = nr.fixture(name)
    imgs = nr.images_of(cfg, 2, iseed)
    with torch.no_grad():
        stock = nr.build_model(name)(torch.from_numpy(imgs)).numpy()
    want, counts, tr = nr.vit_forward_restated(sd, imgs, {}, cfg)
    assert not tr and counts == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth
    assert np.abs(want - stock).max() <= 1e-4 * np.abs(want).max()


# ---- the budget ------------------------------------------------------------------------------------------------------------

def test_c_rms_is_three_times_the_references():
    """c_rms re-measured on both references over every (rows, C, input type) of the GPU test and held against the values
    recorded in numerics_rmsnorm.py"""
    need = {"torch_cpu_fp32": 0.0, "butterfly64": 0.0}
    for rows, C_, in_dt in [(r, c, d) for r in nm.LN_ROW_COUNTS for c in nr.RMS_C for d in ("bf16", "fp16", "fp32")]:
        x, names, w, b = nm.layernorm_rows(rows, C_, in_dt)
        need["torch_cpu_fp32"] = max(need["torch_cpu_fp32"], nr.rmsnorm_needed_c(nr.rms_torch(x, w), x, w, nr.EPS))
        need["butterfly64"] = max(need["butterfly64"], nr.rmsnorm_needed_c(nr.emul_rmsnorm(x, w), x, w, nr.EPS))
    print("[rmsnorm] measured c_rms:", need)
    for k, v in need.items():
        assert v <= nr.C_RMS_MEASURED[k] * 1.005, (k, v)
        assert v >= nr.C_RMS_MEASURED[k] * 0.5, f"{k}: recorded value {nr.C_RMS_MEASURED[k]} is stale (now {v:.3g})"
    assert nr.C_RMS == math.ceil(3 * max(nr.C_RMS_MEASURED.values())) and 3 * max(need.values()) <= nr.C_RMS


@pytest.mark.parametrize("out_dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("C_", [192, 2048])
def test_budget_holds_for_the_references_and_rejects_the_mutants(C_, out_dt):
    in_dt = out_dt
    x, names, w, b = nm.layernorm_rows(77, C_, in_dt)
    want, bud = nr.rmsnorm_budget(x, w, nr.EPS, out_dt)
    nm.assert_within(nm.round_to(nr.emul_rmsnorm(x, w), out_dt), want, bud, f"butterfly C={C_} {out_dt}")
    nm.assert_within(nm.round_to(nr.rms_torch(x, w), out_dt), want, bud, f"torch fp32 C={C_} {out_dt}")
    for mutant in nr.MUTANTS:
        ratio, i = nm.worst_ratio(nm.round_to(nr.emul_rmsnorm(x, w, mutant=mutant), out_dt), want, bud)
        assert ratio > 1.0, (mutant, ratio)


# ---- the fixtures tell the kinds apart ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", nr.MICRO)
def test_fixtures_separate_the_kinds_and_the_embedding_norm(name):
    cfg, sd, iseed = nr.fixture(name)
    bar = nr.SEPARATION * max(nr.BAR.values())
    if cfg.norm == "rms":
        d = nr.separation(name, norm="layernorm")
        print(f"[rmsnorm] {name}: LayerNorm (b = 0) substituted moves the output by {d:.3g} x max|out|")
        assert d >= bar, (name, d)
    if cfg.embed_norm:
        d = nr.separation(name, embed_norm=False)
        print(f"[rmsnorm] {name}: without the embedding norm the output moves by {d:.3g} x max|out|")
        assert d >= bar, (name, d)
    assert cfg.norm == "rms" or cfg.embed_norm


@pytest.mark.parametrize("name", nr.MICRO)
def test_fixture_seeds_leave_no_near_tie(name):
    cfg, sd, iseed = nr.fixture(name)
    gap = nr.boundary_gap_ratios(sd, nr.images_of(cfg, 3, iseed), nr.SCHED, cfg)
    print(f"[rmsnorm] {name}: smallest boundary gap {gap:.3g} x the bf16 score budget")
    assert gap >= nr.GAP_FACTOR
    cost = [nr.format_cost(cfg, nr.SEEDS[name][0], iseed, B) for B in (1, 3)]
    print(f"[rmsnorm] {name}: torch's bf16 forward is {cost[0]:.3g} / {cost[1]:.3g} x max|out| off its fp32 one (B = 1 / 3)")
    assert max(cost) <= nr.FORMAT_HEADROOM * nr.BAR["bf16"]
    assert nr.SEEDS[name] == nr.search_seeds(name)
