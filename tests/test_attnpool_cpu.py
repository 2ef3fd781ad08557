"""Attention-pool heads (timm `global_pool='map'`; include/rajni_hip_attnpool.h) without a GPU: the timm-shaped module against
the restated contract, the synthetic weight streams of every existing config, the wrapper's classification of such models and
every refusal (the wrapper's and the C ABI's - those come before any launch, so they run without a device), the new symbols,
and the seeds of the GPU forward tests."""
import ctypes as C
import dataclasses
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics as nm
import numerics_attnpool as na
import numerics_noclass as nq
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import attn_pool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTNPOOL_SYMBOLS = ("rajni_attention_pool", "rajni_vit_workspace_bytes_pool", "rajni_vit_forward_pool")
# sha256 (16 hex digits) over names and bytes of synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02) in draw order
# (tests/test_swiglu_cpu.py's digest), computed on the parent commit - before 'map' existed - for the two tables that file does
# not hold; the CONFIGS table is checked against that file's own list
PARENT = {
    "vit_giant_patch14_dinov2": "0d03eb4e71135afc",
    "vit_giant_patch14_reg4_dinov2": "679e06c72a109c71",
    "vit_micro_swiglu_patch16_64": "79eba5b0a89ef1ee",
    "vit_micro_swiglu_split_patch16_64": "0228edd067516e55",
    "vit_micro_swiglu_h344_patch16_64": "84ee350dad70e0aa",
    "vit_micro512_swiglu_patch16_64": "7c31f405e44127e2",
    "vit_micro_reg4_swiglu_patch14_56": "90a5fb66b2278b20",
    "vit_micro_nocls_gap_patch16_64": "2380ec2909e246d4",
    "vit_micro_reg4_nocls_gap_patch16_64": "9bd0d71492b841a8",
    "vit_micro_reg1_nocls_gap_d80_patch16_64": "0564f0d6ad3515dc",
    "vit_medium_patch16_gap_256": "fd4563fd3c000b40",
    "vit_betwixt_patch16_reg4_gap_256": "9cfff941269d2102",
}


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def _err(lib):
    return lib.rajni_last_error().decode()


# ---- the module --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", na.MICRO[:3] + ["vit_micro512_map_patch16_64"])
def test_the_module_is_the_restated_contract(name):
    """AttentionPoolLatent (scaled_dot_product_attention inside) against numerics_attnpool.attn_pool_restated (einsum, exp,
    erf), both fp64 on the same weights: two evaluations of one function, 1e-12 of the output's scale"""
    cfg = ts.config_of(name)
    model = ts.create_model(cfg, seed=5, **na.FIX_BASE).double()
    sd = ts.state_dict_numpy(ts.create_model(cfg, seed=5, **na.FIX_BASE))
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((3, 21, cfg.embed_dim))).double()
    with torch.no_grad():
        got = model.attn_pool(x).numpy()
    want = na.attn_pool_restated(sd, x, cfg).numpy()
    assert got.shape == (3, cfg.embed_dim) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # and the kernel's restatement is the same attention: kv and the pre-scaled query by hand
    W = lambda n: torch.from_numpy(sd["attn_pool." + n]).double()
    kv = (x @ W("kv.weight").T + W("kv.bias")).numpy()
    q = ((W("latent").reshape(1, -1) @ W("q.weight").T + W("q.bias")) * cfg.head_dim ** -0.5).reshape(cfg.num_heads, cfg.head_dim).numpy()
    o, _, _ = na.pool_attention(kv, q)
    ap, H, D = model.attn_pool, cfg.num_heads, cfg.head_dim
    with torch.no_grad():
        qm = ap.q(ap.latent.expand(3, -1, -1)).reshape(3, 1, H, D).transpose(1, 2)
        km, vm = ap.kv(x).reshape(3, 21, 2, H, D).permute(2, 0, 3, 1, 4).unbind(0)
        om = torch.nn.functional.scaled_dot_product_attention(qm, km, vm).transpose(1, 2).reshape(3, cfg.embed_dim).numpy()
    assert np.abs(o - om).max() <= 1e-12 * np.abs(om).max()


def test_the_module_has_the_contract_s_attributes():
    m = ts.create_model("vit_micro_map_patch16_64")
    ap = m.attn_pool
    assert tuple(ap.latent.shape) == (1, 1, 128) and ap.latent_len == 1 and ap.pos_embed is None and ap.pool == "token"
    assert ap.num_heads == 2 and ap.scale == 64 ** -0.5
    assert tuple(ap.q.weight.shape) == (128, 128) and tuple(ap.kv.weight.shape) == (256, 128) and tuple(ap.proj.weight.shape) == (128, 128)
    assert isinstance(ap.q_norm, nn.Identity) and isinstance(ap.k_norm, nn.Identity) and isinstance(ap.norm, nn.LayerNorm)
    assert isinstance(ap.mlp, ts.Mlp) and ap.mlp.fc1.out_features == 512
    assert isinstance(m.norm, nn.LayerNorm) and isinstance(m.fc_norm, nn.Identity) and m.cls_token is None
    assert ts.create_model("vit_micro_patch16_64").attn_pool is None
    keys = [k for k in m.state_dict() if k.startswith("attn_pool.")]
    assert keys == ["attn_pool.latent", "attn_pool.q.weight", "attn_pool.q.bias", "attn_pool.kv.weight", "attn_pool.kv.bias",
                    "attn_pool.proj.weight", "attn_pool.proj.bias", "attn_pool.norm.weight", "attn_pool.norm.bias",
                    "attn_pool.mlp.fc1.weight", "attn_pool.mlp.fc1.bias", "attn_pool.mlp.fc2.weight", "attn_pool.mlp.fc2.bias"]


def test_vitconfig_accepts_map_without_a_new_field():
    fields = [f.name for f in dataclasses.fields(ts.ViTConfig)]
    assert fields[-5:] == ["class_token", "mlp", "distilled", "act", "reg_tokens"] and len(fields) == 20
    assert not ts.ViTConfig(global_pool="map").use_fc_norm and ts.ViTConfig(global_pool="avg").use_fc_norm
    assert ts.ViTConfig(global_pool="map", fc_norm=True).use_fc_norm
    assert ts.ViTConfig(global_pool="map", class_token=False).num_prefix_tokens == 0
    with pytest.raises(ValueError, match="global_pool"):
        ts.ViTConfig(global_pool="token", class_token=False)
    with pytest.raises(ValueError, match="global_pool"):
        ts.VisionTransformer(ts.ViTConfig(img_size=64, embed_dim=128, depth=1, num_heads=2, global_pool="max"))


def test_the_map_table():
    assert list(ts.MAP_CONFIGS) == na.MICRO + ["vit_base_patch16_siglip_224", "vit_so400m_patch14_siglip_224"]
    tokens = {n: ts.MAP_CONFIGS[n].num_patches + ts.MAP_CONFIGS[n].num_prefix_tokens for n in na.MICRO}
    assert tokens == {"vit_micro_map_patch16_64": 16, "vit_micro_cls_map_patch16_64": 17, "vit_micro_reg4_map_d80_patch16_64": 20,
                      "vit_micro_map_patch16_400": 625, "vit_micro512_map_patch16_64": 16}
    d80 = ts.MAP_CONFIGS["vit_micro_reg4_map_d80_patch16_64"]
    assert (d80.embed_dim, d80.num_heads, d80.head_dim, d80.reg_tokens, d80.class_token) == (320, 4, 80, 4, False)
    so = ts.MAP_CONFIGS["vit_so400m_patch14_siglip_224"]
    assert (so.embed_dim, so.depth, so.num_heads, so.head_dim, so.hidden_dim) == (1152, 27, 16, 72, 4304)
    assert all(c.global_pool == "map" for c in ts.MAP_CONFIGS.values())
    assert not set(ts.MAP_CONFIGS) & (set(ts.CONFIGS) | set(ts.SWIGLU_CONFIGS) | set(ts.NOCLASS_CONFIGS))
    for n in ts.MAP_CONFIGS:
        assert ts.config_of(n) is ts.MAP_CONFIGS[n]
    with pytest.raises(KeyError):
        ts.config_of("no_such_model")


# ---- the weight streams ------------------------------------------------------------------------------------------------------

def test_the_other_tables_hold_what_they_held():
    import test_swiglu_cpu
    assert list(ts.CONFIGS) == list(test_swiglu_cpu.PARENT)       # (that file holds every CONFIGS entry to its parent digest)
    assert list(ts.SWIGLU_CONFIGS) + list(ts.NOCLASS_CONFIGS) == list(PARENT)


@pytest.mark.parametrize("name", list(PARENT))
def test_existing_configs_keep_their_weight_stream(name):
    sd = ts.synth_state_dict(ts.config_of(name), seed=3, std=0.08, bias_std=0.02)
    assert sd_hash(sd) == PARENT[name] and not any(k.startswith("attn_pool") for k in sd)


def test_the_pool_is_drawn_behind_every_other_tensor():
    """a map config draws exactly what its global_pool='token' twin with the same rows draws, then the pool"""
    cfg = ts.config_of("vit_micro_cls_map_patch16_64")
    twin = dataclasses.replace(cfg, global_pool="token")
    a, b = ts.synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02), ts.synth_state_dict(twin, seed=3, std=0.08, bias_std=0.02)
    assert list(a)[:len(b)] == list(b) and all(np.array_equal(a[k], b[k]) for k in b)
    assert [k for k in list(a)[len(b):]] == ["attn_pool." + n for n in (
        "latent", "q.weight", "q.bias", "kv.weight", "kv.bias", "proj.weight", "proj.bias", "norm.weight", "norm.bias",
        "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]
    reg = ts.config_of("vit_micro_reg4_map_d80_patch16_64")
    keys = list(ts.synth_state_dict(reg, seed=3))
    assert keys.index("reg_token") < keys.index("attn_pool.latent") and "cls_token" not in keys


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", na.MICRO)
def test_check_supported_accepts_the_micro_models(name):
    cfg = ts.config_of(name)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(name), na.SCHED)
    d = w.check_supported()
    assert d["pool"] == "map" and d["ext"] and d["norm"] and not d["fc_norm"]
    assert d["class_token"] == cfg.class_token and d["num_prefix"] == cfg.num_prefix_tokens
    assert d["attn_pool"] == dict(heads=cfg.num_heads, hidden=cfg.hidden_dim, hidden_pad=(cfg.hidden_dim + 63) // 64 * 64,
                                  act="gelu", eps=cfg.ln_eps)
    assert w.importance_query == ("cls" if cfg.class_token else "mean")
    assert attn_pool_module(w.m) is w.m.attn_pool


def test_an_mlp_width_off_the_k_step_is_padded():
    cfg = dataclasses.replace(ts.config_of("vit_micro_map_patch16_64"), mlp_ratio=2.6875, act="quick_gelu")
    d = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg), {}).check_supported()
    assert d["attn_pool"]["hidden"] == 344 and d["attn_pool"]["hidden_pad"] == 384 and d["attn_pool"]["act"] == "quick_gelu"


def _refused(model, match, sched=None, exc=NotImplementedError):
    with pytest.raises(exc, match=match):
        rajni_amd.RAJNIViTWrapper(model, sched or {}).check_supported()


def test_the_wrapper_refuses_what_is_not_the_contract():
    fresh = lambda name="vit_micro_map_patch16_64": ts.create_model(name)
    # 'map' without a pool names global_pool; a pool beside another global_pool, or one that is not the contract, names attn_pool
    m = fresh()
    m.attn_pool = None
    _refused(m, "global_pool")
    m = fresh("vit_micro_gap_patch16_64")
    m.global_pool = "map"
    _refused(m, "global_pool")
    m = fresh("vit_micro_patch16_64")
    m.attn_pool = fresh().attn_pool
    _refused(m, "attn_pool")
    m = fresh()
    m.attn_pool = nn.Linear(4, 4)
    _refused(m, "attn_pool")
    for edit, word in ((lambda ap: setattr(ap, "q_norm", nn.LayerNorm(64)), "q_norm"),
                       (lambda ap: setattr(ap, "k_norm", nn.LayerNorm(64)), "k_norm"),
                       (lambda ap: setattr(ap, "latent_len", 2), "latent_len"),
                       (lambda ap: setattr(ap, "latent", nn.Parameter(torch.zeros(1, 2, 128))), "latent_len"),
                       (lambda ap: setattr(ap, "pos_embed", nn.Parameter(torch.zeros(17, 128))), "pos_embed"),
                       (lambda ap: setattr(ap.mlp, "act", nn.SiLU()), "SiLU"),
                       (lambda ap: setattr(ap.mlp, "act", nn.GELU(approximate="tanh")), "tanh"),
                       (lambda ap: setattr(ap, "norm", nn.LayerNorm(128, elementwise_affine=False)), "attn_pool.norm"),
                       (lambda ap: setattr(ap, "norm", nn.Identity()), "attn_pool.norm"),
                       (lambda ap: setattr(ap, "kv", nn.Linear(128, 128)), "attn_pool.kv"),
                       (lambda ap: setattr(ap, "num_heads", 3), "num_heads"),
                       (lambda ap: setattr(ap, "scale", 1.0), "scale"),
                       (lambda ap: setattr(ap, "pool", "avg"), "attn_pool.pool"),
                       (lambda ap: setattr(ap, "mlp", ts.GluMlp(128, 256)), "attn_pool.mlp")):
        m = fresh()
        edit(m.attn_pool)
        _refused(m, word)
    # timm's explicit fc_norm=True moves the final norm behind the pool: the pool would read the un-normalised stream
    _refused(ts.create_model(dataclasses.replace(ts.config_of("vit_micro_map_patch16_64"), fc_norm=True)), "global_pool='map'")
    # the options that never form the rows the pool reads, or that the pool has no form for
    for name in ("vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64"):
        w = rajni_amd.RAJNIViTWrapper(fresh(name), {})
        with pytest.raises(ValueError):
            w.set_last_block_cls_only(True)
    w = rajni_amd.RAJNIViTWrapper(fresh("vit_micro512_map_patch16_64"), {})
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.set_weight_format("fp8_mfma")
    assert w.set_weight_format("fp8") is w
    m = fresh("vit_micro_cls_map_patch16_64")
    w = rajni_amd.RAJNIViTWrapper(m, {}).set_last_block_cls_only(False)
    w._cls_only_last = True                      # (the pool was attached after the setter)
    with pytest.raises(ValueError, match="global_pool='map'"):
        w.check_supported()


class _FakeCuda:
    """stands in for a device tensor up to ops.pool_norm's device check - the pool refusal comes right behind it"""
    is_cuda = True


def test_pool_norm_keeps_refusing_map():
    with pytest.raises(NotImplementedError, match="pool"):
        ops.pool_norm(_FakeCuda(), "map")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_the_header_is_additive_and_nothing_else_moves():
    assert nat.ATTNPOOL_SYMBOLS == ATTNPOOL_SYMBOLS and nat.POOL_MAP == 6
    header = open(os.path.join(ROOT, "include", "rajni_hip_attnpool.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", code)) == set(ATTNPOOL_SYMBOLS)
    assert '#include "rajni_hip_query.h"' in header and re.search(r"enum \{ RAJNI_POOL_MAP = 6 \};", header)
    assert "unverified" in header.lower()
    lib = nat.lib()
    for s in ATTNPOOL_SYMBOLS:
        assert getattr(lib, s) is not None
    names = [f[0] for f in nat.VitAttnPool._fields_]
    assert names == ["q", "kv_w", "kv_b", "proj_w", "proj_b", "norm_w", "norm_b", "norm_eps", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
                     "hidden", "heads", "act"] and C.sizeof(nat.VitAttnPool) == 112
    m = re.search(r"typedef struct \{(.*?)\} rajni_vit_attn_pool;", code, flags=re.S)
    assert re.findall(r"(\w+);", m.group(1)) == names
    # the old counts, sizes and versions
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert len(nat.EXPORTED_SYMBOLS) == 45 and len(nat.IMAGE_SYMBOLS) == 5 and len(nat.QUERY_SYMBOLS) == 6
    assert not set(ATTNPOOL_SYMBOLS) & (set(nat.EXPORTED_SYMBOLS) | set(nat.LAYERS_SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.QUERY_SYMBOLS))
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.VitPrefix) == 16 and C.sizeof(nat.VitQuery) == 8
    for h in ("rajni_hip.h", "rajni_hip_debug.h", "rajni_hip_layers.h", "rajni_hip_image.h", "rajni_hip_query.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "rajni_vit_attn_pool" not in text and "RAJNI_POOL_MAP" not in text
    # its placement lines, in the table's format
    import placement
    start = header.index("---- placement:")
    table = {}
    for mm in re.finditer(r"^ \*   (rajni_\w+): (.+)$", header[start:header.index("(end of the placement table)")], re.M):
        table[mm.group(1)] = {it.split()[0]: int(it.split()[1]) for it in mm.group(2).split(",")}
    assert table == {"rajni_attention_pool": {"kv": 16, "q": 16, "out": 16}, "rajni_vit_forward_pool": {"images": 16, "logits": 16},
                     "rajni_vit_attn_pool": {n: 16 for n in names if n not in ("norm_eps", "hidden", "heads", "act")}}
    assert not set(table) & set(placement.parse_header())


def test_the_kernel_s_argument_checks_run_without_a_device():
    lib = nat.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    p += (-p) % 16
    BF = nat.RAJNI_BF16
    # rajni_attention_pool(kv, q, out, B, N, H, D, dtype, stream)
    for args, code, word in (((None, p, p, 1, 4, 1, 8, BF), 1, "null"), ((p, None, p, 1, 4, 1, 8, BF), 1, "null"),
                             ((p, p, None, 1, 4, 1, 8, BF), 1, "null"), ((p, p, p, 0, 4, 1, 8, BF), 1, "B > 0"),
                             ((p, p, p, 1, 0, 1, 8, BF), 1, "N >= 1"), ((p, p, p, 1, 4, 0, 8, BF), 1, "H > 0"),
                             ((p, p, p, 1, 4, 1, 4, BF), 2, "head dim"), ((p, p, p, 1, 4, 1, 136, BF), 2, "head dim"),
                             ((p, p, p, 1, 4, 1, 12, BF), 2, "head dim"), ((p, p, p, 65536, 4, 1, 8, BF), 2, "at most 65535 images"),
                             ((p, p, p, 1, 4, 1, 8, 7), 1, "dtype"),
                             ((p + 2, p, p, 1, 4, 1, 8, BF), 1, "kv must be 16-byte aligned"),
                             ((p, p + 4, p, 1, 4, 1, 8, BF), 1, "q must be 16-byte aligned"),
                             ((p, p, p + 8, 1, 4, 1, 8, BF), 1, "out must be 16-byte aligned")):
        assert lib.rajni_attention_pool(*args, None) == code, args
        assert "rajni_attention_pool" in _err(lib) and word in _err(lib), (_err(lib), word)


def _plan():
    plan = nat.VitPlan()
    plan.dtype, plan.B, plan.in_chans, plan.img_size, plan.patch_size = nat.RAJNI_BF16, 3, 3, 64, 16
    plan.C, plan.H, plan.D, plan.depth, plan.hidden, plan.num_classes = 128, 2, 64, 4, 512, 10
    return plan


def _record(p):
    rec = nat.VitAttnPool()
    for name in ("q", "kv_w", "kv_b", "proj_w", "proj_b", "norm_w", "norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
        setattr(rec, name, p)
    rec.norm_eps, rec.hidden, rec.heads, rec.act = 1e-6, 512, 2, nat.MLP_GELU
    return rec


def test_the_forward_names_the_field_it_refuses():
    lib = nat.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    p += (-p) % 16
    ref = lambda r: C.byref(r) if r is not None else None
    fwd = lambda plan, e, pre, q, rec: lib.rajni_vit_forward_pool(C.byref(plan), ref(e), ref(pre), None, None, ref(q), ref(rec), p, p, None)
    plan, ext = _plan(), nat.VitExt()
    ext.pool = nat.POOL_MAP
    nocls = nat.VitQuery(0, nat.QUERY_MEAN)
    # RAJNI_POOL_MAP through every older entry point, and through the new one without the record: the unknown pool value it
    # always was, refused where pool 4 is (behind the plan's own checks: this plan passes them, and launches nothing)
    full, blocks = _plan(), (nat.Block * 4)()
    for name in ("patch_w", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w"):
        setattr(full, name, p)
    full.blocks = blocks
    for call in (lambda: lib.rajni_vit_forward_ext(C.byref(full), C.byref(ext), p, p, None),
                 lambda: lib.rajni_vit_forward_ext_prefix(C.byref(full), C.byref(ext), None, p, p, None),
                 lambda: lib.rajni_vit_forward_layers(C.byref(full), C.byref(ext), None, None, p, p, None),
                 lambda: lib.rajni_vit_forward_image(C.byref(full), C.byref(ext), None, None, None, p, p, None),
                 lambda: lib.rajni_vit_forward_query(C.byref(full), C.byref(ext), None, None, None, C.byref(nocls), p, p, None),
                 lambda: fwd(full, ext, None, nocls, None), lambda: fwd(full, ext, None, None, None)):
        assert call() == 2
        assert "pool must be" in _err(lib) and "(6)" in _err(lib) and "rajni_vit_attn_pool record" in _err(lib), _err(lib)
    four = nat.VitExt()
    four.pool = 4
    assert fwd(full, four, None, None, None) == 2 and _err(lib) == "rajni_vit_forward_ext: pool must be RAJNI_POOL_TOKEN or RAJNI_POOL_AVG (4)"
    # the record with another pool, or with no ext at all
    for e in (None, nat.VitExt()):
        assert fwd(plan, e, None, None, _record(p)) == 1 and "ext.pool must be RAJNI_POOL_MAP" in _err(lib), _err(lib)
    avg = nat.VitExt()
    avg.pool = nat.POOL_AVG
    assert fwd(plan, avg, None, nocls, _record(p)) == 1 and "ext.pool must be RAJNI_POOL_MAP" in _err(lib)
    # refused as RAJNI_POOL_AVG is
    plan.cls_only_last_block = 1
    assert fwd(plan, ext, None, None, _record(p)) == 1 and "plan.cls_only_last_block" in _err(lib)
    plan.cls_only_last_block, plan.act_fp8 = 0, 1
    assert fwd(plan, ext, None, None, _record(p)) == 2 and "plan.act_fp8" in _err(lib)
    plan.act_fp8 = 0
    assert fwd(plan, ext, nat.VitPrefix(2, p, 2), None, _record(p)) == 2 and "prefix.head_rows" in _err(lib)
    # the record's own fields
    absent = nat.VitExt()
    absent.pool, absent.norm_absent = nat.POOL_MAP, 1
    assert fwd(plan, absent, None, None, _record(p)) == 2 and "ext.norm_absent" in _err(lib)
    for field, val, word in (("q", None, "pool.q"), ("kv_w", None, "pool.kv_w"), ("proj_w", None, "pool.proj_w"),
                             ("norm_w", None, "pool.norm_w"), ("norm_b", None, "pool.norm_b"), ("fc1_w", None, "pool.fc1_w"),
                             ("fc2_w", None, "pool.fc2_w"), ("heads", 0, "pool.heads"), ("heads", 3, "pool.heads"),
                             ("heads", 32, "pool.heads"), ("hidden", 0, "pool.hidden"), ("hidden", 344, "pool.hidden"),
                             ("act", 3, "pool.act"), ("act", 2, "pool.act"), ("kv_b", p + 4, "kv_b must be 16-byte aligned"),
                             ("q", p + 8, "q must be 16-byte aligned")):
        rec = _record(p)
        setattr(rec, field, val)
        assert fwd(plan, ext, None, None, rec) == 1 and "rajni_vit_forward_pool" in _err(lib) and word in _err(lib), (_err(lib), word)
    # the query record's and the prefix record's refusals are rajni_vit_forward_query's
    assert fwd(plan, ext, None, nat.VitQuery(0, 0), _record(p)) == 1 and "query.query must be RAJNI_QUERY_MEAN" in _err(lib)
    assert fwd(plan, ext, nat.VitPrefix(3, None, 0), nocls, _record(p)) == 1 and "reg_token" in _err(lib)
    # what passes the records reaches the plan's own checks (this plan has no blocks), with and without a class row
    for q in (None, nocls):
        assert fwd(plan, ext, None, q, _record(p)) == 1 and _err(lib) == "rajni_vit_forward: bad plan"


def test_the_workspace_grows_by_the_pool_s_rows_only():
    lib = nat.lib()
    plan = _plan()
    buf = (C.c_char * 64)()
    rec = _record(C.addressof(buf))
    a256 = lambda v: (v + 255) // 256 * 256
    for q in (None, nat.VitQuery(1, 1), nat.VitQuery(0, 1)):
        qp = C.byref(q) if q is not None else None
        base = lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, qp)
        assert base > 0 and lib.rajni_vit_workspace_bytes_pool(C.byref(plan), None, None, qp, None) == base
        got = lib.rajni_vit_workspace_bytes_pool(C.byref(plan), None, None, qp, C.byref(rec))
        assert got == a256(base) + 3 * a256(3 * 128 * 4) + a256(3 * 512 * 4)      # o, y, n [B, C] and hid [B, hidden], fp32
    assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, None) == lib.rajni_vit_workspace_bytes(C.byref(plan))
    rec.hidden = 344
    assert lib.rajni_vit_workspace_bytes_pool(C.byref(plan), None, None, None, C.byref(rec)) == 0
    assert lib.rajni_vit_workspace_bytes_pool(C.byref(plan), None, None, C.byref(nat.VitQuery(0, 0)), C.byref(_record(0))) == 0


# ---- the kernel's yardstick ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", na.KV_KINDS)
def test_the_fp32_restatement_meets_its_own_budget(kind):
    """the budget is derived, not fitted: a plain fp32 evaluation of the same attention (numpy, another summation order) must
    sit inside it with room, and `big` must be what it says - logits of about +-80"""
    kv, q = na.pool_operands(kind, 2, 625, 2, 64, "bf16")
    want, bud = na.pool_attention_budget(kv, q, "fp32")
    t = kv.reshape(2, 625, 2, 2, 64)
    s = np.einsum("hd,bnhd->bhn", q, t[:, :, 0]).astype(np.float32)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    got = np.einsum("bhn,bnhd->bhd", p / p.sum(axis=-1, keepdims=True), t[:, :, 1]).reshape(2, 128)
    assert nm.worst_ratio(got, want, bud)[0] <= 0.5
    if kind == "big":
        assert 75 <= s.max() <= 85 and -85 <= s.min() <= -75
    if kind == "equal":
        assert np.abs(want - t[:, :, 1].astype(np.float64).mean(axis=1).reshape(2, 128)).max() <= 1e-12


# ---- the seeds of tests/test_gpu_attnpool_forward.py -----------------------------------------------------------------------------

def _fixture(name, seed):
    cfg = ts.config_of(name)
    return cfg, ts.state_dict_numpy(ts.create_model(cfg, seed=seed, round_bf16=True, **na.FIX_BASE))


def search_seeds(name, seeds=range(1, 61)):
    """(weight seed, image seed = weight seed + 4) with the LARGEST smallest boundary gap, in units of the bf16 score budget,
    among the given weight seeds at B = 3 - how numerics_attnpool.SEEDS was filled; not run by the suite"""
    best = (0.0, None)
    for seed in seeds:
        cfg, sd = _fixture(name, seed)
        best = max(best, (nq.boundary_gap_ratios(sd, na.images_of(cfg, 3, seed + 4), na.SCHED, cfg, "bf16"), seed))
    return best[1], best[1] + 4


@pytest.mark.parametrize("name", sorted(na.SEEDS))
def test_no_committed_seed_hinges_on_a_near_tie(name):
    wseed, iseed = na.SEEDS[name]
    cfg, sd = _fixture(name, wseed)
    for B in (3, 1):
        r = nq.boundary_gap_ratios(sd, na.images_of(cfg, B, iseed), na.SCHED, cfg, "bf16")
        print(f"[attnpool] {name} B={B}: smallest boundary gap / bf16 score budget = {r:.3g}")
        assert r >= na.GAP_FACTOR


@pytest.mark.parametrize("name", ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64"])
def test_the_stock_forward_is_the_restatement_with_an_empty_schedule(name):
    cfg, sd = _fixture(name, na.SEEDS[name][0])
    imgs = na.images_of(cfg, 2, 7)
    with torch.no_grad():
        stock = ts.create_model(cfg, seed=na.SEEDS[name][0], round_bf16=True, **na.FIX_BASE).double()(torch.from_numpy(imgs).double()).numpy()
    want, counts, tr = na.vit_forward_restated(sd, imgs, {}, cfg)
    assert counts == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth and not tr
    assert np.abs(stock - want).max() <= 1e-11 * np.abs(want).max()
    pooled, _, _ = na.vit_forward_restated(sd, imgs, {}, cfg, pooled=True)
    assert pooled.shape == (2, cfg.embed_dim)
    assert np.abs(pooled @ sd["head.weight"].astype(np.float64).T + sd["head.bias"] - want).max() <= 1e-12 * np.abs(want).max()
