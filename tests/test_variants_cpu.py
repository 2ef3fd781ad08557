"""timm options of the native forward (q/k-norm, norm_pre, pooled head with fc_norm), without a GPU:
the timm-shaped model, the wrapper's host logic, the ABI additions, and the budgets of tests/numerics_variants.py tested
against fp32 emulations of the kernels' algorithms and against deliberately wrong variants of each."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics as nm
import numerics_variants as nv
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import RAJNIAttention

# sha256 (16 hex digits) over names and bytes of synth_state_dict, in draw order, and the first four stock-forward logits
# of image batch default_rng(1) [2, 3, S, S] on create_model(seed=3, std=0.08, bias_std=0.02, round_bf16=True) - all computed
# on the commit BEFORE the options were added to timm_shaped.py.
#   name: (seed 0 defaults, seed 3 std 0.08 bias_std 0.02, logits or None, number of state-dict keys or None)
PARENT = {
    "vit_tiny_patch16_224": ("7f45a5ef230d35b1", "a4f955f0c9977d03", None, None),
    "vit_small_patch16_224": ("31afed001cbe893a", "2cf2fd17aaf8e678", None, None),
    "vit_base_patch16_224": ("c0be6b3704e0e04b", "75e15e0f1cee5f28", None, None),
    "deit3_base_patch16_224": ("323d7e4699509a23", "3c2f272ff90e580f", None, None),
    "vit_micro_patch16_64": ("0589783db7044cd4", "0b25e3a4f0eed014",
                             [-0.2623729705810547, -1.8372068405151367, 0.4293941855430603, -0.3221176266670227], 56),
    "deit3_micro_patch16_64": ("c073c6a6b084ab96", "c2a3ade870131ac1",
                               [0.7720088362693787, -0.09309306740760803, 0.19203788042068481, 0.016552239656448364], 64),
    "vit_micro512_patch16_64": ("fb50454c3bced2ab", "76d51cf3475f0560",
                                [3.406496524810791, 0.5594394207000732, 0.4985755980014801, -1.0244417190551758], 56),
    "vit_micro_patch14_56": ("6d08b72b262aad12", "fdb7bc9ccf0a1882",
                             [-1.3147423267364502, 0.008388414978981018, 1.125379204750061, 0.15330249071121216], 56),
    "vit_micro_d80_patch16_64": ("0165c5c7a524b02b", "84b42027dc237f6e",
                                 [2.18524432182312, -2.4525961875915527, -0.9395776391029358, 0.4216312766075134], 56),
}


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------
# timm_shaped
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PARENT))
def test_old_configs_keep_their_weight_stream_and_logits(name):
    h0, h3, logits, nkeys = PARENT[name]
    cfg = ts.CONFIGS[name]
    assert not cfg.qk_norm and not cfg.pre_norm and cfg.global_pool == "token" and not cfg.use_fc_norm
    assert sd_hash(ts.synth_state_dict(cfg, seed=0)) == h0
    assert sd_hash(ts.synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02)) == h3
    if logits is not None:
        m = ts.create_model(cfg, seed=3, std=0.08, bias_std=0.02, round_bf16=True)
        assert len(m.state_dict()) == nkeys
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, cfg.img_size, cfg.img_size), dtype=np.float32))
        with torch.no_grad():
            got = m(x).numpy().ravel()[:4]
        np.testing.assert_allclose(got, logits, rtol=0, atol=2e-5)     # (the same graph; BLAS builds differ in the last bits)


def test_new_configs_expose_timm_names_and_draw_after_the_old_tensors():
    cfg = ts.CONFIGS["vit_micro_all_patch16_64"]
    m = ts.create_model(cfg, seed=1, bias_std=0.02)
    keys = set(m.state_dict())
    for k in ("norm_pre.weight", "norm_pre.bias", "fc_norm.weight", "fc_norm.bias", "blocks.0.attn.q_norm.weight",
              "blocks.3.attn.k_norm.bias"):
        assert k in keys
    assert "norm.weight" not in keys and isinstance(m.norm, nn.Identity) and m.global_pool == "avg"      # timm: fc_norm replaces norm
    assert isinstance(m.blocks[0].attn.q_norm, nn.LayerNorm) and m.blocks[0].attn.q_norm.normalized_shape == (64,)
    assert m.num_prefix_tokens == 1
    # a config with one option: every tensor an option-free config has comes first, bit for bit
    plain = ts.synth_state_dict(ts.CONFIGS["vit_micro_patch16_64"], seed=4, std=0.05, bias_std=0.02)
    for name in ("vit_micro_qknorm_patch16_64", "vit_micro_prenorm_patch16_64"):
        sd = ts.synth_state_dict(ts.CONFIGS[name], seed=4, std=0.05, bias_std=0.02)
        assert list(sd)[:len(plain)] == list(plain)
        assert all(np.array_equal(sd[k], plain[k]) for k in plain)
        assert len(sd) > len(plain)
    for name in ("vit_base_patch16_clip_224", "vit_base_patch16_qknorm_224"):
        assert ts.CONFIGS[name].embed_dim == 768 and ts.CONFIGS[name].depth == 12
    assert ts.CONFIGS["vit_base_patch16_clip_224"].pre_norm and ts.CONFIGS["vit_base_patch16_qknorm_224"].qk_norm


def _images(cfg, B=2, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


# (config, the option to drop in the yardstick graph); std / bias_std / seed of the forward fixtures
FORWARD_CASES = [("vit_micro_qknorm_patch16_64", "qk_norm"), ("vit_micro_prenorm_patch16_64", "pre_norm"),
                 ("vit_micro_gap_patch16_64", "avg_pool"), ("vit_micro_gap_patch16_64", "fc_norm"),
                 ("vit_micro_fcnorm_patch16_64", "fc_norm"), ("vit_micro_all_patch16_64", "qk_norm"),
                 ("vit_micro_all_patch16_64", "pre_norm"), ("vit_micro_all_patch16_64", "avg_pool"),
                 ("vit_micro_d80_qknorm_patch16_64", "qk_norm"), ("vit_micro512_qknorm_patch16_64", "qk_norm")]
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}


@pytest.mark.parametrize("name,option", FORWARD_CASES)
def test_stock_forward_honours_each_option_and_the_fixtures_can_tell(name, option):
    """The stock forward (the unpruned yardstick) equals the restated graph with an empty schedule, and ignoring the option
    moves the fp32 logits by at least 5x the 16-bit acceptance bar (1e-2 of the logit scale) - unpruned and pruned -
    so a forward that drops the option cannot pass tests/test_gpu_variants_forward.py."""
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **FIX)
    sd = ts.state_dict_numpy(model)
    imgs = _images(cfg)
    with torch.no_grad():
        stock = model(torch.from_numpy(imgs)).numpy()
    want, counts, _ = nv.vit_forward_restated(sd, imgs, {}, cfg, dtype=torch.float32)
    scale = float(np.abs(want).max())
    assert np.abs(stock - want).max() <= 1e-4 * scale
    assert counts == [cfg.num_patches + 1] * cfg.depth
    for sched in ({}, SCHED):
        full, _, tr = nv.vit_forward_restated(sd, imgs, sched, cfg, dtype=torch.float32)
        forced = {i: t["keep_idx"] for i, t in tr.items()}
        dropped, _, _ = nv.vit_forward_restated(sd, imgs, sched, cfg, dtype=torch.float32, drop=(option,), forced_keep=forced)
        moved, bar = float(np.abs(full - dropped).max()), 1e-2 * float(np.abs(full).max())
        print(f"{name} without {option} ({'pruned' if sched else 'unpruned'}): logits move {moved:.4g}, bar {bar:.4g}")
        assert moved >= 5 * bar


# ---------------------------------------------------------------------------------------------------------------
# wrapper host logic
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vit_micro_qknorm_patch16_64", "vit_micro_prenorm_patch16_64", "vit_micro_gap_patch16_64",
                                  "vit_micro_fcnorm_patch16_64", "vit_micro_all_patch16_64"])
def test_wrapper_accepts_the_options(name):
    cfg = ts.CONFIGS[name]
    m = ts.create_model(cfg)
    before = {k for k, _ in m.named_parameters()}
    w = rajni_amd.RAJNIViTWrapper(m, SCHED)
    d = w.check_supported()
    assert d["ext"] and d["qk_norm"] == cfg.qk_norm and d["norm_pre"] == cfg.pre_norm and d["fc_norm"] == cfg.use_fc_norm
    assert d["pool"] == cfg.global_pool and d["norm"] == (not cfg.use_fc_norm)
    assert {k for k, _ in m.named_parameters()} == before               # the surgery keeps timm's parameter names
    att = m.blocks[1].attn
    assert isinstance(att, RAJNIAttention)
    assert isinstance(att.q_norm, nn.LayerNorm if cfg.qk_norm else nn.Identity)
    assert isinstance(att.k_norm, nn.LayerNorm if cfg.qk_norm else nn.Identity)


def test_plain_models_need_no_extension_record():
    d = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), SCHED).check_supported()
    assert d["ext"] is False and d["pool"] == "token"


class RMSNorm(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))
        self.eps = 1e-6

    def forward(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


def test_unsupported_variants_are_still_refused():
    cfg = ts.CONFIGS["vit_micro_qknorm_patch16_64"]
    # RMSNorm q/k-norm: in a scheduled block at construction, in any block at the model check
    m = ts.create_model(cfg)
    m.blocks[1].attn.q_norm, m.blocks[1].attn.k_norm = RMSNorm(64), RMSNorm(64)
    with pytest.raises(NotImplementedError, match="q_norm is RMSNorm"):
        rajni_amd.RAJNIViTWrapper(m, SCHED)
    m = ts.create_model(cfg)
    m.blocks[0].attn.q_norm, m.blocks[0].attn.k_norm = RMSNorm(64), RMSNorm(64)
    with pytest.raises(NotImplementedError, match="q_norm is RMSNorm"):
        rajni_amd.RAJNIViTWrapper(m, SCHED).check_supported()
    # non-affine, q without k, differing eps between q and k or between blocks
    for edit in (lambda a: setattr(a, "q_norm", nn.LayerNorm(64, elementwise_affine=False)),
                 lambda a: setattr(a, "k_norm", nn.Identity()),
                 lambda a: setattr(a, "k_norm", nn.LayerNorm(64, eps=1e-5)),
                 lambda a: (setattr(a, "q_norm", nn.LayerNorm(64, eps=1e-5)), setattr(a, "k_norm", nn.LayerNorm(64, eps=1e-5)))):
        m = ts.create_model(cfg)
        edit(m.blocks[3].attn)
        with pytest.raises(NotImplementedError):
            rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # pools other than token / avg, an attention pool, two prefix tokens
    for pool in ("map", "avgmax", "max", ""):
        m = ts.create_model("vit_micro_gap_patch16_64")
        m.global_pool = pool
        with pytest.raises(NotImplementedError, match="global_pool"):
            rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = ts.create_model("vit_micro_patch16_64")
    m.attn_pool = nn.Linear(4, 4)
    with pytest.raises(NotImplementedError, match="attn_pool"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = ts.create_model("vit_micro_patch16_64")
    m.num_prefix_tokens = 2
    with pytest.raises(NotImplementedError, match="2 prefix tokens"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # no norm at all, a non-affine norm_pre
    m = ts.create_model("vit_micro_patch16_64")
    m.norm = nn.Identity()
    with pytest.raises(NotImplementedError, match="base_model.norm"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = ts.create_model("vit_micro_prenorm_patch16_64")
    m.norm_pre = nn.LayerNorm(128, elementwise_affine=False)
    with pytest.raises(NotImplementedError, match="norm_pre"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # 'avg' pooling with the CLS-only last block: the rows to be averaged are never formed
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_gap_patch16_64"), {})
    with pytest.raises(ValueError, match="avg"):
        w.set_last_block_cls_only(True)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_fcnorm_patch16_64"), {})
    w.set_last_block_cls_only(True)                                    # token pool + fc_norm: fine
    w.m.global_pool = "avg"
    with pytest.raises(ValueError, match="avg"):
        w.check_supported()


# ---------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = nat.load_library()
    for sym in ("rajni_qk_norm", "rajni_layernorm_stream", "rajni_pool_norm", "rajni_vit_forward_ext"):
        assert sym in nat.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    # the record's layout as the header declares it (LP64): pointer, float, 2 pointers, float, 2 ints, 2 pointers, float
    assert C.sizeof(nat.QkAffine) == 32 and C.sizeof(nat.VitExt) == 72
    assert nat.VitExt.norm_pre_w.offset == 16 and nat.VitExt.norm_absent.offset == 36 and nat.VitExt.fc_norm_w.offset == 48
    # argument checks run before any launch: no device needed
    ext, plan = nat.VitExt(), nat.VitPlan()
    assert lib.rajni_vit_forward_ext(C.byref(plan), C.byref(ext), None, None, None) == 1
    assert lib.rajni_qk_norm(None, None, None, None, None, 1, 1, 64, 1e-6, nat.RAJNI_BF16, None) == 1
    assert b"rajni_qk_norm" in lib.rajni_last_error()
    assert lib.rajni_pool_norm(None, 1, 2, 64, 0, None, None, 0.0, None, None, 0.0, None, 7, 0, None) == 1


# ---------------------------------------------------------------------------------------------------------------
# budgets against emulations and mutants
# ---------------------------------------------------------------------------------------------------------------
DTYPES = ["bf16", "fp16", "fp32"]
EPS = 1e-6


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", nv.HEAD_DIMS)
def test_qk_norm_budget_holds_for_the_emulation_and_rejects_mutants(D, dt):
    rows, H = 45, 3
    qkv, qw, qb, kw, kb = nv.qk_norm_case(rows, H, D, dt)
    want, bud = nv.qk_norm_budget(qkv, H, D, qw, qb, kw, kb, EPS, dt)
    C = H * D
    got = nv.emul_qk_norm(qkv, H, D, qw, qb, kw, kb, EPS, dt)
    nm.assert_within(got[:, :2 * C], want, bud, f"emulated qk_norm D={D} {dt}")
    assert np.array_equal(got[:, 2 * C:], qkv[:, 2 * C:])
    one = nv.emul_qk_norm(qkv, H, D, qw, qb, kw, kb, EPS, dt, one_pass=True)
    with np.errstate(invalid="ignore"):
        assert nm.worst_ratio(one[:, :2 * C], want, bud)[0] > 1.0, "one-pass variance"
    swapped = nv.emul_qk_norm(qkv, H, D, qw, qb, kw, kb, EPS, dt, q_weights_on_k=True)
    assert nm.worst_ratio(swapped[:, :2 * C], want, bud)[0] > 1.0, "q-norm weights applied to k"
    assert nm.worst_ratio(swapped[:, :C], want[:, :C], bud[:, :C])[0] <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [128, 768, 1280])
def test_layernorm_stream_budget_holds_for_the_emulation_and_rejects_one_pass(C, dt):
    x, _, w, b = nm.layernorm_rows(77, C, dt)
    want, bud = nm.layernorm_budget(x, w, b, EPS, dt)
    nm.assert_within(nv.emul_layernorm_stream(x, w, b, EPS, dt), want, bud, f"emulated layernorm_stream C={C} {dt}")
    with np.errstate(invalid="ignore"):
        assert nm.worst_ratio(nv.emul_layernorm_stream(x, w, b, EPS, dt, one_pass=True), want, bud)[0] > 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Np", nv.POOL_NP)
def test_pool_norm_budget_holds_with_a_third_to_spare_and_rejects_mutants(Np, dt):
    B, C = 3, 192
    x, (nw, nb), (fw, fb) = nv.pool_case(B, Np, C, dt)
    for pool, use_norm, use_fc in (("avg", False, True), ("avg", True, True), ("avg", True, False), ("avg", False, False),
                                   ("token", True, True)):
        norm = (nw, nb, EPS) if use_norm else None
        fc = (fw, fb, 1e-5) if use_fc else None
        want, bud = nv.pool_norm_budget(x, pool, norm, fc, dt)
        tag = f"emulated pool_norm Np={Np} {dt} {pool} norm={use_norm} fc_norm={use_fc}"
        nm.assert_within(nv.emul_pool_norm(x, pool, norm, fc, dt), want, bud, tag)
        # the unrounded fp32 emulation needs less than a third of the budget's fp32 part
        w32, b32 = nv.pool_norm_budget(x, pool, norm, fc, "fp32")
        ratio = nm.worst_ratio(nv.emul_pool_norm(x, pool, norm, fc, "fp32", rounded=False), w32, b32)[0]
        print(f"[numerics] {tag}: unrounded fp32 emulation needs {ratio:.3f} of the budget")
        assert ratio < 1 / 3
        # the mutant: a mean that includes the CLS row.  Without a norm in front the stress rows put |p| near 1e3, and a 16-bit
        # output's own rounding (u_out |p|) is then larger than one O(1) row's share of the mean - so it is asserted wherever
        # the rows are normalised first, and on every fp32 case
        if pool == "avg" and Np > 2 and (use_norm or dt == "fp32"):
            cls = nv.emul_pool_norm(x, pool, norm, fc, dt, include_cls=True)
            assert nm.worst_ratio(cls, want, bud)[0] > 1.0, "a mean that includes the CLS row"


def test_restated_graph_equals_the_oracle_on_an_option_free_model():
    """the yardstick graph with no option is the project's oracle (oracle/rajni_oracle.py::vit_forward), selections included"""
    from oracle import rajni_oracle as orc
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, **FIX))
    imgs = _images(cfg, B=3)
    want, stats, tr = orc.vit_forward(sd, imgs, SCHED, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps, return_trace=True)
    got, counts, tr2 = nv.vit_forward_restated(sd, imgs, SCHED, cfg)
    assert counts == stats["token_counts"]
    for i in tr:
        np.testing.assert_array_equal(tr[i]["keep_idx"], tr2[i]["keep_idx"])
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
