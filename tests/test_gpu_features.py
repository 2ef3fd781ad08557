"""Feature outputs on the device: headless models (head = nn.Identity, timm num_classes=0), `forward_features` (the surviving
tokens, RAJNI_POOL_NONE) and its dense form (RAJNI_POOL_DENSE), and `source_idx`.  GPU box only (`-m gpu`).  Batch 3 throughout:
the selections, hence the maps, differ per image.

Exact yardsticks (bit for bit):
  headless pooled output   the same model with head = nn.Linear(C, C), weight the identity, bias zero, through the existing logits
                           path: products with 1.0 and 0.0, fp32 accumulation, one rounding of a value already representable;
  tokens[:, 0]             the headless token-pool forward (the last block's CLS-rows form against all rows);
  dense                    dense[b, source_idx[b, j]] has the bits of tokens[b, j], every other row is all-zero bytes.
Parity yardstick: tests/numerics_features.py in fp64 with its selections injected.  The bar for normalised tokens is
max(BAR[dt], 1.5 x d16), d16 the distance of the same graph run on the CPU in the model's 16-bit dtype from fp64 on the same
fixture - the native forward keeps an fp32 stream, so it should be no farther from fp64 than the 16-bit graph; 1.5 covers the
noise of a max statistic.  Measured figures: DESIGN.md section 2."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import guarded
import numerics_features as nf
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
B = 3
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
FIX512 = dict(seed=4, std=0.06, bias_std=0.02)      # the fixture every embed-dim-512 test of the project draws
SCHED = {1: {"keep_ratio": 0.7}, 2: {"keep_ratio": 0.5}}
WIDE = ts.ViTConfig(img_size=32, embed_dim=1280, num_heads=20, depth=2)      # more than 1024 channels: four chunks per lane
DEEP = ts.ViTConfig(img_size=128, embed_dim=128, num_heads=2, depth=10)      # ten scheduled blocks: the level table chains


def images_of(cfg, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def cfg_of(name_or_cfg):
    return ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg


def wrap(name_or_cfg, sched, dt, head="keep", fix=FIX):
    """head: "keep" the model's classifier, "none" = nn.Identity, "identity" = nn.Linear(C, C) with the identity matrix"""
    cfg = cfg_of(name_or_cfg)
    model = ts.create_model(cfg, round_bf16=True, **fix)
    if head == "none":
        model.head = nn.Identity()
    elif head == "identity":
        model.head = nn.Linear(cfg.embed_dim, cfg.embed_dim)
        with torch.no_grad():
            model.head.weight.copy_(torch.eye(cfg.embed_dim))
            model.head.bias.zero_()
    return rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(TORCH[dt]).eval()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def random_selections(cfg, sched, seed=0):
    """{block: keep_idx [B, P + keep]} drawn at random per image (prefix slots, then ascending patch indices) and the final count"""
    rng = np.random.default_rng(seed)
    P, N = cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    out = {}
    for i in sorted(sched):
        keep = max(1, int(sched[i]["keep_ratio"] * (N - P)))
        out[i] = np.stack([np.concatenate([np.arange(P), P + np.sort(rng.choice(N - P, keep, replace=False))]) for _ in range(B)])
        N = P + keep
    return out, N


def check_dense_against_tokens(w, x, cfg, forced=None):
    """tokens, source_idx and dense of one wrapper; dense must be the tokens at their source rows and zero bytes elsewhere"""
    P, n0 = cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    tokens = w.forward_features(x).clone()
    stats = w.get_last_stats()
    src = stats["source_idx"]
    assert src.dtype == torch.int32 and src.is_cuda and tuple(src.shape) == tuple(tokens.shape[:2])
    dense = w.forward_features(x, dense=True).clone()
    assert w.get_last_stats()["token_counts"] == stats["token_counts"]
    assert torch.equal(w.get_last_stats()["source_idx"], src)
    assert tuple(dense.shape) == (B, n0, cfg.embed_dim) and dense.dtype == tokens.dtype
    s = src.cpu().numpy().astype(np.int64)
    assert (s[:, :P] == np.arange(P)).all() and (np.diff(s, axis=1) > 0).all() and s.max() < n0
    if forced is not None:
        np.testing.assert_array_equal(s, nf.compose_source_idx(forced, B, n0))
    assert not torch.isnan(tokens.float()).any()
    gathered = torch.gather(dense, 1, src.long()[:, :, None].expand(-1, -1, cfg.embed_dim))
    assert same_bits(gathered, tokens), "dense rows at source_idx differ from the tokens"
    mask = torch.ones((B, n0), dtype=torch.bool, device=DEV)
    mask.scatter_(1, src.long(), False)
    assert int(mask.sum()) == B * (n0 - tokens.shape[1])
    assert not dense[mask].contiguous().view(torch.uint8).any(), "a pruned position is not all-zero bytes"
    return tokens, s, dense


# ---- 1. headless pooled output -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [SCHED, {}], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("name, dt", [("vit_micro_patch16_64", "bf16"), ("vit_micro_patch16_64", "fp16"),
                                      ("vit_micro_patch16_64", "fp32"), ("vit_micro_gap_patch16_64", "bf16"),
                                      ("vit_micro_reg4_patch16_64", "bf16"), ("vit_micro_swiglu_patch16_64", "bf16")])
def test_headless_output_is_the_row_an_identity_head_passes_through(name, dt, sched):
    cfg = cfg_of(name)
    x = torch.from_numpy(images_of(cfg)).to(DEV)
    ref = wrap(name, sched, dt, head="identity")
    want = ref(x).clone()
    counts = ref.get_last_stats()["token_counts"]
    w = wrap(name, sched, dt, head="none")
    got = w(x).clone()
    assert tuple(got.shape) == (B, cfg.embed_dim) and got.dtype == TORCH[dt]
    assert w.get_last_stats() == {"token_counts": counts}
    assert w._plan[1].num_classes == 0 and not w._plan[1].head_w and w._plan[1].logits_ld == cfg.embed_dim
    assert float(got.float().abs().max()) > 0.1
    assert same_bits(got, want)


# ---- 2. tokens against the pooled path -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [SCHED, {}], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_row_zero_of_the_tokens_is_the_headless_forward(name, dt, sched):
    cfg = cfg_of(name)
    x = torch.from_numpy(images_of(cfg, seed=3)).to(DEV)
    w = wrap(name, sched, dt, head="none")
    pooled = w(x).clone()
    assert nat.lib().rajni_debug_last_block_cls_rows(C.byref(w._plan[1]), None, None) == 1
    tokens = w.forward_features(x)
    assert tokens.shape[1] == w.get_last_stats()["token_counts"][-1]
    assert same_bits(tokens[:, 0], pooled)
    # and with a head: the features do not depend on it
    assert same_bits(wrap(name, sched, dt).forward_features(x), tokens)


# ---- 3. dense against tokens, forced selections at the binary search's corners ----------------------------------------------

def _corner(cfg, patches):
    """one stage at block 1 that keeps exactly `patches` (the same for every image)"""
    P = cfg.num_prefix_tokens
    ratio = (len(patches) + 0.5) / cfg.num_patches
    idx = np.tile(np.concatenate([np.arange(P), P + np.asarray(patches)]), (B, 1))
    return {1: {"keep_ratio": ratio}}, {1: idx}


@pytest.mark.parametrize("case", ["first", "last", "first_and_last", "keep1_after_three", "all_four"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_dense_is_the_tokens_at_their_source_rows(name, case):
    cfg = cfg_of(name)
    n = cfg.num_patches
    if case == "first":
        sched, forced = _corner(cfg, [0])
    elif case == "last":
        sched, forced = _corner(cfg, [n - 1])
    elif case == "first_and_last":
        sched, forced = _corner(cfg, [0, n - 1])
    else:
        sched = ({0: {"keep_ratio": 0.5}, 1: {"keep_ratio": 0.5}, 2: {"keep_ratio": 0.01}} if case == "keep1_after_three"
                 else {i: {"keep_ratio": 0.8} for i in range(4)})
        forced, n_last = random_selections(cfg, sched, seed=7)
        assert n_last == cfg.num_prefix_tokens + (1 if case == "keep1_after_three" else 5)
    w = wrap(name, sched, "bf16")
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(images_of(cfg, seed=4)).to(DEV)
    tokens, s, _ = check_dense_against_tokens(w, x, cfg, forced)
    assert tokens.shape[1] == forced[max(forced)].shape[1]


@pytest.mark.parametrize("what", ["c512", "c1280", "deep_chain", "stream_bf16", "stream_fp16", "fp32", "fp16"])
def test_dense_across_widths_depths_and_stream_types(what):
    dt, stream, fix = "bf16", False, FIX
    if what == "c512":
        cfg, sched, fix = cfg_of("vit_micro512_patch16_64"), SCHED, FIX512
    elif what == "c1280":
        cfg, sched, fix = WIDE, {0: {"keep_ratio": 0.5}}, dict(seed=4, std=0.03, bias_std=0.02)
    elif what == "deep_chain":
        cfg, sched = DEEP, {i: {"keep_ratio": 0.9} for i in range(10)}
    else:
        cfg, sched = cfg_of("vit_micro_reg4_patch16_64"), SCHED
        dt = {"stream_bf16": "bf16", "stream_fp16": "fp16", "fp32": "fp32", "fp16": "fp16"}[what]
        stream = what.startswith("stream")
    forced, n_last = random_selections(cfg, sched, seed=9)
    w = wrap(cfg, sched, dt, fix=fix)
    if stream:
        w.set_residual_dtype(TORCH[dt])
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(images_of(cfg, seed=6)).to(DEV)
    tokens, s, _ = check_dense_against_tokens(w, x, cfg, forced)
    assert tokens.shape[1] == n_last and float(tokens.float().abs().max()) > 0.1
    if what == "deep_chain":
        assert w.get_last_stats()["token_counts"] == [65, 58, 52, 46, 41, 37, 33, 29, 26, 23] and n_last == 20


# ---- 4. source_idx, free-running -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, sched", [("vit_micro_reg4_patch16_64", SCHED), ("vit_micro_patch16_64", {}),
                                         ("vit_micro_distilled_patch16_64", {3: {"keep_ratio": 0.5}})])
def test_source_idx_is_the_composition_of_the_traced_selections(name, sched):
    cfg = cfg_of(name)
    P, n0 = cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    w = wrap(name, sched, "bf16")
    x = torch.from_numpy(images_of(cfg, seed=8)).to(DEV)
    tokens, s, _ = check_dense_against_tokens(w, x, cfg)
    traced = {i: t["keep_idx"].cpu().numpy() for i, t in w.get_last_trace().items()}
    assert sorted(traced) == sorted(sched)
    np.testing.assert_array_equal(s, nf.compose_source_idx(traced, B, n0))
    assert sorted(w.get_last_stats()) == ["source_idx", "token_counts"]
    if sched == SCHED:
        assert len({tuple(r) for r in s}) > 1, "the maps must differ between the images"
    # a plain forward afterwards reports the token counts alone, as ever
    w(x)
    assert sorted(w.get_last_stats()) == ["token_counts"]


# ---- 5. output bounds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["headless", "tokens", "dense"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_every_output_byte_is_written_and_nothing_beyond(name, mode):
    cfg = cfg_of(name)
    w = wrap(name, SCHED, "bf16", head="none" if mode == "headless" else "keep")
    x = torch.from_numpy(images_of(cfg, seed=10)).to(DEV).to(torch.bfloat16).contiguous()
    want = (w(x) if mode == "headless" else w.forward_features(x, dense=mode == "dense")).clone()
    plan, keep = w._plan[1], w._plan[2]
    ext, pre = keep[4], keep[6]
    assert w._plan[5] == {"headless": "logits"}.get(mode, mode) and not plan.head_w and plan.num_classes == 0
    assert (ext.pool if ext is not None else 0) == {"headless": nat.POOL_TOKEN, "tokens": nat.POOL_NONE, "dense": nat.POOL_DENSE}[mode]
    g = guarded.Guarded(tuple(want.shape), torch.bfloat16, device=DEV)
    nat.check(nat.lib().rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext) if ext is not None else None,
                                                     C.byref(pre) if pre is not None else None, x.data_ptr(), g.ptr(),
                                                     nat.stream_ptr(x.device)), "rajni_vit_forward_ext_prefix")
    torch.cuda.synchronize()
    g.check(f"{name} {mode}", written=True)
    assert not torch.isnan(g.t.float()).any()
    assert same_bits(g.t, want)
    if mode == "dense":
        zero_rows = (g.t.contiguous().view(torch.uint8).view(B, want.shape[1], -1) == 0).all(dim=-1)
        assert int(zero_rows.sum()) == B * (want.shape[1] - w.get_last_stats()["token_counts"][-1])


# ---- 6. parity with the restated graph -----------------------------------------------------------------------------------------

def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[features] {what}: max |d| {err:.4g} = {err / scale:.3g} of the scale {scale:.4g} (bar {rel:.3g})")
    assert err <= rel * scale, f"{what}: max |d| {err:.4g} vs scale {scale:.4g} (bar {rel:.3g})"


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64", "vit_micro_gap_patch16_64",
                                  "vit_micro_swiglu_patch16_64"])
def test_features_against_the_restated_graph(name, dt):
    cfg = cfg_of(name)
    model = ts.create_model(cfg, round_bf16=True, **FIX)
    sd = ts.state_dict_numpy(model)
    imgs = images_of(cfg, seed=5)
    want = nf.features_restated(sd, imgs, SCHED, cfg)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar_tokens = bar_pooled = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU: how far 16-bit arithmetic is from fp64 here
        r16 = nf.features_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=TORCH[dt])
        d16_tokens = float(np.abs(r16["tokens"] - want["tokens"]).max() / np.abs(want["tokens"]).max())
        d16_pooled = float(np.abs(r16["pooled"] - want["pooled"]).max() / np.abs(want["pooled"]).max())
        print(f"[features] {name} {dt}: d16 tokens {d16_tokens:.3g}, pooled {d16_pooled:.3g}")
        bar_tokens, bar_pooled = max(BAR[dt], 1.5 * d16_tokens), max(BAR[dt], 1.5 * d16_pooled)
    w = wrap(name, SCHED, dt, head="none")
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(imgs).to(DEV)
    pooled = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == want["counts"]
    close(pooled, want["pooled"], bar_pooled, f"{name} {dt} pooled")
    if cfg.use_fc_norm:       # no final norm: forward_features is out of scope and says so
        with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
            w.forward_features(x)
        return
    tokens = w.forward_features(x).float().cpu().numpy()
    np.testing.assert_array_equal(w.get_last_stats()["source_idx"].cpu().numpy(), want["source_idx"])
    close(tokens, want["tokens"], bar_tokens, f"{name} {dt} tokens")
    dense = w.forward_features(x, dense=True).float().cpu().numpy()
    close(dense, want["dense"], bar_tokens, f"{name} {dt} dense")


def test_forward_features_refusals_on_the_device():
    x = torch.zeros(B, 3, 64, 64, device=DEV)
    w = wrap("vit_micro_patch16_64", SCHED, "bf16").set_last_block_cls_only(True)
    with pytest.raises(ValueError, match="set_last_block_cls_only"):
        w.forward_features(x)
    w = wrap("vit_micro512_patch16_64", SCHED, "bf16", fix=FIX512).set_weight_format("fp8_mfma")
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.forward_features(x)
    # "fp8" weights work: the features of the dequantised model, through the same kernels
    w = wrap("vit_micro512_patch16_64", SCHED, "bf16", fix=FIX512).set_weight_format("fp8")
    cfg = cfg_of("vit_micro512_patch16_64")
    check_dense_against_tokens(w, torch.from_numpy(images_of(cfg, seed=13)).to(DEV), cfg)


# ---- 7. the logits path is untouched ---------------------------------------------------------------------------------------------

# launches per kernel class of ONE logits forward of vit_micro_patch16_64, bf16, SCHED, batch 3, as the parent commit issues them
LOGITS_LAUNCHES = {"gemm_bf16_tn<bias>": 5, "gemm_bf16_tn<bias,gelu>": 4, "gemm_bf16_tn<bias,ls,resid>": 4, "gemm_bf16_tn<patch>": 1,
                   "attn_bf16_d64": 4, "layernorm_kernel": 9, "score_select_kernel<fused>": 2, "cls_pos_kernel": 1,
                   "gemm_bf16_tn<bias,ls,resid> K<=N": 4}


def _launches(w, x):
    nat.profile_reset()
    nat.profile_enable((1 << nat.NUM_KCLASS) - 1)
    try:
        w(x)
        torch.cuda.synchronize()
    finally:
        nat.profile_enable(0)
    out = {k: v["launches"] for k, v in nat.profile_collect().items()}
    nat.profile_reset()
    return out


def test_logits_before_and_after_forward_features():
    cfg = cfg_of("vit_micro_patch16_64")
    w = wrap("vit_micro_patch16_64", SCHED, "bf16")
    x = torch.from_numpy(images_of(cfg, seed=12)).to(DEV)
    before = w(x).clone()
    launches = _launches(w, x)
    print(f"[features] launches of one logits forward: {launches}")
    assert launches == LOGITS_LAUNCHES
    for dense in (False, True):
        feats = w.forward_features(x, dense=dense)
        assert feats.shape[-1] == cfg.embed_dim
        after = w(x).clone()          # (the optimistic launch must not take the feature plan)
        assert tuple(after.shape) == (B, cfg.num_classes) and same_bits(after, before)
        assert w.get_last_stats() == {"token_counts": [17, 17, 12, 6]}
    assert _launches(w, x) == launches
    # a feature forward is the logits forward less the head GEMM, plus the dense form's map kernel
    fl = {}
    for dense in (False, True):
        nat.profile_reset()
        nat.profile_enable((1 << nat.NUM_KCLASS) - 1)
        try:
            w.forward_features(x, dense=dense)
            torch.cuda.synchronize()
        finally:
            nat.profile_enable(0)
        fl[dense] = {k: v["launches"] for k, v in nat.profile_collect().items()}
        nat.profile_reset()
    assert sum(fl[False].values()) == sum(launches.values()) - 1
    assert sum(fl[True].values()) == sum(launches.values())
