"""Whole forwards of models with an attention-pool head (timm `global_pool='map'`: the SigLIP layout, with and without a class
token, with registers) on the device.  GPU box only (`-m gpu`).

Yardsticks (the reference cannot run such a model), those of tests/test_gpu_noclass_forward.py:
  empty schedule   the timm-shaped model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_attnpool.py::vit_forward_restated, torch fp64: its selections injected (`force_keep_idx`), and
                   free-running, where the device's selections must BE the restatement's - the seeds (numerics_attnpool.SEEDS)
                   leave every boundary gap at 17 .. 43 x the bf16 score budget (tests/test_attnpool_cpu.py asserts at least
                   8 x).  The 625-token model cannot have such a seed (numerics_attnpool.LONG_SEEDS says why): free-running it
                   follows tests/test_gpu_long_forward.py - the device's selections are the restated rule on the device's own
                   traced scores, and the restated graph runs on them.
Bars are the project's: 1e-2 x max|out| for 16-bit models, 1e-3 for fp32, 2e-2 for a 16-bit residual stream."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import numerics_attnpool as na
import numerics_image as ni
import numerics_prefix as npx
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
SCHED = na.SCHED
LONG = "vit_micro_map_patch16_400"
SEEDS = dict(na.SEEDS, **na.LONG_SEEDS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(config, fp32 state dict with bf16-representable values, image seed) - built once, never modified"""
    cfg = ts.config_of(name)
    wseed, iseed = SEEDS[name]
    return cfg, ts.state_dict_numpy(ts.create_model(cfg, seed=wseed, round_bf16=True, **na.FIX_BASE)), iseed


@functools.lru_cache(maxsize=None)
def yardstick(name, B, pooled=False):
    """the restated graph, free-running in fp64: computed once per (model, batch)"""
    cfg, sd, iseed = fixture(name)
    return na.vit_forward_restated(sd, na.images_of(cfg, B, iseed), SCHED, cfg, pooled=pooled)


def model_of(name, **replace):
    cfg = dataclasses.replace(ts.config_of(name), **replace) if replace else ts.config_of(name)
    return ts.create_model(cfg, seed=SEEDS[name][0], round_bf16=True, **na.FIX_BASE)


def wrapped(name, sched, dt, model=None):
    return rajni_amd.RAJNIViTWrapper(model if model is not None else model_of(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[attnpool] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |d| {err:.4g} vs scale {scale:.4g}"


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def traced_selections(w, P):
    """{block: keep_idx} of the last forward, each checked against the restated rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        s = t["scores"].float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(idx, npx.select_tokens(s, idx.shape[1] - P, P))
        assert np.array_equal(t["next_scores"].float().cpu().numpy(), np.take_along_axis(t["scores"].float().cpu().numpy(), idx, axis=1))
        forced[i] = idx
    return forced


# ---- 1. empty schedule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", na.MICRO)
def test_empty_schedule_equals_the_stock_forward(name, dt, B):
    """(The 625-token model in bf16 is the case that decides the tail's precision: with the B-row part of the tail in the model
    dtype it sat at 1.06e-2 / 1.25e-2 of the logit scale - five bf16 roundings of a pooled row at 2e-3 .. 4e-3 each, against
    logits the 625-token average makes small - which is why proj, the pool LayerNorm and the MLP run in fp32.)"""
    cfg, sd, iseed = fixture(name)
    imgs = na.images_of(cfg, B, iseed)
    with torch.no_grad():
        stock = model_of(name)(torch.from_numpy(imgs)).numpy()
    w = wrapped(name, {}, dt)
    d = w.check_supported()
    assert d["pool"] == "map" and d["num_prefix"] == cfg.num_prefix_tokens and w.importance_query == ("cls" if cfg.class_token else "mean")
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    assert got.shape == (B, cfg.num_classes) and w._plan[8][5] is not None and w._plan[2][4].pool == nat.POOL_MAP
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth
    close(got, stock, BAR[dt], f"{name} {dt} B={B} unpruned vs stock forward")
    if dt != "fp32":       # the 16-bit residual stream: the project's 2e-2 bar
        w.set_residual_dtype(TORCH[dt])
        close(w(x).float().cpu().numpy(), stock, 2e-2, f"{name} {dt} B={B} stream, unpruned")


# ---- 2. scheduled --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", na.MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt, B):
    cfg, sd, iseed = fixture(name)
    P = cfg.num_prefix_tokens
    imgs = na.images_of(cfg, B, iseed)
    want, counts, tr = yardstick(name, B)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, SCHED, P)
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(imgs).to(DEV)
    # the yardstick's selections injected
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, selections injected")
    # free-running: the device's selections are the rule on its own scores AND (short models) the restatement's, image for image
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w, P)
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    if name == LONG:
        want, _, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    else:
        for i in sorted(tr):
            np.testing.assert_array_equal(forced[i], tr[i]["keep_idx"], err_msg=f"{name} {dt} B={B} block {i}")
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, free-running")
    if dt != "fp32":
        w.set_residual_dtype(TORCH[dt])
        got = w(x).float().cpu().numpy()
        want_free, _, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=traced_selections(w, P))
        close(got, want_free, 2e-2, f"{name} {dt} B={B} pruned, free-running, 16-bit stream")


# ---- 3. headless: the pooled feature, as SigLIP ships ----------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64", "vit_micro_reg4_map_d80_patch16_64"])
def test_a_headless_model_returns_the_pooled_feature(name, dt):
    cfg, sd, iseed = fixture(name)
    B = 3
    want, counts, tr = yardstick(name, B, pooled=True)
    forced = {i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()}
    x = torch.from_numpy(na.images_of(cfg, B, iseed)).to(DEV)
    model = model_of(name)
    head = model.head
    model.head = nn.Identity()
    w = wrapped(name, SCHED, dt, model).force_keep_idx(forced)
    feat = w(x).clone()
    assert tuple(feat.shape) == (B, cfg.embed_dim) and feat.dtype == TORCH[dt] and w._plan[1].num_classes == 0 and not w._plan[1].head_w
    close(feat.float().cpu().numpy(), want, BAR[dt], f"{name} {dt} headless: the pooled feature")
    # ... and it is the row the head GEMM reads: the model's head on it, in fp64, against the logits of the model with its head
    logits = wrapped(name, SCHED, dt).force_keep_idx(forced)(x).float().cpu().numpy()
    by_hand = feat.double().cpu().numpy() @ head.weight.detach().double().numpy().T + head.bias.detach().double().numpy()
    u = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -20}[dt]      # one rounding of the logits (fp32: the GEMM's accumulation order)
    assert np.abs(logits - by_hand).max() <= 2 * u * np.abs(by_hand).max()


# ---- 4. the pool changes no token ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64", "vit_micro_reg4_map_d80_patch16_64"])
def test_feature_outputs_are_those_of_the_avg_pooled_twin(name, dt):
    """forward_features / forward_intermediates / get_intermediate_layers end in front of the pool: bit-equal to the same trunk
    wrapped with global_pool='avg' (fc_norm=False keeps the final norm), free-running on the same scores"""
    cfg, sd, iseed = fixture(name)
    twin = ts.VisionTransformer(dataclasses.replace(cfg, global_pool="avg", fc_norm=False)).eval()
    twin.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items() if not k.startswith("attn_pool.")}, strict=True)
    a, b = wrapped(name, SCHED, dt), wrapped(name, SCHED, dt, twin)
    assert a.check_supported()["pool"] == "map" and b.check_supported()["pool"] == "avg"
    x = torch.from_numpy(na.images_of(cfg, 3, iseed)).to(DEV)
    P, n0 = cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    for kw in (dict(), dict(dense=True), dict(dense=True, fill="last")):
        fa, fb = a.forward_features(x, **kw).clone(), b.forward_features(x, **kw).clone()
        assert same_bits(fa, fb), (name, dt, kw)
        assert torch.equal(a.get_last_stats()["source_idx"], b.get_last_stats()["source_idx"])
        assert tuple(fa.shape) == ((3, n0, cfg.embed_dim) if kw else (3, npx.token_counts(n0, cfg.depth, SCHED, P)[-1], cfg.embed_dim))
    (fa, ia), (fb, ib) = a.forward_intermediates(x, indices=[1, 3], output_fmt="NLC"), b.forward_intermediates(x, indices=[1, 3], output_fmt="NLC")
    assert same_bits(fa, fb) and all(same_bits(u, v) for u, v in zip(ia, ib))
    # the logits plan with slabs beside it: the pool's tail and the captures in one forward
    only = a.forward_intermediates(x, indices=[1, 3], output_fmt="NLC", intermediates_only=True)
    assert all(same_bits(u, v) for u, v in zip(only, ia))
    ga, gb = a.get_intermediate_layers(x, n=2, reshape=True), b.get_intermediate_layers(x, n=2, reshape=True)
    assert all(same_bits(u, v) for u, v in zip(ga, gb)) and tuple(ga[0].shape) == (3, cfg.embed_dim, 4, 4)
    # and the logits afterwards are the logits before: the feature plans share the packed weights and leave them alone
    first = a(x).clone()
    a.forward_features(x)
    assert same_bits(a(x), first)


def test_the_importance_query_setter_on_a_class_token_map_model():
    name, dt = "vit_micro_cls_map_patch16_64", "bf16"
    cfg, sd, iseed = fixture(name)
    imgs = na.images_of(cfg, 3, iseed)
    w = wrapped(name, SCHED, dt).set_importance_query("mean").trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w._plan[8][4] is not None and w._plan[8][5] is not None
    want, counts, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=traced_selections(w, 1), query="mean")
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} mean query")
    with pytest.raises(ValueError, match="no class token"):
        wrapped("vit_micro_map_patch16_64", SCHED, dt).set_importance_query("cls")


# ---- 5. any input size ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64"])
def test_a_rectangular_input_under_dynamic_img_size(name, dt):
    size = (48, 96)
    cfg, sd, iseed = fixture(name)
    imgs = na.images_of(cfg, 3, iseed, size)
    want, counts, tr = na.vit_forward_restated(ni.sd_at_grid(sd, cfg, (3, 6), dt=dt), imgs, SCHED, cfg)
    assert counts[0] == 18 + cfg.num_prefix_tokens
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(imgs).to(DEV)
    with pytest.raises(ValueError, match="set_dynamic_img_size"):
        w(x)
    w.set_dynamic_img_size().force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and w._plan[8][0] is not None and w._plan[8][5] is not None
    close(got, want, BAR[dt], f"{name} 48x96 {dt}, selections injected")
    assert np.array_equal(w(x).float().cpu().numpy(), got)


# ---- 6. fp8 weights --------------------------------------------------------------------------------------------------------------

def test_fp8_weights_leave_the_pool_in_the_model_dtype():
    """set_weight_format("fp8") on the fp8-capable dims: the restated graph on the dequantised block weights (the pool's and the
    head's as they are) with the device's selections, 1e-2 of the logit scale - the bar of the existing fp8 forward tests"""
    name = "vit_micro512_map_patch16_64"
    cfg, _, iseed = fixture(name)
    model = model_of(name)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = na.images_of(cfg, 6, iseed + 2)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w._weights["attn_pool"]["kv_w"].dtype == torch.bfloat16      # (the B-row matrices are fp32 copies of the bf16 values)
    assert all(w._weights["attn_pool"][k].dtype == torch.float32 for k in ("proj_w", "fc1_w", "fc2_w"))
    assert w._weights["blocks"][0]["qkv_w"].dtype == torch.uint8
    forced = traced_selections(w, 0)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, f"{name}, fp8 weights")
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.set_weight_format("fp8_mfma")


# ---- 7. a NULL record is the old forward ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64"])
def test_a_null_record_is_rajni_vit_forward_query(name, dt):
    cfg = ts.config_of(name)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(na.images_of(cfg, 5, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, keep, qry = w._plan[1], w._plan[2], w._plan[8][4]
    ext, pre = keep[4], keep[6]
    assert w._plan[8][5] is None
    ref = lambda r: C.byref(r) if r is not None else None
    lib = nat.lib()
    assert lib.rajni_vit_workspace_bytes_pool(C.byref(plan), ref(pre), None, ref(qry), None) == \
        lib.rajni_vit_workspace_bytes_query(C.byref(plan), ref(pre), None, ref(qry)) <= plan.workspace_bytes
    outs = []
    for fn, tail in ((lib.rajni_vit_forward_query, ()), (lib.rajni_vit_forward_pool, (None,))):
        out = torch.empty((5, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        nat.check(fn(C.byref(plan), ref(ext), ref(pre), None, None, ref(qry), *tail, x.data_ptr(), out.data_ptr(),
                     nat.stream_ptr(x.device)), "forward")
        torch.cuda.synchronize()
        outs.append(out[:, :plan.num_classes].contiguous())
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], plain.contiguous())


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------------

def test_cli_runs_a_map_model():
    from rajni_amd import run
    acc, thr = run.main(["--model", "vit_micro_map_patch16_64", "--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
    assert thr > 0 and 0.0 <= acc <= 100.0
