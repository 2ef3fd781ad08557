"""Whole forwards at token counts beyond one workgroup's LDS (the tiled score kernels inside the plan workspace) on the device.
GPU box only (`-m gpu`).

Yardstick as in tests/test_gpu_prefix_forward.py: tests/numerics_prefix.py::vit_forward_restated (torch fp64) with its selections
injected; free-running, the device's keep_idx must be exactly the restated rule applied to the device's own traced scores.  Bars are
the project's: 1e-2 x max|logit| for 16-bit models, 1e-3 for fp32, 2e-2 for a 16-bit residual stream.  The fixture is that file's
(seed 11, std 0.08, bias_std 0.1: the weight scale the bars are stated for)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_prefix as npx
import numerics_tiled as nt
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
LONG = ["vit_micro_patch16_400", "vit_micro_reg4_patch16_400"]
_CACHE = {}


def images_of(cfg, B, seed=5):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def fixture(name, B):
    """(cfg, state dict, images, the restated forward with its own selections): computed once per (config, B), never modified"""
    if (name, B) not in _CACHE:
        cfg = ts.CONFIGS[name]
        sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, **FIX))
        imgs = images_of(cfg, B)
        _CACHE[(name, B)] = (cfg, sd, imgs, npx.vit_forward_restated(sd, imgs, SCHED, cfg))
    return _CACHE[(name, B)]


def wrapper(name, dt, sched=SCHED):
    return rajni_amd.RAJNIViTWrapper(ts.create_model(ts.CONFIGS[name], round_bf16=True, **FIX), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[long] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"


def traced_selections(w, P):
    """{block: keep_idx} of the last forward, each checked against the restated rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        s = t["scores"].float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(idx, npx.select_tokens(s, idx.shape[1] - P, P))
        assert (idx[:, :P] == np.arange(P)).all()
        nxt = t["next_scores"].float().cpu().numpy()
        assert np.array_equal(nxt, np.take_along_axis(t["scores"].float().cpu().numpy(), idx, axis=1))
        forced[i] = idx
    return forced


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", LONG)
def test_long_pruned_forward_selection_conditional_and_free_running(name, dt, B):
    cfg, sd, imgs, (want, counts, tr) = fixture(name, B)
    P = 1 + cfg.reg_tokens
    n0 = cfg.num_patches + P
    assert n0 in (626, 630) and counts == npx.token_counts(n0, cfg.depth, SCHED, P)
    w = wrapper(name, dt)
    x = torch.from_numpy(imgs).to(DEV)
    # the yardstick's selections injected: the scores-only launch of the tiled kernels (block 1 recomputes, block 2 carries)
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, selections injected")
    # the plan's workspace is the query's, and the query holds the scratch of (B, n0, H, D)
    plan = w._plan[1]
    H, D = cfg.num_heads, cfg.embed_dim // cfg.num_heads
    assert plan.workspace_bytes >= nt.workspace_bytes(B, n0, H, D) == nat.lib().rajni_score_select_workspace_bytes(B, n0, H, D, plan.dtype)
    # free-running: the fused launch; the rule on the device's own scores, then the graph on those selections
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w, P)
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert s1.shape == (B, n0)
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    want_free, _, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    close(got, want_free, BAR[dt], f"{name} {dt} B={B} pruned, free-running")
    if dt != "fp32":
        w.set_residual_dtype(TORCH[dt])
        got = w(x).float().cpu().numpy()
        want_free, _, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=traced_selections(w, P))
        close(got, want_free, 2e-2, f"{name} {dt} B={B} pruned, free-running, 16-bit stream")


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_long_forward_sub_batches_reproduce_the_full_batch_bit_for_bit(dt):
    name = "vit_micro_reg4_patch16_400"
    cfg = ts.CONFIGS[name]
    w = wrapper(name, dt)
    x = torch.from_numpy(images_of(cfg, 4, seed=7)).to(DEV).to(TORCH[dt])
    full = w(x).clone()
    tc = w.get_last_stats()["token_counts"]
    for lo, hi in ((0, 1), (1, 4)):
        part = w(x[lo:hi].contiguous()).clone()
        assert w.get_last_stats()["token_counts"] == tc
        assert torch.equal(part.view(torch.uint8), full[lo:hi].contiguous().view(torch.uint8)), (lo, hi)


def test_vit_small_patch14_reg4_dinov2_at_its_pretrained_518():
    """1374 tokens: refused before the tiled path.  B = 1 in bf16, pruned: token counts, and every stage's selection the restated
    rule on the device's own scores"""
    name = "vit_small_patch14_reg4_dinov2_518"
    cfg = ts.CONFIGS[name]
    sched = {3: {"keep_ratio": 0.88}, 4: {"keep_ratio": 0.88}, 7: {"keep_ratio": 0.80}, 8: {"keep_ratio": 0.72}}
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(name, seed=3, std=0.04, bias_std=0.1, round_bf16=True), sched)
    w = w.to(DEV).to(torch.bfloat16).eval().trace_scores(True)
    x = torch.from_numpy(images_of(cfg, 1)).to(DEV)
    got = w(x).float().cpu().numpy()
    assert got.shape == (1, cfg.num_classes) and np.isfinite(got).all()
    assert w.get_last_stats()["token_counts"] == npx.token_counts(1374, 12, sched, 5)
    forced = traced_selections(w, 5)
    assert sorted(forced) == [3, 4, 7, 8] and forced[3].shape == (1, 5 + int(0.88 * 1369))
    again = w(x).float().cpu().numpy()
    assert np.array_equal(got, again)
