"""DeiT's distilled models (timm `VisionTransformerDistilled`: token order [cls, dist, patches], logits the average of `head` on
row 0 and `head_dist` on row 1) through the native forward.  GPU box only (`-m gpu`).

Yardsticks (the reference has no distilled models; never the code under test):
  empty schedule   the timm-shaped model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_distilled.py::vit_forward_restated (P = 2, the averaged heads), torch fp64 on the CPU, with its
                   selections injected (`force_keep_idx`); free-running, the device's keep_idx must be exactly the restated rule
                   applied to the device's own traced scores, and the graph is then evaluated on those selections.
Bars are tests/test_gpu_prefix_forward.py's: 1e-2 x max|logit| for bf16 and fp16 models, 1e-3 for fp32.
tests/test_distilled_cpu.py shows for every fixture here that `head` on the class row alone, and a stream without the dist row,
each move the logits by at least 5x the bar, and that the bf16 format's own cost on it leaves a quarter of the bar free
(tests/numerics_distilled.py: FIX, FORWARD_CASES - the forwards held to a bar are exactly those cases).  The restricted last
block (rows 0 and 1 only) must give the bytes of the all-rows form (rajni_debug_set_last_block_all_rows(1))."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_distilled as nd
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
P = 2
README_SCHEDULE = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
                   7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(config, fp32 state dict with bf16-representable values, stock model) - built once per config, never modified"""
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **nd.FIX[name])
    return cfg, ts.state_dict_numpy(model), model


@functools.lru_cache(maxsize=None)
def yardstick(name, sched, B, seed):
    """the restated graph of one fixture, free-running in fp64: computed once, shared by the dtypes"""
    cfg, sd, _ = fixture(name)
    return nd.vit_forward_restated(sd, nd.images_of(cfg, B, seed), nd.SCHEDULES[sched], cfg)


def wrapped(name, sched, dt, fix=None):
    return rajni_amd.RAJNIViTWrapper(ts.create_model(ts.CONFIGS[name], round_bf16=True, **(fix or nd.FIX[name])), sched) \
        .to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[distilled] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"


def traced_selections(w):
    """{block: keep_idx} of the last forward, each checked against the restated rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        s = t["scores"].float().cpu().numpy()
        np.testing.assert_array_equal(idx, nd.select_tokens(s.astype(np.float64), idx.shape[1] - P, P))
        assert (idx[:, :P] == np.arange(P)).all() and (idx[:, P:] >= P).all()
        assert np.array_equal(t["next_scores"].float().cpu().numpy(), np.take_along_axis(s, idx, axis=1))
        forced[i] = idx
    return forced


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- forward against the yardsticks -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", nd.MICRO)
def test_empty_schedule_equals_the_stock_forward(name, dt):
    cfg, sd, stock = fixture(name)
    assert ("unpruned", nd.BATCH, 2) in nd.FORWARD_CASES
    imgs = nd.images_of(cfg, nd.BATCH)
    w = wrapped(name, {}, dt)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + 2] * cfg.depth == [18] * 4
    with torch.no_grad():
        want = stock(torch.from_numpy(imgs)).numpy()
    close(got, want, nd.BAR[dt], f"{name} {dt} B={nd.BATCH} unpruned vs stock forward")
    close(got, yardstick(name, "unpruned", nd.BATCH, 2)[0], nd.BAR[dt], f"{name} {dt} B={nd.BATCH} unpruned vs restated graph")


@pytest.mark.parametrize("sched", ["carried", "last"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", nd.MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt, sched):
    cfg, sd, _ = fixture(name)
    schedule = nd.SCHEDULES[sched]
    assert (sched, nd.BATCH, 5) in nd.FORWARD_CASES
    imgs = nd.images_of(cfg, nd.BATCH, seed=5)
    want, counts, tr = yardstick(name, sched, nd.BATCH, 5)
    assert counts == nd.token_counts(18, cfg.depth, schedule, P)
    w = wrapped(name, schedule, dt)
    x = torch.from_numpy(imgs).to(DEV)
    # the yardstick's selections injected
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    for i, t in w.get_last_trace().items():
        assert tuple(t["keep_idx"].shape) == tuple(t["next_scores"].shape) == tr[i]["keep_idx"].shape
    close(got, want, nd.BAR[dt], f"{name} {dt} {sched}, selections injected")
    # free-running: the rule on the device's own scores, then the graph on those selections
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w)
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    if dt == "fp32":
        # the yardstick's own selections, exactly, as far as its margins allow: block by block while the gap between the last
        # kept and the first dropped patch score exceeds the fp32 score bar (2 x 1e-3 of the score scale) in every image
        for i in sorted(forced):
            s = np.sort(tr[i]["scores"][:, P:], axis=1)[:, ::-1]
            k = forced[i].shape[1] - P
            if k < s.shape[1] and (s[:, k - 1] - s[:, k]).min() <= 2e-3 * np.abs(tr[i]["scores"]).max():
                break
            np.testing.assert_array_equal(forced[i], tr[i]["keep_idx"])
    want_free, _, _ = nd.vit_forward_restated(sd, imgs, schedule, cfg, forced_keep=forced)
    close(got, want_free, nd.BAR[dt], f"{name} {dt} {sched}, free-running")


# ---- the last block on rows 0 and 1 -------------------------------------------------------------------------------------------

def _eligible(w):
    plan, keep = w._plan[1], w._plan[2]
    ext, pre = keep[4], keep[6]
    assert pre is not None and pre.head_rows == 2 and pre.num_prefix == 2
    return nat.lib().rajni_debug_last_block_cls_rows(C.byref(plan), C.byref(ext) if ext is not None else None, C.byref(pre))


@pytest.mark.parametrize("B", [1, 3, 130])       # 130: 2B = 260 rows cross a 256-row GEMM tile
@pytest.mark.parametrize("name, dt", [(nd.MICRO[0], "bf16"), (nd.MICRO[1], "bf16"), (nd.MICRO[0], "fp32")])
def test_two_row_last_block_gives_the_bytes_of_all_rows(name, dt, B):
    cfg, _, _ = fixture(name)
    lib = nat.lib()
    x = torch.from_numpy(nd.images_of(cfg, B, seed=7)).to(DEV).to(TORCH[dt])
    for sched, eligible in (("unpruned", 1), ("carried", 1), ("last", 0)):
        w = wrapped(name, nd.SCHEDULES[sched], dt)
        try:
            rows = w(x).clone()
            assert _eligible(w) == eligible, sched
            counts = w.get_last_stats()["token_counts"]
            lib.rajni_debug_set_last_block_all_rows(1)
            assert _eligible(w) == 0
            full = w(x).clone()
        finally:
            lib.rajni_debug_set_last_block_all_rows(0)
        assert w.get_last_stats()["token_counts"] == counts
        assert torch.isfinite(rows.float()).all()
        assert same_bytes(rows, full), f"{name} {dt} B={B} {sched}: the two-row last block and the all-rows form differ"


@pytest.mark.parametrize("name, dt", [(nd.MICRO[0], "bf16"), (nd.MICRO[1], "fp16"), (nd.MICRO[0], "fp32")])
def test_an_image_does_not_depend_on_its_batch(name, dt):
    cfg, _, _ = fixture(name)
    x = torch.from_numpy(nd.images_of(cfg, 3, seed=8)).to(DEV).to(TORCH[dt])
    for sched in ("carried", "last"):
        w = wrapped(name, nd.SCHEDULES[sched], dt)
        full = w(x).clone()
        for b in range(3):
            assert same_bytes(w(x[b:b + 1].contiguous()), full[b:b + 1]), (name, dt, sched, b)


# ---- fp8 weights ----------------------------------------------------------------------------------------------------------------

def test_fp8_weights():
    """set_weight_format("fp8"): the restated graph on the DEQUANTISED weights with the device's selections, 1e-2 of the logit
    scale (tests/test_gpu_fp8.py's rule: the quantisation error itself is not part of the parity budget)"""
    name = nd.MICRO[1]
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **nd.FIX[name])
    w = rajni_amd.RAJNIViTWrapper(model, nd.SCHEDULES["carried"]).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    assert ("carried", nd.BATCH, 9) in nd.FORWARD_CASES
    imgs = nd.images_of(cfg, nd.BATCH, seed=9)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    a, b, need = nd.feature_matters(sd, imgs, nd.SCHEDULES["carried"], cfg, 1e-2)
    assert a >= need and b >= need
    want, counts, _ = nd.vit_forward_restated(sd, imgs, nd.SCHEDULES["carried"], cfg, forced_keep=forced)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, f"{name}, fp8 weights")
    assert (got.argmax(1) == want.argmax(1)).all()


# ---- DeiT-tiny distilled at 224 -------------------------------------------------------------------------------------------------

def test_deit_tiny_distilled_patch16_224():
    """B = 2 in bf16, README schedule, free-running against the restated graph (fp32 on the CPU) on the device's selections"""
    name = "deit_tiny_distilled_patch16_224"
    fix = dict(seed=3, std=0.04, bias_std=0.1)       # the full-size fixture of tests/test_gpu_prefix_forward.py
    cfg = ts.CONFIGS[name]
    sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, **fix))
    imgs = nd.images_of(cfg, 2)
    w = wrapped(name, README_SCHEDULE, "bf16", fix).trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w)
    want, counts, _ = nd.vit_forward_restated(sd, imgs, README_SCHEDULE, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts == nd.token_counts(198, 12, README_SCHEDULE, P)
    assert _eligible(w) == 1
    cls_only, _, _ = nd.vit_forward_restated(sd, imgs, README_SCHEDULE, cfg, forced_keep=forced, dtype=torch.float32, head="cls")
    moved = float(np.abs(want - cls_only).max())
    print(f"[distilled] {name}: head on the class row alone moves the logits by {moved:.4g} (scale {np.abs(want).max():.4g})")
    assert moved >= 5e-2 * np.abs(want).max()
    close(got, want, 1e-2, f"{name} README schedule, free-running")


# ---- models without a dist token: nothing changes ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_head_rows_0_and_1_are_the_forward_as_it_was(name):
    """a prefix record with head_rows = 0 and one with head_rows = 1 give the bytes of the entry point the wrapper takes today:
    rajni_vit_forward with no record (CLS only) / the record as it was (reg4)"""
    cfg = ts.CONFIGS[name]
    sched = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, seed=11, std=0.08, bias_std=0.1), sched) \
        .to(DEV).to(torch.bfloat16).eval()
    x = torch.from_numpy(nd.images_of(cfg, 7)).to(DEV).to(torch.bfloat16)
    plain = w(x).clone()
    plan, keep = w._plan[1], w._plan[2]
    pre0 = keep[6]
    assert keep[4] is None and (pre0 is None) == (name == "vit_micro_patch16_64")
    assert pre0 is None or pre0.head_rows == 0
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    ws0 = lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), C.byref(pre0) if pre0 is not None else None)
    outs = []
    for hr in (0, 1):
        pre = nat.VitPrefix()
        if pre0 is not None:
            pre.num_prefix, pre.reg_token = pre0.num_prefix, pre0.reg_token
        pre.head_rows = hr
        assert lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), C.byref(pre)) == ws0 == plan.workspace_bytes
        out = torch.empty((7, plan.logits_ld), dtype=torch.bfloat16, device=DEV)
        for i in range(cfg.depth):
            keep[1][i] = -1
        nat.check(lib.rajni_vit_forward_ext_prefix(C.byref(plan), None, C.byref(pre), x.data_ptr(), out.data_ptr(),
                                                   nat.stream_ptr(x.device)), "rajni_vit_forward_ext_prefix")
        torch.cuda.synchronize()
        assert [int(keep[1][i]) for i in range(cfg.depth)] == counts
        outs.append(out[:, :plan.num_classes].contiguous())
    assert same_bytes(outs[0], outs[1]) and same_bytes(outs[0], plain.contiguous())
