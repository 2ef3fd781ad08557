"""Whole forwards of models with rotary position embeddings (include/rajni_hip_rope.h), RAJNIViTWrapper -> C ABI, on the device.
GPU box only (`-m gpu`).

Yardstick (the reference has no RoPE): tests/numerics_rope.py::vit_forward_restated, torch fp64, with the rotation at each
token's source position - its selections injected (`force_keep_idx`), and free-running, where the device's selections must be
the restatement's wherever the restated score gap at the cut exceeds the score budget (the fixtures' seeds leave every gap at
8 budgets or more; tests/test_rope_cpu.py asserts that, and that each mutant of the restated forward - no rotation, stream
positions, rotated prefix rows, rotated v, the other layout, the flipped sign - lies at least 4 bars away on every fixture used
here).  Bars are those of tests/test_gpu_rmsnorm_forward.py: 1e-2 x max|out| for 16-bit models, 1e-3 for fp32; feature outputs at
max(bar, 1.5 x d16) like tests/test_gpu_features.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_noclass as nq
import numerics_prefix as npx
import numerics_rope as nrp
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = nrp.BAR
B = nrp.BATCH
PLAIN, HALF_REG4, MIXED_GAP, D40 = nrp.MICRO


def wrapped(name, sched, dt):
    return rajni_amd.RAJNIViTWrapper(nrp.build_model(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[rope] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
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
        forced[i] = idx
    return forced


def entry_symbol(w):
    from rajni_amd.wrapper import model as wm
    e = w._plan
    return wm._native_call(wm._FORWARDS, e.refs.ext, e.refs.pre, None, e.input.img, e.input.qry, e.input.apr, e.input.nrm, e.input.rop)[0]


def force(w, tr):
    return w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})


def assert_selections_where_the_gap_is_clear(name, sched, got, dt):
    """the device's keep_idx equals the restatement's for every image and block whose restated score gap at the cut exceeds the
    score budget of the model dtype (a nearer tie may legitimately fall either way)"""
    cfg = nrp.fixture(name)[0]
    sd, imgs, tables, _ = nrp.case(name, sched)
    _, _, tr = nrp.vit_forward_restated(sd, imgs, nrp.SCHEDULES[sched], cfg, tables, budget_dt=dt)
    P, checked = cfg.num_prefix_tokens, 0
    for i, t in tr.items():
        s, keep = t["scores"], t["keep_idx"].shape[1] - P
        for b in range(s.shape[0]):
            order = np.argsort(-s[b, P:], kind="stable") + P
            lo, hi = order[keep - 1], order[keep]
            if s[b, lo] - s[b, hi] > max(t["budget"][b, lo], t["budget"][b, hi]):
                np.testing.assert_array_equal(got[i][b], t["keep_idx"][b], err_msg=f"{name} {dt} block {i} image {b}")
                checked += 1
    assert checked > 0


# ---- 1. the four micro configs, selections injected and free-running -------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", nrp.MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt):
    cfg = nrp.fixture(name)[0]
    P = cfg.num_prefix_tokens
    sd, imgs, tables, (want, counts, tr) = nrp.case(name)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, nrp.SCHED, P)
    w = wrapped(name, nrp.SCHED, dt)
    x = torch.from_numpy(imgs).to(DEV)
    got = force(w, tr)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_rope"
    close(got, want, BAR[dt], f"{name} {dt} pruned, selections injected")
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    assert_selections_where_the_gap_is_clear(name, "SCHED", traced_selections(w, P), dt)
    close(got, want, BAR[dt], f"{name} {dt} pruned, free-running")


def test_unpruned_forward_equals_the_stock_module():
    # no schedule: the position is the row index throughout, and the yardstick is the timm-shaped module's own forward
    for name in nrp.MICRO:
        cfg, _, iseed, _ = nrp.fixture(name)
        imgs = nrp.images_of(cfg, B, iseed)
        with torch.no_grad():
            stock = nrp.build_model(name)(torch.from_numpy(imgs)).numpy()
        w = wrapped(name, {}, "fp32")
        got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
        close(got, stock, BAR["fp32"], f"{name} fp32 unpruned vs the stock forward")


# ---- 2. carried scores ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_a_stage_that_carries_its_scores(dt):
    name = PLAIN
    cfg = nrp.fixture(name)[0]
    sd, imgs, tables, (want, counts, tr) = nrp.case(name, "CARRIED")
    w = wrapped(name, nrp.CARRIED, dt).trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    assert_selections_where_the_gap_is_clear(name, "CARRIED", traced_selections(w, 1), dt)
    close(got, want, BAR[dt], f"{name} {dt} update=False in block 2, free-running")


# ---- 3. the last-block forms ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["cls_rows", "cls_only", "all_rows", "no_class_token"])
def test_each_last_block_form(form):
    name = MIXED_GAP if form == "no_class_token" else PLAIN
    sd, imgs, tables, (want, counts, tr) = nrp.case(name)
    w = force(wrapped(name, nrp.SCHED, "bf16"), tr)
    x = torch.from_numpy(imgs).to(DEV)
    if form == "cls_only":
        w.set_last_block_cls_only(True)
    plan = lambda: (C.byref(w._plan.plan), C.byref(w._plan.refs.ext) if w._plan.refs.ext is not None else None, None)
    try:
        if form == "all_rows":
            nat.lib().rajni_debug_set_last_block_all_rows(1)
        got = w(x).float().cpu().numpy()
    finally:
        nat.lib().rajni_debug_set_last_block_all_rows(0)
    if form in ("cls_rows", "all_rows"):      # the default runs the last block on the B class rows; the hook had run every row
        assert nat.lib().rajni_debug_last_block_cls_rows(*plan()) == 1
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR["bf16"], f"{name} bf16, last block: {form}")


# ---- 4. the other users of the source map --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_feature_outputs_share_no_buffer_with_the_rotation(dt):
    name = HALF_REG4
    cfg, sd, iseed, tables = nrp.fixture(name)
    P, Cd, n0 = cfg.num_prefix_tokens, cfg.embed_dim, cfg.num_patches + cfg.num_prefix_tokens
    imgs = nrp.images_of(cfg, B, iseed)
    caps = (1, 2, 3)
    want = nrp.feature_outputs(sd, imgs, nrp.SCHED, cfg, tables, caps=caps)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU (tests/test_gpu_features.py's rule)
        r16 = nrp.feature_outputs(sd, imgs, nrp.SCHED, cfg, tables, forced_keep=forced, caps=caps, dtype=TORCH[dt])
        d16 = max(float(np.abs(r16[k] - want[k]).max() / np.abs(want[k]).max()) for k in ("tokens", "dense_last"))
        d16 = max([d16] + [float(np.abs(r16["slabs"][c] - want["slabs"][c]).max() / np.abs(want["slabs"][c]).max()) for c in caps])
        print(f"[rope] {name} {dt}: d16 {d16:.3g}")
        bar = max(bar, 1.5 * d16)
    w = wrapped(name, nrp.SCHED, dt)
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(imgs).to(DEV)
    tokens = w.forward_features(x).clone()
    src = w.get_last_stats()["source_idx"]
    np.testing.assert_array_equal(src.cpu().numpy(), want["source_idx"])
    close(tokens.float().cpu().numpy(), want["tokens"], bar, f"{name} {dt} tokens")
    last = w.forward_features(x, dense=True, fill="last").clone()
    np.testing.assert_array_equal(w.get_last_stats()["exit_block"].cpu().numpy(), want["exit_block"])
    assert tuple(last.shape) == (B, n0, Cd)
    assert same_bits(torch.gather(last, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    close(last.float().cpu().numpy(), want["dense_last"], bar, f"{name} {dt} dense, fill=last")
    # a capture behind every scheduled block, with fill = last: the slabs' map and the dropped rows' map are written between the
    # rotations of consecutive blocks
    final, inter = w.forward_intermediates(x, indices=list(caps), output_fmt="NLC", norm=False, fill="last", return_prefix_tokens=True)
    assert same_bits(final, last)
    for c, (spatial, prefix) in zip(caps, inter):
        slab = torch.cat([prefix, spatial], 1).float().cpu().numpy()
        alive = want["exit_block"] > c
        close(slab[alive], want["slabs"][c][alive], bar, f"{name} {dt} intermediate of block {c}")
    # ... and the logits of the same wrapper afterwards are still the forward's
    logits, _, _ = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, tables, forced_keep=forced)
    close(w(x).float().cpu().numpy(), logits, BAR[dt], f"{name} {dt} logits behind the feature calls")


# ---- 5. tables per grid --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_dynamic_img_size_fetches_the_tables_of_the_grid(dt):
    name, size = PLAIN, (48, 96)
    sd, imgs, tables, (want, counts, tr) = nrp.case(name, "SCHED", size, pos_dt=dt)
    assert counts[0] == 19 and tables.shape[0] == 18
    w = force(wrapped(name, nrp.SCHED, dt).set_dynamic_img_size(), tr)
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_rope"
    close(got, want, BAR[dt], f"{name} 48x96 {dt}, selections injected")
    # the square input afterwards takes the model's own table again
    sd, imgs, tables, (want, counts, tr) = nrp.case(name)
    got = force(w, tr)(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    close(got, want, BAR[dt], f"{name} 64x64 {dt} behind 48x96")


def test_a_cached_plan_owns_the_tables_it_points_to():
    # nine grids through a cache of eight: the plan of the first grid (batch 2) outlives that grid's cache entry, is replayed, and
    # must still point to live tables - the pair it holds itself - and give the bits a fresh wrapper gives
    name = PLAIN
    cfg, _, iseed, _ = nrp.fixture(name)
    w = wrapped(name, nrp.SCHED, "bf16").set_dynamic_img_size()
    img = lambda b, hw: torch.from_numpy(nrp.images_of(cfg, b, iseed, hw)).to(DEV)
    grids = [(64, 64)] + [(32, 16 * k) for k in range(2, 9)]
    w(img(1, grids[0]))
    for hw in grids[1:]:
        w(img(1, hw))
    first = w(img(2, grids[0])).clone()
    held = w._plan
    w(img(1, (48, 96)))                                   # the ninth grid evicts the first grid's cache entry
    again = w(img(2, grids[0])).clone()
    assert w._plan is held
    for e in w._plans.values():
        assert (e.input.rop.cos, e.input.rop.sin) == (e.input.rot[0].data_ptr(), e.input.rot[1].data_ptr())
    assert len(held.refs.W["rope_cache"]) == 8 and not any(t is held.input.rot[0] for t, _ in held.refs.W["rope_cache"].values())
    fresh = wrapped(name, nrp.SCHED, "bf16").set_dynamic_img_size()(img(2, grids[0]))
    assert same_bits(first, again) and same_bits(again, fresh)


# ---- 6. fp8 weights ------------------------------------------------------------------------------------------------------------

def test_fp8_weights_on_a_rope_model():
    # the fixture's own images and batch (the case tests/test_rope_cpu.py holds the mutants to); the weights the kernels see are
    # the dequantised ones, so the mutants' margins are asserted on THAT state dict too, before anything is compared
    name = PLAIN
    cfg, _, iseed, tables = nrp.fixture(name)
    model = nrp.build_model(name)
    w = rajni_amd.RAJNIViTWrapper(model, nrp.SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = nrp.images_of(cfg, B, iseed)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, 1)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, tables, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    want64, _, _ = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, tables, forced_keep=forced)
    for mut in nrp.MUTANTS:
        other, _, _ = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, tables, forced_keep=forced, mutant=mut)
        sep = float(np.abs(want64 - other).max() / np.abs(want64).max())
        print(f"[rope] {name}, fp8 weights: mutant {mut} {sep:.3g}")
        assert sep >= nrp.MUTANT_FACTOR * 1e-2, f"mutant {mut} moves the fp8 fixture's logits by {sep:.3g} only"
    close(got, want, 1e-2, f"{name}, fp8 weights")
    with pytest.raises(NotImplementedError, match="rotary"):
        w.set_weight_format("fp8_mfma")


# ---- 7. a NULL / all-zero record is the old forward ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64"])
def test_a_null_or_zero_record_is_the_old_forward(name, dt):
    cfg = ts.CONFIGS[name]
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), nq.SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(nq.images_of(cfg, 7, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, refs = w._plan.plan, w._plan.refs
    ext = C.byref(refs.ext) if refs.ext is not None else None
    assert w._plan.input.rop is None and entry_symbol(w) in ("rajni_vit_forward", "rajni_vit_forward_ext")
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    s = nat.stream_ptr(x.device)
    ref = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
    nat.check(lib.rajni_vit_forward_norm(C.byref(plan), ext, None, None, None, None, None, None, x.data_ptr(), ref.data_ptr(), s),
              "rajni_vit_forward_norm")
    for r in (None, nat.VitRope()):
        rp = C.byref(r) if r is not None else None
        assert lib.rajni_vit_workspace_bytes_rope(C.byref(plan), None, None, None, None, None, rp) == lib.rajni_vit_workspace_bytes(C.byref(plan))
        out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        for i in range(cfg.depth):
            refs.tc[i] = -1
        nat.check(lib.rajni_vit_forward_rope(C.byref(plan), ext, None, None, None, None, None, None, rp, x.data_ptr(), out.data_ptr(), s),
                  "rajni_vit_forward_rope")
        torch.cuda.synchronize()
        assert same_bits(out[:, :plan.num_classes], ref[:, :plan.num_classes]) and same_bits(out[:, :plan.num_classes], plain)
        assert [int(refs.tc[i]) for i in range(cfg.depth)] == counts


def test_cli_runs_a_rope_micro_model():
    from rajni_amd import run
    acc, thr = run.main(["--model", HALF_REG4, "--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
    assert thr > 0 and 0.0 <= acc <= 100.0
