"""Whole forwards of models with a relative position bias (include/rajni_hip_relpos.h), RAJNIViTWrapper -> C ABI, on the device.
GPU box only (`-m gpu`).

Yardstick (the reference has no such model): tests/numerics_relpos.py::vit_forward_restated, torch fp64, with the bias looked up
at each token's place in the image and the class row's bias in the importance score (B11) - its selections injected
(`force_keep_idx`), and free-running, where the device's selections must be the restatement's wherever the restated score gap at
the cut exceeds the score budget (the fixtures' seeds leave every gap at 8 budgets or more and keep the fp32 restatement on the
fp64 one's selections; tests/test_relpos_cpu.py asserts that, and that every live mutant lies at least 4 bars away).  Bars are
tests/numerics_rope.py's: 1e-2 x max|out| for 16-bit models, 1e-3 for fp32; feature outputs at max(bar, 1.5 x d16) like
tests/test_gpu_features.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_prefix as npx
import numerics_relpos as nrp
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper import model as wm

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = nrp.BAR
B = nrp.BATCH
BEIT, SHARED, RELPOS, RECT = nrp.MICRO


def wrapped(name, sched, dt):
    return rajni_amd.RAJNIViTWrapper(nrp.build_model(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[relpos] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |d| {err:.4g} vs scale {scale:.4g}"


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def traced_selections(w, P):
    """{block: keep_idx} of the last forward, each checked against the selection rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        s = t["scores"].float().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(idx, npx.select_tokens(s, idx.shape[1] - P, P))
        forced[i] = idx
    return forced


def entry_symbol(w):
    e = w._plan
    return wm._native_call(wm._FORWARDS, e.refs.ext, e.refs.pre, None, e.input.img, e.input.qry, e.input.apr, e.input.nrm, e.input.rop,
                           e.input.mln[0] if e.input.mln else None, e.input.rel)[0]


def force(w, tr):
    return w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})


def assert_selections_where_the_gap_is_clear(name, sched, got, dt):
    cfg = nrp.fixture(name)[0]
    sd, imgs, _ = nrp.case(name, sched)
    _, _, tr = nrp.vit_forward_restated(sd, imgs, nrp.SCHEDULES[sched], cfg, budget_dt=dt)
    P, checked = cfg.num_prefix_tokens, 0
    for i, t in tr.items():
        s, keep = t["scores"], t["keep_idx"].shape[1] - P
        for b in range(s.shape[0]):
            order = np.argsort(-s[b, P:], kind="stable") + P
            lo, hi = order[keep - 1], order[keep]
            if s[b, lo] - s[b, hi] > max(t["budget"][b, lo], t["budget"][b, hi]):
                np.testing.assert_array_equal(got[i][b], t["keep_idx"][b], err_msg=f"{name} {dt} block {i} image {b}")
                checked += 1
    assert checked == len(tr) * s.shape[0]          # the seeds leave no image out


# ---- 1. the four micro configs, selections injected and free-running -------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("sched", ["SCHED", "CARRIED"])
@pytest.mark.parametrize("name", nrp.MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, sched, dt):
    cfg = nrp.fixture(name)[0]
    sd, imgs, (want, counts, tr) = nrp.case(name, sched)
    assert counts == npx.token_counts(cfg.num_patches + 1, cfg.depth, nrp.SCHEDULES[sched], 1)
    w = wrapped(name, nrp.SCHEDULES[sched], dt)
    x = torch.from_numpy(imgs).to(DEV)
    got = force(w, tr)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_relpos"
    assert w._plan.input.rel.block_stride == (0 if cfg.rel_pos == "beit_shared" else 2 * nrp.table_size(*cfg.grid))
    close(got, want, BAR[dt], f"{name} {sched} {dt} pruned, selections injected")
    # the device closer to the truth than to every live mutant (each under the forward's own selections)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    err = float(np.abs(got - want).max())
    for mut in nrp.MUTANTS:
        if nrp.vacuous(cfg, mut) or mut == "score_without_bias":
            continue
        other = nrp.vit_forward_restated(sd, imgs, nrp.SCHEDULES[sched], cfg, forced_keep=forced, mutant=mut)[0]
        assert err < float(np.abs(got - other).max()), mut
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    sel = traced_selections(w, 1)
    assert_selections_where_the_gap_is_clear(name, sched, sel, dt)
    close(got, want, BAR[dt], f"{name} {sched} {dt} pruned, free-running")
    if not nrp.vacuous(cfg, "score_without_bias"):      # ... and that mutant changes a selection the device does not change
        other, _, tro = nrp.vit_forward_restated(sd, imgs, nrp.SCHEDULES[sched], cfg, mutant="score_without_bias")
        assert any(not np.array_equal(tro[i]["keep_idx"], sel[i]) for i in sel)
        assert float(np.abs(got - want).max()) < float(np.abs(got - other).max())


def test_unpruned_forward_equals_the_stock_module():
    # no schedule: the position is the row index throughout, and the yardstick is the timm-shaped module's own forward
    for name in nrp.MICRO:
        cfg, _, iseed = nrp.fixture(name)
        imgs = nrp.images_of(cfg, B, iseed)
        with torch.no_grad():
            stock = nrp.build_model(name)(torch.from_numpy(imgs)).numpy()
        w = wrapped(name, {}, "fp32")
        got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
        assert entry_symbol(w) == "rajni_vit_forward_relpos"
        close(got, stock, BAR["fp32"], f"{name} fp32 unpruned vs the stock forward")


def test_a_changed_table_is_repacked():
    name = SHARED
    cfg, _, iseed = nrp.fixture(name)
    x = torch.from_numpy(nrp.images_of(cfg, B, iseed)).to(DEV)
    w = wrapped(name, {}, "fp32")
    a = w(x).clone()
    with torch.no_grad():
        w.m.rel_pos_bias.relative_position_bias_table.mul_(0.5)
    b = w(x).clone()                                # the same wrapper: the fingerprint of the parameters re-packs the table
    with torch.no_grad():
        stock = w.m(x).float()
    assert not torch.equal(a, b)
    close(b.float().cpu().numpy(), stock.cpu().numpy(), BAR["fp32"], f"{name} fp32 behind an in-place change of the table")


# ---- 2. the last block's row reduction -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_last_block_row_reduction_is_bit_identical_to_all_rows(dt):
    name = RELPOS                                   # a class-token head: the last block runs on the B class rows
    sd, imgs, (want, counts, tr) = nrp.case(name)
    w = force(wrapped(name, nrp.SCHED, dt), tr)
    x = torch.from_numpy(imgs).to(DEV)
    reduced = w(x).clone()
    plan = (C.byref(w._plan.plan), C.byref(w._plan.refs.ext) if w._plan.refs.ext is not None else None, None)
    assert nat.lib().rajni_debug_last_block_cls_rows(*plan) == 1
    try:
        nat.lib().rajni_debug_set_last_block_all_rows(1)
        full = w(x).clone()
    finally:
        nat.lib().rajni_debug_set_last_block_all_rows(0)
    assert same_bits(reduced, full)
    close(reduced.float().cpu().numpy(), want, BAR[dt], f"{name} {dt}, last block on the class rows")


# ---- 3. feature outputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_feature_outputs(dt):
    name = RELPOS                                   # (the BEiT layout has no final norm: forward_features refuses every fc_norm model)
    cfg, sd, iseed = nrp.fixture(name)
    Cd, n0 = cfg.embed_dim, cfg.num_patches + 1
    imgs = nrp.images_of(cfg, B, iseed)
    caps = (1, 2, 3)
    want = nrp.feature_outputs(sd, imgs, nrp.SCHED, cfg, caps=caps)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU (tests/test_gpu_features.py's rule)
        r16 = nrp.feature_outputs(sd, imgs, nrp.SCHED, cfg, forced_keep=forced, caps=caps, dtype=TORCH[dt])
        d16 = max(float(np.abs(r16[k] - want[k]).max() / np.abs(want[k]).max()) for k in ("tokens", "dense", "dense_last"))
        d16 = max([d16] + [float(np.abs(r16["slabs"][c] - want["slabs"][c]).max() / np.abs(want["slabs"][c]).max()) for c in caps])
        print(f"[relpos] {name} {dt}: d16 {d16:.3g}")
        bar = max(bar, 1.5 * d16)
    w = wrapped(name, nrp.SCHED, dt)
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(imgs).to(DEV)
    tokens = w.forward_features(x).clone()
    src = w.get_last_stats()["source_idx"]
    np.testing.assert_array_equal(src.cpu().numpy(), want["source_idx"])
    close(tokens.float().cpu().numpy(), want["tokens"], bar, f"{name} {dt} tokens")
    dense = w.forward_features(x, dense=True).clone()
    close(dense.float().cpu().numpy(), want["dense"], bar, f"{name} {dt} dense")
    last = w.forward_features(x, dense=True, fill="last").clone()
    assert tuple(last.shape) == (B, n0, Cd)
    assert same_bits(torch.gather(last, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    close(last.float().cpu().numpy(), want["dense_last"], bar, f"{name} {dt} dense, fill=last")
    final, inter = w.forward_intermediates(x, indices=list(caps), output_fmt="NLC", norm=False, fill="last", return_prefix_tokens=True)
    assert same_bits(final, last)
    kept = {c: np.zeros((B, n0), bool) for c in caps}
    for c in caps:
        np.put_along_axis(kept[c], wm_source(want, c, n0), True, axis=1)
    for c, (spatial, prefix) in zip(caps, inter):
        slab = torch.cat([prefix, spatial], 1).float().cpu().numpy()
        close(slab[kept[c]], want["slabs"][c][kept[c]], bar, f"{name} {dt} intermediate of block {c}")
    logits = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, forced_keep=forced)[0]
    close(w(x).float().cpu().numpy(), logits, BAR[dt], f"{name} {dt} logits behind the feature calls")


def wm_source(want, c, n0):
    """[B, Nc] the places of the rows alive behind block c"""
    import numerics_noclass as nq
    return nq.source_idx(want["trace"], want["tokens"].shape[0], n0, upto=c)


# ---- 4. fp8 weights ------------------------------------------------------------------------------------------------------------

def test_fp8_weights_on_a_bias_model():
    # the weights the kernels see are the dequantised ones, so the mutants' margins are asserted on THAT state dict too, and the
    # bf16 format's own cost on it is held to FORMAT_HEADROOM of the bar before anything is compared
    name = BEIT
    cfg, _, iseed = nrp.fixture(name)
    model = nrp.build_model(name)
    w = rajni_amd.RAJNIViTWrapper(model, nrp.SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = nrp.images_of(cfg, B, iseed)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, 1)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    want64 = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, forced_keep=forced)[0]
    r16 = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, forced_keep=forced, dtype=torch.bfloat16)[0]
    f = float(np.abs(r16 - want64).max() / np.abs(want64).max())
    print(f"[relpos] {name}, fp8 weights: bf16 format cost {f:.3g}")
    assert f <= nrp.FORMAT_HEADROOM * BAR["bf16"]
    for mut in nrp.MUTANTS:
        if nrp.vacuous(cfg, mut) or mut == "score_without_bias":
            continue
        other = nrp.vit_forward_restated(sd, imgs, nrp.SCHED, cfg, forced_keep=forced, mutant=mut)[0]
        sep = float(np.abs(want64 - other).max() / np.abs(want64).max())
        assert sep >= nrp.MUTANT_FACTOR * BAR["bf16"], f"mutant {mut} moves the fp8 fixture's logits by {sep:.3g} only"
    close(got, want, BAR["bf16"], f"{name}, fp8 weights")


# ---- 5. a NULL / all-zero record is the old forward ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_eva_patch16_64"])
def test_a_null_or_zero_record_is_rajni_vit_forward_mlpnorm(name, dt):
    import numerics_noclass as nq
    cfg = ts.config_of(name)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), nq.SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(nq.images_of(cfg, 7, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    e = w._plan
    plan, refs = e.plan, e.refs
    ref = lambda r: C.byref(r) if r is not None else None
    recs = (ref(refs.ext), ref(refs.pre), None, ref(e.input.img), ref(e.input.qry), ref(e.input.apr), ref(e.input.nrm), ref(e.input.rop),
            ref(e.input.mln[0]) if e.input.mln else None)
    assert e.input.rel is None
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    s = nat.stream_ptr(x.device)
    old = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
    nat.check(lib.rajni_vit_forward_mlpnorm(C.byref(plan), *recs, x.data_ptr(), old.data_ptr(), s), "rajni_vit_forward_mlpnorm")
    sized = (recs[1],) + recs[3:]
    for r in (None, nat.VitRelPos()):
        assert lib.rajni_vit_workspace_bytes_relpos(C.byref(plan), *sized, ref(r)) == lib.rajni_vit_workspace_bytes_mlpnorm(C.byref(plan), *sized)
        out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        for i in range(cfg.depth):
            refs.tc[i] = -1
        nat.check(lib.rajni_vit_forward_relpos(C.byref(plan), *recs, ref(r), x.data_ptr(), out.data_ptr(), s), "rajni_vit_forward_relpos")
        torch.cuda.synchronize()
        assert same_bits(out[:, :plan.num_classes], old[:, :plan.num_classes]) and same_bits(out[:, :plan.num_classes], plain)
        assert [int(refs.tc[i]) for i in range(cfg.depth)] == counts


# ---- 6. the checkpoints' dimensions ------------------------------------------------------------------------------------------------

README_SCHEDULE = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
                   7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}


def test_a_beit_base_sized_forward():
    # BEiT-B/16 at 224 px, batch 8, the README schedule: it runs, the token counts are exact, and the logits are within the bar of
    # the fp32 restated graph under the device's own selections (each checked against the rule on the device's scores).
    # Weights at timm's scale (std 0.02, the tables at 1): no seed was searched at these dimensions
    cfg = ts.config_of("beit_base_patch16_224")
    model = ts.create_model(cfg, seed=5, std=0.02, bias_std=0.02, round_bf16=True)
    imgs = nrp.images_of(cfg, 8, 9)
    sd = ts.state_dict_numpy(model)
    w = rajni_amd.RAJNIViTWrapper(model, README_SCHEDULE).to(DEV).to(torch.bfloat16).eval().trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [197, 197, 197, 197, 173, 152, 152, 152, 121, 87, 87, 87]
    assert entry_symbol(w) == "rajni_vit_forward_relpos" and w._plan.input.rel.gh == 14
    want = nrp.vit_forward_restated(sd, imgs, README_SCHEDULE, cfg, forced_keep=traced_selections(w, 1), dtype=torch.float32)[0]
    close(got, want, BAR["bf16"], "BEiT-B/16 dims, bf16, batch 8, README schedule")


def test_cli_runs_the_micro_models():
    from rajni_amd import run
    for extra in (["--model", BEIT], ["--model", RECT, "--img_size", "48", "96"]):
        acc, thr = run.main(extra + ["--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
        assert thr > 0 and 0.0 <= acc <= 100.0
