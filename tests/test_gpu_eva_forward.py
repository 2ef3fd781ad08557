"""Whole forwards of models with a norm inside the MLP and timm Eva's block layout (include/rajni_hip_mlpnorm.h), RAJNIViTWrapper
-> C ABI, on the device.  GPU box only (`-m gpu`).

Yardstick (the reference has neither): tests/numerics_eva.py::vit_forward_restated, torch fp64 - its selections injected
(`force_keep_idx`), and free-running, where the device's selections must be the restatement's wherever the restated score gap at
the cut exceeds the score budget (the fixtures' seeds leave every gap at 8 budgets or more; tests/test_eva_cpu.py asserts that,
and that each live mutant of the restated forward lies at least its bar away on every fixture used here).  Bars are the
project's: 1e-2 x max|out| for 16-bit models, 1e-3 for fp32; feature outputs at max(bar, 1.5 x d16) like
tests/test_gpu_features.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_eva as ne
import numerics_noclass as nq
import numerics_prefix as npx
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = ne.BAR
B = ne.BATCH
EVA, H342, RMS_GAP, MLPNORM, D40 = ne.MICRO


def wrapped(name, sched, dt):
    return rajni_amd.RAJNIViTWrapper(ne.build_model(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[eva] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
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
    return wm._native_call(wm._FORWARDS, e.refs.ext, e.refs.pre, None, e.input.img, e.input.qry, e.input.apr, e.input.nrm, e.input.rop,
                           e.input.mln[0] if e.input.mln else None)[0]


def force(w, tr):
    return w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})


def assert_selections_equal_the_references(name, sched, got, dt):
    """the device's keep_idx equals the restatement's for every image and block (the fixtures leave every restated gap at the cut
    at GAP_FACTOR score budgets of bf16 or more - held here again in the model dtype's budget, so no case is skipped)"""
    cfg = ne.fixture(name)[0]
    sd, imgs, tables, _ = ne.case(name, sched)
    _, _, tr = ne.vit_forward_restated(sd, imgs, ne.SCHEDULES[sched], cfg, tables, budget_dt=dt)
    P, skipped = cfg.num_prefix_tokens, 0
    for i, t in tr.items():
        s, keep = t["scores"], t["keep_idx"].shape[1] - P
        for b in range(s.shape[0]):
            order = np.argsort(-s[b, P:], kind="stable") + P
            lo, hi = order[keep - 1], order[keep]
            if s[b, lo] - s[b, hi] > max(t["budget"][b, lo], t["budget"][b, hi]):
                np.testing.assert_array_equal(got[i][b], t["keep_idx"][b], err_msg=f"{name} {dt} block {i} image {b}")
            else:
                skipped += 1
    assert skipped <= ne.MAX_SKIPPED


# ---- 1. the five micro configs under both schedules, selections injected and free-running ------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("sched", ["SCHED", "CARRIED"])
@pytest.mark.parametrize("name", ne.MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, sched, dt):
    cfg = ne.fixture(name)[0]
    P = cfg.num_prefix_tokens
    sd, imgs, tables, (want, counts, tr) = ne.case(name, sched)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, ne.SCHEDULES[sched], P)
    w = wrapped(name, ne.SCHEDULES[sched], dt)
    x = torch.from_numpy(imgs).to(DEV)
    got = force(w, tr)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_mlpnorm"
    assert w._plan.input.mln[0].n == cfg.hidden_dim and w._plan.plan.hidden == (cfg.hidden_dim + 63) // 64 * 64
    close(got, want, BAR[dt], f"{name} {sched} {dt} pruned, selections injected")
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    assert_selections_equal_the_references(name, sched, traced_selections(w, P), dt)
    close(got, want, BAR[dt], f"{name} {sched} {dt} pruned, free-running")


def test_unpruned_forward_equals_the_stock_module():
    for name in ne.MICRO:
        cfg, _, iseed, _ = ne.fixture(name)
        imgs = ne.images_of(cfg, B, iseed)
        with torch.no_grad():
            stock = ne.build_model(name)(torch.from_numpy(imgs)).numpy()
        w = wrapped(name, {}, "fp32")
        got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
        close(got, stock, BAR["fp32"], f"{name} fp32 unpruned vs the stock forward")


# ---- 2. fp8 block weights --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [EVA, H342])
def test_fp8_weights(name):
    # the weights the kernels see are the dequantised ones: the yardstick runs on THAT state dict.  The quantisation is part of
    # the model here, so what is left for the device is the format's share of the bf16 bar and no more
    cfg, _, iseed, tables = ne.fixture(name)
    model = ne.build_model(name)
    w = rajni_amd.RAJNIViTWrapper(model, ne.SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = ne.images_of(cfg, B, iseed)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, cfg.num_prefix_tokens)
    sd = ts.state_dict_numpy(model)
    deq = {k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()}
    assert set(deq) <= set(sd)
    sd.update(deq)
    want, counts, _ = ne.vit_forward_restated(sd, imgs, ne.SCHED, cfg, tables, forced_keep=forced)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, ne.FORMAT_HEADROOM * BAR["bf16"], f"{name}, fp8 weights")
    with pytest.raises(NotImplementedError, match="mlp.norm|rotary"):
        w.set_weight_format("fp8_mfma")


# ---- 3. feature outputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_feature_outputs(dt):
    name = EVA
    cfg, sd, iseed, tables = ne.fixture(name)
    P, Cd, n0 = cfg.num_prefix_tokens, cfg.embed_dim, cfg.num_patches + cfg.num_prefix_tokens
    imgs = ne.images_of(cfg, B, iseed)
    caps = (1, 2, 3)
    want = ne.feature_outputs(sd, imgs, ne.SCHED, cfg, tables, caps=caps)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU (tests/test_gpu_features.py's rule)
        r16 = ne.feature_outputs(sd, imgs, ne.SCHED, cfg, tables, forced_keep=forced, caps=caps, dtype=TORCH[dt])
        d16 = max(float(np.abs(r16[k] - want[k]).max() / np.abs(want[k]).max()) for k in ("tokens", "dense_last"))
        d16 = max([d16] + [float(np.abs(r16["slabs"][c] - want["slabs"][c]).max() / np.abs(want["slabs"][c]).max()) for c in caps])
        print(f"[eva] {name} {dt}: d16 {d16:.3g}")
        bar = max(bar, 1.5 * d16)
    w = wrapped(name, ne.SCHED, dt)
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
    final, inter = w.forward_intermediates(x, indices=list(caps), output_fmt="NLC", norm=False, fill="last", return_prefix_tokens=True)
    assert same_bits(final, last)
    for c, (spatial, prefix) in zip(caps, inter):
        slab = torch.cat([prefix, spatial], 1).float().cpu().numpy()
        alive = want["exit_block"] > c
        close(slab[alive], want["slabs"][c][alive], bar, f"{name} {dt} intermediate of block {c}")


# ---- 4. any input size -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_dynamic_img_size(dt):
    name, size = EVA, (48, 96)
    sd, imgs, tables, (want, counts, tr) = ne.case(name, "SCHED", size, pos_dt=dt)
    assert counts[0] == 19 and tables.shape[0] == 18
    w = force(wrapped(name, ne.SCHED, dt).set_dynamic_img_size(), tr)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_mlpnorm"
    close(got, want, BAR[dt], f"{name} 48x96 {dt}, selections injected")


# ---- 5. the last block on the head's rows only -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", [EVA, H342, MLPNORM])
def test_last_block_on_the_heads_rows_is_bit_identical_to_all_rows(name, dt):
    # the norm inside the MLP then runs on the B class rows alone: a row's bits do not depend on the rows beside it
    sd, imgs, tables, (want, counts, tr) = ne.case(name)
    w = force(wrapped(name, ne.SCHED, dt), tr)
    x = torch.from_numpy(imgs).to(DEV)
    rows = w(x).clone()
    plan = (C.byref(w._plan.plan), C.byref(w._plan.refs.ext) if w._plan.refs.ext is not None else None, None)
    assert nat.lib().rajni_debug_last_block_cls_rows(*plan) == 1
    try:
        nat.lib().rajni_debug_set_last_block_all_rows(1)
        every = w(x).clone()
    finally:
        nat.lib().rajni_debug_set_last_block_all_rows(0)
    assert same_bits(rows, every)
    close(rows.float().cpu().numpy(), want, BAR[dt], f"{name} {dt}, last block on the class rows")


# ---- 6. a NULL / all-zero record is the old forward ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_rope_patch16_64"])
def test_a_null_or_zero_record_is_the_old_forward(name, dt):
    cfg = ts.config_of(name)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), nq.SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(nq.images_of(cfg, 7, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, refs, inp = w._plan.plan, w._plan.refs, w._plan.input
    ext = C.byref(refs.ext) if refs.ext is not None else None
    rop = C.byref(inp.rop) if inp.rop is not None else None
    assert inp.mln is None and entry_symbol(w) in ("rajni_vit_forward", "rajni_vit_forward_rope")
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    s = nat.stream_ptr(x.device)
    ref = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
    nat.check(lib.rajni_vit_forward_rope(C.byref(plan), ext, None, None, None, None, None, None, rop, x.data_ptr(), ref.data_ptr(), s),
              "rajni_vit_forward_rope")
    for r in (None, nat.VitMlpNorm()):
        rp = C.byref(r) if r is not None else None
        assert lib.rajni_vit_workspace_bytes_mlpnorm(C.byref(plan), None, None, None, None, None, rop, rp) == \
            lib.rajni_vit_workspace_bytes_rope(C.byref(plan), None, None, None, None, None, rop)
        out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        for i in range(cfg.depth):
            refs.tc[i] = -1
        nat.check(lib.rajni_vit_forward_mlpnorm(C.byref(plan), ext, None, None, None, None, None, None, rop, rp, x.data_ptr(),
                                                out.data_ptr(), s), "rajni_vit_forward_mlpnorm")
        torch.cuda.synchronize()
        assert same_bits(out[:, :plan.num_classes], ref[:, :plan.num_classes]) and same_bits(out[:, :plan.num_classes], plain)
        assert [int(refs.tc[i]) for i in range(cfg.depth)] == counts


# ---- 7. the checkpoints' dimensions ------------------------------------------------------------------------------------------------

def test_eva02_large_dims_agree_with_the_restated_forward():
    # EVA02-L's MLP: 2730 columns, six chunks per lane and a partial last one, 2752 in the buffer.  Two blocks of it at 56 px
    # (17 tokens) keep the test at a second: the width is what this is about
    cfg = ts.EvaViTConfig(**{**ts.config_of("eva02_large_patch14_224").to_dict(), "depth": 2, "img_size": 56, "num_classes": 10})
    model = ts.create_model(cfg, seed=3, round_bf16=True, **ne.FIX_BASE)
    sched = {1: {"keep_ratio": 0.5, "update": True}}
    imgs = ne.images_of(cfg, 2, 7)
    sd, tables = ts.state_dict_numpy(model), ne.tables_of(model)
    want, counts, tr = ne.vit_forward_restated(sd, imgs, sched, cfg, tables)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    # no seed was searched for these dims: the 16-bit bar is tests/test_gpu_features.py's rule, max(bar, 1.5 x what the same graph
    # costs in the model's 16-bit dtype on the CPU)
    r16, _, _ = ne.vit_forward_restated(sd, imgs, sched, cfg, tables, forced_keep=forced, dtype=torch.bfloat16)
    d16 = float(np.abs(r16 - want).max() / np.abs(want).max())
    print(f"[eva] EVA02-L dims: d16 {d16:.3g}")
    for dt, bar in (("bf16", max(BAR["bf16"], 1.5 * d16)), ("fp32", BAR["fp32"])):
        w = force(rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(TORCH[dt]).eval(), tr)
        got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
        assert w._plan.input.mln[0].n == 2730 and w._plan.plan.hidden == 2752 and w.get_last_stats()["token_counts"] == counts
        close(got, want, bar, f"EVA02-L dims, 2 blocks, {dt}")


def test_cli_runs_an_eva_micro_model():
    from rajni_amd import run
    acc, thr = run.main(["--model", EVA, "--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
    assert thr > 0 and 0.0 <= acc <= 100.0
