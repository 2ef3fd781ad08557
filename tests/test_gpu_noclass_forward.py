"""Whole forwards of models without a class token (timm `class_token=False, global_pool='avg'`; P = R >= 0 prefix tokens, the
mean importance query) and of the mean query on a class-token model, on the device.  GPU box only (`-m gpu`).

Yardsticks (the reference cannot run such a model):
  empty schedule   the timm-shaped model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_noclass.py::vit_forward_restated, torch fp64: its selections injected (`force_keep_idx`), and
                   free-running, where the device's selections must BE the restatement's - the fixtures' seeds
                   (numerics_noclass.SEEDS) leave every boundary gap at 16 .. 28 x the bf16 score budget, so no image is excused
                   for a near-tie (tests/test_noclass_cpu.py asserts at least 8 x).
Bars are those of tests/test_gpu_prefix_forward.py for the class-token twins: 1e-2 x max|logit| for 16-bit models, 1e-3 for fp32,
2e-2 for a 16-bit residual stream; feature outputs at max(bar, 1.5 x d16) like tests/test_gpu_features.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_image as ni
import numerics_noclass as nq
import numerics_prefix as npx
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
SCHED = nq.SCHED
MICRO = ["vit_micro_nocls_gap_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64", "vit_micro_reg1_nocls_gap_d80_patch16_64"]
REG4 = "vit_micro_reg4_nocls_gap_patch16_64"


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(config, fp32 state dict with bf16-representable values, image seed) - built once, never modified"""
    cfg = ts.config_of(name)
    wseed, iseed = nq.SEEDS[name]
    return cfg, ts.state_dict_numpy(ts.create_model(cfg, seed=wseed, round_bf16=True, **nq.FIX_BASE)), iseed


@functools.lru_cache(maxsize=None)
def yardstick(name, B, query="mean"):
    """the restated graph, free-running in fp64: computed once per (model, batch)"""
    cfg, sd, iseed = fixture(name)
    return nq.vit_forward_restated(sd, nq.images_of(cfg, B, iseed), SCHED, cfg, query=query)


def model_of(name):
    return ts.create_model(ts.config_of(name), seed=nq.SEEDS[name][0], round_bf16=True, **nq.FIX_BASE)


def wrapped(name, sched, dt):
    return rajni_amd.RAJNIViTWrapper(model_of(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[noclass] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
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
@pytest.mark.parametrize("name", MICRO)
def test_empty_schedule_equals_the_stock_forward(name, dt, B):
    cfg, sd, iseed = fixture(name)
    imgs = nq.images_of(cfg, B, iseed)
    with torch.no_grad():
        stock = model_of(name)(torch.from_numpy(imgs)).numpy()
    w = wrapped(name, {}, dt)
    assert w.importance_query == "mean" and w.check_supported()["num_prefix"] == cfg.reg_tokens
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + cfg.reg_tokens] * cfg.depth
    close(got, stock, BAR[dt], f"{name} {dt} B={B} unpruned vs stock forward")
    if dt != "fp32":       # the 16-bit residual stream: the project's 2e-2 bar
        w.set_residual_dtype(TORCH[dt])
        close(w(x).float().cpu().numpy(), stock, 2e-2, f"{name} {dt} B={B} stream, unpruned")


# ---- 2. scheduled --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt, B):
    cfg, sd, iseed = fixture(name)
    P = cfg.reg_tokens
    want, counts, tr = yardstick(name, B)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, SCHED, P)
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(nq.images_of(cfg, B, iseed)).to(DEV)
    # the yardstick's selections injected
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    for i, t in w.get_last_trace().items():
        assert tuple(t["keep_idx"].shape) == tuple(t["next_scores"].shape) == tr[i]["keep_idx"].shape
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, selections injected")
    # free-running: the device's selections are the rule on its own scores AND the restatement's, image for image
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w, P)
    for i in sorted(tr):
        np.testing.assert_array_equal(forced[i], tr[i]["keep_idx"], err_msg=f"{name} {dt} B={B} block {i}")
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, free-running")
    if dt != "fp32":
        w.set_residual_dtype(TORCH[dt])
        got = w(x).float().cpu().numpy()
        want_free, _, _ = nq.vit_forward_restated(sd, nq.images_of(cfg, B, iseed), SCHED, cfg, forced_keep=traced_selections(w, P))
        close(got, want_free, 2e-2, f"{name} {dt} B={B} pruned, free-running, 16-bit stream")


def test_forced_selection_must_keep_the_register_slots():
    cfg, sd, iseed = fixture(REG4)
    _, _, tr = yardstick(REG4, 3)
    w = wrapped(REG4, SCHED, "bf16")
    x = torch.from_numpy(nq.images_of(cfg, 3, iseed)).to(DEV)
    bad = {i: torch.from_numpy(t["keep_idx"].copy()) for i, t in tr.items()}
    bad[1][0, 2] = 3
    w.force_keep_idx(bad)
    with pytest.raises(ValueError, match="prefix tokens"):
        w(x)


# ---- 3. sub-batches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sub_batches_reproduce_the_full_batch_bit_for_bit(dt):
    for name in MICRO:
        cfg, _, iseed = fixture(name)
        w = wrapped(name, SCHED, dt)
        x = torch.from_numpy(nq.images_of(cfg, 9, iseed + 1)).to(DEV).to(TORCH[dt])
        full = w(x).clone()
        tc = w.get_last_stats()["token_counts"]
        for lo, hi in ((0, 1), (3, 5), (2, 9)):
            part = w(x[lo:hi].contiguous()).clone()
            assert w.get_last_stats()["token_counts"] == tc
            assert same_bits(part, full[lo:hi].contiguous()), (name, lo, hi)


# ---- 4. a NULL / {1, CLS} record is the old forward ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64"])
def test_a_null_or_class_query_record_is_the_old_forward(name, dt):
    cfg = ts.CONFIGS[name]
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(nq.images_of(cfg, 7, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, keep = w._plan[1], w._plan[2]
    ext = keep[4]
    assert keep[6] is None and w._plan[8][4] is None and (ext is None) == (name == "vit_micro_patch16_64")
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    for q in (None, nat.VitQuery(1, nat.QUERY_CLS)):
        qp = C.byref(q) if q is not None else None
        assert lib.rajni_vit_workspace_bytes_query(C.byref(plan), None, None, qp) == lib.rajni_vit_workspace_bytes(C.byref(plan))
        for img in (None, nat.VitImage(64, 64)):
            out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
            for i in range(cfg.depth):
                keep[1][i] = -1
            nat.check(lib.rajni_vit_forward_query(C.byref(plan), C.byref(ext) if ext is not None else None, None, None,
                                                  C.byref(img) if img is not None else None, qp, x.data_ptr(), out.data_ptr(),
                                                  nat.stream_ptr(x.device)), "rajni_vit_forward_query")
            torch.cuda.synchronize()
            assert same_bits(out[:, :plan.num_classes].contiguous(), plain.contiguous())
            assert [int(keep[1][i]) for i in range(cfg.depth)] == counts
    # and the setter's "cls" on a class-token model changes nothing
    assert same_bits(w.set_importance_query("cls")(x), plain) and w._plan[8][4] is None


# ---- 5. the mean query on a class-token model ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_the_mean_query_on_an_avg_pooled_class_token_model(dt):
    name = "vit_micro_gap_patch16_64"
    cfg, sd, iseed = fixture(name)
    want, counts, tr = yardstick(name, 3, "mean")
    want_cls, _, tr_cls = yardstick(name, 3, "cls")
    assert any(not np.array_equal(tr[i]["keep_idx"], tr_cls[i]["keep_idx"]) for i in tr), "the two queries select the same tokens here"
    w = wrapped(name, SCHED, dt).set_importance_query("mean").trace_scores(True)
    x = torch.from_numpy(nq.images_of(cfg, 3, iseed)).to(DEV)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and w._plan[8][4] is not None
    forced = traced_selections(w, 1)
    for i in sorted(tr):
        np.testing.assert_array_equal(forced[i], tr[i]["keep_idx"])
    close(got, want, BAR[dt], f"{name} {dt} mean query, free-running")
    got_cls = w.set_importance_query("cls")(x).float().cpu().numpy()
    want_c, _, _ = nq.vit_forward_restated(sd, nq.images_of(cfg, 3, iseed), SCHED, cfg, forced_keep=traced_selections(w, 1), query="cls")
    close(got_cls, want_c, BAR[dt], f"{name} {dt} class query again")


# ---- 6. feature outputs on the R = 4 model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_feature_outputs_with_registers_and_no_class_token(dt):
    cfg, sd, iseed = fixture(REG4)
    B, P, n0, Cd = 3, 4, 20, cfg.embed_dim
    imgs = nq.images_of(cfg, B, iseed)
    caps = (1, 3)
    want = nq.feature_outputs(sd, imgs, SCHED, cfg, caps=caps)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU (tests/test_gpu_features.py's rule)
        r16 = nq.feature_outputs(sd, imgs, SCHED, cfg, forced_keep=forced, caps=caps, dtype=TORCH[dt])
        d16 = max(float(np.abs(r16[k] - want[k]).max() / np.abs(want[k]).max()) for k in ("tokens", "dense_last"))
        d16 = max([d16] + [float(np.abs(r16["slabs"][c] - want["slabs"][c]).max() / np.abs(want["slabs"][c]).max()) for c in caps])
        print(f"[noclass] {REG4} {dt}: d16 {d16:.3g}")
        bar = max(bar, 1.5 * d16)
    w = wrapped(REG4, SCHED, dt)
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(imgs).to(DEV)
    tokens = w.forward_features(x).clone()
    src = w.get_last_stats()["source_idx"]
    np.testing.assert_array_equal(src.cpu().numpy(), want["source_idx"])
    assert w.get_last_stats()["token_counts"] == want["counts"] and tuple(tokens.shape) == (B, want["counts"][-1], Cd)
    close(tokens.float().cpu().numpy(), want["tokens"], bar, f"{REG4} {dt} tokens")
    # dense: the tokens' bits at their source rows, zero bytes elsewhere
    dense = w.forward_features(x, dense=True).clone()
    assert tuple(dense.shape) == (B, n0, Cd)
    assert same_bits(torch.gather(dense, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    mask = torch.ones((B, n0), dtype=torch.bool, device=DEV).scatter_(1, src.long(), False)
    assert int(mask.sum()) == B * (n0 - tokens.shape[1]) and not dense[mask].contiguous().view(torch.uint8).any()
    close(dense.float().cpu().numpy(), want["dense"], bar, f"{REG4} {dt} dense")
    # fill="last": the survivors' bits again, every pruned position holding the state it left with; exit_block
    last = w.forward_features(x, dense=True, fill="last").clone()
    stats = w.get_last_stats()
    np.testing.assert_array_equal(stats["exit_block"].cpu().numpy(), want["exit_block"])
    np.testing.assert_array_equal(stats["source_idx"].cpu().numpy(), want["source_idx"])
    assert same_bits(torch.gather(last, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    assert not torch.isnan(last.float()).any() and bool((last[mask].float().abs().amax(dim=-1) > 0).all())
    close(last.float().cpu().numpy(), want["dense_last"], bar, f"{REG4} {dt} dense, fill=last")
    # forward_intermediates([1, 3]): the slabs of the unpruned grid, prefix rows apart
    final, inter = w.forward_intermediates(x, indices=[1, 3], output_fmt="NLC", return_prefix_tokens=True)
    assert same_bits(final, dense)
    np.testing.assert_array_equal(w.get_last_stats()["exit_block"].cpu().numpy(), want["exit_block"])
    for c, (spatial, prefix) in zip(caps, inter):
        assert tuple(spatial.shape) == (B, 16, Cd) and tuple(prefix.shape) == (B, P, Cd)
        slab = torch.cat([prefix, spatial], 1).float().cpu().numpy()
        close(slab, want["slabs"][c], bar, f"{REG4} {dt} intermediate of block {c}")
        alive = want["exit_block"] > c
        assert not slab[~alive].any() and alive[:, :P].all()
    nchw = w.forward_intermediates(x, indices=[3], intermediates_only=True)[0]
    assert tuple(nchw.shape) == (B, Cd, 4, 4)
    assert same_bits(nchw.permute(0, 2, 3, 1).reshape(B, 16, Cd), inter[1][0])


def test_the_fc_norm_models_refuse_forward_features_as_their_class_token_twins_do():
    w = wrapped("vit_micro_nocls_gap_patch16_64", SCHED, "bf16")
    x = torch.zeros(2, 3, 64, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
        w.forward_features(x)
    inter = w.forward_intermediates(x, indices=[3], norm=False, intermediates_only=True, output_fmt="NLC")
    assert tuple(inter[0].shape) == (2, 16, 128)


# ---- 7. any input size ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_dynamic_img_size_without_prefix_tokens(dt):
    name, size = "vit_micro_nocls_gap_patch16_64", (48, 96)
    cfg, sd, iseed = fixture(name)
    imgs = nq.images_of(cfg, 3, iseed, size)
    want, counts, tr = nq.vit_forward_restated(ni.sd_at_grid(sd, cfg, (3, 6), dt=dt), imgs, SCHED, cfg)
    assert counts[0] == 18
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(imgs).to(DEV)
    with pytest.raises(ValueError, match="set_dynamic_img_size"):
        w(x)
    w.set_dynamic_img_size().force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} 48x96 {dt}, selections injected")
    assert np.array_equal(w(x).float().cpu().numpy(), got)
    # the transposed grid is another answer, many bars away
    wrong, _, _ = nq.vit_forward_restated(ni.sd_at_grid(sd, cfg, (3, 6), how="transposed", dt=dt), imgs, SCHED, cfg,
                                          forced_keep={i: t["keep_idx"] for i, t in tr.items()})
    print(f"[noclass] 48x96: the transposed grid moves the logits by {np.abs(wrong - want).max() / np.abs(want).max():.3g}")


# ---- 8. fp8 weights --------------------------------------------------------------------------------------------------------------

def test_fp8_weights_with_registers_and_no_class_token():
    """set_weight_format("fp8"): the restated graph on the dequantised weights with the device's selections, 1e-2 of the logit
    scale (tests/test_gpu_prefix_forward.py::test_fp8_weights_with_registers)"""
    cfg, _, iseed = fixture(REG4)
    model = model_of(REG4)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = nq.images_of(cfg, 6, iseed + 2)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, 4)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = nq.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, f"{REG4}, fp8 weights")
    assert (got.argmax(1) == want.argmax(1)).all()
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.set_weight_format("fp8_mfma")(torch.from_numpy(imgs).to(DEV))


# ---- 9. the CLI and the module ----------------------------------------------------------------------------------------------------

def test_cli_runs_a_model_without_a_class_token():
    from rajni_amd import run
    acc, thr = run.main(["--model", REG4, "--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
    assert thr > 0 and 0.0 <= acc <= 100.0
    acc, thr = run.main(["--model", "vit_micro_gap_patch16_64", "--batch_size", "8", "--max_batches", "2", "--warmup", "1",
                         "--synthetic", "--importance_query", "mean"])
    assert thr > 0 and 0.0 <= acc <= 100.0
    with pytest.raises(ValueError, match="no class token"):
        run.main(["--model", REG4, "--batch_size", "8", "--max_batches", "1", "--warmup", "0", "--synthetic", "--importance_query", "cls"])


def test_module_level_attention_without_a_class_token():
    """RAJNIAttention.forward stand-alone as the wrapper configures it: R = 4 registers kept, the mean query, then a carried
    stage (select-only) with P = 0 through rajni_select_topk_query"""
    from rajni_amd.wrapper import RAJNIAttention
    cfg, sd, _ = fixture(REG4)
    att = RAJNIAttention(model_of(REG4).blocks[0].attn, keep_ratio=0.7, update=True).to(DEV).to(torch.bfloat16)
    xn = ts.bf16_round_np(np.random.default_rng(4).standard_normal((3, 20, 128), dtype=np.float32))
    t = lambda n: torch.from_numpy(sd["blocks.0.attn." + n]).double()
    qkv = (torch.from_numpy(xn).double() @ t("qkv.weight").T + t("qkv.bias")).numpy()
    for P in (4, 0):
        att.num_prefix_tokens, att.importance_query, att.update = P, "mean", True
        out, keep_idx, nxt = att(torch.from_numpy(xn).to(DEV).to(torch.bfloat16))
        keep = npx.keep_count(0.7, 20, P)
        assert tuple(out.shape) == (3, P + keep, 128) and tuple(keep_idx.shape) == tuple(nxt.shape) == (3, P + keep)
        ki = keep_idx.cpu().numpy()
        assert (ki[:, :P] == np.arange(P)).all() and (np.diff(ki, axis=1) > 0).all()
        want_nxt = np.take_along_axis(nq.importance_scores(qkv, 2, query="mean"), ki, axis=1)
        assert np.abs(nxt.float().cpu().numpy() - want_nxt).max() <= 1e-2 * np.abs(want_nxt).max()
        att.update = False
        out2, ki2, nxt2 = att(torch.from_numpy(xn).to(DEV).to(torch.bfloat16)[:, :P + keep].contiguous(), prev_scores=nxt)
        keep2 = npx.keep_count(0.7, P + keep, P)
        np.testing.assert_array_equal(ki2.cpu().numpy(), npx.select_tokens(nxt.float().cpu().numpy(), keep2, P))
