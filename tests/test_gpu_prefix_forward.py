"""Whole forwards of models with register tokens (P = 1 + R prefix tokens; timm `reg_tokens=R`) on the device.  GPU box only (`-m gpu`).

Yardsticks (the reference concatenates cls_token only and slices [:, 1:], so it is not one):
  empty schedule   the base model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_prefix.py::vit_forward_restated, torch fp64, with its selections injected (`force_keep_idx`);
                   free-running, the device's keep_idx must be exactly the restated rule applied to the device's own traced scores.
Bars are the project's: 1e-2 x max|logit| for 16-bit models, 1e-3 for fp32, 2e-2 for a 16-bit residual stream.  Before a case is
accepted the same graph shows on the CPU that ignoring the registers (the same patch selections, register rows removed) moves the
fp32 logits by at least 5x the bar."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_prefix as npx
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
MICRO = ["vit_micro_reg4_patch16_64", "deit3_micro_reg4_patch16_64", "vit_micro_reg1_gap_patch14_56"]
# One register in front of an 'avg' pool is a weak signal (the mean over the patch rows dilutes it): with the project's fixture
# seed it moves the fp32 logits by 4.6 - 12.7x the 1e-2 bar on the CPU, under the 5x this file demands of a fixture.  That config
# therefore draws the same distribution (std 0.08, bias_std 0.1: the weight scale the project's 1e-2 bar is stated for - bf16
# error grows with the weight scale, with or without registers) from another seed: 6.9 - 12.5x over B = 1, 3, pruned and
# unpruned (CPU, fp32; the check runs again in every test).
FIX_OF = {"vit_micro_reg1_gap_patch14_56": dict(seed=12, std=0.08, bias_std=0.1)}


def images_of(cfg, B, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def build(name, sched, dt, fix=None):
    fix = fix or FIX_OF.get(name, FIX)
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **fix)
    sd = ts.state_dict_numpy(model)

    def stock(x):                 # the base model's own forward: fp32, CPU, bf16-representable weights
        with torch.no_grad():
            return model(torch.from_numpy(x)).numpy()

    wrapped = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, **fix), sched).to(DEV).to(TORCH[dt]).eval()
    return (cfg, sd, stock), wrapped


def assert_fixture_can_tell(cfg, sd, imgs, sched, bar):
    moved, need = npx.registers_matter(sd, imgs, sched, cfg, bar)
    assert moved >= need, f"ignoring the registers moves the logits by only {moved:.4g} (need {need:.4g})"


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[prefix] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
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


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MICRO)
def test_empty_schedule_equals_the_stock_forward(name, dt, B):
    (cfg, sd, stock), w = build(name, {}, dt)
    imgs = images_of(cfg, B)
    assert_fixture_can_tell(cfg, sd, imgs, {}, BAR[dt])
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + 1 + cfg.reg_tokens] * cfg.depth
    close(got, stock(imgs), BAR[dt], f"{name} {dt} B={B} unpruned vs stock forward")
    if dt != "fp32":       # the 16-bit residual stream: the project's 2e-2 bar
        w.set_residual_dtype(TORCH[dt])
        close(w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy(), stock(imgs), 2e-2, f"{name} {dt} B={B} stream, unpruned")


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt, B):
    (cfg, sd, _), w = build(name, SCHED, dt)
    P = 1 + cfg.reg_tokens
    imgs = images_of(cfg, B, seed=5)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED, BAR[dt])
    want, counts, tr = npx.vit_forward_restated(sd, imgs, SCHED, cfg)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, SCHED, P)
    x = torch.from_numpy(imgs).to(DEV)
    # the yardstick's selections injected
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    for i, t in w.get_last_trace().items():
        assert tuple(t["keep_idx"].shape) == tuple(t["next_scores"].shape) == tr[i]["keep_idx"].shape
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, selections injected")
    # free-running: the rule on the device's own scores, then the graph on those selections
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w, P)
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    want_free, _, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    close(got, want_free, BAR[dt], f"{name} {dt} B={B} pruned, free-running")
    if dt != "fp32":
        w.set_residual_dtype(TORCH[dt])
        got = w(x).float().cpu().numpy()
        want_free, _, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=traced_selections(w, P))
        close(got, want_free, 2e-2, f"{name} {dt} B={B} pruned, free-running, 16-bit stream")


def test_forced_selection_must_keep_the_prefix_slots():
    (cfg, sd, _), w = build("vit_micro_reg4_patch16_64", SCHED, "bf16")
    imgs = images_of(cfg, 2)
    _, _, tr = npx.vit_forward_restated(sd, imgs, SCHED, cfg, dtype=torch.float32)
    bad = {i: torch.from_numpy(t["keep_idx"].copy()) for i, t in tr.items()}
    bad[1][0, 2] = 3
    w.force_keep_idx(bad)
    with pytest.raises(ValueError, match="prefix tokens"):
        w(torch.from_numpy(imgs).to(DEV))
    w.force_keep_idx({1: torch.from_numpy(tr[1]["keep_idx"][:, 4:].copy())})     # the [B, keep+1] layout of a register-free model
    with pytest.raises(ValueError, match="shape"):
        w(torch.from_numpy(imgs).to(DEV))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sub_batches_reproduce_the_full_batch_bit_for_bit(dt):
    for name in ("deit3_micro_reg4_patch16_64", "vit_micro_reg1_gap_patch14_56"):
        (cfg, _, _), w = build(name, SCHED, dt)
        x = torch.from_numpy(images_of(cfg, 9, seed=7)).to(DEV).to(TORCH[dt])
        full = w(x).clone()
        tc = w.get_last_stats()["token_counts"]
        for lo, hi in ((0, 1), (3, 5), (2, 9)):
            part = w(x[lo:hi].contiguous()).clone()
            assert w.get_last_stats()["token_counts"] == tc
            assert torch.equal(part.view(torch.uint8), full[lo:hi].contiguous().view(torch.uint8)), (name, lo, hi)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64"])
def test_a_record_with_one_prefix_token_is_the_old_forward(name, dt):
    """rajni_vit_forward_ext_prefix with a NULL record, num_prefix = 0 and num_prefix = 1 (with and without an ext record) gives the
    bits and the token counts of the entry point the wrapper took; so does the workspace query"""
    cfg = ts.CONFIGS[name]
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, **FIX), SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(images_of(cfg, 7)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, keep = w._plan[1], w._plan[2]
    ext = keep[4]
    assert keep[6] is None and (ext is None) == (name == "vit_micro_patch16_64")
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    for num in (None, 0, 1):
        pre = None
        if num is not None:
            pre = nat.VitPrefix()
            pre.num_prefix = num
        pp = C.byref(pre) if pre is not None else None
        assert lib.rajni_vit_workspace_bytes_prefix(C.byref(plan), pp) == lib.rajni_vit_workspace_bytes(C.byref(plan))
        for e in ([ext] if ext is not None else [None, nat.VitExt()]):
            out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
            for i in range(cfg.depth):
                keep[1][i] = -1
            nat.check(lib.rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(e) if e is not None else None, pp, x.data_ptr(),
                                                       out.data_ptr(), nat.stream_ptr(x.device)), "rajni_vit_forward_ext_prefix")
            torch.cuda.synchronize()
            assert torch.equal(out[:, :plan.num_classes].contiguous().view(torch.uint8), plain.contiguous().view(torch.uint8))
            assert [int(keep[1][i]) for i in range(cfg.depth)] == counts


# ---- opt-ins on the fp8-capable register model, held to the bars of their existing tests ---------------------------------------
# weights: the fixture every micro512 test of the project draws (tests/test_gpu_fp8_mfma.py::_build_f8,
# tests/test_gpu_variants_forward.py::_fp8_setup) - at embed dim 512 a given std gives twice the pre-activations of the
# embed-dim-128 micro models, and the project's bars for this model are stated at std 0.06
FIX512 = dict(seed=4, std=0.06, bias_std=0.02)


def test_cls_only_last_block_with_registers():
    """the bars of tests/test_gpu_forward.py::test_cls_only_last_block_gives_the_same_logits for a bf16 model: 8e-3 of the logit
    scale against the every-row forward (same selections), 1e-2 against the yardstick graph"""
    sched = {1: {"keep_ratio": 0.5}}
    (cfg, sd, stock), w = build("vit_micro512_reg4_patch16_64", sched, "bf16", FIX512)
    imgs = images_of(cfg, 4)
    assert_fixture_can_tell(cfg, sd, imgs, sched, 1e-2)
    x = torch.from_numpy(imgs).to(DEV)
    w.trace_scores(True)
    full = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [21, 21, 13, 13]
    forced = traced_selections(w, 5)
    want, _, _ = npx.vit_forward_restated(sd, imgs, sched, cfg, forced_keep=forced)
    close(full, want, 1e-2, "micro512 reg4, every row vs the restated graph")
    fast = w.set_last_block_cls_only(True)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [21, 21, 13, 13]
    assert all(np.array_equal(v, forced[i]) for i, v in traced_selections(w, 5).items())
    close(fast, full, 8e-3, "micro512 reg4, CLS-only last block vs every row")
    close(fast, want, 1e-2, "micro512 reg4, CLS-only last block vs the restated graph")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_residual_stream_in_the_model_dtype_with_registers(dt):
    (cfg, sd, stock), w = build("vit_micro512_reg4_patch16_64", SCHED, dt, FIX512)
    imgs = images_of(cfg, 4, seed=3)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED, 2e-2)
    w.set_residual_dtype(TORCH[dt]).trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    want, counts, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=traced_selections(w, 5))
    assert w.get_last_stats()["token_counts"] == counts == [21, 21, 17, 12]
    close(got, want, 2e-2, f"micro512 reg4 {dt}, 16-bit residual stream")


def _fp8_setup(fmt, batch):
    cfg = ts.CONFIGS["vit_micro512_reg4_patch16_64"]
    model = ts.create_model(cfg, round_bf16=True, **FIX512)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format(fmt).trace_scores(True)
    imgs = images_of(cfg, batch, seed=9)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, 5)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    return cfg, w, sd, imgs, got, forced


def test_fp8_weights_with_registers():
    """set_weight_format("fp8"): the restated graph on the dequantised weights with the device's selections, 1e-2 of the logit
    scale (tests/test_gpu_variants_forward.py::test_fp8_weights_on_a_qk_norm_model)"""
    cfg, w, sd, imgs, got, forced = _fp8_setup("fp8", 6)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED, 1e-2)
    want, counts, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, "micro512 reg4, fp8 weights")
    assert (got.argmax(1) == want.argmax(1)).all()


@pytest.mark.parametrize("batch", [3, 40])
def test_fp8_mfma_with_registers(batch):
    """set_weight_format("fp8_mfma"): the bars of tests/test_gpu_fp8_mfma.py::_check_against_rule, constants unchanged"""
    cfg, w, sd, imgs, got, forced = _fp8_setup("fp8_mfma", batch)
    with_act, counts, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, act_fp8=True)
    weights_only, _, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    assert w.get_last_stats()["token_counts"] == counts
    scale = float(np.abs(weights_only).max())
    err, cost, dev_cost = (float(np.abs(a - b).max()) for a, b in ((got, with_act), (with_act, weights_only), (got, weights_only)))
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    r_err, r_cost, r_dev = rms(got - with_act), rms(with_act - weights_only), rms(got - weights_only)
    print(f"[prefix] fp8_mfma micro512 reg4 batch {batch}: device vs graph-with-the-rule {err:.4g}, the rule's own effect {cost:.4g}, "
          f"device vs weights-only graph {dev_cost:.4g} (scale {scale:.4g}); rms {r_err:.4g} / {r_cost:.4g} / {r_dev:.4g}")
    assert err <= 1.6 * cost + 1e-2 * scale
    assert dev_cost <= 1.6 * cost + 1e-2 * scale
    assert cost <= 0.2 * scale
    assert r_err <= 1.35 * r_cost + 2e-3 * scale
    assert 0.6 * r_cost - 2e-3 * scale <= r_dev <= 1.4 * r_cost + 2e-3 * scale


# ---- DINOv2 ViT-S/14 with 4 registers at 224 -------------------------------------------------------------------------------------

def test_vit_small_patch14_reg4_dinov2():
    """B = 2 in bf16: unpruned against the stock forward, pruned free-running against the restated graph (fp32), at 1e-2"""
    name = "vit_small_patch14_reg4_dinov2"
    sched = {3: {"keep_ratio": 0.88}, 4: {"keep_ratio": 0.88}, 7: {"keep_ratio": 0.80}, 8: {"keep_ratio": 0.72}}
    fix = dict(seed=3, std=0.04, bias_std=0.1)
    (cfg, sd, stock), w = build(name, {}, "bf16", fix)
    imgs = images_of(cfg, 2)
    x = torch.from_numpy(imgs).to(DEV)
    close(w(x).float().cpu().numpy(), stock(imgs), 1e-2, f"{name} unpruned vs stock forward")
    assert w.get_last_stats()["token_counts"] == [261] * 12
    (_, _, _), wp = build(name, sched, "bf16", fix)
    wp.trace_scores(True)
    got = wp(x).float().cpu().numpy()
    forced = traced_selections(wp, 5)
    want, counts, _ = npx.vit_forward_restated(sd, imgs, sched, cfg, forced_keep=forced, dtype=torch.float32)
    assert wp.get_last_stats()["token_counts"] == counts == npx.token_counts(261, 12, sched, 5)
    close(got, want, 1e-2, f"{name} pruned, free-running")


def test_module_level_attention_keeps_the_registers():
    """RAJNIAttention.forward stand-alone with num_prefix_tokens = 5: [B, 5 + keep] outputs, the rule on its own scores"""
    from rajni_amd.wrapper import RAJNIAttention
    from oracle import rajni_oracle as orc
    cfg = ts.CONFIGS["vit_micro_reg4_patch16_64"]
    model = ts.create_model(cfg, round_bf16=True, **FIX)
    sd = ts.state_dict_numpy(model)
    att = RAJNIAttention(model.blocks[0].attn, keep_ratio=0.7, update=True).to(DEV).to(torch.bfloat16)
    att.num_prefix_tokens = 5
    xn = ts.bf16_round_np(np.random.default_rng(4).standard_normal((3, 21, 128), dtype=np.float32))
    out, keep_idx, nxt = att(torch.from_numpy(xn).to(DEV).to(torch.bfloat16))
    keep = npx.keep_count(0.7, 21, 5)
    assert tuple(out.shape) == (3, 5 + keep, 128) and tuple(keep_idx.shape) == tuple(nxt.shape) == (3, 5 + keep)
    t = lambda n: torch.from_numpy(sd["blocks.0.attn." + n]).double()
    qkv = (torch.from_numpy(xn).double() @ t("qkv.weight").T + t("qkv.bias"))
    scores = orc.importance_scores(qkv.numpy(), 2)
    ki = keep_idx.cpu().numpy()
    assert (ki[:, :5] == np.arange(5)).all() and (ki[:, 5:] >= 5).all() and (np.diff(ki, axis=1) > 0).all()
    want_nxt = np.take_along_axis(scores, ki, axis=1)
    assert np.abs(nxt.float().cpu().numpy() - want_nxt).max() <= 1e-2 * np.abs(want_nxt).max()
    # a carried stage: select-only on the previous stage's scores
    att.update = False
    out2, ki2, nxt2 = att(torch.from_numpy(xn).to(DEV).to(torch.bfloat16)[:, :5 + keep].contiguous(), prev_scores=nxt)
    keep2 = npx.keep_count(0.7, 5 + keep, 5)
    np.testing.assert_array_equal(ki2.cpu().numpy(), npx.select_tokens(nxt.float().cpu().numpy(), keep2, 5))
