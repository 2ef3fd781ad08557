"""Whole forwards of models with timm's q/k-norm, norm_pre and pooled-head options on the device.
GPU box only (`-m gpu`).

Yardsticks (the reference computes something else for such models, so it is not one):
  empty schedule   the base model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_variants.py::vit_forward_restated - the reference's pruned graph with timm's three options
                   added, torch fp64 - with its selections injected (`force_keep_idx`); free-running, the device's keep_idx must
                   be exactly the defined top-k rule applied to the device's own traced scores.
Bars are the project's: 1e-2 x max|logit| for 16-bit models, 1e-3 for fp32.  Before a case is accepted the same graph shows on
the CPU that ignoring the option under test moves the fp32 logits by at least 5x the bar."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics_variants as nv
import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
# config -> the options whose omission the fixture must be able to see
CASES = {"vit_micro_qknorm_patch16_64": ("qk_norm",), "vit_micro_prenorm_patch16_64": ("pre_norm",),
         "vit_micro_gap_patch16_64": ("avg_pool", "fc_norm"), "vit_micro_fcnorm_patch16_64": ("fc_norm",),
         "vit_micro_all_patch16_64": ("qk_norm", "pre_norm", "avg_pool"), "vit_micro_d80_qknorm_patch16_64": ("qk_norm", "avg_pool")}


def images_of(cfg, B, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def build(name, sched, dt, fix=FIX):
    cfg = ts.CONFIGS[name]
    model = ts.create_model(cfg, round_bf16=True, **fix)
    sd = ts.state_dict_numpy(model)

    def stock(x):                 # the base model's own forward: fp32, CPU, bf16-representable weights
        with torch.no_grad():
            return model(torch.from_numpy(x)).numpy()

    wrapped = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, **fix), sched).to(DEV).to(TORCH[dt]).eval()
    return (cfg, sd, stock), wrapped


def assert_fixture_can_tell(cfg, sd, imgs, sched, options, bar):
    full, _, tr = nv.vit_forward_restated(sd, imgs, sched, cfg, dtype=torch.float32)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    for opt in options:
        dropped, _, _ = nv.vit_forward_restated(sd, imgs, sched, cfg, dtype=torch.float32, drop=(opt,), forced_keep=forced)
        moved = float(np.abs(full - dropped).max())
        assert moved >= 5 * bar * float(np.abs(full).max()), f"ignoring {opt} moves the logits by only {moved:.4g}"


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[variants] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_empty_schedule_equals_the_stock_forward(name, dt):
    (cfg, sd, stock), w = build(name, {}, dt)
    imgs = images_of(cfg, 5)
    assert_fixture_can_tell(cfg, sd, imgs, {}, CASES[name], BAR[dt])
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + 1] * cfg.depth
    close(got, stock(imgs), BAR[dt], f"{name} {dt} unpruned vs stock forward")
    if dt != "fp32":       # the 16-bit residual stream (norm_pre is written back in the stream's own type): the project's 2e-2 bar
        w.set_residual_dtype(TORCH[dt])
        close(w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy(), stock(imgs), 2e-2, f"{name} {dt} stream, unpruned")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pruned_forward_selection_conditional_and_free_running(name, dt):
    (cfg, sd, _), w = build(name, SCHED, dt)
    imgs = images_of(cfg, 6, seed=5)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED, CASES[name], BAR[dt])
    want, counts, tr = nv.vit_forward_restated(sd, imgs, SCHED, cfg)
    x = torch.from_numpy(imgs).to(DEV)
    # the yardstick's selections injected
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} pruned, selections injected")
    # free-running: the rule on the device's own scores (computed from the NORMALISED q and k), then the graph on those selections
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, orc.select_tokens(t["scores"].float().cpu().numpy().astype(np.float64), idx.shape[1] - 1))
        forced[i] = idx
    s1 = w.get_last_trace()[1]["scores"].float().cpu().numpy()
    assert np.abs(s1 - tr[1]["scores"]).max() <= (3e-2 if dt != "fp32" else 1e-3) * np.abs(tr[1]["scores"]).max()
    want_free, _, _ = nv.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    close(got, want_free, BAR[dt], f"{name} {dt} pruned, free-running")


@pytest.mark.parametrize("name,option", [("vit_base_patch16_clip_224", "pre_norm"), ("vit_base_patch16_qknorm_224", "qk_norm")])
def test_vit_base_sized_models(name, option):
    """ViT-B/16 at batch 24 in bf16: unpruned against the stock forward, pruned (README schedule) against the restated graph in
    fp32 with the device's own selections; q/k-norm launches sit on both sides of the kernel's dispatch threshold"""
    sched = {3: {"keep_ratio": 0.88}, 4: {"keep_ratio": 0.88}, 7: {"keep_ratio": 0.80}, 8: {"keep_ratio": 0.72}}
    fix = dict(seed=3, std=0.04, bias_std=0.1)
    (cfg, sd, stock), w = build(name, {}, "bf16", fix)
    B = 24
    imgs = images_of(cfg, B)
    assert_fixture_can_tell(cfg, sd, imgs[:2], {}, (option,), 1e-2)
    x = torch.from_numpy(imgs).to(DEV)
    close(w(x).float().cpu().numpy(), stock(imgs), 1e-2, f"{name} unpruned vs stock forward")
    (_, _, _), wp = build(name, sched, "bf16", fix)
    wp.trace_scores(True)
    got = wp(x).float().cpu().numpy()
    forced = {}
    for i, t in wp.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, orc.select_tokens(t["scores"].float().cpu().numpy().astype(np.float64), idx.shape[1] - 1))
        forced[i] = idx
    want, counts, _ = nv.vit_forward_restated(sd, imgs, sched, cfg, forced_keep=forced, dtype=torch.float32)
    assert wp.get_last_stats()["token_counts"] == counts == [197, 197, 197, 197, 173, 152, 152, 152, 121, 87, 87, 87]
    close(got, want, 1e-2, f"{name} pruned, free-running")


# ---- fp8 weight formats on the q/k-norm micro512 model, against their existing bars (tests/test_gpu_fp8.py, test_gpu_fp8_mfma.py)

def _fp8_setup(fmt, batch):
    cfg = ts.CONFIGS["vit_micro512_qknorm_patch16_64"]
    model = ts.create_model(cfg, seed=4, std=0.06, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format(fmt).trace_scores(True)
    imgs = images_of(cfg, batch, seed=9)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, orc.select_tokens(t["scores"].float().cpu().numpy().astype(np.float64), idx.shape[1] - 1))
        forced[i] = idx
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    return cfg, w, sd, imgs, got, forced


def test_fp8_weights_on_a_qk_norm_model():
    """set_weight_format("fp8"): the restated graph on the dequantised weights with the device's selections, 1e-2 of the logit scale"""
    cfg, w, sd, imgs, got, forced = _fp8_setup("fp8", 6)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED, ("qk_norm",), 1e-2)
    want, counts, _ = nv.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, "micro512 q/k-norm, fp8 weights")
    assert (got.argmax(1) == want.argmax(1)).all()


@pytest.mark.parametrize("batch", [3, 40])
def test_fp8_mfma_on_a_qk_norm_model(batch):
    """set_weight_format("fp8_mfma") (q/k-norm runs on the bf16 qkv the fp8 QKV GEMM writes, the e4m3 attention output reads it):
    the bars of tests/test_gpu_fp8_mfma.py::_check_against_rule, constants unchanged"""
    cfg, w, sd, imgs, got, forced = _fp8_setup("fp8_mfma", batch)
    with_act, counts, _ = nv.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, act_fp8=True)
    weights_only, _, _ = nv.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    assert w.get_last_stats()["token_counts"] == counts
    scale = float(np.abs(weights_only).max())
    err, cost, dev_cost = (float(np.abs(a - b).max()) for a, b in ((got, with_act), (with_act, weights_only), (got, weights_only)))
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    r_err, r_cost, r_dev = rms(got - with_act), rms(with_act - weights_only), rms(got - weights_only)
    print(f"[variants] fp8_mfma q/k-norm micro512 batch {batch}: device vs graph-with-the-rule {err:.4g}, the rule's own effect {cost:.4g}, "
          f"device vs weights-only graph {dev_cost:.4g} (scale {scale:.4g}); rms {r_err:.4g} / {r_cost:.4g} / {r_dev:.4g}")
    assert err <= 1.6 * cost + 1e-2 * scale
    assert dev_cost <= 1.6 * cost + 1e-2 * scale
    assert cost <= 0.2 * scale
    assert r_err <= 1.35 * r_cost + 2e-3 * scale
    assert 0.6 * r_cost - 2e-3 * scale <= r_dev <= 1.4 * r_cost + 2e-3 * scale


# ---- bit identity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_zeroed_extension_record_is_the_plain_forward(dt):
    """a model with no option: rajni_vit_forward and rajni_vit_forward_ext with an all-zero record (and with a NULL one) give the
    same bits, pruned, and the same token counts"""
    (cfg, _, _), w = build("vit_micro_patch16_64", SCHED, dt)
    x = torch.from_numpy(images_of(cfg, 7)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    entry = w._plan
    plan, keep = entry[1], entry[2]
    assert keep[4] is None                                   # no option: the wrapper took the plain entry point
    counts = w.get_last_stats()["token_counts"]
    for ext in (nat.VitExt(), None):
        out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        for i in range(cfg.depth):
            keep[1][i] = -1
        nat.check(nat.lib().rajni_vit_forward_ext(C.byref(plan), C.byref(ext) if ext is not None else None, x.data_ptr(),
                                                  out.data_ptr(), nat.stream_ptr(x.device)), "rajni_vit_forward_ext")
        torch.cuda.synchronize()
        assert torch.equal(out[:, :plan.num_classes].view(torch.uint8), plain.contiguous().view(torch.uint8))
        assert [int(keep[1][i]) for i in range(cfg.depth)] == counts


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sub_batches_reproduce_the_full_batch_bit_for_bit(dt):
    """q/k-norm + GAP model (head dim 80: the general q/k-norm form; and the all-options head-dim-64 model): an image's logits
    do not depend on the batch around it"""
    for name in ("vit_micro_d80_qknorm_patch16_64", "vit_micro_all_patch16_64"):
        (cfg, _, _), w = build(name, SCHED, dt)
        x = torch.from_numpy(images_of(cfg, 9, seed=7)).to(DEV).to(TORCH[dt])
        full = w(x).clone()
        tc = w.get_last_stats()["token_counts"]
        for lo, hi in ((0, 1), (3, 5), (2, 9)):
            part = w(x[lo:hi].contiguous()).clone()
            assert w.get_last_stats()["token_counts"] == tc
            assert torch.equal(part.view(torch.uint8), full[lo:hi].contiguous().view(torch.uint8)), (name, lo, hi)


def test_cls_only_last_block_with_token_pool_and_fc_norm_and_its_refusal_with_avg():
    (cfg, sd, stock), w = build("vit_micro_fcnorm_patch16_64", {1: {"keep_ratio": 0.5}}, "bf16")
    imgs = images_of(cfg, 4)
    x = torch.from_numpy(imgs).to(DEV)
    a = w(x).float().cpu().numpy()
    b = w.set_last_block_cls_only(True)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == [17, 17, 9, 9]
    close(b, a, 1e-2, "fc_norm model, CLS-only last block vs every row")
    (_, _, _), g = build("vit_micro_gap_patch16_64", {}, "bf16")
    with pytest.raises(ValueError, match="avg"):
        g.set_last_block_cls_only(True)
    # the C ABI refuses the combination too
    g(x)
    plan, ext = g._plan[1], g._plan[2][4]
    plan.cls_only_last_block = 1
    out = torch.empty((4, plan.logits_ld), dtype=torch.bfloat16, device=DEV)
    rc = nat.lib().rajni_vit_forward_ext(C.byref(plan), C.byref(ext), x.to(torch.bfloat16).data_ptr(), out.data_ptr(), nat.stream_ptr(x.device))
    plan.cls_only_last_block = 0
    assert rc == 1 and b"avg" in nat.lib().rajni_last_error()


def test_module_level_attention_applies_qk_norm():
    """RAJNIAttention.forward stand-alone on a q/k-norm block: the restated block with its own selection injected"""
    from rajni_amd.wrapper import RAJNIAttention
    cfg = ts.CONFIGS["vit_micro_qknorm_patch16_64"]
    model = ts.create_model(cfg, round_bf16=True, **FIX)
    sd = ts.state_dict_numpy(model)
    att = RAJNIAttention(model.blocks[0].attn, keep_ratio=0.7, update=True).to(DEV).to(torch.bfloat16)
    xn = ts.bf16_round_np(np.random.default_rng(4).standard_normal((3, 17, 128), dtype=np.float32))
    out, keep_idx, nxt = att(torch.from_numpy(xn).to(DEV).to(torch.bfloat16))
    t = lambda n: torch.from_numpy(sd["blocks.0.attn." + n]).double()
    qkv = (torch.from_numpy(xn).double() @ t("qkv.weight").T + t("qkv.bias")).reshape(3, 17, 3, 2, 64)
    q, k, v = qkv.unbind(2)
    q = torch.nn.functional.layer_norm(q, (64,), t("q_norm.weight"), t("q_norm.bias"), cfg.ln_eps)
    k = torch.nn.functional.layer_norm(k, (64,), t("k_norm.weight"), t("k_norm.bias"), cfg.ln_eps)
    scores = orc.importance_scores(torch.stack([q, k, v], 2).reshape(3, 17, 384).numpy(), 2)
    ki = keep_idx.cpu().numpy()
    want_nxt = np.take_along_axis(scores, ki, axis=1)
    assert np.abs(nxt.float().cpu().numpy() - want_nxt).max() <= 1e-2 * np.abs(want_nxt).max()
    gi = torch.from_numpy(ki)[:, :, None, None].expand(-1, -1, 2, 64)
    q, k, v = q.gather(1, gi), k.gather(1, gi), v.gather(1, gi)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * 64 ** -0.5, -1)
    want = (torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(3, -1, 128) @ t("proj.weight").T + t("proj.bias")).numpy()
    assert np.abs(out.float().cpu().numpy() - want).max() <= 1.5e-2 * np.abs(want).max()
