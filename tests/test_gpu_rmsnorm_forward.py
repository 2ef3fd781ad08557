"""Whole forwards of models with RMSNorm trunks and / or a norm inside the patch embedding (include/rajni_hip_norm.h; the AIMv2
recipe at micro cost), on the device.  GPU box only (`-m gpu`).

Yardsticks (the reference cannot run such a model):
  empty schedule   the timm-shaped model's own stock-PyTorch forward, fp32 on the CPU, bf16-representable weights;
  pruned           tests/numerics_rmsnorm.py::vit_forward_restated, torch fp64: its selections injected (`force_keep_idx`), and
                   free-running, where the device's selections must BE the restatement's - the fixtures' seeds
                   (numerics_rmsnorm.SEEDS) leave every boundary gap at 8 x the bf16 score budget or more, and
                   tests/test_rmsnorm_cpu.py asserts that and that the same graph with LayerNorm substituted, or without the
                   embedding norm, lies 10 bars away.
Bars are those of tests/test_gpu_noclass_forward.py: 1e-2 x max|out| for 16-bit models, 1e-3 for fp32, under the same criterion;
feature outputs at max(bar, 1.5 x d16) like tests/test_gpu_features.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import numerics_image as ni
import numerics_noclass as nq
import numerics_prefix as npx
import numerics_rmsnorm as nr
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = nr.BAR
SCHED = nr.SCHED
MICRO = nr.MICRO
AIMV2 = "vit_micro_aimv2_patch16_64"
fixture = nr.fixture


@functools.lru_cache(maxsize=None)
def yardstick(name, B):
    """the restated graph, free-running in fp64: computed once per (model, batch)"""
    cfg, sd, iseed = fixture(name)
    return nr.vit_forward_restated(sd, nr.images_of(cfg, B, iseed), SCHED, cfg)


def wrapped(name, sched, dt):
    return rajni_amd.RAJNIViTWrapper(nr.build_model(name), sched).to(DEV).to(TORCH[dt]).eval()


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[rmsnorm] {what}: max |d| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
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
    """the native entry point the wrapper's current plan goes through"""
    from rajni_amd.wrapper import model as wm
    e = w._plan
    return wm._native_call(wm._FORWARDS, e.refs.ext, e.refs.pre, None, e.input.img, e.input.qry, e.input.apr, e.input.nrm)[0]


# ---- 1. empty schedule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MICRO)
def test_empty_schedule_equals_the_stock_forward(name, dt, B):
    cfg, sd, iseed = fixture(name)
    imgs = nr.images_of(cfg, B, iseed)
    with torch.no_grad():
        stock = nr.build_model(name)(torch.from_numpy(imgs)).numpy()
    w = wrapped(name, {}, dt)
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    assert got.shape == stock.shape and entry_symbol(w) == "rajni_vit_forward_norm"
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth
    close(got, stock, BAR[dt], f"{name} {dt} B={B} unpruned vs stock forward")


# ---- 2. scheduled --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MICRO)
def test_pruned_forward_selection_conditional_and_free_running(name, dt, B):
    cfg, sd, iseed = fixture(name)
    P = cfg.num_prefix_tokens
    want, counts, tr = yardstick(name, B)
    assert counts == npx.token_counts(cfg.num_patches + P, cfg.depth, SCHED, P)
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(nr.images_of(cfg, B, iseed)).to(DEV)
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, selections injected")
    # free-running: the device's selections are the rule on its own scores AND the restatement's, image for image
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    forced = traced_selections(w, P)
    for i in sorted(tr):
        np.testing.assert_array_equal(forced[i], tr[i]["keep_idx"], err_msg=f"{name} {dt} B={B} block {i}")
    close(got, want, BAR[dt], f"{name} {dt} B={B} pruned, free-running")


# ---- 3. sub-batches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sub_batches_reproduce_the_full_batch_bit_for_bit(dt):
    for name in MICRO:
        cfg, _, iseed = fixture(name)
        w = wrapped(name, SCHED, dt)
        x = torch.from_numpy(nr.images_of(cfg, 9, iseed + 1)).to(DEV).to(TORCH[dt])
        full = w(x).clone()
        tc = w.get_last_stats()["token_counts"]
        for lo, hi in ((0, 1), (3, 5), (2, 9)):
            part = w(x[lo:hi].contiguous()).clone()
            assert w.get_last_stats()["token_counts"] == tc
            assert same_bits(part, full[lo:hi].contiguous()), (name, lo, hi)


# ---- 4. a NULL / {LAYERNORM, no embedding norm} record is the old forward -----------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_gap_patch16_64"])
def test_a_null_or_layernorm_record_is_the_old_forward(name, dt):
    cfg = ts.CONFIGS[name]
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True), SCHED).to(DEV).to(TORCH[dt]).eval()
    x = torch.from_numpy(nr.images_of(cfg, 7, 2)).to(DEV).to(TORCH[dt])
    plain = w(x).clone()
    plan, refs = w._plan.plan, w._plan.refs
    ext = refs.ext
    assert w._plan.input.nrm is None and entry_symbol(w) in ("rajni_vit_forward", "rajni_vit_forward_ext")
    counts = w.get_last_stats()["token_counts"]
    lib = nat.lib()
    for n in (None, nat.VitNorm()):
        npn = C.byref(n) if n is not None else None
        assert lib.rajni_vit_workspace_bytes_norm(C.byref(plan), None, None, None, None, npn) == lib.rajni_vit_workspace_bytes(C.byref(plan))
        out = torch.empty((7, plan.logits_ld), dtype=TORCH[dt], device=DEV)
        for i in range(cfg.depth):
            refs.tc[i] = -1
        nat.check(lib.rajni_vit_forward_norm(C.byref(plan), C.byref(ext) if ext is not None else None, None, None, None, None, None,
                                             npn, x.data_ptr(), out.data_ptr(), nat.stream_ptr(x.device)), "rajni_vit_forward_norm")
        torch.cuda.synchronize()
        assert same_bits(out[:, :plan.num_classes].contiguous(), plain.contiguous())
        assert [int(refs.tc[i]) for i in range(cfg.depth)] == counts


# ---- 5. feature outputs on the AIMv2 micro model -------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_feature_outputs_of_an_rms_model(dt):
    cfg, sd, iseed = fixture(AIMV2)
    B, P, n0, Cd = 3, 0, 16, cfg.embed_dim
    imgs = nr.images_of(cfg, B, iseed)
    caps = (1, 3)
    want = nr.feature_outputs(sd, imgs, SCHED, cfg, caps=caps)
    forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
    bar = BAR[dt]
    if dt != "fp32":      # the same graph in the model's 16-bit dtype on the CPU (tests/test_gpu_features.py's rule)
        r16 = nr.feature_outputs(sd, imgs, SCHED, cfg, forced_keep=forced, caps=caps, dtype=TORCH[dt])
        d16 = max(float(np.abs(r16[k] - want[k]).max() / np.abs(want[k]).max()) for k in ("tokens", "dense_last"))
        d16 = max([d16] + [float(np.abs(r16["slabs"][c] - want["slabs"][c]).max() / np.abs(want["slabs"][c]).max()) for c in caps])
        print(f"[rmsnorm] {AIMV2} {dt}: d16 {d16:.3g}")
        bar = max(bar, 1.5 * d16)
    w = wrapped(AIMV2, SCHED, dt)
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    x = torch.from_numpy(imgs).to(DEV)
    tokens = w.forward_features(x).clone()
    src = w.get_last_stats()["source_idx"]
    np.testing.assert_array_equal(src.cpu().numpy(), want["source_idx"])
    assert w.get_last_stats()["token_counts"] == want["counts"] and tuple(tokens.shape) == (B, want["counts"][-1], Cd)
    close(tokens.float().cpu().numpy(), want["tokens"], bar, f"{AIMV2} {dt} tokens")
    # dense: the tokens' bits at their source rows, zero bytes elsewhere
    dense = w.forward_features(x, dense=True).clone()
    assert tuple(dense.shape) == (B, n0, Cd)
    assert same_bits(torch.gather(dense, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    mask = torch.ones((B, n0), dtype=torch.bool, device=DEV).scatter_(1, src.long(), False)
    assert int(mask.sum()) == B * (n0 - tokens.shape[1]) and not dense[mask].contiguous().view(torch.uint8).any()
    close(dense.float().cpu().numpy(), want["dense"], bar, f"{AIMV2} {dt} dense")
    # fill="last": the survivors' bits again, every pruned position holding the state it left with
    last = w.forward_features(x, dense=True, fill="last").clone()
    np.testing.assert_array_equal(w.get_last_stats()["exit_block"].cpu().numpy(), want["exit_block"])
    assert same_bits(torch.gather(last, 1, src.long()[:, :, None].expand(-1, -1, Cd)), tokens)
    assert not torch.isnan(last.float()).any() and bool((last[mask].float().abs().amax(dim=-1) > 0).all())
    close(last.float().cpu().numpy(), want["dense_last"], bar, f"{AIMV2} {dt} dense, fill=last")
    # forward_intermediates(norm=False): the un-normalised slabs; norm=True is refused by name
    for fill in ("zero", "last"):
        final, inter = w.forward_intermediates(x, indices=[1, 3], output_fmt="NLC", norm=False, fill=fill)
        assert same_bits(final, dense if fill == "zero" else last)
        for c, spatial in zip(caps, inter):
            slab = spatial.float().cpu().numpy()
            alive = want["exit_block"] > c
            close(slab[alive], want["slabs"][c][alive], bar, f"{AIMV2} {dt} intermediate of block {c}, fill={fill}")
            assert (not slab[~alive].any()) if fill == "zero" else bool((np.abs(slab[~alive]).max(axis=-1) > 0).all())
    with pytest.raises(NotImplementedError, match="RMSNorm"):
        w.forward_intermediates(x, indices=[1], norm=True)
    with pytest.raises(NotImplementedError, match="RMSNorm"):
        w.get_intermediate_layers(x, n=1)          # (its default is norm=True)
    assert len(w.get_intermediate_layers(x, n=2, norm=False)) == 2


def test_normalised_intermediates_work_with_a_layernorm_embedding_norm():
    name = "vit_micro_reg4_embednorm_patch16_64"
    cfg, sd, iseed = fixture(name)
    w = wrapped(name, SCHED, "bf16")
    x = torch.from_numpy(nr.images_of(cfg, 3, iseed)).to(DEV)
    final, inter = w.forward_intermediates(x, indices=[3], output_fmt="NLC", norm=True)
    tokens = w.forward_features(x)
    src = w.get_last_stats()["source_idx"].long()
    # the last block's normalised slab is the final norm's rows on the unpruned grid
    got = torch.gather(final, 1, src[:, :, None].expand(-1, -1, cfg.embed_dim))
    assert same_bits(got, tokens) and same_bits(inter[0], final[:, cfg.num_prefix_tokens:])


# ---- 6. any input size, fp8 weights ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_dynamic_img_size_with_an_embedding_norm(dt):
    name, size = AIMV2, (48, 96)
    cfg, sd, iseed = fixture(name)
    imgs = nr.images_of(cfg, 3, iseed, size)
    want, counts, tr = nr.vit_forward_restated(ni.sd_at_grid(sd, cfg, (3, 6), dt=dt), imgs, SCHED, cfg)
    assert counts[0] == 18
    w = wrapped(name, SCHED, dt)
    x = torch.from_numpy(imgs).to(DEV)
    w.set_dynamic_img_size().force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_norm"
    close(got, want, BAR[dt], f"{name} 48x96 {dt}, selections injected")


def test_fp8_weights_on_the_rms_model():
    name = "vit_micro_rms_patch16_64"
    cfg, _, iseed = fixture(name)
    model = nr.build_model(name)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8").trace_scores(True)
    imgs = nr.images_of(cfg, 6, iseed + 2)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = traced_selections(w, 1)
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = nr.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, f"{name}, fp8 weights")


# ---- 7. refusals, the CLI --------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device():
    x = torch.zeros(2, 3, 64, 64, device=DEV)
    w = wrapped("vit_micro_rms_patch16_64", SCHED, "bf16")
    with pytest.raises(NotImplementedError, match="RMSNorm"):
        w.set_weight_format("fp8_mfma")
    w = wrapped("vit_micro_reg4_embednorm_patch16_64", SCHED, "bf16")
    with pytest.raises(NotImplementedError, match=r"patch_embed\.norm"):
        w.set_weight_format("fp8_mfma")
    m = nr.build_model("vit_micro_rms_patch16_64")
    m.blocks[1].norm2 = nn.LayerNorm(128, eps=1e-6)
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.norm2 is layernorm"):
        rajni_amd.RAJNIViTWrapper(m, SCHED).to(DEV).to(torch.bfloat16).eval()(x)
    cfg = ts.NormViTConfig(img_size=64, embed_dim=128, depth=2, num_heads=2, num_classes=10, global_pool="map", class_token=False,
                           norm="rms")
    m = ts.VisionTransformer(cfg)
    m.attn_pool.norm = nn.LayerNorm(128)
    with pytest.raises(NotImplementedError, match="global_pool='map' on a model with RMSNorm"):
        rajni_amd.RAJNIViTWrapper(m, {}).to(DEV).to(torch.bfloat16).eval()(x)


def test_cli_runs_the_aimv2_micro_model():
    from rajni_amd import run
    acc, thr = run.main(["--model", AIMV2, "--batch_size", "8", "--max_batches", "2", "--warmup", "1", "--synthetic"])
    assert thr > 0 and 0.0 <= acc <= 100.0


# ---- 8. a small crossing ---------------------------------------------------------------------------------------------------------
# norm kind x class token x pool x MLP x registers: eight cases that hold every legal pair of values (a model without a class
# token has no token head).  LayerNorm cases carry a LayerNorm embedding norm - without one they would not need the record; an
# 'avg' head keeps timm's default for it (fc_norm behind the pool, no final norm) on the class-token cases.
CROSS = [("layernorm", 1, "token", "mlp", 0), ("layernorm", 0, "avg", "swiglu", 4), ("rms", 1, "token", "swiglu", 4),
         ("rms", 0, "avg", "mlp", 0), ("layernorm", 1, "avg", "mlp", 4), ("layernorm", 1, "token", "swiglu", 0),
         ("rms", 1, "avg", "swiglu", 0), ("rms", 0, "avg", "swiglu", 4)]


def test_the_crossing_holds_every_legal_pair():
    axes = [("layernorm", "rms"), (1, 0), ("token", "avg"), ("mlp", "swiglu"), (0, 4)]
    legal = [c for c in itertools.product(*axes) if not (c[1] == 0 and c[2] == "token")]
    pairs = lambda c: {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(5), 2)}
    assert len(CROSS) >= 8 and set(CROSS) <= set(legal)
    assert set().union(*map(pairs, legal)) == set().union(*map(pairs, CROSS))


@pytest.mark.parametrize("case", CROSS, ids=["-".join(map(str, c)) for c in CROSS])
def test_crossing_against_the_restatement(case):
    kind, cls, pool, mlp, reg = case
    cfg = ts.NormViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, mlp_ratio=2.0, ln_eps=1e-5,
                           global_pool=pool, fc_norm=None if cls else False, class_token=bool(cls), mlp=mlp, reg_tokens=reg,
                           norm=kind, embed_norm=(kind == "layernorm" or not cls), bias=bool(cls))
    model = nr.build_model(cfg, wseed=nr.quiet_seed(cfg, 7))      # (not a fixture the bf16 format alone pushes to the bar)
    sd = ts.state_dict_numpy(model)
    imgs = nr.images_of(cfg, 3, 7)
    want, counts, tr = nr.vit_forward_restated(sd, imgs, SCHED, cfg)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and entry_symbol(w) == "rajni_vit_forward_norm"
    close(got, want, BAR["bf16"], f"crossing {case}")
