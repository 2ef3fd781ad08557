"""The opt-in fp8 path of BASELINE.json configs[4] ("deit3_base_patch16_224 fp8 weights (CDNA4 fp8 MFMA)"):
`set_weight_format("fp8_mfma")` = e4m3 block weights AND per-row-scaled e4m3 inputs of qkv / fc1 / fc2 on
v_mfma_f32_16x16x128_f8f6f4.  GPU box only (`-m gpu`).

The reference has no fp8 semantics (SURVEY 7 "hard parts"), so parity is defined the way tests/test_gpu_fp8.py
defines it for weights: the ORACLE run on the DEQUANTISED operands - here the dequantised weights and the same
activation-quantisation rule (oracle.quantize_rows_e4m3 / row_scale_e4m3 / hidden_scale_bound, which restate
include/rajni_hip.h's rajni_layernorm_fp8) - and the cost of quantisation against the reference fixture is reported."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import ops, timm_shaped as ts, _native as nat
from rajni_amd.timm_shaped import bf16_round_np
from helpers import load_case, case_images, pruned_blocks
import numerics_fp8 as n8
from numerics_fp8 import e4m3_bytes_to_f64

DEV = "cuda"


@pytest.mark.parametrize("rows,Cc,x_f32", [(300, 768, True), (64, 512, False), (1000, 1024, True), (5, 256, True),
                                           (37, 1280, True), (9, 2048, False),       # > 1024: the four-chunk instantiation
                                           (4099, 768, True), (4096, 1024, True)])   # >= 4096 fp32 rows: two rows per wave
def test_layernorm_fp8_rule(rows, Cc, x_f32):
    rng = np.random.default_rng(rows + Cc)
    x = rng.standard_normal((rows, Cc), dtype=np.float32) * rng.uniform(0.05, 30.0, size=(rows, 1)).astype(np.float32)
    x += rng.standard_normal((rows, 1), dtype=np.float32) * 3
    x[rows // 2] = 0.0                                   # an all-zero row (after the affine map: the bias row)
    if not x_f32:
        x = bf16_round_np(x)
    w = (1 + 0.1 * rng.standard_normal(Cc)).astype(np.float32)
    b = (0.05 * rng.standard_normal(Cc)).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV) if x_f32 else torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    wn, bm = 0.61, 0.07
    q, s, hs = ops.layernorm_fp8(xt, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), 1e-6, hidden_bound=(wn, bm))
    o = orc.layer_norm(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), 1e-6)
    s_ref = np.abs(o).max(axis=1) / 448.0
    s_dev = s.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(s_dev, s_ref, rtol=2e-5)
    deq = e4m3_bytes_to_f64(q) * s_dev[:, None]
    # e4m3: 3 mantissa bits -> half an ulp is 2^-4 relative in the normal range, 2^-10 * scale absolute below it
    bound = np.maximum(np.abs(o) * 2.0 ** -4, s_dev[:, None] * 2.0 ** -10) * 1.001 + 1e-6 * np.abs(o).max()
    assert (np.abs(deq - o) <= bound).all()
    # and byte for byte the stated rule on the device's own fp32 scale (the rare differences are elements whose fp32
    # LayerNorm value sits within an fp32 ulp of a rounding boundary)
    want = orc.quantize_rows_e4m3(o, s_dev.astype(np.float32))
    assert np.mean(want != deq) < 2e-3
    hs_ref = (1.0625 * np.sqrt((o ** 2).sum(axis=1)) * wn + bm) / 448.0
    np.testing.assert_allclose(hs.cpu().numpy(), hs_ref, rtol=2e-5)


@pytest.mark.parametrize("B,N,Np,H", [(2, 197, 173, 12), (3, 17, 13, 2), (2, 87, 87, 3), (1, 152, 121, 3), (2, 224, 224, 2),
                                      (1, 40, 33, 2), (2, 197, 197, 12)])
@pytest.mark.parametrize("loose", [1.0, 24.0])
def test_attention_fp8_output_rule(B, N, Np, H, loose):
    """rajni_attention_fp8: rows = e4m3_rne_sat(attention * (1 / out_scale)) with ONE given scale (a bound; `loose` = how far
    above the true maximum it sits - e4m3 is a floating-point format, a loose bound costs range, not precision), the same
    scale in every row-scale slot; everything else (gather, softmax, products) as rajni_attention."""
    rng = np.random.default_rng(N * 31 + Np + H)
    Cc = H * 64
    qkv = bf16_round_np(rng.standard_normal((B, N, 3 * Cc), dtype=np.float32))
    if Np == N:
        idx_t, g = None, qkv
    else:
        idx = np.stack([np.concatenate([[0], 1 + np.sort(rng.choice(N - 1, Np - 1, replace=False))]) for _ in range(B)])
        idx_t = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        g = orc.gather_rows(qkv, idx.astype(np.int64))
    q, k, v = orc.split_heads(g.astype(np.float64), H)
    want = orc.softmax_attention(q, k, v, 64 ** -0.5)
    scale = float(np.float32(np.abs(want).max() * loose / 448.0))
    xb = torch.from_numpy(qkv).to(DEV).to(torch.bfloat16)
    out, rs = ops.attention_fp8(xb, idx_t, H, 64 ** -0.5, scale)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, Np, Cc)
    ref = ops.attention(xb, idx_t, H, 64 ** -0.5).float().cpu().numpy().astype(np.float64)     # the bf16-output kernel: same products
    n8.check_attention_fp8(out, rs, ref, want, scale)     # bounds and the byte rule: tests/numerics_fp8.py


def test_attention_fp8_refuses_what_it_does_not_serve():
    x = torch.zeros(1, 230, 3 * 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="224"):
        ops.attention_fp8(x, None, 1, 0.125, 1.0)
    x = torch.zeros(1, 40, 3 * 96, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        ops.attention_fp8(x, None, 1, 0.1, 1.0)            # head dim 96
    x = torch.zeros(1, 40, 3 * 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(nat.NativeError):
        ops.attention_fp8(x, None, 1, 0.125, 0.0)          # a scale must be positive


def test_attention_out_scale_is_a_bound_and_matches_the_oracle():
    """ops.attention_out_scale (packed with the weights) restated by oracle.attention_out_scale, and really a bound: the
    largest |attention output| of a random block whose LayerNorm feeds V stays below 448 * scale."""
    rng = np.random.default_rng(11)
    Cc, H, B, N = 256, 4, 2, 50
    g = (1 + 0.2 * rng.standard_normal(Cc)).astype(np.float32)
    be = (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    wv = (0.05 * rng.standard_normal((Cc, Cc))).astype(np.float32)
    bv = (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    s_dev = ops.attention_out_scale(torch.from_numpy(g), torch.from_numpy(be), torch.from_numpy(wv), torch.from_numpy(bv))
    s_orc = float(orc.attention_out_scale(g, be, wv, bv))
    assert abs(s_dev - s_orc) <= 4e-6 * s_orc
    x = rng.standard_normal((B, N, Cc)) * rng.uniform(0.1, 20.0, size=(B, N, 1))
    ln = orc.layer_norm(x, g.astype(np.float64), be.astype(np.float64), 1e-6)
    ln = orc.quantize_rows_e4m3(ln, orc.row_scale_e4m3(ln))
    v = ln @ wv.astype(np.float64).T + bv
    assert np.abs(v).max() <= 448.0 * s_orc


def _f8_operands(rng, M, N, K):
    xq, xs, wp, ws, xd, wd = n8.f8_operands(rng, M, N, K)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return dev(xq), dev(xs), dev(wp), dev(ws), xd, wd


@pytest.fixture(params=[1, 2], ids=["256x128", "256x256"])
def f8_tiling(request):
    """Both fp8 x fp8 tilings (16x16x128 MFMAs on 256x128, 32x32x64 MFMAs on 256x256) must agree with fp64."""
    nat.lib().rajni_debug_force_f8_tiling(request.param)
    yield request.param
    nat.lib().rajni_debug_force_f8_tiling(0)


@pytest.mark.parametrize("M,N,K", [(256, 128, 512), (700, 768, 768), (50, 2304, 768), (1030, 200, 1024), (513, 3072, 768),
                                   (2100, 2304, 1536)])
def test_linear_f8_bias(M, N, K, f8_tiling):
    rng = np.random.default_rng(M + N + K)
    xq, xs, wp, ws, xd, wd = _f8_operands(rng, M, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    y = ops.linear(xq, wp, N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS, w_scale=ws, x_scale=xs)
    assert y.dtype == torch.bfloat16
    want = xd @ wd.T + b
    got = y.float().cpu().numpy()[:, :N]
    n8.check_bias(got, want)


@pytest.mark.parametrize("M,N,K", [(256, 256, 512), (700, 3072, 768), (60, 1000, 1024), (1300, 520, 768), (2100, 3072, 768)])
def test_linear_f8_gelu_requant(M, N, K, f8_tiling):
    """fc1 on the fp8 pipe: bias + exact-erf GELU, output re-quantised to e4m3 with the given per-row scale."""
    rng = np.random.default_rng(M * 3 + N + K)
    xq, xs, wp, ws, xd, wd = _f8_operands(rng, M, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    pre = xd @ wd.T + b
    ys = n8.gelu8_row_scales(rng, pre)                       # a bound, not the max
    y = ops.linear(xq, wp, N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS_GELU, w_scale=ws, x_scale=xs,
                   y_scale=torch.from_numpy(ys).to(DEV))
    assert y.dtype == torch.uint8
    deq = e4m3_bytes_to_f64(y)[:, :N] * ys[:, None].astype(np.float64)
    n8.check_gelu8(deq, pre, ys)


@pytest.mark.parametrize("M,N,K,gather", [(512, 768, 3072, False), (700, 768, 1024, True), (90, 256, 512, False),
                                          (1280, 520, 768, False)])
def test_linear_f8_resid_fp32_stream(M, N, K, gather):
    """fc2 on the fp8 pipe: y = gamma * (xd wd^T + b) + resid on the fp32 residual stream (optionally gathered rows)."""
    rng = np.random.default_rng(M + 7 * N + K)
    xq, xs, wp, ws, xd, wd = _f8_operands(rng, M, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    gam = rng.uniform(0.2, 1.5, size=N).astype(np.float32)
    if gather:
        Bb, Np, Nsrc = 7, M // 7, M // 7 + 20
        idx = np.stack([np.sort(rng.choice(Nsrc, Np, replace=False)) for _ in range(Bb)]).astype(np.int32)
        resid = rng.standard_normal((Bb, Nsrc, N)).astype(np.float32)
        r_rows = np.take_along_axis(resid, idx[:, :, None].astype(np.int64), axis=1).reshape(M, N)
        y = ops.linear(xq.reshape(Bb, Np, K), wp, N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS_RESID,
                       gamma=torch.from_numpy(gam).to(DEV), resid=torch.from_numpy(resid).to(DEV),
                       r_idx=torch.from_numpy(idx).to(DEV), w_scale=ws, x_scale=xs)
    else:
        resid = rng.standard_normal((1, M, N)).astype(np.float32)
        r_rows = resid[0]
        y = ops.linear(xq, wp, N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS_RESID, gamma=torch.from_numpy(gam).to(DEV),
                       resid=torch.from_numpy(resid).to(DEV), w_scale=ws, x_scale=xs)
    assert y.dtype == torch.float32
    want = gam * (xd @ wd.T + b) + r_rows
    got = y.cpu().numpy().reshape(M, -1)[:, :N]
    n8.check_resid_f32(got, want)


def _build_f8(cfg_name, sched, seed, std=0.06):
    cfg = ts.CONFIGS[cfg_name]
    model = ts.create_model(cfg, seed=seed, std=std, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(torch.bfloat16).eval()
    return cfg, model, w


def _oracle_fp8(cfg, model, wrapped, imgs, sched, forced):
    """(oracle with dequantised weights AND the activation-quantisation rule, oracle with dequantised weights only)"""
    sd = ts.state_dict_numpy(model)
    sd.update({k: v.cpu().numpy() for k, v in wrapped.dequantized_state_dict().items()})
    kw = dict(depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps, forced_keep=forced)
    with_act, stats = orc.vit_forward(sd, imgs, sched, act_fp8=True, **kw)
    weights_only, _ = orc.vit_forward(sd, imgs, sched, **kw)
    return with_act, weights_only, stats


# End-to-end parity of this format is a statement about a CHAOTIC quantiser.  Every kernel reproduces the stated rule to
# fp32 / bf16 rounding (the tests above: bytes equal for > 99.5 % of elements), but two runs whose inputs to a
# quantisation point differ by the bf16-level 1e-3 (device vs fp64 oracle, after one attention) round ~1 element in 12
# to the neighbouring e4m3 code - a full step where the typical rounding error is a quarter step - so from the second
# quantisation point on the two noise realisations are nearly independent (measured with tools/f8_forward_diag.py:
# device vs oracle-with-the-rule 0.084 of the logit scale, where the rule itself moves the oracle by 0.076).
# What can be held end to end: the device is no further from the oracle-with-the-rule than ~ the size of the
# perturbation the rule makes, and the perturbation stays small against the logits.
def _check_against_rule(tag, got, with_act, weights_only, scale):
    err = float(np.abs(got - with_act).max())
    cost = float(np.abs(with_act - weights_only).max())
    dev_cost = float(np.abs(got - weights_only).max())
    print(f"\nfp8_mfma {tag}: device vs oracle-with-the-rule {err:.4g} abs = {err / scale:.4g} rel; the rule's own effect on "
          f"the oracle {cost:.4g} = {cost / scale:.4g} rel; device vs oracle with dequantised weights only "
          f"{dev_cost:.4g} = {dev_cost / scale:.4g} rel (logit scale {scale:.3g})")
    assert err <= 1.6 * cost + 1e-2 * scale
    assert dev_cost <= 1.6 * cost + 1e-2 * scale
    assert cost <= 0.2 * scale
    # The maximum is the chaotic statistic; the rms over all logits is stable from run to run and is what catches a
    # wiring bug (a wrong x_scale / hidden-scale pointer, a wrong per-block bound constant): two independent
    # realisations of the same quantisation noise differ by sqrt(2) x the noise rms, a wrong scale by many times that.
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    r_err, r_cost, r_dev = rms(got - with_act), rms(with_act - weights_only), rms(got - weights_only)
    print(f"   rms: device vs oracle-with-the-rule {r_err / scale:.4g}, the rule's own effect {r_cost / scale:.4g}, device vs "
          f"weights-only oracle {r_dev / scale:.4g} of the logit scale")
    # measured (r03, five cases): r_err / r_cost 0.78-1.13, r_dev / r_cost 0.96-1.20
    assert r_err <= 1.35 * r_cost + 2e-3 * scale          # <= sqrt(2): device and oracle noise are partly correlated
    assert 0.6 * r_cost - 2e-3 * scale <= r_dev <= 1.4 * r_cost + 2e-3 * scale    # the device pays the rule's price: not less, not more


@pytest.mark.parametrize("batch", [3, 40])
def test_forward_fp8_mfma_vs_oracle_micro(batch):
    """Whole forward, C = 512 micro model, against the oracle with dequantised weights, the device's selections and the
    same activation-quantisation rule; token counts exact.  batch 3 exercises M < 256 launches (clamped rows)."""
    sched = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
    cfg, model, w = _build_f8("vit_micro512_patch16_64", sched, seed=4)
    w.set_weight_format("fp8_mfma")
    imgs = bf16_round_np(np.random.default_rng(9).standard_normal((batch, 3, 64, 64), dtype=np.float32))
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    again = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert np.array_equal(got, again)                      # deterministic: the same input gives the same bytes
    forced = {i: t["keep_idx"].cpu().numpy() for i, t in w.get_last_trace().items()}
    with_act, weights_only, stats = _oracle_fp8(cfg, model, w, imgs, sched, forced)
    assert stats == w.get_last_stats()
    _check_against_rule(f"micro512 batch {batch}", got, with_act, weights_only, float(np.abs(weights_only).max()))


def test_forward_fp8_mfma_single_block_is_tight():
    """With ONE block the inputs of the first two quantisation points agree to fp32 rounding between device and oracle,
    so the rule can be checked end to end without the chaos of a deep stack: qkv sees bit-equal e4m3 rows (up to
    boundary cases) and the logits must agree inside the rule's own effect.  (The attention-output point is different:
    the device's attention is a bf16-operand computation, ~1e-2 from the oracle's fp64 one, so a few per cent of its
    elements land on the other side of an e4m3 boundary - a 2^-3 relative step each - which is most of what is left.)"""
    import dataclasses
    cfg = dataclasses.replace(ts.CONFIGS["vit_micro512_patch16_64"], depth=1)
    model = ts.create_model(cfg, seed=6, std=0.06, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, {}).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8_mfma")
    imgs = bf16_round_np(np.random.default_rng(3).standard_normal((32, 3, 64, 64), dtype=np.float32))
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    with_act, weights_only, _ = _oracle_fp8(cfg, model, w, imgs, {}, None)
    scale = float(np.abs(weights_only).max())
    err, cost = float(np.abs(got - with_act).max()), float(np.abs(with_act - weights_only).max())
    r_err = float(np.sqrt(np.mean((got - with_act) ** 2)))
    r_cost = float(np.sqrt(np.mean((with_act - weights_only) ** 2)))
    print(f"\nfp8_mfma depth 1: device vs oracle-with-the-rule {err / scale:.4g} rel (rms {r_err / scale:.4g}), the rule's own effect "
          f"{cost / scale:.4g} rel (rms {r_cost / scale:.4g})")
    assert err <= 0.8 * cost + 1e-2 * scale
    assert r_err <= 0.7 * r_cost + 2e-3 * scale


@pytest.mark.parametrize("name", ["base224_fp32", "deit3_fp32", "large384_fp32"])
def test_forward_fp8_mfma_fixtures(name):
    """ViT-B / DeiT-3-B dims (configs[4]'s model) on the reference fixtures, the reference's selections injected:
    against the oracle on dequantised operands with the rule, and the reported cost of the whole quantisation (weights
    + activations) against the reference's fp32 logits."""
    meta, data = load_case(name)
    cfg = ts.CONFIGS[meta["cfg_name"]]
    model = ts.create_model(cfg, seed=meta["seed"], std=meta["std"], bias_std=meta["bias_std"], round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, meta["schedule"]).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8_mfma")
    imgs = case_images(meta, data)
    forced = {i: data[f"blk{i}.keep_idx"] for i in pruned_blocks(meta)}
    w.force_keep_idx({i: torch.from_numpy(v).to(DEV) for i, v in forced.items()})
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == data["token_counts"].tolist()
    with_act, weights_only, _ = _oracle_fp8(cfg, model, w, imgs, meta["schedule"], forced)
    scale = float(np.abs(data["logits"]).max())
    _check_against_rule(name, got, with_act, weights_only, scale)
    total = float(np.abs(got - data["logits"]).max())
    print(f"   whole quantisation (e4m3 weights + activations) vs the reference's fp32 logits: {total:.4g} abs = {total / scale:.4g} rel")
    assert total <= 0.35 * scale


def test_fp8_mfma_refuses_unsupported_shapes():
    """Embed dims that are not multiples of 256 (ViT-Ti: 192) are refused, not mis-computed."""
    cfg = ts.CONFIGS["vit_micro_patch16_64"]            # C = 128
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=1), {}).to(DEV).to(torch.bfloat16).eval()
    w.set_weight_format("fp8_mfma")
    with pytest.raises(NotImplementedError, match="act_fp8"):
        w(torch.randn(2, 3, 64, 64, device=DEV))
