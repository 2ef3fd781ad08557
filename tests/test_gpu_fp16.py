"""fp16 models: every HIP kernel in its float16 form, called through the C ABI (rajni_amd.ops -> librajni_hip.so), and the
whole forward of an fp16 model.  GPU box only (`-m gpu`).

Tolerances: inputs are fp16-representable, the oracle is fp64 on the same values.  What may legitimately differ is the
fp32 accumulation order plus ONE fp16 rounding of a 16-bit output (rel 2^-11 ~ 4.9e-4 of the element), so the 16-bit
outputs are held to 2e-3 of the tensor's scale where the bf16 tests of the same cases use 1e-2 (bf16: 2^-8 per rounding).
Attention rounds P to fp16 for the PV product as well: 4e-3 where bf16 uses 1.5e-2.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from oracle import rajni_oracle as orc
from rajni_amd import ops, timm_shaped as ts, _native as nat
from helpers import load_case, case_state_dict, case_images, pruned_blocks

DEV = "cuda"
F16 = torch.float16
REL16 = 2e-3          # one fp16 output rounding + fp32 accumulation
REL16_ATTN = 4e-3     # ... and P rounded to fp16


def f16_round_np(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(F16)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def close(got, want, rel, what=""):
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max()
    assert err <= rel * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g})"


# ---------------------------------------------------------------------------------------------
# GEMM + epilogues
# ---------------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1, 4, 5], ids=["auto", "small128x128", "wide256x256", "mid256x128"])
def tiling(request):
    nat.lib().rajni_debug_force_gemm_tiling(request.param)
    yield request.param
    nat.lib().rajni_debug_force_gemm_tiling(0)


@pytest.mark.parametrize("M,N,K", [(394, 2304, 768), (256, 768, 768), (130, 3072, 768), (346, 768, 3072),
                                   (7, 1000, 768), (64, 10, 128), (1, 192, 192), (513, 260, 128), (2100, 384, 64)])
def test_linear_bias_f16(M, N, K, tiling):
    rng = np.random.default_rng(M * 7 + N)
    x = f16_round_np(rng.standard_normal((M, K), dtype=np.float32))
    w = f16_round_np(rng.standard_normal((N, K), dtype=np.float32) * 0.05)
    b = f16_round_np(rng.standard_normal(N, dtype=np.float32))
    y = ops.linear(dev16(x), ops.pack_weight(dev16(w), F16), N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS)
    assert y.dtype == F16 and tuple(y.shape) == (M, N)
    close(host(y), x.astype(np.float64) @ w.astype(np.float64).T + b, REL16, f"linear f16 {M}x{N}x{K}")


def test_linear_identity_exact_beyond_bf16(tiling):
    """A = I against a weight of 11-bit integers: exact in fp16, NOT in bf16 - only the f16 MFMA and f16 stores
    reproduce it bit for bit (a bf16 conversion anywhere on the path loses the low bits)."""
    K = N = M = 256
    x = np.eye(M, K, dtype=np.float32)
    w = ((np.arange(N * K, dtype=np.float32).reshape(N, K) * 37) % 2047) - 1023.0
    y = ops.linear(dev16(x), ops.pack_weight(dev16(w), F16), N, None, nat.EPI_BIAS)
    np.testing.assert_array_equal(host(y), w.T.astype(np.float64))


def test_linear_gelu_f16(tiling):
    rng = np.random.default_rng(5)
    M, N, K = 300, 512, 256
    x = f16_round_np(rng.standard_normal((M, K), dtype=np.float32))
    w = f16_round_np(rng.standard_normal((N, K), dtype=np.float32) * 0.1)
    b = f16_round_np(rng.standard_normal(N, dtype=np.float32) * 0.1)
    y = ops.linear(dev16(x), ops.pack_weight(dev16(w), F16), N, torch.from_numpy(b).to(DEV), nat.EPI_BIAS_GELU)
    close(host(y), orc.gelu(x.astype(np.float64) @ w.astype(np.float64).T + b), REL16, "linear+gelu f16")


@pytest.mark.parametrize("stream_f32", [False, True], ids=["f16stream", "f32stream"])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("B,Nsrc,Np,Cc,K", [(3, 50, 37, 256, 192), (150, 197, 173, 768, 768), (9, 65, 40, 384, 1536)])
def test_linear_resid_f16(B, Nsrc, Np, Cc, K, gather, stream_f32, tiling):
    rng = np.random.default_rng(Cc + K + gather)
    x = f16_round_np(rng.standard_normal((B, Np if gather else Nsrc, K), dtype=np.float32))
    w = f16_round_np(rng.standard_normal((Cc, K), dtype=np.float32) * 0.05)
    b = f16_round_np(rng.standard_normal(Cc, dtype=np.float32) * 0.1)
    gam = f16_round_np(rng.standard_normal(Cc, dtype=np.float32))
    resid = rng.standard_normal((B, Nsrc, Cc), dtype=np.float32)
    resid = resid if stream_f32 else f16_round_np(resid)
    idx = np.stack([np.sort(rng.choice(Nsrc, Np, replace=False)) for _ in range(B)]).astype(np.int32)
    rdev = torch.from_numpy(resid).to(DEV) if stream_f32 else dev16(resid)
    y = ops.linear(dev16(x), ops.pack_weight(dev16(w), F16), Cc, torch.from_numpy(b).to(DEV), nat.EPI_BIAS_RESID,
                   gamma=torch.from_numpy(gam).to(DEV), resid=rdev,
                   r_idx=torch.from_numpy(idx).to(DEV) if gather else None)
    lin = x.reshape(-1, K).astype(np.float64) @ w.astype(np.float64).T + b
    r = orc.gather_rows(resid.astype(np.float64), idx.astype(np.int64)) if gather else resid.astype(np.float64)
    want = r.reshape(-1, Cc) + gam * lin
    assert y.dtype == (torch.float32 if stream_f32 else F16)
    close(host(y).reshape(want.shape), want, 1e-5 if stream_f32 else REL16, "linear+resid f16")


def test_linear_f16_rejects_fp8_weights():
    w8, s8 = ops.pack_weight_fp8(torch.randn(256, 256, device=DEV), torch.bfloat16)
    x = torch.randn(8, 256, device=DEV).to(F16)
    with pytest.raises(NotImplementedError, match="bf16 model"):
        ops.linear(x, w8, 256, None, nat.EPI_BIAS, w_scale=s8)


# ---------------------------------------------------------------------------------------------
# LayerNorm, gather
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("x_f32", [False, True])
@pytest.mark.parametrize("rows,Cc", [(394, 768), (5, 192), (33, 1024), (4097, 768), (4100, 384), (4096, 1280)])
def test_layernorm_f16(rows, Cc, x_f32):
    rng = np.random.default_rng(rows)
    x = rng.standard_normal((rows, Cc), dtype=np.float32) * 2 + 0.5
    if not x_f32:
        x = f16_round_np(x)
    w = f16_round_np(1 + 0.1 * rng.standard_normal(Cc, dtype=np.float32))
    b = f16_round_np(0.1 * rng.standard_normal(Cc, dtype=np.float32))
    xd = torch.from_numpy(x).to(DEV) if x_f32 else dev16(x)
    y = ops.layernorm(xd, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), 1e-6, out_dtype=F16)
    assert y.dtype == F16
    close(host(y), orc.layer_norm(x.astype(np.float64), w, b, 1e-6), REL16, "layernorm f16")


@pytest.mark.parametrize("x_f32", [False, True])
def test_layernorm_f16_strided_cls_rows(x_f32):
    rng = np.random.default_rng(1)
    B, N, Cc = 6, 11, 256
    x = rng.standard_normal((B, N, Cc), dtype=np.float32)
    x = x if x_f32 else f16_round_np(x)
    xd = torch.from_numpy(x).to(DEV) if x_f32 else dev16(x)
    w, b = np.ones(Cc, np.float32), np.zeros(Cc, np.float32)
    y = ops.layernorm(xd, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), 1e-6, rows=B, row_stride=N * Cc,
                      out_dtype=F16)
    close(host(y), orc.layer_norm(x[:, 0].astype(np.float64), w, b, 1e-6), REL16, "layernorm f16 cls rows")


def test_gather_rows_f16_bit_exact():
    rng = np.random.default_rng(2)
    B, N, K, E = 4, 197, 173, 2304
    src = dev16(rng.standard_normal((B, N, E), dtype=np.float32))
    idx = np.stack([np.sort(rng.choice(N, K, replace=False)) for _ in range(B)]).astype(np.int32)
    got = ops.gather_rows(src, torch.from_numpy(idx).to(DEV))
    want = torch.gather(src, 1, torch.from_numpy(idx).long().to(DEV).unsqueeze(-1).expand(-1, -1, E))
    assert got.dtype == F16 and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------
# importance + selection
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,H,D", [(4, 197, 12, 64), (2, 577, 16, 64), (3, 17, 2, 64), (2, 87, 3, 32), (2, 61, 4, 80)])
def test_importance_and_score_select_f16(B, N, H, D):
    rng = np.random.default_rng(N * H + D)
    qkv = f16_round_np(rng.standard_normal((B, N, 3 * H * D), dtype=np.float32))
    keep = orc.keep_count(0.7, N)
    scores, idx, nxt = ops.score_select(dev16(qkv), H, keep)
    assert scores.dtype == F16 and nxt.dtype == F16
    s = host(scores)
    want = orc.importance_scores(qkv, H)
    # the kernel returns fp16(fp32 score): within one fp16 rounding of the exact value (plus fp32 noise)
    assert np.all(np.abs(s - want) <= np.abs(want) * 2.0 ** -10 + 1e-7), float(np.abs(s - want).max())
    np.testing.assert_array_equal(idx.cpu().numpy(), orc.select_tokens(s, keep))
    np.testing.assert_array_equal(host(nxt), np.take_along_axis(s, idx.cpu().numpy().astype(np.int64), axis=1))
    assert torch.equal(ops.importance(dev16(qkv), H), scores)


@pytest.mark.parametrize("N", [2, 5, 64, 129, 197, 258, 577, 1030])
def test_select_f16_special_values_and_slice_boundaries(N):
    rng = np.random.default_rng(N)
    B = 7
    vals = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 6e-8, -6e-8, 3.0e-3, 3.0e-3, 2.0 ** -7, -(2.0 ** -7), 0.5,
                     0.5, 65504.0, -65504.0], dtype=np.float32)
    s = rng.choice(vals, size=(B, N)).astype(np.float32)
    s[1] = np.where(rng.random(N) < 0.5, np.float32(0.0), np.float32(-0.0))
    s[2] = rng.standard_normal(N).astype(np.float32)
    s[2, ::3] = s[2, 0]
    # scores that differ only BELOW bf16 precision: 1 + k * 2^-10 share their upper 16 fp32 bits in groups of 8
    s[3] = 1.0 + rng.integers(0, 64, N).astype(np.float32) * 2.0 ** -10
    s[4] = -(0.25 + rng.integers(0, 64, N).astype(np.float32) * 2.0 ** -12)
    s = f16_round_np(s)
    t = torch.from_numpy(s).to(DEV).to(F16)
    for keep in sorted({1, max(1, (N - 1) // 2), max(1, N - 2), N - 1}):
        idx, nxt = ops.select_topk(t, keep)
        want = orc.select_tokens(s, keep)
        np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"N={N} keep={keep}")
        assert np.array_equal(nxt.float().cpu().numpy(), np.take_along_axis(s, want, axis=1), equal_nan=True)


def test_select_f16_below_bf16_precision():
    """Scores 1 + k/1024: distinct in fp16, equal in bf16 within groups of eight.  Ranking on the upper half of the fp32
    pattern (the bf16 key) would break these by index instead of by value."""
    B, N = 3, 197
    rng = np.random.default_rng(11)
    s = np.zeros((B, N), np.float32)
    for b in range(B):
        s[b, 1:] = 1.0 + rng.permutation(N - 1).astype(np.float32) * 2.0 ** -10
    s = f16_round_np(s)
    assert len(np.unique(s[0, 1:])) == N - 1
    for keep in (1, 7, 98, 150):
        idx, _ = ops.select_topk(dev16(s), keep)
        want = orc.select_tokens(s, keep)
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        top = np.argsort(-s[:, 1:], axis=1, kind="stable")[:, :keep] + 1
        np.testing.assert_array_equal(idx.cpu().numpy()[:, 1:], np.sort(top, axis=1))


@pytest.mark.parametrize("B,N,H,D", [(5, 197, 12, 64), (3, 404, 16, 64), (4, 87, 4, 32), (2, 152, 2, 128)])
def test_score_select_f16_one_pass_equals_two_pass(B, N, H, D):
    rng = np.random.default_rng(N + H)
    t = dev16(rng.standard_normal((B, N, 3 * H * D), dtype=np.float32))
    keep = orc.keep_count(0.8, N)
    try:
        nat.lib().rajni_debug_force_score_two_pass(1)
        s2, i2, n2 = ops.score_select(t, H, keep)
    finally:
        nat.lib().rajni_debug_force_score_two_pass(0)
    s1, i1, n1 = ops.score_select(t, H, keep)
    assert torch.equal(s1, s2) and torch.equal(i1, i2) and torch.equal(n1, n2)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1, 2], ids=["persistent", "online_chunked", "full_row"])
def attn_mode(request):
    nat.lib().rajni_debug_force_attention(request.param)
    yield request.param
    nat.lib().rajni_debug_force_attention(0)


def _attn_case(B, N, Np, H, D, seed):
    rng = np.random.default_rng(seed)
    qkv = f16_round_np(rng.standard_normal((B, N, 3 * H * D), dtype=np.float32))
    if Np == N:
        idx, idx_t, g = None, None, qkv
    else:
        idx = np.stack([np.concatenate([[0], 1 + np.sort(rng.choice(N - 1, Np - 1, replace=False))]) for _ in range(B)])
        idx_t = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        g = orc.gather_rows(qkv, idx.astype(np.int64))
    out = ops.attention(dev16(qkv), idx_t, H, D ** -0.5)
    q, k, v = orc.split_heads(g.astype(np.float64), H)
    assert out.dtype == F16 and tuple(out.shape) == (B, Np, H * D)
    return host(out), orc.softmax_attention(q, k, v, D ** -0.5)


@pytest.mark.parametrize("B,N,Np,H", [(2, 197, 173, 12), (1, 577, 404, 16), (3, 17, 13, 2), (2, 87, 87, 3),
                                      (1, 130, 129, 1), (2, 40, 2, 2), (1, 300, 257, 2), (2, 256, 256, 2)])
def test_attention_f16_d64(B, N, Np, H, attn_mode):
    got, want = _attn_case(B, N, Np, H, 64, N * 31 + Np)
    close(got, want, REL16_ATTN, "attention f16")


@pytest.mark.parametrize("D", [8, 16, 32, 40, 64, 80, 96, 128])
def test_attention_f16_head_dims(D):
    got, want = _attn_case(2, 101, 77, 3, D, D)
    close(got, want, REL16_ATTN, f"attention f16 D={D}")


def test_attention_f16_online_softmax_spike(attn_mode):
    rng = np.random.default_rng(3)
    B, N, H = 1, 200, 1
    qkv = rng.standard_normal((B, N, 192), dtype=np.float32) * 0.3
    qkv[0, 5, 0:64] = 4.0
    qkv[0, 170, 64:128] = 4.0
    qkv = f16_round_np(qkv)
    out = ops.attention(dev16(qkv), None, H, 64 ** -0.5)
    q, k, v = orc.split_heads(qkv.astype(np.float64), H)
    close(host(out), orc.softmax_attention(q, k, v, 64 ** -0.5), REL16_ATTN, "attention f16 spike")


# ---------------------------------------------------------------------------------------------
# patch embed
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("S,P,Cc,B,has_cls", [(64, 16, 128, 3, True), (224, 16, 192, 2, True), (64, 16, 128, 2, False),
                                              (32, 8, 64, 5, True), (96, 32, 192, 2, True),
                                              (56, 14, 128, 3, True), (224, 14, 320, 2, False)])
def test_patch_embed_f16(S, P, Cc, B, has_cls, out_f32, tiling):
    rng = np.random.default_rng(S + Cc)
    img = f16_round_np(rng.standard_normal((B, 3, S, S), dtype=np.float32))
    w = f16_round_np(rng.standard_normal((Cc, 3, P, P), dtype=np.float32) * 0.05)
    b = f16_round_np(rng.standard_normal(Cc, dtype=np.float32) * 0.1)
    cls = f16_round_np(rng.standard_normal(Cc, dtype=np.float32))
    npatch = (S // P) ** 2
    pos = f16_round_np(rng.standard_normal((npatch + int(has_cls), Cc), dtype=np.float32))
    x = ops.patch_embed(dev16(img), ops.pack_weight(dev16(w), F16, k_multiple=64), torch.from_numpy(b).to(DEV), dev16(cls),
                        dev16(pos), has_cls, P, Cc, out_f32=out_f32)
    assert x.dtype == (torch.float32 if out_f32 else F16)
    tok = orc.patch_embed(img.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
    if has_cls:
        want = np.concatenate([np.broadcast_to(cls, (B, 1, Cc)), tok], axis=1) + pos[None]
    else:
        want = np.concatenate([np.broadcast_to(cls, (B, 1, Cc)), tok + pos[None]], axis=1)
    close(host(x), want, 1e-5 if out_f32 else REL16, "patch embed f16")


# ---------------------------------------------------------------------------------------------
# whole forward of an fp16 model
# ---------------------------------------------------------------------------------------------

CASES = ["micro_fp32", "microd80_fp32", "microp14_fp32", "tiny224_fp32", "base224_fp32", "deit3_fp32", "large384_fp32"]


def build(meta, dtype=F16):
    cfg = ts.CONFIGS[meta["cfg_name"]]
    model = ts.create_model(cfg, seed=meta["seed"], std=meta["std"], bias_std=meta["bias_std"], round_bf16=True)
    return cfg, rajni_amd.RAJNIViTWrapper(model, meta["schedule"]).to(DEV).to(dtype).eval()


def _forced(meta, data):
    return {i: torch.from_numpy(data[f"blk{i}.keep_idx"]).to(DEV) for i in pruned_blocks(meta)}


@pytest.mark.parametrize("mode", ["f32stream", "f16stream", "cls_only"])
@pytest.mark.parametrize("name", CASES)
def test_forward_f16_selection_conditional(name, mode):
    meta, data = load_case(name)
    cfg, wrapped = build(meta)
    if mode == "f16stream":
        wrapped.set_residual_dtype(F16)
    if mode == "cls_only":
        wrapped.set_last_block_cls_only(True)
    wrapped.force_keep_idx(_forced(meta, data))
    logits = wrapped(torch.from_numpy(case_images(meta, data)).to(DEV))
    assert logits.dtype == F16
    logits = logits.float().cpu().numpy()
    assert wrapped.get_last_stats()["token_counts"] == data["token_counts"].tolist()
    ref = data["logits"]
    scale = np.abs(ref).max()
    err = np.abs(logits - ref).max()
    assert err <= 1e-2 * scale, f"{name} {mode}: max |dlogit| {err:.4g} vs scale {scale:.4g}"
    for i in pruned_blocks(meta):
        assert wrapped.get_last_trace()[i]["next_scores"].dtype == F16


@pytest.mark.parametrize("name", CASES)
def test_forward_f16_free_running(name):
    meta, data = load_case(name)
    cfg, wrapped = build(meta)
    wrapped.trace_scores(True)
    images_np = case_images(meta, data)
    logits = wrapped(torch.from_numpy(images_np).to(DEV)).float().cpu().numpy()
    assert wrapped.get_last_stats()["token_counts"] == data["token_counts"].tolist()
    tr = wrapped.get_last_trace()
    forced = {}
    for i in pruned_blocks(meta):
        assert tr[i]["scores"].dtype == F16
        s = tr[i]["scores"].float().cpu().numpy().astype(np.float64)
        idx = tr[i]["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, orc.select_tokens(s, idx.shape[1] - 1))
        forced[i] = idx
    _, sd = case_state_dict(meta)
    sd16 = {k: f16_round_np(v) for k, v in sd.items()}
    want, stats = orc.vit_forward(sd16, f16_round_np(images_np), meta["schedule"], depth=cfg.depth,
                                  num_heads=cfg.num_heads, ln_eps=cfg.ln_eps, forced_keep=forced, dtype=np.float32)
    scale = np.abs(want).max()
    err = np.abs(logits - want).max()
    assert err <= 1e-2 * scale, f"{name}: max |dlogit| {err:.4g} vs scale {scale:.4g}"
    assert stats["token_counts"] == wrapped.get_last_stats()["token_counts"]


def test_forward_f16_matches_reference_fp16_run():
    """base224_fp16: the reference wrapper run in fp16 on CPU.  With its selections injected, the fp32-stream fp16 build
    is no further from the fp32 computation than the reference's own fp16 run is.  The fp32 computation is the fp64
    oracle of the same model with the SAME selections: the reference's fp32 run (base224_fp32) picked other tokens in
    places, and that selection difference, not arithmetic, sets most of either run's distance to its logits
    (both ~1.4 % of the logit scale), so it is checked only against the fixture-level 2e-2 bar."""
    meta16, data16 = load_case("base224_fp16")
    cfg, wrapped = build(meta16)
    forced = _forced(meta16, data16)
    wrapped.force_keep_idx(forced)
    images = case_images(meta16, data16)
    logits = wrapped(torch.from_numpy(images).to(DEV)).float().cpu().numpy().astype(np.float64)
    assert wrapped.get_last_stats()["token_counts"] == data16["token_counts"].tolist()
    _, sd = case_state_dict(meta16)
    want, _ = orc.vit_forward({k: f16_round_np(v) for k, v in sd.items()}, f16_round_np(images), meta16["schedule"],
                              depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps,
                              forced_keep={i: t.cpu().numpy() for i, t in forced.items()})
    ref16 = data16["logits"].astype(np.float64)
    ours, theirs = np.abs(logits - want).max(), np.abs(ref16 - want).max()
    assert ours <= theirs, f"fp16 build {ours:.4g} vs the reference's fp16 run {theirs:.4g} (scale {np.abs(want).max():.4g})"
    ref32 = load_case("base224_fp32")[1]["logits"]
    assert np.abs(logits - ref32).max() <= 2e-2 * np.abs(ref32).max()


def test_forward_f16_256_images_agree_at_least_as_well_as_bf16():
    meta, data = load_case("base224_agree256")
    images = torch.from_numpy(case_images(meta, data)).to(DEV)
    ref = data["logits"]
    scale = np.abs(ref).max()
    res = {}
    for dt in (torch.bfloat16, F16):
        cfg, wrapped = build(meta, dt)
        wrapped.force_keep_idx(_forced(meta, data))
        lg = wrapped(images).float().cpu().numpy()
        res[dt] = (np.abs(lg - ref).max(), float((lg.argmax(1) == ref.argmax(1)).mean()))
    (e16, a16), (eb, ab) = res[F16], res[torch.bfloat16]
    assert e16 <= 1e-2 * scale, (e16, scale)
    assert e16 <= eb and a16 >= ab, f"fp16 |dlogit| {e16:.4g} top-1 {a16:.4f}; bf16 {eb:.4g} {ab:.4f}"


def test_forward_f16_refuses_mismatched_stream_and_fp8():
    meta, data = load_case("micro_fp32")
    images = torch.from_numpy(case_images(meta, data)).to(DEV)
    cfg, wrapped = build(meta)
    wrapped.set_residual_dtype(torch.bfloat16)
    with pytest.raises(ValueError, match="residual stream"):
        wrapped(images)
    wrapped.set_residual_dtype(torch.float32)
    for fmt in ("fp8", "fp8_mfma"):
        wrapped.set_weight_format(fmt)
        with pytest.raises(NotImplementedError, match="bf16 model"):
            wrapped(images)
    cfg, wb = build(meta, torch.bfloat16)
    wb.set_residual_dtype(F16)
    with pytest.raises(ValueError, match="residual stream"):
        wb(images)
