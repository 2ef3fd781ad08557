"""QuickGELU MLPs on the device: the epilogue RAJNI_EPI_BIAS_QUICK_GELU of rajni_linear in every tiling and operand type, and
whole forwards of QuickGELU models (rajni_vit_ext.mlp_act).  GPU box only (`-m gpu`).

What pins the FUNCTION is the epilogue sweep: biases only (zero operands, so the pre-activation is the fp32 bias exactly), on
nm.gelu_grid() plus the largest finite value of the type, element by element against fp64 x * sigmoid(1.702 x) with the
project's existing activation allowances - 16 bits: u_out |want| + A_GELU_16 (5e-5) + floor, which exact GELU misses at over
130 000 grid points (tests/test_activations_cpu.py); fp32: max(4 x the local error envelope of torch's CPU fp32 evaluation,
2 u32 |want|) + floor.  The GEMM budgets then hold random operands to tests/numerics_activations.py::budget_act, and the
forwards show the epilogue wired into the model: the project's bars (1e-2 x max|logit| for 16-bit models, 1e-3 for fp32, 2e-2
for the 16-bit residual stream), after the CPU has shown that ignoring the activation moves the fp32 logits by at least 5x
the fp32 bar."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_activations as na
import rajni_amd
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import ops, _native as nat, timm_shaped as ts

DEV = "cuda"
F32 = np.float32
QGELU = nat.EPI_BIAS_QUICK_GELU
TILING_IDS = {0: "auto", 1: "small128x128", 4: "wide256x256", 5: "mid256x128"}


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if dt == "fp32" else t.to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


@pytest.fixture
def tiling(request):
    """forces a GEMM tiling (rajni_debug_force_gemm_tiling): 0 = by shape, 1 = 128x128, 4 = 256x256, 5 = 256x128"""
    nat.lib().rajni_debug_force_gemm_tiling(request.param)
    yield request.param
    nat.lib().rajni_debug_force_gemm_tiling(0)


TILINGS = pytest.mark.parametrize("tiling", [0, 1, 4, 5], indirect=True, ids=list(TILING_IDS.values()))


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: epilogue sweeps through the bias path
# ---------------------------------------------------------------------------------------------------------------

def through_bias(bias32, dt, epilogue, tiling=0):
    """epi(0 W^T + bias) for a vector of fp32 biases (tests/test_gpu_numerics.py::through_bias): 261 rows x K 256 where a
    persistent tiling is forced (one full row tile and a ragged one: interior and guarded epilogue paths), else 5 rows x K 64"""
    n = len(bias32)
    rows, K = (261, 256) if tiling in (4, 5) else (5, 64)
    x = torch.zeros((rows, K), dtype=nm.TORCH[dt], device=DEV)
    w = torch.zeros(((n + 255) // 256 * 256, K), dtype=nm.TORCH[dt], device=DEV)
    y = ops.linear(x, w, n, torch.from_numpy(np.ascontiguousarray(bias32, dtype=F32)).to(DEV), epilogue)
    assert tuple(y.shape) == (rows, n)
    assert bool((y == y[:1]).logical_or(y.isnan() & y[:1].isnan()).all()), "rows of a launch with identical inputs differ"
    return y[0].cpu()


_sweep_want = {}


def sweep_reference(dt):
    if dt not in _sweep_want:
        b = na.sweep_grid(dt)
        _sweep_want[dt] = (b, na.quick_gelu64(b.astype(np.float64)))
    return _sweep_want[dt]


@TILINGS
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_quick_gelu_epilogue_on_chosen_preactivations_16bit(dt, tiling):
    """|y - quick_gelu64(b)| <= u_out |want| + A_GELU_16 + floor, and every output finite: on [-8, 8], for +-2^3 .. 2^13 and for
    the largest finite +- value of the type, where exp2 overflows (rcp(inf) = 0: the result is -0, not NaN) or underflows"""
    b, want = sweep_reference(dt)
    got = np.concatenate([host(through_bias(b[i:i + 70000], dt, QGELU, tiling)) for i in range(0, len(b), 70000)])
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite outputs, first at bias {b[~np.isfinite(got)][0]!r}"
    over = np.maximum(np.abs(got - want) - nm.UNIT[dt] * np.abs(want), 0)
    print(f"[activations] quick_gelu {dt} tiling {tiling}: max (|err| - u_out |want|) {over.max():.4g}; at the type's ends "
          f"{got[-2]!r} {got[-1]!r}")
    assert got[b == 0].tolist() == [0.0]                       # act(0) = 0 exactly: the zero-padded hidden columns
    nm.assert_within(got, want, nm.UNIT[dt] * np.abs(want) + nm.A_GELU_16 + nm.FLOOR[dt], f"quick_gelu sweep {dt} tiling {tiling}")


def test_quick_gelu_epilogue_on_chosen_preactivations_fp32():
    """fp32 models (expf and a true division): the project's fp32 GELU rule with QuickGELU's own envelope -
    max(4 x the local error of torch's CPU fp32 x * sigmoid(1.702 x) against fp64, 2 u32 |want|) + floor"""
    b, want = sweep_reference("fp32")
    ref = na.act32_reference_error("quick_gelu", b)
    print(f"[activations] quick_gelu fp32: torch CPU reference max |err| {ref.max():.4g}")
    got = host(through_bias(b, "fp32", QGELU))
    assert np.isfinite(got).all() and got[b == 0].tolist() == [0.0]
    nm.assert_within(got, want, np.maximum(4 * ref, 2 * nm.U32 * np.abs(want)) + nm.FLOOR["fp32"], "quick_gelu sweep fp32")


# ---------------------------------------------------------------------------------------------------------------
# 3: GEMM budgets, random operands
# ---------------------------------------------------------------------------------------------------------------
_cache = {}


def gemm_reference(M, N, K, dt, w8=False):
    """operands, fp64 pre-activation, |x||W|^T + |b| and g (nm.gemm_pre), shared by the cases that differ in tiling only"""
    key = (M, N, K, dt, w8)
    if key not in _cache:
        if len(_cache) >= 3:
            _cache.pop(next(iter(_cache)))
        x, w, b = nm.gemm_operands(M, N, K, dt)
        extra = None
        if w8:      # e4m3 weights with one fp32 scale per row: want and S use the dequantised weight
            q, s = ops.pack_weight_fp8(torch.from_numpy(w), nm.TORCH[dt])
            w = (q[:N].view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64) * s.to(torch.float64)[:, None]).numpy()
            extra = (q, s)
        _cache[key] = (x, w, b) + nm.gemm_pre(x, w, b) + (extra,)
    return _cache[key]


# (394, 2304, 768) reaches the persistent tilings when they are forced; the others run 128 x 128 whatever is asked (M < 256
# or K < 192: choose_gemm), so they are launched once
SHAPES_16 = [(7, 1000, 768, 0), (130, 3072, 768, 0), (513, 260, 128, 0)] + [(394, 2304, 768, t) for t in (0, 1, 4, 5)]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K,tiling", SHAPES_16, indirect=["tiling"], ids=[f"{m}x{n}x{k}-{TILING_IDS[t]}" for m, n, k, t in SHAPES_16])
def test_quick_gelu_gemm_budgets_16bit(M, N, K, tiling, dt):
    x, w, b, pre, S, g, _ = gemm_reference(M, N, K, dt)
    y = ops.linear(dev(x, dt), ops.pack_weight(dev(w, dt), nm.TORCH[dt]), N, dev(b, "fp32"), QGELU)
    assert tuple(y.shape) == (M, N) and y.dtype == nm.TORCH[dt]
    nm.assert_within(host(y), na.quick_gelu64(pre), na.budget_act("quick_gelu", pre, S, g, dt, nm.A_GELU_16),
                     f"gemm QUICK_GELU {dt} {M}x{N}x{K} tiling {tiling}")


@pytest.mark.parametrize("M,N,K", [s[:3] for s in SHAPES_16[:4]])
def test_quick_gelu_gemm_budgets_fp32(M, N, K):
    x, w, b, pre, S, g, _ = gemm_reference(M, N, K, "fp32")
    y = ops.linear(dev(x, "fp32"), ops.pack_weight(dev(w, "fp32"), torch.float32), N, dev(b, "fp32"), QGELU)
    assert tuple(y.shape) == (M, N) and y.dtype == torch.float32
    nm.assert_within(host(y), na.quick_gelu64(pre), na.budget_act("quick_gelu", pre, S, g, "fp32", na.a_act_fp32("quick_gelu", pre)),
                     f"gemm QUICK_GELU fp32 {M}x{N}x{K}")


@TILINGS
def test_quick_gelu_gemm_budgets_fp8_weights(tiling):
    M, N, K = 394, 2304, 768
    x, w, b, pre, S, g, (q, s) = gemm_reference(M, N, K, "bf16", w8=True)
    y = ops.linear(dev(x, "bf16"), q.to(DEV), N, dev(b, "fp32"), QGELU, w_scale=s.to(DEV))
    nm.assert_within(host(y), na.quick_gelu64(pre), na.budget_act("quick_gelu", pre, S, g, "bf16", nm.A_GELU_16),
                     f"gemm QUICK_GELU bf16 x e4m3 weights {M}x{N}x{K} tiling {tiling}")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_quick_gelu_output_with_a_padded_row_stride_stays_inside_its_view(dt):
    """N = 260 (a ragged column tile), ldc = 288, the output poisoned first: every element of the view is written, columns
    >= N of every row (the stride gap) and the rows >= M (the guard behind the view) keep the poison, and the values meet
    the budget"""
    M, N, K, ldc = 513, 260, 128, 288
    x, w, b, pre, S, g, _ = gemm_reference(M, N, K, dt)
    tdt = nm.TORCH[dt]
    xd, wd, bd = dev(x, dt), ops.pack_weight(dev(w, dt), tdt), dev(b, "fp32")
    yg = Guarded((M, N), tdt, DEV, row_stride=ldc)
    a = nat.LinearArgs()
    a.x, a.lda, a.w, a.ldw, a.bias = xd.data_ptr(), K, wd.data_ptr(), wd.shape[1], bd.data_ptr()
    a.y, a.ldc, a.M, a.N, a.K, a.epilogue, a.dtype = yg.ptr(), ldc, M, N, K, QGELU, nat.dtype_code(tdt)
    nat.check(nat.lib().rajni_linear(C.byref(a), nat.stream_ptr()), "rajni_linear")
    torch.cuda.synchronize()
    yg.check(f"QUICK_GELU {dt} {M}x{N}x{K} ldc {ldc}: y")
    a_act = nm.A_GELU_16 if dt != "fp32" else na.a_act_fp32("quick_gelu", pre)
    nm.assert_within(host(yg.t), na.quick_gelu64(pre), na.budget_act("quick_gelu", pre, S, g, dt, a_act),
                     f"gemm QUICK_GELU {dt} {M}x{N}x{K} ldc {ldc}")


def test_quick_gelu_on_the_fp8_matrix_pipe_is_refused():
    M, N, K = 256, 512, 512
    x8 = torch.zeros((M, K), dtype=torch.uint8, device=DEV)
    w8 = torch.zeros((N, K), dtype=torch.uint8, device=DEV)
    ones = lambda n: torch.ones(n, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match="QuickGELU"):
        ops.linear(x8, w8, N, None, QGELU, w_scale=ones(N), x_scale=ones(M), y_scale=ones(M))
    with pytest.raises(nat.NativeError, match="unknown epilogue 3"):
        ops.linear(torch.zeros((M, K), dtype=torch.bfloat16, device=DEV), torch.zeros((N, K), dtype=torch.bfloat16, device=DEV), N, None, 3)


# ---------------------------------------------------------------------------------------------------------------
# 4: forwards
# ---------------------------------------------------------------------------------------------------------------
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
MODELS = ["vit_micro_quickgelu_patch16_64", "vit_micro_clip_quickgelu_patch16_64", "vit_micro_quickgelu_h344_patch16_64"]


def images_of(cfg, B, seed=2):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


_hosts = {}


def host_side(name, fix=FIX):
    """config, state dict and the base model's own stock forward (fp32, CPU, bf16-representable weights), once per model"""
    key = (name, tuple(sorted(fix.items())))
    if key not in _hosts:
        cfg = ts.CONFIGS[name]
        model = ts.create_model(cfg, round_bf16=True, **fix)

        def stock(x):
            with torch.no_grad():
                return model(torch.from_numpy(x)).numpy()
        _hosts[key] = (cfg, ts.state_dict_numpy(model), stock)
    return _hosts[key]


def build(name, sched, dt, fix=FIX):
    cfg, sd, stock = host_side(name, fix)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, **fix), sched).to(DEV).to(nm.TORCH[dt]).eval()
    assert w.check_supported()["mlp_act"] == "quick_gelu"
    return (cfg, sd, stock), w


def assert_fixture_can_tell(cfg, sd, imgs, sched):
    moved = na.activation_moves_logits(sd, imgs, sched, cfg)
    assert moved >= 5 * 1e-3, f"ignoring the activation moves the fp32 logits by only {moved:.4g} of their scale"


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[activations] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"


def device_selections(w):
    """{block: keep_idx} of the last forward, each checked to be the top-k rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, orc.select_tokens(t["scores"].float().cpu().numpy().astype(np.float64), idx.shape[1] - 1))
        forced[i] = idx
    return forced


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MODELS)
def test_empty_schedule_equals_the_stock_forward(name, dt):
    (cfg, sd, stock), w = build(name, {}, dt)
    imgs = images_of(cfg, 5)
    assert_fixture_can_tell(cfg, sd, imgs, {})
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    assert w._plan[2][4] is not None and w._plan[2][4].mlp_act == nat.MLP_QUICK_GELU      # through rajni_vit_forward_ext
    assert w.get_last_stats()["token_counts"] == [cfg.num_patches + 1] * cfg.depth
    want = stock(imgs)
    close(got, want, BAR[dt], f"{name} {dt} unpruned vs stock forward")
    if dt != "fp32":
        w.set_residual_dtype(nm.TORCH[dt])
        close(w(x).float().cpu().numpy(), want, 2e-2, f"{name} {dt} stream, unpruned")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", MODELS)
def test_pruned_forward_selection_conditional_and_free_running(name, dt):
    (cfg, sd, _), w = build(name, SCHED, dt)
    imgs = images_of(cfg, 6, seed=5)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED)
    want, counts, tr = na.vit_forward_restated(sd, imgs, SCHED, cfg, na.quick_gelu_torch)
    x = torch.from_numpy(imgs).to(DEV)
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR[dt], f"{name} {dt} pruned, selections injected")
    w.force_keep_idx(None).trace_scores(True)
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    want_free, _, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, na.quick_gelu_torch, forced_keep=device_selections(w))
    close(got, want_free, BAR[dt], f"{name} {dt} pruned, free-running")


# ---------------------------------------------------------------------------------------------------------------
# 5: the last block on the CLS rows
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_last_block_cls_rows_equal_all_rows_bit_for_bit(dt):
    """the default forward runs the last block's tail (FC1 + QuickGELU among it) on the B CLS rows: the logits are torch.equal
    to the all-rows form; the cls_only_last_block opt-in (another attention kernel) stays within the model's bar of both"""
    (cfg, _, _), w = build("vit_micro_quickgelu_patch16_64", SCHED, dt)
    x = torch.from_numpy(images_of(cfg, 5)).to(DEV)
    lib = nat.lib()
    rows = w(x).clone()
    plan, ext = w._plan[1], w._plan[2][4]
    assert lib.rajni_debug_last_block_cls_rows(C.byref(plan), C.byref(ext), None) == 1
    counts = w.get_last_stats()["token_counts"]
    try:
        lib.rajni_debug_set_last_block_all_rows(1)
        every = w(x).clone()
    finally:
        lib.rajni_debug_set_last_block_all_rows(0)
    assert w.get_last_stats()["token_counts"] == counts
    assert rows.dtype == every.dtype and torch.equal(rows, every), "logits differ between the CLS-row and the all-rows last block"
    opt = w.set_last_block_cls_only(True)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(opt, every.float().cpu().numpy(), BAR[dt], f"QuickGELU micro {dt}, cls_only_last_block vs every row")


# ---------------------------------------------------------------------------------------------------------------
# 6: "fp8" weights
# ---------------------------------------------------------------------------------------------------------------

def test_fp8_weights_on_a_quick_gelu_model():
    """set_weight_format("fp8") on the QuickGELU micro512 model: the restated QuickGELU graph on the dequantised weights with
    the device's own selections - the bar tests/test_gpu_fp8.py applies to the erf model (1e-2 of the logit scale, same argmax)"""
    cfg = ts.CONFIGS["vit_micro512_quickgelu_patch16_64"]
    model = ts.create_model(cfg, seed=4, std=0.06, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(torch.bfloat16).eval()
    with pytest.raises(NotImplementedError, match="QuickGELU"):
        w.set_weight_format("fp8_mfma")
    w.set_weight_format("fp8").trace_scores(True)
    imgs = images_of(cfg, 6, seed=9)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    forced = device_selections(w)
    sd = ts.state_dict_numpy(model)
    assert_fixture_can_tell(cfg, sd, imgs, SCHED)
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    want, counts, _ = na.vit_forward_restated(sd, imgs, SCHED, cfg, na.quick_gelu_torch, forced_keep=forced, dtype=torch.float32)
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, 1e-2, "micro512 QuickGELU, fp8 weights")
    assert (got.argmax(1) == want.argmax(1)).all()


# ---------------------------------------------------------------------------------------------------------------
# 7: ViT-B sized
# ---------------------------------------------------------------------------------------------------------------

def test_vit_base_sized_quick_gelu_model():
    """vit_base_patch16_clip_quickgelu_224 at batch 24 in bf16 (FC1 has 4728 rows: the persistent tilings inside a real
    forward): unpruned against the stock forward, pruned (README schedule) against the restated graph in fp32 with the
    device's own selections"""
    name = "vit_base_patch16_clip_quickgelu_224"
    sched = {3: {"keep_ratio": 0.88}, 4: {"keep_ratio": 0.88}, 7: {"keep_ratio": 0.80}, 8: {"keep_ratio": 0.72}}
    fix = dict(seed=3, std=0.04, bias_std=0.1)
    (cfg, sd, stock), w = build(name, {}, "bf16", fix)
    imgs = images_of(cfg, 24)
    assert_fixture_can_tell(cfg, sd, imgs[:2], {})
    x = torch.from_numpy(imgs).to(DEV)
    close(w(x).float().cpu().numpy(), stock(imgs), 1e-2, f"{name} unpruned vs stock forward")
    (_, _, _), wp = build(name, sched, "bf16", fix)
    wp.trace_scores(True)
    got = wp(x).float().cpu().numpy()
    want, counts, _ = na.vit_forward_restated(sd, imgs, sched, cfg, na.quick_gelu_torch, forced_keep=device_selections(wp),
                                              dtype=torch.float32)
    assert wp.get_last_stats()["token_counts"] == counts == [197, 197, 197, 197, 173, 152, 152, 152, 121, 87, 87, 87]
    close(got, want, 1e-2, f"{name} pruned, free-running")
