"""SwiGLU MLPs on the device: the gated epilogue RAJNI_EPI_BIAS_SWIGLU of rajni_linear - y [M, N] = silu(x Wg^T + bg) * (x Wv^T +
bv) from one [2N, K] weight - in every tiling and operand type, and whole forwards of gated models (rajni_vit_ext.mlp_act =
RAJNI_MLP_SWIGLU).  GPU box only (`-m gpu`).

What pins the FUNCTION is the epilogue sweep: biases only (zero operands, so gate and value are the fp32 biases exactly), the
gate over numerics_activations.sweep_grid crossed with five values, element by element against fp64.  The GEMM budgets hold
random operands to tests/numerics_swiglu.py::budget_swiglu (derived there); the several-tiles, bounds, placement and large-offset
cases pin the two-range tile loader; the forwards show the epilogue wired into the model, on fixtures the CPU has shown able to
tell a swapped or a missing gate (tests/test_swiglu_cpu.py), at the project's bars."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bigmem as bm
import numerics as nm
import numerics_activations as na
import numerics_prefix as npx
import numerics_swiglu as ns
import rajni_amd
from placement import Launch, assert_same_bits, ptr
from rajni_amd import ops, _native as nat, timm_shaped as ts

DEV = "cuda"
F32 = np.float32
SW = nat.EPI_BIAS_SWIGLU
TILING_IDS = {0: "auto", 1: "small128x128", 4: "wide256x256", 5: "mid256x128"}
NBLK_DEFAULT = 1600 * 1024


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if dt == "fp32" else t.to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


@pytest.fixture(autouse=True)
def hooks_reset():
    yield
    lib = nat.lib()
    lib.rajni_debug_set_persistent_workgroups(0)
    lib.rajni_debug_force_gemm_tiling(0)
    lib.rajni_debug_set_gemm_nblock_bytes(NBLK_DEFAULT)
    lib.rajni_debug_set_last_block_all_rows(0)


@pytest.fixture
def tiling(request):
    nat.lib().rajni_debug_force_gemm_tiling(request.param)
    return request.param


TILINGS = pytest.mark.parametrize("tiling", [0, 1, 4, 5], indirect=True, ids=list(TILING_IDS.values()))


def planned_tiling(M, N, K, dt="bf16", w8=False):
    """the tiling rajni_linear would run for a gated launch of that shape, from the dry run (current hooks apply)"""
    a = nat.LinearArgs()
    a.x = a.w = a.y = a.bias = 0x10000
    a.w_scale = 0x10000 if w8 else None
    a.lda = a.ldw = K
    a.ldc, a.M, a.N, a.K, a.epilogue, a.dtype = (N + 7) // 8 * 8, M, N, K, SW, nat.dtype_code(nm.TORCH[dt])
    plan = nat.LinearPlan()
    nat.check(nat.lib().rajni_debug_linear_plan(C.byref(a), 256, C.byref(plan)), "rajni_debug_linear_plan")
    return plan.tiling


# ---------------------------------------------------------------------------------------------------------------
# 1: the epilogue sweep through the bias path
# ---------------------------------------------------------------------------------------------------------------

def through_bias(g32, v, dt, tiling=0):
    """silu(0 W^T + g) * (0 W^T + v) for a vector of fp32 gate biases and one value: 261 rows x K 256 where a persistent tiling
    is forced (one full row tile and a ragged one: interior and guarded epilogue paths), else 5 rows x K 64"""
    n = len(g32)
    rows, K = (261, 256) if tiling in (4, 5) else (5, 64)
    if tiling in (4, 5):        # the forced persistent tiling is the one that runs (else the sweep would test 128 x 128 again)
        assert planned_tiling(rows, n, K, dt) == tiling
    x = torch.zeros((rows, K), dtype=nm.TORCH[dt], device=DEV)
    w = torch.zeros(((2 * n + 255) // 256 * 256, K), dtype=nm.TORCH[dt], device=DEV)
    bias = torch.from_numpy(np.concatenate([np.ascontiguousarray(g32, dtype=F32), np.full(n, v, dtype=F32)])).to(DEV)
    y = ops.linear(x, w, n, bias, SW)
    assert tuple(y.shape) == (rows, n)
    assert bool((y == y[:1]).logical_or(y.isnan() & y[:1].isnan()).all()), "rows of a launch with identical inputs differ"
    return y[0].cpu()


def sweep(dt, v, tiling):
    g = na.sweep_grid(dt)
    got = np.concatenate([host(through_bias(g[i:i + 70000], v, dt, tiling)) for i in range(0, len(g), 70000)])
    return g, got, ns.swiglu64(g.astype(np.float64), v)


@TILINGS
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_swiglu_epilogue_on_chosen_gates_and_values_16bit(dt, tiling):
    """|y - silu64(g) v| <= u_out |want| + A_GELU_16 |v| + floor; no NaN anywhere; finite wherever the fp64 value is inside the
    type's range; g = 0 gives exactly 0"""
    for v in ns.sweep_values(dt):
        g, got, want = sweep(dt, v, tiling)
        what = f"swiglu sweep {dt} tiling {tiling} value {v!r}"
        assert not np.isnan(got).any(), f"{what}: NaN at gate {g[np.isnan(got)][0]!r}"
        inside = np.abs(want) <= ns.TYPE_MAX[dt]
        assert np.isfinite(got[inside]).all(), f"{what}: non-finite at gate {g[inside][~np.isfinite(got[inside])][0]!r}"
        assert (got[g == 0] == 0).all() and (g == 0).sum() == 1
        budget = nm.UNIT[dt] * np.abs(want) + nm.A_GELU_16 * abs(v) + nm.FLOOR[dt]
        print(f"[swiglu] {what}: {int((~inside).sum())} true values beyond the type's range; at the gate's ends {got[-2]!r} {got[-1]!r}")
        nm.assert_within(got[inside], want[inside], budget[inside], what)


def test_swiglu_epilogue_on_chosen_gates_and_values_fp32():
    """fp32 models (expf and a true division): max(4 x the local error of torch's CPU fp32 silu(g) * v against fp64,
    2 u32 |want|) + floor"""
    for v in ns.sweep_values("fp32"):
        g, got, want = sweep("fp32", v, 0)
        what = f"swiglu sweep fp32 value {v!r}"
        env = ns.product32_envelope(g, v)
        assert not np.isnan(got).any(), f"{what}: NaN at gate {g[np.isnan(got)][0]!r}"
        inside = (np.abs(want) <= ns.TYPE_MAX["fp32"]) & np.isfinite(env)
        assert np.isfinite(got[np.abs(want) <= ns.TYPE_MAX["fp32"]]).all() and (got[g == 0] == 0).all()
        print(f"[swiglu] {what}: torch CPU reference max |err| {env[inside].max():.4g}")
        nm.assert_within(got[inside], want[inside], (np.maximum(4 * env, 2 * nm.U32 * np.abs(want)) + nm.FLOOR["fp32"])[inside], what)


# ---------------------------------------------------------------------------------------------------------------
# 2: GEMM budgets, random operands
# ---------------------------------------------------------------------------------------------------------------
_cache = {}


def gemm_reference(M, N, K, dt, w8=False):
    """ns.gemm_case, shared by the cases that differ in tiling only; w8: e4m3 weights with one fp32 scale per row (gate and value
    rows each their own), want and S on the dequantised weight"""
    key = (M, N, K, dt, w8)
    if key not in _cache:
        if len(_cache) >= 3:
            _cache.pop(next(iter(_cache)))
        c = ns.gemm_case(M, N, K, dt)
        if w8:
            q, s = ops.pack_weight_fp8(torch.from_numpy(c["w"]), nm.TORCH[dt])
            wd = (q[:2 * N].view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64) * s.to(torch.float64)[:, None]).numpy()
            c.update(ns.halves(c["x"], wd, c["b"], N), q=q, s=s)
        _cache[key] = c
    return _cache[key]


def check_budget(y, c, dt, what):
    A = nm.A_GELU_16 if dt != "fp32" else ns.a_silu_fp32(c["g"])
    ns.assert_within_range(host(y), ns.swiglu64(c["g"], c["v"]), ns.budget_swiglu(c["g"], c["v"], c["Sg"], c["Sv"], c["gacc"], dt, A),
                           dt, what)


# (394, 1160, 768): a ragged last column tile in every tiling - the gate tile runs past N into the value rows - and a ragged row
# tile; it reaches the persistent tilings when they are forced.  The others run 128 x 128 whatever is asked (M < 256 or K < 192)
SHAPES_16 = [(7, 504, 768, 0), (130, 1536, 768, 0), (513, 136, 128, 0)] + [(394, 1160, 768, t) for t in (0, 1, 4, 5)]
SHAPE_IDS = [f"{m}x{n}x{k}-{TILING_IDS[t]}" for m, n, k, t in SHAPES_16]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K,tiling", SHAPES_16, indirect=["tiling"], ids=SHAPE_IDS)
def test_swiglu_gemm_budgets_16bit(M, N, K, tiling, dt):
    c = gemm_reference(M, N, K, dt)
    if tiling in (4, 5):
        assert planned_tiling(M, N, K, dt) == tiling
    y = ops.linear(dev(c["x"], dt), ops.pack_weight(dev(c["w"], dt), nm.TORCH[dt]), N, dev(c["b"], "fp32"), SW)
    assert tuple(y.shape) == (M, N) and y.dtype == nm.TORCH[dt]
    check_budget(y, c, dt, f"gemm SWIGLU {dt} {M}x{N}x{K} tiling {tiling}")


@pytest.mark.parametrize("M,N,K,tiling", SHAPES_16, indirect=["tiling"], ids=SHAPE_IDS)
def test_swiglu_gemm_budgets_fp8_weights(M, N, K, tiling):
    c = gemm_reference(M, N, K, "bf16", w8=True)
    y = ops.linear(dev(c["x"], "bf16"), c["q"].to(DEV), N, dev(c["b"], "fp32"), SW, w_scale=c["s"].to(DEV))
    assert tuple(y.shape) == (M, N)
    check_budget(y, c, "bf16", f"gemm SWIGLU bf16 x e4m3 weights {M}x{N}x{K} tiling {tiling}")


@pytest.mark.parametrize("M,N,K", [(130, 520, 256), (394, 1160, 768)])
def test_swiglu_gemm_budgets_fp32(M, N, K):
    c = gemm_reference(M, N, K, "fp32")
    y = ops.linear(dev(c["x"], "fp32"), ops.pack_weight(dev(c["w"], "fp32"), torch.float32), N, dev(c["b"], "fp32"), SW)
    assert tuple(y.shape) == (M, N) and y.dtype == torch.float32
    check_budget(y, c, "fp32", f"gemm SWIGLU fp32 {M}x{N}x{K}")


def test_swiglu_on_the_fp8_matrix_pipe_is_refused():
    M, N, K = 256, 512, 512
    x8 = torch.zeros((M, K), dtype=torch.uint8, device=DEV)
    w8 = torch.zeros((2 * N, K), dtype=torch.uint8, device=DEV)
    ones = lambda n: torch.ones(n, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        ops.linear(x8, w8, N, None, SW, w_scale=ones(2 * N), x_scale=ones(M), y_scale=ones(M))


# ---------------------------------------------------------------------------------------------------------------
# 3: several tiles per workgroup - the per-tile pointer advance of the two-range loader
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiling", [4, 5], indirect=True, ids=["wide256x256", "mid256x128"])
@pytest.mark.parametrize("M,N,K", [(394, 1160, 768), (1030, 648, 768)])
def test_swiglu_several_tiles_per_workgroup(M, N, K, tiling):
    """persistent grids capped at 1, 2 and 3 workgroups, and N blocks of one column tile under a cap: bit-equal to the uncapped
    launch, which meets the budget"""
    lib = nat.lib()
    c = gemm_reference(M, N, K, "bf16")
    assert planned_tiling(M, N, K) == tiling
    xd, wd, bd = dev(c["x"], "bf16"), ops.pack_weight(dev(c["w"], "bf16"), torch.bfloat16), dev(c["b"], "fp32")

    def run():
        out = torch.full((M, (N + 7) // 8 * 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.linear(xd, wd, N, bd, SW, out=out)
        return out[:, :N]
    base = run()
    check_budget(base, c, "bf16", f"gemm SWIGLU bf16 {M}x{N}x{K} tiling {tiling} uncapped")
    for cap, nblk in ((1, NBLK_DEFAULT), (2, NBLK_DEFAULT), (3, NBLK_DEFAULT), (2, -1)):
        lib.rajni_debug_set_persistent_workgroups(cap)
        lib.rajni_debug_set_gemm_nblock_bytes(nblk)
        got = run()
        assert not bool(got.isnan().any()), f"cap {cap} nblock {nblk}: NaN left (a tile was skipped)"
        assert torch.equal(got.view(torch.int16), base.view(torch.int16)), f"cap {cap} nblock {nblk} differs from the uncapped launch"


# ---------------------------------------------------------------------------------------------------------------
# 4, 5: bounds, isolation and placement - tests/placement.py: every buffer guarded and poisoned around; the shifted launch at the
# ABI's minimum alignment with odd lda / ldw / ldc (ldc = N + 24), bit-equal to the launch on 256-byte boundaries
# ---------------------------------------------------------------------------------------------------------------

def placement_case(kind, M, N, K, tiling):
    dt = "fp32" if kind == "fp32" else "bf16" if kind == "fp8w" else kind
    tdt = nm.TORCH[dt]
    w8 = kind == "fp8w"
    c = gemm_reference(M, N, K, dt, w8=w8)
    xd, bd = dev(c["x"], dt), dev(c["b"], "fp32")
    wd = c["q"][:2 * N].to(DEV) if w8 else dev(c["w"], dt)
    npad = (2 * N + 255) // 256 * 256

    def case(shifted):
        L = Launch("rajni_linear", shifted, elem_bytes=4 if dt == "fp32" else 2)
        xg = L.inp("x", xd, ld_extra=8)
        wg = L._make("w", (npad, K), wd.dtype, 16 if w8 else 8, False)     # rows 2N.. stay poisoned: never read into a result
        wg.t[:2 * N].copy_(wd)
        a = nat.LinearArgs()
        a.x, a.lda, a.w, a.ldw = xg.ptr(), xg.ld, wg.ptr(), wg.ld
        a.bias = L.inp("bias", bd).ptr()
        a.w_scale = ptr(L.inp("w_scale", c["s"].to(DEV) if w8 else None))
        a.M, a.N, a.K, a.epilogue, a.dtype = M, N, K, SW, nat.dtype_code(tdt)
        yg = L.out("y", (M, N), tdt, ld_extra=24)
        a.y, a.ldc = yg.ptr(), yg.ld
        plan = nat.LinearPlan()
        nat.check(nat.lib().rajni_debug_linear_plan(C.byref(a), 256, C.byref(plan)), "rajni_debug_linear_plan")
        assert plan.tiling == tiling
        nat.check(nat.lib().rajni_linear(C.byref(a), nat.stream_ptr()), "rajni_linear")
        torch.cuda.synchronize()
        if shifted:
            assert (a.lda, a.ldw, a.ldc) == (K + 8, K + (16 if w8 else 8), N + 24) and a.x % 256 == 16 and a.bias % 256 == 16
        return L, yg

    what = f"linear SWIGLU {kind} {M}x{N}x{K} tiling {tiling}"
    (la, ya), (lb, yb) = case(False), case(True)
    la.check(what)          # nothing outside [M, N] written (pad columns, rows behind), every element of [M, N] written,
    lb.check(what)          # and no poison (W rows beyond 2N, the rows around x) reached a result
    assert_same_bits(ya, yb, what)
    check_budget(ya.t, c, dt, what)


@pytest.mark.parametrize("tiling", [1, 4, 5], indirect=True, ids=["small128x128", "wide256x256", "mid256x128"])
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8w"])
def test_swiglu_bounds_isolation_and_placement_16bit(kind, tiling):
    """300 x 328 x 320: two row tiles (the last from row M - 256), a ragged last column tile for 64 and 128 hidden columns"""
    placement_case(kind, 300, 328, 320, tiling)


def test_swiglu_bounds_isolation_and_placement_fp32():
    placement_case("fp32", 300, 328, 320, nat.TILING_F32)


# ---------------------------------------------------------------------------------------------------------------
# 6: large offsets - an output of more than 2^31 elements (m * ldc in 64 bits), tests/test_gpu_large_offsets.py's method
# ---------------------------------------------------------------------------------------------------------------

def test_swiglu_output_past_2_31_elements():
    """bf16, M = 1100 (the persistent 256 x 128 tiling by shape), N = 200, K = 256; x and y at a row stride of 2^21 + 64
    elements, so row 1024 starts 2^31 + 65536 elements from the base: bit-equal to the dense launch, which meets the budget"""
    M, N, K, LD = 1100, 200, 256, (1 << 21) + 64
    assert bm.first_row_past(LD, bm.T31) == 1024 < M
    c = gemm_reference(M, N, K, "bf16")
    xd, wd, bd = dev(c["x"], "bf16"), ops.pack_weight(dev(c["w"], "bf16"), torch.bfloat16), dev(c["b"], "fp32")
    big = bm.Big(DEV)
    try:
        got = {}
        for layout in ("large", "dense"):
            if layout == "large":
                xv, yv = big.rows(M, K, LD, torch.bfloat16), big.rows(M, N, LD, torch.bfloat16)
                xv.copy_(xd)
                bm.assert_crosses_all((M - 1) * LD + N, 2, "swiglu output")
            else:
                xv, yv = xd, torch.empty((M, N + 0), dtype=torch.bfloat16, device=DEV)
            bm.bits(yv).fill_(-1)
            a = nat.LinearArgs()
            a.x, a.lda, a.w, a.ldw, a.bias = xv.data_ptr(), xv.stride(0), wd.data_ptr(), wd.shape[1], bd.data_ptr()
            a.y, a.ldc, a.M, a.N, a.K, a.epilogue, a.dtype = yv.data_ptr(), yv.stride(0), M, N, K, SW, nat.RAJNI_BF16
            nat.check(nat.lib().rajni_linear(C.byref(a), nat.stream_ptr()), "rajni_linear")
            torch.cuda.synchronize()
            got[layout] = yv.contiguous()
        bm.assert_bit_equal(got["large"], got["dense"], "swiglu bf16 1100x200x256: large strides vs dense")
        check_budget(got["dense"], c, "bf16", "gemm SWIGLU bf16 1100x200x256")
    finally:
        big.close()


# ---------------------------------------------------------------------------------------------------------------
# 7: forwards
# ---------------------------------------------------------------------------------------------------------------
BAR = ns.BAR


def build(name, sched, dt):
    cfg = ts.config_of(name)
    fix = ns.fix_of(name)
    model = ts.create_model(cfg, round_bf16=True, **fix)
    sd = ts.state_dict_numpy(model)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, round_bf16=True, **fix), sched).to(DEV).to(nm.TORCH[dt]).eval()
    d = w.check_supported()
    assert d["mlp_act"] == "swiglu" and d["ext"] is True
    return cfg, sd, model, w


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[swiglu] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"


def device_selections(w, P):
    """{block: keep_idx} of the last forward, each checked to be the top-k rule on the device's own traced scores"""
    forced = {}
    for i, t in w.get_last_trace().items():
        idx = t["keep_idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, npx.select_tokens(t["scores"].float().cpu().numpy().astype(np.float64), idx.shape[1] - P, P))
        forced[i] = idx
    return forced


def injected(name, dt, B=3, iseed=5, prepare=None, bar=None):
    """the pruned forward with the fp64 graph's selections injected, against that graph"""
    assert (True, B, iseed) in ns.FORWARD_CASES[name]
    cfg, sd, _, w = build(name, ns.SCHED, dt)
    imgs = ns.images_of(cfg, B, iseed)
    want, counts, tr = ns.vit_forward_restated(sd, imgs, ns.SCHED, cfg)
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    if prepare:
        prepare(w)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    assert w._plan[2][4] is not None and w._plan[2][4].mlp_act == nat.MLP_SWIGLU
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, bar or BAR[dt], f"{name} {dt} pruned, selections injected")
    return cfg, sd, w, imgs, want, counts


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_micro_forward(dt):
    injected("vit_micro_swiglu_patch16_64", dt)


@pytest.mark.parametrize("name", ["vit_micro_swiglu_split_patch16_64", "vit_micro_swiglu_h344_patch16_64",
                                  "vit_micro_reg4_swiglu_patch14_56"])
def test_split_odd_width_and_register_forwards(name):
    injected(name, "bf16")


def test_free_running_forward_and_the_stock_module():
    """unpruned against the base model's own forward; pruned and free-running against the fp64 graph on the device's own
    selections (the agreement rule of tests/test_gpu_activations.py)"""
    name = "vit_micro_swiglu_patch16_64"
    cfg, sd, model, w = build(name, {}, "bf16")
    imgs = ns.images_of(cfg, 3, 2)
    with torch.no_grad():
        stock = model(torch.from_numpy(imgs)).numpy()
    close(w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy(), stock, BAR["bf16"], f"{name} bf16 unpruned vs stock forward")
    cfg, sd, _, w = build(name, ns.SCHED, "bf16")
    imgs = ns.images_of(cfg, 3, 5)
    w.trace_scores(True)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    want, counts, _ = ns.vit_forward_restated(sd, imgs, ns.SCHED, cfg, forced_keep=device_selections(w, 1))
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, BAR["bf16"], f"{name} bf16 pruned, free-running")


def test_micro512_forward_runs_fc1_on_the_wide_tiling():
    """batch 64: FC1 has 1088 rows and 2048 rows of W - the wide tiling by the shape rule - in bf16 and with "fp8" weights"""
    name = "vit_micro512_swiglu_patch16_64"
    assert planned_tiling(64 * 17, 1024, 512) == nat.TILING_WIDE
    cfg, sd, w, imgs, want, counts = injected(name, "bf16", B=64)
    # "fp8" weights: the same graph on the dequantised weights, the bar of tests/test_gpu_fp8.py (1e-2 of the logit scale)
    assert planned_tiling(64 * 17, 1024, 512, w8=True) == nat.TILING_WIDE
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        w.set_weight_format("fp8_mfma")
    w.set_weight_format("fp8")
    x = torch.from_numpy(imgs).to(DEV)
    got = w(x).float().cpu().numpy()
    sd8 = dict(sd)
    sd8.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    forced = {i: f.cpu().numpy() for i, f in w._forced.items()}
    want8, counts8, _ = ns.vit_forward_restated(sd8, imgs, ns.SCHED, cfg, forced_keep=forced)
    assert w.get_last_stats()["token_counts"] == counts8 == counts
    close(got, want8, 1e-2, f"{name} fp8 weights, selections injected")


def test_residual_stream_in_bf16():
    injected("vit_micro_swiglu_patch16_64", "bf16", prepare=lambda w: w.set_residual_dtype(torch.bfloat16), bar=2e-2)


def test_last_block_cls_rows_and_the_cls_only_opt_in():
    """the default forward runs the last block's tail (the gated FC1 among it) on the B CLS rows: byte-equal to the all-rows form;
    set_last_block_cls_only(True) (another attention kernel) meets the model's bar"""
    name = "vit_micro_swiglu_patch16_64"
    cfg, sd, w, imgs, want, counts = injected(name, "bf16")
    x = torch.from_numpy(imgs).to(DEV)
    lib = nat.lib()
    rows = w(x).clone()
    assert lib.rajni_debug_last_block_cls_rows(C.byref(w._plan[1]), C.byref(w._plan[2][4]), None) == 1
    lib.rajni_debug_set_last_block_all_rows(1)
    every = w(x).clone()
    lib.rajni_debug_set_last_block_all_rows(0)
    assert rows.dtype == every.dtype and torch.equal(rows.view(torch.int16), every.view(torch.int16)), \
        "logits differ between the CLS-row and the all-rows last block"
    opt = w.set_last_block_cls_only(True)(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(opt, want, BAR["bf16"], f"{name} bf16, cls_only_last_block")
