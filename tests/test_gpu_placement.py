"""Every kernel at the minimum alignment the ABI states and at row strides off the 128-byte lines.  GPU box only (`-m gpu`).

Each case makes two launches of the same call under the same forced tiling or mode (tests/placement.py::Launch):
  (a) aligned   every buffer dense on a 256-byte boundary - where every other GPU test of the suite puts it;
  (b) shifted   every pointer at a 256-byte boundary plus its minimum of include/rajni_hip.h ("placement": +16 for data and
                fp32 per-column vectors, +4 for row scales and index arrays, one element for score arrays; the score scratch
                and the forward's workspace stay on 256), every row stride the least legal non-dense value whose residue puts
                rows off the 128-byte lines (lda, ldw, ldc = dense + 8 elements, ldr = dense + 24, e4m3 bytes + 16,
                x_row_stride = C + 8).
and asserts that (b) has the bits of (a), that every guard zone, row gap and tail of (b) (and of (a)) is intact with every
output element written, and that (a) meets the float64 reference under the budget tests/numerics.py (numerics_variants.py)
holds that op to.  No kernel or planner branches on an address or a stride's residue, so the equality needs no tolerance.

Nothing here launches below the contract: the refusals are tests/test_placement_cpu.py's, where nothing is launched at all.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_prefix as npx
import numerics_variants as nv
import placement as pl
import rajni_amd
from oracle import rajni_oracle as orc
from placement import Launch, assert_same_bits, ptr
from rajni_amd import _native as nat, ops, timm_shaped as ts

DEV = "cuda"
EPS = 1e-6
F32 = np.float32
BIAS, GELU, RESID = nat.EPI_BIAS, nat.EPI_BIAS_GELU, nat.EPI_BIAS_RESID
_cache = {}


def lib():
    return nat.lib()


def sync(rc, what):
    nat.check(rc, what)
    torch.cuda.synchronize()


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if dt == "fp32" else t.to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def ceil(a, b):
    return (a + b - 1) // b * b


def cached(key, make):
    """float64 references are computed once and shared by the cases that differ in tiling, mode or placement only"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def both(case, what, outputs):
    """run `case(shifted)` -> (Launch, {name: Guarded output}) at both placements; guards, then bit equality; returns (a)'s outputs"""
    la, oa = case(False)
    lb, ob = case(True)
    la.check(what)
    lb.check(what)
    for name in outputs:
        assert_same_bits(oa[name], ob[name], f"{what}: {name}")
    return oa


# =================================================================================================================
# rajni_linear
# =================================================================================================================
TILING_NAMES = {1: "small128x128", 4: "wide256x256", 5: "mid256x128"}


@pytest.fixture(params=[1, 4, 5], ids=[TILING_NAMES[t] for t in (1, 4, 5)])
def tiling(request):
    lib().rajni_debug_force_gemm_tiling(request.param)
    yield request.param
    lib().rajni_debug_force_gemm_tiling(0)


@pytest.fixture(params=[1, 2], ids=["f8_256x128", "f8_256x256"])
def f8_tiling(request):
    lib().rajni_debug_force_f8_tiling(request.param)
    yield request.param
    lib().rajni_debug_force_f8_tiling(0)


R_NP, R_NSRC = 75, 90       # gathered residual rows: 4 images of 75 kept rows out of 90


def lin_reference(kind, M, N, K):
    """operands of nm.gemm_operands in the kind's type ("fp8w": bf16 x with e4m3 weights), want / S / g of nm.gemm_pre"""
    def make():
        dt = {"bf16": "bf16", "fp16": "fp16", "fp8w": "bf16", "fp32": "fp32"}[kind]
        x, w, b = nm.gemm_operands(M, N, K, dt)
        q = s = None
        if kind == "fp8w":
            q, s = ops.pack_weight_fp8(torch.from_numpy(w), torch.bfloat16)
            q = q[:N]
            w = (q.view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64) * s.to(torch.float64)[:, None]).numpy()
        return dict(dt=dt, x=x, w=w, b=b, q=q, s=s, pre=nm.gemm_pre(x, w, b))
    return cached(("lin", kind, M, N, K), make)


def resid_reference(M, N, dt, stream, gathered):
    def make():
        B = M // R_NP
        r, gam, idx = nm.resid_operands(B, R_NSRC if gathered else R_NP, R_NP, N, dt, stream)
        used = orc.gather_rows(r, idx.astype(np.int64)) if gathered else r
        return r, gam, idx, used.reshape(M, N).astype(np.float64)
    return cached(("resid", M, N, dt, stream, gathered), make)


def assert_tiling(a, want):
    """the dry run of the very arguments: the forced tiling is the one that runs (else the case would test another kernel)"""
    plan = nat.LinearPlan()
    nat.check(lib().rajni_debug_linear_plan(C.byref(a), 256, C.byref(plan)), "rajni_debug_linear_plan")
    assert plan.tiling == want, f"forced tiling {want} but the plan says {plan.tiling}"


def linear16_case(kind, M, N, K, epi, stream_f32, mode, tiling):
    ref = lin_reference(kind, M, N, K)
    dt = ref["dt"]
    tdt = nm.TORCH[dt]
    pre, S, g = ref["pre"]
    stream = "fp32" if (stream_f32 and dt != "fp32") else dt
    ydt = nm.TORCH[stream] if epi == RESID else tdt
    if epi == RESID:
        r, gam, idx, r_used = resid_reference(M, N, dt, stream, mode == "gathered")
    w8 = kind == "fp8w"
    xd, bd = dev(ref["x"], dt), dev(ref["b"], "fp32")
    wd = ref["q"].to(DEV) if w8 else dev(ref["w"], dt)
    npad = ceil(N, 256)

    def case(shifted):
        L = Launch("rajni_linear", shifted)
        xg = L.inp("x", xd, ld_extra=8)
        wg = L._make("w", (npad, K), wd.dtype, 16 if w8 else 8, False)     # rows N.. stay poisoned: never read into a result
        wg.t[:N].copy_(wd)
        a = nat.LinearArgs()
        a.x, a.lda, a.w, a.ldw = xg.ptr(), xg.ld, wg.ptr(), wg.ld
        a.bias = L.inp("bias", bd).ptr()
        a.w_scale = ptr(L.inp("w_scale", ref["s"].to(DEV) if w8 else None))
        a.M, a.N, a.K, a.epilogue, a.dtype = M, N, K, epi, nat.dtype_code(tdt)
        if epi == RESID:
            a.gamma = L.inp("gamma", dev(gam, "fp32")).ptr()
            a.stream_f32 = int(stream == "fp32" and dt != "fp32")
            if mode == "inplace":                  # y IS the residual tensor: one stride for both
                yg = L.inp("y = resid", dev(r.reshape(M, N), stream), ld_extra=8, key="y")
                L.mark_output(yg)
                a.resid, a.ldr = yg.ptr(), yg.ld
            else:
                rows = dev(r.reshape(-1, N), stream)
                rg = L.inp("resid", rows, ld_extra=24, after_rows=(256 // R_NP + 2) * R_NSRC + 256)
                a.resid, a.ldr = rg.ptr(), rg.ld
                if mode == "gathered":
                    a.r_idx = L.idx("r_idx", torch.from_numpy(idx.reshape(-1)).to(DEV), fill=R_NSRC - 1).ptr()
                    a.r_np, a.r_nsrc = R_NP, R_NSRC
                yg = L.out("y", (M, N), ydt, ld_extra=8)
        else:
            yg = L.out("y", (M, N), ydt, ld_extra=8)
        a.y, a.ldc = yg.ptr(), yg.ld
        if tiling:
            assert_tiling(a, tiling)
        sync(lib().rajni_linear(C.byref(a), nat.stream_ptr()), "rajni_linear")
        if shifted:
            assert (a.lda, a.ldw, a.ldc) == (K + 8, K + (16 if w8 else 8), N + 8) and a.x % 256 == 16 and a.bias % 256 == 16
        return L, {"y": yg}

    what = f"linear {kind} {M}x{N}x{K} epi {epi} stream {stream} {mode} tiling {tiling}"
    y = host(both(case, what, ["y"])["y"].t)
    if epi == BIAS:
        nm.assert_within(y, pre, nm.budget_bias(pre, S, g, dt), what)
    elif epi == GELU:
        a_gelu = nm.a_gelu_fp32(pre) if dt == "fp32" else nm.A_GELU_16
        nm.assert_within(y, orc.gelu(pre), nm.budget_gelu(pre, S, g, dt, a_gelu), what)
    else:
        want, bud = nm.budget_resid(pre, S, g, r_used, gam.astype(np.float64), stream)
        nm.assert_within(y, want, bud, what)


EPILOGUES = ([(BIAS, 0, None), (GELU, 0, None)] +
             [(RESID, sf, mode) for sf in (0, 1) for mode in ("plain", "gathered", "inplace")])
EPI_IDS = [f"{('bias', 'gelu', 'resid')[e]}{'-f32stream' if sf else ''}{'-' + m if m else ''}" for e, sf, m in EPILOGUES]


@pytest.mark.parametrize("epi,stream_f32,mode", EPILOGUES, ids=EPI_IDS)
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8w"])
def test_linear_16bit(kind, epi, stream_f32, mode, tiling):
    """300 x 328 x 320: two row tiles (the last from row M - 256), a ragged last column tile for 128 and 256, five K steps;
    K <= N, so RESID runs the attention-projection twin"""
    linear16_case(kind, 300, 328, 320, epi, stream_f32, mode, tiling)


@pytest.mark.parametrize("stream_f32", [0, 1], ids=["stream16", "f32stream"])
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8w"])
def test_linear_16bit_resid_k_above_n(kind, stream_f32, tiling):
    """300 x 192 x 320: K > N, the other RESID kernel twin (the fc2 form)"""
    linear16_case(kind, 300, 192, 320, RESID, stream_f32, "gathered", tiling)


@pytest.mark.parametrize("epi,mode", [(BIAS, None), (GELU, None), (RESID, "plain"), (RESID, "gathered"), (RESID, "inplace")],
                         ids=["bias", "gelu", "resid", "resid-gathered", "resid-inplace"])
def test_linear_fp32(epi, mode):
    linear16_case("fp32", 150, 136, 128, epi, 0, mode, 0)


def f8_reference(M, N, K):
    """tests/test_gpu_numerics.py::f8_reference: nm.gemm_operands quantised row by row to e4m3, want and S dequantised"""
    def make():
        x, w, b = nm.gemm_operands(M, N, K, "bf16")
        (xq, xs), (wq, ws) = ops.quantize_rows_fp8(torch.from_numpy(x)), ops.quantize_rows_fp8(torch.from_numpy(w))
        f64 = lambda q, sc: q.to(torch.float32).to(torch.float64).numpy() * sc.to(torch.float64).numpy()[:, None]
        return xq.view(torch.uint8), xs, wq.view(torch.uint8), ws, b, nm.gemm_pre(f64(xq, xs), f64(wq, ws), b)
    return cached(("f8", M, N, K), make)


@pytest.mark.parametrize("epi,stream_f32", [(BIAS, 0), (GELU, 0), (RESID, 0), (RESID, 1)],
                         ids=["bias", "gelu_e4m3", "resid-bf16stream", "resid-f32stream"])
def test_linear_fp8_x_fp8(epi, stream_f32, f8_tiling):
    """e4m3 x and W (strides in bytes, + 16), per-row x_scale / y_scale at + 4; GELU writes e4m3 rows (ldc in bytes, + 16)"""
    M, N, K = 300, 328, 512
    xq, xs, wq, ws, b, (pre, S, g) = f8_reference(M, N, K)
    stream = "fp32" if stream_f32 else "bf16"
    if epi == RESID:
        r, gam, idx, r_used = resid_reference(M, N, "bf16", stream, True)
    if epi == GELU:
        h = orc.gelu(pre)
        ys = (np.abs(h).max(axis=1) * 1.5 / 448.0).astype(F32)

    def case(shifted):
        L = Launch("rajni_linear", shifted)
        xg = L.inp("x", xq.to(DEV), ld_extra=16)
        wg = L._make("w", (ceil(N, 256), K), torch.uint8, 16, False)
        wg.t[:N].copy_(wq.to(DEV))
        a = nat.LinearArgs()
        a.x, a.lda, a.w, a.ldw = xg.ptr(), xg.ld, wg.ptr(), wg.ld
        a.bias = L.inp("bias", dev(b, "fp32")).ptr()
        a.w_scale, a.x_scale = L.inp("w_scale", ws.to(DEV)).ptr(), L.inp("x_scale", xs.to(DEV)).ptr()
        a.M, a.N, a.K, a.epilogue, a.dtype, a.stream_f32 = M, N, K, epi, nat.RAJNI_BF16, stream_f32
        if epi == GELU:
            a.y_scale = L.inp("y_scale", torch.from_numpy(ys).to(DEV)).ptr()
            yg = L._make("y", (M, N), torch.uint8, 0, True, stride=(ceil(N, 16) + 16) if shifted else ceil(N, 16))
        else:
            yg = L.out("y", (M, N), nm.TORCH[stream] if epi == RESID else torch.bfloat16, ld_extra=8)
        if epi == RESID:
            a.gamma = L.inp("gamma", dev(gam, "fp32")).ptr()
            rg = L.inp("resid", dev(r.reshape(-1, N), stream), ld_extra=24, after_rows=(256 // R_NP + 2) * R_NSRC + 256)
            a.resid, a.ldr = rg.ptr(), rg.ld
            a.r_idx = L.idx("r_idx", torch.from_numpy(idx.reshape(-1)).to(DEV), fill=R_NSRC - 1).ptr()
            a.r_np, a.r_nsrc = R_NP, R_NSRC
        a.y, a.ldc = yg.ptr(), yg.ld
        plan = nat.LinearPlan()
        nat.check(lib().rajni_debug_linear_plan(C.byref(a), 256, C.byref(plan)), "rajni_debug_linear_plan")
        if f8_tiling == 1 or epi != RESID:      # (RESID has no 256 x 256 fp8 tiling: the forced value falls back to the stream kernel)
            assert plan.tiling == {1: nat.TILING_F8_STREAM, 2: nat.TILING_F8_WIDE}[f8_tiling], plan.tiling
        sync(lib().rajni_linear(C.byref(a), nat.stream_ptr()), "rajni_linear")
        if shifted:
            assert a.x_scale % 256 == 4 and a.x % 256 == 16 and (a.lda, a.ldw) == (K + 16, K + 16)
        return L, {"y": yg}

    what = f"linear fp8 x fp8 {M}x{N}x{K} epi {epi} stream {stream} tiling {f8_tiling}"
    yt = both(case, what, ["y"])["y"].t
    if epi == GELU:     # the e4m3 rounding bound of tests/test_gpu_guarded.py::_f8f8_case
        deq = yt.view(torch.float8_e4m3fn).to(torch.float32).cpu().numpy().astype(np.float64) * ys.astype(np.float64)[:, None]
        bound = np.maximum(np.abs(h) * 2.0 ** -4, ys.astype(np.float64)[:, None] * 2.0 ** -10) * 1.01 + 2e-4 * np.abs(h).max()
        nm.assert_within(deq, h, bound, what)
    elif epi == BIAS:
        nm.assert_within(host(yt), pre, nm.budget_bias(pre, S, g, "bf16"), what)
    else:
        want, bud = nm.budget_resid(pre, S, g, r_used, gam.astype(np.float64), stream)
        nm.assert_within(host(yt), want, bud, what)


# =================================================================================================================
# LayerNorm
# =================================================================================================================
LN_SHAPES = [(77, 192), (77, 1280), (4109, 192)]      # one and three chunks per lane; the two-rows-per-wave kernel


def ln_reference(rows, C, in_dt, out_dt):
    def make():
        x, names, w, b = nm.layernorm_rows(rows, C, in_dt)
        return (x, w, b) + nm.layernorm_budget(x, w, b, EPS, out_dt)
    return cached(("ln", rows, C, in_dt, out_dt), make)


# (the CLS-row stride at 77 rows only: 4109 x 5 rows would add nothing)
LN_CASES = [(r, c, cls) for r, c in LN_SHAPES for cls in (False, True) if not (cls and r > 100)]
LN_IDS = [f"{r}x{c}{'-cls_rows_stride_5C' if cls else ''}" for r, c, cls in LN_CASES]


@pytest.mark.parametrize("out_dt,x_f32", [("bf16", 0), ("bf16", 1), ("fp16", 0), ("fp16", 1), ("fp32", 0)])
@pytest.mark.parametrize("rows,C,cls_rows", LN_CASES, ids=LN_IDS)
def test_layernorm(rows, C, out_dt, x_f32, cls_rows):
    """x rows C + 8 apart from a base at + 16, or the CLS rows of [rows, 5, C] (stride 5 C, the final norm's launch) from + 16"""
    in_dt = "fp32" if x_f32 else out_dt
    x, w, b, want, bud = ln_reference(rows, C, in_dt, out_dt)
    xd = dev(x, in_dt)

    def case(shifted):
        L = Launch("rajni_layernorm", shifted)
        if cls_rows:
            xg = L._make("x", (rows, 5, C), xd.dtype, 0, False)
            xg.t[:, 0].copy_(xd)                                  # tokens 1.. of every image stay poisoned
            stride = 5 * C
        else:
            xg = L.inp("x", xd, ld_extra=8)
            stride = xg.ld
        wg, bg = L.inp("w", dev(w, "fp32")), L.inp("b", dev(b, "fp32"))
        yg = L.out("y", (rows, C), nm.TORCH[out_dt])
        sync(lib().rajni_layernorm(xg.ptr(), stride, wg.ptr(), bg.ptr(), yg.ptr(), rows, C, EPS, nat.dtype_code(nm.TORCH[out_dt]),
                                   x_f32, nat.stream_ptr()), "rajni_layernorm")
        return L, {"y": yg}

    what = f"layernorm {rows}x{C} {in_dt}->{out_dt} cls_rows={cls_rows}"
    nm.assert_within(host(both(case, what, ["y"])["y"].t), want, bud, what)


@pytest.mark.parametrize("x_f32", [0, 1], ids=["in_bf16", "in_f32stream"])
@pytest.mark.parametrize("rows,C,cls_rows", LN_CASES, ids=LN_IDS)
def test_layernorm_fp8(rows, C, x_f32, cls_rows):
    """e4m3 rows, y_scale and hid_scale (both at + 4) bit for bit; the scales held to tests/test_gpu_numerics.py's rule"""
    in_dt = "fp32" if x_f32 else "bf16"
    x, w, b, want, bud = ln_reference(rows, C, in_dt, "fp32")
    xd = dev(x, in_dt)
    wn, bm = 0.61, 0.07

    def case(shifted):
        L = Launch("rajni_layernorm_fp8", shifted)
        if cls_rows:
            xg = L._make("x", (rows, 5, C), xd.dtype, 0, False)
            xg.t[:, 0].copy_(xd)
            stride = 5 * C
        else:
            xg = L.inp("x", xd, ld_extra=8)
            stride = xg.ld
        wg, bg = L.inp("w", dev(w, "fp32")), L.inp("b", dev(b, "fp32"))
        qg, sg, hg = L.out("y_q", (rows, C), torch.uint8), L.out("y_scale", (rows,), torch.float32), L.out("hid_scale", (rows,), torch.float32)
        sync(lib().rajni_layernorm_fp8(xg.ptr(), stride, wg.ptr(), bg.ptr(), qg.ptr(), sg.ptr(), hg.ptr(), wn, bm, rows, C, EPS, x_f32,
                                       nat.stream_ptr()), "rajni_layernorm_fp8")
        if shifted:
            assert sg.ptr() % 256 == 4 and hg.ptr() % 256 == 4 and qg.ptr() % 256 == 16
        return L, {"y_q": qg, "y_scale": sg, "hid_scale": hg}

    what = f"layernorm_fp8 {rows}x{C} {in_dt} cls_rows={cls_rows}"
    o = both(case, what, ["y_q", "y_scale", "hid_scale"])
    s_want = np.abs(want).max(axis=1) / 448.0
    s = o["y_scale"].t.cpu().numpy().astype(np.float64)
    nm.assert_within(s, s_want, bud.max(axis=1) / 448.0 + 2 * nm.U32 * s_want, f"{what}: y_scale")
    # the bytes: within one e4m3 rounding step of the fp64 LayerNorm (tests/test_gpu_guarded.py::test_layernorm_fp8_guarded)
    deq = o["y_q"].t.view(torch.float8_e4m3fn).to(torch.float32).cpu().numpy().astype(np.float64) * s[:, None]
    nm.assert_within(deq, want, np.maximum(np.abs(want) * 2.0 ** -4, s[:, None] * 2.0 ** -10) * 1.001 + bud + 1e-6 * np.abs(want).max(),
                     f"{what}: y_q")
    hs_want = (1.0625 * np.linalg.norm(want, axis=1) * wn + bm) / 448.0
    # ||o|| is off by at most ||per-element budget||_2 (triangle inequality); the sqrt, fma and division add a few u32
    hs_tol = 1.0625 * wn * np.linalg.norm(bud, axis=1) / 448.0 + 4 * nm.U32 * hs_want
    nm.assert_within(o["hid_scale"].t.cpu().numpy().astype(np.float64), hs_want, hs_tol, f"{what}: hid_scale")


@pytest.mark.parametrize("stream_dt,model_dt", [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
def test_layernorm_stream(stream_dt, model_dt):
    rows, C = 37, 192
    x, w, b, want, bud = ln_reference(rows, C, stream_dt, stream_dt)

    def case(shifted):
        L = Launch("rajni_layernorm_stream", shifted)
        xg = L.inp("x", dev(x, stream_dt))
        L.mark_output(xg)
        wg, bg = L.inp("w", dev(w, "fp32")), L.inp("b", dev(b, "fp32"))
        sync(lib().rajni_layernorm_stream(xg.ptr(), wg.ptr(), bg.ptr(), rows, C, EPS, nat.dtype_code(nm.TORCH[model_dt]),
                                          int(stream_dt == "fp32" and model_dt != "fp32"), nat.stream_ptr()), "rajni_layernorm_stream")
        return L, {"x": xg}

    what = f"layernorm_stream {stream_dt} stream, {model_dt} model"
    nm.assert_within(host(both(case, what, ["x"])["x"].t), want, bud, what)


@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_qk_norm(dt, D):
    rows, H = 21, 2
    qkv, qw, qb, kw, kb = cached(("qk", rows, H, D, dt), lambda: nv.qk_norm_case(rows, H, D, dt))
    want, bud = nv.qk_norm_budget(qkv, H, D, qw, qb, kw, kb, EPS, dt)

    def case(shifted):
        L = Launch("rajni_qk_norm", shifted)
        g = L.inp("qkv", dev(qkv, dt))
        L.mark_output(g)
        v = [L.inp(n, dev(a, "fp32")) for n, a in (("q_w", qw), ("q_b", qb), ("k_w", kw), ("k_b", kb))]
        sync(lib().rajni_qk_norm(g.ptr(), v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), rows, H, D, EPS, nat.dtype_code(nm.TORCH[dt]),
                                 nat.stream_ptr()), "rajni_qk_norm")
        return L, {"qkv": g}

    what = f"qk_norm {dt} D={D}"
    got = both(case, what, ["qkv"])["qkv"].t
    nm.assert_within(host(got)[:, :2 * H * D], want, bud, what)
    assert torch.equal(pl.bits(got[:, 2 * H * D:]), pl.bits(dev(qkv, dt)[:, 2 * H * D:])), f"{what}: the v third changed"


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("pool", ["token", "avg"])
@pytest.mark.parametrize("stream_dt,out_dt", [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16")])
def test_pool_norm(stream_dt, out_dt, pool, P):
    """rajni_pool_norm (P = 1) and rajni_pool_norm_prefix (P = 5), norm and fc_norm both present"""
    B, N, Cc = 3, 14, 192
    x, (nw, nb), (fw, fb) = cached(("pool", B, N, Cc, stream_dt), lambda: nv.pool_case(B, N, Cc, stream_dt))
    want, bud = nv.pool_norm_budget(x[:, P - 1:] if pool == "avg" else x, pool, (nw, nb, EPS), (fw, fb, 1e-5), out_dt)
    entry = "rajni_pool_norm" if P == 1 else "rajni_pool_norm_prefix"
    code, x_f32 = nat.dtype_code(nm.TORCH[out_dt]), int(stream_dt == "fp32" and out_dt != "fp32")
    pk = nat.POOL_AVG if pool == "avg" else nat.POOL_TOKEN

    def case(shifted):
        L = Launch(entry, shifted)
        xg = L.inp("x", dev(x, stream_dt))
        v = [L.inp(n, dev(a, "fp32")) for n, a in (("norm_w", nw), ("norm_b", nb), ("fc_w", fw), ("fc_b", fb))]
        og = L.out("out", (B, Cc), nm.TORCH[out_dt])
        if P == 1:
            rc = lib().rajni_pool_norm(xg.ptr(), B, N, Cc, pk, v[0].ptr(), v[1].ptr(), EPS, v[2].ptr(), v[3].ptr(), 1e-5, og.ptr(), code,
                                       x_f32, nat.stream_ptr())
        else:
            rc = lib().rajni_pool_norm_prefix(xg.ptr(), B, N, P, Cc, pk, v[0].ptr(), v[1].ptr(), EPS, v[2].ptr(), v[3].ptr(), 1e-5,
                                              og.ptr(), code, x_f32, nat.stream_ptr())
        sync(rc, entry)
        return L, {"out": og}

    what = f"{entry} {pool} {stream_dt}->{out_dt}"
    nm.assert_within(host(both(case, what, ["out"])["out"].t), want, bud, what)


# =================================================================================================================
# attention
# =================================================================================================================
@pytest.fixture(params=[0, 1, 2], ids=["persistent", "online_chunked", "full_row"])
def attn_mode(request):
    lib().rajni_debug_force_attention(request.param)
    yield request.param
    lib().rajni_debug_force_attention(0)


def attn_reference(kind, B, N, Np, H, D, dt):
    """a gathered case (keep_idx picks Np of N rows) and an identity case (the first Np rows ARE the image) of one qkv"""
    def make():
        qkv = nm.attention_qkv(kind, B, N, H, D, dt)
        idx = nm.pick_rows(np.random.default_rng(N + Np), B, N, Np)
        g = orc.gather_rows(qkv, idx.astype(np.int64))
        ident = np.ascontiguousarray(qkv[:, :Np])
        return dict(qkv=qkv, idx=idx, gathered=nm.attention_budget(g, H, D ** -0.5, dt), ident=ident,
                    identity=nm.attention_budget(ident, H, D ** -0.5, dt))
    return cached(("attn", kind, B, N, Np, H, D, dt), make)


def attention_case(B, N, Np, H, D, dt, with_idx, what, kind="peaked", nq=None):
    ref = attn_reference(kind, B, N, Np, H, D, dt)
    tdt = nm.TORCH[dt]
    qkv = dev(ref["qkv"] if with_idx else ref["ident"], dt)
    n_src = N if with_idx else Np
    want, bud = ref["gathered" if with_idx else "identity"]

    def case(shifted):
        L = Launch("rajni_attention", shifted)
        qg = L.inp("qkv", qkv)
        ig = L.idx("keep_idx", torch.from_numpy(ref["idx"]).to(DEV), fill=0) if with_idx else None
        og = L.out("out", (B, Np, H * D), tdt)
        if nq is None:
            rc = lib().rajni_attention(qg.ptr(), ptr(ig), og.ptr(), B, n_src, Np, H, D, D ** -0.5, nat.dtype_code(tdt), nat.stream_ptr())
        else:
            og.t.zero_()                            # the rows past the limited launch's last tile are not written
            rc = lib().rajni_debug_attention_rows(qg.ptr(), ptr(ig), og.ptr(), B, n_src, Np, nq, H, D, D ** -0.5, nat.dtype_code(tdt),
                                                  nat.stream_ptr())
        sync(rc, "rajni_attention")
        if shifted:
            assert qg.ptr() % 256 == 16 and og.ptr() % 256 == 16 and (ig is None or ig.ptr() % 256 == 4)
        return L, {"out": og}

    got = host(both(case, what, ["out"])["out"].t)
    rows = slice(None) if nq is None else slice(0, nq)
    nm.assert_within(got[:, rows], want[:, rows], bud[:, rows], what)


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_d64_every_mode(dt, with_idx, attn_mode):
    attention_case(2, 40, 33, 2, 64, dt, with_idx, f"attention (2,40,33,2) D=64 {dt} mode {attn_mode} keep_idx={with_idx}")


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_d64_past_the_persistent_kernel(dt, with_idx):
    attention_case(1, 300, 257, 2, 64, dt, with_idx, f"attention (1,300,257,2) D=64 {dt} keep_idx={with_idx}")


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
@pytest.mark.parametrize("D", [32, 80])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_general_head_dims(dt, D, with_idx):
    attention_case(2, 40, 33, 2, D, dt, with_idx, f"attention (2,40,33,2) D={D} {dt} keep_idx={with_idx}", kind="negative")


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
@pytest.mark.parametrize("D", [64, 80])
def test_attention_fp32(D, with_idx):
    attention_case(2, 40, 33, 2, D, "fp32", with_idx, f"attention fp32 (2,40,33,2) D={D} keep_idx={with_idx}")


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
@pytest.mark.parametrize("D,dt", [(64, "bf16"), (64, "fp16"), (80, "bf16"), (64, "fp32")])
def test_attention_row_limited(D, dt, with_idx):
    """the last block's launch (tests/test_gpu_attention_rows.py): query row 0 of each image only"""
    attention_case(2, 40, 33, 2, D, dt, with_idx, f"attention rows<1 (2,40,33,2) D={D} {dt} keep_idx={with_idx}", nq=1)


@pytest.mark.parametrize("with_idx", [False, True], ids=["identity", "keep_idx"])
def test_attention_fp8(with_idx):
    """e4m3 rows at + 16, row_scale at + 4; held to the bf16 kernel's output within one e4m3 step (tests/test_gpu_numerics.py)"""
    B, N, Np, H, D = 2, 40, 33, 2, 64
    ref = attn_reference("negative", B, N, Np, H, D, "bf16")
    qkv = dev(ref["qkv"] if with_idx else ref["ident"], "bf16")
    n_src = N if with_idx else Np
    want, bud = ref["gathered" if with_idx else "identity"]
    scale = float(F32(np.abs(want).max() / 448.0))

    def case(shifted):
        L = Launch("rajni_attention_fp8", shifted)
        qg = L.inp("qkv", qkv)
        ig = L.idx("keep_idx", torch.from_numpy(ref["idx"]).to(DEV), fill=0) if with_idx else None
        og, rg = L.out("out_q", (B, Np, H * D), torch.uint8), L.out("row_scale", (B * Np,), torch.float32)
        sync(lib().rajni_attention_fp8(qg.ptr(), ptr(ig), og.ptr(), scale, rg.ptr(), B, n_src, Np, H, D, D ** -0.5, nat.stream_ptr()),
             "rajni_attention_fp8")
        if shifted:
            assert rg.ptr() % 256 == 4 and og.ptr() % 256 == 16
        return L, {"out_q": og, "row_scale": rg}

    what = f"attention_fp8 (2,40,33,2) keep_idx={with_idx}"
    o = both(case, what, ["out_q", "row_scale"])
    assert bool((o["row_scale"].t == F32(scale)).all()), what
    deq = o["out_q"].t.view(torch.float8_e4m3fn).to(torch.float32).cpu().numpy().astype(np.float64) * np.float64(F32(scale))
    bound = np.maximum(np.abs(want) * 2.0 ** -4, scale * 2.0 ** -10) * 1.001 + bud + np.abs(want) * 2.0 ** -8 + 1e-6 * np.abs(want).max()
    nm.assert_within(deq, want, bound, what)


# =================================================================================================================
# importance, selection
# =================================================================================================================
def prefix_selection(s, keep, P):
    """the selection rule with P prefix tokens on scores s [B, N] (tests/numerics_prefix.py; P = 1: orc.select_tokens)"""
    sel = npx.select_tokens(s, keep, P)
    if P == 1:
        np.testing.assert_array_equal(sel, orc.select_tokens(s, keep))
    return sel.astype(np.int64)


def imp_reference(B, N, H, D, dt, kind="voffset"):
    def make():
        q = nm.importance_qkv(kind, B, N, H, D, dt)
        return (q,) + nm.importance_budget(q, H, dt)
    return cached(("imp", kind, B, N, H, D, dt), make)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B,N,H,D", [(3, 61, 4, 80), (2, 33, 2, 32)])
def test_score_select_family(B, N, H, D, dt, P):
    """rajni_importance, rajni_score_select[_prefix] and rajni_select_topk[_prefix]: qkv at + 16, scores one element past a
    256-byte boundary, keep_idx at + 4"""
    qkv, want, bud, e32 = imp_reference(B, N, H, D, dt)
    tdt = nm.TORCH[dt]
    code, eb = nat.dtype_code(tdt), tdt.itemsize
    keep = orc.keep_count(0.7, N - P + 1)
    qd = dev(qkv, dt)

    def imp_case(shifted):
        L = Launch("rajni_importance", shifted, elem_bytes=eb)
        qg, sg = L.inp("qkv", qd), L.out("scores_out", (B, N), tdt)
        sync(lib().rajni_importance(qg.ptr(), sg.ptr(), B, N, H, D, EPS, code, nat.stream_ptr()), "rajni_importance")
        if shifted:
            assert sg.ptr() % 256 == eb
        return L, {"scores_out": sg}

    what = f"importance {(B, N, H, D)} {dt}"
    scores = both(imp_case, what, ["scores_out"])["scores_out"].t.clone()
    s = host(scores)
    nm.assert_within(s, want, bud, what)

    def fused_case(shifted):
        entry = "rajni_score_select" if P == 1 else "rajni_score_select_prefix"
        L = Launch(entry, shifted, elem_bytes=eb)
        qg, sg = L.inp("qkv", qd), L.out("scores_out", (B, N), tdt)
        ig, ng = L.out("keep_idx", (B, P + keep), torch.int32), L.out("next_scores", (B, P + keep), tdt)
        if P == 1:
            rc = lib().rajni_score_select(qg.ptr(), B, N, H, D, EPS, keep, sg.ptr(), ig.ptr(), ng.ptr(), code, nat.stream_ptr())
        else:
            rc = lib().rajni_score_select_prefix(qg.ptr(), B, N, H, D, EPS, P, keep, sg.ptr(), ig.ptr(), ng.ptr(), code, nat.stream_ptr())
        sync(rc, entry)
        if shifted:
            assert ig.ptr() % 256 == 4 and ng.ptr() % 256 == eb
        return L, {"scores_out": sg, "keep_idx": ig, "next_scores": ng}

    def select_case(shifted):
        entry = "rajni_select_topk" if P == 1 else "rajni_select_topk_prefix"
        L = Launch(entry, shifted, elem_bytes=eb)
        sg = L.inp("scores", scores)
        ig, ng = L.out("keep_idx", (B, P + keep), torch.int32), L.out("next_scores", (B, P + keep), tdt)
        if P == 1:
            rc = lib().rajni_select_topk(sg.ptr(), B, N, keep, ig.ptr(), ng.ptr(), code, nat.stream_ptr())
        else:
            rc = lib().rajni_select_topk_prefix(sg.ptr(), B, N, P, keep, ig.ptr(), ng.ptr(), code, nat.stream_ptr())
        sync(rc, entry)
        return L, {"keep_idx": ig, "next_scores": ng}

    sel = prefix_selection(s, keep, P)
    for case, names, tag in ((fused_case, ["scores_out", "keep_idx", "next_scores"], "score_select"),
                             (select_case, ["keep_idx", "next_scores"], "select_topk")):
        o = both(case, f"{tag} P={P} {what}", names)
        if "scores_out" in o:
            assert torch.equal(pl.bits(o["scores_out"].t), pl.bits(scores)), f"{tag}: scores differ from rajni_importance's"
        np.testing.assert_array_equal(o["keep_idx"].t.cpu().numpy(), sel, err_msg=f"{tag} P={P} {what}")       # selection: exact
        np.testing.assert_array_equal(host(o["next_scores"].t), np.take_along_axis(s, sel, axis=1), err_msg=f"{tag} P={P} {what}")


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_score_select_ws_forced_tiled(dt):
    """the tile + finish kernels at N = 2 T + 3 (tests/test_gpu_score_tiled.py forces them the same way): the scratch stays on
    its 256-byte boundary, everything else is shifted"""
    B, H, D, P = 2, 2, 64, 2
    N = 2 * nat.SCORE_TILE_TOKENS + 3
    qkv, want, bud, e32 = imp_reference(B, N, H, D, dt, kind="peaked")
    tdt = nm.TORCH[dt]
    code, eb = nat.dtype_code(tdt), tdt.itemsize
    keep = 20
    lib().rajni_debug_force_score_tiled(1)
    try:
        nbytes = lib().rajni_score_select_workspace_bytes(B, N, H, D, code)
        assert nbytes > 0

        def case(shifted):
            L = Launch("rajni_score_select_ws", shifted, elem_bytes=eb)
            qg, sg = L.inp("qkv", dev(qkv, dt)), L.out("scores_out", (B, N), tdt)
            ig, ng = L.out("keep_idx", (B, P + keep), torch.int32), L.out("next_scores", (B, P + keep), tdt)
            wg = L._make("workspace", (nbytes,), torch.uint8, 0, False)
            assert wg.ptr() % 256 == 0
            sync(lib().rajni_score_select_ws(qg.ptr(), B, N, H, D, EPS, P, keep, sg.ptr(), ig.ptr(), ng.ptr(), code, wg.ptr(), nbytes,
                                             nat.stream_ptr()), "rajni_score_select_ws")
            return L, {"scores_out": sg, "keep_idx": ig, "next_scores": ng}

        what = f"score_select_ws tiled {(B, N, H, D)} {dt}"
        o = both(case, what, ["scores_out", "keep_idx", "next_scores"])
    finally:
        lib().rajni_debug_force_score_tiled(0)
    s = host(o["scores_out"].t)
    nm.assert_within(s, want, bud, what)
    sel = prefix_selection(s, keep, P)
    np.testing.assert_array_equal(o["keep_idx"].t.cpu().numpy(), sel, err_msg=what)
    np.testing.assert_array_equal(host(o["next_scores"].t), np.take_along_axis(s, sel, axis=1), err_msg=what)


# =================================================================================================================
# gather, patch embed
# =================================================================================================================
def test_gather_rows_of_48_bytes():
    """B = 2, 40 -> 13 rows of 24 bf16 elements: rows 48 bytes apart from a base at + 16, no row on a 128-byte line twice in a row"""
    B, n_src, n_dst, E = 2, 40, 13, 24
    g = torch.Generator(device=DEV).manual_seed(5)
    src = torch.randn((B, n_src, E), generator=g, device=DEV).to(torch.bfloat16)
    idx = torch.from_numpy(nm.pick_rows(np.random.default_rng(3), B, n_src, n_dst)).to(DEV)

    def case(shifted):
        L = Launch("rajni_gather_rows", shifted)
        sg, ig, og = L.inp("src", src), L.idx("idx", idx, fill=0), L.out("dst", (B, n_dst, E), torch.bfloat16)
        sync(lib().rajni_gather_rows(sg.ptr(), ig.ptr(), og.ptr(), B, n_src, n_dst, E, nat.RAJNI_BF16, nat.stream_ptr()), "rajni_gather_rows")
        return L, {"dst": og}

    got = both(case, "gather_rows", ["dst"])["dst"].t
    assert torch.equal(pl.bits(got), pl.bits(torch.gather(src, 1, idx[:, :, None].expand(-1, -1, E))))


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("fmt", ["bf16", "bf16_to_f32", "fp16", "fp32"])
@pytest.mark.parametrize("S,Pz,Cc,B", [(64, 16, 128, 3), (56, 14, 128, 3)], ids=["patch16_fused", "patch14_columns"])
def test_patch_embed(S, Pz, Cc, B, fmt, P):
    """rajni_patch_embed (P = 1) / rajni_patch_embed_prefix (P = 5): images, weight, bias, cls, reg, pos, x and the column
    workspace of the materialised case at + 16.  The patch rows are a GEMM with bias and one more add (pos): nm.budget_bias
    with the pos row inside want and S; the prefix rows are ONE fp32 add rounded once: exact"""
    dt = fmt.split("_")[0]
    out_f32 = fmt.endswith("_to_f32")
    tdt = nm.TORCH[dt]
    xdt = torch.float32 if out_f32 else tdt
    Cin, K, n = 3, 3 * Pz * Pz, (S // Pz) ** 2
    kpad = ceil(K, 64)

    def make():
        rng = np.random.default_rng([S, Pz, Cc, B, P])
        img = nm.round_to(rng.standard_normal((B, Cin, S, S), dtype=F32), dt)
        w = nm.round_to(0.05 * rng.standard_normal((Cc, K), dtype=F32), dt)
        b = nm.round_to(0.1 * rng.standard_normal(Cc, dtype=F32), dt)
        pre_rows = nm.round_to(rng.standard_normal((P, Cc), dtype=F32), dt)           # cls, then the registers
        pos = nm.round_to(rng.standard_normal((P + n, Cc), dtype=F32), dt)
        cols = img.reshape(B, Cin, S // Pz, Pz, S // Pz, Pz).transpose(0, 2, 4, 1, 3, 5).reshape(B * n, K)
        pre, Sm, g = nm.gemm_pre(cols, w, b)
        p64 = np.tile(pos[P:].astype(np.float64), (B, 1))
        return img, w, b, pre_rows, pos, pre + p64, Sm + np.abs(p64), g
    img, w, b, pre_rows, pos, want, Sm, g = cached(("pe", S, Pz, Cc, B, P, dt), make)
    entry = "rajni_patch_embed" if P == 1 else "rajni_patch_embed_prefix"
    code = nat.dtype_code(tdt)
    nbytes = lib().rajni_patch_embed_workspace_bytes(B, Cin, S, Pz, code)
    assert (nbytes == 0) == (Pz == 16)

    def case(shifted):
        L = Launch(entry, shifted)
        ig = L.inp("images", dev(img, dt))
        wg = L._make("w", (ceil(Cc, 256), kpad), tdt, 0, False)
        wg.t[:Cc].zero_()
        wg.t[:Cc, :K].copy_(dev(w, dt))
        bg, cg, pg = L.inp("bias", dev(b, "fp32")), L.inp("cls", dev(pre_rows[0], dt)), L.inp("pos", dev(pos, dt))
        rg = L.inp("reg", dev(pre_rows[1:], dt)) if P > 1 else None
        xg = L.out("x", (B, P + n, Cc), xdt)
        ws = L._make("workspace", (B * n, kpad), tdt, 0, True) if nbytes else None
        assert ws is None or ws.region == nbytes
        if P == 1:
            rc = lib().rajni_patch_embed(ig.ptr(), wg.ptr(), bg.ptr(), cg.ptr(), pg.ptr(), 1, xg.ptr(), int(out_f32), B, Cin, S, Pz, Cc,
                                         code, ptr(ws), nbytes, nat.stream_ptr())
        else:
            rc = lib().rajni_patch_embed_prefix(ig.ptr(), wg.ptr(), bg.ptr(), cg.ptr(), rg.ptr(), P, pg.ptr(), 1, xg.ptr(), int(out_f32),
                                                B, Cin, S, Pz, Cc, code, ptr(ws), nbytes, nat.stream_ptr())
        sync(rc, entry)
        if shifted:
            assert ig.ptr() % 256 == 16 and xg.ptr() % 256 == 16 and (ws is None or ws.ptr() % 256 == 16)
        return L, {"x": xg}

    what = f"{entry} S={S} patch={Pz} {fmt}"
    x = both(case, what, ["x"])["x"].t
    out_dt = "fp32" if xdt == torch.float32 else dt
    nm.assert_within(host(x[:, P:]).reshape(B * n, Cc), want, nm.budget_bias(want, Sm, g, out_dt), what)
    prefix = (torch.from_numpy(pre_rows) + torch.from_numpy(pos[:P])).to(DEV).to(xdt)
    for bi in range(B):
        assert torch.equal(pl.bits(x[bi, :P]), pl.bits(prefix)), f"{what}: prefix rows of image {bi}"


# =================================================================================================================
# the whole forward
# =================================================================================================================
SCHED = {1: {"keep_ratio": 0.5, "update": True}, 2: {"keep_ratio": 0.75, "update": False}}      # keeps (0, 8, 6, 0) of 16 patches
MICRO = dict(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=16)                # patch 16, hidden 512
BLOCK_TENSORS = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w",
                 "fc2_b", "ls2", "qkv_s", "proj_s", "fc1_s", "fc2_s")
PLAN_TENSORS = (("patch_w", "patch_w"), ("patch_b", "patch_b"), ("cls_token", "cls"), ("pos_embed", "pos"), ("norm_w", "norm_w"),
                ("norm_b", "norm_b"), ("head_w", "head_w"), ("head_b", "head_b"))
LOGITS_LD = 24


def forward_at(w, images, shifted):
    """the wrapper's plan rebuilt by hand with EVERY pointer in a guarded buffer at this launch's placement: weights, vectors,
    keep_idx, scores, next_scores, images, logits (logits_ld = 24) and the workspace (on its 256-byte minimum, exactly
    rajni_vit_workspace_bytes, poisoned)"""
    plan0, (_, _, _, W, ext0, _, pre0), bufs = w._plan[1], w._plan[2], w._plan[3]
    depth, B, ncls = plan0.depth, plan0.B, plan0.num_classes
    tdt = images.dtype
    L = Launch("rajni_vit_plan", shifted, elem_bytes=tdt.itemsize)
    plan = nat.VitPlan.from_buffer_copy(plan0)
    for field, key in PLAN_TENSORS:
        setattr(plan, field, ptr(L.inp(field, W[key])))
    blocks = (nat.Block * depth)(*[nat.Block.from_buffer_copy(plan0.blocks[i]) for i in range(depth)])
    stages = {}
    for i, bw in enumerate(W["blocks"]):
        for name in BLOCK_TENSORS:
            setattr(blocks[i], name, ptr(L.inp(f"block {i} {name}", bw[name], entry="rajni_block", key=name)))
        if i in bufs:
            st = {name: L.out(f"block {i} {name}", tuple(bufs[i][name].shape), bufs[i][name].dtype, entry="rajni_block", key=name)
                  for name in ("keep_idx", "scores", "next_scores")}
            blocks[i].keep_idx, blocks[i].scores, blocks[i].next_scores = st["keep_idx"].ptr(), st["scores"].ptr(), st["next_scores"].ptr()
            stages[i] = st
    plan.blocks = blocks
    tc = (C.c_int32 * depth)(*([-1] * depth))
    plan.token_counts = tc
    ext = qk = pre = None
    if ext0 is not None:
        ext = nat.VitExt.from_buffer_copy(ext0)
        if ext0.qk_norm:
            qk = (nat.QkAffine * depth)()
            for i, bw in enumerate(W["blocks"]):
                for name in pl.CONTRACT["rajni_qk_affine"]:
                    setattr(qk[i], name, ptr(L.inp(f"block {i} {name}", bw[name], entry="rajni_qk_affine", key=name)))
            ext.qk_norm = qk
        for name in pl.CONTRACT["rajni_vit_ext"]:
            setattr(ext, name, ptr(L.inp(name, W[name], entry="rajni_vit_ext")))
    if pre0 is not None:
        pre = nat.VitPrefix()
        pre.num_prefix, pre.reg_token = pre0.num_prefix, L.inp("reg_token", W["reg"], entry="rajni_vit_prefix").ptr()
    nbytes = plan0.workspace_bytes
    ws = L._make("workspace", (nbytes,), torch.uint8, 0, False)
    assert ws.ptr() % 256 == 0
    plan.workspace, plan.workspace_bytes, plan.logits_ld = ws.ptr(), nbytes, LOGITS_LD
    ig = L.inp("images", images, entry="rajni_vit_forward")
    lg = L._make("logits", (B, ncls), tdt, 0, True, entry="rajni_vit_forward", stride=LOGITS_LD)
    sync(lib().rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext) if ext is not None else None,
                                            C.byref(pre) if pre is not None else None, ig.ptr(), lg.ptr(), nat.stream_ptr()),
         "rajni_vit_forward_ext_prefix")
    if shifted:
        assert plan.patch_w % 256 == 16 and blocks[1].keep_idx % 256 == 4 and blocks[1].next_scores % 256 == tdt.itemsize
        assert blocks[0].norm1_w % 256 == 16 and ig.ptr() % 256 == 16 and lg.ptr() % 256 == 16
    return L, lg, stages, [int(tc[i]) for i in range(depth)]


FWD_CASES = [("bf16", False, False), ("bf16", True, False), ("fp16", False, False), ("fp32", False, False), ("bf16", False, True)]


@pytest.mark.parametrize("dt,stream16,variant", FWD_CASES,
                         ids=["bf16-f32stream", "bf16-bf16stream", "fp16", "fp32", "bf16-qknorm-prenorm-5prefix"])
def test_whole_forward(dt, stream16, variant):
    """The micro plan (img 64, patch 16, depth 4, C 128, hidden 512, 16 classes, keeps (0, 8, 6, 0)): logits, selections,
    carried scores and token counts of the shifted plan are the aligned plan's bit for bit, both are the wrapper's own
    forward (a third placement: torch's allocations), and the logits meet the restated float64 graph with the device's
    selections injected at the project's bars (1e-2 of the logit scale for 16-bit models, 2e-2 with a 16-bit stream, 1e-3 fp32)"""
    cfg = ts.ViTConfig(**MICRO, **(dict(qk_norm=True, pre_norm=True, reg_tokens=4) if variant else {}))
    model = ts.create_model(cfg, seed=11, std=0.08, bias_std=0.1, round_bf16=True)
    sd = ts.state_dict_numpy(model)
    tdt = nm.TORCH[dt]
    w = rajni_amd.RAJNIViTWrapper(model, SCHED).to(DEV).to(tdt).eval().trace_scores(True)
    if stream16:
        w.set_residual_dtype(tdt)
    imgs = ts.bf16_round_np(np.random.default_rng(2).standard_normal((4, 3, 64, 64), dtype=F32))
    x = torch.from_numpy(imgs).to(DEV).to(tdt)
    own = w(x).clone()
    P = 1 + cfg.reg_tokens
    assert w.get_last_stats()["token_counts"] == [16 + P, 16 + P, 8 + P, 6 + P]
    trace = {i: {k: v.clone() for k, v in t.items() if v is not None} for i, t in w._plan[3].items()}      # the plan's own buffers
    what = f"forward {dt} stream16={stream16} variant={variant}"
    (la, lga, sta, tca), (lb, lgb, stb, tcb) = forward_at(w, x, False), forward_at(w, x, True)
    for L in (la, lb):
        for name, g, out in L.bufs:       # block 2 carries block 1's scores: its own scores buffer is never written
            g.check(f"{what} [{'shifted' if L.shifted else 'aligned'}]: {name}", written=out and name != "block 2 scores")
    assert_same_bits(lga, lgb, f"{what}: logits")
    assert tca == tcb == w.get_last_stats()["token_counts"], what
    for i in sta:
        for name in ("keep_idx", "next_scores") + (("scores",) if i == 1 else ()):
            assert_same_bits(sta[i][name], stb[i][name], f"{what}: block {i} {name}")
            assert torch.equal(pl.bits(sta[i][name].t), pl.bits(trace[i][name])), f"{what}: block {i} {name} differs from the wrapper's"
    assert torch.equal(pl.bits(lga.t), pl.bits(own)), f"{what}: logits differ from the wrapper's own forward"
    forced = {i: t["keep_idx"].cpu().numpy().astype(np.int64) for i, t in trace.items()}
    want, counts, _ = npx.vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced)
    assert counts == tca
    bar = 1e-3 if dt == "fp32" else (2e-2 if stream16 else 1e-2)
    err, scale = float(np.abs(host(lga.t) - want).max()), float(np.abs(want).max())
    print(f"[placement] {what}: max |dlogit| {err:.4g} (scale {scale:.4g}, bar {bar * scale:.4g})")
    assert err <= bar * scale, f"{what}: max |dlogit| {err:.4g} vs scale {scale:.4g}"
