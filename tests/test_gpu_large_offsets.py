"""Every kernel at offsets past 2^31 bytes, 2^32 bytes and 2^31 elements from a tensor's base pointer.  GPU box only (`-m gpu`).

High-resolution and large-batch workloads put qkv, the MLP hidden buffer and the residual stream beyond those sizes (qkv of 64
images at 2048 px is 2.4e9 bf16 elements), where a 32-bit element index, an unsigned 32-bit byte offset and a signed one all
wrap.  The kernels form such offsets in 64 bits (include/rajni_hip.h, "addressing limits"); these tests are what notices when
one of them is narrowed.

Method.  Every kernel is deterministic and an image's / a row's result does not depend on its place in the batch, so each case
runs the kernel twice - once with operands that reach past the thresholds, once with the same values where every offset is
small (a dense copy of strided rows, or a tail slice: the same memory from a pointer advanced past the threshold) - and the
two outputs must agree bit for bit.  Dense row kernels get periodic inputs (a block of P = 4099 rows repeated; P is prime, and
2^31 and 2^32 are no multiples of a row, so a wrapped offset lands on another phase) and every output row r must equal row
r mod P.  The small call, or the first period, is held to the fp64 reference and the per-element budget the kernel already has
(tests/numerics*.py); no tolerance is introduced here.  Outputs are pre-filled with 0xFF bytes, so a row stored at a wrapped
address leaves NaNs behind where it belonged.

Memory: tests/bigmem.py allocates with torch.empty, touches only the rows in use, counts every test's allocations against a
cap of 24 GiB and frees them when the test ends.  Nothing large is copied to the host or walked from Python.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bigmem as bm
import numerics as nm
import numerics_variants as nv
from oracle import rajni_oracle as orc
from rajni_amd import ops, _native as nat

DEV = "cuda"
EPS = 1e-6
P = bm.PERIOD
F32 = np.float32
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if dt == "fp32" else t.to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def lib():
    return nat.lib()


def stream():
    return nat.stream_ptr()


def poison(t):
    """0xFF bytes (NaN in every float format here) over a view's own elements"""
    bm.bits(t).fill_(-1 if t.element_size() > 1 else 255)
    return t


@pytest.fixture
def big(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    b = bm.Big(DEV)
    yield b
    torch.cuda.synchronize()
    print(f"\n[bigmem] {request.node.name}: peak {torch.cuda.max_memory_allocated() / bm.GIB:.2f} GiB allocated "
          f"({b.peak / bm.GIB:.2f} GiB counted)")
    b.close()


class forced:
    """a debug hook set for the block and reset to 0 after it"""

    def __init__(self, hook, value):
        self.fn, self.value = getattr(lib(), hook), value

    def __enter__(self):
        self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# rajni_linear: crossing by row stride
# ---------------------------------------------------------------------------------------------------------------
M_LIN = 1100                      # ragged against the 128- and 256-row tiles; >= 1024: the persistent tilings take it
LD = (1 << 21) + 64               # row stride in elements: row 1024 starts 2^31 + 65536 elements from the base
LD8 = (1 << 22) + 64              # row stride of e4m3 rows in bytes: row 1024 starts 2^32 + 65536 bytes from the base
assert bm.first_row_past(LD, bm.T31) == 1024 < M_LIN and bm.first_row_past(LD8, bm.T32) == 1024
TILING_IDS = {0: "auto", 1: "small128x128", 4: "wide256x256", 5: "mid256x128"}


def linear_call(x, w, N, bias, epi, y, dtype, gamma=None, resid=None, r_idx=None, r_nsrc=0, stream_f32=0, w_scale=None,
                x_scale=None, y_scale=None):
    """one rajni_linear launch on 2-D (possibly row-strided) views: lda / ldc / ldr are the views' row strides"""
    a = nat.LinearArgs()
    a.x, a.lda, a.w, a.ldw = x.data_ptr(), x.stride(0), w.data_ptr(), w.shape[1]
    a.bias, a.gamma = bias.data_ptr(), nat.ptr(gamma)
    a.w_scale, a.x_scale, a.y_scale = nat.ptr(w_scale), nat.ptr(x_scale), nat.ptr(y_scale)
    a.y, a.ldc = y.data_ptr(), y.stride(0)
    a.M, a.N, a.K, a.epilogue, a.dtype, a.stream_f32 = x.shape[0], N, x.shape[1], epi, dtype, stream_f32
    if resid is not None:
        a.resid, a.ldr = resid.data_ptr(), resid.stride(-2)
        if r_idx is not None:
            a.r_idx, a.r_np, a.r_nsrc = r_idx.data_ptr(), r_idx.shape[1], r_nsrc
    nat.check(lib().rajni_linear(C.byref(a), stream()), "rajni_linear")


def lin_reference(N, K, dt, w8, M=M_LIN):
    def make():
        x, w, b = nm.gemm_operands(M, N, K, dt)
        q = s = None
        if w8:
            q, s = ops.pack_weight_fp8(torch.from_numpy(w), nm.TORCH[dt])
            w = (q[:N].view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64) * s.to(torch.float64)[:, None]).numpy()
        return (x, w, b) + nm.gemm_pre(x, w, b) + (q, s)
    return cached(("lin", M, N, K, dt, w8), make)


def rows_at(big, src, ld):
    """the rows of the dense device tensor `src` [M, cols] at row stride `ld` in a large buffer (ld None: src itself)"""
    if ld is None:
        return src
    v = big.rows(src.shape[0], src.shape[1], ld, src.dtype)
    v.copy_(src)
    return v


def out_at(big, M, cols, ld, dtype):
    """poisoned output rows [M, cols]: at row stride `ld` in a large buffer, or dense"""
    v = big.rows(M, cols, ld, dtype) if ld is not None else torch.empty((M, cols), dtype=dtype, device=DEV)
    return poison(v)


EPI_IDS = {nat.EPI_BIAS: "bias", nat.EPI_BIAS_GELU: "gelu", nat.EPI_BIAS_RESID: "resid"}


def linear_case(big, dt, epi, cross, tiling, N, K, stream_dt=None, inplace=True, w8=False, M=M_LIN):
    """The launch on large-stride operands (`cross`: which of x / y+resid sit at row stride LD; "y_only": y alone, beside a
    dense residual operand) against the same launch on dense operands, bit for bit over all M rows; the dense launch against
    the fp64 budget."""
    assert cross in ("x", "y", "both", "y_only") and (cross != "y_only" or not inplace)
    x, w, b, pre, S, g, q, s = lin_reference(N, K, dt, w8, M)
    tdt = nm.TORCH[dt]
    stream_dt = stream_dt or dt
    ydt = nm.TORCH[stream_dt] if epi == nat.EPI_BIAS_RESID else tdt
    xd, bd = dev(x, dt), dev(b, "fp32")
    wd, wsd = (q.to(DEV), s.to(DEV)) if w8 else (ops.pack_weight(dev(w, dt), tdt), None)
    rd = gd = None
    if epi == nat.EPI_BIAS_RESID:
        r, gam, _ = nm.resid_operands(1, M, M, N, dt, stream_dt)
        rd, gd = dev(r.reshape(M, N), stream_dt), dev(gam, "fp32")
    got = {}
    for layout in ("large", "dense"):
        far_x = LD if layout == "large" and cross in ("x", "both") else None
        far_y = LD if layout == "large" and cross in ("y", "both", "y_only") else None
        far_r = far_y if cross != "y_only" else None
        xv = rows_at(big, xd, far_x)
        yv = out_at(big, M, N, far_y, ydt)
        rv = None
        if rd is not None:
            if inplace:
                yv.copy_(rd)
                rv = yv
            else:
                rv = rows_at(big, rd, far_r)
        with forced("rajni_debug_force_gemm_tiling", tiling):
            linear_call(xv, wd, N, bd, epi, yv, nat.dtype_code(tdt), gamma=gd, resid=rv,
                        stream_f32=int(stream_dt == "fp32" and dt != "fp32"), w_scale=wsd)
        got[layout] = yv.contiguous() if far_y is not None else yv
        if layout == "large":
            for v, far in ((xv, far_x), (yv, far_y)):
                if far is not None:
                    bm.assert_crosses_all((M - 1) * far + v.shape[1], v.element_size(), "linear operand")
    what = f"linear {dt} {EPI_IDS[epi]} {M}x{N}x{K} crossing {cross} tiling {TILING_IDS[tiling]} stream {stream_dt} w8 {w8}"
    bm.assert_bit_equal(got["large"], got["dense"], what + ": large strides vs dense")
    y = host(got["dense"])
    if epi == nat.EPI_BIAS:
        nm.assert_within(y, pre, nm.budget_bias(pre, S, g, dt), what)
    elif epi == nat.EPI_BIAS_GELU:
        a_gelu = nm.a_gelu_fp32(pre) if dt == "fp32" else nm.A_GELU_16
        nm.assert_within(y, orc.gelu(pre), nm.budget_gelu(pre, S, g, dt, a_gelu), what)
    else:
        want, bud = nm.budget_resid(pre, S, g, r.reshape(M, N).astype(np.float64), gam.astype(np.float64), stream_dt)
        nm.assert_within(y, want, bud, what)


@pytest.mark.parametrize("tiling", [0, 1, 4, 5], ids=list(TILING_IDS.values()))
@pytest.mark.parametrize("cross", ["x", "y", "both"])
def test_linear_resid_fp32_stream_in_place_at_large_strides(big, cross, tiling):
    """proj / fc2 as the forward runs them (bf16 x, fp32 residual stream, y in place on resid), M = 1100, N = 256, K = 512.
    Crossing: x (bf16, lda = 2^21 + 64: 4.6 GB), y = resid (fp32, ldc = ldr = 2^21 + 64: 9.2 GB), or both (13.8 GB).  All rows
    are checked; row 512 of y starts 2^32 + 131072 bytes from its base, row 1024 of either 2^31 + 65536 elements (x: 2^32 +
    131072 bytes).  With y crossing, resid rows x ldr >= 2^31: the 256 x 128 tiling's 32-bit residual offsets do not serve
    it and the host must fall back to 128 x 128, by shape (auto) and under the forced hook, with the same bits."""
    linear_case(big, "bf16", nat.EPI_BIAS_RESID, cross, tiling, 256, 512, stream_dt="fp32")


@pytest.mark.parametrize("tiling", [0, 5], ids=["auto", "mid256x128"])
def test_linear_resid_in_place_whole_tile_past_2_31_elements(big, tiling):
    """M = 1300 instead of 1100: at 1100 rows every row past 2^31 elements (1024..) sits in the ragged last row tile, which takes
    the guarded epilogue with 64-bit offsets whatever the host decides; at 1300 rows 1024..1279 form a whole 256-row tile, the
    only kind the 256 x 128 tiling's full-line epilogue (32-bit residual offsets) serves.  y = resid in place, fp32, ldc = ldr =
    2^21 + 64 (10.9 GB): the host must send the launch to 128 x 128.  Row 1024 starts 2^33 + 262144 bytes from the base."""
    linear_case(big, "bf16", nat.EPI_BIAS_RESID, "y", tiling, 256, 512, stream_dt="fp32", M=1300)


M_TILE = 1300     # rows 1024..1279: a whole 256-row tile past 2^31 elements at row stride LD; rows 1280..1299: a ragged tail
assert bm.first_row_past(LD, bm.T31) == 1024 and 1024 + 256 <= M_TILE and M_TILE % 128 != 0
# name: (epilogue, stream dtype or None, e4m3 weights)
WHOLE_TILE = {"bias": (nat.EPI_BIAS, None, False), "gelu": (nat.EPI_BIAS_GELU, None, False),
              "resid16": (nat.EPI_BIAS_RESID, "bf16", False), "resid32": (nat.EPI_BIAS_RESID, "fp32", False),
              "resid32-w8": (nat.EPI_BIAS_RESID, "fp32", True)}


@pytest.mark.parametrize("tiling", [0, 1, 4, 5], ids=list(TILING_IDS.values()))
@pytest.mark.parametrize("name", list(WHOLE_TILE))
def test_linear_whole_tile_past_2_31_elements(big, name, tiling):
    """The stream tilings (256 x 256, 256 x 128) store a tile whose 256 rows and all columns exist through unguarded interior
    epilogues - the bulk of all tiles in a forward - and every other tile through the guarded general one.  At M = 1100 the rows
    past 2^31 elements (1024..) all lie in the ragged last tile, so there only the general epilogue ever forms a large offset.
    Here M = 1300, N = 256, K = 512: rows 1024..1279 are an interior tile on both stream tilings (two on 128 x 128), rows
    1280..1299 the ragged tail.  x and y (RESID: y = resid in place) at row stride 2^21 + 64: x bf16 5.4 GB, y bf16 5.4 GB /
    fp32 10.9 GB; row 1024 starts 2^32 + 131072 bytes into a 16-bit operand, 2^33 + 262144 into an fp32 one.  Epilogues: BIAS and
    GELU (bf16 out), RESID on a bf16 and on an fp32 stream, the latter with e4m3 weights too (another interior epilogue on
    256 x 256).  With an fp32 stream the 256 x 128 tiling is rerouted to 128 x 128 by the host (resid rows x ldr >= 2^31);
    test_linear_interior_store_at_large_ldc_beside_a_dense_residual keeps it on 256 x 128."""
    epi, stream_dt, w8 = WHOLE_TILE[name]
    linear_case(big, "bf16", epi, "both", tiling, 256, 512, stream_dt=stream_dt, w8=w8, M=M_TILE)


@pytest.mark.parametrize("tiling", [0, 5, 4], ids=["auto", "mid256x128", "wide256x256"])
@pytest.mark.parametrize("stream_dt", ["fp32", "bf16"])
def test_linear_interior_store_at_large_ldc_beside_a_dense_residual(big, stream_dt, tiling):
    """RESID out of place with a DENSE residual operand and y at row stride 2^21 + 64, M = 1300: resid rows x ldr is small, so
    the host keeps the 256 x 128 tiling (auto picks it for this shape) and its interior epilogue - residual rows prefetched with
    32-bit offsets, which is right here - stores rows 1024..1279 at (long)row * ldc past 2^31 elements of y (fp32 10.9 GB: row
    1024 starts 2^33 + 262144 bytes from the base; bf16 5.4 GB: 2^32 + 131072).  No other case reaches that store with a large
    ldc: whenever resid crosses with y, the launch goes to 128 x 128."""
    linear_case(big, "bf16", nat.EPI_BIAS_RESID, "y_only", tiling, 256, 512, stream_dt=stream_dt, inplace=False, M=M_TILE)


@pytest.mark.parametrize("tiling", [0, 1, 4, 5], ids=list(TILING_IDS.values()))
def test_linear_resid_fp32_stream_fp8_weights_at_large_strides(big, tiling):
    """the same launch with e4m3 weights (w_scale), x and y = resid both at row stride 2^21 + 64 (13.8 GB); first row past 2^31
    elements: row 1024, 2^32 + 131072 bytes into x, 2^33 + 262144 bytes into y"""
    linear_case(big, "bf16", nat.EPI_BIAS_RESID, "both", tiling, 256, 512, stream_dt="fp32", w8=True)


@pytest.mark.parametrize("tiling", [0, 5], ids=["auto", "mid256x128"])
def test_linear_resid_out_of_place_at_large_strides(big, tiling):
    """resid and y separate tensors, both at row stride 2^21 + 64, fp32 stream (2 x 9.2 GB), N = 200 (ragged against the
    128-column tile), K = 256; row 1024 starts 2^33 + 262144 bytes into each.  The residual operand alone spans >= 2^31 elements."""
    linear_case(big, "bf16", nat.EPI_BIAS_RESID, "y", tiling, 200, 256, stream_dt="fp32", inplace=False)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("tiling", [0, 4], ids=["auto", "wide256x256"])
def test_linear_resid_16bit_stream_at_large_strides(big, dt, tiling):
    """16-bit residual stream (bf16 / fp16 models with resid_bf16): x, resid and y at row stride 2^21 + 64, resid out of place
    (3 x 4.6 GB); row 1024 starts 2^32 + 131072 bytes into each"""
    linear_case(big, dt, nat.EPI_BIAS_RESID, "both", tiling, 200, 256, inplace=False)


@pytest.mark.parametrize("tiling", [0, 1, 4, 5], ids=list(TILING_IDS.values()))
@pytest.mark.parametrize("epi,N,K", [(nat.EPI_BIAS, 200, 256), (nat.EPI_BIAS_GELU, 256, 512)], ids=["bias", "gelu"])
def test_linear_bias_gelu_at_large_strides(big, epi, N, K, tiling):
    """qkv / fc1 (bf16 in, bf16 out): x and y at row stride 2^21 + 64 (2 x 4.6 GB); row 1024 starts 2^32 + 131072 bytes into each"""
    linear_case(big, "bf16", epi, "both", tiling, N, K)


@pytest.mark.parametrize("epi", [nat.EPI_BIAS, nat.EPI_BIAS_GELU, nat.EPI_BIAS_RESID], ids=["bias", "gelu", "resid"])
def test_linear_fp16_at_large_strides(big, epi):
    """fp16 models: x and y (fp16; RESID: the fp32 stream, in place) at row stride 2^21 + 64; row 1024 starts 2^32 + 131072 bytes
    into x"""
    linear_case(big, "fp16", epi, "both", 0, 256, 512, stream_dt="fp32" if epi == nat.EPI_BIAS_RESID else None)


@pytest.mark.parametrize("epi,cross", [(nat.EPI_BIAS, "both"), (nat.EPI_BIAS_GELU, "x"), (nat.EPI_BIAS_RESID, "y")],
                         ids=["bias-both", "gelu-x", "resid-y"])
def test_linear_fp32_at_large_strides(big, epi, cross):
    """the fp32 accuracy path: fp32 x and / or y at row stride 2^21 + 64 (9.2 GB each); row 512 starts 2^32 + 131072 bytes from
    the base, row 1024 2^31 + 65536 elements"""
    linear_case(big, "fp32", epi, cross, 0, 200, 256)


# ---- fp8 x fp8 --------------------------------------------------------------------------------------------------

def f8_reference(M, N, K):
    def make():
        x, w, b = nm.gemm_operands(M, N, K, "bf16")
        (xq, xs), (wq, ws) = ops.quantize_rows_fp8(torch.from_numpy(x)), ops.quantize_rows_fp8(torch.from_numpy(w))
        f64 = lambda qq, sc: qq.to(torch.float32).to(torch.float64).numpy() * sc.to(torch.float64).numpy()[:, None]
        pre, S, g = nm.gemm_pre(f64(xq, xs), f64(wq, ws), b)
        wp = torch.zeros(((N + 255) // 256 * 256, K), dtype=torch.uint8)
        wp[:N] = wq.view(torch.uint8)
        return xq.view(torch.uint8), xs, wp, ws, b, pre, S, g
    return cached(("f8", M, N, K), make)


@pytest.mark.parametrize("M", [M_LIN, M_TILE])
@pytest.mark.parametrize("f8_tiling", [1, 2], ids=["f8_256x128", "f8_256x256"])
@pytest.mark.parametrize("epi", [nat.EPI_BIAS, nat.EPI_BIAS_GELU, nat.EPI_BIAS_RESID], ids=["bias", "gelu_e4m3", "resid"])
def test_linear_fp8_x_fp8_at_large_strides(big, epi, f8_tiling, M):
    """e4m3 x (lda in BYTES = 2^22 + 64: 4.6 GB, row 1024 starts 2^32 + 65536 bytes from the base) on the fp8 matrix pipe,
    M = 1100 (rows 1024.. in the ragged last tile: the guarded epilogue) and 1300 (rows 1024..1279 a whole tile: the interior
    epilogues of both tilings), N = 256, K = 512.  y: bf16 at ldc = 2^21 + 64 elements (BIAS), e4m3 at ldc = 2^22 + 64 bytes (GELU with y_scale)
    or the fp32 stream in place at 2^21 + 64 elements (RESID, 9.2 GB).  Large against dense, bit for bit, all rows; the dense
    launch against the budgets of tests/test_gpu_numerics.py (BIAS, RESID) and the e4m3 rounding bound of
    tests/test_gpu_fp8_mfma.py (GELU)."""
    N, K = 256, 512
    xq, xs, wp, ws, b, pre, S, g = f8_reference(M, N, K)
    t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(DEV)
    xd, xsd, wd, wsd, bd = t(xq), t(xs), t(wp), t(ws), t(b)
    ysd = rd = gd = None
    if epi == nat.EPI_BIAS_GELU:
        h = orc.gelu(pre)
        ys = (np.abs(h).max(axis=1) * np.random.default_rng(5).uniform(1.0, 8.0, size=M) / 448.0).astype(F32)
        ysd = t(ys)
        ydt, far = torch.uint8, LD8
    elif epi == nat.EPI_BIAS_RESID:
        r, gam, _ = nm.resid_operands(1, M, M, N, "bf16", "fp32")
        rd, gd = dev(r.reshape(M, N), "fp32"), dev(gam, "fp32")
        ydt, far = torch.float32, LD
    else:
        ydt, far = torch.bfloat16, LD
    got = {}
    for layout in ("large", "dense"):
        xv = rows_at(big, xd, LD8 if layout == "large" else None)
        yv = out_at(big, M, N, far if layout == "large" else None, ydt)
        if rd is not None:
            yv.copy_(rd)
        with forced("rajni_debug_force_f8_tiling", f8_tiling):
            linear_call(xv, wd, N, bd, epi, yv, nat.RAJNI_BF16, gamma=gd, resid=yv if rd is not None else None,
                        stream_f32=int(rd is not None), w_scale=wsd, x_scale=xsd, y_scale=ysd)
        got[layout] = yv.contiguous()
    bm.assert_crosses_all((M - 1) * LD8 + K, 1, "e4m3 x")
    what = f"fp8 x fp8 linear {EPI_IDS[epi]} tiling {f8_tiling}"
    bm.assert_bit_equal(got["large"], got["dense"], what + ": large strides vs dense")
    if epi == nat.EPI_BIAS_GELU:
        deq = got["dense"].cpu().view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64) * ys[:, None].astype(np.float64)
        bound = np.maximum(np.abs(h) * 2.0 ** -4, ys[:, None] * 2.0 ** -10) * 1.01 + 2e-4 * np.abs(h).max()
        nm.assert_within(deq, h, bound, what)
    elif epi == nat.EPI_BIAS:
        nm.assert_within(host(got["dense"]), pre, nm.budget_bias(pre, S, g, "bf16"), what)
    else:
        want, bud = nm.budget_resid(pre, S, g, r.reshape(M, N).astype(np.float64), gam.astype(np.float64), "fp32")
        nm.assert_within(host(got["dense"]), want, bud, what)


# ---- gathered residual rows -------------------------------------------------------------------------------------
G_NP, G_B, G_NSRC, G_TAIL = 100, 11, 770_000, 1000      # M = 1100; resid [11, 770000, 256] fp32 = 8.67 GB, dense


@pytest.mark.parametrize("tiling", [0, 5, 4, 1], ids=["auto", "mid256x128", "wide256x256", "small128x128"])
def test_linear_gathered_residual_rows_past_2_31_elements(big, tiling):
    """proj with gathered residual rows (r_idx, r_np = 100, M = 1100): resid [11, 770000, 256] fp32, ldr = 256, the kept rows in
    the last 1000 tokens of every image, so resid_rows x ldr = 2.17e9 >= 2^31 while M x ldc is small.  First gathered row past
    2^31 elements: the kept rows of image 10 (8.67e9 bytes from the base); those of every image from 5 on lie past 2^32 bytes.  The 256 x 128
    tiling's 32-bit residual offsets do not reach there: by shape and under the forced hook the host must take 128 x 128.
    Against the same launch on the compacted rows [11, 1000, 256] (indices shifted), bit for bit; that one against fp64."""
    N, K = 256, 512
    x, w, b, pre, S, g, _, _ = lin_reference(N, K, "bf16", False)
    rng = np.random.default_rng(11)
    idx = np.stack([np.sort(rng.choice(G_TAIL, G_NP, replace=False)) for _ in range(G_B)]).astype(np.int32)     # within the tail
    r, gam, _ = nm.resid_operands(G_B, G_TAIL, G_NP, N, "bf16", "fp32")
    small = dev(r, "fp32")                                            # [11, 1000, 256]: the last 1000 tokens of each image
    full = big.dense((G_B, G_NSRC, N), torch.float32)
    assert G_B * G_NSRC * N >= bm.T31 > M_LIN * N
    full[:, G_NSRC - G_TAIL:].copy_(small)
    xd, bd, gd = dev(x, "bf16"), dev(b, "fp32"), dev(gam, "fp32")
    wd = ops.pack_weight(dev(w, "bf16"), torch.bfloat16)
    got = {}
    for layout, res, ix, nsrc in (("large", full, idx + (G_NSRC - G_TAIL), G_NSRC), ("dense", small, idx, G_TAIL)):
        yv = poison(torch.empty((M_LIN, N), dtype=torch.float32, device=DEV))
        with forced("rajni_debug_force_gemm_tiling", tiling):
            linear_call(xd, wd, N, bd, nat.EPI_BIAS_RESID, yv, nat.RAJNI_BF16, gamma=gd, resid=res,
                        r_idx=torch.from_numpy(ix).to(DEV), r_nsrc=nsrc, stream_f32=1)
        got[layout] = yv
    what = f"linear gathered residual, tiling {TILING_IDS[tiling]}"
    bm.assert_bit_equal(got["large"], got["dense"], what + ": rows past 2^31 elements vs compacted rows")
    r_used = orc.gather_rows(r, idx.astype(np.int64)).reshape(M_LIN, N).astype(np.float64)
    want, bud = nm.budget_resid(pre, S, g, r_used, gam.astype(np.float64), "fp32")
    nm.assert_within(host(got["dense"]), want, bud, what)


# ---------------------------------------------------------------------------------------------------------------
# dense row kernels: LayerNorm family, periodic rows
# ---------------------------------------------------------------------------------------------------------------
LN_ROWS, LN_C = 2_800_000, 768            # 2.15e9 elements: y (and x) cross 2^31 elements
assert LN_ROWS * LN_C > bm.T31


def ln_block(in_dt):
    return cached(("ln", in_dt), lambda: nm.layernorm_rows(P, LN_C, in_dt))


def layernorm_call(x, xs, w, b, y, rows, out_dt, x_f32):
    nat.check(lib().rajni_layernorm(x.data_ptr(), xs, w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, LN_C, EPS,
                                    nat.dtype_code(nm.TORCH[out_dt]), int(x_f32), stream()), "rajni_layernorm")


@pytest.mark.parametrize("in_dt,out_dt", [("bf16", "bf16"), ("fp16", "fp16"), ("fp32", "bf16"), ("fp32", "fp16"), ("fp32", "fp32")])
def test_layernorm_2_8m_rows(big, in_dt, out_dt):
    """rajni_layernorm over 2,800,000 x 768: x and y both hold 2.15e9 elements (bf16: 4.3 GB each, fp32: 8.6 GB).  fp32 in with
    a 16-bit out takes the two-rows-per-wave kernel, the others the one-row kernel.  Periodic input; EVERY output row r must be
    bit-equal to row r mod 4099 - row 2,796,203 is the first past 2^31 elements (2^32 bytes in bf16; in fp32 row 1,398,102 is
    the first past 2^32 bytes); rows 0..4098 against fp64."""
    x, names, w, b = ln_block(in_dt)
    xb = big.dense((LN_ROWS, LN_C), nm.TORCH[in_dt])
    bm.periodic_fill(xb, dev(x, in_dt))
    y = poison(big.dense((LN_ROWS, LN_C), nm.TORCH[out_dt]))
    layernorm_call(xb, LN_C, dev(w, "fp32"), dev(b, "fp32"), y, LN_ROWS, out_dt, in_dt == "fp32" and out_dt != "fp32")
    bm.assert_crosses_all(y.numel(), y.element_size(), "layernorm y")
    bm.assert_periodic(y, P, f"layernorm {in_dt}->{out_dt}")
    want, bud = nm.layernorm_budget(x, w, b, EPS, out_dt)
    nm.assert_within(host(y[:P]), want, bud, f"layernorm {in_dt}->{out_dt}, first period")


@pytest.mark.parametrize("in_dt", ["bf16", "fp32"])
def test_layernorm_fp8_2_8m_rows(big, in_dt):
    """rajni_layernorm_fp8 with hid_scale over 2,800,000 x 768: x crosses all three thresholds (bf16 4.3 GB / fp32 8.6 GB), the
    e4m3 output holds 2.15e9 bytes (past 2^31 elements and 2^31 bytes).  Periodic input: the e4m3 rows, y_scale and hid_scale of
    every row r are bit-equal to row r mod 4099 (first row past 2^31 elements: 2,796,203); of rows 0..4098, y_scale against the
    budget of tests/test_gpu_numerics.py::test_layernorm_fp8_row_scales, the dequantised e4m3 rows and hid_scale against fp64
    under the e4m3 rule of tests/test_gpu_fp8_mfma.py::test_layernorm_fp8_rule."""
    x, names, w, b = ln_block(in_dt)
    xb = big.dense((LN_ROWS, LN_C), nm.TORCH[in_dt])
    bm.periodic_fill(xb, dev(x, in_dt))
    q = poison(big.dense((LN_ROWS, LN_C), torch.uint8))
    sc, hs = poison(big.dense((LN_ROWS,), torch.float32)), poison(big.dense((LN_ROWS,), torch.float32))
    wd, bd = dev(w, "fp32"), dev(b, "fp32")
    nat.check(lib().rajni_layernorm_fp8(xb.data_ptr(), LN_C, wd.data_ptr(), bd.data_ptr(), q.data_ptr(), sc.data_ptr(),
                                        hs.data_ptr(), 3.0, 0.5, LN_ROWS, LN_C, EPS, int(in_dt == "fp32"), stream()),
              "rajni_layernorm_fp8")
    assert q.numel() > bm.T31
    for t, nmz in ((q, "e4m3 rows"), (sc, "y_scale"), (hs, "hid_scale")):
        bm.assert_periodic(t, P, f"layernorm_fp8 {in_dt}: {nmz}")
    want, bud = nm.layernorm_budget(x, w, b, EPS, "fp32")
    s_want = np.abs(want).max(axis=1) / 448.0
    tol = bud.max(axis=1) / 448.0 + 2 * nm.U32 * s_want
    s_dev = sc[:P].cpu().numpy().astype(np.float64)
    nm.assert_within(s_dev, s_want, tol, f"layernorm_fp8 {in_dt} scales, first period")
    # the e4m3 rows, dequantised with the device's own scale, under the rule of tests/test_gpu_fp8_mfma.py::
    # test_layernorm_fp8_rule (half an e4m3 ulp: 2^-4 relative, 2^-10 x scale below the normal range).  That test has benign rows;
    # these are the stress rows of nm.layernorm_rows, whose fp32 LayerNorm value may miss fp64 by the kernel's budget `bud`: the
    # rounding then starts from a value within bud of `want` and its half ulp grows by at most 2^-4 bud.
    deq = q[:P].cpu().view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64) * s_dev[:, None]
    bound = np.maximum(np.abs(want) * 2.0 ** -4, s_dev[:, None] * 2.0 ** -10) * 1.001 + 1e-6 * np.abs(want).max() + 1.0625 * bud
    nm.assert_within(deq, want, bound, f"layernorm_fp8 {in_dt} e4m3 rows, first period")
    # hid_scale = (1.0625 ||ln(x)[r]|| w1_rownorm_max + b1_absmax) / 448 with the constants passed above (3.0, 0.5): rtol 2e-5 as
    # in that test, plus the row norm's share of the same budget (| ||a|| - ||b|| | <= ||a - b||)
    hs_want = (1.0625 * np.sqrt((want ** 2).sum(axis=1)) * 3.0 + 0.5) / 448.0
    hs_tol = 2e-5 * hs_want + 1.0625 * 3.0 * np.sqrt((bud ** 2).sum(axis=1)) / 448.0
    nm.assert_within(hs[:P].cpu().numpy().astype(np.float64), hs_want, hs_tol, f"layernorm_fp8 {in_dt} hid_scale, first period")


@pytest.mark.parametrize("stream_dt,model_dt", [("fp32", "bf16"), ("bf16", "bf16")])
def test_layernorm_stream_in_place_2_8m_rows(big, stream_dt, model_dt):
    """rajni_layernorm_stream (norm_pre) in place on 2,800,000 x 768 rows of the residual stream (fp32: 8.6 GB, bf16: 4.3 GB).
    Periodic rows in, periodic rows out (first row past 2^31 elements: 2,796,203), rows 0..4098 against fp64."""
    x, names, w, b = ln_block(stream_dt)
    xb = big.dense((LN_ROWS, LN_C), nm.TORCH[stream_dt])
    bm.periodic_fill(xb, dev(x, stream_dt))
    ops.layernorm_stream(xb, dev(w, "fp32"), dev(b, "fp32"), EPS, model_dtype=nm.TORCH[model_dt])
    bm.assert_crosses_all(xb.numel(), xb.element_size(), "stream x")
    bm.assert_periodic(xb, P, f"layernorm_stream {stream_dt}")
    want, bud = nm.layernorm_budget(x, w, b, EPS, stream_dt)
    nm.assert_within(host(xb[:P]), want, bud, f"layernorm_stream {stream_dt}, first period")


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_layernorm_row_stride_2_23(big, dt):
    """x_row_stride: 300 rows 2^23 elements apart (the final norm reading CLS rows of long images; bf16 5.0 GB, fp32 10 GB, only
    the rows are touched).  Row 256 starts exactly 2^31 elements (bf16: 2^32 bytes) from the base, row 128 2^31 bytes (fp32: 2^32).
    Against the same rows dense, bit for bit; those against fp64."""
    rows, xs = 300, 1 << 23
    out_dt = "bf16"
    x, names, w, b = cached(("lnrs", dt), lambda: nm.layernorm_rows(rows, LN_C, dt))
    xd = dev(x, dt)
    xv = rows_at(big, xd, xs)
    bm.assert_crosses_all((rows - 1) * xs + LN_C, xv.element_size(), "strided x")
    wd, bd = dev(w, "fp32"), dev(b, "fp32")
    got = []
    for src in (xv, xd):
        y = poison(torch.empty((rows, LN_C), dtype=nm.TORCH[out_dt], device=DEV))
        layernorm_call(src, src.stride(0), wd, bd, y, rows, out_dt, dt == "fp32")
        got.append(y)
    bm.assert_bit_equal(got[0], got[1], f"layernorm {dt} rows at stride 2^23 vs dense")
    want, bud = nm.layernorm_budget(x, w, b, EPS, out_dt)
    nm.assert_within(host(got[1]), want, bud, f"layernorm {dt} dense rows")


# ---------------------------------------------------------------------------------------------------------------
# rajni_gather_rows
# ---------------------------------------------------------------------------------------------------------------

def test_gather_rows_src_and_dst_past_2_31_elements(big):
    """B = 16200, n_src = 197, n_dst = 173, E = 768 bf16: src holds 2.45e9 elements (4.90 GB), dst 2.152e9 (4.30 GB); both cross
    all three thresholds (at B = 16000 dst would end 1 % short of 2^31 elements).  Image 16163 of dst holds its 2^31-element boundary
    (2^32 bytes from the base), image 14193 of src.  Reference: torch.gather on the device, 256 images at a time, bit for
    bit over every image."""
    B, n_src, n_dst, E = 16200, 197, 173, 768
    rng = np.random.default_rng(3)
    block = nm.round_to(rng.standard_normal((P, E), dtype=F32), "bf16")
    src = big.dense((B, n_src, E), torch.bfloat16)
    bm.periodic_fill(src.view(B * n_src, E), dev(block, "bf16"))
    idx_small = np.stack([np.sort(rng.choice(n_src, n_dst, replace=False)) for _ in range(61)]).astype(np.int32)
    idx = torch.from_numpy(idx_small).to(DEV).repeat((B + 60) // 61, 1)[:B].contiguous()
    big.reserve(B * n_dst * E * 2)
    dst = ops.gather_rows(src, idx)
    bm.assert_crosses_all(src.numel(), 2, "gather src")
    bm.assert_crosses_all(dst.numel(), 2, "gather dst")
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for b0 in range(0, B, 256):
        b1 = min(B, b0 + 256)
        ix = idx[b0:b1].long()[:, :, None].expand(-1, -1, E)
        bad += (bm.bits(torch.gather(src[b0:b1], 1, ix)) != bm.bits(dst[b0:b1])).sum()
    assert int(bad) == 0, f"gather_rows: {int(bad)} elements differ from torch.gather"


# ---------------------------------------------------------------------------------------------------------------
# rajni_qk_norm
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 32])
def test_qk_norm_in_place_past_2_31_elements(big, D):
    """H = 1, bf16, in place on qkv [rows, 3 D] of 2.15e9 elements (4.3 GB): rows = 11,200,000 at D = 64 (one 128-byte line per
    group), 22,400,000 at D = 32 (the general form).  Periodic rows: after the call every row r - q, k and v thirds - is
    bit-equal to row r mod 4099 (first row past 2^31 elements: 11,184,811 / 22,369,622); of rows 0..4098 the q and k thirds
    against fp64, the v third bit-equal to the input."""
    rows = 11_200_000 * 64 // D
    qkv, qw, qb, kw, kb = cached(("qk", D), lambda: nv.qk_norm_case(P, 1, D, "bf16"))
    t = big.dense((rows, 3 * D), torch.bfloat16)
    block = dev(qkv, "bf16")
    bm.periodic_fill(t, block)
    bm.assert_crosses_all(t.numel(), 2, "qk_norm qkv")
    ops.qk_norm(t, 1, dev(qw, "fp32"), dev(qb, "fp32"), dev(kw, "fp32"), dev(kb, "fp32"), EPS)
    bm.assert_periodic(t, P, f"qk_norm D={D}")
    want, bud = nv.qk_norm_budget(qkv, 1, D, qw, qb, kw, kb, EPS, "bf16")
    nm.assert_within(host(t[:P, :2 * D]), want, bud, f"qk_norm D={D}, first period")
    bm.assert_bit_equal(t[:P, 2 * D:], block[:, 2 * D:], f"qk_norm D={D}: the v third")


# ---------------------------------------------------------------------------------------------------------------
# rajni_attention: qkv crossing through n_src
# ---------------------------------------------------------------------------------------------------------------
A_NSRC, A_TAIL, A_PAT = 16384, 5, 7       # tokens per image, images of the tail call, distinct images (b mod 7)


def attn_images(D):
    """smallest B whose last A_TAIL images all start at or past 2^31 elements of qkv [B, 16384, 3 D] (H = 1)"""
    return bm.first_row_past(A_NSRC * 3 * D, bm.T31) + A_TAIL


assert attn_images(64) == 688


def attn_setup(big, dt, D, n_p):
    """qkv [B, 16384, 3 D] (torch.empty) in which only the kept rows are written: image b keeps n_p rows of its last quarter
    (pattern b mod 7) holding the stress rows of nm.attention_qkv.  Returns qkv, keep_idx [B, n_p], the gathered rows
    [7, n_p, 3 D] (host) and B."""
    B = attn_images(D)
    rng = np.random.default_rng([D, n_p])
    kinds = ["peaked", "negative", "ramp", "cancel"]
    g = np.stack([nm.attention_qkv(kinds[i % len(kinds)], 1, n_p, 1, D, dt, seed=i)[0] for i in range(A_PAT)])     # [7, n_p, 3D]
    pat = np.stack([np.sort(rng.choice(A_NSRC // 4, n_p, replace=False)) + 3 * A_NSRC // 4 for _ in range(A_PAT)]).astype(np.int32)
    qkv = big.dense((B, A_NSRC, 3 * D), nm.TORCH[dt])
    bm.assert_crosses_all(qkv.numel(), qkv.element_size(), "attention qkv")
    assert (B - A_TAIL) * A_NSRC * 3 * D >= bm.T31
    reps = (B + A_PAT - 1) // A_PAT
    idx = torch.from_numpy(pat).to(DEV).repeat(reps, 1)[:B].contiguous()
    rows = (idx.long() + torch.arange(B, device=DEV)[:, None] * A_NSRC).reshape(-1)
    qkv.view(B * A_NSRC, 3 * D)[rows] = dev(g, dt).repeat(reps, 1, 1)[:B].reshape(B * n_p, 3 * D)
    return qkv, idx, g, B


def attn_check(out, tail_out, g, B, D, dt, what, budget=True):
    """the large call's last images == the call on those images alone; every image == its pattern's first image; the tail call
    within the fp64 budget"""
    bm.assert_bit_equal(out[B - A_TAIL:], tail_out, what + f": images {B - A_TAIL}.. of the batch vs alone")
    reps = (B + A_PAT - 1) // A_PAT
    bm.assert_bit_equal(out, out[:A_PAT].repeat(reps, *([1] * (out.dim() - 1)))[:B], what + ": image b vs image b mod 7")
    if budget:
        sel = [(B - A_TAIL + i) % A_PAT for i in range(A_TAIL)]
        want, bud = nm.attention_budget(g[sel], 1, D ** -0.5, dt)
        nm.assert_within(host(tail_out), want, bud, what)


ATTN_CASES = [("bf16", 64, 197, 0), ("bf16", 64, 300, 0), ("bf16", 64, 197, 1), ("bf16", 64, 197, 2), ("fp16", 64, 197, 0),
              ("fp16", 64, 300, 0), ("bf16", 32, 197, 0), ("bf16", 128, 197, 0), ("fp32", 64, 197, 0), ("fp32", 32, 197, 0)]


@pytest.mark.parametrize("dt,D,n_p,mode", ATTN_CASES, ids=[f"{dt}-D{D}-np{n}-mode{m}" for dt, D, n, m in ATTN_CASES])
def test_attention_rows_gathered_past_2_31_elements(big, dt, D, n_p, mode):
    """H = 1, n_src = 16384, keep_idx taking n_p rows from the last quarter of every image; B = 688 at D = 64 (bf16 qkv 4.3 GB,
    fp32 8.7 GB), 1371 at D = 32, 347 at D = 128, so that the last 5 images start past 2^31 elements of qkv (image 683 at
    D = 64: 4,297,064,448 bytes from the base in bf16, twice that in fp32).  n_p = 197: the persistent exact-softmax kernel
    (modes 1 / 2 force the online and the full-row kernels), n_p = 300: the online kernel, D = 32 / 128: the general kernel,
    fp32: the VALU kernels.  The last 5 images of the batch against a call on those 5 alone (tail slice), bit for bit; all images
    against their pattern; the tail call against fp64."""
    qkv, idx, g, B = attn_setup(big, dt, D, n_p)
    with forced("rajni_debug_force_attention", mode):
        out = ops.attention(qkv, idx, 1, D ** -0.5)
        tail = ops.attention(bm.tail_slice(qkv, B - A_TAIL), bm.tail_slice(idx, B - A_TAIL), 1, D ** -0.5)
    attn_check(out, tail, g, B, D, dt, f"attention {dt} D={D} np={n_p} mode {mode}")


def test_attention_fp8_rows_gathered_past_2_31_elements(big):
    """rajni_attention_fp8, n_p = 197, on the same bf16 qkv [688, 16384, 192]: e4m3 rows and row scales of the last 5 images
    (image 683 starts 4,297,064,448 bytes from the base) against a call on those 5 alone, bit for bit; the tail call against the
    bf16 kernel's output with the e4m3 bound of tests/test_gpu_numerics.py::test_attention_fp8_on_stress_logits."""
    D, n_p = 64, 197
    qkv, idx, g, B = attn_setup(big, "bf16", D, n_p)
    sel = [(B - A_TAIL + i) % A_PAT for i in range(A_TAIL)]
    want, _ = nm.attention_budget(g[sel], 1, 0.125, "bf16")
    scale = float(F32(np.abs(want).max() / 448.0))
    out, rs = ops.attention_fp8(qkv, idx, 1, 0.125, scale)
    tq, ti = bm.tail_slice(qkv, B - A_TAIL), bm.tail_slice(idx, B - A_TAIL)
    tail, trs = ops.attention_fp8(tq, ti, 1, 0.125, scale)
    attn_check(out, tail, g, B, D, "bf16", "attention_fp8", budget=False)
    assert bool((rs == F32(scale)).all()) and bool((trs == F32(scale)).all())
    deq = tail.cpu().view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64) * np.float64(F32(scale))
    ref = host(ops.attention(tq, ti, 1, 0.125))
    bound = np.maximum(np.abs(ref) * 2.0 ** -4, scale * 2.0 ** -10) * 1.001 + np.abs(ref) * 2.0 ** -8 + 1e-6 * np.abs(want).max()
    nm.assert_within(deq, ref, bound, "attention_fp8 tail")


def test_attention_output_past_2_31_elements(big):
    """ViT-B attention without pruning, H = 12, D = 64, B = 14195, n_src = n_p = 197, bf16: qkv 12.9 GB, out 2.1477e9 elements
    (4.3 GB) - 17.2 GB in all, 1.7 TFLOP.  Periodic images (7 distinct): every image b of `out` is bit-equal to image b mod 7
    (image 14193 holds the 2^31-element / 2^32-byte boundary of out; image 4732 the first past 2^31 elements
    of qkv); images 0..6 against fp64."""
    B, N, H, D = 14195, 197, 12, 64
    Cc = H * D
    g = np.stack([nm.attention_qkv(k, 1, N, H, D, "bf16", seed=i)[0]
                  for i, k in enumerate(["peaked", "negative", "ramp", "cancel", "uniform", "descending", "peaked"])])
    qkv = big.dense((B, N, 3 * Cc), torch.bfloat16)
    bm.periodic_fill(qkv.view(B, N * 3 * Cc), dev(g, "bf16").view(A_PAT, -1))
    big.reserve(B * N * Cc * 2)
    out = ops.attention(qkv, None, H, D ** -0.5)
    bm.assert_crosses_all(out.numel(), 2, "attention out")
    bm.assert_periodic(out.view(B, N * Cc), A_PAT, "attention out", periods_per_chunk=128)
    want, bud = nm.attention_budget(g, H, D ** -0.5, "bf16")
    nm.assert_within(host(out[:A_PAT]), want, bud, "attention H=12, first 7 images")


# ---------------------------------------------------------------------------------------------------------------
# rajni_importance / rajni_score_select / _prefix / _ws
# ---------------------------------------------------------------------------------------------------------------
S_TAIL = 4


def score_case(big, dt, B, N, num_prefix, period, two_pass=0):
    """qkv [B, N, 192] (H = 1, D = 64) filled with a block of `period` token rows repeated (period prime and no divisor of N:
    every image sees another phase); score + select on the whole batch and on its last S_TAIL images alone, and (once per
    dtype and path: the scores do not depend on num_prefix) rajni_importance on the whole batch against the fused scores"""
    with_importance = num_prefix == 1
    H, D = 1, 64
    block = cached(("score", dt, period),
                   lambda: nm.round_to(np.random.default_rng(period).standard_normal((period, 3 * D), dtype=F32), dt))
    qkv = big.dense((B, N, 3 * D), nm.TORCH[dt])
    bm.periodic_fill(qkv.view(B * N, 3 * D), dev(block, dt))
    bm.assert_crosses_all(qkv.numel(), qkv.element_size(), "score qkv")
    assert (B - S_TAIL) * N * 3 * D >= bm.T31
    keep = ops.keep_count(0.7, N, num_prefix)
    big.reserve(lib().rajni_score_select_workspace_bytes(B, N, H, D, nat.dtype_code(qkv.dtype)))
    tq = bm.tail_slice(qkv, B - S_TAIL)
    with forced("rajni_debug_force_score_two_pass", two_pass):
        scores, idx, nxt = ops.score_select(qkv, H, keep, num_prefix=num_prefix)
        ts, ti, tn = ops.score_select(tq, H, keep, num_prefix=num_prefix)
        imp = (ops.importance(qkv, H), ops.importance(tq, H)) if with_importance else None
    what = f"score_select {dt} B={B} N={N} prefix {num_prefix} two_pass {two_pass}"
    for a, b, nmz in ((scores, ts, "scores_out"), (idx, ti, "keep_idx"), (nxt, tn, "next_scores")):
        bm.assert_bit_equal(a[B - S_TAIL:], b, f"{what}: {nmz} of images {B - S_TAIL}.. of the batch vs alone")
    want, bud, e32 = nm.importance_budget(host(tq).astype(F32), H, dt)
    s = host(ts)
    nm.assert_within(s, want, bud, f"{what} (e32 {e32:.2g})")
    if imp is not None:
        bm.assert_bit_equal(imp[0][B - S_TAIL:], imp[1], f"{what}: rajni_importance of images {B - S_TAIL}.. of the batch vs alone")
        nm.assert_within(host(imp[1]), want, bud, f"{what}: rajni_importance (e32 {e32:.2g})")
    import numerics_prefix as npx
    sel = npx.select_tokens(s, keep, num_prefix)
    np.testing.assert_array_equal(ti.cpu().numpy(), sel, err_msg=what)
    assert np.array_equal(host(tn), np.take_along_axis(s, sel.astype(np.int64), axis=1)), what


@pytest.mark.parametrize("two_pass", [0, 1], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("dt,num_prefix", [("bf16", 1), ("bf16", 5), ("fp32", 1)])
def test_score_select_one_workgroup_images_past_2_31_elements(big, dt, num_prefix, two_pass):
    """the single-workgroup kernels (rajni_score_select / _prefix, rajni_importance): H = 1, D = 64, N = 577, B = 19400, qkv
    2.149e9 elements (bf16 4.3 GB, fp32 8.6 GB).  scores_out, keep_idx and next_scores of images 19396..19399 (image 19396 starts
    4,297,532,928 bytes from the base in bf16) against a call on those images alone, bit for bit; that call against fp64 and
    the selection rule.  With num_prefix = 1 (bf16 and fp32) rajni_importance is held to the same two checks."""
    score_case(big, dt, 19400, 577, num_prefix, P, two_pass)


@pytest.mark.parametrize("dt,num_prefix", [("bf16", 1), ("bf16", 5), ("fp32", 1), ("fp32", 5)])
def test_score_select_tiled_images_past_2_31_elements(big, dt, num_prefix):
    """the tiled kernels (rajni_score_select_ws; grid: 512 token tiles x B): H = 1, D = 64, N = 16384, B = 688, qkv 2.164e9
    elements (bf16 4.3 GB, fp32 8.7 GB) and 2.9 GB of scratch whose vbar region ([B][N][D] fp32) itself passes 2^31 bytes.
    Images 684..687 (image 684 starts 4,303,355,904 bytes from the base in bf16) against a call on those images alone, bit for
    bit; that call against fp64 and the selection rule.  With num_prefix = 1 rajni_importance (scores only, through the same
    scratch) is held to the same two checks."""
    score_case(big, dt, 688, 16384, num_prefix, 16411)


# ---------------------------------------------------------------------------------------------------------------
# rajni_pool_norm[_prefix]
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stream_dt,pool,num_prefix", [("bf16", "token", 1), ("bf16", "avg", 1), ("bf16", "avg", 5), ("fp32", "avg", 1),
                                                       ("fp32", "token", 1)])
def test_pool_norm_images_past_2_31_elements(big, stream_dt, pool, num_prefix):
    """x [14200, 197, 768] (bf16 4.3 GB, the fp32 stream 8.6 GB; 2.148e9 elements), norm and fc_norm on, bf16 out.  Periodic
    images (7 distinct): out row b is bit-equal to row b mod 7 for every b (image 14193 holds the 2^31-element
    boundary: it starts 4,294,688,256 bytes from the base in bf16); rows 0..6 against fp64 (num_prefix = 1; with 5 prefix tokens the mean
    runs over rows 5.., checked against the same budget on those rows)."""
    B, N, Cc = 14200, 197, 768
    x, (nw, nb), (fw, fb) = cached(("pool", stream_dt), lambda: nv.pool_case(A_PAT, N, Cc, stream_dt))
    xb = big.dense((B, N, Cc), nm.TORCH[stream_dt])
    bm.periodic_fill(xb.view(B, N * Cc), dev(x, stream_dt).view(A_PAT, -1))
    bm.assert_crosses_all(xb.numel(), xb.element_size(), "pool x")
    dn, df = (dev(nw, "fp32"), dev(nb, "fp32"), EPS), (dev(fw, "fp32"), dev(fb, "fp32"), 1e-5)
    y = ops.pool_norm(xb, pool, dn, df, out_dtype=torch.bfloat16, num_prefix=num_prefix)
    bm.assert_periodic(y, A_PAT, f"pool_norm {stream_dt} {pool} prefix {num_prefix}", periods_per_chunk=512)
    xr = x if (num_prefix == 1 or pool == "token") else np.concatenate([x[:, :1], x[:, num_prefix:]], axis=1)
    want, bud = nv.pool_norm_budget(xr, pool, (nw, nb, EPS), (fw, fb, 1e-5), "bf16")
    nm.assert_within(host(y[:A_PAT]), want, bud, f"pool_norm {stream_dt} {pool} prefix {num_prefix}, first 7 images")


# ---------------------------------------------------------------------------------------------------------------
# rajni_patch_embed[_prefix]
# ---------------------------------------------------------------------------------------------------------------

def bf16r(a):
    return nm.round_to(a, "bf16")


@pytest.mark.parametrize("patch,Cc,out_f32,regs", [(16, 64, False, 0), (16, 64, False, 4), (16, 768, True, 0), (14, 64, False, 0)],
                         ids=["fused-C64", "fused-C64-reg4", "fused-C768-f32stream", "im2col-p14-C64"])
def test_patch_embed_images_past_2_31_elements(big, patch, Cc, out_f32, regs):
    """images [14300, 3, 224, 224] bf16: 2.1525e9 elements, 4.3 GB.  Patch 16 reads them through the fused loader (C = 64: only
    the images cross; C = 768 into the fp32 stream: x [14300, 197, 768] fp32 is 8.65 GB and crosses too; 4 register tokens:
    rajni_patch_embed_prefix); patch 14 materialises the column matrix [14300 x 256, 640] bf16 (4.69 GB), which crosses as
    well.  Periodic images (7 distinct): every image b of x is bit-equal to image b mod 7 (image 14266 holds the 2^31-element
    boundary of the images: it starts 4,294,864,896 bytes from the base); images 0..6 against the fp64 reference at the tolerance
    of tests/test_gpu_kernels.py::test_patch_embed."""
    B, S = 14300, 224
    rng = np.random.default_rng(patch + Cc)
    img = bf16r(rng.standard_normal((A_PAT, 3, S, S), dtype=F32))
    w = bf16r(rng.standard_normal((Cc, 3, patch, patch), dtype=F32) * 0.05)
    b = bf16r(rng.standard_normal(Cc, dtype=F32) * 0.1)
    cls = bf16r(rng.standard_normal(Cc, dtype=F32))
    reg = bf16r(rng.standard_normal((regs, Cc), dtype=F32)) if regs else None
    npatch, Pn = (S // patch) ** 2, 1 + regs
    pos = bf16r(rng.standard_normal((npatch + Pn, Cc), dtype=F32))
    images = big.dense((B, 3, S, S), torch.bfloat16)
    bm.periodic_fill(images.view(B, -1), dev(img, "bf16").view(A_PAT, -1))
    bm.assert_crosses_all(images.numel(), 2, "images")
    big.reserve(B * (npatch + Pn) * Cc * (4 if out_f32 else 2))
    big.reserve(lib().rajni_patch_embed_workspace_bytes(B, 3, S, patch, nat.RAJNI_BF16))
    x = ops.patch_embed(images, ops.pack_weight(dev(w, "bf16"), k_multiple=64), dev(b, "fp32"), dev(cls, "bf16"), dev(pos, "bf16"),
                        True, patch, Cc, out_f32=out_f32, reg=dev(reg, "bf16") if regs else None)
    if out_f32 and Cc == 768:
        bm.assert_crosses_all(x.numel(), 4, "x")
    bm.assert_periodic(x.view(B, -1), A_PAT, f"patch_embed p{patch} C={Cc}", periods_per_chunk=128)
    tok = orc.patch_embed(img.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
    prefix = [np.broadcast_to(cls, (A_PAT, 1, Cc))] + ([np.broadcast_to(reg, (A_PAT, regs, Cc))] if regs else [])
    want = np.concatenate(prefix + [tok], axis=1) + pos[None]
    got = host(x[:A_PAT])
    rel = 1e-5 if out_f32 else 1e-2
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    assert err <= rel * scale, f"patch embed p{patch} C={Cc}: max err {err:.4g} vs scale {scale:.4g}"


# ---------------------------------------------------------------------------------------------------------------
# one whole forward
# ---------------------------------------------------------------------------------------------------------------
def forward_case(big, cfg_name, B, period, weight_format):
    """`period` distinct images repeated to a batch of B; schedule: one `update` stage, one carried stage.  Logits and every
    stage's keep_idx of image b must be bit-equal to those of image b mod period in a forward of the `period` images alone
    (bit-identity of sub-batches is the project's invariant, tests/test_gpu_forward.py); token_counts the same."""
    import rajni_amd
    from rajni_amd import timm_shaped as ts
    cfg = ts.CONFIGS[cfg_name]
    S = cfg.img_size
    n0 = (S // cfg.patch_size) ** 2 + 1
    hidden = int(cfg.embed_dim * cfg.mlp_ratio)
    assert (B - 5) * n0 * hidden >= bm.T31          # the hidden rows of the last 5 images and more lie past 2^31 elements
    sched = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
    model = ts.create_model(cfg, seed=0, std=0.08, bias_std=0.02, round_bf16=True)
    wrapped = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(torch.bfloat16).eval()
    wrapped.set_weight_format(weight_format)
    small = dev(np.random.default_rng(0).standard_normal((period, 3, S, S), dtype=F32), "bf16")
    ref_logits = wrapped(small).clone()
    ref_counts = list(wrapped.get_last_stats()["token_counts"])
    ref_keep = {i: t["keep_idx"].clone() for i, t in wrapped.get_last_trace().items()}
    assert sorted(ref_keep) == [1, 2]

    images = big.dense((B, 3, S, S), torch.bfloat16)
    bm.periodic_fill(images.view(B, -1), small.view(period, -1))
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, B, 3, S, cfg.patch_size
    p.C, p.H, p.D, p.hidden = cfg.embed_dim, cfg.num_heads, cfg.embed_dim // cfg.num_heads, hidden
    p.act_fp8 = int(weight_format == "fp8_mfma")
    ws_bytes = lib().rajni_vit_workspace_bytes(C.byref(p))
    assert ws_bytes > 4 * bm.GIB
    big.reserve(ws_bytes)
    try:
        logits = wrapped(images)
        counts = list(wrapped.get_last_stats()["token_counts"])
        keep = {i: t["keep_idx"] for i, t in wrapped.get_last_trace().items()}
        reps = (B + period - 1) // period
        what = f"{cfg_name} {weight_format} B={B}"
        assert counts == ref_counts
        bm.assert_bit_equal(logits.contiguous(), ref_logits.repeat(reps, 1)[:B].contiguous(),
                            f"{what}: logits of image b vs image b mod {period} alone")
        for i in (1, 2):
            bm.assert_bit_equal(keep[i], ref_keep[i].repeat(reps, 1)[:B], f"{what}: keep_idx of stage {i}, image b vs image b mod {period} alone")
    finally:
        wrapped._drop_plans()      # the workspace goes back before the fixture empties the cache


@pytest.mark.parametrize("weight_format", ["model", "fp8_mfma"])
def test_whole_forward_with_a_hidden_buffer_past_2_31_elements(big, weight_format):
    """vit_micro512_patch16_64, the smallest config of timm_shaped.CONFIGS that gets there (17 tokens, C = 512, hidden 2048,
    depth 4; the C = 128 ones with 17 tokens reach 5.7e8 hidden elements at the 65535 images one forward takes), bf16 with the
    fp32 residual stream, B = 61690: the workspace is 14 GB, its hidden region [B x 17, 2048] holds 2.1478e9 bf16 elements (past
    2^31 elements and 2^32 bytes; the rows of image 61681, the first past 2^31 elements, start 4,294,971,392 bytes into it), qkv and
    both stream buffers pass 2^31 bytes, and every region after the first starts more than 2^31 bytes into the workspace.
    "model": bf16 weights.  "fp8_mfma" (C % 256 == 0): e4m3 weights and e4m3 activations - norm1 / norm2 write e4m3 rows into
    the xn region and two row-scale vectors, fc1 requantises into the hidden region (2.1478e9 bytes there: past 2^31 bytes and
    elements), attention writes e4m3 rows, and the fp8 GEMMs chain through the workspace.  131 distinct images (1048 rows at
    the 8 tokens of the last stage: the small forward takes the stream GEMM tilings too) repeated; logits and both stages'
    keep_idx of every image against the forward of the 131 alone, bit for bit; token_counts the same."""
    forward_case(big, "vit_micro512_patch16_64", 61690, 131, weight_format)


def test_whole_forward_626_tokens_with_a_hidden_buffer_past_2_31_elements(big):
    """vit_micro_patch16_400 (626 tokens, C = 128, hidden 512, depth 4, bf16 with the fp32 residual stream), B = 6710: many
    tokens per image instead of many images, so attention takes the online kernel and the images cross too.  The workspace is
    15.1 GB, its hidden region [B x 626, 512] holds 2.1506e9 elements (past 2^31 elements and 2^32 bytes; image 6701 is the
    first whose hidden rows lie past 2^31 elements, 4,295,501,824 bytes into the region), qkv and both stream buffers pass 2^31
    bytes; with the images (6.4 GB, past 2^31 elements too) the test holds 21.6 GB.  fp8_mfma needs C % 256 == 0 and is not
    run at C = 128.  61 distinct images repeated; checks as above."""
    forward_case(big, "vit_micro_patch16_400", 6710, 61, "model")
