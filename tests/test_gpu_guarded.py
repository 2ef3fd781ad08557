"""Bounds and isolation of every C-ABI entry point, with poisoned inputs and guarded outputs (tests/guarded.py).
GPU box only (`-m gpu`).

Every output lives in a 0xFF-filled arena with a guard zone before and after it (and, where the ABI has a row stride, a
row gap): after each launch both guards and the gaps must be intact and every element must have been written.  Every
input holds its values in a view of such an arena; the memory the ABI says never enters a result (W rows >= N, the
lda gap, tails of vectors, unselected token rows, the non-CLS queries of importance) keeps the 0xFF pattern, which is
NaN in bf16, fp32 and e4m3, so a read of it that reaches a result fails the value comparison.  Index arrays are the
exception: their tails hold a valid index of a poisoned row, never -1.  Values are compared with a float64 reference at
the tolerances the other tests use for the same path.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rajni_amd
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import timm_shaped as ts, _native as nat

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def lib():
    return nat.lib()


def stream():
    return nat.stream_ptr()


def run(rc, what):
    nat.check(rc, what)
    torch.cuda.synchronize()


def ceil(a, b):
    return (a + b - 1) // b * b


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, g, scale=1.0, dtype=BF16):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def close(got, want, rel, what):
    got, want = got.double(), want.double()
    scale = float(want.abs().max().clamp_min(1e-30))
    err = float((got - want).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g})"


def guarded_input(t, row_stride=None, **kw):
    return Guarded(tuple(t.shape), t.dtype, DEV, row_stride=row_stride, **kw).fill_(t)


def out(shape, dtype, row_stride=None):
    return Guarded(shape, dtype, DEV, row_stride=row_stride)


def index_input(idx, fill):
    """int32 index array whose arena (tail included) holds `fill`: a valid index of a poisoned row"""
    return Guarded(tuple(idx.shape), torch.int32, DEV, fill_int32=fill).fill_(idx.to(torch.int32))


def random_selection(B, n_src, n_keep, g, unselected):
    """[B, n_keep]: slot 0 = CLS (0), the rest ascending, never `unselected`"""
    rows = []
    for _ in range(B):
        cand = torch.tensor([r for r in range(1, n_src) if r != unselected], device=DEV)
        perm = torch.randperm(cand.numel(), generator=g, device=DEV)[: n_keep - 1]
        rows.append(torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), cand[perm].sort().values]))
    return torch.stack(rows)


def e4m3_to_f64(q):
    return q.view(torch.float8_e4m3fn).to(torch.float32).double()


def random_e4m3(shape, g):
    """uniform random e4m3 codes without the two NaN patterns (0x7F, 0xFF)"""
    b = torch.randint(0, 256, shape, generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    b[(b & 0x7F) == 0x7F] = 0x38
    return b


# ---------------------------------------------------------------------------------------------
# rajni_linear
# ---------------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1, 4, 5], ids=["auto", "small128x128", "wide256x256", "mid256x128"])
def tiling(request):
    lib().rajni_debug_force_gemm_tiling(request.param)
    yield request.param
    lib().rajni_debug_force_gemm_tiling(0)


@pytest.fixture(params=[1, 2], ids=["f8_256x128", "f8_256x256"])
def f8_tiling(request):
    lib().rajni_debug_force_f8_tiling(request.param)
    yield request.param
    lib().rajni_debug_force_f8_tiling(0)


# (M, N, K): M ragged around 128 / 256 row tiles, N not a multiple of 128 (10: not even of 8, like a 10-class head)
LIN_SHAPES = [(1, 200, 128), (127, 8, 64), (129, 320, 256), (255, 1000, 192), (257, 10, 256), (1025, 320, 256),
              (2900, 1000, 256)]
RESID_SHAPES = [(129, 200, 192), (1025, 320, 256)]


class Resid:
    """the residual operand of a RESID launch: 'plain' (row m), 'gathered' (rows through r_idx; the unselected rows of
    every image are poisoned, the r_idx tail points at one of them) or 'inplace' (y is the residual tensor)"""

    def __init__(self, mode, M, N, dtype, ldr, g):
        self.mode = mode
        if mode == "gathered":
            r_np = 37 if M >= 37 else M
            while M % r_np:
                r_np -= 1
            B, nsrc = M // r_np, r_np + 5
            unsel = nsrc - 1
            idx = random_selection(B, nsrc, r_np, g, unsel)
            full = randn((B, nsrc, N), g, dtype=dtype)
            self.g = Guarded((B, nsrc, N), dtype, DEV, row_stride=ldr, after_rows=(256 // r_np + 2) * nsrc + 256)
            sel = (idx + torch.arange(B, device=DEV)[:, None] * nsrc).reshape(-1)
            self.g.t.view(-1, N)[sel] = full.view(-1, N)[sel]
            self.idx = index_input(idx.reshape(-1), unsel)
            self.r_np, self.r_nsrc = r_np, nsrc
            self.rows = full.view(-1, N)[sel]
        else:
            self.rows = randn((M, N), g, dtype=dtype)
            self.g = guarded_input(self.rows, row_stride=ldr)
            self.idx, self.r_np, self.r_nsrc = None, 0, 0
        self.ldr = ldr

    def fill_args(self, a):
        a.resid, a.ldr = self.g.ptr(), self.ldr
        if self.idx is not None:
            a.r_idx, a.r_np, a.r_nsrc = self.idx.ptr(), self.r_np, self.r_nsrc


def _args(x, lda, w, ldw, M, N, K, epi, dtype, y, ldc, bias, gamma=None, w_scale=None, x_scale=None, y_scale=None):
    a = nat.LinearArgs()
    a.x, a.lda, a.w, a.ldw = x.ptr(), lda, w.ptr(), ldw
    a.bias = bias.ptr() if bias is not None else None
    a.gamma = gamma.ptr() if gamma is not None else None
    a.w_scale = w_scale.ptr() if w_scale is not None else None
    a.x_scale = x_scale.ptr() if x_scale is not None else None
    a.y_scale = y_scale.ptr() if y_scale is not None else None
    a.y, a.ldc = y.ptr(), ldc
    a.M, a.N, a.K, a.epilogue, a.dtype = M, N, K, epi, dtype
    return a


def _weights(kind, N, K, g, wscale=0.05):
    """(guarded packed W with poisoned rows N..ceil256(N), guarded w_scale or None, float64 W the kernel multiplies by)"""
    npad = ceil(N, 256)
    if kind == "fp8":
        q = random_e4m3((N, K), g)
        s = (torch.rand(N, generator=g, device=DEV) * 1.5 + 0.5) * (wscale / 12.8)
        wg = Guarded((npad, K), torch.uint8, DEV)
        wg.t[:N] = q
        return wg, guarded_input(s), e4m3_to_f64(q) * s.double()[:, None]
    dt = F32 if kind == "f32" else BF16
    w = randn((N, K), g, wscale, dt)
    wg = Guarded((npad, K), dt, DEV)
    wg.t[:N] = w
    return wg, None, w.double()


def _epi_ref(lin, epi, gamma=None, resid=None):
    if epi == nat.EPI_BIAS_GELU:
        return 0.5 * lin * (1.0 + torch.special.erf(lin / np.sqrt(2.0)))
    if epi == nat.EPI_BIAS_RESID:
        return resid.double() + gamma.double() * lin
    return lin


def _linear_case(kind, M, N, K, epi, seed, resid_mode=None, stream_f32=False):
    """one rajni_linear launch: x with a poisoned lda gap and tail rows, W with poisoned rows N..ceil256(N), poisoned
    bias / gamma / w_scale tails; y (ldc > N) guarded and fully written"""
    g = gen(seed)
    dt = F32 if kind == "f32" else BF16
    lda, ldc, ldr = K + 64, ceil(N, 8) + 24, ceil(N, 8) + 8
    x = randn((M, K), g, dtype=dt)
    xg = guarded_input(x, row_stride=lda)
    wg, sg, w64 = _weights(kind, N, K, g, 0.1 if epi == nat.EPI_BIAS_RESID else 0.05)
    b = randn(N, g, 0.5, F32)
    bg = guarded_input(b)
    lin = x.double() @ w64.T + b.double()
    ydt = F32 if (stream_f32 or kind == "f32") else BF16
    gam = gg = res = None
    if epi == nat.EPI_BIAS_RESID:
        gam = randn(N, g, 1.0, F32)
        gg = guarded_input(gam)
        res = Resid(resid_mode, M, N, ydt, ldc if resid_mode == "inplace" else ldr, g)
    yg = res.g if res is not None and res.mode == "inplace" else out((M, N), ydt, row_stride=ldc)
    a = _args(xg, lda, wg, K, M, N, K, epi, nat.dtype_code(dt), yg, ldc, bg, gamma=gg, w_scale=sg)
    if res is not None:
        res.fill_args(a)
        a.stream_f32 = int(stream_f32 and kind != "f32")
    want = _epi_ref(lin, epi, gam, res.rows if res is not None else None)
    run(lib().rajni_linear(C.byref(a), stream()), "rajni_linear")
    what = f"linear {kind} {M}x{N}x{K} epi {epi} resid {resid_mode} f32stream {stream_f32}"
    for gd, nm in ((xg, "x"), (wg, "w"), (bg, "bias"), (gg, "gamma"), (sg, "w_scale")):
        if gd is not None:
            gd.check(f"{what}: input {nm}", written=False)
    if res is not None and res.mode != "inplace":
        res.g.check(f"{what}: input resid", written=False)
    yg.check(f"{what}: y")
    if kind == "f32":
        rel = 2e-6 if epi == nat.EPI_BIAS_RESID else 6e-6
    else:
        rel = 1e-5 if (epi == nat.EPI_BIAS_RESID and stream_f32) else 1e-2
    close(yg.t, want, rel, what)


@pytest.mark.parametrize("M,N,K", LIN_SHAPES)
@pytest.mark.parametrize("epi", [nat.EPI_BIAS, nat.EPI_BIAS_GELU], ids=["bias", "gelu"])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_linear_bias_gelu_guarded(kind, epi, M, N, K, tiling):
    _linear_case(kind, M, N, K, epi, seed=M + N + K + epi)


@pytest.mark.parametrize("M,N,K", RESID_SHAPES)
@pytest.mark.parametrize("mode", ["plain", "gathered", "inplace"])
@pytest.mark.parametrize("stream_f32", [False, True], ids=["bf16stream", "f32stream"])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_linear_resid_guarded(kind, stream_f32, mode, M, N, K, tiling):
    _linear_case(kind, M, N, K, nat.EPI_BIAS_RESID, seed=M + N + 3, resid_mode=mode, stream_f32=stream_f32)


@pytest.mark.parametrize("M,N,K", [(1, 200, 128), (255, 1000, 192), (257, 10, 256), (1025, 320, 64)])
@pytest.mark.parametrize("epi,mode", [(nat.EPI_BIAS, None), (nat.EPI_BIAS_GELU, None), (nat.EPI_BIAS_RESID, "plain"),
                                      (nat.EPI_BIAS_RESID, "gathered"), (nat.EPI_BIAS_RESID, "inplace")],
                         ids=["bias", "gelu", "resid", "resid_gathered", "resid_inplace"])
def test_linear_f32_guarded(epi, mode, M, N, K):
    _linear_case("f32", M, N, K, epi, seed=M * 3 + N + epi, resid_mode=mode)


def _f8f8_case(M, N, K, epi, seed, resid_mode=None, stream_f32=False):
    """fp8 x fp8 (x_scale): e4m3 x with a poisoned lda gap and tail rows, poisoned x_scale / y_scale / w_scale tails"""
    g = gen(seed)
    lda = K + 64
    xq = random_e4m3((M, K), g)
    xs = (torch.rand(M, generator=g, device=DEV) * 1.5 + 0.5) / 64.0
    xg, xsg = guarded_input(xq, row_stride=lda), guarded_input(xs)
    wq = random_e4m3((N, K), g)
    ws = (torch.rand(N, generator=g, device=DEV) * 1.5 + 0.5) / 64.0
    wg = Guarded((ceil(N, 256), K), torch.uint8, DEV)
    wg.t[:N] = wq
    wsg = guarded_input(ws)
    b = randn(N, g, 1.0, F32)
    bg = guarded_input(b)
    pre = (e4m3_to_f64(xq) * xs.double()[:, None]) @ (e4m3_to_f64(wq) * ws.double()[:, None]).T + b.double()
    what = f"f8xf8 linear {M}x{N}x{K} epi {epi} resid {resid_mode} f32stream {stream_f32}"
    ysg = gg = res = None
    if epi == nat.EPI_BIAS_GELU:
        h = _epi_ref(pre, epi)
        ys = (h.abs().amax(dim=1) * (1.0 + 7.0 * torch.rand(M, generator=g, device=DEV, dtype=torch.float64)) / 448.0).float()
        ysg = guarded_input(ys)
        ldc = ceil(N, 16) + 16
        yg = out((M, N), torch.uint8, row_stride=ldc)
    elif epi == nat.EPI_BIAS_RESID:
        ydt = F32 if stream_f32 else BF16
        ldc = ceil(N, 8) + 24
        gam = randn(N, g, 1.0, F32)
        gg = guarded_input(gam)
        res = Resid(resid_mode, M, N, ydt, ldc if resid_mode == "inplace" else ceil(N, 8) + 8, g)
        yg = res.g if resid_mode == "inplace" else out((M, N), ydt, row_stride=ldc)
        want = _epi_ref(pre, epi, gam, res.rows)
    else:
        ldc = ceil(N, 8) + 24
        yg = out((M, N), BF16, row_stride=ldc)
        want = pre
    a = _args(xg, lda, wg, K, M, N, K, epi, nat.RAJNI_BF16, yg, ldc, bg, gamma=gg, w_scale=wsg, x_scale=xsg, y_scale=ysg)
    if res is not None:
        res.fill_args(a)
        a.stream_f32 = int(stream_f32)
    run(lib().rajni_linear(C.byref(a), stream()), "rajni_linear")
    for gd, nm in ((xg, "x"), (xsg, "x_scale"), (wg, "w"), (wsg, "w_scale"), (bg, "bias"), (gg, "gamma"), (ysg, "y_scale")):
        if gd is not None:
            gd.check(f"{what}: input {nm}", written=False)
    yg.check(f"{what}: y")
    if epi == nat.EPI_BIAS_GELU:
        deq = e4m3_to_f64(yg.t) * ys.double()[:, None]
        bound = torch.maximum(h.abs() * 2.0 ** -4, ys.double()[:, None] * 2.0 ** -10) * 1.01 + 2e-4 * h.abs().max()
        assert bool(((deq - h).abs() <= bound).all()), f"{what}: e4m3 output outside the rounding bound"
    elif epi == nat.EPI_BIAS:
        err = float((yg.t.double() - want).abs().max())
        assert err <= 2.0 ** -8 * float(want.abs().max()) + 1e-3, f"{what}: max err {err:.4g}"
    else:
        close(yg.t, want, 1e-4 if stream_f32 else 1e-2, what)


@pytest.mark.parametrize("M,N,K", [(1, 200, 512), (255, 1000, 512), (257, 320, 768), (1025, 200, 512)])
@pytest.mark.parametrize("epi", [nat.EPI_BIAS, nat.EPI_BIAS_GELU], ids=["bias", "gelu_e4m3"])
def test_linear_f8f8_bias_gelu_guarded(epi, M, N, K, f8_tiling):
    _f8f8_case(M, N, K, epi, seed=M + N + K + 7 * epi)


@pytest.mark.parametrize("mode", ["plain", "gathered", "inplace"])
@pytest.mark.parametrize("stream_f32", [False, True], ids=["bf16stream", "f32stream"])
@pytest.mark.parametrize("M,N,K", [(129, 200, 512), (1025, 768, 512)])
def test_linear_f8f8_resid_guarded(M, N, K, stream_f32, mode, f8_tiling):
    _f8f8_case(M, N, K, nat.EPI_BIAS_RESID, seed=M + N + 11, resid_mode=mode, stream_f32=stream_f32)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1, 2], ids=["persistent", "online_chunked", "full_row"])
def attn_mode(request):
    lib().rajni_debug_force_attention(request.param)
    yield request.param
    lib().rajni_debug_force_attention(0)


def _attn_inputs(B, n_p, H, D, gathered, dtype, seed):
    """qkv in a guarded arena: identity = every row valid (the arena tail poisoned); gathered = n_src > n_p rows of which
    the unselected ones are poisoned in full, keep_idx's arena tail holds one of them"""
    g = gen(seed)
    Cc = H * D
    if not gathered:
        qkv = randn((B, n_p, 3 * Cc), g, dtype=dtype)
        return guarded_input(qkv), None, qkv, n_p
    n_src = n_p + max(2, n_p // 4)
    unsel = n_src - 1
    idx = random_selection(B, n_src, n_p, g, unsel)
    full = randn((B, n_src, 3 * Cc), g, dtype=dtype)
    qg = Guarded((B, n_src, 3 * Cc), dtype, DEV)
    sel = (idx + torch.arange(B, device=DEV)[:, None] * n_src).reshape(-1)
    qg.t.view(-1, 3 * Cc)[sel] = full.view(-1, 3 * Cc)[sel]
    return qg, index_input(idx, unsel), full.view(-1, 3 * Cc)[sel].view(B, n_p, 3 * Cc), n_src


def _attn_ref(kept, H, D, scale):
    B, n_p, _ = kept.shape
    q, k, v = kept.double().view(B, n_p, 3, H, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, n_p, H * D)


ATTN_NP = [1, 2, 31, 32, 33, 64, 65, 129, 224, 256, 257, 404]


@pytest.mark.parametrize("n_p", ATTN_NP)
@pytest.mark.parametrize("gathered", [False, True], ids=["identity", "gathered"])
def test_attention_d64_guarded(n_p, gathered, attn_mode):
    """(mode 2 past 256 tokens takes the chunked kernel, like mode 1)"""
    B, H, D = (2, 3, 64) if n_p % 2 else (1, 2, 64)
    _attention_case(B, n_p, H, D, gathered, BF16, seed=n_p * 7 + gathered)


@pytest.mark.parametrize("D", [8, 40, 72, 128])
@pytest.mark.parametrize("n_p", [1, 33, 129, 257])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_attention_head_dims_guarded(D, n_p, dtype):
    _attention_case(2 if n_p < 200 else 1, n_p, 2, D, D in (8, 72), dtype, seed=D * 1000 + n_p)


@pytest.mark.parametrize("n_p", [2, 31, 65, 257])
@pytest.mark.parametrize("gathered", [False, True], ids=["identity", "gathered"])
def test_attention_f32_d64_guarded(n_p, gathered):
    _attention_case(2, n_p, 2, 64, gathered, F32, seed=n_p + 5 * gathered)


def _attention_case(B, n_p, H, D, gathered, dtype, seed):
    qg, ig, kept, n_src = _attn_inputs(B, n_p, H, D, gathered, dtype, seed)
    og = out((B, n_p, H * D), dtype)
    scale = D ** -0.5
    run(lib().rajni_attention(qg.ptr(), ig.ptr() if ig is not None else None, og.ptr(), B, n_src, n_p, H, D, scale,
                              nat.dtype_code(dtype), stream()), "rajni_attention")
    what = f"attention B={B} np={n_p} H={H} D={D} {dtype} gathered={gathered}"
    qg.check(f"{what}: qkv", written=False)
    og.check(f"{what}: out")
    rel = 1.5e-2 if dtype == BF16 else (5e-6 if D == 64 else 2e-5)
    close(og.t, _attn_ref(kept, H, D, scale), rel, what)


@pytest.mark.parametrize("n_p", [1, 31, 33, 65, 129, 224])
@pytest.mark.parametrize("gathered", [False, True], ids=["identity", "gathered"])
def test_attention_fp8_guarded(n_p, gathered):
    B, H, D = (2, 3, 64) if n_p % 2 else (1, 2, 64)
    qg, ig, kept, n_src = _attn_inputs(B, n_p, H, D, gathered, BF16, seed=n_p * 3 + gathered)
    want = _attn_ref(kept, H, D, D ** -0.5)
    out_scale = float(np.float32(float(want.abs().max()) / 448.0))
    og = out((B, n_p, H * D), torch.uint8)
    rg = out((B * n_p,), F32)
    run(lib().rajni_attention_fp8(qg.ptr(), ig.ptr() if ig is not None else None, og.ptr(), out_scale, rg.ptr(), B, n_src, n_p,
                                  H, D, D ** -0.5, stream()), "rajni_attention_fp8")
    what = f"attention_fp8 B={B} np={n_p} gathered={gathered}"
    qg.check(f"{what}: qkv", written=False)
    og.check(f"{what}: out_q")
    rg.check(f"{what}: row_scale")
    assert bool((rg.t == np.float32(out_scale)).all())
    deq = e4m3_to_f64(og.t) * float(np.float32(out_scale))
    assert float((deq - want).abs().max()) <= (2.0 ** -4 + 1.5e-2) * float(want.abs().max()), what


# ---------------------------------------------------------------------------------------------
# importance, selection
# ---------------------------------------------------------------------------------------------

def _keeps(N):
    return sorted({1, max(1, (N - 1) // 2), N - 1})


def _qkv_cls_query_only(B, N, H, D, dtype, seed):
    """qkv whose Q third is poisoned for tokens 1..N-1 (importance reads only the CLS query)"""
    g = gen(seed)
    qkv = randn((B, N, 3 * H * D), g, dtype=dtype)
    qg = guarded_input(qkv)
    qg.arena[qg.offset:qg.end].view(B, N, -1)[:, 1:, : H * D * qg.esize] = 0xFF
    return qg, qkv


@pytest.mark.parametrize("two_pass", [0, 1], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,N,H,D", [(3, 2, 2, 64), (2, 3, 2, 64), (2, 64, 3, 64), (2, 65, 2, 40), (2, 197, 4, 64),
                                     (1, 577, 16, 64)])
def test_score_select_guarded(B, N, H, D, dtype, two_pass):
    qg, qkv = _qkv_cls_query_only(B, N, H, D, dtype, seed=N * H + D)
    want = orc.importance_scores(qkv.float().cpu().numpy(), H)
    rel = 6e-3 if dtype == BF16 else 2e-5
    lib().rajni_debug_force_score_two_pass(two_pass)
    try:
        sg = out((B, N), dtype)
        run(lib().rajni_importance(qg.ptr(), sg.ptr(), B, N, H, D, 1e-6, nat.dtype_code(dtype), stream()), "rajni_importance")
        sg.check(f"importance N={N}: scores")
        if N > 2:   # two tokens: centred V norms are equal, z = rounding noise / eps - no value to compare, only bounds
            close(sg.t, torch.from_numpy(want).to(DEV), rel, f"importance N={N} H={H} D={D}")
        else:
            assert bool(torch.isfinite(sg.t).all())
        for keep in _keeps(N):
            what = f"score_select B={B} N={N} H={H} D={D} keep={keep} {dtype}"
            s2, ig, ng = out((B, N), dtype), out((B, keep + 1), torch.int32), out((B, keep + 1), dtype)
            run(lib().rajni_score_select(qg.ptr(), B, N, H, D, 1e-6, keep, s2.ptr(), ig.ptr(), ng.ptr(), nat.dtype_code(dtype),
                                         stream()), "rajni_score_select")
            for gd, nm in ((s2, "scores"), (ig, "keep_idx"), (ng, "next_scores")):
                gd.check(f"{what}: {nm}")
            assert torch.equal(s2.t, sg.t), what
            s = s2.t.float().cpu().numpy()
            sel = orc.select_tokens(s, keep)
            np.testing.assert_array_equal(ig.t.cpu().numpy(), sel, err_msg=what)
            assert np.array_equal(ng.t.float().cpu().numpy(), np.take_along_axis(s, sel, axis=1)), what
        qg.check("score_select: qkv", written=False)
    finally:
        lib().rajni_debug_force_score_two_pass(0)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N", [2, 3, 64, 65, 197, 577])
def test_select_topk_guarded(N, dtype):
    """scores in an arena whose tail is NaN: NaN ranks as +inf, so a read past row B-1's last score changes the pick"""
    B = 3
    g = gen(N)
    s = randn((B, N), g, dtype=dtype)
    s[1, :: 3] = s[1, 0].clone()                      # runs of ties
    sg = guarded_input(s)
    for keep in _keeps(N):
        what = f"select_topk N={N} keep={keep} {dtype}"
        ig, ng = out((B, keep + 1), torch.int32), out((B, keep + 1), dtype)
        run(lib().rajni_select_topk(sg.ptr(), B, N, keep, ig.ptr(), ng.ptr(), nat.dtype_code(dtype), stream()), "rajni_select_topk")
        ig.check(f"{what}: keep_idx")
        ng.check(f"{what}: next_scores")
        sh = s.float().cpu().numpy()
        sel = orc.select_tokens(sh, keep)
        np.testing.assert_array_equal(ig.t.cpu().numpy(), sel, err_msg=what)
        assert np.array_equal(ng.t.float().cpu().numpy(), np.take_along_axis(sh, sel, axis=1)), what
    sg.check("select_topk: scores", written=False)


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------

def _ln_inputs(rows, Cc, xdt, stride, seed, cls_rows=0):
    """x rows `stride` apart (gap poisoned), or with cls_rows = N: rows CLS rows of [rows, N, C] with tokens 1.. poisoned;
    w, b in arenas with poisoned tails"""
    g = gen(seed)
    x = (torch.randn((rows, Cc), generator=g, device=DEV) * 2 + 0.5).to(xdt)
    if cls_rows:
        xg = Guarded((rows, cls_rows, Cc), xdt, DEV)
        xg.t[:, 0] = x
        stride = cls_rows * Cc
    else:
        xg = guarded_input(x, row_stride=stride)
    w = (1 + 0.1 * torch.randn(Cc, generator=g, device=DEV)).to(BF16).float()
    b = (0.1 * torch.randn(Cc, generator=g, device=DEV)).to(BF16).float()
    return xg, stride, guarded_input(w), guarded_input(b), x, w, b


def _ln_ref(x, w, b):
    x = x.double()
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * w.double() + b.double()


LN_C = [8, 64, 200, 768, 1024, 1032, 2048]


# rows_f32x: >= 4096 fp32 rows of C <= 1024, the two-rows-per-wave kernels
@pytest.mark.parametrize("kind,Cc", [(k, c) for k in ("bf16", "f32x_bf16y", "f32", "rows_f32x", "cls_rows") for c in LN_C
                                     if k != "rows_f32x" or c <= 1024])
def test_layernorm_guarded(kind, Cc):
    rows = 4100 if kind == "rows_f32x" else 37
    xdt = BF16 if kind in ("bf16", "cls_rows") else F32
    ydt = F32 if kind == "f32" else BF16
    xg, stride, wg, bg, x, w, b = _ln_inputs(rows, Cc, xdt, Cc + 24, seed=Cc + rows, cls_rows=5 if kind == "cls_rows" else 0)
    yg = out((rows, Cc), ydt)
    x_f32 = int(xdt == F32 and ydt != F32)
    run(lib().rajni_layernorm(xg.ptr(), stride, wg.ptr(), bg.ptr(), yg.ptr(), rows, Cc, 1e-6, nat.dtype_code(ydt), x_f32,
                              stream()), "rajni_layernorm")
    what = f"layernorm {kind} rows={rows} C={Cc}"
    for gd, nm in ((xg, "x"), (wg, "w"), (bg, "b")):
        gd.check(f"{what}: {nm}", written=False)
    yg.check(f"{what}: y")
    close(yg.t, _ln_ref(x, w, b), 3e-6 if ydt == F32 else 1e-2, what)


# C <= 1024 takes the two-chunk instantiations, wider rows the four-chunk ones
@pytest.mark.parametrize("kind,Cc", [(k, c) for k in ("bf16", "f32x", "rows_f32x", "cls_rows") for c in LN_C
                                     if k != "rows_f32x" or c <= 1024])
def test_layernorm_fp8_guarded(kind, Cc):
    rows = 4099 if kind == "rows_f32x" else 37
    xdt = F32 if kind in ("f32x", "rows_f32x") else BF16
    xg, stride, wg, bg, x, w, b = _ln_inputs(rows, Cc, xdt, Cc + 8, seed=Cc * 3 + rows, cls_rows=3 if kind == "cls_rows" else 0)
    qg, sg, hg = out((rows, Cc), torch.uint8), out((rows,), F32), out((rows,), F32)
    wn, bm = 0.61, 0.07
    run(lib().rajni_layernorm_fp8(xg.ptr(), stride, wg.ptr(), bg.ptr(), qg.ptr(), sg.ptr(), hg.ptr(), wn, bm, rows, Cc, 1e-6,
                                  int(xdt == F32), stream()), "rajni_layernorm_fp8")
    what = f"layernorm_fp8 {kind} rows={rows} C={Cc}"
    for gd, nm in ((xg, "x"), (wg, "w"), (bg, "b")):
        gd.check(f"{what}: {nm}", written=False)
    for gd, nm in ((qg, "y_q"), (sg, "y_scale"), (hg, "hid_scale")):
        gd.check(f"{what}: {nm}")
    o = _ln_ref(x, w, b)
    s_ref = o.abs().amax(dim=1) / 448.0
    s_dev = sg.t.double()
    assert bool(((s_dev - s_ref).abs() <= 2e-5 * s_ref).all()), what
    deq = e4m3_to_f64(qg.t) * s_dev[:, None]
    bound = torch.maximum(o.abs() * 2.0 ** -4, s_dev[:, None] * 2.0 ** -10) * 1.001 + 1e-6 * o.abs().max()
    assert bool(((deq - o).abs() <= bound).all()), what
    hs_ref = (1.0625 * o.norm(dim=1) * wn + bm) / 448.0
    assert bool(((hg.t.double() - hs_ref).abs() <= 2e-5 * hs_ref).all()), what


# ---------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [8, 16, 40, 768, 2304])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_gather_rows_guarded(E, dtype):
    """bit exact; unselected source rows poisoned, the idx tail points at one of them"""
    B, n_src, n_dst = 3, 41, 29
    g = gen(E)
    src = randn((B, n_src, E), g, dtype=dtype)
    unsel = n_src - 1
    idx = random_selection(B, n_src, n_dst, g, unsel)
    sg = Guarded((B, n_src, E), dtype, DEV)
    for bi in range(B):
        sg.t[bi, idx[bi]] = src[bi, idx[bi]]
    ig = index_input(idx, unsel)
    og = out((B, n_dst, E), dtype)
    run(lib().rajni_gather_rows(sg.ptr(), ig.ptr(), og.ptr(), B, n_src, n_dst, E, nat.dtype_code(dtype), stream()),
        "rajni_gather_rows")
    og.check(f"gather E={E} {dtype}: dst")
    sg.check(f"gather E={E} {dtype}: src", written=False)
    assert torch.equal(og.t, torch.gather(src, 1, idx[:, :, None].expand(-1, -1, E)))


# ---------------------------------------------------------------------------------------------
# patch embed
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bf16", "bf16_to_f32", "f32"])
@pytest.mark.parametrize("S,P,Cc,B,has_cls", [(32, 8, 64, 3, True), (64, 16, 128, 2, False), (96, 32, 192, 2, True),   # fused loader
                                              (28, 7, 64, 3, True), (70, 10, 64, 2, True), (56, 14, 128, 2, False)])  # columns
def test_patch_embed_guarded(S, P, Cc, B, has_cls, fmt):
    """weight rows >= C and the pos / cls / bias tails poisoned (the zero K-padding columns stay zero: the ABI requires
    them); the column workspace exactly rajni_patch_embed_workspace_bytes, prefilled with 0xFF and guarded - the kernel
    must write its zero K-padding itself"""
    g = gen(S * P + Cc)
    dt = F32 if fmt == "f32" else BF16
    Cin, K = 3, 3 * P * P
    kpad = ceil(K, 64)
    npatch = (S // P) ** 2
    img = randn((B, Cin, S, S), g, dtype=dt)
    w = randn((Cc, K), g, 0.05, dt)
    b = randn(Cc, g, 0.1, dt).float()
    cls = randn(Cc, g, dtype=dt)
    pos = randn((npatch + int(has_cls), Cc), g, dtype=dt)
    wg = Guarded((ceil(Cc, 256), kpad), dt, DEV)
    wg.t[:Cc] = 0
    wg.t[:Cc, :K] = w
    ig, bg, cg, pg = guarded_input(img), guarded_input(b), guarded_input(cls), guarded_input(pos)
    xdt = F32 if fmt != "bf16" else BF16
    xg = out((B, npatch + 1, Cc), xdt)
    nbytes = lib().rajni_patch_embed_workspace_bytes(B, Cin, S, P, nat.dtype_code(dt))
    fused = P >= 8 and P & (P - 1) == 0
    assert (nbytes == 0) == fused
    ws = out((B * npatch, kpad), dt) if nbytes else None
    assert ws is None or ws.region == nbytes
    run(lib().rajni_patch_embed(ig.ptr(), wg.ptr(), bg.ptr(), cg.ptr(), pg.ptr(), int(has_cls), xg.ptr(), int(fmt == "bf16_to_f32"),
                                B, Cin, S, P, Cc, nat.dtype_code(dt), ws.ptr() if ws is not None else None, nbytes, stream()),
        "rajni_patch_embed")
    what = f"patch embed S={S} P={P} C={Cc} {fmt}"
    for gd, nm in ((ig, "images"), (wg, "w"), (bg, "bias"), (cg, "cls"), (pg, "pos")):
        gd.check(f"{what}: {nm}", written=False)
    xg.check(f"{what}: x")
    if ws is not None:
        ws.check(f"{what}: workspace")
        assert bool((ws.t[:, K:] == 0).all()), f"{what}: K padding of the column matrix is not zero"
    cols = img.double().view(B, Cin, S // P, P, S // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, npatch, K)
    tok = cols @ w.double().T + b.double()
    cls_row = cls.double().view(1, 1, Cc).expand(B, 1, Cc)
    if has_cls:
        want = torch.cat([cls_row, tok], dim=1) + pos.double()[None]
    else:
        want = torch.cat([cls_row, tok + pos.double()[None]], dim=1)
    close(xg.t, want, {"bf16": 1e-2, "bf16_to_f32": 1e-5, "f32": 3e-6}[fmt], what)


# ---------------------------------------------------------------------------------------------
# the whole forward
# ---------------------------------------------------------------------------------------------

def _mlp200():
    return ts.ViTConfig(img_size=64, embed_dim=128, depth=3, num_heads=2, num_classes=10, mlp_ratio=200 / 128)


SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
LAST_PRUNES = {1: {"keep_ratio": 0.75, "update": True}, 3: {"keep_ratio": 0.5, "update": False}}

# (config, format, schedule, resid_bf16, cls_only_last_block)
FWD_CASES = [
    ("vit_micro_patch16_64", "bf16", SCHED, False, False),
    ("vit_micro_patch16_64", "bf16", SCHED, True, True),
    ("vit_micro_patch16_64", "bf16", LAST_PRUNES, False, True),
    ("vit_micro_patch16_64", "fp32", SCHED, False, True),
    ("vit_micro_patch16_64", "fp8", LAST_PRUNES, True, False),
    ("vit_micro_d80_patch16_64", "bf16", SCHED, False, True),
    ("vit_micro_d80_patch16_64", "fp32", LAST_PRUNES, False, False),
    ("vit_micro_patch14_56", "bf16", SCHED, True, False),
    ("vit_micro_patch14_56", "fp8", SCHED, False, True),
    ("deit3_micro_patch16_64", "bf16", SCHED, False, True),
    ("deit3_micro_patch16_64", "fp32", LAST_PRUNES, False, False),
    ("mlp200", "bf16", SCHED, False, True),
    ("mlp200", "fp8", LAST_PRUNES, False, False),
    ("vit_micro512_patch16_64", "fp8_mfma", SCHED, False, False),
    ("vit_micro512_patch16_64", "fp8_mfma", SCHED, True, True),
    ("vit_micro512_patch16_64", "fp8_mfma", LAST_PRUNES, False, True),
]


def _wrapped(cfg_name, fmt, sched, resid_bf16, cls_only):
    cfg = _mlp200() if cfg_name == "mlp200" else ts.CONFIGS[cfg_name]
    model = ts.create_model(cfg, seed=3, std=0.06, bias_std=0.02, round_bf16=True)
    dtype = F32 if fmt == "fp32" else BF16
    w = rajni_amd.RAJNIViTWrapper(model, sched).to(DEV).to(dtype).eval().trace_scores(True)
    if fmt in ("fp8", "fp8_mfma"):
        w.set_weight_format(fmt)
    if resid_bf16:
        w.set_residual_dtype(torch.bfloat16)
    w.set_last_block_cls_only(cls_only)
    return cfg, w, dtype


def _forward_guarded(w, images, ws_fill):
    """rajni_vit_forward on a copy of the wrapper's plan with a guarded workspace (exactly rajni_vit_workspace_bytes,
    prefilled with ws_fill), guarded logits (logits_ld >= ceil8(num_classes) + 8) and guarded per-stage buffers"""
    entry = w._plan
    plan0, bufs = entry[1], entry[3]
    plan = nat.VitPlan.from_buffer_copy(plan0)
    depth, B, ncls = plan.depth, plan.B, plan.num_classes
    blocks = (nat.Block * depth)(*[nat.Block.from_buffer_copy(plan0.blocks[i]) for i in range(depth)])
    plan.blocks = blocks
    tc = (C.c_int32 * depth)(*([-1] * depth))
    plan.token_counts = tc
    stages = {}
    dt = BF16 if plan.dtype == nat.RAJNI_BF16 else F32
    for i, kb in bufs.items():
        keep1 = kb["keep_idx"].shape[1]
        n = kb["scores"].shape[1]
        st = dict(keep_idx=out((B, keep1), torch.int32), next_scores=out((B, keep1), dt), scores=out((B, n), dt))
        blocks[i].keep_idx, blocks[i].next_scores, blocks[i].scores = (st["keep_idx"].ptr(), st["next_scores"].ptr(),
                                                                      st["scores"].ptr())
        stages[i] = st
    nbytes = lib().rajni_vit_workspace_bytes(C.byref(plan))
    assert nbytes == plan0.workspace_bytes
    ws = Guarded((nbytes,), torch.uint8, DEV)
    ws.t.fill_(ws_fill)
    plan.workspace, plan.workspace_bytes = ws.ptr(), nbytes
    ld = ceil(ncls, 8) + 8
    plan.logits_ld = ld
    lg = out((B, ncls), dt, row_stride=ld)
    run(lib().rajni_vit_forward(C.byref(plan), images.data_ptr(), lg.ptr(), stream()), "rajni_vit_forward")
    return lg, [int(tc[i]) for i in range(depth)], stages, ws


@pytest.mark.parametrize("cfg_name,fmt,sched,resid_bf16,cls_only", FWD_CASES,
                         ids=[f"{c[0]}-{c[1]}-{'lastprunes' if c[2] is LAST_PRUNES else 'sched'}"
                              f"{'-residbf16' if c[3] else ''}{'-clsonly' if c[4] else ''}" for c in FWD_CASES])
def test_forward_workspace_independence_and_bounds(cfg_name, fmt, sched, resid_bf16, cls_only):
    cfg, w, dtype = _wrapped(cfg_name, fmt, sched, resid_bf16, cls_only)
    images = torch.randn((3, 3, cfg.img_size, cfg.img_size), generator=gen(7), device=DEV).to(dtype)
    base = w(images)                                        # builds the plan (and is the wrapper's own answer)
    runs = [_forward_guarded(w, images, f) for f in (0x00, 0x00, 0xFF)]
    what = f"forward {cfg_name} {fmt}"
    for k, (lg, counts, stages, ws) in enumerate(runs):
        ws.check(f"{what} run {k}: workspace", written=False)
        lg.check(f"{what} run {k}: logits")
        assert counts == w.get_last_stats()["token_counts"], what
        for i, st in stages.items():
            recomputed = w.pruning_schedule[i]["update"] or (i - 1) not in w.pruning_schedule
            st["keep_idx"].check(f"{what} run {k} stage {i}: keep_idx")
            st["next_scores"].check(f"{what} run {k} stage {i}: next_scores")
            st["scores"].check(f"{what} run {k} stage {i}: scores", written=recomputed)
    a, b, c = runs

    def same(x, y, name):   # bitwise: the bytes of the views
        assert torch.equal(x.arena[x.offset:x.end], y.arena[y.offset:y.end]), f"{what}: {name} differ"

    for other, tag in ((b, "two runs with a zeroed workspace"), (c, "zeroed vs 0xFF workspace")):
        same(a[0], other[0], f"{tag}: logits")
        assert a[1] == other[1], f"{what}: {tag}: token counts"
        for i in a[2]:
            for nm in ("keep_idx", "next_scores", "scores"):
                same(a[2][i][nm], other[2][i][nm], f"{tag}: stage {i} {nm}")
    assert torch.equal(a[0].t, base), f"{what}: logits differ from the wrapper's own forward"
