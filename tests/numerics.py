"""Stress inputs and per-element error budgets for the numerics tests (tests/test_numerics_cpu.py checks the budgets
against CPU emulations and mutants, tests/test_gpu_numerics.py holds every HIP kernel to them).  Pure numpy / torch-CPU.

Every expected value is fp64 numpy on inputs ALREADY rounded to the kernel's input type; a budget bounds
|got - want| element by element, so a wrong small value cannot hide behind a large one elsewhere in the tensor.

Notation: u_out = unit roundoff of the output type, u32 = 2^-24; every budget has half the smallest subnormal of the
output type as an absolute floor (a correctly rounded result may sit that far from a value below the format's range).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import rajni_oracle as orc

U32 = 2.0 ** -24
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}
FLOOR = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25, "fp32": 2.0 ** -150}      # half the smallest subnormal
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
FP16_MIN_NORMAL = 2.0 ** -14


# shapes shared by tests/test_numerics_cpu.py (emulations) and tests/test_gpu_numerics.py (kernels)
GEMM_SHAPES = [(394, 2304, 768), (130, 3072, 768), (346, 768, 3072), (7, 1000, 768), (513, 260, 128), (1, 192, 192),
               (2100, 384, 64)]
ATTN_SHAPES = [(2, 197, 173, 12), (1, 577, 404, 16), (1, 130, 129, 1), (2, 40, 33, 2), (1, 300, 257, 2), (2, 256, 256, 2),
               (3, 17, 13, 2)]                                        # (B, N, Np, H), head dim 64
ATTN_DGEN_SHAPES = [(2, 197, 173, 3), (1, 300, 257, 2), (3, 17, 13, 2)]   # head dims 32 / 80 / 128 (the general kernels)
ATTN_F32_SHAPES = [(2, 70, 33, 2), (1, 45, 45, 3)]                     # fp32 path, head dims 64 and 80
IMP_SHAPES = [(4, 197, 12, 64), (2, 577, 16, 64), (3, 61, 4, 80), (2, 33, 2, 32)]
LN_C = [192, 768, 1024, 1280]
GELU_X0 = np.float32(4.24264069)        # 3 sqrt2: the upper clamp of the packed polynomial GELU's argument


def pick_rows(rng, B, N, Np):
    """kept-token indices [B, Np]: CLS first, then ascending (all rows when Np == N)"""
    if Np == N:
        return np.tile(np.arange(N), (B, 1))
    return np.stack([np.concatenate([[0], 1 + np.sort(rng.choice(N - 1, Np - 1, replace=False))]) for _ in range(B)])


def gelu_grid():
    """pre-activations of the GELU sweeps: 120001 points on [-8, 8], 20001 more on +-[4.2, 4.3] (dense around the clamp
    point), the clamp point and its fp32 neighbours, +-2^3 .. 2^13"""
    g = np.concatenate([np.linspace(-8, 8, 120001).astype(np.float32), np.linspace(4.2, 4.3, 20001).astype(np.float32),
                        [np.nextafter(GELU_X0, np.float32(0)), GELU_X0, np.nextafter(GELU_X0, np.float32(9))],
                        (2.0 ** np.arange(3, 14)).astype(np.float32)]).astype(np.float32)
    return np.concatenate([g, -g[g != 0]])


def round_to(a, dt: str) -> np.ndarray:
    """fp32 array holding `a` rounded (nearest even) to `dt`"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "fp32":
        return a
    if dt == "fp16":
        return a.astype(np.float16).astype(np.float32)
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def truncate_to(a, dt: str) -> np.ndarray:
    """`a` (fp32) rounded TOWARD ZERO to `dt` - the mutant of a round-to-nearest store (normal range)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "fp32":
        return a
    drop = 16 if dt == "bf16" else 13
    t = (a.view(np.uint32) >> drop << drop).view(np.float32)
    if dt == "fp16":
        t = np.where(np.abs(a) < FP16_MIN_NORMAL, a.astype(np.float16).astype(np.float32), t)
    return t


def _spread(rng, n, lo, hi):
    return (10.0 ** rng.uniform(lo, hi, size=n)).astype(np.float32)


def _noise(rng, shape, dt):
    """standard normal; for fp16 with |value| >= 2^-6 so that the scaled operand never is an fp16 subnormal"""
    n = rng.standard_normal(shape, dtype=np.float32)
    if dt == "fp16":
        n = np.where(np.abs(n) < 2.0 ** -6, np.copysign(np.float32(2.0 ** -6), n), n)
    return n


# ---------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------
# Row / column scale ranges (decades).  bf16 and fp32 share the fp32 exponent range: x rows 10^U(-3,3), W rows
# 0.05 * 10^U(-2,2), bias 10^U(-3,1).  fp16 (largest finite 65504, smallest normal 6.1e-5): x rows 10^U(-2,2), W rows
# 0.05 * 10^U(-1,1), bias 10^U(-3,1), residual rows 10^U(-2,2) and the noise floor of _noise: the smallest operand is
# 1e-2 * 2^-6 = 1.6e-4 (x) / 5e-3 * 2^-6 = 7.8e-5 (W), both normal, and |x W^T| stays near 100 * 0.5 * sqrt(K) * 5 < 1.6e4
# at K = 3072 (gemm_case asserts max |want| <= 6e4).
GEMM_RANGES = {"bf16": ((-3, 3), (-2, 2)), "fp32": ((-3, 3), (-2, 2)), "fp16": ((-2, 2), (-1, 1))}


def gemm_operands(M, N, K, dt, seed=0):
    """x [M,K], w [N,K] rounded to `dt`, bias fp32 [N] (rounded to `dt` too: what a model of that type holds)"""
    rng = np.random.default_rng([seed, M, N, K])
    (xl, xh), (wl, wh) = GEMM_RANGES[dt]
    x = _noise(rng, (M, K), dt) * _spread(rng, M, xl, xh)[:, None]
    w = _noise(rng, (N, K), dt) * (0.05 * _spread(rng, N, wl, wh))[:, None]
    b = _spread(rng, N, -3, 1) * rng.choice(np.float32([-1, 1]), size=N)
    return round_to(x, dt), round_to(w, dt), round_to(b, dt)


def resid_operands(B, Nsrc, Np, N, dt, stream_dt, seed=0):
    """residual rows [B,Nsrc,N] spread per row (rounded to the stream type), LayerScale gamma [N] spread per column over
    10^U(-2,0) with random signs (fp32, rounded to `dt`), and sorted gather indices [B,Np]"""
    rng = np.random.default_rng([seed, B, Nsrc, N, 7])
    lo, hi = (-2, 2) if "fp16" in (dt, stream_dt) else (-3, 3)
    r = _noise(rng, (B, Nsrc, N), stream_dt) * _spread(rng, B * Nsrc, lo, hi).reshape(B, Nsrc, 1)
    gam = _spread(rng, N, -2, 0) * rng.choice(np.float32([-1, 1]), size=N)
    idx = np.stack([np.sort(rng.choice(Nsrc, Np, replace=False)) for _ in range(B)]).astype(np.int32)
    return round_to(r, stream_dt), round_to(gam, dt), idx


def gemm_pre(x, w, b):
    """(pre, S, g): pre = x W^T + b and S = |x| |W|^T + |b| in fp64, g = (K + 2) u32.
    g is the worst case of K products accumulated in fp32 in ANY order with round-to-nearest adds (gamma_K of the
    standard summation analysis, to first order) plus the bias add and one more operation of the epilogue."""
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), np.asarray(b, np.float64)
    return x64 @ w64.T + b64, np.abs(x64) @ np.abs(w64).T + np.abs(b64), (x.shape[1] + 2) * U32


A_GELU_16 = 5e-5     # the packed polynomial GELU of the 16-bit epilogues: documented 4.24e-5 absolute, plus margin
GELU_SLOPE = 1.13    # max |gelu'(x)| (1.129 at x = sqrt(2))


def budget_bias(pre, S, g, out_dt):
    u = UNIT[out_dt]
    return u * np.abs(pre) + (1 + u) * g * S + FLOOR[out_dt]


def budget_gelu(pre, S, g, out_dt, a_gelu):
    return UNIT[out_dt] * np.abs(orc.gelu(pre)) + GELU_SLOPE * g * S + a_gelu + FLOOR[out_dt]


def budget_resid(pre, S, g, r, gam, out_dt):
    """want = r + gamma * pre (fp64); the 2 u32 term: the fused multiply-add and the fp32 value of the stream"""
    want = r + gam * pre
    return want, UNIT[out_dt] * np.abs(want) + np.abs(gam) * g * S + 2 * U32 * (np.abs(r) + np.abs(gam * pre)) + FLOOR[out_dt]


def gelu32_reference_error(x32):
    """|torch CPU fp32 gelu - fp64 gelu| at the fp32 points x32, as a LOCAL envelope (running maximum over the 129
    neighbouring points of the sorted grid: a single reference value may be exact by chance), in x32's order"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).ravel()
    order = np.argsort(x32, kind="stable")
    xs = x32[order]
    err = np.abs(torch.nn.functional.gelu(torch.from_numpy(xs)).numpy().astype(np.float64) - orc.gelu(xs.astype(np.float64)))
    pad = np.pad(err, 64, mode="edge")
    env = np.lib.stride_tricks.sliding_window_view(pad, 129).max(axis=1)
    out = np.empty_like(env)
    out[order] = env
    return out


def a_gelu_fp32(pre):
    """fp32 (erff) GELU epilogue: 4x the error of torch's CPU fp32 gelu against fp64 at the same pre-activations,
    floor 2 u32 |gelu|"""
    p32 = pre.astype(np.float32)
    return np.maximum(4 * gelu32_reference_error(p32).reshape(pre.shape), 2 * U32 * np.abs(orc.gelu(pre)))


def old_global_ok(got, want, rel):
    """the suite's previous criterion: max |got - want| <= rel * max |want| over the whole tensor"""
    return np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
LN_CASES = ["plain", "massive", "mean100", "mean1000", "tiny", "constant", "big"]
# c_ln: multiple of u32 * max|w| * (kappa_row + |n|) a two-pass fp32 LayerNorm may be off by.  Not derivable without
# assuming a reduction tree, so it is MEASURED against two references (never against the kernel) over every (rows, C,
# input type) the GPU test launches - LN_ROW_COUNTS x {192, 768, 1024, 1280} x {bf16, fp16, fp32}, every case among the rows
# of each - by tests/test_numerics_cpu.py::test_layernorm_c_ln_is_three_times_the_references, unrounded fp32 results:
#   torch CPU fp32 layer_norm                           c <= 2.79   (worst: 4109 x 192, bf16 input)
#   numpy two-pass, 64-lane butterfly sums (fp32)       c <= 5.54   (worst: 4109 x 1280, fp32 input)
#   a one-pass E[x^2] - E[x]^2 variance needs           c >= 2.6e3  (fp16 input; >= 1e5 on fp32 input)
# c_ln = 3 x the larger, rounded up: the margin covers another (still two-pass) summation order and the hardware rsqrt.
C_LN_MEASURED = {"torch_cpu_fp32": 2.79, "butterfly64_two_pass": 5.54}
C_LN = 17.0
LN_ROW_COUNTS = (77, 4109)     # below / above 4096 rows: the one-row and the two-rows-per-wave kernels


def layernorm_rows(rows, C, in_dt, seed=0):
    """x [rows, C] (rounded to in_dt), case name per row, w, b (fp32 values).  The cases alternate row by row, so the rows
    a wave / workgroup handles together differ.  `mean1000` (std 0.05 on mean 1000) is not representable in 16 bits:
    16-bit inputs get `plain` rows in its place."""
    rng = np.random.default_rng([seed, rows, C])
    x = rng.standard_normal((rows, C), dtype=np.float32)
    names = []
    for r in range(rows):
        case = LN_CASES[(r + r // len(LN_CASES)) % len(LN_CASES)]
        if case == "mean1000" and in_dt != "fp32":
            case = "plain"
        names.append(case)
        if case == "massive":
            a, b = rng.choice(C, 2, replace=False)
            x[r, a] += 300.0
            x[r, b] -= 180.0
        elif case == "mean100":
            x[r] = 100.0 + 0.1 * x[r]
        elif case == "mean1000":
            x[r] = 1000.0 + 0.05 * x[r]
        elif case == "tiny":
            x[r] *= 1e-4
        elif case == "constant":
            x[r] = np.float32(rng.uniform(-8, 8))
        elif case == "big":
            x[r] = np.clip(x[r] * 1e4, -6e4, 6e4)
    w = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return round_to(x, in_dt), np.array(names), w, b


def layernorm_budget(x, w, b, eps, out_dt, c_ln=C_LN):
    """(want, budget): |err| <= u_out |want| + c_ln u32 max|w| (kappa_row + |n|), kappa_row = max|x_row| / sqrt(var_row + eps)"""
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=-1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=-1, keepdims=True)
    n = (x64 - mu) / np.sqrt(var + eps)
    want = n * w + b
    kappa = np.abs(x64).max(axis=-1, keepdims=True) / np.sqrt(var + eps)
    return want, UNIT[out_dt] * np.abs(want) + c_ln * U32 * np.abs(w).max() * (kappa + np.abs(n)) + FLOOR[out_dt]


def layernorm_needed_c(y32, x, w, b, eps):
    """smallest c_ln for which the UNROUNDED fp32 result y32 of a reference implementation meets the budget"""
    want, unit = layernorm_budget(x, w, b, eps, "fp32", c_ln=1.0)
    unit = unit - UNIT["fp32"] * np.abs(want) - FLOOR["fp32"]
    return float((np.abs(y32.astype(np.float64) - want) / unit).max())


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
ATTN_KINDS = ["peaked", "negative", "ramp", "descending", "cancel", "uniform"]     # + "vbig" for fp16


def _unit_vectors(rng, H, D):
    u = rng.standard_normal((H, D))
    return (u / np.linalg.norm(u, axis=-1, keepdims=True)).astype(np.float32)


def attention_qkv(kind, B, N, H, D, dt, seed=0):
    """qkv [B, N, 3*H*D] ([3][H][D] on the last axis), rounded to `dt`.  Logits are q.k / sqrt(D):
    peaked      q, k = 3 n: logits ~ 9 N(0,1), tails near +-40
    negative    q = 0.5 n + a u, k = 0.5 n - a u, a^2 = 32 sqrt(D): every logit in about [-38, -26]
    ramp        logit of key j ~ 5 j / 32: block maxima (32 keys) rise ~7 log2 units - the lazy rescale of attention.hip
                (taken when a block maximum exceeds the running one by more than 8) is skipped, then taken
    descending  the mirror image: the first block dominates
    cancel      V = +-50 alternating by key + 0.1 n: outputs are small differences of large terms
    uniform     all keys equal: every output is the mean of V
    vbig        (fp16) V = 3e4 + 100 n: outputs near the top of the fp16 range"""
    rng = np.random.default_rng([seed, B, N, H, D, ATTN_KINDS.index(kind) if kind in ATTN_KINDS else 9])
    t = rng.standard_normal((B, N, 3, H, D), dtype=np.float32)
    u = _unit_vectors(rng, H, D)
    if kind == "peaked":
        t[:, :, 0:2] *= 3.0
    elif kind == "negative":
        a = np.float32(math.sqrt(32.0 * math.sqrt(D)))
        t[:, :, 0] = 0.5 * t[:, :, 0] + a * u
        t[:, :, 1] = 0.5 * t[:, :, 1] - a * u
    elif kind in ("ramp", "descending"):
        a = np.float32(2.0 * D ** 0.25)
        j = np.arange(N, dtype=np.float32)
        if kind == "descending":
            j = j[::-1]
        cj = (5.0 * j / 64.0) * np.float32(D ** 0.25)          # a * cj / sqrt(D) = 5 j / 32
        t[:, :, 0] = 0.1 * t[:, :, 0] + a * u
        t[:, :, 1] = 0.3 * t[:, :, 1] + cj[None, :, None, None] * u
    elif kind == "cancel":
        sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.float32)
        t[:, :, 2] = 50.0 * sign[None, :, None, None] + 0.1 * t[:, :, 2]
    elif kind == "uniform":
        t[:, :, 1] = t[:, :1, 1]
    elif kind == "vbig":
        t[:, :, 2] = 3e4 + 100.0 * t[:, :, 2]
    else:
        raise ValueError(kind)
    return round_to(t.reshape(B, N, 3 * H * D), dt)


def p_truncation_probe(dt, N=33, D=64):
    """qkv [1, N, 3D] on which a P operand rounded by TRUNCATION leaves the attention budget (on unstructured inputs it cannot:
    a truncation error is at most 2 u_P per P value, u_P on average, inside the u_P A term).  One head; key 0 holds the row
    maximum with V = 0, every other key is the same key with the same V row, placed so that its P = exp2(logit difference)
    lies in (0.5 (1 + 1.7 u), 0.5 (1 + 2 u)): rounding to nearest moves it by < 0.3 u, truncation by > 1.7 u relative -
    and the output is that P times V, normalised."""
    u = UNIT[dt]
    c = 0.125 * 1.4426950408889634
    cands = round_to(1.0 + np.arange(0, 2048) * u * 2, dt).astype(np.float64)            # representable values in [1, 2]
    k1, b = -4.75, 2.0 ** -3
    pj = np.exp2(c * ((k1 - 1.0) + b * cands))                                           # q = (1, b, 0 ...), key 0 = (1, 0, ...)
    ok = np.where((pj > 0.5 * (1 + 1.7 * u)) & (pj < 0.5 * (1 + 1.97 * u)))[0]
    assert len(ok), "no representable key lands P in the window"
    t = np.zeros((1, N, 3, 1, D), np.float32)
    t[:, :, 0, 0, 0], t[:, :, 0, 0, 1] = 1.0, b
    t[:, 0, 1, 0, 0] = 1.0
    t[:, 1:, 1, 0, 0], t[:, 1:, 1, 0, 1] = k1, cands[ok[0]]
    t[:, 1:, 2, 0] = np.random.default_rng(5).standard_normal(D, dtype=np.float32)
    g = round_to(t.reshape(1, N, 3 * D), dt)
    assert np.array_equal(g[..., :2 * D], t.reshape(1, N, 3 * D)[..., :2 * D])           # q and k are exact in dt
    return g


def attention_budget(qkv_g, H, scale, dt):
    """qkv_g [B, Np, 3C]: the GATHERED rows (fp32 values of type dt).  Returns (want, budget) [B, Np, C].
    |err| <= u_out |want| + (u_P + 4 ds) A (+ Np 2^-25 max|V| for fp16), A = softmax |V|,
    ds = (D + 2) u32 scale max_j sum_d |q_d k_jd| (the logit's fp32 accumulation error, which exp turns into a relative
    error of p; 4 = numerator and denominator, twice for the exp2 argument's own rounding and the 1/l).
    fp32 (VALU path): u_P = u32 and 8 u32 max|logit - rowmax| more for the fast exp2 (its argument s*c - m carries
    a rounding error relative to its own magnitude, and the hardware exp2 is accurate to about one ulp)."""
    q, k, v = orc.split_heads(qkv_g.astype(np.float64), H)           # [B,H,Np,D]
    B, _, Np, D = q.shape
    s = np.einsum("bhqd,bhkd->bhqk", q, k) * scale
    sabs = np.einsum("bhqd,bhkd->bhqk", np.abs(q), np.abs(k)).max(axis=-1) * scale       # [B,H,Np]
    mx = s.max(axis=-1, keepdims=True)
    p = np.exp(s - mx)
    p /= p.sum(axis=-1, keepdims=True)
    want = np.einsum("bhqk,bhkd->bqhd", p, v).reshape(B, Np, H * D)
    A = np.einsum("bhqk,bhkd->bqhd", p, np.abs(v)).reshape(B, Np, H * D)
    ds = (D + 2) * U32 * sabs                                         # [B,H,Np]
    fac = (UNIT[dt] if dt != "fp32" else U32) + 4 * ds
    if dt == "fp32":
        fac = fac + 8 * U32 * np.abs(s - mx).max(axis=-1)
    fac = np.repeat(fac.transpose(0, 2, 1)[..., None], D, axis=-1).reshape(B, Np, H * D)
    bud = UNIT[dt] * np.abs(want) + fac * A + FLOOR[dt]
    if dt == "fp16":
        vmax = np.abs(v).max(axis=(2, 3))                              # [B,H]
        bud = bud + np.repeat((Np * 2.0 ** -25 * vmax)[:, None, :, None], D, axis=-1).reshape(B, 1, H * D)
    return want, bud


# ---------------------------------------------------------------------------------------------------------------
# importance scores
# ---------------------------------------------------------------------------------------------------------------
IMP_KINDS = ["peaked", "negative", "voffset", "vflat", "voutlier"]


def importance_qkv(kind, B, N, H, D, dt, seed=0):
    """peaked / negative as attention_qkv (the CLS query against every key); voffset V = 50 + 0.5 n (centring over tokens
    cancels two digits); vflat V rows = one row + 0.02 n (norms of the centred rows nearly equal); voutlier one token's V x 200"""
    rng = np.random.default_rng([seed, B, N, H, D, 20 + IMP_KINDS.index(kind)])
    if kind in ("peaked", "negative"):
        return attention_qkv(kind, B, N, H, D, dt, seed=seed + 1)
    t = rng.standard_normal((B, N, 3, H, D), dtype=np.float32)
    if kind == "voffset":
        t[:, :, 2] = 50.0 + 0.5 * t[:, :, 2]
    elif kind == "vflat":
        t[:, :, 2] = t[:, :1, 2] + 0.02 * t[:, :, 2]
    elif kind == "voutlier":
        t[:, N // 2, 2] *= 200.0
    return round_to(t.reshape(B, N, 3 * H * D), dt)


def importance_budget(qkv, H, dt, eps=1e-6):
    """(want, budget, e32): |err| <= (u_out + 4 e32) |want|, e32 = the largest relative error of the fp32 run of the oracle
    against its fp64 run on these inputs (4x: the device's fixed-order sums differ from numpy's)"""
    want = orc.importance_scores(qkv, H, eps)
    s32 = orc.importance_scores(qkv, H, eps, dtype=np.float32).astype(np.float64)
    e32 = float((np.abs(s32 - want) / np.abs(want)).max())
    return want, (UNIT[dt] + 4 * e32) * np.abs(want) + FLOOR[dt], e32


def worst_ratio(got, want, budget):
    """max err / budget and the flat index where it occurs"""
    r = np.abs(np.asarray(got, np.float64) - want) / budget
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r.ravel()[i]), i


def assert_within(got, want, budget, what):
    ratio, i = worst_ratio(got, want, budget)
    g, w, b = np.asarray(got, np.float64).ravel()[i], np.asarray(want).ravel()[i], np.broadcast_to(budget, np.shape(want)).ravel()[i]
    print(f"[numerics] {what}: worst err/budget {ratio:.3f}")
    assert ratio <= 1.0, (f"{what}: element {np.unravel_index(i, np.shape(want))} got {g!r} want {w!r} |err| {abs(g - w):.4g} "
                          f"> budget {b:.4g} (x{ratio:.3g}); {int((np.abs(np.asarray(got, np.float64) - want) > budget).sum())} "
                          f"of {np.size(want)} elements over")
