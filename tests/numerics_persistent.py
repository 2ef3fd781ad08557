"""Cases, inputs, fp64 references and the restated tile walk of the persistent-kernel tests (tests/test_persistent_cpu.py
checks the cases on the CPU, tests/test_gpu_persistent.py runs them).  Pure numpy / torch; nothing here needs a GPU.

The persistent kernels (gemm_bf16_tn_stream, gemm_f8_tn_stream, gemm_f8_tn_wide, attn_bf16_d64_stream) walk several tiles or
items per workgroup; what is fragile in them is the step from one to the next.  rajni_debug_set_persistent_workgroups(n)
caps the grid and changes nothing else, so a shape of a few tiles walks all of them through one, two, three ... workgroups.

Budgets are those of tests/numerics.py; the fp8 x fp8 epilogues and e4m3 outputs use the bounds of tests/numerics_fp8.py
(the rule tests/test_gpu_fp8_mfma.py holds them to).  Two bounds are formed here because no test stated them before:
  * fp8 x fp8 RESID on the bf16 stream: the fp32-stream bound of numerics_fp8 plus the rounding of the bf16 store,
    u_bf16 |want| per element (f8_resid_bound);
  * patch embed: the GEMM BIAS budget with the position row as a second bias term - one more fp32 add (patch_case).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import numerics as nm
import numerics_fp8 as n8
from oracle import rajni_oracle as orc
from rajni_amd import ops

# ---------------------------------------------------------------------------------------------------------------
# the tile walk of the stream GEMMs, restated from csrc/gemm.hip (xcd_tile_of, tile_mn, the loop of gemm_bf16_tn_stream)
# ---------------------------------------------------------------------------------------------------------------
BM = 256
BN = {4: 256, 5: 128}                 # rajni_debug_force_gemm_tiling: 4 = wide 256x256, 5 = mid 256x128
BN_F8 = {1: 128, 2: 256}              # rajni_debug_force_f8_tiling: 1 = 256x128, 2 = 256x256
K_MIN = {4: 192, 5: 256}              # NS + 1 K steps of 64


def xcd_tile_of(v, total):
    """tile id of the v-th workgroup slot: slots v and v + 8 share an XCD, each XCD owns a contiguous range of ids"""
    q, r, xcd, loc = total >> 3, total & 7, v & 7, v >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + loc


def tile_mn(t, tiles_m, tiles_n, nblk):
    """(row tile, column tile) of tile id t: ids run (N block, row tile, column in block)"""
    if nblk >= tiles_n:
        return t // tiles_n, t % tiles_n
    per = nblk * tiles_m
    blk, r = t // per, t % per
    nb = min(nblk, tiles_n - blk * nblk)
    return r // nb, blk * nblk + r % nb


def forced_nblk(tiles_n, nblock_bytes):
    """column tiles per N block under rajni_debug_set_gemm_nblock_bytes(-k) (k column tiles) or (0) (plain order)"""
    return tiles_n if nblock_bytes == 0 else min(-nblock_bytes, tiles_n)


def walk(total, tiles_n, nblk, grid):
    """per workgroup, the (row tile, column tile) sequence it computes: slot v = workgroup, then v + grid, ..."""
    tiles_m = total // tiles_n
    return [[tile_mn(xcd_tile_of(v, total), tiles_m, tiles_n, nblk) for v in range(wg, total, grid)] for wg in range(grid)]


def is_interior(tm, tn, M, N, bn):
    """a tile whose 256 rows and bn columns all exist (the kernels' `inter`: decides the epilogue path and NSTORE wait)"""
    return tm * BM + BM <= M and tn * bn + bn <= N


def steps_taken(M, N, bn, nblk, grid):
    """(set of 'ii' 'ir' 'ri' 'rr' steps some workgroup takes between consecutive tiles (i = interior, r = ragged), whether
    some step crosses an N block)"""
    tiles_m, tiles_n = -(-M // BM), -(-N // bn)
    kinds, crosses = set(), False
    for seq in walk(tiles_m * tiles_n, tiles_n, nblk, grid):
        for (a, b) in zip(seq, seq[1:]):
            kinds.add("ir"[not is_interior(*a, M, N, bn)] + "ir"[not is_interior(*b, M, N, bn)])
            crosses |= a[1] // nblk != b[1] // nblk
    return kinds, crosses


# ---------------------------------------------------------------------------------------------------------------
# GEMM cases
# ---------------------------------------------------------------------------------------------------------------
M, N = 549, 580                       # three row tiles, the last ragged (rows 293..548); 3 x 256 or 5 x 128 ragged column tiles
B_IMG, NP, NSRC = 3, 183, 197         # M = B_IMG * NP rows gathered from NSRC per image
LD = (N + 7) // 8 * 8                 # leading dimension of 16-bit / fp32 outputs and residual rows
GEMM_CAPS = (1, 2, 3, 4, 7)
PATCH_CAPS = (1, 2, 3, 5)
ATTN_CAPS = (1, 2, 4, 7)
GEMM16_CASES = [(fmt, tiling, K) for fmt in ("bf16", "fp16", "w8") for tiling in (4, 5) for K in (K_MIN[tiling], 832)]
F8_CASES = [(tiling, K) for tiling in (1, 2) for K in (512, 1280)]
NBLOCK_UNDER_CAP = (2, (-1, -2))      # (cap, rajni_debug_set_gemm_nblock_bytes values): N blocks of 1 and 2 column tiles


ALL = (slice(None), slice(None))


class Form:
    """one epilogue form of a GEMM case: expected values, budget, and want_of(pre block, sel): how the expected values of the
    block sel = (row index, column index) follow from its pre-activation"""

    def __init__(self, name, epi, want_of, pre, budget, stream=None, gather=False, r=None, gam=None, idx=None):
        self.name, self.epi, self.want_of, self.budget = name, epi, want_of, budget
        self.want = want_of(pre, ALL)
        self.stream, self.gather, self.r, self.gam, self.idx = stream, gather, r, gam, idx


def pad_cols(a, ld):
    return a if a.shape[-1] == ld else np.concatenate([a, np.zeros(a.shape[:-1] + (ld - a.shape[-1],), a.dtype)], axis=-1)


def plain_m0(tm, rows=M):
    """first X row of row tile tm in the 16-bit stream kernels: a ragged last tile starts at M - 256"""
    return rows - BM if tm * BM + BM > rows else tm * BM


def clamped_m0(tm, rows=M):
    """... in the fp8 x fp8 kernels and the fused patch loader: tm * 256, rows past the end clamped to the last"""
    return tm * BM


@functools.lru_cache(maxsize=2)
def gemm16_case(fmt, K):
    """operands and the six epilogue forms of a 16-bit-activation case; fmt: bf16, fp16, or w8 (e4m3 weights on bf16)"""
    dt = "bf16" if fmt == "w8" else fmt
    x, w, b = nm.gemm_operands(M, N, K, dt)
    q = s = None
    wref = w
    if fmt == "w8":
        q, s = ops.pack_weight_fp8(torch.from_numpy(w), nm.TORCH[dt])
        wref = (q[:N].view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64) * s.to(torch.float64)[:, None]).numpy()
    pre, S, g = nm.gemm_pre(x, wref, b)
    forms = [Form("BIAS", 0, lambda p, sel: p, pre, nm.budget_bias(pre, S, g, dt)),
             Form("GELU", 1, lambda p, sel: orc.gelu(p), pre, nm.budget_gelu(pre, S, g, dt, nm.A_GELU_16))]
    for stream in (dt, "fp32"):
        for gather in (True, False):
            nsrc = NSRC if gather else NP
            r, gam, idx = nm.resid_operands(B_IMG, nsrc, NP, N, dt, stream)
            r_used = (orc.gather_rows(r, idx.astype(np.int64)) if gather else r).reshape(M, N).astype(np.float64)
            gam64 = gam.astype(np.float64)
            _, bud = nm.budget_resid(pre, S, g, r_used, gam64, stream)
            forms.append(Form(f"RESID {stream} {'gathered' if gather else 'in place'}", 2,
                              lambda p, sel, r_used=r_used, gam64=gam64: r_used[sel] + gam64[sel[1]] * p, pre, bud, stream, gather,
                              pad_cols(r, LD), gam, idx))
    return dict(dt=dt, x=x, w=w, b=b, q=q, s=s, pre=pre, forms=forms, m0=plain_m0)


def f8_resid_bound(want, stream):
    """fp8 x fp8 RESID: numerics_fp8's fp32-stream bound; a bf16 stream adds the rounding of its store, u_bf16 |want|"""
    return n8.resid_f32_bound(want) + (nm.UNIT["bf16"] * np.abs(want) if stream == "bf16" else 0.0)


@functools.lru_cache(maxsize=2)
def f8_case(K):
    """fp8 x fp8 operands (uniform random e4m3 codes, as tests/test_gpu_fp8_mfma.py draws them) and the epilogue forms"""
    rng = np.random.default_rng([K, M, N])
    xq, xs, wp, ws, xd, wd = n8.f8_operands(rng, M, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    pre = xd @ wd.T + b
    ys = n8.gelu8_row_scales(rng, pre)
    h = orc.gelu(pre)
    forms = [Form("BIAS", 0, lambda p, sel: p, pre, np.broadcast_to(n8.bias_bound(pre), pre.shape)),
             Form("GELU8", 1, lambda p, sel: orc.gelu(p), pre, n8.gelu8_bound(h, ys))]
    gam = rng.uniform(0.2, 1.5, size=N).astype(np.float32)
    for stream in ("bf16", "fp32"):
        for gather in (True, False):
            nsrc = NSRC if gather else NP
            r = nm.round_to(rng.standard_normal((B_IMG, nsrc, N)).astype(np.float32), stream)
            idx = np.stack([np.sort(rng.choice(nsrc, NP, replace=False)) for _ in range(B_IMG)]).astype(np.int32)
            r_used = (orc.gather_rows(r, idx.astype(np.int64)) if gather else r).reshape(M, N).astype(np.float64)
            want_of = lambda p, sel, r_used=r_used: gam.astype(np.float64)[sel[1]] * p + r_used[sel]
            bud = np.broadcast_to(f8_resid_bound(want_of(pre, ALL), stream), pre.shape)
            forms.append(Form(f"RESID {stream} {'gathered' if gather else 'in place'}", 2, want_of, pre, bud, stream, gather,
                              pad_cols(r, LD), gam, idx))
    return dict(xq=xq, xs=xs, wp=wp, ws=ws, b=b, pre=pre, ys=ys, forms=forms, m0=clamped_m0)


def f8_forms(case, tiling):
    """the 256 x 256 fp8 tiling exists for the BIAS and GELU8 epilogues only"""
    return [f for f in case["forms"] if tiling == 1 or f.epi != 2]


# ---- patch embed on the stream tilings ------------------------------------------------------------------------
PATCH_S, PATCH_B, PATCH_C = 64, 35, 320
PATCH_CASES = ([(dt, out_f32, tiling, 16) for dt in ("bf16", "fp16") for out_f32 in (False, True) for tiling in (4, 5)] +
               [(dt, out_f32, 4, 8) for dt in ("bf16", "fp16") for out_f32 in (False, True)])


@functools.lru_cache(maxsize=2)
def patch_case(dt, out_f32, P):
    """images [35, 3, 64, 64] -> x [35, 1 + (64 / P)^2, 320], position rows with a CLS row.  Budget of a patch row: the GEMM
    BIAS budget with the position row as a second bias (pre + pos, S + |pos|, one more fp32 add in g); the CLS row is one
    add of two values of the model type."""
    rng = np.random.default_rng([PATCH_S, P, 11])
    npatch, K = (PATCH_S // P) ** 2, 3 * P * P
    img = nm.round_to(rng.standard_normal((PATCH_B, 3, PATCH_S, PATCH_S), dtype=np.float32), dt)
    w = nm.round_to(rng.standard_normal((PATCH_C, 3, P, P), dtype=np.float32) * 0.05, dt)
    b = nm.round_to(rng.standard_normal(PATCH_C, dtype=np.float32) * 0.1, dt)
    cls = nm.round_to(rng.standard_normal(PATCH_C, dtype=np.float32), dt)
    pos = nm.round_to(rng.standard_normal((npatch + 1, PATCH_C), dtype=np.float32), dt)
    out_dt = "fp32" if out_f32 else dt
    cols = img.reshape(PATCH_B, 3, PATCH_S // P, P, PATCH_S // P, P).transpose(0, 2, 4, 1, 3, 5).reshape(PATCH_B * npatch, K)
    pre, S, g = nm.gemm_pre(cols, w.reshape(PATCH_C, K), b)
    pos_rows = np.tile(pos[1:].astype(np.float64), (PATCH_B, 1))
    bud = nm.budget_bias(pre + pos_rows, S + np.abs(pos_rows), g + nm.U32, out_dt)
    form = Form("PATCH", 0, lambda p, sel: p + pos_rows[sel], pre, bud)
    cls_want = cls.astype(np.float64) + pos[0]
    cls_bud = nm.UNIT[out_dt] * np.abs(cls_want) + 2 * nm.U32 * (np.abs(cls) + np.abs(pos[0])) + nm.FLOOR[out_dt]
    return dict(img=img, w=w, b=b, cls=cls, pos=pos, npatch=npatch, K=K, out_dt=out_dt, pre=pre, forms=[form],
                cls_want=cls_want, cls_bud=cls_bud, m0=clamped_m0, rows=PATCH_B * npatch, cols=PATCH_C)


def swapped_fraction(form, pre, b, rows, cols, bn, m0):
    """For every output tile of rows x cols in 256 x bn tiles: the fraction of the tile's elements whose expected value leaves
    the budget when the tile is computed from ANOTHER row tile's X rows, resp. another column tile's W rows (the bias stays
    the column's own: the epilogue indexes it by output column).  Returns the smallest fraction over all tiles and swaps."""
    tiles_m, tiles_n = -(-rows // BM), -(-cols // bn)
    prod = pre - b
    worst = 1.0
    for tm in range(tiles_m):
        rr = np.arange(tm * BM, min(rows, tm * BM + BM))
        for tn in range(tiles_n):
            cc = np.arange(tn * bn, min(cols, tn * bn + bn))
            for tm2 in range(tiles_m):
                for tn2 in range(tiles_n):
                    if (tm2 == tm) == (tn2 == tn):
                        continue        # swap exactly one of the two operands
                    rs = np.minimum(m0(tm2, rows) + rr - m0(tm, rows), rows - 1) if tm2 != tm else rr
                    cs = np.minimum(tn2 * bn + cc - tn * bn, cols - 1) if tn2 != tn else cc
                    sel = np.ix_(rr, cc)
                    wrong = form.want_of(prod[np.ix_(rs, cs)] + b[cc], sel)
                    bad = np.abs(wrong - form.want[sel]) > form.budget[sel]
                    worst = min(worst, float(bad.mean()))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# attention cases
# ---------------------------------------------------------------------------------------------------------------
ATTN_NP = (20, 33, 87, 121, 150, 173, 224, 256)       # one token count per instantiation, NSUB = ceil(np / 32) = 1..8
ATTN_B, ATTN_H, ATTN_D = 5, 3, 64                     # 15 items
ATTN_SCALE = ATTN_D ** -0.5
ATTN_KINDS = ("peaked", "cancel", "normal")
ATTN_EXTRA = 19                                       # gathered form: n_src = np + 19


def attention_inputs(kind, n_src, dt):
    if kind == "normal":
        rng = np.random.default_rng([n_src, 3])
        return nm.round_to(rng.standard_normal((ATTN_B, n_src, 3 * ATTN_H * ATTN_D), dtype=np.float32), dt)
    return nm.attention_qkv(kind, ATTN_B, n_src, ATTN_H, ATTN_D, dt)


@functools.lru_cache(maxsize=8)
def attention_case(kind, n_kept, gathered, dt):
    """(qkv [B, n_src, 3C], keep_idx [B, np] or None, want, budget) - a distinct random selection per image"""
    n_src = n_kept + ATTN_EXTRA if gathered else n_kept
    qkv = attention_inputs(kind, n_src, dt)
    idx = None
    g = qkv
    if gathered:
        idx = nm.pick_rows(np.random.default_rng([n_kept, 5]), ATTN_B, n_src, n_kept).astype(np.int32)
        assert len({tuple(r) for r in idx}) == ATTN_B
        g = orc.gather_rows(qkv, idx.astype(np.int64))
    want, bud = nm.attention_budget(g, ATTN_H, ATTN_SCALE, dt)
    return qkv, idx, want, bud


def items_of(a):
    """[B, Np, H * D] -> [B * H, Np, D]: item = image * H + head, the order the persistent kernel walks"""
    Bq, n, _ = a.shape
    return a.reshape(Bq, n, ATTN_H, ATTN_D).transpose(0, 2, 1, 3).reshape(Bq * ATTN_H, n, ATTN_D)


# ---------------------------------------------------------------------------------------------------------------
# the budgets of tests/numerics.py on torch tensors (fp64, any device) - for references computed on the GPU;
# tests/test_persistent_cpu.py holds them equal to the numpy originals
# ---------------------------------------------------------------------------------------------------------------

def gelu_t(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def gemm_pre_t(x, w, b):
    x64, w64, b64 = x.double(), w.double(), b.double()
    return x64 @ w64.T + b64, x64.abs() @ w64.abs().T + b64.abs(), (x.shape[1] + 2) * nm.U32


def budget_gelu_t(pre, S, g, out_dt, a_gelu):
    return nm.UNIT[out_dt] * gelu_t(pre).abs() + nm.GELU_SLOPE * g * S + a_gelu + nm.FLOOR[out_dt]


def budget_resid_t(pre, S, g, r, gam, out_dt):
    want = r + gam * pre
    return want, nm.UNIT[out_dt] * want.abs() + gam.abs() * g * S + 2 * nm.U32 * (r.abs() + (gam * pre).abs()) + nm.FLOOR[out_dt]


def attention_budget_t(qkv_g, H, scale, dt):
    """nm.attention_budget for the 16-bit types, image by image (the [H, Np, Np] logits of one image at a time)"""
    assert dt in ("bf16", "fp16")
    Bq, n, threeC = qkv_g.shape
    D = threeC // 3 // H
    want = torch.empty((Bq, n, H * D), dtype=torch.float64, device=qkv_g.device)
    bud = torch.empty_like(want)
    for i in range(Bq):
        t = qkv_g[i].double().reshape(n, 3, H, D).permute(1, 2, 0, 3)        # [3, H, Np, D]
        q, k, v = t[0], t[1], t[2]
        s = torch.einsum("hqd,hkd->hqk", q, k) * scale
        sabs = torch.einsum("hqd,hkd->hqk", q.abs(), k.abs()).amax(dim=-1) * scale      # [H, Np]
        p = torch.exp(s - s.amax(dim=-1, keepdim=True))
        p = p / p.sum(dim=-1, keepdim=True)
        w_ = torch.einsum("hqk,hkd->qhd", p, v)
        A = torch.einsum("hqk,hkd->qhd", p, v.abs())
        fac = (nm.UNIT[dt] + 4 * (D + 2) * nm.U32 * sabs).T[:, :, None]                 # [Np, H, 1]
        b_ = nm.UNIT[dt] * w_.abs() + fac * A + nm.FLOOR[dt]
        if dt == "fp16":
            b_ = b_ + (n * 2.0 ** -25 * v.abs().amax(dim=(1, 2)))[None, :, None]
        want[i], bud[i] = w_.reshape(n, H * D), b_.reshape(n, H * D)
    return want, bud


def worst_ratio_t(got, want, budget):
    r = (got.double() - want).abs() / budget
    return float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())


def factor_tiles(total):
    """(row tiles, column tiles) with row tiles * column tiles == total, as square as the factors of `total` allow"""
    b = max(d for d in range(1, int(total ** 0.5) + 1) if total % d == 0)
    return total // b, b
