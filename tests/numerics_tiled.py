"""Helpers of the tiled score tests (tests/test_score_tiled_cpu.py, tests/test_gpu_score_tiled.py): the scratch layout of
rajni_score_select_workspace_bytes restated, and a numpy fp32 restatement of the tiled kernels' summation order."""
from __future__ import annotations

import numpy as np

TILE = 32          # ST_TILE of csrc/score_select.hip (pinned against the library by test_workspace_size_is_the_documented_layout)
MAX_N = 16384 + 32      # ST_MAX_N: 16384 patch tokens + RAJNI_MAX_PREFIX


def align256(v: int) -> int:
    return (v + 255) // 256 * 256


def workspace_bytes(B: int, N: int, H: int, D: int) -> int:
    """fp32 logits [B][H][N], vbar [B][N][D], per-tile column sums [B][tiles][D], per-tile (max, sum exp) [B][tiles][H][2],
    each region rounded up to 256 bytes"""
    tiles = (N + TILE - 1) // TILE
    return sum(align256(4 * n) for n in (B * H * N, B * N * D, B * tiles * D, B * tiles * H * 2))


def single_workgroup_lds_bytes(N: int, H: int, D: int) -> int:
    """LDS of the single-workgroup kernel in its smaller (two-pass) layout, for N well above a handful of tokens:
    (C + max(H N, N D) rounded to 4 + 2 N + 2 H + 512 + D + 16 + 16) words"""
    region = (max(H * N, N * D) + 3) // 4 * 4
    return 4 * (H * D + region + 2 * N + 2 * H + 512 + D + 16 + 16)


def tiled_scores_f32(qkv: np.ndarray, H: int, eps: float = 1e-6) -> np.ndarray:
    """importance scores [B, N] in fp32 with the tiled kernels' order of the long sums: per-tile partial sums (TILE consecutive
    tokens) joined in tile order for the softmax denominator (rescaled to the global maximum) and the token mean of vbar; the
    norms are taken against that mean.  Every operation is fp32 (np.float32 arrays and scalars)."""
    f = np.float32
    qkv = np.asarray(qkv, dtype=f)
    B, N, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    t = qkv.reshape(B, N, 3, H, D)
    q, k, v = t[:, 0, 0], t[:, :, 1], t[:, :, 2]                    # [B,H,D], [B,N,H,D], [B,N,H,D]
    logits = (np.einsum("bhd,bnhd->bhn", q, k).astype(f) * f(1.0 / np.sqrt(f(D)))).astype(f)
    vbar = np.zeros((B, N, D), f)
    for h in range(H):                                              # heads in head order
        vbar = (vbar + v[:, :, h]).astype(f)
    vbar = (vbar * f(1.0 / H)).astype(f)
    tiles = [(s, min(s + TILE, N)) for s in range(0, N, TILE)]
    m_t = np.stack([logits[:, :, a:b].max(axis=2) for a, b in tiles], axis=2)                                  # [B,H,tiles]
    s_t = np.stack([np.exp(logits[:, :, a:b] - m_t[:, :, i:i + 1], dtype=f).sum(axis=2, dtype=f) for i, (a, b) in enumerate(tiles)], axis=2)
    mx = m_t.max(axis=2)
    se = np.zeros((B, H), f)
    for i in range(len(tiles)):                                     # tiles in tile order
        se = (se + s_t[:, :, i] * np.exp(m_t[:, :, i] - mx, dtype=f)).astype(f)
    p = (np.exp(logits - mx[:, :, None], dtype=f) / se[:, :, None]).astype(f)
    acls = np.zeros((B, N), f)
    for h in range(H):
        acls = (acls + p[:, h]).astype(f)
    acls = (acls / f(H)).astype(f)
    csum = np.zeros((B, D), f)
    for a, b in tiles:
        csum = (csum + vbar[:, a:b].sum(axis=1, dtype=f)).astype(f)
    mean = (csum / f(N)).astype(f)
    dlt = (vbar - mean[:, None]).astype(f)
    vn = np.sqrt((dlt * dlt).sum(axis=2, dtype=f), dtype=f)
    mu = (vn.sum(axis=1, dtype=f) / f(N)).astype(f)
    dv = (vn - mu[:, None]).astype(f)
    sd = (np.sqrt((dv * dv).sum(axis=1, dtype=f) / f(N - 1), dtype=f) + f(eps)).astype(f)
    z = (dv / sd[:, None]).astype(f)
    sig = (f(1.0) / (f(1.0) + np.exp(-z, dtype=f))).astype(f)
    return (acls * sig).astype(f)
