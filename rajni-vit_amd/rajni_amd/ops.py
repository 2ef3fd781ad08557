"""Tensor-level entry points over the C ABI (one function per `rajni_*` symbol of
include/rajni_hip.h).  They only validate, allocate outputs with torch, and pass raw pointers plus
torch's current stream; all compute is in librajni_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import _native as nat


def keep_count(keep_ratio: float, n_tokens: int, num_prefix: int = 1) -> int:
    """`keep = max(1, int(keep_ratio * (N - 1)))` - Python-double semantics of the reference
    (rajni/wrapper/attention.py:31-32); data independent.  With `num_prefix` = P prefix tokens (CLS + register tokens)
    only the N - P patch tokens are ranked: max(1, int(keep_ratio * (N - P)))."""
    return max(1, int(keep_ratio * (n_tokens - num_prefix)))


def _dt(t: torch.Tensor) -> int:
    return nat.dtype_code(t.dtype)


def pack_weight(w: torch.Tensor, dtype=torch.bfloat16, device=None, k_multiple: int = 1) -> torch.Tensor:
    """[N, K...] Linear/Conv weight -> contiguous [ceil256(N), K] in `dtype`, zero padded rows
    (the GEMM stages whole 128- or 256-row W tiles).  `k_multiple` = 64 also zero-pads the columns to
    whole K steps - the patch-embed weight of a patch size whose Cin*P*P is not one (3*14*14 = 588 -> 640)."""
    n = w.shape[0]
    w2 = w.detach().reshape(n, -1)
    npad = (n + 255) // 256 * 256
    k = w2.shape[1]
    kpad = (k + k_multiple - 1) // k_multiple * k_multiple
    out = torch.zeros((npad, kpad), dtype=dtype, device=device if device is not None else w.device)
    out[:n, :k].copy_(w2)
    return out


FP8_E4M3_MAX = 448.0   # largest finite e4m3 "fn" value (OCP fp8: no infinities, one NaN pattern)


def quantize_rows_fp8(w: torch.Tensor):
    """Per-output-row symmetric fp8 e4m3 quantisation of a [N, K] weight held in the model dtype:
    scale[n] = max|w[n,:]| / 448 (1 for an all-zero row), q = round-to-nearest-even(w / scale) in e4m3.
    Returns (q as torch.float8_e4m3fn [N, K], scale fp32 [N]).  Host-side; runs wherever `w` lives."""
    w32 = w.detach().to(torch.float32)
    amax = w32.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    q = (w32 / scale[:, None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return q, scale


def pack_weight_fp8(w: torch.Tensor, model_dtype=torch.bfloat16, device=None, k_multiple: int = 1):
    """[N, K...] Linear weight -> (uint8 [ceil256(N), K] of e4m3 bytes with zero padded rows, fp32 scale [N]).
    The weight is first rounded to `model_dtype` (what the reference model would hold), then quantised.
    `k_multiple` zero-pads the columns (e4m3 0x00 = +0) like pack_weight."""
    n = w.shape[0]
    w2 = w.detach().reshape(n, -1).to(model_dtype)
    k = w2.shape[1]
    kpad = (k + k_multiple - 1) // k_multiple * k_multiple
    if kpad % 16 != 0:
        raise ValueError("fp8 weights need the (padded) input dimension to be a multiple of 16")
    q, scale = quantize_rows_fp8(w2)
    dev = device if device is not None else w.device
    npad = (n + 255) // 256 * 256
    out = torch.zeros((npad, kpad), dtype=torch.uint8, device=dev)
    out[:n, :k].copy_(q.view(torch.uint8))
    return out, scale.to(dev).contiguous()


def dequantize_fp8(q_packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K] weight the fp8 kernels multiply by: e4m3 value x row scale (the oracle side of parity tests)."""
    n = scale.shape[0]
    return q_packed[:n].view(torch.float8_e4m3fn).to(torch.float32) * scale.to(torch.float32)[:, None]


def pack_vec(v: Optional[torch.Tensor], like_dtype=torch.bfloat16, device=None) -> Optional[torch.Tensor]:
    """bias / LayerNorm / LayerScale vector -> fp32 copy of the value the model dtype holds."""
    if v is None:
        return None
    return v.detach().to(like_dtype).to(torch.float32).to(device if device is not None else v.device).contiguous()


def _placed(t: Optional[torch.Tensor], name: str, align: int = 16, in_place: bool = False) -> Optional[torch.Tensor]:
    """The placement contract of include/rajni_hip.h for one operand: `t` made contiguous with its data pointer a multiple
    of `align` bytes (16: data tensors and fp32 per-column vectors; 4: row scales and index arrays).  A contiguous view
    keeps its storage offset (`buf[1:].view(rows, C)`), so a read-only input below the contract is cloned into a fresh
    allocation; an operand the kernel writes (`in_place`: qk_norm, layernorm_stream, a caller's `out`) cannot be moved
    and raises ValueError.  An operand that meets the contract is returned as it is (the same object)."""
    if t is None:
        return None
    if in_place:
        if not t.is_contiguous():
            raise ValueError(f"{name} is written in place: it must be contiguous")
        if t.data_ptr() % align:
            raise ValueError(f"{name} must be {align}-byte aligned (it is written in place and cannot be copied)")
        return t
    t = t.contiguous()
    if t.data_ptr() % align:
        t = t.clone(memory_format=torch.contiguous_format)
        assert t.data_ptr() % align == 0, f"{name}: a fresh allocation is not {align}-byte aligned"
    return t


def _score_scratch(qkv: torch.Tensor, B: int, N: int, H: int, D: int) -> Optional[torch.Tensor]:
    """scratch of the tiled score kernels (rajni_score_select_ws), None for every shape one workgroup's LDS holds"""
    nbytes = nat.lib().rajni_score_select_workspace_bytes(B, N, H, D, _dt(qkv))
    return torch.empty(nbytes, dtype=torch.uint8, device=qkv.device) if nbytes else None


QUERIES = {"cls": nat.QUERY_CLS, "mean": nat.QUERY_MEAN}


def query_code(query: str) -> int:
    """"cls" (row 0 is the importance query) or "mean" (the mean of the N query rows, include/rajni_hip_query.h)"""
    if query not in QUERIES:
        raise ValueError(f'query must be "cls" or "mean", got {query!r}')
    return QUERIES[query]


def _score_select_query(qkv, B, N, H, D, eps, P, keep, query, scores, idx, nxt):
    """rajni_score_select_query with its own scratch (the mean query, or a sequence without prefix tokens)"""
    qc = query_code(query)
    nbytes = nat.lib().rajni_score_select_query_workspace_bytes(B, N, H, D, _dt(qkv), qc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device) if nbytes else None
    with nat.device_guard(qkv.device):
        nat.check(nat.lib().rajni_score_select_query(qkv.data_ptr(), B, N, H, D, eps, P, keep, qc, nat.ptr(scores), nat.ptr(idx),
                                                     nat.ptr(nxt), _dt(qkv), nat.ptr(ws), nbytes, nat.stream_ptr(qkv.device)),
                  "rajni_score_select_query")


def importance(qkv: torch.Tensor, num_heads: int, eps: float = 1e-6, query: str = "cls") -> torch.Tensor:
    nat.require_device(qkv, "qkv")
    qkv = _placed(qkv, "qkv")
    B, N, threeC = qkv.shape
    D = threeC // 3 // num_heads
    out = torch.empty((B, N), dtype=qkv.dtype, device=qkv.device)
    if query != "cls":
        _score_select_query(qkv, B, N, num_heads, D, eps, 0, 0, query, out, None, None)
        return out
    ws = _score_scratch(qkv, B, N, num_heads, D)
    with nat.device_guard(qkv.device):
        if ws is None:
            nat.check(nat.lib().rajni_importance(qkv.data_ptr(), out.data_ptr(), B, N, num_heads, D, eps, _dt(qkv),
                                                 nat.stream_ptr(qkv.device)), "rajni_importance")
        else:       # more tokens than one workgroup's LDS holds: the tiled kernels, through scratch
            nat.check(nat.lib().rajni_score_select_ws(qkv.data_ptr(), B, N, num_heads, D, eps, 1, 0, out.data_ptr(), None, None,
                                                      _dt(qkv), ws.data_ptr(), ws.numel(), nat.stream_ptr(qkv.device)),
                      "rajni_score_select_ws")
    return out


def select_topk(scores: torch.Tensor, keep: int, num_prefix: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores [B, N] -> (keep_idx int32 [B, P+keep], next_scores [B, P+keep]); the first P = `num_prefix` tokens are always
    kept (slots 0..P-1) and take no rank slot."""
    nat.require_device(scores, "scores")
    scores = _placed(scores, "scores", scores.element_size())
    B, N = scores.shape
    P = int(num_prefix)
    idx = torch.empty((B, keep + P), dtype=torch.int32, device=scores.device)
    nxt = torch.empty((B, keep + P), dtype=scores.dtype, device=scores.device)
    with nat.device_guard(scores.device):
        if P == 0:      # a sequence without a class row (include/rajni_hip_query.h)
            nat.check(nat.lib().rajni_select_topk_query(scores.data_ptr(), B, N, 0, keep, idx.data_ptr(), nxt.data_ptr(),
                                                        _dt(scores), nat.stream_ptr(scores.device)), "rajni_select_topk_query")
        elif P == 1:
            nat.check(nat.lib().rajni_select_topk(scores.data_ptr(), B, N, keep, idx.data_ptr(), nxt.data_ptr(),
                                                  _dt(scores), nat.stream_ptr(scores.device)), "rajni_select_topk")
        else:
            nat.check(nat.lib().rajni_select_topk_prefix(scores.data_ptr(), B, N, P, keep, idx.data_ptr(), nxt.data_ptr(),
                                                         _dt(scores), nat.stream_ptr(scores.device)), "rajni_select_topk_prefix")
    return idx, nxt


class RelPos(NamedTuple):
    """One block's relative position bias for the stand-alone entries (include/rajni_hip_relpos.h), fp32 on the device:
    table [H, (2 gh - 1) * (2 gw - 1)], prefix_q / prefix_k / prefix_qk [H], grid = (gh, gw)."""
    table: torch.Tensor
    prefix_q: torch.Tensor
    prefix_k: torch.Tensor
    prefix_qk: torch.Tensor
    grid: Tuple[int, int]


def _rel_pos_placed(rel_pos: "RelPos", num_heads: int) -> "RelPos":
    gh, gw = (int(g) for g in rel_pos.grid)
    T = (2 * gh - 1) * (2 * gw - 1)
    if tuple(rel_pos.table.shape) != (num_heads, T):
        raise ValueError(f"rel_pos.table must be [H, (2 gh - 1) * (2 gw - 1)] = [{num_heads}, {T}], got {tuple(rel_pos.table.shape)}")
    vals = []
    for name in ("prefix_q", "prefix_k", "prefix_qk"):
        v = getattr(rel_pos, name)
        if tuple(v.shape) != (num_heads,):
            raise ValueError(f"rel_pos.{name} must be [H] = [{num_heads}], got {tuple(v.shape)}")
        vals.append(_placed(v.float(), "rel_pos." + name, 4))
    return RelPos(_placed(rel_pos.table.float(), "rel_pos.table", 4), *vals, (gh, gw))


def score_select(qkv: torch.Tensor, num_heads: int, keep: int, eps: float = 1e-6, want_scores: bool = True,
                 num_prefix: int = 1, query: str = "cls", rel_pos: Optional[RelPos] = None):
    """qkv [B, N, 3C] -> (scores [B, N] or None, keep_idx int32 [B, P+keep], next_scores [B, P+keep]), P = `num_prefix`
    as in select_topk (the scores themselves do not depend on P).  `query`: "cls" (row 0) or "mean" (the mean query row);
    P = 0 (a sequence without a class row) goes through rajni_score_select_query with either.
    `rel_pos`: the class row's logits get prefix_q[h] on the patch keys and prefix_qk[h] on the P prefix keys before its softmax
    (rajni_score_select_relpos; keep = 0 gives the scores alone); the class query and P >= 1 only."""
    nat.require_device(qkv, "qkv")
    qkv = _placed(qkv, "qkv")
    B, N, threeC = qkv.shape
    D = threeC // 3 // num_heads
    P = int(num_prefix)
    scores = torch.empty((B, N), dtype=qkv.dtype, device=qkv.device) if want_scores else None
    idx = torch.empty((B, keep + P), dtype=torch.int32, device=qkv.device) if keep > 0 or rel_pos is None else None
    nxt = torch.empty((B, keep + P), dtype=qkv.dtype, device=qkv.device) if keep > 0 or rel_pos is None else None
    if rel_pos is not None:
        if query != "cls" or P == 0:
            raise NotImplementedError("score_select: a relative position bias needs the class query and a class row "
                                      "(the mean importance query has no position)")
        rp = _rel_pos_placed(rel_pos, num_heads)
        ws = _score_scratch(qkv, B, N, num_heads, D)
        with nat.device_guard(qkv.device):
            nat.check(nat.lib().rajni_score_select_relpos(qkv.data_ptr(), B, N, num_heads, D, eps, P, keep, nat.ptr(scores),
                                                          nat.ptr(idx), nat.ptr(nxt), _dt(qkv), nat.ptr(ws),
                                                          ws.numel() if ws is not None else 0, rp.prefix_q.data_ptr(),
                                                          rp.prefix_qk.data_ptr(), nat.stream_ptr(qkv.device)),
                      "rajni_score_select_relpos")
        return scores, idx, nxt
    if query != "cls" or P == 0:
        _score_select_query(qkv, B, N, num_heads, D, eps, P, keep, query, scores, idx, nxt)
        return scores, idx, nxt
    ws = _score_scratch(qkv, B, N, num_heads, D)
    with nat.device_guard(qkv.device):
        if ws is not None:      # more tokens than one workgroup's LDS holds: the tiled kernels, through scratch
            nat.check(nat.lib().rajni_score_select_ws(qkv.data_ptr(), B, N, num_heads, D, eps, P, keep, nat.ptr(scores),
                                                      idx.data_ptr(), nxt.data_ptr(), _dt(qkv), ws.data_ptr(), ws.numel(),
                                                      nat.stream_ptr(qkv.device)), "rajni_score_select_ws")
        elif P == 1:
            nat.check(nat.lib().rajni_score_select(qkv.data_ptr(), B, N, num_heads, D, eps, keep, nat.ptr(scores),
                                                   idx.data_ptr(), nxt.data_ptr(), _dt(qkv),
                                                   nat.stream_ptr(qkv.device)), "rajni_score_select")
        else:
            nat.check(nat.lib().rajni_score_select_prefix(qkv.data_ptr(), B, N, num_heads, D, eps, P, keep, nat.ptr(scores),
                                                          idx.data_ptr(), nxt.data_ptr(), _dt(qkv),
                                                          nat.stream_ptr(qkv.device)), "rajni_score_select_prefix")
    return scores, idx, nxt


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """src [B, N, E], idx [B, K] int32 -> [B, K, E]"""
    nat.require_device(src, "src")
    src = _placed(src, "src")
    idx = _placed(idx.to(torch.int32), "idx", 4)
    B, N, E = src.shape
    K = idx.shape[1]
    out = torch.empty((B, K, E), dtype=src.dtype, device=src.device)
    with nat.device_guard(src.device):
        nat.check(nat.lib().rajni_gather_rows(src.data_ptr(), idx.data_ptr(), out.data_ptr(), B, N, K, E, _dt(src),
                                              nat.stream_ptr(src.device)), "rajni_gather_rows")
    return out


def attention(qkv: torch.Tensor, keep_idx: Optional[torch.Tensor], num_heads: int, scale: float,
              rel_pos: Optional[RelPos] = None, pos: Optional[torch.Tensor] = None, num_prefix: int = 1) -> torch.Tensor:
    """qkv [B, N, 3C]; keep_idx [B, Np] int32 or None -> [B, Np, C].
    `rel_pos`: the bias of include/rajni_hip_relpos.h on the logits (rajni_attention_relpos); `pos` [B, Np] int32 is then the place
    each packed row had in the unpruned sequence (None: the packed row index), the first `num_prefix` places being prefix rows."""
    nat.require_device(qkv, "qkv")
    qkv = _placed(qkv, "qkv")
    B, N, threeC = qkv.shape
    Cc = threeC // 3
    D = Cc // num_heads
    if keep_idx is not None:
        keep_idx = _placed(keep_idx.to(torch.int32), "keep_idx", 4)
        Np = keep_idx.shape[1]
    else:
        Np = N
    out = torch.empty((B, Np, Cc), dtype=qkv.dtype, device=qkv.device)
    if rel_pos is not None:
        rp = _rel_pos_placed(rel_pos, num_heads)
        if pos is not None:
            if tuple(pos.shape) != (B, Np):
                raise ValueError(f"pos must be [B, Np] = [{B}, {Np}], got {tuple(pos.shape)}")
            pos = _placed(pos.to(torch.int32), "pos", 4)
        with nat.device_guard(qkv.device):
            nat.check(nat.lib().rajni_attention_relpos(qkv.data_ptr(), nat.ptr(keep_idx), out.data_ptr(), B, N, Np, num_heads, D,
                                                       float(scale), _dt(qkv), rp.table.data_ptr(), rp.prefix_q.data_ptr(),
                                                       rp.prefix_k.data_ptr(), rp.prefix_qk.data_ptr(), rp.grid[0], rp.grid[1],
                                                       int(num_prefix), nat.ptr(pos), nat.stream_ptr(qkv.device)),
                      "rajni_attention_relpos")
        return out
    if pos is not None:
        raise ValueError("attention: pos without rel_pos")
    with nat.device_guard(qkv.device):
        nat.check(nat.lib().rajni_attention(qkv.data_ptr(), nat.ptr(keep_idx), out.data_ptr(), B, N, Np, num_heads, D,
                                            float(scale), _dt(qkv), nat.stream_ptr(qkv.device)), "rajni_attention")
    return out


def attention_pool(kv: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The attention of timm's AttentionPoolLatent alone (rajni_attention_pool, include/rajni_hip_attnpool.h): kv [B, N, 2C]
    (K half, then V half, each [H][D]) in the model dtype, q [H, D] fp32 with the scale folded in -> [B, C] in kv's dtype.
    fp32 logits, softmax and weighted sum; an image's bits do not depend on the batch."""
    nat.require_device(kv, "kv")
    if kv.dim() != 3 or q.dim() != 2 or kv.shape[2] != 2 * q.shape[0] * q.shape[1]:
        raise ValueError(f"attention_pool: kv must be [B, N, 2 * H * D] and q [H, D], got {tuple(kv.shape)} and {tuple(q.shape)}")
    if q.dtype != torch.float32:
        raise ValueError(f"attention_pool: q must be float32 (the pre-scaled query), got {q.dtype}")
    kv, q = _placed(kv, "kv"), _placed(q.to(kv.device), "q")
    B, N, _ = kv.shape
    H, D = q.shape
    out = torch.empty((B, H * D), dtype=kv.dtype, device=kv.device)
    with nat.device_guard(kv.device):
        nat.check(nat.lib().rajni_attention_pool(kv.data_ptr(), q.data_ptr(), out.data_ptr(), B, N, H, D, _dt(kv),
                                                 nat.stream_ptr(kv.device)), "rajni_attention_pool")
    return out


def attention_out_scale(norm1_w: torch.Tensor, norm1_b: torch.Tensor, wv: torch.Tensor, bv: Optional[torch.Tensor]) -> float:
    """out_scale of `attention_fp8` from a block's parameters (the bound of rajni_attention_fp8, include/rajni_hip.h):
    (1.0625 * (sqrt(C) * max|gamma1| + ||beta1||_2) * max_c ||Wv[c]||_2 + max|bv|) / 448, evaluated in fp32.
    `wv` are the V rows of the qkv weight AS THE KERNELS HOLD THEM (dequantised e4m3), [C, C]."""
    g, b = norm1_w.detach().to(torch.float32), norm1_b.detach().to(torch.float32)
    w32 = wv.detach().to(torch.float32)
    c = torch.tensor(float(w32.shape[1]), dtype=torch.float32).sqrt()
    bound = torch.tensor(1.0625, dtype=torch.float32) * (c * g.abs().max().cpu() + b.norm().cpu()) * w32.norm(dim=1).max().cpu()
    if bv is not None:
        bound = bound + bv.detach().to(torch.float32).abs().max().cpu()
    return float(bound / torch.tensor(448.0, dtype=torch.float32))


def attention_fp8(qkv: torch.Tensor, keep_idx: Optional[torch.Tensor], num_heads: int, scale: float, out_scale: float):
    """attention with e4m3 output rows (opt-in fp8_mfma format): qkv bf16 [B, N, 3C], head dim 64, at most 224 kept tokens
    -> (bytes uint8 [B, Np, C] = e4m3_rne_sat(attn / out_scale), row scales fp32 [B * Np] = out_scale)"""
    nat.require_device(qkv, "qkv")
    qkv = _placed(qkv, "qkv")
    B, N, threeC = qkv.shape
    Cc = threeC // 3
    D = Cc // num_heads
    if keep_idx is not None:
        keep_idx = _placed(keep_idx.to(torch.int32), "keep_idx", 4)
        Np = keep_idx.shape[1]
    else:
        Np = N
    out = torch.empty((B, Np, Cc), dtype=torch.uint8, device=qkv.device)
    rs = torch.empty(B * Np, dtype=torch.float32, device=qkv.device)
    with nat.device_guard(qkv.device):
        nat.check(nat.lib().rajni_attention_fp8(qkv.data_ptr(), nat.ptr(keep_idx), out.data_ptr(), float(out_scale), rs.data_ptr(),
                                                B, N, Np, num_heads, D, float(scale), nat.stream_ptr(qkv.device)),
                  "rajni_attention_fp8")
    return out, rs


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, rows: Optional[int] = None,
              row_stride: Optional[int] = None, out_dtype=torch.bfloat16) -> torch.Tensor:
    """LayerNorm over the last axis; w, b fp32.  x may be `out_dtype` or fp32 (the fp32 residual
    stream); the result is `out_dtype`.  With rows/row_stride reads a strided subset of rows."""
    nat.require_device(x, "x")
    x, w, b = _placed(x, "x"), _placed(w, "w"), _placed(b, "b")
    x_f32 = int(x.dtype == torch.float32 and out_dtype != torch.float32)
    Cc = x.shape[-1]
    if rows is None:
        rows = x.numel() // Cc
        row_stride = Cc
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    else:
        out = torch.empty((rows, Cc), dtype=out_dtype, device=x.device)
    with nat.device_guard(x.device):
        nat.check(nat.lib().rajni_layernorm(x.data_ptr(), row_stride, w.data_ptr(), b.data_ptr(), out.data_ptr(), rows,
                                            Cc, float(eps), nat.dtype_code(out_dtype), x_f32,
                                            nat.stream_ptr(x.device)), "rajni_layernorm")
    return out


def layernorm_fp8(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float,
                  hidden_bound: Optional[Tuple[float, float]] = None):
    """LayerNorm over the last axis with the output row quantised for the fp8 matrix pipe (rajni_layernorm_fp8):
    returns (q uint8 [..., C] of e4m3 bytes, scale fp32 [rows]) and, with `hidden_bound = (max row norm of the
    dequantised fc1 weight, max |fc1 bias|)`, also the per-row scale of the MLP hidden activations."""
    nat.require_device(x, "x")
    x, w, b = _placed(x, "x"), _placed(w, "w"), _placed(b, "b")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("layernorm_fp8: x must be fp32 (the residual stream) or bf16")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    hs = torch.empty(rows, dtype=torch.float32, device=x.device) if hidden_bound is not None else None
    wn, bm = (float(hidden_bound[0]), float(hidden_bound[1])) if hidden_bound is not None else (0.0, 0.0)
    with nat.device_guard(x.device):
        nat.check(nat.lib().rajni_layernorm_fp8(x.data_ptr(), Cc, w.data_ptr(), b.data_ptr(), q.data_ptr(), scale.data_ptr(),
                                                nat.ptr(hs), wn, bm, rows, Cc, float(eps), int(x.dtype == torch.float32),
                                                nat.stream_ptr(x.device)), "rajni_layernorm_fp8")
    return (q, scale) if hs is None else (q, scale, hs)


def qk_norm(qkv: torch.Tensor, num_heads: int, q_w: torch.Tensor, q_b: Optional[torch.Tensor], k_w: torch.Tensor,
            k_b: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """timm's `q, k = q_norm(q), k_norm(k)`: LayerNorm over the head dim of the q and k thirds of qkv [..., 3C], IN PLACE
    (v is not touched); q_w / k_w fp32 [D], biases fp32 [D] or None.  Returns qkv."""
    nat.require_device(qkv, "qkv")
    if not qkv.is_contiguous():
        raise ValueError("qk_norm works in place: qkv must be contiguous")
    qkv = _placed(qkv, "qkv", in_place=True)
    threeC = qkv.shape[-1]
    rows = qkv.numel() // threeC
    D = threeC // 3 // num_heads
    for v in (q_w, q_b, k_w, k_b):
        if v is not None and (v.dtype != torch.float32 or v.numel() != D or not v.is_contiguous()):
            raise ValueError(f"qk_norm: weights and biases must be contiguous fp32 [{D}]")
    q_w, q_b, k_w, k_b = _placed(q_w, "q_w"), _placed(q_b, "q_b"), _placed(k_w, "k_w"), _placed(k_b, "k_b")
    with nat.device_guard(qkv.device):
        nat.check(nat.lib().rajni_qk_norm(qkv.data_ptr(), q_w.data_ptr(), nat.ptr(q_b), k_w.data_ptr(), nat.ptr(k_b), rows,
                                          num_heads, D, float(eps), _dt(qkv), nat.stream_ptr(qkv.device)), "rajni_qk_norm")
    return qkv


def rope_qk(qkv: torch.Tensor, num_heads: int, cos: torch.Tensor, sin: torch.Tensor, num_prefix: int = 1,
            src: Optional[torch.Tensor] = None, half: bool = False) -> torch.Tensor:
    """Rotary position embedding of the q and k thirds of qkv [B, N, 3C], IN PLACE (v and the first `num_prefix` rows of every
    image are not touched; include/rajni_hip_rope.h).  cos / sin: fp32 [rows, D] (one table for all heads) or [H, rows, D],
    one row per patch of the grid.  Row t >= num_prefix of image b takes table row (src[b, t] if src is given else t) -
    num_prefix; `src` int32 [B, N] is checked here against the tables' rows (the native entry point does not).  `half`:
    rotate_half pairs (j, j + D/2) instead of timm rot()'s (2i, 2i + 1).  Returns qkv.  (With `src` the check reads its extremes back:
    one host synchronisation per call - a stand-alone op's price; the whole forward composes its own map and has none.)"""
    nat.require_device(qkv, "qkv")
    if qkv.dim() != 3:
        raise ValueError(f"rope_qk: qkv must be [B, N, 3C], got {tuple(qkv.shape)}")
    qkv = _placed(qkv, "qkv", in_place=True)
    B, N, threeC = qkv.shape
    if num_heads < 1 or threeC % (3 * num_heads):
        raise ValueError(f"rope_qk: qkv's last axis ({threeC}) must be 3 * num_heads * head_dim with num_heads = {num_heads}")
    D = threeC // 3 // num_heads
    if cos.shape != sin.shape or cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.dim() not in (2, 3) \
            or cos.shape[-1] != D or (cos.dim() == 3 and cos.shape[0] != num_heads):
        raise ValueError(f"rope_qk: cos and sin must be fp32 [rows, {D}] or [{num_heads}, rows, {D}] of one shape, got "
                         f"{tuple(cos.shape)} / {tuple(sin.shape)}")
    rows = cos.shape[-2]
    if src is None:
        if N - num_prefix > rows:
            raise ValueError(f"rope_qk: {N - num_prefix} patch rows but the tables have {rows}")
    else:
        if src.dtype != torch.int32 or tuple(src.shape) != (B, N):
            raise ValueError(f"rope_qk: src must be int32 [{B}, {N}]")
        p = src[:, num_prefix:]
        if p.numel() and (int(p.min()) < num_prefix or int(p.max()) >= num_prefix + rows):
            raise ValueError(f"rope_qk: src names positions outside the tables' {rows} rows")
    cos, sin, src = _placed(cos, "cos"), _placed(sin, "sin"), _placed(src, "src", 4)
    with nat.device_guard(qkv.device):
        nat.check(nat.lib().rajni_rope_qk(qkv.data_ptr(), nat.ptr(src), cos.data_ptr(), sin.data_ptr(),
                                          rows * D if cos.dim() == 3 else 0, B, N, num_prefix, num_heads, D,
                                          nat.ROPE_HALF if half else nat.ROPE_INTERLEAVED, _dt(qkv), nat.stream_ptr(qkv.device)),
                  "rajni_rope_qk")
    return qkv


def hidden_norm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float, n: Optional[int] = None,
                rms: bool = False) -> torch.Tensor:
    """The norm inside an MLP (include/rajni_hip_mlpnorm.h), IN PLACE on x [rows, ld] (bf16 / fp16 / fp32): columns [0, n) of
    every row become LayerNorm (`rms`: RMSNorm, b not read) of those n columns with fp32 w / b [n] (b None = 0); the divisor of
    the statistics is n.  `n` defaults to w's length; columns [n, ld) are the zero padding of the hidden buffer and must hold
    zeros - they hold zeros afterwards.  ld % 8 == 0, n <= HIDDEN_NORM_MAX.  Returns x."""
    nat.require_device(x, "x")
    if x.dim() != 2:
        raise ValueError(f"hidden_norm: x must be [rows, ld], got {tuple(x.shape)}")
    x = _placed(x, "x", in_place=True)
    rows, ld = x.shape
    n = int(w.numel()) if n is None else int(n)
    if w.dtype != torch.float32 or w.dim() != 1 or w.numel() != n or (b is not None and (b.dtype != torch.float32 or b.shape != w.shape)):
        raise ValueError(f"hidden_norm: w and b must be fp32 [{n}]")
    w, b = _placed(w, "w"), _placed(b, "b")
    with nat.device_guard(x.device):
        nat.check(nat.lib().rajni_hidden_norm(nat.NORM_RMS if rms else nat.NORM_LAYERNORM, x.data_ptr(), ld, w.data_ptr(), nat.ptr(b),
                                              rows, n, float(eps), _dt(x), 0, nat.stream_ptr(x.device)), "rajni_hidden_norm")
    return x


def layernorm_stream(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float,
                     model_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """timm's `x = norm_pre(x)`: LayerNorm over the last axis written back IN PLACE into the residual stream x (fp32, or the
    model's 16-bit type).  `model_dtype` is the model's dtype when x is its fp32 stream (default: x's own).  Returns x."""
    nat.require_device(x, "x")
    if not x.is_contiguous():
        raise ValueError("layernorm_stream works in place: x must be contiguous")
    x, w, b = _placed(x, "x", in_place=True), _placed(w, "w"), _placed(b, "b")
    Cc = x.shape[-1]
    dt = nat.dtype_code(model_dtype if model_dtype is not None else x.dtype)
    x_f32 = int(x.dtype == torch.float32 and dt != nat.RAJNI_F32)
    if not x_f32 and nat.dtype_code(x.dtype) != dt:
        raise ValueError("layernorm_stream: x must be fp32 or the model dtype")
    with nat.device_guard(x.device):
        nat.check(nat.lib().rajni_layernorm_stream(x.data_ptr(), w.data_ptr(), nat.ptr(b), x.numel() // Cc, Cc, float(eps), dt,
                                                   x_f32, nat.stream_ptr(x.device)), "rajni_layernorm_stream")
    return x


def pool_norm(x: torch.Tensor, pool: str = "token", norm=None, fc_norm=None, out_dtype=torch.bfloat16,
              num_prefix: int = 1) -> torch.Tensor:
    """timm's head input: fc_norm(pool(norm(x))) for x [B, N, C] (`out_dtype`, or fp32 = the fp32 residual stream) -> [B, C]
    in `out_dtype`.  pool: "token" (x[:, 0]) or "avg" (mean of x[:, num_prefix:]); norm / fc_norm: (w, b or None, eps) or None."""
    nat.require_device(x, "x")
    if pool not in ("token", "avg"):
        raise NotImplementedError(f"pool_norm: pool '{pool}' is not supported ('token' or 'avg')")
    x = _placed(x, "x")
    B, N, Cc = x.shape
    x_f32 = int(x.dtype == torch.float32 and out_dtype != torch.float32)
    nw, nb, ne = norm if norm is not None else (None, None, 0.0)
    fw, fb, fe = fc_norm if fc_norm is not None else (None, None, 0.0)
    nw, nb, fw, fb = _placed(nw, "norm_w"), _placed(nb, "norm_b"), _placed(fw, "fc_w"), _placed(fb, "fc_b")
    out = torch.empty((B, Cc), dtype=out_dtype, device=x.device)
    pk = nat.POOL_AVG if pool == "avg" else nat.POOL_TOKEN
    with nat.device_guard(x.device):
        if int(num_prefix) == 1:
            nat.check(nat.lib().rajni_pool_norm(x.data_ptr(), B, N, Cc, pk,
                                                nat.ptr(nw), nat.ptr(nb), float(ne), nat.ptr(fw), nat.ptr(fb), float(fe),
                                                out.data_ptr(), nat.dtype_code(out_dtype), x_f32, nat.stream_ptr(x.device)),
                      "rajni_pool_norm")
        else:
            nat.check(nat.lib().rajni_pool_norm_prefix(x.data_ptr(), B, N, int(num_prefix), Cc, pk,
                                                       nat.ptr(nw), nat.ptr(nb), float(ne), nat.ptr(fw), nat.ptr(fb), float(fe),
                                                       out.data_ptr(), nat.dtype_code(out_dtype), x_f32,
                                                       nat.stream_ptr(x.device)), "rajni_pool_norm_prefix")
    return out


def linear(x: torch.Tensor, w_packed: torch.Tensor, n_out: int, bias: Optional[torch.Tensor] = None,
           epilogue: int = nat.EPI_BIAS, gamma: Optional[torch.Tensor] = None,
           resid: Optional[torch.Tensor] = None, r_idx: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, w_scale: Optional[torch.Tensor] = None,
           x_scale: Optional[torch.Tensor] = None, y_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epi(x @ W^T): x [..., K]; w_packed from pack_weight(); bias/gamma fp32 [n_out].
    With `w_scale` (fp32 [n_out]) w_packed is the uint8 e4m3 tensor of pack_weight_fp8() and x is bf16.
    resid [B, N_src, n_out] (+ r_idx [B, Np] int32 to gather its rows) for EPI_BIAS_RESID; an fp32
    resid selects the fp32 residual stream (the output is then fp32 too).
    With `x_scale` (fp32 [M]) x is the uint8 e4m3 tensor of layernorm_fp8() and the product runs on the fp8 matrix
    pipe (w_scale required); with EPI_BIAS_GELU `y_scale` (fp32 [M]) is required and the result is uint8 e4m3.
    EPI_BIAS_QUICK_GELU (x * sigmoid(1.702 x)) is EPI_BIAS_GELU with the other function, for every format but `x_scale`
    (NotImplementedError from the library).
    EPI_BIAS_SWIGLU is the gated FC1, y [.., n_out] = silu(x Wg^T + bg) * (x Wv^T + bv): w_packed is pack_weight() of the
    [2 n_out, K] weight whose rows [0, n_out) are the gates and [n_out, 2 n_out) the values (timm's packed order), bias and
    w_scale are [2 n_out] in the same order.  Every format but `x_scale`, like QuickGELU."""
    nat.require_device(x, "x")
    x, w_packed = _placed(x, "x"), _placed(w_packed, "w")
    bias, gamma, w_scale = _placed(bias, "bias"), _placed(gamma, "gamma"), _placed(w_scale, "w_scale")
    x_scale, y_scale = _placed(x_scale, "x_scale", 4), _placed(y_scale, "y_scale", 4)
    K = x.shape[-1]
    M = x.numel() // K
    f8 = x_scale is not None
    if f8 and (x.dtype != torch.uint8 or w_scale is None):
        raise ValueError("x_scale needs the uint8 e4m3 activations of layernorm_fp8() and fp8 weights (w_scale)")
    act_dtype = torch.bfloat16 if f8 else x.dtype
    out8 = f8 and epilogue == nat.EPI_BIAS_GELU
    ld = (n_out + 15) // 16 * 16 if out8 else (n_out + 7) // 8 * 8
    stream_f32 = int(resid is not None and resid.dtype == torch.float32 and act_dtype != torch.float32)
    if out is not None:
        if out.data_ptr() % 16:
            raise ValueError("y must be 16-byte aligned (a caller's `out` is written in place and cannot be copied)")
    else:
        out = torch.empty((M, ld), dtype=torch.uint8 if out8 else (torch.float32 if stream_f32 else act_dtype), device=x.device)
    a = nat.LinearArgs()
    a.x, a.lda, a.w, a.ldw = x.data_ptr(), K, w_packed.data_ptr(), w_packed.shape[1]
    a.bias, a.gamma, a.w_scale = nat.ptr(bias), nat.ptr(gamma), nat.ptr(w_scale)
    if w_scale is not None and w_packed.dtype != torch.uint8:
        raise ValueError("w_scale given but w_packed is not the uint8 tensor of pack_weight_fp8()")
    a.y, a.ldc = out.data_ptr(), out.shape[-1] if out.dim() == 2 else out.stride(-2)
    a.M, a.N, a.K, a.epilogue, a.dtype, a.stream_f32 = M, n_out, K, epilogue, nat.dtype_code(act_dtype), stream_f32
    a.x_scale, a.y_scale = nat.ptr(x_scale), nat.ptr(y_scale)
    if resid is not None:
        resid = _placed(resid, "resid")
        a.resid, a.ldr = resid.data_ptr(), resid.shape[-1]
        if r_idx is not None:
            r_idx = _placed(r_idx.to(torch.int32), "r_idx", 4)
            a.r_idx, a.r_np, a.r_nsrc = r_idx.data_ptr(), r_idx.shape[1], resid.shape[1]
    with nat.device_guard(x.device):
        nat.check(nat.lib().rajni_linear(C.byref(a), nat.stream_ptr(x.device)), "rajni_linear")
    y = out[:, :n_out] if ld != n_out else out
    return y.reshape(*x.shape[:-1], n_out) if ld == n_out else y


def patch_embed(images: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, cls: torch.Tensor,
                pos: torch.Tensor, pos_has_cls: bool, patch: int, embed_dim: int,
                out_f32: bool = False, reg: Optional[torch.Tensor] = None, size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """images [B, Cin, S, S] -> x [B, P + (S/patch)^2, C]: CLS, the R = P - 1 register tokens `reg` ([R, C] in the images'
    dtype, None = no registers), then the patches; `pos` has (P if pos_has_cls else 0) + (S/patch)^2 rows.
    With `size=(H, W)` the images are [B, Cin, H, W] (rajni_patch_embed_image): (H/patch) * (W/patch) patches, row-major."""
    nat.require_device(images, "images")
    images, w_packed, bias = _placed(images, "images"), _placed(w_packed, "w"), _placed(bias, "bias")
    cls, pos = _placed(cls, "cls"), _placed(pos, "pos")
    B, Cin, S, Wd = images.shape
    if size is None and S != Wd:
        raise ValueError(f"patch_embed: images [B, Cin, S, S] expected, got {tuple(images.shape)}; pass size=(H, W) for a rectangle")
    if size is not None and (int(size[0]), int(size[1])) != (S, Wd):
        raise ValueError(f"patch_embed: size={tuple(size)} but the images are {tuple(images.shape)}")
    if reg is not None:
        if reg.dim() != 2 or reg.shape[1] != embed_dim or reg.shape[0] < 1 or reg.dtype != images.dtype:
            raise ValueError(f"patch_embed: reg must be [R, {embed_dim}] in the images' dtype, got {tuple(reg.shape)} {reg.dtype}")
        reg = _placed(reg, "reg")
    P = 1 + (reg.shape[0] if reg is not None else 0)
    n = (S // patch) * (Wd // patch) + P
    x = torch.empty((B, n, embed_dim), dtype=torch.float32 if out_f32 else images.dtype, device=images.device)
    kpad = (Cin * patch * patch + 63) // 64 * 64
    if w_packed.shape[1] != kpad:
        raise ValueError(f"patch_embed: weight must be packed with k_multiple=64 ([*, {kpad}]), got {tuple(w_packed.shape)}")
    # 0: im2col fused into the loads
    nbytes = (nat.lib().rajni_patch_embed_workspace_bytes(B, Cin, S, patch, _dt(images)) if size is None
              else nat.lib().rajni_patch_embed_workspace_bytes_image(B, Cin, S, Wd, patch, _dt(images)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=images.device) if nbytes else None
    with nat.device_guard(images.device):
        if size is not None:
            nat.check(nat.lib().rajni_patch_embed_image(images.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), cls.data_ptr(),
                                                        nat.ptr(reg), P, pos.data_ptr(), int(pos_has_cls), x.data_ptr(),
                                                        int(out_f32), B, Cin, S, Wd, patch, embed_dim, _dt(images), nat.ptr(ws),
                                                        nbytes, nat.stream_ptr(images.device)), "rajni_patch_embed_image")
        elif reg is None:
            nat.check(nat.lib().rajni_patch_embed(images.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), cls.data_ptr(),
                                                  pos.data_ptr(), int(pos_has_cls), x.data_ptr(), int(out_f32), B, Cin, S, patch,
                                                  embed_dim, _dt(images), nat.ptr(ws), nbytes, nat.stream_ptr(images.device)),
                      "rajni_patch_embed")
        else:
            nat.check(nat.lib().rajni_patch_embed_prefix(images.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), cls.data_ptr(),
                                                         reg.data_ptr(), P, pos.data_ptr(), int(pos_has_cls), x.data_ptr(),
                                                         int(out_f32), B, Cin, S, patch, embed_dim, _dt(images), nat.ptr(ws),
                                                         nbytes, nat.stream_ptr(images.device)), "rajni_patch_embed_prefix")
    return x


def resample_pos_embed(pos: torch.Tensor, src_grid: Tuple[int, int], dst_grid: Tuple[int, int], prefix_rows: int = 0,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """timm's resample_abs_pos_embed (rajni_resample_pos_embed): pos [prefix_rows + sh * sw, C] -> [prefix_rows + dh * dw, C]
    in pos's dtype; the prefix rows are copied, the patch rows go fp32 -> bicubic with antialiasing -> one rounding.  Equal
    grids return the source's bits.  `out` (contiguous, 16-byte aligned, the result's shape and dtype) is written in place."""
    nat.require_device(pos, "pos")
    (sh, sw), (dh, dw), pr = (int(v) for v in src_grid), (int(v) for v in dst_grid), int(prefix_rows)
    if pos.dim() != 2 or pos.shape[0] != pr + sh * sw:
        raise ValueError(f"resample_pos_embed: pos must be [{pr} + {sh} * {sw}, C], got {tuple(pos.shape)}")
    pos = _placed(pos, "pos")
    Cc = pos.shape[1]
    if out is None:
        out = torch.empty((pr + dh * dw, Cc), dtype=pos.dtype, device=pos.device)
    else:
        if tuple(out.shape) != (pr + dh * dw, Cc) or out.dtype != pos.dtype or out.device != pos.device:
            raise ValueError(f"resample_pos_embed: out must be [{pr + dh * dw}, {Cc}] {pos.dtype} on {pos.device}")
        out = _placed(out, "out", in_place=True)
    with nat.device_guard(pos.device):
        nat.check(nat.lib().rajni_resample_pos_embed(pos.data_ptr(), sh, sw, out.data_ptr(), dh, dw, Cc, pr, _dt(pos),
                                                     nat.stream_ptr(pos.device)), "rajni_resample_pos_embed")
    return out
