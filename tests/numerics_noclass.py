"""Yardsticks for the mean importance query and for models without a class token (timm `class_token=False`,
`global_pool='avg'`; include/rajni_hip_query.h), pure numpy / torch-CPU, shared by tests/test_noclass_cpu.py and the
tests/test_gpu_noclass_*.py files.

The reference cannot run such a model (its model.py:35 expands cls_token), so the rule is the project's own, restated here:
  qbar[b, h, :] = (1 / N) sum_n q[b, h, n, :] over the N tokens of the block's current sequence (prefix tokens included);
  A[b, n] = mean_h softmax_n(qbar[b, h] . k[b, h, n] / sqrt(D)); everything else is oracle.rajni_oracle.importance_scores;
  token order [reg_0 .. reg_{R-1}, patch_0 .. patch_{n-1}], P = R prefix tokens (0 allowed) that are always kept and never
  ranked - tests/numerics_prefix.py::select_tokens and ::keep_count as they stand; 'avg' pooling is the mean of rows P..N-1."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import rajni_oracle as orc
import numerics as nm
import numerics_prefix as npx
from numerics_variants import _t, _ln

QUERY_KINDS = ["qoffset", "qcancel"]


def importance_scores(qkv, num_heads, eps=1e-6, dtype=np.float64, query="mean"):
    """oracle.rajni_oracle.importance_scores with the query named: "cls" is that function operation for operation (row 0),
    "mean" puts the mean of the N query rows, taken in `dtype`, in row 0's place"""
    qkv = np.asarray(qkv, dtype=dtype)
    B, N, threeC = qkv.shape
    C = threeC // 3
    D = C // num_heads
    t = qkv.reshape(B, N, 3, num_heads, D)
    if query == "cls":
        q = t[:, 0, 0]
    elif query == "mean":
        q = t[:, :, 0].mean(axis=1)           # [B,H,D]
    else:
        raise ValueError(query)
    k = t[:, :, 1]
    v = t[:, :, 2]
    logits = np.einsum("bhd,bnhd->bhn", q, k) / math.sqrt(D)
    logits = logits - logits.max(axis=-1, keepdims=True)
    e = np.exp(logits)
    attn = e / e.sum(axis=-1, keepdims=True)
    a = attn.mean(axis=1)
    vbar = v.mean(axis=2)
    vbar = vbar - vbar.mean(axis=1, keepdims=True)
    vnorm = np.sqrt((vbar * vbar).sum(axis=-1))
    mu = vnorm.mean(axis=1, keepdims=True)
    std = np.sqrt(((vnorm - mu) ** 2).sum(axis=1, keepdims=True) / (N - 1)) + eps
    z = (vnorm - mu) / std
    return a * (1.0 / (1.0 + np.exp(-z)))


def query_qkv(kind, B, N, H, D, dt, seed=0):
    """the query's own stress inputs (K and V standard normal):
    qoffset   Q = 50 + 0.5 n: the mean dominates every row and the softmax of qbar . k is peaked
    qcancel   Q rows alternate +r and -r (r one row of 3 n) + 0.02 n: the mean cancels two digits"""
    rng = np.random.default_rng([seed, B, N, H, D, 40 + QUERY_KINDS.index(kind)])
    t = rng.standard_normal((B, N, 3, H, D), dtype=np.float32)
    if kind == "qoffset":
        t[:, :, 0] = 50.0 + 0.5 * t[:, :, 0]
    else:
        r = 3.0 * rng.standard_normal((B, 1, H, D), dtype=np.float32)
        sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.float32)
        t[:, :, 0] = sign[None, :, None, None] * r + 0.02 * t[:, :, 0]
    return nm.round_to(t.reshape(B, N, 3 * H * D), dt)


def fixture_qkv(seed, j, B, N, H, D):
    """qkv of case j of tests/golden/noclass_importance (make_golden_noclass.py): fp32, K and V standard normal, every Q row of
    an image the same row of integer multiples of 2^-6 in [-4, 4] - the mean query IS row 0, exactly, in any summation order
    (N a power of two)"""
    rng = np.random.default_rng([seed, j])
    t = rng.standard_normal((B, N, 3, H, D), dtype=np.float32)
    t[:, :, 0] = rng.integers(-256, 257, size=(B, 1, H, D)).astype(np.float32) / np.float32(64.0)
    return t.reshape(B, N, 3 * H * D)


def load_fixture():
    """[(case dict, qkv fp32, the reference's scores fp32)] - the stored qkv checked against the recipe"""
    import json
    import os
    from helpers import GOLDEN
    with open(os.path.join(GOLDEN, "noclass_importance.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "noclass_importance.npz"))
    out = []
    for j, c in enumerate(meta["cases"]):
        qkv = fixture_qkv(meta["seed"], j, c["B"], c["N"], c["H"], c["D"])
        if c["stored_qkv"]:
            np.testing.assert_array_equal(qkv, data[f"c{j}.qkv"])
        out.append((c, qkv, data[f"c{j}.scores"]))
    return out


NORMAL_RANGE = 2.0 ** -80


def importance_budget_normal_range(qkv, H, dt, eps=1e-6, query="mean"):
    """(mask, budget): importance_budget with e32 taken over the elements whose score is at least 2^-80 only, for those
    elements.  e32 is ONE number for the whole tensor; on `qoffset` (logits spread over +-150) most scores lie below the fp32
    range, the fp32 run flushes them to 0 - a relative error of 1 - and (u_out + 4 x 1) |want| no longer says anything about
    the tokens that carry the softmax.  Above 2^-80 every fp32 intermediate of the rule is a normal number, so the fp32 run's
    error there is the arithmetic's and not the format's range; the mean query's derived term is added as it stands."""
    want, bud, e32 = importance_budget(qkv, H, dt, eps, query)
    mask = np.abs(want) >= NORMAL_RANGE
    s32 = importance_scores(qkv, H, eps, dtype=np.float32, query=query).astype(np.float64)
    e32n = float((np.abs(s32 - want)[mask] / np.abs(want)[mask]).max())
    return mask, bud - 4 * (e32 - e32n) * np.abs(want), e32n


def importance_budget(qkv, H, dt, eps=1e-6, query="mean"):
    """(want, budget, e32): numerics.importance_budget for the named query - |err| <= (u_out + 4 e32) |want| + floor, e32 the
    largest relative error of the restatement's fp32 run (fp32 mean included) against its fp64 run - plus, for the mean query,
    a derived term.  The fp32 run takes the mean by numpy's pairwise sum, whose error grows like log N; a kernel that sums N
    rows in another fixed order may legitimately be off by the worst case of ANY order,
        |d qbar[c]| <= (N + 1) 2^-24 mean_n |q[n, c]|      (N - 1 adds, the 1 / N and the multiply by it),
    which on `qoffset` and `qcancel` is far above what e32 happens to see.  It is carried to the logits of head h as
    dl[h] = max_n sum_c |d qbar[c]| |k[n, c]| / sqrt(D); a softmax whose logits move by at most dl moves by at most
    (exp(2 dl) - 1) p relatively, so the term is sigmoid(z) mean_h((exp(2 dl[h]) - 1) p[h, n]).  The factor 4 stays 4."""
    want = importance_scores(qkv, H, eps, query=query)
    s32 = importance_scores(qkv, H, eps, dtype=np.float32, query=query).astype(np.float64)
    e32 = float((np.abs(s32 - want) / np.abs(want)).max())
    bud = (nm.UNIT[dt] + 4 * e32) * np.abs(want) + nm.FLOOR[dt]
    if query == "mean":
        q64 = np.asarray(qkv, np.float64)
        B, N, threeC = q64.shape
        D = threeC // 3 // H
        t = q64.reshape(B, N, 3, H, D)
        dq = (N + 1) * nm.U32 * np.abs(t[:, :, 0]).mean(axis=1)                               # [B,H,D]
        dl = (np.einsum("bhd,bnhd->bhn", dq, np.abs(t[:, :, 1])) / math.sqrt(D)).max(axis=-1)   # [B,H]
        logits = np.einsum("bhd,bnhd->bhn", t[:, :, 0].mean(axis=1), t[:, :, 1]) / math.sqrt(D)
        p = np.exp(logits - logits.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        a = p.mean(axis=1)
        sig = want / a
        bud = bud + sig * (np.expm1(2 * dl)[:, :, None] * p).mean(axis=1)
    return want, bud, e32


# ---- the forward ---------------------------------------------------------------------------------------------------------------

def pos_embedded_tokens(sd, patches, cfg, dtype):
    """timm _pos_embed with or without a class token: patches [B, n, C] torch -> [B, P + n, C]"""
    B = patches.shape[0]
    prefix = []
    if cfg.class_token:
        prefix.append(_t(sd["cls_token"], dtype).expand(B, -1, -1))
    if cfg.reg_tokens:
        prefix.append(_t(sd["reg_token"], dtype).expand(B, -1, -1))
    pos = _t(sd["pos_embed"], dtype)
    if cfg.no_embed_class:
        return torch.cat(prefix + [patches + pos], 1)
    return torch.cat(prefix + [patches], 1) + pos


def default_query(cfg):
    return "cls" if cfg.class_token else "mean"


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, query=None, features=None,
                         budget_dt=None):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx / next_scores}) of the pruned graph of a model
    with or without a class token: tests/numerics_prefix.py::vit_forward_restated with P = cfg.num_prefix_tokens and the
    importance query named (default: "cls" with a class token, "mean" without).  `features`: instead of the logits,
    "tokens" returns norm(x) of the surviving tokens [B, Nf, C]; "states" returns (that, {block: stream behind it [B, N_i, C]}).
    `budget_dt`: the trace also holds "budget", importance_budget's for that output type on the scores each block ranks (a
    carried stage inherits the budget with the scores)."""
    schedule = orc.normalise_schedule(schedule)
    query = query or default_query(cfg)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()      # (a 16-bit run: fp32 arrays out)
    Pn = cfg.num_prefix_tokens
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = pos_embedded_tokens(sd, x, cfg, dtype)
    if cfg.pre_norm:
        x = _ln(x, sd, "norm_pre", eps, dtype)
    scores, counts, trace, states, bud, full_bud = None, [], {}, {}, None, None
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _ln(x, sd, p + "norm1", eps, dtype)
        qkv = (xn @ W(p + "attn.qkv.weight").T + W(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                flat = host(torch.stack([q, k, v], 2).reshape(B, N, 3 * C))
                full = importance_scores(flat, H, dtype=np_dt, query=query)
                if budget_dt:
                    full_bud = importance_budget(flat, H, budget_dt, query=query)[1]
            else:
                full, full_bud = scores, bud
            keep = npx.keep_count(sc["keep_ratio"], N, Pn)
            keep_idx = npx.select_tokens(full, keep, Pn) if forced_keep is None or i not in forced_keep \
                else np.asarray(forced_keep[i], np.int64)
            assert keep_idx.shape == (B, Pn + keep)
            scores = np.take_along_axis(full, keep_idx, axis=1)
            trace[i] = {"scores": full, "keep_idx": keep_idx, "next_scores": scores}
            if budget_dt:
                trace[i]["budget"] = full_bud
                bud = np.take_along_axis(full_bud, keep_idx, axis=1)
            gi = torch.from_numpy(keep_idx)[:, :, None, None].expand(-1, -1, H, D)
            q, k, v = q.gather(1, gi), k.gather(1, gi), v.gather(1, gi)
            x = x.gather(1, torch.from_numpy(keep_idx)[:, :, None].expand(-1, -1, C))
        else:
            scores = None
        att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5, dim=-1)
        out = torch.einsum("bhqk,bkhd->bqhd", att, v).reshape(B, -1, C)
        out = out @ W(p + "attn.proj.weight").T + W(p + "attn.proj.bias")
        x = x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = _ln(x, sd, p + "norm2", eps, dtype)
        h = torch.nn.functional.gelu(h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias"))
        h = h @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias")
        x = x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
        states[i] = x
    if "norm.weight" in sd:
        x = _ln(x, sd, "norm", eps, dtype)
    if features == "tokens":
        return host(x), counts, trace
    if features == "states":
        return (host(x), states), counts, trace
    x = x[:, Pn:].mean(1) if cfg.global_pool == "avg" else x[:, 0]
    if cfg.use_fc_norm:
        x = _ln(x, sd, "fc_norm", eps, dtype)
    logits = x @ W("head.weight").T + W("head.bias")
    return host(logits), counts, trace


def scatter_dense(rows, src, n0):
    """rows [B, Nf, C] numpy at the positions src [B, Nf] of a zero [B, n0, C]"""
    out = np.zeros((rows.shape[0], n0, rows.shape[2]), rows.dtype)
    np.put_along_axis(out, src[:, :, None], rows, axis=1)
    return out


def source_idx(trace, B, n0, upto=None):
    """where each token of the stream behind block `upto` (None: the final stream) sat in the unpruned sequence"""
    src = np.tile(np.arange(n0), (B, 1))
    for i in sorted(trace):
        if upto is None or i <= upto:
            src = np.take_along_axis(src, trace[i]["keep_idx"], axis=1)
    return src


def feature_outputs(sd, images, schedule, cfg, forced_keep=None, caps=(), dtype=torch.float64, query=None):
    """What the feature surfaces return, restated: dict(tokens [B, Nf, C]; source_idx [B, Nf]; dense (pruned rows zero);
    dense_last (a token scheduled block i drops holds norm(x at the entry of block i)); exit_block [B, n0]; slabs {c: the stream
    behind block c scattered to the unpruned grid, un-normalised, pruned rows zero}; counts; trace)"""
    (tokens, states), counts, trace = vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype,
                                                           query=query, features="states")
    B, n0, depth = tokens.shape[0], counts[0], cfg.depth
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    src = source_idx(trace, B, n0)
    dense = scatter_dense(tokens, src, n0)
    dense_last, exit_block = dense.copy(), np.full((B, n0), depth, np.int32)
    for i in sorted(trace):
        assert i > 0, "a stage at block 0 drops rows of the embedded stream, which this helper does not keep"
        before = source_idx(trace, B, n0, upto=i - 1)                       # positions of the tokens entering block i
        entry = host(_ln(states[i - 1], sd, "norm", cfg.ln_eps, dtype))
        kept = np.zeros(before.shape, bool)
        np.put_along_axis(kept, trace[i]["keep_idx"], True, axis=1)
        for b in range(B):
            dense_last[b, before[b, ~kept[b]]] = entry[b, ~kept[b]]
            exit_block[b, before[b, ~kept[b]]] = i
    slabs = {c: scatter_dense(host(states[c]), source_idx(trace, B, n0, upto=c), n0) for c in caps}
    return dict(tokens=tokens, source_idx=src, dense=dense, dense_last=dense_last, exit_block=exit_block, slabs=slabs,
                counts=counts, trace=trace)


# ---- fixtures whose selections cannot hinge on a near-tie ---------------------------------------------------------------------
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
FIX_BASE = dict(std=0.08, bias_std=0.1)        # the weight scale the project's 1e-2 bar is stated for
GAP_FACTOR = 8.0
# (weight seed, image seed) per micro config, found by tests/test_noclass_cpu.py::search_seeds: among weight seeds 1..80 the one
# whose smallest boundary gap - over the images of the B = 3 batch (image 0 is the B = 1 batch) and both scheduled blocks, in
# the fp64 restatement with the mean query - is the largest multiple of the bf16 score budget (16 .. 28 x; at least
# GAP_FACTOR is demanded, and tests/test_noclass_cpu.py asserts it of the committed seeds).  The class-token model of the
# mean-query test (vit_micro_gap_patch16_64) has an entry too.
SEEDS = {
    "vit_micro_nocls_gap_patch16_64": (45, 49),
    "vit_micro_reg4_nocls_gap_patch16_64": (77, 81),
    "vit_micro_reg1_nocls_gap_d80_patch16_64": (41, 45),
    "vit_micro_gap_patch16_64": (19, 23),
}


def images_of(cfg, B, seed, size=None):
    from rajni_amd import timm_shaped as ts
    h, w = size or (cfg.img_size, cfg.img_size)
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, h, w), dtype=np.float32))


def boundary_gap_ratios(sd, images, schedule, cfg, dt="bf16", query=None):
    """min over images and scheduled blocks of (score gap at the keep boundary) / (score budget at the boundary) in the fp64
    restatement.  The budget is importance_budget's for output type `dt` on the scores the block ranks - for a carried stage
    (update = False) the budget it inherited with the scores - at the two tokens either side of the boundary (the larger)."""
    query = query or default_query(cfg)
    _, _, tr = vit_forward_restated(sd, images, schedule, cfg, query=query, budget_dt=dt)
    P = cfg.num_prefix_tokens
    worst = math.inf
    for i, t in tr.items():
        s = t["scores"]
        keep = t["keep_idx"].shape[1] - P
        if keep >= s.shape[1] - P:
            continue
        for b in range(s.shape[0]):
            order = np.argsort(-s[b, P:], kind="stable") + P
            lo, hi = order[keep - 1], order[keep]
            worst = min(worst, (s[b, lo] - s[b, hi]) / max(t["budget"][b, lo], t["budget"][b, hi]))
    return worst
