"""Inputs, budgets, CPU emulations and the yardstick graph for the timm options of the native forward (q/k-norm,
norm_pre, pooled head with fc_norm).  Pure numpy / torch-CPU, shared by
tests/test_variants_cpu.py, tests/test_gpu_variants_kernels.py and tests/test_gpu_variants_forward.py.

The LayerNorm budget and the stress rows are tests/numerics.py's, imported as they stand (C_LN = 17)."""
from __future__ import annotations

import numpy as np
import torch

import numerics as nm
from oracle import rajni_oracle as orc

F32 = np.float32
HEAD_DIMS = [32, 64, 72, 80, 128]
QK_R4_GROUPS = 65536            # csrc/variants.hip QK_NORM_R4_GROUPS: launches of at least this many groups run 4 per slot
POOL_NP = [2, 88, 197, 577]


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' algorithms (csrc/variants.hip), operation by operation
# ---------------------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
            + np.asarray(c, F32).astype(np.float64)).astype(F32)


def _lane_tree(v, steps):
    """v [..., L] fp32 per-lane partials -> the butterfly sum every lane ends with (lane 0's), xor distances `steps`"""
    v = np.asarray(v, F32)
    lanes = np.arange(v.shape[-1])
    for s in steps:
        v = (v + v[..., lanes ^ s]).astype(F32)
    return v[..., 0]


def _seq_sum8(c):
    """[..., 8] -> sequential fp32 sum (a lane's own 8 elements)"""
    s = np.zeros(c.shape[:-1], F32)
    for j in range(8):
        s = (s + c[..., j]).astype(F32)
    return s


def _group_layernorm32(x, w, b, eps, lanes, steps, one_pass=False):
    """x [G, D] fp32 values; lanes hold 8 consecutive elements each (lanes past D / 8 hold zeros), two-pass statistics
    summed per lane then over the lanes; `one_pass`: the E[x^2] - E[x]^2 mutant."""
    G, D = x.shape
    ch = np.zeros((G, lanes, 8), F32)
    ch.reshape(G, lanes * 8)[:, :D] = x
    inv_d = F32(1.0) / F32(D)
    mean = (_lane_tree(_seq_sum8(ch), steps) * inv_d).astype(F32)
    if one_pass:
        ex2 = (_lane_tree(_seq_sum8((ch * ch).astype(F32)), steps) * inv_d).astype(F32)
        var = (ex2 - mean * mean).astype(F32)
    else:
        d = (ch - mean[:, None, None]).astype(F32)
        d.reshape(G, lanes * 8)[:, D:] = 0
        var = (_lane_tree(_seq_sum8((d * d).astype(F32)), steps) * inv_d).astype(F32)
    with np.errstate(invalid="ignore"):                  # (the one-pass mutant's variance can come out negative: NaN)
        rstd = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    n = ((x - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    return _fma32(n, w, b if b is not None else F32(0))


def _qk_lanes(D):
    lw = 4 if D <= 32 else (8 if D <= 64 else 16)
    return lw, [s for s in (1, 2, 4, 8) if s < lw]


def emul_qk_norm(qkv, H, D, qw, qb, kw, kb, eps, dt, one_pass=False, q_weights_on_k=False):
    """qkv [rows, 3HD] (fp32 values of type dt) -> the kernel's result, rounded to dt; v untouched"""
    rows = qkv.shape[0]
    lanes, steps = _qk_lanes(D)
    out = qkv.copy()
    C = H * D
    q = _group_layernorm32(qkv[:, :C].reshape(rows * H, D), qw, qb, eps, lanes, steps, one_pass)
    if q_weights_on_k:
        kw, kb = qw, qb
    k = _group_layernorm32(qkv[:, C:2 * C].reshape(rows * H, D), kw, kb, eps, lanes, steps, one_pass)
    out[:, :C] = nm.round_to(q, dt).reshape(rows, C)
    out[:, C:2 * C] = nm.round_to(k, dt).reshape(rows, C)
    return out


def _wave_layernorm32(x, w, b, eps, one_pass=False):
    """rows x [R, C]: chunk c of 8 elements sits in lane c % 64; per-lane sums over its chunks, then a 64-lane butterfly"""
    R, C = x.shape
    nchunk = C // 8
    ch = x.reshape(R, nchunk, 8)

    def wave_sum(vals):                                   # vals [R, nchunk, 8]
        lane = np.zeros((R, 64), F32)
        for c in range(nchunk):                           # chunks in ascending order per lane, elements in order
            for j in range(8):
                lane[:, c % 64] = (lane[:, c % 64] + vals[:, c, j]).astype(F32)
        return _lane_tree(lane, (32, 16, 8, 4, 2, 1))

    mean = (wave_sum(ch) / F32(C)).astype(F32)
    if one_pass:
        var = ((wave_sum((ch * ch).astype(F32)) / F32(C)).astype(F32) - mean * mean).astype(F32)
    else:
        d = (ch - mean[:, None, None]).astype(F32)
        var = (wave_sum((d * d).astype(F32)) / F32(C)).astype(F32)
    with np.errstate(invalid="ignore"):                  # (the one-pass mutant's variance can come out negative: NaN)
        rstd = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    n = ((x - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    return _fma32(n, w, b if b is not None else F32(0))


def emul_layernorm_stream(x, w, b, eps, dt, one_pass=False):
    return nm.round_to(_wave_layernorm32(np.asarray(x, F32), w, b, eps, one_pass), dt)


def emul_pool_norm(x, pool, norm, fc_norm, out_dt, include_cls=False, one_pass=False, rounded=True):
    """x [B, N, C] fp32 values -> [B, C]: 8 waves take rows r0 + k, r0 + k + 8, ...; s_k += s_{k+4}; ((s0 + s1) + s2) + s3.
    `include_cls`: the mutant whose mean starts at row 0."""
    B, N, C = x.shape
    r0, r1 = (1, N) if pool == "avg" else (0, 1)
    if include_cls and pool == "avg":
        r0 = 0
    out = np.zeros((B, C), F32)
    for i in range(B):
        rows = np.asarray(x[i, r0:r1], F32)
        if norm is not None:
            rows = _wave_layernorm32(rows, norm[0], norm[1], norm[2], one_pass)
        acc = np.zeros((8, C), F32)
        for r in range(rows.shape[0]):
            acc[r % 8] = (acc[r % 8] + rows[r]).astype(F32)
        acc[:4] = (acc[:4] + acc[4:]).astype(F32)
        s = acc[0]
        for k in (1, 2, 3):
            s = (s + acc[k]).astype(F32)
        if r1 - r0 > 1:
            s = (s * (F32(1.0) / F32(r1 - r0))).astype(F32)
        if fc_norm is not None:
            s = _wave_layernorm32(s[None], fc_norm[0], fc_norm[1], fc_norm[2], one_pass)[0]
        out[i] = s
    return nm.round_to(out, out_dt) if rounded else out


# ---------------------------------------------------------------------------------------------------------------
# inputs and budgets
# ---------------------------------------------------------------------------------------------------------------

def qk_norm_case(rows, H, D, dt, seed=0):
    """qkv [rows, 3HD] whose (token, head) groups of q and k are nm.layernorm_rows stress rows (the cases alternate group by
    group), v standard normal; two DIFFERENT affine pairs (q, k), values of type dt held in fp32"""
    g, _, qw, qb = nm.layernorm_rows(rows * 2 * H, D, dt, seed=seed)
    rng = np.random.default_rng([seed, rows, H, D, 3])
    kw = nm.round_to((1 + 0.1 * rng.standard_normal(D)).astype(F32), dt)
    kb = nm.round_to((0.1 * rng.standard_normal(D)).astype(F32), dt)
    qw, qb = nm.round_to(qw, dt), nm.round_to(qb, dt)
    qkv = np.empty((rows, 3 * H * D), F32)
    qkv[:, :2 * H * D] = g.reshape(rows, 2 * H * D)
    qkv[:, 2 * H * D:] = nm.round_to(rng.standard_normal((rows, H * D), dtype=F32), dt)
    return qkv, qw, qb, kw, kb


def qk_norm_budget(qkv, H, D, qw, qb, kw, kb, eps, dt):
    """(want, budget) [rows, 2HD] for the q and k thirds: nm.layernorm_budget per (token, head) group, C_LN as it stands"""
    rows, C = qkv.shape[0], H * D
    wq, bq = nm.layernorm_budget(qkv[:, :C].reshape(rows * H, D), qw, qb, eps, dt)
    wk, bk = nm.layernorm_budget(qkv[:, C:2 * C].reshape(rows * H, D), kw, kb, eps, dt)
    return (np.concatenate([wq.reshape(rows, C), wk.reshape(rows, C)], axis=1),
            np.concatenate([bq.reshape(rows, C), bk.reshape(rows, C)], axis=1))


def pool_case(B, Np, C, dt, seed=0):
    """x [B, Np, C]: the tokens of each image are nm.layernorm_rows stress rows; (w, b) pairs for norm and fc_norm"""
    x, _, nw, nb = nm.layernorm_rows(B * Np, C, dt, seed=seed)
    rng = np.random.default_rng([seed, B, Np, C, 5])
    fw = (1 + 0.1 * rng.standard_normal(C)).astype(F32)
    fb = (0.1 * rng.standard_normal(C)).astype(F32)
    return x.reshape(B, Np, C), (nw, nb), (fw, fb)


def _ln_terms(x64, w, eps):
    """rows x64 [..., C] -> (n, sigma', the unrounded part of nm.layernorm_budget: C_LN u32 max|w| (kappa + |n|))"""
    mu = x64.mean(axis=-1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=-1, keepdims=True)
    sig = np.sqrt(var + eps)
    n = (x64 - mu) / sig
    kappa = np.abs(x64).max(axis=-1, keepdims=True) / sig
    return n, sig, nm.C_LN * nm.U32 * np.abs(w).max() * (kappa + np.abs(n))


def pool_norm_budget(x, pool, norm, fc_norm, out_dt):
    """(want, budget) [B, C] of out = fc_norm(mean_rows norm(x)), x [B, N, C] values of the input type.

    Let y_r = norm(x_r) (x_r itself without a norm), p = mean_r y_r over the R pooled rows, both in fp64.
      e[c]: error of the fp32 pooled value.  Summing R fp32 terms in any order and one multiply by 1/R is off by at most
            (R - 1 + 2) u32 sum_r |y_r[c]| / R, so with Np = R + 1 tokens  e_pool = (Np + 2) u32 mean_r |y_r[c]|;  a norm in
            front adds each row's own LayerNorm error, the unrounded term of nm.layernorm_budget, averaged over the rows.
      no fc_norm:  |err| <= u_out |p| + e + floor.
      fc_norm (weight w, n = (p - mu) / sigma'):  nm.layernorm_budget on p, plus e propagated to first order through the
            LayerNorm,  d out[c] = w[c] / sigma' (d[c] - mean(d) - n[c] mean(n d)):
            |w[c]| / sigma' (e[c] + mean_c e + |n[c]| mean_c(|n| e)).
    One row ('token', or Np = 2) has R = 1: the same formulas (the sum is exact, the bound is not tightened for it)."""
    x64 = np.asarray(x, np.float64)
    B, N, C = x64.shape
    rows = x64[:, 1:] if pool == "avg" else x64[:, :1]
    e_ln = 0.0
    if norm is not None:
        n, sig, unr = _ln_terms(rows, norm[0], norm[2])
        rows = n * norm[0] + (norm[1] if norm[1] is not None else 0.0)
        e_ln = unr.mean(axis=1)
    p = rows.mean(axis=1)                                                      # [B, C]
    e = (rows.shape[1] + 1 + 2) * nm.U32 * np.abs(rows).mean(axis=1) + e_ln
    if fc_norm is None:
        return p, nm.UNIT[out_dt] * np.abs(p) + e + nm.FLOOR[out_dt]
    fw, fb, feps = fc_norm
    want, bud = nm.layernorm_budget(p, fw, fb if fb is not None else 0.0, feps, out_dt)
    n, sig, _ = _ln_terms(p, fw, feps)
    prop = np.abs(fw) / sig * (e + e.mean(axis=-1, keepdims=True) + np.abs(n) * (np.abs(n) * e).mean(axis=-1, keepdims=True))
    return want, bud + prop


# ---------------------------------------------------------------------------------------------------------------
# the yardstick for pruned forwards: the reference's pruned graph (rajni/wrapper/model.py:30-69, attention.py:17-60, restated
# in oracle/rajni_oracle.py::vit_forward) with timm's three options added, in torch
# ---------------------------------------------------------------------------------------------------------------

def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _ln(x, sd, prefix, eps, dtype):
    w = _t(sd[prefix + ".weight"], dtype)
    b = _t(sd[prefix + ".bias"], dtype) if prefix + ".bias" in sd else None
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)


def _quant_rows(x, scale=None):
    """the act_fp8 rule on a torch tensor (oracle/rajni_oracle.py quantize_rows_e4m3); scale None = the row maximum's"""
    a = x.numpy()
    s = orc.row_scale_e4m3(a) if scale is None else scale
    return torch.from_numpy(orc.quantize_rows_e4m3(a, s)).to(x.dtype)


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, drop=(), act_fp8=False):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx}) for a timm-named numpy state dict `sd` of
    a rajni_amd.timm_shaped config.  Options present in `cfg` are applied as timm applies them unless named in `drop`
    ("qk_norm", "pre_norm", "avg_pool", "fc_norm" - the fixture-validity check: what the logits would be if the option
    were ignored).  Importance is computed from the NORMALISED q and k (the CLS row of the attention the block performs)."""
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    P = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), P("patch_embed.proj.weight"), P("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    cls = P("cls_token").expand(B, -1, -1)
    x = torch.cat([cls, x + P("pos_embed")], 1) if cfg.no_embed_class else torch.cat([cls, x], 1) + P("pos_embed")
    if cfg.pre_norm and "pre_norm" not in drop:
        x = _ln(x, sd, "norm_pre", eps, dtype)
    scores, counts, trace = None, [], {}
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _ln(x, sd, p + "norm1", eps, dtype)
        osc = None
        if act_fp8:
            xn = _quant_rows(xn)
            osc = orc.attention_out_scale(sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "attn.qkv.weight"][2 * C:],
                                          sd[p + "attn.qkv.bias"][2 * C:])
        qkv = (xn @ P(p + "attn.qkv.weight").T + P(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)                                             # [B, N, H, D]
        if cfg.qk_norm and "qk_norm" not in drop:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        keep_idx = None
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                full = orc.importance_scores(torch.stack([q, k, v], 2).reshape(B, N, 3 * C).numpy(), H, dtype=np_dt)
            else:
                full = scores
            keep = orc.keep_count(sc["keep_ratio"], N)
            keep_idx = orc.select_tokens(full, keep) if forced_keep is None or i not in forced_keep \
                else np.asarray(forced_keep[i], np.int64)
            scores = np.take_along_axis(full, keep_idx, axis=1)
            trace[i] = {"scores": full, "keep_idx": keep_idx, "next_scores": scores}
            gi = torch.from_numpy(keep_idx)[:, :, None, None].expand(-1, -1, H, D)
            q, k, v = q.gather(1, gi), k.gather(1, gi), v.gather(1, gi)
            x = x.gather(1, torch.from_numpy(keep_idx)[:, :, None].expand(-1, -1, C))
        else:
            scores = None
        att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5, dim=-1)
        out = torch.einsum("bhqk,bkhd->bqhd", att, v).reshape(B, -1, C)
        if osc is not None and orc.attention_out_is_fp8(D, out.shape[1]):
            out = _quant_rows(out, np.float32(osc))
        out = out @ P(p + "attn.proj.weight").T + P(p + "attn.proj.bias")
        x = x + (out * P(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = _ln(x, sd, p + "norm2", eps, dtype)
        if act_fp8:
            hs = orc.hidden_scale_bound(h.numpy(), sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
            h = _quant_rows(h)
        h = torch.nn.functional.gelu(h @ P(p + "mlp.fc1.weight").T + P(p + "mlp.fc1.bias"))
        if act_fp8:
            h = _quant_rows(h, hs)
        h = h @ P(p + "mlp.fc2.weight").T + P(p + "mlp.fc2.bias")
        x = x + (h * P(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
    if "norm.weight" in sd:
        x = _ln(x, sd, "norm", eps, dtype)
    x = x[:, 1:].mean(1) if cfg.global_pool == "avg" and "avg_pool" not in drop else x[:, 0]
    if cfg.use_fc_norm and "fc_norm" not in drop:
        x = _ln(x, sd, "fc_norm", eps, dtype)
    logits = x @ P("head.weight").T + P("head.bias")
    return logits.numpy(), counts, trace
