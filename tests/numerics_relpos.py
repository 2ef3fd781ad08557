"""Yardsticks for a relative position bias on the pruned token set (include/rajni_hip_relpos.h), pure numpy / torch-CPU, shared by
tests/test_relpos_cpu.py and the tests/test_gpu_relpos_*.py files.

The rule, restated:
  logit[q][k] = scale * (q . k) + bias(pos[q], pos[k])          (the bias is NOT multiplied by scale)
  bias(a, b)  = table[h][(dy + gh - 1) * (2 gw - 1) + (dx + gw - 1)]   both patches: dy = y_a - y_b, dx = x_a - x_b
                prefix_q[h]    a prefix (a < P), b a patch
                prefix_k[h]    a a patch, b prefix
                prefix_qk[h]   both prefix
  pos[t] = the place packed row t had in the unpruned sequence, whatever the blocks in front have pruned.
The reference has no such model, so the importance rule is the project's own: the class row's logits
get prefix_q[h] on the patch keys and prefix_qk[h] on the prefix keys before its softmax - importance is scored on the attention
the block computes."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import numerics as nm
import numerics_eva as ne
import numerics_noclass as nq
import numerics_prefix as npx
import numerics_rmsnorm as nr
from numerics_variants import _t, _ln
from oracle import rajni_oracle as orc


# ---------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------

def table_size(gh, gw):
    return (2 * gh - 1) * (2 * gw - 1)


def dense_bias(table, pq, pk, pqk, gh, gw, P, pos_q, pos_k):
    """[H, nq, nk] fp64: the bias of every (query, key) pair.  table [H, T]; pq / pk / pqk [H]; pos_q [nq], pos_k [nk]: places in
    the unpruned sequence (P prefix places first, then the grid row-major)"""
    table = np.asarray(table, np.float64)
    pos_q, pos_k = np.asarray(pos_q, np.int64), np.asarray(pos_k, np.int64)
    H = table.shape[0]
    assert table.shape[1] == table_size(gh, gw)
    a, b = np.maximum(pos_q - P, 0), np.maximum(pos_k - P, 0)
    dy = (a // gw)[:, None] - (b // gw)[None, :]
    dx = (a % gw)[:, None] - (b % gw)[None, :]
    out = table[:, (dy + gh - 1) * (2 * gw - 1) + (dx + gw - 1)]                  # [H, nq, nk]
    qpre, kpre = (pos_q < P)[:, None], (pos_k < P)[None, :]
    for h in range(H):
        out[h] = np.where(qpre & kpre, pqk[h], np.where(qpre, pq[h], np.where(kpre, pk[h], out[h])))
    return out


def batch_bias(table, pq, pk, pqk, gh, gw, P, pos):
    """[B, H, Np, Np] for pos [B, Np]"""
    return np.stack([dense_bias(table, pq, pk, pqk, gh, gw, P, p, p) for p in np.asarray(pos)])


def attention_budget(qkv_g, H, scale, dt, bias):
    """tests/numerics.py::attention_budget with the biased logit: qkv_g [B, Np, 3C] the gathered rows, bias [B, H, Np, Np] fp64.
    The kernels add the bias to q . k in front of the scale, S' = q . k + bias * (1 / scale), and run the unbiased code on S'
    (attention.hip), so ds - the absolute error of the logit - gains, beside the accumulation term:
        u32 max|bias|                            the product bias * (1 / scale)  (1 / scale itself is exact: scale = 2^-3)
        u32 (scale max sum|q k| + max|bias|)     the add: it rounds S', and |scale S'| <= scale sum|q k| + |bias|
    i.e. the issue's 2 u32 max|bias|, and one more u32 of the accumulation bound because the add rounds the whole biased S and
    not the bias alone (a fused add in exp2 units would round there too).  Everything else is nm.attention_budget's rule."""
    q, k, v = orc.split_heads(qkv_g.astype(np.float64), H)           # [B,H,Np,D]
    B, _, Np, D = q.shape
    s = np.einsum("bhqd,bhkd->bhqk", q, k) * scale + bias
    sabs = np.einsum("bhqd,bhkd->bhqk", np.abs(q), np.abs(k)).max(axis=-1) * scale       # [B,H,Np]
    bmax = np.abs(bias).max(axis=-1)                                                      # [B,H,Np]
    mx = s.max(axis=-1, keepdims=True)
    p = np.exp(s - mx)
    p /= p.sum(axis=-1, keepdims=True)
    want = np.einsum("bhqk,bhkd->bqhd", p, v).reshape(B, Np, H * D)
    A = np.einsum("bhqk,bhkd->bqhd", p, np.abs(v)).reshape(B, Np, H * D)
    ds = (D + 2) * nm.U32 * sabs + nm.U32 * (sabs + 2 * bmax)
    fac = (nm.UNIT[dt] if dt != "fp32" else nm.U32) + 4 * ds
    if dt == "fp32":
        fac = fac + 8 * nm.U32 * np.abs(s - mx).max(axis=-1)
    fac = np.repeat(fac.transpose(0, 2, 1)[..., None], D, axis=-1).reshape(B, Np, H * D)
    bud = nm.UNIT[dt] * np.abs(want) + fac * A + nm.FLOOR[dt]
    if dt == "fp16":
        vmax = np.abs(v).max(axis=(2, 3))
        bud = bud + np.repeat((Np * 2.0 ** -25 * vmax)[:, None, :, None], D, axis=-1).reshape(B, 1, H * D)
    return want, bud


def importance_scores(qkv, num_heads, pq, pqk, P, eps=1e-6, dtype=np.float64):
    """oracle/rajni_oracle.py::importance_scores, operation for operation, with the class row's bias (B11): pq [H] on the patch
    keys, pqk [H] on the P prefix keys, added to the scaled logits before the softmax"""
    qkv = np.asarray(qkv, dtype=dtype)
    B, N, threeC = qkv.shape
    C = threeC // 3
    D = C // num_heads
    t = qkv.reshape(B, N, 3, num_heads, D)
    q_cls, k, v = t[:, 0, 0], t[:, :, 1], t[:, :, 2]
    logits = np.einsum("bhd,bnhd->bhn", q_cls, k) / math.sqrt(D)
    cb = np.where(np.arange(N)[None, :] < P, np.asarray(pqk, dtype)[:, None], np.asarray(pq, dtype)[:, None])   # [H, N]
    logits = logits + cb[None].astype(dtype)
    logits = logits - logits.max(axis=-1, keepdims=True)
    e = np.exp(logits)
    attn = e / e.sum(axis=-1, keepdims=True)
    a_cls = attn.mean(axis=1)
    vbar = v.mean(axis=2)
    vbar = vbar - vbar.mean(axis=1, keepdims=True)
    vnorm = np.sqrt((vbar * vbar).sum(axis=-1))
    mu = vnorm.mean(axis=1, keepdims=True)
    std = np.sqrt(((vnorm - mu) ** 2).sum(axis=1, keepdims=True) / (N - 1)) + eps
    z = (vnorm - mu) / std
    return a_cls * (1.0 / (1.0 + np.exp(-z)))


def importance_budget(qkv, H, dt, pq, pqk, P, eps=1e-6):
    """nm.importance_budget's envelope, built from this file's restated function: (want, budget, e32)"""
    want = importance_scores(qkv, H, pq, pqk, P, eps)
    s32 = importance_scores(qkv, H, pq, pqk, P, eps, dtype=np.float32).astype(np.float64)
    e32 = float((np.abs(s32 - want) / np.abs(want)).max())
    return want, (nm.UNIT[dt] + 4 * e32) * np.abs(want) + nm.FLOOR[dt], e32


# ---------------------------------------------------------------------------------------------------------------
# kernel fixtures
# ---------------------------------------------------------------------------------------------------------------
TABLE_KINDS = ("normal", "onehot")
TABLE_STD = 2.0


def kernel_tables(kind, H, gh, gw, seed=0):
    """(table [H, T], pq, pk, pqk [H]) fp32.  normal: N(0, TABLE_STD^2) everywhere.  onehot: every head's table is zero but for
    an entry of 8 at each of the four corner offsets - index 0 and T - 1, the ends of the table, among them - and at (0, 0), and the
    three prefix values are 8 / 0 / -8: with `uniform` inputs the output is then a pure function of the indexing."""
    rng = np.random.default_rng([seed, H, gh, gw, TABLE_KINDS.index(kind)])
    T = table_size(gh, gw)
    if kind == "normal":
        return tuple((TABLE_STD * rng.standard_normal(s)).astype(np.float32) for s in ((H, T), (H,), (H,), (H,)))
    table = np.zeros((H, T), np.float32)
    W = 2 * gw - 1
    corners = [0, W - 1, (2 * gh - 2) * W, T - 1]
    table[:, corners + [(gh - 1) * W + (gw - 1)]] = 8.0
    return table, np.full(H, 8.0, np.float32), np.zeros(H, np.float32), np.full(H, -8.0, np.float32)


def kept_positions(rng, B, N, Np, P):
    """[B, Np] random kept sets: the P prefix places, then ascending patch places"""
    if Np == N:
        return np.tile(np.arange(N), (B, 1))
    return np.stack([np.concatenate([np.arange(P), P + np.sort(rng.choice(N - P, Np - P, replace=False))]) for _ in range(B)])


# ---------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("no_bias", "packed_positions", "transposed", "axes_swapped", "bias_times_scale", "prefix_as_patch",
           "score_without_bias", "block0_table_everywhere")


def native_tables(sd, cfg):
    """(table [nb, H, T], pq, pk, pqk [nb, H]) fp64 - the native contract's inputs read straight from the state dict (not through
    the wrapper's decomposition, which tests/test_relpos_cpu.py holds against this): nb = depth, or 1 for a shared bias.  BEiT's
    three extra table rows are prefix_q / prefix_k / prefix_qk; timm's RelPosBias pads the prefix rows and columns with zeros."""
    gh, gw = cfg.grid
    T = table_size(gh, gw)
    name = "relative_position_bias_table"
    keys = {"beit": [f"blocks.{i}.attn.{name}" for i in range(cfg.depth)], "beit_shared": ["rel_pos_bias." + name],
            "relpos": [f"blocks.{i}.attn.rel_pos.{name}" for i in range(cfg.depth)], "srelpos": ["shared_rel_pos." + name]}[cfg.rel_pos]
    rows = np.stack([np.asarray(sd[k], np.float64) for k in keys])                 # [nb, T (+ 3), H]
    zero = np.zeros((len(keys), cfg.num_heads))
    if cfg.rel_pos.startswith("beit"):
        return rows[:, :T].transpose(0, 2, 1), rows[:, T], rows[:, T + 1], rows[:, T + 2]
    return rows.transpose(0, 2, 1), zero, zero.copy(), zero.copy()


def _block_bias(tabs, i, gh, gw, P, pos, mutant, scale):
    """[B, H, Np, Np] fp64: block i's bias at the positions pos [B, Np], under `mutant`"""
    if mutant == "no_bias":
        return 0.0
    j = 0 if (tabs[0].shape[0] == 1 or mutant == "block0_table_everywhere") else i
    table, pq, pk, pqk = (t[j] for t in tabs)
    if mutant == "packed_positions":
        pos = np.tile(np.arange(pos.shape[1]), (pos.shape[0], 1))
    if mutant == "axes_swapped":        # the table read at (dx, dy): the same as decoding a place column-major, y = p % gh, x = p // gh
        a = np.maximum(pos - P, 0)
        y, x = a % gh, a // gh
        pos = np.where(pos < P, pos, P + y * gw + x)
    if mutant == "prefix_as_patch":     # a prefix row takes the bias of patch 0's place and no value of its own
        pos = np.maximum(pos, P)
    b = batch_bias(table, pq, pk, pqk, gh, gw, P, pos)
    if mutant == "transposed":
        b = b.transpose(0, 1, 3, 2)
    if mutant == "bias_times_scale":
        b = b * scale
    return b


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, features=None, budget_dt=None,
                         mutant=None, zero_tables=False):
    """(logits [B, classes], token counts, trace) of the pruned graph of a model with a relative position bias:
    tests/numerics_eva.py's function (its helpers, operation for operation) without the rotation and with the bias on the logits
    of every block and on the class row's logits of every scoring block (B11).  `zero_tables`: every table and value zero - the
    graph of tests/numerics_eva.py on the same state dict.  `mutant`: one of MUTANTS -
      no_bias                  no bias anywhere
      packed_positions         the table indexed by the packed row instead of the token's place in the image
      transposed               query and key exchanged
      axes_swapped             dy and dx exchanged
      bias_times_scale         the bias multiplied by the attention scale
      prefix_as_patch          the prefix rows looked up in the table as patch 0, their three values unused (in attention; the
                               scores keep the rule)
      score_without_bias       importance scored without the class row's bias (it moves nothing under forced selections: its
                               separation is measured free running)
      block0_table_everywhere  block 0's table in every block"""
    assert mutant is None or mutant in MUTANTS, mutant
    schedule = orc.normalise_schedule(schedule)
    kind = cfg.norm
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    Pn = cfg.num_prefix_tokens
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    gh, gw = cfg.grid
    scale = D ** -0.5
    tabs = native_tables(sd, cfg)
    if zero_tables:
        tabs = tuple(np.zeros_like(t) for t in tabs)
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B, n = x.shape[0], x.shape[1]
    assert n == gh * gw and not cfg.abs_pos and cfg.class_token and not cfg.embed_norm
    prefix = [W("cls_token").expand(B, -1, -1)] + ([W("reg_token").expand(B, -1, -1)] if cfg.reg_tokens else [])
    x = torch.cat(prefix + [x], 1)
    if cfg.pre_norm:
        x = nr._norm(x, sd, "norm_pre", eps, dtype, kind)
    src = np.tile(np.arange(Pn + n), (B, 1))                 # where each token of the stream sat in the unpruned sequence
    scores, counts, trace, states, bud, full_bud = None, [], {}, {}, None, None
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = nr._norm(x, sd, p + "norm1", eps, dtype, kind)
        wq, bq = ne.packed_qkv(sd, p, C)
        qkv = (xn @ _t(wq, dtype).T + _t(bq, dtype)).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                flat = host(torch.stack([q, k, v], 2).reshape(B, N, 3 * C))
                j = 0 if (tabs[0].shape[0] == 1 or mutant == "block0_table_everywhere") else i
                off = mutant in ("no_bias", "score_without_bias")
                spq, spqk = (np.zeros(H), np.zeros(H)) if off else (tabs[1][j], tabs[3][j])
                if mutant == "bias_times_scale":
                    spq, spqk = spq * scale, spqk * scale
                full = importance_scores(flat, H, spq, spqk, Pn, dtype=np_dt)
                if budget_dt:
                    full_bud = importance_budget(flat, H, budget_dt, spq, spqk, Pn)[1]
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
            src = np.take_along_axis(src, keep_idx, axis=1)
        else:
            scores = None
        bias = _block_bias(tabs, i, gh, gw, Pn, src, mutant, scale)
        logits = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
        if not isinstance(bias, float):
            logits = logits + torch.from_numpy(bias).to(dtype)
        att = torch.softmax(logits, dim=-1)
        out = nr._linear(torch.einsum("bhqk,bkhd->bqhd", att, v).reshape(B, -1, C), sd, p + "attn.proj", dtype)
        g1, g2 = ne._gamma(sd, p, 1, dtype, None), ne._gamma(sd, p, 2, dtype, None)
        x = x + (out if g1 is None else out * g1)
        h = ne._mlp(nr._norm(x, sd, p + "norm2", eps, dtype, kind), sd, p, cfg, dtype)
        x = x + (h if g2 is None else h * g2)
        states[i] = x
    raw = x
    if "norm.weight" in sd:
        x = nr._norm(x, sd, "norm", eps, dtype, kind)
    if features == "tokens":
        return host(x), counts, trace
    if features == "states":
        return (host(x), states, raw), counts, trace
    x = x[:, Pn:].mean(1) if cfg.global_pool == "avg" else x[:, 0]
    if cfg.use_fc_norm:
        x = nr._norm(x, sd, "fc_norm", eps, dtype, kind)
    if "head.weight" in sd:
        x = nr._linear(x, sd, "head", dtype)
    return host(x), counts, trace


def feature_outputs(sd, images, schedule, cfg, forced_keep=None, caps=(), dtype=torch.float64):
    """tests/numerics_eva.py::feature_outputs on this file's graph"""
    (tokens, states, _), counts, trace = vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype,
                                                              features="states")
    B, n0, depth = tokens.shape[0], counts[0], cfg.depth
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    src = nq.source_idx(trace, B, n0)
    dense = nq.scatter_dense(tokens, src, n0)
    dense_last = dense.copy()
    for i in sorted(trace):
        assert i > 0
        before = nq.source_idx(trace, B, n0, upto=i - 1)
        entry = host(nr._norm(states[i - 1], sd, "norm", cfg.ln_eps, dtype, cfg.norm))
        kept = np.zeros(before.shape, bool)
        np.put_along_axis(kept, trace[i]["keep_idx"], True, axis=1)
        for b in range(B):
            dense_last[b, before[b, ~kept[b]]] = entry[b, ~kept[b]]
    slabs = {c: nq.scatter_dense(host(states[c]), nq.source_idx(trace, B, n0, upto=c), n0) for c in caps}
    return dict(tokens=tokens, source_idx=src, dense=dense, dense_last=dense_last, slabs=slabs, counts=counts, trace=trace)


# ---------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------
# tests/numerics_rope.py's schedules, rule and constants: both prune in block 1, so blocks 2 and 3 run on a pruned stream, where
# row t is no longer patch t - what the packed_positions mutant gets wrong
SCHED, CARRIED, SCHEDULES = ne.SCHED, ne.CARRIED, ne.SCHEDULES
FIX_BASE = nq.FIX_BASE
GAP_FACTOR = nq.GAP_FACTOR
BAR = nr.BAR
MUTANT_FACTOR = ne.MUTANT_FACTOR
FORMAT_HEADROOM = nr.FORMAT_HEADROOM
BATCH = 3
MICRO = ["beit_micro_patch16_64", "beit_micro_shared_patch16_64", "vit_micro_relpos_patch16_64", "beit_micro_patch16_48x96"]
CASES = [("SCHED", None), ("CARRIED", None)]
# (weight seed, image seed = weight seed + 4) per micro config: the first weight seed from 1 up with the property `holds` -
# tests/numerics_rope.py's search and criteria, and one more: the fp32 restated graph selects the tokens the fp64 one selects, on
# every image of the batch under both schedules, so that no image is left out of a free-running comparison.
# tests/test_relpos_cpu.py asserts all of it of the committed seeds; search_seeds finds them.
# The walk, seed by seed, up to the committed one (f = format cost in % of the output scale, limit 0.80; g = the smallest
# boundary gap in bf16 score budgets, limit 8; m = the smallest separation of a live mutant in %, limit 4 - 0.00 is
# score_without_bias leaving every selection as it was; s = an fp32 selection differs; the first criterion that fails is recorded):
#   beit_micro_patch16_64:        1:g6.3 2:m0.00 3:f1.00 4:m0.00 5:g1.6 6:g2.2 7:m0.00 8:g3.1 9:g0.4 10:f0.82 11:m0.00 12:m0.00 13:g6.6
#   beit_micro_shared_patch16_64: 1:g2.3 2:m0.00 3:g5.4 4:m0.00 5:f1.03 6:m0.00 7:g2.2 8:g0.6 9:g0.8 10:g4.5 11:m0.00 12:g4.1 13:m0.00
#                                 14:g2.3 15:m0.00 16:g2.8 17:m0.00 18:g3.3 19:g1.9 20:g6.5 21:g1.3 22:m0.00 23:g1.6 24:f0.87
#   vit_micro_relpos_patch16_64:  1:f1.77 2:g6.4 3:f0.99 4:f0.97 5:g3.2
#   beit_micro_patch16_48x96:     1:g0.4 2:m0.00 3:g1.8 4:g0.9 5:m0.00 6:f0.96 7:g3.4 8:g0.2 9:g0.0 10:g2.4 11:g4.7 12:m0.00 13:g1.1
#                                 14:g3.3 15:m0.00 16:g1.1
SEEDS = {
    "beit_micro_patch16_64": (14, 18),
    "beit_micro_shared_patch16_64": (25, 29),
    "vit_micro_relpos_patch16_64": (6, 10),
    "beit_micro_patch16_48x96": (17, 21),
}


def build_model(name_or_cfg, wseed=None):
    """the timm-shaped module of a fixture: bf16-representable weights at the project's scale, the bias tables at std 1"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg
    seed = SEEDS[name_or_cfg][0] if wseed is None else wseed
    return ts.create_model(cfg, seed=seed, round_bf16=True, **FIX_BASE)


@functools.lru_cache(maxsize=None)
def fixture(name, wseed=None):
    """(config, fp32 state dict with bf16-representable values, image seed) - built once, never modified"""
    from rajni_amd import timm_shaped as ts
    m = build_model(name, wseed)
    return m.cfg, ts.state_dict_numpy(m), (SEEDS[name][1] if wseed is None else wseed + 4)


def images_of(cfg, B, seed):
    return nq.images_of(cfg, B, seed, (cfg.img_size, cfg.img_width) if cfg.img_width else None)


@functools.lru_cache(maxsize=None)
def case(name, sched="SCHED", B=BATCH, wseed=None):
    """(sd, images, the fp64 free-running forward (logits, counts, trace)) - computed once, shared, never modified"""
    cfg, sd, iseed = fixture(name, wseed)
    imgs = images_of(cfg, B, iseed)
    return sd, imgs, vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg)


def boundary_gap_ratios(name, sched="SCHED", B=BATCH, wseed=None, dt="bf16"):
    """tests/numerics_eva.py::boundary_gap_ratios on this file's graph"""
    cfg = fixture(name, wseed)[0]
    sd, imgs, _ = case(name, sched, B, wseed)
    _, _, tr = vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, budget_dt=dt)
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


def vacuous(cfg, mutant):
    """a mutant that IS the forward on this config: block 0's table everywhere where one table serves every block; scoring
    without the class row's bias where that bias is zero (timm's RelPosBias pads the prefix rows with zeros).  (axes_swapped is
    live on a square grid too: a learned table is not symmetric under exchanging its axes.)"""
    if mutant == "block0_table_everywhere":
        return cfg.rel_pos in ("beit_shared", "srelpos")
    if mutant == "score_without_bias":
        return cfg.rel_pos in ("relpos", "srelpos")
    return False


def mutant_separations(name, sched="SCHED", B=BATCH, wseed=None):
    """{mutant: max |logits - mutant's logits| / max |logits|} in fp64, the mutant under the forward's own selections"""
    cfg = fixture(name, wseed)[0]
    sd, imgs, (want, _, tr) = case(name, sched, B, wseed)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    out = {}
    for mut in MUTANTS:
        other, _, _ = vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, mutant=mut,
                                           forced_keep=None if mut == "score_without_bias" else forced)
        out[mut] = float(np.abs(want - other).max() / np.abs(want).max())
    return out


def selections_agree(name, sched="SCHED", B=BATCH, wseed=None):
    """the fp32 restated graph, free running, selects what the fp64 one selects - on every image"""
    cfg = fixture(name, wseed)[0]
    sd, imgs, (_, _, tr) = case(name, sched, B, wseed)
    _, _, tr32 = vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, dtype=torch.float32)
    return all(np.array_equal(tr[i]["keep_idx"], tr32[i]["keep_idx"]) for i in tr)


def format_cost(name, wseed, B, dtype=torch.bfloat16):
    """tests/numerics_rmsnorm.py::format_cost on this file's fixtures"""
    cfg = fixture(name, wseed)[0]
    imgs = torch.from_numpy(images_of(cfg, B, wseed + 4))
    with torch.no_grad():
        a = build_model(name, wseed)(imgs).numpy()
        b = build_model(name, wseed).to(dtype)(imgs.to(dtype)).float().numpy()
    return float(np.abs(a - b).max() / np.abs(a).max())


def holds(name, wseed, verbose=False):
    """the property SEEDS is chosen for, at weight seed `wseed`"""
    cfg = fixture(name, wseed)[0]
    f = max(format_cost(name, wseed, B) for B in (1, BATCH))
    if f > FORMAT_HEADROOM * BAR["bf16"]:
        return (False, f"f{100 * f:.2f}") if verbose else False
    for sched, _ in CASES:
        g = boundary_gap_ratios(name, sched, wseed=wseed)
        if g < GAP_FACTOR:
            return (False, f"g{g:.1f}") if verbose else False
        sep = mutant_separations(name, sched, wseed=wseed)
        m = min(v for k, v in sep.items() if not vacuous(cfg, k))
        if m < MUTANT_FACTOR * BAR["bf16"]:
            return (False, f"m{100 * m:.2f}") if verbose else False
        if not selections_agree(name, sched, wseed=wseed):
            return (False, "s") if verbose else False
    return (True, "ok") if verbose else True


def search_seeds(name, limit=200, verbose=False):
    """the first weight seed from 1 up with the property (image seed = weight seed + 4)"""
    walk = []
    for seed in range(1, limit + 1):
        ok, why = holds(name, seed, verbose=True)
        fixture.cache_clear(); case.cache_clear()
        walk.append(f"{seed}:{why}")
        if ok:
            if verbose:
                print(name, " ".join(walk))
            return seed, seed + 4
    raise AssertionError(name)
