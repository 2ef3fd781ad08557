"""Yardsticks for rotary position embeddings on the pruned token set (include/rajni_hip_rope.h), pure numpy / torch-CPU in fp64,
shared by tests/test_rope_cpu.py and the tests/test_gpu_rope_*.py files.

The reference has no RoPE, so the rule is the project's own, restated here:
  y[j] = x[j] cos[p][j] + s(j) x[partner(j)] sin[p][j]
  interleaved: partner(j) = j ^ 1,          s = -1 for even j, +1 for odd      (timm rot(): pairs (2i, 2i + 1))
  half:        partner(j) = (j + D/2) % D,   s = -1 for j < D/2, +1 otherwise   (rotate_half)
on q and k of every block, behind q/k-norm and in front of scoring and attention; v and the P prefix rows pass through; the
table row p of a token is the place it had in the image, whatever the blocks in front have pruned.  Importance is computed from
the rotated q and k; the mean query averages the rotated queries.
The forward is tests/numerics_rmsnorm.py::vit_forward_restated (its helpers, operation for operation) with the rotation at
source positions, a model without an absolute position embedding, and the mutants that a wrong rotation would be."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import numerics as nm
import numerics_noclass as nq
import numerics_prefix as npx
import numerics_rmsnorm as nr
from numerics_variants import _t, _ln

INTERLEAVED, HALF = 0, 1


# ---------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------

def partner_and_sign(D, layout):
    j = np.arange(D)
    if layout == INTERLEAVED:
        return j ^ 1, np.where(j % 2 == 0, -1.0, 1.0)
    if layout == HALF:
        return (j + D // 2) % D, np.where(j < D // 2, -1.0, 1.0)
    raise ValueError(layout)


def rope64(x, cos, sin, layout):
    """the rule in fp64: x [..., D], cos / sin broadcastable to it"""
    x = np.asarray(x, np.float64)
    part, sign = partner_and_sign(x.shape[-1], layout)
    return x * np.asarray(cos, np.float64) + sign * x[..., part] * np.asarray(sin, np.float64)


def rope_budget(x, cos, sin, layout, dt):
    """(want, budget).  Derived, not measured: two fp32 products and one add, in any order or contraction, then one rounding to
    the output type -
        |err| <= UNIT[dt] |want| + 2 U32 (|x cos| + |x' sin|) + FLOOR[dt]
    (each product is off by at most U32 of itself, the sum by U32 of at most |x cos| + |x' sin| (1 + U32); a fused
    multiply-add drops one of the three)."""
    x = np.asarray(x, np.float64)
    part, _ = partner_and_sign(x.shape[-1], layout)
    want = rope64(x, cos, sin, layout)
    mag = np.abs(x * np.asarray(cos, np.float64)) + np.abs(x[..., part] * np.asarray(sin, np.float64))
    return want, nm.UNIT[dt] * np.abs(want) + 2 * nm.U32 * mag + nm.FLOOR[dt]


def table_rows(B, N, P, src):
    """[B, N - P] table row of every patch row: (src[b, t] if src is given else t) - P"""
    t = np.tile(np.arange(P, N), (B, 1)) if src is None else np.asarray(src)[:, P:]
    return t - P


def rope_qkv(qkv, cos, sin, P, layout, src=None, dt="fp32"):
    """(want, budget) for qkv [B, N, 3, H, D]: q and k of the rows t >= P rotated by table row table_rows(...), with cos / sin
    [rows, D] (one table for all heads) or [H, rows, D]; v and the prefix rows unchanged (budget 0 there)."""
    qkv = np.asarray(qkv, np.float64)
    B, N, _, H, D = qkv.shape
    want, bud = qkv.copy(), np.zeros_like(qkv)
    p = table_rows(B, N, P, src)
    cos, sin = np.asarray(cos, np.float64), np.asarray(sin, np.float64)
    if cos.ndim == 2:
        c, s = cos[p][:, :, None, :], sin[p][:, :, None, :]                    # [B, n, 1, D]
    else:
        c, s = cos[:, p].transpose(1, 2, 0, 3), sin[:, p].transpose(1, 2, 0, 3)   # [H, B, n, D] -> [B, n, H, D]
    for third in (0, 1):
        want[:, P:, third], bud[:, P:, third] = rope_budget(qkv[:, P:, third], c, s, layout, dt)
    return want, bud


# ---------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("no_rope", "stream_positions", "rotate_prefix", "rotate_v", "other_layout", "sign_flipped")


def model_tables(model, grid=None):
    """the model's rotary table as the wrapper fetches it: sin || cos, fp32 values as a float64 array [n, 2D] / [depth, H, n, 2D]"""
    with torch.no_grad():
        emb = model.rope.get_embed() if grid is None else model.rope.get_embed(shape=grid)
    return emb.float().cpu().numpy().astype(np.float64)


def _rotate(t, emb_i, rows, P, layout, dtype, prefix_rows=None):
    """t [B, N, H, D] torch: rows P.. rotated by table rows `rows` [B, N - P] of emb_i ([n, 2D] or [H, n, 2D], sin || cos);
    `prefix_rows` [P]: the prefix rows rotated too, by those table rows (the rotate_prefix mutant)"""
    D = t.shape[-1]
    part, sign = partner_and_sign(D, layout)
    part, sign = torch.from_numpy(part), torch.from_numpy(sign).to(dtype)
    emb = torch.from_numpy(np.asarray(emb_i)).to(dtype)

    def at(r):                                      # r [B, m] -> sin, cos [B, m, H or 1, D]
        r = torch.from_numpy(np.asarray(r, np.int64))
        e = emb[r][:, :, None] if emb.dim() == 2 else emb[:, r].permute(1, 2, 0, 3)
        return e[..., :D], e[..., D:]

    def rot(x, r):
        s, c = at(r)
        return x * c + sign * x[..., part] * s

    out = [t[:, :P] if prefix_rows is None else rot(t[:, :P], np.tile(prefix_rows, (t.shape[0], 1))), rot(t[:, P:], rows)]
    return torch.cat(out, 1)


def vit_forward_restated(sd, images, schedule, cfg, tables, forced_keep=None, dtype=torch.float64, query=None, features=None,
                         budget_dt=None, mutant=None):
    """(logits [B, classes], token counts, trace) of the pruned graph of a RoPE model: tests/numerics_rmsnorm.py's function with
    the rotation behind q/k-norm.  `tables`: model_tables(model) for the input's grid.  `mutant`: one of MUTANTS -
      no_rope            no rotation at all
      stream_positions   the table row is the row's index in the CURRENT stream, not the token's place in the image
      rotate_prefix      the prefix rows are rotated too (prefix row t by table row n - 1 - t; row 0 of an axial table is the
                         identity); on a model without prefix rows this mutant IS the forward
      rotate_v           v is rotated like k
      other_layout       the other pairing of the elements
      sign_flipped       -sin in sin's place (the rotation run backwards)"""
    from oracle import rajni_oracle as orc
    assert mutant is None or mutant in MUTANTS, mutant
    schedule = orc.normalise_schedule(schedule)
    kind = cfg.norm
    query = query or nq.default_query(cfg)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    Pn = cfg.num_prefix_tokens
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    layout = HALF if cfg.rope_half else INTERLEAVED
    if mutant == "other_layout":
        layout = HALF + INTERLEAVED - layout
    tables = np.asarray(tables, np.float64)
    if mutant == "sign_flipped":
        tables = np.concatenate([-tables[..., :D], tables[..., D:]], -1)
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B, n = x.shape[0], x.shape[1]
    assert tables.shape[-2] == n and tables.shape[-1] == 2 * D, (tables.shape, n, D)
    if cfg.embed_norm:
        x = nr._norm(x, sd, "patch_embed.norm", eps, dtype, kind)
    if cfg.abs_pos:
        x = nq.pos_embedded_tokens(sd, x, cfg, dtype)
    else:
        prefix = ([W("cls_token").expand(B, -1, -1)] if cfg.class_token else []) + \
                 ([W("reg_token").expand(B, -1, -1)] if cfg.reg_tokens else [])
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
        qkv = nr._linear(xn, sd, p + "attn.qkv", dtype).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        if mutant != "no_rope":
            emb_i = tables[i] if tables.ndim == 4 else tables
            rows = table_rows(B, N, Pn, None if mutant == "stream_positions" else src)
            pre = (n - 1 - np.arange(Pn)) if mutant == "rotate_prefix" else None
            q, k = _rotate(q, emb_i, rows, Pn, layout, dtype, pre), _rotate(k, emb_i, rows, Pn, layout, dtype, pre)
            if mutant == "rotate_v":
                v = _rotate(v, emb_i, rows, Pn, layout, dtype)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                flat = host(torch.stack([q, k, v], 2).reshape(B, N, 3 * C))
                full = nq.importance_scores(flat, H, dtype=np_dt, query=query)
                if budget_dt:
                    full_bud = nq.importance_budget(flat, H, budget_dt, query=query)[1]
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
        att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5, dim=-1)
        out = nr._linear(torch.einsum("bhqk,bkhd->bqhd", att, v).reshape(B, -1, C), sd, p + "attn.proj", dtype)
        x = x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = nr._mlp(nr._norm(x, sd, p + "norm2", eps, dtype, kind), sd, p, cfg, dtype)
        x = x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
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


def feature_outputs(sd, images, schedule, cfg, tables, forced_keep=None, caps=(), dtype=torch.float64):
    """tests/numerics_rmsnorm.py::feature_outputs on this file's graph"""
    (tokens, states, _), counts, trace = vit_forward_restated(sd, images, schedule, cfg, tables, forced_keep=forced_keep, dtype=dtype,
                                                              features="states")
    B, n0, depth = tokens.shape[0], counts[0], cfg.depth
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    src = nq.source_idx(trace, B, n0)
    dense = nq.scatter_dense(tokens, src, n0)
    dense_last, exit_block = dense.copy(), np.full((B, n0), depth, np.int32)
    for i in sorted(trace):
        assert i > 0
        before = nq.source_idx(trace, B, n0, upto=i - 1)
        entry = host(nr._norm(states[i - 1], sd, "norm", cfg.ln_eps, dtype, cfg.norm))
        kept = np.zeros(before.shape, bool)
        np.put_along_axis(kept, trace[i]["keep_idx"], True, axis=1)
        for b in range(B):
            dense_last[b, before[b, ~kept[b]]] = entry[b, ~kept[b]]
            exit_block[b, before[b, ~kept[b]]] = i
    slabs = {c: nq.scatter_dense(host(states[c]), nq.source_idx(trace, B, n0, upto=c), n0) for c in caps}
    return dict(tokens=tokens, source_idx=src, dense=dense, dense_last=dense_last, exit_block=exit_block, slabs=slabs,
                counts=counts, trace=trace)


# ---------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------
# Both schedules prune in block 1, so blocks 2 and 3 rotate a pruned stream: row t of it is no longer patch t, which is what the
# stream_positions mutant gets wrong.  (Block 0 is left alone: tests/numerics_noclass.py's feature helpers keep no state in
# front of it.)  CARRIED re-ranks block 1's scores in block 2 without rescoring (update = False).
SCHED = {1: {"keep_ratio": 0.5, "update": True}, 2: {"keep_ratio": 0.75, "update": True}}
CARRIED = {1: {"keep_ratio": 0.5, "update": True}, 2: {"keep_ratio": 0.75, "update": False}}
FIX_BASE = nq.FIX_BASE
GAP_FACTOR = nq.GAP_FACTOR
BAR = nr.BAR                       # tests/test_gpu_rmsnorm_forward.py's bars, per dtype: 1e-2 x max|logit| for 16-bit, 1e-3 for fp32
MUTANT_FACTOR = 4.0                # every mutant moves the logits by at least this many bars (the 16-bit bar: the widest)
# ... and a fixture must not be one the 16-bit format alone pushes to the bar (tests/numerics_rmsnorm.py's rule and constant):
# torch's own bf16 forward of the module on the CPU stays within this share of the bf16 bar at B = 1 and B = 3
FORMAT_HEADROOM = nr.FORMAT_HEADROOM
BATCH = 3
MICRO = ["vit_micro_rope_patch16_64", "vit_micro_rope_half_reg4_patch16_64", "vit_micro_rope_mixed_gap_patch16_64",
         "vit_micro_rope_d40_patch14_56"]
# (weight seed, image seed = weight seed + 4) per micro config: the first weight seed from 1 up with the property that, on the
# B = 3 batch under SCHED in the fp64 restatement, every boundary gap is at least GAP_FACTOR bf16 score budgets AND every mutant
# moves the logits by at least MUTANT_FACTOR x BAR["bf16"] x max|logit| - and, for the fixtures that also run under CARRIED or at
# 48 x 96 (EXTRA), the same there - AND whose format cost is within FORMAT_HEADROOM.  tests/test_rope_cpu.py asserts all of it of the committed seeds; search_seeds finds them (a few
# minutes for the four).  The format criterion is what moves three of them off seed 1: torch's own bf16 forward of the seed-1
# fixtures is 1.19 % (half_reg4, B = 3) and 1.19 % / 1.08 % (d40, B = 1 / 3) off its fp32 one - over the bar before any kernel
# has run - and 0.80 % on the first gap-clean seed of the plain model.
# The walk, seed by seed, up to the committed one (f = format cost in % of the output scale, limit 0.80; g = the smallest
# boundary gap in bf16 score budgets, limit 8 - a figure printed as 8.0 lies just under it; m = the smallest mutant separation in %,
# limit 4; the first criterion that fails is the one recorded):
#   vit_micro_rope_patch16_64:
#     1:f0.84 2:f0.99 3:f1.01 4:f1.05 5:f1.06 6:f0.80 7:g1.0 8:f0.90 9:g0.2 10:g8.0 11:f0.84 12:f1.12 13:g1.7 14:f0.84
#     15:f0.81 16:g3.4 17:f0.81 18:g2.6 19:g4.8 20:f0.82 21:f1.08 22:f0.86 23:f1.21 24:f0.81 25:g0.7 26:g2.4 27:f1.25 28:f0.90
#     29:f1.08 30:f0.94 31:f0.83 32:f0.93 33:f0.93 34:g2.0 35:f1.43 36:f1.71 37:f0.80 38:g1.6 39:f0.98 40:f0.91 41:f0.88
#     42:f0.81 43:f1.12 44:g1.5 45:g3.8 46:g5.7 47:f0.97 48:f0.85 49:g1.2 50:f1.93 51:f0.87
#   vit_micro_rope_half_reg4_patch16_64:
#     1:f1.19 2:f0.88 3:f1.37 4:f1.24 5:g8.0 6:f1.28 7:g1.7 8:f1.22 9:f0.93 10:f1.39 11:f1.53 12:f1.22 13:f0.80 14:m2.77
#     15:f1.00 16:g0.9 17:f0.99 18:f1.12 19:f1.06 20:f1.55 21:f1.23 22:f0.94 23:f1.05 24:f0.87 25:g2.9 26:f1.08 27:f1.38
#     28:g3.7 29:g0.8 30:f2.00 31:g6.2 32:g5.2 33:f1.16 34:f1.30 35:f1.09 36:f0.94 37:f0.82 38:f1.29 39:f1.20 40:f1.24 41:g7.9
#     42:f1.74 43:f1.11 44:f1.51 45:f1.14 46:g2.4 47:f0.99 48:f1.67 49:g2.8 50:g3.3
#   vit_micro_rope_mixed_gap_patch16_64: seed 1 has the property
#   vit_micro_rope_d40_patch14_56:
#     1:f1.19 2:f1.08 3:f1.75 4:f1.38 5:f0.98 6:f1.58 7:f1.52 8:f1.97 9:f1.20 10:f1.13 11:f1.23
SEEDS = {
    "vit_micro_rope_patch16_64": (52, 56),
    "vit_micro_rope_half_reg4_patch16_64": (51, 55),
    "vit_micro_rope_mixed_gap_patch16_64": (1, 5),
    "vit_micro_rope_d40_patch14_56": (12, 16),
}
# the other (schedule, input size) pairs a fixture runs under on the device, beside (SCHED, its own size)
EXTRA = {
    "vit_micro_rope_patch16_64": [("CARRIED", None), ("SCHED", (48, 96))],
}
SCHEDULES = {"SCHED": SCHED, "CARRIED": CARRIED}


def build_model(name_or_cfg, wseed=None):
    """the timm-shaped module of a fixture: bf16-representable weights at the project's scale"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg
    seed = SEEDS[name_or_cfg][0] if wseed is None else wseed
    return ts.create_model(cfg, seed=seed, round_bf16=True, **FIX_BASE)


@functools.lru_cache(maxsize=None)
def fixture(name, wseed=None):
    """(config, fp32 state dict with bf16-representable values, image seed, rotary table of the model's grid) - built once,
    never modified"""
    from rajni_amd import timm_shaped as ts
    m = build_model(name, wseed)
    iseed = SEEDS[name][1] if wseed is None else wseed + 4
    return m.cfg, ts.state_dict_numpy(m), iseed, model_tables(m)


images_of = nq.images_of


def grid_of(cfg, size=None):
    h, w = size or (cfg.img_size, cfg.img_size)
    return h // cfg.patch_size, w // cfg.patch_size


@functools.lru_cache(maxsize=None)
def case(name, sched="SCHED", size=None, B=BATCH, wseed=None, pos_dt=None):
    """(sd for the input's grid, images, tables for the input's grid, the fp64 free-running forward (logits, counts, trace)).
    `pos_dt`: the model dtype a resampled position embedding is rounded to (tests/numerics_image.py::sd_at_grid)"""
    import numerics_image as ni
    cfg, sd, iseed, tables = fixture(name, wseed)
    if size is not None:
        sd = ni.sd_at_grid(sd, cfg, grid_of(cfg, size), dt=pos_dt)
        tables = model_tables(build_model(name, wseed), grid_of(cfg, size))
    imgs = images_of(cfg, B, iseed, size)
    return sd, imgs, tables, vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, tables)


def boundary_gap_ratios(name, sched="SCHED", size=None, B=BATCH, wseed=None, dt="bf16"):
    """tests/numerics_noclass.py::boundary_gap_ratios on this file's graph"""
    cfg = fixture(name, wseed)[0]
    sd, imgs, tables, _ = case(name, sched, size, B, wseed)
    _, _, tr = vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, tables, budget_dt=dt)
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
    """a mutant that IS the forward on this config: rotate_prefix without prefix rows"""
    return mutant == "rotate_prefix" and cfg.num_prefix_tokens == 0


def mutant_separations(name, sched="SCHED", size=None, B=BATCH, wseed=None):
    """{mutant: max |logits - mutant's logits| / max |logits|} in fp64, the mutant under the forward's own selections"""
    cfg = fixture(name, wseed)[0]
    sd, imgs, tables, (want, _, tr) = case(name, sched, size, B, wseed)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    out = {}
    for mut in MUTANTS:
        other, _, _ = vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, tables, forced_keep=forced, mutant=mut)
        out[mut] = float(np.abs(want - other).max() / np.abs(want).max())
    return out


def format_cost(name, wseed, B, dtype=torch.bfloat16):
    """tests/numerics_rmsnorm.py::format_cost on this file's fixtures: max |d| / max |out| between the stock forward in fp32 and
    torch's own forward of the same module in `dtype` on the CPU"""
    cfg = fixture(name, wseed)[0]
    imgs = torch.from_numpy(images_of(cfg, B, wseed + 4))
    with torch.no_grad():
        a = build_model(name, wseed)(imgs).numpy()
        b = build_model(name, wseed).to(dtype)(imgs.to(dtype)).float().numpy()
    return float(np.abs(a - b).max() / np.abs(a).max())


def holds(name, wseed):
    """the property SEEDS is chosen for, at weight seed `wseed`"""
    cfg = fixture(name, wseed)[0]
    if max(format_cost(name, wseed, B) for B in (1, BATCH)) > FORMAT_HEADROOM * BAR["bf16"]:
        return False
    for sched, size in [("SCHED", None)] + EXTRA.get(name, []):
        if boundary_gap_ratios(name, sched, size, wseed=wseed) < GAP_FACTOR:
            return False
        sep = mutant_separations(name, sched, size, wseed=wseed)
        if any(v < MUTANT_FACTOR * BAR["bf16"] for m, v in sep.items() if not vacuous(cfg, m)):
            return False
    return True


def search_seeds(name, limit=120):
    """the first weight seed from 1 up with the property (image seed = weight seed + 4)"""
    for seed in range(1, limit + 1):
        if holds(name, seed):
            return seed, seed + 4
    raise AssertionError(name)
