"""Yardsticks for the norm inside the MLP and timm Eva's block layout (include/rajni_hip_mlpnorm.h; the EVA02 image towers), pure
numpy / torch-CPU in fp64, shared by tests/test_eva_cpu.py and the tests/test_gpu_eva_*.py / test_gpu_hidden_norm_kernel.py files.

The reference has none of it, so the rules are the project's own, restated here:
  mlp.norm   h = act(fc1(x)) (or silu(fc1_g(x)) * fc1_x(x));  h = norm(h) over the MLP's own width, of the model's one kind;
             y = fc2(h).  The statistics divide by the width n, never by the zero-padded width of the hidden buffer.
  Eva block  x += gamma_1 * attn(norm1(x));  x += gamma_2 * mlp(norm2(x))      (gamma None: 1)
  Eva qkv    one bias-free weight [3C, C] with the bias cat(q_bias, 0, v_bias), or q_proj / k_proj (no bias) / v_proj apart;
             the rows are q, k, v in that order.
The forward is tests/numerics_rope.py::vit_forward_restated (its helpers, operation for operation; the rotation only where the
config has one) with those three rules, and the mutants that a wrong reading of them would be."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import numerics as nm
import numerics_noclass as nq
import numerics_prefix as npx
import numerics_rmsnorm as nr
import numerics_rope as nrope
from numerics_variants import _t, _ln, _lane_tree

F32 = np.float32
CAP = 4096                      # RAJNI_HIDDEN_NORM_MAX

# ---------------------------------------------------------------------------------------------------------------
# the row kernel
# ---------------------------------------------------------------------------------------------------------------


def hidden_norm64(x, w, b, eps, n, kind):
    """fp64: rows x [R, ld] -> [R, ld] with columns [0, n) normalised over those n columns and the rest +0"""
    x64 = np.asarray(x, np.float64)[:, :n]
    out = np.zeros(np.asarray(x).shape, np.float64)
    if kind == "rms":
        out[:, :n] = x64 / np.sqrt((x64 * x64).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)
    else:
        mu = x64.mean(-1, keepdims=True)
        nrm = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + eps)
        out[:, :n] = nrm * np.asarray(w, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
    return out


def chain_length(n):
    """the longest chain of fp32 additions behind one of the kernel's sums: a lane adds the 8 elements of each of its
    ceil(ceil(n / 8) / 64) chunks in turn, then 6 butterfly steps"""
    return 8 * math.ceil(math.ceil(n / 8) / 64) + 6


def hidden_norm_budget(x, w, b, eps, n, kind, out_dt):
    """(want, budget) per element.  DERIVED, first order in u = 2^-24, from the row's own magnitudes - not measured on any
    implementation.  A sum of fp32 terms t_i along chains of at most L additions is off by at most L u sum|t_i| in any order.
      mean:  |d mean| <= em = (L + 1) u mean|x|                          (the sum, one division)
      d_i = x_i - mean:  |d d_i| <= em + u |d_i|
      var = sum d_i^2 / n:  relative error <= (L + 3) u + em^2 / (var + eps)   (a square and its operand's rounding, the sum, the
             division; the mean's error enters squared only, since sum d_i = 0); + eps and the root: rstd is off by half of that
             relatively, plus 4 u for the addition of eps, the hardware rsqrt (1 ulp) and slack
      n_i = d_i rstd:  |d n_i| <= (em + u |d_i|) rstd + |n_i| (rel(rstd) + u)
      y_i = fma(n_i, w_i, b_i): |w_i| |d n_i| + u |y_i|, then ONE rounding to the output type.
    RMS has no mean: em = 0, d_i = x_i, and the products (x rstd) w round twice."""
    x64 = np.asarray(x, np.float64)[:, :n]
    w64 = np.abs(np.asarray(w, np.float64))
    want = hidden_norm64(x, w, b, eps, n, kind)
    L, u = chain_length(n), nm.U32
    if kind == "rms":
        var = (x64 * x64).mean(-1, keepdims=True)
        d, em = x64, 0.0
    else:
        mu = x64.mean(-1, keepdims=True)
        d = x64 - mu
        var = (d * d).mean(-1, keepdims=True)
        em = (L + 1) * u * np.abs(x64).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    rel_rstd = 0.5 * ((L + 3) * u + em * em / (var + eps)) + 4 * u
    dn = (em + u * np.abs(d)) * rstd + np.abs(d) * rstd * (rel_rstd + u)
    bud = np.zeros_like(want)
    bud[:, :n] = w64 * dn + (u + nm.UNIT[out_dt]) * np.abs(want[:, :n]) + nm.FLOOR[out_dt]
    return want, bud


def worst(got, want, bud, n):
    """max |got - want| / budget over the columns [0, n) (the padding columns have no budget: they are held to +0 bit for bit)"""
    return nm.worst_ratio(np.asarray(got, np.float64)[:, :n], want[:, :n], bud[:, :n])[0]


def emul_hidden_norm(x, w, b, eps, n, kind, mutant=None):
    """rows x [R, ld] of fp32 values -> the kernel's UNROUNDED fp32 result, operation by operation: chunk c of 8 elements sits
    in lane c % 64; a lane adds its chunks in ascending order, elements in order (the elements past n of a partial chunk stay
    out); a 64-lane butterfly; two passes - the mean, then the squared deviations from it.  Mutants: "one_pass" takes the
    variance as E[x^2] - mean^2; "divisor_ld" divides both sums by ld."""
    x = np.asarray(x, F32)
    R, ld = x.shape
    nch = (n + 7) // 8
    xp = np.zeros((R, nch * 8), F32)
    xp[:, :n] = x[:, :n]
    valid = (np.arange(nch * 8) < n).reshape(nch, 8)
    div = F32(ld if mutant == "divisor_ld" else n)

    def wave_sum(vals):
        lane = np.zeros((R, 64), F32)
        for c in range(nch):
            for j in range(8):
                if valid[c, j]:
                    lane[:, c % 64] = (lane[:, c % 64] + vals[:, c, j]).astype(F32)
        return _lane_tree(lane, (32, 16, 8, 4, 2, 1))

    ch = xp.reshape(R, nch, 8)
    if kind == "rms":
        mean = np.zeros(R, F32)
        var = (wave_sum((ch * ch).astype(F32)) / div).astype(F32)
    else:
        mean = (wave_sum(ch) / div).astype(F32)
        if mutant == "one_pass":
            var = ((wave_sum((ch * ch).astype(F32)) / div).astype(F32) - (mean * mean).astype(F32)).astype(F32)
            var = np.maximum(var, F32(0))
        else:
            dev = (ch - mean[:, None, None]).astype(F32)
            var = (wave_sum((dev * dev).astype(F32)) / div).astype(F32)
    rstd = (F32(1.0) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
    out = np.zeros((R, ld), F32)
    nx = ((xp[:, :n] - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    w32 = np.asarray(w, F32)
    if kind == "rms":
        out[:, :n] = (nx * w32).astype(F32)
    else:      # the fused multiply-add rounds once: the product and the sum in fp64, then to fp32
        out[:, :n] = (nx.astype(np.float64) * w32 + (0.0 if b is None else np.asarray(b, F32).astype(np.float64))).astype(F32)
    return out


def kernel_rows(rows, n, ld, dt, seed=0):
    """x [rows, ld] rounded to dt with zeros in columns [n, ld), w, b fp32.  Rows cycle through: plain; a large mean with a small
    spread (100 +- 0.1; fp32: 1000 +- 0.05), which the two-pass form is for; one repeated value (zero variance); tiny values;
    a few massive elements."""
    rng = np.random.default_rng([seed, rows, n])
    x = np.zeros((rows, ld), F32)
    v = rng.standard_normal((rows, n), dtype=F32)
    names = []
    for r in range(rows):
        case = ("plain", "big_mean", "constant", "tiny", "massive")[r % 5]
        names.append(case)
        if case == "big_mean":
            v[r] = (1000.0 + 0.05 * v[r]) if dt == "fp32" else (100.0 + 0.1 * v[r])
        elif case == "constant":
            v[r] = F32(rng.uniform(-8, 8))
        elif case == "tiny":
            v[r] *= 1e-4
        elif case == "massive":
            v[r, rng.integers(n)] += 300.0
    x[:, :n] = v
    w = (1 + 0.1 * rng.standard_normal(n)).astype(F32)
    b = (0.1 * rng.standard_normal(n)).astype(F32)
    return nm.round_to(x, dt), np.array(names), w, b


# ---------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("no_mlp_norm", "divisor_ld", "norm_before_gate", "k_bias_nonzero", "gamma_ignored", "qkv_order")


def packed_qkv(sd, p, C, mutant=None):
    """(weight [3C, C], bias [3C]) of block prefix p in whichever spelling the state dict has, as float64 arrays"""
    zero = np.zeros(C)
    if p + "attn.qkv.weight" in sd:
        w = np.asarray(sd[p + "attn.qkv.weight"], np.float64)
        if p + "attn.q_bias" in sd:
            qb, vb = np.asarray(sd[p + "attn.q_bias"], np.float64), np.asarray(sd[p + "attn.v_bias"], np.float64)
            b = np.concatenate([qb, qb if mutant == "k_bias_nonzero" else zero, vb])
        else:
            b = np.asarray(sd[p + "attn.qkv.bias"], np.float64) if p + "attn.qkv.bias" in sd else np.zeros(3 * C)
            if mutant == "k_bias_nonzero":
                b = np.concatenate([b[:C], b[:C], b[2 * C:]])
    else:
        ws = [np.asarray(sd[p + f"attn.{n}.weight"], np.float64) for n in ("q_proj", "k_proj", "v_proj")]
        bs = [np.asarray(sd[p + f"attn.{n}.bias"], np.float64) if p + f"attn.{n}.bias" in sd else zero for n in ("q_proj", "k_proj", "v_proj")]
        if mutant == "k_bias_nonzero":
            bs[1] = bs[0]
        w, b = np.concatenate(ws), np.concatenate(bs)
    if mutant == "qkv_order":
        w, b = np.concatenate(np.split(w, 3)[::-1]), np.concatenate(np.split(b, 3)[::-1])
    return w, b


def _inner_norm(h, sd, p, cfg, dtype, n=None):
    """mlp.norm over the last axis of h; n: the statistics taken over n >= width columns, the ones past the width zeros (the
    divisor_ld mutant)"""
    width = h.shape[-1]
    w = _t(sd[p + "mlp.norm.weight"], dtype)
    n = n or width
    if cfg.norm == "rms":
        return h * torch.rsqrt((h * h).sum(-1, keepdim=True) / n + cfg.ln_eps) * w
    mu = h.sum(-1, keepdim=True) / n
    var = (((h - mu) ** 2).sum(-1, keepdim=True) + (n - width) * mu * mu) / n
    y = (h - mu) * torch.rsqrt(var + cfg.ln_eps) * w
    return y + _t(sd[p + "mlp.norm.bias"], dtype) if p + "mlp.norm.bias" in sd else y


def _mlp(h, sd, p, cfg, dtype, mutant=None):
    has_norm = p + "mlp.norm.weight" in sd and mutant != "no_mlp_norm"
    pad = (cfg.hidden_dim + 63) // 64 * 64 if mutant == "divisor_ld" else None
    if cfg.mlp == "swiglu":
        g, v = nr._linear(h, sd, p + "mlp.fc1_g", dtype), nr._linear(h, sd, p + "mlp.fc1_x", dtype)
    elif cfg.mlp == "swiglu_packed":
        g, v = nr._linear(h, sd, p + "mlp.fc1", dtype).chunk(2, dim=-1)
    else:
        g, v = nr._linear(h, sd, p + "mlp.fc1", dtype), None
    if has_norm and mutant == "norm_before_gate":      # the norm on the value (a plain MLP: on fc1's output), the gate behind it
        if v is None:
            g = _inner_norm(g, sd, p, cfg, dtype)
        else:
            v = _inner_norm(v, sd, p, cfg, dtype)
        has_norm = False
    if v is not None:
        h = torch.nn.functional.silu(g) * v
    else:
        h = g * torch.sigmoid(1.702 * g) if cfg.act == "quick_gelu" else torch.nn.functional.gelu(g)
    if has_norm:
        h = _inner_norm(h, sd, p, cfg, dtype, pad)
    return nr._linear(h, sd, p + "mlp.fc2", dtype)


def _gamma(sd, p, which, dtype, mutant):
    for name in (p + f"gamma_{which}", p + f"ls{which}.gamma"):
        if name in sd:
            return None if mutant == "gamma_ignored" else _t(sd[name], dtype)
    return None


def vit_forward_restated(sd, images, schedule, cfg, tables=None, forced_keep=None, dtype=torch.float64, query=None, features=None,
                         budget_dt=None, mutant=None):
    """(logits [B, classes], token counts, trace) of the pruned graph of an Eva-style model.  `tables`: the rotary table of the
    input's grid (numerics_rope.model_tables), None for a model without rope.  `mutant`: one of MUTANTS -
      no_mlp_norm        mlp.norm left out
      divisor_ld         its statistics divided by the zero-padded width of the hidden buffer (the padding columns are zeros)
      norm_before_gate   the norm applied to the value in front of the gate (a plain MLP: in front of the activation)
      k_bias_nonzero     k gets q's bias
      gamma_ignored      gamma_1 / gamma_2 (or ls1 / ls2) taken as 1
      qkv_order          the packed projection's thirds in the order v, k, q"""
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
    layout = nrope.HALF if cfg.rope_half else nrope.INTERLEAVED
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B, n = x.shape[0], x.shape[1]
    if tables is not None:
        tables = np.asarray(tables, np.float64)
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
        wq, bq = packed_qkv(sd, p, C, mutant)
        qkv = (xn @ _t(wq, dtype).T + _t(bq, dtype)).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        if tables is not None:
            emb_i = tables[i] if tables.ndim == 4 else tables
            rows = nrope.table_rows(B, N, Pn, src)
            q, k = nrope._rotate(q, emb_i, rows, Pn, layout, dtype), nrope._rotate(k, emb_i, rows, Pn, layout, dtype)
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
        g1, g2 = _gamma(sd, p, 1, dtype, mutant), _gamma(sd, p, 2, dtype, mutant)
        x = x + (out if g1 is None else out * g1)
        h = _mlp(nr._norm(x, sd, p + "norm2", eps, dtype, kind), sd, p, cfg, dtype, mutant)
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


def feature_outputs(sd, images, schedule, cfg, tables, forced_keep=None, caps=(), dtype=torch.float64):
    """tests/numerics_rope.py::feature_outputs on this file's graph"""
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
SCHED, CARRIED, SCHEDULES = nrope.SCHED, nrope.CARRIED, nrope.SCHEDULES
FIX_BASE = nq.FIX_BASE
# ... at embed dim 128.  The 320-wide fixture draws its linear weights at std 0.03: the hidden value of a gated MLP is a product of
# two pre-activations, and at std 0.08 the bf16 format alone puts torch's own forward of that model 1.2 % - 3.9 % off its fp32 one on
# every weight seed from 1 to 1270 (tests/numerics_swiglu.py lowers the std of its 512-wide fixture for the same reason).
FIX_WIDE = dict(FIX_BASE, std=0.03)


def fix_of(cfg):
    return FIX_BASE if cfg.embed_dim <= 128 else FIX_WIDE
GAP_FACTOR = nq.GAP_FACTOR
BAR = nr.BAR                       # the project's bars, per dtype: 1e-2 x max|logit| for 16-bit, 1e-3 for fp32
MUTANT_FACTOR = nrope.MUTANT_FACTOR
# ... in bars of the 16-bit forward tests, the widest - except the two mutants that are weak by construction, which are held to the
# same number of fp32 bars: the fp32 forward test (bar 1e-3) is the one that tells them from the forward.
#   k_bias_nonzero  a bias on k adds q_i . b to every score of query i, the same for every key, and the softmax does not see it:
#                   without rope the mutant IS the forward (vacuous, below), and with rope all that is left is the position
#                   dependence the rotation gives b - 0.4 % to 1.5 % of the logit scale over 200 weight seeds per rope fixture.
#   divisor_ld      344 (342) columns in a buffer of 384: the normalised hidden row comes out sqrt(384 / 344) - 1 = 5.7 % (6.0 %)
#                   too large, in one branch of the residual stream - 1.9 % to 3.8 % of the logit scale over the same seeds.  At
#                   16 bits it is the kernel test that catches this mutant, by orders of magnitude (tests/test_eva_cpu.py holds
#                   the restated kernel's divisor-ld form outside the derived budget).
MUTANT_BAR = {m: "bf16" for m in ("no_mlp_norm", "norm_before_gate", "gamma_ignored", "qkv_order")}
MUTANT_BAR.update(k_bias_nonzero="fp32", divisor_ld="fp32")


def mutant_bar(mutant):
    """the separation a live mutant must reach, as a share of max |logit|"""
    return MUTANT_FACTOR * BAR[MUTANT_BAR[mutant]]


FORMAT_HEADROOM = nr.FORMAT_HEADROOM
BATCH = 3
MAX_SKIPPED = 0                    # no (model, schedule) case is left out of the GPU tests for want of a clean seed
MICRO = ["vit_micro_eva_patch16_64", "vit_micro_eva_h342_patch16_64", "vit_micro_eva_rms_gap_patch16_64",
         "vit_micro_mlpnorm_patch16_64", "vit_micro_eva_d40_patch14_56"]
# (weight seed, image seed = weight seed + 4) per micro config: the first weight seed from 1 up with the property that, on the
# B = 3 batch under SCHED and under CARRIED (and, for EXTRA's fixture, at 48 x 96) in the fp64 restatement, every boundary gap is
# at least GAP_FACTOR bf16 score budgets AND every mutant that is not vacuous on the config moves the logits by at least its bar
# (mutant_bar), AND whose format cost (torch's own bf16 forward of the module on the CPU against its fp32 one, B = 1 and B = 3) is
# within FORMAT_HEADROOM of the bf16 bar - tests/numerics_rope.py's search and criteria.  tests/test_eva_cpu.py asserts all of it of
# the committed seeds; search_seeds finds them.
# The format criterion is what sends the search far: a gated MLP with a norm behind it rounds the hidden row twice, and torch's bf16
# forward of these models is 1.3 % - 2.5 % off its fp32 one on a median seed (0.80 % is the limit; of seeds 1..199 it leaves eva 5,
# h342 1, rms_gap 42, mlpnorm 18).  The fixtures are therefore QUIET ones, as tests/numerics_swiglu.py says of its own: their bars say
# that the norm and Eva's spellings are wired in correctly, not how far a typical bf16 model of this kind lands from its fp32 self.
SEEDS = {
    "vit_micro_eva_patch16_64": (2138, 2142),
    "vit_micro_eva_h342_patch16_64": (3201, 3205),
    "vit_micro_eva_rms_gap_patch16_64": (36, 40),
    "vit_micro_mlpnorm_patch16_64": (39, 43),
    "vit_micro_eva_d40_patch14_56": (4, 8),
}
# the (schedule, input size) pairs every fixture runs under on the device, and the one more of a single fixture
CASES = [("SCHED", None), ("CARRIED", None)]
EXTRA = {"vit_micro_eva_patch16_64": [("SCHED", (48, 96))]}


def build_model(name_or_cfg, wseed=None):
    """the timm-shaped module of a fixture: bf16-representable weights at the project's scale"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg
    seed = SEEDS[name_or_cfg][0] if wseed is None else wseed
    return ts.create_model(cfg, seed=seed, round_bf16=True, **fix_of(cfg))


def tables_of(model, grid=None):
    return nrope.model_tables(model, grid) if model.rope is not None else None


@functools.lru_cache(maxsize=None)
def fixture(name, wseed=None):
    """(config, fp32 state dict with bf16-representable values, image seed, rotary table of the model's grid or None) - built
    once, never modified"""
    from rajni_amd import timm_shaped as ts
    m = build_model(name, wseed)
    iseed = SEEDS[name][1] if wseed is None else wseed + 4
    return m.cfg, ts.state_dict_numpy(m), iseed, tables_of(m)


images_of = nq.images_of
grid_of = nrope.grid_of


@functools.lru_cache(maxsize=None)
def case(name, sched="SCHED", size=None, B=BATCH, wseed=None, pos_dt=None):
    """(sd for the input's grid, images, tables for the input's grid, the fp64 free-running forward (logits, counts, trace))"""
    import numerics_image as ni
    cfg, sd, iseed, tables = fixture(name, wseed)
    if size is not None:
        sd = ni.sd_at_grid(sd, cfg, grid_of(cfg, size), dt=pos_dt)
        tables = tables_of(build_model(name, wseed), grid_of(cfg, size))
    imgs = images_of(cfg, B, iseed, size)
    return sd, imgs, tables, vit_forward_restated(sd, imgs, SCHEDULES[sched], cfg, tables)


def boundary_gap_ratios(name, sched="SCHED", size=None, B=BATCH, wseed=None, dt="bf16"):
    """tests/numerics_noclass.py::boundary_gap_ratios on this file's graph: the smallest gap at a top-k boundary over every image
    and every scheduled block, in score budgets of `dt`"""
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


def vacuous(cfg, sd, mutant):
    """a mutant that IS the forward on this config: gamma_ignored without LayerScale, divisor_ld where the hidden buffer has no
    padding, k_bias_nonzero where k is not rotated (the softmax is invariant to a bias on k), the two norm mutants without mlp.norm"""
    if mutant == "k_bias_nonzero":
        return cfg.rope == "none"
    if mutant == "gamma_ignored":
        return not any(k.endswith(("gamma_1", "ls1.gamma")) for k in sd)
    if mutant == "divisor_ld":
        return cfg.hidden_dim % 64 == 0
    if mutant in ("no_mlp_norm", "norm_before_gate"):
        return not cfg.mlp_norm
    return False


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
    """tests/numerics_rmsnorm.py::format_cost on this file's fixtures"""
    cfg = fixture(name, wseed)[0]
    imgs = torch.from_numpy(images_of(cfg, B, wseed + 4))
    with torch.no_grad():
        a = build_model(name, wseed)(imgs).numpy()
        b = build_model(name, wseed).to(dtype)(imgs.to(dtype)).float().numpy()
    return float(np.abs(a - b).max() / np.abs(a).max())


def holds(name, wseed, verbose=False):
    """the property SEEDS is chosen for, at weight seed `wseed`"""
    cfg, sd = fixture(name, wseed)[:2]
    if max(format_cost(name, wseed, B) for B in (1, BATCH)) > FORMAT_HEADROOM * BAR["bf16"]:
        return False
    for sched, size in CASES + EXTRA.get(name, []):
        if boundary_gap_ratios(name, sched, size, wseed=wseed) < GAP_FACTOR:
            return False
        sep = mutant_separations(name, sched, size, wseed=wseed)
        if any(v < mutant_bar(m) for m, v in sep.items() if not vacuous(cfg, sd, m)):
            return False
    return True


def search_seeds(name, limit=200):
    """the first weight seed from 1 up with the property (image seed = weight seed + 4)"""
    for seed in range(1, limit + 1):
        ok = holds(name, seed)
        fixture.cache_clear(); case.cache_clear()
        if ok:
            return seed, seed + 4
    raise AssertionError(name)
