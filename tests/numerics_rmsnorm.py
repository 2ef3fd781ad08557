"""Yardsticks for RMSNorm trunks and the patch-embedding norm (include/rajni_hip_norm.h; the AIMv2 image towers), pure numpy /
torch-CPU, shared by tests/test_rmsnorm_cpu.py and the tests/test_gpu_rmsnorm_*.py files.

The reference has neither, so the rule is the project's own, restated here:
  rms(x)[c]  = x[c] * rsqrt(mean_c x[c]^2 + eps) * w[c]            no mean, no bias, eps inside the root
  embed norm   x[b, P + j] = norm(conv(patch j) + conv_bias) + pos[pos_off + j]; prefix rows are not normalised
  one kind per model: norm1, norm2, norm, fc_norm, norm_pre and patch_embed.norm; q/k-norm stays a LayerNorm.
The forward is tests/numerics_noclass.py::vit_forward_restated with the norm kind, the embedding norm, the gated MLPs of
tests/numerics_swiglu.py, optional linear biases and a headless tail added; everything else is that function's."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import numerics as nm
import numerics_noclass as nq
import numerics_prefix as npx
from numerics_variants import _t, _ln, _lane_tree

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------
# the row kernels
# ---------------------------------------------------------------------------------------------------------------
# c_rms: multiple of u32 * max|w| * |n| an fp32 RMSNorm may be off by (n = x * rsqrt(mean x^2 + eps)).  RMSNorm subtracts
# nothing, so there is no cancellation and no kappa term: a sum of C non-negative squares carries a relative error of a few
# u32 whatever the order, the root halves it, and two multiplies follow.  The constant is MEASURED like numerics.C_LN, against
# two references and never against the kernel, over nm.LN_ROW_COUNTS x (nm.LN_C + [2048]) x {bf16, fp16, fp32} inputs, on the
# unrounded fp32 results (tests/test_rmsnorm_cpu.py::test_c_rms_is_three_times_the_references re-measures both):
#   torch CPU fp32 F.rms_norm                                 c <= 5.03
#   numpy, per-lane chunk sums then a 64-lane butterfly       c <= 6.13
# (every case of nm.layernorm_rows needs 2.5 .. 4 at C = 2048: the sum's own rounding, not one stress row, sets the value)
# c_rms = the ceiling of 3 x the larger: the margin covers fused multiply-adds in the sum and the hardware rsqrt.
C_RMS_MEASURED = {"torch_cpu_fp32": 5.03, "butterfly64": 6.13}
C_RMS = float(math.ceil(3 * max(C_RMS_MEASURED.values())))
RMS_C = list(nm.LN_C) + [2048]
EPS = 1e-5


def rms64(x, w, eps):
    x64 = np.asarray(x, np.float64)
    n = x64 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + eps)
    return n, n * np.asarray(w, np.float64)


def rmsnorm_budget(x, w, eps, out_dt, c_rms=C_RMS):
    """(want, budget): |err| <= u_out |want| + c_rms u32 max|w| |n| + floor"""
    n, want = rms64(x, w, eps)
    return want, nm.UNIT[out_dt] * np.abs(want) + c_rms * nm.U32 * np.abs(w).max() * np.abs(n) + nm.FLOOR[out_dt]


def rmsnorm_needed_c(y32, x, w, eps):
    """smallest c_rms for which the UNROUNDED fp32 result y32 of a reference implementation meets the budget"""
    n, want = rms64(x, w, eps)
    unit = nm.U32 * np.abs(w).max() * np.abs(n)
    err = np.abs(y32.astype(np.float64) - want)
    ok = unit > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / unit[ok]).max())


def rms_torch(x, w, eps=EPS):
    xt = torch.from_numpy(np.asarray(x, F32))
    return torch.nn.functional.rms_norm(xt, (xt.shape[-1],), torch.from_numpy(np.asarray(w, F32)), eps).numpy()


def emul_rmsnorm(x, w, eps=EPS, mutant=None):
    """rows x [R, C] fp32 values -> the kernels' fp32 result, operation by operation: chunk c of 8 elements sits in lane c % 64;
    a lane adds the squares of its chunks in ascending order, elements in order; a 64-lane butterfly; rsqrt(sum / C + eps);
    (x * rstd) * w.  Mutants: "layernorm" subtracts the mean (b = 0), "eps_outside" computes 1 / (sqrt(ms) + eps),
    "short_sum" leaves the last chunk out of the sum."""
    x = np.asarray(x, F32)
    R, C = x.shape
    nchunk = C // 8
    ch = x.reshape(R, nchunk, 8)

    def wave_sum(vals, upto):
        lane = np.zeros((R, 64), F32)
        for c in range(upto):
            for j in range(8):
                lane[:, c % 64] = (lane[:, c % 64] + vals[:, c, j]).astype(F32)
        return _lane_tree(lane, (32, 16, 8, 4, 2, 1))

    if mutant == "layernorm":
        mean = (wave_sum(ch, nchunk) / F32(C)).astype(F32)
        ch = (ch - mean[:, None, None]).astype(F32)
        x = ch.reshape(R, C)
    ms = (wave_sum((ch * ch).astype(F32), nchunk - 1 if mutant == "short_sum" else nchunk) / F32(C)).astype(F32)
    if mutant == "eps_outside":
        rstd = (F32(1.0) / (np.sqrt(ms).astype(F32) + F32(eps))).astype(F32)
    else:
        rstd = (F32(1.0) / np.sqrt((ms + F32(eps)).astype(F32))).astype(F32)
    return ((x * rstd[:, None]).astype(F32) * np.asarray(w, F32)).astype(F32)


MUTANTS = ("layernorm", "eps_outside", "short_sum")


def embed_norm64(x, w, b, pos, eps, kind):
    """fp64: norm(x) + pos for rows x [R, C]; (n, want).  kind "rms" takes w only, "layernorm" w, b (None = 0) and the mean"""
    x64 = np.asarray(x, np.float64)
    if kind == "rms":
        n, y = rms64(x64, w, eps)
    else:
        mu = x64.mean(axis=-1, keepdims=True)
        n = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(axis=-1, keepdims=True) + eps)
        y = n * np.asarray(w, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
    return n, y + np.asarray(pos, np.float64)


def embed_norm_budget(x, w, b, pos, eps, kind, out_dt):
    """(want, budget): the norm's own budget (rmsnorm_budget's, or numerics.layernorm_budget's with its kappa term) without
    its output rounding, plus ONE rounding of the sum: the fp32 add of the position row and the store's rounding to out_dt"""
    if kind == "rms":
        y, bud = rmsnorm_budget(x, w, eps, "fp32")
    else:
        y, bud = nm.layernorm_budget(np.asarray(x, F32), w, np.zeros_like(w) if b is None else b, eps, "fp32")
    want = y + np.asarray(pos, np.float64)
    return want, bud + nm.U32 * np.abs(want) + nm.UNIT[out_dt] * np.abs(want) + nm.FLOOR[out_dt]


# ---------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------

def _norm(x, sd, prefix, eps, dtype, kind):
    if kind == "rms":
        w = _t(sd[prefix + ".weight"], dtype)
        return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w
    if prefix + ".bias" not in sd:          # (the LayerNorm substituted for an RMSNorm: b = 0)
        sd = {**sd, prefix + ".bias": np.zeros_like(sd[prefix + ".weight"])}
    return _ln(x, sd, prefix, eps, dtype)


def _linear(x, sd, name, dtype):
    y = x @ _t(sd[name + ".weight"], dtype).T
    return y + _t(sd[name + ".bias"], dtype) if name + ".bias" in sd else y


def _mlp(h, sd, p, cfg, dtype):
    if cfg.mlp == "swiglu":
        h = torch.nn.functional.silu(_linear(h, sd, p + "mlp.fc1_g", dtype)) * _linear(h, sd, p + "mlp.fc1_x", dtype)
    elif cfg.mlp == "swiglu_packed":
        g, v = _linear(h, sd, p + "mlp.fc1", dtype).chunk(2, dim=-1)
        h = torch.nn.functional.silu(g) * v
    else:
        h = _linear(h, sd, p + "mlp.fc1", dtype)
        h = h * torch.sigmoid(1.702 * h) if cfg.act == "quick_gelu" else torch.nn.functional.gelu(h)
    return _linear(h, sd, p + "mlp.fc2", dtype)


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, query=None, features=None,
                         budget_dt=None, norm=None, embed_norm=None):
    """(logits [B, classes] - or the pooled feature [B, C] of a headless model -, token counts, trace) of the pruned graph.
    `norm` / `embed_norm` override cfg.norm / cfg.embed_norm: the SUBSTITUTED graphs the fixtures are held apart from (a
    LayerNorm with b = 0 in an RMSNorm's place; the embedding norm left out).  `features` and `budget_dt` are
    tests/numerics_noclass.py::vit_forward_restated's."""
    from oracle import rajni_oracle as orc
    schedule = orc.normalise_schedule(schedule)
    kind = norm or cfg.norm
    with_embed_norm = cfg.embed_norm if embed_norm is None else embed_norm
    query = query or nq.default_query(cfg)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    Pn = cfg.num_prefix_tokens
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    if with_embed_norm:
        x = _norm(x, sd, "patch_embed.norm", eps, dtype, kind)
    x = nq.pos_embedded_tokens(sd, x, cfg, dtype)
    if cfg.pre_norm:
        x = _norm(x, sd, "norm_pre", eps, dtype, kind)
    scores, counts, trace, states, bud, full_bud = None, [], {}, {}, None, None
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _norm(x, sd, p + "norm1", eps, dtype, kind)
        qkv = _linear(xn, sd, p + "attn.qkv", dtype).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
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
        else:
            scores = None
        att = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5, dim=-1)
        out = _linear(torch.einsum("bhqk,bkhd->bqhd", att, v).reshape(B, -1, C), sd, p + "attn.proj", dtype)
        x = x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = _mlp(_norm(x, sd, p + "norm2", eps, dtype, kind), sd, p, cfg, dtype)
        x = x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
        states[i] = x
    raw = x
    if "norm.weight" in sd:
        x = _norm(x, sd, "norm", eps, dtype, kind)
    if features == "tokens":
        return host(x), counts, trace
    if features == "states":
        return (host(x), states, raw), counts, trace
    x = x[:, Pn:].mean(1) if cfg.global_pool == "avg" else x[:, 0]
    if cfg.use_fc_norm:
        x = _norm(x, sd, "fc_norm", eps, dtype, kind)
    if "head.weight" in sd:
        x = _linear(x, sd, "head", dtype)
    return host(x), counts, trace


def feature_outputs(sd, images, schedule, cfg, forced_keep=None, caps=(), dtype=torch.float64):
    """tests/numerics_noclass.py::feature_outputs on this file's graph: dict(tokens, source_idx, dense, dense_last, exit_block,
    slabs {c: the un-normalised stream behind block c on the unpruned grid, pruned rows zero}, counts, trace)"""
    (tokens, states, _), counts, trace = vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype,
                                                              features="states")
    B, n0, depth = tokens.shape[0], counts[0], cfg.depth
    host = lambda t: t.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    src = nq.source_idx(trace, B, n0)
    dense = nq.scatter_dense(tokens, src, n0)
    dense_last, exit_block = dense.copy(), np.full((B, n0), depth, np.int32)
    for i in sorted(trace):
        assert i > 0
        before = nq.source_idx(trace, B, n0, upto=i - 1)
        entry = host(_norm(states[i - 1], sd, "norm", cfg.ln_eps, dtype, cfg.norm))
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
SCHED = nq.SCHED
FIX_BASE = nq.FIX_BASE
GAP_FACTOR = nq.GAP_FACTOR
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}       # tests/test_gpu_noclass_forward.py's, per dtype
SEPARATION = 10.0                                        # a substituted graph moves the output by at least 10 x bar x max|out|
# An RMSNorm and a LayerNorm of a row without a mean are the same function, and randomly drawn weights give the stream rows
# next to none.  Every RMS fixture's position embedding therefore carries a constant (bf16-representable) on top of what was drawn:
# each stream row then has a mean of about that size next to a spread of about one.
POS_OFFSET = 0.5
# ... and a fixture must not be one the 16-bit format alone pushes to the bar: torch's own bf16 forward of the module on the CPU
# (format_cost, below) stays within this share of the bf16 bar at B = 1 and B = 3.  (A LayerNorm fixture gets no offset: its
# prefix rows would be near-constant rows, whose LayerNorm amplifies every rounding - torch's bf16 forward of such a fixture
# was 1.1 - 1.6 % off its fp32 one.)
FORMAT_HEADROOM = 0.8
MICRO = ["vit_micro_rms_patch16_64", "vit_micro_aimv2_patch16_64", "vit_micro_aimv2_d128_patch14_56",
         "vit_micro_reg4_embednorm_patch16_64"]
RMS_MICRO = MICRO[:3]
# (weight seed, image seed) per micro config: among weight seeds 1..40 the first whose smallest boundary gap - over the images
# of the B = 3 batch (image 0 is the B = 1 batch) and both scheduled blocks, in the fp64 restatement - is at least GAP_FACTOR
# times the bf16 score budget and whose format cost is within FORMAT_HEADROOM (tests/test_rmsnorm_cpu.py asserts both of the
# committed seeds, and search_seeds finds them)
SEEDS = {
    "vit_micro_rms_patch16_64": (25, 29),
    "vit_micro_aimv2_patch16_64": (5, 9),
    "vit_micro_aimv2_d128_patch14_56": (9, 13),
    "vit_micro_reg4_embednorm_patch16_64": (13, 17),
}


def build_model(name_or_cfg, wseed=None):
    """the timm-shaped module of a fixture: bf16-representable weights at the project's scale, POS_OFFSET on pos_embed"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg
    seed = SEEDS[name_or_cfg][0] if wseed is None else wseed
    m = ts.create_model(cfg, seed=seed, round_bf16=True, **FIX_BASE)
    if cfg.norm == "rms":
        with torch.no_grad():
            m.pos_embed.copy_(torch.from_numpy(ts.bf16_round_np(m.pos_embed.numpy() + np.float32(POS_OFFSET))))
    return m


def format_cost(cfg, wseed, iseed, B, dtype=torch.bfloat16):
    """max |d| / max |out| between the fixture's stock forward in fp32 and torch's own forward of the same module in `dtype` on
    the CPU - a cruder 16-bit model than the device's (its residual stream is 16-bit too), so an upper mark of what the format
    costs this fixture"""
    imgs = torch.from_numpy(images_of(cfg, B, iseed))
    with torch.no_grad():
        a = build_model(cfg, wseed)(imgs).numpy()
        b = build_model(cfg, wseed).to(dtype)(imgs.to(dtype)).float().numpy()
    return float(np.abs(a - b).max() / np.abs(a).max())


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(config, fp32 state dict with bf16-representable values, image seed) - built once, never modified"""
    from rajni_amd import timm_shaped as ts
    return ts.config_of(name), ts.state_dict_numpy(build_model(name)), SEEDS[name][1]


images_of = nq.images_of


def boundary_gap_ratios(sd, images, schedule, cfg, dt="bf16"):
    """tests/numerics_noclass.py::boundary_gap_ratios on this file's graph"""
    _, _, tr = vit_forward_restated(sd, images, schedule, cfg, budget_dt=dt)
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


def quiet_seed(cfg, iseed, B=3, limit=40):
    """the first weight seed whose format cost on that batch is within FORMAT_HEADROOM of the bf16 bar (fixtures that run with
    injected selections only: no boundary gap to hold)"""
    for seed in range(1, limit + 1):
        if format_cost(cfg, seed, iseed, B) <= FORMAT_HEADROOM * BAR["bf16"]:
            return seed
    raise AssertionError(cfg)


def search_seeds(name, limit=40):
    """the first weight seed (image seed = weight seed + 4) whose boundary gaps are at least GAP_FACTOR budgets"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name)
    for seed in range(1, limit + 1):
        sd = ts.state_dict_numpy(build_model(cfg, seed))
        if boundary_gap_ratios(sd, images_of(cfg, 3, seed + 4), SCHED, cfg) >= GAP_FACTOR and \
                max(format_cost(cfg, seed, seed + 4, B) for B in (1, 3)) <= FORMAT_HEADROOM * BAR["bf16"]:
            return seed, seed + 4
    raise AssertionError(name)


def separation(name, B=3, **substitute):
    """max |out - out_substituted| / max |out| of the fixture's fp64 outputs, under the fixture's own selections"""
    cfg, sd, iseed = fixture(name)
    imgs = images_of(cfg, B, iseed)
    want, _, tr = vit_forward_restated(sd, imgs, SCHED, cfg)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    other, _, _ = vit_forward_restated(sd, imgs, SCHED, cfg, forced_keep=forced, **substitute)
    return float(np.abs(want - other).max() / np.abs(want).max())
