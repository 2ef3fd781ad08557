"""References, budgets and the yardstick graph for the gated MLP (SwiGLU): hidden = silu(g) * v with g, v the two halves of a
packed FC1, silu(t) = t * sigmoid(t) - timm's GluMlp(act_layer=nn.SiLU, gate_last=False) / SwiGLUPacked and its split twin
SwiGLU.  Pure numpy / torch-CPU, shared by tests/test_swiglu_cpu.py and tests/test_gpu_swiglu.py.

  silu64 / swiglu64       the fp64 functions (numerically stable at both ends)
  SILU_SLOPE              max |silu'| computed numerically, as numerics_activations.max_slope does (1.0998)
  budget_swiglu           the per-element budget of the GEMM tests (derived below)
  product32_envelope      the local error envelope of torch's CPU fp32 evaluation of silu(g) * v against fp64
  vit_forward_restated    tests/numerics_prefix.py's pruned graph (registers, LayerScale, no_embed_class) with the gated MLP
                          in its packed or split form, and two deliberate mistakes for the fixture-validity check
  vit_forward_ideal_bf16  the same graph with every stored activation rounded to bf16: what the FORMAT costs (the rule of
                          tests/numerics_distilled.py), by which the weight seeds are chosen
"""
from __future__ import annotations

import numpy as np
import torch

import numerics as nm
import numerics_activations as na
import numerics_prefix as npx
from numerics_variants import _ln, _t
from oracle import rajni_oracle as orc


def silu64(x):
    """x * sigmoid(x) in fp64; the sigmoid through exp(-|x|) so that neither end overflows"""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return x * np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def swiglu64(g, v):
    return silu64(g) * np.asarray(v, np.float64)


def swiglu_torch(g, v):
    """what timm's GluMlp computes from the two chunks, in their dtype"""
    return torch.nn.functional.silu(g) * v


_slope = []


def silu_slope():
    if not _slope:
        _slope.append(na.max_slope(silu64))
    return _slope[0]


# ---------------------------------------------------------------------------------------------------------------
# GEMM budget.  The kernel holds g' = g + eg and v' = v + ev with |eg| <= dg = g_acc S_g, |ev| <= dv = g_acc S_v (nm.gemm_pre:
# K products accumulated in fp32 in any order, the bias add and one more operation), evaluates s' = silu(g') (1 + small) with
# |s' - silu(g')| <= A, and rounds s' v' once to the output type.  With L = max |silu'|:
#   |s' v' - silu(g) v| <= |silu(g') - silu(g)| |v'| + |silu(g)| |ev| + A |v'|
#                       <= L dg (|v| + dv) + |silu(g)| dv + A (|v| + dv)
# and the output rounding adds u_out |want| (to first order) and the type's floor:
#   budget = u_out |want| + L dg (|v| + dv) + (|silu(g)| + A) dv + A |v| + floor
# ---------------------------------------------------------------------------------------------------------------

def budget_swiglu(g, v, Sg, Sv, gacc, out_dt, A):
    dg, dv = gacc * Sg, gacc * Sv
    want = swiglu64(g, v)
    return (nm.UNIT[out_dt] * np.abs(want) + silu_slope() * dg * (np.abs(v) + dv) + (np.abs(silu64(g)) + A) * dv + A * np.abs(v)
            + nm.FLOOR[out_dt])


def local_envelope(err, order_key):
    """running maximum of `err` over the 129 neighbouring points in the order of `order_key` (a single reference value may be
    exact by chance) - nm.gelu32_reference_error's construction"""
    err, key = np.asarray(err, np.float64).ravel(), np.asarray(order_key).ravel()
    order = np.argsort(key, kind="stable")
    pad = np.pad(err[order], 64, mode="edge")
    env = np.lib.stride_tricks.sliding_window_view(pad, 129).max(axis=1)
    out = np.empty_like(env)
    out[order] = env
    return out


def silu32_envelope(g32):
    """|torch CPU fp32 silu - fp64 silu| at the fp32 points g32, as a local envelope in g32's order and shape"""
    g32 = np.ascontiguousarray(g32, dtype=np.float32)
    got = torch.nn.functional.silu(torch.from_numpy(g32.ravel())).numpy().astype(np.float64)
    return local_envelope(np.abs(got - silu64(g32.ravel().astype(np.float64))), g32.ravel()).reshape(g32.shape)


def a_silu_fp32(g):
    """the fp32 epilogue's allowance for the gate (nm.a_gelu_fp32's rule): 4x the reference's own error, floor 2 u32 |silu|"""
    return np.maximum(4 * silu32_envelope(g.astype(np.float32)), 2 * nm.U32 * np.abs(silu64(g)))


def product32_envelope(g32, v):
    """|torch CPU fp32 silu(g) * v - fp64| for one fp32 value v over the fp32 points g32, as a local envelope over g (inf
    where the fp32 reference itself overflows)"""
    g32 = np.ascontiguousarray(g32, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        got = swiglu_torch(torch.from_numpy(g32), torch.tensor(np.float32(v))).numpy().astype(np.float64)
        err = np.abs(got - swiglu64(g32.astype(np.float64), np.float64(np.float32(v))))
    return local_envelope(np.where(np.isnan(err), np.inf, err), g32)


TYPE_MAX = {"bf16": 3.3895313892515355e38, "fp16": 65504.0, "fp32": float(np.finfo(np.float32).max)}


def sweep_values(dt):
    """the value half of the epilogue sweep: 1, -3, 0.37, 0 and the largest finite value of the type divided by 8, each as
    the type holds it (the bias is fp32, so 0.37 is the fp32 nearest)"""
    return [float(np.float32(x)) for x in (1.0, -3.0, 0.37, 0.0, TYPE_MAX[dt] / 8)]


def gemm_case(M, N, K, dt, seed=0):
    """operands of a gated launch - nm.gemm_operands for [2N, K], the value half drawn like the gate half - with the fp64
    pre-activations and accumulation bounds of each half: dict(x, w, b, g, v, Sg, Sv, gacc)"""
    x, w, b = nm.gemm_operands(M, 2 * N, K, dt, seed)
    return dict(x=x, w=w, b=b, **halves(x, w, b, N))


def halves(x, w, b, N):
    pre, S, gacc = nm.gemm_pre(x, w, b)
    return dict(g=pre[:, :N], v=pre[:, N:], Sg=S[:, :N], Sv=S[:, N:], gacc=gacc)


def assert_within_range(got, want, budget, dt, what):
    """nm.assert_within over the elements whose true value, with its budget, the output type can hold; beyond the type's
    range (fp16 products of two pre-activations reach it) the output may be the infinity of the right sign or the largest
    finite value - and is never NaN anywhere"""
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} NaN outputs"
    inside = np.abs(want) + budget <= TYPE_MAX[dt]
    out = ~inside
    if out.any():
        ok = (np.sign(got[out]) == np.sign(want[out])) & (np.abs(got[out]) >= TYPE_MAX[dt] * (1 - 2 * nm.UNIT[dt]) - budget[out])
        assert ok.all(), f"{what}: {int((~ok).sum())} outputs beyond the type's range are neither +-inf nor at its end"
    print(f"[swiglu] {what}: {int(out.sum())} of {got.size} true values beyond the range of {dt}")
    nm.assert_within(got[inside], want[inside], budget[inside], what)


# ---------------------------------------------------------------------------------------------------------------
# the yardstick for pruned forwards
# ---------------------------------------------------------------------------------------------------------------

def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _fc1_halves(sd, p, W, hidden):
    """(gate weight, gate bias, value weight, value bias) of block prefix p, from the packed or the split state dict"""
    if p + "mlp.fc1_g.weight" in sd:
        return W(p + "mlp.fc1_g.weight"), W(p + "mlp.fc1_g.bias"), W(p + "mlp.fc1_x.weight"), W(p + "mlp.fc1_x.bias")
    w, b = W(p + "mlp.fc1.weight"), W(p + "mlp.fc1.bias")
    assert w.shape[0] == 2 * hidden
    return w[:hidden], b[:hidden], w[hidden:], b[hidden:]


MODES = ("swiglu", "swapped", "no_gate")


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, mode="swiglu", ideal_bf16=False):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx / next_scores}) of the pruned graph of a
    gated-MLP config: numerics_prefix.vit_forward_restated (P = 1 + reg_tokens prefix tokens, LayerScale, no_embed_class) with
    hidden = silu(g) * v.  `mode` = "swapped" computes silu(v) * g and "no_gate" v alone - the two mistakes the fixtures must
    be able to tell.  `ideal_bf16` (fp64 only): every activation a 16-bit forward stores is rounded to bf16 and the residual
    stream to fp32 (numerics_distilled.vit_forward_ideal_bf16's rule)."""
    assert cfg.mlp in ("swiglu_packed", "swiglu") and not cfg.qk_norm and not cfg.pre_norm and cfg.global_pool == "token"
    assert not cfg.use_fc_norm and not cfg.distilled and mode in MODES and (not ideal_bf16 or dtype == torch.float64)
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    Pn = 1 + cfg.reg_tokens
    W = lambda n: _t(sd[n], dtype)
    r16 = _bf16 if ideal_bf16 else (lambda t: t)
    r32 = (lambda t: t.to(torch.float32).to(dtype)) if ideal_bf16 else (lambda t: t)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = r32(npx.pos_embedded_tokens(sd, x, cfg, dtype, Pn))
    scores, counts, trace = None, [], {}
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = r16(_ln(x, sd, p + "norm1", eps, dtype))
        qkv = r16(xn @ W(p + "attn.qkv.weight").T + W(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                full = orc.importance_scores(qkv.reshape(B, N, 3 * C).numpy(), H, dtype=np_dt)
            else:
                full = scores
            keep = npx.keep_count(sc["keep_ratio"], N, Pn)
            keep_idx = npx.select_tokens(full, keep, Pn) if forced_keep is None or i not in forced_keep \
                else np.asarray(forced_keep[i], np.int64)
            assert keep_idx.shape == (B, Pn + keep)
            scores = np.take_along_axis(full, keep_idx, axis=1)
            trace[i] = {"scores": full, "keep_idx": keep_idx, "next_scores": scores}
            gi = torch.from_numpy(keep_idx)[:, :, None, None].expand(-1, -1, H, D)
            q, k, v = q.gather(1, gi), k.gather(1, gi), v.gather(1, gi)
            x = x.gather(1, torch.from_numpy(keep_idx)[:, :, None].expand(-1, -1, C))
        else:
            scores = None
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5
        pm = r16(torch.exp(s - s.amax(-1, keepdim=True)))
        out = r16(torch.einsum("bhqk,bkhd->bqhd", pm, v) / pm.sum(-1).permute(0, 2, 1)[..., None]).reshape(B, -1, C)
        out = out @ W(p + "attn.proj.weight").T + W(p + "attn.proj.bias")
        x = r32(x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out))
        h = r16(_ln(x, sd, p + "norm2", eps, dtype))
        wg, bg, wv, bv = _fc1_halves(sd, p, W, cfg.hidden_dim)
        g_, v_ = h @ wg.T + bg, h @ wv.T + bv
        h = r16({"swiglu": lambda: swiglu_torch(g_, v_), "swapped": lambda: swiglu_torch(v_, g_), "no_gate": lambda: v_}[mode]())
        h = h @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias")
        x = r32(x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h))
    x = r16(_ln(x, sd, "norm", eps, dtype))[:, 0]
    logits = r16(x @ W("head.weight").T + W("head.bias"))
    return logits.numpy(), counts, trace


def gate_matters(sd, images, schedule, cfg):
    """fixture validity, fp32 on the CPU: max |dlogit| / max |logit| between the graph and the same graph - same selections -
    under each of the two mistakes: (halves swapped, gate dropped)"""
    full, _, tr = vit_forward_restated(sd, images, schedule, cfg, dtype=torch.float32)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    scale = float(np.abs(full).max())
    return tuple(float(np.abs(full - vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced, dtype=torch.float32,
                                                           mode=m)[0]).max()) / scale for m in ("swapped", "no_gate"))


def format_cost(sd, images, schedule, cfg):
    """max |ideal bf16 forward - fp64 graph| / max |logit| on the fp64 graph's own selections"""
    want, _, tr = vit_forward_restated(sd, images, schedule, cfg)
    got, _, _ = vit_forward_restated(sd, images, schedule, cfg, forced_keep={i: t["keep_idx"] for i, t in tr.items()}, ideal_bf16=True)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the forward fixtures tests/test_gpu_swiglu.py runs and tests/test_swiglu_cpu.py validates -------------------------------
# Weights: std 0.08 and bias_std 0.02 at embed dim 128, the distribution tests/numerics_distilled.py uses there.  At embed dim
# 512 that file's std 0.06 is not usable for a gated MLP at batch 64: the hidden value is a product of two pre-activations, and
# the bf16 FORMAT alone (format_cost below, CPU, no device) then costs 1.7 - 2.0 % of the logit scale on seeds 1 - 3, 1.0 - 1.3 %
# at std 0.04, 0.8 - 0.9 % at 0.03 and 0.4 - 0.5 % at 0.02.  The 512-wide fixture therefore uses std 0.02 - timm's own
# trunc_normal(.02) init and create_model()'s default - under which both mistakes still move the logits by 37 % and more of
# their scale.  The seed is chosen on the CPU alone, by that file's rule: the FIRST seed from 1 up for which, on
# every case of the model in FORWARD_CASES,
#   (a) each of the two mistakes (halves swapped, gate dropped) moves the fp32 logits by at least 5 x the fp32 bar (1e-3), and
#   (b) an ideal bf16 forward (the format's own cost, no device involved) stays within 0.75 x the 1e-2 bar.
# tests/test_swiglu_cpu.py::test_fixtures_can_tell_and_seeds_follow_the_rule re-derives every seed below from the rule.
# What this selection means: the rule turns down most draws (12 of the first 13 seeds for the register fixture, 4 or 5 of the
# first 6 for the other 128-wide ones), and the 512-wide fixture has smaller weights than the project's other 512-wide fixtures, so
# the forward fixtures are QUIET ones - chosen so that the bf16 format itself leaves room under the bar.  Their bars therefore say
# that the gated epilogue is wired into the model correctly (a swapped or missing gate moves the logits by 37 % and more), not
# how far a typical gated bf16 model lands from its fp32 self: on an arbitrary draw the format alone costs 0.8 - 2.5 % of the
# logit scale.  The numerical guarantee of the kernel is carried by the epilogue sweep and the per-element GEMM budgets.
STD = {128: dict(std=0.08, bias_std=0.02), 512: dict(std=0.02, bias_std=0.02)}
FORMAT_HEADROOM = 0.75
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}     # prunes at two blocks
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
# model -> [(pruned, batch, image seed)]: every forward the GPU file holds to a bar
FORWARD_CASES = {
    "vit_micro_swiglu_patch16_64": [(True, 3, 5), (False, 3, 2)],
    "vit_micro_swiglu_split_patch16_64": [(True, 3, 5)],
    "vit_micro_swiglu_h344_patch16_64": [(True, 3, 5)],
    "vit_micro_reg4_swiglu_patch14_56": [(True, 3, 5)],
    "vit_micro512_swiglu_patch16_64": [(True, 64, 5)],
}
SEEDS = {
    "vit_micro_swiglu_patch16_64": 6,              # 1 - 5 fail (b): the format costs 0.80 - 1.48 % on one of the two cases
    "vit_micro_swiglu_split_patch16_64": 3,        # 1, 2 fail (b): 0.79, 0.84 %
    "vit_micro_swiglu_h344_patch16_64": 5,         # 1 - 4 fail (b): 0.89 - 1.62 %
    "vit_micro_reg4_swiglu_patch14_56": 13,        # 1 - 12 fail (b): 0.75 - 1.52 %
    "vit_micro512_swiglu_patch16_64": 1,
}


def fix_of(name):
    from rajni_amd import timm_shaped as ts
    return dict(seed=SEEDS[name], **STD[ts.config_of(name).embed_dim])


def images_of(cfg, B, seed=2):
    from rajni_amd import timm_shaped as ts
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def seed_passes(name, seed):
    """(passes, [(moved_swapped, moved_no_gate, format cost) per case]) of the rule above for one candidate seed"""
    from rajni_amd import timm_shaped as ts
    cfg = ts.config_of(name)
    sd = ts.state_dict_numpy(ts.create_model(cfg, round_bf16=True, seed=seed, **STD[cfg.embed_dim]))
    figures = []
    for pruned, B, iseed in FORWARD_CASES[name]:
        imgs = images_of(cfg, B, iseed)
        sched = SCHED if pruned else {}
        a, b = gate_matters(sd, imgs, sched, cfg)
        figures.append((a, b, format_cost(sd, imgs, sched, cfg)))
    ok = all(a >= 5e-3 and b >= 5e-3 and c <= FORMAT_HEADROOM * 1e-2 for a, b, c in figures)
    return ok, figures


def first_seed(name, limit=40):
    for seed in range(1, limit + 1):
        if seed_passes(name, seed)[0]:
            return seed
    raise AssertionError(f"{name}: no seed up to {limit} passes the rule")
