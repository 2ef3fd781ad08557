"""References, budgets and the yardstick graph for the MLP activations beside exact GELU: QuickGELU, x * sigmoid(1.702 x) (the
OpenAI CLIP, MetaCLIP and DFN towers).  Pure numpy / torch-CPU, shared by tests/test_activations_cpu.py and
tests/test_gpu_activations.py.  Everything the exact-GELU tests have in tests/numerics.py has its twin here, built the same
way, so that the two activations are held to the same rules:

  quick_gelu64          the fp64 function (numerically stable at both ends)
  budget_act            nm.budget_gelu with the activation's own value and its own maximal slope, the slope computed
                        numerically from the fp64 function on a dense grid (1.0998 for QuickGELU, 1.129 for GELU)
  act32_reference_error the local error envelope of torch's CPU fp32 evaluation against fp64 (nm.gelu32_reference_error)
  a_act_fp32            the fp32 epilogue's allowance: 4x that envelope, floor 2 u32 |act|   (nm.a_gelu_fp32)
  vit_forward_restated  tests/numerics_variants.py's pruned graph with the activation as a callable
"""
from __future__ import annotations

import numpy as np
import torch

import numerics as nm
from numerics_variants import _ln, _t
from oracle import rajni_oracle as orc

QUICK_GELU_ALPHA = 1.702


def quick_gelu64(x):
    """x * sigmoid(1.702 x) in fp64; the sigmoid through exp(-|t|) so that neither end overflows"""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(QUICK_GELU_ALPHA * x))
    return x * np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def quick_gelu_torch(x):
    """what timm's / open_clip's QuickGELU module computes, in x's dtype"""
    return x * torch.sigmoid(QUICK_GELU_ALPHA * x)


ACT64 = {"gelu": orc.gelu, "quick_gelu": quick_gelu64}
ACT_TORCH = {"gelu": torch.nn.functional.gelu, "quick_gelu": quick_gelu_torch}


def max_slope(act64, lo=-12.0, hi=12.0, n=2_400_001):
    """max |act'(x)| on [lo, hi], by central differences of the fp64 function on a dense grid (h = 1e-5: the truncation error
    h^2 |act'''| / 6 is below 1e-10, the rounding error 2^-52 |act| / h below 1e-9)"""
    x = np.linspace(lo, hi, n)
    h = 1e-5
    return float(np.abs((act64(x + h) - act64(x - h)) / (2 * h)).max())


_slopes = {}


def slope_of(kind):
    if kind not in _slopes:
        _slopes[kind] = max_slope(ACT64[kind])
    return _slopes[kind]


def budget_act(kind, pre, S, g, out_dt, a_act):
    """nm.budget_gelu for the activation `kind`: one output rounding of the true value, the GEMM's accumulation error g S
    carried through the activation's steepest slope, the activation's own allowance and the output type's floor"""
    return nm.UNIT[out_dt] * np.abs(ACT64[kind](pre)) + slope_of(kind) * g * S + a_act + nm.FLOOR[out_dt]


def act32_reference_error(kind, x32):
    """|torch CPU fp32 act - fp64 act| at the fp32 points x32 as a LOCAL envelope: the running maximum over the 129
    neighbouring points of the sorted grid (a single reference value may be exact by chance), in x32's order - built exactly
    like nm.gelu32_reference_error"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).ravel()
    order = np.argsort(x32, kind="stable")
    xs = x32[order]
    err = np.abs(ACT_TORCH[kind](torch.from_numpy(xs)).numpy().astype(np.float64) - ACT64[kind](xs.astype(np.float64)))
    pad = np.pad(err, 64, mode="edge")
    env = np.lib.stride_tricks.sliding_window_view(pad, 129).max(axis=1)
    out = np.empty_like(env)
    out[order] = env
    return out


def a_act_fp32(kind, pre):
    """the fp32 epilogue's allowance (nm.a_gelu_fp32's rule): 4x the reference's own error, floor 2 u32 |act|"""
    p32 = pre.astype(np.float32)
    return np.maximum(4 * act32_reference_error(kind, p32).reshape(pre.shape), 2 * nm.U32 * np.abs(ACT64[kind](pre)))


def sweep_grid(dt):
    """nm.gelu_grid() plus the largest finite value of the type, both signs"""
    top = {"bf16": 3.3895313892515355e38, "fp16": 65504.0, "fp32": float(np.finfo(np.float32).max)}[dt]
    return np.concatenate([nm.gelu_grid(), np.float32([top, -top])]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the yardstick for pruned forwards: numerics_variants.vit_forward_restated with the MLP activation as a callable
# (that one hard-codes gelu).  Plain token-head models with or without norm_pre: what the QuickGELU configs are.
# ---------------------------------------------------------------------------------------------------------------

def vit_forward_restated(sd, images, schedule, cfg, act, forced_keep=None, dtype=torch.float64):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx / next_scores}); `act`: torch callable"""
    assert not cfg.qk_norm and cfg.global_pool == "token" and not cfg.use_fc_norm and not cfg.reg_tokens
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    P = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), P("patch_embed.proj.weight"), P("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    cls = P("cls_token").expand(B, -1, -1)
    x = torch.cat([cls, x + P("pos_embed")], 1) if cfg.no_embed_class else torch.cat([cls, x], 1) + P("pos_embed")
    if cfg.pre_norm:
        x = _ln(x, sd, "norm_pre", eps, dtype)
    scores, counts, trace = None, [], {}
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _ln(x, sd, p + "norm1", eps, dtype)
        qkv = (xn @ P(p + "attn.qkv.weight").T + P(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                full = orc.importance_scores(qkv.reshape(B, N, 3 * C).numpy(), H, dtype=np_dt)
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
        out = out @ P(p + "attn.proj.weight").T + P(p + "attn.proj.bias")
        x = x + (out * P(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = _ln(x, sd, p + "norm2", eps, dtype)
        h = act(h @ P(p + "mlp.fc1.weight").T + P(p + "mlp.fc1.bias"))
        h = h @ P(p + "mlp.fc2.weight").T + P(p + "mlp.fc2.bias")
        x = x + (h * P(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
    x = _ln(x, sd, "norm", eps, dtype)[:, 0]
    logits = x @ P("head.weight").T + P("head.bias")
    return logits.numpy(), counts, trace


def activation_moves_logits(sd, imgs, sched, cfg):
    """fixture validity (the rule of tests/test_gpu_variants_forward.py): max |dlogit| / max |logit| between the fp32 graph
    with QuickGELU and the same graph - same selections - with exact GELU in its place, i.e. with the activation ignored"""
    full, _, tr = vit_forward_restated(sd, imgs, sched, cfg, quick_gelu_torch, dtype=torch.float32)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    ignored, _, _ = vit_forward_restated(sd, imgs, sched, cfg, torch.nn.functional.gelu, forced_keep=forced, dtype=torch.float32)
    return float(np.abs(full - ignored).max()) / float(np.abs(full).max())
