"""Yardsticks for DeiT's distilled models (timm `VisionTransformerDistilled` in eval mode), pure numpy / torch-CPU, shared by
tests/test_distilled_cpu.py and tests/test_gpu_distilled.py.

The reference has no distilled models, so the semantics are timm's, with the project's pruning rule for prefix tokens
(tests/numerics_prefix.py) at P = 2:
  token order [cls, dist, patch_0 .. patch_{n-1}]; the pos-embed has n + 2 rows (added to every row) or n rows (no_embed_class);
  the dist token is a prefix token like a register: never pruned, never ranked, no rank slot; importance is
  oracle.rajni_oracle.importance_scores as it stands (CLS is the query, every statistic runs over all N tokens, dist included);
  keep = max(1, int(keep_ratio * (N - 2))), keep_idx = [0, 1, ascending patch indices >= 2];
  logits = (head(norm(x)[:, 0]) + head_dist(norm(x)[:, 1])) / 2.
The block loop is tests/numerics_prefix.py::vit_forward_restated's (plain blocks: the distilled configs have no q/k-norm, pre-norm
or fp8 activations); only the head differs, and `head=` / `drop_dist=` select the two ways of ignoring the feature that the
fixtures must be able to tell from the real thing."""
from __future__ import annotations

import numpy as np
import torch

from oracle import rajni_oracle as orc
from numerics_variants import _t, _ln
from numerics_prefix import keep_count, select_tokens, token_counts, pos_embedded_tokens  # noqa: F401  (re-exported)

P = 2       # cls + dist


def as_prefix_sd(sd):
    """the state dict with dist_token under the name the prefix restatement reads its rows behind CLS from"""
    out = dict(sd)
    out["reg_token"] = sd["dist_token"]
    return out


def without_dist(sd, cfg):
    """the same model with the dist row removed from the stream: no dist token, the pos-embed's dist row gone"""
    out = {k: v for k, v in sd.items() if k != "dist_token"}
    if not cfg.no_embed_class:
        out["pos_embed"] = np.concatenate([sd["pos_embed"][:, :1], sd["pos_embed"][:, P:]], axis=1)
    return out


def selections_without_dist(forced):
    """keep_idx [B, 2 + keep] -> [B, 1 + keep] naming the same patches in the stream without the dist row"""
    return {i: np.concatenate([np.zeros((len(k), 1), np.int64), np.asarray(k, np.int64)[:, P:] - 1], axis=1)
            for i, k in forced.items()}


def averaged_heads(n0, n1, sd, dtype=torch.float64):
    """(head(n0) + head_dist(n1)) / 2, each classifier evaluated on its own as timm does"""
    W = lambda n: _t(sd[n], dtype)
    return ((n0 @ W("head.weight").T + W("head.bias")) + (n1 @ W("head_dist.weight").T + W("head_dist.bias"))) / 2


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, head="distilled", drop_dist=False):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx / next_scores}) of the pruned graph of a
    distilled model.  head = "distilled": the averaged two heads on rows 0 and 1; "cls": `head` on row 0 alone.
    drop_dist: the stream is built without the dist row (P = 1; `sd` from without_dist, selections from
    selections_without_dist) and the averaged heads read rows 0 and 1 of what is there - the class row and the first
    surviving patch row."""
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    Pn = 1 if drop_dist else P
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = pos_embedded_tokens(sd if drop_dist else as_prefix_sd(sd), x, cfg, dtype, Pn)
    scores, counts, trace = None, [], {}
    for i in range(cfg.depth):
        counts.append(x.shape[1])
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _ln(x, sd, p + "norm1", eps, dtype)
        qkv = (xn @ W(p + "attn.qkv.weight").T + W(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                full = orc.importance_scores(qkv.reshape(B, N, 3 * C).numpy(), H, dtype=np_dt)
            else:
                full = scores
            keep = keep_count(sc["keep_ratio"], N, Pn)
            keep_idx = select_tokens(full, keep, Pn) if forced_keep is None or i not in forced_keep \
                else np.asarray(forced_keep[i], np.int64)
            assert keep_idx.shape == (B, Pn + keep)
            scores = np.take_along_axis(full, keep_idx, axis=1)
            trace[i] = {"scores": full, "keep_idx": keep_idx, "next_scores": scores}
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
    x = _ln(x, sd, "norm", eps, dtype)
    if head == "cls":
        logits = x[:, 0] @ W("head.weight").T + W("head.bias")
    else:
        assert head == "distilled"
        logits = averaged_heads(x[:, 0], x[:, 1], sd, dtype)
    return logits.numpy(), counts, trace


def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def vit_forward_ideal_bf16(sd, images, schedule, cfg, forced_keep):
    """What the bf16 FORMAT costs on this graph, whatever computes it: the restated graph in fp64 with every activation a 16-bit
    forward stores rounded to bf16 (LayerNorm rows, qkv, the softmax weights, attention output, MLP hidden rows, the normalised
    head rows, the logits) and the residual stream rounded to fp32, on the given selections.  Its distance from the fp64 graph
    is the error of an ideal bf16 forward; a fixture whose ideal error already sits at the 1e-2 bar cannot tell a correct
    forward from a wrong one, so fixtures are chosen by this figure (FIX below), never by a device result."""
    dtype = torch.float64
    f32 = lambda x: x.to(torch.float32).to(dtype)
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = f32(pos_embedded_tokens(as_prefix_sd(sd), x, cfg, dtype, P))
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        N = x.shape[1]
        xn = _bf16(_ln(x, sd, p + "norm1", eps, dtype))
        q, k, v = _bf16(xn @ W(p + "attn.qkv.weight").T + W(p + "attn.qkv.bias")).reshape(B, N, 3, H, D).unbind(2)
        if i in forced_keep:
            ki = torch.from_numpy(np.asarray(forced_keep[i], np.int64))
            gi = ki[:, :, None, None].expand(-1, -1, H, D)
            q, k, v = q.gather(1, gi), k.gather(1, gi), v.gather(1, gi)
            x = x.gather(1, ki[:, :, None].expand(-1, -1, C))
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5
        pm = _bf16(torch.exp(s - s.amax(-1, keepdim=True)))
        out = _bf16(torch.einsum("bhqk,bkhd->bqhd", pm, v) / pm.sum(-1).permute(0, 2, 1)[..., None]).reshape(B, -1, C)
        out = out @ W(p + "attn.proj.weight").T + W(p + "attn.proj.bias")
        x = f32(x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out))
        h = _bf16(_ln(x, sd, p + "norm2", eps, dtype))
        h = _bf16(torch.nn.functional.gelu(h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias")))
        h = h @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias")
        x = f32(x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h))
    x = _bf16(_ln(x, sd, "norm", eps, dtype))
    return _bf16(averaged_heads(x[:, 0], x[:, 1], sd, dtype)).numpy()


def format_cost(sd, images, schedule, cfg):
    """max |ideal bf16 forward - fp64 graph| / max|logit| on the fp64 graph's own selections"""
    want, _, tr = vit_forward_restated(sd, images, schedule, cfg)
    got = vit_forward_ideal_bf16(sd, images, schedule, cfg, {i: t["keep_idx"] for i, t in tr.items()})
    return float(np.abs(got - want).max() / np.abs(want).max())


def fused_head(sd):
    """what the wrapper hands the native forward: ([classes, 2C] = [W / 2 | W_dist / 2], (b + b_dist) / 2), fp32 numpy"""
    w = np.concatenate([np.float32(0.5) * sd["head.weight"], np.float32(0.5) * sd["head_dist.weight"]], axis=1).astype(np.float32)
    b = (np.float32(0.5) * (sd["head.bias"].astype(np.float32) + sd["head_dist.bias"].astype(np.float32))).astype(np.float32)
    return w, b


def feature_matters(sd, images, schedule, cfg, bar):
    """The fixture-validity check, fp32 on the CPU: the logits of the graph against (a) `head` applied to the class row alone
    and (b) the graph on the same patch selections with the dist row dropped from the stream.  Each must move the logits by
    at least 5 x bar x max|logit|.  Returns (moved_a, moved_b, need)."""
    full, _, tr = vit_forward_restated(sd, images, schedule, cfg, dtype=torch.float32)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    cls_only, _, _ = vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced, dtype=torch.float32, head="cls")
    dropped, _, _ = vit_forward_restated(without_dist(sd, cfg), images, schedule, cfg, forced_keep=selections_without_dist(forced),
                                         dtype=torch.float32, drop_dist=True)
    scale = float(np.abs(full).max())
    a, b, need = float(np.abs(full - cls_only).max()), float(np.abs(full - dropped).max()), 5 * bar * scale
    print(f"[distilled] {'pruned' if schedule else 'unpruned'}: head on the class row alone moves the logits by {a:.4g} "
          f"({a / (bar * scale):.1f} x bar), dropping the dist row by {b:.4g} ({b / (bar * scale):.1f} x bar); 5 x bar = {need:.4g}")
    return a, b, need


# ---- the forward fixtures tests/test_gpu_distilled.py runs and tests/test_distilled_cpu.py validates --------------------------
# Weights: the distribution the project's bars are stated for at each embed dim (std 0.08 at 128, 0.06 at 512; bias_std 0.02).
# The seed is chosen on the CPU alone, by a rule: the FIRST seed from 1 up for which, on every case of FORWARD_CASES,
#   (a) both ways of ignoring the feature move the fp32 logits by at least 5 x the 1e-2 bar (feature_matters), and
#   (b) an ideal bf16 forward (vit_forward_ideal_bf16: the format's own cost, no device involved) stays within 0.75 x that bar.
# (b) is needed because on these 4-block, 10-class models the bf16 format alone costs 0.3 - 1.4 % of the logit scale depending on
# the draw (seed 4 at embed dim 512, the project's usual fixture there: 1.41 % on the "carried" schedule - over the bar before
# any kernel has run).  Seeds 1, 2 (128) and 1 - 8 (512) fail (b); 3 and 9 are the first that pass both.
FIX = {"vit_micro_distilled_patch16_64": dict(seed=3, std=0.08, bias_std=0.02),
       "vit_micro512_distilled_patch16_64": dict(seed=9, std=0.06, bias_std=0.02)}
FORMAT_HEADROOM = 0.75
# (schedule, batch, image seed) of every forward that is held to a bar
FORWARD_CASES = [("unpruned", 3, 2), ("carried", 3, 5), ("last", 3, 5), ("carried", 3, 9)]
MICRO = list(FIX)
SCHEDULES = {
    "unpruned": {},
    "carried": {1: {"keep_ratio": 0.5, "update": True}, 2: {"keep_ratio": 0.5, "update": False}},
    # the LAST block prunes: no restricted last block, and the final norm reads rows 0 and 1 out of a [B, N, C] stream
    "last": {1: {"keep_ratio": 0.75, "update": True}, 3: {"keep_ratio": 0.5, "update": True}},
}
BATCH = 3
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}      # tests/test_gpu_prefix_forward.py's, per dtype


def images_of(cfg, B, seed=2):
    from rajni_amd import timm_shaped as ts
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))
