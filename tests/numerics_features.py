"""Yardstick for the feature outputs (headless models, `forward_features`), torch on the CPU, shared by
tests/test_features_cpu.py and tests/test_gpu_features.py.

The semantics are timm's, on the pruned graph (tests/numerics_prefix.py holds the prefix-token and selection rules):
  tokens      forward_features: norm(x) for every token that survives the last block, [B, Nf, C];
  pooled      forward_head(pre_logits=True): fc_norm(pool(norm(x))), [B, C] - what a num_classes=0 model's forward returns;
  source_idx  [B, Nf]: the position in the UNPRUNED sequence of each surviving token - the scheduled blocks' selections
              composed, walked from the last scheduled block back to the first;
  dense       [B, P + n, C]: tokens scattered back to those positions, every other row zero.
One function restates the whole graph (every option of ViTConfig) and returns all four, in fp64 or in the model's dtype."""
from __future__ import annotations

import numpy as np
import torch

from oracle import rajni_oracle as orc
from numerics_variants import _t, _ln
from numerics_prefix import keep_count, select_tokens


def compose_source_idx(selections, B, n0):
    """selections {block: keep_idx [B, P + keep]} -> [B, Nf] int64: j <- idx_k[b, j] from the last scheduled block to the first;
    no scheduled block gives the identity over the n0 tokens"""
    src = None
    for i in sorted(selections, reverse=True):
        idx = np.asarray(selections[i], np.int64)
        src = idx if src is None else np.take_along_axis(idx, src, axis=1)
    return np.broadcast_to(np.arange(n0, dtype=np.int64), (B, n0)).copy() if src is None else src


def scatter_dense(tokens, source_idx, n0):
    """tokens [B, Nf, C], source_idx [B, Nf] -> [B, n0, C] with tokens[b, j] at row source_idx[b, j], zeros elsewhere"""
    B, _, C = tokens.shape
    out = np.zeros((B, n0, C), dtype=tokens.dtype)
    for b in range(B):
        out[b, source_idx[b]] = tokens[b]
    return out


def _mlp(h, sd, p, cfg, W):
    if cfg.mlp == "swiglu":
        g, v = h @ W(p + "mlp.fc1_g.weight").T + W(p + "mlp.fc1_g.bias"), h @ W(p + "mlp.fc1_x.weight").T + W(p + "mlp.fc1_x.bias")
        h = torch.nn.functional.silu(g) * v
    elif cfg.mlp == "swiglu_packed":
        g, v = (h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias")).chunk(2, dim=-1)
        h = torch.nn.functional.silu(g) * v
    else:
        h = h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias")
        h = h * torch.sigmoid(1.702 * h) if cfg.act == "quick_gelu" else torch.nn.functional.gelu(h)
    return h @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias")


def features_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64):
    """dict(pooled [B, C], tokens [B, Nf, C], source_idx [B, Nf] int64, dense [B, P + n, C], counts, trace) of the pruned graph
    for a timm-named numpy state dict `sd`; arrays are numpy (float64, or float32 holding the values of a 16-bit `dtype`)."""
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    P = cfg.num_prefix_tokens
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    prefix = [W("cls_token").expand(B, -1, -1)]
    if cfg.reg_tokens:
        prefix.append(W("reg_token").expand(B, -1, -1))
    if cfg.distilled:
        prefix.append(W("dist_token").expand(B, -1, -1))
    x = torch.cat(prefix + [x + W("pos_embed")], 1) if cfg.no_embed_class else torch.cat(prefix + [x], 1) + W("pos_embed")
    n0 = x.shape[1]
    if cfg.pre_norm:
        x = _ln(x, sd, "norm_pre", eps, dtype)
    scores, counts, trace = None, [], {}
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
                full = orc.importance_scores(torch.stack([q, k, v], 2).reshape(B, N, 3 * C).to(
                    torch.float64 if dtype == torch.float64 else torch.float32).numpy(), H, dtype=np_dt)
            else:
                full = scores
            keep = keep_count(sc["keep_ratio"], N, P)
            keep_idx = select_tokens(full, keep, P) if forced_keep is None or i not in forced_keep \
                else np.asarray(forced_keep[i], np.int64)
            assert keep_idx.shape == (B, P + keep)
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
        h = _mlp(_ln(x, sd, p + "norm2", eps, dtype), sd, p, cfg, W)
        x = x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
    if "norm.weight" in sd:
        x = _ln(x, sd, "norm", eps, dtype)
    pooled = x[:, P:].mean(1) if cfg.global_pool == "avg" else x[:, 0]
    if cfg.use_fc_norm:
        pooled = _ln(pooled, sd, "fc_norm", eps, dtype)
    as_np = lambda t: t.double().numpy() if dtype == torch.float64 else t.float().numpy()
    tokens = as_np(x)
    src = compose_source_idx({i: t["keep_idx"] for i, t in trace.items()}, B, n0)
    return dict(pooled=as_np(pooled), tokens=tokens, source_idx=src, dense=scatter_dense(tokens, src, n0), counts=counts,
                trace=trace)
