"""Yardsticks for models with register tokens (P = 1 + R prefix tokens; timm `reg_tokens=R`), pure numpy / torch-CPU, shared
by tests/test_prefix_cpu.py and the tests/test_gpu_prefix_*.py files.

The reference handles one prefix token only (it concatenates cls_token and slices [:, 1:]), so the semantics are timm's
VisionTransformer._pos_embed / .pool, restated here:
  token order [cls, reg_0 .. reg_{R-1}, patch_0 .. patch_{n-1}]; the pos-embed has n rows (patch rows only) or P + n rows;
  importance is oracle.rajni_oracle.importance_scores as it stands (CLS is the query, every statistic runs over all N tokens);
  only patch tokens are ranked: keep = max(1, int(keep_ratio * (N - P))), keep_idx = [0 .. P-1, ascending patch indices >= P]
  under the project's tie rule (larger score first, then lower index; NaN = +inf; -0 = +0);
  'avg' pooling is the mean of rows P..N-1."""
from __future__ import annotations

import numpy as np
import torch

from oracle import rajni_oracle as orc
from numerics_variants import _t, _ln, _quant_rows


def keep_count(keep_ratio: float, n_tokens: int, num_prefix: int = 1) -> int:
    """Python-double multiply, truncation, never below 1 - over the N - P patch tokens"""
    return max(1, int(keep_ratio * (n_tokens - num_prefix)))


def token_counts(n0, depth, schedule, num_prefix=1):
    schedule = orc.normalise_schedule(schedule)
    out, n = [], n0
    for i in range(depth):
        out.append(n)
        if i in schedule:
            n = keep_count(schedule[i]["keep_ratio"], n, num_prefix) + num_prefix
    return out


def select_tokens(scores: np.ndarray, keep: int, num_prefix: int = 1) -> np.ndarray:
    """keep_idx [B, P + keep]: 0..P-1, then the `keep` best of scores[:, P:] in ascending index order.  Larger score first,
    then lower index (a stable sort on the negated key); NaN ranks as +inf; -0 == +0 in a float compare."""
    s = np.asarray(scores)
    B, N = s.shape
    P = num_prefix
    out = np.zeros((B, P + keep), dtype=np.int64)
    out[:, :P] = np.arange(P)
    for b in range(B):
        p = s[b, P:].astype(np.float64)
        key = np.where(np.isnan(p), np.inf, p)
        order = np.argsort(-key, kind="stable")[:keep]
        out[b, P:] = np.sort(order) + P
    return out


def pos_embedded_tokens(sd, patches, cfg, dtype, P):
    """timm _pos_embed: patches [B, n, C] torch -> [B, P + n, C]"""
    B = patches.shape[0]
    prefix = [_t(sd["cls_token"], dtype).expand(B, -1, -1)]
    if P > 1:
        prefix.append(_t(sd["reg_token"], dtype).expand(B, -1, -1))
    pos = _t(sd["pos_embed"], dtype)
    if cfg.no_embed_class:
        return torch.cat(prefix + [patches + pos], 1)
    return torch.cat(prefix + [patches], 1) + pos


def without_registers(sd, cfg):
    """(state dict, P = 1) of the same model with its register rows removed: reg_token gone, the pos-embed's register rows gone"""
    P = 1 + cfg.reg_tokens
    out = {k: v for k, v in sd.items() if k != "reg_token"}
    if not cfg.no_embed_class:
        out["pos_embed"] = np.concatenate([sd["pos_embed"][:, :1], sd["pos_embed"][:, P:]], axis=1)
    return out


def selections_without_registers(forced, P):
    """keep_idx [B, P + keep] of the model with registers -> [B, 1 + keep] naming the same patches in the model without"""
    return {i: np.concatenate([np.zeros((len(k), 1), np.int64), np.asarray(k, np.int64)[:, P:] - (P - 1)], axis=1)
            for i, k in forced.items()}


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, num_prefix=None, act_fp8=False):
    """(logits [B, classes] numpy, token counts, trace {block: scores / keep_idx / next_scores}) of the pruned graph with
    P = `num_prefix` prefix tokens (default: the config's 1 + reg_tokens).  tests/numerics_variants.py::vit_forward_restated
    with the prefix rules of this module's docstring; timm's other options are applied as the config says."""
    schedule = orc.normalise_schedule(schedule)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    Pn = 1 + cfg.reg_tokens if num_prefix is None else num_prefix
    W = lambda n: _t(sd[n], dtype)
    H, D, C, eps = cfg.num_heads, cfg.head_dim, cfg.embed_dim, cfg.ln_eps
    x = torch.nn.functional.conv2d(_t(images, dtype), W("patch_embed.proj.weight"), W("patch_embed.proj.bias"),
                                   stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = pos_embedded_tokens(sd, x, cfg, dtype, Pn)
    if cfg.pre_norm:
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
        qkv = (xn @ W(p + "attn.qkv.weight").T + W(p + "attn.qkv.bias")).reshape(B, N, 3, H, D)
        q, k, v = qkv.unbind(2)
        if cfg.qk_norm:
            q, k = _ln(q, sd, p + "attn.q_norm", eps, dtype), _ln(k, sd, p + "attn.k_norm", eps, dtype)
        if i in schedule:
            sc = schedule[i]
            if sc["update"] or scores is None:
                full = orc.importance_scores(torch.stack([q, k, v], 2).reshape(B, N, 3 * C).numpy(), H, dtype=np_dt)
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
        if osc is not None and orc.attention_out_is_fp8(D, out.shape[1]):
            out = _quant_rows(out, np.float32(osc))
        out = out @ W(p + "attn.proj.weight").T + W(p + "attn.proj.bias")
        x = x + (out * W(p + "ls1.gamma") if p + "ls1.gamma" in sd else out)
        h = _ln(x, sd, p + "norm2", eps, dtype)
        if act_fp8:
            hs = orc.hidden_scale_bound(h.numpy(), sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
            h = _quant_rows(h)
        h = torch.nn.functional.gelu(h @ W(p + "mlp.fc1.weight").T + W(p + "mlp.fc1.bias"))
        if act_fp8:
            h = _quant_rows(h, hs)
        h = h @ W(p + "mlp.fc2.weight").T + W(p + "mlp.fc2.bias")
        x = x + (h * W(p + "ls2.gamma") if p + "ls2.gamma" in sd else h)
    if "norm.weight" in sd:
        x = _ln(x, sd, "norm", eps, dtype)
    x = x[:, Pn:].mean(1) if cfg.global_pool == "avg" else x[:, 0]
    if cfg.use_fc_norm:
        x = _ln(x, sd, "fc_norm", eps, dtype)
    logits = x @ W("head.weight").T + W("head.bias")
    return logits.numpy(), counts, trace


def registers_matter(sd, images, schedule, cfg, bar):
    """The fixture-validity check: the fp32 logits of the graph, and of the same graph on the same patch selections with the
    register rows removed, differ by at least 5 x bar x max|logit|.  Returns (moved, 5 x bar x scale)."""
    P = 1 + cfg.reg_tokens
    full, _, tr = vit_forward_restated(sd, images, schedule, cfg, dtype=torch.float32)
    forced = selections_without_registers({i: t["keep_idx"] for i, t in tr.items()}, P)
    dropped, _, _ = vit_forward_restated(without_registers(sd, cfg), images, schedule, cfg, forced_keep=forced,
                                         dtype=torch.float32, num_prefix=1)
    moved, need = float(np.abs(full - dropped).max()), 5 * bar * float(np.abs(full).max())
    print(f"[prefix] ignoring the {cfg.reg_tokens} register(s) ({'pruned' if schedule else 'unpruned'}) moves the logits by "
          f"{moved:.4g}; 5 x bar = {need:.4g}")
    return moved, need
