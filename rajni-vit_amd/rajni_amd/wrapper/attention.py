"""`RAJNIAttention` - pruned attention of one scheduled block, on the MI355X.

Mirrors the reference module (`rajni/wrapper/attention.py:5-60`): same constructor, same attributes
borrowed from the timm `Attention`, same `forward(x, prev_scores=None) -> (out, keep_idx,
next_scores)`.  Differences are in HOW: QKV and proj are hand-written MFMA GEMMs, score + top-k +
compaction is one kernel, and the gather of the kept rows (attention.py:42-43) is fused into the
attention kernel's tile loads, so no gathered copy of qkv exists.

`RAJNIViTWrapper.forward` does not call this module's forward (it runs the whole network as one
native plan); it is kept for API parity and for block-level use and tests.
"""
from typing import Optional

import torch
import torch.nn as nn

from .. import _native as nat
from .. import ops


def qk_norm_modules(attn: nn.Module, where: str = "RAJNIAttention"):
    """(q_norm, k_norm) of a timm Attention when it normalises q and k (timm `qk_norm=True`: two affine nn.LayerNorm over
    the head dim with one eps), None when it does not (no attribute, None or nn.Identity).  Anything else - RMSNorm, a
    non-affine norm, one of the two missing, differing eps - is refused: the reference silently drops it."""
    mods = [getattr(attn, name, None) for name in ("q_norm", "k_norm")]
    plain = [m is None or isinstance(m, nn.Identity) for m in mods]
    if all(plain):
        return None
    for name, mod, off in zip(("q_norm", "k_norm"), mods, plain):
        if off or not isinstance(mod, nn.LayerNorm) or mod.weight is None:
            raise NotImplementedError(
                f"{where}: attn.{name} is {type(mod).__name__}; only an affine nn.LayerNorm on both q and k is supported "
                "(the reference silently drops it, SURVEY Q5) - refusing instead of computing something different")
    q, k = mods
    if tuple(q.normalized_shape) != tuple(k.normalized_shape) or len(q.normalized_shape) != 1:
        raise NotImplementedError(f"{where}: attn.q_norm / attn.k_norm must normalise the head dim alone")
    if float(q.eps) != float(k.eps):
        raise NotImplementedError(f"{where}: attn.q_norm and attn.k_norm have different eps ({q.eps} / {k.eps})")
    return q, k


class RAJNIAttention(nn.Module):
    def __init__(self, attn: nn.Module, keep_ratio: float, update: bool):
        super().__init__()
        # attribute contract of a timm Attention (attention.py:8-12)
        self.num_heads = attn.num_heads
        self.scale = attn.scale
        self.qkv = attn.qkv
        self.proj = attn.proj
        self.proj_drop = attn.proj_drop
        # timm qk_norm=True: LayerNorm over the head dim of q and k (ops.qk_norm); the modules stay attributes, so the
        # parameter set and the state-dict names are the timm Attention's
        qk = qk_norm_modules(attn)
        self.q_norm = qk[0] if qk else getattr(attn, "q_norm", None) or nn.Identity()
        self.k_norm = qk[1] if qk else getattr(attn, "k_norm", None) or nn.Identity()
        # the pairing of a model's rotary table (timm Eva's attribute; RAJNIViTWrapper reads it from every block).  This module's
        # own forward takes no table: the rotation of a RoPE model runs in the whole-forward plan only
        self.rotate_half = bool(getattr(attn, "rotate_half", False))
        self.keep_ratio = keep_ratio
        self.update = update
        # prefix tokens at the front of x (CLS + timm register tokens): always kept, never ranked.  RAJNIViTWrapper sets it
        # from the base model; 1 = the reference's single class token
        self.num_prefix_tokens = 1
        # the importance query: "cls" (row 0, the reference's rule) or "mean" (the mean of the query rows: the rule of a model
        # without a class token, whose num_prefix_tokens is its register count R >= 0).  RAJNIViTWrapper sets both
        self.importance_query = "cls"
        self._packed = None
        self._packed_key = None

    # ---- weights in the layout the kernels want (rebuilt when parameters change) -------------
    def _weights(self, device, dtype):
        params = [self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias]
        qk = qk_norm_modules(self)
        if qk:
            params += [qk[0].weight, qk[0].bias, qk[1].weight, qk[1].bias]
        key = (str(device), dtype) + tuple((p.data_ptr(), p._version) for p in params if p is not None)
        if self._packed_key != key:
            self._packed = dict(
                qkv_w=ops.pack_weight(self.qkv.weight, dtype, device),
                qkv_b=ops.pack_vec(self.qkv.bias, dtype, device),
                proj_w=ops.pack_weight(self.proj.weight, dtype, device),
                proj_b=ops.pack_vec(self.proj.bias, dtype, device))
            if qk:
                self._packed.update(qk_eps=float(qk[0].eps),
                                    q_w=ops.pack_vec(qk[0].weight, dtype, device), q_b=ops.pack_vec(qk[0].bias, dtype, device),
                                    k_w=ops.pack_vec(qk[1].weight, dtype, device), k_b=ops.pack_vec(qk[1].bias, dtype, device))
            self._packed_key = key
        return self._packed

    @torch.no_grad()
    def forward(self, x: torch.Tensor, prev_scores: Optional[torch.Tensor] = None):
        """x: [B, N, C] (already normed).  Returns out [B, Np, C], keep_idx [B, Np] int64,
        next_scores [B, Np]; Np = num_prefix_tokens + keep."""
        nat.require_device(x, "x")
        B, N, Cc = x.shape
        w = self._weights(x.device, x.dtype)
        qkv = ops.linear(x, w["qkv_w"], 3 * Cc, w["qkv_b"], nat.EPI_BIAS)            # attention.py:21-22
        if "q_w" in w:                                                                # timm: q, k = q_norm(q), k_norm(k)
            ops.qk_norm(qkv, self.num_heads, w["q_w"], w["q_b"], w["k_w"], w["k_b"], w["qk_eps"])
        P = int(getattr(self, "num_prefix_tokens", 1))
        keep = ops.keep_count(self.keep_ratio, N, P)                                  # attention.py:31-32
        if self.update or prev_scores is None:                                        # attention.py:25-28
            _, keep_idx, next_scores = ops.score_select(qkv, self.num_heads, keep, want_scores=False, num_prefix=P,
                                                        query=getattr(self, "importance_query", "cls"))
        else:
            keep_idx, next_scores = ops.select_topk(prev_scores.to(x.dtype), keep, num_prefix=P)   # attention.py:34-39,58
        out = ops.attention(qkv, keep_idx, self.num_heads, self.scale)                # attention.py:42-54
        out = ops.linear(out, w["proj_w"], Cc, w["proj_b"], nat.EPI_BIAS)             # attention.py:55
        if isinstance(self.proj_drop, nn.Dropout) and self.proj_drop.p > 0 and self.training:
            raise NotImplementedError("RAJNIAttention: proj_drop > 0 in training mode (inference path only)")
        return out, keep_idx.long(), next_scores                                      # attention.py:60
