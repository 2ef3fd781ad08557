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


def qkv_form(attn: nn.Module, where: str = "RAJNIAttention") -> str:
    """How an attention module spells its q / k / v projection, recognised by what is there: "fused" - `qkv`, an nn.Linear with
    or without a bias; "fused_qv_bias" - a bias-free `qkv` beside the [C] parameters `q_bias` and `v_bias` (timm EvaAttention: k
    has no bias); "split" - `q_proj` / `k_proj` / `v_proj`, three nn.Linear of one shape, with `qkv` absent or None.  A
    half-formed spelling raises NotImplementedError, and so does an inner attention norm (`attn.norm` other than Identity / None:
    Eva's scale_norm, which no released EVA02 checkpoint has)."""
    norm = getattr(attn, "norm", None)
    if norm is not None and not isinstance(norm, nn.Identity):
        raise NotImplementedError(f"{where}: attn.norm ({type(norm).__name__}), a norm between attention and proj, is not supported")
    qkv = getattr(attn, "qkv", None)
    split = [getattr(attn, n, None) for n in ("q_proj", "k_proj", "v_proj")]
    qb, vb = getattr(attn, "q_bias", None), getattr(attn, "v_bias", None)
    if qkv is None:
        if not all(isinstance(m, nn.Linear) for m in split) or len({tuple(m.weight.shape) for m in split}) != 1 \
                or split[0].in_features != split[0].out_features:
            raise NotImplementedError(f"{where}: attn.qkv is absent, so q_proj, k_proj and v_proj must be three nn.Linear (C -> C)")
        if qb is not None or vb is not None:
            raise NotImplementedError(f"{where}: attn.q_bias / attn.v_bias beside q_proj / k_proj / v_proj: the biases of a split "
                                      "projection are the three linears' own")
        return "split"
    if not isinstance(qkv, nn.Linear):
        raise NotImplementedError(f"{where}: attn.qkv must be nn.Linear, got {type(qkv).__name__}")
    if any(m is not None for m in split):
        raise NotImplementedError(f"{where}: attn.qkv together with q_proj / k_proj / v_proj: one spelling of the projection per model")
    if qb is None and vb is None:
        return "fused"
    if qb is None or vb is None:
        raise NotImplementedError(f"{where}: attn.q_bias and attn.v_bias come together (timm EvaAttention); the module has only "
                                  f"{'v_bias' if qb is None else 'q_bias'}")
    Cdim = qkv.in_features
    if qkv.bias is not None or tuple(qb.shape) != (Cdim,) or tuple(vb.shape) != (Cdim,):
        raise NotImplementedError(f"{where}: attn.q_bias / attn.v_bias must be [{Cdim}] beside a bias-free attn.qkv")
    return "fused_qv_bias"


def packed_qkv(attn: nn.Module, where: str = "RAJNIAttention"):
    """(weight [3C, C], bias [3C] or None) of any spelling qkv_form knows, rows in the order q, k, v: the `qkv` weight itself; the
    bias cat(q_bias, 0, v_bias); or cat(q_proj, k_proj, v_proj) with the three biases concatenated, a missing one as zeros (no
    bias at all when none of the three has one).  Detached tensors on the module's device, values untouched."""
    form = qkv_form(attn, where)
    if form == "fused":
        return attn.qkv.weight.detach(), None if attn.qkv.bias is None else attn.qkv.bias.detach()
    if form == "fused_qv_bias":
        q, v = attn.q_bias.detach(), attn.v_bias.detach()
        return attn.qkv.weight.detach(), torch.cat([q, torch.zeros_like(q), v])
    lins = (attn.q_proj, attn.k_proj, attn.v_proj)
    w = torch.cat([m.weight.detach() for m in lins])
    if all(m.bias is None for m in lins):
        return w, None
    return w, torch.cat([m.bias.detach() if m.bias is not None else torch.zeros_like(m.weight[:, 0]).detach() for m in lins])


class RAJNIAttention(nn.Module):
    def __init__(self, attn: nn.Module, keep_ratio: float, update: bool):
        super().__init__()
        # attribute contract of a timm Attention (attention.py:8-12)
        self.num_heads = attn.num_heads
        self.scale = attn.scale
        # the q / k / v projection in the spelling the model has (qkv_form): the attributes stay, for the same reason
        self.qkv = getattr(attn, "qkv", None)
        for name in ("q_proj", "k_proj", "v_proj", "q_bias", "v_bias", "norm"):
            if getattr(attn, name, None) is not None:
                setattr(self, name, getattr(attn, name))
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
        # a learned relative position bias (BEiT's table and _get_rel_pos_bias(), timm RelPosAttention's rel_pos module): the
        # attributes stay, for the same reason, and RAJNIViTWrapper reads the bias through them.  This module's own forward takes
        # no table either - the bias runs in the whole-forward plan only - and refuses to run without it
        for name in ("relative_position_bias_table", "rel_pos", "window_size"):
            if getattr(attn, name, None) is not None:
                setattr(self, name, getattr(attn, name))
        if getattr(attn, "relative_position_bias_table", None) is not None:
            # BEiT: the table and its index buffer become this module's own, and _get_rel_pos_bias below is timm's gather - held,
            # here and now, to what the wrapped attention's own method returns (a bias is recognised by what it computes)
            index, get = getattr(attn, "relative_position_index", None), getattr(attn, "_get_rel_pos_bias", None)
            if not callable(get):
                self._get_rel_pos_bias = None      # RAJNIViTWrapper refuses the model, as it does without this wrapper
            elif not isinstance(index, torch.Tensor) or index.dim() != 2:
                raise NotImplementedError("RAJNIAttention: attn.relative_position_bias_table without an [n, n] "
                                          "attn.relative_position_index: the bias cannot be read, and the model is not run without it")
            else:
                self.register_buffer("relative_position_index", index,
                                     persistent="relative_position_index" not in getattr(attn, "_non_persistent_buffers_set", ()))
                with torch.no_grad():
                    theirs = get()
                theirs = theirs[0] if theirs.dim() == 4 else theirs
                if theirs.shape != self._get_rel_pos_bias().shape[1:] or not torch.equal(theirs, self._get_rel_pos_bias()[0]):
                    raise NotImplementedError("RAJNIAttention: attn._get_rel_pos_bias() does not return "
                                              "relative_position_bias_table[relative_position_index] as timm's BEiT attention does")
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

    @torch.no_grad()
    def _get_rel_pos_bias(self):
        """timm Beit Attention._get_rel_pos_bias: [1, H, n, n]"""
        n = self.relative_position_index.shape[0]
        b = self.relative_position_bias_table[self.relative_position_index.reshape(-1)].view(n, n, -1)
        return b.permute(2, 0, 1).contiguous().unsqueeze(0)

    # ---- weights in the layout the kernels want (rebuilt when parameters change) -------------
    def _weights(self, device, dtype):
        qkv_w, qkv_b = packed_qkv(self)
        params = [p for p in self.parameters(recurse=True)]
        qk = qk_norm_modules(self)
        if qk:
            params += [qk[0].weight, qk[0].bias, qk[1].weight, qk[1].bias]
        key = (str(device), dtype) + tuple((p.data_ptr(), p._version) for p in params if p is not None)
        if self._packed_key != key:
            self._packed = dict(
                qkv_w=ops.pack_weight(qkv_w, dtype, device),
                qkv_b=ops.pack_vec(qkv_b, dtype, device),
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
        if getattr(self, "relative_position_bias_table", None) is not None or getattr(self, "rel_pos", None) is not None:
            raise NotImplementedError("RAJNIAttention: this attention has a relative position bias, which the module's own forward "
                                      "does not apply: run the model through RAJNIViTWrapper's forward")
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
