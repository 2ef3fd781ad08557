"""`RAJNIViTWrapper(base_model, pruning_schedule)` - drop-in for the reference wrapper
(`rajni/wrapper/model.py:6-69`) whose forward runs as ONE native plan on the MI355X.

Kept from the reference: constructor signature, in-place surgery on the base model (scheduled
blocks get a `RAJNIAttention`, every block gets `has_pruner`; model.py:12-23), parameter sharing,
`forward(images) -> logits`, `get_last_stats() -> {"token_counts": [...]}` (None before the first
forward).  Deliberate fixes: schedule keys are normalised to int (B1: a JSON-loaded
schedule prunes), a `no_embed_class` pos-embed works (B3), and timm's `qk_norm`, `pre_norm`, `global_pool='avg'`
and `fc_norm` options are computed as timm computes them instead of being dropped (B4), and so are
timm's register tokens (`reg_tokens=R`: `reg_token` [1, R, C] behind the class token, never pruned, never ranked) and
DeiT's distilled models (timm `VisionTransformerDistilled`: `dist_token` behind the class token, a prefix token like a
register, and eval logits `(head(x[:, 0]) + head_dist(x[:, 1])) / 2`).  Beyond the reference's surface: a headless base model
(`head = nn.Identity`, timm num_classes=0) returns its pooled feature [B, C], and `forward_features(x, dense=False)` returns the
final normalised tokens of the pruned graph, or the unpruned sequence with pruned positions zero (`fill="last"`: holding the
feature each token had when it left the stream), with their source positions in `get_last_stats()["source_idx"]`; and
`forward_intermediates` / `get_intermediate_layers` (timm's and DINOv2's signatures) return the states behind several blocks from
one forward, each on that unpruned grid; and `set_dynamic_img_size(True)` (timm's `dynamic_img_size`): any [B, C, H, W] the
patch size divides, the position embedding resampled to the input's token grid as timm's resample_abs_pos_embed does; and
models WITHOUT a class token (timm `class_token=False, global_pool='avg'`: the `*_gap_*` checkpoints, with or without
registers), which the reference cannot run at all: their importance query is the mean of the query rows
(`set_importance_query`, include/rajni_hip_query.h - this project's own rule), selectable on class-token models too; and
attention-pool heads (timm `global_pool='map'`, `attn_pool` = AttentionPoolLatent: the SigLIP image towers, with or without a
class token): one learned query over every token that survives the last block, then proj and a residual MLP on B rows
(include/rajni_hip_attnpool.h; `attn_pool_module` holds the pool to its contract); and rotary position embeddings (`model.rope`, a module whose `get_embed`
returns sin || cos tables - `rope_tables` holds it to its contract; include/rajni_hip_rope.h): q and k of every block rotated by
the place each surviving token had in the image, with or without a learned absolute embedding (`pos_embed` None).

Not kept: the Python per-block loop.  `forward` builds (once per batch shape) a `rajni_vit_plan`
- packed weights, workspace, per-stage index buffers - and calls `rajni_vit_forward`, which enqueues
every kernel of the network on the current stream with no host synchronisation.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn as nn

from .. import _native as nat
from .. import ops
from .attention import RAJNIAttention, qk_norm_modules, qkv_form, packed_qkv


class PlanRefs(NamedTuple):
    """what a native plan points to, kept alive with it"""
    blocks: object
    tc: object        # token_counts, written by every forward
    ws: object        # the workspace
    W: object         # the packed weights: a stale optimistic launch keeps them alive
    ext: object       # rajni_vit_ext, or None
    qk: object
    pre: object       # rajni_vit_prefix, or None


class PlanInput(NamedTuple):
    """the records that depend on the input and the model's head, each None where absent, and the patch grid"""
    img: object       # rajni_vit_image
    pos: object       # the position rows the plan points to
    gh: int
    gw: int
    qry: object       # rajni_vit_query
    apr: object       # rajni_vit_attn_pool
    nrm: object = None   # rajni_vit_norm
    rop: object = None   # rajni_vit_rope
    rot: object = None   # the (cos, sin) tensors that record points to: a plan owns what it points to, whatever the cache evicts
    mln: object = None   # (rajni_vit_mlp_norm, the two pointer arrays it points to)
    rel: object = None   # rajni_vit_relpos (its tensors live in the packed weights, which PlanRefs.W keeps alive)


class PlanEntry(NamedTuple):
    """one cached plan of RAJNIViTWrapper (callers outside this module index it by position)"""
    key: tuple
    plan: object
    refs: PlanRefs
    bufs: dict        # per scheduled block: keep_idx, next_scores, scores
    counts: list
    mode: object
    out_shape: tuple
    layers: object    # (blocks array, norm, fill, slab shape): the layers record minus `out`, or None
    input: PlanInput


# The native entry points, narrowest first: each takes the records of the one in front of it and one more, and a call goes
# through the one that takes the widest record it has - an mlp-norm record: _mlpnorm, else a rope record: _rope, else a norm record: _norm, else a pool record: _pool, else a query record: _query, else an image
# record: _image, else layers: _layers, else prefix: _ext_prefix, else ext: _ext, else the plain one.  (The symbol is part of
# the interface: nat.check puts it into the error message.)
_FORWARDS = ("rajni_vit_forward", "rajni_vit_forward_ext", "rajni_vit_forward_ext_prefix", "rajni_vit_forward_layers",
             "rajni_vit_forward_image", "rajni_vit_forward_query", "rajni_vit_forward_pool",
             "rajni_vit_forward_norm", "rajni_vit_forward_rope", "rajni_vit_forward_mlpnorm",
             "rajni_vit_forward_relpos")                                   # (ext, pre, lay, img, qry, apr, nrm, rop, mln, rel)
_SIZES = ("rajni_vit_workspace_bytes", "rajni_vit_workspace_bytes_prefix", "rajni_vit_workspace_bytes_image",
          "rajni_vit_workspace_bytes_query", "rajni_vit_workspace_bytes_pool",
          "rajni_vit_workspace_bytes_norm", "rajni_vit_workspace_bytes_rope",
          "rajni_vit_workspace_bytes_mlpnorm", "rajni_vit_workspace_bytes_relpos")          # (pre, img, qry, apr, nrm, rop, mln, rel)
NORM_MAX_C = 2048      # the row kernels hold a row in one wave's registers: C <= 64 lanes * 4 chunks * 8 elements


def _native_call(symbols, *records):
    """(symbol, record arguments) for records given in the order the entry points take them, None where absent"""
    n = max((i + 1 for i, rec in enumerate(records) if rec is not None), default=0)
    return symbols[n], [C.byref(rec) if rec is not None else None for rec in records[:n]]


def normalise_schedule(schedule) -> Dict[int, Dict]:
    """{block index: {"keep_ratio": float, "update": bool}} with int keys.  A missing `keep_ratio`
    raises KeyError like the reference (model.py:18); `update` defaults to True (model.py:19)."""
    out: Dict[int, Dict] = {}
    for k, cfg in (schedule or {}).items():
        out[int(k)] = {"keep_ratio": float(cfg["keep_ratio"]), "update": bool(cfg.get("update", True))}
    return out


def plan_token_counts(n0: int, depth: int, schedule: Dict[int, Dict], num_prefix: int = 1) -> List[int]:
    """Tokens at the entry of every block (model.py:43) - a pure function of (N0, depth, schedule, prefix tokens); every
    count includes the `num_prefix` prefix tokens, which are never dropped."""
    counts, n = [], n0
    for i in range(depth):
        counts.append(n)
        if i in schedule:
            n = ops.keep_count(schedule[i]["keep_ratio"], n, num_prefix) + num_prefix
    return counts


def compose_exit_block(selections: Dict[int, torch.Tensor], B: int, n0: int, depth: int, device) -> torch.Tensor:
    """{scheduled block: keep_idx [B, P + keep]} -> int32 [B, n0]: the block that drops the token of each position of the
    unpruned sequence, `depth` for the tokens that survive.  Block by block: every token that enters scheduled block i is
    marked i at its source position, and the ones the block keeps are marked again further on - by the next scheduled block,
    or `depth` at the end.  Torch ops on `device`, no host sync."""
    pos = torch.arange(n0, device=device).expand(B, n0)
    exit_block = torch.full((B, n0), depth, dtype=torch.int32, device=device)
    for i in sorted(selections):
        exit_block.scatter_(1, pos, torch.full_like(pos, i, dtype=torch.int32))
        pos = torch.gather(pos, 1, selections[i].long())
    exit_block.scatter_(1, pos, torch.full_like(pos, depth, dtype=torch.int32))
    return exit_block


def take_indices(num_blocks: int, indices=None) -> tuple:
    """timm's `feature_take_indices` restated (timm is not a dependency): the ascending block indices `forward_intermediates`
    captures.  None: every block; an int k: the last k; a sequence: those blocks, negative values counting from the end.
    Duplicates, an empty result and anything outside [-num_blocks, num_blocks) raise ValueError."""
    if indices is None:
        out = list(range(num_blocks))
    elif isinstance(indices, bool):
        raise ValueError(f"indices must be None, an int or a sequence of ints, got {indices!r}")
    elif isinstance(indices, int):
        if not 1 <= indices <= num_blocks:
            raise ValueError(f"indices={indices}: the last k blocks need 1 <= k <= {num_blocks}")
        out = list(range(num_blocks - indices, num_blocks))
    else:
        out = []
        for i in indices:
            if isinstance(i, bool) or not isinstance(i, int):
                raise ValueError(f"indices must hold ints, got {i!r}")
            if not -num_blocks <= i < num_blocks:
                raise ValueError(f"block index {i} is out of range for {num_blocks} blocks")
            out.append(i + num_blocks if i < 0 else i)
    if not out:
        raise ValueError("indices selects no block")
    if len(set(out)) != len(out):
        raise ValueError(f"indices names a block twice: {list(indices)}")
    return tuple(sorted(out))


def model_is_distilled(m: nn.Module) -> bool:
    """True for timm's VisionTransformerDistilled layout: BOTH `dist_token` [1, 1, C] and `head_dist`, an nn.Linear shaped like
    `head`, on a token-pooled model without fc_norm or register tokens.  False when the model has neither attribute.  Every
    half-formed or combined case raises NotImplementedError."""
    dist, head_dist = getattr(m, "dist_token", None), getattr(m, "head_dist", None)
    if dist is None and head_dist is None:
        return False
    if dist is None or head_dist is None:
        raise NotImplementedError("RAJNIViTWrapper: a distillation token and head_dist come together (DeiT distilled); the model "
                                  f"has only {'dist_token' if head_dist is None else 'head_dist'}")
    if getattr(m, "reg_token", None) is not None:
        raise NotImplementedError("RAJNIViTWrapper: a distillation token together with register tokens is not supported")
    Cdim = m.cls_token.shape[-1]
    if tuple(dist.shape) != (1, 1, Cdim):
        raise NotImplementedError(f"RAJNIViTWrapper: the distillation token must be [1, 1, {Cdim}], got {tuple(dist.shape)}")
    head = getattr(m, "head", None)
    if (not isinstance(head, nn.Linear) or not isinstance(head_dist, nn.Linear) or head_dist.in_features != Cdim
            or head.in_features != Cdim or head_dist.out_features != head.out_features):
        raise NotImplementedError("RAJNIViTWrapper: distillation needs head and head_dist to be nn.Linear of one shape "
                                  f"({Cdim} -> classes)")
    fc_norm = getattr(m, "fc_norm", None)
    if getattr(m, "global_pool", "token") != "token" or (fc_norm is not None and not isinstance(fc_norm, nn.Identity)):
        raise NotImplementedError("RAJNIViTWrapper: distillation needs a token head (global_pool='token', no fc_norm): the two "
                                  "classifiers read the class row and the distillation row")
    if getattr(m, "distilled_training", False) and m.training:
        raise NotImplementedError("RAJNIViTWrapper: distillation training (distilled_training in training mode) returns two "
                                  "outputs; this is the inference path, which averages them")
    return True


def model_has_class_token(m: nn.Module) -> bool:
    return getattr(m, "cls_token", None) is not None


def model_embed_dim(m: nn.Module) -> int:
    """C: the width of the class token, else of the position embedding, else (a model with neither: no class token and rotary
    positions alone) the patch projection's output channels"""
    for t in (getattr(m, "cls_token", None), getattr(m, "pos_embed", None)):
        if t is not None:
            return int(t.shape[-1])
    return int(m.patch_embed.proj.out_channels)


def classify_rope_embed(emb, heads: int, head_dim: int, depth: int) -> str:
    """"shared", "per_head" or "per_block": what a rotary table returned by `rope.get_embed` covers - [n, 2D] one table for all
    heads and blocks, [H, n, 2D] one per head, [depth, H, n, 2D] one per block and head (mixed RoPE) - sin on the first D of
    the last axis, cos on the last D.  Anything else raises NotImplementedError naming the shape."""
    why = "RAJNIViTWrapper: model.rope.get_embed() must return sin || cos tables"
    if not isinstance(emb, torch.Tensor) or not emb.is_floating_point() or emb.dim() not in (2, 3, 4):
        raise NotImplementedError(f"{why} [n, 2D], [H, n, 2D] or [depth, H, n, 2D]; got "
                                  f"{tuple(emb.shape) if isinstance(emb, torch.Tensor) else type(emb).__name__}")
    if emb.shape[-1] != 2 * head_dim:
        raise NotImplementedError(f"{why} whose last axis is 2 * head_dim = {2 * head_dim}; got {tuple(emb.shape)} "
                                  f"(a table for part of the head dim, or sin and cos apart, is not supported)")
    if emb.dim() >= 3 and emb.shape[-3] != heads:
        raise NotImplementedError(f"{why}; a per-head table needs {heads} heads, got {tuple(emb.shape)}")
    if emb.dim() == 4 and emb.shape[0] != depth:
        raise NotImplementedError(f"{why}; a per-block table needs {depth} blocks, got {tuple(emb.shape)}")
    return {2: "shared", 3: "per_head", 4: "per_block"}[emb.dim()]


def rope_tables(m: nn.Module, heads: int, head_dim: int, depth: int, grid=None):
    """None for a model without rotary positions (`model.rope` missing or None), else (kind, emb): the table of the model's own
    grid, or of `grid` = (gh, gw) fetched as `get_embed(shape=(gh, gw))`, and what it covers (classify_rope_embed).  The
    contract mirrors timm's `Eva` / `RotaryEmbeddingCat` and is written from memory of timm 1.x, unverified against an installed
    timm: `rope` is a module whose `get_embed(shape=None)` returns sin || cos on the last axis, 2 * head_dim wide."""
    rope = getattr(m, "rope", None)
    if rope is None:
        return None
    get = getattr(rope, "get_embed", None)
    if not callable(get):
        raise NotImplementedError(f"RAJNIViTWrapper: model.rope ({type(rope).__name__}) has no get_embed(): rotary positions are "
                                  "taken from a module whose get_embed(shape=None) returns sin || cos tables")
    with torch.no_grad():
        emb = get() if grid is None else get(shape=tuple(grid))
    return classify_rope_embed(emb, heads, head_dim, depth), emb


# ---- a learned relative position bias on the attention logits (include/rajni_hip_relpos.h) --------------------------------
# The module contract, WRITTEN FROM MEMORY OF timm 1.x AND UNVERIFIED against an installed timm (as the rotary contract is):
#   BEiT              blocks[i].attn.relative_position_bias_table (a tensor) and blocks[i].attn._get_rel_pos_bias()
#   vit_relpos        blocks[i].attn.rel_pos (a module) and its get_bias()
#   shared            base_model.rel_pos_bias (a module, called: rel_pos_bias()) or base_model.shared_rel_pos.get_bias()
# each returning the dense bias [H, n0, n0] (a leading batch axis of 1 is accepted) that timm adds to the scaled logits.  A bias
# is recognised by what it computes: the dense tensor is decomposed (decompose_rel_pos_bias) and refused if it is not a function
# of the patch offset with constant prefix rows and columns.
REL_POS_ATTRS = ("relative_position_bias_table", "rel_pos")            # on an attention
REL_POS_MODEL_ATTRS = ("rel_pos_bias", "shared_rel_pos")               # on the model


def _attn_bias_source(attn: nn.Module, where: str):
    """the callable that returns an attention's own dense bias, or None; an attribute outside the contract is refused"""
    table, rp = getattr(attn, "relative_position_bias_table", None), getattr(attn, "rel_pos", None)
    if table is not None and rp is not None:
        raise NotImplementedError(f"{where}: attn.relative_position_bias_table together with attn.rel_pos: one bias per attention")
    if table is not None:
        get = getattr(attn, "_get_rel_pos_bias", None)
        if not callable(get):
            raise NotImplementedError(f"{where}: attn.relative_position_bias_table without a callable attn._get_rel_pos_bias(): the "
                                      "bias cannot be read, and the model is not run without it")
        return get
    if rp is not None:
        get = getattr(rp, "get_bias", None)
        if not callable(get):
            raise NotImplementedError(f"{where}: attn.rel_pos ({type(rp).__name__}) has no get_bias(): the bias cannot be read, and "
                                      "the model is not run without it")
        return get
    return None


def rel_pos_sources(m: nn.Module, blocks):
    """(per-block callables or None, the shared callable or None).  Blocks that disagree on having a bias are refused."""
    per = [_attn_bias_source(blk.attn, f"RAJNIViTWrapper: block {i}") for i, blk in enumerate(blocks)]
    have = [g is not None for g in per]
    if any(have) and not all(have):
        raise NotImplementedError(f"RAJNIViTWrapper: block {have.index(True)} has a relative position bias and block "
                                  f"{have.index(False)} has none: every block or no block")
    shared = None
    rpb, srp = getattr(m, "rel_pos_bias", None), getattr(m, "shared_rel_pos", None)
    if rpb is not None and srp is not None:
        raise NotImplementedError("RAJNIViTWrapper: base_model.rel_pos_bias together with base_model.shared_rel_pos")
    if rpb is not None:
        if not callable(rpb):
            raise NotImplementedError(f"RAJNIViTWrapper: base_model.rel_pos_bias ({type(rpb).__name__}) is not callable: the shared "
                                      "bias cannot be read, and the model is not run without it")
        shared = rpb
    elif srp is not None:
        shared = getattr(srp, "get_bias", None)
        if not callable(shared):
            raise NotImplementedError(f"RAJNIViTWrapper: base_model.shared_rel_pos ({type(srp).__name__}) has no get_bias(): the "
                                      "shared bias cannot be read, and the model is not run without it")
    return (per if all(have) and per else None), shared


def model_has_rel_pos(m: nn.Module, blocks) -> bool:
    """any attribute of the contract is present and not None (cheap: the setters ask before a forward has described the model)"""
    return any(getattr(m, a, None) is not None for a in REL_POS_MODEL_ATTRS) or \
        any(getattr(blk.attn, a, None) is not None for blk in blocks for a in REL_POS_ATTRS)


def dense_rel_pos_bias(get, heads: int, where: str) -> torch.Tensor:
    """the dense bias a source returns, as fp32 [H, n0, n0] on the host"""
    try:
        with torch.no_grad():
            b = get()
    except Exception as e:      # (a getter that wants arguments, a module without a forward ...: outside the contract)
        raise NotImplementedError(f"{where}: reading the bias failed ({type(e).__name__}: {e}): the model is not run without it") from None
    if not isinstance(b, torch.Tensor):
        raise NotImplementedError(f"{where}: the relative position bias is a {type(b).__name__}, not a tensor")
    if b.dim() == 4 and b.shape[0] == 1:
        b = b[0]
    if b.dim() != 3 or b.shape[0] != heads or b.shape[1] != b.shape[2]:
        raise NotImplementedError(f"{where}: the relative position bias must be [H, n0, n0] (or [1, H, n0, n0]) with H = {heads}, "
                                  f"got {tuple(b.shape)}")
    return b.detach().to(device="cpu", dtype=torch.float32)


def decompose_rel_pos_bias(dense: torch.Tensor, gh: int, gw: int, P: int, where: str = "relative position bias"):
    """dense [H, n0, n0] fp32, n0 = P + gh * gw -> (table [H, (2 gh - 1)(2 gw - 1)], prefix_q [H], prefix_k [H], prefix_qk [H]) of
    include/rajni_hip_relpos.h, exactly: bit for bit the patch-patch part must depend on (dy, dx) = (query - key) alone and the
    prefix rows and columns must be constant per head in each of the three categories.  A bias that fails is refused, naming the
    first element that breaks the structure."""
    H, n0 = dense.shape[0], dense.shape[1]
    n = gh * gw
    if n0 != P + n:
        raise NotImplementedError(f"{where}: the bias covers {n0} tokens but the model has {P} prefix tokens and a {gh} x {gw} grid")
    ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    idx = (ys[:, None] - ys[None, :] + gh - 1) * (2 * gw - 1) + (xs[:, None] - xs[None, :] + gw - 1)      # [n, n]
    patch = dense[:, P:, P:]
    table = torch.zeros(H, (2 * gh - 1) * (2 * gw - 1), dtype=torch.float32)
    table[:, idx.reshape(-1)] = patch.reshape(H, -1)        # every offset occurs: each entry is written (by some pair)

    def first_bad(got, want, q0, k0, what):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        if bad.numel():
            h, q, k = (int(v) for v in bad[0])
            raise NotImplementedError(f"{where}: not a function of the relative offset: element [head {h}, query {q + q0}, key "
                                      f"{k + k0}] = {float(got[h, q, k])!r} but {what} holds {float(want[h, q, k])!r}")
    first_bad(patch.contiguous(), table[:, idx].contiguous(), P, P, "another pair of the same offset (dy, dx)")
    pq, pk, pqk = (torch.zeros(H, dtype=torch.float32) for _ in range(3))
    if P:
        pq, pk, pqk = dense[:, 0, P].clone(), dense[:, P, 0].clone(), dense[:, 0, 0].clone()
        first_bad(dense[:, :P, P:].contiguous(), pq[:, None, None].expand(H, P, n).contiguous(), 0, P, "the first prefix-query / patch-key pair")
        first_bad(dense[:, P:, :P].contiguous(), pk[:, None, None].expand(H, n, P).contiguous(), P, 0, "the first patch-query / prefix-key pair")
        first_bad(dense[:, :P, :P].contiguous(), pqk[:, None, None].expand(H, P, P).contiguous(), 0, 0, "the first prefix / prefix pair")
    return table, pq, pk, pqk


def rel_pos_grid(m: nn.Module, blocks, n_patches: int):
    """(gh, gw) of the model's own input: patch_embed.grid_size or an attention's window_size where it is a pair of that many
    patches, else the integer square root"""
    for gs in (getattr(m.patch_embed, "grid_size", None), getattr(blocks[0].attn, "window_size", None),
               getattr(getattr(blocks[0].attn, "rel_pos", None), "window_size", None)):
        if isinstance(gs, (tuple, list)) and len(gs) == 2 and all(isinstance(v, int) and v > 0 for v in gs) and gs[0] * gs[1] == n_patches:
            return int(gs[0]), int(gs[1])
    r = math.isqrt(n_patches)
    if r * r != n_patches:
        raise NotImplementedError(f"RAJNIViTWrapper: cannot tell the grid of a relative position bias over {n_patches} patches: "
                                  "patch_embed.grid_size does not give it and it is not square")
    return r, r


def rope_layout(blocks) -> bool:
    """True for rotate_half pairs (j, j + D/2), False for timm rot()'s (2i, 2i + 1): `blocks[i].attn.rotate_half`, False where
    the attribute is missing; all blocks must agree"""
    kinds = [bool(getattr(blk.attn, "rotate_half", False)) for blk in blocks]
    if any(k != kinds[0] for k in kinds):
        raise NotImplementedError(f"RAJNIViTWrapper: block {kinds.index(not kinds[0])}: attn.rotate_half differs between blocks "
                                  "(one pairing of the rotary table per model)")
    return kinds[0]


def _num_prefix_without_class_token(m: nn.Module) -> int:
    """R of a model whose `cls_token` is None (timm class_token=False): the prefix tokens are its registers alone.  Accepted
    only when the model is consistent - no distillation pair, a well-formed `reg_token`, a declared `num_prefix_tokens` equal
    to R, a pos_embed of n or R + n rows, and an 'avg' pool or no head; everything else keeps the refusal a missing class token
    always had (NotImplementedError naming cls_token)."""
    why = "RAJNIViTWrapper: the model has no cls_token (class_token=False)"
    if getattr(m, "dist_token", None) is not None or getattr(m, "head_dist", None) is not None:
        raise NotImplementedError(f"{why} but a distillation token or head_dist: distillation reads the class row")
    reg = getattr(m, "reg_token", None)
    Cdim = model_embed_dim(m)
    R = 0
    if reg is not None:
        if reg.dim() != 3 or reg.shape[0] != 1 or reg.shape[1] < 1 or reg.shape[2] != Cdim:
            raise NotImplementedError(f"{why}: reg_token must be [1, R, {Cdim}] with R >= 1, got {tuple(reg.shape)}")
        R = int(reg.shape[1])
    declared = getattr(m, "num_prefix_tokens", R)
    if declared != R:
        raise NotImplementedError(f"{why} and declares {declared} prefix tokens but its parameters supply {R} (reg_token alone): "
                                  "the class token is the importance query of such a model and is required")
    if R > nat.MAX_PREFIX:
        raise NotImplementedError(f"{why} and {R} prefix tokens; at most {nat.MAX_PREFIX} are supported")
    n_patches = getattr(m.patch_embed, "num_patches", None)
    if isinstance(n_patches, int) and m.pos_embed is not None and m.pos_embed.shape[-2] not in (n_patches, n_patches + R):
        raise NotImplementedError(f"{why}: pos_embed has {m.pos_embed.shape[-2]} rows; with {R} register tokens and {n_patches} "
                                  f"patches it must have {n_patches} (no_embed_class) or {n_patches + R}")
    pool = getattr(m, "global_pool", "token")
    if pool not in ("avg", "map") and not isinstance(getattr(m, "head", None), nn.Identity):
        raise NotImplementedError(f"{why} and global_pool={pool!r}: without a class row the head must pool with 'avg' or 'map' "
                                  "(or be nn.Identity)")
    return R


def model_num_prefix(m: nn.Module) -> int:
    """P prefix tokens the base model's PARAMETERS supply: `cls_token` and `reg_token` [1, R, C] (timm reg_tokens=R, P = 1 + R)
    or `dist_token` [1, 1, C] (DeiT distilled, P = 2); R alone for a consistent model without a class token (timm
    class_token=False).  Raises NotImplementedError for what the native forward does not compute (a half-formed model without a
    class token, a half-formed distillation pair, a malformed or oversized register set, a declared `num_prefix_tokens` that
    disagrees)."""
    cls = getattr(m, "cls_token", None)
    if cls is None:
        return _num_prefix_without_class_token(m)
    if model_is_distilled(m):
        declared = getattr(m, "num_prefix_tokens", 2)
        if declared != 2:
            raise NotImplementedError(f"RAJNIViTWrapper: the model declares {declared} prefix tokens but a distillation model "
                                      "has 2 (cls_token + dist_token)")
        return 2
    reg = getattr(m, "reg_token", None)
    P = 1
    if reg is not None:
        if reg.dim() != 3 or reg.shape[0] != 1 or reg.shape[1] < 1 or reg.shape[2] != cls.shape[-1]:
            raise NotImplementedError(f"RAJNIViTWrapper: reg_token must be [1, R, {cls.shape[-1]}] with R >= 1, got {tuple(reg.shape)}")
        P = 1 + int(reg.shape[1])
    declared = getattr(m, "num_prefix_tokens", P)
    if declared != P:
        raise NotImplementedError(f"RAJNIViTWrapper: the model declares {declared} prefix tokens but its parameters supply {P} "
                                  "(cls_token + reg_token); distillation or other prefix tokens are not supported")
    if P > nat.MAX_PREFIX:
        raise NotImplementedError(f"RAJNIViTWrapper: {P} prefix tokens; at most {nat.MAX_PREFIX} are supported")
    return P


def classify_mlp_act(act: Optional[nn.Module]) -> str:
    """"gelu" or "quick_gelu": what a block's `mlp.act` COMPUTES, not what it is called.  Exact-erf `nn.GELU` is GELU.
    Anything else is probed once on the CPU - a fixed fp32 grid on [-6, 6] through the module - and is QuickGELU when it
    matches x * sigmoid(1.702 x) to 1e-6: timm's and open_clip's `QuickGELU` and transformers' `QuickGELUActivation` pass
    without being imported, a class of that name that computes something else does not.  Everything unmatched (tanh-GELU,
    SiLU, ReLU ...) raises NotImplementedError naming the class."""
    if isinstance(act, nn.GELU):
        if getattr(act, "approximate", "none") == "none":
            return "gelu"
    elif isinstance(act, nn.Module):
        grid = torch.linspace(-6.0, 6.0, 193, dtype=torch.float32)
        try:
            with torch.no_grad():
                got = act(grid.clone())
        except Exception:
            got = None
        if (isinstance(got, torch.Tensor) and got.shape == grid.shape and got.dtype == torch.float32
                and float((got - grid * torch.sigmoid(1.702 * grid)).abs().max()) <= 1e-6):
            return "quick_gelu"
    name = type(act).__name__ + ("(approximate=%r)" % act.approximate if isinstance(act, nn.GELU) else "")
    raise NotImplementedError(f"mlp.act must be exact-erf nn.GELU (timm default) or QuickGELU, x * sigmoid(1.702 x); "
                              f"{name} computes neither")


def classify_norm(mod: Optional[nn.Module], dim: int) -> str:
    """"layernorm" or "rms": what a norm module over `dim` channels COMPUTES, not what it is called.  An affine `nn.LayerNorm`
    over (dim,) is "layernorm".  Anything else is "rms" when it has a `weight` of shape [dim], no bias, a float `eps`, and its
    output on a fixed fp32 probe (a CPU fp32 copy of the module, 4 rows with non-zero means) matches
    x * rsqrt(mean(x^2) + eps) * weight to 1e-6: `torch.nn.RMSNorm` with an explicit eps, timm's `RmsNorm` and look-alikes pass
    without being imported, a class of that name that computes something else does not.  `eps=None` is refused - torch resolves
    it per dtype, so the module has no one eps.  Everything unmatched raises NotImplementedError naming the class."""
    name = type(mod).__name__
    if isinstance(mod, nn.LayerNorm):
        if mod.weight is not None and tuple(mod.normalized_shape) == (dim,):
            return "layernorm"
        raise NotImplementedError(f"{name} must be affine (elementwise_affine=True) over the {dim} channels")
    weight = getattr(mod, "weight", None)
    if isinstance(mod, nn.Module) and isinstance(weight, torch.Tensor) and tuple(weight.shape) == (dim,) \
            and getattr(mod, "bias", None) is None:
        eps = getattr(mod, "eps", None)
        if eps is None:
            raise NotImplementedError(f"{name} has eps=None, which torch resolves per dtype: give the module an explicit eps")
        if isinstance(eps, float):
            g = torch.Generator().manual_seed(0)
            x = torch.randn(4, dim, generator=g, dtype=torch.float32) * 1.5 + torch.tensor([[0.0], [0.5], [-1.0], [2.0]])
            try:
                with torch.no_grad():
                    probe = copy.deepcopy(mod).to(device="cpu", dtype=torch.float32)
                    got = probe(x.clone())
                    want = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * probe.weight
            except Exception:
                got = None
            if (isinstance(got, torch.Tensor) and got.shape == x.shape and got.dtype == torch.float32
                    and float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))):
                return "rms"
    raise NotImplementedError(f"a norm layer must be an affine nn.LayerNorm or an RMSNorm, x * rsqrt(mean(x^2) + eps) * weight "
                              f"without a bias; {name} computes neither")


def _is_silu(act) -> bool:
    """`act` computes t * sigmoid(t): nn.SiLU, or any module that matches it on classify_mlp_act's fp32 probe grid to 1e-6"""
    if not isinstance(act, nn.Module):
        return False
    grid = torch.linspace(-6.0, 6.0, 193, dtype=torch.float32)
    try:
        with torch.no_grad():
            got = act(grid.clone())
    except Exception:
        return False
    return (isinstance(got, torch.Tensor) and got.shape == grid.shape and got.dtype == torch.float32
            and float((got - grid * torch.sigmoid(grid)).abs().max()) <= 1e-6)


def gated_mlp_form(mlp: nn.Module) -> Optional[str]:
    """None for a plain MLP (fc1 -> act -> fc2); "packed" for timm's GluMlp layout - ONE fc1 whose output is twice fc2's
    input, chunked into (x1, x2) - and "split" for timm's SwiGLU layout (fc1_g and fc1_x).  Recognised by structure, not by
    class name.  Raises NotImplementedError for a gated MLP the native forward does not compute: a gate other than SiLU
    (GELU-gated GEGLU and the like).  (A plain Mlp whose act is SiLU is not gated: classify_mlp_act refuses it as before.  A
    `norm` between the gate and fc2 is mlp_norm_module's.)"""
    fc1, fc2 = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    fc1_g, fc1_x = getattr(mlp, "fc1_g", None), getattr(mlp, "fc1_x", None)
    if isinstance(fc1_g, nn.Linear) and isinstance(fc1_x, nn.Linear) and isinstance(fc2, nn.Linear):
        if fc1_g.weight.shape != fc1_x.weight.shape or fc1_g.out_features != fc2.in_features:
            raise NotImplementedError(f"{type(mlp).__name__}: fc1_g and fc1_x must have one shape, with fc2.in_features outputs")
        form = "split"
    elif isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear) and fc1.out_features == 2 * fc2.in_features:
        form = "packed"
    else:
        return None
    name = type(mlp).__name__
    act = getattr(mlp, "act", None)
    if not _is_silu(act):
        raise NotImplementedError(f"{name}: a gated MLP is supported with the SiLU gate only (SwiGLU), t * sigmoid(t); its act "
                                  f"{type(act).__name__} computes something else")
    return form


def mlp_norm_module(mlp: nn.Module) -> Optional[nn.Module]:
    """the norm between an MLP's activation (or gate) and fc2 - timm `Mlp.norm` / `SwiGLU.norm` / `GluMlp.norm`, EVA02's
    sub-LayerNorm - or None where there is none (no attribute, None or nn.Identity)"""
    norm = getattr(mlp, "norm", None)
    return None if norm is None or isinstance(norm, nn.Identity) else norm


def block_layer_scales(blk: nn.Module, where: str):
    """(gamma of the attention branch, gamma of the MLP branch), each a [C] tensor or None, in either spelling: timm Block's
    `ls1` / `ls2` (Identity, or a LayerScale with `.gamma`) or timm EvaBlock's `gamma_1` / `gamma_2` (a parameter or None), the
    second taken where the first is absent.  A block with both spellings is refused."""
    out = []
    for ls_name, g_name in (("ls1", "gamma_1"), ("ls2", "gamma_2")):
        has_ls, has_g = hasattr(blk, ls_name), hasattr(blk, g_name)
        if has_ls and has_g:
            raise NotImplementedError(f"{where}: both {ls_name} and {g_name}: one spelling of LayerScale per block")
        if has_g:
            g = getattr(blk, g_name)
            if g is not None and not (isinstance(g, torch.Tensor) and g.dim() == 1):
                raise NotImplementedError(f"{where}: {g_name} must be a [C] parameter or None")
            out.append(g)
            continue
        ls = getattr(blk, ls_name, None)
        if ls is not None and not isinstance(ls, nn.Identity) and not hasattr(ls, "gamma"):
            raise NotImplementedError(f"{ls_name} must be Identity or a LayerScale with .gamma")
        out.append(ls.gamma if (ls is not None and hasattr(ls, "gamma")) else None)
    return out[0], out[1]


def gated_fc1(mlp: nn.Module, form: str):
    """(gate weight, value weight, gate bias, value bias) of a gated MLP, each [hidden, C] / [hidden] or None.  timm's
    order (gate_last missing or False) has the gate in the first half of the packed fc1; gate_last=True swaps the halves."""
    if form == "split":
        return mlp.fc1_g.weight, mlp.fc1_x.weight, mlp.fc1_g.bias, mlp.fc1_x.bias
    h = mlp.fc2.in_features
    w, b = mlp.fc1.weight, mlp.fc1.bias
    first, second = (w[:h], None if b is None else b[:h]), (w[h:], None if b is None else b[h:])
    g, v = (second, first) if getattr(mlp, "gate_last", False) else (first, second)
    return g[0], v[0], g[1], v[1]


def attn_pool_module(m: nn.Module) -> Optional[nn.Module]:
    """The model's attention pool (timm `global_pool='map'`: `attn_pool`, an AttentionPoolLatent) or None for every other
    head.  Recognised by structure, not by class name: `latent` [1, 1, C], Linear `q` (C -> C), `kv` (C -> 2C) and `proj`
    (C -> C), `num_heads` dividing C with `scale` = head_dim ** -0.5, `latent_len == 1`, no pool `pos_embed`, Identity
    `q_norm` / `k_norm`, an affine LayerNorm `norm` over C and a plain `mlp` (fc1 -> act -> fc2) whose act classify_mlp_act
    accepts.  (The contract is written from memory of timm 1.x - include/rajni_hip_attnpool.h.)  Raises NotImplementedError
    naming `global_pool` for 'map' without a pool, and naming `attn_pool` for a pool beside another global_pool or one that is
    not this contract."""
    pool_kind = getattr(m, "global_pool", "token")
    ap = getattr(m, "attn_pool", None)
    if ap is None:
        if pool_kind == "map":
            raise NotImplementedError("RAJNIViTWrapper: global_pool='map' needs the model's attn_pool (timm AttentionPoolLatent); "
                                      "it has none")
        return None
    if pool_kind != "map":
        raise NotImplementedError(f"RAJNIViTWrapper: attn_pool beside global_pool={pool_kind!r} is not supported (an attention "
                                  "pool is the head of global_pool='map')")
    why = "RAJNIViTWrapper: attn_pool is not timm's AttentionPoolLatent as global_pool='map' builds it"
    Cdim = model_embed_dim(m)
    latent = getattr(ap, "latent", None)
    lin = {name: getattr(ap, name, None) for name in ("q", "kv", "proj")}
    if not isinstance(latent, torch.Tensor) or any(not isinstance(v, nn.Linear) for v in lin.values()):
        raise NotImplementedError(f"{why}: it needs `latent` and Linear `q`, `kv` and `proj`")
    if int(getattr(ap, "latent_len", 1)) != 1 or tuple(latent.shape) != (1, 1, Cdim):
        raise NotImplementedError(f"{why}: latent_len > 1 (latent {tuple(latent.shape)}) is not supported - one query row, "
                                  f"latent [1, 1, {Cdim}]")
    if getattr(ap, "pos_embed", None) is not None:
        raise NotImplementedError(f"{why}: a position embedding inside the pool (attn_pool.pos_embed) is not supported")
    for name in ("q_norm", "k_norm"):
        mod = getattr(ap, name, None)
        if mod is not None and not isinstance(mod, nn.Identity):
            raise NotImplementedError(f"{why}: attn_pool.{name} ({type(mod).__name__}) is not supported - the pool's q/k-norm "
                                      "must be nn.Identity")
    for name, rows in (("q", Cdim), ("kv", 2 * Cdim), ("proj", Cdim)):
        if tuple(lin[name].weight.shape) != (rows, Cdim):
            raise NotImplementedError(f"{why}: attn_pool.{name} must be Linear({Cdim}, {rows}), got weight "
                                      f"{tuple(lin[name].weight.shape)}")
    heads = getattr(ap, "num_heads", None)
    if not isinstance(heads, int) or heads < 1 or Cdim % heads or (Cdim // heads) % 8 or not 8 <= Cdim // heads <= 128:
        raise NotImplementedError(f"{why}: attn_pool.num_heads = {heads!r} must divide {Cdim} into head dims that are multiples "
                                  "of 8 in 8..128")
    scale = getattr(ap, "scale", None)
    if scale is None or abs(float(scale) - (Cdim // heads) ** -0.5) > 1e-6 * (Cdim // heads) ** -0.5:
        raise NotImplementedError(f"{why}: attn_pool.scale = {scale!r} must be head_dim ** -0.5")
    if getattr(ap, "pool", "token") != "token":
        raise NotImplementedError(f"{why}: attn_pool.pool = {ap.pool!r} is not supported ('token')")
    norm = getattr(ap, "norm", None)
    if not isinstance(norm, nn.LayerNorm) or norm.weight is None or tuple(norm.normalized_shape) != (Cdim,):
        raise NotImplementedError(f"{why}: attn_pool.norm must be an affine nn.LayerNorm over the embed dim")
    mlp = getattr(ap, "mlp", None)
    fc1, fc2 = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    mlp_norm = getattr(mlp, "norm", None)
    if (not isinstance(fc1, nn.Linear) or not isinstance(fc2, nn.Linear) or fc1.in_features != Cdim or fc2.out_features != Cdim
            or fc1.out_features != fc2.in_features or (mlp_norm is not None and not isinstance(mlp_norm, nn.Identity))):
        raise NotImplementedError(f"{why}: attn_pool.mlp must be a plain Mlp (fc1 -> act -> fc2, no norm, not gated)")
    try:
        classify_mlp_act(getattr(mlp, "act", None))
    except NotImplementedError as e:
        raise NotImplementedError(f"{why}: attn_pool.{e}") from None
    return ap


class RAJNIViTWrapper(nn.Module):
    def __init__(self, base_model: nn.Module, pruning_schedule: Dict[int, Dict]):
        super().__init__()
        self.m = base_model
        self.blocks = base_model.blocks
        self.pruning_schedule = normalise_schedule(pruning_schedule)

        try:                       # block-level use of RAJNIAttention keeps the registers too; check_supported() reports problems
            prefix = model_num_prefix(base_model)
        except NotImplementedError:
            prefix = 1
        # the importance query (set_importance_query): None = the model's default, "cls" with a class token, "mean" without
        self._query = None
        for i, blk in enumerate(self.blocks):
            if i in self.pruning_schedule:
                cfg = self.pruning_schedule[i]
                if not isinstance(blk.attn, RAJNIAttention):
                    blk.attn = RAJNIAttention(blk.attn, keep_ratio=cfg["keep_ratio"], update=cfg["update"])
                else:  # re-wrapping an already wrapped base
                    blk.attn.keep_ratio, blk.attn.update = cfg["keep_ratio"], cfg["update"]
                blk.attn.num_prefix_tokens = prefix
                blk.attn.importance_query = self.importance_query
                blk.has_pruner = True
            else:
                blk.has_pruner = False

        self._last_stats = None
        self._weights = None       # packed device tensors (kept alive here)
        self._weights_key = None   # epoch of the last re-pack (part of the plan key)
        self._weights_sig = None   # [data_ptr..., _version...] of the base model's parameters at that re-pack
        self._weights_cfg = None
        self._plan = None          # most recent (key, VitPlan, keep-alive objects, stage buffers, counts)
        self._plans = {}           # small cache by key: a ragged last batch must not evict the main plan
        self._forced: Dict[int, torch.Tensor] = {}
        self._trace_scores = False
        # residual stream precision between blocks: fp32 (default; see DESIGN.md "numerics") or the
        # model's 16-bit dtype like the reference's bf16 / fp16 model (`set_residual_dtype(torch.bfloat16)` or
        # `(torch.float16)`; it must match the model dtype at forward)
        self._resid_bf16 = False   # 16-bit stream (rajni_vit_plan.resid_bf16)
        self._resid_dtype = torch.float32
        # storage format of the four big Linear weights of every block: "model" = the model dtype,
        # "fp8" = e4m3 bytes + per-row fp32 scale (`set_weight_format("fp8")`, bf16 models only)
        self._weight_format = "model"
        # opt-in: compute the last block for the CLS row only (the head reads nothing else, model.py:65-66)
        self._cls_only_last = False
        # timm's dynamic_img_size: any [B, C, H, W] the patch size divides, the position embedding resampled to its grid
        self._dynamic_img_size = bool(getattr(base_model, "dynamic_img_size", False))

    # ------------------------------------------------------------------------------------------
    def get_last_stats(self):
        return self._last_stats

    def get_last_trace(self) -> Dict[int, Dict[str, torch.Tensor]]:
        """Per scheduled block: keep_idx [B,Np] int64, next_scores [B,Np] (Np = prefix tokens + keep) and (if enabled
        with `trace_scores(True)`) the full scores [B,N] the stage ranked.  Test/diagnostic surface."""
        if self._plan is None:
            return {}
        out = {}
        for i, bufs in self._plan.bufs.items():
            idx = self._forced.get(i, bufs["keep_idx"])
            d = {"keep_idx": idx.long(), "next_scores": bufs["next_scores"]}
            # a stage ranks freshly computed scores iff `update` or nothing was carried into it
            # (attention.py:25); otherwise it ranked the previous stage's next_scores
            sched = self.pruning_schedule
            recomputed = sched[i]["update"] or (i - 1) not in sched
            if bufs["scores"] is not None and recomputed:
                d["scores"] = bufs["scores"]
            elif not recomputed:
                d["scores"] = self._plan.bufs[i - 1]["next_scores"]
            out[i] = d
        return out

    def _drop_plans(self):
        self._plan = None
        self._plans = {}

    def set_residual_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("residual stream dtype must be torch.float32, torch.bfloat16 or torch.float16")
        self._resid_bf16 = dtype != torch.float32
        self._resid_dtype = dtype
        self._drop_plans()
        return self

    @property
    def importance_query(self) -> str:
        """"cls" or "mean": what every scoring block uses as the importance query"""
        if self._query is not None:
            return self._query
        return "cls" if model_has_class_token(self.m) else "mean"

    def set_importance_query(self, query: str):
        """"cls": the class row (row 0) is the importance query - the reference's rule, the default of every model that has a
        class token.  "mean": the mean of the N query rows of the block's current sequence (include/rajni_hip_query.h; this
        project's own rule, pruning quality unmeasured) - the default and the only legal value for a model without a class
        token, selectable on class-token models too (the avg-pooled ones read the mean of the tokens)."""
        ops.query_code(query)
        if query == "cls" and not model_has_class_token(self.m):
            raise ValueError('set_importance_query("cls"): the model has no class token; "mean" is its only importance query')
        if query == "mean" and model_has_rel_pos(self.m, self.blocks):
            raise NotImplementedError('set_importance_query("mean"): not supported on a model with a relative position bias - '
                                      "importance is scored on the class row's biased logits, and a mean query has no position")
        if query != self.importance_query:
            self._drop_plans()
        self._query = query
        for blk in self.blocks:
            if isinstance(blk.attn, RAJNIAttention):
                blk.attn.importance_query = query
        return self

    def set_dynamic_img_size(self, on: bool = True):
        """timm's `dynamic_img_size=True`: accept any [B, C, H, W] whose H and W are multiples of the patch size.  The position
        embedding is resampled to the input's token grid as timm's resample_abs_pos_embed does (bicubic, antialias; one native
        launch per new grid, cached), prefix rows passed through.  Off (the default unless the base model says otherwise) the
        wrapper takes square inputs at the embedding's own grid, plus the reference's `pos_embed[:, :N]` slice."""
        if on and model_has_rel_pos(self.m, self.blocks):
            raise NotImplementedError("set_dynamic_img_size(True): not supported on a model with a relative position bias - timm "
                                      "resizes the bias table when the checkpoint is loaded, not per input; the model's own grid "
                                      "(rectangular or not) works")
        if bool(on) != self._dynamic_img_size:
            self._dynamic_img_size = bool(on)
            self._drop_plans()
        return self

    def _pos_source_grid(self, pos_rows: int, P: int):
        """(prefix rows of pos_embed, (src_h, src_w)): `patch_embed.grid_size` when it is a pair whose product is the embedding's
        patch-row count, else the integer square root of that count; the embedding has P prefix rows or none (no_embed_class)"""
        gs = getattr(self.m.patch_embed, "grid_size", None)
        if isinstance(gs, (tuple, list)) and len(gs) == 2 and all(isinstance(v, int) and v > 0 for v in gs):
            for pr in (P, 0):
                if gs[0] * gs[1] == pos_rows - pr:
                    return pr, (int(gs[0]), int(gs[1]))
        for pr in (P, 0):
            n = pos_rows - pr
            r = math.isqrt(n) if n > 0 else 0
            if r > 0 and r * r == n:
                return pr, (r, r)
        raise NotImplementedError(f"RAJNIViTWrapper: dynamic_img_size cannot tell the grid of a pos_embed of {pos_rows} rows "
                                  f"({P} prefix tokens): patch_embed.grid_size does not give it and it is not square")

    def _pos_for_grid(self, W, gh: int, gw: int, P: int, device, dtype):
        """(pos tensor [pr + gh * gw, C], pos_has_cls) under dynamic_img_size: the packed embedding itself at its own grid,
        otherwise the resampled rows - one launch, cached per (gh, gw, device, dtype) beside the packed weights, 8 entries"""
        pr, src = self._pos_source_grid(W["pos"].shape[0], P)
        if (gh, gw) == src:
            return W["pos"], int(pr > 0)
        cache = W.setdefault("pos_cache", {})
        key = (gh, gw, device, dtype)
        if key not in cache:
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            with nat.device_guard(device):
                cache[key] = ops.resample_pos_embed(W["pos"], src, (gh, gw), pr)
        return cache[key], int(pr > 0)

    def _rope_for_grid(self, W, gh: int, gw: int, device):
        """(cos, sin) fp32 device tensors [..., gh * gw, D] of the model's rotary table, converted once per grid and cached
        beside the packed weights like the resampled position embedding (8 entries; a plan keeps the pair it points to alive itself,
        PlanInput.rot, as it keeps its position rows).  The model's own table at its own grid;
        under dynamic_img_size the table of the input's grid, fetched as get_embed(shape=(gh, gw))."""
        d = W["desc"]
        cache = W.setdefault("rope_cache", {})
        key = (gh, gw, device)
        if key not in cache:
            kind, emb = rope_tables(self.m, d["H"], d["D"], d["depth"], (gh, gw) if self._dynamic_img_size else None)
            if kind != d["rope"]:
                raise NotImplementedError(f"RAJNIViTWrapper: model.rope.get_embed(shape=({gh}, {gw})) returns a {kind} table but "
                                          f"the model's own is {d['rope']}")
            if emb.shape[-2] != gh * gw:
                raise ValueError(f"model.rope's table has {emb.shape[-2]} rows but the input yields {gh * gw} patches; "
                                 "set_dynamic_img_size(True) fetches the table of the input's grid")
            sin, cos = emb.detach().to(device=device, dtype=torch.float32).chunk(2, dim=-1)
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            cache[key] = (cos.contiguous(), sin.contiguous())
        return cache[key]

    def set_weight_format(self, fmt: str):
        """"model" (default), "fp8" or "fp8_mfma".
        "fp8": keep qkv/proj/fc1/fc2 weights as fp8 e4m3 with one fp32 scale per output row (BASELINE config 5,
        SURVEY 8(f)-4).  Activations, accumulation, patch-embed and head stay as they are; results equal the same
        model run with the DEQUANTISED weights (the bf16 matrix pipe does the arithmetic).
        "fp8_mfma": the same weights, AND the inputs of qkv / fc1 / fc2 as per-row-scaled e4m3 (norm1 / norm2 emit
        them, fc1's GELU epilogue re-quantises the hidden activations), so that those three products run on the
        CDNA4 fp8 matrix pipe (v_mfma_f32_16x16x128_f8f6f4, fp32 accumulation).  Results equal the model run with
        the dequantised weights and the same activation quantisation (tests/test_gpu_fp8_mfma.py holds the rule);
        the reference has no fp8 semantics, so this is an opt-in numerics contract of the build's own.  Needs
        embed dim and MLP width that are multiples of 256."""
        if fmt not in ("model", "fp8", "fp8_mfma"):
            raise ValueError('weight format must be "model", "fp8" or "fp8_mfma"')
        if fmt == "fp8_mfma" and self._is_distilled():
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a distillation model (DeiT distilled) '
                                      'yet; "fp8" weights work')
        if fmt == "fp8_mfma" and isinstance(getattr(self.m, "head", None), nn.Identity):
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a headless model (head = nn.Identity); '
                                      '"fp8" weights work')
        if fmt == "fp8_mfma" and getattr(self.m, "global_pool", "token") == "map":
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a model with an attention pool '
                                      '(global_pool=\'map\'); "fp8" weights work')
        if fmt == "fp8_mfma" and self._norm_feature_or_none():
            raise NotImplementedError(f'set_weight_format("fp8_mfma"): not supported on a model with {self._norm_feature_or_none()}: '
                                      'the e4m3-output norm kernels are LayerNorm only ("fp8" weights work)')
        if fmt == "fp8_mfma" and getattr(self.m, "rope", None) is not None:
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a model with rotary position embeddings '
                                      '(model.rope): the e4m3 attention and its bounds were fitted to unrotated q and k ("fp8" '
                                      'weights work)')
        if fmt == "fp8_mfma" and model_has_rel_pos(self.m, self.blocks):
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a model with a relative position bias: the '
                                      'e4m3 attention and its bounds were fitted to logits without a bias ("fp8" weights work)')
        if fmt == "fp8_mfma" and any(mlp_norm_module(blk.mlp) is not None for blk in self.blocks):
            raise NotImplementedError('set_weight_format("fp8_mfma"): not supported on a model with a norm inside the MLP (mlp.norm): '
                                      'the fp8 x fp8 FC1 epilogue scales the hidden rows for FC2 before the norm could run ("fp8" '
                                      'weights work)')
        if fmt == "fp8_mfma" and self._mlp_act_or_none() == "quick_gelu":
            raise NotImplementedError('set_weight_format("fp8_mfma"): the model\'s MLPs use QuickGELU; the fp8 x fp8 FC1 epilogue '
                                      'and its hidden-activation bound are exact GELU only ("fp8" weights work)')
        if fmt == "fp8_mfma" and self._mlp_act_or_none() == "swiglu":
            raise NotImplementedError('set_weight_format("fp8_mfma"): the model\'s MLPs are gated (SwiGLU); the fp8 x fp8 FC1 epilogue '
                                      'and its hidden-activation bound are exact GELU only ("fp8" weights work)')
        if fmt != self._weight_format:
            self._weight_format = fmt
            self._weights = self._weights_key = None
            self._drop_plans()
        return self

    def dequantized_state_dict(self):
        """fp32 copies of the block Linear weights as the fp8 kernels see them (q * scale), keyed like the
        base model's state_dict.  Test surface: feed these to the oracle for the fp8 parity check."""
        if self._weights is None or self._weight_format not in ("fp8", "fp8_mfma"):
            raise RuntimeError("run a forward with set_weight_format('fp8') or ('fp8_mfma') first")
        out = {}
        hid, hpad = self._weights["desc"]["hidden"], self._weights["desc"]["hidden_pad"]
        gated = self._weights["desc"]["mlp_act"] == "swiglu"
        for i, bw in enumerate(self._weights["blocks"]):
            for ours, theirs in (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
                w = ops.dequantize_fp8(bw[ours + "_w"], bw[ours + "_s"])
                if ours == "fc1" and gated:
                    # gate rows, then value rows, as packed; keyed like the base model: a packed fc1 (in ITS order, gate_last
                    # models have the value first), or the split pair
                    mlp = self.blocks[i].mlp
                    wg, wv = w[:hid], w[hpad:hpad + hid]
                    if gated_mlp_form(mlp) == "split":
                        out[f"blocks.{i}.mlp.fc1_g.weight"], out[f"blocks.{i}.mlp.fc1_x.weight"] = wg, wv
                        continue
                    w = torch.cat([wv, wg] if getattr(mlp, "gate_last", False) else [wg, wv])
                elif ours == "fc1":
                    w = w[:hid]               # rows / columns past the model's MLP width are zero padding
                elif ours == "fc2":
                    w = w[:, :hid]
                elif ours == "qkv" and qkv_form(self.blocks[i].attn) == "split":      # keyed like the base model here too
                    for name, part in zip(("q_proj", "k_proj", "v_proj"), w.chunk(3)):
                        out[f"blocks.{i}.attn.{name}.weight"] = part
                    continue
                out[f"blocks.{i}.{theirs}.weight"] = w
        return out

    def set_last_block_cls_only(self, on: bool = True):
        """When the last block is not a pruning stage, run it for the CLS row only: CLS-query attention over all
        tokens, proj / MLP on B rows.  The logits are the same function of the input (the reference's head reads
        x[:, 0] only); the other rows of the last block are never formed.  Off by default: the default forward
        executes the reference's op graph row for row."""
        if on and not model_has_class_token(self.m):
            raise ValueError("set_last_block_cls_only: the model has no class token; there is no class row to form")
        if on and self._is_distilled():
            raise ValueError("set_last_block_cls_only: the model is a distillation model (DeiT distilled) whose head reads two rows; "
                             "the CLS-only last block forms the class row only (the default forward already computes the last "
                             "block for those two rows)")
        if on and self._pool_kind() == "avg":
            raise ValueError("set_last_block_cls_only: the model pools with global_pool='avg'; the CLS-only last block never "
                             "forms the rows to be averaged")
        if on and self._pool_kind() == "map":
            raise ValueError("set_last_block_cls_only: the model pools with global_pool='map'; the CLS-only last block never "
                             "forms the rows the attention pool reads")
        if on and model_has_rel_pos(self.m, self.blocks):
            raise NotImplementedError("set_last_block_cls_only: not supported on a model with a relative position bias - the "
                                      "CLS-query kernel of that opt-in takes no bias (the default forward already computes the "
                                      "last block for the rows the head reads)")
        if bool(on) != self._cls_only_last:
            self._cls_only_last = bool(on)
            self._drop_plans()
        return self

    def trace_scores(self, on: bool = True):
        self._trace_scores = bool(on)
        self._drop_plans()
        return self

    def force_keep_idx(self, forced: Optional[Dict[int, torch.Tensor]]):
        """Test hook for selection-conditional parity: use the given keep_idx
        ([B, P+keep]: the P prefix tokens 0..P-1 first - P = 1, the class token, without register tokens - then
        ascending patch indices) in the listed blocks instead of the device selection."""
        self._forced = {}
        for k, v in (forced or {}).items():
            self._forced[int(k)] = v.to(torch.int32).contiguous()
        self._drop_plans()
        return self

    # ------------------------------------------------------------------------------------------
    def _pool_kind(self) -> str:
        """'token', 'avg' or 'map': `base_model.global_pool` when the attribute exists, else 'token'.  ('map' is the attention
        pool; `attn_pool_module` holds the model's `attn_pool` to its contract.)"""
        pool = getattr(self.m, "global_pool", "token")
        if pool not in ("token", "avg", "map"):
            raise NotImplementedError(f"RAJNIViTWrapper: global_pool={pool!r} is not supported ('token', 'avg' or 'map')")
        return pool

    def _is_distilled(self) -> bool:
        """the base model has the distillation pair, well formed or not (`_describe` reports what is wrong with it)"""
        return getattr(self.m, "dist_token", None) is not None or getattr(self.m, "head_dist", None) is not None

    def _mlp_act_or_none(self) -> Optional[str]:
        """the blocks' MLP activation where they agree on a supported one, else None (`_describe` reports why)"""
        try:
            kinds = {"swiglu" if gated_mlp_form(blk.mlp) else classify_mlp_act(getattr(blk.mlp, "act", None)) for blk in self.blocks}
        except (NotImplementedError, AttributeError):
            return None
        return kinds.pop() if len(kinds) == 1 else None

    def _norm_feature_or_none(self) -> Optional[str]:
        """"RMSNorm" / "patch_embed.norm" where the model needs the norm record (rajni_vit_norm), else None (`_describe` reports
        what is wrong with a norm it does not recognise)"""
        pe_norm = getattr(self.m.patch_embed, "norm", None)
        try:
            dim = model_embed_dim(self.m)
            if classify_norm(self.blocks[0].norm1, dim) == "rms":
                return "RMSNorm"
        except (NotImplementedError, AttributeError):
            pass
        return "patch_embed.norm" if pe_norm is not None and not isinstance(pe_norm, nn.Identity) else None

    def check_supported(self) -> Dict:
        """Raise NotImplementedError if the base model has a feature the native forward does not compute (host only, no
        device needed; `forward` runs the same check).  Returns the model description."""
        return self._describe()

    def _describe(self):
        m = self.m
        num_prefix = model_num_prefix(m)
        pe = m.patch_embed.proj
        if not isinstance(pe, nn.Conv2d) or pe.kernel_size != pe.stride or pe.kernel_size[0] != pe.kernel_size[1]:
            raise NotImplementedError("RAJNIViTWrapper: patch_embed.proj must be a square Conv2d with stride == kernel")
        pe_norm = getattr(m.patch_embed, "norm", None)
        pe_norm = None if isinstance(pe_norm, nn.Identity) else pe_norm
        # timm num_classes=0 (the DINOv2 checkpoints, any backbone use): head is nn.Identity and forward returns the pooled feature
        headless = isinstance(m.head, nn.Identity)
        if not headless and not isinstance(m.head, nn.Linear):
            raise NotImplementedError("RAJNIViTWrapper: base_model.head must be nn.Linear or nn.Identity")
        if headless and self._weight_format == "fp8_mfma":
            raise NotImplementedError('weight format "fp8_mfma" on a headless model (head = nn.Identity) is not supported; '
                                      '"fp8" weights work')
        blk0 = self.blocks[0]
        has_cls = model_has_class_token(m)
        if not has_cls and self._cls_only_last:
            raise ValueError("a model without a class token with set_last_block_cls_only(True): there is no class row to form")
        if not has_cls and self._weight_format == "fp8_mfma":
            raise NotImplementedError('weight format "fp8_mfma" on a model without a class token is not supported; "fp8" weights work')
        Cdim = model_embed_dim(m)
        heads = blk0.attn.num_heads
        try:      # (before anything reads its eps: an unrecognised norm is refused as that)
            classify_norm(blk0.norm1, Cdim)
        except NotImplementedError as e:
            raise NotImplementedError(f"RAJNIViTWrapper: blocks.0.norm1: {e}") from None
        # FC2's K and the hidden buffer's width: of a gated MLP (SwiGLU) too, whose FC1 has twice as many rows
        desc = dict(C=Cdim, H=heads, D=Cdim // heads, depth=len(self.blocks), hidden=blk0.mlp.fc2.in_features,
                    num_classes=0 if headless else m.head.out_features, patch=pe.kernel_size[0], in_chans=pe.in_channels,
                    ln_eps=float(blk0.norm1.eps), scale=float(blk0.attn.scale), headless=headless)
        desc["hidden_pad"] = (desc["hidden"] + 63) // 64 * 64

        # ONE norm kind per model (rajni_vit_norm.kind): norm1, norm2, norm, fc_norm, norm_pre and patch_embed.norm are all
        # affine LayerNorms or all RMSNorms; blocks.0.norm1 says which, and every other one is held to it by name
        def kind_of(mod, name):
            try:
                return classify_norm(mod, Cdim)
            except NotImplementedError as e:
                raise NotImplementedError(f"RAJNIViTWrapper: {name}: {e}") from None

        desc["norm_kind"] = kind_of(blk0.norm1, "blocks.0.norm1")

        def same_kind(mod, name):
            kind = kind_of(mod, name)
            if kind != desc["norm_kind"]:
                raise NotImplementedError(f"RAJNIViTWrapper: {name} is {kind} but blocks.0.norm1 is {desc['norm_kind']}: mixed "
                                          f"norm kinds in one model are not supported")

        desc["embed_norm"] = pe_norm is not None
        if pe_norm is not None:
            same_kind(pe_norm, "patch_embed.norm")
            desc["embed_norm_eps"] = float(pe_norm.eps)
        feature = "RMSNorm" if desc["norm_kind"] == "rms" else ("patch_embed.norm" if pe_norm is not None else None)
        if feature and Cdim > NORM_MAX_C:
            raise NotImplementedError(f"RAJNIViTWrapper: {feature} on an embed dim of {Cdim}: the row kernels hold a row in one "
                                      f"wave's registers and take C <= {NORM_MAX_C}")
        if feature and self._weight_format == "fp8_mfma":
            raise NotImplementedError(f'weight format "fp8_mfma" on a model with {feature} is not supported: the e4m3-output norm '
                                      f'kernels are LayerNorm only; "fp8" weights work')
        for i, blk in enumerate(self.blocks):
            for nm, ln in (("norm1", blk.norm1), ("norm2", blk.norm2)):
                same_kind(ln, f"blocks.{i}.{nm}")
                if float(ln.eps) != desc["ln_eps"]:
                    raise NotImplementedError(f"RAJNIViTWrapper: blocks.{i}.{nm} has eps {float(ln.eps)} but blocks.0.norm1 has "
                                              f"{desc['ln_eps']}: the block norms and the final norm share one eps")
            try:
                form = gated_mlp_form(blk.mlp)
                kind = "swiglu" if form else classify_mlp_act(getattr(blk.mlp, "act", None))
            except NotImplementedError as e:
                raise NotImplementedError(f"block {i}: {e}") from None
            if desc.setdefault("mlp_act", kind) != kind:
                raise NotImplementedError(f"block {i}: mlp.act differs between blocks ({kind} after {desc['mlp_act']})")
            # the norm inside the MLP (rajni_vit_mlp_norm): in every block or in none, of the model's one kind, with one eps
            mlp_norm = mlp_norm_module(blk.mlp)
            if i == 0:
                desc["mlp_norm"] = mlp_norm is not None
            if (mlp_norm is not None) != desc["mlp_norm"]:
                which = f"mlp.norm ({type(mlp_norm).__name__})" if mlp_norm is not None else "no mlp.norm"
                raise NotImplementedError(f"block {i}: {type(blk.mlp).__name__}: {which} where block 0 has "
                                          f"{'one' if desc['mlp_norm'] else 'none'}: a norm inside the MLP in every block or in none")
            if mlp_norm is not None:
                try:
                    kind = classify_norm(mlp_norm, desc["hidden"])
                except NotImplementedError as e:
                    raise NotImplementedError(f"RAJNIViTWrapper: blocks.{i}.mlp.norm: {e}") from None
                if kind != desc["norm_kind"]:
                    raise NotImplementedError(f"RAJNIViTWrapper: blocks.{i}.mlp.norm is {kind} but blocks.0.norm1 is "
                                              f"{desc['norm_kind']}: mixed norm kinds in one model are not supported")
                if float(mlp_norm.eps) != desc.setdefault("mlp_norm_eps", float(mlp_norm.eps)):
                    raise NotImplementedError(f"RAJNIViTWrapper: blocks.{i}.mlp.norm has eps {float(mlp_norm.eps)} but blocks.0.mlp.norm "
                                              f"has {desc['mlp_norm_eps']}: the norms inside the MLPs share one eps")
            try:      # the spellings of the block: LayerScale and the q / k / v projection
                block_layer_scales(blk, f"block {i}")
                qkv_form(blk.attn, f"block {i}")
            except NotImplementedError as e:
                raise NotImplementedError(f"RAJNIViTWrapper: {e}") from None
            qk = qk_norm_modules(blk.attn, f"block {i}")
            if i == 0:
                desc["qk_norm"] = qk is not None
                desc["qk_eps"] = float(qk[0].eps) if qk else 0.0
            if (qk is not None) != desc["qk_norm"] or (qk and float(qk[0].eps) != desc["qk_eps"]):
                raise NotImplementedError(f"block {i}: attn.q_norm / attn.k_norm differ between blocks (presence or eps)")
            if qk and tuple(qk[0].normalized_shape) != (desc["D"],):
                raise NotImplementedError(f"block {i}: attn.q_norm must be nn.LayerNorm over the head dim {desc['D']}")
            if blk.attn.num_heads != heads or float(blk.attn.scale) != desc["scale"]:
                raise NotImplementedError(f"block {i}: heads/scale differ between blocks")
        if desc["mlp_norm"] and desc["hidden"] > nat.HIDDEN_NORM_MAX:
            raise NotImplementedError(f"RAJNIViTWrapper: mlp.norm over an MLP width of {desc['hidden']}: the row kernel holds a row "
                                      f"in one wave's registers and takes up to {nat.HIDDEN_NORM_MAX} columns")
        if desc["mlp_norm"] and self._weight_format == "fp8_mfma":      # (the norm was attached after the setter)
            raise NotImplementedError('weight format "fp8_mfma" on a model with a norm inside the MLP (mlp.norm) is not supported; '
                                      '"fp8" weights work')
        # timm's head: norm -> pool -> fc_norm -> head, `norm` and `fc_norm` each an affine LayerNorm or Identity
        desc["pool"] = self._pool_kind()
        # the attention pool of global_pool='map' (None for every other head): its heads, its MLP's width and activation
        ap = attn_pool_module(m)
        if ap is not None:
            if feature:
                raise NotImplementedError(f"RAJNIViTWrapper: global_pool='map' on a model with {feature} is not supported: the "
                                          f"attention-pool tail's norms are LayerNorm only")
            if self._cls_only_last:
                raise ValueError("global_pool='map' with set_last_block_cls_only(True): that opt-in never forms the rows the "
                                 "attention pool reads")
            if self._weight_format == "fp8_mfma":
                raise NotImplementedError('weight format "fp8_mfma" on a model with an attention pool (global_pool=\'map\') is '
                                          'not supported; "fp8" weights work')
            hid = ap.mlp.fc2.in_features
            desc["attn_pool"] = dict(heads=int(ap.num_heads), hidden=hid, hidden_pad=(hid + 63) // 64 * 64,
                                     act=classify_mlp_act(ap.mlp.act), eps=float(ap.norm.eps))
        # prefix tokens: the class token plus timm's register tokens (never pruned, never ranked; 'avg' pools behind them)
        desc["num_prefix"] = num_prefix
        desc["class_token"] = has_cls
        # rows of each image the head reads: 2 = DeiT distilled, the class and distillation rows through two averaged heads
        desc["head_rows"] = 2 if has_cls and model_is_distilled(m) else 1
        if desc["head_rows"] == 2 and self._cls_only_last:
            raise ValueError("a distillation model with set_last_block_cls_only(True): that opt-in forms the class row only")
        n_patches = getattr(m.patch_embed, "num_patches", None)
        if has_cls and num_prefix > 1 and isinstance(n_patches, int) and m.pos_embed is not None and m.pos_embed.shape[-2] not in (n_patches, n_patches + num_prefix):
            raise NotImplementedError(f"RAJNIViTWrapper: pos_embed has {m.pos_embed.shape[-2]} rows; with {num_prefix} prefix tokens "
                                      f"and {n_patches} patches it must have {n_patches} (no_embed_class) or {n_patches + num_prefix}")
        fc_norm = getattr(m, "fc_norm", None)
        desc["fc_norm"] = fc_norm is not None and not isinstance(fc_norm, nn.Identity)
        desc["norm"] = not isinstance(m.norm, nn.Identity)
        if desc["norm"]:
            same_kind(m.norm, "norm")
            if float(m.norm.eps) != desc["ln_eps"]:
                raise NotImplementedError(f"RAJNIViTWrapper: base_model.norm has eps {float(m.norm.eps)} but the blocks' norms "
                                          f"have {desc['ln_eps']}: the block norms and the final norm share one eps")
        if not desc["norm"] and not desc["fc_norm"]:
            raise NotImplementedError("RAJNIViTWrapper: base_model.norm must be a norm layer with the blocks' eps "
                                      "(nn.Identity only together with an fc_norm)")
        if desc["pool"] == "map" and not desc["norm"]:
            raise NotImplementedError("RAJNIViTWrapper: global_pool='map' on a model whose norm is nn.Identity (timm fc_norm=True "
                                      "moves the final norm behind the pool): the attention pool then reads the un-normalised "
                                      "stream, which has no native row kernel yet")
        norm_pre = getattr(m, "norm_pre", None)
        desc["norm_pre"] = norm_pre is not None and not isinstance(norm_pre, nn.Identity)
        for name, mod, on in (("fc_norm", fc_norm, desc["fc_norm"]), ("norm_pre", norm_pre, desc["norm_pre"])):
            if on:
                same_kind(mod, name)
        if desc["pool"] == "avg" and self._cls_only_last:
            raise ValueError("global_pool='avg' with set_last_block_cls_only(True): that opt-in never forms the rows to be averaged")
        # plans that need none of these keep calling rajni_vit_forward
        desc["ext"] = (desc["qk_norm"] or desc["norm_pre"] or desc["fc_norm"] or not desc["norm"] or desc["pool"] != "token"
                       or desc["mlp_act"] != "gelu")
        # ... and plans that need no norm record keep the entry point they had
        desc["norm_record"] = feature is not None
        # rotary positions (rajni_vit_rope): what the model's own table covers and how it pairs the elements; None without
        rope = rope_tables(m, heads, desc["D"], desc["depth"])
        desc["rope"] = rope[0] if rope else None
        if rope:
            desc["rope_half"] = rope_layout(self.blocks)
            for i, blk in enumerate(self.blocks):
                npt = getattr(blk.attn, "num_prefix_tokens", num_prefix)
                if npt != num_prefix:
                    raise NotImplementedError(f"RAJNIViTWrapper: block {i}: attn.num_prefix_tokens = {npt} but the model has "
                                              f"{num_prefix} prefix tokens: the rotation skips exactly the prefix rows")
            if self._weight_format == "fp8_mfma":      # (the table was attached after the setter)
                raise NotImplementedError('weight format "fp8_mfma" on a model with rotary position embeddings (model.rope) is '
                                          'not supported; "fp8" weights work')
        # a learned relative position bias (rajni_vit_relpos): None, "block" (every attention has its own, with or without a
        # shared one beside it) or "shared" (the model's alone), and the grid it is stated on.  Everything outside the native
        # contract is refused here, on the host, before any launch
        per, shared = rel_pos_sources(m, self.blocks)
        desc["rel_pos"] = "block" if per else "shared" if shared else None
        if desc["rel_pos"]:
            what = "a model with a relative position bias"
            if desc["D"] != 64:
                raise NotImplementedError(f"RAJNIViTWrapper: {what} and head dim {desc['D']}: the bias kernels are head dim 64 only")
            if self._weight_format == "fp8_mfma":
                raise NotImplementedError(f'weight format "fp8_mfma" on {what} is not supported; "fp8" weights work')
            if not has_cls or self.importance_query != "cls":
                raise NotImplementedError(f"RAJNIViTWrapper: {what} " + ("without a class token" if not has_cls else
                                          'with the mean importance query (set_importance_query("mean"))') + ": importance is "
                                          "scored on the class row's biased logits, and a mean query has no position")
            if self._dynamic_img_size:
                raise NotImplementedError(f"RAJNIViTWrapper: {what} with dynamic_img_size: timm resizes the bias table when the "
                                          "checkpoint is loaded, not per input")
            if rope:
                raise NotImplementedError(f"RAJNIViTWrapper: {what} that also has rotary position embeddings (model.rope): RoPE "
                                          "together with a bias is not supported")
            if self._cls_only_last:
                raise NotImplementedError(f"RAJNIViTWrapper: {what} with set_last_block_cls_only(True): the CLS-query kernel of "
                                          "that opt-in takes no bias")
            first = dense_rel_pos_bias(per[0] if per else shared, heads, "RAJNIViTWrapper: relative position bias")
            gh, gw = rel_pos_grid(m, self.blocks, first.shape[1] - num_prefix)
            if gh > nat.RELPOS_MAX_GRID or gw > nat.RELPOS_MAX_GRID:
                raise NotImplementedError(f"RAJNIViTWrapper: a relative position bias on a {gh} x {gw} grid: the cap is "
                                          f"{nat.RELPOS_MAX_GRID} x {nat.RELPOS_MAX_GRID} patches")
            desc["rel_pos_grid"] = (gh, gw)
        return desc

    def _all_params(self):
        """The base model's parameters.  Walking the module tree costs ~150 us per call - exposed latency in the
        sync -> forward -> sync metric of evaluate_model - so the walk is cached, and the cache is VALIDATED on every
        call with plain dict lookups: every (parent, name, child module) and (owner, name, Parameter) slot recorded by
        the walk must still hold the same object.  A replaced module (`model.head = nn.Linear(C, 10)`) or a re-assigned
        `nn.Parameter` therefore re-walks and re-packs on the very next forward, like the reference, which reads the
        live modules on every call; in-place changes, `.to()` and `load_state_dict` are seen through data_ptr / _version."""
        slots = getattr(self, "_param_slots", None)
        if slots is not None:
            mods, pars = slots
            ok = True
            for parent, name, child in mods:
                if parent._modules.get(name) is not child:
                    ok = False
                    break
            if ok:
                for owner, name, par in pars:
                    if owner._parameters.get(name) is not par:
                        ok = False
                        break
            if ok:
                return self._param_list
        mods, pars = [], []
        for mod in self.m.modules():
            for name, child in mod._modules.items():
                mods.append((mod, name, child))
            for name, par in mod._parameters.items():
                pars.append((mod, name, par))
        self._param_slots = (mods, pars)
        self._param_list = [p for p in self.m.parameters()]
        return self._param_list

    def _pack_weights(self, device, dtype):
        params = self._all_params()
        # fingerprint of the live weights: storage pointers (`.to()`, `param.data = ...`) and version counters (in-place
        # edits, load_state_dict) - two flat list comprehensions and one C-speed list compare per forward (this sits in
        # the sync -> forward -> sync metric); `_weights_key` is just the epoch of the last re-pack
        sig = [p.data_ptr() for p in params]
        sig += [p._version for p in params]
        cfg_key = (device, dtype, self._weight_format, getattr(self.m, "global_pool", "token"))
        if self._weights is not None and self._weights_sig == sig and self._weights_cfg == cfg_key:
            return self._weights
        key = (getattr(self, "_weights_epoch", 0) + 1)
        self._weights_epoch = key
        desc = self._describe()
        m = self.m
        fp8 = self._weight_format in ("fp8", "fp8_mfma")
        if self._weight_format == "fp8_mfma" and desc["head_rows"] == 2:
            raise NotImplementedError('weight format "fp8_mfma" on a distillation model (DeiT distilled) is not supported yet')
        if self._weight_format == "fp8_mfma" and desc["mlp_act"] == "swiglu":   # (the MLP was swapped after the setter)
            raise NotImplementedError('weight format "fp8_mfma" with a gated (SwiGLU) MLP: the fp8 x fp8 FC1 epilogue is exact GELU only')
        if self._weight_format == "fp8_mfma" and desc["mlp_act"] != "gelu":   # (the activation was swapped after the setter)
            raise NotImplementedError('weight format "fp8_mfma" with a QuickGELU MLP: the fp8 x fp8 FC1 epilogue is exact GELU only')
        if fp8 and dtype != torch.bfloat16:
            raise NotImplementedError("fp8 weights need a bf16 model (activations stay bf16)")
        pw = lambda w: ops.pack_weight(w, dtype, device)
        # block Linear weight -> (packed tensor, per-row scale or None)
        pq = (lambda w: ops.pack_weight_fp8(w, dtype, device)) if fp8 else (lambda w: (pw(w), None))
        pv = lambda v: ops.pack_vec(v, dtype, device)
        zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=device)
        W = dict(desc=desc)
        W["patch_w"] = ops.pack_weight(m.patch_embed.proj.weight, dtype, device, k_multiple=64)
        W["patch_b"] = pv(m.patch_embed.proj.bias) if m.patch_embed.proj.bias is not None else zeros(desc["C"])
        W["cls"] = m.cls_token.detach().to(device=device, dtype=dtype).reshape(-1).contiguous() if desc["class_token"] else None
        # the prefix rows behind the class token: timm's registers, or the distillation token (one row, the same record);
        # without a class token the registers are all the prefix rows there are
        reg_src = m.dist_token if desc["head_rows"] == 2 else \
            (m.reg_token if desc["num_prefix"] > (1 if desc["class_token"] else 0) else None)
        W["reg"] = (reg_src.detach().to(device=device, dtype=dtype).reshape(-1, desc["C"]).contiguous()
                    if reg_src is not None else None)
        # (pos_embed None - rotary positions alone: _build_plan hands the patch GEMM a zero table of the input's grid)
        W["pos"] = (m.pos_embed.detach().to(device=device, dtype=dtype).reshape(-1, desc["C"]).contiguous()
                    if m.pos_embed is not None else None)
        rms = desc["norm_kind"] == "rms"      # no bias vector is packed or passed: the RMS kernels read none
        nb = lambda mod: None if rms else pv(getattr(mod, "bias", None))
        W["norm_w"], W["norm_b"] = (pv(m.norm.weight), nb(m.norm)) if desc["norm"] else (None, None)
        if desc["norm"] and W["norm_b"] is None and not rms:
            W["norm_b"] = zeros(desc["C"])
        pe_norm = m.patch_embed.norm if desc["embed_norm"] else None
        W["embed_norm_w"], W["embed_norm_b"] = (pv(pe_norm.weight), nb(pe_norm)) if pe_norm is not None else (None, None)
        for name in ("norm_pre", "fc_norm"):      # rajni_vit_ext (a missing bias stays None = 0)
            mod = getattr(m, name, None) if desc[name] else None
            W[name + "_w"], W[name + "_b"] = (pv(mod.weight), nb(mod)) if mod is not None else (None, None)
            W[name + "_eps"] = float(mod.eps) if mod is not None else 0.0
        if desc["headless"]:
            W["head_w"] = W["head_b"] = None      # rajni_vit_plan: head_w NULL and num_classes 0, no head GEMM
        elif desc["head_rows"] == 2:
            # (head(n0) + head_dist(n1)) / 2 as ONE linear layer over [n0 | n1]: weight [classes, 2C] = [W / 2 | W_dist / 2]
            # (halving is exact), bias (b + b_dist) / 2 in fp32.  Plain tensors built here, not parameters of the module.
            W["head_w"] = pw(torch.cat([0.5 * m.head.weight.detach().float(), 0.5 * m.head_dist.weight.detach().float()], dim=1))
            hb = [pv(h.bias) if h.bias is not None else zeros(desc["num_classes"]) for h in (m.head, m.head_dist)]
            W["head_b"] = (0.5 * (hb[0] + hb[1])).contiguous()      # the sum of the two held values, not rounded to the model dtype again
        else:
            W["head_w"] = pw(m.head.weight)
            W["head_b"] = pv(m.head.bias) if m.head.bias is not None else zeros(desc["num_classes"])
        if "attn_pool" in desc:
            # the attention pool (rajni_vit_attn_pool), never e4m3 whatever the block weights' format is - like the head.  kv runs
            # on all surviving rows and is packed in the model dtype; proj / fc1 / fc2 run on B rows in fp32 (the 16-bit roundings
            # of a pooled row cost 0.2 - 0.4 % of the logit scale each): fp32 copies of the values the model dtype holds.
            # Its query does not depend on the image: q = q_lin(latent) * scale, once per pack, fp32 from the same values.
            # An MLP width that is not whole 64-wide K steps is zero-padded as the blocks' is.
            ap, pd = m.attn_pool, desc["attn_pool"]
            f32 = lambda t: t.detach().to(device=device, dtype=dtype).to(torch.float32)
            pw32 = lambda w_, **kw: ops.pack_weight(f32(w_), torch.float32, device, **kw)
            qv = f32(ap.latent).reshape(1, desc["C"]) @ f32(ap.q.weight).t()
            if ap.q.bias is not None:
                qv = qv + f32(ap.q.bias)
            hid, hpad = pd["hidden"], pd["hidden_pad"]
            fc1_b = pv(ap.mlp.fc1.bias) if ap.mlp.fc1.bias is not None else zeros(hid)
            W["attn_pool"] = dict(
                q=(qv * float(ap.scale)).reshape(pd["heads"], desc["C"] // pd["heads"]).contiguous(),
                kv_w=pw(ap.kv.weight), kv_b=pv(ap.kv.bias), proj_w=pw32(ap.proj.weight), proj_b=pv(ap.proj.bias),
                norm_w=pv(ap.norm.weight), norm_b=pv(ap.norm.bias) if ap.norm.bias is not None else zeros(desc["C"]),
                fc1_w=pw32(ap.mlp.fc1.weight), fc1_b=torch.cat([fc1_b, zeros(hpad - hid)]) if hpad != hid else fc1_b,
                fc2_w=pw32(ap.mlp.fc2.weight, k_multiple=64), fc2_b=pv(ap.mlp.fc2.bias))
        blocks = []
        for blk in self.blocks:
            a = blk.attn
            g1, g2 = (pv(g) for g in block_layer_scales(blk, "RAJNIViTWrapper"))
            for dp in (getattr(blk, "drop_path1", None), getattr(blk, "drop_path2", None)):
                if dp is not None and not isinstance(dp, nn.Identity) and self.training:
                    raise NotImplementedError("drop_path in training mode: this is the inference path")
            # (q_proj / k_proj / v_proj, or a bias-free qkv beside q_bias / v_bias: packed here, once, into the one [3C, C] weight)
            qkv_weight, qkv_bias = packed_qkv(a)
            (qkv_w, qkv_s), (proj_w, proj_s) = pq(qkv_weight), pq(a.proj.weight)
            # An MLP width that is not whole 64-wide K steps (so400m: 4304) is zero-padded: fc1 gets zero rows (it
            # has them anyway, up to the next 256) with zero bias, GELU(0) = 0 (QuickGELU(0) = 0 alike) lands in the padding columns of the
            # hidden buffer, and fc2's zero-padded input columns ignore them - exact, no kernel involved.
            hid, hpad = desc["hidden"], desc["hidden_pad"]
            gated = desc["mlp_act"] == "swiglu"
            if gated:
                # SwiGLU: fc1_w is [2 hpad, C] - gate rows [0, hpad), value rows [hpad, 2 hpad), the order RAJNI_EPI_BIAS_SWIGLU
                # reads with N = hpad.  An odd width is zero-padded PER HALF (zero rows, zero bias, unit scales):
                # silu(0) * 0 = 0 lands in the padding columns of the hidden buffer
                wg, wv, bg, bv = gated_fc1(blk.mlp, gated_mlp_form(blk.mlp))
                rows = lambda w: torch.cat([w.detach(), w.new_zeros((hpad - hid, w.shape[1]))]) if hpad != hid else w.detach()
                # (fp8: an all-zero row quantises with scale 1, quantize_rows_fp8 - the padding rows' scales need no patching)
                (fc1_w, fc1_s) = pq(torch.cat([rows(wg), rows(wv)]))
            else:
                (fc1_w, fc1_s) = pq(blk.mlp.fc1.weight)
            if fp8:
                fc2_w, fc2_s = ops.pack_weight_fp8(blk.mlp.fc2.weight, dtype, device, k_multiple=64)
                if hpad != hid and not gated:
                    fc1_s = torch.cat([fc1_s, torch.ones(hpad - hid, dtype=fc1_s.dtype, device=fc1_s.device)])
            else:
                fc2_w, fc2_s = ops.pack_weight(blk.mlp.fc2.weight, dtype, device, k_multiple=64), None
            if gated:
                half = lambda b: torch.cat([pv(b) if b is not None else zeros(hid), zeros(hpad - hid)])
                fc1_b = torch.cat([half(bg), half(bv)]).contiguous()
            else:
                fc1_b = pv(blk.mlp.fc1.bias) if blk.mlp.fc1.bias is not None else zeros(hid)
                if hpad != hid:
                    fc1_b = torch.cat([fc1_b, zeros(hpad - hid)])
            blocks.append(dict(
                norm1_w=pv(blk.norm1.weight), norm1_b=nb(blk.norm1),
                qkv_w=qkv_w, qkv_s=qkv_s, qkv_b=pv(qkv_bias) if qkv_bias is not None else zeros(3 * desc["C"]),
                proj_w=proj_w, proj_s=proj_s, proj_b=pv(a.proj.bias) if a.proj.bias is not None else zeros(desc["C"]),
                ls1=g1, norm2_w=pv(blk.norm2.weight), norm2_b=nb(blk.norm2),
                fc1_w=fc1_w, fc1_s=fc1_s, fc1_b=fc1_b,
                fc2_w=fc2_w, fc2_s=fc2_s, fc2_b=pv(blk.mlp.fc2.bias), ls2=g2))
            if desc["mlp_norm"]:      # rajni_vit_mlp_norm: [hidden] fp32, the true width (no bias vector for the RMS kind)
                mn = mlp_norm_module(blk.mlp)
                blocks[-1].update(mlp_norm_w=pv(mn.weight), mlp_norm_b=nb(mn))
            if desc["qk_norm"]:
                q, k = qk_norm_modules(a)
                blocks[-1].update(q_norm_w=pv(q.weight), q_norm_b=pv(q.bias), k_norm_w=pv(k.weight), k_norm_b=pv(k.bias))
            if self._weight_format == "fp8_mfma":
                # constants of the hidden-activation bound (rajni_layernorm_fp8): largest row norm of the DEQUANTISED
                # fc1 weight and largest |bias| as the kernels hold it
                wd = ops.dequantize_fp8(fc1_w, fc1_s)
                blocks[-1]["fc1_rownorm_max"] = float(wd.norm(dim=1).max())
                blocks[-1]["fc1_bias_absmax"] = float(fc1_b.abs().max())
                # the one scale of the e4m3 attention output (rajni_attention_fp8), from the V rows of the dequantised qkv weight
                C = desc["C"]
                vd = ops.dequantize_fp8(qkv_w, qkv_s)[2 * C:3 * C]
                blocks[-1]["attn_out_scale"] = ops.attention_out_scale(blocks[-1]["norm1_w"], blocks[-1]["norm1_b"], vd,
                                                                       blocks[-1]["qkv_b"][2 * C:3 * C])
        if desc["rel_pos"]:
            # rajni_vit_relpos: every block's dense bias - its own plus the shared one (timm adds both) - decomposed into the
            # table and the three prefix values, fp32.  Packed here, once; the tables are parameters of the model, so a change
            # re-packs them with everything else (the fingerprint above)
            per, shared = rel_pos_sources(m, self.blocks)
            gh, gw = desc["rel_pos_grid"]
            sh = dense_rel_pos_bias(shared, desc["H"], "RAJNIViTWrapper: the shared relative position bias") if shared else None
            parts = []
            for i in range(desc["depth"] if per else 1):
                where = f"RAJNIViTWrapper: block {i}: relative position bias" if per else "RAJNIViTWrapper: the shared relative position bias"
                dense = dense_rel_pos_bias(per[i], desc["H"], where) if per else sh
                if per and sh is not None:
                    dense = dense + sh
                parts.append(decompose_rel_pos_bias(dense, gh, gw, desc["num_prefix"], where))
            stack = lambda j: torch.stack([p_[j] for p_ in parts]).to(device=device, dtype=torch.float32).contiguous()
            W["rel_pos"] = dict(table=stack(0), prefix_q=stack(1), prefix_k=stack(2), prefix_qk=stack(3),
                                block_stride=desc["H"] * (2 * gh - 1) * (2 * gw - 1) if per else 0)
        W["blocks"] = blocks
        self._weights, self._weights_key = W, key
        self._weights_sig, self._weights_cfg = sig, cfg_key
        self._drop_plans()
        return W

    def _build_plan(self, B: int, S: int, device, dtype, mode: str = "logits"):
        """`mode`: "logits" (the model's forward: logits, or the pooled feature of a headless model), or the feature outputs
        "tokens" / "dense" / "dense_last" (forward_features): a second plan of the same packed weights with no head and
        ext.pool = POOL_NONE / POOL_DENSE / POOL_DENSE_LAST.  A tuple ("layers", base mode, captured blocks, norm, fill)
        (forward_intermediates) is the base mode's plan with a layers record beside it, under a key of its own.
        `S` is the side of a square input or, under dynamic_img_size, (H, W) of a rectangular one: the plan then carries an image
        record (rajni_vit_image) and runs through rajni_vit_forward_image."""
        W = self._pack_weights(device, dtype)
        d = W["desc"]
        P = d["num_prefix"]
        has_cls, query = d["class_token"], self.importance_query
        if query == "cls" and not has_cls:      # (the class token was removed after the setter)
            raise ValueError('importance query "cls" on a model without a class token; set_importance_query("mean")')
        full_mode, layers = mode, None
        if isinstance(mode, tuple):
            _, mode, caps, lnorm, lfill = mode
            self._check_layers(d, caps, lnorm)
        features = mode != "logits"
        if features:
            self._check_features(d)
        key = (B, S, device, dtype, self._weights_key, tuple(sorted(self._forced)), self._trace_scores, self._resid_bf16,
               self._cls_only_last) + ((query, has_cls) if (query, has_cls) != ("cls", True) else ()) + (P, full_mode)
        if self._plan is not None and self._plan.key == key:
            return self._plan
        if key in self._plans:
            self._plan = self._plans[key]
            return self._plan
        # S: the side of a square input, or (H, W) of a rectangular one (dynamic_img_size only)
        Hh, Wd = (S, S) if isinstance(S, int) else S
        if Hh % d["patch"] != 0 or Wd % d["patch"] != 0:
            raise ValueError(f"image size {S} is not a multiple of the patch size {d['patch']}")
        gh, gw = Hh // d["patch"], Wd // d["patch"]
        n0 = gh * gw + P
        pos = W["pos"]
        pos_rows = pos.shape[0] if pos is not None else 0
        if pos is None:
            # no absolute embedding: a zero table of the grid's patch rows (cached like the resampled embeddings), which the
            # patch GEMM adds as it adds any other - no kernel knows the difference
            cache = W.setdefault("pos_cache", {})
            zkey = ("zero", gh * gw, device, dtype)
            if zkey not in cache:
                if len(cache) >= 8:
                    cache.pop(next(iter(cache)))
                cache[zkey] = torch.zeros((gh * gw, d["C"]), dtype=dtype, device=device)
            pos, pos_has_cls = cache[zkey], 0
        elif self._dynamic_img_size:
            if getattr(self.m, "dynamic_img_pad", False) or getattr(self.m.patch_embed, "dynamic_img_pad", False):
                raise NotImplementedError("RAJNIViTWrapper: dynamic_img_pad (padding images to a multiple of the patch size) is "
                                          "not supported")
            pos, pos_has_cls = self._pos_for_grid(W, gh, gw, P, device, dtype)
        elif pos_rows == n0 or (P == 1 and has_cls and pos_rows > n0):
            pos_has_cls = 1      # reference: x + pos_embed[:, :N]  (model.py:37); timm: a row for every prefix token too
        elif pos_rows == n0 - P:
            pos_has_cls = 0      # timm no_embed_class: the prefix rows get no pos-embed
        else:
            raise ValueError(f"pos_embed has {pos_rows} rows but the input yields {n0} tokens ({P} of them prefix tokens); "
                             "set_dynamic_img_size(True) resamples the embedding to the input's grid")
        counts = plan_token_counts(n0, d["depth"], self.pruning_schedule, P)

        blocks = (nat.Block * d["depth"])()
        bufs: Dict[int, Dict[str, Optional[torch.Tensor]]] = {}
        for i, bw in enumerate(W["blocks"]):
            cb = blocks[i]
            for name in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_w", "norm2_b",
                         "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2", "qkv_s", "proj_s", "fc1_s", "fc2_s"):
                setattr(cb, name, nat.ptr(bw[name]))
            if self._weight_format == "fp8_mfma":
                cb.fc1_rownorm_max, cb.fc1_bias_absmax = bw["fc1_rownorm_max"], bw["fc1_bias_absmax"]
                cb.attn_out_scale = bw["attn_out_scale"]
            if i in self.pruning_schedule:
                cfg = self.pruning_schedule[i]
                N = counts[i]
                keep = ops.keep_count(cfg["keep_ratio"], N, P)
                if keep > N - P:
                    raise ValueError(f"block {i}: keep_ratio {cfg['keep_ratio']} > 1 selects more tokens than exist")
                kb = dict(keep_idx=torch.empty((B, keep + P), dtype=torch.int32, device=device),
                          next_scores=torch.empty((B, keep + P), dtype=dtype, device=device),
                          scores=torch.empty((B, N), dtype=dtype, device=device) if self._trace_scores else None)
                bufs[i] = kb
                cb.keep, cb.update = keep, int(cfg["update"])
                cb.keep_idx, cb.next_scores, cb.scores = kb["keep_idx"].data_ptr(), kb["next_scores"].data_ptr(), \
                    nat.ptr(kb["scores"])
                if i in self._forced:
                    f = self._forced[i].to(device)
                    if tuple(f.shape) != (B, keep + P):
                        raise ValueError(f"forced keep_idx for block {i} has shape {tuple(f.shape)}, want {(B, keep + P)}")
                    if (P > 1 or not has_cls) and not bool((f[:, :P].cpu() == torch.arange(P, dtype=torch.int32)).all()):
                        raise ValueError(f"forced keep_idx for block {i}: slots 0..{P - 1} must hold the prefix tokens 0..{P - 1}")
                    self._forced[i] = f
                    cb.forced_keep_idx = f.data_ptr()
            else:
                cb.keep = 0

        plan = nat.VitPlan()
        plan.dtype = nat.dtype_code(dtype)
        plan.B, plan.in_chans, plan.img_size, plan.patch_size = B, d["in_chans"], Hh, d["patch"]
        plan.C, plan.H, plan.D, plan.depth, plan.hidden = d["C"], d["H"], d["D"], d["depth"], d["hidden_pad"]
        headless = features or d["headless"]
        plan.num_classes, plan.ln_eps, plan.attn_scale = 0 if headless else d["num_classes"], d["ln_eps"], d["scale"]
        plan.pos_has_cls = pos_has_cls
        plan.patch_w, plan.patch_b = W["patch_w"].data_ptr(), W["patch_b"].data_ptr()
        plan.cls_token, plan.pos_embed = nat.ptr(W["cls"]), pos.data_ptr()
        plan.blocks = blocks
        plan.norm_w, plan.norm_b = nat.ptr(W["norm_w"]), nat.ptr(W["norm_b"])
        plan.head_w, plan.head_b = (None, None) if headless else (W["head_w"].data_ptr(), W["head_b"].data_ptr())
        tc = (C.c_int32 * d["depth"])()
        plan.token_counts = tc
        # (a headless plan's output rows are the C elements the final norm writes, dense)
        plan.logits_ld = d["C"] if headless else (d["num_classes"] + 7) // 8 * 8
        plan.resid_bf16 = int(self._resid_bf16)
        plan.cls_only_last_block = int(self._cls_only_last)
        plan.act_fp8 = int(self._weight_format == "fp8_mfma")
        pre = qry = None
        if (query, has_cls) != ("cls", True):   # the query record beside the plan (rajni_vit_query); None: the entry points as ever
            qry = nat.VitQuery(int(has_cls), ops.query_code(query))
        if not has_cls:     # no class row: the record counts the registers alone (R = 0: no record)
            if P > 0:
                pre = nat.VitPrefix()
                pre.num_prefix, pre.reg_token, pre.head_rows = P, W["reg"].data_ptr(), 0
        elif P > 1:         # the prefix record beside the plan (rajni_vit_prefix); None: CLS only, the entry points as ever
            pre = nat.VitPrefix()
            pre.num_prefix, pre.reg_token = P, W["reg"].data_ptr()
            # (register models: the record as it always was; the feature plan of a distilled model reads no head rows)
            pre.head_rows = 2 if d["head_rows"] == 2 and not features else 0
        img = None
        if Hh != Wd:        # the image record beside the plan (rajni_vit_image); None: a square input, the entry points as ever
            img = nat.VitImage(Hh, Wd)
        apr = None
        if d["pool"] == "map" and not features:   # the attention-pool record beside the plan (rajni_vit_attn_pool); the feature
            pw_, pd = W["attn_pool"], d["attn_pool"]   # outputs end at norm(x), in front of the pool, and carry none
            apr = nat.VitAttnPool()
            for name in ("q", "kv_w", "kv_b", "proj_w", "proj_b", "norm_w", "norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
                setattr(apr, name, nat.ptr(pw_[name]))
            apr.norm_eps, apr.hidden, apr.heads = pd["eps"], pd["hidden_pad"], pd["heads"]
            apr.act = nat.MLP_QUICK_GELU if pd["act"] == "quick_gelu" else nat.MLP_GELU
        nrm = None
        if d["norm_record"]:      # the norm record beside the plan (rajni_vit_norm); None: LayerNorm everywhere, the entry points as ever
            nrm = nat.VitNorm()
            nrm.kind = nat.NORM_RMS if d["norm_kind"] == "rms" else nat.NORM_LAYERNORM
            if d["embed_norm"]:
                nrm.embed_norm_w, nrm.embed_norm_b = nat.ptr(W["embed_norm_w"]), nat.ptr(W["embed_norm_b"])
                nrm.embed_norm_eps = d["embed_norm_eps"]
        rop = rot = None
        if d["rope"]:             # the rope record beside the plan (rajni_vit_rope); None: no rotation, the entry points as ever
            rot = cos, sin = self._rope_for_grid(W, gh, gw, device)
            rop = nat.VitRope()
            rop.cos, rop.sin, rop.rows = cos.data_ptr(), sin.data_ptr(), gh * gw
            rop.head_stride = gh * gw * d["D"] if d["rope"] != "shared" else 0
            rop.block_stride = d["H"] * gh * gw * d["D"] if d["rope"] == "per_block" else 0
            rop.layout = nat.ROPE_HALF if d["rope_half"] else nat.ROPE_INTERLEAVED
        mln = None
        if d["mlp_norm"]:         # the mlp-norm record beside the plan (rajni_vit_mlp_norm); None: the entry points as ever
            rec = nat.VitMlpNorm()
            mw = (C.c_void_p * d["depth"])(*[bw["mlp_norm_w"].data_ptr() for bw in W["blocks"]])
            mb = (C.c_void_p * d["depth"])(*[nat.ptr(bw["mlp_norm_b"]) for bw in W["blocks"]])
            rec.w, rec.b, rec.eps, rec.n = mw, mb, d["mlp_norm_eps"], d["hidden"]
            mln = (rec, mw, mb)
        mrec = mln[0] if mln else None
        rel = None
        if d["rel_pos"]:          # the relpos record beside the plan (rajni_vit_relpos); None: no bias, the entry points as ever
            if (gh, gw) != d["rel_pos_grid"]:
                raise ValueError(f"the model's relative position bias is stated on a {d['rel_pos_grid'][0]} x {d['rel_pos_grid'][1]} "
                                 f"grid but the input yields {gh} x {gw} patches (the table is resized when a checkpoint is "
                                 "loaded, not per input)")
            rp = W["rel_pos"]
            rel = nat.VitRelPos()
            rel.table, rel.prefix_q, rel.prefix_k, rel.prefix_qk = (rp[k].data_ptr() for k in ("table", "prefix_q", "prefix_k", "prefix_qk"))
            rel.block_stride, rel.gh, rel.gw = rp["block_stride"], gh, gw
        symbol, records = _native_call(_SIZES, pre, img, qry, apr, nrm, rop, mrec, rel)
        nbytes = getattr(nat.lib(), symbol)(C.byref(plan), *records)
        if nbytes == 0 and symbol not in _SIZES[:2]:
            # the image, query, pool, norm, rope or mlp-norm record is refused: say why (the forward's own refusal; nothing is launched)
            dry = nat.VitExt(pool=nat.POOL_MAP) if apr is not None else None
            forward, records = _native_call(_FORWARDS, dry, pre, None, img, qry, apr, nrm, rop, mrec, rel)
            nat.check(getattr(nat.lib(), forward)(C.byref(plan), *records, 16, 16, None), forward)
            raise nat.NativeError(f"{symbol} refused the plan")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        plan.workspace, plan.workspace_bytes = ws.data_ptr(), nbytes
        ext = qk = None
        if d["ext"] or features:        # the options beside the plan (rajni_vit_ext); None: the plain rajni_vit_forward
            if d["pool"] == "avg" and self._cls_only_last:
                raise ValueError("global_pool='avg' with set_last_block_cls_only(True): that opt-in never forms the rows to be averaged")
            ext = nat.VitExt()
            if d["qk_norm"]:
                qk = (nat.QkAffine * d["depth"])()
                for i, bw in enumerate(W["blocks"]):
                    for name in ("q_norm_w", "q_norm_b", "k_norm_w", "k_norm_b"):
                        setattr(qk[i], name, nat.ptr(bw[name]))
                ext.qk_norm, ext.qk_eps = qk, d["qk_eps"]
            ext.norm_pre_w, ext.norm_pre_b, ext.norm_pre_eps = nat.ptr(W["norm_pre_w"]), nat.ptr(W["norm_pre_b"]), W["norm_pre_eps"]
            ext.fc_norm_w, ext.fc_norm_b, ext.fc_norm_eps = nat.ptr(W["fc_norm_w"]), nat.ptr(W["fc_norm_b"]), W["fc_norm_eps"]
            ext.norm_absent = int(not d["norm"])
            ext.pool = {"avg": nat.POOL_AVG, "map": nat.POOL_MAP}.get(d["pool"], nat.POOL_TOKEN)
            if features:      # timm forward_features ends at norm(x): no pool, no fc_norm
                ext.pool = {"tokens": nat.POOL_NONE, "dense": nat.POOL_DENSE, "dense_last": nat.POOL_DENSE_LAST}[mode]
                ext.fc_norm_w = ext.fc_norm_b = None
            ext.mlp_act = {"quick_gelu": nat.MLP_QUICK_GELU, "swiglu": nat.MLP_SWIGLU}.get(d["mlp_act"], nat.MLP_GELU)
        # what `logits` receives: [B, logits_ld], or the tokens behind the last block / the unpruned sequence's rows
        n_last = counts[-1] if (d["depth"] - 1) not in self.pruning_schedule else \
            ops.keep_count(self.pruning_schedule[d["depth"] - 1]["keep_ratio"], counts[-1], P) + P
        out_shape = {"logits": (B, plan.logits_ld), "tokens": (B, n_last, d["C"]), "dense": (B, n0, d["C"]),
                     "dense_last": (B, n0, d["C"])}[mode]
        if full_mode is not mode:      # the layers record (rajni_vit_layers) minus `out`, and the slabs' shape
            cap_arr = (C.c_int * len(caps))(*caps)
            layers = (cap_arr, int(lnorm), int(lfill == "last"), (len(caps), B, n0, d["C"]))
        self._plan = PlanEntry(key, plan, PlanRefs(blocks, tc, ws, W, ext, qk, pre), bufs, counts, full_mode, out_shape, layers,
                               PlanInput(img, pos, gh, gw, qry, apr, nrm, rop, rot, mln, rel))
        if len(self._plans) >= 4:     # workspaces are large: keep only a few batch shapes alive
            self._plans.pop(next(iter(self._plans)))
        self._plans[key] = self._plan
        return self._plan

    # ------------------------------------------------------------------------------------------
    def _check_features(self, d):
        """what forward_features does not compute"""
        if not d["norm"]:
            raise NotImplementedError("forward_features: base_model.norm is nn.Identity (the fc_norm models): their features are "
                                      "the un-normalised stream, which forward_intermediates(x, norm=False, "
                                      "intermediates_only=True) returns")
        if self._weight_format == "fp8_mfma":
            raise NotImplementedError('forward_features: not supported with weight format "fp8_mfma" ("fp8" weights work)')
        if self._cls_only_last:
            raise ValueError("forward_features with set_last_block_cls_only(True): that opt-in never forms the rows to be returned")

    def _check_layers(self, d, caps, norm):
        """what forward_intermediates does not compute"""
        if norm and self._norm_feature_or_none() == "RMSNorm":
            raise NotImplementedError("forward_intermediates(norm=True): the model's norms are RMSNorm and the normalised slabs "
                                      "are LayerNorm only; norm=False returns the un-normalised states")
        if norm and not d["norm"]:
            raise NotImplementedError("forward_intermediates(norm=True): base_model.norm is nn.Identity (the fc_norm models); "
                                      "norm=False returns the un-normalised states")
        if self._weight_format == "fp8_mfma":
            raise NotImplementedError('forward_intermediates: not supported with weight format "fp8_mfma" ("fp8" weights work)')
        if self._cls_only_last and caps[-1] == d["depth"] - 1:
            raise ValueError("forward_intermediates with set_last_block_cls_only(True) and the last block captured: that opt-in "
                             "never forms the rows to be returned")

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """logits [B, num_classes]; on a headless model (head = nn.Identity, timm num_classes=0) the pooled feature [B, C],
        fc_norm(pool(norm(x))) on the pruned token set - timm's forward of such a model"""
        out, entry = self._run(x, "logits")
        plan = entry.plan
        if plan.num_classes == 0:
            return out
        return out[:, : plan.num_classes] if plan.logits_ld != plan.num_classes else out

    @torch.no_grad()
    def forward_features(self, x: torch.Tensor, dense: bool = False, fill: str = "zero") -> torch.Tensor:
        """timm's forward_features on the pruned graph, norm(x), for every model the wrapper supports (with or without a head):
        `dense=False`: [B, Nf, C], the tokens that survive the last block, in stream order;
        `dense=True`:  [B, P + n, C], the unpruned sequence's shape - every surviving token at the position it came from, pruned
                       positions zero;
        `dense=True, fill="last"`: the same, but a token that scheduled block i drops keeps the feature it had when it left:
                       its position holds norm(x_entry_i), the final norm of the residual stream at the entry of block i (as
                       DINOv2's get_intermediate_layers(norm=True) normalises intermediate states).  No row is zero.
        Afterwards `get_last_stats()["source_idx"]` is an int32 device tensor [B, Nf]: the position in the unpruned sequence of
        each surviving row (slots 0..P-1 are the prefix tokens 0..P-1, the rest strictly ascending), in every mode; with
        `fill="last"` there is `"exit_block"` too, int32 [B, P + n] on the device: the scheduled block that dropped the token of
        each position, `depth` for the survivors."""
        if fill not in ("zero", "last"):
            raise ValueError(f'forward_features: fill must be "zero" or "last", got {fill!r}')
        if fill == "last" and not dense:
            raise ValueError('forward_features: fill="last" fills the pruned positions of the dense output; it needs dense=True')
        out, entry = self._run(x, ("dense_last" if fill == "last" else "dense") if dense else "tokens")
        self._selection_stats(entry, x, exit_block=fill == "last")
        return out

    def _selection_stats(self, entry, x, exit_block: bool):
        """`source_idx` (and `exit_block`) of the forward just run into get_last_stats(): torch ops on the device, no host sync"""
        n0 = entry.counts[0]
        src = None            # the selections composed on the device, last stage first: no host sync
        for i in sorted(entry.bufs, reverse=True):
            idx = self._forced.get(i, entry.bufs[i]["keep_idx"]).long()
            src = idx if src is None else torch.gather(idx, 1, src)
        if src is None:
            src = torch.arange(n0, device=x.device).expand(x.shape[0], n0)
        self._last_stats["source_idx"] = src.to(torch.int32).contiguous()
        if exit_block:
            self._last_stats["exit_block"] = compose_exit_block(
                {i: self._forced.get(i, entry.bufs[i]["keep_idx"]) for i in entry.bufs}, x.shape[0], n0, entry.plan.depth, x.device)

    @torch.no_grad()
    def forward_intermediates(self, x: torch.Tensor, indices=None, return_prefix_tokens: bool = False, norm: bool = False,
                              stop_early: bool = False, output_fmt: str = "NCHW", intermediates_only: bool = False,
                              fill: str = "zero"):
        """timm's forward_intermediates on the pruned graph - its signature and defaults, plus `fill` - from ONE forward: the
        state behind every block of `indices` (take_indices: None = every block, an int k = the last k, a sequence = those
        blocks), each scattered back to the unpruned sequence like forward_features(dense=True).
        A token alive behind captured block c has f(x_after_c) at its position; a token that scheduled block i <= c dropped has
        zeros (`fill="zero"`) or f(x_entry_i), the state it had when it left (`fill="last"`).  f is base_model.norm with
        `norm=True` (DINOv2 normalises intermediate states with the final norm) and one rounding of the stream to the model
        dtype with `norm=False` (timm's default).  A block that is both scheduled and captured drops first.
        Returns `(final, intermediates)`, `final` = forward_features(x, dense=True, fill=fill) from the same call, or with
        `intermediates_only=True` the list alone (then the forward is the logits plan's, and models without a final norm work
        with norm=False).  Each intermediate is the patch rows of its slab: "NLC" [B, n, C], a view into one allocation, or
        "NCHW" [B, C, h, w], a torch permute made contiguous - a copy; with `return_prefix_tokens=True` a pair (spatial,
        prefix [B, P, C]).
        Afterwards get_last_stats() holds `source_idx` and `exit_block` (both fills): the alive mask of the intermediate of
        block c is `exit_block > c`.  `stop_early=True` is not implemented (the forward always runs every block)."""
        if fill not in ("zero", "last"):
            raise ValueError(f'forward_intermediates: fill must be "zero" or "last", got {fill!r}')
        if output_fmt not in ("NCHW", "NLC"):
            raise ValueError(f'forward_intermediates: output_fmt must be "NCHW" or "NLC", got {output_fmt!r}')
        if stop_early:
            raise NotImplementedError("forward_intermediates(stop_early=True): the native forward runs every block; cut the base "
                                      "model's blocks instead")
        caps = take_indices(len(self.blocks), indices)
        self._check_layers(dict(norm=not isinstance(self.m.norm, nn.Identity), depth=len(self.blocks)), caps, norm)
        base = "logits" if intermediates_only else ("dense_last" if fill == "last" else "dense")
        (final, slabs), entry = self._run(x, ("layers", base, caps, bool(norm), fill))
        self._selection_stats(entry, x, exit_block=True)
        P = entry.key[-2]
        B, gh, gw, Cdim = x.shape[0], entry.input.gh, entry.input.gw, entry.plan.C
        inter = []
        for l in range(len(caps)):
            spatial = slabs[l, :, P:]
            if output_fmt == "NCHW":
                spatial = spatial.reshape(B, gh, gw, Cdim).permute(0, 3, 1, 2).contiguous()
            inter.append((spatial, slabs[l, :, :P]) if return_prefix_tokens else spatial)
        return inter if intermediates_only else (final, inter)

    @torch.no_grad()
    def get_intermediate_layers(self, x: torch.Tensor, n=1, reshape: bool = False, return_class_token: bool = False,
                                norm: bool = True, fill: str = "zero"):
        """DINOv2's get_intermediate_layers on the pruned graph (its signature and tuple return, plus `fill`): the patch tokens
        behind the last `n` blocks (or the blocks of a sequence `n`), through the final norm by default, [B, n, C] each or with
        `reshape=True` [B, C, h, w]; `return_class_token=True` gives (patches, class_token [B, C]) pairs.  A thin layer over
        forward_intermediates."""
        inter = self.forward_intermediates(x, indices=n, return_prefix_tokens=True, norm=norm,
                                           output_fmt="NCHW" if reshape else "NLC", intermediates_only=True, fill=fill)
        if return_class_token:
            return tuple((spatial, prefix[:, 0]) for spatial, prefix in inter)
        return tuple(spatial for spatial, _ in inter)

    @property
    def dynamic_img_size(self) -> bool:
        return self._dynamic_img_size

    def _check_input_shape(self, x: torch.Tensor):
        if x.dim() == 4 and x.shape[-1] != x.shape[-2] and not self._dynamic_img_size and model_has_rel_pos(self.m, self.blocks):
            return      # a rectangular fixed grid: _build_plan holds the input to the grid the model's bias is stated on
        if x.dim() != 4 or (x.shape[-1] != x.shape[-2] and not self._dynamic_img_size):
            raise ValueError(f"expected images [B, C, S, S], got {tuple(x.shape)}"
                             + ("" if x.dim() != 4 else "; set_dynamic_img_size(True) takes [B, C, H, W]"))

    def _run(self, x: torch.Tensor, mode: str):
        nat.require_device(x, "input images")
        self._check_input_shape(x)
        anchor = self.m.cls_token if model_has_class_token(self.m) else self.m.pos_embed   # a parameter every model has ...
        if anchor is None:                                                                  # ... but one with rotary positions alone
            anchor = self.m.patch_embed.proj.weight
        dtype = anchor.dtype
        if self._resid_bf16 and dtype in (torch.bfloat16, torch.float16) and self._resid_dtype != dtype:
            raise ValueError(f"a {self._resid_dtype} residual stream needs a {self._resid_dtype} model (the model is {dtype}); "
                             f"the 16-bit stream is kept in the model dtype")
        if anchor.device != x.device:
            raise nat.NativeError(f"model is on {anchor.device} but images are on {x.device}")
        if x.dtype != dtype:
            x = x.to(dtype)
        x = x.contiguous()
        # (a square input keeps the key it always had; a rectangle carries (H, W) where that had S)
        B, S = x.shape[0], (x.shape[-1] if x.shape[-1] == x.shape[-2] else (x.shape[-2], x.shape[-1]))
        with nat.device_guard(x.device):
            def launch(entry):
                out = torch.empty(entry.out_shape, dtype=dtype, device=x.device)
                lay = slabs = None
                if entry.layers is not None:      # forward_intermediates: the slabs beside `out`, one allocation
                    cap_arr, lnorm, lfill, slab_shape = entry.layers
                    slabs = torch.empty(slab_shape, dtype=dtype, device=x.device)
                    lay = nat.VitLayers()
                    lay.n, lay.blocks, lay.norm, lay.fill, lay.out, lay.slab_stride = len(cap_arr), cap_arr, lnorm, lfill, slabs.data_ptr(), 0
                symbol, records = _native_call(_FORWARDS, entry.refs.ext, entry.refs.pre, lay, entry.input.img, entry.input.qry,
                                               entry.input.apr, entry.input.nrm, entry.input.rop,
                                               entry.input.mln[0] if entry.input.mln else None, entry.input.rel)
                nat.check(getattr(nat.lib(), symbol)(C.byref(entry.plan), *records, x.data_ptr(), out.data_ptr(),
                                                     nat.stream_ptr(x.device)), symbol)
                return out if lay is None else (out, slabs)
            # Optimistic launch: with a plan of this batch shape at hand the kernels are enqueued FIRST and the check
            # that the base model's weights are still the packed ones (a walk over ~150 parameters, ~0.1 ms of Python)
            # runs while the GPU works - in the sync -> forward -> sync metric of evaluate_model that check would
            # otherwise sit in front of every forward.  Packed weights are copies, so a launch on a stale plan reads
            # consistent (old) data; if the check finds a change the forward is simply enqueued again on the new plan
            # and the first result is dropped.  Option setters drop `_plan`, so they always take the slow path.
            # ONE STREAM PER WRAPPER: the stale launch's workspace and packed weights stay referenced by `cached` until
            # this function returns and are handed back to the allocator in stream order - a second stream driving the
            # same wrapper concurrently is not supported (the reference is one-forward-at-a-time too).
            cached = self._plan
            # (the mode is the key's last element: a logits plan must not be launched into a feature buffer)
            if cached is not None and cached.key[:4] == (B, S, x.device, dtype) and cached.key[-1] == mode:
                logits = launch(cached)
                entry = self._build_plan(B, S, x.device, dtype, mode)
                if entry is not cached:
                    logits = launch(entry)
            else:
                entry = self._build_plan(B, S, x.device, dtype, mode)
                logits = launch(entry)
        plan, tc = entry.plan, entry.refs.tc
        self._last_stats = {"token_counts": [int(tc[i]) for i in range(plan.depth)]}   # model.py:68
        return logits, entry
