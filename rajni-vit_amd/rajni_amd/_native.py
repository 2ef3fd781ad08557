"""ctypes binding of librajni_hip.so (C ABI: include/rajni_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every kernel is ours.  There is NO
fallback: if the library is missing or the tensors are not on a ROCm device the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAJNI_HIP_LIB") or os.path.join(_HERE, "lib", "librajni_hip.so")

RAJNI_F32, RAJNI_BF16, RAJNI_F16 = 0, 1, 2
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID = 0, 1, 2
EPI_BIAS_QUICK_GELU = 16      # y = quick_gelu(x W^T + b); not with fp8 activations (x_scale)
EPI_BIAS_SWIGLU = 18          # y [M, N] = silu(x Wg^T + bg) * (x Wv^T + bv), w [2N, K] gate rows then value rows; not with x_scale
NUM_KCLASS = 17
POOL_TOKEN, POOL_AVG = 0, 1
POOL_NONE, POOL_DENSE = 2, 3         # headless plans only: every surviving token [B, Nf, C] / scattered back to [B, P + n, C]
POOL_DENSE_LAST = 5                  # ... scattered back, pruned positions holding the token's state at the block that dropped it; 4 is unknown
MLP_GELU, MLP_QUICK_GELU = 0, 1      # rajni_vit_ext.mlp_act
MLP_SWIGLU = 3                       # ... the gated FC1 (fc1_w [2 * hidden, C]); 2 is an unknown value

c_void_p, c_int, c_long, c_float, c_size_t = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_size_t


class NativeError(RuntimeError):
    pass


class LinearArgs(C.Structure):
    _fields_ = [("x", c_void_p), ("lda", c_long), ("w", c_void_p), ("ldw", c_long),
                ("bias", c_void_p), ("gamma", c_void_p), ("resid", c_void_p), ("ldr", c_long),
                ("r_idx", c_void_p), ("r_np", c_int), ("r_nsrc", c_int),
                ("y", c_void_p), ("ldc", c_long), ("M", c_int), ("N", c_int), ("K", c_int),
                ("epilogue", c_int), ("dtype", c_int), ("stream_f32", c_int), ("w_scale", c_void_p),
                ("x_scale", c_void_p), ("y_scale", c_void_p)]


class LinearPlan(C.Structure):
    """rajni_linear_plan (include/rajni_hip_debug.h): what rajni_debug_linear_plan says a linear call would launch"""
    _fields_ = [("tiling", c_int), ("tiles_n", c_int), ("total_tiles", c_int), ("nblk", c_int), ("grid", c_int),
                ("lds_bytes", c_int)]


TILING_SMALL, TILING_F32, TILING_WIDE, TILING_MID, TILING_F8_STREAM, TILING_F8_WIDE = 1, 2, 4, 5, 8, 9


class Block(C.Structure):
    _fields_ = [("norm1_w", c_void_p), ("norm1_b", c_void_p),
                ("qkv_w", c_void_p), ("qkv_b", c_void_p),
                ("proj_w", c_void_p), ("proj_b", c_void_p), ("ls1", c_void_p),
                ("norm2_w", c_void_p), ("norm2_b", c_void_p),
                ("fc1_w", c_void_p), ("fc1_b", c_void_p),
                ("fc2_w", c_void_p), ("fc2_b", c_void_p), ("ls2", c_void_p),
                ("keep", c_int), ("update", c_int),
                ("keep_idx", c_void_p), ("scores", c_void_p), ("next_scores", c_void_p),
                ("forced_keep_idx", c_void_p),
                ("qkv_s", c_void_p), ("proj_s", c_void_p), ("fc1_s", c_void_p), ("fc2_s", c_void_p),
                ("fc1_rownorm_max", c_float), ("fc1_bias_absmax", c_float), ("attn_out_scale", c_float)]


class VitPlan(C.Structure):
    _fields_ = [("dtype", c_int), ("B", c_int), ("in_chans", c_int), ("img_size", c_int),
                ("patch_size", c_int), ("C", c_int), ("H", c_int), ("D", c_int), ("depth", c_int),
                ("hidden", c_int), ("num_classes", c_int), ("ln_eps", c_float),
                ("attn_scale", c_float), ("pos_has_cls", c_int),
                ("patch_w", c_void_p), ("patch_b", c_void_p), ("cls_token", c_void_p),
                ("pos_embed", c_void_p), ("blocks", C.POINTER(Block)),
                ("norm_w", c_void_p), ("norm_b", c_void_p), ("head_w", c_void_p), ("head_b", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("token_counts", C.POINTER(C.c_int32)), ("logits_ld", c_int), ("cls_only_last_block", c_int),
                ("resid_bf16", c_int), ("act_fp8", c_int)]


class QkAffine(C.Structure):
    _fields_ = [("q_norm_w", c_void_p), ("q_norm_b", c_void_p), ("k_norm_w", c_void_p), ("k_norm_b", c_void_p)]


class VitExt(C.Structure):
    """rajni_vit_ext: the timm options beside the plan (q/k-norm, norm_pre, pooled head, fc_norm, the MLP activation); all
    zero = none.  `mlp_act` fills what was the record's tail padding: offset 68, size 72 as before."""
    _fields_ = [("qk_norm", C.POINTER(QkAffine)), ("qk_eps", c_float),
                ("norm_pre_w", c_void_p), ("norm_pre_b", c_void_p), ("norm_pre_eps", c_float),
                ("norm_absent", c_int), ("pool", c_int),
                ("fc_norm_w", c_void_p), ("fc_norm_b", c_void_p), ("fc_norm_eps", c_float),
                ("mlp_act", c_int)]


class VitPrefix(C.Structure):
    """rajni_vit_prefix: prefix tokens beyond CLS (timm register tokens, or DeiT's distillation token), beside the plan and
    the ext record.  `head_rows` (2: the distilled head reads rows 0 and 1) fills what was the padding behind num_prefix:
    offset 4, size 16 as before.  Positional construction stays (num_prefix, reg_token)."""
    _fields_ = [("num_prefix", c_int), ("head_rows", c_int), ("reg_token", c_void_p)]

    def __init__(self, num_prefix=0, reg_token=None, head_rows=0):
        super().__init__(num_prefix=num_prefix, head_rows=head_rows, reg_token=reg_token)


class VitLayers(C.Structure):
    """rajni_vit_layers (include/rajni_hip_layers.h): the blocks whose output rajni_vit_forward_layers scatters back to the
    unpruned sequence, one slab [B, P + n, C] each.  `blocks` is a HOST int array the caller keeps alive."""
    _fields_ = [("n", c_int), ("blocks", C.POINTER(c_int)), ("norm", c_int), ("fill", c_int), ("out", c_void_p),
                ("slab_stride", C.c_longlong)]


class VitImage(C.Structure):
    """rajni_vit_image (include/rajni_hip_image.h): the input's height and width in pixels, beside the plan"""
    _fields_ = [("height", c_int), ("width", c_int)]


class VitQuery(C.Structure):
    """rajni_vit_query (include/rajni_hip_query.h): whether the sequence has a class row, and the importance query"""
    _fields_ = [("class_token", c_int), ("query", c_int)]


QUERY_CLS, QUERY_MEAN = 0, 1     # RAJNI_QUERY_CLS, RAJNI_QUERY_MEAN
MAX_LAYERS = 64     # RAJNI_MAX_LAYERS
MAX_PREFIX = 32     # RAJNI_MAX_PREFIX
SCORE_TILE_TOKENS = 32      # ST_TILE of csrc/score_select.hip: tokens per workgroup of the tiled score kernels
SCORE_TILED_MAX_TOKENS = 16384 + MAX_PREFIX   # ST_MAX_N: the tiled path's cap

_SIGS = {
    "rajni_abi_version": (c_int, []),
    "rajni_last_error": (C.c_char_p, []),
    "rajni_device_check": (c_int, []),
    "rajni_importance": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "rajni_select_topk": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "rajni_score_select": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                   c_void_p, c_int, c_void_p]),
    "rajni_gather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rajni_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                c_int, c_void_p]),
    "rajni_attention_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                    c_void_p]),
    "rajni_layernorm": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                                c_int, c_int, c_void_p]),
    "rajni_layernorm_fp8": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                    c_int, c_int, c_float, c_int, c_void_p]),
    "rajni_linear": (c_int, [C.POINTER(LinearArgs), c_void_p]),
    "rajni_qk_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "rajni_layernorm_stream": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_int, c_void_p]),
    "rajni_pool_norm": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_float,
                                c_void_p, c_int, c_int, c_void_p]),
    "rajni_debug_force_gemm_tiling": (None, [c_int]),
    "rajni_debug_force_f8_tiling": (None, [c_int]),
    "rajni_debug_set_resid_stagger": (None, [c_int]),
    "rajni_debug_set_gemm_nblock_bytes": (None, [c_int]),
    "rajni_debug_set_persistent_workgroups": (None, [c_int]),
    "rajni_debug_linear_plan": (c_int, [C.POINTER(LinearArgs), c_int, C.POINTER(LinearPlan)]),
    "rajni_debug_force_attention": (None, [c_int]),
    "rajni_debug_attention_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                           c_int, c_void_p]),
    "rajni_debug_set_last_block_all_rows": (None, [c_int]),
    "rajni_debug_last_block_cls_rows": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix)]),
    "rajni_debug_force_score_two_pass": (None, [c_int]),
    "rajni_debug_force_score_tiled": (None, [c_int]),
    "rajni_debug_set_gemm_stamps": (None, [c_void_p]),
    "rajni_patch_embed_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "rajni_patch_embed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                  c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_vit_workspace_bytes": (c_size_t, [C.POINTER(VitPlan)]),
    "rajni_vit_forward": (c_int, [C.POINTER(VitPlan), c_void_p, c_void_p, c_void_p]),
    "rajni_vit_forward_ext": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), c_void_p, c_void_p, c_void_p]),
    "rajni_select_topk_prefix": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "rajni_score_select_prefix": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_int, c_void_p]),
    "rajni_score_select_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "rajni_score_select_ws": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_patch_embed_prefix": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                         c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_pool_norm_prefix": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                       c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    "rajni_vit_workspace_bytes_prefix": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix)]),
    "rajni_vit_forward_ext_prefix": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), c_void_p, c_void_p,
                                             c_void_p]),
    "rajni_profile_enable": (None, [C.c_uint]),
    "rajni_profile_class_name": (C.c_char_p, [c_int]),
    "rajni_profile_collect": (c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]),
    "rajni_profile_reset": (None, []),
}

EXPORTED_SYMBOLS = tuple(_SIGS.keys())
# include/rajni_hip_layers.h, additive to the boundary above: bound beside it, EXPORTED_SYMBOLS and the ABI version stay
_LAYERS_SIGS = {
    "rajni_vit_forward_layers": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                         c_void_p, c_void_p, c_void_p]),
}
LAYERS_SYMBOLS = ("rajni_vit_forward_layers",)
# include/rajni_hip_image.h, additive in the same way: rectangular images and the position-embedding resample
_IMAGE_SIGS = {
    "rajni_resample_pos_embed": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rajni_patch_embed_image": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_patch_embed_workspace_bytes_image": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "rajni_vit_workspace_bytes_image": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage)]),
    "rajni_vit_forward_image": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                        C.POINTER(VitImage), c_void_p, c_void_p, c_void_p]),
}
IMAGE_SYMBOLS = tuple(_IMAGE_SIGS.keys())
# include/rajni_hip_query.h, additive in the same way: the mean importance query and sequences without a class row
_QUERY_SIGS = {
    "rajni_score_select_query_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "rajni_score_select_query": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_select_topk_query": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "rajni_patch_embed_query": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rajni_vit_workspace_bytes_query": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                   C.POINTER(VitQuery)]),
    "rajni_vit_forward_query": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                        C.POINTER(VitImage), C.POINTER(VitQuery), c_void_p, c_void_p, c_void_p]),
}
QUERY_SYMBOLS = tuple(_QUERY_SIGS.keys())
# include/rajni_hip_attnpool.h, additive in the same way: the attention-pool head (timm global_pool='map')
POOL_MAP = 6                         # rajni_vit_ext.pool through rajni_vit_forward_pool with a record; 4 stays unknown


class VitAttnPool(C.Structure):
    """rajni_vit_attn_pool (include/rajni_hip_attnpool.h): the weights of timm's AttentionPoolLatent, beside the plan"""
    _fields_ = [("q", c_void_p), ("kv_w", c_void_p), ("kv_b", c_void_p), ("proj_w", c_void_p), ("proj_b", c_void_p),
                ("norm_w", c_void_p), ("norm_b", c_void_p), ("norm_eps", c_float),
                ("fc1_w", c_void_p), ("fc1_b", c_void_p), ("fc2_w", c_void_p), ("fc2_b", c_void_p),
                ("hidden", c_int), ("heads", c_int), ("act", c_int)]


_ATTNPOOL_SIGS = {
    "rajni_attention_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rajni_vit_workspace_bytes_pool": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                  C.POINTER(VitQuery), C.POINTER(VitAttnPool)]),
    "rajni_vit_forward_pool": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                       C.POINTER(VitImage), C.POINTER(VitQuery), C.POINTER(VitAttnPool), c_void_p, c_void_p,
                                       c_void_p]),
}
ATTNPOOL_SYMBOLS = tuple(_ATTNPOOL_SIGS.keys())
# include/rajni_hip_norm.h, additive in the same way: RMSNorm trunks and the patch-embedding norm (the AIMv2 ViTs)
NORM_LAYERNORM, NORM_RMS = 0, 1      # rajni_vit_norm.kind


class VitNorm(C.Structure):
    """rajni_vit_norm (include/rajni_hip_norm.h): the kind of every norm of the forward but q/k-norm, and patch_embed.norm"""
    _fields_ = [("kind", c_int), ("embed_norm_eps", c_float), ("embed_norm_w", c_void_p), ("embed_norm_b", c_void_p)]


_NORM_SIGS = {
    "rajni_norm_rows": (c_int, [c_int, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_int,
                                c_void_p]),
    "rajni_embed_norm": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                 c_int, c_int, c_void_p]),
    "rajni_vit_workspace_bytes_norm": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                  C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm)]),
    "rajni_vit_forward_norm": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                       C.POINTER(VitImage), C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                       c_void_p, c_void_p, c_void_p]),
}
NORM_SYMBOLS = tuple(_NORM_SIGS.keys())
# include/rajni_hip_rope.h, additive in the same way: rotary position embeddings on the pruned token set
ROPE_INTERLEAVED, ROPE_HALF = 0, 1   # rajni_vit_rope.layout


class VitRope(C.Structure):
    """rajni_vit_rope (include/rajni_hip_rope.h): fp32 cos / sin tables [rows, D] per patch of the grid, shared or per head
    (head_stride) and per block (block_stride), and the pairing of the rotation"""
    _fields_ = [("cos", c_void_p), ("sin", c_void_p), ("head_stride", C.c_longlong), ("block_stride", C.c_longlong),
                ("rows", c_int), ("layout", c_int)]


_ROPE_SIGS = {
    "rajni_rope_qk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.c_longlong, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_void_p]),
    "rajni_vit_workspace_bytes_rope": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                  C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                                  C.POINTER(VitRope)]),
    "rajni_vit_forward_rope": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                       C.POINTER(VitImage), C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                       C.POINTER(VitRope), c_void_p, c_void_p, c_void_p]),
}
ROPE_SYMBOLS = tuple(_ROPE_SIGS.keys())
# include/rajni_hip_mlpnorm.h, additive in the same way: a norm inside the MLP, between the activation (or the gate) and fc2
HIDDEN_NORM_MAX = 4096   # RAJNI_HIDDEN_NORM_MAX: the widest row rajni_hidden_norm takes


class VitMlpNorm(C.Structure):
    """rajni_vit_mlp_norm (include/rajni_hip_mlpnorm.h): per-block fp32 weight / bias pointers [n], the eps and the model's MLP
    width n (plan.hidden is the zero-padded one)"""
    _fields_ = [("w", C.POINTER(c_void_p)), ("b", C.POINTER(c_void_p)), ("eps", C.c_float), ("n", c_int)]


_MLPNORM_SIGS = {
    "rajni_hidden_norm": (c_int, [c_int, c_void_p, C.c_long, c_void_p, c_void_p, c_int, c_int, C.c_float, c_int, c_int, c_void_p]),
    "rajni_vit_workspace_bytes_mlpnorm": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                     C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                                     C.POINTER(VitRope), C.POINTER(VitMlpNorm)]),
    "rajni_vit_forward_mlpnorm": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                          C.POINTER(VitImage), C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                          C.POINTER(VitRope), C.POINTER(VitMlpNorm), c_void_p, c_void_p, c_void_p]),
}
MLPNORM_SYMBOLS = tuple(_MLPNORM_SIGS.keys())
# include/rajni_hip_relpos.h, additive in the same way: a relative position bias on the attention logits (BEiT, vit_relpos)
RELPOS_MAX_GRID = 32     # RAJNI_RELPOS_MAX_GRID: patches per grid side


class VitRelPos(C.Structure):
    """rajni_vit_relpos (include/rajni_hip_relpos.h): fp32 table [blocks or 1][H][(2 gh - 1)(2 gw - 1)], the three prefix
    values [blocks or 1][H] each, the table's block stride (0: shared) and the patch grid"""
    _fields_ = [("table", c_void_p), ("prefix_q", c_void_p), ("prefix_k", c_void_p), ("prefix_qk", c_void_p),
                ("block_stride", C.c_longlong), ("gh", c_int), ("gw", c_int)]


_RELPOS_SIGS = {
    "rajni_attention_relpos": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rajni_score_select_relpos": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "rajni_vit_workspace_bytes_relpos": (c_size_t, [C.POINTER(VitPlan), C.POINTER(VitPrefix), C.POINTER(VitImage),
                                                    C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                                    C.POINTER(VitRope), C.POINTER(VitMlpNorm), C.POINTER(VitRelPos)]),
    "rajni_vit_forward_relpos": (c_int, [C.POINTER(VitPlan), C.POINTER(VitExt), C.POINTER(VitPrefix), C.POINTER(VitLayers),
                                         C.POINTER(VitImage), C.POINTER(VitQuery), C.POINTER(VitAttnPool), C.POINTER(VitNorm),
                                         C.POINTER(VitRope), C.POINTER(VitMlpNorm), C.POINTER(VitRelPos), c_void_p, c_void_p,
                                         c_void_p]),
}
RELPOS_SYMBOLS = tuple(_RELPOS_SIGS.keys())
RESAMPLE_MAX_GRID = 128     # RAJNI_RESAMPLE_MAX_GRID: grid cells per axis, source and destination
ABI_VERSION = 8     # include/rajni_hip.h; bumped whenever a struct or an entry point changes
_lib: Optional[C.CDLL] = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the C-ABI library (no GPU needed to load it).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeError(
            f"librajni_hip.so not found at {path}. Build it with `python rajni-vit_amd/build.py` "
            "(hipcc --offload-arch=gfx950). rajni_amd has no CPU or PyTorch fallback by design.")
    lib = C.CDLL(path)
    for name, (res, args) in (list(_SIGS.items()) + list(_LAYERS_SIGS.items()) + list(_IMAGE_SIGS.items()) + list(_QUERY_SIGS.items())
                              + list(_ATTNPOOL_SIGS.items()) + list(_NORM_SIGS.items()) + list(_ROPE_SIGS.items())
                              + list(_MLPNORM_SIGS.items()) + list(_RELPOS_SIGS.items())):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.rajni_abi_version() != ABI_VERSION:   # struct layouts below would not match: refuse, do not guess
        raise NativeError(f"{path} has ABI version {lib.rajni_abi_version()}, this package binds version {ABI_VERSION}: "
                          "rebuild it with `python rajni-vit_amd/build.py --force`")
    _lib = lib
    return lib


def lib() -> C.CDLL:
    return load_library()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().rajni_last_error().decode("utf-8", "replace")
        if rc == 2:
            raise NotImplementedError(f"{what}: {msg}")
        raise NativeError(f"{what} failed (code {rc}): {msg}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(device):
    """Context manager that makes `device` the current HIP device for the native calls inside it.  The C ABI takes
    raw pointers and a stream; kernel launches, hipFuncSetAttribute and the per-device CU count all go to the
    CURRENT device, so a model on cuda:1 while cuda:0 is current must switch first.  Free when already current."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() == idx:
        return _NO_GUARD
    return torch.cuda.device(idx)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return RAJNI_BF16
    if dt == torch.float16:
        return RAJNI_F16
    if dt == torch.float32:
        return RAJNI_F32
    raise NotImplementedError(f"rajni_amd: dtype {dt} is not supported (bfloat16 is the built compute type)")


def require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise NativeError(
            f"{name} is on {t.device}: rajni_amd runs on a ROCm (MI355X / gfx950) device only and has "
            "no CPU fallback. Move the model and inputs to 'cuda'.")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---- measurement hooks -------------------------------------------------------------------------

def profile_enable(mask: int) -> None:
    lib().rajni_profile_enable(mask)


def profile_reset() -> None:
    lib().rajni_profile_reset()


def profile_collect():
    """{kernel class name: dict(launches, ms, flops, bytes)} accumulated since the last reset."""
    n = NUM_KCLASS
    la = (C.c_longlong * n)()
    ms = (C.c_double * n)()
    fl = (C.c_double * n)()
    by = (C.c_double * n)()
    check(lib().rajni_profile_collect(la, ms, fl, by), "rajni_profile_collect")
    out = {}
    for i in range(n):
        if la[i]:
            out[lib().rajni_profile_class_name(i).decode()] = dict(
                kclass=i, launches=int(la[i]), ms=float(ms[i]), flops=float(fl[i]), bytes=float(by[i]))
    return out
