"""A minimal timm-*shaped* Vision Transformer.

timm is not installed in the build/bench images, and the reference wrapper
(`/root/reference/rajni/wrapper/model.py:9-10,34-37,45-48,65-66`,
`attention.py:8-12`) only consumes an attribute contract, not timm itself:

  base : .patch_embed(x)->[B,N-1,C]  .cls_token [1,1,C]  .pos_embed [1,N,C]
         (timm class_token=False: .cls_token is None and the sequence has no class row - the `*_gap_*` models; the
          reference cannot run those, RAJNIViTWrapper scores them with the mean query)
         .pos_drop  .blocks  .norm  .head
         (+ timm's optional .reg_token [1,R,C] / .num_prefix_tokens = 1 + R: register tokens behind the
          class token, which the reference does not handle and RAJNIViTWrapper does; and DeiT's distilled
          form, timm VisionTransformerDistilled: .dist_token [1,1,C] behind the class token, .head_dist,
          .num_prefix_tokens = 2, eval logits = (head(x[:, 0]) + head_dist(x[:, 1])) / 2)
  block: .norm1 .attn .norm2 .mlp  (+ optional .ls1 .ls2 .drop_path1 .drop_path2), blk(x)
  attn : .num_heads .scale .qkv (Linear C->3C laid out [3][H][D]) .proj .proj_drop

This module provides exactly that contract so tests, `bench.py` and the CLI have
a base model to wrap.  It is the *unpruned stock-PyTorch baseline* (the "4x"
denominator of BASELINE.json), not the product path: the product path is the HIP
forward behind `RAJNIViTWrapper`.

Weights are synthesised from a numpy PCG64 stream so that the same state dict
can be rebuilt bit-for-bit on the GPU box from `(config, seed)` alone (there is
no network for checkpoints).  Parameter names follow timm's state-dict naming
so a real timm checkpoint loads with `load_state_dict`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass(frozen=True)
class ViTConfig:
    img_size: int = 224
    patch_size: int = 16
    in_chans: int = 3
    embed_dim: int = 768
    depth: int = 12
    num_heads: int = 12
    mlp_ratio: float = 4.0
    num_classes: int = 1000
    layer_scale: Optional[float] = None   # DeiT-3 style LayerScale init value
    no_embed_class: bool = False          # DeiT-3: pos_embed has no CLS row
    ln_eps: float = 1e-6
    # timm VisionTransformer options (defaults = none of them: the modules and the synthetic weight stream of every
    # config above this line are unchanged)
    qk_norm: bool = False                 # LayerNorm(head_dim) on q and k in every block
    pre_norm: bool = False                # norm_pre after the pos-embed (CLIP-derived ViTs)
    global_pool: str = "token"            # 'token' (x[:, 0]), 'avg' (mean of x[:, 1:]) or 'map' (an AttentionPoolLatent head
                                          # over every row: the SigLIP towers)
    fc_norm: Optional[bool] = None        # None = timm's default: an fc_norm (and no final norm) iff global_pool == 'avg'
    class_token: bool = True              # timm class_token: False = no class row at all (cls_token is None, the prefix tokens
                                          # are the registers alone; needs global_pool='avg' or 'map' and no distillation, as timm
                                          # asserts).  (In front of mlp, distilled, act and reg_tokens, which existing tests
                                          # hold to be the last four fields)
    mlp: str = "mlp"                      # the block's MLP: "mlp" (fc1 -> act -> fc2), "swiglu_packed" (timm GluMlp with
                                          # act_layer=nn.SiLU, gate_last=False, alias SwiGLUPacked: ONE fc1 of 2 * hidden_dim
                                          # outputs, gate half first - the DINOv2 giant ViTs) or "swiglu" (timm SwiGLU: fc1_g and
                                          # fc1_x apart).  hidden_dim stays fc2's input width.  On gated configs `act` keeps its
                                          # default and is unused: the gate is SiLU.  (In front of distilled, act and reg_tokens:
                                          # existing tests hold those three to be the last fields)
    distilled: bool = False               # DeiT distilled (timm VisionTransformerDistilled): a dist_token behind the class
                                          # token and a second classifier head_dist; not together with reg_tokens.  (In front of
                                          # act and reg_tokens: existing tests hold those two to be the last fields)
    act: str = "gelu"                     # MLP activation: "gelu" (exact erf) or "quick_gelu" (x * sigmoid(1.702 x): the OpenAI
                                          # CLIP, MetaCLIP and DFN towers); no weights are drawn for it.  (Keyword only in
                                          # practice; it sits in front of reg_tokens because tests/test_prefix_cpu.py holds
                                          # reg_tokens to be the last field)
    reg_tokens: int = 0                   # register tokens behind the class token (timm reg_tokens; DINOv2 "reg4": 4)

    # What NormViTConfig (below) makes fields: plain class attributes here, so that every config answers `cfg.norm`,
    # `cfg.embed_norm` and `cfg.bias` while this class keeps the twenty fields existing tests count.
    norm = "layernorm"
    embed_norm = False
    bias = True
    # ... and what RopeViTConfig makes fields, in the same way
    rope = "none"
    rope_half = False
    abs_pos = True
    # ... and what EvaViTConfig makes fields
    mlp_norm = False
    eva_block = False
    qkv_split = False
    # ... and what RelPosViTConfig makes fields
    rel_pos = "none"
    img_width = None

    def __post_init__(self):
        if self.rel_pos not in ("none", "beit", "beit_shared", "relpos", "srelpos"):
            raise ValueError(f"ViTConfig: rel_pos must be 'none', 'beit', 'beit_shared', 'relpos' or 'srelpos', got {self.rel_pos!r}")
        if self.rel_pos != "none" and (self.rope != "none" or not self.class_token or self.distilled):
            raise ValueError("ViTConfig: rel_pos needs a class token and goes with neither rope nor distilled")
        if self.img_width is not None and (self.rel_pos == "none" or self.abs_pos):
            raise ValueError("ViTConfig: img_width (a rectangular grid) is for rel_pos models without an absolute embedding")
        if self.rope not in ("none", "axial", "mixed"):
            raise ValueError(f"ViTConfig: rope must be 'none', 'axial' or 'mixed', got {self.rope!r}")
        if self.rope != "none" and self.head_dim % 4:
            raise ValueError(f"ViTConfig: rope needs a head dim that is a multiple of 4 (two axes of rotated pairs), got {self.head_dim}")
        if self.norm not in ("layernorm", "rms"):
            raise ValueError(f"ViTConfig: norm must be 'layernorm' or 'rms', got {self.norm!r}")
        if self.distilled and self.reg_tokens:
            raise ValueError("ViTConfig: distilled together with reg_tokens is not a timm model")
        if self.mlp not in ("mlp", "swiglu_packed", "swiglu"):
            raise ValueError(f"ViTConfig: mlp must be 'mlp', 'swiglu_packed' or 'swiglu', got {self.mlp!r}")
        if not self.class_token and self.global_pool == "token":
            raise ValueError("ViTConfig: class_token=False needs global_pool='avg' or 'map' (timm asserts it: a token head has no row to read)")
        if not self.class_token and self.distilled:
            raise ValueError("ViTConfig: class_token=False together with distilled is not a timm model")

    @property
    def num_prefix_tokens(self) -> int:
        return int(self.class_token) + self.reg_tokens + int(self.distilled)

    @property
    def use_fc_norm(self) -> bool:
        return self.global_pool == "avg" if self.fc_norm is None else bool(self.fc_norm)

    @property
    def grid(self):
        """(gh, gw) of the model's own input: img_size is its height, and its width too unless img_width says otherwise"""
        return self.img_size // self.patch_size, (self.img_width or self.img_size) // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid[0] * self.grid[1]

    @property
    def head_dim(self) -> int:
        return self.embed_dim // self.num_heads

    @property
    def hidden_dim(self) -> int:
        return int(self.embed_dim * self.mlp_ratio)

    def to_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class NormViTConfig(ViTConfig):
    """ViTConfig plus the norm options of the AIMv2 image towers.  A subclass, not three more fields of ViTConfig: existing
    tests hold that class to its twenty fields and to the order of the last five.  (Keyword only in practice.)"""
    norm: str = "layernorm"               # every norm of the trunk but q/k-norm: "layernorm" or "rms" (timm RmsNorm: a weight,
                                          # no bias, no mean)
    embed_norm: bool = False              # timm embed_norm_layer: PatchEmbed.norm of that kind on the projected patch rows,
                                          # in front of the position embedding
    bias: bool = True                     # False: no bias in qkv, proj and the MLP (the patch projection keeps its own)


@dataclass(frozen=True)
class RopeViTConfig(NormViTConfig):
    """NormViTConfig plus rotary position embeddings (EVA02, timm's vit_*_rope_* line, the Perception Encoder towers, DINOv3).  A
    subclass for NormViTConfig's reason.  (Keyword only in practice.)"""
    rope: str = "none"                    # "none"; "axial": one table for all heads and blocks, D / 4 frequency bands per image
                                          # axis; "mixed": learned per-block, per-head frequencies over both axes (RoPE-Mixed)
    rope_half: bool = False               # False: the pairs are (2i, 2i + 1) (timm rot()); True: (i, i + D / 2) (rotate_half)
    abs_pos: bool = True                  # False: no learned absolute position embedding at all (pos_embed is None)


@dataclass(frozen=True)
class EvaViTConfig(RopeViTConfig):
    """RopeViTConfig plus the rest of timm's `Eva` model (the EVA02 image towers).  A subclass for NormViTConfig's reason.
    (Keyword only in practice.)"""
    mlp_norm: bool = False                # a norm of the trunk's kind over the hidden width, between the activation (or the
                                          # gate) and fc2: timm Mlp / SwiGLU `norm_layer`, EVA02's sub-LayerNorm (scale_mlp)
    eva_block: bool = False               # timm EvaBlock / EvaAttention spellings: LayerScale as the parameters `gamma_1` /
                                          # `gamma_2` (None without layer_scale) with no ls1 / ls2 modules; a bias-free `qkv`
                                          # beside the parameters `q_bias` / `v_bias` (k has no bias); `attn.norm` = Identity
    qkv_split: bool = False               # `q_proj` / `k_proj` (no bias) / `v_proj` apart and `attn.qkv` None (qkv_fused=False)


@dataclass(frozen=True)
class RelPosViTConfig(EvaViTConfig):
    """EvaViTConfig plus a learned relative position bias on the attention logits (BEiT / BEiTv2, timm's vit_relpos_* and
    vit_srelpos_* line).  A subclass for NormViTConfig's reason.  (Keyword only in practice.)"""
    rel_pos: str = "none"                 # "beit": every block's attention owns `relative_position_bias_table`
                                          # [(2 gh - 1)(2 gw - 1) + 3, H] (three rows for the class token's pairs),
                                          # `relative_position_index` and `_get_rel_pos_bias()`; "beit_shared": one model-level
                                          # `rel_pos_bias` module (BEiT use_shared_rel_pos_bias); "relpos": every attention owns a
                                          # `rel_pos` module with `get_bias()` and zero rows / columns for the prefix tokens
                                          # (timm RelPosBias); "srelpos": one model-level `shared_rel_pos` of that kind
    img_width: Optional[int] = None       # the input's width where it differs from img_size (its height): a rectangular grid


# The model names BASELINE.json's configs use.
CONFIGS: Dict[str, ViTConfig] = {
    "vit_tiny_patch16_224": ViTConfig(embed_dim=192, depth=12, num_heads=3),
    "vit_small_patch16_224": ViTConfig(embed_dim=384, depth=12, num_heads=6),
    "vit_base_patch16_224": ViTConfig(embed_dim=768, depth=12, num_heads=12),
    "vit_large_patch16_224": ViTConfig(embed_dim=1024, depth=24, num_heads=16),
    "vit_large_patch16_384": ViTConfig(img_size=384, embed_dim=1024, depth=24, num_heads=16),
    "deit3_base_patch16_224": ViTConfig(embed_dim=768, depth=12, num_heads=12,
                                        layer_scale=1e-6, no_embed_class=True),
    # head dim 80, patch 14: the general attention / importance kernels and the materialised patch columns
    "vit_huge_patch14_224": ViTConfig(patch_size=14, embed_dim=1280, depth=32, num_heads=16),
    # tiny head_dim-64 model for fast parity tests (not a timm name)
    "vit_micro_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2,
                                      num_classes=10),
    # the same with DeiT-3's LayerScale and no_embed_class pos-embed (N-1 rows): loader / B3 tests (not a timm name)
    "deit3_micro_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                        layer_scale=1e-6, no_embed_class=True),
    # embed dim 512 / MLP width 2048 (multiples of 256, K >= 512: what the fp8 x fp8 kernel needs) at micro cost (not a timm name)
    "vit_micro512_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10),
    # patch 14 (ViT-L/14, ViT-H/14, DINOv2): 3*14*14 = 588 input features, not whole 64-wide K steps
    "vit_micro_patch14_56": ViTConfig(img_size=56, patch_size=14, embed_dim=128, depth=4, num_heads=2,
                                      num_classes=10),
    # the same with head dim 80 (ViT-H's), for the general-head-dim kernels (not a timm name)
    "vit_micro_d80_patch16_64": ViTConfig(img_size=64, embed_dim=320, depth=4, num_heads=4,
                                          num_classes=10),
    # ---- timm options beyond plain ViT / DeiT ----
    # CLIP-derived ViT-B/16 (timm `vit_base_patch16_clip_224`: pre_norm, LayerNorm eps 1e-5, exact GELU, token head; the
    # `_quickgelu_` variants - the same towers with the other activation - are further down)
    "vit_base_patch16_clip_224": ViTConfig(embed_dim=768, depth=12, num_heads=12, pre_norm=True, ln_eps=1e-5),
    # ViT-B/16 with q/k LayerNorm (timm `vit_base_patch16_224(qk_norm=True)`; not a checkpoint name)
    "vit_base_patch16_qknorm_224": ViTConfig(embed_dim=768, depth=12, num_heads=12, qk_norm=True),
    # micro models, one option each and all together (not timm names)
    "vit_micro_qknorm_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, qk_norm=True),
    "vit_micro_prenorm_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, pre_norm=True),
    "vit_micro_gap_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, global_pool="avg"),
    "vit_micro_fcnorm_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, fc_norm=True),
    "vit_micro_all_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, qk_norm=True,
                                          pre_norm=True, global_pool="avg"),
    # q/k-norm on the fp8-capable micro model, and on head dim 80 (a 10-lane group of the general q/k-norm form)
    "vit_micro512_qknorm_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10, qk_norm=True),
    "vit_micro_d80_qknorm_patch16_64": ViTConfig(img_size=64, embed_dim=320, depth=4, num_heads=4, num_classes=10,
                                                 qk_norm=True, global_pool="avg"),
    # ---- register tokens (timm reg_tokens=R: token order [cls, reg_0 .. reg_{R-1}, patches]) ----
    # class token + 4 registers, a pos-embed with a row for every prefix token (not timm names)
    "vit_micro_reg4_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, reg_tokens=4),
    # the same with no_embed_class (pos-embed on the patch rows only) and LayerScale: the DINOv2 / DeiT-3 layout
    "deit3_micro_reg4_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                             layer_scale=1e-6, no_embed_class=True, reg_tokens=4),
    # one register, patch 14 (materialised patch columns), 'avg' pool over the patch rows behind both prefix tokens
    "vit_micro_reg1_gap_patch14_56": ViTConfig(img_size=56, patch_size=14, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                               global_pool="avg", reg_tokens=1),
    # registers on the fp8-capable micro model
    "vit_micro512_reg4_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10, reg_tokens=4),
    # timm `vit_small_patch14_reg4_dinov2` dimensions (DINOv2 ViT-S/14 with 4 registers: no_embed_class, LayerScale) at
    # img_size 224 = 261 tokens, and at the pretrained size 518 = 1374 tokens: more than one workgroup's LDS holds, scored by
    # the tiled score kernels (up to 16416 tokens, every head dim and dtype)
    "vit_small_patch14_reg4_dinov2": ViTConfig(img_size=224, patch_size=14, embed_dim=384, depth=12, num_heads=6,
                                               layer_scale=1e-5, no_embed_class=True, reg_tokens=4),
    "vit_small_patch14_reg4_dinov2_518": ViTConfig(img_size=518, patch_size=14, embed_dim=384, depth=12, num_heads=6,
                                                   layer_scale=1e-5, no_embed_class=True, reg_tokens=4),
    # ---- more tokens than one workgroup's LDS holds (the tiled score kernels) at micro cost (not timm names) ----
    # 400 px at patch 16: 626 tokens x 2 heads of 64 = 42 056 LDS words in the single-workgroup layout, 40 960 available
    "vit_micro_patch16_400": ViTConfig(img_size=400, embed_dim=128, depth=4, num_heads=2, num_classes=10),
    # the same with 4 registers in the DINOv2 / DeiT-3 layout (630 tokens)
    "vit_micro_reg4_patch16_400": ViTConfig(img_size=400, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                            layer_scale=1e-6, no_embed_class=True, reg_tokens=4),
    # ---- QuickGELU MLPs: the original OpenAI CLIP towers, MetaCLIP, DFN (timm `*_clip_quickgelu_*`) ----
    "vit_base_patch16_clip_quickgelu_224": ViTConfig(embed_dim=768, depth=12, num_heads=12, pre_norm=True, ln_eps=1e-5,
                                                     act="quick_gelu"),
    "vit_base_patch32_clip_quickgelu_224": ViTConfig(patch_size=32, embed_dim=768, depth=12, num_heads=12, pre_norm=True,
                                                     ln_eps=1e-5, act="quick_gelu"),
    "vit_large_patch14_clip_quickgelu_224": ViTConfig(patch_size=14, embed_dim=1024, depth=24, num_heads=16, pre_norm=True,
                                                      ln_eps=1e-5, act="quick_gelu"),
    # micro models (not timm names): the activation alone, the CLIP layout, the fp8-capable dims, and an MLP width that is
    # not whole 64-wide K steps (344 -> 384 zero-padded hidden columns: act(0) must be exactly 0)
    "vit_micro_quickgelu_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                                act="quick_gelu"),
    "vit_micro_clip_quickgelu_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                                     pre_norm=True, ln_eps=1e-5, act="quick_gelu"),
    "vit_micro512_quickgelu_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10,
                                                   act="quick_gelu"),
    "vit_micro_quickgelu_h344_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, mlp_ratio=2.6875,
                                                     num_classes=10, act="quick_gelu"),
    # ---- DeiT distilled (timm VisionTransformerDistilled): token order [cls, dist, patches], two averaged heads ----
    "deit_tiny_distilled_patch16_224": ViTConfig(embed_dim=192, depth=12, num_heads=3, distilled=True),
    "deit_small_distilled_patch16_224": ViTConfig(embed_dim=384, depth=12, num_heads=6, distilled=True),
    "deit_base_distilled_patch16_224": ViTConfig(embed_dim=768, depth=12, num_heads=12, distilled=True),
    "deit_base_distilled_patch16_384": ViTConfig(img_size=384, embed_dim=768, depth=12, num_heads=12, distilled=True),
    # micro models (not timm names): 18 tokens; the second on the fp8-capable dims
    "vit_micro_distilled_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, distilled=True),
    "vit_micro512_distilled_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10,
                                                   distilled=True),
}

# The gated-MLP configs live in a table of their own: the key list of CONFIGS is held fixed by tests/test_distilled_cpu.py.
# create_model() and config_of() know both tables.
SWIGLU_CONFIGS: Dict[str, ViTConfig] = {
    # ---- SwiGLU MLPs: the DINOv2 giant ViTs (timm `vit_giant_patch14_dinov2`, `vit_giant_patch14_reg4_dinov2`: ViT-g/14,
    # 1536 wide, 24 heads of 64, 40 blocks, LayerScale, SwiGLUPacked with hidden 4096, pretrained at 518 px) ----
    "vit_giant_patch14_dinov2": ViTConfig(img_size=518, patch_size=14, embed_dim=1536, depth=40, num_heads=24,
                                          mlp_ratio=4096 / 1536, layer_scale=1e-5, mlp="swiglu_packed"),
    "vit_giant_patch14_reg4_dinov2": ViTConfig(img_size=518, patch_size=14, embed_dim=1536, depth=40, num_heads=24,
                                               mlp_ratio=4096 / 1536, layer_scale=1e-5, no_embed_class=True,
                                               mlp="swiglu_packed", reg_tokens=4),
    # micro models (not timm names): the packed form, the split form with the same dims, a hidden width that is not whole
    # 64-wide K steps (344 -> 384 zero-padded columns PER HALF: silu(0) * 0 must be exactly 0), the fp8-capable dims (at
    # batch 64 FC1 has 1088 rows and 2048 W rows: the wide tiling), and the giant's combination of features
    "vit_micro_swiglu_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, mlp_ratio=2.0, num_classes=10,
                                             mlp="swiglu_packed"),
    "vit_micro_swiglu_split_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, mlp_ratio=2.0,
                                                   num_classes=10, mlp="swiglu"),
    "vit_micro_swiglu_h344_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, mlp_ratio=2.6875,
                                                  num_classes=10, mlp="swiglu_packed"),
    "vit_micro512_swiglu_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, mlp_ratio=2.0,
                                                num_classes=10, mlp="swiglu_packed"),
    "vit_micro_reg4_swiglu_patch14_56": ViTConfig(img_size=56, patch_size=14, embed_dim=128, depth=4, num_heads=2,
                                                  mlp_ratio=2.0, num_classes=10, layer_scale=1e-6, no_embed_class=True,
                                                  mlp="swiglu_packed", reg_tokens=4),
}


# Models without a class token (timm class_token=False, global_pool='avg'), in a table of their own for the same reason.
NOCLASS_CONFIGS: Dict[str, ViTConfig] = {
    # micro models (not timm names): no prefix token at all (timm's default head for 'avg': fc_norm behind the pool, no final
    # norm); 4 registers in the DINOv2 / DeiT-3 layout (no_embed_class, LayerScale) with the final norm in front of the pool
    # (fc_norm=False, so the feature outputs exist); head dim 80 with one register and a pos-embed row for it (R + n rows)
    "vit_micro_nocls_gap_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                                global_pool="avg", class_token=False),
    "vit_micro_reg4_nocls_gap_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                                     layer_scale=1e-6, no_embed_class=True, global_pool="avg", fc_norm=False,
                                                     class_token=False, reg_tokens=4),
    "vit_micro_reg1_nocls_gap_d80_patch16_64": ViTConfig(img_size=64, embed_dim=320, depth=4, num_heads=4, num_classes=10,
                                                         global_pool="avg", class_token=False, reg_tokens=1),
    # The dimensions of two timm checkpoints of the family.  timm is not importable where this was written: both entries were
    # WRITTEN FROM MEMORY AND ARE UNVERIFIED (width, depth, heads, MLP ratio, fc_norm and LayerScale may each be off); no test
    # depends on their being exact - they exist to give the cost tools a real-size shape.
    "vit_medium_patch16_gap_256": ViTConfig(img_size=256, embed_dim=512, depth=12, num_heads=8, layer_scale=1e-6,
                                            global_pool="avg", fc_norm=False, class_token=False),
    "vit_betwixt_patch16_reg4_gap_256": ViTConfig(img_size=256, embed_dim=640, depth=12, num_heads=10, layer_scale=1e-5,
                                                  no_embed_class=True, global_pool="avg", class_token=False, reg_tokens=4),
}


# Models with an attention-pool head (timm global_pool='map': AttentionPoolLatent over every row of norm(x)), in a table of
# their own for the same reason.
MAP_CONFIGS: Dict[str, ViTConfig] = {
    # micro models (not timm names): the SigLIP layout (no class token, 16 tokens); a class token in front of the pool (17
    # tokens, the pool reads the class row too); head dim 80 with 4 registers; 625 tokens (more than one pass of the pool
    # kernel's token slots, and the tiled score kernels); the fp8-capable dims
    "vit_micro_map_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                          global_pool="map", class_token=False),
    "vit_micro_cls_map_patch16_64": ViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                              global_pool="map"),
    "vit_micro_reg4_map_d80_patch16_64": ViTConfig(img_size=64, embed_dim=320, depth=4, num_heads=4, num_classes=10,
                                                   global_pool="map", class_token=False, reg_tokens=4),
    "vit_micro_map_patch16_400": ViTConfig(img_size=400, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                           global_pool="map", class_token=False),
    "vit_micro512_map_patch16_64": ViTConfig(img_size=64, embed_dim=512, depth=4, num_heads=8, num_classes=10,
                                             global_pool="map", class_token=False),
    # The dimensions of two SigLIP image towers.  timm is not importable where this was written: both entries were WRITTEN FROM
    # MEMORY AND ARE UNVERIFIED (width, depth, heads, MLP width and eps may each be off; the checkpoints ship with
    # num_classes=0, here they keep a 1000-way head like every other real-size entry); no test depends on their being exact -
    # they exist to give the cost tools a real-size shape.  so400m: 1152 wide, 27 blocks, 16 heads of 72, MLP width 4304
    # (not whole 64-wide K steps: zero-padded to 4352)
    "vit_base_patch16_siglip_224": ViTConfig(embed_dim=768, depth=12, num_heads=12, global_pool="map", class_token=False),
    "vit_so400m_patch14_siglip_224": ViTConfig(patch_size=14, embed_dim=1152, depth=27, num_heads=16, mlp_ratio=4304 / 1152,
                                               global_pool="map", class_token=False),
}


# RMSNorm trunks and a norm inside the patch embedding, in a table of their own for the same reason.
_AIMV2 = dict(patch_size=14, depth=24, num_classes=0, ln_eps=1e-5, global_pool="avg", fc_norm=False, class_token=False,
              mlp="swiglu", norm="rms", embed_norm=True, bias=False)
NORM_CONFIGS: Dict[str, ViTConfig] = {
    # Apple's AIMv2 image towers (timm `aimv2_*_patch14_224`): RmsNorm(eps=1e-5) for norm1, norm2, norm and patch_embed.norm, the
    # split SwiGLU MLP, no class token, global_pool='avg' without fc_norm, headless, no bias in qkv / proj / the MLP.  timm is
    # not importable where this was written: the entries were WRITTEN FROM MEMORY OF timm 1.x AND ARE UNVERIFIED (width, depth,
    # heads, MLP width, eps and which linears carry a bias may each be off); no test depends on their being exact.  The _336 and
    # _448 checkpoints differ in img_size alone.  aimv2_3b is 3072 wide: beyond the row kernels' C <= 2048, so RAJNIViTWrapper
    # refuses it - it is listed to say so.
    "aimv2_large_patch14_224": NormViTConfig(embed_dim=1024, num_heads=8, mlp_ratio=2816 / 1024, **_AIMV2),
    "aimv2_huge_patch14_224": NormViTConfig(embed_dim=1536, num_heads=12, mlp_ratio=4096 / 1536, **_AIMV2),
    "aimv2_1b_patch14_224": NormViTConfig(embed_dim=2048, num_heads=16, mlp_ratio=5632 / 2048, **_AIMV2),
    "aimv2_3b_patch14_224": NormViTConfig(embed_dim=3072, num_heads=24, mlp_ratio=8192 / 3072, **_AIMV2),
    # micro models (not timm names): vit_micro_patch16_64 with RMS norms; the AIMv2 recipe at micro cost (16 tokens, head dim
    # 64); the same with head dim 128 and patch 14 (the general head-dim kernels, the materialised patch columns); a LayerNorm
    # model with a LayerNorm patch_embed.norm, a class token and 4 registers and a pos-embed row for each of them
    "vit_micro_rms_patch16_64": NormViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10, norm="rms"),
    "vit_micro_aimv2_patch16_64": NormViTConfig(img_size=64, embed_dim=128, num_heads=2, mlp_ratio=2.0,
                                                **{**_AIMV2, "patch_size": 16, "depth": 4}),
    "vit_micro_aimv2_d128_patch14_56": NormViTConfig(img_size=56, embed_dim=256, num_heads=2, mlp_ratio=2.0,
                                                     **{**_AIMV2, "depth": 4}),
    "vit_micro_reg4_embednorm_patch16_64": NormViTConfig(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10,
                                                         reg_tokens=4, embed_norm=True),
}


# Rotary position embeddings, in a table of their own for the same reason.
_MICRO = dict(img_size=64, embed_dim=128, depth=4, num_heads=2, num_classes=10)
ROPE_CONFIGS: Dict[str, ViTConfig] = {
    # micro models (not timm names).  Axial, interleaved pairs, a class token, the absolute embedding kept, head dim 64 (EVA02's
    # combination); axial, rotate_half, a class token and 4 registers, no absolute embedding, LayerScale (the DINOv3 recipe);
    # mixed - a table per block and head -, no class token, 'avg' pool; head dim 40 (the half-layout partner straddles a
    # 16-byte chunk), rotate_half, patch 14
    "vit_micro_rope_patch16_64": RopeViTConfig(**_MICRO, rope="axial"),
    "vit_micro_rope_half_reg4_patch16_64": RopeViTConfig(**_MICRO, layer_scale=1e-6, reg_tokens=4, rope="axial", rope_half=True,
                                                         abs_pos=False),
    "vit_micro_rope_mixed_gap_patch16_64": RopeViTConfig(**_MICRO, global_pool="avg", class_token=False, rope="mixed"),
    "vit_micro_rope_d40_patch14_56": RopeViTConfig(img_size=56, patch_size=14, embed_dim=320, depth=4, num_heads=8, num_classes=10,
                                                   rope="axial", rope_half=True),
    # ViT-B/16 dimensions for the cost tools (not checkpoint names: EVA02's SwiGLU-with-norm MLP and DINOv3's checkpoints are
    # out of scope): axial with the absolute embedding, and the DINOv3 recipe
    "vit_base_patch16_rope_224": RopeViTConfig(embed_dim=768, depth=12, num_heads=12, rope="axial"),
    "vit_base_patch16_rope_half_reg4_224": RopeViTConfig(embed_dim=768, depth=12, num_heads=12, layer_scale=1e-5, reg_tokens=4,
                                                         rope="axial", rope_half=True, abs_pos=False),
}


# timm's `Eva` models, in a table of their own for the same reason.
_EVA = dict(patch_size=14, rope="axial", eva_block=True)
EVA_CONFIGS: Dict[str, ViTConfig] = {
    # ---- the EVA02 towers at 224 px.  timm is not importable where this was written: the four entries are WRITTEN FROM MEMORY
    # of timm 1.x AND ARE UNVERIFIED (whether q / k / v are fused, the heads' presence and the pooling may each be off): Ti and S
    # with the packed SwiGLU and no norm inside it, B and L with the split SwiGLU and its sub-LayerNorm over 2048 / 2730 ----
    "eva02_tiny_patch14_224": EvaViTConfig(embed_dim=192, depth=12, num_heads=3, mlp_ratio=512 / 192, mlp="swiglu_packed", **_EVA),
    "eva02_small_patch14_224": EvaViTConfig(embed_dim=384, depth=12, num_heads=6, mlp_ratio=1024 / 384, mlp="swiglu_packed", **_EVA),
    "eva02_base_patch14_224": EvaViTConfig(embed_dim=768, depth=12, num_heads=12, mlp_ratio=2048 / 768, mlp="swiglu",
                                           mlp_norm=True, qkv_split=True, **_EVA),
    "eva02_large_patch14_224": EvaViTConfig(embed_dim=1024, depth=24, num_heads=16, mlp_ratio=2730 / 1024, mlp="swiglu",
                                            mlp_norm=True, qkv_split=True, **_EVA),
    # micro models (not timm names).  The Eva block with LayerScale, the split SwiGLU and its norm over 344 columns (whole
    # 16-byte chunks, 384 zero-padded); 342 columns (a partial last chunk) with q / k / v apart; the RMS kind without a class
    # token; a plain GELU MLP with mlp.norm on the ordinary block and no rope; head dim 40
    "vit_micro_eva_patch16_64": EvaViTConfig(**_MICRO, mlp_ratio=2.6875, layer_scale=1e-6, mlp="swiglu", mlp_norm=True,
                                             rope="axial", eva_block=True),
    "vit_micro_eva_h342_patch16_64": EvaViTConfig(**_MICRO, mlp_ratio=342 / 128, mlp="swiglu", mlp_norm=True, rope="axial",
                                                  eva_block=True, qkv_split=True),
    "vit_micro_eva_rms_gap_patch16_64": EvaViTConfig(**_MICRO, mlp_ratio=2.6875, layer_scale=1e-6, mlp="swiglu", mlp_norm=True,
                                                     rope="axial", eva_block=True, norm="rms", global_pool="avg",
                                                     class_token=False),
    "vit_micro_mlpnorm_patch16_64": EvaViTConfig(**_MICRO, mlp_ratio=2.6875, mlp_norm=True),
    "vit_micro_eva_d40_patch14_56": EvaViTConfig(img_size=56, patch_size=14, embed_dim=320, depth=4, num_heads=8, num_classes=10,
                                                 mlp_ratio=2.0, mlp="swiglu", mlp_norm=True, rope="axial", eva_block=True),
}
# Models with a relative position bias, in a table of their own for the same reason.
_BEIT = dict(eva_block=True, abs_pos=False, global_pool="avg", rel_pos="beit")
RELPOS_CONFIGS: Dict[str, ViTConfig] = {
    # ---- the real checkpoints' dimensions.  timm is not importable where this was written: the entries are WRITTEN FROM MEMORY of
    # timm 1.x AND ARE UNVERIFIED (the LayerScale init values and the pooling may be off) ----
    "beit_base_patch16_224": RelPosViTConfig(embed_dim=768, depth=12, num_heads=12, layer_scale=0.1, **_BEIT),
    "beit_large_patch16_224": RelPosViTConfig(embed_dim=1024, depth=24, num_heads=16, layer_scale=1e-5, **_BEIT),
    "beitv2_base_patch16_224": RelPosViTConfig(embed_dim=768, depth=12, num_heads=12, layer_scale=1e-5, **_BEIT),
    "vit_relpos_base_patch16_clsgap_224": RelPosViTConfig(embed_dim=768, depth=12, num_heads=12, abs_pos=False, global_pool="avg",
                                                          fc_norm=False, rel_pos="relpos"),
    # ---- micro models (not timm names).  BEiT's layout - q / v bias, gamma_1 / gamma_2, no absolute embedding, mean pool with
    # fc_norm - with a table per block; its shared-bias twin; a rel_pos model with a class-token head; a 48 x 96 input (3 x 6
    # grid: the only one on which exchanging dy and dx shows) ----
    "beit_micro_patch16_64": RelPosViTConfig(**_MICRO, layer_scale=0.1, **_BEIT),
    "beit_micro_shared_patch16_64": RelPosViTConfig(**_MICRO, layer_scale=0.1, **{**_BEIT, "rel_pos": "beit_shared"}),
    "vit_micro_relpos_patch16_64": RelPosViTConfig(**_MICRO, abs_pos=False, rel_pos="relpos"),
    "beit_micro_patch16_48x96": RelPosViTConfig(**{**_MICRO, "img_size": 48}, img_width=96, layer_scale=0.1, **_BEIT),
}
ALL_CONFIG_TABLES = (CONFIGS, SWIGLU_CONFIGS, NOCLASS_CONFIGS, MAP_CONFIGS, NORM_CONFIGS, ROPE_CONFIGS, EVA_CONFIGS, RELPOS_CONFIGS)


def config_of(name: str) -> ViTConfig:
    """the built-in config of that name, from CONFIGS, SWIGLU_CONFIGS, NOCLASS_CONFIGS, MAP_CONFIGS, NORM_CONFIGS, ROPE_CONFIGS,
    EVA_CONFIGS or RELPOS_CONFIGS"""
    tables = ALL_CONFIG_TABLES
    for table in tables:
        if name in table:
            return table[name]
    raise KeyError(f"'{name}' is not a built-in config {[n for t in tables for n in sorted(t)]}")


class RmsNorm(nn.Module):
    """timm `RmsNorm`: x * rsqrt(mean(x^2) + eps) * weight over the last axis - a weight, no bias, no mean.  The statistics are
    fp32 whatever the input's dtype; the normalised row returns to that dtype before the weight multiplies it."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.normalized_shape = (dim,)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + self.eps)).to(x.dtype) * self.weight


def make_norm(cfg: "ViTConfig", dim: int) -> nn.Module:
    return RmsNorm(dim, eps=cfg.ln_eps) if cfg.norm == "rms" else nn.LayerNorm(dim, eps=cfg.ln_eps)


class PatchEmbed(nn.Module):
    def __init__(self, cfg: ViTConfig):
        super().__init__()
        self.img_size = (cfg.img_size, cfg.img_width or cfg.img_size)
        self.patch_size = (cfg.patch_size, cfg.patch_size)
        self.num_patches = cfg.num_patches
        if cfg.rel_pos != "none":      # timm PatchEmbed.grid_size (the other configs' modules stay as they were)
            self.grid_size = cfg.grid
        self.proj = nn.Conv2d(cfg.in_chans, cfg.embed_dim, cfg.patch_size, cfg.patch_size)
        self.norm = make_norm(cfg, cfg.embed_dim) if cfg.embed_norm else nn.Identity()

    def forward(self, x):
        return self.norm(self.proj(x).flatten(2).transpose(1, 2))


def rot_interleaved(x):
    """timm rot(): y[2i] = -x[2i + 1], y[2i + 1] = x[2i]"""
    return torch.stack([-x[..., 1::2], x[..., ::2]], -1).reshape(x.shape)


def rot_half(x):
    """rotate_half: y[j] = -x[j + D/2] for j < D/2, x[j - D/2] otherwise"""
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def apply_rot_embed_cat(x, emb, half: bool = False):
    """timm apply_rot_embed_cat: x [B, H, n, D], emb [n, 2D] or [H, n, 2D] = sin || cos on the last axis.  fp32 arithmetic,
    cast back to x's dtype."""
    sin, cos = emb.float().chunk(2, dim=-1)
    xf = x.float()
    return (xf * cos + (rot_half(xf) if half else rot_interleaved(xf)) * sin).to(x.dtype)


class RotaryEmbedding(nn.Module):
    """The rotary tables of a model, after timm's `RotaryEmbeddingCat` (written from memory of timm 1.x, unverified against an
    installed timm): `get_embed(shape=None)` returns sin || cos on the last axis for the patches of a (gh, gw) grid (default: the
    model's own), row-major - [n, 2D] for "axial" (one table for all heads and blocks), [depth, H, n, 2D] for "mixed".  The
    tables are deterministic functions of the grid: positions are the patch coordinates (y, x) = 0, 1, 2 ...

    axial: D / 4 bands w_i = temperature ** (-i / (D / 4)); the D / 2 angles of patch (y, x) are [y w_0 .. y w_{D/4-1},
           x w_0 .. x w_{D/4-1}].
    mixed: `freqs` [depth, H, D / 2, 2], a parameter (drawn from the synthetic weight stream); angle i is
           x freqs[..., i, 0] + y freqs[..., i, 1].
    Angle i goes to the pair the layout names: elements (2i, 2i + 1) (interleaved) or (i, i + D / 2) (half)."""

    def __init__(self, head_dim: int, grid, kind: str = "axial", half: bool = False, num_heads: int = 1, depth: int = 1,
                 temperature: float = 100.0):
        super().__init__()
        assert kind in ("axial", "mixed") and head_dim % 4 == 0
        self.dim, self.kind, self.half, self.grid, self.temperature = head_dim, kind, half, tuple(grid), temperature
        self.freqs = nn.Parameter(torch.zeros(depth, num_heads, head_dim // 2, 2)) if kind == "mixed" else None

    def get_embed(self, shape=None):
        gh, gw = shape if shape is not None else self.grid
        y, x = torch.meshgrid(torch.arange(gh, dtype=torch.float32), torch.arange(gw, dtype=torch.float32), indexing="ij")
        y, x = y.reshape(-1), x.reshape(-1)                               # [n], row-major like the patch embedding
        if self.kind == "axial":
            bands = self.temperature ** (-torch.arange(self.dim // 4, dtype=torch.float32) / (self.dim // 4))
            ang = torch.cat([y[:, None] * bands, x[:, None] * bands], -1)  # [n, D / 2]
        else:
            f = self.freqs.detach().float().cpu()
            ang = x[:, None] * f[:, :, None, :, 0] + y[:, None] * f[:, :, None, :, 1]   # [depth, H, n, D / 2]
        ang = torch.cat([ang, ang], -1) if self.half else ang.repeat_interleave(2, dim=-1)
        dev = self.freqs.device if self.freqs is not None else None
        return torch.cat([ang.sin(), ang.cos()], -1).to(dev)


def relative_position_index(gh: int, gw: int, class_token: bool) -> torch.Tensor:
    """timm gen_relative_position_index: [n, n] (n = gh * gw, + 1 with class_token) indices into a table whose row
    (dy + gh - 1) * (2 gw - 1) + (dx + gw - 1) holds the pair (query - key) = (dy, dx); with class_token three more rows: the class
    query against a patch key, a patch query against the class key, class against class"""
    ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    c = torch.stack([ys.reshape(-1), xs.reshape(-1)])                     # [2, n]
    rel = c[:, :, None] - c[:, None, :]                                   # [2, n, n]: query - key
    idx = (rel[0] + gh - 1) * (2 * gw - 1) + (rel[1] + gw - 1)
    if not class_token:
        return idx
    T = (2 * gh - 1) * (2 * gw - 1)
    out = torch.zeros(gh * gw + 1, gh * gw + 1, dtype=idx.dtype)
    out[1:, 1:] = idx
    out[0, 0:] = T
    out[0:, 0] = T + 1
    out[0, 0] = T + 2
    return out


class RelativePositionBias(nn.Module):
    """BEiT's shared bias (timm `RelativePositionBias`, the model's `rel_pos_bias`): forward() returns [H, N, N], N = gh * gw + 1.
    Written from memory of timm 1.x, unverified against an installed timm."""

    def __init__(self, window_size, num_heads: int):
        super().__init__()
        gh, gw = window_size
        self.window_size = (gh, gw)
        self.window_area = gh * gw
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * gh - 1) * (2 * gw - 1) + 3, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(gh, gw, True), persistent=False)

    def forward(self):
        n = self.window_area + 1
        return self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


class RelPosBias(nn.Module):
    """timm `RelPosBias` (the `rel_pos` of a vit_relpos attention, the `shared_rel_pos` of a vit_srelpos model): a table over the
    patch pairs alone, get_bias() returns [1, H, N, N] with zero rows and columns for the prefix tokens.  From memory of timm 1.x."""

    def __init__(self, window_size, num_heads: int, prefix_tokens: int = 0):
        super().__init__()
        gh, gw = window_size
        self.window_size = (gh, gw)
        self.window_area = gh * gw
        self.prefix_tokens = prefix_tokens
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * gh - 1) * (2 * gw - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(gh, gw, False), persistent=False)

    def get_bias(self):
        n = self.window_area
        b = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1)
        return F.pad(b, [self.prefix_tokens, 0, self.prefix_tokens, 0]).unsqueeze(0).contiguous()

    def forward(self, attn, shared_rel_pos=None):
        return attn + self.get_bias()


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int, qk_norm: bool = False, ln_eps: float = 1e-6, bias: bool = True,
                 rotate_half: bool = False, num_prefix_tokens: int = 1, eva: bool = False, qkv_split: bool = False,
                 rel_pos: str = "none", grid=None):
        super().__init__()
        if rel_pos == "beit":       # timm Beit Attention: the table, its index and _get_rel_pos_bias()
            gh, gw = grid
            self.window_size = (gh, gw)
            self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * gh - 1) * (2 * gw - 1) + 3, num_heads))
            self.register_buffer("relative_position_index", relative_position_index(gh, gw, True), persistent=False)
        elif rel_pos == "beit_shared":   # timm: the attributes exist and are None when the model owns the bias
            self.window_size, self.relative_position_bias_table, self.relative_position_index = None, None, None
        elif rel_pos == "relpos":   # timm RelPosAttention
            self.rel_pos = RelPosBias(grid, num_heads, prefix_tokens=num_prefix_tokens)
        elif rel_pos == "srelpos":
            self.rel_pos = None
        self.rotate_half = rotate_half                  # the pairing of a rotary table handed to forward (timm Eva's attribute)
        self.num_prefix_tokens = num_prefix_tokens      # rows in front that carry no position
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        if qkv_split:      # timm EvaAttention(qkv_fused=False): three projections, k without a bias
            self.qkv = None
            self.q_proj, self.k_proj, self.v_proj = nn.Linear(dim, dim, bias=bias), nn.Linear(dim, dim, bias=False), nn.Linear(dim, dim, bias=bias)
        else:
            self.qkv = nn.Linear(dim, dim * 3, bias=bias and not eva)
        if eva:            # timm EvaAttention: q and v biases as parameters beside a bias-free qkv (k's is a buffer of zeros)
            fused_bias = bias and not qkv_split
            self.q_bias = nn.Parameter(torch.zeros(dim)) if fused_bias else None
            self.v_bias = nn.Parameter(torch.zeros(dim)) if fused_bias else None
            self.norm = nn.Identity()      # (scale_norm=False: the inner attention norm of no released EVA02 checkpoint)
        self.q_norm = nn.LayerNorm(self.head_dim, eps=ln_eps) if qk_norm else nn.Identity()
        self.k_norm = nn.LayerNorm(self.head_dim, eps=ln_eps) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim, bias=bias)
        self.proj_drop = nn.Dropout(0.0)

    def _get_rel_pos_bias(self):
        """timm Beit Attention._get_rel_pos_bias: [1, H, N, N]"""
        n = self.window_size[0] * self.window_size[1] + 1
        b = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1)
        return b.permute(2, 0, 1).contiguous().unsqueeze(0)

    def forward(self, x, rope=None, shared_rel_pos_bias=None):
        B, N, C = x.shape
        if self.qkv is None:
            qkv = torch.stack([self.q_proj(x), self.k_proj(x), self.v_proj(x)], 2)
        elif getattr(self, "q_bias", None) is not None:
            qkv = F.linear(x, self.qkv.weight, torch.cat([self.q_bias, torch.zeros_like(self.q_bias), self.v_bias]))
        else:
            qkv = self.qkv(x)
        q, k, v = qkv.reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        if rope is not None:      # timm EvaAttention: behind q/k-norm, the prefix rows pass through
            P = self.num_prefix_tokens
            q = torch.cat([q[:, :, :P], apply_rot_embed_cat(q[:, :, P:], rope, self.rotate_half)], 2)
            k = torch.cat([k[:, :, :P], apply_rot_embed_cat(k[:, :, P:], rope, self.rotate_half)], 2)
        bias = None      # a learned relative position bias: the attention's own, the model's shared one, or (timm adds both) their sum
        if getattr(self, "relative_position_bias_table", None) is not None:
            bias = self._get_rel_pos_bias()
        elif getattr(self, "rel_pos", None) is not None:
            bias = self.rel_pos.get_bias()
        if shared_rel_pos_bias is not None:
            bias = shared_rel_pos_bias if bias is None else bias + shared_rel_pos_bias
        if bias is None:
            x = F.scaled_dot_product_attention(q, k, v)
        else:
            x = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.to(q.dtype))
        x = x.transpose(1, 2).reshape(B, N, C)
        if hasattr(self, "norm"):
            x = self.norm(x)
        return self.proj_drop(self.proj(x))


class LayerScale(nn.Module):
    def __init__(self, dim: int, init: float):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x) (OpenAI CLIP; timm / open_clip `QuickGELU`)"""

    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int, act: str = "gelu", bias: bool = True):
        super().__init__()
        if act not in ("gelu", "quick_gelu"):
            raise ValueError(f"act must be 'gelu' or 'quick_gelu', got {act!r}")
        self.fc1 = nn.Linear(dim, hidden, bias=bias)
        self.act = nn.GELU() if act == "gelu" else QuickGELU()
        self.drop1 = nn.Dropout(0.0)
        self.norm = nn.Identity()
        self.fc2 = nn.Linear(hidden, dim, bias=bias)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        return self.drop2(self.fc2(self.norm(self.drop1(self.act(self.fc1(x))))))


class GluMlp(nn.Module):
    """timm `GluMlp` (with act_layer=nn.SiLU and gate_last=False: `SwiGLUPacked`): one packed fc1 of 2 * hidden outputs,
    x1, x2 = fc1(x).chunk(2, -1); gate_last=False: act(x1) * x2, gate_last=True: x1 * act(x2)"""

    def __init__(self, dim: int, hidden: int, act_layer=nn.SiLU, gate_last: bool = False, bias: bool = True):
        super().__init__()
        self.chunk_dim = -1
        self.gate_last = gate_last
        self.fc1 = nn.Linear(dim, 2 * hidden, bias=bias)
        self.act = act_layer()
        self.drop1 = nn.Dropout(0.0)
        self.norm = nn.Identity()
        self.fc2 = nn.Linear(hidden, dim, bias=bias)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        x1, x2 = self.fc1(x).chunk(2, dim=self.chunk_dim)
        x = x1 * self.act(x2) if self.gate_last else self.act(x1) * x2
        return self.drop2(self.fc2(self.norm(self.drop1(x))))


class SwiGLU(nn.Module):
    """timm `SwiGLU`: the gate and the value projection apart, act(fc1_g(x)) * fc1_x(x)"""

    def __init__(self, dim: int, hidden: int, act_layer=nn.SiLU, bias: bool = True):
        super().__init__()
        self.fc1_g = nn.Linear(dim, hidden, bias=bias)
        self.fc1_x = nn.Linear(dim, hidden, bias=bias)
        self.act = act_layer()
        self.drop1 = nn.Dropout(0.0)
        self.norm = nn.Identity()
        self.fc2 = nn.Linear(hidden, dim, bias=bias)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        x = self.act(self.fc1_g(x)) * self.fc1_x(x)
        return self.drop2(self.fc2(self.norm(self.drop1(x))))


def make_mlp(cfg: "ViTConfig") -> nn.Module:
    if cfg.mlp == "swiglu_packed":
        mlp = GluMlp(cfg.embed_dim, cfg.hidden_dim, bias=cfg.bias)
    elif cfg.mlp == "swiglu":
        mlp = SwiGLU(cfg.embed_dim, cfg.hidden_dim, bias=cfg.bias)
    else:
        mlp = Mlp(cfg.embed_dim, cfg.hidden_dim, cfg.act, bias=cfg.bias)
    if cfg.mlp_norm:      # timm `norm_layer`: over the hidden width, between the activation (or the gate) and fc2
        mlp.norm = make_norm(cfg, cfg.hidden_dim)
    return mlp


class AttentionPoolLatent(nn.Module):
    """timm `AttentionPoolLatent` as `VisionTransformer(global_pool='map')` builds it (latent_len=1, no pool pos_embed, no
    q/k-norm, pool='token'): ONE learned query attends over every row of x, then proj and a residual MLP.  Written from memory of
    timm 1.x (timm is not importable here) - attribute names and forward are the contract the wrapper recognises."""

    def __init__(self, dim: int, num_heads: int, mlp_ratio: float = 4.0, ln_eps: float = 1e-6, act: str = "gelu"):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.pool = "token"
        self.latent_dim = dim
        self.latent_len = 1
        self.latent = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = None
        self.q = nn.Linear(dim, dim)
        self.kv = nn.Linear(dim, dim * 2)
        self.q_norm = nn.Identity()
        self.k_norm = nn.Identity()
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)
        self.norm = nn.LayerNorm(dim, eps=ln_eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), act)

    def forward(self, x):
        B, N, C = x.shape
        q = self.q(self.latent.expand(B, -1, -1)).reshape(B, self.latent_len, self.num_heads, self.head_dim).transpose(1, 2)
        kv = self.kv(x).reshape(B, N, 2, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        k, v = kv.unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        x = F.scaled_dot_product_attention(q, k, v)
        x = self.proj_drop(self.proj(x.transpose(1, 2).reshape(B, self.latent_len, C)))
        x = x + self.mlp(self.norm(x))
        return x[:, 0]      # pool == 'token'


class Block(nn.Module):
    def __init__(self, cfg: ViTConfig):
        super().__init__()
        C = cfg.embed_dim
        self.norm1 = make_norm(cfg, C)
        self.attn = Attention(C, cfg.num_heads, cfg.qk_norm, cfg.ln_eps, cfg.bias, rotate_half=cfg.rope_half,
                              num_prefix_tokens=cfg.num_prefix_tokens, eva=cfg.eva_block, qkv_split=cfg.qkv_split,
                              **(dict(rel_pos=cfg.rel_pos, grid=cfg.grid) if cfg.rel_pos != "none" else {}))
        gamma = lambda: nn.Parameter(cfg.layer_scale * torch.ones(C)) if cfg.layer_scale else None
        if cfg.eva_block:      # timm EvaBlock: the LayerScale vectors are parameters of the block, None without init_values
            self.gamma_1 = gamma()
        else:
            self.ls1 = LayerScale(C, cfg.layer_scale) if cfg.layer_scale else nn.Identity()
        self.drop_path1 = nn.Identity()
        self.norm2 = make_norm(cfg, C)
        self.mlp = make_mlp(cfg)
        if cfg.eva_block:
            self.gamma_2 = gamma()
        else:
            self.ls2 = LayerScale(C, cfg.layer_scale) if cfg.layer_scale else nn.Identity()
        self.drop_path2 = nn.Identity()

    def forward(self, x, rope=None, shared_rel_pos_bias=None):
        if shared_rel_pos_bias is not None or getattr(self.attn, "rel_pos", None) is not None or \
                getattr(self.attn, "relative_position_bias_table", None) is not None:
            # timm Beit Block / RelPosBlock: the model's shared bias (or None) goes to the attention beside x
            a = self.attn(self.norm1(x), shared_rel_pos_bias=shared_rel_pos_bias)
            g1, g2 = (getattr(self, "gamma_1", None), getattr(self, "gamma_2", None)) if not hasattr(self, "ls1") else (None, None)
            a = self.ls1(a) if hasattr(self, "ls1") else (a if g1 is None else g1 * a)
            x = x + self.drop_path1(a)
            h = self.mlp(self.norm2(x))
            h = self.ls2(h) if hasattr(self, "ls2") else (h if g2 is None else g2 * h)
            return x + self.drop_path2(h)
        if not hasattr(self, "ls1"):      # timm EvaBlock.forward
            a = self.attn(self.norm1(x)) if rope is None else self.attn(self.norm1(x), rope=rope)
            x = x + self.drop_path1(a if self.gamma_1 is None else self.gamma_1 * a)
            h = self.mlp(self.norm2(x))
            return x + self.drop_path2(h if self.gamma_2 is None else self.gamma_2 * h)
        x = x + self.drop_path1(self.ls1(self.attn(self.norm1(x)) if rope is None else self.attn(self.norm1(x), rope=rope)))
        x = x + self.drop_path2(self.ls2(self.mlp(self.norm2(x))))
        return x


class VisionTransformer(nn.Module):
    """timm-shaped ViT (class token, learned absolute pos-embed, pre-norm blocks)."""

    def __init__(self, cfg: ViTConfig):
        super().__init__()
        self.cfg = cfg
        self.num_classes = cfg.num_classes
        self.embed_dim = cfg.embed_dim
        self.num_prefix_tokens = cfg.num_prefix_tokens
        self.num_reg_tokens = cfg.reg_tokens
        self.no_embed_class = cfg.no_embed_class
        self.patch_embed = PatchEmbed(cfg)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, cfg.embed_dim)) if cfg.class_token else None   # timm: None
        self.reg_token = nn.Parameter(torch.zeros(1, cfg.reg_tokens, cfg.embed_dim)) if cfg.reg_tokens else None
        if cfg.distilled:      # timm VisionTransformerDistilled (a plain model has neither attribute, like timm's)
            self.dist_token = nn.Parameter(torch.zeros(1, 1, cfg.embed_dim))
            self.distilled_training = False
        n_pos = cfg.num_patches if cfg.no_embed_class else cfg.num_patches + cfg.num_prefix_tokens
        self.pos_embed = nn.Parameter(torch.zeros(1, n_pos, cfg.embed_dim)) if cfg.abs_pos else None
        g = cfg.img_size // cfg.patch_size
        self.rope = (RotaryEmbedding(cfg.head_dim, (g, g), cfg.rope, cfg.rope_half, cfg.num_heads, cfg.depth)
                     if cfg.rope != "none" else None)
        if cfg.rel_pos == "beit_shared":      # timm Beit(use_shared_rel_pos_bias=True)
            self.rel_pos_bias = RelativePositionBias(cfg.grid, cfg.num_heads)
        elif cfg.rel_pos == "beit":
            self.rel_pos_bias = None
        elif cfg.rel_pos == "srelpos":        # timm VisionTransformerRelPos(shared_rel_pos=True)
            self.shared_rel_pos = RelPosBias(cfg.grid, cfg.num_heads, prefix_tokens=cfg.num_prefix_tokens)
        elif cfg.rel_pos == "relpos":
            self.shared_rel_pos = None
        self.pos_drop = nn.Dropout(0.0)
        if cfg.global_pool not in ("token", "avg", "map"):
            raise ValueError(f"global_pool must be 'token', 'avg' or 'map', got {cfg.global_pool!r}")
        self.global_pool = cfg.global_pool
        # timm: an attn_pool attribute on every model, None unless global_pool == 'map'
        self.attn_pool = (AttentionPoolLatent(cfg.embed_dim, cfg.num_heads, cfg.mlp_ratio, cfg.ln_eps, cfg.act)
                          if cfg.global_pool == "map" else None)
        self.norm_pre = make_norm(cfg, cfg.embed_dim) if cfg.pre_norm else nn.Identity()
        self.blocks = nn.Sequential(*[Block(cfg) for _ in range(cfg.depth)])
        # timm: the final norm moves behind the pooling (fc_norm) when fc_norm is in use
        self.norm = nn.Identity() if cfg.use_fc_norm else make_norm(cfg, cfg.embed_dim)
        self.fc_norm = make_norm(cfg, cfg.embed_dim) if cfg.use_fc_norm else nn.Identity()
        self.head_drop = nn.Dropout(0.0)
        self.head = nn.Linear(cfg.embed_dim, cfg.num_classes) if cfg.num_classes > 0 else nn.Identity()   # timm num_classes=0
        if cfg.distilled:
            if cfg.global_pool != "token" or cfg.use_fc_norm:
                raise ValueError("a distilled model has a token head and no fc_norm")
            self.head_dist = nn.Linear(cfg.embed_dim, cfg.num_classes)

    def _pos_embed(self, x):
        # timm: prefix tokens [cls, reg...] in front; the pos-embed covers them unless no_embed_class
        prefix = [self.cls_token.expand(x.shape[0], -1, -1)] if self.cls_token is not None else []
        if self.reg_token is not None:
            prefix.append(self.reg_token.expand(x.shape[0], -1, -1))
        if self.cfg.distilled:
            prefix.append(self.dist_token.expand(x.shape[0], -1, -1))
        if self.pos_embed is None:
            x = torch.cat(prefix + [x], dim=1)
        elif self.no_embed_class:
            x = torch.cat(prefix + [x + self.pos_embed], dim=1)
        else:
            x = torch.cat(prefix + [x], dim=1) + self.pos_embed
        return self.pos_drop(x)

    def forward_features(self, x):
        x = self._pos_embed(self.patch_embed(x))
        x = self.norm_pre(x)
        if self.cfg.rel_pos != "none":      # timm Beit / VisionTransformerRelPos.forward_features
            shared = self.rel_pos_bias() if getattr(self, "rel_pos_bias", None) is not None else None
            if getattr(self, "shared_rel_pos", None) is not None:
                shared = self.shared_rel_pos.get_bias()
            for blk in self.blocks:
                x = blk(x, shared_rel_pos_bias=shared)
        elif self.rope is None:
            x = self.blocks(x)
        else:      # timm Eva.forward_features: the table (a per-block slice of a mixed one) goes to every block
            emb = self.rope.get_embed()
            for i, blk in enumerate(self.blocks):
                x = blk(x, rope=emb[i] if emb.dim() == 4 else emb)
        return self.norm(x)

    def forward(self, x):
        x = self.forward_features(x)
        if self.cfg.distilled:     # timm VisionTransformerDistilled.forward_head
            x, x_dist = self.head(self.head_drop(x[:, 0])), self.head_dist(self.head_drop(x[:, 1]))
            if self.distilled_training and self.training and not torch.jit.is_scripting():
                return x, x_dist
            return (x + x_dist) / 2
        if self.attn_pool is not None:      # timm forward_head: the pool reads every row, prefix rows included
            x = self.attn_pool(x)
        else:
            x = x[:, self.num_prefix_tokens:].mean(dim=1) if self.global_pool == "avg" else x[:, 0]
        return self.head(self.head_drop(self.fc_norm(x)))


# ----------------------------------------------------------------------------------------------
# deterministic synthetic weights
# ----------------------------------------------------------------------------------------------

def synth_state_dict(cfg: ViTConfig, seed: int = 0, std: float = 0.02,
                     bias_std: float = 0.0) -> Dict[str, np.ndarray]:
    """timm-named float32 state dict drawn from numpy PCG64(seed).

    `std` is the normal std of every linear / conv / pos-embed weight (timm's init is
    trunc_normal(.02)); parity fixtures use a larger std so importance scores are well
    separated (with std .02 the keep-boundary gap is ~1e-7).  LayerNorm gains
    are drawn around 1 and biases around 0 so that LN/bias code paths are exercised.
    """
    rng = np.random.default_rng(seed)
    C, Hd, P = cfg.embed_dim, cfg.hidden_dim, cfg.patch_size

    def nrm(*shape, s=std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(s)).astype(np.float32)

    sd: Dict[str, np.ndarray] = {}
    rms, lin_bias = cfg.norm == "rms", cfg.bias      # (an RmsNorm has no bias and a bias-free linear none: nothing is drawn)
    if cfg.class_token:      # (a model without one draws nothing in its place)
        sd["cls_token"] = nrm(1, 1, C)
    n_pos = cfg.num_patches if cfg.no_embed_class else cfg.num_patches + cfg.num_prefix_tokens
    if cfg.abs_pos:          # (a model without an absolute embedding draws nothing in its place)
        sd["pos_embed"] = nrm(1, n_pos, C)
    fan_in = cfg.in_chans * P * P
    sd["patch_embed.proj.weight"] = nrm(C, cfg.in_chans, P, P, s=1.0 / math.sqrt(fan_in))
    sd["patch_embed.proj.bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        for ln in ("norm1", "norm2"):
            sd[p + ln + ".weight"] = (1.0 + nrm(C, s=bias_std)).astype(np.float32)
            if not rms:
                sd[p + ln + ".bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
        sd[p + "attn.qkv.weight"] = nrm(3 * C, C)
        if lin_bias:
            sd[p + "attn.qkv.bias"] = nrm(3 * C, s=bias_std) if bias_std else np.zeros(3 * C, np.float32)
        sd[p + "attn.proj.weight"] = nrm(C, C)
        if lin_bias:
            sd[p + "attn.proj.bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
        if cfg.mlp == "swiglu":      # timm SwiGLU: gate, then value (a plain config draws exactly what it always drew)
            for fc in ("fc1_g", "fc1_x"):
                sd[p + f"mlp.{fc}.weight"] = nrm(Hd, C)
                if lin_bias:
                    sd[p + f"mlp.{fc}.bias"] = nrm(Hd, s=bias_std) if bias_std else np.zeros(Hd, np.float32)
        else:
            H1 = 2 * Hd if cfg.mlp == "swiglu_packed" else Hd   # packed: rows [0, Hd) the gate, [Hd, 2 Hd) the value
            sd[p + "mlp.fc1.weight"] = nrm(H1, C)
            if lin_bias:
                sd[p + "mlp.fc1.bias"] = nrm(H1, s=bias_std) if bias_std else np.zeros(H1, np.float32)
        sd[p + "mlp.fc2.weight"] = nrm(C, Hd)
        if lin_bias:
            sd[p + "mlp.fc2.bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
        if cfg.layer_scale:
            # a trained DeiT-3 has gammas of order 0.1-1; keep the configured init but jitter it
            # so the LayerScale multiply is observable in parity tests.
            sd[p + "ls1.gamma"] = (np.float32(cfg.layer_scale) + np.abs(nrm(C, s=0.5))).astype(np.float32)
            sd[p + "ls2.gamma"] = (np.float32(cfg.layer_scale) + np.abs(nrm(C, s=0.5))).astype(np.float32)
    if not cfg.use_fc_norm:
        sd["norm.weight"] = (1.0 + nrm(C, s=bias_std)).astype(np.float32)
        if not rms:
            sd["norm.bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
    if cfg.num_classes > 0:      # (timm num_classes=0: head is nn.Identity)
        sd["head.weight"] = nrm(cfg.num_classes, C)
        sd["head.bias"] = nrm(cfg.num_classes, s=bias_std) if bias_std else np.zeros(cfg.num_classes, np.float32)

    # the timm options' tensors are drawn AFTER everything above, so a config without them keeps its stream
    def ln(prefix, n):
        sd[prefix + ".weight"] = (1.0 + nrm(n, s=bias_std)).astype(np.float32)
        if affine_bias:
            sd[prefix + ".bias"] = nrm(n, s=bias_std) if bias_std else np.zeros(n, np.float32)

    affine_bias = not rms
    if cfg.pre_norm:
        ln("norm_pre", C)
    if cfg.qk_norm:      # (q/k-norm stays a LayerNorm whatever cfg.norm says)
        affine_bias = True
        for i in range(cfg.depth):
            ln(f"blocks.{i}.attn.q_norm", cfg.head_dim)
            ln(f"blocks.{i}.attn.k_norm", cfg.head_dim)
        affine_bias = not rms
    if cfg.use_fc_norm:
        ln("fc_norm", C)
    if cfg.reg_tokens:      # after every other draw: only pos_embed's row count differs from the register-free config
        sd["reg_token"] = nrm(1, cfg.reg_tokens, C)
    if cfg.distilled:       # after every other draw too; pos_embed's two extra rows were drawn with it, above
        sd["dist_token"] = nrm(1, 1, C)
        sd["head_dist.weight"] = nrm(cfg.num_classes, C)
        sd["head_dist.bias"] = nrm(cfg.num_classes, s=bias_std) if bias_std else np.zeros(cfg.num_classes, np.float32)
    if cfg.global_pool == "map":      # after every other draw: the attention pool (timm AttentionPoolLatent)
        p = "attn_pool."
        sd[p + "latent"] = nrm(1, 1, C, s=C ** -0.5)      # timm: trunc_normal_(std=latent_dim ** -0.5)
        for name, rows, cols in (("q", C, C), ("kv", 2 * C, C), ("proj", C, C)):
            sd[p + name + ".weight"] = nrm(rows, cols)
            sd[p + name + ".bias"] = nrm(rows, s=bias_std) if bias_std else np.zeros(rows, np.float32)
        ln(p + "norm", C)
        sd[p + "mlp.fc1.weight"] = nrm(Hd, C)
        sd[p + "mlp.fc1.bias"] = nrm(Hd, s=bias_std) if bias_std else np.zeros(Hd, np.float32)
        sd[p + "mlp.fc2.weight"] = nrm(C, Hd)
        sd[p + "mlp.fc2.bias"] = nrm(C, s=bias_std) if bias_std else np.zeros(C, np.float32)
    if cfg.embed_norm:      # after every other draw: the norm inside the patch embedding
        ln("patch_embed.norm", C)
    if cfg.rope == "mixed":      # after every other draw: per-block, per-head frequencies, radians per patch on each axis
        sd["rope.freqs"] = nrm(cfg.depth, cfg.num_heads, cfg.head_dim // 2, 2, s=1.0)
    if cfg.mlp_norm:             # after every other draw: the norm inside every MLP
        for i in range(cfg.depth):
            ln(f"blocks.{i}.mlp.norm", Hd)
    if cfg.rel_pos != "none":    # after every other draw: the bias tables.  A FIXTURE CHOICE: standard deviation 1, not timm's
        gh, gw = cfg.grid        # trunc_normal(.02), which would not move a logit - trained tables are of order one
        rows = (2 * gh - 1) * (2 * gw - 1) + (3 if cfg.rel_pos.startswith("beit") else 0)
        name = "relative_position_bias_table"
        if cfg.rel_pos == "beit_shared":
            sd["rel_pos_bias." + name] = nrm(rows, cfg.num_heads, s=1.0)
        elif cfg.rel_pos == "srelpos":
            sd["shared_rel_pos." + name] = nrm(rows, cfg.num_heads, s=1.0)
        else:
            for i in range(cfg.depth):
                sd[f"blocks.{i}.attn." + ("rel_pos." if cfg.rel_pos == "relpos" else "") + name] = nrm(rows, cfg.num_heads, s=1.0)
    # Eva's spellings draw nothing: the tensors above under the names the modules have.  The packed qkv's rows are q, k, v in
    # that order; k has no bias in either spelling, and the values drawn for it are dropped
    for i in range(cfg.depth if (cfg.eva_block or cfg.qkv_split) else 0):
        p = f"blocks.{i}."
        bias = sd.pop(p + "attn.qkv.bias", None)
        if cfg.qkv_split:
            wq, wk, wv = np.split(sd.pop(p + "attn.qkv.weight"), 3)
            sd[p + "attn.q_proj.weight"], sd[p + "attn.k_proj.weight"], sd[p + "attn.v_proj.weight"] = wq.copy(), wk.copy(), wv.copy()
            if bias is not None:
                sd[p + "attn.q_proj.bias"], sd[p + "attn.v_proj.bias"] = bias[:C].copy(), bias[2 * C:].copy()
        elif bias is not None:
            sd[p + "attn.q_bias"], sd[p + "attn.v_bias"] = bias[:C].copy(), bias[2 * C:].copy()
        if cfg.eva_block and cfg.layer_scale:
            sd[p + "gamma_1"], sd[p + "gamma_2"] = sd.pop(p + "ls1.gamma"), sd.pop(p + "ls2.gamma")
    return sd


def bf16_round_np(a: np.ndarray) -> np.ndarray:
    """Round a float32 array to the nearest bf16-representable float32 (RNE)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def create_model(name_or_cfg, seed: int = 0, std: float = 0.02, bias_std: float = 0.0,
                 round_bf16: bool = False) -> VisionTransformer:
    """Build a timm-shaped ViT with deterministic synthetic weights.

    `round_bf16=True` rounds every weight to a bf16-representable value while keeping the
    parameters in fp32, so that an fp32 oracle and a bf16 device model see identical weights.
    """
    cfg = config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg
    model = VisionTransformer(cfg)
    sd = synth_state_dict(cfg, seed=seed, std=std, bias_std=bias_std)
    if round_bf16:
        sd = {k: bf16_round_np(v) for k, v in sd.items()}
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return model.eval()


def state_dict_numpy(model: nn.Module) -> Dict[str, np.ndarray]:
    """float32 numpy copy of a (timm-shaped) model's state dict."""
    return {k: v.detach().to(torch.float32).cpu().numpy() for k, v in model.state_dict().items()}
