"""Yardsticks for attention-pool heads (timm `global_pool='map'`, AttentionPoolLatent; include/rajni_hip_attnpool.h), pure
numpy / torch-CPU, shared by tests/test_attnpool_cpu.py and the tests/test_gpu_attnpool_*.py files.

The reference cannot run such a model, and timm is not installed: the pool is restated here from the contract the header
states, independently of rajni_amd.timm_shaped.AttentionPoolLatent (no module, no scaled_dot_product_attention):
    q = q_lin(latent) . [H, D];  k, v = kv_lin(x) . [B, N, 2, H, D];  o[b, h] = softmax_n(D^-0.5 q[h] . k[b, n, h]) @ v[b, :, h]
    y = proj(o);  y = y + fc2(act(fc1(norm(y))))
over ALL N rows of norm(x), prefix rows included.  The trunk is tests/numerics_noclass.py::vit_forward_restated."""
from __future__ import annotations

import math

import numpy as np
import torch

import numerics as nm
import numerics_noclass as nq
from numerics_variants import _t, _ln

# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
KV_KINDS = ["normal", "big", "equal"]


def pool_attention(kv, q):
    """kv [B, N, 2C] and q [H, D] (the scale folded in) -> (out [B, C], A [B, C] = softmax |v|, s [B, H, N] the logits), fp64"""
    kv, q = np.asarray(kv, np.float64), np.asarray(q, np.float64)
    B, N, C2 = kv.shape
    H, D = q.shape
    assert C2 == 2 * H * D
    t = kv.reshape(B, N, 2, H, D)
    s = np.einsum("hd,bnhd->bhn", q, t[:, :, 0])
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    out = np.einsum("bhn,bnhd->bhd", p, t[:, :, 1]).reshape(B, H * D)
    A = np.einsum("bhn,bnhd->bhd", p, np.abs(t[:, :, 1])).reshape(B, H * D)
    return out, A, s


def pool_attention_budget(kv, q, dt):
    """(want, budget) [B, C] in the style of numerics.attention_budget, for a kernel that keeps P in fp32:
        |err| <= u_out |want| + (u32 + 2 N u32 + 4 ds + 8 u32 spread) A + floor
    u_out: the one rounding of the output (u32 for fp32).  A = softmax |v|.  2 N u32: numerator and denominator are sums of N
    fp32 terms in SOME fixed order - the worst case of any order is (N - 1) u32 of the sum of magnitudes each.
    ds = (D + 4) u32 max_n sum_d |q_d k_nd|: the logit's fp32 accumulation (D products, the adds between lane groups, the
    change of base), which exp turns into a relative error of p; 4 = numerator and denominator, twice for the exp2 argument's
    own rounding.  8 u32 spread, spread = max_n |s_n - max s|: the exp2 argument s - m carries a rounding error relative to
    its own magnitude, the hardware exp2 is accurate to about an ulp, and an online softmax rescales by exp2 of differences of
    at most that size."""
    want, A, s = pool_attention(kv, q)
    kv64, q64 = np.asarray(kv, np.float64), np.asarray(q, np.float64)
    B, N, _ = kv64.shape
    H, D = q64.shape
    sabs = np.einsum("hd,bnhd->bhn", np.abs(q64), np.abs(kv64.reshape(B, N, 2, H, D)[:, :, 0])).max(axis=-1)     # [B, H]
    spread = np.abs(s - s.max(axis=-1, keepdims=True)).max(axis=-1)                                              # [B, H]
    fac = nm.U32 + 2 * N * nm.U32 + 4 * (D + 4) * nm.U32 * sabs + 8 * nm.U32 * spread
    fac = np.repeat(fac[:, :, None], D, axis=-1).reshape(B, H * D)
    return want, nm.UNIT[dt] * np.abs(want) + fac * A + nm.FLOOR[dt]


def pool_operands(kind, B, N, H, D, dt, seed=0):
    """(kv [B, N, 2C] fp32 values of type dt, q [H, D] fp32):
    normal   K and V standard normal, q normal / sqrt(D): logits of order 1
    big      K rows = a_n u_h + 0.1 noise with q_h . u_h = 1 and a_n spread over [-80, 80]: logits of about +-80 - without the
             maximum subtracted exp overflows (e^80) or the whole row underflows
    equal    every K row of an image the same row: all logits equal, the output is the plain mean of V"""
    rng = np.random.default_rng([seed, B, N, H, D, KV_KINDS.index(kind)])
    q = (rng.standard_normal((H, D), dtype=np.float32) / np.float32(math.sqrt(D))).astype(np.float32)
    t = rng.standard_normal((B, N, 2, H, D), dtype=np.float32)
    if kind == "big":
        u = q / (q * q).sum(axis=-1, keepdims=True)
        a = rng.uniform(-80.0, 80.0, size=(B, N, H, 1)).astype(np.float32)
        a[:, 0] = 80.0
        a[:, N // 2] = -80.0 if N > 1 else 80.0
        t[:, :, 0] = a * u[None, None] + 0.1 * t[:, :, 0]
    elif kind == "equal":
        t[:, :, 0] = t[:, :1, 0]
    return nm.round_to(t.reshape(B, N, 2 * H * D), dt), q


# ---- the module and the whole forward ---------------------------------------------------------------------------------------------

def attn_pool_restated(sd, x, cfg, dtype=torch.float64, prefix="attn_pool."):
    """x [B, N, C] torch (norm(x) of the tokens that reach the head) -> [B, C]: the pool from its state-dict entries alone"""
    W = lambda n: _t(sd[prefix + n], dtype)
    B, N, C = x.shape
    H, D = cfg.num_heads, cfg.head_dim
    q = (W("latent").reshape(1, C) @ W("q.weight").T + W("q.bias")).reshape(H, D) * D ** -0.5
    kv = (x @ W("kv.weight").T + W("kv.bias")).reshape(B, N, 2, H, D)
    s = torch.einsum("hd,bnhd->bhn", q, kv[:, :, 0])
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    p = p / p.sum(dim=-1, keepdim=True)
    o = torch.einsum("bhn,bnhd->bhd", p, kv[:, :, 1]).reshape(B, C)
    y = o @ W("proj.weight").T + W("proj.bias")
    h = _ln(y, sd, prefix + "norm", cfg.ln_eps, dtype) @ W("mlp.fc1.weight").T + W("mlp.fc1.bias")
    h = h * torch.sigmoid(1.702 * h) if cfg.act == "quick_gelu" else 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return y + h @ W("mlp.fc2.weight").T + W("mlp.fc2.bias")


def vit_forward_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64, query=None, pooled=False):
    """(logits [B, classes] numpy - or with `pooled` the [B, C] row the head reads -, token counts, trace) of the pruned graph
    of a global_pool='map' model: the trunk is numerics_noclass.vit_forward_restated(features="tokens") - norm(x) of the
    surviving tokens -, then the pool over all of them, fc_norm where the config has one, and the head"""
    assert cfg.global_pool == "map" and "norm.weight" in sd
    tokens, counts, trace = nq.vit_forward_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype, query=query,
                                                    features="tokens")
    y = attn_pool_restated(sd, torch.from_numpy(tokens).to(dtype), cfg, dtype)
    if cfg.use_fc_norm:
        y = _ln(y, sd, "fc_norm", cfg.ln_eps, dtype)
    if not pooled:
        y = y @ _t(sd["head.weight"], dtype).T + _t(sd["head.bias"], dtype)
    return y.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy(), counts, trace


# ---- fixtures whose selections cannot hinge on a near-tie ---------------------------------------------------------------------
SCHED = nq.SCHED
FIX_BASE = nq.FIX_BASE
GAP_FACTOR = nq.GAP_FACTOR
MICRO = ["vit_micro_map_patch16_64", "vit_micro_cls_map_patch16_64", "vit_micro_reg4_map_d80_patch16_64",
         "vit_micro_map_patch16_400", "vit_micro512_map_patch16_64"]
# (weight seed, image seed) per micro config, found by tests/test_attnpool_cpu.py::search_seeds as numerics_noclass.SEEDS was:
# among the weight seeds tried, the one whose smallest keep-boundary gap - over the images of the B = 3 batch (image 0 is the
# B = 1 batch) and both scheduled blocks, in the fp64 restatement with the model's default query - is the largest multiple of
# the bf16 score budget; tests/test_attnpool_cpu.py asserts at least GAP_FACTOR of the committed seeds.  (The trunk draws the
# pool's weights last, so the selections do not depend on them.)  Found: 26 x, 39 x, 17 x and 43 x.
SEEDS = {
    "vit_micro_map_patch16_64": (45, 49),
    "vit_micro_cls_map_patch16_64": (15, 19),
    "vit_micro_reg4_map_d80_patch16_64": (37, 41),
    "vit_micro512_map_patch16_64": (41, 45),
}
# The 625-token model cannot have such a seed: block 1 ranks 625 scores and keeps 468, so neighbouring scores at the boundary
# lie about 1 / 625 of their size apart while the bf16 budget is 2^-8 of it - the best of weight seeds 1..24 leaves 0.43 x.
# Its free-running test therefore follows tests/test_gpu_long_forward.py, the project's rule for the 626-token models: the
# device's selections must be the restated rule on the device's OWN traced scores, and the restated graph runs on them.
LONG_SEEDS = {"vit_micro_map_patch16_400": (10, 14)}


def images_of(cfg, B, seed, size=None):
    return nq.images_of(cfg, B, seed, size)
