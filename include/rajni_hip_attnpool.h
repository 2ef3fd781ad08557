/* Attention-pool heads: timm's `global_pool='map'` (AttentionPoolLatent), the head of the SigLIP image towers.  Additive to
 * rajni_hip.h: no record, enum value, entry point or workspace size of that header (or of rajni_hip_layers.h / rajni_hip_image.h /
 * rajni_hip_query.h) changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * The module (written from memory of timm 1.x; unverified against an installed timm): ONE learned query row `latent` [1, 1, C]
 * attends over ALL N rows of norm(x), prefix rows included -
 *     q       = q_lin(latent) . reshape(Hp, Dp)                       the same for every image
 *     k, v    = kv_lin(norm(x)) . reshape(B, N, 2, Hp, Dp)            output laid out [2][Hp][Dp]
 *     o[b, h] = softmax_n(scale * q[h] . k[b, n, h]) @ v[b, :, h]     scale = Dp ** -0.5
 *     y       = proj(o . reshape(B, C));  y = y + fc2(act(fc1(pool_norm(y))))          [B, C]
 * and timm's forward_head goes on with fc_norm and head.  The pool's q_norm / k_norm are Identity, latent_len is 1 and it has
 * no position embedding of its own: anything else is not this record.  On the pruned graph N is the number of tokens that
 * survive the last block, so the kv projection and the pool shrink with the schedule.
 *
 * The query never depends on the image: the caller passes it ready, `q` [Hp, Dp] fp32 = (q_lin(latent)) * scale, computed once
 * per set of weights.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`).  A pointer below its minimum is
 * refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL optional pointer is aligned.
 *   rajni_attention_pool: kv 16, q 16, out 16
 *   rajni_vit_forward_pool: images 16, logits 16
 *   rajni_vit_attn_pool: q 16, kv_w 16, kv_b 16, proj_w 16, proj_b 16, norm_w 16, norm_b 16, fc1_w 16, fc1_b 16, fc2_w 16, fc2_b 16
 * (end of the placement table) */
#ifndef RAJNI_HIP_ATTNPOOL_H
#define RAJNI_HIP_ATTNPOOL_H

#include "rajni_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rajni_vit_ext.pool, beside RAJNI_POOL_TOKEN .. RAJNI_POOL_DENSE_LAST (5).  4 stays unknown.  Legal through
 * rajni_vit_forward_pool with a record only: every other entry point refuses it as the unknown pool value it is there. */
enum { RAJNI_POOL_MAP = 6 };

/* The pool's weights, beside the plan and the other records.  kv_w is in the plan's dtype (the kv GEMM runs on all B * N
 * surviving rows, like a block's qkv).  Everything behind the pool kernel runs on B rows and in FP32 whatever the plan's dtype -
 * the kernel's output, proj, the pool LayerNorm, FC1, the activation, FC2 and the residual - so proj_w, fc1_w and fc2_w are FP32
 * matrices (the values the model dtype holds, widened); the pooled row is rounded to the plan's dtype once, where fc_norm / the
 * head reads it.  (A 16-bit rounding of a pooled row costs 0.2 - 0.4 % of the logit scale and the 16-bit tail had five;
 * DESIGN.md section 1, B7.)  All matrices are packed as every rajni_linear weight is (rows padded up to a multiple of 256;
 * fc1_w / fc2_w with `hidden` zero-padded to whole 64-wide K steps, the padding rows of fc1 with zero bias: act(0) = 0 lands in
 * the padding columns and fc2's zero columns ignore them).  Biases and LayerNorm vectors are fp32; a NULL bias is 0.  No e4m3
 * form: the pool stays as it is next to e4m3 block weights, as the head does. */
typedef struct {
  const float* q;                              /* [heads, C / heads] fp32: q_lin(latent) * scale */
  const void* kv_w; const float* kv_b;         /* [2C(pad), C] in the plan's dtype, [2C]: K rows first, then V rows */
  const void* proj_w; const float* proj_b;     /* [C(pad), C] FP32, [C] */
  const float* norm_w; const float* norm_b;    /* the pool's own LayerNorm in front of its MLP, [C] */
  float norm_eps;
  const void* fc1_w; const float* fc1_b;       /* [hidden(pad), C] FP32, [hidden] */
  const void* fc2_w; const float* fc2_b;       /* [C(pad), hidden] FP32, [C] */
  int hidden;                                  /* the pool MLP's width, a multiple of 64 (zero-padded, above) */
  int heads;                                   /* Hp: C % heads == 0 and C / heads a multiple of 8 in 8..128 */
  int act;                                     /* RAJNI_MLP_GELU or RAJNI_MLP_QUICK_GELU: the pool MLP's activation */
} rajni_vit_attn_pool;

/* The pool's attention alone: out[b, h * D + d] = sum_n softmax_n(q[h] . kv[b, n, h * D : (h + 1) * D])[n] * kv[b, n, C + h * D + d],
 * C = H * D.  kv [B, N, 2C] in `dtype` (K half, then V half: what the kv GEMM writes), q [H, D] fp32 with the scale folded
 * in, out [B, C] in `dtype`.  Logits, softmax (maximum subtracted) and the weighted sum are fp32, rounded once to `dtype`.
 * One workgroup per (image, head); its lanes are split into a fixed number of token slots that depends on D alone, slot s
 * takes tokens s, s + S, s + 2S ... in order with an online softmax, and the slots are merged in slot order: the summation
 * order depends on (N, D) alone, there are no atomics, and an image gives the same bits at any batch size and batch
 * position.  LDS use does not grow with N.  N >= 1 (any N the buffers hold), D % 8 == 0 and 8 <= D <= 128,
 * B <= RAJNI_MAX_GRID_YZ; inputs are finite.  Placement: kv 16, q 16, out 16. */
int rajni_attention_pool(const void* kv, const float* q, void* out, int B, int N, int H, int D, int dtype, rajni_stream_t stream);

/* rajni_vit_forward_query plus the record.  pool == NULL: exactly the launches of rajni_vit_forward_query and the same bits
 * (and so ext.pool == RAJNI_POOL_MAP is refused there).  With a record ext.pool must be RAJNI_POOL_MAP (else RAJNI_ERR_INVALID,
 * naming ext.pool) and the tail behind the last block is
 *   final norm on all B * N rows -> kv GEMM (into the qkv workspace, dead behind the last block) -> rajni_attention_pool ->
 *   proj on B rows -> the pool's LayerNorm -> FC1 + act -> FC2 + residual (all four fp32) -> fc_norm (when ext.fc_norm_w; else
 *   one rounding to the plan's dtype) -> head GEMM,
 * or on a headless plan the caller's buffer [B, C] instead of the head GEMM.  Everything in front of the tail is
 * rajni_vit_forward_query's; the last block always runs every row.  Works with and without a class row
 * (query.class_token), registers, every mlp_act, e4m3 block weights, the 16-bit stream, the layers record and the image
 * record.  Refused before the first launch, each naming its field: ext.norm_absent (RAJNI_ERR_UNSUPPORTED: the pool reads
 * norm(x) and there is no cast-only row kernel), plan.cls_only_last_block (RAJNI_ERR_INVALID: that opt-in never forms the
 * rows to be pooled), plan.act_fp8 and prefix.head_rows == 2 (RAJNI_ERR_UNSUPPORTED), a NULL weight, pool.hidden,
 * pool.heads, pool.act out of range (RAJNI_ERR_INVALID).
 * The workspace is rajni_vit_workspace_bytes_pool(...) bytes: rajni_vit_workspace_bytes_query's (unchanged, in front) plus
 * the fp32 B-row intermediates of the pool ([B, C] three times and [B, hidden]); pool == NULL returns exactly rajni_vit_workspace_bytes_query's size.  0 = refused:
 * the size functions run the forward's own checks of the records that size the workspace (prefix, image, query, pool.hidden)
 * and the forward's own carve, so a non-zero size is the byte count the forward asks for.
 * Placement: as rajni_vit_forward_query, and the record's pointers 16. */
size_t rajni_vit_workspace_bytes_pool(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                      const rajni_vit_query* query, const rajni_vit_attn_pool* pool);
int rajni_vit_forward_pool(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                           const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                           const rajni_vit_attn_pool* pool, const void* images, void* logits, rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_ATTNPOOL_H */
