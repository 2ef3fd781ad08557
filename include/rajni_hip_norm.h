/* RMSNorm trunks and a norm inside the patch embedding (timm `PatchEmbed.norm`, `embed_norm_layer`): the AIMv2 image towers.
 * Additive to rajni_hip.h: no record, enum value, entry point or workspace size of that header (or of rajni_hip_layers.h /
 * rajni_hip_image.h / rajni_hip_query.h / rajni_hip_attnpool.h) changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * The models (the AIMv2 arguments are written from memory of timm 1.x; unverified against an installed timm): RmsNorm(eps=1e-5)
 * for norm1, norm2, norm and patch_embed.norm, a split SwiGLU MLP, no class token, global_pool='avg' without fc_norm, no bias
 * in qkv / proj / the MLP.
 *
 * RMSNorm over the last axis of a row x[0..C-1] with weight w and no bias, statistics in fp32:
 *     rstd = rsqrt((1 / C) * sum_c x[c]^2 + eps)        eps inside the square root
 *     y[c] = (x[c] * rstd) * w[c]                        rounded once to the output dtype
 * The sum runs in the order of the LayerNorm kernels' sums - a lane's 8-element chunks in order, then the 6-step wave butterfly -
 * so the same row gives the same bits at any batch size and batch position.  No mean is computed and no bias pointer is read.
 *
 * One forward has ONE norm kind: it applies to norm1, norm2, norm, fc_norm, norm_pre and the patch-embedding norm.  q/k-norm
 * (rajni_vit_ext.qk_norm) stays a LayerNorm whatever the kind.
 *
 * The patch-embedding norm, applied to the projected patch rows before the position embedding is added:
 *     x[b, P + j] = embed_norm(conv(patch j) + conv_bias) + pos[pos_off + j]
 * The P prefix rows (class token, registers, distillation token) are not normalised.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`).  A pointer below its minimum is
 * refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL optional pointer is aligned.
 *   rajni_norm_rows: x 16, w 16, b 16, y 16
 *   rajni_embed_norm: x 16, w 16, b 16, pos 16
 *   rajni_vit_forward_norm: images 16, logits 16
 *   rajni_vit_norm: embed_norm_w 16, embed_norm_b 16
 * (end of the placement table) */
#ifndef RAJNI_HIP_NORM_H
#define RAJNI_HIP_NORM_H

#include "rajni_hip_attnpool.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RAJNI_NORM_LAYERNORM = 0, RAJNI_NORM_RMS = 1 };

/* Beside the plan and the other records; NULL or all zero: LayerNorm everywhere and no patch-embedding norm.  With kind
 * RAJNI_NORM_RMS every `*_b` norm pointer of the plan, the blocks and the ext record (norm_b, norm1_b, norm2_b, norm_pre_b,
 * fc_norm_b) is not read and may be NULL. */
typedef struct {
  int kind;                       /* every norm of the forward except q/k-norm */
  float embed_norm_eps;
  const float* embed_norm_w;      /* [C] fp32, NULL: no patch_embed.norm */
  const float* embed_norm_b;      /* [C] fp32 or NULL (= 0); not read when kind is RMS */
} rajni_vit_norm;

/* rajni_layernorm with the kind named: y[r] = norm(x[r]) for `rows` rows of C elements, x rows `x_row_stride` elements apart
 * (fp32 when x_f32, else `dtype`), y dense in `dtype`.  RAJNI_NORM_LAYERNORM is rajni_layernorm's launch and bits.  RAJNI_NORM_RMS
 * runs the same kernels' RMS forms under the same choice (two rows per wave for fp32 rows with a 16-bit output, C <= 1024 and
 * rows >= 4096) and does not read b, which may be NULL.  C % 8 == 0, C <= 2048, x_row_stride % 8 == 0.  Any other kind is
 * RAJNI_ERR_INVALID.  Placement: x 16, w 16, b 16, y 16. */
int rajni_norm_rows(int kind, const void* x, long x_row_stride, const float* w, const float* b, void* y, int rows, int C,
                    float eps, int dtype, int x_f32, rajni_stream_t stream);

/* The patch-embedding norm alone, in place on the stream x [B, N, C] (fp32 when x_f32, else `dtype`): for every image b and
 * patch row j in [0, N - num_prefix)
 *     x[b, num_prefix + j] = norm(x[b, num_prefix + j]) + pos[pos_off + j]
 * with pos [pos_off + N - num_prefix, C] in `dtype`; the sum is formed in fp32 and rounded once to the stream's type.  Prefix
 * rows are neither read nor written.  One wave per row, 16-byte accesses.  kind RMS does not read b; kind LAYERNORM takes a NULL
 * b as 0.  C % 8 == 0, C <= 2048, 0 <= num_prefix <= RAJNI_MAX_PREFIX < N.  Placement: x 16, w 16, b 16, pos 16. */
int rajni_embed_norm(int kind, void* x, const float* w, const float* b, const void* pos, int pos_off, int B, int N,
                     int num_prefix, int C, float eps, int dtype, int x_f32, rajni_stream_t stream);

/* rajni_vit_forward_pool plus the record.  norm == NULL or all zero: exactly the launches of rajni_vit_forward_pool and the same
 * bits.  kind RAJNI_NORM_RMS: every norm launch of the forward (norm1, norm2, norm_pre, the final norm in each of its forms -
 * head rows, pooled, every token, dense, the dropped rows of RAJNI_POOL_DENSE_LAST - and fc_norm) is the RMS form of the same
 * kernel; the null-pointer checks that ask for the `*_b` vectors are relaxed for that kind only.  embed_norm_w != NULL: the patch
 * GEMM adds a zeroed position table (carved from the second stream buffer, idle until the first pruned block; the prefix rows
 * of that table are the real ones) and rajni_embed_norm follows it, in front of norm_pre.  A plan without an embedding norm
 * issues exactly the launches it issued before.
 * Refused before the first launch, each naming the combination: any other kind (RAJNI_ERR_INVALID); RMS or an embedding norm
 * with plan.act_fp8, RMS or an embedding norm with an attention-pool record, RMS with layers.norm = 1 (RAJNI_ERR_UNSUPPORTED;
 * layers.norm = 0 slabs are cast-only and work with both kinds).
 * The workspace is rajni_vit_workspace_bytes_norm(...) bytes - the record adds nothing to rajni_vit_workspace_bytes_pool's
 * size; 0 = refused, with rajni_last_error holding the refusal.
 * Placement: as rajni_vit_forward_pool, and embed_norm_w / embed_norm_b 16. */
size_t rajni_vit_workspace_bytes_norm(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                      const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm);
int rajni_vit_forward_norm(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                           const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                           const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const void* images, void* logits,
                           rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_NORM_H */
