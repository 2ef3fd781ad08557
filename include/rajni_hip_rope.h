/* Rotary position embeddings (RoPE) on the pruned token set: q and k rotated by where each token sat in the image (EVA02, timm's
 * vit_*_rope_* line, the Perception Encoder towers, DINOv3).
 * Additive to rajni_hip.h: no record, enum value, entry point or workspace size of that header (or of rajni_hip_layers.h /
 * rajni_hip_image.h / rajni_hip_query.h / rajni_hip_attnpool.h / rajni_hip_norm.h) changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * The native layer is table driven and knows nothing about frequency schemes: the caller hands over cos and sin, fp32,
 * [rows, D] each, one row per patch of the grid (rows = grid height * grid width, row-major as the patch embedding emits them).
 *
 * The rule, in place on the q and k thirds of qkv [B * N, 3, H, D], arithmetic in fp32, the result rounded once to `dtype`:
 *     y[j] = x[j] * cos[p][j] + s(j) * x[partner(j)] * sin[p][j]
 *     RAJNI_ROPE_INTERLEAVED (0): partner(j) = j ^ 1,          s = -1 for even j, +1 for odd      (timm rot(): pairs (2i, 2i+1))
 *     RAJNI_ROPE_HALF        (1): partner(j) = (j + D/2) % D,   s = -1 for j < D/2, +1 otherwise   (rotate_half)
 * No structure of the tables is assumed (not cos[2i] == cos[2i+1], nor any other).  The v third is neither read nor written.
 * The first num_prefix rows of every image (class, register and distillation tokens carry no position) are neither read nor
 * written.  For row t >= num_prefix of image b the position is
 *     p = (src ? src[b * N + t] : t) - num_prefix
 * where src [B, N] int32 is the map into the unpruned sequence that the forward composes from the blocks' selections.
 *
 * head_stride, in elements: 0 = one table shared by all heads (axial RoPE), rows * D = one table per head, head h at
 * cos + h * head_stride.  In the forward record block_stride is 0, or (head_stride ? H : 1) * rows * D = one table (set) per
 * block (mixed RoPE), block i at cos + i * block_stride.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`).  A pointer below its minimum is
 * refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL optional pointer is aligned.
 *   rajni_rope_qk: qkv 16, src 4, cos 16, sin 16
 *   rajni_vit_forward_rope: images 16, logits 16
 *   rajni_vit_rope: cos 16, sin 16
 * (end of the placement table) */
#ifndef RAJNI_HIP_ROPE_H
#define RAJNI_HIP_ROPE_H

#include "rajni_hip_norm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RAJNI_ROPE_INTERLEAVED = 0, RAJNI_ROPE_HALF = 1 };

/* Beside the plan and the other records; NULL or all zero: no rotation. */
typedef struct {
  const float* cos;               /* [blocks or 1][H or 1][rows, D] fp32 */
  const float* sin;               /* the same shape */
  long long head_stride;          /* elements: 0 or rows * D */
  long long block_stride;         /* elements: 0 or (head_stride ? H : 1) * rows * D */
  int rows;                       /* patches of the grid: must equal the forward's n0 - P */
  int layout;                     /* RAJNI_ROPE_INTERLEAVED or RAJNI_ROPE_HALF */
} rajni_vit_rope;

/* The kernel alone: the rule above on qkv [B * N, 3, H, D] in `dtype` (bf16 / fp16 / fp32), in place.  src [B, N] int32 or NULL
 * (position = row index).  One wave per token walks its 2H q and k heads, 16 bytes per lane; a shared table row is loaded once
 * per token.  D % 8 == 0, 8 <= D <= 128; 0 <= num_prefix <= RAJNI_MAX_PREFIX, num_prefix < N; head_stride >= 0 and a multiple of 4.
 * THIS ENTRY POINT DOES NOT VALIDATE src: it has no row count to hold it against.  Every src[b * N + t] - num_prefix with
 * t >= num_prefix must lie in [0, rows) of the tables handed over, or the kernel reads outside them.  (In the forward a
 * position outside the grid cannot occur: the map is composed of selections over the grid's own tokens.)
 * Placement: qkv 16, src 4, cos 16, sin 16. */
int rajni_rope_qk(void* qkv, const int32_t* src, const float* cos, const float* sin, long long head_stride, int B, int N,
                  int num_prefix, int H, int D, int layout, int dtype, rajni_stream_t stream);

/* rajni_vit_forward_norm plus the record.  rope == NULL or all zero: exactly the launches of rajni_vit_forward_norm and the same
 * bits.  Otherwise every block rotates q and k behind q/k-norm and in front of everything that reads them - scoring in all its
 * forms, the three last-block forms, attention - so importance is computed from the rotated q and k, the ones attention itself
 * uses (a mean query averages the rotated queries).  Before the first scheduled block the position is the row index; behind one
 * the forward composes the selections into a map of B * n0 * 4 bytes in the workspace, refreshed only when the token set has
 * changed.  Composes with every other record.
 * Refused before the first launch, each naming the combination: a layout other than 0 or 1, NULL cos or sin with a non-zero
 * record, rows != n0 - P, a head_stride other than 0 or rows * D, a block_stride other than 0 or (head_stride ? H : 1) * rows * D
 * (RAJNI_ERR_INVALID); RoPE with plan.act_fp8 (RAJNI_ERR_UNSUPPORTED).
 * The workspace is rajni_vit_workspace_bytes_rope(...) bytes: rajni_vit_workspace_bytes_norm's plus the map (nothing without a
 * record); 0 = refused, with rajni_last_error holding the refusal.
 * Placement: as rajni_vit_forward_norm, and cos / sin 16. */
size_t rajni_vit_workspace_bytes_rope(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                      const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                      const rajni_vit_rope* rope);
int rajni_vit_forward_rope(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                           const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                           const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                           const void* images, void* logits, rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_ROPE_H */
