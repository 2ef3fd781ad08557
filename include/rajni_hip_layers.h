/* Intermediate-layer features of the whole forward: the states behind several blocks, each scattered back to the unpruned
 * sequence, from ONE forward.  Additive to rajni_hip.h: no record, enum, entry point or workspace size of that header
 * changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * For the capture list c_0 < c_1 < ... < c_{n-1} of block indices, slab l is [B, P + n0, C] in the plan's dtype (P prefix
 * tokens first, then the n0 patch positions of the unpruned sequence).  With x_after_c the residual stream behind block c
 * and x_entry_i the stream at the entry of block i, its rows are
 *   a token alive behind block c_l (prefix tokens always are):  f applied to x_after_{c_l}[b, j], at the token's position in
 *                                                               the unpruned sequence;
 *   a token that scheduled block i <= c_l dropped:              fill = 0: all zero bits;
 *                                                               fill = 1: f applied to x_entry_i[b, j], the state it had
 *                                                               when it left, as RAJNI_POOL_DENSE_LAST stores it.
 * f is the plan's final LayerNorm (norm_w, norm_b, ln_eps) with norm = 1, and one rounding of the stream value to the
 * plan's dtype with norm = 0 (a plain copy on an fp32 plan).  A block that is both scheduled and captured drops first: its
 * slab holds the block's output for the tokens it kept and the entry state for the ones it dropped.  Every row of every
 * slab is written exactly once; there is no memset pass and there are no atomics. */
#ifndef RAJNI_HIP_LAYERS_H
#define RAJNI_HIP_LAYERS_H

#include "rajni_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAJNI_MAX_LAYERS 64

typedef struct {
  int n;                 /* 1..RAJNI_MAX_LAYERS */
  const int* blocks;     /* HOST int[n], strictly ascending, 0 <= blocks[l] < plan.depth: the output of that block */
  int norm;              /* 1: through plan.norm_w / norm_b / ln_eps; 0: cast only */
  int fill;              /* 0: zero rows, 1: last state */
  void* out;             /* [n][B, P + n0, C] in the plan's dtype, 16-byte aligned */
  long long slab_stride; /* elements from slab to slab; 0 = B * (P + n0) * C; otherwise >= that and % 8 == 0 */
} rajni_vit_layers;

/* The forward of rajni_vit_forward_ext_prefix that also writes the slabs of `layers`.  layers == NULL: exactly the launches
 * of that entry point and the same bits.  Otherwise it composes with everything the plan, ext and prefix records can say
 * (a head or none, every pool, registers, the distilled head, q/k-norm, every mlp_act, e4m3 weights, the 16-bit stream) and
 * `logits` receives what it would have received without the record, bit for bit.  Behind every captured block the forward
 * issues one map launch (a chain of them past four scheduled blocks) and one launch that writes the slab; with fill = 1
 * every scheduled block that a capture follows issues one launch that writes its dropped rows to all those slabs at once.
 * Capturing block depth - 1 makes the last block run all rows, as the token outputs do; earlier captures leave the
 * last block's CLS-rows forms in place.  No workspace is added: rajni_vit_workspace_bytes_prefix is the size query.
 *
 * Refused before the first launch and before the workspace check: n outside 1..RAJNI_MAX_LAYERS, null blocks or out,
 * blocks not strictly ascending or outside [0, depth), norm or fill outside 0..1, a slab_stride below the dense size or
 * off a multiple of 8, an out that is not 16-byte aligned, plan.cls_only_last_block with block depth - 1 captured
 * (RAJNI_ERR_INVALID); norm = 1 with ext.norm_absent, and plan.act_fp8 (RAJNI_ERR_UNSUPPORTED). */
int rajni_vit_forward_layers(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                             const rajni_vit_layers* layers, const void* images, void* logits, rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_LAYERS_H */
