/* A norm inside the MLP, between the activation (or the SwiGLU gate) and fc2: timm `Mlp(norm_layer=...)`, `SwiGLU.norm`, the
 * sub-LayerNorm of the EVA02 image towers (EVA02-B: 2048 wide, EVA02-L: 2730).
 * Additive to rajni_hip.h: no record, enum value, entry point or workspace size of that header (or of rajni_hip_layers.h /
 * rajni_hip_image.h / rajni_hip_query.h / rajni_hip_attnpool.h / rajni_hip_norm.h / rajni_hip_rope.h) changes, and
 * RAJNI_ABI_VERSION stays what it is.
 *
 * The rule, in place on every row of x [rows, ld], over its first n columns only, statistics in fp32:
 *     RAJNI_NORM_LAYERNORM: mean = (1 / n) sum_c x[c];  rstd = rsqrt((1 / n) sum_c (x[c] - mean)^2 + eps)    (two passes)
 *                           x[c] = ((x[c] - mean) * rstd) * w[c] + b[c]          b == NULL: 0
 *     RAJNI_NORM_RMS:       rstd = rsqrt((1 / n) sum_c x[c]^2 + eps);  x[c] = (x[c] * rstd) * w[c]          b is not read
 * rounded once to the buffer's type.  The divisor is n, never ld.  Columns [n, ld) - the zero padding of the hidden buffer to
 * whole K steps, which FC1's zero rows fill with act(0) = 0 - hold zeros on entry and hold zeros on exit: the elements past n of
 * a partial last 16-byte chunk (n % 8 != 0) stay out of both sums and are stored as +0, whole chunks past n are neither read
 * nor written, and nothing past ld is touched.  The sums run in the order of the other row kernels - a lane's 8-element
 * chunks in order, then the 6-step wave butterfly - so a row gives the same bits at any batch size, batch position and row count.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`).  A pointer below its minimum is
 * refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL optional pointer is aligned.
 *   rajni_hidden_norm: x 16, w 16, b 16
 *   rajni_vit_forward_mlpnorm: images 16, logits 16
 *   rajni_vit_mlp_norm: w 16, b 16
 * (end of the placement table) */
#ifndef RAJNI_HIP_MLPNORM_H
#define RAJNI_HIP_MLPNORM_H

#include "rajni_hip_rope.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the widest row rajni_hidden_norm takes: one wave holds the row in registers, 8 chunks of 8 elements per lane */
#define RAJNI_HIDDEN_NORM_MAX 4096

/* Beside the plan and the other records; NULL or all zero: no norm inside the MLP. */
typedef struct {
  const float* const* w;          /* [depth] pointers, each [n] fp32 */
  const float* const* b;          /* [depth] pointers, each [n] fp32 or NULL (= 0); the array itself may be NULL; not read when the
                                     forward's norm kind is RMS */
  float eps;
  int n;                          /* the model's MLP width; plan.hidden is the zero-padded one */
} rajni_vit_mlp_norm;

/* The kernel alone: the rule above on x [rows, ld], in `dtype` (bf16 / fp16 / fp32), or fp32 whatever `dtype` is when x_f32.
 * One wave per row, 16-byte accesses, the row read once.  0 < n <= RAJNI_HIDDEN_NORM_MAX (a wider row is RAJNI_ERR_UNSUPPORTED,
 * the message states the cap); ld >= n, ld % 8 == 0.  Placement: x 16, w 16, b 16. */
int rajni_hidden_norm(int kind, void* x, long ld, const float* w, const float* b, int rows, int n, float eps, int dtype, int x_f32,
                      rajni_stream_t stream);

/* rajni_vit_forward_rope plus the record.  mlp_norm == NULL or all zero: exactly the launches of rajni_vit_forward_rope and the
 * same bits.  Otherwise every block issues one rajni_hidden_norm launch between FC1 and FC2, on the rows its MLP runs on (the
 * head's rows alone in a last block that computes only those), of the forward's one norm kind (rajni_vit_norm.kind), under
 * every ext.mlp_act.  Composes with every other record.
 * Refused before the first launch, each naming the combination: n <= 0 or n > plan.hidden, a NULL w or w[i]
 * (RAJNI_ERR_INVALID); n over RAJNI_HIDDEN_NORM_MAX, the record with plan.act_fp8 (RAJNI_ERR_UNSUPPORTED).
 * The workspace is rajni_vit_workspace_bytes_mlpnorm(...) bytes - the record adds nothing to rajni_vit_workspace_bytes_rope's
 * size; 0 = refused, with rajni_last_error holding the refusal.
 * Placement: as rajni_vit_forward_rope, and every w[i] / b[i] 16. */
size_t rajni_vit_workspace_bytes_mlpnorm(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                         const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                         const rajni_vit_rope* rope, const rajni_vit_mlp_norm* mlp_norm);
int rajni_vit_forward_mlpnorm(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                              const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                              const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                              const rajni_vit_mlp_norm* mlp_norm, const void* images, void* logits, rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_MLPNORM_H */
