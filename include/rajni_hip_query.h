/* ViTs without a class token: the mean-query importance rule and the "no class row" forward.  Additive to rajni_hip.h: no
 * record, enum, entry point or workspace size of that header (or of rajni_hip_layers.h / rajni_hip_image.h) changes, and
 * RAJNI_ABI_VERSION stays what it is.
 *
 * THE RULE IS THIS PROJECT'S OWN EXTENSION, as fp8 and register tokens were: the reference cannot run a model without a class
 * token at all (its model.py:35 expands cls_token), so there is nothing to be faithful to.  For a block that scores, on its
 * current sequence of N tokens (prefix tokens included):
 *     qbar[b, h, :] = (1 / N) * sum_{n = 0 .. N-1} q[b, h, n, :]      fp32, from the qkv rows as stored (behind q/k-norm)
 *     A[b, n]       = mean_h softmax_n(qbar[b, h] . k[b, h, n] / sqrt(D))
 * and everything else is importance.py:23-34 unchanged (the V term, centring, unbiased std, eps, sigmoid, product, one
 * rounding to the I/O dtype).  A global-average-pooled head reads the mean of the tokens, so the mean query is the O(N * C)
 * analogue of "what the pooled output attends to".  Nobody has measured pruning quality on trained weights - for this rule
 * or for any other rule of this project.
 * The sum is fp32 in a fixed order that depends on the shape alone (no atomics): the same input gives the same bits on every
 * run, at any batch size and batch position, and under rajni_debug_force_score_two_pass.  The one-workgroup kernel and the
 * tiled path order the sum differently; they agree within the budget of the numerics tests, not bit for bit.
 *
 * Selection is the prefix rule with P allowed to be 0: the P prefix tokens are always kept and take no rank slot, keep_idx is
 * [B, P + keep] ascending, next_scores is gathered at keep_idx.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`; "elem" = one element of `dtype`).
 * A pointer below its minimum is refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL
 * optional pointer is aligned.
 *   rajni_score_select_query: qkv 16, scores_out elem, keep_idx 4, next_scores elem, workspace 256
 *   rajni_select_topk_query: scores elem, keep_idx 4, next_scores elem
 *   rajni_patch_embed_query: images 16, w 16, bias 16, reg 16, pos 16, x 16, workspace 16
 *   rajni_vit_forward_query: images 16, logits 16 (the records: as in rajni_hip.h; rajni_vit_query holds no pointer)
 * (end of the placement table) */
#ifndef RAJNI_HIP_QUERY_H
#define RAJNI_HIP_QUERY_H

#include "rajni_hip_image.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RAJNI_QUERY_CLS = 0, RAJNI_QUERY_MEAN = 1 };

/* Beside the plan and the other records.  class_token = 1: the sequence starts with the class row, as everywhere else in this
 * ABI; `query` picks the importance query of every scoring block (RAJNI_QUERY_CLS: row 0, RAJNI_QUERY_MEAN: the rule above).
 * class_token = 0: the sequence has no class row -
 *   - plan.cls_token is not read and may be NULL;
 *   - the prefix tokens are exactly the R registers of rajni_vit_prefix.reg_token: prefix.num_prefix = R (0..RAJNI_MAX_PREFIX;
 *     a NULL prefix record is R = 0), reg_token [R, C] non-NULL iff R > 0; plan.pos_embed holds (pos_has_cls ? R : 0) + n rows;
 *   - the head must pool with RAJNI_POOL_AVG (rows R..N-1), or the output is a feature output (RAJNI_POOL_NONE / _DENSE /
 *     _DENSE_LAST) - a token head has no row to read: `ext.pool` RAJNI_POOL_TOKEN (or ext NULL) is RAJNI_ERR_INVALID;
 *   - `query` must be RAJNI_QUERY_MEAN, prefix.head_rows == 2 and plan.cls_only_last_block are RAJNI_ERR_INVALID, plan.act_fp8 is
 *     RAJNI_ERR_UNSUPPORTED;
 *   - the last block always runs every row.
 * Every refusal names the field and comes before the first launch. */
typedef struct {
  int class_token; /* 1: the sequence has a class row (row 0); 0: it has none */
  int query;       /* RAJNI_QUERY_CLS or RAJNI_QUERY_MEAN */
} rajni_vit_query;

/* rajni_score_select_ws with the query named and num_prefix 0..RAJNI_MAX_PREFIX: N >= max(2, num_prefix + 1), keep == 0
 * computes scores only (scores_out required), keep in 1..N - num_prefix selects.  RAJNI_QUERY_CLS: the launches and the bits
 * of rajni_score_select_ws.  The workspace is rajni_score_select_query_workspace_bytes(...) bytes, 256-byte aligned: with
 * RAJNI_QUERY_CLS what rajni_score_select_workspace_bytes returns, with RAJNI_QUERY_MEAN B * C * 4 bytes more (rounded to the
 * carve's 256-byte offsets) wherever the tiled path runs, for the fp32 mean query a launch of its own writes in front of the
 * tiles.  Placement: qkv 16, scores_out elem, keep_idx 4, next_scores elem, workspace 256. */
size_t rajni_score_select_query_workspace_bytes(int B, int N, int H, int D, int dtype, int query);
int rajni_score_select_query(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep, int query,
                             void* scores_out, int32_t* keep_idx, void* next_scores, int dtype, void* workspace,
                             size_t workspace_bytes, rajni_stream_t stream);

/* rajni_select_topk_prefix with num_prefix 0..RAJNI_MAX_PREFIX: the selection alone, from scores a block carried
 * (update = False) - keep in 1..N - num_prefix, N >= max(2, num_prefix + 1).  num_prefix >= 1: the launch and the bits of
 * rajni_select_topk_prefix.  Placement: scores elem, keep_idx 4, next_scores elem. */
int rajni_select_topk_query(const void* scores, int B, int N, int num_prefix, int keep, int32_t* keep_idx, void* next_scores,
                            int dtype, rajni_stream_t stream);

/* rajni_patch_embed_image without a class row: x [B, R + (H / P) * (W / P), C], rows 0..R-1 = reg[r] (+ pos[r] when
 * pos_has_cls), `pos` holds (pos_has_cls ? R : 0) + (H / P) * (W / P) rows; R = num_reg in 0..RAJNI_MAX_PREFIX, reg NULL iff
 * R == 0.  Placement: images 16, w 16, bias 16, reg 16, pos 16, x 16, workspace 16; the workspace is
 * rajni_patch_embed_workspace_bytes_image's. */
int rajni_patch_embed_query(const void* images, const void* w, const float* bias, const void* reg, int num_reg, const void* pos,
                            int pos_has_cls, void* x, int x_f32, int B, int Cin, int H, int W, int P, int C, int dtype,
                            void* workspace, size_t workspace_bytes, rajni_stream_t stream);

/* The forward of rajni_vit_forward_image with the query record.  query == NULL or {1, RAJNI_QUERY_CLS}: exactly the launches of
 * that entry point and the same bits.  {1, RAJNI_QUERY_MEAN}: the same forward with the mean query in every scoring block.
 * {0, RAJNI_QUERY_MEAN}: the sequence without a class row (above); n0 = (height / patch) * (width / patch) + R, and every count
 * the other records speak of is against that n0 and P = R.  ext, prefix, layers and image may each be NULL.
 * rajni_vit_workspace_bytes_query returns 0 for a record the forward refuses (rajni_last_error then holds that refusal).
 * Placement: as rajni_vit_forward_image (rajni_vit_query holds no pointer). */
size_t rajni_vit_workspace_bytes_query(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                       const rajni_vit_query* query);
int rajni_vit_forward_query(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                            const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                            const void* images, void* logits, rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_QUERY_H */
