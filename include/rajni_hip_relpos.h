/* A learned relative position bias on the attention logits, on the pruned token set: BEiT / BEiTv2 and timm's vit_relpos_* /
 * vit_srelpos_* line.
 * Additive to rajni_hip.h: no record, enum value, entry point or workspace size of that header (or of rajni_hip_layers.h /
 * rajni_hip_image.h / rajni_hip_query.h / rajni_hip_attnpool.h / rajni_hip_norm.h / rajni_hip_rope.h / rajni_hip_mlpnorm.h)
 * changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * The native layer is table driven and knows no model family.  With a gh x gw patch grid (row-major, as the patch embedding
 * emits it), T = (2 gh - 1) * (2 gw - 1), all fp32:
 *     table     [blocks or 1][H][T]   entry (dy + gh - 1) * (2 gw - 1) + (dx + gw - 1) is the bias of a patch query at (yq, xq)
 *                                     against a patch key at (yk, xk), dy = yq - yk, dx = xq - xk
 *     prefix_q  [blocks or 1][H]      a prefix query against a patch key
 *     prefix_k  [blocks or 1][H]      a patch query against a prefix key
 *     prefix_qk [blocks or 1][H]      a prefix query against a prefix key
 * All prefix tokens (class, registers) share the three values.  block_stride, in elements of `table`: 0 = one table for all
 * blocks, H * T = one per block; the three value arrays then step by 0 or H.
 *
 * The rule, in fp32 on the fp32 logit:
 *     logit[q][k] = scale * (q . k) + bias(pos[q], pos[k])
 * The bias is NOT multiplied by scale.  pos[t] is the place packed row t had in the unpruned sequence: pos[b * np + t] of the
 * `pos` argument, or t where that is NULL; rows with pos < num_prefix are prefix rows, the others are patch pos - num_prefix.
 * The kernels add the bias to q . k in front of the scale, S' = (q . k) + bias * (1 / scale), before the row maximum is taken,
 * and run the softmax of rajni_attention on S': three fp32 roundings (1 / scale, exact for a power of two; the product; the
 * add) on top of rajni_attention's own, and a zero bias adds +0, which changes no bit.  scale must be positive and finite.
 * A patch position past the grid is clamped to its last patch: no entry point reads outside the table.
 *
 * Importance (this project's own rule, DESIGN.md section 1, B11: the reference has no such model): the class row's logits get
 * prefix_q[h] for patch keys and prefix_qk[h] for prefix keys before its softmax - importance is scored on the attention the
 * block computes.  The class row is a prefix row, so neither the table nor `pos` enters a score.
 *
 * Caps: head dim 64 only; gh, gw <= RAJNI_RELPOS_MAX_GRID.  np <= 256 runs the one-shot form of the head-dim-64 kernel
 * (per-token codes in 4 * 32 * ceil(np / 32) bytes of LDS, the table read through the cache), larger np the chunked
 * online-softmax form; fp32 models the fp32 kernel.  The persistent form is not used with a bias.
 *
 * ---- placement: the table of rajni_hip.h continued (one entry point per line, `name bytes`).  A pointer below its minimum is
 * refused with RAJNI_ERR_INVALID and a message that names it, before anything is launched; a NULL optional pointer is aligned.
 *   rajni_attention_relpos: qkv 16, keep_idx 4, out 16, table 4, prefix_q 4, prefix_k 4, prefix_qk 4, pos 4
 *   rajni_score_select_relpos: qkv 16, scores_out 2, keep_idx 4, next_scores 2, workspace 256, prefix_q 4, prefix_qk 4
 *   rajni_vit_forward_relpos: images 16, logits 16
 *   rajni_vit_relpos: table 4, prefix_q 4, prefix_k 4, prefix_qk 4
 * (end of the placement table) */
#ifndef RAJNI_HIP_RELPOS_H
#define RAJNI_HIP_RELPOS_H

#include "rajni_hip_mlpnorm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest grid side: 32 x 32 patches (512 px at patch 16), a head's table then holds 63 * 63 floats */
#define RAJNI_RELPOS_MAX_GRID 32

/* Beside the plan and the other records; NULL or all zero: no bias. */
typedef struct {
  const float* table;             /* [blocks or 1][H][(2 gh - 1) * (2 gw - 1)] fp32 */
  const float* prefix_q;          /* [blocks or 1][H] fp32 */
  const float* prefix_k;          /* the same shape */
  const float* prefix_qk;         /* the same shape */
  long long block_stride;         /* elements of table: 0 or H * (2 gh - 1) * (2 gw - 1) */
  int gh, gw;                     /* the patch grid: must equal the forward's */
} rajni_vit_relpos;

/* rajni_attention plus the bias.  table [H][T], prefix_q / prefix_k / prefix_qk [H]: one block's.  pos [B, np] int32 or NULL
 * (position = packed row index).  Head dim 64 only (RAJNI_ERR_UNSUPPORTED otherwise), 1 <= gh, gw <= RAJNI_RELPOS_MAX_GRID
 * (a larger grid is RAJNI_ERR_UNSUPPORTED, the message states the cap), 0 <= num_prefix <= RAJNI_MAX_PREFIX.  All-zero tables and
 * values give rajni_attention's result bit for bit.
 * Placement: qkv 16, keep_idx 4, out 16, table 4, prefix_q 4, prefix_k 4, prefix_qk 4, pos 4. */
int rajni_attention_relpos(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int H, int D, float scale,
                           int dtype, const float* table, const float* prefix_q, const float* prefix_k, const float* prefix_qk,
                           int gh, int gw, int num_prefix, const int32_t* pos, rajni_stream_t stream);

/* rajni_score_select_ws plus the class row's bias: prefix_q [H] on the patch keys, prefix_qk [H] on the num_prefix prefix keys
 * (rows 0 .. num_prefix - 1 of the unpacked block input), before the class row's softmax.  The workspace is
 * rajni_score_select_workspace_bytes(...) bytes, as for rajni_score_select_ws.  Zero values give rajni_score_select_ws's
 * result bit for bit.
 * Placement: as rajni_score_select_ws, and prefix_q 4, prefix_qk 4. */
int rajni_score_select_relpos(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep, void* scores_out,
                              int32_t* keep_idx, void* next_scores, int dtype, void* workspace, size_t workspace_bytes,
                              const float* prefix_q, const float* prefix_qk, rajni_stream_t stream);

/* rajni_vit_forward_mlpnorm plus the record.  relpos == NULL or all zero: exactly the launches of rajni_vit_forward_mlpnorm and
 * the same bits.  Otherwise every block's attention adds block i's bias (table + i * block_stride, the values + i * (block_stride
 * ? H : 0)) by the rule above, and every block that scores adds the class row's bias.  Behind a scheduled block the positions
 * of the packed rows come from the composed selections, this block's included: a map of B * n0 * 4 bytes in the workspace.
 * The last block's row reduction (query tiles without a wanted row are skipped) stays and gives the bits of all rows.
 * Refused before the first launch, each naming the combination: NULL table or value pointers with a non-zero record, gh * gw
 * != n0 - P, a block_stride other than 0 or H * T (RAJNI_ERR_INVALID); gh or gw over RAJNI_RELPOS_MAX_GRID, a head dim other than
 * 64, plan.act_fp8, the mean importance query or a sequence without a class row, a rope record together with the bias,
 * plan.cls_only_last_block (RAJNI_ERR_UNSUPPORTED).
 * The workspace is rajni_vit_workspace_bytes_relpos(...) bytes: rajni_vit_workspace_bytes_mlpnorm's plus the map (nothing
 * without a record); 0 = refused, with rajni_last_error holding the refusal.
 * Placement: as rajni_vit_forward_mlpnorm, and table / prefix_q / prefix_k / prefix_qk 4. */
size_t rajni_vit_workspace_bytes_relpos(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                        const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                        const rajni_vit_rope* rope, const rajni_vit_mlp_norm* mlp_norm, const rajni_vit_relpos* relpos);
int rajni_vit_forward_relpos(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                             const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                             const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                             const rajni_vit_mlp_norm* mlp_norm, const rajni_vit_relpos* relpos, const void* images, void* logits,
                             rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_RELPOS_H */
