/* rajni_hip_debug.h - test and tuning hooks of librajni_hip.so.  NOT part of the drop-in boundary
 * (include/rajni_hip.h): nothing on the product path calls these.  They set process-global, unsynchronised
 * switches, so they must not be flipped while another thread is inside a rajni_* call; the tests and the
 * probes under tools/ use them from one thread, before the launch they want to steer. */
#ifndef RAJNI_HIP_DEBUG_H
#define RAJNI_HIP_DEBUG_H

#include "rajni_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* attention kernel choice: 0 = by np (default: persistent full-row kernel for np <= 256), 1 = chunked
 * online-softmax kernel, 2 = one-shot full-row kernel (np <= 256) */
void rajni_debug_force_attention(int mode);

/* The attention of the boundary header limited to the query rows [0, nq), 1 <= nq <= np: same arguments, same kernel and
 * instantiation as the all-rows call (chosen by np, D and dtype), but query tiles that hold none of the wanted rows are
 * switched off or not launched.  A tile that straddles nq is computed and stored whole (32 rows with head dim 64 on 16-bit
 * operands, 128 with other head dims, 64 on fp32), nothing past it is written; the rows written hold the bits the all-rows
 * call writes (tested).  The forward uses nq = 1 in its last block. */
int rajni_debug_attention_rows(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int nq,
                               int H, int D, float scale, int dtype, rajni_stream_t stream);

/* Last block of the whole forward: 0 (default) = when only x[:, 0] is observable behind it (last block not a pruning stage,
 * token-pooled head, no act_fp8, cls_only_last_block off) attention runs for the first query tile and proj / LN2 / FC1 / fc2
 * on the B CLS rows - the all-rows kernels on fewer rows, logits bit for bit the same; 1 = every row of the last block is
 * computed, the reference's op graph row for row.  Token counts, stats and traces are the same either way. */
void rajni_debug_set_last_block_all_rows(int on);
/* the eligibility test alone, on the host (ext / prefix may be NULL; no device pointer is followed): 1 when the forward of
 * this plan computes its last block for the rows the head reads only (the CLS rows; with rajni_vit_prefix.head_rows == 2 rows
 * 0 and 1 of each image, 2B rows), 0 when for all rows */
int rajni_debug_last_block_cls_rows(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix);

/* GEMM tiling: 0 = by shape (default), 1 = 128x128x64 (4 waves), 4 = 256x256x64 persistent,
 * 5 = 256x128x64 3-stage persistent */
void rajni_debug_force_gemm_tiling(int mode);

/* fp8 x fp8 GEMM tiling: 0 = by shape (default), 1 = 256x128x128 always, 2 = 256x256x128 wherever it exists (bias and
 * GELU epilogues) */
void rajni_debug_force_f8_tiling(int mode);

/* every other workgroup of an XCD sleeps `units` x 8192 cycles before its first tile of a residual-epilogue GEMM, so
 * that the two halves of the chip do not burst in the same instant; default 1 (best in the forward by 0.1-0.3 %), 0 = off */
void rajni_debug_set_resid_stagger(int units);

/* W bytes one N block of the persistent tile order may occupy (default 1600 KiB); 0 = the plain column-fastest
 * order; -k = blocks of k column tiles regardless of size.  Results are bit-identical for every value (tested). */
void rajni_debug_set_gemm_nblock_bytes(int bytes);

/* Persistent launches (the 256-row stream tilings of rajni_linear and rajni_patch_embed on 16-bit, fp8-weight and fp8 x fp8
 * operands; the head-dim-64 attention kernel for up to 256 kept tokens, rajni_attention_fp8 and rajni_debug_attention_rows
 * included) use at most `n` workgroups; 0 (default) = as many as the device takes.  ONLY the grid changes: tiling, tile and
 * item order, N blocks and dynamic LDS stay, so each workgroup walks more tiles or items through its next-tile / next-item
 * pipeline.  Results are bit-identical for every n (tested); rajni_debug_linear_plan reports the capped grid. */
void rajni_debug_set_persistent_workgroups(int n);

/* Dry run of a linear call: the same argument checks, format / epilogue resolution and tiling choice, for a device of
 * `cus` compute units (no device needed), and no launch.  Returns the code the call itself would return before launching and
 * sets the same last-error text; on RAJNI_OK `*out` holds what would be launched.  The pointers in `args` are checked
 * (null, alignment) and never followed. */
enum { RAJNI_TILING_SMALL = 1,       /* 128x128x64, one workgroup per tile */
       RAJNI_TILING_F32 = 2,         /* 128x128x32 on fp32 operands */
       RAJNI_TILING_WIDE = 4,        /* 256x256x64 persistent */
       RAJNI_TILING_MID = 5,         /* 256x128x64 persistent, 3 stages */
       RAJNI_TILING_F8_STREAM = 8,   /* fp8 x fp8 256x128x128 persistent */
       RAJNI_TILING_F8_WIDE = 9 };   /* fp8 x fp8 256x256x128 persistent */
typedef struct rajni_linear_plan {
  int tiling;                       /* RAJNI_TILING_* */
  int tiles_n, total_tiles, nblk;   /* column tiles, tiles, column tiles per N block of the tile order (0: plain order) */
  int grid;                         /* workgroups */
  int lds_bytes;                    /* dynamic LDS per workgroup: stages + epilogue scratch */
} rajni_linear_plan;
int rajni_debug_linear_plan(const rajni_linear_args* args, int cus, rajni_linear_plan* out);

/* score+select: 1 = read K and V in two passes with vbar reusing the logits' LDS region (what N = 577 x 16 heads
 * needs) even when the one-pass layout fits; 0 = default.  Scores are bit-identical either way (tested). */
void rajni_debug_force_score_two_pass(int on);

/* score+select: 1 = rajni_score_select_workspace_bytes asks for scratch and rajni_score_select_ws (and the whole forward)
 * takes the tiled kernels for EVERY shape, also those one workgroup holds; 0 = default.  Entry points without scratch are
 * not affected. */
void rajni_debug_force_score_tiled(int on);

/* diagnostic builds (-DRAJNI_GEMM_STAMPS / -DRAJNI_ATTN_STAMPS / -DRAJNI_SS_STAMPS) only: device buffer receiving
 * 4 x uint64 s_memtime stamps per workgroup; NULL disables */
void rajni_debug_set_gemm_stamps(void* buf);

#ifdef __cplusplus
}
#endif
#endif
