/*
 * rajni_hip.h - C ABI of librajni_hip.so: the MI355X (gfx950) token-pruning forward path.
 *
 * The reference (dRaniwal/RAJNI-ViT) has no FFI of its own: its hot path is Python calling ATen
 * (SURVEY.md section 8b).  Each entry point below therefore replaces a *Python* call site of the reference,
 * cited as file:line relative to /root/reference/rajni/.  Conventions:
 *   - plain C, no torch types; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller owns all buffers, nothing is allocated or freed inside, no host sync inside;
 *   - every launch goes to the hipStream_t given (pass torch's current stream);
 *   - returns RAJNI_OK (0) or an error code; rajni_last_error() gives a host string (thread local);
 *   - `dtype` is the activation/weight element type of the model: RAJNI_BF16 (the fast path: bf16
 *     MFMA, fp32 accumulation), RAJNI_F16 (fp16 models: the same kernels, tilings and fusion on the f16
 *     MFMA forms - same rate, 3 more mantissa bits; outputs rounded to nearest even, overflow to +-inf;
 *     fp8 weights / activations need RAJNI_BF16 and return RAJNI_ERR_UNSUPPORTED with it) or RAJNI_F32
 *     (accuracy path: every tensor fp32, v_mfma_f32_16x16x4_f32 GEMMs, VALU attention; ~1/16 of the
 *     16-bit MFMA rate).
 *   - activations are row-major [B, N, C]; qkv is [B, N, 3*C] with the last axis laid out
 *     [3][H][D] (timm convention; importance.py:14, attention.py:46-47);
 *   - keep_idx is int32 on the device ([B, keep+1], slot 0 = CLS = 0, rest ascending; [B, P+keep] with P prefix
 *     tokens, see the *_prefix entry points); the Python surface widens to int64 to match attention.py:38.
 */
#ifndef RAJNI_HIP_H
#define RAJNI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rajni_stream_t; /* hipStream_t */

enum { RAJNI_F32 = 0, RAJNI_BF16 = 1, RAJNI_F16 = 2 };

enum {
  RAJNI_OK = 0,
  RAJNI_ERR_INVALID = 1,     /* bad argument (null pointer, shape, alignment) */
  RAJNI_ERR_UNSUPPORTED = 2, /* valid request the build does not implement (dtype, head dim ...) */
  RAJNI_ERR_LAUNCH = 3       /* HIP runtime error at launch */
};

/* epilogues of rajni_linear */
enum {
  RAJNI_EPI_BIAS = 0,      /* y = x W^T + b                                  attention.py:22 (qkv) */
  RAJNI_EPI_BIAS_GELU = 1, /* y = gelu_erf(x W^T + b)                        model.py:59 (mlp.fc1+act) */
  RAJNI_EPI_BIAS_RESID = 2,/* y = resid[row or gathered row] + gamma*(x W^T + b)
                              attention.py:55 + model.py:55-58 (proj, gather x, ls1, add);
                              model.py:59 (mlp.fc2, ls2, add)                                       */
  RAJNI_EPI_BIAS_QUICK_GELU = 16,/* y = quick_gelu(x W^T + b), quick_gelu(v) = v * sigmoid(1.702 v): the MLP activation of the
                              OpenAI CLIP, MetaCLIP and DFN towers.  BIAS_GELU in every other respect (output type, tilings,
                              profile class); bf16, fp16, fp32 and fp8 WEIGHTS.  With x_scale (fp8 x fp8) it is
                              RAJNI_ERR_UNSUPPORTED: the re-quantising e4m3 epilogue exists for exact GELU only.
                              Codes 3..15, 17 and >= 19 are unknown.                                      */
  RAJNI_EPI_BIAS_SWIGLU = 18 /* y[M, N] = silu(x Wg^T + bg) * (x Wv^T + bv), silu(t) = t * sigmoid(t): the gated FC1 of timm's
                              GluMlp(act_layer=nn.SiLU, gate_last=False) / SwiGLUPacked (the DINOv2 giant ViTs).  w is
                              [2N, K]: row n is the gate of output column n, row N + n its value (timm's packed order);
                              it is allocated with 2N padded up to a multiple of 256 rows, which always covers the last
                              value tile (N + roundup(N, 128) <= roundup(2N, 256)).  bias and w_scale are [2N] in the
                              same order; ldc >= N; N <= 2^30.  Evaluated in fp32 on the accumulators, rounded once to
                              `dtype`; a finite (gate, value) never gives NaN and silu(0) * 0 = 0.  bf16, fp16, fp32 and
                              fp8 WEIGHTS; output type, store path and profile class are BIAS_GELU's.  With x_scale
                              (fp8 x fp8) it is RAJNI_ERR_UNSUPPORTED: the re-quantising e4m3 epilogue exists for exact
                              GELU only.                                                                */
};

/* ---- addressing limits ----
 * Tensors may be of any size the device holds: every kernel forms row, image and workspace offsets in 64 bits, so buffers of
 * 2^31 elements / 2^32 bytes and more are supported (qkv of a 2048 px batch, the MLP hidden buffer of a large batch), and
 * rajni_vit_workspace_bytes() may exceed 2^32.  Counts are 32-bit ints: B, rows, M, N, K, n_src each stay below 2^31.
 * Where a kernel keeps a 32-bit offset on purpose (registers), the host routes around it or refuses the call:
 *   - rajni_linear, RAJNI_EPI_BIAS_RESID with an fp32 stream on the 256 x 128 tiling: the residual rows are addressed with
 *     32-bit element offsets.  A residual operand that spans 2^31 elements or more (resid rows x ldr, gathered: the rows of
 *     all source images) is sent to the 128 x 128 tiling instead, under the forced tiling hook too.  Same bits, slower.
 *   - rajni_attention (16-bit, head dim 64, np <= 256: the persistent kernel) and rajni_attention_fp8: rows are addressed
 *     inside ONE image with a 32-bit byte offset; the image base is 64-bit.  n_src * 3 * H * 64 * 2 bytes must stay below
 *     2^32, else RAJNI_ERR_UNSUPPORTED (16416 tokens, the score path's cap, fit with up to 340 heads).
 *   - rajni_qk_norm: (token, head) groups are counted in 32 bits: rows * 2 * H < RAJNI_QK_NORM_MAX_GROUPS, else
 *     RAJNI_ERR_UNSUPPORTED.  Split the rows over several calls (the op is row-wise).
 *   - rajni_attention and the tiled score path (rajni_score_select_ws with scratch) put the image index on a grid axis:
 *     B <= RAJNI_MAX_GRID_YZ (rajni_attention: H too), else RAJNI_ERR_UNSUPPORTED.  Split the batch (images are independent).
 *     rajni_vit_forward (and its _ext / _prefix forms) checks plan->B against the same limit with the rest of the plan.
 * All of these refusals happen before anything is launched. */
#define RAJNI_MAX_GRID_YZ 65535
#define RAJNI_QK_NORM_MAX_GROUPS ((1LL << 31) - 1024)

/* ---- placement: minimum alignment of every pointer ----
 * The kernels reach memory in 16-byte pieces wherever they can, so WHERE a buffer sits is part of the contract.  Minimum
 * alignment in bytes of each pointer of each entry point ("elem" = one element of `dtype`: 2 bytes for bf16 / fp16, 4 for fp32):
 *   - data tensors (activations, weights, qkv, images, the residual stream, outputs, e4m3 bytes, cls / reg / pos, the
 *     patch-embed column workspace): 16.  Row strides keep their own rules and no others: lda / ldw / ldc / ldr,
 *     x_row_stride and logits_ld are multiples of 8 elements (bytes % 16 for e4m3 operands), so every row starts on a
 *     16-byte boundary and nothing more is assumed - not a 128-byte line, not a dense row.  (rajni_linear with
 *     dtype RAJNI_F32 reads the residual row one element at a time and asks for no ldr rule.)
 *   - fp32 per-column vectors (bias, gamma / LayerScale, LayerNorm and q/k-norm w and b, w_scale): 16 - every kernel
 *     that takes one reads it as float4 somewhere (LayerNorm rows, the stream tilings' epilogues).
 *   - arrays indexed per element: x_scale, y_scale, row_scale, hid_scale (fp32) and keep_idx / idx / r_idx (int32): 4;
 *     score arrays (scores, scores_out, next_scores): elem.
 *   - scratch of the tiled score path and rajni_vit_plan.workspace: 256 (the forward carves its workspace at 256-byte
 *     offsets from the base, and the score scratch is one of the pieces).
 * A pointer below its minimum is refused with RAJNI_ERR_INVALID and a message that names it, before anything is
 * launched; a NULL optional pointer is aligned.  No kernel or tiling choice looks at an address or at a stride's
 * residue: the same values at another legal placement give the same bits.  The table (one entry point per line, `name
 * bytes`; the whole forward per struct):
 *   rajni_importance: qkv 16, scores_out elem
 *   rajni_select_topk: scores elem, keep_idx 4, next_scores elem
 *   rajni_score_select: qkv 16, scores_out elem, keep_idx 4, next_scores elem
 *   rajni_select_topk_prefix: scores elem, keep_idx 4, next_scores elem
 *   rajni_score_select_prefix: qkv 16, scores_out elem, keep_idx 4, next_scores elem
 *   rajni_score_select_ws: qkv 16, scores_out elem, keep_idx 4, next_scores elem, workspace 256
 *   rajni_gather_rows: src 16, idx 4, dst 16
 *   rajni_attention: qkv 16, keep_idx 4, out 16
 *   rajni_attention_fp8: qkv 16, keep_idx 4, out_q 16, row_scale 4
 *   rajni_layernorm: x 16, w 16, b 16, y 16
 *   rajni_layernorm_fp8: x 16, w 16, b 16, y_q 16, y_scale 4, hid_scale 4
 *   rajni_linear: x 16, w 16, y 16, resid 16, bias 16, gamma 16, w_scale 16, x_scale 4, y_scale 4, r_idx 4
 *   rajni_patch_embed: images 16, w 16, bias 16, cls 16, pos 16, x 16, workspace 16
 *   rajni_patch_embed_prefix: images 16, w 16, bias 16, cls 16, reg 16, pos 16, x 16, workspace 16
 *   rajni_qk_norm: qkv 16, q_w 16, q_b 16, k_w 16, k_b 16
 *   rajni_layernorm_stream: x 16, w 16, b 16
 *   rajni_pool_norm: x 16, norm_w 16, norm_b 16, fc_w 16, fc_b 16, out 16
 *   rajni_pool_norm_prefix: x 16, norm_w 16, norm_b 16, fc_w 16, fc_b 16, out 16
 *   rajni_vit_forward: images 16, logits 16
 *   rajni_vit_plan: patch_w 16, patch_b 16, cls_token 16, pos_embed 16, norm_w 16, norm_b 16, head_w 16, head_b 16, workspace 256
 *   rajni_block: norm1_w 16, norm1_b 16, qkv_w 16, qkv_b 16, proj_w 16, proj_b 16, ls1 16, norm2_w 16, norm2_b 16, fc1_w 16, fc1_b 16, fc2_w 16, fc2_b 16, ls2 16, keep_idx 4, scores elem, next_scores elem, forced_keep_idx 4, qkv_s 16, proj_s 16, fc1_s 16, fc2_s 16
 *   rajni_qk_affine: q_norm_w 16, q_norm_b 16, k_norm_w 16, k_norm_b 16
 *   rajni_vit_ext: norm_pre_w 16, norm_pre_b 16, fc_norm_w 16, fc_norm_b 16
 *   rajni_vit_prefix: reg_token 16
 * (end of the placement table) */

#define RAJNI_ABI_VERSION 8 /* bumped whenever a struct or an entry point changes; checked by the ctypes binding */
int rajni_abi_version(void); /* == RAJNI_ABI_VERSION of the header the library was built from */
const char* rajni_last_error(void);
/* 0 when a gfx950 device is usable by this process, else an error code (message in last_error) */
int rajni_device_check(void);

/* ---- a1: compute_importance(qkv, num_heads, eps)                         importance.py:4-34 ----
 * scores_out [B,N] in `dtype` (the reference returns qkv's dtype, importance.py:34). */
int rajni_importance(const void* qkv, void* scores_out, int B, int N, int H, int D, float eps,
                     int dtype, rajni_stream_t stream);

/* ---- a5,a6,a10: top-k + sort + CLS prepend + score carry                 attention.py:31-39,58 ----
 * scores [B,N] in `dtype`; keep = max(1, int(keep_ratio*(N-1))) is computed by the caller
 * (attention.py:31-32, Python-double semantics).  Tie rule (the reference leaves it unspecified):
 * larger score first, then lower index; NaN ranks as +inf.
 * keep_idx [B,keep+1] int32; next_scores [B,keep+1] in `dtype` (may be NULL). */
int rajni_select_topk(const void* scores, int B, int N, int keep, int32_t* keep_idx,
                      void* next_scores, int dtype, rajni_stream_t stream);

/* ---- a1+a6+a10 fused (one launch per pruning stage): scores never leave the chip between the
 * two steps.  scores_out may be NULL. */
int rajni_score_select(const void* qkv, int B, int N, int H, int D, float eps, int keep,
                       void* scores_out, int32_t* keep_idx, void* next_scores, int dtype,
                       rajni_stream_t stream);

/* ---- a7,a13: torch.gather(t, 1, keep_idx[..., None].expand(...))   attention.py:42-43, model.py:55-56
 * src [B,n_src,row_elems] -> dst [B,n_dst,row_elems]; row_elems*elem_size must be a multiple of 16. */
int rajni_gather_rows(const void* src, const int32_t* idx, void* dst, int B, int n_src, int n_dst,
                      int row_elems, int dtype, rajni_stream_t stream);

/* ---- a8: softmax(q k^T * scale) v on the kept tokens                      attention.py:46-54 ----
 * qkv [B,n_src,3*H*D]; keep_idx [B,np] int32 or NULL (NULL: identity, np == n_src - the unpruned
 * block of model.py:62).  The row gather of attention.py:42-43 is fused into the tile loads.
 * out [B,np,H*D].  D % 8 == 0, 8 <= D <= 128 (D = 64 has the tuned
 * kernels; other head dims take a general MFMA kernel). */
int rajni_attention(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np,
                    int H, int D, float scale, int dtype, rajni_stream_t stream);
/* The same attention (bf16 qkv) with its output rows quantised for an fp8 x fp8 proj (opt-in "fp8_mfma" format; the
 * reference has no fp8 semantics - this is the build's rule):
 *   out_q[b,q,c] = e4m3_rne_sat(attn[b,q,c] * (1 / out_scale))  as bytes [B,np,H*D];  row_scale[b*np + q] = out_scale
 * (the per-row dequantisation scales the proj launch takes as rajni_linear_args.x_scale).  ONE scale per launch: an
 * attention row spans H (image, head) work items, so no item can know the row's maximum; the caller passes a bound -
 * attention output is a convex combination of V rows, |V[j,c]| <= ||ln1(x)[j]||_2 ||Wv[c]||_2 + |bv[c]| and
 * ||ln1(x)[j]||_2 <= sqrt(C) max|gamma1| + ||beta1||_2 (a normalised row has norm <= sqrt(C)), so
 *   out_scale = (1.0625 * (sqrt(C) * max|gamma1| + ||beta1||_2) * max_c ||Wv[c]||_2 + max|bv|) / 448
 * (the 1.0625 covers the e4m3 rounding of the LayerNorm rows; the conversion saturates).  e4m3 is a floating-point
 * format: a bound a few binades above the true maximum costs range at the bottom, not precision.
 * Head dim 64 and np <= 224 only (RAJNI_ERR_UNSUPPORTED otherwise). */
int rajni_attention_fp8(const void* qkv, const int32_t* keep_idx, void* out_q, float out_scale, float* row_scale,
                        int B, int n_src, int np, int H, int D, float scale, rajni_stream_t stream);

/* ---- LayerNorm over the last axis (blk.norm1 / norm2 / m.norm)            model.py:51,59,65 ----
 * x rows are `x_row_stride` elements apart (lets the final norm read CLS rows only), y is dense
 * [rows, C] in `dtype`.  x is `dtype`, or fp32 when x_f32 != 0 (the fp32 residual stream).
 * w,b are fp32 [C]. C % 8 == 0. */
int rajni_layernorm(const void* x, long x_row_stride, const float* w, const float* b, void* y,
                    int rows, int C, float eps, int dtype, int x_f32, rajni_stream_t stream);
/* The same LayerNorm with its output quantised per row for the fp8 matrix pipe (opt-in "fp8_mfma" format, BASELINE
 * configs[4]; the reference has no fp8 semantics - these are the build's, SURVEY 7 "hard parts"):
 *   y_scale[r] = max_c |ln(x)[r,c]| / 448   (1 for an all-zero row),   y_q[r,c] = e4m3_rne_sat(ln(x)[r,c] * (1 / y_scale[r]))
 * with ln(x) evaluated in fp32; y_q is [rows, C] bytes (OCP e4m3 "fn").  When hid_scale != NULL it also receives a
 * per-row scale for the block's MLP hidden activations, from a bound rather than their maximum (which no GEMM
 * epilogue can know): |gelu(ln(x) W1^T + b1)| <= ||ln(x)[r]||_2 * max_n ||W1[n]||_2 + max |b1|, so
 *   hid_scale[r] = (1.0625 * ||ln(x)[r]||_2 * w1_rownorm_max + b1_absmax) / 448   (1 when that is 0);
 * e4m3 is a floating-point format, so a bound a few binades above the true maximum costs no precision.
 * x is fp32 when x_f32 != 0, else bf16.  C % 8 == 0, C <= 2048. */
int rajni_layernorm_fp8(const void* x, long x_row_stride, const float* w, const float* b, void* y_q,
                        float* y_scale, float* hid_scale, float w1_rownorm_max, float b1_absmax,
                        int rows, int C, float eps, int x_f32, rajni_stream_t stream);

/* ---- linear layers with fused epilogues (a3, a9, a13, a15) ----
 * y[M,N] = epi(x[M,K] W[N,K]^T).  W must be allocated with its row count padded up to a multiple
 * of 256 (rows >= N are never read into results but must be readable); K % 64 == 0; lda/ldw/ldc/ldr
 * in elements, multiples of 8.  bias/gamma are fp32 [N] (NULL = 0 / 1).
 * RESID: resid row for output row m is  (m / r_np) * r_nsrc + r_idx[m]  when r_idx != NULL
 * (r_idx = keep_idx flattened [B*r_np]), else m. */
typedef struct {
  const void* x; long lda;
  const void* w; long ldw;
  const float* bias;
  const float* gamma;
  const void* resid; long ldr;
  const int32_t* r_idx; int r_np; int r_nsrc;
  void* y; long ldc;
  int M, N, K;
  int epilogue;
  int dtype;
  int stream_f32;  /* RESID only: resid and y are the fp32 residual stream (1) instead of `dtype` (0: a bf16 or fp16 stream) */
  /* fp8 weights (BASELINE config 5): when non-NULL, `w` holds fp8 e4m3 (OCP "fn": no inf, max 448) bytes
   * [N(pad256),K], ldw in bytes and a multiple of 16, and w_scale[n] (fp32 [N]) is the dequantisation
   * scale of row n: y = epi(x (q*s)^T) with bf16 x and fp32 accumulation.  dtype must be RAJNI_BF16. */
  const float* w_scale;
  /* fp8 activations on the fp8 matrix pipe (v_mfma_f32_16x16x128_f8f6f4; requires w_scale): when x_scale != NULL,
   * `x` holds e4m3 bytes [M,K] (lda in bytes, % 16 == 0) and x_scale[m] (fp32 [M]) is the dequantisation scale of
   * row m - what rajni_layernorm_fp8 writes: y = epi((xq*xs) (wq*ws)^T), fp32 accumulation.  K % 256 == 0, K >= 512.
   * With epilogue RAJNI_EPI_BIAS_GELU, y_scale (fp32 [M], required) selects an e4m3 OUTPUT: y is [M,N] bytes
   * (ldc in bytes, % 16 == 0) holding e4m3_rne_sat(gelu(.) * (1 / y_scale[m])) - the next linear's x / x_scale. */
  const float* x_scale;
  const float* y_scale;
} rajni_linear_args;
int rajni_linear(const rajni_linear_args* args, rajni_stream_t stream);

/* ---- a12: patch-embed + CLS + pos-embed                                    model.py:34-37 ----
 * images [B,Cin,S,S] -> x [B, 1+(S/P)^2, C].  conv weight w [C(pad256), ceil64(Cin*P*P)] (k order c,ky,kx,
 * zero-padded columns), bias fp32 [C]; cls [C]; pos [(1 or 0)+(S/P)^2, C] (`pos_has_cls`=0 is timm
 * no_embed_class: SURVEY B3); x is written as fp32 when x_f32 != 0.  S % P == 0.  For a power-of-two P >= 8
 * with S % 8 == 0 and Cin*P*P % 64 == 0 the im2col is fused into the GEMM's tile loads and no workspace is
 * needed; any other patch size (14: ViT-L/14, ViT-H/14, DINOv2) materialises the zero-padded column matrix in
 * `workspace` (16-byte aligned, >= rajni_patch_embed_workspace_bytes(...), which is 0 for the fused case). */
int rajni_patch_embed(const void* images, const void* w, const float* bias, const void* cls,
                      const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int S,
                      int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream);
size_t rajni_patch_embed_workspace_bytes(int B, int Cin, int S, int P, int dtype);

/* ---- a11-a16: the whole RAJNIViTWrapper.forward                            model.py:30-69 ---- */
typedef struct {
  const float* norm1_w; const float* norm1_b;
  const void* qkv_w; const float* qkv_b;      /* [3C(pad),C], [3C] */
  const void* proj_w; const float* proj_b;    /* [C(pad),C], [C]  */
  const float* ls1;                           /* [C] or NULL      */
  const float* norm2_w; const float* norm2_b;
  const void* fc1_w; const float* fc1_b;      /* [Hd(pad),C], [Hd] */
  const void* fc2_w; const float* fc2_b;      /* [C(pad),Hd], [C]  */
  const float* ls2;
  /* schedule entry for this block (model.py:13-20): keep = 0 -> not scheduled (model.py:62) */
  int keep;                /* kept PATCH tokens (attention.py:31-32), output has keep+1 tokens */
  int update;              /* attention.py:25: recompute scores iff update or no carried scores */
  int32_t* keep_idx;       /* [B,keep+1] out (required when keep>0) */
  void* scores;            /* [B,N] out, dtype (optional) */
  void* next_scores;       /* [B,keep+1] out, dtype (required when keep>0: carried to the next block) */
  const int32_t* forced_keep_idx; /* test hook: use this selection instead (selection-conditional parity) */
  /* per-row scales of fp8 e4m3 weights (see rajni_linear_args.w_scale); NULL = that weight is `dtype` */
  const float* qkv_s; const float* proj_s; const float* fc1_s; const float* fc2_s;
  /* act_fp8 plans only: max_n ||W1deq[n,:]||_2 and max_n |b1[n]| of this block's fc1 (the hidden-activation
   * bound of rajni_layernorm_fp8) */
  float fc1_rownorm_max, fc1_bias_absmax;
  /* act_fp8 plans only: out_scale of rajni_attention_fp8 for this block (> 0: where the block's attention launch has
   * head dim 64 and at most 224 tokens, the attention output is emitted as e4m3 rows and proj runs on the fp8 matrix
   * pipe; 0: proj keeps bf16 activations x e4m3 weights) */
  float attn_out_scale;
} rajni_block;

typedef struct {
  int dtype;
  int B, in_chans, img_size, patch_size;
  int C, H, D, depth, hidden, num_classes;
  float ln_eps, attn_scale;
  int pos_has_cls;
  const void* patch_w; const float* patch_b; const void* cls_token; const void* pos_embed;
  const rajni_block* blocks;                   /* host array [depth] */
  const float* norm_w; const float* norm_b;
  const void* head_w; const float* head_b;     /* [classes(pad),C], [classes] */
  void* workspace; size_t workspace_bytes;     /* >= rajni_vit_workspace_bytes() */
  int32_t* token_counts;                       /* HOST int32[depth] out: tokens at block entry (model.py:43) */
  int logits_ld;                               /* row stride of `logits` in elements (0 = num_classes); % 8 == 0 */
  int cls_only_last_block;                     /* 1: when the last block is not a pruning stage, compute it for the
                                                  CLS row only - attention with the CLS query over all tokens,
                                                  proj / MLP on B rows.  model.py:65-66 feeds only x[:, 0] to the
                                                  head, so the logits are the same function; the other rows of the
                                                  last block are never formed.  This opt-in's CLS attention is a kernel
                                                  of its own (logits within a 16-bit ulp); 0 (default) computes the same
                                                  rows with the all-rows kernels, bit for bit the all-rows logits */
  int resid_bf16;                              /* 0 (default): the residual stream x is kept in fp32 between
                                                  blocks (2x closer to the fp32 reference than a bf16 stream, see
                                                  DESIGN.md); 1: keep it in the model's 16-bit dtype (bf16 or fp16)
                                                  like the reference's 16-bit model.  (The name predates fp16 models;
                                                  ignored for RAJNI_F32) */
  int act_fp8;                                 /* 1 (opt-in, needs e4m3 block weights): norm1 / norm2 emit per-row
                                                  scaled e4m3 activations, QKV / FC1 / FC2 run on the fp8 matrix
                                                  pipe, FC1's GELU epilogue re-quantises the hidden activations
                                                  (rajni_layernorm_fp8, rajni_linear_args.x_scale); blocks with attn_out_scale > 0
                                                  also emit the attention output as e4m3 rows and run proj on that pipe
                                                  (rajni_attention_fp8).  Attention's products, patch embed, head and the
                                                  residual stream are unchanged.
                                                  C % 256 == 0 and hidden % 256 == 0.  0 (default): bf16 activations */
} rajni_vit_plan;

size_t rajni_vit_workspace_bytes(const rajni_vit_plan* plan);
/* images [B,Cin,S,S] dtype; logits [B,num_classes] dtype
 *
 * A HEADLESS plan - head_w == NULL and num_classes == 0 (timm num_classes=0: head is nn.Identity; head_b is not read) - launches
 * no head GEMM: the buffer passed as `logits` receives the row the head would have read, fc_norm(pool(norm(x))), [B, C] in the
 * plan's dtype - written by the final LayerNorm / pool_norm launch itself, which writes dense rows: logits_ld is 0 or C (a
 * stride below C or off a multiple of 8 is RAJNI_ERR_INVALID, a wider one RAJNI_ERR_UNSUPPORTED).  With rajni_vit_ext.pool =
 * RAJNI_POOL_NONE / RAJNI_POOL_DENSE / RAJNI_POOL_DENSE_LAST the buffer receives tokens instead, [B, Nf, C] / [B, P + n, C] (the
 * last: every pruned position holds the token's state at the block that dropped it instead of zeros).  One of head_w and
 * num_classes without the other is RAJNI_ERR_INVALID (a null weight pointer).  A headless plan with act_fp8 or with
 * rajni_vit_prefix.head_rows == 2 is RAJNI_ERR_UNSUPPORTED; everything else works as with a head - token or avg pool,
 * fc_norm, norm_absent, registers, q/k-norm, norm_pre, every mlp_act, e4m3 weights, the 16-bit stream, and the last
 * block's CLS-rows form.  The workspace is that of the same plan with a head. */
int rajni_vit_forward(const rajni_vit_plan* plan, const void* images, void* logits,
                      rajni_stream_t stream);

/* ---- timm VisionTransformer options the reference drops (deviation B4) ----
 * The reference wrapper reads none of attn.q_norm / attn.k_norm, norm_pre, global_pool and fc_norm (model.py:34-37,
 * 65-66, attention.py:8-12 take a fixed attribute set), so it mis-computes every model that has one.  The semantics
 * below are timm's (timm/models/vision_transformer.py: Attention.forward, VisionTransformer.forward_features, .pool,
 * .forward_head).  All statistics are fp32 and two-pass, every sum has one fixed order: the same input gives the same
 * bits.  LayerNorm weights are fp32 and required, biases fp32 or NULL (= 0). */

/* q = q_norm(q); k = k_norm(k)   (timm Attention.forward: `q, k = self.q_norm(q), self.k_norm(k)`, both
 * nn.LayerNorm(D), one module for all heads), IN PLACE on the q and k thirds of qkv [rows, 3*H*D]; the v third is
 * neither read nor written.  Score+select, attention and the fp8 attention output read the buffer afterwards, so the
 * importance scores are the CLS row of the attention the block performs.  D % 8 == 0, 8 <= D <= 128 (D = 64: a group
 * is one 128-byte line of 8 lanes; other head dims share a general form). */
int rajni_qk_norm(void* qkv, const float* q_w, const float* q_b, const float* k_w, const float* k_b, int rows, int H,
                  int D, float eps, int dtype, rajni_stream_t stream);

/* x = norm_pre(x)   (timm forward_features: `x = self.norm_pre(x)` after _pos_embed), IN PLACE on the residual stream
 * x [rows, C]: fp32 when x_f32 != 0 (or dtype is RAJNI_F32), else `dtype`.  C % 8 == 0, C <= 2048. */
int rajni_layernorm_stream(void* x, const float* w, const float* b, int rows, int C, float eps, int dtype, int x_f32,
                           rajni_stream_t stream);

/* out[b] = fc_norm(pool(norm(x[b])))   (timm forward_features' `x = self.norm(x)`, then .pool and forward_head's
 * `x = self.fc_norm(x)`): x [B,N,C] is the residual stream (fp32 when x_f32 != 0, else `dtype`), out [B,C] `dtype` - the
 * row the head GEMM reads.  pool = RAJNI_POOL_TOKEN: x[:, 0]; RAJNI_POOL_AVG: the mean of x[:, 1:], i.e. of the patch
 * tokens that SURVIVED pruning (what timm computes on whatever token set reaches the head), summed in a fixed order
 * in fp32.  norm_w == NULL / fc_w == NULL: that norm is nn.Identity.  C % 8 == 0, C <= 2048. */
/* Two more values exist for the whole forward only (rajni_vit_ext.pool; rajni_pool_norm refuses them), both for a HEADLESS
 * plan (below) and both behind the final norm, which must be present and not followed by an fc_norm:
 *   RAJNI_POOL_NONE (timm global_pool=''): no pooling.  The output is every surviving token of the final stream through the
 *     final norm, [B, Nf, C] dense, Nf the token count behind the last block - timm's forward_features on the pruned graph.
 *   RAJNI_POOL_DENSE (this project's own): [B, P + n, C], n = (img_size / patch_size)^2 - the shape the unpruned model's
 *     forward_features returns.  Row s of image b holds norm(x)[b, j] when token j of the final stream sat at position s of
 *     the unpruned sequence (prefix tokens at 0..P-1, patch p at P + p: the scheduled blocks' selections composed, the forced
 *     one where a block has it); every other row is all zero bits.  The normalised rows have the bits RAJNI_POOL_NONE gives.
 *   RAJNI_POOL_DENSE_LAST (5; 4 is unknown): RAJNI_POOL_DENSE with no zero row - a token that leaves the stream keeps the feature
 *     it had when it left.  Row s holds norm(x)[b, j] for a token that survives the last block, exactly the row RAJNI_POOL_DENSE
 *     writes; for a token that scheduled block i drops (it entered the block and is not in the block's selection) it holds
 *     norm(x_entry_i)[b, j], x_entry_i the residual stream at the entry of block i (behind norm_pre; the embedded stream for
 *     i = 0) and norm the final LayerNorm, as DINOv2's get_intermediate_layers(norm=True) applies it to intermediate states.
 *     Prefix tokens never leave.  Every row is written exactly once, by the launch behind the block that drops it or by the
 *     final one; the rows wait in the stream buffer the block's residual gather read from, so no workspace is added. */
enum { RAJNI_POOL_TOKEN = 0, RAJNI_POOL_AVG = 1, RAJNI_POOL_NONE = 2, RAJNI_POOL_DENSE = 3, RAJNI_POOL_DENSE_LAST = 5 };
enum { RAJNI_MLP_GELU = 0, RAJNI_MLP_QUICK_GELU = 1, RAJNI_MLP_SWIGLU = 3 };   /* rajni_vit_ext.mlp_act */
int rajni_pool_norm(const void* x, int B, int N, int C, int pool, const float* norm_w, const float* norm_b,
                    float norm_eps, const float* fc_w, const float* fc_b, float fc_eps, void* out, int dtype, int x_f32,
                    rajni_stream_t stream);

/* The extension record of the whole forward: everything a plan cannot say, beside it (so the plan's layout and
 * RAJNI_ABI_VERSION stay what they are).  An all-zero record is the plain forward. */
typedef struct {
  const float* q_norm_w; const float* q_norm_b;   /* [D], [D] or NULL */
  const float* k_norm_w; const float* k_norm_b;
} rajni_qk_affine;

typedef struct {
  const rajni_qk_affine* qk_norm;   /* host array [depth] (every block, pruned or not), or NULL: no q/k-norm */
  float qk_eps;
  const float* norm_pre_w; const float* norm_pre_b; float norm_pre_eps;   /* norm_pre_w == NULL: no norm_pre */
  int norm_absent;                  /* 1: base_model.norm is nn.Identity (plan.norm_w / norm_b are not read) */
  int pool;                         /* RAJNI_POOL_TOKEN (0) or RAJNI_POOL_AVG; AVG with plan.cls_only_last_block is
                                       RAJNI_ERR_INVALID: that opt-in never forms the rows to be averaged.
                                       RAJNI_POOL_NONE / RAJNI_POOL_DENSE (see the enum): the token outputs of a headless plan.
                                       With a head (per-token classification), an fc_norm or norm_absent (there is no
                                       cast-only row kernel) they are RAJNI_ERR_UNSUPPORTED, with plan.cls_only_last_block
                                       RAJNI_ERR_INVALID; the last block then runs all rows.  RAJNI_POOL_DENSE_LAST (5) is a
                                       token output too, with the same refusals under its own name.  Any other value (4
                                       included) is RAJNI_ERR_UNSUPPORTED */
  const float* fc_norm_w; const float* fc_norm_b; float fc_norm_eps;      /* fc_norm_w == NULL: no fc_norm */
  int mlp_act;                      /* RAJNI_MLP_GELU (0) or RAJNI_MLP_QUICK_GELU: the activation of every block's FC1.  It sits in
                                       what were the four bytes of tail padding behind fc_norm_eps (offset 68 of 72: the record
                                       is 8-byte aligned), so no field moves and the size stays; a caller built against the
                                       record without it passes zeroed or ignored padding - callers zero the record, "an
                                       all-zero record is the plain forward" - and gets exact GELU as before.  Hence
                                       RAJNI_ABI_VERSION does not move.  Any other value is RAJNI_ERR_INVALID; QUICK_GELU with
                                       plan.act_fp8 is RAJNI_ERR_UNSUPPORTED (see RAJNI_EPI_BIAS_QUICK_GELU).
                                       RAJNI_MLP_SWIGLU (3; 2 is unknown): every block's FC1 is gated (RAJNI_EPI_BIAS_SWIGLU).  plan.hidden
                                       stays FC2's K and the hidden buffer's width; rajni_block.fc1_w is [2 * hidden (pad
                                       256), C] - gate rows, then value rows - and fc1_b / fc1_s are [2 * hidden].  The
                                       workspace carve does not change.  With plan.act_fp8 it is RAJNI_ERR_UNSUPPORTED */
} rajni_vit_ext;

/* rajni_vit_forward with the options of `ext` (NULL or all zero: exactly the launches of rajni_vit_forward).
 * norm_pre runs after patch embed + CLS + pos-embed, q/k-norm after every block's QKV GEMM, and the tail is
 * norm -> pool -> fc_norm -> head.  No workspace beyond rajni_vit_workspace_bytes(). */
int rajni_vit_forward_ext(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const void* images, void* logits,
                          rajni_stream_t stream);

/* ---- prefix tokens beyond CLS: timm's register tokens (`reg_tokens=R`, e.g. vit_*_patch14_reg4_dinov2) ----
 * The reference knows one prefix token (it concatenates cls_token only and slices [:, 1:]); the semantics here are timm's
 * VisionTransformer._pos_embed and .pool.  With P = 1 + R prefix tokens and n patches the token order is
 * [cls, reg_0 .. reg_{R-1}, patch_0 .. patch_{n-1}]; pos_embed has n rows (added to the patch rows only, `pos_has_cls` = 0)
 * or P + n rows in token order (added to every row, `pos_has_cls` != 0).  Importance is unchanged (CLS is the query, the
 * softmax and the V statistics run over all N tokens, registers included).  Only patch tokens are ranked:
 * keep = max(1, int(keep_ratio * (N - P))), keep_idx is [B, P+keep] with slots 0..P-1 = 0..P-1 and the rest ascending
 * patch indices >= P, next_scores = scores gathered at keep_idx (prefix slots included).  'avg' pooling is the mean of
 * rows P..N-1.  Every *_prefix entry point with num_prefix = 1 issues the launches of its namesake and gives the same bits.
 * 1 <= num_prefix <= RAJNI_MAX_PREFIX. */
#define RAJNI_MAX_PREFIX 32

/* The prefix record of the whole forward: travels beside the plan and the ext record (their layouts stay what they are).
 *
 * head_rows = 2 is timm's VisionTransformerDistilled in eval mode (the distilled DeiT checkpoints): token order
 * [cls, dist, patches], the dist token a prefix token exactly like a register (never pruned, never ranked, no rank slot; its
 * [1, C] row travels as reg_token, num_prefix = 2), and the head reads rows 0 and 1 of the normalised stream:
 *   logits = (head(norm(x)[:, 0]) + head_dist(norm(x)[:, 1])) / 2
 * as ONE linear layer with K = 2C: the final LayerNorm writes the two normalised rows of image b side by side as row b of
 * [B, 2C], plan.head_w is [classes(pad), 2C] = [0.5 * head.weight | 0.5 * head_dist.weight] and plan.head_b is
 * 0.5 * (head.bias + head_dist.bias).  Both products accumulate in fp32 and the sum is rounded once.  A last block that
 * does not prune is computed for those two rows only, bit for bit the all-rows logits.  head_rows = 2 needs num_prefix == 2
 * (else RAJNI_ERR_INVALID) and a plain token head: ext.pool == RAJNI_POOL_TOKEN, no fc_norm, a final norm
 * (RAJNI_ERR_UNSUPPORTED); with plan.cls_only_last_block it is RAJNI_ERR_INVALID (that opt-in forms the CLS row only), with
 * plan.act_fp8 RAJNI_ERR_UNSUPPORTED.  Any value outside 0..2 is RAJNI_ERR_INVALID.  All of it before the first launch. */
typedef struct {
  int num_prefix;          /* P = 1 + number of register tokens; 0 or 1: CLS only (reg_token is not read) */
  int head_rows;           /* rows of each image the head reads: 0 or 1 = row 0 (the class token), 2 = rows 0 and 1 (above).  It
                              sits in what were the four bytes of padding behind num_prefix (offset 4 of 16: reg_token is 8-byte
                              aligned), so no field moves, the size stays and RAJNI_ABI_VERSION does not move; callers zero the
                              record, and a zero here is the forward as it was, launch for launch */
  const void* reg_token;   /* [num_prefix-1, C] in the plan's dtype, 16-byte aligned; required when num_prefix > 1.
                              plan.pos_embed then has (plan.pos_has_cls ? num_prefix : 0) + n rows */
} rajni_vit_prefix;

/* rajni_select_topk / rajni_score_select over scores [B,N] whose first num_prefix tokens are always kept and take no rank
 * slot: 1 <= keep <= N - num_prefix, keep_idx and next_scores are [B, num_prefix+keep]. */
int rajni_select_topk_prefix(const void* scores, int B, int N, int num_prefix, int keep, int32_t* keep_idx,
                             void* next_scores, int dtype, rajni_stream_t stream);
int rajni_score_select_prefix(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep,
                              void* scores_out, int32_t* keep_idx, void* next_scores, int dtype,
                              rajni_stream_t stream);
/* rajni_patch_embed writing x [B, num_prefix+(S/P)^2, C]: row 0 = cls, rows 1..num_prefix-1 = reg [num_prefix-1, C]
 * (`dtype`; may be NULL when num_prefix = 1), then the patches; pos [(pos_has_cls ? num_prefix : 0)+(S/P)^2, C].
 * cls, reg and pos are 16-byte aligned like every data tensor (see "placement"). */
int rajni_patch_embed_prefix(const void* images, const void* w, const float* bias, const void* cls, const void* reg,
                             int num_prefix, const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int S,
                             int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream);
/* rajni_pool_norm whose RAJNI_POOL_AVG is the mean of x[:, num_prefix:] (same fixed fp32 summation order). */
int rajni_pool_norm_prefix(const void* x, int B, int N, int num_prefix, int C, int pool, const float* norm_w,
                           const float* norm_b, float norm_eps, const float* fc_w, const float* fc_b, float fc_eps,
                           void* out, int dtype, int x_f32, rajni_stream_t stream);
/* The whole forward with prefix tokens: the stream starts with num_prefix + n tokens, rajni_block.keep counts kept PATCH
 * tokens (keep <= N - num_prefix), rajni_block.keep_idx / next_scores / forced_keep_idx are [B, num_prefix+keep],
 * token_counts count every token.  The fp8_mfma attention limit of 224 rows counts the prefix rows.  prefix == NULL, or
 * num_prefix <= 1 with no reg_token: exactly the launches of rajni_vit_forward_ext, the same bits.  ext may be NULL. */
size_t rajni_vit_workspace_bytes_prefix(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix);
int rajni_vit_forward_ext_prefix(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                 const void* images, void* logits, rajni_stream_t stream);

/* ---- importance scores beyond one workgroup's LDS (high-resolution inputs) ----
 * rajni_importance / rajni_score_select[_prefix] run one workgroup per image with the logits [H][N] and the head-mean
 * values [N][D] in LDS, and refuse (RAJNI_ERR_UNSUPPORTED) what 160 KiB cannot hold: about 600 tokens at head dim 64, 475
 * at 80, 300 at 128.  Larger shapes are scored by a tile kernel (grid: 32-token tiles x B) and a one-workgroup-per-image
 * finish kernel that pass fp32 logits, head-mean values and per-tile partial sums through caller-provided scratch - two
 * launches, no host synchronisation, capturable.  All sums are fixed trees in tile order: an image's scores do not depend
 * on B or on its place in the batch.  They meet the same error budget as the single-workgroup kernel's but are not bit-equal
 * to them (the summation orders differ).  The tiled path takes N <= 16416 (16384 patch tokens + RAJNI_MAX_PREFIX), every supported head dim and dtype.
 *
 * rajni_score_select_workspace_bytes: host only; 0 for every shape the single-workgroup kernel holds (and for shapes no
 * path takes: those are refused by the call itself).
 * rajni_score_select_ws: rajni_score_select_prefix with that scratch (256-byte aligned; may be NULL when the size is 0, and
 * then the call IS rajni_score_select_prefix / rajni_importance: same kernel, same bits).  keep == 0 computes scores only
 * (scores_out required; keep_idx / next_scores may be NULL); with keep >= 1 scores_out may be NULL. */
size_t rajni_score_select_workspace_bytes(int B, int N, int H, int D, int dtype);
int rajni_score_select_ws(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep,
                          void* scores_out, int32_t* keep_idx, void* next_scores, int dtype, void* workspace,
                          size_t workspace_bytes, rajni_stream_t stream);

/* ---- measurement hooks (bench.py roofline): HIP-event timing per kernel class on the launch
 * stream.  mask bit i enables class i; classes listed by rajni_profile_class_name(). ---- */
enum { RAJNI_NUM_KCLASS = 17 };
void rajni_profile_enable(unsigned mask);
const char* rajni_profile_class_name(int kclass);
/* synchronises the recorded events, ADDS them into the accumulators, returns them: per class the
 * number of launches, total milliseconds, algorithmic flops and algorithmic bytes. */
int rajni_profile_collect(long long* launches, double* ms, double* flops, double* bytes);
void rajni_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* RAJNI_HIP_H */
