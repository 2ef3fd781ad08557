// Shared device/host helpers for the gfx950 kernels.  CDNA4 only: wave64, MFMA, LDS-DMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/rajni_hip.h"
#include "../../include/rajni_hip_debug.h"
#include "../../include/rajni_hip_layers.h"
#include "../../include/rajni_hip_image.h"
#include "../../include/rajni_hip_query.h"
#include "../../include/rajni_hip_attnpool.h"
#include "../../include/rajni_hip_norm.h"
#include "../../include/rajni_hip_rope.h"
#include "../../include/rajni_hip_mlpnorm.h"
#include "../../include/rajni_hip_relpos.h"

typedef unsigned short bf16_t;  // raw bf16 bits in memory
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float(((unsigned)u) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
  return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// 8 bf16 (one 16-byte chunk) -> 8 floats
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
  f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 v;
  v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]);
  v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
  return v;
}

// ---- fp16 models: raw fp16 storage as a DISTINCT C++ type (bf16_t is unsigned short, so a second unsigned-short
// typedef would silently pick the bf16 specialisations below).  Conversions round to nearest even
// (v_cvt_f16_f32 / v_cvt_pk_f16_f32; never the round-toward-zero pkrtz form), overflow goes to +-inf as in torch.
typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
__device__ __forceinline__ float h2f(f16_t h) { return (float)h; }
__device__ __forceinline__ f16_t f2h(float f) { return (_Float16)f; }
__device__ __forceinline__ unsigned pack2h(float lo, float hi) {
  f16x2 v = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float h_lo(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[0]; }
__device__ __forceinline__ float h_hi(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[1]; }

// the 16-bit activation formats (A = bf16_t or f16_t) behind one set of names: two values per 32-bit word,
// 8 per 16-byte chunk
template <typename A> __device__ __forceinline__ unsigned pack2(float lo, float hi);
template <> __device__ __forceinline__ unsigned pack2<bf16_t>(float lo, float hi) { return pack2bf(lo, hi); }
template <> __device__ __forceinline__ unsigned pack2<f16_t>(float lo, float hi) { return pack2h(lo, hi); }
template <typename A> __device__ __forceinline__ float lo16(unsigned u);
template <> __device__ __forceinline__ float lo16<bf16_t>(unsigned u) { return bf_lo(u); }
template <> __device__ __forceinline__ float lo16<f16_t>(unsigned u) { return h_lo(u); }
template <typename A> __device__ __forceinline__ float hi16(unsigned u);
template <> __device__ __forceinline__ float hi16<bf16_t>(unsigned u) { return bf_hi(u); }
template <> __device__ __forceinline__ float hi16<f16_t>(unsigned u) { return h_hi(u); }
template <typename A> __device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  f[0] = lo16<A>(v.x); f[1] = hi16<A>(v.x); f[2] = lo16<A>(v.y); f[3] = hi16<A>(v.y);
  f[4] = lo16<A>(v.z); f[5] = hi16<A>(v.z); f[6] = lo16<A>(v.w); f[7] = hi16<A>(v.w);
}
template <typename A> __device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 v;
  v.x = pack2<A>(f[0], f[1]); v.y = pack2<A>(f[2], f[3]);
  v.z = pack2<A>(f[4], f[5]); v.w = pack2<A>(f[6], f[7]);
  return v;
}
// The MFMA forms the kernels issue, by operand format.  Fragments travel as bf16 vectors in both formats (the
// same LDS reads and registers; hipcc's waitcnt insertion treats differently typed LDS reads differently, see
// gemm.hip) and are reinterpreted for the f16 instruction - same shapes, same cycles (v_mfma_f32_*_f16).
template <typename A> __device__ __forceinline__ f32x4 mfma_16x16x32(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  if constexpr (__is_same(A, f16_t))
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <typename A> __device__ __forceinline__ f32x16 mfma_32x32x16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (__is_same(A, f16_t))
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <typename A> __device__ __forceinline__ f32x4 mfma_16x16x16(const s16x4& a, const s16x4& b, const f32x4& c) {
  if constexpr (__is_same(A, f16_t))
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// 8 consecutive elements of the activation dtype (bf16_t, f16_t or float) <-> 8 floats
template <typename T> __device__ __forceinline__ void load8(const T* p, float* f);
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
template <> __device__ __forceinline__ void load8<f16_t>(const f16_t* p, float* f) {
  unpack8<f16_t>(*reinterpret_cast<const uint4*>(p), f);
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float* f);
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float* f) {
  *reinterpret_cast<uint4*>(p) = pack8(f);
}
template <> __device__ __forceinline__ void store8<f16_t>(f16_t* p, const float* f) {
  *reinterpret_cast<uint4*>(p) = pack8<f16_t>(f);
}
template <> __device__ __forceinline__ void store8<float>(float* p, const float* f) {
  reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}
// value as the activation dtype would hold it, and scalar load/store
template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <> __device__ __forceinline__ float round_to<f16_t>(float v) { return h2f(f2h(v)); }
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float ld1(const f16_t* p) { return h2f(*p); }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void st1(f16_t* p, float v) { *p = f2h(v); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- host side -----------------------------------------------------------------------------
void rajni_set_error(const char* fmt, ...);
// the device the calling thread's launches go to, and its CU count (hipDeviceProp_t::multiProcessorCount,
// read once per device; 256 on MI355X).  Per-device caches are sized RAJNI_MAX_DEVICES.
#define RAJNI_MAX_DEVICES 32
int rajni_current_device();
int rajni_num_cus();
// workgroups of a persistent launch that would take `grid`: the test hook rajni_debug_set_persistent_workgroups
// (include/rajni_hip_debug.h) caps it; 0 (default) = as computed.  Only the grid changes - tiles, items and their order do not.
extern int rajni_g_persistent_cap;
inline int rajni_persistent_grid(int grid) { return rajni_g_persistent_cap > 0 && grid > rajni_g_persistent_cap ? rajni_g_persistent_cap : grid; }

enum KClass {
  KC_GEMM_BIAS = 0, KC_GEMM_GELU = 1, KC_GEMM_RESID = 2, KC_GEMM_PATCH = 3, KC_ATTENTION = 4,
  KC_LAYERNORM = 5, KC_SCORE_SELECT = 6, KC_IMPORTANCE = 7, KC_SELECT = 8, KC_GATHER = 9,
  KC_CLS_POS = 10, KC_OTHER = 11,
  KC_GEMM_RESID_SQ = 12,  // residual GEMM with K <= N (the attention projection): bound by its fp32-stream epilogue
  KC_GEMM8_BIAS = 13, KC_GEMM8_GELU = 14, KC_GEMM8_RESID = 15,  // fp8 x fp8 GEMMs (act_fp8 plans)
  KC_GEMM8_RESID_SQ = 16   // ... with K <= N (proj on e4m3 attention output)
};
// event bracket around one launch when the class is enabled
struct ProfScope {
  int kc; hipStream_t s; void* rec;
  ProfScope(int kclass, hipStream_t stream, double flops, double bytes);
  ~ProfScope();
};

#define RAJNI_CHECK_LAUNCH(name)                                              \
  do {                                                                        \
    hipError_t e__ = hipGetLastError();                                       \
    if (e__ != hipSuccess) {                                                  \
      rajni_set_error("%s launch failed: %s", name, hipGetErrorString(e__));  \
      return RAJNI_ERR_LAUNCH;                                                \
    }                                                                         \
  } while (0)

#define RAJNI_REQUIRE(cond, code, ...)       \
  do {                                       \
    if (!(cond)) {                           \
      rajni_set_error(__VA_ARGS__);          \
      return code;                           \
    }                                        \
  } while (0)

// The placement contract of include/rajni_hip.h ("placement"): each pointer of an entry point with the minimum alignment the
// kernels behind it need.  The first pointer below its minimum is refused by name (RAJNI_ERR_INVALID); a null pointer passes
// (the null checks name it).  Host-side integer tests only: every entry point runs them before its first HIP call.
struct PlacedPtr { const char* name; const void* p; int align; };
int rajni_check_placement(const char* who, const PlacedPtr* ptrs, int n);
#define RAJNI_REQUIRE_PLACED(who, ...)                                                        \
  do {                                                                                        \
    const PlacedPtr placed__[] = {__VA_ARGS__};                                               \
    const int rc__ = rajni_check_placement(who, placed__, (int)(sizeof(placed__) / sizeof(placed__[0]))); \
    if (rc__ != RAJNI_OK) return rc__;                                                        \
  } while (0)
inline int rajni_elem_bytes(int dtype) { return dtype == RAJNI_F32 ? 4 : 2; }   // score arrays: element alignment

// diagnostic builds only (-DRAJNI_GEMM_STAMPS / -DRAJNI_ATTN_STAMPS): device buffer for s_memtime stamps
extern unsigned long long* rajni_g_stamps;

// internal launchers shared between the per-op ABI and the whole-forward plan
int launch_linear(const rajni_linear_args& a, hipStream_t s);
int launch_patch_embed(const void* images, const void* w, const float* bias, const void* cls,
                       const void* pos, int pos_has_cls, void* x, int out_f32, int B, int Cin, int H, int W,
                       int P, int C, int dtype, void* ws, size_t ws_bytes, hipStream_t s,
                       int num_prefix = 1, const void* reg = nullptr,    // reg: [num_prefix-1, C] register tokens behind CLS
                       int has_cls = 1);   // 0 (rajni_hip_query.h): no class row - cls is not read, num_prefix = R >= 0, reg [R, C]
size_t patch_embed_workspace_bytes(int B, int Cin, int H, int W, int P, int dtype);   // images [B, Cin, H, W]; 0: im2col fused into the GEMM loads
// (kind, here and below: RAJNI_NORM_LAYERNORM, or RAJNI_NORM_RMS of rajni_hip_norm.h - the same kernel's RMS form, b not read)
int launch_layernorm(const void* x, long xs, const float* w, const float* b, void* y, int rows,
                     int C, float eps, int x_f32, int dtype, hipStream_t s, int kind = RAJNI_NORM_LAYERNORM);
int launch_layernorm_fp8(const void* x, long xs, const float* w, const float* b, void* yq, float* yscale,
                         float* hscale, float wnorm, float bmax, int rows, int C, float eps, int x_f32, hipStream_t s);
int launch_attention(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int nq,
                     int H, int D, float scale, int dtype, hipStream_t s);   // nq: query rows [0, nq) only (np = all)
// a relative position bias on the logits (rajni_hip_relpos.h): one block's table [H][T] and values [H], the positions of the
// packed rows (null: the row index) and the grid.  A kernel argument of the head-dim-64 and fp32 attention kernels; all zero: none
struct RelBias {
  const float* table; const float* pq; const float* pk; const float* pqk;
  const int32_t* pos;     // [B, np]
  int gw, npatch, P, center, T;   // grid width, gh * gw, prefix rows, index of (dy, dx) = (0, 0), entries per head
  float inv_scale;                // 1 / scale: the bias joins q . k in front of the scale
};
int launch_attention_relpos(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int nq, int H, int D,
                            float scale, int dtype, const float* table, const float* pq, const float* pk, const float* pqk,
                            int gh, int gw, int num_prefix, const int32_t* pos, hipStream_t s);
int launch_attention_fp8(const void* qkv, const int32_t* keep_idx, void* out_q, float out_scale, float* row_scale,
                         int B, int n_src, int np, int H, int D, float scale, hipStream_t s);
int launch_attention_cls(const void* qkv, void* out, int B, int N, int H, int D, float scale, int dtype,
                         hipStream_t s, float q_scale = 0.f);   // q_scale > 0: the row passes through rajni_attention_fp8's e4m3 rounding
// the latent-query attention pool (rajni_hip_attnpool.h): kv [B, N, 2 * H * D], q [H, D] fp32 with the scale folded in, out [B, H * D]
// in `dtype`, or fp32 with out_f32 (the whole forward's tail)
int launch_attention_pool(const void* kv, const float* q, void* out, int B, int N, int H, int D, int dtype, hipStream_t s,
                          int out_f32 = 0);
// ws: scratch of rajni_score_select_workspace_bytes(B, N, H, D, dtype) bytes (256-byte aligned; may be null when that
// is 0): shapes beyond one workgroup's LDS are scored by the tiled kernels through it
int launch_score_select(const void* qkv, const void* scores_in, int B, int N, int H, int D,
                        float eps, int keep, void* scores_out, int32_t* keep_idx,
                        void* next_scores, int dtype, hipStream_t s, int num_prefix = 1, void* ws = nullptr,
                        size_t ws_bytes = 0, int query = RAJNI_QUERY_CLS, const float* rb_pq = nullptr,
                        const float* rb_pqk = nullptr, int rb_prefix = 0);   // RAJNI_QUERY_MEAN: ws sized by rajni_score_select_query_workspace_bytes
int launch_gather_rows(const void* src, const int32_t* idx, void* dst, int B, int n_src, int n_dst,
                       int row_bytes, hipStream_t s);
// RAJNI_POOL_DENSE: the selections composed into src [B, Nf] (levels[0] = the last scheduled block's; host arrays), and the
// final norm written to the rows of the unpruned sequence [B, S, C] they name, zeros elsewhere
int launch_source_idx(int32_t* src, const int32_t* const* idx, const int* width, const int* nsrc, int n_levels, int B, int Nf,
                      hipStream_t s);
// (zero_fill = 0, RAJNI_POOL_DENSE_LAST: the rows src does not name are left as they are)
int launch_layernorm_dense(const void* x, const int32_t* src, const float* w, const float* b, void* y, int B, int Nf, int S,
                           int C, float eps, int x_f32, int dtype, hipStream_t s, int zero_fill = 1, int kind = RAJNI_NORM_LAYERNORM);
// RAJNI_POOL_DENSE_LAST: the patch rows of the stream x [B, N, C] that the selection keep [B, Np] drops, through the final norm to
// row src[b, j] of y [B, S, C]; src [B, N] = where each token of x sat in the unpruned sequence
int launch_layernorm_dropped(const void* x, const int32_t* keep, const int32_t* src, const float* w, const float* b, void* y,
                             int B, int N, int Np, int P, int S, int C, float eps, int x_f32, int dtype, hipStream_t s,
                             int kind = RAJNI_NORM_LAYERNORM);
// rajni_vit_forward_layers: launch_layernorm_dense without the norm (the stream row rounded once to `dtype`), and
// launch_layernorm_dropped to the `ny` outputs ys[k] [B, S, C] at once (a host array), through the norm or cast only
int launch_rows_dense_cast(const void* x, const int32_t* src, void* y, int B, int Nf, int S, int C, int x_f32, int dtype,
                           hipStream_t s, int zero_fill = 1);
int launch_rows_dropped_multi(const void* x, const int32_t* keep, const int32_t* src, const float* w, const float* b,
                              void* const* ys, int ny, int norm, int B, int N, int Np, int P, int S, int C, float eps, int x_f32,
                              int dtype, hipStream_t s);
// variants.hip: the timm options of rajni_vit_ext (b pointers may be NULL = no bias; nw / fw NULL = that norm is absent)
int launch_qk_norm(void* qkv, const float* qw, const float* qb, const float* kw, const float* kb, int rows, int H, int D,
                   float eps, int dtype, hipStream_t s);
int launch_layernorm_stream(void* x, const float* w, const float* b, int rows, int C, float eps, int x_f32, int dtype, hipStream_t s,
                            int kind = RAJNI_NORM_LAYERNORM);
int launch_pool_norm(const void* x, int B, int N, int C, int pool, const float* nw, const float* nb, float neps,
                     const float* fw, const float* fb, float feps, void* out, int x_f32, int dtype, hipStream_t s,
                     int num_prefix = 1, int kind = RAJNI_NORM_LAYERNORM);
// patch_embed.norm (rajni_hip_norm.h): the patch rows of the stream x [B, N, C] normalised in place, + pos[pos_off + j]
int launch_embed_norm(int kind, void* x, const float* w, const float* b, const void* pos, int pos_off, int B, int N, int num_prefix,
                      int C, float eps, int dtype, int x_f32, hipStream_t s);
// rope.hip (rajni_hip_rope.h): q and k of qkv [B * N, 3, H, D] rotated in place by the row of cos / sin [rows, D] that
// src [B, N] (NULL: the row index) names for each patch token; head_stride 0 = one table for all heads
int launch_rope_qk(void* qkv, const int32_t* src, const float* cost, const float* sint, long head_stride, int B, int N, int num_prefix,
                   int H, int D, int layout, int dtype, hipStream_t s);
// hidden_norm.hip (rajni_hip_mlpnorm.h): the first n columns of every row of x [rows, ld] normalised in place - the norm between
// FC1's epilogue and FC2; columns [n, ld) keep their zeros
int launch_hidden_norm(int kind, void* x, long ld, const float* w, const float* b, long rows, int n, float eps, int dtype, int x_f32,
                       hipStream_t s);
// image.hip: position-embedding rows [prefix + sh * sw, C] -> [prefix + dh * dw, C], bicubic with antialiasing (timm's
// resample_abs_pos_embed); prefix rows copied
int launch_resample_pos_embed(const void* src, int sh, int sw, void* dst, int dh, int dw, int C, int prefix, int dtype, hipStream_t s);
