// Row kernels of the timm VisionTransformer options the reference drops:
//   qk_norm           attn.q_norm / attn.k_norm: LayerNorm over the head dim, in place on the q and k thirds of qkv
//   layernorm_stream  norm_pre: LayerNorm written back into the residual stream
//   pool_norm         the head's norm -> pool ('token' or 'avg' over the surviving patch tokens) -> fc_norm
// All statistics are fp32 and two-pass like layernorm_kernel (rowops.hip); every reduction has one fixed order, so the
// same input gives the same bits whatever the batch around it.
#include "common.h"

namespace {

// ---- sums over LW consecutive lanes (LW = 4, 8, 16; inside one 16-lane DPP row), no LDS ---------------------------
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: after each step every lane of the (growing)
// set holds the same bits - fp32 addition is commutative, and the operands of each add are the two halves' sums.
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int LW> __device__ __forceinline__ float group_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  if constexpr (LW >= 8) v += dpp_f<0x141>(v);
  if constexpr (LW >= 16) v += dpp_f<0x140>(v);
  return v;
}

// One (token, head) group of D elements per LW-lane slot, 8 elements (16 bytes of a 16-bit type) per lane; lanes past D / 8
// of a slot idle (D = 72, 80, 88 ...: 9, 10, 11 of 16 lanes).  D = 64 is LW = 8 with every lane busy: a group is one 128-byte
// line of bf16, a wave instruction touches 8 whole consecutive lines.  R groups per slot are in flight together - like
// LayerNorm this kernel is bound by latency, not by bandwidth, at one group per slot.
// Groups are numbered g = row * 2H + h2 over the q heads (h2 < H) and k heads (h2 >= H) of a row: the first 2C elements
// of each 3C-element row; v is never touched.  Each element is read and written by the same lane: in place is safe.
template <typename T, int LW, int R>
__global__ void __launch_bounds__(256) qk_norm_kernel(T* qkv, const float* __restrict__ qw, const float* __restrict__ qb,
                                                      const float* __restrict__ kw, const float* __restrict__ kb,
                                                      int groups, int H, int D, float eps) {
  constexpr int SLOTS = 64 / LW;
  const int lane = threadIdx.x & 63, slot = lane / LW, sl = lane % LW;
  const int g0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (SLOTS * R);   // (the launcher keeps groups below 2^31 - 2^10)
  if (g0 >= groups) return;                               // wave-uniform: the DPP sums below run with all 64 lanes
  const bool busy = sl * 8 < D;
  const int H2 = 2 * H;
  const long ld = 3L * H * D;
  float v[R][8];
  T* at[R];
  int hh[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int g = g0 + r * SLOTS + slot;
    if (g >= groups) g = groups - 1;                      // clamped: a short last wave re-reads the last group (and stores nothing)
    const int row = g / H2;
    hh[r] = g - row * H2;
    at[r] = qkv + (long)row * ld + hh[r] * D + sl * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[r][j] = 0.f;
    if (busy) load8<T>(at[r], v[r]);
  }
  const float inv_d = 1.0f / (float)D;
  float mean[R], rstd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[r][j];
    mean[r] = s;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) mean[r] = group_sum<LW>(mean[r]) * inv_d;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float ss = 0.f;
    if (busy) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[r][j] - mean[r];
        ss += d * d;
      }
    }
    rstd[r] = ss;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) rstd[r] = rsqrtf(group_sum<LW>(rstd[r]) * inv_d + eps);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool live = busy && g0 + r * SLOTS + slot < groups;
    if (live) {
      const bool isq = hh[r] < H;
      const float* w = isq ? qw : kw;
      const float* b = isq ? qb : kb;
      float wv[8], bv[8], o[8];
      load8<float>(w + sl * 8, wv);
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = 0.f;
      if (b != nullptr) load8<float>(b + sl * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaf((v[r][j] - mean[r]) * rstd[r], wv[j], bv[j]);
      store8<T>(at[r], o);
    }
  }
}

constexpr int QK_NORM_R4_GROUPS = 65536;   // launches of at least this many groups run four groups per slot
constexpr int LS_MAX_CHUNKS = 4;  // 16-byte chunks per lane: C <= 2048, as in rowops.hip

// the row a wave holds in v[][] (chunks c = lane + 64 i < nchunk) -> its LayerNorm, in place in the registers
// RMS (rajni_hip_norm.h): v -> (v * rsqrt(mean(v^2) + eps)) * w instead - no mean, b never read; the sum of squares in the
// order of the sums below
template <bool RMS = false>
__device__ __forceinline__ void wave_layernorm(float (&v)[LS_MAX_CHUNKS][8], int lane, int nchunk, int C,
                                               const float* __restrict__ w, const float* __restrict__ b, float eps) {
  if constexpr (RMS) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < LS_MAX_CHUNKS; ++i)
      if (lane + i * 64 < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
      }
    const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LS_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float wv[8];
        load8<float>(w + c * 8, wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = (v[i][j] * rstd) * wv[j];
      }
    }
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  const float mean = wave_sum(sum) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[i][j] - mean;
        ss += d * d;
      }
    }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8];
      load8<float>(w + c * 8, wv);
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = 0.f;
      if (b != nullptr) load8<float>(b + c * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = fmaf((v[i][j] - mean) * rstd, wv[j], bv[j]);
    }
  }
}

// x[row] = LayerNorm(x[row]) in the stream's own type; a row is owned by one wave and held in registers between its
// load and its store, so in place is safe
template <typename T, bool RMS = false>
__global__ void __launch_bounds__(256) layernorm_stream_kernel(T* x, const float* __restrict__ w, const float* __restrict__ b,
                                                               int rows, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nchunk = C >> 3;
  T* xr = x + (long)row * C;
  float v[LS_MAX_CHUNKS][8];
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) load8<T>(xr + (lane + i * 64) * 8, v[i]);
  wave_layernorm<RMS>(v, lane, nchunk, C, w, b, eps);
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) store8<T>(xr + (lane + i * 64) * 8, v[i]);
}

// patch_embed.norm (rajni_hip_norm.h): x[b, P + j] = norm(x[b, P + j]) + pos[pos_off + j] for the N - P patch rows of every image
// of the stream x [B, N, C], in place and in the stream's own type; the P prefix rows are not touched.  pos rows are in the
// model's 16-bit type TP (float with an fp32 model).  One wave per patch row: the row waits in registers between its load and
// its store, the norm is wave_layernorm's and the position row is added in fp32 before the one rounding of the store.
template <typename T, typename TP, bool RMS>
__global__ void __launch_bounds__(256) embed_norm_kernel(T* x, const float* __restrict__ w, const float* __restrict__ b,
                                                         const TP* __restrict__ pos, int pos_off, int B, int N, int P, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int patches = N - P;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * patches) return;
  const int img = (int)(row / patches), j = (int)(row - (long)img * patches);
  const int nchunk = C >> 3;
  T* xr = x + ((long)img * N + P + j) * C;
  const TP* pr = pos + (long)(pos_off + j) * C;
  float v[LS_MAX_CHUNKS][8];
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) load8<T>(xr + (lane + i * 64) * 8, v[i]);
  wave_layernorm<RMS>(v, lane, nchunk, C, w, b, eps);
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) {
      float pv[8];
      load8<TP>(pr + (lane + i * 64) * 8, pv);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] += pv[e];
      store8<T>(xr + (lane + i * 64) * 8, v[i]);
    }
}

// One workgroup of 8 waves per image.  out[img] = fc_norm(mean_{r0 <= r < r1} norm(x[img, r])), either norm optional.
// Summation order (fixed): wave k adds its rows r0 + k, r0 + k + 8, ... in ascending order; then s_k += s_{k+4} (k < 4);
// then ((s_0 + s_1) + s_2) + s_3.  'token' pooling is r0 = 0, r1 = 1: one row, the sums are that row; 'avg' is r0 = the number
// of prefix tokens (CLS + registers), r1 = N.
constexpr int POOL_WAVES = 8;
template <typename TX, typename TY, bool RMS = false>
__global__ void __launch_bounds__(64 * POOL_WAVES) pool_norm_kernel(const TX* __restrict__ x, int N, int C, int r0, int r1,
                                                                   const float* __restrict__ nw, const float* __restrict__ nb, float neps,
                                                                   const float* __restrict__ fw, const float* __restrict__ fb, float feps,
                                                                   TY* __restrict__ out) {
  __shared__ float red[4][64 * 8 * LS_MAX_CHUNKS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nchunk = C >> 3;
  const TX* xi = x + (long)blockIdx.x * N * C;
  float acc[LS_MAX_CHUNKS][8];
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  for (int r = r0 + wave; r < r1; r += POOL_WAVES) {
    float v[LS_MAX_CHUNKS][8];
#pragma unroll
    for (int i = 0; i < LS_MAX_CHUNKS; ++i)
      if (lane + i * 64 < nchunk) load8<TX>(xi + (long)r * C + (lane + i * 64) * 8, v[i]);
    if (nw != nullptr) wave_layernorm<RMS>(v, lane, nchunk, C, nw, nb, neps);
#pragma unroll
    for (int i = 0; i < LS_MAX_CHUNKS; ++i)
      if (lane + i * 64 < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] += v[i][j];
      }
  }
  // waves 4..7 -> LDS -> waves 0..3; waves 1..3 -> LDS -> wave 0   (each element is written and read by the same lane index)
  for (int step = 0; step < 2; ++step) {
    const bool writer = step == 0 ? wave >= 4 : (wave >= 1 && wave < 4);
    if (writer) {
#pragma unroll
      for (int i = 0; i < LS_MAX_CHUNKS; ++i)
        if (lane + i * 64 < nchunk) {
#pragma unroll
          for (int j = 0; j < 8; ++j) red[wave & 3][((lane + i * 64) << 3) + j] = acc[i][j];
        }
    }
    __syncthreads();
    if (step == 0 && wave < 4) {
#pragma unroll
      for (int i = 0; i < LS_MAX_CHUNKS; ++i)
        if (lane + i * 64 < nchunk) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] += red[wave][((lane + i * 64) << 3) + j];
        }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  const float inv = 1.0f / (float)(r1 - r0);
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float s = acc[i][j];
#pragma unroll
        for (int k = 1; k < 4; ++k) s += red[k][((lane + i * 64) << 3) + j];
        acc[i][j] = r1 - r0 > 1 ? s * inv : s;
      }
    }
  if (fw != nullptr) wave_layernorm<RMS>(acc, lane, nchunk, C, fw, fb, feps);
  TY* o = out + (long)blockIdx.x * C;
#pragma unroll
  for (int i = 0; i < LS_MAX_CHUNKS; ++i)
    if (lane + i * 64 < nchunk) store8<TY>(o + (lane + i * 64) * 8, acc[i]);
}

template <typename T, int LW>
void launch_qk_norm_t(void* qkv, const float* qw, const float* qb, const float* kw, const float* kb, int groups, int H, int D,
                      float eps, hipStream_t s) {
  constexpr int SLOTS = 64 / LW;
  // four groups per slot in flight once the launch has waves to spare (>= 8 waves per CU of 256 left at R = 4)
  if (groups >= QK_NORM_R4_GROUPS) {
    const int waves = (groups + SLOTS * 4 - 1) / (SLOTS * 4);
    hipLaunchKernelGGL((qk_norm_kernel<T, LW, 4>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (T*)qkv, qw, qb, kw, kb,
                       groups, H, D, eps);
  } else {
    const int waves = (groups + SLOTS - 1) / SLOTS;
    hipLaunchKernelGGL((qk_norm_kernel<T, LW, 1>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (T*)qkv, qw, qb, kw, kb,
                       groups, H, D, eps);
  }
}
template <typename T>
void launch_qk_norm_lw(void* qkv, const float* qw, const float* qb, const float* kw, const float* kb, int groups, int H, int D,
                       float eps, hipStream_t s) {
  if (D <= 32) launch_qk_norm_t<T, 4>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
  else if (D <= 64) launch_qk_norm_t<T, 8>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
  else launch_qk_norm_t<T, 16>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
}

template <typename TX, bool RMS = false>
void launch_pool_norm_t(const void* x, int B, int N, int C, int r0, int r1, const float* nw, const float* nb, float neps,
                        const float* fw, const float* fb, float feps, void* out, int dtype, hipStream_t s) {
  const dim3 grid(B), block(64 * POOL_WAVES);
  if (dtype == RAJNI_F32)
    hipLaunchKernelGGL((pool_norm_kernel<TX, float, RMS>), grid, block, 0, s, (const TX*)x, N, C, r0, r1, nw, nb, neps, fw, fb, feps, (float*)out);
  else if (dtype == RAJNI_F16)
    hipLaunchKernelGGL((pool_norm_kernel<TX, f16_t, RMS>), grid, block, 0, s, (const TX*)x, N, C, r0, r1, nw, nb, neps, fw, fb, feps, (f16_t*)out);
  else
    hipLaunchKernelGGL((pool_norm_kernel<TX, bf16_t, RMS>), grid, block, 0, s, (const TX*)x, N, C, r0, r1, nw, nb, neps, fw, fb, feps, (bf16_t*)out);
}

}  // namespace

int launch_qk_norm(void* qkv, const float* qw, const float* qb, const float* kw, const float* kb, int rows, int H, int D,
                   float eps, int dtype, hipStream_t s) {
  // (shape limits before the pointers: a refused shape is refused whatever else the call holds)
  RAJNI_REQUIRE(rows > 0 && H > 0, RAJNI_ERR_INVALID, "rajni_qk_norm: bad shape (rows=%d H=%d)", rows, H);
  RAJNI_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_qk_norm: need a head dim that is a multiple of 8 up to 128 (D=%d)", D);
  // the kernel indexes (token, head) groups with 32-bit ints and rounds the count up to whole workgroups
  RAJNI_REQUIRE((long)rows * 2 * H < RAJNI_QK_NORM_MAX_GROUPS, RAJNI_ERR_UNSUPPORTED,
                "rajni_qk_norm: %ld (token, head) groups (rows * 2 * H) - the limit is %ld", (long)rows * 2 * H,
                (long)RAJNI_QK_NORM_MAX_GROUPS - 1);
  RAJNI_REQUIRE(qkv && qw && kw, RAJNI_ERR_INVALID, "rajni_qk_norm: null pointer");
  const int groups = rows * 2 * H;
  const double es = dtype == RAJNI_F32 ? 4.0 : 2.0;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * groups * D, 2.0 * es * groups * (double)D);
  if (dtype == RAJNI_F32) launch_qk_norm_lw<float>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
  else if (dtype == RAJNI_F16) launch_qk_norm_lw<f16_t>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
  else launch_qk_norm_lw<bf16_t>(qkv, qw, qb, kw, kb, groups, H, D, eps, s);
  RAJNI_CHECK_LAUNCH("qk_norm_kernel");
  return RAJNI_OK;
}

int launch_layernorm_stream(void* x, const float* w, const float* b, int rows, int C, float eps, int x_f32, int dtype, hipStream_t s,
                            int kind) {
  RAJNI_REQUIRE(x && w, RAJNI_ERR_INVALID, "rajni_layernorm_stream: null pointer");
  RAJNI_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 64 * 8 * LS_MAX_CHUNKS, RAJNI_ERR_UNSUPPORTED,
                "rajni_layernorm_stream: need C %% 8 == 0, C <= 2048 (C=%d)", C);
  const bool f32 = dtype == RAJNI_F32 || x_f32;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * rows * C, (f32 ? 8.0 : 4.0) * rows * C);
  const dim3 grid((rows + 3) / 4), block(256);
  if (kind == RAJNI_NORM_RMS) {
    const float* nob = nullptr;
    if (f32) hipLaunchKernelGGL((layernorm_stream_kernel<float, true>), grid, block, 0, s, (float*)x, w, nob, rows, C, eps);
    else if (dtype == RAJNI_F16) hipLaunchKernelGGL((layernorm_stream_kernel<f16_t, true>), grid, block, 0, s, (f16_t*)x, w, nob, rows, C, eps);
    else hipLaunchKernelGGL((layernorm_stream_kernel<bf16_t, true>), grid, block, 0, s, (bf16_t*)x, w, nob, rows, C, eps);
  } else if (f32) hipLaunchKernelGGL((layernorm_stream_kernel<float>), grid, block, 0, s, (float*)x, w, b, rows, C, eps);
  else if (dtype == RAJNI_F16) hipLaunchKernelGGL((layernorm_stream_kernel<f16_t>), grid, block, 0, s, (f16_t*)x, w, b, rows, C, eps);
  else hipLaunchKernelGGL((layernorm_stream_kernel<bf16_t>), grid, block, 0, s, (bf16_t*)x, w, b, rows, C, eps);
  RAJNI_CHECK_LAUNCH("layernorm_stream_kernel");
  return RAJNI_OK;
}

int launch_pool_norm(const void* x, int B, int N, int C, int pool, const float* nw, const float* nb, float neps,
                     const float* fw, const float* fb, float feps, void* out, int x_f32, int dtype, hipStream_t s, int num_prefix,
                     int kind) {
  RAJNI_REQUIRE(x && out, RAJNI_ERR_INVALID, "rajni_pool_norm: null pointer");
  // (0: a sequence without a class row, from rajni_hip_query.h's forward alone - rajni_pool_norm_prefix refuses it itself)
  RAJNI_REQUIRE(num_prefix >= 0 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_pool_norm: num_prefix must be 0..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(pool == RAJNI_POOL_TOKEN || pool == RAJNI_POOL_AVG, RAJNI_ERR_UNSUPPORTED,
                "rajni_pool_norm: pool must be RAJNI_POOL_TOKEN or RAJNI_POOL_AVG (%d)", pool);
  RAJNI_REQUIRE(B > 0 && N > 0 && C > 0 && C % 8 == 0 && C <= 64 * 8 * LS_MAX_CHUNKS, RAJNI_ERR_UNSUPPORTED,
                "rajni_pool_norm: need C %% 8 == 0, C <= 2048 (C=%d)", C);
  RAJNI_REQUIRE(pool == RAJNI_POOL_TOKEN || N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "rajni_pool_norm: 'avg' needs at least one patch token (N=%d, %d prefix tokens)", N, num_prefix);
  const int r0 = pool == RAJNI_POOL_AVG ? num_prefix : 0, r1 = pool == RAJNI_POOL_AVG ? N : 1;
  const bool f32 = dtype == RAJNI_F32 || x_f32;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * B * (r1 - r0) * C, (f32 ? 4.0 : 2.0) * B * (r1 - r0) * C);
  if (kind == RAJNI_NORM_RMS) {   // (neither bias is read)
    if (f32) launch_pool_norm_t<float, true>(x, B, N, C, r0, r1, nw, nullptr, neps, fw, nullptr, feps, out, dtype, s);
    else if (dtype == RAJNI_F16) launch_pool_norm_t<f16_t, true>(x, B, N, C, r0, r1, nw, nullptr, neps, fw, nullptr, feps, out, dtype, s);
    else launch_pool_norm_t<bf16_t, true>(x, B, N, C, r0, r1, nw, nullptr, neps, fw, nullptr, feps, out, dtype, s);
  } else if (f32) launch_pool_norm_t<float>(x, B, N, C, r0, r1, nw, nb, neps, fw, fb, feps, out, dtype, s);
  else if (dtype == RAJNI_F16) launch_pool_norm_t<f16_t>(x, B, N, C, r0, r1, nw, nb, neps, fw, fb, feps, out, dtype, s);
  else launch_pool_norm_t<bf16_t>(x, B, N, C, r0, r1, nw, nb, neps, fw, fb, feps, out, dtype, s);
  RAJNI_CHECK_LAUNCH("pool_norm_kernel");
  return RAJNI_OK;
}

// the patch rows of the stream x [B, N, C] (fp32 when x_f32, else `dtype`) through patch_embed.norm, then + pos[pos_off + j]
// (pos in `dtype`); see embed_norm_kernel
int launch_embed_norm(int kind, void* x, const float* w, const float* b, const void* pos, int pos_off, int B, int N, int num_prefix,
                      int C, float eps, int dtype, int x_f32, hipStream_t s) {
  RAJNI_REQUIRE(kind == RAJNI_NORM_LAYERNORM || kind == RAJNI_NORM_RMS, RAJNI_ERR_INVALID,
                "rajni_embed_norm: kind must be RAJNI_NORM_LAYERNORM or RAJNI_NORM_RMS (%d)", kind);
  RAJNI_REQUIRE(x && w && pos, RAJNI_ERR_INVALID, "rajni_embed_norm: null pointer");
  RAJNI_REQUIRE(B > 0 && num_prefix >= 0 && num_prefix <= RAJNI_MAX_PREFIX && N > num_prefix && pos_off >= 0, RAJNI_ERR_INVALID,
                "rajni_embed_norm: need B > 0, 0 <= num_prefix <= %d, N > num_prefix and pos_off >= 0 (B=%d N=%d num_prefix=%d pos_off=%d)",
                RAJNI_MAX_PREFIX, B, N, num_prefix, pos_off);
  RAJNI_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * LS_MAX_CHUNKS, RAJNI_ERR_UNSUPPORTED,
                "rajni_embed_norm: need C %% 8 == 0, C <= 2048 (C=%d)", C);
  const long rows = (long)B * (N - num_prefix);
  RAJNI_REQUIRE((rows + 3) / 4 < (1L << 31), RAJNI_ERR_UNSUPPORTED, "rajni_embed_norm: too many rows (%ld)", rows);
  const bool f32 = dtype == RAJNI_F32 || x_f32;
  ProfScope prof(KC_LAYERNORM, s, 9.0 * rows * C, ((f32 ? 8.0 : 4.0) + (dtype == RAJNI_F32 ? 4.0 : 2.0)) * rows * C);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const float* nob = nullptr;
#define RAJNI_EMBED_NORM(T, TP)                                                                                                 \
  do {                                                                                                                          \
    if (kind == RAJNI_NORM_RMS)                                                                                                 \
      hipLaunchKernelGGL((embed_norm_kernel<T, TP, true>), grid, block, 0, s, (T*)x, w, nob, (const TP*)pos, pos_off, B, N,      \
                         num_prefix, C, eps);                                                                                   \
    else                                                                                                                        \
      hipLaunchKernelGGL((embed_norm_kernel<T, TP, false>), grid, block, 0, s, (T*)x, w, b, (const TP*)pos, pos_off, B, N,       \
                         num_prefix, C, eps);                                                                                   \
  } while (0)
  if (dtype == RAJNI_F32) RAJNI_EMBED_NORM(float, float);
  else if (dtype == RAJNI_F16 && x_f32) RAJNI_EMBED_NORM(float, f16_t);
  else if (dtype == RAJNI_F16) RAJNI_EMBED_NORM(f16_t, f16_t);
  else if (x_f32) RAJNI_EMBED_NORM(float, bf16_t);
  else RAJNI_EMBED_NORM(bf16_t, bf16_t);
#undef RAJNI_EMBED_NORM
  RAJNI_CHECK_LAUNCH("embed_norm_kernel");
  return RAJNI_OK;
}
