// Position-embedding resample for inputs whose token grid differs from the checkpoint's (include/rajni_hip_image.h): timm's
// resample_abs_pos_embed - F.interpolate(mode="bicubic", antialias=True, align_corners=False) on the fp32 patch rows, the
// prefix rows passed through - as one launch.  It runs once per (grid, device, dtype); the wrapper caches the result.
//
// The rule is separable.  Per axis, scale = n_in / n_out, support = 2 * max(scale, 1), output i has its centre at
// c = scale * (i + 0.5) and the taps j in [max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)), weighted
// k((j - c + 0.5) / max(scale, 1)) / sum, k the Keys cubic with a = -0.5.  A tap range never exceeds n_in <= 128 entries.
#include "common.h"

namespace {

constexpr int RS_THREADS = 128;                       // >= RAJNI_RESAMPLE_MAX_GRID: thread t evaluates tap t of both axes
static_assert(RS_THREADS >= RAJNI_RESAMPLE_MAX_GRID, "one thread per tap");

__device__ __forceinline__ double keys_cubic(double t) {
  const double a = -0.5;
  t = fabs(t);
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}

// taps [lo, lo + n) of output i on an axis of n_in -> n_out samples; raw[t] = the unnormalised fp64 weight of tap t (t < n)
__device__ __forceinline__ void axis_taps(int i, int n_in, int n_out, int tid, double* raw, int& lo, int& n) {
  const double scale = (double)n_in / (double)n_out;
  const double support = scale >= 1.0 ? 2.0 * scale : 2.0, inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  const double c = scale * ((double)i + 0.5);
  const int a = (int)(c - support + 0.5), b = (int)(c + support + 0.5);
  lo = a > 0 ? a : 0;
  n = (b < n_in ? b : n_in) - lo;
  if (tid < n) raw[tid] = keys_cubic(((double)(lo + tid) - c + 0.5) * inv);
}

// One workgroup per output row.  Rows [0, copy_rows) are copied (the prefix rows; every row when the grids are equal).  A
// patch row builds its two weight tables in LDS - fp64, the sum in ascending tap order, one rounding to fp32 - and then every
// thread owns 16-byte chunks of the row: fp32 FMA over the source rows (outer) and columns (inner), ascending, the weight of a
// tap pair wy * wx rounded to fp32 first.  One store per chunk.
template <typename T>
__global__ void __launch_bounds__(RS_THREADS) resample_pos_kernel(const T* __restrict__ src, T* __restrict__ dst, int sh, int sw, int dh,
                                                                  int dw, int C, int prefix, int copy_rows) {
  __shared__ double raw[2][RS_THREADS];
  __shared__ float wy[RS_THREADS], wx[RS_THREADS];
  const int tid = threadIdx.x, row = blockIdx.x;
  if (row < copy_rows) {   // (workgroup-uniform)
    const int n16 = C * (int)sizeof(T) / 16;
    const uint4* s = reinterpret_cast<const uint4*>(src + (long)row * C);
    uint4* d = reinterpret_cast<uint4*>(dst + (long)row * C);
    for (int c = tid; c < n16; c += RS_THREADS) d[c] = s[c];
    return;
  }
  const int t = row - prefix, oy = t / dw, ox = t - oy * dw;
  int y0, ny, x0, nx;
  axis_taps(oy, sh, dh, tid, raw[0], y0, ny);
  axis_taps(ox, sw, dw, tid, raw[1], x0, nx);
  __syncthreads();
  if (tid < ny) {
    double sum = 0.0;
    for (int j = 0; j < ny; ++j) sum += raw[0][j];
    wy[tid] = (float)(raw[0][tid] / sum);
  }
  if (tid < nx) {
    double sum = 0.0;
    for (int k = 0; k < nx; ++k) sum += raw[1][k];
    wx[tid] = (float)(raw[1][tid] / sum);
  }
  __syncthreads();
  const int nchunk = C >> 3;
  for (int c = tid; c < nchunk; c += RS_THREADS) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int j = 0; j < ny; ++j) {
      const T* srow = src + ((long)prefix + (long)(y0 + j) * sw + x0) * C + c * 8;
      const float wj = wy[j];
      for (int k = 0; k < nx; ++k) {
        const float w = wj * wx[k];
        float v[8];
        load8<T>(srow + (long)k * C, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, v[e], acc[e]);
      }
    }
    store8<T>(dst + (long)row * C + c * 8, acc);
  }
}

}  // namespace

int launch_resample_pos_embed(const void* src, int sh, int sw, void* dst, int dh, int dw, int C, int prefix, int dtype, hipStream_t s) {
  const char* who = "rajni_resample_pos_embed";
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  RAJNI_REQUIRE(sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1 && sh <= RAJNI_RESAMPLE_MAX_GRID && sw <= RAJNI_RESAMPLE_MAX_GRID &&
                    dh <= RAJNI_RESAMPLE_MAX_GRID && dw <= RAJNI_RESAMPLE_MAX_GRID,
                RAJNI_ERR_UNSUPPORTED, "%s: grids must be 1..%d per axis on both sides (%d x %d -> %d x %d)", who,
                RAJNI_RESAMPLE_MAX_GRID, sh, sw, dh, dw);
  RAJNI_REQUIRE(C > 0 && C % 8 == 0, RAJNI_ERR_UNSUPPORTED, "%s: C %% 8 == 0 required (C=%d)", who, C);
  RAJNI_REQUIRE(prefix >= 0 && prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID, "%s: prefix_rows must be 0..%d (%d)", who,
                RAJNI_MAX_PREFIX, prefix);
  RAJNI_REQUIRE(src && dst, RAJNI_ERR_INVALID, "%s: null pointer", who);
  const int rows = prefix + dh * dw;
  const int copy_rows = (sh == dh && sw == dw) ? rows : prefix;   // equal grids: the source's bits
  const double es = dtype == RAJNI_F32 ? 4.0 : 2.0;
  ProfScope prof(KC_CLS_POS, s, 0.0, es * C * ((double)rows + (double)prefix + (double)sh * sw));
  const dim3 grid(rows), block(RS_THREADS);
  if (dtype == RAJNI_F32)
    hipLaunchKernelGGL(resample_pos_kernel<float>, grid, block, 0, s, (const float*)src, (float*)dst, sh, sw, dh, dw, C, prefix, copy_rows);
  else if (dtype == RAJNI_F16)
    hipLaunchKernelGGL(resample_pos_kernel<f16_t>, grid, block, 0, s, (const f16_t*)src, (f16_t*)dst, sh, sw, dh, dw, C, prefix, copy_rows);
  else
    hipLaunchKernelGGL(resample_pos_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)src, (bf16_t*)dst, sh, sw, dh, dw, C, prefix, copy_rows);
  RAJNI_CHECK_LAUNCH("resample_pos_kernel");
  return RAJNI_OK;
}
