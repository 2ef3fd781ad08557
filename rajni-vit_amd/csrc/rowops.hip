// HBM-bound row kernels: LayerNorm (SURVEY k1,k17,k20) and the keep_idx row gather (k10,k15).
// One wave per row, 16-byte accesses, everything else in registers.
#include "common.h"

namespace {

#ifndef RAJNI_LN8_ROWS
#define RAJNI_LN8_ROWS 2  // ... of the e4m3-output LayerNorm
#endif
#ifndef RAJNI_LN_ROWS
#define RAJNI_LN_ROWS 2   // rows per wave of the benchmark path's LayerNorm (1 = the one-row kernel; 3: 728, 4: 750 us per forward against 715)
#endif
constexpr int LN_MAX_CHUNKS = 4;  // 16-byte chunks per lane: C <= 64*8*4 = 2048

// the RMS forms' last pass: the row a wave holds in v -> (v * rstd) * w, rounded once to TY, as whole 16-byte stores
template <typename TY>
__device__ __forceinline__ void rms_store_row(const float (&v)[LN_MAX_CHUNKS][8], int lane, int nchunk, float rstd,
                                              const float* __restrict__ w, TY* __restrict__ yr) {
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], o[8];
      load8<float>(w + c * 8, wv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[i][j] * rstd) * wv[j];
      store8<TY>(yr + c * 8, o);
    }
  }
}
// ... and their first: the row -> v, and rsqrt(mean(v^2) + eps)
template <typename TX>
__device__ __forceinline__ float rms_load_row(const TX* __restrict__ xr, float (&v)[LN_MAX_CHUNKS][8], int lane, int nchunk, int C,
                                              float eps) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      load8<TX>(xr + c * 8, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  return rsqrtf(wave_sum(ss) / (float)C + eps);
}

// RMS (rajni_hip_norm.h): y = (x * rsqrt(mean(x^2) + eps)) * w - no mean, and b is never read.  The sum of squares runs in the
// order of the LayerNorm sums: a lane's chunks in order, their 8 elements in order, then wave_sum.  The same holds for every
// kernel below that takes the flag; RMS = false is the code as it always was.
template <typename TX, typename TY, bool RMS = false>
__global__ void __launch_bounds__(256) layernorm_kernel(const TX* __restrict__ x, long xs,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ b,
                                                        TY* __restrict__ y, int rows, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nchunk = C >> 3;
  const TX* xr = x + (long)row * xs;
  float v[LN_MAX_CHUNKS][8];
  if constexpr (RMS) {
    const float rstd = rms_load_row<TX>(xr, v, lane, nchunk, C, eps);
    rms_store_row<TY>(v, lane, nchunk, rstd, w, y + (long)row * C);
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      load8<TX>(xr + c * 8, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[i][j] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
  TY* yr = y + (long)row * C;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8], o[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaf((v[i][j] - mean) * rstd, wv[j], bv[j]);
      store8<TY>(yr + c * 8, o);
    }
  }
}

// R rows per wave (fp32 rows in, bf16 out, C <= 1024): R times the loads in flight per wave.  The one-row kernel keeps 3 KB per wave in
// flight at 8 waves per SIMD - Little's law put that short of the HBM rate: LayerNorm was a latency-bound kernel, not a bandwidth-bound one
// (two rows, still 64 VGPRs = 8 waves: 772 -> 715 us per forward; the e4m3-output kernel, with four wave reductions per row, loses with two).
template <int NC, int R, typename TY = bf16_t, bool RMS = false>
__global__ void __launch_bounds__(256) layernorm_rows_kernel(const float* __restrict__ x, long xs, const float* __restrict__ w,
                                                             const float* __restrict__ b, TY* __restrict__ y, int rows, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + wave) * R;
  if (r0 >= rows) return;
  const int nchunk = C >> 3;
  float v[R][NC][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float* xr = x + (long)(r0 + r < rows ? r0 + r : rows - 1) * xs;      // clamped: a short last group re-reads its last row
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) load8<float>(xr + c * 8, v[r][i]);
    }
  }
  float mean[R], rstd[R];
  if constexpr (RMS) {   // one reduction per row, no mean, no bias: the RMS form of everything below
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = lane + i * 64;
        if (c < nchunk) {
#pragma unroll
          for (int j = 0; j < 8; ++j) ss += v[r][i][j] * v[r][i][j];
        }
      }
      rstd[r] = rsqrtf(wave_sum(ss) / (float)C + eps);
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float wv[8];
        load8<float>(w + c * 8, wv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (v[r][i][j] * rstd[r]) * wv[j];
          if (r0 + r < rows) store8<TY>(y + (long)(r0 + r) * C + c * 8, o);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[r][i][j];
      }
    }
    mean[r] = wave_sum(sum) / (float)C;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[r][i][j] - mean[r];
          ss += d * d;
        }
      }
    }
    rstd[r] = rsqrtf(wave_sum(ss) / (float)C + eps);
  }
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fmaf((v[r][i][j] - mean[r]) * rstd[r], wv[j], bv[j]);
        if (r0 + r < rows) store8<TY>(y + (long)(r0 + r) * C + c * 8, o);
      }
    }
  }
}

// LayerNorm whose output row is quantised for the fp8 matrix pipe (see rajni_layernorm_fp8 in the header): the
// wave holds the whole normalised row in registers, so the row maximum is one more wave reduction.
//   yscale[r] = max |o| / 448 (1 if 0);  yq = e4m3_rne_sat(o * (1 / yscale[r]))   - the reciprocal is a correctly
//   rounded fp32 division and the product one fp32 multiply, so a host restatement reproduces the bytes;
//   hscale[r] (optional) = (1.0625 * ||o||_2 * wnorm + bmax) / 448: per-row scale of the MLP hidden activations
//   from the Cauchy-Schwarz bound (the margin covers the <= 2^-4 relative change of ||o|| under quantisation).
// NC: 16-byte chunks per lane.  2 serves C <= 1024 - every ViT-B / ViT-L row - in 50 VGPRs instead of 70: 8 waves per SIMD instead of
// 7, and no dead third / fourth chunk iterations: 31 -> 28 us per launch on ViT-B at batch 256 (the bf16-output kernel gains nothing
// from the same change: it sits on the HBM rate; this one was short of waves to cover its four wave reductions per row)
template <typename TX, int NC>
__global__ void __launch_bounds__(256) layernorm_fp8_kernel(const TX* __restrict__ x, long xs,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            unsigned char* __restrict__ yq, float* __restrict__ yscale,
                                                            float* __restrict__ hscale, float wnorm, float bmax,
                                                            int rows, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nchunk = C >> 3;
  const TX* xr = x + (long)row * xs;
  float v[NC][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      load8<TX>(xr + c * 8, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[i][j] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
  float amax = 0.f, osq = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float o = fmaf((v[i][j] - mean) * rstd, wv[j], bv[j]);
        v[i][j] = o;
        amax = fmaxf(amax, fabsf(o));
        osq = fmaf(o, o, osq);
      }
    }
  }
  amax = wave_max(amax);
  osq = wave_sum(osq);
  const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
  const float inv = 1.0f / scale;
  unsigned char* yr = yq + (long)row * C;
  int plo[NC], phi[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    plo[i] = phi[i] = 0;
    const int c = lane + i * 64;
    if (c < nchunk) {
      float q[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = __builtin_amdgcn_fmed3f(v[i][j] * inv, -448.f, 448.f);
      int lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
      int hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
      plo[i] = lo; phi[i] = hi;
    }
  }
  // 16-byte stores: an even lane takes its odd neighbour's 8 bytes (adjacent chunks) - with 8-byte stores a wave
  // instruction wrote half sectors
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    const int nlo = __shfl_down(plo[i], 1, 64), nhi = __shfl_down(phi[i], 1, 64);
    if (c < nchunk && (lane & 1) == 0) {
      if (c + 1 < nchunk) *reinterpret_cast<uint4*>(yr + c * 8) = make_uint4((unsigned)plo[i], (unsigned)phi[i], (unsigned)nlo, (unsigned)nhi);
      else *reinterpret_cast<uint2*>(yr + c * 8) = make_uint2((unsigned)plo[i], (unsigned)phi[i]);
    }
  }
  if (lane == 0) {
    yscale[row] = scale;
    if (hscale != nullptr) {
      const float bound = fmaf(1.0625f * sqrtf(osq), wnorm, bmax);
      hscale[row] = bound > 0.f ? bound / 448.0f : 1.0f;
    }
  }
}

// The e4m3-output LayerNorm with R rows per wave, stage by stage ACROSS the rows (their four wave reductions each overlap instead of
// queueing up): fp32 rows, C <= 1024.  Same arithmetic per row as layernorm_fp8_kernel: the same bytes.
template <int NC, int R>
__global__ void __launch_bounds__(256) layernorm_fp8_rows_kernel(const float* __restrict__ x, long xs, const float* __restrict__ w,
                                                                 const float* __restrict__ b, unsigned char* __restrict__ yq,
                                                                 float* __restrict__ yscale, float* __restrict__ hscale, float wnorm,
                                                                 float bmax, int rows, int C, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + wave) * R;
  if (r0 >= rows) return;
  const int nchunk = C >> 3;
  float v[R][NC][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float* xr = x + (long)(r0 + r < rows ? r0 + r : rows - 1) * xs;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) load8<float>(xr + c * 8, v[r][i]);
    }
  }
  float mean[R], rstd[R], amax[R], osq[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[r][i][j];
      }
    }
    mean[r] = sum;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) mean[r] = wave_sum(mean[r]) / (float)C;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[r][i][j] - mean[r];
          ss += d * d;
        }
      }
    }
    rstd[r] = ss;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) rstd[r] = rsqrtf(wave_sum(rstd[r]) / (float)C + eps);
#pragma unroll
  for (int r = 0; r < R; ++r) { amax[r] = 0.f; osq[r] = 0.f; }
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float o = fmaf((v[r][i][j] - mean[r]) * rstd[r], wv[j], bv[j]);
          v[r][i][j] = o;
          amax[r] = fmaxf(amax[r], fabsf(o));
          osq[r] = fmaf(o, o, osq[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) { amax[r] = wave_max(amax[r]); osq[r] = wave_sum(osq[r]); }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + r;
    const bool live = row < rows;
    const float scale = amax[r] > 0.f ? amax[r] / 448.0f : 1.0f;
    const float inv = 1.0f / scale;
    unsigned char* yr = yq + (long)row * C;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      int lo = 0, hi = 0;
      const int c = lane + i * 64;
      if (c < nchunk) {
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = __builtin_amdgcn_fmed3f(v[r][i][j] * inv, -448.f, 448.f);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
      }
      const int nlo = __shfl_down(lo, 1, 64), nhi = __shfl_down(hi, 1, 64);
      if (live && c < nchunk && (lane & 1) == 0) {
        if (c + 1 < nchunk) *reinterpret_cast<uint4*>(yr + c * 8) = make_uint4((unsigned)lo, (unsigned)hi, (unsigned)nlo, (unsigned)nhi);
        else *reinterpret_cast<uint2*>(yr + c * 8) = make_uint2((unsigned)lo, (unsigned)hi);
      }
    }
    if (live && lane == 0) {
      yscale[row] = scale;
      if (hscale != nullptr) {
        const float bound = fmaf(1.0625f * sqrtf(osq[r]), wnorm, bmax);
        hscale[row] = bound > 0.f ? bound / 448.0f : 1.0f;
      }
    }
  }
}

// dst[b, j, :] = src[b, idx[b, j], :]   rows of `row_chunks` 16-byte chunks; one wave per row
__global__ void __launch_bounds__(256) gather_rows_kernel(const uint4* __restrict__ src,
                                                         const int* __restrict__ idx,
                                                         uint4* __restrict__ dst, int B, int n_src,
                                                         int n_dst, int row_chunks) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long total = (long)B * n_dst;
  for (long r = (long)blockIdx.x * 4 + wave; r < total; r += (long)gridDim.x * 4) {
    const int b = (int)(r / n_dst);
    const int s = idx[r];
    const uint4* sp = src + ((long)b * n_src + s) * row_chunks;
    uint4* dp = dst + r * row_chunks;
    for (int c = lane; c < row_chunks; c += 64) dp[c] = sp[c];
  }
}

// ---- RAJNI_POOL_DENSE (forward.hip): the final norm scattered back to the unpruned sequence ----
// src[b, j] = position in the unpruned sequence of token j of the final stream: the scheduled blocks' selections composed,
// walked from the last scheduled block back to the first (t.idx[0] is the last one's).  One thread per (b, j).  A launch
// walks up to SRC_LEVELS selections; a longer schedule chains launches (`first` = 0: j resumes from src).  Every step is
// clamped to the tokens that entered its block, so a forced selection with a bad index cannot send the next read outside
// the previous level's row.
constexpr int SRC_LEVELS = 4;
struct SrcLevels {
  const int32_t* idx[SRC_LEVELS];   // [B, width] keep_idx (or forced_keep_idx) of a scheduled block
  int width[SRC_LEVELS];            // its row width: prefix tokens + keep
  int nsrc[SRC_LEVELS];             // tokens that entered that block: its values are < nsrc
  int n;
};
__global__ void __launch_bounds__(256) source_idx_kernel(int32_t* __restrict__ src, SrcLevels t, int B, int Nf, int first) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Nf) return;
  const int b = (int)(i / Nf);
  int j = first ? (int)(i - (long)b * Nf) : src[i];
#pragma unroll
  for (int k = 0; k < SRC_LEVELS; ++k)
    if (k < t.n) {
      j = t.idx[k][(long)b * t.width[k] + j];
      j = j < 0 ? 0 : (j >= t.nsrc[k] ? t.nsrc[k] - 1 : j);
    }
  src[i] = j;
}

// y[b, s, :] = norm(x[b, j, :]) where src[b, j] == s, else zeros: one wave per OUTPUT row (b, s) of [B, S, C], so every output
// byte is written exactly once (no memset pass, no atomics, no inverse map).  src[b, :] is strictly ascending (every
// selection is ascending), so the wave binary-searches it for s - wave-uniform: the row index is made scalar, the search runs
// on the scalar unit.  A hit is layernorm_kernel's arithmetic instruction for instruction (load8, two-pass fp32 statistics,
// wave_sum in the same order, fmaf((v - mean) * rstd, w, b)): the same bits.  16-byte stores either way.
// ZERO = false (RAJNI_POOL_DENSE_LAST): a miss stores nothing - layernorm_dropped_kernel wrote that row when its token left.
template <typename TX, typename TY, bool ZERO = true, bool RMS = false>
__global__ void __launch_bounds__(256) layernorm_dense_kernel(const TX* __restrict__ x, const int32_t* __restrict__ src,
                                                              const float* __restrict__ w, const float* __restrict__ b,
                                                              TY* __restrict__ y, int B, int Nf, int S, int C, float eps) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * S) return;
  const int img = (int)(row / S), s = (int)(row - (long)img * S);
  const int32_t* sb = src + (long)img * Nf;
  int lo = 0, hi = Nf;                    // the first j in [0, Nf) with sb[j] >= s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < s) lo = mid + 1; else hi = mid;
  }
  const bool hit = lo < Nf && sb[lo] == s;
  const int nchunk = C >> 3;
  TY* yr = y + row * C;
  if (!hit) {
    if constexpr (ZERO) {
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
        const int c = lane + i * 64;
        if (c < nchunk) store8<TY>(yr + c * 8, z);
      }
    }
    return;
  }
  const TX* xr = x + ((long)img * Nf + lo) * C;
  float v[LN_MAX_CHUNKS][8];
  if constexpr (RMS) {
    const float rstd = rms_load_row<TX>(xr, v, lane, nchunk, C, eps);
    rms_store_row<TY>(v, lane, nchunk, rstd, w, yr);
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      load8<TX>(xr + c * 8, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[i][j] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8], o[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaf((v[i][j] - mean) * rstd, wv[j], bv[j]);
      store8<TY>(yr + c * 8, o);
    }
  }
}

// ---- RAJNI_POOL_DENSE_LAST (forward.hip): the rows a scheduled block drops, through the final norm, at their source rows ----
// x [B, N, C] is the stream that ENTERED the block, keep [B, Np] the block's selection (P prefix slots, then strictly
// ascending patch indices), src [B, N] the position in the unpruned sequence of each entering token (the earlier blocks'
// selections composed).  One wave per INPUT row (b, j), j >= P: the wave binary-searches keep[b, P:] for j, wave-uniform on
// the scalar unit as layernorm_dense_kernel searches src.  A hit (the token stays) stores nothing; a miss writes
// y[b, src[b, j], :] = norm(x[b, j, :]) with layernorm_kernel's arithmetic instruction for instruction (load8, two-pass fp32
// statistics, wave_sum in the same order, fmaf((v - mean) * rstd, w, b)): the bits layernorm_dense_kernel gives the same row.
// What is read from keep and src is clamped as source_idx_kernel clamps: keep values are only compared, and a src value
// outside [0, S) cannot form an address outside y.
template <typename TX, typename TY, bool RMS = false>
__global__ void __launch_bounds__(256) layernorm_dropped_kernel(const TX* __restrict__ x, const int32_t* __restrict__ keep,
                                                                const int32_t* __restrict__ src, const float* __restrict__ w,
                                                                const float* __restrict__ b, TY* __restrict__ y, int B, int N,
                                                                int Np, int P, int S, int C, float eps) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int patches = N - P;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * patches) return;
  const int img = (int)(row / patches), j = P + (int)(row - (long)img * patches);
  const int32_t* kb = keep + (long)img * Np;
  auto kept = [&](int slot) { const int k = kb[slot]; return k < 0 ? 0 : (k >= N ? N - 1 : k); };
  int lo = P, hi = Np;                    // the first slot in [P, Np) with kept(slot) >= j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kept(mid) < j) lo = mid + 1; else hi = mid;
  }
  if (lo < Np && kept(lo) == j) return;   // kept: the row travels on
  int s = src[(long)img * N + j];
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  const int nchunk = C >> 3;
  const TX* xr = x + ((long)img * N + j) * C;
  float v[LN_MAX_CHUNKS][8];
  if constexpr (RMS) {
    const float rstd = rms_load_row<TX>(xr, v, lane, nchunk, C, eps);
    rms_store_row<TY>(v, lane, nchunk, rstd, w, y + ((long)img * S + s) * C);
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      load8<TX>(xr + c * 8, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[i][e];
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[i][e] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
  TY* yr = y + ((long)img * S + s) * C;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float wv[8], bv[8], o[8];
      load8<float>(w + c * 8, wv);
      load8<float>(b + c * 8, bv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf((v[i][e] - mean) * rstd, wv[e], bv[e]);
      store8<TY>(yr + c * 8, o);
    }
  }
}

// ---- rajni_vit_forward_layers (forward.hip): the states behind several blocks, each on the unpruned grid ----
// 8 output elements packed once and stored to several rows: one 16-byte store (two for fp32) each time
template <typename TY> struct Out8 { uint4 q; };
template <> struct Out8<float> { float4 a, b; };
template <typename TY> __device__ __forceinline__ Out8<TY> out8(const float* f) {
  Out8<TY> o;
  o.q = pack8<TY>(f);
  return o;
}
template <> __device__ __forceinline__ Out8<float> out8<float>(const float* f) {
  Out8<float> o;
  o.a = make_float4(f[0], f[1], f[2], f[3]);
  o.b = make_float4(f[4], f[5], f[6], f[7]);
  return o;
}
template <typename TY> __device__ __forceinline__ void put8(TY* p, const Out8<TY>& o) { *reinterpret_cast<uint4*>(p) = o.q; }
template <> __device__ __forceinline__ void put8<float>(float* p, const Out8<float>& o) {
  reinterpret_cast<float4*>(p)[0] = o.a;
  reinterpret_cast<float4*>(p)[1] = o.b;
}

// layernorm_dense_kernel without the norm: y[b, s, :] = the stream row x[b, j, :] rounded once to TY where src[b, j] == s, else
// zeros (ZERO = false: a miss stores nothing).  The same mapping - one wave per OUTPUT row, the scalar binary search over the
// strictly ascending src[b, :] - and one pass of 16-byte loads and 16-byte stores; TX == TY == float is a plain copy.
template <typename TX, typename TY, bool ZERO = true>
__global__ void __launch_bounds__(256) rows_dense_cast_kernel(const TX* __restrict__ x, const int32_t* __restrict__ src,
                                                              TY* __restrict__ y, int B, int Nf, int S, int C) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * S) return;
  const int img = (int)(row / S), s = (int)(row - (long)img * S);
  const int32_t* sb = src + (long)img * Nf;
  int lo = 0, hi = Nf;                    // the first j in [0, Nf) with sb[j] >= s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < s) lo = mid + 1; else hi = mid;
  }
  const bool hit = lo < Nf && sb[lo] == s;
  const int nchunk = C >> 3;
  TY* yr = y + row * C;
  if (!hit) {
    if constexpr (ZERO) {
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
        const int c = lane + i * 64;
        if (c < nchunk) store8<TY>(yr + c * 8, z);
      }
    }
    return;
  }
  const TX* xr = x + ((long)img * Nf + lo) * C;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      float v[8];
      load8<TX>(xr + c * 8, v);
      store8<TY>(yr + c * 8, v);
    }
  }
}

// The rows a scheduled block drops, to several outputs: layernorm_dropped_kernel's mapping (one wave per INPUT row, the scalar
// search of keep[b, P:], the clamps) and, with NORM, its arithmetic instruction for instruction, so a row has the bits that
// kernel gives it; without NORM the row is rounded once to TY.  The finished row stays in registers, packed, and goes as whole
// rows of 16-byte stores to row src[b, j] of every target t.y[k] - each a [B, S, C] slab.  The targets travel by value in the
// kernel arguments and the loop over them is wave-uniform.
struct RowTargets {
  void* y[RAJNI_MAX_LAYERS];
  int n;
};
template <typename TX, typename TY, bool NORM>
__global__ void __launch_bounds__(256) rows_dropped_multi_kernel(const TX* __restrict__ x, const int32_t* __restrict__ keep,
                                                                 const int32_t* __restrict__ src, const float* __restrict__ w,
                                                                 const float* __restrict__ b, RowTargets t, int B, int N, int Np,
                                                                 int P, int S, int C, float eps) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int patches = N - P;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= (long)B * patches) return;
  const int img = (int)(row / patches), j = P + (int)(row - (long)img * patches);
  const int32_t* kb = keep + (long)img * Np;
  auto kept = [&](int slot) { const int k = kb[slot]; return k < 0 ? 0 : (k >= N ? N - 1 : k); };
  int lo = P, hi = Np;                    // the first slot in [P, Np) with kept(slot) >= j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kept(mid) < j) lo = mid + 1; else hi = mid;
  }
  if (lo < Np && kept(lo) == j) return;   // kept: the row travels on
  int s = src[(long)img * N + j];
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  const int nchunk = C >> 3;
  const TX* xr = x + ((long)img * N + j) * C;
  float v[LN_MAX_CHUNKS][8];
  Out8<TY> o8[LN_MAX_CHUNKS];
  if constexpr (NORM) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        load8<TX>(xr + c * 8, v[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v[i][e];
      }
    }
    const float mean = wave_sum(sum) / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[i][e] - mean;
          ss += d * d;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float wv[8], bv[8], o[8];
        load8<float>(w + c * 8, wv);
        load8<float>(b + c * 8, bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf((v[i][e] - mean) * rstd, wv[e], bv[e]);
        o8[i] = out8<TY>(o);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        load8<TX>(xr + c * 8, v[i]);
        o8[i] = out8<TY>(v[i]);
      }
    }
  }
  const long off = ((long)img * S + s) * C;
  for (int k = 0; k < t.n; ++k) {
    TY* yr = static_cast<TY*>(t.y[k]) + off;
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) put8<TY>(yr + c * 8, o8[i]);
    }
  }
}

}  // namespace

static int launch_layernorm_f16(const void* x, long xs, const float* w, const float* b, void* y, int rows,
                                int C, float eps, int x_f32, hipStream_t s);
static int launch_rmsnorm(const void* x, long xs, const float* w, void* y, int rows, int C, float eps, int x_f32, int dtype,
                          hipStream_t s);

int launch_layernorm(const void* x, long xs, const float* w, const float* b, void* y, int rows,
                     int C, float eps, int x_f32, int dtype, hipStream_t s, int kind) {
  RAJNI_REQUIRE(kind == RAJNI_NORM_LAYERNORM || kind == RAJNI_NORM_RMS, RAJNI_ERR_INVALID,
                "rajni_norm_rows: kind must be RAJNI_NORM_LAYERNORM or RAJNI_NORM_RMS (%d)", kind);
  if (kind == RAJNI_NORM_RMS) return launch_rmsnorm(x, xs, w, y, rows, C, eps, x_f32, dtype, s);
  RAJNI_REQUIRE(x && w && b && y, RAJNI_ERR_INVALID, "rajni_layernorm: null pointer");
  RAJNI_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS && xs % 8 == 0,
                RAJNI_ERR_UNSUPPORTED, "rajni_layernorm: need C %% 8 == 0, C <= 2048, stride %% 8 == 0 (C=%d)", C);
  const bool f32io = dtype == RAJNI_F32;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * rows * C, (f32io ? 8.0 : (x_f32 ? 6.0 : 4.0)) * rows * C);
  const dim3 grid((rows + 3) / 4), block(256);
  if (dtype == RAJNI_F16) return launch_layernorm_f16(x, xs, w, b, y, rows, C, eps, x_f32, s);
  if (f32io)
    hipLaunchKernelGGL((layernorm_kernel<float, float>), grid, block, 0, s, (const float*)x, xs, w, b, (float*)y, rows, C, eps);
  else if (x_f32 && RAJNI_LN_ROWS > 1 && C <= 1024 && rows >= 4096)
    hipLaunchKernelGGL((layernorm_rows_kernel<2, RAJNI_LN_ROWS>), dim3((rows + 4 * RAJNI_LN_ROWS - 1) / (4 * RAJNI_LN_ROWS)), block, 0, s,
                       (const float*)x, xs, w, b, (bf16_t*)y, rows, C, eps);
  else if (x_f32)
    hipLaunchKernelGGL((layernorm_kernel<float, bf16_t>), grid, block, 0, s, (const float*)x, xs, w, b, (bf16_t*)y, rows, C, eps);
  else
    hipLaunchKernelGGL((layernorm_kernel<bf16_t, bf16_t>), grid, block, 0, s, (const bf16_t*)x, xs, w, b, (bf16_t*)y, rows, C, eps);
  RAJNI_CHECK_LAUNCH("layernorm_kernel");
  return RAJNI_OK;
}
// fp16 models: the same kernels and the same choice, fp16 output (and input when the stream is fp16)
static int launch_layernorm_f16(const void* x, long xs, const float* w, const float* b, void* y, int rows,
                                int C, float eps, int x_f32, hipStream_t s) {
  const dim3 grid((rows + 3) / 4), block(256);
  if (x_f32 && RAJNI_LN_ROWS > 1 && C <= 1024 && rows >= 4096)
    hipLaunchKernelGGL((layernorm_rows_kernel<2, RAJNI_LN_ROWS, f16_t>), dim3((rows + 4 * RAJNI_LN_ROWS - 1) / (4 * RAJNI_LN_ROWS)), block, 0, s,
                       (const float*)x, xs, w, b, (f16_t*)y, rows, C, eps);
  else if (x_f32)
    hipLaunchKernelGGL((layernorm_kernel<float, f16_t>), grid, block, 0, s, (const float*)x, xs, w, b, (f16_t*)y, rows, C, eps);
  else
    hipLaunchKernelGGL((layernorm_kernel<f16_t, f16_t>), grid, block, 0, s, (const f16_t*)x, xs, w, b, (f16_t*)y, rows, C, eps);
  RAJNI_CHECK_LAUNCH("layernorm_kernel");
  return RAJNI_OK;
}

// kind RMS: launch_layernorm's choice of kernel, row mapping and profile class on the RMS instantiations; b does not exist
template <typename TX, typename TY>
static void launch_rmsnorm_t(const void* x, long xs, const float* w, void* y, int rows, int C, float eps, hipStream_t s) {
  const dim3 block(256);
  if constexpr (__is_same(TX, float) && !__is_same(TY, float)) {
    if (RAJNI_LN_ROWS > 1 && C <= 1024 && rows >= 4096) {
      hipLaunchKernelGGL((layernorm_rows_kernel<2, RAJNI_LN_ROWS, TY, true>), dim3((rows + 4 * RAJNI_LN_ROWS - 1) / (4 * RAJNI_LN_ROWS)),
                         block, 0, s, (const float*)x, xs, w, (const float*)nullptr, (TY*)y, rows, C, eps);
      return;
    }
  }
  hipLaunchKernelGGL((layernorm_kernel<TX, TY, true>), dim3((rows + 3) / 4), block, 0, s, (const TX*)x, xs, w, (const float*)nullptr,
                     (TY*)y, rows, C, eps);
}
static int launch_rmsnorm(const void* x, long xs, const float* w, void* y, int rows, int C, float eps, int x_f32, int dtype,
                          hipStream_t s) {
  RAJNI_REQUIRE(x && w && y, RAJNI_ERR_INVALID, "rajni_norm_rows: null pointer");
  RAJNI_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS && xs % 8 == 0,
                RAJNI_ERR_UNSUPPORTED, "rajni_norm_rows: need C %% 8 == 0, C <= 2048, stride %% 8 == 0 (C=%d)", C);
  const bool f32io = dtype == RAJNI_F32;
  ProfScope prof(KC_LAYERNORM, s, 4.0 * rows * C, (f32io ? 8.0 : (x_f32 ? 6.0 : 4.0)) * rows * C);
  if (f32io) launch_rmsnorm_t<float, float>(x, xs, w, y, rows, C, eps, s);
  else if (dtype == RAJNI_F16 && x_f32) launch_rmsnorm_t<float, f16_t>(x, xs, w, y, rows, C, eps, s);
  else if (dtype == RAJNI_F16) launch_rmsnorm_t<f16_t, f16_t>(x, xs, w, y, rows, C, eps, s);
  else if (x_f32) launch_rmsnorm_t<float, bf16_t>(x, xs, w, y, rows, C, eps, s);
  else launch_rmsnorm_t<bf16_t, bf16_t>(x, xs, w, y, rows, C, eps, s);
  RAJNI_CHECK_LAUNCH("layernorm_kernel<rms>");
  return RAJNI_OK;
}

int launch_layernorm_fp8(const void* x, long xs, const float* w, const float* b, void* yq, float* yscale,
                         float* hscale, float wnorm, float bmax, int rows, int C, float eps, int x_f32, hipStream_t s) {
  RAJNI_REQUIRE(x && w && b && yq && yscale, RAJNI_ERR_INVALID, "rajni_layernorm_fp8: null pointer");
  RAJNI_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS && xs % 8 == 0,
                RAJNI_ERR_UNSUPPORTED, "rajni_layernorm_fp8: need C %% 8 == 0, C <= 2048, stride %% 8 == 0 (C=%d)", C);
  RAJNI_REQUIRE(wnorm >= 0.f && bmax >= 0.f, RAJNI_ERR_INVALID, "rajni_layernorm_fp8: the hidden bound's constants must be >= 0");
  ProfScope prof(KC_LAYERNORM, s, 10.0 * rows * C, (x_f32 ? 5.0 : 3.0) * rows * C);
  const dim3 grid((rows + 3) / 4), block(256);
  const bool small = C <= 64 * 8 * 2;
  if (x_f32 && small && RAJNI_LN8_ROWS > 1 && rows >= 4096)
    hipLaunchKernelGGL((layernorm_fp8_rows_kernel<2, RAJNI_LN8_ROWS>), dim3((rows + 4 * RAJNI_LN8_ROWS - 1) / (4 * RAJNI_LN8_ROWS)), block, 0, s,
                       (const float*)x, xs, w, b, (unsigned char*)yq, yscale, hscale, wnorm, bmax, rows, C, eps);
  else if (x_f32 && small)
    hipLaunchKernelGGL((layernorm_fp8_kernel<float, 2>), grid, block, 0, s, (const float*)x, xs, w, b, (unsigned char*)yq,
                       yscale, hscale, wnorm, bmax, rows, C, eps);
  else if (x_f32)
    hipLaunchKernelGGL((layernorm_fp8_kernel<float, LN_MAX_CHUNKS>), grid, block, 0, s, (const float*)x, xs, w, b, (unsigned char*)yq,
                       yscale, hscale, wnorm, bmax, rows, C, eps);
  else if (small)
    hipLaunchKernelGGL((layernorm_fp8_kernel<bf16_t, 2>), grid, block, 0, s, (const bf16_t*)x, xs, w, b, (unsigned char*)yq,
                       yscale, hscale, wnorm, bmax, rows, C, eps);
  else
    hipLaunchKernelGGL((layernorm_fp8_kernel<bf16_t, LN_MAX_CHUNKS>), grid, block, 0, s, (const bf16_t*)x, xs, w, b, (unsigned char*)yq,
                       yscale, hscale, wnorm, bmax, rows, C, eps);
  RAJNI_CHECK_LAUNCH("layernorm_fp8_kernel");
  return RAJNI_OK;
}

int launch_gather_rows(const void* src, const int32_t* idx, void* dst, int B, int n_src, int n_dst,
                       int row_bytes, hipStream_t s) {
  RAJNI_REQUIRE(src && idx && dst, RAJNI_ERR_INVALID, "rajni_gather_rows: null pointer");
  RAJNI_REQUIRE(B > 0 && n_src > 0 && n_dst > 0 && row_bytes > 0 && row_bytes % 16 == 0,
                RAJNI_ERR_INVALID, "rajni_gather_rows: row bytes must be a multiple of 16 (%d)", row_bytes);
  const long rows = (long)B * n_dst;
  long blocks = (rows + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  ProfScope prof(KC_GATHER, s, 0.0, 2.0 * rows * row_bytes);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((int)blocks), dim3(256), 0, s, (const uint4*)src, idx,
                     (uint4*)dst, B, n_src, n_dst, row_bytes / 16);
  RAJNI_CHECK_LAUNCH("gather_rows_kernel");
  return RAJNI_OK;
}

// src [B, Nf] int32 = the composition of `n_levels` selections, levels[0] the LAST scheduled block's (see source_idx_kernel);
// n_levels == 0 gives the identity.  idx / width / nsrc are host arrays.
int launch_source_idx(int32_t* src, const int32_t* const* idx, const int* width, const int* nsrc, int n_levels, int B, int Nf,
                      hipStream_t s) {
  RAJNI_REQUIRE(src && B > 0 && Nf > 0 && n_levels >= 0, RAJNI_ERR_INVALID, "source_idx: bad arguments");
  const long total = (long)B * Nf;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  int done = 0;
  do {
    SrcLevels t{};
    for (; t.n < SRC_LEVELS && done < n_levels; ++t.n, ++done) {
      RAJNI_REQUIRE(idx[done] && width[done] > 0 && nsrc[done] > 0, RAJNI_ERR_INVALID, "source_idx: level %d is empty", done);
      t.idx[t.n] = idx[done]; t.width[t.n] = width[done]; t.nsrc[t.n] = nsrc[done];
    }
    ProfScope prof(KC_OTHER, s, 0.0, 4.0 * total * (t.n + 1));
    hipLaunchKernelGGL(source_idx_kernel, grid, block, 0, s, src, t, B, Nf, done == t.n ? 1 : 0);
    RAJNI_CHECK_LAUNCH("source_idx_kernel");
  } while (done < n_levels);
  return RAJNI_OK;
}

template <bool ZERO, bool RMS = false>
static void launch_dense_kernels(dim3 grid, dim3 block, const void* x, const int32_t* src, const float* w, const float* b, void* y,
                                 int B, int Nf, int S, int C, float eps, int x_f32, int dtype, hipStream_t s) {
  if (dtype == RAJNI_F32)
    hipLaunchKernelGGL((layernorm_dense_kernel<float, float, ZERO, RMS>), grid, block, 0, s, (const float*)x, src, w, b, (float*)y, B, Nf, S, C, eps);
  else if (dtype == RAJNI_F16 && x_f32)
    hipLaunchKernelGGL((layernorm_dense_kernel<float, f16_t, ZERO, RMS>), grid, block, 0, s, (const float*)x, src, w, b, (f16_t*)y, B, Nf, S, C, eps);
  else if (dtype == RAJNI_F16)
    hipLaunchKernelGGL((layernorm_dense_kernel<f16_t, f16_t, ZERO, RMS>), grid, block, 0, s, (const f16_t*)x, src, w, b, (f16_t*)y, B, Nf, S, C, eps);
  else if (x_f32)
    hipLaunchKernelGGL((layernorm_dense_kernel<float, bf16_t, ZERO, RMS>), grid, block, 0, s, (const float*)x, src, w, b, (bf16_t*)y, B, Nf, S, C, eps);
  else
    hipLaunchKernelGGL((layernorm_dense_kernel<bf16_t, bf16_t, ZERO, RMS>), grid, block, 0, s, (const bf16_t*)x, src, w, b, (bf16_t*)y, B, Nf, S, C, eps);
}

// y [B, S, C] `dtype`: row src[b, j] of image b = LayerNorm(x[b, j]) for the Nf rows of the stream x [B, Nf, C] (fp32 when x_f32,
// else `dtype`), every other row zero - or, with zero_fill == 0 (RAJNI_POOL_DENSE_LAST), left as it is.  src [B, Nf] strictly
// ascending per image, values in [0, S).
int launch_layernorm_dense(const void* x, const int32_t* src, const float* w, const float* b, void* y, int B, int Nf, int S,
                           int C, float eps, int x_f32, int dtype, hipStream_t s, int zero_fill, int kind) {
  const bool rms = kind == RAJNI_NORM_RMS;   // (b is not read)
  RAJNI_REQUIRE(x && src && w && (b || rms) && y, RAJNI_ERR_INVALID, "layernorm_dense: null pointer");
  RAJNI_REQUIRE(B > 0 && Nf > 0 && S >= Nf && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS, RAJNI_ERR_UNSUPPORTED,
                "layernorm_dense: need C %% 8 == 0, C <= 2048 and 0 < Nf <= S (C=%d Nf=%d S=%d)", C, Nf, S);
  const long rows = (long)B * S;
  RAJNI_REQUIRE((rows + 3) / 4 < (1L << 31), RAJNI_ERR_UNSUPPORTED, "layernorm_dense: too many output rows (%ld)", rows);
  const bool f32io = dtype == RAJNI_F32;
  const double eb = f32io ? 4.0 : 2.0, xb = (f32io || x_f32) ? 4.0 : 2.0;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * B * Nf * C, xb * B * Nf * C + eb * (zero_fill ? rows : (long)B * Nf) * C);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (rms && zero_fill) launch_dense_kernels<true, true>(grid, block, x, src, w, nullptr, y, B, Nf, S, C, eps, x_f32, dtype, s);
  else if (rms) launch_dense_kernels<false, true>(grid, block, x, src, w, nullptr, y, B, Nf, S, C, eps, x_f32, dtype, s);
  else if (zero_fill) launch_dense_kernels<true>(grid, block, x, src, w, b, y, B, Nf, S, C, eps, x_f32, dtype, s);
  else launch_dense_kernels<false>(grid, block, x, src, w, b, y, B, Nf, S, C, eps, x_f32, dtype, s);
  RAJNI_CHECK_LAUNCH("layernorm_dense_kernel");
  return RAJNI_OK;
}

// RAJNI_POOL_DENSE_LAST: y [B, S, C] `dtype` receives row src[b, j] = LayerNorm(x[b, j]) for every patch token j of the stream
// x [B, N, C] (fp32 when x_f32, else `dtype`) that the selection keep [B, Np] does NOT name; no other row is touched.  keep
// holds P prefix slots, then strictly ascending patch indices; src [B, N] holds values in [0, S).
int launch_layernorm_dropped(const void* x, const int32_t* keep, const int32_t* src, const float* w, const float* b, void* y,
                             int B, int N, int Np, int P, int S, int C, float eps, int x_f32, int dtype, hipStream_t s, int kind) {
  const bool rms = kind == RAJNI_NORM_RMS;   // (b is not read)
  RAJNI_REQUIRE(x && keep && src && w && (b || rms) && y, RAJNI_ERR_INVALID, "layernorm_dropped: null pointer");
  RAJNI_REQUIRE(B > 0 && P >= 0 && P < Np && Np <= N && N <= S && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS,
                RAJNI_ERR_UNSUPPORTED, "layernorm_dropped: need C %% 8 == 0, C <= 2048 and 0 <= P < Np <= N <= S (C=%d P=%d Np=%d N=%d S=%d)",
                C, P, Np, N, S);
  const long rows = (long)B * (N - P), dropped = (long)B * (N - Np);
  RAJNI_REQUIRE((rows + 3) / 4 < (1L << 31), RAJNI_ERR_UNSUPPORTED, "layernorm_dropped: too many rows (%ld)", rows);
  const bool f32io = dtype == RAJNI_F32;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * dropped * C, ((f32io || x_f32 ? 4.0 : 2.0) + (f32io ? 4.0 : 2.0)) * dropped * C);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define RAJNI_LN_DROPPED(TX, TY)                                                                                            \
  do {                                                                                                                      \
    if (rms)                                                                                                                \
      hipLaunchKernelGGL((layernorm_dropped_kernel<TX, TY, true>), grid, block, 0, s, (const TX*)x, keep, src, w,           \
                         (const float*)nullptr, (TY*)y, B, N, Np, P, S, C, eps);                                            \
    else                                                                                                                    \
      hipLaunchKernelGGL((layernorm_dropped_kernel<TX, TY>), grid, block, 0, s, (const TX*)x, keep, src, w, b, (TY*)y, B, N, \
                         Np, P, S, C, eps);                                                                                 \
  } while (0)
  if (f32io) RAJNI_LN_DROPPED(float, float);
  else if (dtype == RAJNI_F16 && x_f32) RAJNI_LN_DROPPED(float, f16_t);
  else if (dtype == RAJNI_F16) RAJNI_LN_DROPPED(f16_t, f16_t);
  else if (x_f32) RAJNI_LN_DROPPED(float, bf16_t);
  else RAJNI_LN_DROPPED(bf16_t, bf16_t);
#undef RAJNI_LN_DROPPED
  RAJNI_CHECK_LAUNCH("layernorm_dropped_kernel");
  return RAJNI_OK;
}

template <bool ZERO>
static void launch_dense_cast_kernels(dim3 grid, dim3 block, const void* x, const int32_t* src, void* y, int B, int Nf, int S, int C,
                                      int x_f32, int dtype, hipStream_t s) {
  if (dtype == RAJNI_F32)
    hipLaunchKernelGGL((rows_dense_cast_kernel<float, float, ZERO>), grid, block, 0, s, (const float*)x, src, (float*)y, B, Nf, S, C);
  else if (dtype == RAJNI_F16 && x_f32)
    hipLaunchKernelGGL((rows_dense_cast_kernel<float, f16_t, ZERO>), grid, block, 0, s, (const float*)x, src, (f16_t*)y, B, Nf, S, C);
  else if (dtype == RAJNI_F16)
    hipLaunchKernelGGL((rows_dense_cast_kernel<f16_t, f16_t, ZERO>), grid, block, 0, s, (const f16_t*)x, src, (f16_t*)y, B, Nf, S, C);
  else if (x_f32)
    hipLaunchKernelGGL((rows_dense_cast_kernel<float, bf16_t, ZERO>), grid, block, 0, s, (const float*)x, src, (bf16_t*)y, B, Nf, S, C);
  else
    hipLaunchKernelGGL((rows_dense_cast_kernel<bf16_t, bf16_t, ZERO>), grid, block, 0, s, (const bf16_t*)x, src, (bf16_t*)y, B, Nf, S, C);
}

// launch_layernorm_dense without the norm: row src[b, j] of y [B, S, C] `dtype` = x[b, j] rounded once to `dtype`, every other
// row zero, or with zero_fill == 0 left as it is
int launch_rows_dense_cast(const void* x, const int32_t* src, void* y, int B, int Nf, int S, int C, int x_f32, int dtype,
                           hipStream_t s, int zero_fill) {
  RAJNI_REQUIRE(x && src && y, RAJNI_ERR_INVALID, "rows_dense_cast: null pointer");
  RAJNI_REQUIRE(B > 0 && Nf > 0 && S >= Nf && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS, RAJNI_ERR_UNSUPPORTED,
                "rows_dense_cast: need C %% 8 == 0, C <= 2048 and 0 < Nf <= S (C=%d Nf=%d S=%d)", C, Nf, S);
  const long rows = (long)B * S;
  RAJNI_REQUIRE((rows + 3) / 4 < (1L << 31), RAJNI_ERR_UNSUPPORTED, "rows_dense_cast: too many output rows (%ld)", rows);
  const bool f32io = dtype == RAJNI_F32;
  const double eb = f32io ? 4.0 : 2.0, xb = (f32io || x_f32) ? 4.0 : 2.0;
  ProfScope prof(KC_LAYERNORM, s, 0.0, xb * B * Nf * C + eb * (zero_fill ? rows : (long)B * Nf) * C);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (zero_fill) launch_dense_cast_kernels<true>(grid, block, x, src, y, B, Nf, S, C, x_f32, dtype, s);
  else launch_dense_cast_kernels<false>(grid, block, x, src, y, B, Nf, S, C, x_f32, dtype, s);
  RAJNI_CHECK_LAUNCH("rows_dense_cast_kernel");
  return RAJNI_OK;
}

// launch_layernorm_dropped to `ny` outputs ys[k] [B, S, C] at once (1 <= ny <= RAJNI_MAX_LAYERS, a host array): the patch rows
// of x [B, N, C] that keep [B, Np] does not name, through the norm (norm != 0) or rounded once to `dtype`, to row src[b, j] of
// every output
int launch_rows_dropped_multi(const void* x, const int32_t* keep, const int32_t* src, const float* w, const float* b,
                              void* const* ys, int ny, int norm, int B, int N, int Np, int P, int S, int C, float eps, int x_f32,
                              int dtype, hipStream_t s) {
  RAJNI_REQUIRE(x && keep && src && ys && (!norm || (w && b)), RAJNI_ERR_INVALID, "rows_dropped_multi: null pointer");
  RAJNI_REQUIRE(ny >= 1 && ny <= RAJNI_MAX_LAYERS, RAJNI_ERR_INVALID, "rows_dropped_multi: 1..%d outputs (%d)", RAJNI_MAX_LAYERS, ny);
  RAJNI_REQUIRE(B > 0 && P >= 0 && P < Np && Np <= N && N <= S && C > 0 && C % 8 == 0 && C <= 64 * 8 * LN_MAX_CHUNKS,
                RAJNI_ERR_UNSUPPORTED, "rows_dropped_multi: need C %% 8 == 0, C <= 2048 and 0 <= P < Np <= N <= S (C=%d P=%d Np=%d N=%d S=%d)",
                C, P, Np, N, S);
  const long rows = (long)B * (N - P), dropped = (long)B * (N - Np);
  RAJNI_REQUIRE((rows + 3) / 4 < (1L << 31), RAJNI_ERR_UNSUPPORTED, "rows_dropped_multi: too many rows (%ld)", rows);
  RowTargets t{};
  for (t.n = 0; t.n < ny; ++t.n) {
    RAJNI_REQUIRE(ys[t.n] != nullptr, RAJNI_ERR_INVALID, "rows_dropped_multi: output %d is null", t.n);
    t.y[t.n] = ys[t.n];
  }
  const bool f32io = dtype == RAJNI_F32;
  ProfScope prof(KC_LAYERNORM, s, norm ? 8.0 * dropped * C : 0.0,
                 ((f32io || x_f32 ? 4.0 : 2.0) + (f32io ? 4.0 : 2.0) * ny) * dropped * C);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define RAJNI_ROWS_DROPPED(TX, TY)                                                                                              \
  do {                                                                                                                          \
    if (norm)                                                                                                                   \
      hipLaunchKernelGGL((rows_dropped_multi_kernel<TX, TY, true>), grid, block, 0, s, (const TX*)x, keep, src, w, b, t, B, N, Np, \
                         P, S, C, eps);                                                                                         \
    else                                                                                                                        \
      hipLaunchKernelGGL((rows_dropped_multi_kernel<TX, TY, false>), grid, block, 0, s, (const TX*)x, keep, src, w, b, t, B, N, Np, \
                         P, S, C, eps);                                                                                         \
  } while (0)
  if (f32io) RAJNI_ROWS_DROPPED(float, float);
  else if (dtype == RAJNI_F16 && x_f32) RAJNI_ROWS_DROPPED(float, f16_t);
  else if (dtype == RAJNI_F16) RAJNI_ROWS_DROPPED(f16_t, f16_t);
  else if (x_f32) RAJNI_ROWS_DROPPED(float, bf16_t);
  else RAJNI_ROWS_DROPPED(bf16_t, bf16_t);
#undef RAJNI_ROWS_DROPPED
  RAJNI_CHECK_LAUNCH("rows_dropped_multi_kernel");
  return RAJNI_OK;
}
