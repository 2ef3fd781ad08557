// The norm inside the MLP (include/rajni_hip_mlpnorm.h): LayerNorm / RMSNorm over the first n columns of every row of the hidden
// buffer x [rows, ld], in place, between FC1's epilogue and FC2 (EVA02's sub-LayerNorm).  n is the model's MLP width - any
// positive number, 2730 for EVA02-L - and ld the buffer's, zero-padded to whole K steps.
#include "common.h"

namespace {

// One wave per row, four rows per workgroup, 8-element chunks (16 bytes of a 16-bit type) per lane: chunk lane + 64 i of the row
// sits in v[i], so the row is read once and the two-pass statistics of layernorm_kernel (rowops.hip) run on registers - mean
// first, then the squared deviations from it.  The sums run in that kernel's order: a lane's chunks in order, their elements in
// order, then the 6-step wave butterfly, whatever NC is - a row gives the same bits at any row count and row position.
// NC chunks per lane hold n <= 512 NC; the launcher takes the smallest of 1, 2, 4, 6, 8 that does.
// The last chunk of a row with n % 8 != 0 is partial: it is read whole (ld % 8 == 0 keeps it inside the row), its elements past n
// stay out of both sums and are stored as +0.  Whole chunks past n are neither read nor written: the zeros FC1 left stay.
template <typename T, int NC, bool RMS>
__global__ void __launch_bounds__(256) hidden_norm_kernel(T* __restrict__ x, long ld, const float* __restrict__ w,
                                                          const float* __restrict__ b, long rows, int n, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  T* const xr = x + row * ld;
  float v[NC][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int e0 = (lane + i * 64) * 8;
    if (e0 < n) {
      load8<T>(xr + e0, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (e0 + j >= n) v[i][j] = 0.f;
        if constexpr (RMS) sum += v[i][j] * v[i][j];
        else sum += v[i][j];
      }
    }
  }
  float mean = 0.f, rstd;
  if constexpr (RMS) {
    rstd = rsqrtf(wave_sum(sum) / (float)n + eps);
  } else {
    mean = wave_sum(sum) / (float)n;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int e0 = (lane + i * 64) * 8;
      if (e0 < n) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = e0 + j < n ? v[i][j] - mean : 0.f;
          ss += d * d;
        }
      }
    }
    rstd = rsqrtf(wave_sum(ss) / (float)n + eps);
  }
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int e0 = (lane + i * 64) * 8;
    if (e0 < n) {
      float wv[8], bv[8], o[8];
      if (e0 + 8 <= n) {
        load8<float>(w + e0, wv);
        if (!RMS && b) load8<float>(b + e0, bv);
      } else {      // the partial chunk: w and b end at n
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          wv[j] = e0 + j < n ? w[e0 + j] : 0.f;
          bv[j] = (!RMS && b && e0 + j < n) ? b[e0 + j] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float r;
        if constexpr (RMS) r = (v[i][j] * rstd) * wv[j];
        else r = fmaf((v[i][j] - mean) * rstd, wv[j], b ? bv[j] : 0.f);
        o[j] = e0 + j < n ? r : 0.f;
      }
      store8<T>(xr + e0, o);
    }
  }
}

template <typename T, int NC>
void launch_nc(int kind, void* x, long ld, const float* w, const float* b, long rows, int n, float eps, hipStream_t s) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (kind == RAJNI_NORM_RMS)
    hipLaunchKernelGGL((hidden_norm_kernel<T, NC, true>), grid, block, 0, s, (T*)x, ld, w, b, rows, n, eps);
  else
    hipLaunchKernelGGL((hidden_norm_kernel<T, NC, false>), grid, block, 0, s, (T*)x, ld, w, b, rows, n, eps);
}
template <typename T>
void launch_t(int kind, void* x, long ld, const float* w, const float* b, long rows, int n, float eps, hipStream_t s) {
  if (n <= 512) launch_nc<T, 1>(kind, x, ld, w, b, rows, n, eps, s);
  else if (n <= 1024) launch_nc<T, 2>(kind, x, ld, w, b, rows, n, eps, s);
  else if (n <= 2048) launch_nc<T, 4>(kind, x, ld, w, b, rows, n, eps, s);
  else if (n <= 3072) launch_nc<T, 6>(kind, x, ld, w, b, rows, n, eps, s);
  else launch_nc<T, 8>(kind, x, ld, w, b, rows, n, eps, s);
}

}  // namespace

int launch_hidden_norm(int kind, void* x, long ld, const float* w, const float* b, long rows, int n, float eps, int dtype, int x_f32,
                       hipStream_t s) {
  RAJNI_REQUIRE(kind == RAJNI_NORM_LAYERNORM || kind == RAJNI_NORM_RMS, RAJNI_ERR_INVALID,
                "rajni_hidden_norm: kind must be RAJNI_NORM_LAYERNORM or RAJNI_NORM_RMS (%d)", kind);
  RAJNI_REQUIRE(n > 0 && rows > 0, RAJNI_ERR_INVALID, "rajni_hidden_norm: bad shape (rows=%ld n=%d)", rows, n);
  RAJNI_REQUIRE(n <= RAJNI_HIDDEN_NORM_MAX, RAJNI_ERR_UNSUPPORTED,
                "rajni_hidden_norm: a width of %d is over the cap of %d columns (one wave holds the row in registers)", n,
                RAJNI_HIDDEN_NORM_MAX);
  RAJNI_REQUIRE(ld >= n && ld % 8 == 0, RAJNI_ERR_INVALID,
                "rajni_hidden_norm: ld must be at least n and a multiple of 8 (ld=%ld n=%d)", ld, n);
  // one workgroup of four waves per four rows on grid axis x
  RAJNI_REQUIRE((rows + 3) / 4 <= 0x7fffffffL, RAJNI_ERR_UNSUPPORTED, "rajni_hidden_norm: %ld rows - the limit is %ld", rows,
                4L * 0x7fffffffL);
  RAJNI_REQUIRE(x && w, RAJNI_ERR_INVALID, "rajni_hidden_norm: null pointer (%s)", x ? "w" : "x");
  const bool f32 = x_f32 || dtype == RAJNI_F32;
  ProfScope prof(KC_LAYERNORM, s, 8.0 * rows * n, 2.0 * (f32 ? 4.0 : 2.0) * rows * (double)n);
  if (f32) launch_t<float>(kind, x, ld, w, b, rows, n, eps, s);
  else if (dtype == RAJNI_F16) launch_t<f16_t>(kind, x, ld, w, b, rows, n, eps, s);
  else launch_t<bf16_t>(kind, x, ld, w, b, rows, n, eps, s);
  RAJNI_CHECK_LAUNCH("hidden_norm_kernel");
  return RAJNI_OK;
}

extern "C" int rajni_hidden_norm(int kind, void* x, long ld, const float* w, const float* b, int rows, int n, float eps, int dtype,
                                 int x_f32, rajni_stream_t stream) {
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID, "rajni_hidden_norm: bad dtype %d",
                dtype);
  RAJNI_REQUIRE_PLACED("rajni_hidden_norm", {"x", x, 16}, {"w", w, 16}, {"b", b, 16});
  return launch_hidden_norm(kind, x, ld, w, b, rows, n, eps, dtype, x_f32, (hipStream_t)stream);
}
