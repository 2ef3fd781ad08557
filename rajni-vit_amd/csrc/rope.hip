// Rotary position embeddings (include/rajni_hip_rope.h): q and k of qkv [B * N, 3, H, D] rotated in place by the tables' row for
// the place each token had in the image.  Table driven: the kernel knows nothing about frequency schemes and assumes no
// structure in cos / sin.
#include "common.h"

namespace {

// 4 consecutive elements of the activation dtype -> 4 floats (8 bytes of a 16-bit type, 16 of fp32)
template <typename T> __device__ __forceinline__ void load4(const T* p, float* f) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  f[0] = lo16<T>(v.x); f[1] = hi16<T>(v.x); f[2] = lo16<T>(v.y); f[3] = hi16<T>(v.y);
}
template <> __device__ __forceinline__ void load4<float>(const float* p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
}

// One wave per patch token (prefix rows get no wave: never read, never written).  The wave walks the token's 2H q and k heads -
// the first 2C elements of its 3C-element row; v is never touched - one head per LW-lane slot, 8 elements (16 bytes of a 16-bit
// type) per lane, lanes past D / 8 of a slot idle, as in qk_norm_kernel (variants.hip).  At D = 64 a head is one 128-byte line
// of bf16 and a wave instruction touches 8 whole consecutive lines.  A lane's place in the head, sl * 8, is the same for every
// head it visits, so with a shared table (head_stride 0) its cos and sin chunks are loaded once per token; per-head tables
// are loaded per head.  R heads per slot are in flight together.
// The partner of element j: HALF = false, j ^ 1, inside the lane's own chunk.  HALF = true, (j + D/2) % D: D/2 is a multiple of 4
// and D of 8, so the partners of a lane's elements [0, 4) and [4, 8) are two runs of 4 consecutive elements that do not wrap -
// two 4-element loads per lane from lines the wave's own 16-byte loads fetch (at D = 24 and 40 they straddle a chunk boundary,
// at D % 16 == 0 they are the halves of one chunk), no second pass over memory.  The sign is constant over each run.
// Every load of a batch is issued before its first store and a head belongs to one wave: in place is safe.
template <typename T, int LW, bool HALF>
__global__ void __launch_bounds__(256) rope_qk_kernel(T* qkv, const int32_t* __restrict__ src, const float* __restrict__ cost,
                                                      const float* __restrict__ sint, long head_stride, long tokens, int N, int P,
                                                      int H, int D) {
  constexpr int SLOTS = 64 / LW, R = 4;
  const int lane = threadIdx.x & 63, slot = lane / LW, sl = lane % LW;
  const long wv = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= tokens) return;
  const int patches = N - P;
  const long img = wv / patches;
  const int t = P + (int)(wv - img * patches);
  const long row = img * N + t;
  const int pos = (src ? src[row] : t) - P;
  const int j0 = sl * 8;
  const bool busy = j0 < D;
  const int H2 = 2 * H, half = D >> 1;
  T* const base = qkv + row * 3L * H * D + j0;
  const long toff = (long)pos * D + j0;
  // the two partner runs of the half layout, and their signs
  const int pa = (j0 + half) % D - j0, pb = (j0 + 4 + half) % D - j0;
  const float sa = j0 < half ? -1.f : 1.f, sb = j0 + 4 < half ? -1.f : 1.f;
  float c[8], sn[8];
  if (busy && head_stride == 0) {
    load8<float>(cost + toff, c);
    load8<float>(sint + toff, sn);
  }
  for (int h0 = 0; h0 < H2; h0 += SLOTS * R) {
    float x[R][8], y[R][8];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int h2 = h0 + r * SLOTS + slot;
      live[r] = busy && h2 < H2;
      if (live[r]) {
        const T* at = base + (long)h2 * D;
        load8<T>(at, x[r]);
        if constexpr (HALF) {
          load4<T>(at + pa, y[r]);
          load4<T>(at + pb, y[r] + 4);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
      const int h2 = h0 + r * SLOTS + slot;
      if (head_stride != 0) {
        const long o = (long)(h2 < H ? h2 : h2 - H) * head_stride + toff;
        load8<float>(cost + o, c);
        load8<float>(sint + o, sn);
      }
      float o8[8];
      if constexpr (HALF) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o8[j] = fmaf(x[r][j], c[j], sa * (y[r][j] * sn[j]));
#pragma unroll
        for (int j = 4; j < 8; ++j) o8[j] = fmaf(x[r][j], c[j], sb * (y[r][j] * sn[j]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          o8[j] = fmaf(x[r][j], c[j], -(x[r][j + 1] * sn[j]));
          o8[j + 1] = fmaf(x[r][j + 1], c[j + 1], x[r][j] * sn[j + 1]);
        }
      }
      store8<T>(base + (long)h2 * D, o8);
    }
  }
}

template <typename T, int LW>
void launch_rope_t(void* qkv, const int32_t* src, const float* cost, const float* sint, long head_stride, long tokens, int N, int P,
                   int H, int D, int layout, hipStream_t s) {
  const dim3 grid((unsigned)((tokens + 3) / 4)), block(256);
  if (layout == RAJNI_ROPE_HALF)
    hipLaunchKernelGGL((rope_qk_kernel<T, LW, true>), grid, block, 0, s, (T*)qkv, src, cost, sint, head_stride, tokens, N, P, H, D);
  else
    hipLaunchKernelGGL((rope_qk_kernel<T, LW, false>), grid, block, 0, s, (T*)qkv, src, cost, sint, head_stride, tokens, N, P, H, D);
}
template <typename T>
void launch_rope_lw(void* qkv, const int32_t* src, const float* cost, const float* sint, long head_stride, long tokens, int N, int P,
                    int H, int D, int layout, hipStream_t s) {
  if (D <= 32) launch_rope_t<T, 4>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
  else if (D <= 64) launch_rope_t<T, 8>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
  else launch_rope_t<T, 16>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
}

}  // namespace

int launch_rope_qk(void* qkv, const int32_t* src, const float* cost, const float* sint, long head_stride, int B, int N, int P,
                   int H, int D, int layout, int dtype, hipStream_t s) {
  // (shape limits before the pointers: a refused shape is refused whatever else the call holds)
  RAJNI_REQUIRE(B > 0 && H > 0 && P >= 0 && P <= RAJNI_MAX_PREFIX && N > P, RAJNI_ERR_INVALID,
                "rajni_rope_qk: bad shape (B=%d N=%d num_prefix=%d H=%d; num_prefix must be 0..%d and below N)", B, N, P, H,
                RAJNI_MAX_PREFIX);
  RAJNI_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_rope_qk: need a head dim that is a multiple of 8 up to 128 (D=%d)", D);
  RAJNI_REQUIRE(layout == RAJNI_ROPE_INTERLEAVED || layout == RAJNI_ROPE_HALF, RAJNI_ERR_INVALID,
                "rajni_rope_qk: layout must be RAJNI_ROPE_INTERLEAVED or RAJNI_ROPE_HALF (%d)", layout);
  RAJNI_REQUIRE(head_stride >= 0 && head_stride % 4 == 0, RAJNI_ERR_INVALID,
                "rajni_rope_qk: head_stride must be 0 (one table for all heads) or a positive multiple of 4 elements (%ld)", head_stride);
  const long tokens = (long)B * (N - P);
  // one workgroup of four waves per four tokens on grid axis x
  RAJNI_REQUIRE((tokens + 3) / 4 <= 0x7fffffffL, RAJNI_ERR_UNSUPPORTED, "rajni_rope_qk: %ld patch tokens - the limit is %ld", tokens,
                4L * 0x7fffffffL);
  RAJNI_REQUIRE(qkv && cost && sint, RAJNI_ERR_INVALID, "rajni_rope_qk: null pointer");
  const double es = dtype == RAJNI_F32 ? 4.0 : 2.0;
  // reads and writes the q and k thirds; the table rows once per token (per head with per-head tables)
  ProfScope prof(KC_OTHER, s, 6.0 * tokens * H * D, 4.0 * es * tokens * H * (double)D + 8.0 * tokens * D * (head_stride ? H : 1));
  if (dtype == RAJNI_F32) launch_rope_lw<float>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
  else if (dtype == RAJNI_F16) launch_rope_lw<f16_t>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
  else launch_rope_lw<bf16_t>(qkv, src, cost, sint, head_stride, tokens, N, P, H, D, layout, s);
  RAJNI_CHECK_LAUNCH("rope_qk_kernel");
  return RAJNI_OK;
}

extern "C" int rajni_rope_qk(void* qkv, const int32_t* src, const float* cos, const float* sin, long long head_stride, int B, int N,
                             int num_prefix, int H, int D, int layout, int dtype, rajni_stream_t stream) {
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID, "rajni_rope_qk: bad dtype %d", dtype);
  RAJNI_REQUIRE_PLACED("rajni_rope_qk", {"qkv", qkv, 16}, {"src", src, 4}, {"cos", cos, 16}, {"sin", sin, 16});
  return launch_rope_qk(qkv, src, cos, sin, (long)head_stride, B, N, num_prefix, H, D, layout, dtype, (hipStream_t)stream);
}
