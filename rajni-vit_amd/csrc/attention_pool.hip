// Latent-query attention pool (timm AttentionPoolLatent, include/rajni_hip_attnpool.h): the attention of ONE learned query
// row over every token that reaches the head,
//   out[b, h*D + d] = softmax_n(q[h] . k[b,n,h]) . v[b,n,h,d],  kv [B, N, 2C] = [K half | V half], q [H, D] fp32 (scale folded in).
// One workgroup of 4 waves per (image, head).  A token's K (and V) row of this head is D elements = G = D / 8 chunks of 8:
// G neighbouring lanes read it, 8 elements each - for 16-bit D = 64 one whole 128-byte line per row and read - so a wave
// holds TPW = 64 / G token slots (the lanes behind TPW * G idle) and the workgroup S = 4 * TPW.  Slot s walks tokens
// s, s + S, s + 2S ... in order with an online softmax (running maximum m, sum l and 8 accumulators per lane), then the S
// slot states meet in LDS and are merged in slot order: the summation order depends on (N, D) alone, nothing depends on the
// batch, no atomics, and LDS is S * (D + 2) floats whatever N is (at most 10 KiB, at D = 8).
// fp32 math on the stored activations; the output is rounded once to the model dtype (O = T), or stays fp32 (O = float: the
// whole forward's tail, which keeps its B-row part in fp32).
#include "common.h"

namespace {

constexpr int AP_WAVES = 4;
constexpr int AP_MAX_LDS_FLOATS = AP_WAVES * 64 * (8 + 2);   // S * (D + 2) = 4 * (64 / G) * (8 G + 2) is largest at G = 1

template <typename T, typename O>
__global__ void __launch_bounds__(AP_WAVES * 64) attn_pool_kernel(const T* kv, const float* q, O* out, int N, int H, int D) {
  __shared__ __attribute__((aligned(16))) float ap_sm[AP_MAX_LDS_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, head = blockIdx.x, b = blockIdx.y;
  const int G = D >> 3, TPW = 64 / G, S = AP_WAVES * TPW;
  const int t = lane / G, g = lane - t * G;             // token slot of this lane inside the wave, and its chunk of the row
  const bool live = t < TPW;                            // (lanes behind TPW * G hold no slot; they still take part in the shuffles)
  const int C = H * D;
  const long C2 = 2L * C;
  const int chunk = live ? g * 8 : 0;
  float qf[8];
  {
    const float* qp = q + head * D + chunk;
    const float4 a = reinterpret_cast<const float4*>(qp)[0], c = reinterpret_cast<const float4*>(qp)[1];
    qf[0] = a.x; qf[1] = a.y; qf[2] = a.z; qf[3] = a.w; qf[4] = c.x; qf[5] = c.y; qf[6] = c.z; qf[7] = c.w;
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] *= 1.4426950408889634f;   // log2 domain
  }
  const T* img = kv + (long)b * N * C2 + head * D + chunk;
  float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int gbase = lane - g;                           // first lane of this lane's group
  for (int n0 = wave * TPW; n0 < N; n0 += S) {          // (wave-uniform trip count)
    const int n = n0 + t;
    const bool on = live && n < N;
    float kf[8], vf[8];
    if (on) {
      const T* row = img + (long)n * C2;
      load8<T>(row, kf);
      load8<T>(row + C, vf);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { kf[j] = 0.f; vf[j] = 0.f; }
    }
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) part = fmaf(qf[j], kf[j], part);
    float s = 0.f;   // the row's logit: the G partial sums in chunk order, the same bits in every lane of the group
    for (int j = 0; j < G; ++j) s += __shfl(part, (gbase + j) & 63, 64);
    if (on) {
      const float mn = fmaxf(m, s);
      // (m = -inf in front of the slot's first token: alpha = 0)
      const float alpha = __builtin_amdgcn_exp2f(m - mn), p = __builtin_amdgcn_exp2f(s - mn);
      l = fmaf(l, alpha, p);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(acc[j], alpha, p * vf[j]);
      m = mn;
    }
  }
  // slot state -> LDS: [S][D + 2] = {acc[D], m, l}
  const int W = D + 2;
  if (live) {
    float* st = ap_sm + (wave * TPW + t) * W;
#pragma unroll
    for (int j = 0; j < 8; ++j) st[chunk + j] = acc[j];
    if (g == 0) { st[D] = m; st[D + 1] = l; }
  }
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) {   // merge in slot order (an empty slot has m = -inf, l = 0: weight 0; N >= 1, so slot 0 never is)
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, ap_sm[s * W + D]);
    float L = 0.f, o = 0.f;
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(ap_sm[s * W + D] - M);
      L = fmaf(ap_sm[s * W + D + 1], wgt, L);
      o = fmaf(ap_sm[s * W + d], wgt, o);
    }
    st1(out + (long)b * C + head * D + d, o / L);
  }
}

}  // namespace

template <typename T>
void launch_pool_t(const void* kv, const float* q, void* out, int B, int N, int H, int D, int out_f32, hipStream_t s) {
  const dim3 grid(H, B), block(AP_WAVES * 64);
  if (out_f32) hipLaunchKernelGGL((attn_pool_kernel<T, float>), grid, block, 0, s, (const T*)kv, q, (float*)out, N, H, D);
  else hipLaunchKernelGGL((attn_pool_kernel<T, T>), grid, block, 0, s, (const T*)kv, q, (T*)out, N, H, D);
}

int launch_attention_pool(const void* kv, const float* q, void* out, int B, int N, int H, int D, int dtype, hipStream_t s, int out_f32) {
  RAJNI_REQUIRE(kv && q && out, RAJNI_ERR_INVALID, "rajni_attention_pool: null pointer");
  RAJNI_REQUIRE(B > 0 && N > 0 && H > 0, RAJNI_ERR_INVALID, "rajni_attention_pool: need B > 0, N >= 1 and H > 0 (B=%d N=%d H=%d)", B, N, H);
  RAJNI_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_attention_pool: the head dim must be a multiple of 8 in 8..128 (D=%d)", D);
  RAJNI_REQUIRE(B <= RAJNI_MAX_GRID_YZ, RAJNI_ERR_UNSUPPORTED,
                "rajni_attention_pool: B=%d - one launch takes at most %d images (the image index is a grid axis)", B, RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE((long long)H * D < (1LL << 30), RAJNI_ERR_UNSUPPORTED, "rajni_attention_pool: H * D is too large (%d x %d)", H, D);
  const double es = dtype == RAJNI_F32 ? 4.0 : 2.0;
  ProfScope prof(KC_ATTENTION, s, 4.0 * B * H * (double)N * D, (2.0 * B * (double)N + B) * H * D * es);
  if (dtype == RAJNI_F32) launch_pool_t<float>(kv, q, out, B, N, H, D, 1, s);
  else if (dtype == RAJNI_F16) launch_pool_t<f16_t>(kv, q, out, B, N, H, D, out_f32, s);
  else launch_pool_t<bf16_t>(kv, q, out, B, N, H, D, out_f32, s);
  RAJNI_CHECK_LAUNCH("attn_pool_kernel");
  return RAJNI_OK;
}
