// RAJNI importance score + per-image top-k selection + order-preserving compaction
// (SURVEY k3-k9,k14; reference importance.py:4-34, attention.py:31-39,58) in ONE launch per stage.
//
// One 1024-thread workgroup per image (16 waves: the two read passes are bound by loads in flight per CU).  HBM traffic = the K and V thirds of qkv, read once with
// 16-byte loads; logits, head-mean V, norms and scores live in LDS; selection is a rank count
// (N <= 577 scores, broadcast LDS reads) followed by wave ballot + popcount prefix compaction, which
// yields the ascending index list directly (the reference's topk -> sort).
//
// Numerics: fp32 throughout; the final score is rounded to the I/O dtype (what the reference
// returns, importance.py:34) and ranking is done on the rounded values - like the reference ranks
// its own dtype-rounded scores - with the DEFINED tie rule: larger first, then lower index; NaN = +inf.
// All reductions use fixed trees, so the same input always selects the same tokens.
#include "common.h"

namespace {

#ifndef RAJNI_SS_THREADS
#define RAJNI_SS_THREADS 1024
#endif
constexpr int SS_THREADS = RAJNI_SS_THREADS;
// threads (and LDS floats) of the token-mean partial sums: 512 like the 8-wave version of the kernel, so that the
// 16-wave one needs no more LDS (N = 589 with 16 heads still fits 160 KiB) and sums in the same fixed order
constexpr int SS_PART = 512;
#ifndef RAJNI_SS_KU
#define RAJNI_SS_KU 8   // K-pass chunks in flight per lane
#endif
#ifndef RAJNI_SS_KUM
#define RAJNI_SS_KUM 4  // ... in the one-pass form, next to RAJNI_SS_VUM V head rows of the lane's V item
#endif
#ifndef RAJNI_SS_VUM
#define RAJNI_SS_VUM 6
#endif

// the class row's relative position bias (rajni_hip_relpos.h): [H] fp32 each - pq on the patch keys, pqk on the P prefix keys
// (rows 0 .. P - 1)
struct ScoreBias { const float* pq; const float* pqk; int P; };
struct ScoreArgs {          // T = activation dtype (bf16_t, f16_t or float)
  const void* qkv;          // T [B,N,3C] or null (select-only)
  const void* scores_in;    // T [B,N] (select-only)
  int N, H, D;
  float eps;
  int keep;                 // 0: scores only
  int P;                    // prefix tokens (CLS + registers; registers alone, possibly none, without a class row): rows 0..P-1 are always kept and never ranked
  void* scores_out;         // T [B,N] or null
  int* keep_idx;            // [B,P+keep]
  void* next_scores;        // T [B,P+keep] or null
  unsigned long long* stamps;   // diagnostic builds (-DRAJNI_SS_STAMPS): 16 x u64 s_memtime per workgroup, or null
};
// the argument of the instantiations with the bias: ScoreArgs itself keeps its size, so no kernel that takes it changes
struct ScoreArgsRB : ScoreArgs { ScoreBias rb; };
__device__ __forceinline__ const ScoreBias* rb_of(const ScoreArgs&) { return nullptr; }
__device__ __forceinline__ const ScoreBias* rb_of(const ScoreArgsRB& a) { return &a.rb; }
// the class row's logit of head h against key row n, with its bias (fp32 add, before the softmax)
template <bool RB>
__device__ __forceinline__ float ss_logit(const ScoreBias* rb, float scaled_dot, int h, int n) {
  if constexpr (RB) return scaled_dot + (n < rb->P ? rb->pqk[h] : rb->pq[h]);
  else return scaled_dot;
}
#ifdef RAJNI_SS_STAMPS
#define SS_STAMP(i) do { if (a.stamps != nullptr && threadIdx.x == 0) a.stamps[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SS_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ float rank_key(float s) { return (s != s) ? INFINITY : s; }

// lanes that share one token's rank count, by the number of ranked (patch) tokens
__host__ __device__ inline int ss_tpt(int npatch) {
  return npatch * 8 <= SS_THREADS ? 8 : npatch * 4 <= SS_THREADS ? 4 : npatch * 2 <= SS_THREADS ? 2 : 1;
}
// words of the packed-key image of N tokens (P of them prefix): tpt slices of `cstride` 16-byte chunks.  It lives in the
// logits' region, which is smaller than this for a handful of tokens (N = 2, H = 1, D = 8: 20 words against 32), so the
// kernel and ss_lds_bytes both size the region to hold it.
__host__ __device__ inline int ss_key_words(int N, int P) {
  const int tpt = ss_tpt(N - P);
  const int chunks = (N + 3) >> 2, cps = (chunks + tpt - 1) / tpt;
  return (cps | 1) * tpt * 4;
}
// The mean query (RAJNI_QUERY_MEAN, rajni_hip_query.h): row partitions of the column sums of the Q third.  Partition q sums
// rows q, q + QP, ... in row order and the QP partial sums join in partition order: a fixed order that hangs on C alone.
__host__ __device__ inline int ss_qparts(int C) {
  const int cp = C >> 3, a = cp > 0 && cp <= SS_THREADS ? SS_THREADS / cp : 1;
  return a < 16 ? a : 16;
}
// (qmean: the partial sums [QP][C] of the mean query live in the region before the logits do)
__host__ __device__ inline int ss_region_words(int N, int H, int D, int P, bool merged, bool qmean = false) {
  const int lg = (H * N + 3) & ~3;
  int r = merged ? lg + N * D : (((H * N > N * D) ? H * N : N * D) + 3) & ~3;
  const int kw = ss_key_words(N, P);
  r = r > kw ? r : kw;
  const int qw = qmean ? ss_qparts(H * D) * H * D : 0;
  return r > qw ? r : qw;
}

// sum over an aligned group of `width` (4, 8 or 16) consecutive lanes, every lane gets the total; DPP adds in
// a fixed tree (bitwise reproducible): xor 1, xor 2, mirror within 8, mirror within 16
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float group_sum(float v, int width) {
  v = dpp_add<0xB1>(v);                    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);                    // quad_perm [2,3,0,1]
  if (width >= 8) v = dpp_add<0x141>(v);   // row_half_mirror
  if (width >= 16) v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

// The selection tail both kernels share: rank the patch tokens of image b by the scores in `sc` [N] (already rounded to T)
// and compact the kept ones.  `keys` (fp32 scores: N floats, read 16 bytes at a time, so up to 3 floats past N must be
// readable) and `keys32` (16-bit scores: ss_key_words(N, P) words, 16-byte aligned) are LDS the caller no longer needs;
// `wcount` holds SS_THREADS / 64 ints.  Called by all SS_THREADS threads of the workgroup, after a barrier behind `sc`.
template <typename T>
__device__ __forceinline__ void select_tail(const ScoreArgs& a, int b, float* sc, float* keys, unsigned* keys32, int* wcount) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int N = a.N;

  // ---- rank patch tokens P..N-1, keep rank < keep, compact in ascending index order behind the P prefix slots
  //      (attention.py:34-39: topk -> sort -> +1 -> prepend CLS; attention.py:58: carried scores)
  const int keep = a.keep, P = a.P;
  int* kout = a.keep_idx + (long)b * (keep + P);
  T* nout = a.next_scores ? reinterpret_cast<T*>(a.next_scores) + (long)b * (keep + P) : nullptr;
  int running = 0;
  // tpt = 1, 2, 4 or 8 lanes share a token's rank count (each a slice of the j range, summed by shuffles): with
  // 197 tokens one lane per token left 60 % of the workgroup idle through a 196-step loop
  const int tpt = ss_tpt(N - P);
  const int per_iter = SS_THREADS / tpt, sl = tid & (tpt - 1);
  // The count loop is VALU bound (N^2 compares over 4 SIMDs: stamps put it at 14k of the kernel's 88k cycles at 197
  // tokens, 95k of 297k at 577, when a compare was ~8 instructions: two range tests, >, ==, index test, or / and / add).
  // 16-bit scores (bf16 and fp16): ONE unsigned compare per pair on a packed key
  //     key32[j] = sortable16(score_j) << 16 | (0xFFFF - j)        (NaN = +inf, -0 = +0; N <= 65535)
  // (sortable16 of the score's own 16-bit pattern: for bf16 that is the upper half of the fp32 pattern, for fp16 not)
  // "j beats i" (larger score, or equal score and lower index - the defined tie rule) <=> key32[j] > key32[i], and the
  // prefix slots and the padding hold 0 (below every real key), so slices need no range tests: v_cmp + add-with-carry.
  // fp32 scores keep the float compare (the accuracy path).
  constexpr bool PACKED = sizeof(T) == 2;
  const int chunks = (N + 3) >> 2, cps = (chunks + tpt - 1) / tpt;   // 16-byte chunks of keys; per slice
  const int cstride = cps | 1;     // slices an ODD number of chunks apart: the tpt broadcast reads of a step hit distinct banks
  if constexpr (PACKED) {
    for (int w = tid; w < cstride * tpt * 4; w += SS_THREADS) {
      const int slw = w / (cstride * 4), off = w - slw * cstride * 4;
      const int n = off < cps * 4 ? slw * cps * 4 + off : N;     // token of word w (padding words: none)
      unsigned k = 0;
      if (n >= P && n < N) {
        if constexpr (__is_same(T, f16_t)) {
          // fp16 scores: the upper half of the fp32 pattern would merge fp16 values that differ below bf16 precision,
          // so the key is built from the fp16 pattern itself (exact: sc holds fp16 values; NaN -> +inf first)
          unsigned u = __builtin_bit_cast(unsigned short, f2h(rank_key(sc[n])));
          u = (u == 0x8000u) ? 0u : u;                              // -0 ranks as +0
          u = (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);       // monotone half -> unsigned
          k = (u << 16) | (unsigned)(0xFFFF - n);
        } else {   // bf16 scores: the upper half of the fp32 pattern is the bf16 pattern
          unsigned u = __float_as_uint(rank_key(sc[n]));
          u = (u == 0x80000000u) ? 0u : u;                            // -0 ranks as +0
          u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);             // monotone float -> unsigned
          k = (u & 0xFFFF0000u) | (unsigned)(0xFFFF - n);
        }
      }
      keys32[w] = k;
    }
  } else {
    for (int n = tid; n < N; n += SS_THREADS) keys[n] = rank_key(sc[n]);
  }
  __syncthreads();
  SS_STAMP(7);
  const int slice = (N - P + tpt - 1) / tpt;
  for (int base_i = P; base_i < N; base_i += per_iter) {
    const int i = base_i + tid / tpt;
    const bool valid = i < N;
    float si = 0.f;
    int rank = 0;
    if (valid) {
      si = sc[i];
      if constexpr (PACKED) {
        const int si_ = i / (cps * 4);                                  // slice and word that hold token i's key
        const unsigned ki = keys32[si_ * cstride * 4 + (i - si_ * cps * 4)];
        const uint4* kp = reinterpret_cast<const uint4*>(keys32) + sl * cstride;
#pragma unroll 4
        for (int c = 0; c < cps; ++c) {
          const uint4 k4 = kp[c];
          rank += (k4.x > ki) + (k4.y > ki) + (k4.z > ki) + (k4.w > ki);
        }
      } else {
        const float ki = keys[i];
        const int j0 = P + sl * slice, j1 = j0 + slice < N ? j0 + slice : N;
        // j beats i when its key is larger, or equal with a lower index (the defined tie rule)
        auto beats = [&](float kj, int j) { return (j >= j0 && j < j1 && (kj > ki || (kj == ki && j < i))) ? 1 : 0; };
#pragma unroll 4
        for (int j = j0 & ~3; j < j1; j += 4) {    // aligned 16-byte reads; entries outside [j0, j1) are masked
          const float4 k4 = *reinterpret_cast<const float4*>(keys + j);   // may run 3 floats into `sc`: masked
          rank += beats(k4.x, j) + beats(k4.y, j + 1) + beats(k4.z, j + 2) + beats(k4.w, j + 3);
        }
      }
    }
    SS_STAMP(8);
    if (tpt >= 2) rank += __shfl_xor(rank, 1, 64);
    if (tpt >= 4) rank += __shfl_xor(rank, 2, 64);
    if (tpt >= 8) rank += __shfl_xor(rank, 4, 64);
    const bool kept = valid && sl == 0 && rank < keep;
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    SS_STAMP(9);
    int prefix = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SS_THREADS / 64; ++w) {
      const int cnt = wcount[w];
      prefix += (w < wave) ? cnt : 0;
      total += cnt;
    }
    if (kept) {
      const int pos = running + prefix + __popcll(bal & ((1ull << lane) - 1ull));
      kout[P + pos] = i;
      if (nout) st1(nout + P + pos, si);
    }
    running += total;
    __syncthreads();
    SS_STAMP(10);
  }
  if (tid < P) {   // the prefix slots: CLS and the register tokens, in place
    kout[tid] = tid;
    if (nout) st1(nout + tid, sc[tid]);
  }
  SS_STAMP(6);
}

// MERGED: logits and vbar have LDS regions of their own and K and V rows are read in ONE pass (a token's K and V
// thirds are 3072 contiguous bytes of its 4608-byte qkv row, and no V load has to wait for the softmax statistics);
// otherwise (N = 577 with 16 heads: 185 KiB would be needed) vbar reuses the logits' region after the statistics.
// QMEAN: the importance query is the mean of the N query rows (RAJNI_QUERY_MEAN) instead of row 0; everything behind the
// fill of `qcls` is the same code.
// Args = ScoreArgsRB: the class row's logits get their relative position bias (never with QMEAN: the mean query has no
// position).  A template parameter, so that the instantiations without a bias are the code they were (tools/isa_identity.py).
template <bool COMPUTE, typename T, bool MERGED, bool QMEAN = false, typename Args = ScoreArgs>
__global__ void __launch_bounds__(SS_THREADS) score_select_kernel(const Args a) {
  constexpr bool RB = !__is_same(Args, ScoreArgs);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int N = a.N, H = a.H, D = a.D, C = H * D;
  const int lg_sz = (H * N + 3) & ~3;
  const int region_sz = ss_region_words(N, H, D, a.P, MERGED, QMEAN);
  float* qcls = sm;                    // [C]: the query, row 0 or the mean row
  float* region = qcls + C;            // logits [H][N]  (then / followed by)  vbar [N][D]
  float* vbar = MERGED ? region + lg_sz : region;
  float* acls = region + region_sz;    // [N]
  float* sc = acls + N;                // vnorm [N] then scores [N]
  float* hstat = sc + N;               // [2H]
  float* part = hstat + 2 * H;         // [SS_PART]
  float* mean = part + SS_PART;        // [D]
  float* misc = mean + D;              // [16]
  int* wcount = reinterpret_cast<int*>(misc + 16);  // [SS_THREADS / 64]

  SS_STAMP(0);
  if (COMPUTE) {
    const T* base = reinterpret_cast<const T*>(a.qkv) + (long)b * N * 3 * C;
    const int LP = D >> 3;             // lanes per 2*D-byte head row
    // head dims 32 / 64 / 128: LP is 4 / 8 / 16 and the lanes of a head row are summed by DPP adds; any other
    // D % 8 == 0 (80, 96, 72 ...) takes the plain forms below (one lane per (token, head) dot product, serial norms)
    const bool pow2 = LP == 4 || LP == 8 || LP == 16;
    const int sub = tid % LP;
    const int grp = tid / LP, ngrp = SS_THREADS / LP;   // threads past ngrp * LP sit the head-row passes out

    if constexpr (QMEAN) {
      // ---- mean query row -> LDS: qcls[c] = (1 / N) sum_n q[n, c], fp32.  Item (partition q, 16-byte chunk c) sums rows
      //      q, q + QP, ... in row order (four loads in flight, added in order) into region[q][c]; then column c joins its QP
      //      partial sums in partition order.  No atomics: the same bits on every run and in both LDS layouts.
      const int CPQ = C >> 3, QP = ss_qparts(C);
      for (int item = tid; item < QP * CPQ; item += SS_THREADS) {
        const int q = item / CPQ, c = item - q * CPQ;
        const T* qp = base + c * 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = q; n < N; n += 4 * QP) {
          float f[4][8];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (n + u * QP < N) load8<T>(qp + (long)(n + u * QP) * 3 * C, f[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (n + u * QP < N) {
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[j] += f[u][j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) region[q * C + c * 8 + j] = acc[j];
      }
      __syncthreads();
      const float inv_n = 1.0f / (float)N;
      for (int c = tid; c < C; c += SS_THREADS) {
        float t = 0.f;
        for (int q = 0; q < QP; ++q) t += region[q * C + c];
        qcls[c] = t * inv_n;
      }
      __syncthreads();   // the partial sums are dead: the region takes the logits
    } else {
      // ---- CLS query row -> LDS (importance.py:18)
      for (int c = tid; c < (C >> 3); c += SS_THREADS) {
        float f[8];
        load8<T>(base + c * 8, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) qcls[c * 8 + j] = f[j];
      }
      __syncthreads();
    }

    // ---- logits[h][n] = q_cls[h] . k[n,h] / sqrt(D)   (importance.py:19)
    // Work item = one 16-byte chunk c of K row n (C/8 chunks per row, lane-contiguous -> coalesced); the LP
    // chunks of a head sit in LP consecutive lanes and are summed with DPP adds (ds_bpermute shuffles and an
    // integer division per item made this loop 34 of the kernel's 60 us).  U loads in flight per thread.
    const float inv_sqrt_d = 1.0f / sqrtf((float)D);
    const float inv_h = 1.0f / (float)H;
    constexpr int U = RAJNI_SS_KU;
    const int CP = C >> 3;
    const int dn = SS_THREADS / CP, dc = SS_THREADS - dn * CP;   // K item index += SS_THREADS
    // one K chunk: dot with the CLS query chunk, summed over the head's LP lanes, lane 0 of the group stores
    auto k_item = [&](const float (&kf)[8], int n, int c) {
      const float4 q0 = *reinterpret_cast<const float4*>(qcls + c * 8);
      const float4 q1 = *reinterpret_cast<const float4*>(qcls + c * 8 + 4);
      float dot = kf[0] * q0.x;
      dot = fmaf(kf[1], q0.y, dot); dot = fmaf(kf[2], q0.z, dot); dot = fmaf(kf[3], q0.w, dot);
      dot = fmaf(kf[4], q1.x, dot); dot = fmaf(kf[5], q1.y, dot); dot = fmaf(kf[6], q1.z, dot);
      dot = fmaf(kf[7], q1.w, dot);
      dot = group_sum(dot, LP);
      if ((c & (LP - 1)) == 0) region[(c / LP) * N + n] = ss_logit<RB>(rb_of(a), dot * inv_sqrt_d, c / LP, n);
    };
    auto k_pass = [&]() {
      if (!pow2) {
        for (int item = tid; item < N * H; item += SS_THREADS) {   // consecutive lanes = consecutive heads of a row
          const int n = item / H, h = item - n * H;
          const T* kp = base + (long)n * 3 * C + C + h * D;
          float dot = 0.f;
          for (int c = 0; c < LP; ++c) {
            float kf[8];
            load8<T>(kp + c * 8, kf);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = fmaf(kf[j], qcls[h * D + c * 8 + j], dot);
          }
          region[h * N + n] = ss_logit<RB>(rb_of(a), dot * inv_sqrt_d, h, n);
        }
      } else {
        int n = tid / CP, c = tid - n * CP;
        while (n < N) {
          float kf[U][8];
          int nn[U], cc[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            nn[u] = n; cc[u] = c;
            if (n < N) load8<T>(base + (long)n * 3 * C + C + c * 8, kf[u]);
            n += dn; c += dc;
            if (c >= CP) { c -= CP; ++n; }
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (nn[u] < N) k_item(kf[u], nn[u], cc[u]);
        }
      }
    };
    // ---- vbar[n][:] = mean_h v[n,h,:]   (importance.py:24): thread (token n, 16-byte slice `sub` of the head dim),
    //      12 head rows in flight, summed in head order (fixed tree)
    auto v_item = [&](int n) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const T* vp = base + (long)n * 3 * C + 2 * C + sub * 8;
      for (int h0 = 0; h0 < H; h0 += 12) {
        float vf[12][8];
#pragma unroll
        for (int u = 0; u < 12; ++u)
          if (h0 + u < H) load8<T>(vp + (h0 + u) * D, vf[u]);
#pragma unroll
        for (int u = 0; u < 12; ++u)
          if (h0 + u < H) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += vf[u][j];
          }
      }
      float* dst = vbar + n * D + sub * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = acc[j] * inv_h;
    };
    auto v_pass = [&]() {
      for (int n = grp < ngrp ? grp : N; n < N; n += ngrp) v_item(n);
    };
    // ---- per-head softmax statistics over ALL N tokens (importance.py:20), then A_cls[n] = mean_h softmax_h[n]
    //      (importance.py:21)
    auto softmax_stats = [&]() {
      for (int h = wave; h < H; h += SS_THREADS / 64) {
        float mx = -INFINITY;
        for (int n = lane; n < N; n += 64) mx = fmaxf(mx, region[h * N + n]);
        mx = wave_max(mx);
        float se = 0.f;
        for (int n = lane; n < N; n += 64) se += __expf(region[h * N + n] - mx);
        se = wave_sum(se);
        if (lane == 0) { hstat[h] = mx; hstat[H + h] = se; }
      }
      __syncthreads();
      // A_cls[n] = (1/H) sum_h exp(l[h][n] - max_h) / sum_h: FOUR lanes per token, lane q sums heads q, q + 4, ... in head
      // order, the four partial sums join in a fixed quad tree (one lane per token left 80 % of the workgroup idle
      // through 12 dependent exp / divide steps: 2.5k of the kernel's 79k cycles at 197 tokens)
      for (int n0 = 0; n0 < N; n0 += SS_THREADS / 4) {
        const int n = n0 + (tid >> 2), q = tid & 3;
        float s = 0.f;
        if (n < N)
          for (int h = q; h < H; h += 4) s += __expf(region[h * N + n] - hstat[h]) / hstat[H + h];
        s = dpp_add<0xB1>(s);
        s = dpp_add<0x4E>(s);
        if (n < N && q == 0) acls[n] = s / (float)H;
      }
    };

    if (MERGED && pow2) {
      // ONE pass over the K and V thirds: per iteration a thread has U K chunks and the H head rows of one V
      // item in flight (every result is the same fixed-order sum as in the two-pass form: bit-identical scores)
      constexpr int UM = RAJNI_SS_KUM, VU = RAJNI_SS_VUM;
      int n = tid / CP, c = tid - n * CP;
      int nv = grp < ngrp ? grp : N;
      while (n < N || nv < N) {
        float kf[UM][8];
        int nn[UM], cc[UM];
#pragma unroll
        for (int u = 0; u < UM; ++u) {
          nn[u] = n; cc[u] = c;
          if (n < N) load8<T>(base + (long)n * 3 * C + C + c * 8, kf[u]);
          n += dn; c += dc;
          if (c >= CP) { c -= CP; ++n; }
        }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool vdo = nv < N;
        const T* vp = base + (long)(vdo ? nv : 0) * 3 * C + 2 * C + sub * 8;
        float vf[VU][8];
#pragma unroll
        for (int u = 0; u < VU; ++u)
          if (vdo && u < H) load8<T>(vp + u * D, vf[u]);
#pragma unroll
        for (int u = 0; u < UM; ++u)
          if (nn[u] < N) k_item(kf[u], nn[u], cc[u]);
        if (vdo) {
#pragma unroll
          for (int u = 0; u < VU; ++u)
            if (u < H) {
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[j] += vf[u][j];
            }
          for (int h0 = VU; h0 < H; h0 += VU) {       // further rounds of VU head rows, summed in head order
#pragma unroll
            for (int u = 0; u < VU; ++u)
              if (h0 + u < H) load8<T>(vp + (h0 + u) * D, vf[u]);
#pragma unroll
            for (int u = 0; u < VU; ++u)
              if (h0 + u < H) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += vf[u][j];
              }
          }
          float* dst = vbar + nv * D + sub * 8;
#pragma unroll
          for (int j = 0; j < 8; ++j) dst[j] = acc[j] * inv_h;
          nv += ngrp;
        }
      }
      __syncthreads();
      SS_STAMP(1);
      softmax_stats();
      __syncthreads();
      SS_STAMP(2);
    } else {
      k_pass();
      __syncthreads();
      SS_STAMP(1);
      softmax_stats();
      __syncthreads();  // logits are dead: region becomes vbar (two-pass layout)
      SS_STAMP(2);
      v_pass();
      __syncthreads();
    }
    SS_STAMP(3);
    // ---- token mean of vbar, fixed-order two-level sum (importance.py:25)
    {
      const int d = tid % D, prt = tid / D, nparts = SS_PART / D;      // threads past nparts * D idle
      // four independent chains (tokens prt, prt + nparts, ...: chain = step mod 4), joined in a fixed tree: one
      // dependent LDS-read + add chain of N / nparts = 25 steps was 3k of the kernel's cycles
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      int n = prt < nparts ? prt : N;
      for (; n + 3 * nparts < N; n += 4 * nparts) {
        s0 += vbar[n * D + d]; s1 += vbar[(n + nparts) * D + d];
        s2 += vbar[(n + 2 * nparts) * D + d]; s3 += vbar[(n + 3 * nparts) * D + d];
      }
      if (n < N) s0 += vbar[n * D + d];
      if (n + nparts < N) s1 += vbar[(n + nparts) * D + d];
      if (n + 2 * nparts < N) s2 += vbar[(n + 2 * nparts) * D + d];
      const float s = (s0 + s1) + (s2 + s3);
      if (prt < nparts) part[prt * D + d] = s;
      __syncthreads();
      if (tid < D) {
        float t = 0.f;
        for (int q = 0; q < nparts; ++q) t += part[q * D + tid];
        mean[tid] = t / (float)N;
      }
      __syncthreads();
    }
    // ---- ||vbar[n] - mean||_2   (importance.py:27)
    if (!pow2) {
      for (int n = tid; n < N; n += SS_THREADS) {
        float ss = 0.f;
        for (int d = 0; d < D; ++d) {
          const float dlt = vbar[n * D + d] - mean[d];
          ss = fmaf(dlt, dlt, ss);
        }
        sc[n] = sqrtf(ss);
      }
    } else
    for (int n = grp; n < N; n += ngrp) {
      const float* src = vbar + n * D + sub * 8;
      const float* mp = mean + sub * 8;
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dlt = src[j] - mp[j];
        ss = fmaf(dlt, dlt, ss);
      }
      ss = group_sum(ss, LP);
      if (sub == 0) sc[n] = sqrtf(ss);
    }
    __syncthreads();
    SS_STAMP(4);
    // ---- mu, unbiased std + eps over tokens   (importance.py:28-29)
    //      (every wave reducing the norms itself - one barrier and the broadcast fewer - was measured: +400 cycles)
    if (wave == 0) {
      float s = 0.f;
      for (int n = lane; n < N; n += 64) s += sc[n];
      const float mu = wave_sum(s) / (float)N;
      float ss = 0.f;
      for (int n = lane; n < N; n += 64) {
        const float dlt = sc[n] - mu;
        ss = fmaf(dlt, dlt, ss);
      }
      ss = wave_sum(ss);
      if (lane == 0) {
        misc[0] = mu;
        misc[1] = sqrtf(ss / (float)(N - 1)) + a.eps;
      }
    }
    __syncthreads();
    // ---- score = A_cls * sigmoid(z), rounded to the I/O dtype   (importance.py:31-34)
    {
      const float mu = misc[0], sd = misc[1];
      for (int n = tid; n < N; n += SS_THREADS) {
        const float z = (sc[n] - mu) / sd;
        const float sig = 1.0f / (1.0f + __expf(-z));
        const float sv = round_to<T>(acls[n] * sig);   // what the reference returns: qkv's dtype
        if (a.scores_out != nullptr) st1(reinterpret_cast<T*>(a.scores_out) + (long)b * N + n, sv);
        sc[n] = sv;
      }
    }
    __syncthreads();
  } else {
    for (int n = tid; n < N; n += SS_THREADS) sc[n] = ld1(reinterpret_cast<const T*>(a.scores_in) + (long)b * N + n);
    __syncthreads();
  }

  SS_STAMP(5);
  if (a.keep <= 0) return;
  // A_cls and the logits' region are dead: they hold the ranking keys (fp32 / packed 16-bit; the region has >= ss_key_words(N, P) words)
  select_tail<T>(a, b, sc, acls, reinterpret_cast<unsigned*>(region), wcount);
}

size_t ss_lds_bytes(int N, int H, int D, int P, bool merged, bool qmean = false) {
  const size_t C = (size_t)H * D;
  const size_t region = (size_t)ss_region_words(N, H, D, P, merged, qmean);
  return (C + region + 2 * (size_t)N + 2 * (size_t)H + SS_PART + D + 16 + SS_THREADS / 64) * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------------
// The TILED form: shapes whose [H][N] logits and [N][D] head-mean values do not fit one workgroup's LDS.
//   score_tile_kernel    grid (token tiles, B): a workgroup owns ST_TILE consecutive tokens, reads the CLS query row and its
//                        tokens' K and V thirds once (16-byte loads) and writes, to the caller's scratch: fp32 logits
//                        [B][H][N], fp32 vbar [B][N][D], the tile's column sums of vbar [B][tiles][D] and the tile's
//                        per-head softmax statistics (max, sum exp) [B][tiles][H][2].
//   score_finish_kernel  one workgroup per image: joins the tiles' statistics and column sums in tile order, computes
//                        A_cls, the norms (vbar read back from the scratch: L2 resident), mu / std and the scores, then
//                        runs select_tail.  Its LDS holds O(N) words - never [N][D].
// Every sum is a fixed tree over a fixed order that depends on (N, H, D) alone: the same image gives the same bits at any
// batch size and batch position.  The sums are not the single-workgroup kernel's, so the two paths agree within the
// budget of the numerics tests and not bit for bit.
constexpr int ST_TILE = 32;       // tokens per workgroup: a constant (never a function of B or the CU count: the sum order hangs on it)
constexpr int ST_THREADS = 256;   // 32 tokens x 8 lanes per 64-wide head row; 4 waves at ~88 VGPRs: 5 workgroups per CU, so a CU overlaps tiles
constexpr int ST_KU = 4;          // K chunks in flight per lane
constexpr int ST_MAX_N = 16384 + RAJNI_MAX_PREFIX;   // cap of the tiled path: 2048 px at patch 16 with any prefix count (the finish kernel's LDS would hold ~19.8k tokens; the packed key 65535)

struct TiledArgs {
  int tiles;
  float* logits;    // [B][H][N]
  float* vbar;      // [B][N][D]
  float* colsum;    // [B][tiles][D]
  float* stats;     // [B][tiles][H][2]: max, sum of exp(l - max) over the tile's tokens
  float* qbar;      // [B][C] the mean query (score_qmean_kernel wrote it), or null: the query is row 0
};

// RAJNI_QUERY_MEAN on the tiled path: qbar[b][c] = (1 / N) sum_n q[b, n, c], fp32, before the tiles launch.  A workgroup owns
// SQ_COLS consecutive columns of one image: thread (partition q, 16-byte chunk c) sums rows q, q + SQ_PARTS, ... in row order
// (four loads in flight, added in order), the partial sums meet in LDS and column c joins them in partition order.  The order
// hangs on nothing but N: bit-repeatable, the same bits at any batch size and position.
constexpr int SQ_COLS = 64, SQ_PARTS = 32, SQ_THREADS = (SQ_COLS / 8) * SQ_PARTS;
template <typename T>
__global__ void __launch_bounds__(SQ_THREADS) score_qmean_kernel(const T* __restrict__ qkv, float* __restrict__ qbar, int N, int C) {
  __shared__ float part[SQ_PARTS][SQ_COLS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int q = tid / (SQ_COLS / 8), cl = tid - q * (SQ_COLS / 8);
  const int c0 = blockIdx.x * SQ_COLS + cl * 8;      // first of this thread's 8 columns
  const T* qp = qkv + (size_t)b * N * 3 * C + c0;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < C) {
    for (int n = q; n < N; n += 4 * SQ_PARTS) {
      float f[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (n + u * SQ_PARTS < N) load8<T>(qp + (size_t)(n + u * SQ_PARTS) * 3 * C, f[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (n + u * SQ_PARTS < N) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += f[u][j];
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[q][cl * 8 + j] = acc[j];
  __syncthreads();
  const int c = blockIdx.x * SQ_COLS + tid;
  if (tid < SQ_COLS && c < C) {
    float t = 0.f;
    for (int r = 0; r < SQ_PARTS; ++r) t += part[r][tid];
    qbar[(size_t)b * C + c] = t * (1.0f / (float)N);
  }
}

template <typename T, typename Args = ScoreArgs>
__global__ void __launch_bounds__(ST_THREADS) score_tile_kernel(const Args a, const TiledArgs t) {
  constexpr bool RB = !__is_same(Args, ScoreArgs);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int N = a.N, H = a.H, D = a.D, C = H * D;
  const int t0 = tile * ST_TILE, tn = N - t0 < ST_TILE ? N - t0 : ST_TILE;   // this tile's tokens: t0 .. t0 + tn - 1
  float* qcls = sm;                 // [C]
  float* lt = qcls + C;             // logits of the tile [H][ST_TILE]
  float* vt = lt + H * ST_TILE;     // vbar of the tile [ST_TILE][D]
  const T* base = reinterpret_cast<const T*>(a.qkv) + (size_t)b * N * 3 * C;
  const T* tbase = base + (size_t)t0 * 3 * C;
  const int LP = D >> 3;
  const bool pow2 = LP == 4 || LP == 8 || LP == 16;     // as in score_select_kernel: DPP group sums, else the plain forms
  const int sub = tid % LP, grp = tid / LP, ngrp = ST_THREADS / LP;

  if (t.qbar != nullptr) {   // the mean query (workgroup-uniform)
    for (int c = tid; c < C; c += ST_THREADS) qcls[c] = t.qbar[(size_t)b * C + c];
  } else {
    for (int c = tid; c < (C >> 3); c += ST_THREADS) {
      float f[8];
      load8<T>(base + c * 8, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) qcls[c * 8 + j] = f[j];
    }
  }
  __syncthreads();

  // ---- logits of the tile's tokens (the lane mappings of score_select_kernel, over tn tokens instead of N)
  const float inv_sqrt_d = 1.0f / sqrtf((float)D);
  const float inv_h = 1.0f / (float)H;
  const int CP = C >> 3;
  if (!pow2) {
    for (int item = tid; item < tn * H; item += ST_THREADS) {
      const int n = item / H, h = item - n * H;
      const T* kp = tbase + (size_t)n * 3 * C + C + h * D;
      float dot = 0.f;
      for (int c = 0; c < LP; ++c) {
        float kf[8];
        load8<T>(kp + c * 8, kf);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot = fmaf(kf[j], qcls[h * D + c * 8 + j], dot);
      }
      lt[h * ST_TILE + n] = ss_logit<RB>(rb_of(a), dot * inv_sqrt_d, h, t0 + n);
    }
  } else {
    const int dn = ST_THREADS / CP, dc = ST_THREADS - dn * CP;   // item index += ST_THREADS
    int n = tid / CP, c = tid - n * CP;
    while (n < tn) {
      float kf[ST_KU][8];
      int nn[ST_KU], cc[ST_KU];
#pragma unroll
      for (int u = 0; u < ST_KU; ++u) {
        nn[u] = n; cc[u] = c;
        if (n < tn) load8<T>(tbase + (size_t)n * 3 * C + C + c * 8, kf[u]);
        n += dn; c += dc;
        if (c >= CP) { c -= CP; ++n; }
      }
#pragma unroll
      for (int u = 0; u < ST_KU; ++u)
        if (nn[u] < tn) {
          const float4 q0 = *reinterpret_cast<const float4*>(qcls + cc[u] * 8);
          const float4 q1 = *reinterpret_cast<const float4*>(qcls + cc[u] * 8 + 4);
          float dot = kf[u][0] * q0.x;
          dot = fmaf(kf[u][1], q0.y, dot); dot = fmaf(kf[u][2], q0.z, dot); dot = fmaf(kf[u][3], q0.w, dot);
          dot = fmaf(kf[u][4], q1.x, dot); dot = fmaf(kf[u][5], q1.y, dot); dot = fmaf(kf[u][6], q1.z, dot);
          dot = fmaf(kf[u][7], q1.w, dot);
          dot = group_sum(dot, LP);     // the LP lanes of a head row are one aligned group with one token: all in or all out
          if ((cc[u] & (LP - 1)) == 0) lt[(cc[u] / LP) * ST_TILE + nn[u]] = ss_logit<RB>(rb_of(a), dot * inv_sqrt_d, cc[u] / LP, t0 + nn[u]);
        }
    }
  }
  // ---- vbar of the tile's tokens: thread (token, 16-byte slice of the head dim), heads summed in head order
  for (int n = grp < ngrp ? grp : tn; n < tn; n += ngrp) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const T* vp = tbase + (size_t)n * 3 * C + 2 * C + sub * 8;
    for (int h0 = 0; h0 < H; h0 += 8) {
      float vf[8][8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (h0 + u < H) load8<T>(vp + (h0 + u) * D, vf[u]);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (h0 + u < H) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += vf[u][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv_h;
    float* dst = vt + n * D + sub * 8;
    reinterpret_cast<float4*>(dst)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    reinterpret_cast<float4*>(dst)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    store8<float>(t.vbar + ((size_t)b * N + t0 + n) * D + sub * 8, acc);
  }
  __syncthreads();

  // ---- the tile's softmax statistics per head (one token per lane: ST_TILE <= 64), its logits, its column sums
  for (int h = wave; h < H; h += ST_THREADS / 64) {
    const float l = lane < tn ? lt[h * ST_TILE + lane] : -INFINITY;
    const float mx = wave_max(l);
    const float se = wave_sum(lane < tn ? __expf(l - mx) : 0.f);
    if (lane == 0)
      *reinterpret_cast<float2*>(t.stats + (((size_t)b * t.tiles + tile) * H + h) * 2) = make_float2(mx, se);
  }
  for (int i = tid; i < H * ST_TILE; i += ST_THREADS) {
    const int h = i / ST_TILE, j = i - h * ST_TILE;
    if (j < tn) t.logits[((size_t)b * H + h) * N + t0 + j] = lt[i];
  }
  if (tid < D) {   // four chains (token j mod 4), joined in a fixed tree
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int j = 0; j < tn; j += 4) {
      s0 += vt[j * D + tid];
      if (j + 1 < tn) s1 += vt[(j + 1) * D + tid];
      if (j + 2 < tn) s2 += vt[(j + 2) * D + tid];
      if (j + 3 < tn) s3 += vt[(j + 3) * D + tid];
    }
    t.colsum[((size_t)b * t.tiles + tile) * D + tid] = (s0 + s1) + (s2 + s3);
  }
}

template <typename T>
__global__ void __launch_bounds__(SS_THREADS) score_finish_kernel(const ScoreArgs a, const TiledArgs t) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int N = a.N, H = a.H, D = a.D, tiles = t.tiles;
  const int kw = ss_key_words(N, a.P), n4 = (N + 3) & ~3;
  float* acls = sm;                           // [N], then the ranking keys (max(N, key words) words)
  float* sc = acls + (kw > n4 ? kw : n4);     // vnorm [N] then scores [N]
  float* hstat = sc + N;                      // [2H]
  float* part = hstat + 2 * H;                // [SS_THREADS]
  float* mean = part + SS_THREADS;            // [D]
  float* misc = mean + D;                     // [16]
  int* wcount = reinterpret_cast<int*>(misc + 16);   // [SS_THREADS / 64]
  const float* logits = t.logits + (size_t)b * H * N;
  const float* vbar = t.vbar + (size_t)b * N * D;
  const int LP = D >> 3;
  const bool pow2 = LP == 4 || LP == 8 || LP == 16;
  const int sub = tid % LP, grp = tid / LP, ngrp = SS_THREADS / LP;

  // ---- per-head softmax statistics over all N tokens from the tiles': max of the maxima, sum of the rescaled sums
  //      (lane l takes tiles l, l + 64, ... in tile order, then the wave's fixed tree)
  for (int h = wave; h < H; h += SS_THREADS / 64) {
    const float* st = t.stats + ((size_t)b * tiles * H + h) * 2;
    float mx = -INFINITY;
    for (int i = lane; i < tiles; i += 64) mx = fmaxf(mx, st[(size_t)i * H * 2]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int i = lane; i < tiles; i += 64) se += st[(size_t)i * H * 2 + 1] * __expf(st[(size_t)i * H * 2] - mx);
    se = wave_sum(se);
    if (lane == 0) { hstat[h] = mx; hstat[H + h] = se; }
  }
  // ---- token mean of vbar from the tiles' column sums: partial sums over tiles prt, prt + nparts, ..., joined in order
  {
    const int d = tid % D, prt = tid / D, nparts = SS_THREADS / D;
    if (prt < nparts) {
      float s = 0.f;
      for (int i = prt; i < tiles; i += nparts) s += t.colsum[((size_t)b * tiles + i) * D + d];
      part[prt * D + d] = s;
    }
    __syncthreads();
    if (tid < D) {
      float s = 0.f;
      for (int q = 0; q < nparts; ++q) s += part[q * D + tid];
      mean[tid] = s / (float)N;
    }
    __syncthreads();
  }
  // ---- A_cls[n] = mean_h softmax_h[n]: four lanes per token as in score_select_kernel
  for (int n0 = 0; n0 < N; n0 += SS_THREADS / 4) {
    const int n = n0 + (tid >> 2), q = tid & 3;
    float s = 0.f;
    if (n < N)
      for (int h = q; h < H; h += 4) s += __expf(logits[(size_t)h * N + n] - hstat[h]) / hstat[H + h];
    s = dpp_add<0xB1>(s);
    s = dpp_add<0x4E>(s);
    if (n < N && q == 0) acls[n] = s / (float)H;
  }
  // ---- ||vbar[n] - mean||_2
  if (!pow2) {
    for (int n = tid; n < N; n += SS_THREADS) {
      float ss = 0.f;
      for (int d = 0; d < D; d += 8) {
        float v[8];
        load8<float>(vbar + (size_t)n * D + d, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dlt = v[j] - mean[d + j];
          ss = fmaf(dlt, dlt, ss);
        }
      }
      sc[n] = sqrtf(ss);
    }
  } else {
    const int rounds = (N + ngrp - 1) / ngrp;     // whole groups step together: the DPP adds need every lane of a group
    for (int r = 0; r < rounds; ++r) {
      const int n = r * ngrp + grp;
      float ss = 0.f;
      if (n < N) {
        float v[8];
        load8<float>(vbar + (size_t)n * D + sub * 8, v);
        const float* mp = mean + sub * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dlt = v[j] - mp[j];
          ss = fmaf(dlt, dlt, ss);
        }
      }
      ss = group_sum(ss, LP);
      if (n < N && sub == 0) sc[n] = sqrtf(ss);
    }
  }
  __syncthreads();
  // ---- mu, unbiased std + eps over tokens
  if (wave == 0) {
    float s = 0.f;
    for (int n = lane; n < N; n += 64) s += sc[n];
    const float mu = wave_sum(s) / (float)N;
    float ss = 0.f;
    for (int n = lane; n < N; n += 64) {
      const float dlt = sc[n] - mu;
      ss = fmaf(dlt, dlt, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) {
      misc[0] = mu;
      misc[1] = sqrtf(ss / (float)(N - 1)) + a.eps;
    }
  }
  __syncthreads();
  {
    const float mu = misc[0], sd = misc[1];
    for (int n = tid; n < N; n += SS_THREADS) {
      const float z = (sc[n] - mu) / sd;
      const float sig = 1.0f / (1.0f + __expf(-z));
      const float sv = round_to<T>(acls[n] * sig);
      if (a.scores_out != nullptr) st1(reinterpret_cast<T*>(a.scores_out) + (size_t)b * N + n, sv);
      sc[n] = sv;
    }
  }
  __syncthreads();
  if (a.keep <= 0) return;
  select_tail<T>(a, b, sc, acls, reinterpret_cast<unsigned*>(acls), wcount);   // A_cls is dead: its words hold the keys
}

size_t st_tile_lds_bytes(int H, int D) { return ((size_t)H * D + (size_t)H * ST_TILE + (size_t)ST_TILE * D) * sizeof(float); }
size_t st_finish_lds_bytes(int N, int H, int D, int P) {
  const size_t kw = (size_t)ss_key_words(N, P), n4 = ((size_t)N + 3) & ~(size_t)3;
  return ((kw > n4 ? kw : n4) + (size_t)N + 2 * (size_t)H + SS_THREADS + D + 16 + SS_THREADS / 64) * sizeof(float);
}
inline size_t st_align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct TiledLayout { int tiles; size_t logits, vbar, colsum, stats, qbar, total; };   // byte offsets of the scratch regions
// (qmean: the mean query [B][C] behind everything else, so that no other offset moves)
TiledLayout st_layout(int B, int N, int H, int D, bool qmean = false) {
  TiledLayout l{};
  l.tiles = (N + ST_TILE - 1) / ST_TILE;
  size_t off = 0;
  auto take = [&](size_t floats) { const size_t o = off; off += st_align256(floats * sizeof(float)); return o; };
  l.logits = take((size_t)B * H * N);
  l.vbar = take((size_t)B * N * D);
  l.colsum = take((size_t)B * l.tiles * D);
  l.stats = take((size_t)B * l.tiles * H * 2);
  l.qbar = qmean ? take((size_t)B * H * D) : 0;
  l.total = off;
  return l;
}

int g_ss_force_tiled = 0;      // test hook: 1 = the tiled path wherever scratch is passed, even when one workgroup holds the shape

inline bool ss_shape_ok(int B, int N, int H, int D) { return B > 0 && N >= 2 && H > 0 && D >= 8 && D <= 128 && D % 8 == 0; }
// the single-workgroup layout cannot hold the shape (P = 1: the prefix count only matters for a handful of tokens)
inline bool ss_needs_tiles(int N, int H, int D, bool qmean = false) { return ss_lds_bytes(N, H, D, 1, false, qmean) > 160 * 1024; }

int g_ss_force_two_pass = 0;   // test hook (rajni_hip_debug.h): 1 = the two-pass layout even when the merged one fits

}  // namespace

extern "C" void rajni_debug_force_score_two_pass(int on) { g_ss_force_two_pass = on; }
extern "C" void rajni_debug_force_score_tiled(int on) { g_ss_force_tiled = on; }

// Scratch bytes rajni_score_select_ws needs: 0 wherever one workgroup holds the shape (and for shapes no path takes)
extern "C" size_t rajni_score_select_workspace_bytes(int B, int N, int H, int D, int dtype) {
  if (!(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16) || !ss_shape_ok(B, N, H, D) || N > ST_MAX_N) return 0;
  if (!ss_needs_tiles(N, H, D) && g_ss_force_tiled == 0) return 0;
  return st_layout(B, N, H, D).total;
}

// Scratch bytes rajni_score_select_query needs (rajni_hip_query.h): with RAJNI_QUERY_CLS what rajni_score_select_workspace_bytes
// returns; the mean query adds its [B][C] fp32 row behind that layout wherever the tiled path runs
extern "C" size_t rajni_score_select_query_workspace_bytes(int B, int N, int H, int D, int dtype, int query) {
  if (query != RAJNI_QUERY_MEAN) return query == RAJNI_QUERY_CLS ? rajni_score_select_workspace_bytes(B, N, H, D, dtype) : 0;
  if (!(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16) || !ss_shape_ok(B, N, H, D) || N > ST_MAX_N) return 0;
  if (!ss_needs_tiles(N, H, D, true) && g_ss_force_tiled == 0) return 0;
  return st_layout(B, N, H, D, true).total;
}

namespace {
// the tiled path: (the mean query's launch,) tile kernel + finish kernel, nothing else on the stream
int launch_score_tiled(ScoreArgs a, int B, int dtype, void* ws, size_t ws_bytes, hipStream_t s, bool qmean, const ScoreBias& rb) {
  const int N = a.N, H = a.H, D = a.D;
  RAJNI_REQUIRE(B <= RAJNI_MAX_GRID_YZ, RAJNI_ERR_UNSUPPORTED,
                "score/select: B=%d - one launch of the tiled path takes at most %d images (grid: token tiles x images)", B,
                RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE(N <= ST_MAX_N, RAJNI_ERR_UNSUPPORTED,
                "score/select: N=%d is beyond the tiled path's cap of %d tokens (one workgroup's LDS holds far fewer at H=%d D=%d)",
                N, ST_MAX_N, H, D);
  const size_t tl = st_tile_lds_bytes(H, D), fl = st_finish_lds_bytes(N, H, D, a.P);
  RAJNI_REQUIRE(tl <= 64 * 1024 && fl <= 160 * 1024, RAJNI_ERR_UNSUPPORTED,
                "score/select: N=%d H=%d D=%d needs %zu B (tile) / %zu B (finish) of LDS (caps: 64 KiB, 160 KiB; N <= %d)",
                N, H, D, tl, fl, ST_MAX_N);
  const TiledLayout l = st_layout(B, N, H, D, qmean);
  RAJNI_REQUIRE(ws != nullptr && ws_bytes >= l.total, RAJNI_ERR_INVALID,
                "score/select: the tiled path needs %zu B of scratch (%s), got %zu", l.total,
                qmean ? "rajni_score_select_query_workspace_bytes" : "rajni_score_select_workspace_bytes", ws_bytes);
  RAJNI_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, RAJNI_ERR_INVALID, "score/select: scratch must be 256-byte aligned");
  char* base = static_cast<char*>(ws);
  TiledArgs t{};
  t.tiles = l.tiles;
  t.logits = reinterpret_cast<float*>(base + l.logits); t.vbar = reinterpret_cast<float*>(base + l.vbar);
  t.colsum = reinterpret_cast<float*>(base + l.colsum); t.stats = reinterpret_cast<float*>(base + l.stats);
  t.qbar = qmean ? reinterpret_cast<float*>(base + l.qbar) : nullptr;
  typedef void (*kern_t)(const ScoreArgs, const TiledArgs);
  const kern_t tile = dtype == RAJNI_F16 ? &score_tile_kernel<f16_t> : dtype == RAJNI_F32 ? &score_tile_kernel<float> : &score_tile_kernel<bf16_t>;
  const kern_t fin = dtype == RAJNI_F16 ? &score_finish_kernel<f16_t> : dtype == RAJNI_F32 ? &score_finish_kernel<float> : &score_finish_kernel<bf16_t>;
  if (fl > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fin), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl);
    if (e != hipSuccess) {
      rajni_set_error("hipFuncSetAttribute(score_finish, %zu): %s", fl, hipGetErrorString(e));
      return RAJNI_ERR_LAUNCH;
    }
  }
  // algorithmic bytes: the K and V thirds and the CLS query row (mean query: the Q third) once, the scratch written once and
  // read once, the scores
  const double es = dtype == RAJNI_F32 ? 4.0 : 2.0;
  const double bytes = ((qmean ? 3.0 : 2.0) * N * H * D + (qmean ? 0 : H * D)) * es * B + 2.0 * (double)l.total + 4.0 * N * B;
  ProfScope prof(a.keep > 0 ? KC_SCORE_SELECT : KC_IMPORTANCE, s, 0.0, bytes);
  if (qmean) {
    const int C = H * D;
    const dim3 grid((C + SQ_COLS - 1) / SQ_COLS, B), block(SQ_THREADS);
    if (dtype == RAJNI_F32) hipLaunchKernelGGL(score_qmean_kernel<float>, grid, block, 0, s, (const float*)a.qkv, t.qbar, N, C);
    else if (dtype == RAJNI_F16) hipLaunchKernelGGL(score_qmean_kernel<f16_t>, grid, block, 0, s, (const f16_t*)a.qkv, t.qbar, N, C);
    else hipLaunchKernelGGL(score_qmean_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)a.qkv, t.qbar, N, C);
    RAJNI_CHECK_LAUNCH("score_qmean_kernel");
  }
  if (rb.pq != nullptr) {
    typedef void (*kern_rb_t)(const ScoreArgsRB, const TiledArgs);
    const kern_rb_t tile_rb = dtype == RAJNI_F16 ? &score_tile_kernel<f16_t, ScoreArgsRB>
                              : dtype == RAJNI_F32 ? &score_tile_kernel<float, ScoreArgsRB> : &score_tile_kernel<bf16_t, ScoreArgsRB>;
    ScoreArgsRB ar{};
    static_cast<ScoreArgs&>(ar) = a; ar.rb = rb;
    hipLaunchKernelGGL(tile_rb, dim3(l.tiles, B), dim3(ST_THREADS), tl, s, ar, t);
  } else {
    hipLaunchKernelGGL(tile, dim3(l.tiles, B), dim3(ST_THREADS), tl, s, a, t);
  }
  RAJNI_CHECK_LAUNCH("score_tile_kernel");
  hipLaunchKernelGGL(fin, dim3(B), dim3(SS_THREADS), fl, s, a, t);
  RAJNI_CHECK_LAUNCH("score_finish_kernel");
  return RAJNI_OK;
}
}  // namespace

// qkv != null: compute scores (and select when keep > 0); qkv == null: select from scores_in.
int launch_score_select(const void* qkv, const void* scores_in, int B, int N, int H, int D,
                        float eps, int keep, void* scores_out, int32_t* keep_idx,
                        void* next_scores, int dtype, hipStream_t s, int P, void* ws, size_t ws_bytes, int query,
                        const float* rb_pq, const float* rb_pqk, int rb_prefix) {
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID, "score/select: bad dtype %d", dtype);
  // (P = 0, a sequence without a class row, reaches here from rajni_hip_query.h alone: the other entry points refuse it themselves)
  RAJNI_REQUIRE(P >= 0 && P <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID, "score/select: num_prefix must be 0..%d (%d)", RAJNI_MAX_PREFIX, P);
  RAJNI_REQUIRE(query == RAJNI_QUERY_CLS || query == RAJNI_QUERY_MEAN, RAJNI_ERR_INVALID,
                "score/select: query must be RAJNI_QUERY_CLS or RAJNI_QUERY_MEAN (%d)", query);
  RAJNI_REQUIRE(B > 0 && N >= P + 1 && N >= 2, RAJNI_ERR_INVALID, "score/select: need B > 0 and N >= %d (B=%d N=%d)", P + 1 > 2 ? P + 1 : 2, B, N);
  RAJNI_REQUIRE(keep >= 0 && keep <= N - P, RAJNI_ERR_INVALID,
                "score/select: keep=%d out of range for N=%d with %d prefix tokens (keep_ratio must be <= 1)", keep, N, P);
  RAJNI_REQUIRE(keep == 0 || keep_idx != nullptr, RAJNI_ERR_INVALID, "score/select: keep_idx is null");
  ScoreArgs a{};
  a.N = N; a.keep = keep; a.eps = eps; a.P = P;
  a.scores_out = scores_out; a.keep_idx = keep_idx; a.next_scores = next_scores;
  a.stamps = rajni_g_stamps;
  // the class row's relative position bias: both value arrays or neither, a computed score, the class query
  RAJNI_REQUIRE((rb_pq != nullptr) == (rb_pqk != nullptr), RAJNI_ERR_INVALID, "score/select: prefix_q and prefix_qk come together");
  RAJNI_REQUIRE(!rb_pq || (qkv != nullptr && query == RAJNI_QUERY_CLS && rb_prefix >= 1 && rb_prefix <= RAJNI_MAX_PREFIX && rb_prefix < N),
                RAJNI_ERR_UNSUPPORTED, "score/select: a relative position bias needs computed scores, the class query and 1..%d prefix "
                "rows (the mean importance query has no position)", RAJNI_MAX_PREFIX);
  const ScoreBias rb{rb_pq, rb_pqk, rb_prefix};
  size_t lds;
  bool merged = false;
  const bool qmean = qkv != nullptr && query == RAJNI_QUERY_MEAN;
  if (qkv != nullptr) {
    RAJNI_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, RAJNI_ERR_UNSUPPORTED,
                  "importance: head dim %d not supported (multiples of 8 up to 128)", D);
    RAJNI_REQUIRE(H > 0, RAJNI_ERR_INVALID, "importance: H must be positive");
    a.qkv = qkv; a.H = H; a.D = D;
    // a shape one workgroup holds takes the kernel it always took; scratch serves the others (and any shape under the test hook)
    if (ws != nullptr && (ss_needs_tiles(N, H, D, qmean) || g_ss_force_tiled != 0)) return launch_score_tiled(a, B, dtype, ws, ws_bytes, s, qmean, rb);
    merged = ss_lds_bytes(N, H, D, P, true, qmean) <= 160 * 1024 && g_ss_force_two_pass == 0;   // else vbar reuses the logits' region
    lds = ss_lds_bytes(N, H, D, P, merged, qmean);
  } else {
    RAJNI_REQUIRE(scores_in != nullptr, RAJNI_ERR_INVALID, "select: scores is null");
    a.scores_in = scores_in; a.H = 1; a.D = 32;
    lds = ss_lds_bytes(N, 1, 32, P, false);
  }
  RAJNI_REQUIRE(lds <= 160 * 1024 || qkv == nullptr || N <= ST_MAX_N, RAJNI_ERR_UNSUPPORTED,
                "score/select: N=%d H=%d D=%d needs %zu B of LDS (> 160 KiB), and the tiled path (rajni_score_select_ws) is capped at N <= %d",
                N, H, D, lds, ST_MAX_N);
  RAJNI_REQUIRE(lds <= 160 * 1024, RAJNI_ERR_UNSUPPORTED,
                "score/select: N=%d H=%d D=%d needs %zu B of LDS (> 160 KiB)%s", N, H, D, lds,
                qkv != nullptr ? "; rajni_score_select_ws scores such shapes through caller-provided scratch" : "");
  const bool f32 = dtype == RAJNI_F32;
  typedef void (*kern_t)(const ScoreArgs);
  typedef void (*kern_rb_t)(const ScoreArgsRB);
  const kern_rb_t kern_rb = !rb_pq ? nullptr
      : dtype == RAJNI_F16 ? (merged ? &score_select_kernel<true, f16_t, true, false, ScoreArgsRB> : &score_select_kernel<true, f16_t, false, false, ScoreArgsRB>)
      : f32 ? (merged ? &score_select_kernel<true, float, true, false, ScoreArgsRB> : &score_select_kernel<true, float, false, false, ScoreArgsRB>)
            : (merged ? &score_select_kernel<true, bf16_t, true, false, ScoreArgsRB> : &score_select_kernel<true, bf16_t, false, false, ScoreArgsRB>);
  const kern_t kern = qmean
      ? (dtype == RAJNI_F16 ? (merged ? &score_select_kernel<true, f16_t, true, true> : &score_select_kernel<true, f16_t, false, true>)
         : f32 ? (merged ? &score_select_kernel<true, float, true, true> : &score_select_kernel<true, float, false, true>)
               : (merged ? &score_select_kernel<true, bf16_t, true, true> : &score_select_kernel<true, bf16_t, false, true>))
      : dtype == RAJNI_F16
      ? (qkv ? (merged ? &score_select_kernel<true, f16_t, true> : &score_select_kernel<true, f16_t, false>)
             : &score_select_kernel<false, f16_t, false>)
      : qkv ? (merged ? (f32 ? &score_select_kernel<true, float, true> : &score_select_kernel<true, bf16_t, true>)
                                    : (f32 ? &score_select_kernel<true, float, false> : &score_select_kernel<true, bf16_t, false>))
                          : (f32 ? &score_select_kernel<false, float, false> : &score_select_kernel<false, bf16_t, false>);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(kern_rb ? reinterpret_cast<const void*>(kern_rb) : reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      rajni_set_error("hipFuncSetAttribute(score_select, %zu): %s", lds, hipGetErrorString(e));
      return RAJNI_ERR_LAUNCH;
    }
  }
  const double es = f32 ? 4.0 : 2.0;
  const double bytes = qkv ? ((qmean ? 3.0 : 2.0) * N * H * D + (qmean ? 0 : H * D)) * es * B + 4.0 * N * B : 6.0 * N * B;
  ProfScope prof(qkv ? (keep > 0 ? KC_SCORE_SELECT : KC_IMPORTANCE) : KC_SELECT, s, 0.0, bytes);
  if (kern_rb) {
    ScoreArgsRB ar{};
    static_cast<ScoreArgs&>(ar) = a; ar.rb = rb;
    hipLaunchKernelGGL(kern_rb, dim3(B), dim3(SS_THREADS), lds, s, ar);
  } else {
    hipLaunchKernelGGL(kern, dim3(B), dim3(SS_THREADS), lds, s, a);
  }
  RAJNI_CHECK_LAUNCH("score_select_kernel");
  return RAJNI_OK;
}
