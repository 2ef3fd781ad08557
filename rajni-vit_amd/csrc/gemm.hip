// bf16 "TN" GEMM with fused epilogues for the packed-token linears (SURVEY k2,k13,k17,k18,k20).
//
//   Y[m][n] = epi( sum_k X[m][k] * W[n][k] )        X = activations [M,K], W = torch Linear weight [N,K]
//
// Common gfx950 design:
//   * both operands are K-contiguous, so every MFMA fragment is one 16-byte LDS read;
//   * tiles are staged HBM->LDS with LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction);
//     the LDS image is XOR-swizzled on the SOURCE address (LDS-DMA writes lane-linear) and the same
//     involution is applied on the fragment reads -> conflict-free ds_read_b128;
//   * v_mfma_f32_16x16x32_bf16 with W as the A operand and X as the B operand, so that a lane owns
//     ONE output row m and - through a permutation of which W row feeds which fragment row - a
//     chosen set of output columns (MAP_SEC / MAP_NAT below): epilogue loads/stores are 16-byte and
//     cover whole 64-byte sectors per row, and per-row epilogue data (gathered residual row,
//     patch->token row remap) is per-lane constant;
//   * workgroup -> tile mapping: every XCD gets a contiguous range of tile ids; ids run (N block of
//     ~1.5 MiB of W, row tile, column in block), see tile_mn.
//
// Tilings (chosen per launch, see choose_gemm):
//   wide  256 x 256 x 64, 8 waves, 2 LDS stages, persistent stream  - wide outputs (qkv, fc1)
//   mid   256 x 128 x 64, 8 waves, 3 LDS stages, persistent stream  - N = 768-class outputs (proj, fc2)
//   small 128 x 128 x 64, 4 waves, 2 stages, 2 workgroups per CU    - M < 1024 (head, tiny batches)
//   f32   128 x 128 x 32(fp32) on v_mfma_f32_16x16x4_f32            - fp32 models
// (Measured in round 1 and removed from this file, numbers in DESIGN.md section 4: 256x128x32 / 128x128x32
//  tilings with 64-byte rows, the wide tile on four waves of 128x128, per-SIMD-partner issue patterns,
//  front-loaded fragment reads / DMA, non-temporal epilogue accesses, cache-policy bits on the DMA loads, row
//  super-blocks in the tile order, round-balanced grids.)
#include <stdlib.h>
#include <type_traits>
#include "common.h"

namespace {

enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_PATCH = 3,
       EPI_GELU8 = 4,     // fp8 x fp8 kernel only (gemm_f8.h): bias + GELU, output re-quantised to e4m3 with a per-row scale
       EPI_QGELU = 5,     // bias + QuickGELU: EPI_GELU in everything but the function applied (see epi_act)
       EPI_SWIGLU = 6 };  // gated FC1: W is [2N, K] (gate rows, then value rows), the output silu(gate) * value is [M, N] (see gated_w_row)
// The activation epilogues of the 16-bit and fp32 kernels: a 16-bit (or fp32) output in the bias epilogue's column order and
// store path, FC1's non-temporal hidden store, the profile class KC_GEMM_GELU.  Whatever asks "is this an UNGATED FC1 epilogue"
// asks here.  (EPI_SWIGLU is FC1's epilogue too and is NOT one of these on purpose: it has a tail of its own, epilogue_tile_gated -
// half as many output columns, no TSTORE scratch - and names its non-temporal store, its store count (tile_stores) and its
// profile class where they are decided.)
constexpr bool epi_act(int epi) { return epi == EPI_GELU || epi == EPI_QGELU; }
enum { ALOAD_PLAIN = 0, ALOAD_PATCH = 1 };

struct GemmParams {
  const void* X; long lda;      // activations (bf16, or fp32 on the fp32 model path)
  const void* W; long ldw;      // weights, same element type (or fp8 e4m3 bytes, see wscale)
  const float* wscale;          // W8 kernels: W is fp8 e4m3 [N,K] and wscale[n] its per-row dequantisation scale
  const float* xscale;          // fp8 x fp8 kernel: X is fp8 e4m3 [M,K] and xscale[m] its per-row dequantisation scale
  const float* yscale;          // ... EPI_GELU8: output row m is stored as e4m3(gelu(.) / yscale[m])
  const float* bias;
  const float* gamma;
  const void* R; long ldr;      // residual stream rows (bf16 or fp32, see SF32)
  const int* ridx; int r_np, r_nsrc;
  void* Y; long ldc;            // output (fp32 when SF32: RESID / PATCH write the residual stream)
  int M, N, K;
  int tiles_n, total_tiles;
  int nblk;                     // persistent tilings: column tiles per N block of the tile order (tile_mn)
  // patch-embed A loader / epilogue
  int cin, S, log2ps, gw, npatch;   // S: image width in pixels, the row stride
  int IH;                       // image height in pixels: the channel stride is IH * S
  int nprefix;                  // prefix rows per image ahead of the patch rows: CLS + register tokens (>= 1)
  const void* pos; int pos_off; // pos-embed rows, activation dtype
  unsigned long long* stamps;   // diagnostic builds only (RAJNI_GEMM_STAMPS): 4 s_memtime values per block
  int stagger;                  // residual launches: every other workgroup of an XCD sleeps stagger x 8k cycles before its
                                // first tile (see g_resid_stagger); 0 = off
};

// exact-erf GELU (timm nn.GELU()) for the 16-bit paths, two values per instruction (v_pk_*_f32, no
// transcendentals):  gelu(x) = xl*(0.5 + h(x)),  h(x) = 0.5*erf(x/sqrt2) ~= xc*P(xc^2),
// xc = clamp(x, +-3*sqrt2), xl = max(x, -3*sqrt2), P = degree-8 least-squares fit on Chebyshev nodes (coefficients from
// tools/fit_gelu.py).  |gelu error| <= 4.24e-5 absolute - 1/50 of a bf16 ulp at |y| ~ 1 - against fp64 erf over [-8, 8]
// (tools/fit_gelu.py, this evaluation order; the maximum sits at the clamp point), and <= 1.21e-5 for every x below the
// clamp: the final multiplier is xl, not x, so the residual 0.5 + h(-X0) = 2.8e-6 is never scaled by a large |x| (with x
// itself the tail read -4.2e-5 at x = -15 and -2.8e-2 at x = -1e4, pre-activations a 16-bit model can produce).  Above the
// clamp the same residual is a RELATIVE error of 2.8e-6, far inside a 16-bit output's rounding.  For x >= -X0 the result is
// bit for bit what the unclamped multiplier gave.  Cost: the clamp is v_max_f32 + v_min_f32 where it was one v_med3_f32
// (+1 of ~9 VALU issues per element; 0.5 % of the ViT-B forward).  Two forms that keep the count were
// measured and not taken: a lower clamp at -4.24506521, where this evaluation order gives h = -0.5 exactly on the device (the
// tail is then exactly 0, but the error between the two clamp points rises to 4.98e-5 and the constant depends on the
// instruction sequence), and x * clamp(0.5 + x P(x^2), 0, 1) without an argument clamp (fewer instructions than before and
// exact tails, but other fp32 bits for every x: two selection-sensitive fp8 forward tests then miss their bars).
// tests/test_gpu_numerics.py holds the 16-bit epilogues to 5e-5 + one output rounding on a chosen grid.
// The FC1 epilogue is VALU bound: the previous exp+rcp form
// (Abramowitz-Stegun 7.1.26) cost ~20k cycles per 256x256 tile, a third of the tile's time.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// two pairs at once, the two Horner chains interleaved statement by statement: a packed fp32 op that reads the
// result of the one issued right before it costs a wait state (hipcc pads with s_nop 0: the single-chain form had one
// behind almost every v_pk_fma_f32 - ~600 per tile and wave, a quarter on top of the epilogue's VALU time); two
// independent chains fill each other's slots.
__device__ __forceinline__ void gelu_pk4(f32x2& a, f32x2& b) {
  const float X0 = 4.24264069f;
  const f32x2 lo = f32x2{-X0, -X0}, hi = f32x2{X0, X0};
  const f32x2 al = __builtin_elementwise_max(a, lo), bl = __builtin_elementwise_max(b, lo);
  const f32x2 ac = __builtin_elementwise_min(al, hi), bc = __builtin_elementwise_min(bl, hi);
  const f32x2 ua = ac * ac, ub = bc * bc;
  f32x2 qa = f32x2{5.405088552e-11f, 5.405088552e-11f}, qb = qa;
#define RAJNI_GELU_STEP(c) { const f32x2 k = f32x2{c, c}; qa = qa * ua + k; qb = qb * ub + k; }
  RAJNI_GELU_STEP(-5.202485173e-09f)
  RAJNI_GELU_STEP(2.215015442e-07f)
  RAJNI_GELU_STEP(-5.557312053e-06f)
  RAJNI_GELU_STEP(9.274613401e-05f)
  RAJNI_GELU_STEP(-1.104852507e-03f)
  RAJNI_GELU_STEP(9.805144109e-03f)
  RAJNI_GELU_STEP(-6.633033261e-02f)
  RAJNI_GELU_STEP(3.988969665e-01f)
#undef RAJNI_GELU_STEP
  const f32x2 ha = ac * qa, hb = bc * qb;
  const f32x2 half = f32x2{0.5f, 0.5f};
  const f32x2 ya = al * ha + al * half, yb = bl * hb + bl * half;
  a = ya; b = yb;
}

// QuickGELU (the OpenAI CLIP / MetaCLIP / DFN towers): x * sigmoid(1.702 x) = x * rcp(1 + exp2(-1.702 log2(e) x)), in fp32
// on the accumulators with the hardware v_exp_f32 / v_rcp_f32 (1 ulp each): |error| <= 7e-7 on [-8, 8] against fp64, far
// inside a 16-bit output's rounding.  The ends need no clamp: for large x the exponential underflows to 0 and the factor is
// rcp(1) = 1; for large -x it overflows to +inf (so does the argument product itself beyond |x| ~ 1.4e38), 1 + inf = inf,
// rcp(inf) = +0 and x * 0 = -0 for every finite x - no inf - inf, 0 * inf or inf / inf can form, so a finite pre-activation
// never yields NaN or inf.  act(0) = 0 * rcp(2) = 0 exactly: the zero-padded hidden columns of odd MLP widths stay zero.
// This is the plain form, and it is the cheaper epilogue of the two: measured on ViT-B FC1 launches 158 us against 170 us with
// gelu_pk4 (the FC1 class -6.9 %, DESIGN.md section 4 (13), profiles/quickgelu_ab.txt) - two transcendentals and three plain
// fp32 operations per element cost less than the clamped degree-8 packed polynomial.
__device__ __forceinline__ float quick_gelu1(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.4554669595930157f * x));
}
// (The two sites that apply an activation - epilogue_row and the interior path of epilogue_tile - keep the GELU loop spelled
//  out as it always was, with the QuickGELU loop beside it: routed through one shared helper, hipcc allocated the GELU
//  kernels' registers differently, and every kernel that existed before QuickGELU is held to identical machine code.)

// SiLU, the gate of the SwiGLU epilogue (EPI_SWIGLU): quick_gelu1 with the constant -log2(e), t * rcp(1 + exp2(-log2(e) t)).
// The ends behave as described there (silu(-huge) = -0, silu(0) = 0 exactly, no clamp), and the product silu(g) * v adds no
// case: silu(g) is finite for every finite g, so with v finite no 0 * inf can form - a finite (g, v) never yields NaN, and
// silu(0) * 0 = 0 keeps the zero-padded hidden columns zero.
__device__ __forceinline__ float silu1(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// ---- EPI_SWIGLU: the gated FC1.  W is [2N, K]: row n is the gate of hidden column n, row N + n its value; the output is
// [M, N].  A tile of BN W rows covers BN / 2 hidden columns, and the permutation that puts a column's gate and value into ONE
// lane sits in the tile LOADER alone: LDS tile row L is filled from the global W row gated_w_row(L) below, everything behind
// the loader - the LDS image, the swizzle keys (functions of the LDS row L only), w_frag_row and MAP_SEC - is what the bias
// epilogue has.  The LDS-DMA writes lane-linear and the swizzle is applied to the SOURCE chunk of a row, so which global row
// a piece's lanes read changes nothing in LDS: the conflict argument of w_key / w_key8 holds unchanged, row for row.
//   16-bit tilings: wave wn owns LDS rows 64 wn .. 64 wn + 63.  Its first 32 rows are the gates of hidden columns
//   h0 + 32 wn .. + 31 (h0 = first hidden column of the tile), its last 32 rows their values.  Under MAP_SEC a lane's v[j]
//   is tile column 64 wn + 8 g + j and v[8 + j] tile column 64 wn + 32 + 8 g + j: the gate and the value of hidden column
//   h0 + 32 wn + 8 g + j.  The product needs no exchange, the lane writes 8 consecutive outputs as one 16-byte store and
//   the 4 lanes of a row one whole 64-byte sector.
//   fp32 tiling: a lane owns the 16 consecutive tile columns 64 wn + 16 g .. + 15 - the first 8 are gates, the last 8 values.
// A staging piece is 8 (16-bit, fp32) or 16 (fp8 weights) consecutive LDS rows starting at a multiple of its size, so it never
// straddles a gate / value boundary of either layout: its lanes' rows stay consecutive global rows.
// Rows read: gates [h0, h0 + BN/2) - past N for a ragged last tile, into the value rows, never stored - and values
// [N + h0, N + h0 + BN/2) <= N + roundup(N, 128) <= roundup(2N, 256), the padded allocation of W (include/rajni_hip.h).
template <bool F32>
__device__ __forceinline__ long gated_w_row(int L, int N, int h0) {
  if (F32) return (long)((L >> 3) & 1) * N + h0 + (L >> 6) * 32 + ((L >> 4) & 3) * 8 + (L & 7);
  return (long)((L >> 5) & 1) * N + h0 + (L >> 6) * 32 + (L & 31);
}

// load / store 16 consecutive stream elements (the 16-bit activation format A, or fp32) as floats
template <bool F32, typename A>
__device__ __forceinline__ void load16(const void* base, long off, float* f) {
  if (F32) {
    const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float4 t = q[i]; f[4*i] = t.x; f[4*i+1] = t.y; f[4*i+2] = t.z; f[4*i+3] = t.w; }
  } else {
    const A* q = reinterpret_cast<const A*>(base) + off;
    unpack8<A>(*reinterpret_cast<const uint4*>(q), f);
    unpack8<A>(*reinterpret_cast<const uint4*>(q + 8), f + 8);
  }
}
template <bool F32, typename A>
__device__ __forceinline__ void load8s(const void* base, long off, float* f) {   // 8 stream elements
  if (F32) load8<float>(reinterpret_cast<const float*>(base) + off, f);
  else load8<A>(reinterpret_cast<const A*>(base) + off, f);
}
template <bool F32, typename A>
__device__ __forceinline__ void store8s(void* base, long off, const float* v) {
  if (F32) store8<float>(reinterpret_cast<float*>(base) + off, v);
  else store8<A>(reinterpret_cast<A*>(base) + off, v);
}
template <bool F32, typename A>
__device__ __forceinline__ float load1(const void* base, long off) {
  return F32 ? reinterpret_cast<const float*>(base)[off] : ld1(reinterpret_cast<const A*>(base) + off);
}
template <bool F32, typename A>
__device__ __forceinline__ void store16(void* base, long off, const float* v) {
  if (F32) {
    float4* q = reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
  } else {
    A* q = reinterpret_cast<A*>(base) + off;
    *reinterpret_cast<uint4*>(q) = pack8<A>(v);
    *reinterpret_cast<uint4*>(q + 8) = pack8<A>(v + 8);
  }
}
template <bool F32, typename A>
__device__ __forceinline__ void store1(void* base, long off, float v) {
  if (F32) reinterpret_cast<float*>(base)[off] = v;
  else st1(reinterpret_cast<A*>(base) + off, v);
}

// FC1's hidden activations (the largest tensor of a block: written once, read once by FC2) are stored NON-TEMPORAL:
// measured on the whole forward (tools/ab_libs.sh, round 3) FC1 -2..-3 %, +0.5 % end to end.  The rest of that experiment -
// keeping the fp32 residual stream resident in the 256 MiB Infinity Cache by also moving the QKV output and FC2's X-operand
// DMA past it - was negative: non-temporal X loads cost FC2 +15 % (its row panels are re-read by six column tiles out of L2),
// non-temporal QKV stores cost attention +4 %; neither made the residual epilogues or LayerNorm faster.
#ifndef RAJNI_FC1_NT
#define RAJNI_FC1_NT 1
#endif
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ void store_u4(void* ptr, const uint4& v) {
  if constexpr (NT) __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4*>(ptr));
  else *reinterpret_cast<uint4*>(ptr) = v;
}

// Vector stores per wave that an epilogue path issues for an INTERIOR tile of mi row groups (16 rows x 64 columns each).  The
// stream kernels let a tile's first counted wait leave that many outstanding (NSTORE, through tile_stores below), so count and
// code must not drift apart: a store loop's trip count is the constant counted here, spelled-out stores carry a static_assert.
constexpr int LINE_ROWS = 8;          // a whole-line access of a wave: 8 rows x 128 bytes per instruction (the LDS transpose below)
constexpr int ROW_STORES_SEC = 2;     // accumulator layout, per row: 2 x 8 16-bit values (MAP_SEC) ...
constexpr int ROW_STORES_NAT = 4;     // ... or 4 float4 (natural order)
constexpr int RM_HALVES = 2;          // ROWMAJOR, ROWMAJOR_WIDE: a row group's 64 fp32 columns leave as 2 halves of 128 bytes
constexpr int stores_acc_layout(bool nat, int mi) { return (nat ? ROW_STORES_NAT : ROW_STORES_SEC) * mi; }
constexpr int stores_rowmajor(int mi) { return RM_HALVES * (16 / LINE_ROWS) * mi; }
constexpr int stores_tstore(int mi) { return (16 / LINE_ROWS) * mi; }   // TSTORE: a row group's 64 16-bit columns are one line per row

// One output row m, columns nb..nb+15 (v = accumulators + bias on entry).
// SF32: the residual-stream tensors this launch touches (R and Y of RESID, Y of PATCH) are fp32.
// v[0..7] are columns nbA..nbA+7 and v[8..15] columns nbB..nbB+7 of output row m (nbB = nbA + 32: the
// sector mapping MAP_SEC below).
template <int EPI, bool SF32, typename A>
__device__ __forceinline__ void epilogue_row(const GemmParams& p, int m, int nbA, int nbB, float* v, const float* gam) {
  long orow = m;
  const bool full = nbB + 8 <= p.N;   // both halves inside N (nbA < nbB)
  if (EPI == EPI_GELU) {
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      f32x2 a = f32x2{v[j], v[j + 1]}, b = f32x2{v[j + 2], v[j + 3]};
      gelu_pk4(a, b);
      v[j] = a[0]; v[j + 1] = a[1]; v[j + 2] = b[0]; v[j + 3] = b[1];
    }
  } else if (EPI == EPI_QGELU) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = quick_gelu1(v[j]);
  } else if (EPI == EPI_RESID) {
    long rrow = m;
    if (p.ridx != nullptr) {
      const int b = m / p.r_np;
      rrow = (long)b * p.r_nsrc + p.ridx[m];
    }
    const long rbase = rrow * p.ldr;
    if (full) {
      float rf[16];
      load8s<SF32, A>(p.R, rbase + nbA, rf);
      load8s<SF32, A>(p.R, rbase + nbB, rf + 8);
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = fmaf(gam[j], v[j], rf[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int n = (j < 8 ? nbA : nbB - 8) + j;
        if (n < p.N) v[j] = fmaf(gam[j], v[j], load1<SF32, A>(p.R, rbase + n));
      }
    }
  } else if (EPI == EPI_PATCH) {
    const int b = m / p.npatch, pp = m - b * p.npatch;
    orow = (long)b * (p.npatch + p.nprefix) + p.nprefix + pp;
    const A* pr = reinterpret_cast<const A*>(p.pos) + (long)(pp + p.pos_off) * p.ldc;
    if (full) {
      float pf[16];
      unpack8<A>(*reinterpret_cast<const uint4*>(pr + nbA), pf);
      unpack8<A>(*reinterpret_cast<const uint4*>(pr + nbB), pf + 8);
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] += pf[j];
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int n = (j < 8 ? nbA : nbB - 8) + j;
        if (n < p.N) v[j] += ld1(pr + n);
      }
    }
  }
  constexpr bool OUT32 = SF32 && (EPI == EPI_RESID || EPI == EPI_PATCH);
  const long ybase = orow * p.ldc;
  if (full) {
    static_assert(ROW_STORES_SEC == 2, "the two stores of a full row below");
    store8s<OUT32, A>(p.Y, ybase + nbA, v);
    store8s<OUT32, A>(p.Y, ybase + nbB, v + 8);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = (j < 8 ? nbA : nbB - 8) + j;
      if (n < p.N) store1<OUT32, A>(p.Y, ybase + n, v[j]);
    }
  }
}

// ---- fp32 residual stream epilogues (RESID / PATCH with SF32) use the NATURAL column order --------
// With the permuted order a lane owns 16 consecutive columns = 64 bytes of fp32, so each of its four
// 16-byte accesses lands in a different 64-byte sector from its three row neighbours: one wave
// instruction touches 64 sectors.  Measured (tools/proj_probe.py): the fp32-stream proj GEMM took 151 us
// against 72 us with a bias-only bf16 epilogue.  In the natural order (W fragment row r of n-tile ni =
// column 16*ni + r) a lane owns columns 16*ni + 4*g + {0..3}: the four lanes of a row cover one whole
// 64-byte sector per access - 16 sectors per wave instruction, 4x fewer memory transactions.
constexpr bool nat_order(int epi, bool sf32) { return sf32 && (epi == EPI_RESID || epi == EPI_PATCH); }

// Which W tile row feeds fragment row r of n-tile ni decides which output columns a lane owns
// (accumulator element j = ni*4 + rg of a lane in lane group g; n0w = first column of the wave):
//   MAP_NAT  col = 16*ni + 4*g + rg          fp32 stream: 4 lanes of a row = one 64-byte sector (above)
//   MAP_SEC  col = 32*(ni>>1) + 8*g + 4*(ni&1) + rg   bf16 outputs: a lane owns 2 x 8 consecutive columns
//            and the 4 lanes of a row write one whole 64-byte sector per 16-byte store instruction.
//            (With 16 consecutive columns per lane every store instruction wrote 4 quarter sectors
//            per row: the wide tiling's epilogue took 9.5k cycles per 256x256 tile, store-issue bound.)
//   MAP_F8   col = 16*g + 4*ni + rg           fp8 outputs: a lane owns 16 consecutive columns = one 16-byte store,
//            the 4 lanes of a row one whole 64-byte sector
enum { MAP_NAT = 1, MAP_SEC = 2, MAP_F8 = 3 };
constexpr int col_map(int epi, bool sf32) { return epi == EPI_GELU8 ? MAP_F8 : nat_order(epi, sf32) ? MAP_NAT : MAP_SEC; }

// ---- epilogue scratch: LDS per wave behind the stages, through which an epilogue transposes its wave's block into whole
// 128-byte lines.  This is the ONE statement of which instantiation has how much: the kernels form their scratch pointer
// from it (non-null exactly when it is non-zero) and the host sizes the dynamic LDS with it (lds_bytes of each family).
#ifndef RAJNI_TSTORE
#define RAJNI_TSTORE 1      // bf16 outputs (BIAS, GELU) of the stream tilings leave as whole lines too
#endif
#ifndef RAJNI_F8W_LINES
#define RAJNI_F8W_LINES 1   // ... and the bf16 output of the fp8 x fp8 256 x 256 kernel (gemm_f8.h)
#endif
constexpr bool resid_nat(int epi, bool sf32) { return nat_order(epi, sf32) && epi == EPI_RESID; }
// fp32-stream RESID of gemm_bf16_tn_stream (mi = row groups per wave: 4 on 256 x 128, 8 on 256 x 256):
//   ROWMAJOR       256 x 128, 16-bit and fp8 weights alike: residual rows prefetched in full lines (prefetch_resid_rowmajor)
//   ROWMAJOR_WIDE  256 x 256: loads in the epilogue, group by group; the only one of the two that excludes fp8 weights (with
//                  the weight scale on top that instantiation spills: 256 x 256 with fp8 weights keeps the accumulator-layout
//                  epilogue)
constexpr bool epi_rowmajor(int epi, bool sf32, int mi) { return resid_nat(epi, sf32) && mi <= 4; }
constexpr bool epi_rowmajor_wide(int epi, bool sf32, int mi, bool w8) { return resid_nat(epi, sf32) && mi > 4 && !w8; }
constexpr bool epi_tstore(int epi) { return RAJNI_TSTORE && (epi == EPI_BIAS || epi_act(epi)); }
constexpr int stream_scratch_bytes(int epi, bool sf32, int mi, bool w8) {   // wide::gemm_bf16_tn_stream
  return (epi_rowmajor(epi, sf32, mi) || epi_rowmajor_wide(epi, sf32, mi, w8) || epi_tstore(epi)) ? 2048 : 0;
}
constexpr int f8_scratch_bytes(int epi, bool sf32) {   // f8::gemm_f8_tn_stream: fp32-stream RESID and bf16 outputs
  return (resid_nat(epi, sf32) || epi == EPI_BIAS) ? 2048 : 0;
}
constexpr int f8w_scratch_bytes(int epi) { return (epi == EPI_BIAS && RAJNI_F8W_LINES) ? 4096 : 0; }   // f8w::gemm_f8_tn_wide
constexpr int LDS_MAX_BYTES = 160 * 1024;   // per workgroup on gfx950

// The per-wave transpose through that scratch, rows of 128 bytes: a lane WRITES 16-byte chunks of the row it owns in the MFMA
// layout (lines_put), the wave passes lines_turn, and every read instruction (lines_get: row 8 j + (lane >> 3), chunk lane & 7)
// fetches LINE_ROWS rows x 128 bytes, which meet global memory as whole lines.  Chunk c of row r sits in slot c ^ (r & 7) of
// its row, a row being one half of a 256-byte bank row.  Conflict free both ways: the eight contiguous lanes of a ds_write_b128
// group write one chunk of eight consecutive rows - eight keys, eight slots; the sixteen lanes of a ds_read_b128 group read
// the eight chunks of two consecutive rows, the two halves of the bank row.  A block ends with a plain wave barrier behind
// its reads: they are issued before the next block's writes (LDS is in order per wave).
__device__ __forceinline__ void lines_put(char* scratch, int row, int chunk, const bf16x8& v) {
  const int slot = chunk ^ (row & 7);
  *reinterpret_cast<bf16x8*>(scratch + row * 128 + slot * 16) = v;
}
__device__ __forceinline__ void lines_turn() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ bf16x8 lines_get(const char* scratch, int row, int chunk) {
  const int slot = chunk ^ (row & 7);
  return *reinterpret_cast<const bf16x8*>(scratch + row * 128 + slot * 16);
}

template <int MAP>
__device__ __forceinline__ int out_col(int n0w, int g, int j) {
  const int ni = j >> 2, rg = j & 3;
  return MAP == MAP_NAT ? n0w + 16 * ni + 4 * g + rg
       : MAP == MAP_F8 ? n0w + 16 * g + 4 * ni + rg : n0w + 32 * (ni >> 1) + 8 * g + 4 * (ni & 1) + rg;
}
// W tile row (relative to the wave's first W row) read by fragment row l15 of n-tile ni
template <int MAP>
__device__ __forceinline__ int w_frag_row(int l15, int ni) {
  return MAP == MAP_NAT ? ni * 16 + l15
       : MAP == MAP_F8 ? 16 * (l15 >> 2) + 4 * ni + (l15 & 3) : 32 * (ni >> 1) + 8 * (l15 >> 2) + 4 * (ni & 1) + (l15 & 3);
}
// swizzle key of a W tile row for 128-byte-row tilings: the 16 rows one ds_read_b128 lane group
// touches must land in 16 distinct 16-byte slots of the 256-byte bank row
template <int MAP>
__device__ __forceinline__ int w_key(int row) {
  return MAP == MAP_NAT ? (row >> 1) & 7
       : MAP == MAP_F8 ? ((row >> 4) & 3) * 2 + ((row >> 1) & 1) : ((row >> 3) & 3) * 2 + ((row >> 1) & 1);
}

// ---- fp8 (e4m3) weights: 64-byte tile rows (BK = 64 one-byte elements) -----------------------------
// A W fragment of v_mfma_f32_16x16x32_bf16 is 8 consecutive k of one row = 8 BYTES here (ds_read_b64),
// converted to bf16 in registers (v_cvt_scalef32_pk_bf16_fp8, exact); the per-row scale multiplies the
// fp32 accumulator in the epilogue, so the arithmetic is x . (q * s) - a bf16 activation times the
// DEQUANTISED weight - with fp32 accumulation.  LDS-DMA still moves 16-byte units, so the swizzle
// works on the four 16-byte units of a row: a ds_read_b64 lane group (32 lanes: 16 rows x 2 halves)
// is conflict free when the 4 rows of every (row % 4) class sit in 4 distinct units.
template <int MAP>
__device__ __forceinline__ int w_key8(int row) {
  return MAP == MAP_NAT ? (row >> 2) & 3 : (row >> 3) & 3;
}
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(uint2 raw) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw.x, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw.x, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw.y, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw.y, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// The 8 fp8 bytes are read from LDS through a __bf16 vector type ON PURPOSE: hipcc's waitcnt insertion
// puts s_waitcnt vmcnt(0) in front of every LDS read that type-based alias analysis cannot separate
// from the LDS-DMA writes - with a uint2 read each W fragment read drained the whole DMA queue (the
// mid tiling ran at 390 instead of 840 TFLOP/s).  Reads typed like the bf16 fragments are left alone.
typedef __attribute__((ext_vector_type(4))) __bf16 fp8x8_raw;
template <bool W8> struct WFragT { typedef bf16x8 type; };
template <> struct WFragT<true> { typedef fp8x8_raw type; };
__device__ __forceinline__ bf16x8 w_frag_bf16(const bf16x8& f) { return f; }
__device__ __forceinline__ bf16x8 w_frag_bf16(const fp8x8_raw& f) { return fp8x8_to_bf16(__builtin_bit_cast(uint2, f)); }

// natural-order epilogue of one output row (fp32 stream): v = accumulators + bias on entry
template <int EPI, typename A>
__device__ __forceinline__ void epilogue_row_nat(const GemmParams& p, int m, int n0w, int g, float* v, const float* gam) {
  long orow = m, rrow = m;
  int pp = 0;
  if (EPI == EPI_RESID && p.ridx != nullptr) {
    const int b = m / p.r_np;
    rrow = (long)b * p.r_nsrc + p.ridx[m];
  }
  if (EPI == EPI_PATCH) {
    const int b = m / p.npatch;
    pp = m - b * p.npatch;
    orow = (long)b * (p.npatch + p.nprefix) + p.nprefix + pp;
  }
  const float* R = reinterpret_cast<const float*>(p.R);
  const A* P = reinterpret_cast<const A*>(p.pos);
  float* Y = reinterpret_cast<float*>(p.Y);
#pragma unroll
  for (int ni = 0; ni < ROW_STORES_NAT; ++ni) {   // one float4 store per n-tile
    const int c = n0w + 16 * ni + 4 * g;
    float* vv = v + 4 * ni;
    if (c + 4 <= p.N) {
      if (EPI == EPI_RESID) {
        const float4 r = *reinterpret_cast<const float4*>(R + rrow * p.ldr + c);
        vv[0] = fmaf(gam[4 * ni + 0], vv[0], r.x); vv[1] = fmaf(gam[4 * ni + 1], vv[1], r.y);
        vv[2] = fmaf(gam[4 * ni + 2], vv[2], r.z); vv[3] = fmaf(gam[4 * ni + 3], vv[3], r.w);
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(P + (long)(pp + p.pos_off) * p.ldc + c);
        vv[0] += lo16<A>(q.x); vv[1] += hi16<A>(q.x); vv[2] += lo16<A>(q.y); vv[3] += hi16<A>(q.y);
      }
      *reinterpret_cast<float4*>(Y + orow * p.ldc + c) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < p.N) {
          float o = vv[e];
          if (EPI == EPI_RESID) o = fmaf(gam[4 * ni + e], o, R[rrow * p.ldr + c + e]);
          else o += ld1(P + (long)(pp + p.pos_off) * p.ldc + c + e);
          Y[orow * p.ldc + c + e] = o;
          vv[e] = o;
        }
    }
  }
}

// Residual rows of a tile, loaded EARLY (during the last K step) for the fp32-stream RESID epilogue:
// that epilogue is a latency-bound HBM stream with only 8 waves per CU, so what sets its rate is how
// many loads are in flight and how much of their latency hides under MFMAs.  Measured on proj
// (tools/proj_probe.py): 155 us -> 135 us with all loads of the tile issued before the first store,
// -> (see profiles) with the loads issued one K step before the epilogue.
// (default cache policy on purpose: non-temporal loads / stores here cost 1-2 % of the forward - the LayerNorm
// launch that reads the stream next profits from the lines the default policy leaves in L2)
template <int MI>
struct ResidPrefetch {
  float4 r[MI][4];
  bool valid;
};
// Round 3 - the ACCESS SHAPE of this epilogue was its bottleneck (tools/pull_probe.hip: 128 KB of loads then 128 KB of stores
// per workgroup, every CU at once / 16 CUs only, cycles per tile): the accumulator layout's shape - a wave instruction = 16 rows
// x 64 bytes, four lanes per row - 14.7 k / 10.8 k; full lines - 8 rows x 128 bytes per instruction - 11.1 k / 3.6 k.  One CU
// pulls 64-byte pieces at a third of the rate of whole 128-byte lines, whatever the other CUs do.  ROWMAJOR (the persistent
// 256 x 128 tiling, which has 16 KiB of LDS to spare): residual rows are loaded, and outputs stored, 8 rows x 128 bytes at a
// time - row group mi, column half hc, instruction j: row 16 mi + 8 j + (lane >> 3), columns 32 hc + 4 (lane & 7) .. + 3 - and
// the accumulators reach that layout through a 2 KiB per-wave LDS transpose (epilogue_tile).
template <int MI>
__device__ __forceinline__ void prefetch_resid_rowmajor(const GemmParams& p, ResidPrefetch<MI>& pre, int m_base, int n0w, int lane) {
  pre.valid = false;
  if (n0w + 64 <= p.N && m_base + MI * 16 <= p.M) {     // interior tile: no guards needed
    // (opaque to loop-invariant code motion: hoisted out of the persistent tile loop, the lane's 64-bit base pointers of
    //  R and Y were two more registers live across the K loop - the fp8-weight instantiation spilled them)
    asm volatile("" : "+v"(lane));
    const float* R = reinterpret_cast<const float*>(p.R) + n0w + 4 * (lane & 7);
    // (the gathered / direct choice is hoisted over the whole block: a per-load "index or load" select makes hipcc
    //  branch around every load and wait vmcnt(0) behind each - eight serialised L2 round trips inside the K loop)
    // (element offsets as 32-bit ints: the host sends tensors of 2^31 elements or more to the 128 x 128 tiling - eight
    //  64-bit offsets held across the last K step were what made the fp8-weight instantiation spill)
    int roff[MI][2];
    if (p.ridx != nullptr) {
      int gi[MI][2];                                      // gathered-row indices first, all in flight together
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) gi[mi][j] = p.ridx[m_base + mi * 16 + j * 8 + (lane >> 3)];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int m = m_base + mi * 16 + j * 8 + (lane >> 3);
          roff[mi][j] = ((m / p.r_np) * p.r_nsrc + gi[mi][j]) * (int)p.ldr;
        }
    } else {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) roff[mi][j] = (m_base + mi * 16 + j * 8 + (lane >> 3)) * (int)p.ldr;
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        pre.r[mi][j] = *reinterpret_cast<const float4*>(R + roff[mi][j]);            // column half 0
        pre.r[mi][2 + j] = *reinterpret_cast<const float4*>(R + roff[mi][j] + 32);   // column half 1
      }
    pre.valid = true;
  }
}
template <int EPI, bool SF32, int MI>
__device__ __forceinline__ void prefetch_resid(const GemmParams& p, ResidPrefetch<MI>& pre, int m_base, int n0w,
                                               int l15, int g) {
  pre.valid = false;
  if constexpr (nat_order(EPI, SF32) && EPI == EPI_RESID && MI <= 4) {
    if (n0w + 64 <= p.N && m_base + MI * 16 <= p.M) {   // interior tile: no guards needed
      const float* R = reinterpret_cast<const float*>(p.R);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int m = m_base + mi * 16 + l15;
        long rrow = m;
        if (p.ridx != nullptr) rrow = (long)(m / p.r_np) * p.r_nsrc + p.ridx[m];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          pre.r[mi][ni] = *reinterpret_cast<const float4*>(R + rrow * p.ldr + n0w + 16 * ni + 4 * g);
      }
      pre.valid = true;
    }
  }
}

// The fewest vector stores per wave over the paths an instantiation's epilogue_tile can take for an INTERIOR tile (the
// per-path counts stand ahead of epilogue_row): NSTORE of the stream kernels.
constexpr int tile_stores(int epi, bool sf32, int mi, bool rowmajor, bool tstore) {
  if (epi == EPI_SWIGLU) return mi;                      // epilogue_tile_gated: one 16-byte store per row group
  int n = stores_acc_layout(nat_order(epi, sf32), mi);   // the path every instantiation has (no scratch, gathered rows)
  if (rowmajor && stores_rowmajor(mi) < n) n = stores_rowmajor(mi);
  if (tstore && stores_tstore(mi) < n) n = stores_tstore(mi);
  return n;
}

// Column constants of a lane on the read side of the fp32-stream transposes (ROWMAJOR, ROWMAJOR_WIDE): its 4 columns n0w + 32 hc
// + 4 cc .. of either half hc.  fp8 weights: out = resid + gamma * (acc * ws + bias); resid + (gamma * ws) * acc ... is NOT used -
// gamma * ws would round differently from the other tilings' (acc * ws) + bias, and sub-batches (128 x 128) must match bit for bit.
template <bool W8>
struct LineConsts {
  float bias[RM_HALVES][4], gam[RM_HALVES][4], wsc[RM_HALVES][W8 ? 4 : 1];
  __device__ __forceinline__ void load(const GemmParams& p, int n0w, int cc) {
#pragma unroll
    for (int hc = 0; hc < RM_HALVES; ++hc) {
      const int n = n0w + 32 * hc + 4 * cc;
      const float4 bq = p.bias != nullptr ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 gq = p.gamma != nullptr ? *reinterpret_cast<const float4*>(p.gamma + n) : make_float4(1.f, 1.f, 1.f, 1.f);
      bias[hc][0] = bq.x; bias[hc][1] = bq.y; bias[hc][2] = bq.z; bias[hc][3] = bq.w;
      gam[hc][0] = gq.x; gam[hc][1] = gq.y; gam[hc][2] = gq.z; gam[hc][3] = gq.w;
      if constexpr (W8) {
        const float4 wq = *reinterpret_cast<const float4*>(p.wscale + n);
        wsc[hc][0] = wq.x; wsc[hc][1] = wq.y; wsc[hc][2] = wq.z; wsc[hc][3] = wq.w;
      }
    }
  }
  // one float4 of outputs: accumulators a of column half hc onto the residual values r
  __device__ __forceinline__ float4 out(int hc, const f32x4& a, const float4& r) const {
    float4 o;
    o.x = fmaf(gam[hc][0], W8 ? fmaf(a[0], wsc[hc][0], bias[hc][0]) : a[0] + bias[hc][0], r.x);
    o.y = fmaf(gam[hc][1], W8 ? fmaf(a[1], wsc[hc][1], bias[hc][1]) : a[1] + bias[hc][1], r.y);
    o.z = fmaf(gam[hc][2], W8 ? fmaf(a[2], wsc[hc][2], bias[hc][2]) : a[2] + bias[hc][2], r.z);
    o.w = fmaf(gam[hc][3], W8 ? fmaf(a[3], wsc[hc][3], bias[hc][3]) : a[3] + bias[hc][3], r.w);
    return o;
  }
};

// shared tail of every 16-bit tiling: bias/gamma for this lane's columns, then one row per m-tile (A: bf16_t or f16_t,
// the format of the 16-bit outputs and of the residual stream when it is not fp32)
template <typename A, int EPI, bool SF32, int MI, bool W8 = false>
__device__ __forceinline__ void epilogue_tile(const GemmParams& p, f32x4 (&acc)[4][MI], int m_base, int n0w,
                                              int l15, int g, ResidPrefetch<MI>& pre, int m_lo = 0,
                                              bool interior = false, char* scratch = nullptr) {
  constexpr int MAP = col_map(EPI, SF32);
  constexpr bool NAT = MAP == MAP_NAT;
  if constexpr (NAT && EPI == EPI_RESID && MI <= 4) {
    if (scratch != nullptr && pre.valid) {
      // ROWMAJOR epilogue of an interior tile (see prefetch_resid_rowmajor): per row group and column half, the wave's 16 x 32
      // accumulator block goes through its 2 KiB LDS scratch, meets the residual rows loaded in that shape, and leaves as lines.
      int lane = g * 16 + l15;
      asm volatile("" : "+v"(lane));                              // (not hoisted out of the tile loop: see prefetch_resid_rowmajor)
      const int rr = lane >> 3, cc = lane & 7;                    // read-back: row rr (+ 8 j), 16-byte chunk cc of the half
      LineConsts<W8> k;
      k.load(p, n0w, cc);
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): every load so far has landed, on every path (see the note below)
      float* Y = reinterpret_cast<float*>(p.Y) + n0w + 4 * cc;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int hc = 0; hc < RM_HALVES; ++hc) {
#pragma unroll
          for (int q = 0; q < 2; ++q) lines_put(scratch, l15, 4 * q + g, __builtin_bit_cast(bf16x8, acc[2 * hc + q][mi]));   // n-tile 2 hc + q
          lines_turn();
#pragma unroll
          for (int j = 0; j < 16 / LINE_ROWS; ++j) {
            const int row = LINE_ROWS * j + rr;
            const f32x4 a = __builtin_bit_cast(f32x4, lines_get(scratch, row, cc));
            *reinterpret_cast<float4*>(Y + (long)(m_base + mi * 16 + row) * p.ldc + 32 * hc) = k.out(hc, a, pre.r[mi][2 * hc + j]);
          }
          __builtin_amdgcn_wave_barrier();
        }
      return;
    }
  }
  if constexpr (NAT && EPI == EPI_RESID && MI > 4 && !W8) {
    // the 256 x 256 tiling (fc2 where its tile count fills the rounds better; in place, no gathered rows): the same full-line
    // epilogue, one 16-row group at a time with its residual rows loaded right here (128 accumulators leave no registers
    // to prefetch them under the last K step or to run a group ahead: both forms spilled 196-392 bytes)
    if (scratch != nullptr && interior && p.ridx == nullptr) {
      int lane = g * 16 + l15;
      asm volatile("" : "+v"(lane));
      const int rr = lane >> 3, cc = lane & 7;
      LineConsts<false> k;
      k.load(p, n0w, cc);
      const float* R = reinterpret_cast<const float*>(p.R) + n0w + 4 * cc;
      float* Y = reinterpret_cast<float*>(p.Y) + n0w + 4 * cc;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        float4 r[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const long ro = (long)(m_base + mi * 16 + 8 * j + rr) * p.ldr;
          r[j] = *reinterpret_cast<const float4*>(R + ro);
          r[2 + j] = *reinterpret_cast<const float4*>(R + ro + 32);
        }
#pragma unroll
        for (int hc = 0; hc < RM_HALVES; ++hc) {
#pragma unroll
          for (int q = 0; q < 2; ++q) lines_put(scratch, l15, 4 * q + g, __builtin_bit_cast(bf16x8, acc[2 * hc + q][mi]));
          lines_turn();
#pragma unroll
          for (int j = 0; j < 16 / LINE_ROWS; ++j) {
            const int row = LINE_ROWS * j + rr;
            const f32x4 a = __builtin_bit_cast(f32x4, lines_get(scratch, row, cc));
            *reinterpret_cast<float4*>(Y + (long)(m_base + mi * 16 + row) * p.ldc + 32 * hc) = k.out(hc, a, r[2 * hc + j]);
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) on every path (see the note below)
      return;
    }
  }
  if constexpr (MAP == MAP_SEC && (EPI == EPI_BIAS || epi_act(EPI))) {
    // interior tile of a bf16-output launch (QKV, FC1 - the bulk of all tiles): no row or column guard, the
    // lane's 2 x 8 columns of bias (and fp8 scale) as four 16-byte loads, two 16-byte stores per row.  The
    // guarded general path below costs ~3x the instructions in exec-mask branches alone.
    if (interior) {
      const int ca = n0w + 8 * g, cb = ca + 32;
      float bs[16], ws[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) { bs[j] = 0.f; ws[j] = 1.f; }
      if (p.bias != nullptr) {
        load8<float>(p.bias + ca, bs);
        load8<float>(p.bias + cb, bs + 8);
      }
      if constexpr (W8) {
        load8<float>(p.wscale + ca, ws);
        load8<float>(p.wscale + cb, ws + 8);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): see the note in the general path
      A* Y = reinterpret_cast<A*>(p.Y);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {   // accumulator (ni, rg) = j>>2, j&3  ->  v[0..7] columns ca.., v[8..15] columns cb..
          const int ni = j >> 2, rg = j & 3, o = (ni >> 1) * 8 + (ni & 1) * 4 + rg;
          v[o] = W8 ? fmaf(acc[ni][mi][rg], ws[o], bs[o]) : acc[ni][mi][rg] + bs[o];
        }
        if (EPI == EPI_GELU) {
#pragma unroll
          for (int j = 0; j < 16; j += 4) {
            f32x2 a = f32x2{v[j], v[j + 1]}, b = f32x2{v[j + 2], v[j + 3]};
            gelu_pk4(a, b);
            v[j] = a[0]; v[j + 1] = a[1]; v[j + 2] = b[0]; v[j + 3] = b[1];
          }
        } else if (EPI == EPI_QGELU) {
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = quick_gelu1(v[j]);
        }
        if (scratch != nullptr) {
          // whole 128-byte lines: the wave's 16 x 64 bf16 block (one line per row) through its 2 KiB LDS scratch - written as
          // the lane's two 16-byte pieces (chunks g and 4 + g of row l15), read back 8 rows x 128 bytes per instruction
          int lane = g * 16 + l15;
          asm volatile("" : "+v"(lane));
          const int rr = lane >> 3, cc = lane & 7;
          lines_put(scratch, l15, g, __builtin_bit_cast(bf16x8, pack8<A>(v)));
          lines_put(scratch, l15, 4 + g, __builtin_bit_cast(bf16x8, pack8<A>(v + 8)));
          lines_turn();
#pragma unroll
          for (int j = 0; j < 16 / LINE_ROWS; ++j) {
            const int row = LINE_ROWS * j + rr;
            const uint4 q = __builtin_bit_cast(uint4, lines_get(scratch, row, cc));
            store_u4<RAJNI_FC1_NT && epi_act(EPI)>(Y + (long)(m_base + mi * 16 + row) * p.ldc + n0w + 8 * cc, q);
          }
          __builtin_amdgcn_wave_barrier();
        } else {
          A* row = Y + (long)(m_base + mi * 16 + l15) * p.ldc;
          static_assert(ROW_STORES_SEC == 2, "the two stores of a row below");
          store_u4<RAJNI_FC1_NT && epi_act(EPI)>(row + ca, pack8<A>(v));
          store_u4<RAJNI_FC1_NT && epi_act(EPI)>(row + cb, pack8<A>(v + 8));
        }
      }
      return;
    }
  }
  float bias[16], gam[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = out_col<MAP>(n0w, g, j);
    bias[j] = (p.bias != nullptr && n < p.N) ? p.bias[n] : 0.f;
    gam[j] = (EPI == EPI_RESID && p.gamma != nullptr && n < p.N) ? p.gamma[n] : 1.f;
  }
  float wsc[W8 ? 16 : 1];
  if constexpr (W8) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = out_col<MAP>(n0w, g, j);
      wsc[j] = n < p.N ? p.wscale[n] : 0.f;
    }
  }
  // Every vector-memory LOAD issued so far (these, and the residual rows prefetched in the last K step) has
  // landed after this explicit wait, on EVERY path - including the ones that skip all uses (a row tile
  // past M).  Without it hipcc's waitcnt pass carries "register X may still be the target of a load" back
  // into the persistent K loop, and the first reuse of X there gets an s_waitcnt vmcnt(0) that drains the
  // DMA queue in every K step (measured: -15 % on the 3-stage tiling).  It costs nothing here: the uses
  // below need the same wait, and vector-memory ops retire in order.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  // W8 dequantises inside the bias add - ONE fused multiply-add fmaf(acc, scale of W row n, bias), the same expression on every
  // epilogue path of every tiling, so that which tiling served a launch never shows in the result
  auto sb = [&](float a, int j) { return W8 ? fmaf(a, wsc[W8 ? j : 0], bias[j]) : a + bias[j]; };
  if constexpr (NAT && EPI == EPI_RESID && MI <= 4) {
    if (pre.valid) {   // interior tile whose residual rows were prefetched during the last K step
      float* Y = reinterpret_cast<float*>(p.Y);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < ROW_STORES_NAT; ++ni) {
          float4 o;
          o.x = fmaf(gam[4 * ni + 0], sb(acc[ni][mi][0], 4 * ni + 0), pre.r[mi][ni].x);
          o.y = fmaf(gam[4 * ni + 1], sb(acc[ni][mi][1], 4 * ni + 1), pre.r[mi][ni].y);
          o.z = fmaf(gam[4 * ni + 2], sb(acc[ni][mi][2], 4 * ni + 2), pre.r[mi][ni].z);
          o.w = fmaf(gam[4 * ni + 3], sb(acc[ni][mi][3], 4 * ni + 3), pre.r[mi][ni].w);
          *reinterpret_cast<float4*>(Y + (long)(m_base + mi * 16 + l15) * p.ldc + n0w + 16 * ni + 4 * g) = o;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m_base + mi * 16 + l15;
    if (m >= p.M || m < m_lo) continue;
    float v[16];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) v[ni * 4 + rg] = sb(acc[ni][mi][rg], ni * 4 + rg);
    if (NAT) epilogue_row_nat<EPI, A>(p, m, n0w, g, v, gam);
    else epilogue_row<EPI, SF32, A>(p, m, n0w + 8 * g, n0w + 32 + 8 * g, v, gam);
  }
}
// EPI_SWIGLU tail of every 16-bit tiling (see gated_w_row): hw = the wave's first hidden column; the lane's accumulators of
// n-tiles 0, 1 are the gates and of n-tiles 2, 3 the values of hidden columns hw + 8 g .. + 7.  fp8 weights dequantise inside
// the bias add with the one fmaf(acc, scale, bias) every path uses, the gate with row n's scale and the value with row N + n's.
// Stored non-temporal like FC1's GELU output (RAJNI_FC1_NT): an interior tile issues MI 16-byte stores per wave (tile_stores).
// `interior` additionally means N % 4 == 0, so that the value half of bias / w_scale is 16-byte aligned like the gate half.
template <typename A, int MI, bool W8>
__device__ __forceinline__ void epilogue_tile_gated(const GemmParams& p, f32x4 (&acc)[4][MI], int m_base, int hw,
                                                    int l15, int g, int m_lo, bool interior) {
  const int hc = hw + 8 * g;
  A* Y = reinterpret_cast<A*>(p.Y);
  float bs[16], ws[16];   // [0..7] gate, [8..15] value
#pragma unroll
  for (int j = 0; j < 16; ++j) { bs[j] = 0.f; ws[j] = 1.f; }
  if (interior) {
    if (p.bias != nullptr) {
      load8<float>(p.bias + hc, bs);
      load8<float>(p.bias + (long)p.N + hc, bs + 8);
    }
    if constexpr (W8) {
      load8<float>(p.wscale + hc, ws);
      load8<float>(p.wscale + (long)p.N + hc, ws + 8);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = hc + j < p.N;
      if (p.bias != nullptr && in) { bs[j] = p.bias[hc + j]; bs[8 + j] = p.bias[(long)p.N + hc + j]; }
      if constexpr (W8) {
        if (in) { ws[j] = p.wscale[hc + j]; ws[8 + j] = p.wscale[(long)p.N + hc + j]; }
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) on every path: see the note in epilogue_tile
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m_base + mi * 16 + l15;
    if (!interior && (m >= p.M || m < m_lo)) continue;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ni = j >> 2, rg = j & 3;
      const float gt = W8 ? fmaf(acc[ni][mi][rg], ws[j], bs[j]) : acc[ni][mi][rg] + bs[j];
      const float vl = W8 ? fmaf(acc[2 + ni][mi][rg], ws[8 + j], bs[8 + j]) : acc[2 + ni][mi][rg] + bs[8 + j];
      o[j] = silu1(gt) * vl;
    }
    A* row = Y + (long)m * p.ldc + hc;
    if (interior || hc + 8 <= p.N) {
      store_u4<RAJNI_FC1_NT>(row, pack8<A>(o));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (hc + j < p.N) st1(row + j, o[j]);
    }
  }
}

// XCD-aware tile id: blocks b and b+8 share an XCD; give each XCD a contiguous range of tiles
__device__ __forceinline__ int xcd_tile_of(int v, int total) {
  const int q = total >> 3, r = total & 7, xcd = v & 7, loc = v >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}
__device__ __forceinline__ int xcd_tile(int total) { return xcd_tile_of(blockIdx.x, total); }

// Tile order of the stream kernels.  An XCD works through a contiguous range of tile ids, its 32 CUs on 32 consecutive ones.
// With id = (row tile, column tile) column-fastest, those 32 tiles span ALL column tiles: every XCD
// streams the whole W once per round, and W (4.7 MB for FC1) does not stay in a 4 MB L2 next to the X
// panels - measured 387 MB fetched per FC1 launch for 63 MB of operands.  Instead the columns are cut
// into blocks of `nblk` column tiles and the ids run (block, row tile, column in block): an XCD stays in
// one block for many rounds (its W slice stays L2 resident), at the price of reading X once per block.
__device__ __forceinline__ void stream_tile_mn(const GemmParams& p, int tiles_m, int t, int& tm, int& tn) {
  if (p.nblk >= p.tiles_n) { tm = t / p.tiles_n; tn = t - tm * p.tiles_n; return; }
  const int per = p.nblk * tiles_m, blk = t / per, r = t - blk * per;
  const int left = p.tiles_n - blk * p.nblk, nb = left < p.nblk ? left : p.nblk;
  const int rr = r / nb;
  tm = rr; tn = blk * p.nblk + (r - rr * nb);
}

// DMA source (K offset 0, swizzled) of a lane's 16 bytes of a W staging piece: chunk `unit` of tile row `row` = global row `grow`.
// 16-bit weights: 8 rows x 128 bytes per piece (row lane >> 3, chunk lane & 7); fp8: 16 rows x 64 bytes (lane >> 2, lane & 3).
template <int MAP, bool W8>
__device__ __forceinline__ const char* w_row_src(const GemmParams& p, long grow, int row, int unit) {
  if constexpr (W8) return reinterpret_cast<const char*>(p.W) + grow * p.ldw + ((unit ^ w_key8<MAP>(row)) << 4);
  else return reinterpret_cast<const char*>(p.W) + (grow * p.ldw + (unit ^ w_key<MAP>(row)) * 8) * 2;
}

namespace wide { __device__ __forceinline__ int key_x(int row) { return (row >> 1) & 7; } }   // swizzle key of an X tile row (128-byte rows)

// Staging of the two fp8 x fp8 kernels (gemm_f8.h): rows of 128 bytes, a piece = 1 KiB = 8 rows, wave w stages X pieces XP w ..
// and W pieces PW w .. of a 256-row X tile and the BN-row W tile behind it (at X_BYTES).  One source pointer per piece and lane:
// row r_in = lane >> 3, chunk pch = lane & 7 swizzled with the row's key (key_w(row) for W).  X rows are clamped to M - 1
// (duplicates are computed but never stored); W is allocated with its rows padded to a multiple of 256.
template <int BN, int XP, int PW, typename KeyW>
__device__ __forceinline__ void byte_tile_point_at(const GemmParams& p, int tm, int tn, int wave, int r_in, int pch, KeyW key_w,
                                                   const char* (&xp)[XP], const char* (&wp)[PW]) {
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int row = (wave * XP + i) * 8 + r_in;
    int m = tm * 256 + row;
    if (m > p.M - 1) m = p.M - 1;
    xp[i] = reinterpret_cast<const char*>(p.X) + (long)m * p.lda + ((pch ^ wide::key_x(row)) << 4);
  }
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int row = (wave * PW + i) * 8 + r_in;
    wp[i] = reinterpret_cast<const char*>(p.W) + (long)(tn * BN + row) * p.ldw + ((pch ^ key_w(row)) << 4);
  }
}
// piece q of this wave (X 0 .. XP-1, then W), K byte offset k0, into the stage at dx
template <int X_BYTES, int XP, int PW>
__device__ __forceinline__ void byte_tile_dma_piece(const char* const (&xp)[XP], const char* const (&wp)[PW], int wave, int q,
                                                    int k0, char* dx) {
  if (q < XP)
    __builtin_amdgcn_global_load_lds(GLB_PTR(xp[q] + k0), LDS_PTR(dx + (wave * XP + q) * 1024), 16, 0, 0);
  else
    __builtin_amdgcn_global_load_lds(GLB_PTR(wp[q - XP] + k0), LDS_PTR(dx + X_BYTES + (wave * PW + q - XP) * 1024), 16, 0, 0);
}

// RAJNI_GEMM_STAMPS builds: the four s_memtime values of a tile (tools/gemm_stamps.py, tools/f8_stamps.py)
__device__ __forceinline__ void write_stamps(const GemmParams& p, int tile, unsigned long long t0, unsigned long long t1,
                                             unsigned long long t2, unsigned long long t3) {
  unsigned long long* o = p.stamps + (size_t)tile * 4;
  o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
}

// global source of the 16-byte chunk (row m, K offset k..) of the X operand; ET = element type
template <int ALOAD, typename ET = bf16_t>
struct XSource {
  static constexpr int CH = 16 / (int)sizeof(ET);   // elements per 16-byte chunk
  const ET* base;  // PLAIN: row pointer (+ swizzled chunk); PATCH: patch origin in the image
  int kofs;        // PATCH: this lane's k offset inside a K step
  __device__ __forceinline__ void init(const GemmParams& p, int m, int chunk) {
    const ET* X = reinterpret_cast<const ET*>(p.X);
    if (ALOAD == ALOAD_PLAIN) {
      base = X + (long)m * p.lda + chunk * CH;
      kofs = 0;
    } else {
      const int b = m / p.npatch, pp = m - b * p.npatch;
      const int py = pp / p.gw, px = pp - py * p.gw;
      base = X + ((long)b * p.cin * p.IH + (py << p.log2ps)) * p.S + (px << p.log2ps);
      kofs = chunk * CH;
    }
  }
  __device__ __forceinline__ const ET* at(const GemmParams& p, int k0) const {
    if (ALOAD == ALOAD_PLAIN) return base + k0;
    const int k = k0 + kofs, ps2 = 2 * p.log2ps;
    const int ch = k >> ps2, rem = k & ((1 << ps2) - 1);
    const int ky = rem >> p.log2ps, kx = rem & ((1 << p.log2ps) - 1);
    return base + ((long)ch * p.IH + ky) * p.S + kx;
  }
};

// =============================================================================================
// stream tilings: 256(M) x BN x 64(K), 8 waves, ONE persistent workgroup per CU that walks its tiles
// as one continuous stream of K steps.  Measured on the chip (tools/mfma_probe.hip, tools/
// gemm_stamps.py, PMC runs under profiles/): these GEMMs are bound by the bytes a CU can stage per
// second through its load path (35-50 GB/s/CU sustained), not by MFMA issue, LDS or HBM, so the
// levers are bytes per FLOP (tile size, full 128-byte lines) and how far ahead the DMA runs.
//   wide <WM=2,WN=4,MI=8,NS=2>: 256x256, wave tile 128x64, 2 stages x 64 KiB; 16 KiB staged per 2.1
//        MFLOP, DMA one step ahead.  Best for wide outputs (qkv, fc1).
//   mid  <WM=4,WN=2,MI=4,NS=3>: 256x128, wave tile 64x64, 3 stages x 48 KiB; 24 KiB per 2.1 MFLOP
//        but DMA two steps ahead and twice the tiles: for N = 768-class outputs (proj, fc2), where
//        591 tiles of 256x256 make 2.3 rounds on 256 CUs.
// K step j (stage s = j mod NS), registers holding the ks=0 fragments of step j on entry:
//   half 1: MFMAs(j,ks0)  ||  LDS reads of (j,ks1)
//   s_waitcnt lgkmcnt(0) vmcnt((NS-2)*PIECES) ; s_barrier  -> stage s is free, step j+1 has landed
//   half 2: MFMAs(j,ks1)  ||  LDS reads of (j+1,ks0)  ||  LDS-DMA of step j+NS into stage s
// The stream continues ACROSS tile boundaries (the DMA pointers switch to the next tile NS steps
// early), so the next tile's first loads fly during the epilogue.  One raw s_barrier per K step;
// every LDS read and DMA issue sits between MFMAs (sched_group_barrier pins the order).
// =============================================================================================
#define RAJNI_GEMM_NBLK_BYTES (1600 * 1024)
namespace wide {
constexpr int BM = 256, BK = 64;
constexpr int X_BYTES = BM * BK * 2;            // 32 KiB

template <int WN_, int NS_, bool W8_ = false, int NW_ = 8> struct Cfg {   // WN_ = 64-column groups of the tile
  static constexpr int BN = WN_ * 64;
  static constexpr int WB = W8_ ? 1 : 2;         // bytes per W element
  static constexpr int W_BYTES = BN * BK * WB;
  static constexpr int STAGE_BYTES = X_BYTES + W_BYTES;
  static constexpr int LDS_BYTES = NS_ * STAGE_BYTES;
  static constexpr int XP = X_BYTES / 1024 / NW_;   // X pieces (1 KiB) per wave per K step: 4 with 8 waves
  static constexpr int PW = W_BYTES / 1024 / NW_;   // W pieces per wave per K step
  static constexpr int PIECES = XP + PW;
  // W pieces 32 tile rows apart share their swizzle key (every map): one pointer per piece of the first 32 rows
  static constexpr int NPW = PW < (W8_ ? 2 : 4) ? PW : (W8_ ? 2 : 4);
};
// dynamic LDS of gemm_bf16_tn_stream<EPI, ., SF32, ., WN, MI, NS, W8>: the stages plus the eight waves' epilogue scratch
template <int EPI, bool SF32, int WN, int MI, int NS, bool W8>
constexpr int lds_bytes() { return Cfg<WN, NS, W8>::LDS_BYTES + 8 * stream_scratch_bytes(EPI, SF32, MI, W8); }

// issue order of one half step: MI groups of {NI MFMAs, 1-2 fragment reads, DMA pieces}, reads and pieces spread
// evenly over the groups (front-loading either was measured and is slower: the forward 9.03 -> 9.45 ms)
__host__ __device__ constexpr int dma_first(int g, int pieces, int groups) { return g * pieces / groups; }
__host__ __device__ constexpr int rd_first(int g, int mi, int ni) { return g + g * ni / mi; }
template <int G, int MI, bool DMA, int PIECES, int NI = 4>
__device__ __forceinline__ void sched_half() {
  if constexpr (G < MI) {
    __builtin_amdgcn_sched_group_barrier(0x008, NI, 0);
    if constexpr (rd_first(G + 1, MI, NI) - rd_first(G, MI, NI) > 0)
      __builtin_amdgcn_sched_group_barrier(0x100, rd_first(G + 1, MI, NI) - rd_first(G, MI, NI), 0);
    if constexpr (DMA) {
      constexpr int nd = dma_first(G + 1, PIECES, MI) - dma_first(G, PIECES, MI);
      if constexpr (nd > 0) __builtin_amdgcn_sched_group_barrier(0x020, nd, 0);
    }
    sched_half<G + 1, MI, DMA, PIECES, NI>();
  }
}
template <int N> __device__ __forceinline__ void wait_step() {   // lgkmcnt(0) + counted vmcnt
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(N) : "memory");
}

// Eight waves of (MI*16) x 64 outputs each.
// TAG does nothing in the body: residual launches with K <= N (the attention projection, bound by its fp32-stream
// epilogue) run an instantiation of their own so that profilers list them apart from fc2, like bench.py's classes.
template <int EPI, int ALOAD, bool SF32, int WM, int WN, int MI, int NS, bool W8 = false, int TAG = 0, typename A = bf16_t>
__global__ void __launch_bounds__(WM * WN * 64, 2) gemm_bf16_tn_stream(const GemmParams p) {
  using C = Cfg<WN, NS, W8, WM * WN>;
  constexpr int NI = 4;                        // 16-column n-tiles per wave
  using WFrag = typename WFragT<W8>::type;   // a W fragment as it sits in LDS: 8 bf16, or 8 fp8 bytes
  constexpr int MAP = col_map(EPI, SF32);      // W-row permutation = which output columns a lane owns
  constexpr bool GATED = EPI == EPI_SWIGLU;    // W rows come from two ranges (gated_w_row); a tile has BN / 2 output columns
  constexpr int BNO = GATED ? C::BN / 2 : C::BN;
  static_assert(!GATED || C::PW <= C::NPW, "the gated loader has one pointer per W piece: no fixed 32-row stride between pieces");
  static_assert(WM * WN == 8 && WM * MI * 16 == BM, "8 waves covering 256 rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // fp32-stream RESID launches (ROWMAJOR covers both weight formats on the 256 x 128 tiling; only ROWMAJOR_WIDE, on 256 x
  // 256, excludes fp8 weights) and bf16 outputs: full-line loads / stores through a 2 KiB per-wave LDS transpose behind the
  // stages - stream_scratch_bytes, which also sizes the host's dynamic LDS (lds_bytes); see prefetch_resid_rowmajor
  constexpr bool ROWMAJOR = epi_rowmajor(EPI, SF32, MI);
  constexpr int SCRATCH = stream_scratch_bytes(EPI, SF32, MI, W8);
  static_assert(lds_bytes<EPI, SF32, WN, MI, NS, W8>() <= LDS_MAX_BYTES, "stages + epilogue scratch exceed the workgroup's LDS");

  // ---- staging: a piece = 1 KiB = 8 rows x 128 B; wave w stages X pieces 4w..4w+3, W pieces PW*w..
  //      (fp8 W: a piece = 16 rows x 64 B, lane -> row lane>>2, 16-byte unit lane&3)
  // NOTE on addressing: the DMA takes a 64-bit per-lane pointer (global_load_lds ... off); scalar base +
  // 32-bit lane offset and buffer_load ... lds were built and measured, neither is faster.
  // Register diet (the RESID instantiations are register bound, and a spilled lane constant is reloaded
  // behind an s_waitcnt vmcnt(0) that drains the DMA queue):
  //   * a ragged last row tile starts at M - 256 instead of clamping its rows (the rows it shares with the
  //     previous tile are recomputed and masked in the epilogue), so every tile's rows are evenly spaced:
  //     X needs TWO pointers per lane (pieces 0/2 and 1/3 differ by 16 rows = a scalar), and
  //   * going to the next tile is `pointer += scalar delta` - no second pointer set, nothing for the
  //     compiler to hoist (it used to precompute the next tile's 6 pointers at the start of every tile).
  auto tile_m0 = [&](int tm_) { return tm_ * BM + BM > p.M ? p.M - BM : tm_ * BM; };   // host: M >= 256
  const int tiles_m = p.total_tiles / p.tiles_n;
  auto tile_mn = [&](int t, int& tm_, int& tn_) { stream_tile_mn(p, tiles_m, t, tm_, tn_); };
  XSource<ALOAD> xs[ALOAD == ALOAD_PLAIN ? 1 : C::XP];   // fused im2col loader: one source per piece
  const char* xp[2];                                 // plain loader: even and odd pieces (16 rows apart each)
  const char* ws[C::NPW];
  auto point_at = [&](int tile) {   // DMA source pointers of a tile
    int tm, tn;
    tile_mn(tile, tm, tn);
    const int r_in = lane >> 3, pch = lane & 7;
    if constexpr (ALOAD == ALOAD_PLAIN) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (wave * C::XP + i) * 8 + r_in;     // key_x(row + 16) == key_x(row)
        xp[i] = reinterpret_cast<const char*>(p.X) + ((long)(tile_m0(tm) + row) * p.lda + (pch ^ key_x(row)) * 8) * 2;
      }
    } else {
#pragma unroll
      for (int i = 0; i < C::XP; ++i) {
        const int row = (wave * C::XP + i) * 8 + r_in;
        int m = tm * BM + row;
        if (m > p.M - 1) m = p.M - 1;  // clamp: duplicates are computed but never stored
        xs[i].init(p, m, pch ^ key_x(row));
      }
    }
#pragma unroll
    for (int i = 0; i < C::NPW; ++i) {
      const int row = W8 ? (wave * C::PW + i) * 16 + (lane >> 2) : (wave * C::PW + i) * 8 + r_in;
      const long grow = GATED ? gated_w_row<false>(row, p.N, tn * BNO) : (long)(tn * C::BN + row);
      ws[i] = w_row_src<MAP, W8>(p, grow, row, W8 ? lane & 3 : pch);
    }
  };
  auto advance = [&](int from, int to) {   // retarget the DMA from tile `from` to tile `to`
    if constexpr (ALOAD == ALOAD_PLAIN) {
      int tm0, tn0, tm1, tn1;
      tile_mn(from, tm0, tn0);
      tile_mn(to, tm1, tn1);
      const long dx = (long)(tile_m0(tm1) - tile_m0(tm0)) * p.lda * 2;
      const long dw = (long)(tn1 - tn0) * BNO * p.ldw * C::WB;   // gated: both row ranges move by the tile's BN / 2 hidden columns
      xp[0] += dx; xp[1] += dx;
#pragma unroll
      for (int i = 0; i < C::NPW; ++i) ws[i] += dw;
    } else {
      point_at(to);
    }
  };
  auto dma_piece = [&](int q, int k0, char* dx) {   // piece q of this wave: X 0..3 then W 0..PW-1
    if (q < C::XP) {
      if constexpr (ALOAD == ALOAD_PLAIN)
        __builtin_amdgcn_global_load_lds(GLB_PTR(xp[q & 1] + ((long)(q >> 1) * 16 * p.lda + k0) * 2),
                                         LDS_PTR(dx + (wave * C::XP + q) * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds(GLB_PTR(xs[q].at(p, k0)), LDS_PTR(dx + (wave * C::XP + q) * 1024), 16, 0, 0);
    } else {
      const int i = q - C::XP;   // W piece i: pointer i % NPW, (i / NPW) * 32 tile rows further down
      if constexpr (C::PW <= C::NPW)
        __builtin_amdgcn_global_load_lds(GLB_PTR(ws[i] + k0 * C::WB), LDS_PTR(dx + X_BYTES + (wave * C::PW + i) * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds(GLB_PTR(ws[i % C::NPW] + ((long)(i / C::NPW) * 32 * p.ldw + k0) * C::WB),
                                         LDS_PTR(dx + X_BYTES + (wave * C::PW + i) * 1024), 16, 0, 0);
    }
  };
  auto stage = [&](int kt, int st) {
#pragma unroll
    for (int q = 0; q < C::PIECES; ++q) dma_piece(q, kt * BK, smem + st * C::STAGE_BYTES);
  };

  // ---- fragment addresses: rows base + (lane&15) have key (lane&15)>>1 for every mi, the permuted
  //      W rows have one key for every ni, so each (operand, ks) needs ONE address + immediates
  const int wm = wave / WN, wn = wave % WN;
  const int l15 = lane & 15, g = lane >> 4;
  const int xr0 = wm * (MI * 16) + l15;
  const int wr0 = wn * 64 + w_frag_row<MAP>(l15, 0);
  // byte offset of n-tile ni's W rows from n-tile 0's (lane independent; the swizzle key is the same)
  auto w_ni_off = [](int ni) { return (w_frag_row<MAP>(0, ni) - w_frag_row<MAP>(0, 0)) * (64 * C::WB); };
  int xo[2], wo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    xo[ks] = xr0 * 128 + (((ks * 4 + g) ^ key_x(xr0)) << 4);
    if constexpr (W8)   // 8-byte fragment ks*4+g = half (g&1) of 16-byte unit (ks*4+g)>>1
      wo[ks] = X_BYTES + wr0 * 64 + ((((ks * 4 + g) >> 1) ^ w_key8<MAP>(wr0)) << 4) + ((g & 1) << 3);
    else
      wo[ks] = X_BYTES + wr0 * 128 + (((ks * 4 + g) ^ w_key<MAP>(wr0)) << 4);
  }

  f32x4 acc[4][MI];  // [ni][mi]

  // one half step: MFMAs on (xc,wc) || fragments (stage rst, sub-step rks) -> (xn,wn_), xn[mi] issued
  // right after the group that consumed xc[mi] || if DMA: K-tile dkt of the pointed-at tile -> stage dst
  auto half = [&](auto dma_c, auto read_c, bf16x8 (&xc)[MI], WFrag (&wc)[NI], bf16x8 (&xn)[MI], WFrag (&wn_)[NI],
                  int rst, int rks, int dkt, int dst) {
    constexpr bool DMA = decltype(dma_c)::value;
    constexpr bool READ = decltype(read_c)::value;
    const char* sb = smem + rst * C::STAGE_BYTES;
    char* dx = smem + dst * C::STAGE_BYTES;
    const int k0 = dkt * BK;
    bf16x8 wv[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) wv[ni] = w_frag_bf16(wc[ni]);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        acc[ni][mi] = mfma_16x16x32<A>(wv[ni], xc[mi], acc[ni][mi]);
      if constexpr (READ) {
        xn[mi] = *reinterpret_cast<const bf16x8*>(sb + xo[rks] + mi * 2048);
#pragma unroll
        for (int wi = mi * NI / MI; wi < (mi + 1) * NI / MI; ++wi)
          wn_[wi] = *reinterpret_cast<const WFrag*>(sb + wo[rks] + w_ni_off(wi));
      }
      if constexpr (DMA) {
#pragma unroll
        for (int q = dma_first(mi, C::PIECES, MI); q < dma_first(mi + 1, C::PIECES, MI); ++q) dma_piece(q, k0, dx);
      }
    }
    if constexpr (READ) sched_half<0, MI, DMA, C::PIECES, NI>();
  };
  using T = std::true_type; using F = std::false_type;
  const int nk = p.K / BK;        // >= NS + 1 (host checked)
  int v = blockIdx.x;
  int tile = xcd_tile_of(v, p.total_tiles);
  bf16x8 xa[MI], xb[MI];
  WFrag wa[NI], wb[NI];
  if constexpr (EPI == EPI_RESID) {
    if (p.stagger > 0 && ((blockIdx.x >> 3) & 1))
      for (int i = 0; i < p.stagger; ++i) __builtin_amdgcn_s_sleep(127);
  }

  constexpr int WBASE = (NS - 2) * C::PIECES;
  auto interior = [&](int t) {   // a tile whose 256 rows and BN columns all exist
    int tm_, tn_;
    tile_mn(t, tm_, tn_);
    if constexpr (GATED) return tm_ * BM + BM <= p.M && tn_ * BNO + BNO <= p.N && (p.N & 3) == 0;   // see epilogue_tile_gated
    return tm_ * BM + BM <= p.M && tn_ * C::BN + C::BN <= p.N;
  };
  ResidPrefetch<MI> pre;
  point_at(tile);
#pragma unroll
  for (int j = 0; j < NS; ++j) stage(j, j);
  wait_step<((NS - 1) * C::PIECES > 8) ? 0 : (NS - 1) * C::PIECES>();   // step 0 landed (NS=3: drain all)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < NI; ++i) wa[i] = *reinterpret_cast<const WFrag*>(smem + wo[0] + w_ni_off(i));
#pragma unroll
  for (int i = 0; i < MI; ++i) xa[i] = *reinterpret_cast<const bf16x8*>(smem + xo[0] + i * 2048);
  int st = 0;  // LDS stage of the current K step
  // Output stores of a tile are still in flight when the next tile's K loop starts.  gfx9 counts stores in
  // vmcnt as well and retires vector-memory ops in order, so the first counted wait of a tile may leave
  // exactly the epilogue's stores outstanding instead of waiting for them to reach L2: an interior tile's
  // epilogue issues NSTORE stores per wave after the DMA of K step 1 (a lower bound is all that is needed).
  constexpr int NSTORE_ALL = tile_stores(EPI, SF32, MI, ROWMAJOR || epi_rowmajor_wide(EPI, SF32, MI, W8), epi_tstore(EPI));
  constexpr int NSTORE = NSTORE_ALL < 48 ? NSTORE_ALL : 48;   // vmcnt is a 6-bit counter
  bool prev_full = false;          // the previous tile of this workgroup was interior

  while (true) {
#ifdef RAJNI_GEMM_STAMPS
    const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
    int tm, tn;
    tile_mn(tile, tm, tn);
    const int m0 = ALOAD == ALOAD_PLAIN ? tile_m0(tm) : tm * BM, n0 = tn * C::BN;
    const int m_lo = tm * BM;            // rows below it belong to the previous tile (ragged last tile only)
    const bool inter = interior(tile);
    const int vn = v + gridDim.x;
    const bool more = vn < p.total_tiles;
    pre.valid = false;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < MI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto kstep = [&](int kt) {   // one K step
      // the DMA of step kt loads K-tile kt+NS; from kt = nk-NS on that is the NEXT tile's K-tile
      // 0.. (when there is no next tile the pointers stay put: harmless re-loads nobody reads)
      if (kt == nk - NS && more) advance(tile, xcd_tile_of(vn, p.total_tiles));
      const int dkt = kt + NS < nk ? kt + NS : kt + NS - nk;
      const int st1 = st + 1 == NS ? 0 : st + 1;
      if (kt == nk - 1 && inter) {
        if constexpr (ROWMAJOR) prefetch_resid_rowmajor<MI>(p, pre, m0 + wm * (MI * 16), n0 + wn * 64, lane);
        else prefetch_resid<EPI, SF32, MI>(p, pre, m0 + wm * (MI * 16), n0 + wn * 64, l15, g);
      }
      half(F{}, T{}, xa, wa, xb, wb, st, 1, 0, 0);
      // my reads of stage st are done and my DMA pieces of step kt+1 have landed ...
      if (NSTORE > 0 && kt == 0 && prev_full) wait_step<WBASE + NSTORE>();
      else wait_step<WBASE>();
      __builtin_amdgcn_s_barrier();   // ... and everyone else's: stage st is free, stage st1 readable
      asm volatile("" ::: "memory");
      half(T{}, T{}, xb, wb, xa, wa, st1, 0, dkt, st);
      st = st1;
    };
    for (int kt = 0; kt < nk; ++kt) kstep(kt);
#ifdef RAJNI_GEMM_STAMPS
    asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[3][MI - 1][3]));
    const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
#endif

    // ---- epilogue (the next tile's first loads are in flight)
    if constexpr (GATED)
      epilogue_tile_gated<A, MI, W8>(p, acc, m0 + wm * (MI * 16), tn * BNO + wn * 32, l15, g, m_lo, inter);
    else
      epilogue_tile<A, EPI, SF32, MI, W8>(p, acc, m0 + wm * (MI * 16), n0 + wn * 64, l15, g, pre, m_lo, inter,
                                       SCRATCH > 0 ? smem + C::LDS_BYTES + wave * SCRATCH : nullptr);
#ifdef RAJNI_GEMM_STAMPS
    if (p.stamps != nullptr && wave == 0) {
      const unsigned long long ts3 = __builtin_amdgcn_s_memtime();
      if (lane == 0) write_stamps(p, tile, ts0, ts0, ts2, ts3);
    }
#endif
    prev_full = inter;
    if (!more) break;
    v = vn;
    tile = xcd_tile_of(v, p.total_tiles);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the trailing (unused) DMA before LDS is released
}
}  // namespace wide

// =============================================================================================
// small tiling: 128 x 128 x 64, 2 stages
// =============================================================================================
namespace small {
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;        // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;    // X + W
constexpr int LDS_BYTES = 2 * STAGE_BYTES;     // double buffered: 64 KiB
// 128-byte rows: slot = (row&1)*8 + (chunk ^ key)
__device__ __forceinline__ int key_x(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int key_w(int row) { return ((row >> 4) & 3) * 2 + ((row >> 1) & 1); }

template <int EPI, int ALOAD, bool SF32, bool W8 = false, typename A = bf16_t>
__global__ void __launch_bounds__(256, 2) gemm_bf16_tn_128x128(const GemmParams p) {
  constexpr int MAP = col_map(EPI, SF32);      // W-row permutation = which output columns a lane owns
  constexpr int PW = W8 ? 2 : 4;               // W pieces per wave per K step (fp8 tile is 8 KiB)
  constexpr bool GATED = EPI == EPI_SWIGLU;    // W rows come from two ranges (gated_w_row); a tile has BN / 2 output columns
  using WFrag = typename WFragT<W8>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = xcd_tile(p.total_tiles);
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- staging: wave w stages pieces 4w..4w+3 of each operand; a piece = 8 rows x 128 B
  const int r_in = lane >> 3, pch = lane & 7;
  XSource<ALOAD> xs[4];
  const char* ws[PW];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + r_in;
    int m = m0 + row;
    if (m > p.M - 1) m = p.M - 1;
    xs[i].init(p, m, pch ^ key_x(row));
  }
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int row = W8 ? (wave * PW + i) * 16 + (lane >> 2) : (wave * PW + i) * 8 + r_in;
    const long grow = GATED ? gated_w_row<false>(row, p.N, tn * (BN / 2)) : (long)(n0 + row);
    ws[i] = w_row_src<MAP, W8>(p, grow, row, W8 ? lane & 3 : pch);
  }
  auto stage = [&](int kt, int buf) {
    char* sx = smem + buf * STAGE_BYTES;
    char* sw = sx + TILE_BYTES;
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(xs[i].at(p, k0)), LDS_PTR(sx + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < PW; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(ws[i] + k0 * (W8 ? 1 : 2)), LDS_PTR(sw + (wave * PW + i) * 1024), 16, 0, 0);
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  int xoff[4], xkey[4], woff[4], wkey[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xr = wm * 64 + i * 16 + l15;
    xoff[i] = xr * 128; xkey[i] = key_x(xr);
    const int wr = wn * 64 + w_frag_row<MAP>(l15, i);
    woff[i] = wr * (W8 ? 64 : 128); wkey[i] = W8 ? w_key8<MAP>(wr) : w_key<MAP>(wr);
  }

  f32x4 acc[4][4];  // [ni][mi]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  ResidPrefetch<4> pre;
  pre.valid = false;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt has landed for every wave; everyone is done reading the other buffer
    if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
    else prefetch_resid<EPI, SF32, 4>(p, pre, m0 + wm * 64, n0 + wn * 64, l15, g);   // lands under the last MFMAs
    const char* sx = smem + (kt & 1) * STAGE_BYTES;
    const char* sw = sx + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + g;
      bf16x8 xf[4], wf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xf[i] = *reinterpret_cast<const bf16x8*>(sx + xoff[i] + ((c ^ xkey[i]) << 4));
        if constexpr (W8)
          wf[i] = w_frag_bf16(*reinterpret_cast<const WFrag*>(sw + woff[i] + (((c >> 1) ^ wkey[i]) << 4) + ((c & 1) << 3)));
        else
          wf[i] = *reinterpret_cast<const bf16x8*>(sw + woff[i] + ((c ^ wkey[i]) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          acc[ni][mi] = mfma_16x16x32<A>(wf[ni], xf[mi], acc[ni][mi]);
    }
  }

  if constexpr (GATED) epilogue_tile_gated<A, 4, W8>(p, acc, m0 + wm * 64, tn * (BN / 2) + wn * 32, l15, g, 0, false);
  else epilogue_tile<A, EPI, SF32, 4, W8>(p, acc, m0 + wm * 64, n0 + wn * 64, l15, g, pre);
}
}  // namespace small

#include "gemm_f8.h"   // namespace f8: the fp8 x fp8 persistent kernel (v_mfma_f32_16x16x128_f8f6f4)

// =============================================================================================
// fp32 model path: 128 x 128 x 32(fp32) tile - byte-for-byte the LDS geometry of the small bf16
// tiling (128-byte rows, same swizzle keys, same LDS-DMA staging) - with v_mfma_f32_16x16x4_f32
// (exact fp32 FMA chain, 1/16 of the bf16 rate).  A lane reads 16 bytes = 4 consecutive k of its
// row for BOTH operands and feeds them to 4 MFMAs, element t of every lane group g covering
// k = 4*(4*ks+g)+t: the k order inside a K step is permuted identically for X and W, so the sum is
// the same.  All tensors (x, w, resid, pos, y) are fp32.
// =============================================================================================
namespace f32 {
constexpr int BM = 128, BN = 128, BK = 32;
constexpr int TILE_BYTES = BM * BK * 4;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;
using small::key_w;
using small::key_x;

template <int EPI>
__device__ __forceinline__ void epilogue_row_f32(const GemmParams& p, int m, int nb, float* v, const float* gam) {
  long orow = m;
  if (EPI == EPI_GELU) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = 0.5f * v[j] * (1.0f + erff(v[j] * 0.70710678118654752f));
  } else if (EPI == EPI_QGELU) {   // accurate expf and a true division; expf -> +inf for large -v: v / inf = -0, never NaN
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = v[j] / (1.0f + expf(-1.702f * v[j]));
  } else if (EPI == EPI_RESID) {
    long rrow = m;
    if (p.ridx != nullptr) {
      const int b = m / p.r_np;
      rrow = (long)b * p.r_nsrc + p.ridx[m];
    }
    const long roff = rrow * p.ldr + nb;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (nb + j < p.N) v[j] = fmaf(gam[j], v[j], reinterpret_cast<const float*>(p.R)[roff + j]);
  } else if (EPI == EPI_PATCH) {
    const int b = m / p.npatch, pp = m - b * p.npatch;
    orow = (long)b * (p.npatch + p.nprefix) + p.nprefix + pp;
    const float* pr = reinterpret_cast<const float*>(p.pos) + (long)(pp + p.pos_off) * p.ldc + nb;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (nb + j < p.N) v[j] += pr[j];
  }
  const long yoff = orow * p.ldc + nb;
  if (nb + 16 <= p.N) {
    store16<true, bf16_t>(p.Y, yoff, v);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (nb + j < p.N) reinterpret_cast<float*>(p.Y)[yoff + j] = v[j];
  }
}

template <int EPI, int ALOAD>
__global__ void __launch_bounds__(256, 2) gemm_f32_tn_128x128(const GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = xcd_tile(p.total_tiles);
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const float* W = reinterpret_cast<const float*>(p.W);

  const int r_in = lane >> 3, pch = lane & 7;
  XSource<ALOAD, float> xs[4];
  const float* ws[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + r_in;
    int m = m0 + row;
    if (m > p.M - 1) m = p.M - 1;
    xs[i].init(p, m, pch ^ key_x(row));
    const long grow = EPI == EPI_SWIGLU ? gated_w_row<true>(row, p.N, tn * (BN / 2)) : (long)(n0 + row);
    ws[i] = W + grow * p.ldw + (pch ^ key_w(row)) * 4;
  }
  auto stage = [&](int kt, int buf) {
    char* sx = smem + buf * STAGE_BYTES;
    char* sw = sx + TILE_BYTES;
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(xs[i].at(p, k0)), LDS_PTR(sx + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(ws[i] + k0), LDS_PTR(sw + (wave * 4 + i) * 1024), 16, 0, 0);
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  int xoff[4], xkey[4], woff[4], wkey[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xr = wm * 64 + i * 16 + l15;
    xoff[i] = xr * 128; xkey[i] = key_x(xr);
    const int wr = wn * 64 + 16 * (l15 >> 2) + i * 4 + (l15 & 3);
    woff[i] = wr * 128; wkey[i] = key_w(wr);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
    const char* sx = smem + (kt & 1) * STAGE_BYTES;
    const char* sw = sx + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + g;
      f32x4 xf[4], wf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xf[i] = *reinterpret_cast<const f32x4*>(sx + xoff[i] + ((c ^ xkey[i]) << 4));
        wf[i] = *reinterpret_cast<const f32x4*>(sw + woff[i] + ((c ^ wkey[i]) << 4));
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ni][tt], xf[mi][tt], acc[ni][mi], 0, 0, 0);
    }
  }

  if constexpr (EPI == EPI_SWIGLU) {
    // the lane's tile columns 16 g .. + 7 are the gates and 16 g + 8 .. + 15 the values of hidden columns hc .. hc + 7
    // (gated_w_row<true>).  This kernel's GELU rule: accurate expf and a true division; expf -> +inf for large -g gives
    // g / inf = -0, and -0 * v = +-0 for finite v - never NaN
    const int hc = tn * (BN / 2) + wn * 32 + 8 * g;
    float bg[8], bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = p.bias != nullptr && hc + j < p.N;
      bg[j] = in ? p.bias[hc + j] : 0.f;
      bv[j] = in ? p.bias[(long)p.N + hc + j] : 0.f;
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = m0 + wm * 64 + mi * 16 + l15;
      if (m >= p.M) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gt = acc[j >> 2][mi][j & 3] + bg[j], vl = acc[2 + (j >> 2)][mi][j & 3] + bv[j];
        o[j] = gt / (1.0f + expf(-gt)) * vl;
      }
      float* yr = reinterpret_cast<float*>(p.Y) + (long)m * p.ldc + hc;
      if (hc + 8 <= p.N) {
        store8<float>(yr, o);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (hc + j < p.N) yr[j] = o[j];
      }
    }
    return;
  }
  const int nb = n0 + wn * 64 + 16 * g;
  float bias[16], gam[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = nb + j;
    bias[j] = (p.bias != nullptr && n < p.N) ? p.bias[n] : 0.f;
    gam[j] = (EPI == EPI_RESID && p.gamma != nullptr && n < p.N) ? p.gamma[n] : 1.f;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + wm * 64 + mi * 16 + l15;
    if (m >= p.M) continue;
    float v[16];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) v[ni * 4 + rg] = acc[ni][mi][rg] + bias[ni * 4 + rg];
    epilogue_row_f32<EPI>(p, m, nb, v, gam);
  }
}

}  // namespace f32

// x[b,0,:] = cls + pos[0]  (or cls alone when pos has no CLS row)
template <bool SF32, typename T>
__global__ void cls_pos_kernel(const T* cls, const T* pos, int pos_has_cls, void* x,
                               long img_stride, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  float v = ld1(cls + c);
  if (pos_has_cls) v += ld1(pos + c);
  store1<SF32, T>(x, (long)b * img_stride + c, v);
}

// x[b,r,:] = prefix[r] + pos[r] for the P prefix rows of image b (row 0 = cls, rows 1..P-1 = the register tokens; the
// prefix row alone when pos has no prefix rows).  One thread = 8 consecutive channels: one 16-byte store into a 16-bit
// stream, two into the fp32 one, a wave a run of whole lines.  (P = 1 keeps cls_pos_kernel: the same launches as ever.)
template <bool SF32, typename T>
__global__ void __launch_bounds__(256) prefix_pos_kernel(const T* cls, const T* reg, const T* pos, int pos_has_prefix, void* x,
                                                         long img_stride, int B, int P, int C) {
  const int c8 = C >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * P * c8) return;
  const int br = i / c8, c = (i - br * c8) * 8;
  const int b = br / P, r = br - b * P;
  float v[8];
  load8<T>((r == 0 ? cls : reg + (long)(r - 1) * C) + c, v);
  if (pos_has_prefix) {
    float pf[8];
    load8<T>(pos + (long)r * C + c, pf);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += pf[j];
  }
  const long off = (long)b * img_stride + (long)r * C + c;
  if constexpr (SF32) store8<float>(reinterpret_cast<float*>(x) + off, v);
  else store8<T>(reinterpret_cast<T*>(x) + off, v);
}

// ---- host side: choose a tiling (pure functions of the shape, the CU count, the instantiation's traits and the hooks),
//      then launch it
// LDS stages of the wide tiling: 2 for bf16 weights (2 x 64 KiB); fp8 weights leave room for 3 (3 x 48 KiB)
#ifndef RAJNI_W8_WIDE_NS
#define RAJNI_W8_WIDE_NS 2
#endif
#define RAJNI_W8_WIDE_NS_OR(w8) ((w8) ? RAJNI_W8_WIDE_NS : 2)
// test / tuning hooks (include/rajni_hip_debug.h): process-global, unsynchronised - not for concurrent use
int g_force_tiling = 0;  // 0 auto, 1 small (128x128x64, 2 stages), 4 wide 256x256x64, 5 mid 256x128x64 (tests)
int g_force_f8_tiling = 0;   // test hook: 0 by shape, 1 = 256 x 128 always, 2 = 256 x 256 wherever it exists
int g_nblk_bytes = RAJNI_GEMM_NBLK_BYTES;   // W bytes of one N block (0 = plain order, < 0 = forced block size: tuning)

// column tiles per N block of the persistent tile order (see tile_mn).  Measured on the ViT-B shapes
// (tools/nblk_bench.py): blocks of ~1.5 MiB of W help once every block spans at least two rounds of tiles
// (QKV at 197 tokens 179 -> 161 us, FC1 254 -> 239 us); with fewer rounds W is not re-read often enough
// to pay for reading X once per block, and K = 3072 (fc2) never pays.
inline int n_block(int tiles_n, int tiles_m, int bn, int K, int wbytes, int cus, int nblk_bytes) {
  if (nblk_bytes < 0) return -nblk_bytes < tiles_n ? -nblk_bytes : tiles_n;
  if (nblk_bytes == 0) return tiles_n;
  const long per_tile = (long)bn * K * wbytes;
  const int fit = (int)(nblk_bytes / per_tile);
  if (fit < 1 || fit >= tiles_n) return tiles_n;
  const int blocks = (tiles_n + fit - 1) / fit;
  const int rounds = tiles_n * tiles_m / cus;
  if (rounds < 2 * blocks) return tiles_n;
  return (tiles_n + blocks - 1) / blocks;
}

// N = 768-class outputs with a long K (fc2): 256x128 tiles are the default, but when the tile count of the
// 256x256 tiling happens to fill its rounds much better, it wins by 6-20 % (tools/fc2_grid_probe.py: 19 of 19
// shapes of ViT-B / ViT-L / ViT-H at batch 64-512 picked right; fc2 at 152 tokens 226 -> 212 us, at batch 512
// 660 -> 537 us).  Cost model: full rounds of 256 tiles plus a partial round whose tiles run faster the emptier
// the chip is (board power cap: DESIGN.md section 4 (10)); one 256x256 round = 1.83 256x128 rounds.  Not used for
// K <= N (proj): there the epilogue dominates a tile and the ratio is larger (measured: 4 misses of 11).
inline double eff_rounds(long tiles, int cus) {
  const long full = tiles / cus;
  const double frac = (double)tiles / (double)cus - (double)full;
  return (double)full + (frac > 0.0 ? 0.6 + 0.4 * frac : 0.0);
}
inline bool wide_wins_on_rounds(int M, int N, int cus) {
  const long rows = (M + 255) / 256;
  return 1.83 * eff_rounds(rows * ((N + 255) / 256), cus) < eff_rounds(rows * ((N + 127) / 128), cus);
}

// persistent grid: one workgroup per CU of the device the launch goes to (hipDeviceProp_t::multiProcessorCount;
// 256 on MI355X).  A grid balanced to whole rounds, as hipBLASLt picks for fc2, was measured: 0.7 % slower over
// the 20 GEMM shapes of the schedule.
inline int stream_grid(int total_tiles, int cus) { return rajni_persistent_grid(total_tiles <= cus ? total_tiles : cus); }

// what a choice needs to know of the instantiations behind a launch
struct TileTraits {
  int epi;
  bool resid_nat;             // fp32-stream RESID: the 256 x 128 tiling's epilogue addresses the residual with 32-bit offsets
  int lds_wide, lds_narrow;   // dynamic LDS of the 256 x 256 / 256 x 128 kernel (lds_wide = 0: there is no 256 x 256 kernel)
};
// tiles of bm x bn.  bm = 256: a persistent stream (grid <= cus) whose tile order runs in N blocks of W, wbytes per element;
// otherwise one workgroup per tile in the plain order.  A gated launch (EPI_SWIGLU) computes [M, K] x [2N, K]^T: a tile
// still stages bn rows of W - which is what the N blocks are sized by - but covers bn / 2 of the N output columns
rajni_linear_plan make_plan(const GemmParams& p, int tiling, int bm, int bn, int lds, int cus = 0, int wbytes = 0, int nblk_bytes = 0,
                            bool gated = false) {
  const int tiles_m = (p.M + bm - 1) / bm;
  const int bno = gated ? bn / 2 : bn;
  rajni_linear_plan c{};
  c.tiling = tiling; c.lds_bytes = lds;
  c.tiles_n = (p.N + bno - 1) / bno;
  c.grid = c.total_tiles = c.tiles_n * tiles_m;
  if (bm == 256) {
    c.nblk = n_block(c.tiles_n, tiles_m, bn, p.K, wbytes, cus, nblk_bytes);
    c.grid = stream_grid(c.total_tiles, cus);
  }
  return c;
}

// 16-bit activations (wide / mid / small); `force` = rajni_debug_force_gemm_tiling
rajni_linear_plan choose_gemm(const GemmParams& p, const TileTraits& r, int cus, int force, int nblk_bytes) {
  int mode = force;
  // the shape rule sees the GEMM that is computed: a gated launch has 2N columns of W
  const bool gated = r.epi == EPI_SWIGLU;
  const int wn = gated ? 2 * p.N : p.N;
  if ((mode == 4 || mode == 5) && p.M < 256) mode = 1;   // stream tiles may start at M - 256
  if (mode == 4 && p.K < 192) mode = 1;                   // the persistent streams need >= NS + 1 K steps
  if (mode == 5 && p.K < 256) mode = 1;
  // the 256 x 128 tiling's full-line residual epilogue addresses the residual tensor with 32-bit element offsets
  const long resid_rows = p.ridx != nullptr ? (long)(p.M / p.r_np) * p.r_nsrc : (long)p.M;
  const bool mid_ok = !r.resid_nat || resid_rows * p.ldr < (1L << 31);
  if (mode == 5 && !mid_ok) mode = 1;
  if (mode == 0) {
    // measured on ViT-B shapes (tools/gemm_bench.py, tools/proj_probe.py, profiles/):
    //   wide outputs (qkv, fc1): persistent 256x256 (950 / 870 TFLOP/s vs 750 / 700 for 128x128);
    //   N = 768-class outputs (proj, fc2): 591 tiles of 256x256 make 2.3 rounds on 256 CUs, the
    //   persistent 256x128 3-stage tiling is best (proj 125 us, fc2 284 us vs 127 / 310 for 128x128);
    //   small problems (head, tiny batches): 128x128.
    if (p.M >= 1024 && wn >= 1536 && p.K >= 192) mode = 4;
    else if (p.M >= 1024 && p.K >= 256) mode = (p.K > wn && p.K >= 1536 && wide_wins_on_rounds(p.M, wn, cus)) ? 4 : (mid_ok ? 5 : 1);
    else mode = 1;
  }
  // W blocks of the tile order: fp8 W gets the same blocks as bf16 (measured), hence 2 bytes per element
  if (mode == 4) return make_plan(p, RAJNI_TILING_WIDE, 256, 256, r.lds_wide, cus, 2, nblk_bytes, gated);
  if (mode == 5) return make_plan(p, RAJNI_TILING_MID, 256, 128, r.lds_narrow, cus, 2, nblk_bytes, gated);
  return make_plan(p, RAJNI_TILING_SMALL, 128, 128, small::LDS_BYTES, 0, 0, 0, gated);
}

// fp8 x fp8 (gemm_f8.h), persistent: 256 x 256 for wide outputs without a residual epilogue (QKV, FC1), 256 x 128
// otherwise (FC2, small problems); `force` = rajni_debug_force_f8_tiling
rajni_linear_plan choose_gemm_f8(const GemmParams& p, const TileTraits& r, int cus, int force, int nblk_bytes) {
  if (r.lds_wide != 0) {   // EPI_BIAS, EPI_GELU8
    const bool wide_ok = p.K >= 384;
    // measured on ViT-B at batch 256 (K = 768: 6 K steps per tile, so per-tile costs weigh double against the bf16
    // tilings): FC1 + GELU -> e4m3 132 us on 256 x 256 vs 139 us on 256 x 128.  QKV -> bf16: 256 x 256 since its
    // epilogue stores whole lines (tools/f8_qkv_tiling.py, us at 197 / 173 / 152 / 121 / 87 tokens: 120.5 / 118.8 / 93.7 /
    // 74.3 / 61.6 against 128.1 / 102.0 / 103.4 / 78.6 / 60.8 on 256 x 128; batch 512: 264.5 / 234.4 / 205.6 / 150.0 /
    // 112.3 against 288.3 / 251.6 / 220.1 / 155.8 / 100.4) - except where its tiles end just past a whole number of
    // rounds in a short launch (6.08 and 6.12 rounds above: the nearly empty last round costs 12-16 %)
    auto rounds_ok = [&]() {
      const double rounds = (double)((p.M + 255) / 256) * ((p.N + f8w::BN - 1) / f8w::BN) / cus;
      const double frac = rounds - (long)rounds;
      return !(rounds < 8.0 && frac > 0.0 && frac < 0.2);
    };
    const bool want = force == 2 ||
                      (force == 0 && p.M >= 1024 && p.N >= 1536 && (r.epi == EPI_GELU8 || (RAJNI_F8W_LINES && rounds_ok())));
    if (wide_ok && want) return make_plan(p, RAJNI_TILING_F8_WIDE, 256, f8w::BN, r.lds_wide, cus, 1, nblk_bytes);
  }
  return make_plan(p, RAJNI_TILING_F8_STREAM, 256, f8::BN, r.lds_narrow, cus, 1, nblk_bytes);
}

// Every other workgroup of an XCD starts a residual-epilogue launch `units` x 8192 cycles late, so that the two halves of
// the chip do not hit their prologue loads and epilogue bursts in the same instant.  Round 2 (tools/stagger_probe.py,
// tools/ab_forward.py stagger): proj alone -4 % at 1 unit, fc2 alone flat; in the forward 2 units were best (+0.5-0.8 %).
// Round 3, with the full-line epilogue: stand-alone proj now LOSES with any offset (84.4 us at 0, 88.5 at 1, 97.4 at 2 units;
// four or eight phase groups worse still), in the forward 1 unit is best by 0.1-0.3 % (8.850 / 8.804 ms against 8.872 / 8.825
// at 2 units and 8.878 / 8.838 at 0).  rajni_debug_set_resid_stagger(0) turns it off.
int g_resid_stagger = 1;

// How a launch is asked for: its profile class, whether a residual launch has K <= N (the TAG = 1 twin, see
// gemm_bf16_tn_stream), the stream - and, for rajni_debug_linear_plan, the CU count to plan for (0: the current device's)
// and where the plan goes INSTEAD of a launch.
struct LaunchCtl { int kclass; bool sq; hipStream_t s; int cus; rajni_linear_plan* plan_only; };
// W rows per output column: 2 for the gated epilogue (its flop and byte counts are those of the [2N, K] W it multiplies by)
constexpr int w_rows_per_col(int epi) { return epi == EPI_SWIGLU ? 2 : 1; }
inline int cus_of(const LaunchCtl& l) { return l.cus > 0 ? l.cus : rajni_num_cus(); }

// Launch `Kernel` as planned - the one launch of every GEMM kernel.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per
// (kernel, device): the flags belong to the kernel's own instantiation of this function, one per device (a process may
// drive several GPUs; one process per GPU is the deployment, but a model on cuda:1 in a process whose first launch was on
// cuda:0 must not inherit that device's "done").
template <auto Kernel>
int launch_planned(const rajni_linear_plan& c, int threads, GemmParams& p, const LaunchCtl& l, double bytes, const char* name,
                   int wrows = 1) {
  if (l.plan_only != nullptr) { *l.plan_only = c; return RAJNI_OK; }   // the dry run ends here, ahead of every HIP call
  static bool done_by_device[RAJNI_MAX_DEVICES] = {};
  bool& done = done_by_device[rajni_current_device()];
  if (!done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, c.lds_bytes);
    if (e != hipSuccess) {
      rajni_set_error("hipFuncSetAttribute(gemm): %s", hipGetErrorString(e));
      return RAJNI_ERR_LAUNCH;
    }
    done = true;
  }
  p.tiles_n = c.tiles_n; p.total_tiles = c.total_tiles; p.nblk = c.nblk;
  ProfScope prof(l.kclass, l.s, 2.0 * p.M * (double)p.N * p.K * wrows, bytes);
  hipLaunchKernelGGL(Kernel, dim3(c.grid), dim3(threads), c.lds_bytes, l.s, p);
  RAJNI_CHECK_LAUNCH(name);
  return RAJNI_OK;
}
// algorithmic bytes: X + W + output (+ the residual rows read), each at its element size - fp32 where the residual stream is
inline double gemm_bytes(const GemmParams& p, double xsz, double wsz, double ysz, int wrows = 1) {   // gated: 2N W rows, N output columns
  return xsz * (double)p.M * p.K + ysz * (double)p.M * p.N + wsz * (double)p.N * p.K * wrows;
}
constexpr double out_bytes(int epi, bool sf32) {   // per output element of the 16-bit and fp8 x fp8 families
  const double ysz = epi == EPI_GELU8 ? 1.0 : (sf32 && (epi == EPI_RESID || epi == EPI_PATCH)) ? 4.0 : 2.0;
  return ysz + (epi == EPI_RESID ? (sf32 ? 4.0 : 2.0) : 0.0);
}

// 16-bit activations, A = bf16_t or f16_t (W8: fp8 weights on bf16)
template <int EPI, int ALOAD, bool SF32, bool W8, typename A, int WM, int WN, int MI, int NS>
int launch_stream(const rajni_linear_plan& c, GemmParams& p, const LaunchCtl& l, double bytes) {
  if constexpr (EPI == EPI_RESID)
    if (l.sq) return launch_planned<&wide::gemm_bf16_tn_stream<EPI, ALOAD, SF32, WM, WN, MI, NS, W8, 1, A>>(c, 512, p, l, bytes, "gemm_bf16_tn");
  return launch_planned<&wide::gemm_bf16_tn_stream<EPI, ALOAD, SF32, WM, WN, MI, NS, W8, 0, A>>(c, 512, p, l, bytes, "gemm_bf16_tn",
                                                                                              w_rows_per_col(EPI));
}
template <int EPI, int ALOAD, bool SF32, bool W8 = false, typename A = bf16_t>
int launch_gemm(GemmParams& p, const LaunchCtl& l) {
  constexpr int NS = RAJNI_W8_WIDE_NS_OR(W8);
  constexpr TileTraits T{EPI, resid_nat(EPI, SF32), wide::lds_bytes<EPI, SF32, 4, 8, NS, W8>(), wide::lds_bytes<EPI, SF32, 2, 4, 3, W8>()};
  const rajni_linear_plan c = choose_gemm(p, T, cus_of(l), g_force_tiling, g_nblk_bytes);
  p.stamps = rajni_g_stamps;
  p.stagger = g_resid_stagger;
  const double bytes = gemm_bytes(p, 2.0, W8 ? 1.0 : 2.0, out_bytes(EPI, SF32), w_rows_per_col(EPI));
  if (c.tiling == RAJNI_TILING_WIDE) return launch_stream<EPI, ALOAD, SF32, W8, A, 2, 4, 8, NS>(c, p, l, bytes);
  if (c.tiling == RAJNI_TILING_MID) return launch_stream<EPI, ALOAD, SF32, W8, A, 4, 2, 4, 3>(c, p, l, bytes);
  return launch_planned<&small::gemm_bf16_tn_128x128<EPI, ALOAD, SF32, W8, A>>(c, 256, p, l, bytes, "gemm_bf16_tn", w_rows_per_col(EPI));
}
template <int EPI, bool SF32>
int launch_gemm_f8(GemmParams& p, const LaunchCtl& l) {
  constexpr bool HAS_WIDE = EPI == EPI_BIAS || EPI == EPI_GELU8;
  constexpr TileTraits T{EPI, resid_nat(EPI, SF32), HAS_WIDE ? f8w::lds_bytes(EPI) : 0, f8::lds_bytes(EPI, SF32)};
  const rajni_linear_plan c = choose_gemm_f8(p, T, cus_of(l), g_force_f8_tiling, g_nblk_bytes);
  p.stamps = rajni_g_stamps;
  const double bytes = gemm_bytes(p, 1.0, 1.0, out_bytes(EPI, SF32));
  if constexpr (HAS_WIDE)
    if (c.tiling == RAJNI_TILING_F8_WIDE) return launch_planned<&f8w::gemm_f8_tn_wide<EPI>>(c, 512, p, l, bytes, "gemm_f8_tn_wide");
  if constexpr (EPI == EPI_RESID)
    if (l.sq) return launch_planned<&f8::gemm_f8_tn_stream<EPI, SF32, 1>>(c, 512, p, l, bytes, "gemm_f8_tn");
  return launch_planned<&f8::gemm_f8_tn_stream<EPI, SF32, 0>>(c, 512, p, l, bytes, "gemm_f8_tn");
}
template <int EPI, int ALOAD>
int launch_gemm_f32(GemmParams& p, const LaunchCtl& l) {   // (as found: the residual rows a RESID launch reads are not counted)
  constexpr int WR = w_rows_per_col(EPI);
  return launch_planned<&f32::gemm_f32_tn_128x128<EPI, ALOAD>>(make_plan(p, RAJNI_TILING_F32, 128, 128, f32::LDS_BYTES, 0, 0, 0, WR == 2),
                                                              256, p, l, gemm_bytes(p, 4.0, 4.0, 4.0, WR), "gemm_f32_tn", WR);
}

// rajni_linear and its dry run: the refusals, then the one table - format x epilogue (x fp32 residual stream for RESID)
enum { FMT_F8F8, FMT_W8, FMT_F32, FMT_BF16, FMT_F16 };   // fp8 x fp8, fp8 weights on bf16, and the three plain dtypes
template <bool W8, typename A>
int linear16(int epi, bool sf32, GemmParams& p, const LaunchCtl& l) {
  return epi == EPI_BIAS ? launch_gemm<EPI_BIAS, ALOAD_PLAIN, false, W8, A>(p, l)
       : epi == EPI_GELU ? launch_gemm<EPI_GELU, ALOAD_PLAIN, false, W8, A>(p, l)
       : epi == EPI_QGELU ? launch_gemm<EPI_QGELU, ALOAD_PLAIN, false, W8, A>(p, l)
       : epi == EPI_SWIGLU ? launch_gemm<EPI_SWIGLU, ALOAD_PLAIN, false, W8, A>(p, l)
       : sf32 ? launch_gemm<EPI_RESID, ALOAD_PLAIN, true, W8, A>(p, l) : launch_gemm<EPI_RESID, ALOAD_PLAIN, false, W8, A>(p, l);
}
int linear(const rajni_linear_args& a, LaunchCtl l) {
  RAJNI_REQUIRE(a.dtype == RAJNI_BF16 || a.dtype == RAJNI_F32 || a.dtype == RAJNI_F16, RAJNI_ERR_INVALID,
                "rajni_linear: bad dtype %d", a.dtype);
  RAJNI_REQUIRE(a.dtype != RAJNI_F16 || (a.w_scale == nullptr && a.x_scale == nullptr), RAJNI_ERR_UNSUPPORTED,
                "rajni_linear: fp8 weights or activations need a bf16 model (dtype fp16 given)");
  RAJNI_REQUIRE(a.x && a.w && a.y, RAJNI_ERR_INVALID, "rajni_linear: null pointer");
  RAJNI_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.K % 64 == 0, RAJNI_ERR_INVALID,
                "rajni_linear: M,N>0 and K %% 64 == 0 required (M=%d N=%d K=%d)", a.M, a.N, a.K);
  RAJNI_REQUIRE(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldc % 8 == 0, RAJNI_ERR_INVALID,
                "rajni_linear: leading dimensions must be multiples of 8 elements");
  {
    const PlacedPtr data[] = {{"x", a.x, 16}, {"w", a.w, 16}, {"y", a.y, 16}, {"resid", a.resid, 16}};
    for (const PlacedPtr& d : data)
      RAJNI_REQUIRE((uintptr_t)d.p % 16 == 0, RAJNI_ERR_INVALID, "rajni_linear: pointers must be 16-byte aligned (%s)", d.name);
  }
  // the stream tilings read bias, gamma and w_scale 16 bytes at a time (gemm_tail, gemm_f8.h); the row scales and r_idx are
  // read one element at a time
  RAJNI_REQUIRE_PLACED("rajni_linear", {"bias", a.bias, 16}, {"gamma", a.gamma, 16}, {"w_scale", a.w_scale, 16}, {"x_scale", a.x_scale, 4},
                       {"y_scale", a.y_scale, 4}, {"r_idx", a.r_idx, 4});
  GemmParams p{};
  p.X = a.x; p.lda = a.lda;
  p.W = a.w; p.ldw = a.ldw;
  p.bias = a.bias; p.gamma = a.gamma;
  p.R = a.resid; p.ldr = a.ldr;
  p.ridx = a.r_idx; p.r_np = a.r_np > 0 ? a.r_np : 1; p.r_nsrc = a.r_nsrc;
  p.Y = a.y; p.ldc = a.ldc;
  p.M = a.M; p.N = a.N; p.K = a.K;
  p.wscale = a.w_scale;
  const int fmt = a.x_scale != nullptr ? FMT_F8F8 : a.w_scale != nullptr ? FMT_W8
                : a.dtype == RAJNI_F32 ? FMT_F32 : a.dtype == RAJNI_F16 ? FMT_F16 : FMT_BF16;
  const bool f8 = fmt == FMT_F8F8;
  if (f8) {   // fp8 e4m3 activations AND weights on the fp8 matrix pipe
    RAJNI_REQUIRE(a.w_scale != nullptr && a.dtype == RAJNI_BF16, RAJNI_ERR_INVALID,
                  "rajni_linear: fp8 activations (x_scale) need fp8 weights (w_scale) and dtype bf16");
    RAJNI_REQUIRE(a.K % 256 == 0 && a.K >= 512, RAJNI_ERR_UNSUPPORTED,
                  "rajni_linear: the fp8 x fp8 kernel needs K %% 256 == 0 and K >= 512 (K=%d)", a.K);
    RAJNI_REQUIRE(a.lda % 16 == 0 && a.ldw % 16 == 0, RAJNI_ERR_INVALID, "rajni_linear: fp8 operands need lda, ldw %% 16 == 0 (bytes)");
    p.xscale = a.x_scale; p.yscale = a.y_scale;
  } else {
    RAJNI_REQUIRE(a.y_scale == nullptr, RAJNI_ERR_INVALID, "rajni_linear: y_scale without x_scale");
    if (fmt == FMT_W8) {   // fp8 e4m3 weights, bf16 activations
      RAJNI_REQUIRE(a.dtype == RAJNI_BF16, RAJNI_ERR_UNSUPPORTED, "rajni_linear: fp8 weights need bf16 activations");
      RAJNI_REQUIRE(a.ldw % 16 == 0, RAJNI_ERR_INVALID, "rajni_linear: fp8 weights need ldw %% 16 == 0");
    }
  }
  int epi;
  switch (a.epilogue) {
    case RAJNI_EPI_BIAS:
      RAJNI_REQUIRE(!f8 || a.y_scale == nullptr, RAJNI_ERR_UNSUPPORTED, "rajni_linear: an fp8 output (y_scale) exists for the GELU epilogue only");
      epi = EPI_BIAS; l.kclass = f8 ? KC_GEMM8_BIAS : KC_GEMM_BIAS;
      break;
    case RAJNI_EPI_BIAS_GELU:
      RAJNI_REQUIRE(!f8 || (a.y_scale != nullptr && a.ldc % 16 == 0), RAJNI_ERR_UNSUPPORTED,
                    "rajni_linear: the fp8 x fp8 GELU epilogue writes e4m3 (y_scale required, ldc %% 16 == 0 bytes)");
      epi = f8 ? EPI_GELU8 : EPI_GELU; l.kclass = f8 ? KC_GEMM8_GELU : KC_GEMM_GELU;
      break;
    case RAJNI_EPI_BIAS_QUICK_GELU:
      RAJNI_REQUIRE(!f8, RAJNI_ERR_UNSUPPORTED,
                    "rajni_linear: the QuickGELU epilogue is unsupported with fp8 activations (x_scale): the fp8 x fp8 kernel's "
                    "re-quantising epilogue exists for exact GELU only");
      epi = EPI_QGELU; l.kclass = KC_GEMM_GELU;
      break;
    case RAJNI_EPI_BIAS_SWIGLU:
      RAJNI_REQUIRE(!f8, RAJNI_ERR_UNSUPPORTED,
                    "rajni_linear: the SwiGLU epilogue is unsupported with fp8 activations (x_scale): the fp8 x fp8 kernel's "
                    "re-quantising epilogue exists for exact GELU only");
      // the N + n row offsets and the 2N-row shape rule are ints
      RAJNI_REQUIRE(a.N <= (1 << 30), RAJNI_ERR_INVALID, "rajni_linear: the SwiGLU epilogue needs N <= 2^30 (N=%d)", a.N);
      epi = EPI_SWIGLU; l.kclass = KC_GEMM_GELU;
      break;
    case RAJNI_EPI_BIAS_RESID:
      // fp32 asks for no ldr rule: its epilogue (epilogue_row_f32) reads the residual row one element at a time, so any
      // stride serves; the 16-bit and fp8 x fp8 epilogues read it 16 bytes at a time.  Only fp8 x fp8 can meet a y_scale
      // here and names it
      if (f8) RAJNI_REQUIRE(a.resid != nullptr && a.ldr % 8 == 0 && a.y_scale == nullptr, RAJNI_ERR_INVALID,
                            "rajni_linear: RESID epilogue needs resid, ldr %% 8 == 0 and no y_scale");
      else if (fmt == FMT_F32) RAJNI_REQUIRE(a.resid != nullptr, RAJNI_ERR_INVALID, "rajni_linear: RESID epilogue needs resid");
      else RAJNI_REQUIRE(a.resid != nullptr && a.ldr % 8 == 0, RAJNI_ERR_INVALID,
                         "rajni_linear: RESID epilogue needs resid and ldr %% 8 == 0");
      epi = EPI_RESID; l.sq = a.K <= a.N;   // K <= N (the attention projection): a profile class and a kernel twin of its own
      l.kclass = f8 ? (l.sq ? KC_GEMM8_RESID_SQ : KC_GEMM8_RESID) : (l.sq ? KC_GEMM_RESID_SQ : KC_GEMM_RESID);
      break;
    default:
      rajni_set_error("rajni_linear: unknown epilogue %d", a.epilogue);
      return RAJNI_ERR_INVALID;
  }
  const bool sf32 = a.stream_f32 != 0;
  switch (fmt) {
    case FMT_F8F8: return epi == EPI_BIAS ? launch_gemm_f8<EPI_BIAS, false>(p, l) : epi == EPI_GELU8 ? launch_gemm_f8<EPI_GELU8, false>(p, l)
                        : sf32 ? launch_gemm_f8<EPI_RESID, true>(p, l) : launch_gemm_f8<EPI_RESID, false>(p, l);
    case FMT_F32: return epi == EPI_BIAS ? launch_gemm_f32<EPI_BIAS, ALOAD_PLAIN>(p, l) : epi == EPI_GELU ? launch_gemm_f32<EPI_GELU, ALOAD_PLAIN>(p, l)
                       : epi == EPI_QGELU ? launch_gemm_f32<EPI_QGELU, ALOAD_PLAIN>(p, l)
                       : epi == EPI_SWIGLU ? launch_gemm_f32<EPI_SWIGLU, ALOAD_PLAIN>(p, l) : launch_gemm_f32<EPI_RESID, ALOAD_PLAIN>(p, l);
    case FMT_W8: return linear16<true, bf16_t>(epi, sf32, p, l);
    case FMT_F16: return linear16<false, f16_t>(epi, sf32, p, l);
    default: return linear16<false, bf16_t>(epi, sf32, p, l);
  }
}

}  // namespace

extern "C" void rajni_debug_force_gemm_tiling(int mode) { g_force_tiling = mode; }
extern "C" void rajni_debug_force_f8_tiling(int mode) { g_force_f8_tiling = mode; }
extern "C" void rajni_debug_set_resid_stagger(int units) { g_resid_stagger = units; }
extern "C" void rajni_debug_set_gemm_nblock_bytes(int bytes) { g_nblk_bytes = bytes; }
// diagnostic builds (-DRAJNI_GEMM_STAMPS): device buffer of 4 x u64 per workgroup, or NULL
extern "C" void rajni_debug_set_gemm_stamps(void* buf) { rajni_g_stamps = (unsigned long long*)buf; }

int launch_linear(const rajni_linear_args& a, hipStream_t s) { return linear(a, LaunchCtl{0, false, s, 0, nullptr}); }
// rajni_linear up to, not including, its launch (launch_planned), planned for a device of `cus` CUs
extern "C" int rajni_debug_linear_plan(const rajni_linear_args* args, int cus, rajni_linear_plan* out) {
  RAJNI_REQUIRE(args != nullptr, RAJNI_ERR_INVALID, "rajni_linear: null args");
  RAJNI_REQUIRE(out != nullptr && cus > 0, RAJNI_ERR_INVALID, "rajni_debug_linear_plan: needs out and cus > 0");
  return linear(*args, LaunchCtl{0, false, nullptr, cus, out});
}

// the fused im2col loader reads 16-byte runs of a patch row with shifts: power-of-two patches of >= 8 pixels
// whose K = Cin*P*P is whole K steps.  Everything else (P = 14: ViT-L/14, ViT-H/14, DINOv2, CLIP) goes through a
// materialised, zero-padded column matrix.
// (W is the image width, the row stride: a 16-byte run must not straddle rows; the height is free)
static bool patch_fused(int Cin, int W, int P) {
  return P >= 8 && (P & (P - 1)) == 0 && W % 8 == 0 && (Cin * P * P) % 64 == 0;
}
size_t patch_embed_workspace_bytes(int B, int Cin, int H, int W, int P, int dtype) {
  if (P <= 0 || H <= 0 || W <= 0 || H % P != 0 || W % P != 0 || patch_fused(Cin, W, P)) return 0;
  const size_t kpad = ((size_t)Cin * P * P + 63) / 64 * 64, gh = H / P, gw = W / P;
  return (size_t)B * gh * gw * kpad * (dtype == RAJNI_F32 ? 4 : 2);
}
// cols[m, k] = images[b, c, gy*P + py, gx*P + px] for k = (c*P + py)*P + px < Cin*P*P, 0 for the padding; images are
// [B, Cin, H, W], npatch = (H/P) * gw patches per image, gw = W/P;
// one thread = 8 consecutive k of one patch row (one 16-byte store for bf16)
template <typename T>
__global__ void __launch_bounds__(256) im2col_kernel(const T* img, T* cols, int Cin, int H, int W, int P, int gw, int npatch, int kpad, long total8) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int k8 = kpad >> 3;
  const long m = i / k8;
  const int k0 = (int)(i - m * k8) * 8;
  const int b = (int)(m / npatch), pp = (int)(m - (long)b * npatch);
  const int gy = pp / gw, gx = pp - gy * gw;
  const int K = Cin * P * P;
  T v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    T e = T(0);
    if (k < K) {
      const int c = k / (P * P), r = k - c * P * P, py = r / P, px = r - py * P;
      e = img[(((long)b * Cin + c) * H + gy * P + py) * W + gx * P + px];
    }
    v[j] = e;
  }
  T* dst = cols + m * kpad + k0;
#pragma unroll
  for (int j = 0; j < 8; ++j) dst[j] = v[j];
}

// (dtype, out_f32) -> (the residual stream is fp32, the element type of images and parameters): f(bool constant, T{})
template <typename F>
static void with_stream_types(int dtype, int out_f32, F&& f) {
  if (dtype == RAJNI_F32) f(std::true_type{}, float{});
  else if (dtype == RAJNI_F16) out_f32 ? f(std::true_type{}, f16_t{}) : f(std::false_type{}, f16_t{});
  else out_f32 ? f(std::true_type{}, bf16_t{}) : f(std::false_type{}, bf16_t{});
}
int launch_patch_embed(const void* images, const void* w, const float* bias, const void* cls,
                       const void* pos, int pos_has_cls, void* x, int out_f32, int B, int Cin, int H, int W,
                       int P, int C, int dtype, void* ws, size_t ws_bytes, hipStream_t s, int num_prefix, const void* reg, int has_cls) {
  if (has_cls) {
    RAJNI_REQUIRE(images && w && cls && pos && x, RAJNI_ERR_INVALID, "rajni_patch_embed: null pointer");
    RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                  "rajni_patch_embed: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
    RAJNI_REQUIRE(num_prefix == 1 || reg != nullptr, RAJNI_ERR_INVALID, "rajni_patch_embed: %d prefix tokens but reg_token is null", num_prefix);
    RAJNI_REQUIRE(num_prefix == 1 || ((uintptr_t)cls % 16 == 0 && (uintptr_t)reg % 16 == 0 && (uintptr_t)pos % 16 == 0),
                  RAJNI_ERR_INVALID, "rajni_patch_embed: cls, reg_token and pos must be 16-byte aligned");
  } else {   // no class row: the prefix rows are the num_prefix registers, possibly none
    RAJNI_REQUIRE(images && w && pos && x, RAJNI_ERR_INVALID, "rajni_patch_embed: null pointer");
    RAJNI_REQUIRE(num_prefix >= 0 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                  "rajni_patch_embed: without a class row num_prefix (the register count) must be 0..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
    RAJNI_REQUIRE((num_prefix > 0) == (reg != nullptr), RAJNI_ERR_INVALID,
                  "rajni_patch_embed: %d register tokens but reg_token is %s", num_prefix, reg ? "given" : "null");
    RAJNI_REQUIRE((uintptr_t)reg % 16 == 0 && (uintptr_t)pos % 16 == 0, RAJNI_ERR_INVALID,
                  "rajni_patch_embed: reg_token and pos must be 16-byte aligned");
  }
  if (H == W)   // (the square entry points: their wording)
    RAJNI_REQUIRE(P >= 1 && W % P == 0 && B > 0 && Cin > 0, RAJNI_ERR_INVALID,
                  "rajni_patch_embed: the patch size must divide the image (P=%d S=%d)", P, W);
  RAJNI_REQUIRE(P >= 1 && H > 0 && W > 0 && H % P == 0 && W % P == 0 && B > 0 && Cin > 0, RAJNI_ERR_INVALID,
                "rajni_patch_embed: the patch size must divide the image (P=%d H=%d W=%d)", P, H, W);
  RAJNI_REQUIRE(C % 8 == 0, RAJNI_ERR_UNSUPPORTED, "rajni_patch_embed: C %% 8 == 0 required");
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID,
                "rajni_patch_embed: bad dtype %d", dtype);
  const int K = Cin * P * P, kpad = (K + 63) / 64 * 64;
  const int gw = W / P, npatch = (H / P) * gw;
  GemmParams p{};
  p.W = w; p.ldw = kpad;
  p.bias = bias;
  p.Y = x; p.ldc = C;
  p.M = B * npatch; p.N = C; p.K = kpad;
  p.gw = gw; p.npatch = npatch;
  p.pos = pos; p.pos_off = pos_has_cls ? num_prefix : 0;
  p.nprefix = num_prefix;
  const bool fused = patch_fused(Cin, W, P);
  if (fused) {
    int log2ps = 0;
    while ((1 << log2ps) < P) ++log2ps;
    p.X = images; p.lda = 0;
    p.cin = Cin; p.S = W; p.IH = H; p.log2ps = log2ps;
  } else {
    const size_t need = patch_embed_workspace_bytes(B, Cin, H, W, P, dtype);
    RAJNI_REQUIRE(ws != nullptr && ws_bytes >= need && (uintptr_t)ws % 16 == 0, RAJNI_ERR_INVALID,
                  "rajni_patch_embed: patch size %d needs a %zu-byte, 16-byte aligned column workspace (got %zu)", P, need, ws_bytes);
    ProfScope prof(KC_CLS_POS, s, 0.0, 2.0 * (double)need);
    const long total8 = (long)B * npatch * (kpad / 8);
    const dim3 grid((unsigned)((total8 + 255) / 256)), block(256);
    if (dtype == RAJNI_F32)
      hipLaunchKernelGGL(im2col_kernel<float>, grid, block, 0, s, (const float*)images, (float*)ws, Cin, H, W, P, gw, npatch, kpad, total8);
    else   // a byte copy: the bf16 instantiation serves fp16 images too
      hipLaunchKernelGGL(im2col_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)images, (bf16_t*)ws, Cin, H, W, P, gw, npatch, kpad, total8);
    RAJNI_CHECK_LAUNCH("im2col_kernel");
    p.X = ws; p.lda = kpad;
  }
  int rc = RAJNI_OK;
  const LaunchCtl l{KC_GEMM_PATCH, false, s, 0, nullptr};
  with_stream_types(dtype, out_f32, [&](auto sf32, auto t) {
    using T = decltype(t);
    constexpr bool SF32 = decltype(sf32)::value;
    if constexpr (std::is_same<T, float>::value)
      rc = fused ? launch_gemm_f32<EPI_PATCH, ALOAD_PATCH>(p, l) : launch_gemm_f32<EPI_PATCH, ALOAD_PLAIN>(p, l);
    else
      rc = fused ? launch_gemm<EPI_PATCH, ALOAD_PATCH, SF32, false, T>(p, l) : launch_gemm<EPI_PATCH, ALOAD_PLAIN, SF32, false, T>(p, l);
  });
  if (rc != RAJNI_OK) return rc;
  ProfScope prof(KC_CLS_POS, s, 0.0, 6.0 * B * num_prefix * C);
  const long stride = (long)(npatch + num_prefix) * C;
  const dim3 block(256);
  if (!has_cls) {
    // the R register rows: prefix_pos_kernel with register 0 in the class row's place and the others behind it (R = 0: no
    // prefix row, no launch)
    if (num_prefix == 0) return RAJNI_OK;
    const dim3 grid((B * num_prefix * (C / 8) + 255) / 256);
    with_stream_types(dtype, out_f32, [&](auto sf32, auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((prefix_pos_kernel<decltype(sf32)::value, T>), grid, block, 0, s, (const T*)reg, (const T*)reg + C, (const T*)pos,
                         pos_has_cls, x, stride, B, num_prefix, C);
    });
    RAJNI_CHECK_LAUNCH("prefix_pos_kernel");
  } else if (num_prefix > 1) {
    const dim3 grid((B * num_prefix * (C / 8) + 255) / 256);
    with_stream_types(dtype, out_f32, [&](auto sf32, auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((prefix_pos_kernel<decltype(sf32)::value, T>), grid, block, 0, s, (const T*)cls, (const T*)reg, (const T*)pos,
                         pos_has_cls, x, stride, B, num_prefix, C);
    });
    RAJNI_CHECK_LAUNCH("prefix_pos_kernel");
  } else {
    const dim3 grid((B * C + 255) / 256);
    with_stream_types(dtype, out_f32, [&](auto sf32, auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((cls_pos_kernel<decltype(sf32)::value, T>), grid, block, 0, s, (const T*)cls, (const T*)pos, pos_has_cls, x,
                         stride, B, C);
    });
    RAJNI_CHECK_LAUNCH("cls_pos_kernel");
  }
  return RAJNI_OK;
}
