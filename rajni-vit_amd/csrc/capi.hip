// extern "C" surface of librajni_hip.so (include/rajni_hip.h): argument checks, error strings,
// the HIP-event measurement hooks, and thin wrappers over the launchers.
#include <stdarg.h>
#include <string.h>
#include <vector>
#include "common.h"

namespace {
thread_local char g_err[512] = "";

struct ProfRec { int kc; hipEvent_t e0, e1; double flops, bytes; };
unsigned g_prof_mask = 0;
std::vector<ProfRec> g_pending;
std::vector<hipEvent_t> g_pool;
long long g_launches[RAJNI_NUM_KCLASS];
double g_ms[RAJNI_NUM_KCLASS], g_flops[RAJNI_NUM_KCLASS], g_bytes[RAJNI_NUM_KCLASS];

hipEvent_t get_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
const char* const kNames[RAJNI_NUM_KCLASS] = {
    "gemm_bf16_tn<bias>", "gemm_bf16_tn<bias,gelu>", "gemm_bf16_tn<bias,ls,resid>",
    "gemm_bf16_tn<patch>", "attn_bf16_d64", "layernorm_kernel", "score_select_kernel<fused>",
    "score_select_kernel<scores>", "score_select_kernel<select>", "gather_rows_kernel",
    "cls_pos_kernel", "other", "gemm_bf16_tn<bias,ls,resid> K<=N",
    "gemm_f8_tn<bias>", "gemm_f8_tn<bias,gelu,requant>", "gemm_f8_tn<bias,ls,resid>",
    "gemm_f8_tn<bias,ls,resid> K<=N"};
}  // namespace

unsigned long long* rajni_g_stamps = nullptr;
int rajni_g_persistent_cap = 0;   // test hook: at most this many workgroups per persistent launch (0 = no cap)
extern "C" void rajni_debug_set_persistent_workgroups(int n) { rajni_g_persistent_cap = n > 0 ? n : 0; }

int rajni_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= RAJNI_MAX_DEVICES) return 0;
  return dev;
}
int rajni_num_cus() {
  static int cus[RAJNI_MAX_DEVICES] = {};     // 0 = not read yet (benign race: every writer stores the same value)
  const int dev = rajni_current_device();
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

void rajni_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int rajni_check_placement(const char* who, const PlacedPtr* ptrs, int n) {
  for (int i = 0; i < n; ++i)
    RAJNI_REQUIRE(reinterpret_cast<uintptr_t>(ptrs[i].p) % (uintptr_t)ptrs[i].align == 0, RAJNI_ERR_INVALID,
                  "%s: %s must be %d-byte aligned", who, ptrs[i].name, ptrs[i].align);
  return RAJNI_OK;
}

ProfScope::ProfScope(int kclass, hipStream_t stream, double flops, double bytes)
    : kc(kclass), s(stream), rec(nullptr) {
  if (!(g_prof_mask & (1u << kclass))) return;
  ProfRec r{kclass, get_event(), get_event(), flops, bytes};
  if (!r.e0 || !r.e1) return;
  (void)hipEventRecord(r.e0, s);
  g_pending.push_back(r);
  rec = reinterpret_cast<void*>(g_pending.size());  // index + 1
}
ProfScope::~ProfScope() {
  if (!rec) return;
  const size_t i = reinterpret_cast<size_t>(rec) - 1;
  (void)hipEventRecord(g_pending[i].e1, s);
}

extern "C" {

int rajni_abi_version(void) { return RAJNI_ABI_VERSION; }
const char* rajni_last_error(void) { return g_err; }

int rajni_device_check(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    rajni_set_error("no HIP device visible: %s", hipGetErrorString(e));
    return RAJNI_ERR_LAUNCH;
  }
  int dev = 0;
  (void)hipGetDevice(&dev);
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, dev);
  if (e != hipSuccess) {
    rajni_set_error("hipGetDeviceProperties: %s", hipGetErrorString(e));
    return RAJNI_ERR_LAUNCH;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    rajni_set_error("device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
    return RAJNI_ERR_UNSUPPORTED;
  }
  return RAJNI_OK;
}

#define NEED_DTYPE(name)                                                                                     \
  RAJNI_REQUIRE(dtype == RAJNI_BF16 || dtype == RAJNI_F32 || dtype == RAJNI_F16, RAJNI_ERR_INVALID, name ": bad dtype %d", \
                dtype)

int rajni_importance(const void* qkv, void* scores_out, int B, int N, int H, int D, float eps,
                     int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_importance");
  RAJNI_REQUIRE_PLACED("rajni_importance", {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(qkv && scores_out, RAJNI_ERR_INVALID, "rajni_importance: null pointer");
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, 0, scores_out, nullptr, nullptr, dtype,
                             (hipStream_t)stream);
}

int rajni_select_topk(const void* scores, int B, int N, int keep, int32_t* keep_idx,
                      void* next_scores, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_select_topk");
  RAJNI_REQUIRE_PLACED("rajni_select_topk", {"scores", scores, rajni_elem_bytes(dtype)}, {"keep_idx", keep_idx, 4},
                       {"next_scores", next_scores, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(scores && keep_idx, RAJNI_ERR_INVALID, "rajni_select_topk: null pointer");
  RAJNI_REQUIRE(keep >= 1, RAJNI_ERR_INVALID, "rajni_select_topk: keep must be >= 1");
  return launch_score_select(nullptr, scores, B, N, 0, 0, 0.f, keep, nullptr, keep_idx, next_scores, dtype,
                             (hipStream_t)stream);
}

int rajni_score_select(const void* qkv, int B, int N, int H, int D, float eps, int keep,
                       void* scores_out, int32_t* keep_idx, void* next_scores, int dtype,
                       rajni_stream_t stream) {
  NEED_DTYPE("rajni_score_select");
  RAJNI_REQUIRE_PLACED("rajni_score_select", {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)},
                       {"keep_idx", keep_idx, 4}, {"next_scores", next_scores, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(qkv && keep_idx, RAJNI_ERR_INVALID, "rajni_score_select: null pointer");
  RAJNI_REQUIRE(keep >= 1, RAJNI_ERR_INVALID, "rajni_score_select: keep must be >= 1");
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, keep, scores_out, keep_idx, next_scores, dtype,
                             (hipStream_t)stream);
}

int rajni_select_topk_prefix(const void* scores, int B, int N, int num_prefix, int keep, int32_t* keep_idx,
                             void* next_scores, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_select_topk_prefix");
  RAJNI_REQUIRE_PLACED("rajni_select_topk_prefix", {"scores", scores, rajni_elem_bytes(dtype)}, {"keep_idx", keep_idx, 4},
                       {"next_scores", next_scores, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(scores && keep_idx, RAJNI_ERR_INVALID, "rajni_select_topk_prefix: null pointer");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_select_topk_prefix: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "rajni_select_topk_prefix: need B > 0 and at least one patch token (B=%d N=%d num_prefix=%d)", B, N, num_prefix);
  RAJNI_REQUIRE(keep >= 1 && keep <= N - num_prefix, RAJNI_ERR_INVALID,
                "rajni_select_topk_prefix: keep must be 1..%d (%d)", N - num_prefix, keep);
  return launch_score_select(nullptr, scores, B, N, 0, 0, 0.f, keep, nullptr, keep_idx, next_scores, dtype,
                             (hipStream_t)stream, num_prefix);
}

int rajni_score_select_prefix(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep,
                              void* scores_out, int32_t* keep_idx, void* next_scores, int dtype,
                              rajni_stream_t stream) {
  NEED_DTYPE("rajni_score_select_prefix");
  RAJNI_REQUIRE_PLACED("rajni_score_select_prefix", {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)},
                       {"keep_idx", keep_idx, 4}, {"next_scores", next_scores, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(qkv && keep_idx, RAJNI_ERR_INVALID, "rajni_score_select_prefix: null pointer");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_score_select_prefix: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "rajni_score_select_prefix: need B > 0 and at least one patch token (B=%d N=%d num_prefix=%d)", B, N, num_prefix);
  RAJNI_REQUIRE(keep >= 1 && keep <= N - num_prefix, RAJNI_ERR_INVALID,
                "rajni_score_select_prefix: keep must be 1..%d (%d)", N - num_prefix, keep);
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, keep, scores_out, keep_idx, next_scores, dtype,
                             (hipStream_t)stream, num_prefix);
}

int rajni_score_select_ws(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep,
                          void* scores_out, int32_t* keep_idx, void* next_scores, int dtype, void* workspace,
                          size_t workspace_bytes, rajni_stream_t stream) {
  NEED_DTYPE("rajni_score_select_ws");
  // (the grid limit of the tiled path before the pointers: a refused shape is refused whatever else the call holds)
  RAJNI_REQUIRE(B <= RAJNI_MAX_GRID_YZ || rajni_score_select_workspace_bytes(B, N, H, D, dtype) == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_score_select_ws: B=%d - one launch of the tiled path takes at most %d images (grid: token tiles x images)",
                B, RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE_PLACED("rajni_score_select_ws", {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)},
                       {"keep_idx", keep_idx, 4}, {"next_scores", next_scores, rajni_elem_bytes(dtype)}, {"workspace", workspace, 256});
  RAJNI_REQUIRE(qkv != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_ws: qkv is null");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_score_select_ws: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "rajni_score_select_ws: need B > 0 and at least one patch token (B=%d N=%d num_prefix=%d)", B, N, num_prefix);
  RAJNI_REQUIRE(keep >= 0 && keep <= N - num_prefix, RAJNI_ERR_INVALID,
                "rajni_score_select_ws: keep must be 0 (scores only) or 1..%d (%d)", N - num_prefix, keep);
  RAJNI_REQUIRE(keep == 0 || keep_idx != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_ws: keep_idx is null with keep=%d", keep);
  RAJNI_REQUIRE(keep > 0 || scores_out != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_ws: scores_out is null with keep=0");
  const size_t need = rajni_score_select_workspace_bytes(B, N, H, D, dtype);
  RAJNI_REQUIRE(need == 0 || workspace != nullptr, RAJNI_ERR_INVALID,
                "rajni_score_select_ws: workspace is null but N=%d H=%d D=%d needs %zu B (rajni_score_select_workspace_bytes)", N, H, D, need);
  RAJNI_REQUIRE(workspace_bytes >= need, RAJNI_ERR_INVALID,
                "rajni_score_select_ws: workspace_bytes=%zu but N=%d H=%d D=%d needs %zu B", workspace_bytes, N, H, D, need);
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, keep, scores_out, keep_idx, next_scores, dtype,
                             (hipStream_t)stream, num_prefix, need ? workspace : nullptr, need ? workspace_bytes : 0);
}

int rajni_gather_rows(const void* src, const int32_t* idx, void* dst, int B, int n_src, int n_dst,
                      int row_elems, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_gather_rows");
  RAJNI_REQUIRE_PLACED("rajni_gather_rows", {"src", src, 16}, {"idx", idx, 4}, {"dst", dst, 16});
  const int es = dtype == RAJNI_F32 ? 4 : 2;   // a byte copy: bf16 and fp16 rows alike
  return launch_gather_rows(src, idx, dst, B, n_src, n_dst, row_elems * es, (hipStream_t)stream);
}

int rajni_attention(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np,
                    int H, int D, float scale, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_attention");
  RAJNI_REQUIRE_PLACED("rajni_attention", {"qkv", qkv, 16}, {"keep_idx", keep_idx, 4}, {"out", out, 16});
  return launch_attention(qkv, keep_idx, out, B, n_src, np, np, H, D, scale, dtype, (hipStream_t)stream);
}

// rajni_attention with a relative position bias (include/rajni_hip_relpos.h)
int rajni_attention_relpos(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int H, int D, float scale,
                           int dtype, const float* table, const float* prefix_q, const float* prefix_k, const float* prefix_qk,
                           int gh, int gw, int num_prefix, const int32_t* pos, rajni_stream_t stream) {
  NEED_DTYPE("rajni_attention_relpos");
  RAJNI_REQUIRE_PLACED("rajni_attention_relpos", {"qkv", qkv, 16}, {"keep_idx", keep_idx, 4}, {"out", out, 16}, {"table", table, 4},
                       {"prefix_q", prefix_q, 4}, {"prefix_k", prefix_k, 4}, {"prefix_qk", prefix_qk, 4}, {"pos", pos, 4});
  return launch_attention_relpos(qkv, keep_idx, out, B, n_src, np, np, H, D, scale, dtype, table, prefix_q, prefix_k, prefix_qk, gh, gw,
                                 num_prefix, pos, (hipStream_t)stream);
}

// rajni_score_select_ws with the class row's relative position bias (include/rajni_hip_relpos.h)
int rajni_score_select_relpos(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep, void* scores_out,
                              int32_t* keep_idx, void* next_scores, int dtype, void* workspace, size_t workspace_bytes,
                              const float* prefix_q, const float* prefix_qk, rajni_stream_t stream) {
  const char* who = "rajni_score_select_relpos";
  NEED_DTYPE("rajni_score_select_relpos");
  RAJNI_REQUIRE(B <= RAJNI_MAX_GRID_YZ || rajni_score_select_workspace_bytes(B, N, H, D, dtype) == 0, RAJNI_ERR_UNSUPPORTED,
                "%s: B=%d - one launch of the tiled path takes at most %d images (grid: token tiles x images)", who, B, RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE_PLACED(who, {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)}, {"keep_idx", keep_idx, 4},
                       {"next_scores", next_scores, rajni_elem_bytes(dtype)}, {"workspace", workspace, 256}, {"prefix_q", prefix_q, 4},
                       {"prefix_qk", prefix_qk, 4});
  RAJNI_REQUIRE(qkv != nullptr && prefix_q != nullptr && prefix_qk != nullptr, RAJNI_ERR_INVALID, "%s: null pointer", who);
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID, "%s: num_prefix must be 1..%d (%d)", who,
                RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "%s: need B > 0 and at least one patch token (B=%d N=%d num_prefix=%d)", who, B, N, num_prefix);
  RAJNI_REQUIRE(keep >= 0 && keep <= N - num_prefix, RAJNI_ERR_INVALID, "%s: keep must be 0 (scores only) or 1..%d (%d)", who,
                N - num_prefix, keep);
  RAJNI_REQUIRE(keep == 0 || keep_idx != nullptr, RAJNI_ERR_INVALID, "%s: keep_idx is null with keep=%d", who, keep);
  RAJNI_REQUIRE(keep > 0 || scores_out != nullptr, RAJNI_ERR_INVALID, "%s: scores_out is null with keep=0", who);
  const size_t need = rajni_score_select_workspace_bytes(B, N, H, D, dtype);
  RAJNI_REQUIRE(need == 0 || workspace != nullptr, RAJNI_ERR_INVALID,
                "%s: workspace is null but N=%d H=%d D=%d needs %zu B (rajni_score_select_workspace_bytes)", who, N, H, D, need);
  RAJNI_REQUIRE(workspace_bytes >= need, RAJNI_ERR_INVALID, "%s: workspace_bytes=%zu but N=%d H=%d D=%d needs %zu B", who,
                workspace_bytes, N, H, D, need);
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, keep, scores_out, keep_idx, next_scores, dtype, (hipStream_t)stream,
                             num_prefix, need ? workspace : nullptr, need ? workspace_bytes : 0, RAJNI_QUERY_CLS, prefix_q, prefix_qk,
                             num_prefix);
}

// rajni_attention limited to the query rows [0, nq) (include/rajni_hip_debug.h)
extern "C" int rajni_debug_attention_rows(const void* qkv, const int32_t* keep_idx, void* out, int B, int n_src, int np, int nq,
                                          int H, int D, float scale, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_debug_attention_rows");
  RAJNI_REQUIRE_PLACED("rajni_attention", {"qkv", qkv, 16}, {"keep_idx", keep_idx, 4}, {"out", out, 16});
  return launch_attention(qkv, keep_idx, out, B, n_src, np, nq, H, D, scale, dtype, (hipStream_t)stream);
}

extern "C" int rajni_attention_fp8(const void* qkv, const int32_t* keep_idx, void* out_q, float out_scale, float* row_scale,
                                   int B, int n_src, int np, int H, int D, float scale, rajni_stream_t stream) {
  RAJNI_REQUIRE_PLACED("rajni_attention_fp8", {"qkv", qkv, 16}, {"keep_idx", keep_idx, 4}, {"out_q", out_q, 16}, {"row_scale", row_scale, 4});
  return launch_attention_fp8(qkv, keep_idx, out_q, out_scale, row_scale, B, n_src, np, H, D, scale, (hipStream_t)stream);
}

int rajni_layernorm(const void* x, long x_row_stride, const float* w, const float* b, void* y,
                    int rows, int C, float eps, int dtype, int x_f32, rajni_stream_t stream) {
  NEED_DTYPE("rajni_layernorm");
  RAJNI_REQUIRE_PLACED("rajni_layernorm", {"x", x, 16}, {"w", w, 16}, {"b", b, 16}, {"y", y, 16});
  return launch_layernorm(x, x_row_stride, w, b, y, rows, C, eps, x_f32, dtype, (hipStream_t)stream);
}

int rajni_norm_rows(int kind, const void* x, long x_row_stride, const float* w, const float* b, void* y, int rows, int C,
                    float eps, int dtype, int x_f32, rajni_stream_t stream) {
  NEED_DTYPE("rajni_norm_rows");
  RAJNI_REQUIRE_PLACED("rajni_norm_rows", {"x", x, 16}, {"w", w, 16}, {"b", b, 16}, {"y", y, 16});
  return launch_layernorm(x, x_row_stride, w, b, y, rows, C, eps, x_f32, dtype, (hipStream_t)stream, kind);
}

int rajni_embed_norm(int kind, void* x, const float* w, const float* b, const void* pos, int pos_off, int B, int N,
                     int num_prefix, int C, float eps, int dtype, int x_f32, rajni_stream_t stream) {
  NEED_DTYPE("rajni_embed_norm");
  RAJNI_REQUIRE_PLACED("rajni_embed_norm", {"x", x, 16}, {"w", w, 16}, {"b", b, 16}, {"pos", pos, 16});
  return launch_embed_norm(kind, x, w, b, pos, pos_off, B, N, num_prefix, C, eps, dtype, x_f32, (hipStream_t)stream);
}

int rajni_layernorm_fp8(const void* x, long x_row_stride, const float* w, const float* b, void* y_q,
                        float* y_scale, float* hid_scale, float w1_rownorm_max, float b1_absmax,
                        int rows, int C, float eps, int x_f32, rajni_stream_t stream) {
  RAJNI_REQUIRE_PLACED("rajni_layernorm_fp8", {"x", x, 16}, {"w", w, 16}, {"b", b, 16}, {"y_q", y_q, 16}, {"y_scale", y_scale, 4},
                       {"hid_scale", hid_scale, 4});
  return launch_layernorm_fp8(x, x_row_stride, w, b, y_q, y_scale, hid_scale, w1_rownorm_max, b1_absmax, rows, C, eps,
                              x_f32, (hipStream_t)stream);
}

int rajni_qk_norm(void* qkv, const float* q_w, const float* q_b, const float* k_w, const float* k_b, int rows, int H,
                  int D, float eps, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_qk_norm");
  RAJNI_REQUIRE_PLACED("rajni_qk_norm", {"qkv", qkv, 16}, {"q_w", q_w, 16}, {"q_b", q_b, 16}, {"k_w", k_w, 16}, {"k_b", k_b, 16});
  return launch_qk_norm(qkv, q_w, q_b, k_w, k_b, rows, H, D, eps, dtype, (hipStream_t)stream);
}

int rajni_layernorm_stream(void* x, const float* w, const float* b, int rows, int C, float eps, int dtype, int x_f32,
                           rajni_stream_t stream) {
  NEED_DTYPE("rajni_layernorm_stream");
  RAJNI_REQUIRE_PLACED("rajni_layernorm_stream", {"x", x, 16}, {"w", w, 16}, {"b", b, 16});
  return launch_layernorm_stream(x, w, b, rows, C, eps, x_f32, dtype, (hipStream_t)stream);
}

int rajni_pool_norm(const void* x, int B, int N, int C, int pool, const float* norm_w, const float* norm_b,
                    float norm_eps, const float* fc_w, const float* fc_b, float fc_eps, void* out, int dtype, int x_f32,
                    rajni_stream_t stream) {
  NEED_DTYPE("rajni_pool_norm");
  RAJNI_REQUIRE_PLACED("rajni_pool_norm", {"x", x, 16}, {"norm_w", norm_w, 16}, {"norm_b", norm_b, 16}, {"fc_w", fc_w, 16},
                       {"fc_b", fc_b, 16}, {"out", out, 16});
  return launch_pool_norm(x, B, N, C, pool, norm_w, norm_b, norm_eps, fc_w, fc_b, fc_eps, out, x_f32, dtype, (hipStream_t)stream);
}

int rajni_pool_norm_prefix(const void* x, int B, int N, int num_prefix, int C, int pool, const float* norm_w,
                           const float* norm_b, float norm_eps, const float* fc_w, const float* fc_b, float fc_eps,
                           void* out, int dtype, int x_f32, rajni_stream_t stream) {
  NEED_DTYPE("rajni_pool_norm_prefix");
  RAJNI_REQUIRE_PLACED("rajni_pool_norm_prefix", {"x", x, 16}, {"norm_w", norm_w, 16}, {"norm_b", norm_b, 16}, {"fc_w", fc_w, 16},
                       {"fc_b", fc_b, 16}, {"out", out, 16});
  RAJNI_REQUIRE(x && out, RAJNI_ERR_INVALID, "rajni_pool_norm_prefix: null pointer");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_pool_norm_prefix: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(pool != RAJNI_POOL_AVG || N >= num_prefix + 1, RAJNI_ERR_INVALID,
                "rajni_pool_norm_prefix: 'avg' needs at least one patch token (N=%d num_prefix=%d)", N, num_prefix);
  return launch_pool_norm(x, B, N, C, pool, norm_w, norm_b, norm_eps, fc_w, fc_b, fc_eps, out, x_f32, dtype,
                          (hipStream_t)stream, num_prefix);
}

int rajni_linear(const rajni_linear_args* args, rajni_stream_t stream) {
  RAJNI_REQUIRE(args != nullptr, RAJNI_ERR_INVALID, "rajni_linear: null args");
  return launch_linear(*args, (hipStream_t)stream);
}

int rajni_patch_embed(const void* images, const void* w, const float* bias, const void* cls,
                      const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int S,
                      int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream) {
  NEED_DTYPE("rajni_patch_embed");
  RAJNI_REQUIRE_PLACED("rajni_patch_embed", {"images", images, 16}, {"w", w, 16}, {"bias", bias, 16}, {"cls", cls, 16}, {"pos", pos, 16},
                       {"x", x, 16}, {"workspace", workspace, 16});
  return launch_patch_embed(images, w, bias, cls, pos, pos_has_cls, x, x_f32, B, Cin, S, S, P, C, dtype,
                            workspace, workspace_bytes, (hipStream_t)stream);
}
int rajni_patch_embed_prefix(const void* images, const void* w, const float* bias, const void* cls, const void* reg,
                             int num_prefix, const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int S,
                             int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream) {
  NEED_DTYPE("rajni_patch_embed_prefix");
  RAJNI_REQUIRE_PLACED("rajni_patch_embed_prefix", {"images", images, 16}, {"w", w, 16}, {"bias", bias, 16}, {"cls", cls, 16},
                       {"reg", reg, 16}, {"pos", pos, 16}, {"x", x, 16}, {"workspace", workspace, 16});
  RAJNI_REQUIRE(images && w && cls && pos && x, RAJNI_ERR_INVALID, "rajni_patch_embed_prefix: null pointer");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_patch_embed_prefix: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(num_prefix == 1 || reg != nullptr, RAJNI_ERR_INVALID,
                "rajni_patch_embed_prefix: %d prefix tokens but reg is null", num_prefix);
  return launch_patch_embed(images, w, bias, cls, pos, pos_has_cls, x, x_f32, B, Cin, S, S, P, C, dtype,
                            workspace, workspace_bytes, (hipStream_t)stream, num_prefix, num_prefix > 1 ? reg : nullptr);
}
size_t rajni_patch_embed_workspace_bytes(int B, int Cin, int S, int P, int dtype) {
  return patch_embed_workspace_bytes(B, Cin, S, S, P, dtype);
}

// ---- include/rajni_hip_image.h
int rajni_patch_embed_image(const void* images, const void* w, const float* bias, const void* cls, const void* reg,
                            int num_prefix, const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int H, int W,
                            int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream) {
  NEED_DTYPE("rajni_patch_embed_image");
  RAJNI_REQUIRE_PLACED("rajni_patch_embed_image", {"images", images, 16}, {"w", w, 16}, {"bias", bias, 16}, {"cls", cls, 16},
                       {"reg", reg, 16}, {"pos", pos, 16}, {"x", x, 16}, {"workspace", workspace, 16});
  RAJNI_REQUIRE(images && w && cls && pos && x, RAJNI_ERR_INVALID, "rajni_patch_embed_image: null pointer");
  RAJNI_REQUIRE(num_prefix >= 1 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_patch_embed_image: num_prefix must be 1..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(num_prefix == 1 || reg != nullptr, RAJNI_ERR_INVALID,
                "rajni_patch_embed_image: %d prefix tokens but reg is null", num_prefix);
  return launch_patch_embed(images, w, bias, cls, pos, pos_has_cls, x, x_f32, B, Cin, H, W, P, C, dtype,
                            workspace, workspace_bytes, (hipStream_t)stream, num_prefix, num_prefix > 1 ? reg : nullptr);
}
size_t rajni_patch_embed_workspace_bytes_image(int B, int Cin, int H, int W, int P, int dtype) {
  return patch_embed_workspace_bytes(B, Cin, H, W, P, dtype);
}
int rajni_resample_pos_embed(const void* src, int src_h, int src_w, void* dst, int dst_h, int dst_w, int C, int prefix_rows,
                             int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_resample_pos_embed");
  RAJNI_REQUIRE_PLACED("rajni_resample_pos_embed", {"src", src, 16}, {"dst", dst, 16});
  return launch_resample_pos_embed(src, src_h, src_w, dst, dst_h, dst_w, C, prefix_rows, dtype, (hipStream_t)stream);
}

// ---- include/rajni_hip_query.h
int rajni_score_select_query(const void* qkv, int B, int N, int H, int D, float eps, int num_prefix, int keep, int query,
                             void* scores_out, int32_t* keep_idx, void* next_scores, int dtype, void* workspace,
                             size_t workspace_bytes, rajni_stream_t stream) {
  if (query == RAJNI_QUERY_CLS && num_prefix >= 1)   // the launches and the bits of rajni_score_select_ws
    return rajni_score_select_ws(qkv, B, N, H, D, eps, num_prefix, keep, scores_out, keep_idx, next_scores, dtype, workspace,
                                 workspace_bytes, stream);
  NEED_DTYPE("rajni_score_select_query");
  RAJNI_REQUIRE(query == RAJNI_QUERY_CLS || query == RAJNI_QUERY_MEAN, RAJNI_ERR_INVALID,
                "rajni_score_select_query: query must be RAJNI_QUERY_CLS or RAJNI_QUERY_MEAN (%d)", query);
  const size_t need = rajni_score_select_query_workspace_bytes(B, N, H, D, dtype, query);
  RAJNI_REQUIRE(B <= RAJNI_MAX_GRID_YZ || need == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_score_select_query: B=%d - one launch of the tiled path takes at most %d images (grid: token tiles x images)",
                B, RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE_PLACED("rajni_score_select_query", {"qkv", qkv, 16}, {"scores_out", scores_out, rajni_elem_bytes(dtype)},
                       {"keep_idx", keep_idx, 4}, {"next_scores", next_scores, rajni_elem_bytes(dtype)}, {"workspace", workspace, 256});
  RAJNI_REQUIRE(qkv != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_query: qkv is null");
  RAJNI_REQUIRE(num_prefix >= 0 && num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_score_select_query: num_prefix must be 0..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= num_prefix + 1 && N >= 2, RAJNI_ERR_INVALID,
                "rajni_score_select_query: need B > 0, at least one patch token and N >= 2 (B=%d N=%d num_prefix=%d)", B, N, num_prefix);
  RAJNI_REQUIRE(keep >= 0 && keep <= N - num_prefix, RAJNI_ERR_INVALID,
                "rajni_score_select_query: keep must be 0 (scores only) or 1..%d (%d)", N - num_prefix, keep);
  RAJNI_REQUIRE(keep == 0 || keep_idx != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_query: keep_idx is null with keep=%d", keep);
  RAJNI_REQUIRE(keep > 0 || scores_out != nullptr, RAJNI_ERR_INVALID, "rajni_score_select_query: scores_out is null with keep=0");
  RAJNI_REQUIRE(need == 0 || workspace != nullptr, RAJNI_ERR_INVALID,
                "rajni_score_select_query: workspace is null but N=%d H=%d D=%d needs %zu B (rajni_score_select_query_workspace_bytes)",
                N, H, D, need);
  RAJNI_REQUIRE(workspace_bytes >= need, RAJNI_ERR_INVALID,
                "rajni_score_select_query: workspace_bytes=%zu but N=%d H=%d D=%d needs %zu B", workspace_bytes, N, H, D, need);
  return launch_score_select(qkv, nullptr, B, N, H, D, eps, keep, scores_out, keep_idx, next_scores, dtype,
                             (hipStream_t)stream, num_prefix, need ? workspace : nullptr, need ? workspace_bytes : 0, query);
}

int rajni_select_topk_query(const void* scores, int B, int N, int num_prefix, int keep, int32_t* keep_idx, void* next_scores,
                            int dtype, rajni_stream_t stream) {
  if (num_prefix >= 1) return rajni_select_topk_prefix(scores, B, N, num_prefix, keep, keep_idx, next_scores, dtype, stream);
  NEED_DTYPE("rajni_select_topk_query");
  RAJNI_REQUIRE_PLACED("rajni_select_topk_query", {"scores", scores, rajni_elem_bytes(dtype)}, {"keep_idx", keep_idx, 4},
                       {"next_scores", next_scores, rajni_elem_bytes(dtype)});
  RAJNI_REQUIRE(scores && keep_idx, RAJNI_ERR_INVALID, "rajni_select_topk_query: null pointer");
  RAJNI_REQUIRE(num_prefix == 0, RAJNI_ERR_INVALID, "rajni_select_topk_query: num_prefix must be 0..%d (%d)", RAJNI_MAX_PREFIX, num_prefix);
  RAJNI_REQUIRE(B > 0 && N >= 2, RAJNI_ERR_INVALID, "rajni_select_topk_query: need B > 0 and N >= 2 (B=%d N=%d)", B, N);
  RAJNI_REQUIRE(keep >= 1 && keep <= N, RAJNI_ERR_INVALID, "rajni_select_topk_query: keep must be 1..%d (%d)", N, keep);
  return launch_score_select(nullptr, scores, B, N, 0, 0, 0.f, keep, nullptr, keep_idx, next_scores, dtype, (hipStream_t)stream, 0);
}

int rajni_patch_embed_query(const void* images, const void* w, const float* bias, const void* reg, int num_reg, const void* pos,
                            int pos_has_cls, void* x, int x_f32, int B, int Cin, int H, int W, int P, int C, int dtype,
                            void* workspace, size_t workspace_bytes, rajni_stream_t stream) {
  NEED_DTYPE("rajni_patch_embed_query");
  RAJNI_REQUIRE_PLACED("rajni_patch_embed_query", {"images", images, 16}, {"w", w, 16}, {"bias", bias, 16}, {"reg", reg, 16},
                       {"pos", pos, 16}, {"x", x, 16}, {"workspace", workspace, 16});
  RAJNI_REQUIRE(images && w && pos && x, RAJNI_ERR_INVALID, "rajni_patch_embed_query: null pointer");
  RAJNI_REQUIRE(num_reg >= 0 && num_reg <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "rajni_patch_embed_query: num_reg must be 0..%d (%d)", RAJNI_MAX_PREFIX, num_reg);
  RAJNI_REQUIRE((num_reg > 0) == (reg != nullptr), RAJNI_ERR_INVALID, "rajni_patch_embed_query: num_reg = %d but reg is %s", num_reg,
                reg ? "given" : "null");
  return launch_patch_embed(images, w, bias, nullptr, pos, pos_has_cls, x, x_f32, B, Cin, H, W, P, C, dtype, workspace,
                            workspace_bytes, (hipStream_t)stream, num_reg, reg, 0);
}

// ---- include/rajni_hip_attnpool.h
int rajni_attention_pool(const void* kv, const float* q, void* out, int B, int N, int H, int D, int dtype, rajni_stream_t stream) {
  NEED_DTYPE("rajni_attention_pool");
  RAJNI_REQUIRE_PLACED("rajni_attention_pool", {"kv", kv, 16}, {"q", q, 16}, {"out", out, 16});
  return launch_attention_pool(kv, q, out, B, N, H, D, dtype, (hipStream_t)stream);
}

void rajni_profile_enable(unsigned mask) { g_prof_mask = mask; }
const char* rajni_profile_class_name(int k) {
  return (k >= 0 && k < RAJNI_NUM_KCLASS) ? kNames[k] : "";
}
void rajni_profile_reset(void) {
  for (auto& r : g_pending) { (void)hipEventSynchronize(r.e1); g_pool.push_back(r.e0); g_pool.push_back(r.e1); }
  g_pending.clear();
  for (int i = 0; i < RAJNI_NUM_KCLASS; ++i) { g_launches[i] = 0; g_ms[i] = g_flops[i] = g_bytes[i] = 0.0; }
}
int rajni_profile_collect(long long* launches, double* ms, double* flops, double* bytes) {
  for (auto& r : g_pending) {
    hipError_t e = hipEventSynchronize(r.e1);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, r.e0, r.e1);
    if (e != hipSuccess) {
      rajni_set_error("profile: %s", hipGetErrorString(e));
      return RAJNI_ERR_LAUNCH;
    }
    g_launches[r.kc] += 1; g_ms[r.kc] += t; g_flops[r.kc] += r.flops; g_bytes[r.kc] += r.bytes;
    g_pool.push_back(r.e0); g_pool.push_back(r.e1);
  }
  g_pending.clear();
  for (int i = 0; i < RAJNI_NUM_KCLASS; ++i) {
    if (launches) launches[i] = g_launches[i];
    if (ms) ms[i] = g_ms[i];
    if (flops) flops[i] = g_flops[i];
    if (bytes) bytes[i] = g_bytes[i];
  }
  return RAJNI_OK;
}

}  // extern "C"
