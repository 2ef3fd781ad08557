// Whole-forward orchestration: RAJNIViTWrapper.forward (reference model.py:30-69) as one host call
// that enqueues every kernel on the caller's stream.  Token counts are data independent,
// so all shapes are known up front: no allocation, no host sync, no device->host traffic inside.
//
// A call is a plan and up to nine optional records.  make_spec resolves them once into a Spec, and everything below takes that
// Spec: check_all (every refusal, before the first launch), carve (the workspace), the block loop and the tails.
//
// Per block:  LN1 -> QKV GEMM (all N tokens) -> an attention form -> the tail (launch_tail):
// proj GEMM whose epilogue gathers the residual row, applies LayerScale and adds -> LN2 -> FC1 GEMM + GELU ->
// FC2 GEMM + LayerScale + residual (in place).  The attention form is one of
//   [score+select] -> attention on the kept tokens (gather fused into its loads), all rows;
//   the first query tile of that attention, tail on the B CLS rows (last block, the same bits: last_block_cls_rows);
//   the same tile, its rows 0 and 1 gathered dense, tail on those 2B rows (last block of a distilled model, HR == 2);
//   the CLS-query kernel, tail on the B CLS rows (last block, the cls_only_last_block opt-in);
// and hands the tail an AttnRows record.  The reference's three gathers (qkv, scores, x) never exist as kernels here.
// With plan.act_fp8 (opt-in): LN1 / LN2 emit per-row-scaled e4m3 rows, QKV / FC1 / FC2 run on the fp8 matrix pipe
// (gemm_f8.h) and FC1's GELU epilogue re-quantises the hidden activations; where attention emits e4m3 rows
// (attn_emits_e4m3) proj runs there too.  The residual stream, patch embed and head are unchanged.
//
// Behind the last block, one of the tails:
//   final norm of the rows the head reads -> pool -> fc_norm -> head GEMM.  A headless plan (head_w NULL, num_classes 0) stops
//     in front of the GEMM and lets the norm launch write the caller's buffer;
//   the token outputs of a headless plan: RAJNI_POOL_NONE normalises every surviving row into the caller's buffer, and
//     RAJNI_POOL_DENSE / _DENSE_LAST scatter them back to the unpruned sequence (source_idx_kernel + layernorm_dense_kernel);
//   the attention pool (launch_pool_tail): final norm on every surviving row -> kv GEMM -> launch_attention_pool -> proj, the
//     pool's LayerNorm, FC1 + act and FC2 + residual on B rows in fp32 -> fc_norm or one rounding to the model dtype -> head.
//
// What each record changes (a NULL record changes no launch): ext - q/k-norm behind QKV, norm_pre behind the embedding, FC1's
// epilogue, and which tail runs; RAJNI_POOL_DENSE_LAST also sends the rows each scheduled block drops through the final norm to
// their source rows, behind that block's tail.  prefix - P prefix tokens (never pruned) instead of the class token alone, and
// with head_rows 2 the distilled head.  layers - behind a captured block the stream goes to that block's slab on the unpruned
// grid, and with fill = 1 every scheduled block writes the rows it drops to the slabs of all captures at or behind it.  image -
// n0 = (height / patch) * (width / patch) + P tokens, and plan.pos_embed holds the rows of that grid.  query - the importance
// query of the scoring blocks and whether there is a class row; without one P counts the registers alone and the last block
// runs every row.  pool - the attention-pool tail and its B fp32 rows, carved behind everything else.  norm - with kind RMS every
// norm launch is the RMS form of the same kernel; with an embedding norm the patch GEMM adds a zeroed position table and
// launch_embed_norm follows it (rajni_hip_norm.h).  rope - every block rotates q and k in place behind q/k-norm, in front of
// everything that reads w.qkv, by the table row of each token's place in the image; behind a scheduled block that place comes
// from the composed selections in w.rsrc (rajni_hip_rope.h).  mln - every block's tail normalises the first mln->n columns of
// w.hid in place between FC1 and FC2 (rajni_hip_mlpnorm.h).  relpos - every attention launch adds block i's relative position
// bias to its logits and every scoring launch the class row's; the place of each packed row in the image comes from the composed
// selections in w.bsrc, this block's included (rajni_hip_relpos.h).
#include "common.h"

#include <vector>

namespace {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int RAJNI_IMAGE_MAX_TOKENS = 16384 + RAJNI_MAX_PREFIX;   // ST_MAX_N of score_select.hip: the score path's cap

struct Workspace {
  char *xa, *xb, *xn, *qkv, *att, *hid, *clsn, *scf, *cols;
  int32_t* idx01;          // head_rows == 2: [B, 2] = {0, 1} per image, the selection that names the two rows the head reads
  char* sst; size_t sst_bytes;   // scratch of the tiled score kernels: zero bytes wherever one workgroup holds (n0, H, D)
  float *xs, *hs;          // act_fp8 plans: per-row scales of the e4m3 LayerNorm output / MLP hidden activations
  // the B-row intermediates of the attention-pool tail (rajni_hip_attnpool.h), behind everything above: po [B, C] the pool
  // kernel's output, py [B, C] proj's output and the MLP's residual stream (FC2 adds in place), pn [B, C] the pool LayerNorm's
  // rows, phid [B, pool.hidden] - all fp32 whatever the plan's dtype: the B-row part of the tail runs in fp32
  char *po, *py, *pn, *phid;
  int32_t* rsrc;           // a rope record: [B, n0] = where each token of the stream sat in the unpruned sequence (w.qkv is live there)
  int32_t* bsrc;           // a relpos record: [B, n0] = where each packed row of the attention (behind the block's own selection) sat
  size_t total, cols_bytes;
};

// One call, resolved: the plan, the optional records beside it (NULL: absent) and every fact derived from them, each computed
// here once with the NULL defaults applied.  make_spec follows no pointer a refusal has yet to vouch for; `w` is carved by
// check_all behind every other refusal, since the workspace size is the last of them.
struct Spec {
  const char* who;                  // the entry point a prefix refusal names: that of the widest record present
  const rajni_vit_plan* p;
  const rajni_vit_ext* ext; const rajni_vit_prefix* pre; const rajni_vit_layers* lay; const rajni_vit_image* img;
  const rajni_vit_query* qry;       // {1, RAJNI_QUERY_CLS} arrives here as NULL
  const rajni_vit_attn_pool* ap;
  const rajni_vit_norm* nrm;        // all zero arrives here as NULL
  int kind;                         // every norm of the forward but q/k-norm: RAJNI_NORM_LAYERNORM without the record
  bool rms, embed_norm;             // kind == RAJNI_NORM_RMS; the record carries a patch_embed.norm
  const rajni_vit_rope* rop;        // all zero arrives here as NULL
  const rajni_vit_mlp_norm* mln;    // all zero arrives here as NULL
  const rajni_vit_relpos* rel;      // all zero arrives here as NULL
  hipStream_t s;
  bool nocls;                       // no class row: the prefix tokens are the registers alone
  int qmode;                        // the importance query of the scoring blocks
  int has_cls, P, HR;               // class rows (0 / 1); prefix tokens, never pruned; rows of each image the head reads (1 / 2)
  int height, width, n0;            // the input in pixels; tokens entering block 0, prefix tokens included
  int pool;                         // ext.pool (RAJNI_POOL_TOKEN without ext)
  bool dense_last, norm_absent;
  const void* reg_token;            // the registers (or the dist token) the patch embed writes behind the class row, or NULL
  int fc1_epi, sf32;                // FC1's epilogue (ext.mlp_act); 16-bit model with an fp32 residual stream
  const rajni_qk_affine* qk_norm;
  bool last_captured;               // the layers record captures the last block
  size_t slab_ld;                   // elements between two slabs of the layers record
  Workspace w;
};

enum { ENTRY_FORWARD = 0, ENTRY_SIZE = 1 };

Spec make_spec(int family, const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* pre,
               const rajni_vit_layers* lay, const rajni_vit_image* img, const rajni_vit_query* qry, const rajni_vit_attn_pool* ap,
               hipStream_t s, const rajni_vit_norm* nrm = nullptr, const rajni_vit_rope* rop = nullptr,
               const rajni_vit_mlp_norm* mln = nullptr, const rajni_vit_relpos* rel = nullptr) {
  // a NULL trailing record makes a call the next-narrower entry point's, by name too (the size of a pool record is the query
  // size function's plus the pool rows, and there is no size function for a layers record)
  static const char* const names[2][9] = {
      {"rajni_vit_forward_ext_prefix", "rajni_vit_forward_layers", "rajni_vit_forward_image", "rajni_vit_forward_query",
       "rajni_vit_forward_pool", "rajni_vit_forward_norm", "rajni_vit_forward_rope", "rajni_vit_forward_mlpnorm",
       "rajni_vit_forward_relpos"},
      {"rajni_vit_workspace_bytes_prefix", "rajni_vit_workspace_bytes_prefix", "rajni_vit_workspace_bytes_image",
       "rajni_vit_workspace_bytes_query", "rajni_vit_workspace_bytes_query", "rajni_vit_workspace_bytes_norm",
       "rajni_vit_workspace_bytes_rope", "rajni_vit_workspace_bytes_mlpnorm", "rajni_vit_workspace_bytes_relpos"}};
  if (qry && qry->class_token == 1 && qry->query == RAJNI_QUERY_CLS) qry = nullptr;
  if (nrm && nrm->kind == RAJNI_NORM_LAYERNORM && !nrm->embed_norm_w) nrm = nullptr;   // what NULL means
  if (rop && !rop->cos && !rop->sin && !rop->head_stride && !rop->block_stride && !rop->rows && !rop->layout) rop = nullptr;
  if (mln && !mln->w && !mln->b && mln->eps == 0.f && !mln->n) mln = nullptr;
  if (rel && !rel->table && !rel->prefix_q && !rel->prefix_k && !rel->prefix_qk && !rel->block_stride && !rel->gh && !rel->gw) rel = nullptr;
  Spec c{};
  c.rop = rop; c.mln = mln; c.rel = rel;
  c.who = names[family][rel ? 8 : mln ? 7 : rop ? 6 : nrm ? 5 : (ap && family == ENTRY_FORWARD) ? 4 : qry ? 3 : img ? 2 : lay ? 1 : 0];
  c.p = plan; c.ext = ext; c.pre = pre; c.lay = lay; c.img = img; c.qry = qry; c.ap = ap; c.nrm = nrm; c.s = s;
  c.kind = nrm ? nrm->kind : RAJNI_NORM_LAYERNORM;
  c.rms = c.kind == RAJNI_NORM_RMS;
  c.embed_norm = nrm != nullptr && nrm->embed_norm_w != nullptr;
  c.nocls = qry != nullptr && qry->class_token == 0;
  c.qmode = qry ? qry->query : RAJNI_QUERY_CLS;
  c.has_cls = c.nocls ? 0 : 1;
  // NULL, 0 and 1 all mean CLS only; without a class row the record counts the registers alone
  c.P = c.nocls ? (pre ? pre->num_prefix : 0) : ((pre && pre->num_prefix > 1) ? pre->num_prefix : 1);
  // NULL, 0 and 1 all mean the CLS row; 2 is the distilled head (cls and dist rows); no class row, no head rows
  c.HR = (!c.nocls && pre && pre->head_rows == 2) ? 2 : 1;
  c.reg_token = c.P > c.has_cls ? pre->reg_token : nullptr;
  c.pool = ext ? ext->pool : RAJNI_POOL_TOKEN;
  c.dense_last = c.pool == RAJNI_POOL_DENSE_LAST;
  c.norm_absent = ext != nullptr && ext->norm_absent != 0;
  c.qk_norm = ext ? ext->qk_norm : nullptr;
  c.fc1_epi = (ext && ext->mlp_act == RAJNI_MLP_QUICK_GELU) ? RAJNI_EPI_BIAS_QUICK_GELU
              : (ext && ext->mlp_act == RAJNI_MLP_SWIGLU) ? RAJNI_EPI_BIAS_SWIGLU : RAJNI_EPI_BIAS_GELU;
  if (!plan) return c;
  const rajni_vit_plan& p = *plan;
  c.height = img ? img->height : p.img_size;   // NULL is the square image of plan.img_size pixels
  c.width = img ? img->width : p.img_size;
  // (check_image refuses a grid beyond the int range before anything reads n0)
  c.n0 = p.patch_size > 0 ? (int)((long long)(c.height / p.patch_size) * (c.width / p.patch_size) + c.P) : c.P;
  c.sf32 = (p.dtype != RAJNI_F32 && !p.resid_bf16) ? 1 : 0;
  c.last_captured = lay && lay->blocks && lay->n >= 1 && lay->n <= RAJNI_MAX_LAYERS && lay->blocks[lay->n - 1] == p.depth - 1;
  c.slab_ld = lay ? (lay->slab_stride ? (size_t)lay->slab_stride : (size_t)p.B * c.n0 * p.C) : 0;
  return c;
}

// the workspace and, with a pool record, the pool rows behind it: one layout, one total
Workspace carve(const Spec& c) {
  const rajni_vit_plan& p = *c.p;
  const int HR = c.HR;
  const size_t n0 = (size_t)c.n0;
  const size_t rows = (size_t)p.B * n0, es = p.dtype == RAJNI_F32 ? 4 : 2, xs = (p.dtype == RAJNI_F32 || !p.resid_bf16) ? 4 : 2;
  Workspace w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
  const size_t oxa = take(rows * p.C * xs), oxb = take(rows * p.C * xs), oxn = take(rows * p.C * es);
  const size_t oqkv = take(rows * 3 * p.C * es), oatt = take(rows * p.C * es);
  const size_t ohid = take(rows * p.hidden * es), ocls = take((size_t)p.B * HR * p.C * es);
  const size_t oscf = take(rows * es);
  w.cols_bytes = patch_embed_workspace_bytes(p.B, p.in_chans, c.height, c.width, p.patch_size, p.dtype);   // 0 when fused
  const size_t ocols = take(w.cols_bytes);
  const size_t oxs = take(p.act_fp8 ? rows * sizeof(float) : 0), ohs = take(p.act_fp8 ? rows * sizeof(float) : 0);
  w.sst_bytes = rajni_score_select_query_workspace_bytes(p.B, (int)n0, p.H, p.D, p.dtype, c.qmode);   // (CLS: rajni_score_select_workspace_bytes)
  const size_t osst = take(w.sst_bytes);
  const size_t oidx = take(HR == 2 ? (size_t)p.B * 2 * sizeof(int32_t) : 0);   // behind the rest: nothing above moves
  const size_t prow = c.ap ? (size_t)p.B * p.C * sizeof(float) : 0;            // the pool rows likewise
  const size_t opo = take(prow), opy = take(prow), opn = take(prow), oph = take(c.ap ? (size_t)p.B * c.ap->hidden * sizeof(float) : 0);
  const size_t orsrc = take(c.rop ? rows * sizeof(int32_t) : 0);               // and the rope record's source map
  const size_t obsrc = take(c.rel ? rows * sizeof(int32_t) : 0);               // and the relpos record's
  char* base = (char*)p.workspace;
  w.xa = base + oxa; w.xb = base + oxb; w.xn = base + oxn; w.qkv = base + oqkv; w.att = base + oatt;
  w.hid = base + ohid; w.clsn = base + ocls; w.scf = base + oscf; w.cols = base + ocols;
  w.sst = w.sst_bytes ? base + osst : nullptr;
  w.idx01 = HR == 2 ? reinterpret_cast<int32_t*>(base + oidx) : nullptr;
  w.xs = reinterpret_cast<float*>(base + oxs); w.hs = reinterpret_cast<float*>(base + ohs);
  w.po = base + opo; w.py = base + opy; w.pn = base + opn; w.phid = base + oph;
  w.rsrc = c.rop ? reinterpret_cast<int32_t*>(base + orsrc) : nullptr;
  w.bsrc = c.rel ? reinterpret_cast<int32_t*>(base + obsrc) : nullptr;
  w.total = off;
  return w;
}

// next_scores[b, j] = scores[b, idx[b, j]]   (attention.py:58) - used with a forced selection
template <typename T>
__global__ void carry_scores_kernel(const T* scores, const int* idx, T* out, int B, int N, int np) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * np) return;
  const int b = i / np;
  out[i] = scores[(long)b * N + idx[i]];
}

// idx[b, r] = r for r in {0, 1}: filled on the stream (capturable, no host copy)
__global__ void head_rows_idx_kernel(int* idx, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = i & 1;
}

// the placement contract (include/rajni_hip.h) for everything a plan points to, with images and logits
int check_placement(const rajni_vit_plan& p, const void* images, const void* logits) {
  const char* who = "rajni_vit_forward";
  const int eb = rajni_elem_bytes(p.dtype);
  RAJNI_REQUIRE_PLACED(who, {"images", images, 16}, {"logits", logits, 16}, {"patch_w", p.patch_w, 16}, {"patch_b", p.patch_b, 16},
                       {"cls_token", p.cls_token, 16}, {"pos_embed", p.pos_embed, 16}, {"norm_w", p.norm_w, 16}, {"norm_b", p.norm_b, 16},
                       {"head_w", p.head_w, 16}, {"head_b", p.head_b, 16}, {"workspace", p.workspace, 256});
  for (int i = 0; i < p.depth; ++i) {
    const rajni_block& k = p.blocks[i];
    char blk[48];
    snprintf(blk, sizeof(blk), "%s: block %d", who, i);
    RAJNI_REQUIRE_PLACED(blk, {"norm1_w", k.norm1_w, 16}, {"norm1_b", k.norm1_b, 16}, {"qkv_w", k.qkv_w, 16}, {"qkv_b", k.qkv_b, 16},
                         {"proj_w", k.proj_w, 16}, {"proj_b", k.proj_b, 16}, {"ls1", k.ls1, 16}, {"norm2_w", k.norm2_w, 16},
                         {"norm2_b", k.norm2_b, 16}, {"fc1_w", k.fc1_w, 16}, {"fc1_b", k.fc1_b, 16}, {"fc2_w", k.fc2_w, 16},
                         {"fc2_b", k.fc2_b, 16}, {"ls2", k.ls2, 16}, {"keep_idx", k.keep_idx, 4}, {"scores", k.scores, eb},
                         {"next_scores", k.next_scores, eb}, {"forced_keep_idx", k.forced_keep_idx, 4}, {"qkv_s", k.qkv_s, 16},
                         {"proj_s", k.proj_s, 16}, {"fc1_s", k.fc1_s, 16}, {"fc2_s", k.fc2_s, 16});
  }
  return RAJNI_OK;
}

// no head: the buffer passed as `logits` receives the row the head would have read, or the tokens (RAJNI_POOL_NONE / _DENSE /
// _DENSE_LAST)
inline bool headless(const rajni_vit_plan& p) { return p.head_w == nullptr && p.num_classes == 0; }
inline bool pool_is_tokens(const rajni_vit_ext* e) {
  return e && (e->pool == RAJNI_POOL_NONE || e->pool == RAJNI_POOL_DENSE || e->pool == RAJNI_POOL_DENSE_LAST);
}

int check_plan(const Spec& c) {
  const rajni_vit_plan& p = *c.p;
  RAJNI_REQUIRE(p.dtype == RAJNI_BF16 || p.dtype == RAJNI_F32 || p.dtype == RAJNI_F16, RAJNI_ERR_INVALID,
                "rajni_vit_forward: bad dtype %d", p.dtype);
  RAJNI_REQUIRE(p.B > 0 && p.depth > 0 && p.blocks != nullptr, RAJNI_ERR_INVALID, "rajni_vit_forward: bad plan");
  // every block's attention puts the image index on a grid axis: refuse here, not in the middle of the forward
  RAJNI_REQUIRE(p.B <= RAJNI_MAX_GRID_YZ, RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: B=%d - one forward takes at most %d images (split the batch: images are independent)", p.B,
                RAJNI_MAX_GRID_YZ);
  RAJNI_REQUIRE(p.C == p.H * p.D && p.D >= 8 && p.D <= 128 && p.D % 8 == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: need C == H*D and a head dim that is a multiple of 8 up to 128 (C=%d H=%d D=%d)", p.C, p.H, p.D);
  RAJNI_REQUIRE(p.C % 64 == 0 && p.hidden % 64 == 0, RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: C and hidden must be multiples of 64");
  // a headless plan (head_w == NULL and num_classes == 0) is legal; half of that pair is a missing weight
  RAJNI_REQUIRE(p.patch_w && (p.cls_token || c.nocls) && p.pos_embed && (p.head_w != nullptr) == (p.num_classes != 0) &&
                    (c.norm_absent || (p.norm_w && (p.norm_b || c.rms))),
                RAJNI_ERR_INVALID, "rajni_vit_forward: null weight pointer");
  RAJNI_REQUIRE(!(headless(p) && p.act_fp8), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: a headless plan (feature output) is unsupported with act_fp8");
  if (p.dtype == RAJNI_F16) {
    bool w8 = false;
    for (int i = 0; i < p.depth; ++i)
      w8 = w8 || p.blocks[i].qkv_s || p.blocks[i].proj_s || p.blocks[i].fc1_s || p.blocks[i].fc2_s;
    RAJNI_REQUIRE(!w8 && !p.act_fp8, RAJNI_ERR_UNSUPPORTED,
                  "rajni_vit_forward: fp8 weights or activations need a bf16 model (dtype fp16 given)");
  }
  if (p.act_fp8) {
    RAJNI_REQUIRE(p.dtype == RAJNI_BF16, RAJNI_ERR_UNSUPPORTED, "rajni_vit_forward: act_fp8 needs a bf16 model");
    RAJNI_REQUIRE(p.C % 256 == 0 && p.hidden % 256 == 0 && p.C >= 512, RAJNI_ERR_UNSUPPORTED,
                  "rajni_vit_forward: act_fp8 needs C %% 256 == 0, C >= 512 and hidden %% 256 == 0 (C=%d hidden=%d)", p.C, p.hidden);
    for (int i = 0; i < p.depth; ++i)
      RAJNI_REQUIRE(p.blocks[i].qkv_s && p.blocks[i].fc1_s && p.blocks[i].fc2_s, RAJNI_ERR_INVALID,
                    "rajni_vit_forward: act_fp8 needs e4m3 qkv / fc1 / fc2 weights with scales (block %d)", i);
  }
  return RAJNI_OK;
}

// the ext record against the plan (RAJNI_POOL_MAP is an unknown value without a pool record)
int check_ext(const Spec& c) {
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_ext& e = *c.ext;
  // (RAJNI_POOL_NONE, RAJNI_POOL_DENSE and RAJNI_POOL_DENSE_LAST, the token outputs, are legal too - 4 is not; the wording of this
  // refusal is what callers match on)
  RAJNI_REQUIRE((e.pool >= RAJNI_POOL_TOKEN && e.pool <= RAJNI_POOL_DENSE) || e.pool == RAJNI_POOL_DENSE_LAST ||
                    (c.ap && e.pool == RAJNI_POOL_MAP), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward_ext: pool must be RAJNI_POOL_TOKEN or RAJNI_POOL_AVG (%d)%s", e.pool,
                e.pool == RAJNI_POOL_MAP ? " - RAJNI_POOL_MAP needs rajni_vit_forward_pool and its rajni_vit_attn_pool record" : "");
  RAJNI_REQUIRE(!(e.pool == RAJNI_POOL_AVG && p.cls_only_last_block), RAJNI_ERR_INVALID,
                "rajni_vit_forward_ext: 'avg' pooling with cls_only_last_block - that opt-in never forms the rows to be averaged");
  if (pool_is_tokens(&e)) {
    const char* name = e.pool == RAJNI_POOL_NONE ? "RAJNI_POOL_NONE" : e.pool == RAJNI_POOL_DENSE ? "RAJNI_POOL_DENSE" : "RAJNI_POOL_DENSE_LAST";
    RAJNI_REQUIRE(headless(p), RAJNI_ERR_UNSUPPORTED,
                  "rajni_vit_forward_ext: %s needs a headless plan (head_w NULL, num_classes 0) - per-token classification is "
                  "not implemented", name);
    RAJNI_REQUIRE(!e.fc_norm_w && !e.norm_absent, RAJNI_ERR_UNSUPPORTED,
                  "rajni_vit_forward_ext: %s needs the final norm and no fc_norm (fc_norm %s, norm %s) - there is no cast-only "
                  "row kernel yet", name, e.fc_norm_w ? "present" : "absent", e.norm_absent ? "absent" : "present");
    RAJNI_REQUIRE(!p.cls_only_last_block, RAJNI_ERR_INVALID,
                  "rajni_vit_forward_ext: %s with cls_only_last_block - that opt-in never forms the rows to be returned", name);
  }
  if (e.qk_norm)
    for (int i = 0; i < p.depth; ++i)
      RAJNI_REQUIRE(e.qk_norm[i].q_norm_w && e.qk_norm[i].k_norm_w, RAJNI_ERR_INVALID,
                    "rajni_vit_forward_ext: q/k-norm weights missing (block %d)", i);
  if (e.qk_norm)
    for (int i = 0; i < p.depth; ++i) {
      char blk[56];
      snprintf(blk, sizeof(blk), "rajni_vit_forward_ext: block %d", i);
      RAJNI_REQUIRE_PLACED(blk, {"q_norm_w", e.qk_norm[i].q_norm_w, 16}, {"q_norm_b", e.qk_norm[i].q_norm_b, 16},
                           {"k_norm_w", e.qk_norm[i].k_norm_w, 16}, {"k_norm_b", e.qk_norm[i].k_norm_b, 16});
    }
  RAJNI_REQUIRE_PLACED("rajni_vit_forward_ext", {"norm_pre_w", e.norm_pre_w, 16}, {"norm_pre_b", e.norm_pre_b, 16},
                       {"fc_norm_w", e.fc_norm_w, 16}, {"fc_norm_b", e.fc_norm_b, 16});
  // (RAJNI_MLP_SWIGLU, the gated FC1, is the third legal value; the wording of this refusal is what callers match on)
  RAJNI_REQUIRE(e.mlp_act == RAJNI_MLP_GELU || e.mlp_act == RAJNI_MLP_QUICK_GELU || e.mlp_act == RAJNI_MLP_SWIGLU, RAJNI_ERR_INVALID,
                "rajni_vit_forward_ext: mlp_act must be RAJNI_MLP_GELU or RAJNI_MLP_QUICK_GELU (%d)", e.mlp_act);
  RAJNI_REQUIRE(!(e.mlp_act == RAJNI_MLP_SWIGLU && p.act_fp8), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward_ext: a SwiGLU MLP (mlp_act) is unsupported with act_fp8 - the fp8 x fp8 FC1 epilogue and its "
                "hidden-activation bound are exact GELU only");
  RAJNI_REQUIRE(!(e.mlp_act != RAJNI_MLP_GELU && p.act_fp8), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward_ext: a QuickGELU MLP (mlp_act) is unsupported with act_fp8 - the fp8 x fp8 FC1 epilogue and its "
                "hidden-activation bound are exact GELU only");
  return RAJNI_OK;
}

// test hook (rajni_debug_set_last_block_all_rows): 1 = the last block runs every row, the reference's op graph row for row
int g_last_block_all_rows = 0;

// The head reads x[:, 0] only (model.py:65-66), so past the last block's K and V nothing but the CLS row of each image is
// observable.  When this holds for block i entering with N tokens, the block runs attention for the first query tile and
// proj / LN2 / FC1 / fc2 on the B CLS rows - the kernels of the all-rows form on fewer rows, hence the same bits (a row
// of an attention, LayerNorm or rajni_linear result does not depend on which other rows are in the launch).  Not for: a
// last block that prunes (its selection is part of the trace), an avg-pooled head (reads every row), act_fp8 plans and
// the cls_only_last_block opt-in (they keep the opt-in's own branch and numerics contract).  With the distilled head
// (head_rows == 2) the observable rows are 0 and 1 of each image, and the block runs on those 2B rows under the same test.
// Nor for a last block whose output the layers record captures: the slab reads every row.
// Nor for a sequence without a class row (rajni_hip_query.h): no head reads a single row of it.
inline bool last_block_cls_rows(const Spec& c, int i, int N) {
  const rajni_vit_plan& p = *c.p;
  return i == p.depth - 1 && p.blocks[i].keep == 0 && N > 1 && c.pool == RAJNI_POOL_TOKEN &&
         !p.act_fp8 && !p.cls_only_last_block && !g_last_block_all_rows && !c.last_captured && !c.nocls;
}

// y[M, N] = epi(x[M, K] wt[N, K]^T + bias), every operand dense
rajni_linear_args linear_args(int dtype, const void* x, const void* wt, const float* bias, const float* w_scale, void* y,
                              int M, int N, int K, int epilogue) {
  rajni_linear_args g{};
  g.dtype = dtype;
  g.x = x; g.lda = K; g.w = wt; g.ldw = K; g.bias = bias; g.w_scale = w_scale;
  g.y = y; g.ldc = N; g.M = M; g.N = N; g.K = K; g.epilogue = epilogue;
  return g;
}

// the rows a block's attention left in w.att for the tail, and the residual row of each
struct AttnRows {
  int M; long lda;                          // B * tokens rows of stride C, or the B CLS rows of stride C / N * C
  const float* x_scale;                     // e4m3 rows (launch_attention_fp8 wrote them): their scale, else null
  long ldr;                                 // residual: row stride in the stream before proj ...
  const int32_t* idx; int np, nsrc;         // ... and the selection it is gathered by (null: row m)
};

// norm1 + qkv on ALL N tokens (model.py:51, attention.py:21-22)
rajni_linear_args qkv_args(const Spec& f, const rajni_block& blk, int M) {
  rajni_linear_args g = linear_args(f.p->dtype, f.w.xn, blk.qkv_w, blk.qkv_b, blk.qkv_s, f.w.qkv, M, 3 * f.p->C, f.p->C, RAJNI_EPI_BIAS);
  if (f.p->act_fp8) g.x_scale = f.w.xs;
  return g;
}
// proj + (gathered) residual + LayerScale (attention.py:55-56, model.py:55-58): x -> y is the stream before / after
rajni_linear_args proj_args(const Spec& f, const rajni_block& blk, const AttnRows& r, const void* x, void* y) {
  rajni_linear_args g = linear_args(f.p->dtype, f.w.att, blk.proj_w, blk.proj_b, blk.proj_s, y, r.M, f.p->C, f.p->C, RAJNI_EPI_BIAS_RESID);
  g.lda = r.lda; g.x_scale = r.x_scale;
  g.gamma = blk.ls1; g.resid = x; g.ldr = r.ldr; g.stream_f32 = f.sf32;
  if (r.idx) { g.r_idx = r.idx; g.r_np = r.np; g.r_nsrc = r.nsrc; }
  return g;
}
// MLP (model.py:59): fc1 + GELU (or the QuickGELU / gated SwiGLU of ext.mlp_act: N = hidden is the OUTPUT width either way,
// the gated fc1_w has 2 * hidden rows); act_fp8: e4m3 in, e4m3 out (per-row scales)
rajni_linear_args fc1_args(const Spec& f, const rajni_block& blk, int M) {
  rajni_linear_args g = linear_args(f.p->dtype, f.w.xn, blk.fc1_w, blk.fc1_b, blk.fc1_s, f.w.hid, M, f.p->hidden, f.p->C, f.fc1_epi);
  if (f.p->act_fp8) { g.x_scale = f.w.xs; g.y_scale = f.w.hs; }
  return g;
}
// fc2 + LayerScale + residual, in place on the stream y
rajni_linear_args fc2_args(const Spec& f, const rajni_block& blk, int M, void* y) {
  rajni_linear_args g = linear_args(f.p->dtype, f.w.hid, blk.fc2_w, blk.fc2_b, blk.fc2_s, y, M, f.p->C, f.p->hidden, RAJNI_EPI_BIAS_RESID);
  if (f.p->act_fp8) g.x_scale = f.w.hs;
  g.gamma = blk.ls2; g.resid = y; g.ldr = f.p->C; g.stream_f32 = f.sf32;
  return g;
}

// LayerNorm of `rows` stream rows into w.xn; act_fp8 plans: e4m3 rows + their scales into w.xs, and with hs the hidden
// scale of the rows' MLP (norm2 only; norm1 passes null and zeros)
int layernorm(const Spec& f, const void* x, const float* g, const float* b, int rows, float* hs, float wnorm, float bmax) {
  const rajni_vit_plan& p = *f.p;
  if (p.act_fp8) return launch_layernorm_fp8(x, p.C, g, b, f.w.xn, f.w.xs, hs, wnorm, bmax, rows, p.C, p.ln_eps, f.sf32, f.s);
  return launch_layernorm(x, p.C, g, b, f.w.xn, rows, p.C, p.ln_eps, f.sf32, p.dtype, f.s, f.kind);
}

// act_fp8 plans: this block's attention over np tokens emits e4m3 rows + their (one) scale into w.xs - norm1's row scales
// there were consumed by QKV - wherever the persistent head-dim-64 kernel serves the launch (rajni_attention_fp8)
inline bool attn_emits_e4m3(const rajni_vit_plan& p, const rajni_block& blk, int np) {
  return p.act_fp8 && blk.attn_out_scale > 0.f && blk.proj_s != nullptr && p.D == 64 && np <= 224;
}

// everything of a block behind its attention: proj + residual -> LN2 -> fc1 + GELU -> fc2 + residual
struct Tail { rajni_linear_args proj, fc1, fc2; const float *mln_w, *mln_b; };   // mln_w: this block's norm between fc1 and fc2, or null
Tail tail_args(const Spec& f, const rajni_block& blk, const AttnRows& r, const void* x, void* y) {
  const long i = &blk - f.p->blocks;
  return Tail{proj_args(f, blk, r, x, y), fc1_args(f, blk, r.M), fc2_args(f, blk, r.M, y), f.mln ? f.mln->w[i] : nullptr,
              (f.mln && f.mln->b && !f.rms) ? f.mln->b[i] : nullptr};
}
// would rajni_linear take all three?  (the dry run: every refusal, no launch; 256 CUs - no refusal depends on the count)
bool tail_ok(const Tail& t) {
  rajni_linear_plan unused;
  return rajni_debug_linear_plan(&t.proj, 256, &unused) == RAJNI_OK && rajni_debug_linear_plan(&t.fc1, 256, &unused) == RAJNI_OK &&
         rajni_debug_linear_plan(&t.fc2, 256, &unused) == RAJNI_OK;
}
int launch_tail(const Spec& f, const rajni_block& blk, const Tail& t) {
  int rc = launch_linear(t.proj, f.s);
  if (rc != RAJNI_OK) return rc;
  rc = layernorm(f, t.proj.y, blk.norm2_w, blk.norm2_b, t.proj.M, f.w.hs, blk.fc1_rownorm_max, blk.fc1_bias_absmax);
  if (rc != RAJNI_OK) return rc;
  rc = launch_linear(t.fc1, f.s);
  if (rc != RAJNI_OK) return rc;
  if (t.mln_w) {   // the rows FC1 has just written, their first mln->n columns; the zero padding behind them stays
    rc = launch_hidden_norm(f.kind, f.w.hid, f.p->hidden, t.mln_w, t.mln_b, t.fc1.M, f.mln->n, f.mln->eps, f.p->dtype, 0, f.s);
    if (rc != RAJNI_OK) return rc;
  }
  return launch_linear(t.fc2, f.s);
}

// the prefix record on its own terms, under the name of the entry point the call came through
int check_prefix(const Spec& c) {
  const rajni_vit_prefix* pre = c.pre;
  const char* who = c.who;
  if (!pre) return RAJNI_OK;
  RAJNI_REQUIRE(pre->num_prefix >= 0 && pre->num_prefix <= RAJNI_MAX_PREFIX, RAJNI_ERR_INVALID,
                "%s: num_prefix must be 0..%d (%d)", who, RAJNI_MAX_PREFIX, pre->num_prefix);
  if (c.nocls) {   // the registers alone: reg_token [num_prefix, C]
    RAJNI_REQUIRE((pre->num_prefix > 0) == (pre->reg_token != nullptr), RAJNI_ERR_INVALID,
                  "%s: query.class_token = 0 with prefix.num_prefix = %d registers but reg_token is %s", who, pre->num_prefix,
                  pre->reg_token ? "given" : "null");
    RAJNI_REQUIRE(pre->head_rows == 0 || pre->head_rows == 1, RAJNI_ERR_INVALID,
                  "%s: prefix.head_rows = %d with query.class_token = 0 - a sequence without a class row has no head rows", who,
                  pre->head_rows);
    return RAJNI_OK;
  }
  RAJNI_REQUIRE(pre->num_prefix <= 1 || pre->reg_token != nullptr, RAJNI_ERR_INVALID,
                "%s: %d prefix tokens but reg_token is null", who, pre->num_prefix);
  RAJNI_REQUIRE(pre->num_prefix > 1 || pre->reg_token == nullptr, RAJNI_ERR_INVALID,
                "%s: reg_token given but num_prefix is %d", who, pre->num_prefix);
  RAJNI_REQUIRE(pre->head_rows >= 0 && pre->head_rows <= 2, RAJNI_ERR_INVALID, "%s: head_rows must be 0..2 (%d)", who, pre->head_rows);
  RAJNI_REQUIRE(pre->head_rows != 2 || pre->num_prefix == 2, RAJNI_ERR_INVALID,
                "%s: head_rows=2 (the distilled head reads the cls and dist rows) needs num_prefix == 2 (%d)", who, pre->num_prefix);
  return RAJNI_OK;
}

// the distilled head (head_rows == 2) against the plan and the ext record: it is norm -> rows 0 and 1 -> one linear layer
int check_head_rows(const Spec& c) {
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_ext* e = c.ext;
  if (c.HR != 2) return RAJNI_OK;
  RAJNI_REQUIRE(!headless(p), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: head_rows=2 with a headless plan - the two rows exist to feed the averaged heads");
  RAJNI_REQUIRE(!e || (e->pool == RAJNI_POOL_TOKEN && !e->fc_norm_w && !e->norm_absent), RAJNI_ERR_UNSUPPORTED,
                "rajni_vit_forward: head_rows=2 needs a token head behind the final norm (pool=%d, fc_norm %s, norm %s)", e->pool,
                e->fc_norm_w ? "present" : "absent", e->norm_absent ? "absent" : "present");
  RAJNI_REQUIRE(!p.cls_only_last_block, RAJNI_ERR_INVALID,
                "rajni_vit_forward: head_rows=2 with cls_only_last_block - that opt-in forms the CLS row only");
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED, "rajni_vit_forward: head_rows=2 is unsupported with act_fp8");
  return RAJNI_OK;
}

// the query record against the plan, the ext and the prefix record (rajni_hip_query.h): host-side integer tests, every refusal
// names its field
// (query_form: the record on its own terms - all a size function asks of it; the rest is what a missing class row rules out)
int query_form(const rajni_vit_query& q) {
  const char* who = "rajni_vit_forward_query";
  RAJNI_REQUIRE(q.class_token == 0 || q.class_token == 1, RAJNI_ERR_INVALID, "%s: query.class_token must be 0 or 1 (%d)", who, q.class_token);
  RAJNI_REQUIRE(q.query == RAJNI_QUERY_CLS || q.query == RAJNI_QUERY_MEAN, RAJNI_ERR_INVALID,
                "%s: query.query must be RAJNI_QUERY_CLS or RAJNI_QUERY_MEAN (%d)", who, q.query);
  RAJNI_REQUIRE(q.class_token || q.query == RAJNI_QUERY_MEAN, RAJNI_ERR_INVALID,
                "%s: query.query must be RAJNI_QUERY_MEAN with query.class_token = 0 - there is no class row to be the query", who);
  return RAJNI_OK;
}
int check_query(const Spec& c) {
  const char* who = "rajni_vit_forward_query";
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_ext* e = c.ext;
  const int rc = query_form(*c.qry);
  if (rc != RAJNI_OK || !c.nocls) return rc;
  RAJNI_REQUIRE(!p.cls_only_last_block, RAJNI_ERR_INVALID,
                "%s: plan.cls_only_last_block with query.class_token = 0 - there is no class row to form", who);
  // (RAJNI_POOL_MAP reads every row too; whether it is legal at this entry point is check_ext's to say)
  RAJNI_REQUIRE(e != nullptr && (e->pool == RAJNI_POOL_AVG || e->pool == RAJNI_POOL_MAP || pool_is_tokens(e)), RAJNI_ERR_INVALID,
                "%s: ext.pool must be RAJNI_POOL_AVG or a token output with query.class_token = 0 - a token head has no row to "
                "read (%s)", who, e ? "RAJNI_POOL_TOKEN" : "ext is NULL");
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED, "%s: plan.act_fp8 is unsupported with query.class_token = 0", who);
  return RAJNI_OK;
}

// the attention-pool record against the plan, the ext and the prefix record (rajni_hip_attnpool.h): host-side tests, every
// refusal names its field
inline bool pool_hidden_ok(const rajni_vit_attn_pool& ap) { return ap.hidden > 0 && ap.hidden % 64 == 0; }
int check_pool(const Spec& c) {
  const char* who = "rajni_vit_forward_pool";
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_ext* e = c.ext;
  const rajni_vit_attn_pool& ap = *c.ap;
  RAJNI_REQUIRE(e != nullptr && e->pool == RAJNI_POOL_MAP, RAJNI_ERR_INVALID,
                "%s: ext.pool must be RAJNI_POOL_MAP with a rajni_vit_attn_pool record (%s%d)", who, e ? "ext.pool = " : "ext is NULL: pool ",
                e ? e->pool : RAJNI_POOL_TOKEN);
  RAJNI_REQUIRE(!p.cls_only_last_block, RAJNI_ERR_INVALID,
                "%s: plan.cls_only_last_block with RAJNI_POOL_MAP - that opt-in never forms the rows to be pooled", who);
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED, "%s: plan.act_fp8 is unsupported with RAJNI_POOL_MAP", who);
  RAJNI_REQUIRE(c.HR != 2, RAJNI_ERR_UNSUPPORTED,
                "%s: prefix.head_rows = 2 with RAJNI_POOL_MAP - the two rows exist to feed the averaged token heads", who);
  RAJNI_REQUIRE(!e->norm_absent, RAJNI_ERR_UNSUPPORTED,
                "%s: ext.norm_absent with RAJNI_POOL_MAP - the pool reads norm(x), and there is no cast-only row kernel", who);
  const char* missing = !ap.q ? "q" : !ap.kv_w ? "kv_w" : !ap.proj_w ? "proj_w" : !ap.norm_w ? "norm_w" : !ap.norm_b ? "norm_b"
                        : !ap.fc1_w ? "fc1_w" : !ap.fc2_w ? "fc2_w" : nullptr;
  RAJNI_REQUIRE(missing == nullptr, RAJNI_ERR_INVALID, "%s: null weight pointer (pool.%s)", who, missing ? missing : "");
  RAJNI_REQUIRE(ap.heads > 0 && p.C > 0 && p.C % ap.heads == 0 && (p.C / ap.heads) % 8 == 0 && p.C / ap.heads >= 8 && p.C / ap.heads <= 128,
                RAJNI_ERR_INVALID, "%s: pool.heads must divide C into head dims that are multiples of 8 in 8..128 (heads=%d C=%d)", who,
                ap.heads, p.C);
  RAJNI_REQUIRE(pool_hidden_ok(ap), RAJNI_ERR_INVALID,
                "%s: pool.hidden must be a positive multiple of 64 (zero-pad the MLP width) (%d)", who, ap.hidden);
  RAJNI_REQUIRE(ap.act == RAJNI_MLP_GELU || ap.act == RAJNI_MLP_QUICK_GELU, RAJNI_ERR_INVALID,
                "%s: pool.act must be RAJNI_MLP_GELU or RAJNI_MLP_QUICK_GELU (%d)", who, ap.act);
  RAJNI_REQUIRE_PLACED("rajni_vit_forward_pool: pool", {"q", ap.q, 16}, {"kv_w", ap.kv_w, 16}, {"kv_b", ap.kv_b, 16}, {"proj_w", ap.proj_w, 16},
                       {"proj_b", ap.proj_b, 16}, {"norm_w", ap.norm_w, 16}, {"norm_b", ap.norm_b, 16}, {"fc1_w", ap.fc1_w, 16},
                       {"fc1_b", ap.fc1_b, 16}, {"fc2_w", ap.fc2_w, 16}, {"fc2_b", ap.fc2_b, 16});
  return RAJNI_OK;
}

// the norm record against the plan and the pool and layers records (rajni_hip_norm.h): host-side tests, every refusal names the
// combination
int check_norm(const Spec& c) {
  const char* who = "rajni_vit_forward_norm";
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_norm& n = *c.nrm;
  RAJNI_REQUIRE(n.kind == RAJNI_NORM_LAYERNORM || n.kind == RAJNI_NORM_RMS, RAJNI_ERR_INVALID,
                "%s: norm.kind must be RAJNI_NORM_LAYERNORM or RAJNI_NORM_RMS (%d)", who, n.kind);
  const char* what = c.rms ? "RMSNorm (norm.kind = RAJNI_NORM_RMS)" : "a patch-embedding norm (norm.embed_norm_w)";
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED,
                "%s: %s is unsupported with plan.act_fp8 - the e4m3-output norm kernels are LayerNorm only", who, what);
  RAJNI_REQUIRE(!c.ap, RAJNI_ERR_UNSUPPORTED,
                "%s: %s is unsupported with an attention-pool record (RAJNI_POOL_MAP) - that tail's norms are LayerNorm only", who, what);
  RAJNI_REQUIRE(!(c.rms && c.lay && c.lay->norm == 1), RAJNI_ERR_UNSUPPORTED,
                "%s: RMSNorm (norm.kind = RAJNI_NORM_RMS) with layers.norm = 1 - the normalised slabs are LayerNorm only; "
                "layers.norm = 0 gives the un-normalised states", who);
  RAJNI_REQUIRE(!c.embed_norm || (p.C > 0 && p.C % 8 == 0 && p.C <= 2048), RAJNI_ERR_UNSUPPORTED,
                "%s: a patch-embedding norm needs C %% 8 == 0, C <= 2048 (C=%d)", who, p.C);
  RAJNI_REQUIRE_PLACED("rajni_vit_forward_norm: norm", {"embed_norm_w", n.embed_norm_w, 16}, {"embed_norm_b", n.embed_norm_b, 16});
  return RAJNI_OK;
}

// the rope record against the plan and the grid (rajni_hip_rope.h): host-side integer tests, every refusal names the combination
int check_rope(const Spec& c) {
  const char* who = c.who;          // (a rope record is the widest there is: the rope entry point of the call's family)
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_rope& r = *c.rop;
  RAJNI_REQUIRE(r.layout == RAJNI_ROPE_INTERLEAVED || r.layout == RAJNI_ROPE_HALF, RAJNI_ERR_INVALID,
                "%s: rope.layout must be RAJNI_ROPE_INTERLEAVED or RAJNI_ROPE_HALF (%d)", who, r.layout);
  RAJNI_REQUIRE(r.cos && r.sin, RAJNI_ERR_INVALID, "%s: null pointer (rope.%s) with a non-zero rope record", who, r.cos ? "sin" : "cos");
  RAJNI_REQUIRE(p.patch_size > 0 && p.H > 0 && p.D > 0, RAJNI_ERR_INVALID, "%s: bad plan", who);
  RAJNI_REQUIRE(r.rows == c.n0 - c.P, RAJNI_ERR_INVALID,
                "%s: rope.rows must equal the patches of the grid, n0 - P = %d (%d): one table row per patch", who, c.n0 - c.P, r.rows);
  const long long table = (long long)r.rows * p.D;
  RAJNI_REQUIRE(r.head_stride == 0 || r.head_stride == table, RAJNI_ERR_INVALID,
                "%s: rope.head_stride must be 0 (one table for all heads) or rows * D = %lld (%lld)", who, table, r.head_stride);
  const long long per_block = (r.head_stride ? p.H : 1) * table;
  RAJNI_REQUIRE(r.block_stride == 0 || r.block_stride == per_block, RAJNI_ERR_INVALID,
                "%s: rope.block_stride must be 0 (one table for all blocks) or (head_stride ? H : 1) * rows * D = %lld (%lld)", who,
                per_block, r.block_stride);
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED,
                "%s: RoPE (a rope record) is unsupported with plan.act_fp8 - the e4m3 attention and its bounds were fitted to "
                "unrotated q and k", who);
  RAJNI_REQUIRE_PLACED("rajni_vit_forward_rope: rope", {"cos", r.cos, 16}, {"sin", r.sin, 16});
  return RAJNI_OK;
}

// the mlp-norm record against the plan (rajni_hip_mlpnorm.h): host-side tests, every refusal names the combination
int check_mlp_norm(const Spec& c) {
  const char* who = c.who;          // (an mlp-norm record is the widest there is: the mlpnorm entry point of the call's family)
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_mlp_norm& m = *c.mln;
  RAJNI_REQUIRE(m.n > 0 && m.n <= p.hidden, RAJNI_ERR_INVALID,
                "%s: mlp_norm.n must be the MLP width, 1..plan.hidden = %d (%d): plan.hidden is the zero-padded width", who, p.hidden,
                m.n);
  RAJNI_REQUIRE(m.n <= RAJNI_HIDDEN_NORM_MAX, RAJNI_ERR_UNSUPPORTED,
                "%s: mlp_norm.n = %d is over rajni_hidden_norm's cap of %d columns", who, m.n, RAJNI_HIDDEN_NORM_MAX);
  RAJNI_REQUIRE(m.w, RAJNI_ERR_INVALID, "%s: null pointer (mlp_norm.w) with a non-zero mlp_norm record", who);
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED,
                "%s: a norm inside the MLP (an mlp_norm record) is unsupported with plan.act_fp8 - FC1's e4m3 epilogue scales the "
                "hidden rows for FC2 before the norm could run", who);
  RAJNI_REQUIRE(p.depth > 0 && p.blocks, RAJNI_ERR_INVALID, "%s: bad plan", who);
  for (int i = 0; i < p.depth; ++i) {
    RAJNI_REQUIRE(m.w[i], RAJNI_ERR_INVALID, "%s: null pointer (mlp_norm.w[%d]) with a non-zero mlp_norm record", who, i);
    char blk[64];
    snprintf(blk, sizeof(blk), "rajni_vit_forward_mlpnorm: mlp_norm block %d", i);
    RAJNI_REQUIRE_PLACED(blk, {"w", m.w[i], 16}, {"b", m.b ? m.b[i] : nullptr, 16});
  }
  return RAJNI_OK;
}

// the relpos record against the plan, the grid and the other records (rajni_hip_relpos.h): host-side tests, every refusal names
// the combination
int check_relpos(const Spec& c) {
  const char* who = c.who;          // (a relpos record is the widest there is: the relpos entry point of the call's family)
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_relpos& r = *c.rel;
  RAJNI_REQUIRE(r.table && r.prefix_q && r.prefix_k && r.prefix_qk, RAJNI_ERR_INVALID,
                "%s: null pointer (relpos.%s) with a non-zero relpos record", who,
                !r.table ? "table" : !r.prefix_q ? "prefix_q" : !r.prefix_k ? "prefix_k" : "prefix_qk");
  RAJNI_REQUIRE(p.patch_size > 0 && p.H > 0 && p.D > 0, RAJNI_ERR_INVALID, "%s: bad plan", who);
  RAJNI_REQUIRE(r.gh >= 1 && r.gw >= 1, RAJNI_ERR_INVALID, "%s: relpos.gh and relpos.gw must be positive (%d x %d)", who, r.gh, r.gw);
  RAJNI_REQUIRE(r.gh <= RAJNI_RELPOS_MAX_GRID && r.gw <= RAJNI_RELPOS_MAX_GRID, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias on a %d x %d grid - the cap is %d x %d patches", who, r.gh, r.gw, RAJNI_RELPOS_MAX_GRID,
                RAJNI_RELPOS_MAX_GRID);
  RAJNI_REQUIRE(r.gh == c.height / p.patch_size && r.gw == c.width / p.patch_size, RAJNI_ERR_INVALID,
                "%s: relpos.gh x relpos.gw must equal the forward's patch grid, %d x %d (%d x %d)", who, c.height / p.patch_size,
                c.width / p.patch_size, r.gh, r.gw);
  const long long per_block = (long long)p.H * (2 * r.gh - 1) * (2 * r.gw - 1);
  RAJNI_REQUIRE(r.block_stride == 0 || r.block_stride == per_block, RAJNI_ERR_INVALID,
                "%s: relpos.block_stride must be 0 (one table for all blocks) or H * (2 gh - 1) * (2 gw - 1) = %lld (%lld)", who,
                per_block, r.block_stride);
  RAJNI_REQUIRE(p.D == 64, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias (a relpos record) with head dim %d - the bias kernels are head dim 64 only", who, p.D);
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias (a relpos record) is unsupported with plan.act_fp8 - the e4m3 attention and its "
                "bounds were fitted to logits without a bias", who);
  RAJNI_REQUIRE(!c.nocls && c.qmode == RAJNI_QUERY_CLS, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias (a relpos record) with %s - importance is scored on the class row's biased logits, "
                "and a mean query has no position", who, c.nocls ? "query.class_token = 0" : "the mean importance query (RAJNI_QUERY_MEAN)");
  RAJNI_REQUIRE(!c.rop, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias (a relpos record) together with RoPE (a rope record) - no model has both", who);
  RAJNI_REQUIRE(!p.cls_only_last_block, RAJNI_ERR_UNSUPPORTED,
                "%s: a relative position bias (a relpos record) with plan.cls_only_last_block - the CLS-query kernel of that "
                "opt-in takes no bias", who);
  RAJNI_REQUIRE(p.attn_scale > 0.f && p.attn_scale < INFINITY, RAJNI_ERR_INVALID,
                "%s: plan.attn_scale must be positive and finite with a relpos record (the bias is divided by it)", who);
  RAJNI_REQUIRE_PLACED("rajni_vit_forward_relpos: relpos", {"table", r.table, 4}, {"prefix_q", r.prefix_q, 4}, {"prefix_k", r.prefix_k, 4},
                       {"prefix_qk", r.prefix_qk, 4});
  return RAJNI_OK;
}

// the token walk (model.py:43,50): a scheduled block leaves its kept patch tokens and the P prefix tokens ...
inline int tokens_after(const rajni_block& blk, int N, int P) { return blk.keep > 0 ? blk.keep + P : N; }
// ... so this many enter block i
int tokens_entering(const Spec& c, int i) {
  int N = c.n0;
  for (int j = 0; j < i; ++j) N = tokens_after(c.p->blocks[j], N, c.P);
  return N;
}

inline int logits_stride(const rajni_vit_plan& p) { return p.logits_ld > 0 ? p.logits_ld : (headless(p) ? p.C : p.num_classes); }

// the pruning schedule and the logits stride: what the block loop and the head rely on, refused before anything is launched
int check_schedule(const Spec& c) {
  const rajni_vit_plan& p = *c.p;
  for (int i = 0; i < p.depth; ++i) {
    const rajni_block& blk = p.blocks[i];
    if (blk.keep <= 0) continue;
    const int patches = tokens_entering(c, i) - c.P;
    RAJNI_REQUIRE(blk.keep <= patches, RAJNI_ERR_INVALID, "block %d: keep=%d but only %d patch tokens", i, blk.keep, patches);
    RAJNI_REQUIRE(blk.keep_idx && blk.next_scores, RAJNI_ERR_INVALID, "block %d: keep_idx/next_scores buffers missing", i);
  }
  const int ld = logits_stride(p);
  RAJNI_REQUIRE(ld % 8 == 0 && ld >= p.num_classes, RAJNI_ERR_INVALID,
                "rajni_vit_forward: logits row stride must be a multiple of 8 and >= num_classes (%d)", ld);
  if (headless(p)) {
    // the final norm / pool_norm launch writes the caller's buffer directly, and those kernels write dense rows
    RAJNI_REQUIRE(ld >= p.C, RAJNI_ERR_INVALID, "rajni_vit_forward: a headless plan writes rows of C elements: logits row stride "
                  "must be >= C (%d < %d)", ld, p.C);
    RAJNI_REQUIRE(ld == p.C, RAJNI_ERR_UNSUPPORTED, "rajni_vit_forward: a headless plan writes dense rows: logits row stride "
                  "must be 0 or C (%d, C = %d)", ld, p.C);
  }
  return RAJNI_OK;
}

// RAJNI_POOL_DENSE_LAST: the refusals of a token output that check_plan, check_head_rows and check_schedule word without the
// pool, here under its name and with their codes
int check_dense_last(const Spec& c) {
  const char* who = "rajni_vit_forward_ext: RAJNI_POOL_DENSE_LAST";
  const rajni_vit_plan& p = *c.p;
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED, "%s is unsupported with act_fp8", who);
  RAJNI_REQUIRE(c.HR != 2, RAJNI_ERR_UNSUPPORTED,
                "%s with head_rows=2 - the two rows exist to feed the averaged heads, and a token output has no head", who);
  const int ld = p.logits_ld;
  RAJNI_REQUIRE(ld == 0 || (ld % 8 == 0 && ld >= p.C), RAJNI_ERR_INVALID,
                "%s: logits row stride must be a multiple of 8 and >= C (%d, C = %d)", who, ld, p.C);
  RAJNI_REQUIRE(ld == 0 || ld == p.C, RAJNI_ERR_UNSUPPORTED, "%s writes dense rows: logits row stride must be 0 or C (%d, C = %d)",
                who, ld, p.C);
  return RAJNI_OK;
}

// the layers record against the plan and the ext record (rajni_hip_layers.h): host-side integer tests, in front of every other
// refusal of the forward
int check_layers(const Spec& c) {
  const char* who = "rajni_vit_forward_layers";
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_layers& y = *c.lay;
  RAJNI_REQUIRE(y.n >= 1 && y.n <= RAJNI_MAX_LAYERS, RAJNI_ERR_INVALID, "%s: layers.n must be 1..%d (%d)", who, RAJNI_MAX_LAYERS, y.n);
  RAJNI_REQUIRE(y.blocks != nullptr && y.out != nullptr, RAJNI_ERR_INVALID, "%s: null pointer (layers.%s)", who,
                y.blocks ? "out" : "blocks");
  RAJNI_REQUIRE(p.depth > 0 && p.B > 0 && p.C > 0 && p.patch_size > 0 && p.img_size >= p.patch_size, RAJNI_ERR_INVALID, "%s: bad plan", who);
  for (int l = 0; l < y.n; ++l)
    RAJNI_REQUIRE(y.blocks[l] >= 0 && y.blocks[l] < p.depth && (l == 0 || y.blocks[l] > y.blocks[l - 1]), RAJNI_ERR_INVALID,
                  "%s: layers.blocks must be strictly ascending block indices in [0, %d) (blocks[%d] = %d)", who, p.depth, l, y.blocks[l]);
  RAJNI_REQUIRE(y.norm == 0 || y.norm == 1, RAJNI_ERR_INVALID, "%s: layers.norm must be 0 or 1 (%d)", who, y.norm);
  RAJNI_REQUIRE(y.fill == 0 || y.fill == 1, RAJNI_ERR_INVALID, "%s: layers.fill must be 0 (zero rows) or 1 (last state) (%d)", who, y.fill);
  const long long dense = (long long)p.B * c.n0 * p.C;
  RAJNI_REQUIRE(y.slab_stride == 0 || (y.slab_stride >= dense && y.slab_stride % 8 == 0), RAJNI_ERR_INVALID,
                "%s: layers.slab_stride must be 0 or a multiple of 8 that is >= B * (P + n) * C = %lld (%lld)", who, dense, y.slab_stride);
  RAJNI_REQUIRE_PLACED(who, {"layers.out", y.out, 16});
  RAJNI_REQUIRE(!(y.norm == 1 && c.norm_absent), RAJNI_ERR_UNSUPPORTED,
                "%s: layers.norm = 1 on a plan without a final norm (ext.norm_absent) - norm = 0 gives the un-normalised states", who);
  RAJNI_REQUIRE(!p.act_fp8, RAJNI_ERR_UNSUPPORTED, "%s is unsupported with act_fp8", who);
  RAJNI_REQUIRE(!(p.cls_only_last_block && y.blocks[y.n - 1] == p.depth - 1), RAJNI_ERR_INVALID,
                "%s: block %d captured with cls_only_last_block - that opt-in never forms the rows to be returned", who, p.depth - 1);
  return RAJNI_OK;
}

// the image record against the plan (rajni_hip_image.h): host-side integer tests, in front of every other refusal
int check_image(const Spec& c) {
  const char* who = "rajni_vit_forward_image";
  const rajni_vit_plan& p = *c.p;
  const rajni_vit_image& im = *c.img;
  RAJNI_REQUIRE(p.patch_size > 0, RAJNI_ERR_INVALID, "%s: bad plan (patch_size %d)", who, p.patch_size);
  RAJNI_REQUIRE(im.height > 0 && im.width > 0 && im.height % p.patch_size == 0 && im.width % p.patch_size == 0, RAJNI_ERR_INVALID,
                "%s: image.height and image.width must be positive multiples of the patch size %d (%d x %d)", who, p.patch_size,
                im.height, im.width);
  RAJNI_REQUIRE(p.img_size == im.height, RAJNI_ERR_INVALID, "%s: plan.img_size must equal image.height (%d != %d)", who, p.img_size,
                im.height);
  const long long n0 = (long long)(im.height / p.patch_size) * (im.width / p.patch_size) + c.P;   // (c.n0 is an int)
  RAJNI_REQUIRE(n0 <= RAJNI_IMAGE_MAX_TOKENS, RAJNI_ERR_UNSUPPORTED,
                "%s: N=%lld is beyond the tiled path's cap of %d tokens (%d x %d patches and %d prefix tokens)", who, n0,
                RAJNI_IMAGE_MAX_TOKENS, im.height / p.patch_size, im.width / p.patch_size, c.P);
  return RAJNI_OK;
}

// the attention-pool tail (rajni_hip_attnpool.h) on the final stream `cur` [B, N, C]: every launch but the pool kernel is one
// the blocks and the head use.  w.xn, w.qkv and w.att are dead behind the last block: B * N rows of C and of 2C <= 3C fit
int launch_pool_tail(const Spec& f, const void* cur, int N, void* logits) {
  const rajni_vit_plan& p = *f.p;
  const rajni_vit_attn_pool& ap = *f.ap;
  const rajni_vit_ext& e = *f.ext;   // (check_pool: there is one, and its pool is RAJNI_POOL_MAP)
  const int B = p.B, C = p.C, dt = p.dtype;
  int rc = launch_layernorm(cur, C, p.norm_w, p.norm_b, f.w.xn, B * N, C, p.ln_eps, f.sf32, dt, f.s);
  if (rc != RAJNI_OK) return rc;
  rc = launch_linear(linear_args(dt, f.w.xn, ap.kv_w, ap.kv_b, nullptr, f.w.qkv, B * N, 2 * C, C, RAJNI_EPI_BIAS), f.s);
  if (rc != RAJNI_OK) return rc;
  // From here on B rows, in fp32 whatever the model dtype (fp32 copies of proj / fc1 / fc2, the fp32 GEMMs and LayerNorm of an
  // fp32 model): each 16-bit rounding of a pooled row costs 0.2 - 0.4 % of the logit scale and there would be five of them
  // (DESIGN.md section 1, B7), while B rows cost next to nothing.  The pooled row is rounded ONCE, where the head reads it.
  rc = launch_attention_pool(f.w.qkv, ap.q, f.w.po, B, N, ap.heads, C / ap.heads, dt, f.s, 1);
  if (rc != RAJNI_OK) return rc;
  // y = proj(o), then y += fc2(act(fc1(norm(y)))) in place
  const int f32 = RAJNI_F32;
  rc = launch_linear(linear_args(f32, f.w.po, ap.proj_w, ap.proj_b, nullptr, f.w.py, B, C, C, RAJNI_EPI_BIAS), f.s);
  if (rc != RAJNI_OK) return rc;
  rc = launch_layernorm(f.w.py, C, ap.norm_w, ap.norm_b, f.w.pn, B, C, ap.norm_eps, 0, f32, f.s);
  if (rc != RAJNI_OK) return rc;
  rc = launch_linear(linear_args(f32, f.w.pn, ap.fc1_w, ap.fc1_b, nullptr, f.w.phid, B, ap.hidden, C,
                                 ap.act == RAJNI_MLP_QUICK_GELU ? RAJNI_EPI_BIAS_QUICK_GELU : RAJNI_EPI_BIAS_GELU), f.s);
  if (rc != RAJNI_OK) return rc;
  rajni_linear_args fc2 = linear_args(f32, f.w.phid, ap.fc2_w, ap.fc2_b, nullptr, f.w.py, B, C, ap.hidden, RAJNI_EPI_BIAS_RESID);
  fc2.resid = f.w.py; fc2.ldr = C;
  rc = launch_linear(fc2, f.s);
  if (rc != RAJNI_OK) return rc;
  // timm forward_head: fc_norm behind the pool, or none - rajni_pool_norm's token form on [B, 1, C] fp32 rows with no norm in
  // front: with fc_norm_w NULL it is the one rounding to the model dtype (the caller's buffer on a headless plan)
  void* const row = headless(p) ? logits : (void*)f.w.clsn;
  rc = launch_pool_norm(f.w.py, B, 1, C, RAJNI_POOL_TOKEN, nullptr, nullptr, 0.f, e.fc_norm_w, e.fc_norm_b, e.fc_norm_eps, row,
                        dt != RAJNI_F32, dt, f.s, 1);
  if (rc != RAJNI_OK) return rc;
  if (headless(p)) return RAJNI_OK;
  rajni_linear_args head = linear_args(dt, row, p.head_w, p.head_b, nullptr, logits, B, p.num_classes, C, RAJNI_EPI_BIAS);
  head.ldc = logits_stride(p);
  return launch_linear(head, f.s);
}

// src [B, Nf] = where each token of the stream that enters block `upto` (p.depth: the final stream) sat in the unpruned
// sequence: the selections of the scheduled blocks in front of it (the forced one where a block has it), last block first
int launch_source_idx_before(const Spec& c, int upto, int32_t* src, int Nf) {
  const rajni_vit_plan& p = *c.p;
  std::vector<const int32_t*> idx;
  std::vector<int> width, nsrc;
  for (int i = upto - 1; i >= 0; --i) {
    const rajni_block& blk = p.blocks[i];
    if (blk.keep <= 0) continue;
    idx.push_back(blk.forced_keep_idx ? blk.forced_keep_idx : blk.keep_idx);
    width.push_back(blk.keep + c.P);
    nsrc.push_back(tokens_entering(c, i));
  }
  return launch_source_idx(src, idx.data(), width.data(), nsrc.data(), (int)idx.size(), p.B, Nf, c.s);
}

// Every refusal of the forward, before the first launch.  The order is part of the contract - callers match the first message:
// the prefix record under the entry point's name; null pointers; the query record (whether there is a class row decides every
// count); the pool record; the norm record; the image record (every count below is against its grid); the rope record; the mlp-norm record; the layers
// record; then the plan, the
// placement of what it points to, the ext record, the distilled head, the schedule, and last the workspace, carved here.
int check_all(Spec& c, const void* images, const void* logits) {
  int rc = check_prefix(c);
  if (rc != RAJNI_OK) return rc;
  RAJNI_REQUIRE(c.p && images && logits, RAJNI_ERR_INVALID, "rajni_vit_forward: null pointer");
  const rajni_vit_plan& p = *c.p;
  if (c.qry && (rc = check_query(c)) != RAJNI_OK) return rc;
  if (c.ap && (rc = check_pool(c)) != RAJNI_OK) return rc;
  if (c.nrm && (rc = check_norm(c)) != RAJNI_OK) return rc;
  if (c.img && (rc = check_image(c)) != RAJNI_OK) return rc;
  if (c.rop && (rc = check_rope(c)) != RAJNI_OK) return rc;
  if (c.mln && (rc = check_mlp_norm(c)) != RAJNI_OK) return rc;
  if (c.rel && (rc = check_relpos(c)) != RAJNI_OK) return rc;
  if (c.lay && (rc = check_layers(c)) != RAJNI_OK) return rc;
  if (c.dense_last && (rc = check_dense_last(c)) != RAJNI_OK) return rc;
  if ((rc = check_plan(c)) != RAJNI_OK) return rc;
  if ((rc = check_placement(p, images, logits)) != RAJNI_OK) return rc;
  if (c.pre) RAJNI_REQUIRE_PLACED("rajni_vit_forward", {"reg_token", c.pre->reg_token, 16});
  if (c.ext && (rc = check_ext(c)) != RAJNI_OK) return rc;
  if ((rc = check_head_rows(c)) != RAJNI_OK) return rc;
  if ((rc = check_schedule(c)) != RAJNI_OK) return rc;
  c.w = carve(c);
  RAJNI_REQUIRE(p.workspace != nullptr && p.workspace_bytes >= c.w.total, RAJNI_ERR_INVALID,
                "rajni_vit_forward: workspace too small (%zu < %zu)", p.workspace_bytes, c.w.total);
  return RAJNI_OK;
}

// what the forward of this call needs in plan.workspace, 0 where the records that size it (prefix, image, query, pool) are
// refused: the same checks and the same carve as the forward's, so the two cannot disagree
size_t workspace_bytes(const Spec& c) {
  if (!c.p || c.p->patch_size <= 0) return 0;
  if (c.qry && query_form(*c.qry) != RAJNI_OK) return 0;
  if (check_prefix(c) != RAJNI_OK || (c.img && check_image(c) != RAJNI_OK)) return 0;
  if (c.ap && (!pool_hidden_ok(*c.ap) || c.p->B <= 0 || c.p->C <= 0)) return 0;
  if (c.nrm && check_norm(c) != RAJNI_OK) return 0;
  if (c.rop && check_rope(c) != RAJNI_OK) return 0;
  if (c.mln && check_mlp_norm(c) != RAJNI_OK) return 0;
  if (c.rel && check_relpos(c) != RAJNI_OK) return 0;
  return carve(c).total;
}

// the whole forward; NULL records and records that say what NULL means enqueue the same launches
int vit_forward(Spec f, const void* images, void* logits) {
  int rc = check_all(f, images, logits);
  if (rc != RAJNI_OK) return rc;
  const rajni_vit_plan& p = *f.p;
  const rajni_vit_ext* ext = f.ext;
  const rajni_vit_layers* lay = f.lay;
  const Workspace& w = f.w;
  hipStream_t s = f.s;
  const int B = p.B, C = p.C, dt = p.dtype, P = f.P, HR = f.HR, S0 = f.n0;
  int N = f.n0;

  // patch_embed.norm sits between the projection and the position embedding: the patch GEMM then adds a table whose patch rows
  // are zero and launch_embed_norm adds the real rows behind its norm.  The table lives in w.xb, idle until a block's tail writes
  // it ((P + n) * C elements of the model dtype fit in B times as many of the stream's); its prefix rows are the real ones, for
  // the kernel that writes the prefix rows
  const void* pos = p.pos_embed;
  const int poff = p.pos_has_cls ? P : 0;
  if (f.embed_norm) {
    const size_t rowb = (size_t)C * rajni_elem_bytes(dt);
    hipError_t e = poff ? hipMemcpyAsync(w.xb, p.pos_embed, poff * rowb, hipMemcpyDeviceToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(w.xb + poff * rowb, 0, (size_t)(N - P) * rowb, s);
    RAJNI_REQUIRE(e == hipSuccess, RAJNI_ERR_LAUNCH, "rajni_vit_forward_norm: zeroed position table: %s", hipGetErrorString(e));
    pos = w.xb;
  }
  rc = launch_patch_embed(images, p.patch_w, p.patch_b, p.cls_token, pos, p.pos_has_cls,
                          w.xa, f.sf32, B, p.in_chans, f.height, f.width, p.patch_size, C, dt, w.cols, w.cols_bytes, s,
                          P, f.reg_token, f.has_cls);
  if (rc != RAJNI_OK) return rc;
  if (f.embed_norm) {
    rc = launch_embed_norm(f.kind, w.xa, f.nrm->embed_norm_w, f.nrm->embed_norm_b, p.pos_embed, poff, B, N, P, C,
                           f.nrm->embed_norm_eps, dt, f.sf32, s);
    if (rc != RAJNI_OK) return rc;
  }
  if (ext && ext->norm_pre_w) {   // timm forward_features: x = norm_pre(x), written back into the stream
    rc = launch_layernorm_stream(w.xa, ext->norm_pre_w, ext->norm_pre_b, B * N, C, ext->norm_pre_eps, f.sf32, dt, s, f.kind);
    if (rc != RAJNI_OK) return rc;
  }

  if (HR == 2) {
    hipLaunchKernelGGL(head_rows_idx_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, s, w.idx01, 2 * B);
    RAJNI_CHECK_LAUNCH("head_rows_idx_kernel");
  }

  // the layers record: slab l is lay->out + l * slab_ld elements; `cap` walks the ascending capture list with the
  // block loop, so slabs [cap, n) are the ones a block at or in front of the next capture still writes to
  auto slab = [&](int l) { return static_cast<void*>(static_cast<char*>(lay->out) + (size_t)l * f.slab_ld * rajni_elem_bytes(dt)); };
  int cap = 0;

  char* cur = w.xa;
  char* oth = w.xb;
  const void* carried = nullptr;  // scores of the tokens currently in `cur` (model.py:39,53,63)
  // the rope record: w.rsrc names the place of every token of `cur` in the unpruned sequence once a scheduled block has run
  // (before that the place is the row index and the kernel gets no map); stale whenever a selection has changed the token set
  bool rope_mapped = false, rope_stale = false;
  // the relpos record: w.bsrc names the place of every packed row of the attention once a scheduled block has selected (its own
  // selection included); it stays good through the unscheduled blocks behind it, whose token set is the same
  const rajni_vit_relpos* rel = f.rel;
  bool rel_mapped = false;
  const int rel_gh = rel ? rel->gh : 0, rel_gw = rel ? rel->gw : 0;
  const float *rb_t = nullptr, *rb_q = nullptr, *rb_k = nullptr, *rb_qk = nullptr;   // block i's table and values
  // a block's attention over np rows gathered by idx from n_src, query rows [0, nq): with block i's bias where there is a record
  auto attend = [&](const int32_t* idx, void* out, int n_src, int np, int nq) {
    if (!rel) return launch_attention(w.qkv, idx, out, B, n_src, np, nq, p.H, p.D, p.attn_scale, dt, s);
    return launch_attention_relpos(w.qkv, idx, out, B, n_src, np, nq, p.H, p.D, p.attn_scale, dt, rb_t, rb_q, rb_k, rb_qk, rel_gh, rel_gw, P,
                                   rel_mapped ? w.bsrc : nullptr, s);
  };

  for (int i = 0; i < p.depth; ++i) {
    const rajni_block& blk = p.blocks[i];
    if (p.token_counts) p.token_counts[i] = N;  // model.py:43
    const int M = B * N;
    rc = layernorm(f, cur, blk.norm1_w, blk.norm1_b, M, nullptr, 0.f, 0.f);
    if (rc != RAJNI_OK) return rc;
    rc = launch_linear(qkv_args(f, blk, M), s);
    if (rc != RAJNI_OK) return rc;
    if (const rajni_qk_affine* qkn = f.qk_norm) {   // timm Attention.forward: q, k = q_norm(q), k_norm(k) - in place, so everything below reads normalised q and k
      rc = launch_qk_norm(w.qkv, qkn[i].q_norm_w, qkn[i].q_norm_b, qkn[i].k_norm_w, qkn[i].k_norm_b, M, p.H, p.D, ext->qk_eps, dt, s);
      if (rc != RAJNI_OK) return rc;
    }
    if (const rajni_vit_rope* rp = f.rop) {   // behind q/k-norm, in front of scoring, the last-block forms and attention
      if (rope_stale) {
        rc = launch_source_idx_before(f, i, w.rsrc, N);
        if (rc != RAJNI_OK) return rc;
        rope_stale = false; rope_mapped = true;
      }
      rc = launch_rope_qk(w.qkv, rope_mapped ? w.rsrc : nullptr, rp->cos + (size_t)i * rp->block_stride, rp->sin + (size_t)i * rp->block_stride,
                          (long)rp->head_stride, B, N, P, p.H, p.D, rp->layout, dt, s);
      if (rc != RAJNI_OK) return rc;
    }

    if (rel) {
      const size_t vo = rel->block_stride ? (size_t)i * p.H : 0;
      rb_t = rel->table + (size_t)i * rel->block_stride;
      rb_q = rel->prefix_q + vo; rb_k = rel->prefix_k + vo; rb_qk = rel->prefix_qk + vo;
    }

    // ---- the two CLS forms of the last block: only x[:, 0] reaches the head (model.py:65-66), so the tail runs on the B CLS
    //      rows - the residual row of image b is its CLS row, row b * N of `cur` - and leaves the stream [B, 1, C] in `oth`
    const long cls_ld = (long)N * C;
    if (p.cls_only_last_block && i == p.depth - 1 && blk.keep == 0 && N > 1) {
      // caller opted in: attention for the CLS query alone (over all N keys), a kernel of its own writing [B, C]
      // (an act_fp8 block whose all-rows form would emit e4m3 attention rows rounds the CLS row the same way)
      rc = launch_attention_cls(w.qkv, w.att, B, N, p.H, p.D, p.attn_scale, dt, s, attn_emits_e4m3(p, blk, N) ? blk.attn_out_scale : 0.f);
      if (rc != RAJNI_OK) return rc;
      rc = launch_tail(f, blk, tail_args(f, blk, AttnRows{B, C, nullptr, cls_ld, nullptr, 0, 0}, cur, oth));
      if (rc != RAJNI_OK) return rc;
      cur = oth; N = 1;
      break;
    }
    if (HR == 2 && last_block_cls_rows(f, i, N)) {
      // the distilled head reads rows 0 and 1: the first query tile (into w.xn, which QKV has consumed), its rows 0 and 1
      // gathered dense into w.att, and the ordinary tail as a pruned block that keeps {0, 1} - the proj epilogue gathers
      // the two residual rows through idx01 and the stream leaves [B, 2, C] in `oth`
      const Tail t = tail_args(f, blk, AttnRows{2 * B, C, nullptr, C, w.idx01, 2, N}, cur, oth);
      if (tail_ok(t)) {
        rc = attend(nullptr, w.xn, N, N, 2);
        if (rc != RAJNI_OK) return rc;
        rc = launch_gather_rows(w.xn, w.idx01, w.att, B, N, 2, C * rajni_elem_bytes(dt), s);
        if (rc != RAJNI_OK) return rc;
        rc = launch_tail(f, blk, t);
        if (rc != RAJNI_OK) return rc;
        cur = oth; N = 2;
        break;
      }
    } else if (last_block_cls_rows(f, i, N)) {
      // the all-rows kernels on the rows the head reads: the first query tile, proj on its CLS rows in place (stride N * C)
      const Tail t = tail_args(f, blk, AttnRows{B, cls_ld, nullptr, cls_ld, nullptr, 0, 0}, cur, oth);
      if (tail_ok(t)) {   // (a refused shape or stride: all rows below, as if this branch were not here)
        rc = attend(nullptr, w.att, N, N, 1);
        if (rc != RAJNI_OK) return rc;
        rc = launch_tail(f, blk, t);
        if (rc != RAJNI_OK) return rc;
        cur = oth; N = 1;
        break;
      }
    }

    const int Np = tokens_after(blk, N, P);
    const int32_t* idx = nullptr;
    if (blk.keep > 0) {  // scheduled block (model.py:50)
      const bool recompute = blk.update || carried == nullptr;  // attention.py:25
      if (blk.forced_keep_idx) {
        const void* full = carried;
        if (recompute) {
          void* dst = blk.scores ? blk.scores : (void*)w.scf;
          rc = launch_score_select(w.qkv, nullptr, B, N, p.H, p.D, 1e-6f, 0, dst, nullptr, nullptr, dt, s, f.nocls ? P : 1, w.sst, w.sst_bytes, f.qmode,
                                   rb_q, rb_qk, rel ? P : 0);
          if (rc != RAJNI_OK) return rc;
          full = dst;
        }
        const int n = B * Np;
        if (dt == RAJNI_F32)
          hipLaunchKernelGGL(carry_scores_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, s,
                             (const float*)full, blk.forced_keep_idx, (float*)blk.next_scores, B, N, Np);
        else   // (a 16-bit copy: serves fp16 scores too)
          hipLaunchKernelGGL(carry_scores_kernel<bf16_t>, dim3((n + 255) / 256), dim3(256), 0, s,
                             (const bf16_t*)full, blk.forced_keep_idx, (bf16_t*)blk.next_scores, B, N, Np);
        RAJNI_CHECK_LAUNCH("carry_scores_kernel");
        idx = blk.forced_keep_idx;
      } else {
        if (recompute)
          rc = launch_score_select(w.qkv, nullptr, B, N, p.H, p.D, 1e-6f, blk.keep, blk.scores,
                                   blk.keep_idx, blk.next_scores, dt, s, P, w.sst, w.sst_bytes, f.qmode, rb_q, rb_qk, rel ? P : 0);
        else
          rc = launch_score_select(nullptr, carried, B, N, 0, 0, 0.f, blk.keep, nullptr,
                                   blk.keep_idx, blk.next_scores, dt, s, P);
        if (rc != RAJNI_OK) return rc;
        idx = blk.keep_idx;
      }
      carried = blk.next_scores;  // attention.py:58,60
      if (rel) {   // the places of the Np rows this block's attention runs on
        rc = launch_source_idx_before(f, i + 1, w.bsrc, Np);
        if (rc != RAJNI_OK) return rc;
        rel_mapped = true;
      }
    } else {
      carried = nullptr;          // model.py:63
    }

    // ---- attention on the kept tokens, gather fused (attention.py:42-54)
    const bool att8 = attn_emits_e4m3(p, blk, Np);
    if (att8) rc = launch_attention_fp8(w.qkv, idx, w.att, blk.attn_out_scale, w.xs, B, N, Np, p.H, p.D, p.attn_scale, s);
    else rc = attend(idx, w.att, N, Np, Np);
    if (rc != RAJNI_OK) return rc;
    // a pruned block gathers its residual rows from `cur` into `oth`; an unpruned one runs proj in place (each element is
    // read and written by the same lane: in place is safe)
    char* y = idx ? oth : cur;
    rc = launch_tail(f, blk, tail_args(f, blk, AttnRows{B * Np, C, att8 ? w.xs : nullptr, C, idx, Np, N}, cur, y));
    if (rc != RAJNI_OK) return rc;
    // (slabs with fill = 1: the same rows, to every slab of a capture at or behind this block)
    const bool slabs_last = idx && lay && lay->fill == 1 && cap < lay->n;
    if (idx && (f.dense_last || slabs_last)) {
      // the rows this block drops leave the stream here and keep the state they entered with: `cur` still holds it (the tail
      // gathered the kept rows into `oth`).  Where each entering token sat in the unpruned sequence goes to w.qkv, dead
      // between the tail and the next block's QKV GEMM (B * N * 4 bytes always fit); then the final norm of the dropped rows
      int32_t* src = reinterpret_cast<int32_t*>(w.qkv);
      rc = launch_source_idx_before(f, i, src, N);
      if (rc != RAJNI_OK) return rc;
      if (f.dense_last) {
        rc = launch_layernorm_dropped(cur, idx, src, p.norm_w, p.norm_b, logits, B, N, Np, P, S0, C, p.ln_eps, f.sf32, dt, s, f.kind);
        if (rc != RAJNI_OK) return rc;
      }
      if (slabs_last) {
        void* ys[RAJNI_MAX_LAYERS];
        for (int l = cap; l < lay->n; ++l) ys[l - cap] = slab(l);
        rc = launch_rows_dropped_multi(cur, idx, src, p.norm_w, p.norm_b, ys, lay->n - cap, lay->norm, B, N, Np, P, S0, C, p.ln_eps,
                                       f.sf32, dt, s);
        if (rc != RAJNI_OK) return rc;
      }
    }
    if (idx) { oth = cur; cur = y; rope_stale = true; }
    N = Np;
    if (lay && cap < lay->n && lay->blocks[cap] == i) {
      // a captured block: the stream behind it, scattered to slab `cap` through the map of the selections up to and including
      // this block's (w.qkv again: the launches above have read their map, in stream order)
      int32_t* src = reinterpret_cast<int32_t*>(w.qkv);
      rc = launch_source_idx_before(f, i + 1, src, N);
      if (rc != RAJNI_OK) return rc;
      rc = lay->norm ? launch_layernorm_dense(cur, src, p.norm_w, p.norm_b, slab(cap), B, N, S0, C, p.ln_eps, f.sf32, dt, s, lay->fill ? 0 : 1, f.kind)
                     : launch_rows_dense_cast(cur, src, slab(cap), B, N, S0, C, f.sf32, dt, s, lay->fill ? 0 : 1);
      if (rc != RAJNI_OK) return rc;
      ++cap;
    }
  }

  // ---- final norm on the CLS rows only (LN is per token; model.py:65-66) + head
  // (with a pooled head, fc_norm or no norm: norm on every row that is pooled -> pool -> fc_norm, one kernel)
  // a headless plan: the same launch writes the caller's buffer instead of w.clsn, and there is no head GEMM
  void* const rowout = headless(p) ? logits : (void*)w.clsn;
  if (f.ap) return launch_pool_tail(f, cur, N, logits);
  if (f.pool == RAJNI_POOL_NONE)  // every surviving token through the final norm: [B, N, C]
    return launch_layernorm(cur, C, p.norm_w, p.norm_b, logits, B * N, C, p.ln_eps, f.sf32, dt, s, f.kind);
  if (f.pool == RAJNI_POOL_DENSE || f.dense_last) {
    // [B, P + n, C]: token j of the final stream at the row it came from, zeros elsewhere (RAJNI_POOL_DENSE_LAST: the other
    // rows were written behind the blocks that dropped them and stay).  The composed selection lives in w.qkv, dead behind
    // the last block (B * N * 4 bytes always fit)
    int32_t* src = reinterpret_cast<int32_t*>(w.qkv);
    rc = launch_source_idx_before(f, p.depth, src, N);
    if (rc != RAJNI_OK) return rc;
    return launch_layernorm_dense(cur, src, p.norm_w, p.norm_b, logits, B, N, S0, C, p.ln_eps, f.sf32, dt, s,
                                  f.dense_last ? 0 : 1, f.kind);
  }
  if (ext && (f.pool != RAJNI_POOL_TOKEN || ext->fc_norm_w || f.norm_absent))
    rc = launch_pool_norm(cur, B, N, C, f.pool, f.norm_absent ? nullptr : p.norm_w, p.norm_b, p.ln_eps,
                          ext->fc_norm_w, ext->fc_norm_b, ext->fc_norm_eps, rowout, f.sf32, dt, s, P, f.kind);
  else if (HR == 2) {
    // rows 0 and 1 of every image, normalised side by side: row b of [B, 2C].  A stream that still holds all N rows (a last
    // block that prunes, or the all-rows form) first gives up its two rows to the other stream buffer, dense
    if (N > 2) {
      oth = cur == w.xa ? w.xb : w.xa;
      rc = launch_gather_rows(cur, w.idx01, oth, B, N, 2, C * ((f.sf32 || dt == RAJNI_F32) ? 4 : 2), s);
      if (rc != RAJNI_OK) return rc;
      cur = oth;
    }
    rc = launch_layernorm(cur, C, p.norm_w, p.norm_b, w.clsn, 2 * B, C, p.ln_eps, f.sf32, dt, s, f.kind);
  } else
    rc = launch_layernorm(cur, (long)N * C, p.norm_w, p.norm_b, rowout, B, C, p.ln_eps, f.sf32, dt, s, f.kind);
  if (rc != RAJNI_OK) return rc;
  if (headless(p)) return RAJNI_OK;
  rajni_linear_args head = linear_args(dt, w.clsn, p.head_w, p.head_b, nullptr, logits, B, p.num_classes, HR * C, RAJNI_EPI_BIAS);
  head.ldc = logits_stride(p);
  return launch_linear(head, s);
}

}  // namespace

// The entry points (include/rajni_hip*.h): each passes the records it takes.  A NULL trailing record behaves as the
// next-narrower entry point, including the name a prefix refusal carries: make_spec names the call by its widest record.
extern "C" int rajni_vit_forward(const rajni_vit_plan* plan, const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_ext(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const void* images, void* logits,
                                     rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_ext_prefix(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                            const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_layers(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                        const rajni_vit_layers* layers, const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, nullptr, nullptr, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_image(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                       const rajni_vit_layers* layers, const rajni_vit_image* image, const void* images, void* logits,
                                       rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, nullptr, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_query(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                       const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                       const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, nullptr, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_pool(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                      const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                      const rajni_vit_attn_pool* pool, const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, pool, (hipStream_t)stream), images, logits);
}
extern "C" int rajni_vit_forward_norm(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                      const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                      const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const void* images, void* logits,
                                      rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, pool, (hipStream_t)stream, norm), images, logits);
}
extern "C" int rajni_vit_forward_rope(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                      const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                      const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                                      const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, pool, (hipStream_t)stream, norm, rope), images, logits);
}
extern "C" int rajni_vit_forward_mlpnorm(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                         const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                         const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                                         const rajni_vit_mlp_norm* mlp_norm, const void* images, void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, pool, (hipStream_t)stream, norm, rope, mlp_norm),
                     images, logits);
}
extern "C" int rajni_vit_forward_relpos(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                                        const rajni_vit_layers* layers, const rajni_vit_image* image, const rajni_vit_query* query,
                                        const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm, const rajni_vit_rope* rope,
                                        const rajni_vit_mlp_norm* mlp_norm, const rajni_vit_relpos* relpos, const void* images,
                                        void* logits, rajni_stream_t stream) {
  return vit_forward(make_spec(ENTRY_FORWARD, plan, ext, prefix, layers, image, query, pool, (hipStream_t)stream, norm, rope, mlp_norm, relpos),
                     images, logits);
}
extern "C" size_t rajni_vit_workspace_bytes_relpos(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix,
                                                   const rajni_vit_image* image, const rajni_vit_query* query,
                                                   const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                                   const rajni_vit_rope* rope, const rajni_vit_mlp_norm* mlp_norm,
                                                   const rajni_vit_relpos* relpos) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, pool, nullptr, norm, rope, mlp_norm, relpos));
}
extern "C" size_t rajni_vit_workspace_bytes(const rajni_vit_plan* plan) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
}
extern "C" size_t rajni_vit_workspace_bytes_prefix(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, nullptr, nullptr, nullptr, nullptr));
}
extern "C" size_t rajni_vit_workspace_bytes_image(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, nullptr, nullptr, nullptr));
}
extern "C" size_t rajni_vit_workspace_bytes_query(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                                  const rajni_vit_query* query) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, nullptr, nullptr));
}
extern "C" size_t rajni_vit_workspace_bytes_pool(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                                 const rajni_vit_query* query, const rajni_vit_attn_pool* pool) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, pool, nullptr));
}

extern "C" size_t rajni_vit_workspace_bytes_norm(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                                 const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, pool, nullptr, norm));
}

extern "C" size_t rajni_vit_workspace_bytes_rope(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image,
                                                 const rajni_vit_query* query, const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                                 const rajni_vit_rope* rope) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, pool, nullptr, norm, rope));
}

extern "C" size_t rajni_vit_workspace_bytes_mlpnorm(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix,
                                                    const rajni_vit_image* image, const rajni_vit_query* query,
                                                    const rajni_vit_attn_pool* pool, const rajni_vit_norm* norm,
                                                    const rajni_vit_rope* rope, const rajni_vit_mlp_norm* mlp_norm) {
  return workspace_bytes(make_spec(ENTRY_SIZE, plan, nullptr, prefix, nullptr, image, query, pool, nullptr, norm, rope, mlp_norm));
}

extern "C" void rajni_debug_set_last_block_all_rows(int on) { g_last_block_all_rows = on; }

// 1 when the forward of this plan (with this ext / prefix record, either may be NULL) computes its last block for the rows the
// head reads only (the CLS rows; rows 0 and 1 with head_rows == 2), 0 when for all rows: the eligibility test alone, on the
// host, nothing launched and no device pointer followed
extern "C" int rajni_debug_last_block_cls_rows(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix) {
  if (!plan || !plan->blocks || plan->depth <= 0 || plan->patch_size <= 0) return 0;
  const Spec c = make_spec(ENTRY_FORWARD, plan, ext, prefix, nullptr, nullptr, nullptr, nullptr, nullptr);
  return last_block_cls_rows(c, plan->depth - 1, tokens_entering(c, plan->depth - 1)) ? 1 : 0;
}
