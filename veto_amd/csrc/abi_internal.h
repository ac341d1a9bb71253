// What the host-side translation units of the C ABI (abi_core / abi_forward / abi_train / abi_optim / abi_detect / abi_debug .hip) share: the
// error string, the argument checks that several entry points make, the workspace carver, the handle with its weight store and
// profiler, the GEMM launch helper and the argument builders of the launches that both a forward and a test hook of it make.
// Host only; no kernel source includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "../../include/veto_amd.h"
#include "kernels.h"

using namespace veto;

#pragma GCC visibility push(hidden)      // nothing below is part of the library's interface

extern thread_local std::string g_abi_err;      // what veto_last_error returns: ONE object per thread (defined in abi_core.hip)

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_abi_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess) return fail(VETO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

#define ABI_TRY(expr)       /* a check or step that has set the error itself */ \
  do {                                                                             \
    const int rc__ = (expr);                                                       \
    if (rc__ != VETO_OK) return rc__;                                              \
  } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A workspace layout is ONE function that walks a Carver over its regions, each starting at a multiple of 256 bytes, and returns
// Carver::off behind the last: on the caller's buffer it hands out the pointers, on base == nullptr the same walk only sizes, so
// the size an entry point asks for and the bytes it uses cannot disagree.
struct Carver {
  char* base;
  size_t off = 0;
  size_t take_offset(size_t bytes) {
    const size_t at = off;
    off += align_up(bytes, 256);
    return at;
  }
  template <class T = char>
  T* take(size_t bytes) {
    const size_t at = take_offset(bytes);
    return base ? (T*)(base + at) : nullptr;
  }
};

// ---- the checks several entry points make: each returns VETO_OK or the code of the error it has set ------------------------------
// The head of an entry point that takes an argument struct: "null argument" (also_given: the other pointers that message covers),
// then "<type> size mismatch"
template <class T>
inline int check_struct(const T* a, const char* type_name, bool also_given) {
  if (!a || !also_given) return fail(VETO_ERR_INVALID, "null argument");
  if (a->struct_size != (int32_t)sizeof(T)) return fail(VETO_ERR_INVALID, "%s size mismatch", type_name);
  return VETO_OK;
}
#define CHECK_STRUCT_AND(type, a, also_given) ABI_TRY(check_struct<type>(a, #type, also_given))
#define CHECK_STRUCT(type, a) CHECK_STRUCT_AND(type, a, true)

// (a null workspace is VETO_ERR_INVALID where the entry point's "null argument" has covered it before, VETO_ERR_WORKSPACE here)
inline int check_workspace(const void* workspace, size_t bytes, size_t need, bool must_be_aligned) {
  if (!workspace || bytes < need) return fail(VETO_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, bytes);
  if (must_be_aligned && ((uintptr_t)workspace & 255) != 0) return fail(VETO_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  return VETO_OK;
}

// veto_rpn_args_t / veto_rpn_loss_args_t: the image and level counts, and the shape of pyramid level l
template <class T>
inline int check_rpn_counts(const T* a) {
  if (a->n_img <= 0 || a->n_img > 65535) return fail(VETO_ERR_INVALID, "n_img %d outside 1..65535", a->n_img);
  if (a->n_lvl <= 0 || a->n_lvl > VETO_RPN_MAX_LEVELS) return fail(VETO_ERR_INVALID, "n_lvl %d outside 1..%d", a->n_lvl, VETO_RPN_MAX_LEVELS);
  return VETO_OK;
}
template <class T>
inline int check_rpn_level(const T* a, int l) {
  if (a->level_a[l] <= 0 || a->level_h[l] <= 0 || a->level_w[l] <= 0)
    return fail(VETO_ERR_INVALID, "level %d: bad shape (A %d, H %d, W %d)", l, a->level_a[l], a->level_h[l], a->level_w[l]);
  return VETO_OK;
}

// A sampler's rows per image (config_key: where the reference's configuration keeps it) and the positives among them
inline int check_batch_size(int batch, int cap, const char* config_key) {
  if (batch < 1 || batch > cap) return fail(VETO_ERR_INVALID, "batch_size_per_image %d outside 1..%d (%s)", batch, cap, config_key);
  return VETO_OK;
}
inline int check_positives(const char* field, int n_pos, int batch) {
  if (n_pos < 0 || n_pos > batch)
    return fail(VETO_ERR_INVALID, "%s %d outside 0..%d (BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION)", field, n_pos, batch);
  return VETO_OK;
}

// The box coder's weights: a decoder divides by them (positive), an encoder only multiplies (finite)
inline int check_reg_weights(const float* w, bool positive, const char* suffix) {
  for (int k = 0; k < 4; ++k)
    if (positive ? !(w[k] > 0.f) : !std::isfinite(w[k]))
      return fail(VETO_ERR_INVALID, "reg_weights[%d] = %g%s%s", k, w[k], positive ? " must be > 0" : "", suffix);
  return VETO_OK;
}

// The head of MEET / vote group k holds the background, every class c of the group (incre_idx_list[c] == k + 1) and the "other
// group" column: it must be exactly that wide, and the kernel's column table holds 104 columns
inline int check_group_width(int width, int k, const int32_t* incre_idx_list, int n_rel_cls) {
  if (width < 3 || width - 1 > 104) return fail(VETO_ERR_INVALID, "bad group %d (width %d)", k, width);
  int n = 0;
  for (int c = 0; c < n_rel_cls; ++c) n += incre_idx_list[c] == k + 1;
  if (n > width - 2) return fail(VETO_ERR_INVALID, "group %d has more classes than its head is wide", k);
  if (n != width - 2) return fail(VETO_ERR_INVALID, "group %d: %d classes but head width %d", k, n, width);
  return VETO_OK;
}

// What the argument structs of the relation post-processors have in common (the caller adds n_img and its own inputs)
template <class T>
inline PostArgs post_args(const T* a) {
  PostArgs p{};
  p.obj_logits = a->obj_logits; p.rel_pairs = a->rel_pairs;
  p.n_obj = a->n_obj; p.n_pair = a->n_pair; p.n_rel_cls = a->n_rel_cls; p.n_obj_cls = a->n_obj_cls;
  p.obj_scores = a->obj_scores; p.obj_pred = a->obj_pred; p.out_prob = a->rel_prob_sorted;
  p.out_pairs = a->rel_pairs_sorted; p.out_labels = a->rel_labels_sorted; p.out_triple = a->triple_sorted;
  return p;
}

// veto_post_meet_args_t / veto_post_vote_args_t as the batch call's struct: one image of n_pair pairs, no offsets
template <class T>
inline veto_post_groups_batch_args_t one_image_groups(const T* a, const float* const* heads, int experts, int voting, int32_t* kept_count) {
  veto_post_groups_batch_args_t b{};
  b.n_img = 1; b.n_obj = a->n_obj; b.n_pair = a->n_pair; b.n_groups = a->n_groups; b.experts_per_group = experts;
  b.n_rel_cls = a->n_rel_cls; b.n_obj_cls = a->n_obj_cls; b.voting = voting; b.max_pairs_per_image = a->n_pair;
  b.head_logits = heads; b.group_widths = a->group_widths; b.incre_idx_list = a->incre_idx_list; b.pairs_per_image = &a->n_pair;
  b.obj_logits = a->obj_logits; b.rel_pairs = a->rel_pairs; b.obj_scores = a->obj_scores; b.obj_pred = a->obj_pred;
  b.rel_prob_sorted = a->rel_prob_sorted; b.rel_pairs_sorted = a->rel_pairs_sorted; b.rel_labels_sorted = a->rel_labels_sorted;
  b.triple_sorted = a->triple_sorted; b.kept_count = kept_count;
  return b;
}

struct Param {
  std::string name;
  size_t numel = 0;
  size_t offset = 0;  // floats into the raw arena
  bool loaded = false;
};

typedef __bf16* SplitW;  // [N, 2K] split rows (common.h)

// The four Linears of a transformer layer, in the order of LayerW::exp_m: state-dict names behind "layers.<l>." and the shape [N, K]
enum { LIN_QKV = 0, LIN_OUT = 1, LIN_FC1 = 2, LIN_FC2 = 3 };
struct LayerLinear { const char* weight; const char* bias; int N, K; };
const LayerLinear kLayerLinears[4] = {{"0.fn.to_qkv.weight", nullptr, 3 * kDim, kDim},
                                      {"0.fn.to_out.0.weight", "0.fn.to_out.0.bias", kDim, kDim},
                                      {"1.fn.net.0.weight", "1.fn.net.0.bias", 2 * kDim, kDim},
                                      {"1.fn.net.3.weight", "1.fn.net.3.bias", kDim, 2 * kDim}};

struct MixedLinear {   // one Linear on mixed rows (common.h): weight rows, fp32 bias, the device int holding the e4m3 exponent
  const void* w;
  const float* b;
  const int* exp;
};

struct LayerW {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *out_b, *fc1_b, *fc2_b;
  SplitW qkv = nullptr, out = nullptr, fc1 = nullptr, fc2 = nullptr;
  // VETO_MIXED: the same four weights as mixed rows (common.h) and their e4m3 exponents (device ints: qkv, out, fc1, fc2)
  SplitW qkv_m = nullptr, out_m = nullptr, fc1_m = nullptr, fc2_m = nullptr;
  int* exp_m = nullptr;
  SplitW split(int lin) const { return lin == LIN_QKV ? qkv : lin == LIN_OUT ? out : lin == LIN_FC1 ? fc1 : fc2; }
  SplitW mixed_rows(int lin) const { return lin == LIN_QKV ? qkv_m : lin == LIN_OUT ? out_m : lin == LIN_FC1 ? fc1_m : fc2_m; }
  MixedLinear mixed(int lin) const {
    const float* const bias[4] = {nullptr, out_b, fc1_b, fc2_b};
    return MixedLinear{mixed_rows(lin), bias[lin], exp_m + lin};
  }
};

struct ProfRec {
  int name_id;
  hipEvent_t start, stop;
  double flops, bytes;
};

// The derived operands finalize_weights builds, and the two builds an operand can have: the one the training path reads (a Linear's
// split rows, the patch weight, the projection and head transposes) and the one only the inference forward reads (a Linear's mixed
// rows, the layer-0 constants, the folded last layer's factors)
enum operand_id { OP_PATCH, OP_LOC_T, OP_CLS_T, OP_HEAD_T, OP_QKV0, OP_FOLD, OP_LINEAR0 };      // OP_LINEAR0 + 4 l + i: Linear i of layer l
enum { STALE_TRAIN = 1, STALE_INFER = 2 };

struct veto_handle_s {
  veto_config_t cfg;
  int dh = 0;
  int chunk = 0;
  std::vector<Param> params;
  std::map<std::string, int> index;
  float* raw = nullptr;      // fp32 copies of every state-dict tensor, each at a multiple of 64 floats (Param::offset)
  size_t raw_floats = 0;     // ... and their end: the floats of the arena, and of a gradient buffer laid out like it
  char* derived = nullptr;   // split planes, transposes, folded tables
  bool dirty = true;         // a weight was uploaded since the derived operands were built
  bool infer_dirty = false;  // ... the training-side operands are current, an inference-only one (mixed rows, layer-0 tables, folded last layer) is not
  // Per-tensor refresh.  deps[i]: the derived operands (operand_id) that read weight i -- THE dependency table, filled once by
  // veto_create (abi_core.hip, operands_of); a tensor read in place has none.  stale[op]: which builds of the operand have not seen
  // its tensors' last upload (STALE_TRAIN | STALE_INFER); everything is stale until the first finalize_weights.
  // built[]: what the last finalize_weights launched, per veto_build_kind (veto_debug_last_finalize)
  std::vector<std::vector<int>> deps;
  std::vector<uint8_t> stale;
  int32_t built[VETO_BUILD_KINDS] = {};
  // generation of the derived weight operands (bumped by every finalize_weights) and, per training workspace, the generation its
  // saved activations were computed with: veto_backward refuses a workspace whose forward saw other weights
  uint64_t weight_gen = 0;
  // (a handful of workspaces at most: a training loop re-uses one; the table is cleared by every weight upload and bounded besides)
  static constexpr size_t kMaxTrainWorkspaces = 8;
  std::map<const void*, uint64_t> train_gen;
  void stamp_train_workspace(const void* ws) {
    if (train_gen.size() >= kMaxTrainWorkspaces && !train_gen.count(ws)) {   // evict the entry of the oldest generation
      auto old = train_gen.begin();
      for (auto it = train_gen.begin(); it != train_gen.end(); ++it)
        if (it->second < old->second) old = it;
      train_gen.erase(old);
    }
    train_gen[ws] = weight_gen;
    for (auto it = train_plan.begin(); it != train_plan.end();) it = train_gen.count(it->first) ? std::next(it) : train_plan.erase(it);
  }
  // ... and the plan (veto_train_plan_t, flattened to bytes) its forward ran under; no entry: veto_forward_train, no plan.  Both calls of
  // a step must agree on it: the plan decides the workspace layout and which activations the forward kept
  std::map<const void*, std::string> train_plan;
  std::vector<LayerW> layers;
  SplitW patch_w = nullptr;
  // last layer, folded CLS attention (attention.hip): Mcat [heads*576, 2*576], Ncat [576, 2*heads*576], and their fp32 staging
  SplitW fold_m = nullptr, fold_n = nullptr;
  float* fold_tmp = nullptr;
  // ... in block form (fold_dhp > 0: the head width padded to 32 k's divides a 192-column tile): Mcat = Wq^T Wk and Ncat = Wo Wv
  // are products of rank dh per head, so u = (a0 Wq_pad^T) . blockdiag(Wk) and out = (abar . blockdiag(Wv)^T) Wo_pad^T take four
  // GEMMs of 67 GF in all (zero blocks skipped: GemmArgs::kb_tiles) instead of two of 80 GF each
  SplitW fold_q = nullptr, fold_k = nullptr, fold_v = nullptr, fold_o = nullptr;
  int fold_dhp = 0;
  // layer 0, per-object form of LayerNorm + QKV (rowops.hip): Wqkv diag(gamma) as a GEMM operand, vec = [c2 | b0 | qkv_cls]
  SplitW q0_w = nullptr;
  float* q0_vec = nullptr;
  float* patch_bias = nullptr;
  float* loc_wt = nullptr;
  float* cls_wt = nullptr;
  float* head_wt = nullptr;
  // veto_forward_saturation: device counters [layers][VETO_SAT_SITES][4], allocated by veto_create (VETO_MIXED handles).  The call
  // hands them to forward_impl as an argument -- no handle state changes, so a concurrent veto_forward on the same handle is unaffected --
  // and forward_impl then takes the launch-per-stage form of the mixed path (every mixed-row operand exists in memory) and counts
  // behind every producer
  unsigned long long* sat_buf = nullptr;
  // profiling
  bool prof_on = false;
  std::vector<std::string> prof_names;
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> event_pool;
  struct Agg { double ms = 0; int64_t n = 0; double flops = 0, bytes = 0; };
  std::vector<Agg> prof_agg;

  const float* p(const std::string& name) const { return raw + params[index.at(name)].offset; }
  void add(const std::string& name, size_t numel) {
    Param q;
    q.name = name;
    q.numel = numel;
    index[name] = (int)params.size();
    params.push_back(q);
  }
};

constexpr const char* kT = "fusion_transformer.transformer.";

inline std::string lname(int l, const char* rest) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%slayers.%d.%s", kT, l, rest);
  return buf;
}

inline int prof_id(veto_handle_t h, const char* name) {
  for (size_t i = 0; i < h->prof_names.size(); ++i)
    if (h->prof_names[i] == name) return (int)i;
  h->prof_names.push_back(name);
  h->prof_agg.emplace_back();
  return (int)h->prof_names.size() - 1;
}

struct ProfScope {
  veto_handle_t h;
  hipStream_t s;
  int rec = -1;
  ProfScope(veto_handle_t h_, hipStream_t s_, const char* name, double flops, double bytes) : h(h_), s(s_) {
    if (!h || !h->prof_on) return;
    ProfRec r;
    r.name_id = prof_id(h, name);
    r.flops = flops;
    r.bytes = bytes;
    for (hipEvent_t* e : {&r.start, &r.stop}) {
      if (!h->event_pool.empty()) { *e = h->event_pool.back(); h->event_pool.pop_back(); }
      else if (hipEventCreate(e) != hipSuccess) return;
    }
    (void)hipEventRecord(r.start, s);      // profiling is best effort: a failed record shows up as a missing timing
    h->prof_recs.push_back(r);
    rec = (int)h->prof_recs.size() - 1;
  }
  ~ProfScope() {
    if (rec >= 0) (void)hipEventRecord(h->prof_recs[rec].stop, s);
  }
};

// abi_core.hip.  train_only: just the operands the training path reads (split rows of the Linears, the patch / pair-projection / head
// re-layouts).  A training loop uploads every weight after every optimizer step; the mixed rows (a max-|w| reduction per tensor), the
// table form of layer 0 and the folded last layer are the inference path's, and are built when an inference forward next needs them
// (infer_dirty).  Only the operands that read a tensor uploaded since their last build are rebuilt (veto_handle_s::deps / stale).
// infer_layers >= 0 (the frozen-fused training step): of the inference-only operands just those of layers < infer_layers, the layer-0
// constants, and the folded last layer when infer_layers covers it -- the rest stays stale for an inference forward to build.
int finalize_weights(veto_handle_t h, hipStream_t s, bool train_only = false, int infer_layers = -1);

// abi_forward.hip: the inference forward as the frozen region of a training step (veto_train_plan_t.frozen_fused).  The prelude and
// layers < k run through forward_impl's stages, chunk by chunk, in `workspace` (frozen_forward_workspace_bytes).  k < layers: the fp32
// residual rows behind layer k - 1 go to handoff [n_pair * 19, 576] and nothing else is computed; k == layers: the whole forward, the
// logits to out_logits and the CLS rows to cls_rows [n_pair, 576]
size_t frozen_forward_workspace_bytes(veto_handle_t h, int n_obj, int n_pair, int k);
int frozen_forward(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace, size_t workspace_bytes, int k, float* handoff,
                   float* out_logits, float* cls_rows);

// A dropout site (kernels.h, DropSite) into the argument structs that go into a kernel by value and so keep fields of their own:
// ObjPrepArgs / AssembleArgs (their rows are token or object rows: no row_step), and the transform of launch_prep_grad
template <class Args>
inline void set_drop(Args& a, const DropSite& d) { a.drop_seed = d.seed; a.drop_thresh = d.thresh; a.drop_scale = d.scale; }
inline GradXform drop_xform(const DropSite& d) {
  GradXform xf;
  if (d.thresh) { xf.mode = XF_DROP; xf.seed = d.seed; xf.thresh = d.thresh; xf.scale = d.scale; xf.row_step = d.row_step; }
  return xf;
}

// ---- the weight-gradient GEMM (abi_train.hip): dW[n, k] = A^T . B over m reduction rows, split-K ---------------------------------
// The split of one call: ks ranges of the reduction, its length padded to mp (a multiple of 32 * ks), and the floats of the ordered
// mode's ks partial planes.  k_splits > 0: the caller's count; else just under 2 full rounds of the 256 persistent workgroups with at
// least min_ksteps k-steps per tile, at most `cap` (0 = none).  Launch, plane sizes and operand paddings all come from here.
struct WgradSplit { int ks; size_t mp, plane_floats; };
WgradSplit wgrad_split(int n, int k, int m, int k_splits, int min_ksteps, int cap);
constexpr int kWgradLinearKsteps = 64, kWgradLinearCap = 64;      // a layer's Linears (TrainWs::mp2 has room for 64 splits)
constexpr int kWgradPatchKsteps = 8;                              // the patch projection (few object rows: tiles of 8 k-steps already)
// The launch.  zero != nullptr: a [m, 2n] and b [m, 2k] are split rows, transposed on their way out of LDS (GemmArgs::tn), `zero` what
// is read for the reduction rows past m; nullptr: explicit transposed split copies [n, 2mp] / [k, 2mp].  planes == nullptr: dw is zeroed
// and the ranges add into it with float atomics; else (ordered mode) range j writes plane j and launch_fold_rows adds them in order.
// scope: the profile entry around GEMM and fold, or nullptr
hipError_t launch_wgrad(veto_handle_t h, hipStream_t s, const char* scope, const __bf16* a, const __bf16* b, const __bf16* zero, int m, int n,
                        int k, const WgradSplit& sp, float* dw, float* planes);

// (abi_core.hip) lda / ldc of split operands are in bf16 elements (2K / 2N for contiguous rows).
int run_gemm(veto_handle_t h, hipStream_t s, const char* name, const __bf16* a, SplitW w, const float* bias, const float* resid, long ldr,
             float* c, __bf16* c_split, long ldc, int M, int N, int K, int epi, long lda = 0, int w_row0 = 0, DropSite drop = DropSite(),
             const int* w_exp = nullptr, int kb_tiles = 0, int kb_steps = 0);

// ---- argument builders of the launches that the inference forward, the training forward and the test hooks share ---------------
// Per-object embeddings (everything but the training path's dropout site).  bn_batch_stats given: training-mode BatchNorm on this
// batch's statistics (biased variance), which the caller has launch_bn_batch_stats fill first
inline ObjPrepArgs obj_prep_args(veto_handle_t h, const veto_inputs_t* in, float* lc) {
  ObjPrepArgs a{};
  a.boxes = in->boxes; a.box_mode = in->box_mode; a.labels = in->obj_labels; a.obj_logits = in->obj_logits;
  a.embed = h->p("obj_embed.weight"); a.num_obj_cls = h->cfg.num_obj_cls; a.embed_dim = h->cfg.embed_dim;
  a.bn_w = h->p("pos_embed.0.weight"); a.bn_b = h->p("pos_embed.0.bias");
  a.bn_mean = in->bn_batch_stats ? in->bn_batch_stats : h->p("pos_embed.0.running_mean");
  a.bn_var = in->bn_batch_stats ? in->bn_batch_stats + 4 : h->p("pos_embed.0.running_var");
  a.pos_w = h->p("pos_embed.1.weight"); a.pos_b = h->p("pos_embed.1.bias");
  a.loc_wt = h->loc_wt; a.loc_b = h->p("location_projection.0.bias");
  a.cls_wt = h->cls_wt; a.cls_b = h->p("class_projection.0.bias");
  a.lc = lc; a.pos_out = nullptr; a.n_obj = in->n_obj;
  return a;
}

// Token assembly of n_pair pairs into x and the layer-0 LayerNorm1 rows a (split rows; the caller sets stats / a_fmt / x_f24 / dropout)
inline AssembleArgs assemble_args(veto_handle_t h, const float* patch_tab, const float* lc, const int32_t* subj, const int32_t* obj, float* x,
                                  __bf16* a_rows, int n_pair) {
  AssembleArgs a{};
  a.patch_tab = patch_tab; a.lc = lc; a.cls_token = h->p(std::string(kT) + "cls_token");
  a.pos_embedding = h->p(std::string(kT) + "pos_embedding");
  a.ln_w = h->layers[0].ln1_w; a.ln_b = h->layers[0].ln1_b;
  a.subj = subj; a.obj = obj; a.x = x; a.a = a_rows; a.n_pair = n_pair;
  return a;
}

struct RowNorm {   // optional LayerNorm of a panel launch's result rows (FfnArgs::ln_w / ln_b), written as mixed rows to `rows`
  const float* w = nullptr;
  const float* b = nullptr;
  void* rows = nullptr;
};

// FeedForward panel (launch_ffn_fused): x <- x + fc2(gelu(fc1(a))) on M rows; next: LayerNorm rows of the result
inline FfnArgs ffn_panel_args(const void* a, MixedLinear fc1, MixedLinear fc2, float* x, int M, RowNorm next = RowNorm()) {
  FfnArgs f{};
  f.a = (const char*)a; f.w1 = (const char*)fc1.w; f.w2 = (const char*)fc2.w; f.b1 = fc1.b; f.b2 = fc2.b;
  f.resid = x; f.out = x; f.ldr = kDim; f.ldo = kDim; f.M = M; f.exp1 = fc1.exp; f.exp2 = fc2.exp;
  f.ln_w = next.w; f.ln_b = next.b; f.ln_out = (char*)next.rows;
  return f;
}

// Out-projection panel (launch_out_fused): x <- x + out(a) on M rows; ln2: LayerNorm rows of the result
inline FfnArgs out_panel_args(const void* a, MixedLinear out, float* x, int M, RowNorm ln2 = RowNorm()) {
  FfnArgs f{};
  f.a = (const char*)a; f.w2 = (const char*)out.w; f.b2 = out.b; f.resid = x; f.out = x; f.ldr = kDim; f.ldo = kDim;
  f.M = M; f.exp2 = out.exp; f.ln_w = ln2.w; f.ln_b = ln2.b; f.ln_out = (char*)ln2.rows;
  return f;
}

// Full layer tail (launch_layer_tail): x1 = x + out(a), LayerNorm2 (ln2.w / ln2.b) of x1 written to ln2.rows, x <- x1 + fc2(gelu(fc1(.)));
// next: LayerNorm of the result with next.w / next.b, to next.rows or (rows == nullptr) in place over ln2.rows
inline FfnArgs layer_tail_args(const void* a, MixedLinear out, RowNorm ln2, MixedLinear fc1, MixedLinear fc2, float* x, int M,
                               RowNorm next = RowNorm()) {
  FfnArgs f = ffn_panel_args(a, fc1, fc2, x, M);
  f.wo = (const char*)out.w; f.bo = out.b; f.expo = out.exp; f.lnm_w = ln2.w; f.lnm_b = ln2.b; f.ln_out = (char*)ln2.rows;
  f.ln_w = next.w; f.ln_b = next.b; f.ln1_out = (char*)next.rows;
  return f;
}

#pragma GCC visibility pop
