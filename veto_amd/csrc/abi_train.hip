// ================================================================================================================
// Training path: forward that keeps every activation the backward needs, and the
// backward itself.  One pass over all pairs (no chunking), precise mode, no dropout (the caller refuses p > 0).
// Every layer runs on all 19 tokens (the CLS-only shortcut of the inference path would complicate the backward).
// ================================================================================================================
#include "abi_internal.h"

#include <cmath>
#include <cstring>
#include <mutex>

namespace {

struct TrainLayer {
  float* xin;    // [mpad, 576]   input of the layer (residual stream)
  __bf16* a1;    // split LN1(xin)
  float* qkv;    // [mpad, 1728]
  __bf16* ao;    // split attention output
  float* xmid;   // [mpad, 576]   after the attention residual
  __bf16* a2;    // split LN2(xmid)
  float* pre;    // [mpad, 1152]  fc1 pre-activation
  __bf16* hid;   // split gelu(pre)
};

struct TrainWs {
  int32_t *subj, *obj;
  float *lc, *patch_tab, *xout;
  __bf16* pa;
  std::vector<TrainLayer> layers;
  // backward scratch
  float *dx, *dmid, *dtmp, *dbig;
  __bf16 *dsplit, *wdg, *zero;
  __bf16* dsplit_b;   // the last two thirds of dsplit: rows of 2 * 1152 bf16 (the fc2 input-gradient epilogue writes fc1's gradient rows there
                      // while its own operand, rows of 2 * 576 bf16, occupies the first third)
  float *ln_partial, *col_partial, *colp, *dgb, *head_partial;
  float *dpatch, *dlc, *dpos, *dpre, *xhat, *bn_out, *dbn_out, *emb, *demb, *prob, *dloc_wt, *dcls_wt, *dwcat_t;
  __bf16* wcat_t;   // Wcat^T [2112, 2*1152] split rows: weight operand of the patch projection's input gradient
  float* dpa;       // dPA [prow, 2112] fp32: gradient w.r.t. the patch rows
  size_t mp2;    // padded reduction length of the weight-gradient GEMMs
  // ordered mode (veto_train_opts_t.deterministic) only, behind everything else so that the default layout and size stay what they were:
  // the split-K partial planes of the weight-gradient GEMMs, [k_splits][N][K] fp32 of the largest call; nullptr = the default (atomic) path
  float* planes;
  size_t total;
};

// q / k / v of the training path as 3-byte floats (common.h) between the QKV projection, the attention and the attention backward: all
// three split them into 16-bit hi + lo parts anyway, so the 16-bit significand in memory is what they would have kept -- 1.7 KB per token
// row and layer less to keep and to move (round 6).  MFMA head widths only; VETO_TRAIN_QKV_F24=0: fp32.
bool train_qkv_f24(veto_handle_t h) {
  static const bool off = env_knob_is("VETO_TRAIN_QKV_F24", "0");
  return !off && (h->dh == 72 || h->dh == 96);
}

// VETO_TRAIN_RECOMPUTE=1 (off by default): the LayerNorm1 / LayerNorm2 rows and the GELU rows of a layer are not kept for the backward but
// recomputed there from the residual rows and the pre-activation that ARE kept (the same kernels on the same inputs: bit-identical operands,
// bit-identical gradients): 8.6 GB less workspace at cfg-2 for three more passes per layer (~3 ms per step).  With 288 GB of HBM the default keeps them.
bool train_recompute() {
  static const bool on = env_knob_is("VETO_TRAIN_RECOMPUTE", "1");
  return on;
}

// dpre = dh * gelu'(pre) in the epilogue of fc2's input-gradient GEMM (round 6); VETO_TRAIN_GELU_EPI=0: inside the operand preparation of
// the fc1 backward, a pass of its own over an fp32 copy of dh (rounds 1-5)
bool train_gelu_epilogue() {
  static const bool off = env_knob_is("VETO_TRAIN_GELU_EPI", "0");
  return !off;
}

// VETO_TRAIN_LN_SPLIT=1 (off by default; round 6, measured SLOWER): the LayerNorm backward kernels emit the split rows and bias partials of the
// Linear behind them instead of a preparation pass per Linear reading the fp32 gradient rows back.  63.0 ms per step with, 61.6 without on one
// box: the kernel is at its register limit (two statistics passes over 18 values per lane and tensor) and spills with the extra column
// sums, split conversion and dropout hash, and its 4-byte split stores are slower than the pass they replace.  Kept as a tested variant.
bool train_ln_emits_split() {
  static const bool on = env_knob_is("VETO_TRAIN_LN_SPLIT", "1");
  return on;
}

int wgrad_splits(int n, int k, int m, int k_splits, int min_ksteps = 64);

// the Linears of a layer and the patch projection, as (N, K) of their weight-gradient GEMMs: the ordered mode's planes hold the largest
size_t wgrad_plane_floats(int m_tokens, int patch_rows) {
  size_t most = 0;
  auto take = [&](int n, int k, int m, int min_ksteps) {
    int ks = wgrad_splits(n, k, m, 0, min_ksteps);
    if (ks > 64) ks = 64;
    const size_t need = (size_t)ks * n * k;
    if (need > most) most = need;
  };
  for (const LayerLinear& q : kLayerLinears) take(q.N, q.K, m_tokens, 64);      // (the last layer's compact rows are fewer: no more splits)
  take(2048, 2 * kDim, patch_rows, 8);
  return most;
}

// What a step computes (include/veto_amd.h, veto_train_plan_t), derived once by make_sched from the plan.  The default-constructed
// one is the step without a plan: everything wanted, batch statistics, one attention dropout rate.
// The backward chain: head -> layers L-1 .. 0 (fc2, fc1, LayerNorm2, out, attention, qkv, LayerNorm1) -> pos_embedding / cls_token ->
// patch projection (and the map gradients) -> location / class projections -> pos_embed.1, pos_embed.0, obj_embed.
struct Sched {
  bool full = true;
  std::vector<uint8_t> on;        // per weight index (veto_weight_info): its gradient is wanted
  std::vector<float> p_attn;      // per layer; empty: opts->p_attn everywhere
  bool bn_eval = false;
  bool maps = true;               // d_roi_rgb / d_roi_depth may be asked for
  bool below = true;              // a stage under layer 0 has a consumer
  std::vector<uint8_t> need_in;   // per layer: the gradient w.r.t. the layer's input has a consumer
  int keep_from = 0;              // the lowest layer whose saved activations the backward reads (layers: none, the head reads xout only)
  std::string key;                // the plan as bytes: what the forward stamps the workspace with
  bool want(veto_handle_t h, const std::string& name) const { return full || on[h->index.at(name)] != 0; }
  bool need(int l) const { return full || need_in[l] != 0; }
};

TrainWs carve_train(char* base, veto_handle_t h, int n_obj, int n_pair, bool ordered = false, const Sched& sch = Sched()) {
  TrainWs w;
  Carver c{base};
  const int L = h->cfg.layers, E = h->cfg.embed_dim;
  const size_t M = (size_t)n_pair * kTokens;
  const size_t mpad = (size_t)gemm_rows_padded((int)M);
  const size_t prow = (size_t)gemm_rows_padded(n_obj * 16);
  w.subj = c.take<int32_t>((size_t)n_pair * 4);
  w.obj = c.take<int32_t>((size_t)n_pair * 4);
  w.lc = c.take<float>((size_t)n_obj * 2 * 2 * kDim * 4);
  w.pa = c.take<__bf16>(prow * 2 * 2048 * 2);
  w.patch_tab = c.take<float>((size_t)n_obj * 16 * 2 * kDim * 4);
  w.layers.resize(L);
  const size_t cpad = (size_t)gemm_rows_padded(n_pair);
  const bool recompute = train_recompute();
  __bf16* a_scr = recompute ? c.take<__bf16>(mpad * 2 * kDim * 2) : nullptr;      // LayerNorm rows of whichever Linear is next (forward) / being differentiated (backward)
  __bf16* hid_scr = recompute ? c.take<__bf16>(mpad * 4 * kDim * 2) : nullptr;    // the same for the GELU rows
  // (a plan: the layers under the lowest one the backward reads -- never the last, whose buffers are the compact ones -- alternate between
  // the buffers of the first two of them: a layer reads its own set and writes the input rows of the next)
  const int shared = sch.keep_from < L - 1 ? sch.keep_from : L - 1;
  for (int l = 0; l < L; ++l) {
    TrainLayer& t = w.layers[l];
    if (l < shared && l >= 2) {
      t = w.layers[l - 2];
      continue;
    }
    // (the last layer runs on the pairs' CLS rows behind its attention: those buffers are compact, one row per pair -- sized for every token
    // row until round 6, 4.4 GB too many at cfg-2)
    const size_t rows = l == L - 1 ? cpad : mpad;
    t.xin = c.take<float>(mpad * kDim * 4);
    t.a1 = recompute ? a_scr : c.take<__bf16>(mpad * 2 * kDim * 2);
    t.qkv = c.take<float>(mpad * 3 * kDim * (train_qkv_f24(h) ? 3 : 4));
    t.ao = c.take<__bf16>(rows * 2 * kDim * 2);
    t.xmid = c.take<float>(rows * kDim * 4);
    t.a2 = recompute ? a_scr : c.take<__bf16>(rows * 2 * kDim * 2);
    t.pre = c.take<float>(rows * 2 * kDim * 4);
    t.hid = recompute ? hid_scr : c.take<__bf16>(rows * 4 * kDim * 2);
  }
  w.xout = c.take<float>(cpad * kDim * 4);      // (compact: the last layer's CLS rows)
  w.dx = c.take<float>(mpad * kDim * 4);
  w.dmid = c.take<float>(mpad * kDim * 4);
  w.dtmp = c.take<float>(mpad * kDim * 4);
  // (fc2's input gradient as fp32 rows [M, 1152]: only the VETO_TRAIN_GELU_EPI=0 form writes it; sized [M, 1728] until round 6, 2 GB at cfg-2)
  w.dbig = c.take<float>(train_gelu_epilogue() ? 256 : mpad * 2 * kDim * 4);
  {   // the token-row gradients (6 * 576 bf16 per row) and, for the input gradient of the patch projection, the split rows of
      // dpatch (prow rows x 2 * 1152 bf16) share this buffer: size it for the larger (n_obj * 16 can exceed 19 * n_pair / 1.5)
    const size_t tok = mpad * 6 * kDim * 2, obj = prow * 4 * kDim * 2;
    w.dsplit = c.take<__bf16>(tok > obj ? tok : obj);
    w.dsplit_b = (__bf16*)((char*)w.dsplit + mpad * 2 * kDim * 2);
  }
  w.mp2 = (M + 32 * 64 + 31) / 32 * 32;   // room for any split count up to 64
  w.zero = c.take<__bf16>(1024);           // what the weight-gradient GEMM reads for reduction rows past the last one
  w.wdg = c.take<__bf16>((size_t)3 * kDim * kDim * 4);
  w.ln_partial = c.take<float>(layernorm_backward_partial_floats((int)M) * 4);
  w.col_partial = c.take<float>((size_t)column_sums_chunks() * 3 * kDim * 4);
  w.colp = c.take<float>((w.mp2 / 32) * 3 * kDim * 4);
  w.dgb = c.take<float>(2 * kDim * 4);
  w.head_partial = c.take<float>(head_backward_partial_floats(h->cfg.num_out) * 4);
  w.dpatch = c.take<float>((size_t)n_obj * 16 * 2 * kDim * 4);
  w.dlc = c.take<float>((size_t)n_obj * 2 * 2 * kDim * 4);
  w.dpos = c.take<float>((size_t)n_obj * kPosDim * 4);
  w.dpre = c.take<float>((size_t)n_obj * kPosDim * 4);
  w.xhat = c.take<float>((size_t)n_obj * 4 * 4);
  w.bn_out = c.take<float>((size_t)n_obj * 4 * 4);
  w.dbn_out = c.take<float>((size_t)n_obj * 4 * 4);
  w.emb = c.take<float>((size_t)n_obj * E * 4);
  w.demb = c.take<float>((size_t)n_obj * E * 4);
  w.prob = c.take<float>((size_t)n_obj * 256 * 4);
  w.dloc_wt = c.take<float>((size_t)kPosDim * 2 * kDim * 4);
  w.dcls_wt = c.take<float>((size_t)E * 2 * kDim * 4);
  w.dwcat_t = c.take<float>((size_t)2048 * 2 * kDim * 4);
  w.wcat_t = c.take<__bf16>((size_t)kPatchTRows * 2 * 2 * kDim * 2);
  w.dpa = c.take<float>((size_t)gemm_rows_padded(n_obj * 16) * kPatchTRows * 4);
  w.planes = ordered ? c.take<float>(wgrad_plane_floats((int)M, n_obj * 16) * 4) : nullptr;
  w.total = c.off;
  return w;
}

// dw[N,K] = dy[M,N]^T . x[M,K]: the weight-gradient shape (reduction over the M rows).  Both operands are
// transposed into split rows ([N, 2*Mp] and [K, 2*Mp]) and the persistent GEMM runs split-K with atomic adds.
int wgrad_splits(int n, int k, int m, int k_splits, int min_ksteps) {
  if (k_splits > 0) return k_splits;
  const int out_tiles = ((n + 255) / 256) * (k / 192);
  int ks = 2 * 256 / out_tiles;                         // just under 2 full rounds of the 256 persistent workgroups
  const int max_ks = (m + 32 * min_ksteps - 1) / (32 * min_ksteps);     // at least min_ksteps k-steps per tile
  if (ks > max_ks) ks = max_ks;
  return ks < 1 ? 1 : ks;
}

size_t wgrad_mp(int m, int ks) { return ((size_t)m + 32 * (size_t)ks - 1) / (32 * (size_t)ks) * 32 * (size_t)ks; }

// Backward of y = x W^T (+ b) over the token rows: dW[N, K] = dY^T x, db[N] = column sums of dY (if db), dX[M, K] = dY W.
// One pass over dY (prep_grad_kernel) produces its split rows -- the A operand of the input-gradient GEMM AND, read through
// transposing LDS loads, of the weight-gradient GEMM (GemmArgs::tn; the saved activation x_split is its other operand as it
// is) -- and the bias partials.  No transposed copies of dY or x exist.
// dy == nullptr: the producer (attention backward) has already written the split rows into w.dsplit; no bias then.
// presplit / presplit_partials: the producer wrote the split rows itself (to `presplit`; nullptr = w.dsplit) together with
// `presplit_partials` rows of column sums in w.colp (0 = none: no bias gradient then).
// gelu_pre (fc2 only): the input gradient is not written as fp32 rows: the GEMM's epilogue multiplies it by gelu'(gelu_pre) and writes the
// split rows of fc1's backward to w.dsplit_b and their column-sum partials to w.colp (*next_partials rows): the pass that read dH and the
// pre-activation back (0.9 ms per layer) is gone.
// Partial training: dw == nullptr (a frozen weight) leaves out the weight-gradient GEMM with its zero-fill or fold, db == nullptr the bias
// sums, dx == nullptr without gelu_pre (nothing below this Linear has a consumer) the weight transpose and the input-gradient GEMM.
int run_linear_backward(veto_handle_t h, hipStream_t s, const TrainWs& w, const float* dy, int M, int N, const __bf16* x_split, int K,
                        const float* weight, float* dw, float* db, float* dx, const GradXform& xf = GradXform(),
                        const __bf16* presplit = nullptr, int presplit_partials = 0, const float* gelu_pre = nullptr, int* next_partials = nullptr) {
  if (!dy && db && presplit_partials <= 0) return fail(VETO_ERR_INVALID, "a pre-split gradient without column partials cannot feed a bias gradient");
  const __bf16* gsplit = !dy && presplit ? presplit : w.dsplit;
  int ks = wgrad_splits(N, K, M, 0);
  if (ks > 64) ks = 64;      // (w.mp2 has room for 64 splits)
  const size_t mp = wgrad_mp(M, ks);
  if (mp > w.mp2) return fail(VETO_ERR_WORKSPACE, "weight-gradient partial buffer too small");
  if (dy) HIP_TRY(launch_prep_grad(dy, N, M, N, w.dsplit, (int)mp, db ? w.colp : nullptr, xf, s));
  if (db) HIP_TRY(launch_column_sums(w.colp, N, dy ? (int)(mp / 32) : presplit_partials, N, db, w.col_partial, column_sums_chunks(), s));
  if (dw && !w.planes) HIP_TRY(hipMemsetAsync(dw, 0, (size_t)N * K * 4, s));
  if (dw) {
    GemmArgs g{};
    g.a = gsplit; g.w = x_split; g.c = w.planes ? w.planes : dw;
    g.M = N; g.N = K; g.K = (int)mp; g.ldc = K; g.k_splits = ks;
    g.tn = 1; g.lda = 2 * (long)N; g.ldw = 2 * (long)K; g.k_valid = M; g.zero = w.zero;
    ProfScope ps(h, s, "bwd_wgrad", 2.0 * M * (double)N * K, 0);
    HIP_TRY(launch_gemm_split(g, w.planes ? EPI_PLANES : EPI_ATOMIC, 0, s));
    if (w.planes) HIP_TRY(launch_fold_rows(w.planes, (long)N * K, ks, (long)N * K, dw, s));      // the planes in split order
  }
  if (!dx && !gelu_pre) return VETO_OK;
  HIP_TRY(launch_transpose_split(weight, K, N, K, w.wdg, N, s));     // W [N, K] -> W^T split rows [K, 2N]
  {
    GemmArgs g{};
    g.a = gsplit; g.w = w.wdg; g.c = dx;
    g.M = M; g.N = K; g.K = N; g.ldc = K;
    ProfScope ps(h, s, "bwd_dgrad", 2.0 * M * (double)N * K, 0);
    if (gelu_pre) {
      if (gsplit == w.dsplit_b || !next_partials) return fail(VETO_ERR_INVALID, "internal: the fused gelu' epilogue writes w.dsplit_b");
      g.c = nullptr; g.c_split = w.dsplit_b; g.ldc = 2L * K; g.resid = gelu_pre; g.ldr = K; g.col_partial = w.colp;
      *next_partials = (M + 255) / 256 * 4;      // one partial row per 64-row slice of every 256-row tile
      HIP_TRY(launch_gemm_split(g, EPI_GELU_BWD, 0, s));
    } else {
      HIP_TRY(launch_gemm_split(g, EPI_F32, 0, s));
    }
  }
  return VETO_OK;
}

// dropout sites of the training path: 1 = pos_embed Dropout(0.1), 2 = pos_drop on the tokens, 3 + l = to_out of layer l.  Elements are
// numbered as include/veto_amd.h says, sites 2 and up by TOKEN row: where a site is applied to the last layer's compact CLS rows, row p is
// token row 19 p (row_step), so that the masks do not depend on which rows the implementation chooses to compute.
// sch: a plan's own rate for the attention site of layer site - 3 (veto_train_plan_t.p_attn_layer)
DropSite drop_site(const veto_train_opts_t* o, int site, int row_step = 1, const Sched* sch = nullptr) {
  DropSite d;
  d.row_step = row_step;
  if (!o) return d;
  const float p = site == 1 ? o->p_pos : site == 2 ? o->p_emb : sch && !sch->p_attn.empty() ? sch->p_attn[site - 3] : o->p_attn;
  if (!(p > 0.f)) return d;
  d.seed = o->seed + (unsigned long long)site * 0x632BE59BD9B4E019ull;
  d.thresh = (unsigned)(p * 16777216.0f);
  d.scale = 1.f / (1.f - p);
  return d;
}

// `deterministic` was appended to veto_train_opts_t: a caller built against the struct without it passes the shorter size and gets 0
constexpr int32_t kTrainOptsSizeV1 = (int32_t)offsetof(veto_train_opts_t, deterministic);

bool opts_ordered(const veto_train_opts_t* o) { return o && o->struct_size == (int32_t)sizeof(veto_train_opts_t) && o->deterministic != 0; }

int check_train_opts(const veto_train_opts_t* o) {
  if (!o) return VETO_OK;
  if (o->struct_size != (int32_t)sizeof(veto_train_opts_t) && o->struct_size != kTrainOptsSizeV1)
    return fail(VETO_ERR_INVALID, "veto_train_opts_t size mismatch");
  for (float p : {o->p_pos, o->p_emb, o->p_attn})
    if (!(p >= 0.f && p < 1.f)) return fail(VETO_ERR_INVALID, "dropout probabilities must be in [0, 1)");
  return VETO_OK;
}

// The plan, checked and flattened; plan == nullptr: the step without one
int make_sched(veto_handle_t h, const veto_train_opts_t* opts, const veto_train_plan_t* plan, Sched* out) {
  Sched sch;
  if (!plan) {
    *out = sch;
    return VETO_OK;
  }
  if (!h) return fail(VETO_ERR_INVALID, "null argument");
  if (plan->struct_size != (int32_t)sizeof(veto_train_plan_t)) return fail(VETO_ERR_INVALID, "veto_train_plan_t size mismatch");
  if (!plan->trainable) return fail(VETO_ERR_INVALID, "veto_train_plan_t.trainable is NULL");
  const int L = h->cfg.layers;
  sch.full = false;
  sch.on.assign(plan->trainable, plan->trainable + h->params.size());
  for (uint8_t& f : sch.on) f = f ? 1 : 0;
  if (plan->p_attn_layer) {
    sch.p_attn.assign(plan->p_attn_layer, plan->p_attn_layer + L);
    for (float p : sch.p_attn) {
      if (!(p >= 0.f && p < 1.f)) return fail(VETO_ERR_INVALID, "dropout probabilities must be in [0, 1)");
      if (p > 0.f && !opts) return fail(VETO_ERR_INVALID, "veto_train_plan_t.p_attn_layer needs the opts (the seed of the masks)");
    }
  }
  sch.bn_eval = plan->bn_eval != 0;
  sch.maps = plan->d_roi != 0;
  if (sch.bn_eval && (sch.want(h, "pos_embed.0.weight") || sch.want(h, "pos_embed.0.bias")))
    return fail(VETO_ERR_INVALID, "bn_eval with a trainable pos_embed.0.weight / bias needs a BatchNorm backward on fixed statistics, which is not built");
  const std::string T = kT;
  sch.below = sch.maps;
  for (const char* name : {"pos_embed.0.weight", "pos_embed.0.bias", "pos_embed.1.weight", "pos_embed.1.bias", "obj_embed.weight",
                           "location_projection.0.weight", "location_projection.0.bias", "class_projection.0.weight", "class_projection.0.bias"})
    sch.below = sch.below || sch.want(h, name);
  for (const char* name : {"pos_embedding", "cls_token", "patch_embed.proj_d.weight", "patch_embed.proj_d.bias", "patch_embed.proj_v.weight",
                           "patch_embed.proj_v.bias"})
    sch.below = sch.below || sch.want(h, T + name);
  sch.need_in.assign(L, 0);
  sch.keep_from = L;
  bool need = sch.below;
  for (int l = 0; l < L; ++l) {
    sch.need_in[l] = need;
    bool any = false;
    for (const LayerLinear& q : kLayerLinears) any = any || sch.want(h, lname(l, q.weight)) || (q.bias && sch.want(h, lname(l, q.bias)));
    for (const char* name : {"0.norm.weight", "0.norm.bias", "1.norm.weight", "1.norm.bias"}) any = any || sch.want(h, lname(l, name));
    if ((any || need) && sch.keep_from == L) sch.keep_from = l;
    need = need || any;
  }
  sch.key.assign(1, 'P');      // (never empty: no entry in train_plan means no plan)
  sch.key.append(sch.on.begin(), sch.on.end());
  sch.key.append((const char*)sch.p_attn.data(), sch.p_attn.size() * sizeof(float));
  sch.key.push_back(sch.bn_eval ? 'e' : 'b');
  sch.key.push_back(sch.maps ? 'm' : '-');
  *out = sch;
  return VETO_OK;
}

int check_train_inputs(veto_handle_t h, const veto_inputs_t* in, const veto_train_opts_t* opts, void* workspace, size_t workspace_bytes,
                       const Sched& sch = Sched()) {
  CHECK_STRUCT_AND(veto_inputs_t, in, h && workspace);
  if (in->n_obj <= 0 || in->n_pair <= 0 || in->n_img <= 0) return fail(VETO_ERR_INVALID, "empty batch");
  if (!in->roi_rgb || !in->roi_depth || !in->boxes || !in->rel_pairs || !in->img_obj_offset || !in->img_pair_offset)
    return fail(VETO_ERR_INVALID, "missing input pointer");
  if (!in->obj_labels && !in->obj_logits) return fail(VETO_ERR_INVALID, "neither obj_labels nor obj_logits given");
  if (!in->bn_batch_stats && !sch.bn_eval) return fail(VETO_ERR_INVALID, "the training path needs bn_batch_stats (training-mode BatchNorm)");
  if (h->cfg.precision == VETO_FAST) return fail(VETO_ERR_INVALID, "the training path runs on split-bf16 operands (precise / mixed handles) only");
  ABI_TRY(check_train_opts(opts));
  if (workspace_bytes < carve_train(nullptr, h, in->n_obj, in->n_pair, opts_ordered(opts), sch).total)
    return fail(VETO_ERR_WORKSPACE, !sch.full ? "training workspace too small (veto_train_workspace_bytes_plan)" : opts_ordered(opts) ? "training workspace too small (ordered mode: veto_train_workspace_bytes_opts)" : "training workspace too small");
  return VETO_OK;
}

}  // namespace

extern "C" {

size_t veto_train_workspace_bytes(veto_handle_t h, int32_t n_obj, int32_t n_pair) {
  if (!h || n_obj <= 0 || n_pair <= 0) return 0;
  return carve_train(nullptr, h, n_obj, n_pair).total;
}

size_t veto_train_workspace_bytes_opts(veto_handle_t h, int32_t n_obj, int32_t n_pair, const veto_train_opts_t* opts) {
  if (!h || n_obj <= 0 || n_pair <= 0 || check_train_opts(opts) != VETO_OK) return 0;
  return carve_train(nullptr, h, n_obj, n_pair, opts_ordered(opts)).total;
}

size_t veto_train_workspace_bytes_plan(veto_handle_t h, int32_t n_obj, int32_t n_pair, const veto_train_opts_t* opts,
                                       const veto_train_plan_t* plan) {
  if (!plan) return veto_train_workspace_bytes_opts(h, n_obj, n_pair, opts);
  Sched sch;
  if (!h || n_obj <= 0 || n_pair <= 0 || check_train_opts(opts) != VETO_OK || make_sched(h, opts, plan, &sch) != VETO_OK) return 0;
  return carve_train(nullptr, h, n_obj, n_pair, opts_ordered(opts), sch).total;
}

static int forward_train_impl(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, const Sched& sch,
                              void* workspace, size_t workspace_bytes, float* out_logits) {
  ABI_TRY(check_train_inputs(h, in, opts, workspace, workspace_bytes, sch));
  if (!out_logits) return fail(VETO_ERR_INVALID, "null out_logits");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->dirty) ABI_TRY(finalize_weights(h, s, true));
  h->train_gen.erase(workspace);     // (stamped at the end: a failed forward leaves no workspace that veto_backward would accept)
  h->train_plan.erase(workspace);
  const int n_obj = in->n_obj, n_pair = in->n_pair, L = h->cfg.layers, H = h->cfg.heads, n_out = h->cfg.num_out;
  const int M = n_pair * kTokens;
  TrainWs ws = carve_train((char*)workspace, h, n_obj, n_pair, opts_ordered(opts), sch);
  HIP_TRY(launch_pair_indices(in->rel_pairs, in->img_obj_offset, in->img_pair_offset, in->n_img, n_pair, ws.subj, ws.obj, nullptr,
                              nullptr, s));
  {
    veto_inputs_t in_bn = *in;      // (an eval-mode pos_embed.0: the running statistics, as the inference forward reads them)
    if (sch.bn_eval) in_bn.bn_batch_stats = nullptr;
    else HIP_TRY(launch_bn_batch_stats(in->boxes, in->box_mode, n_obj, in->bn_batch_stats, s));
    ObjPrepArgs a = obj_prep_args(h, &in_bn, ws.lc);
    const DropSite d = drop_site(opts, 1);
    a.drop_seed = d.seed; a.drop_thresh = d.thresh; a.drop_scale = d.scale;
    HIP_TRY(launch_obj_prep(a, s));
  }
  HIP_TRY(launch_patchify(in->roi_depth, in->roi_rgb, ws.pa, n_obj, s));
  ABI_TRY(run_gemm(h, s, "gemm_patch", ws.pa, h->patch_w, h->patch_bias, nullptr, 0, ws.patch_tab, nullptr, 2 * kDim, n_obj * 16,
                   2 * kDim, 2048, EPI_F32));
  {
    AssembleArgs a = assemble_args(h, ws.patch_tab, ws.lc, ws.subj, ws.obj, ws.layers[0].xin, ws.layers[0].a1, n_pair);
    const DropSite d = drop_site(opts, 2);
    a.drop_seed = d.seed; a.drop_thresh = d.thresh; a.drop_scale = d.scale;
    HIP_TRY(launch_assemble(a, s));
  }
  const bool q24 = train_qkv_f24(h);
  const int qepi = q24 ? EPI_F24 : EPI_F32;
  for (int l = 0; l < L; ++l) {
    const LayerW& w = h->layers[l];
    TrainLayer& t = ws.layers[l];
    if (l == L - 1) {
      // Last layer: only x[:, 0] reaches the loss (model_veto.py:23), so -- as at inference -- keys / values cover the 19
      // tokens, everything behind the attention runs on the CLS row of each pair.  The saved activations of this layer
      // (ao, xmid, a2, pre, hid, ws.xout) are COMPACT: row p = pair p.  The backward mirrors this.
      ABI_TRY(run_gemm(h, s, "gemm_kv_last", t.a1, w.qkv, nullptr, nullptr, 0, q24 ? (float*)((char*)t.qkv + 3 * kDim) : t.qkv + kDim, nullptr,
                       3 * kDim, M, 2 * kDim, kDim, qepi, 0, kDim));
      ABI_TRY(run_gemm(h, s, "gemm_q_cls", t.a1, w.qkv, nullptr, nullptr, 0, t.qkv, nullptr, (long)kTokens * 3 * kDim, n_pair, kDim, kDim,
                       qepi, (long)kTokens * 2 * kDim, 0));
      {
        AttnArgs a{};
        a.qkv = t.qkv; a.n_pair = n_pair; a.heads = H; a.cls_only = 1; a.o = t.ao; a.qkv_f24 = q24 ? 1 : 0;
        HIP_TRY(launch_attention(a, s));
      }
      ABI_TRY(run_gemm(h, s, "gemm_out_cls", t.ao, w.out, w.out_b, t.xin, (long)kTokens * kDim, t.xmid, nullptr, kDim, n_pair, kDim, kDim,
                       EPI_RESID, 0, 0, drop_site(opts, 3 + l, kTokens, &sch)));
      HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, n_pair, s));
      ABI_TRY(run_gemm(h, s, "gemm_fc1_cls", t.a2, w.fc1, w.fc1_b, nullptr, 0, t.pre, t.hid, 4 * kDim, n_pair, 2 * kDim, kDim, EPI_PRE_GELU));
      ABI_TRY(run_gemm(h, s, "gemm_fc2_cls", t.hid, w.fc2, w.fc2_b, t.xmid, kDim, ws.xout, nullptr, kDim, n_pair, kDim, 2 * kDim, EPI_RESID));
      break;
    }
    float* xnext = ws.layers[l + 1].xin;
    ABI_TRY(run_gemm(h, s, "gemm_qkv", t.a1, w.qkv, nullptr, nullptr, 0, t.qkv, nullptr, 3 * kDim, M, 3 * kDim, kDim, qepi));
    {
      AttnArgs a{};
      a.qkv = t.qkv; a.n_pair = n_pair; a.heads = H; a.cls_only = 0; a.o = t.ao; a.qkv_f24 = q24 ? 1 : 0;
      HIP_TRY(launch_attention(a, s));
    }
    ABI_TRY(run_gemm(h, s, "gemm_out", t.ao, w.out, w.out_b, t.xin, kDim, t.xmid, nullptr, kDim, M, kDim, kDim, EPI_RESID, 0, 0,
                     drop_site(opts, 3 + l, 1, &sch)));
    HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, M, s));
    // (the epilogue writes the fp32 pre-activation -- gelu' needs it -- AND its exact-erf GELU as fc2's split rows: round 6; before, a pass
    // of its own read the pre-activation back, 0.55 ms per layer)
    ABI_TRY(run_gemm(h, s, "gemm_fc1", t.a2, w.fc1, w.fc1_b, nullptr, 0, t.pre, t.hid, 4 * kDim, M, 2 * kDim, kDim, EPI_PRE_GELU));
    ABI_TRY(run_gemm(h, s, "gemm_fc2", t.hid, w.fc2, w.fc2_b, t.xmid, kDim, xnext, nullptr, kDim, M, kDim, 2 * kDim, EPI_RESID));
    HIP_TRY(launch_layernorm(xnext, kDim, h->layers[l + 1].ln1_w, h->layers[l + 1].ln1_b, ws.layers[l + 1].a1, M, s));
  }
  HIP_TRY(launch_head(ws.xout, h->head_wt, h->p("rel_out.bias"), out_logits, n_pair, n_out, s, (long)kDim));
  h->stamp_train_workspace(workspace);
  if (!sch.full) h->train_plan[workspace] = sch.key;
  return VETO_OK;
}

int veto_forward_train(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, void* workspace,
                       size_t workspace_bytes, float* out_logits) {
  return forward_train_impl(h, stream, in, opts, Sched(), workspace, workspace_bytes, out_logits);
}

int veto_forward_train_plan(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts,
                            const veto_train_plan_t* plan, void* workspace, size_t workspace_bytes, float* out_logits) {
  if (!plan) return veto_forward_train(h, stream, in, opts, workspace, workspace_bytes, out_logits);
  if (!h) return fail(VETO_ERR_INVALID, "null argument");
  ABI_TRY(check_train_opts(opts));
  Sched sch;
  ABI_TRY(make_sched(h, opts, plan, &sch));
  return forward_train_impl(h, stream, in, opts, sch, workspace, workspace_bytes, out_logits);
}

static int backward_impl(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, const Sched& sch,
                         void* workspace, size_t workspace_bytes, const float* dlogits, float* grads) {
  ABI_TRY(check_train_inputs(h, in, opts, workspace, workspace_bytes, sch));
  if (!dlogits || !grads) return fail(VETO_ERR_INVALID, "null gradient pointer");
  if (!sch.maps && opts && (opts->d_roi_rgb || opts->d_roi_depth))
    return fail(VETO_ERR_INVALID, "veto_backward_plan: d_roi_rgb / d_roi_depth asked for under a plan with d_roi == 0");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->cfg.device));
  // the backward reads the derived operands the matching forward used: a weight upload in between would pair this
  // workspace's activations with different weights
  if (h->dirty) return fail(VETO_ERR_WEIGHTS, "weights were reloaded between veto_forward_train and veto_backward");
  {
    auto it = h->train_gen.find(workspace);
    if (it == h->train_gen.end()) return fail(VETO_ERR_INVALID, "veto_backward: this workspace holds no veto_forward_train activations");
    if (it->second != h->weight_gen)
      return fail(VETO_ERR_WEIGHTS, "veto_backward: the weights were refreshed (by a later forward) since this workspace's veto_forward_train");
    auto pl = h->train_plan.find(workspace);
    if (sch.full ? pl != h->train_plan.end() : pl == h->train_plan.end() || pl->second != sch.key)
      return fail(VETO_ERR_INVALID, "veto_backward: this workspace's forward ran under another plan (veto_train_plan_t) than this backward");
  }
  const int n_obj = in->n_obj, n_pair = in->n_pair, L = h->cfg.layers, H = h->cfg.heads, n_out = h->cfg.num_out, E = h->cfg.embed_dim;
  const int M = n_pair * kTokens;
  const bool ordered = opts_ordered(opts);
  TrainWs ws = carve_train((char*)workspace, h, n_obj, n_pair, ordered, sch);
  const std::string T = kT;
  // (a frozen tensor has no gradient pointer: every launch below that would only write it is left out)
  auto W = [&](const std::string& name) { return sch.want(h, name); };
  auto G = [&](const std::string& name) -> float* { return W(name) ? grads + h->params[h->index.at(name)].offset : nullptr; };
  auto copy_grad = [&](const std::string& name, const float* src, size_t n) {
    float* g = G(name);
    return g ? hipMemcpyAsync(g, src, n * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
  };
  struct LinGrad { const float* w; float *dw, *db; int N, K; };      // a layer's Linear (kLayerLinears): weight, its and the bias's gradient
  auto lin = [&](int l, int i) {
    const LayerLinear& q = kLayerLinears[i];
    return LinGrad{h->p(lname(l, q.weight)), G(lname(l, q.weight)), q.bias ? G(lname(l, q.bias)) : nullptr, q.N, q.K};
  };
  if (sch.full) {
    HIP_TRY(hipMemsetAsync(grads, 0, veto_grad_floats(h) * 4, s));
  } else {      // the regions of the trainable tensors only, neighbours in one fill (tensors lie in index order, padded to 64 floats)
    for (size_t i = 0; i < h->params.size();) {
      if (!sch.on[i]) { ++i; continue; }
      size_t j = i;
      while (j + 1 < h->params.size() && sch.on[j + 1]) ++j;
      HIP_TRY(hipMemsetAsync(grads + h->params[i].offset, 0, (h->params[j].offset + h->params[j].numel - h->params[i].offset) * 4, s));
      i = j + 1;
    }
  }
  HIP_TRY(hipMemsetAsync(ws.zero, 0, 1024, s));

  // ---- classifier head: gradient of the compact CLS rows (not written when nothing under the head has a consumer) --------
  HIP_TRY(launch_head_backward(dlogits, h->p("rel_out.weight"), ws.xout, sch.keep_from < L ? ws.dx : nullptr, G("rel_out.weight"),
                               G("rel_out.bias"), ws.head_partial, n_pair, n_out, (long)kDim, s));

  // ---- transformer layers, last to first -------------------------------------------------------------------------
  // A layer's stages in chain order: fc2, fc1, LayerNorm2, out, attention, qkv, LayerNorm1.  own[i]: stage i has a trainable tensor;
  // deeper[i]: something behind it (in this layer, a lower one or under layer 0) has a consumer, so its input gradient is computed.
  // The walk ends behind the first stage with deeper[i] == false: every later stage of every lower layer is without a consumer too.
  int dx_presplit = 0;      // > 0: ws.dsplit / ws.colp already hold the split rows / that many rows of column partials of ws.dx
  for (int l = L - 1; l >= sch.keep_from; --l) {
    const LayerW& w = h->layers[l];
    TrainLayer& t = ws.layers[l];
    const bool last = l == L - 1;
    const int R = last ? n_pair : M;     // rows behind the attention: the CLS rows only in the last layer (compact buffers)
    // x_out = x_mid + gelu(LN2(x_mid) W1^T + b1) W2^T + b2
    // dpre = dh * gelu'(pre): in the epilogue of fc2's input-gradient GEMM (round 6; VETO_TRAIN_GELU_EPI=0: a pass of its own inside the
    // operand preparation of the fc1 backward, rounds 1-5)
    // (the gradient of this layer's output: compact CLS rows from the head in the last layer, else the rows the LayerNorm1 backward of the
    // layer above left -- with their split rows and bias partials when it emitted them)
    const float* dy2 = dx_presplit ? nullptr : ws.dx;
    const bool recompute = train_recompute();
    const LinGrad qkv = lin(l, LIN_QKV), out = lin(l, LIN_OUT), fc1 = lin(l, LIN_FC1), fc2 = lin(l, LIN_FC2);
    const bool ln1 = W(lname(l, "0.norm.weight")) || W(lname(l, "0.norm.bias")), ln2 = W(lname(l, "1.norm.weight")) || W(lname(l, "1.norm.bias"));
    enum { S_FC2, S_FC1, S_LN2, S_OUT, S_ATTN, S_QKV, S_LN1, S_COUNT };
    const bool own[S_COUNT] = {fc2.dw || fc2.db, fc1.dw || fc1.db, ln2, out.dw || out.db, false, qkv.dw != nullptr, ln1};
    bool deeper[S_COUNT];
    for (int i = S_COUNT - 1, acc = sch.need(l); i >= 0; --i) {
      deeper[i] = acc;
      acc = acc || own[i];
    }
    if (recompute && fc2.dw) HIP_TRY(launch_gelu_split(t.pre, t.hid, (size_t)R, 2 * kDim, s));      // gelu(pre): fc2's operand, as the forward's epilogue wrote it
    if (train_gelu_epilogue()) {
      int partials = 0;
      ABI_TRY(run_linear_backward(h, s, ws, dy2, R, fc2.N, t.hid, fc2.K, fc2.w, fc2.dw, fc2.db, nullptr, GradXform(), nullptr, dx_presplit,
                                  deeper[S_FC2] ? t.pre : nullptr, &partials));
      if (!deeper[S_FC2]) break;
      if (recompute && fc1.dw) HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, R, s));      // LayerNorm2 rows: fc1's operand
      ABI_TRY(run_linear_backward(h, s, ws, nullptr, R, fc1.N, t.a2, fc1.K, fc1.w, fc1.dw, fc1.db, deeper[S_FC1] ? ws.dtmp : nullptr, GradXform(),
                                  ws.dsplit_b, partials));
    } else {
      ABI_TRY(run_linear_backward(h, s, ws, dy2, R, fc2.N, t.hid, fc2.K, fc2.w, fc2.dw, fc2.db, deeper[S_FC2] ? ws.dbig : nullptr, GradXform(), nullptr,
                                  dx_presplit));
      if (!deeper[S_FC2]) break;
      GradXform gelu;              // dpre = dh * gelu'(pre), folded into the operand preparation of the fc1 backward
      gelu.mode = XF_GELU;
      gelu.pre = t.pre;
      if (recompute && fc1.dw) HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, R, s));
      ABI_TRY(run_linear_backward(h, s, ws, ws.dbig, R, fc1.N, t.a2, fc1.K, fc1.w, fc1.dw, fc1.db, deeper[S_FC1] ? ws.dtmp : nullptr, gelu));
    }
    if (!deeper[S_FC1]) break;
    // x_mid = x_in + dropout(attention(LN1(x_in) Wqkv^T) Wo^T + bo): the projection sees the masked gradient
    const DropSite dsite = drop_site(opts, 3 + l, l == L - 1 ? kTokens : 1, &sch);      // (last layer: compact CLS rows, as in the forward)
    const bool ln_split = train_ln_emits_split();
    if (ln_split)
      HIP_TRY(launch_layernorm_backward(t.xmid, ws.dtmp, w.ln2_w, ws.dx, ws.dmid, ln2 ? ws.dgb : nullptr, ws.ln_partial, R, s, ws.dsplit, ws.colp,
                                        dsite.seed, dsite.thresh, dsite.scale, dsite.row_step, ordered));
    else
      HIP_TRY(launch_layernorm_backward(t.xmid, ws.dtmp, w.ln2_w, ws.dx, ws.dmid, ln2 ? ws.dgb : nullptr, ws.ln_partial, R, s, nullptr, nullptr, 0, 0, 1.f, 1,
                                        ordered));
    HIP_TRY(copy_grad(lname(l, "1.norm.weight"), ws.dgb, kDim));
    HIP_TRY(copy_grad(lname(l, "1.norm.bias"), ws.dgb + kDim, kDim));
    if (!deeper[S_LN2]) break;
    GradXform drop;
    if (dsite.thresh) {
      drop.mode = XF_DROP;
      drop.seed = dsite.seed;
      drop.thresh = dsite.thresh;
      drop.scale = dsite.scale;
      drop.row_step = dsite.row_step;
    }
    ABI_TRY(run_linear_backward(h, s, ws, ln_split ? nullptr : ws.dmid, R, out.N, t.ao, out.K, out.w, out.dw, out.db, deeper[S_OUT] ? ws.dtmp : nullptr,
                                drop, nullptr, ln_split ? layernorm_backward_col_partials(R) : 0));
    if (!deeper[S_OUT]) break;
    HIP_TRY(launch_attention_backward(t.qkv, ws.dtmp, nullptr, ws.dsplit, n_pair, H, last ? 1 : 0, s, train_qkv_f24(h)));
    if (recompute && qkv.dw) HIP_TRY(launch_layernorm(t.xin, kDim, w.ln1_w, w.ln1_b, t.a1, M, s));      // LayerNorm1 rows: the QKV projection's operand
    ABI_TRY(run_linear_backward(h, s, ws, nullptr, M, qkv.N, t.a1, qkv.K, qkv.w, qkv.dw, qkv.db, deeper[S_QKV] ? ws.dtmp : nullptr));
    if (!deeper[S_QKV]) break;
    const float* dres = ws.dmid;
    if (last) {
      // the residual gradient d x_mid lives on the CLS rows only: spread the compact rows over a zeroed token matrix
      HIP_TRY(hipMemsetAsync(ws.dx, 0, (size_t)M * kDim * 4, s));
      HIP_TRY(hipMemcpy2DAsync(ws.dx, (size_t)kTokens * kDim * 4, ws.dmid, (size_t)kDim * 4, (size_t)kDim * 4, (size_t)n_pair,
                               hipMemcpyDeviceToDevice, s));
      dres = ws.dx;
    }
    // (in the last layer dres == ws.dx is also the output: every element is read and written by the same thread)
    if (ln_split && l > 0) {      // (its result is the gradient matrix of fc2 of the layer below)
      HIP_TRY(launch_layernorm_backward(t.xin, ws.dtmp, w.ln1_w, dres, ws.dx, ln1 ? ws.dgb : nullptr, ws.ln_partial, M, s, ws.dsplit, ws.colp, 0, 0, 1.f, 1,
                                        ordered));
      dx_presplit = layernorm_backward_col_partials(M);
    } else {
      HIP_TRY(launch_layernorm_backward(t.xin, ws.dtmp, w.ln1_w, dres, ws.dx, ln1 ? ws.dgb : nullptr, ws.ln_partial, M, s, nullptr, nullptr, 0, 0, 1.f, 1,
                                        ordered));
      dx_presplit = 0;
    }
    HIP_TRY(copy_grad(lname(l, "0.norm.weight"), ws.dgb, kDim));
    HIP_TRY(copy_grad(lname(l, "0.norm.bias"), ws.dgb + kDim, kDim));
  }
  if (!sch.below) return VETO_OK;      // (the walk above ended inside a layer, or behind layer keep_from)

  // ---- token assembly: cls_token, pos_embedding, per-object tables -----------------------------------------------
  // x0[p, t] = token + pos_embedding (ONE 576-vector broadcast over all tokens, model_veto.py:43,62): its gradient is
  // the sum over every token row; the cls_token's is the sum over row 0 of every pair
  {
    const DropSite d = drop_site(opts, 2);   // pos_drop sits between (token + pos_embedding) and the first layer
    if (d.thresh) HIP_TRY(launch_dropout_apply(ws.dx, ws.dx, (size_t)M, kDim, d.seed, d.thresh, d.scale, s));
  }
  if (float* g = G(T + "pos_embedding")) HIP_TRY(launch_column_sums(ws.dx, kDim, M, kDim, g, ws.col_partial, column_sums_chunks(), s));
  if (float* g = G(T + "cls_token")) HIP_TRY(launch_column_sums(ws.dx, (long)kTokens * kDim, n_pair, kDim, g, ws.col_partial, column_sums_chunks(), s));
  const std::string pe = T + "patch_embed.";
  const bool want_maps = opts && (opts->d_roi_rgb || opts->d_roi_depth);
  const bool patch_w = W(pe + "proj_d.weight") || W(pe + "proj_v.weight"), patch_b = W(pe + "proj_d.bias") || W(pe + "proj_v.bias");
  const bool pos_side = W("pos_embed.0.weight") || W("pos_embed.0.bias") || W("pos_embed.1.weight") || W("pos_embed.1.bias");
  const bool loc_w = W("location_projection.0.weight"), cls_w = W("class_projection.0.weight"), emb_w = W("obj_embed.weight");
  const bool lc_side = pos_side || loc_w || cls_w || emb_w || W("location_projection.0.bias") || W("class_projection.0.bias");
  if (!(patch_w || patch_b || want_maps || lc_side)) return VETO_OK;
  if (ordered) {
    HIP_TRY(launch_assemble_backward_ordered(ws.dx, ws.subj, ws.obj, ws.lc, in->img_obj_offset, in->img_pair_offset, in->n_img, ws.dpatch,
                                             ws.dlc, n_obj, s));
  } else {
    HIP_TRY(hipMemsetAsync(ws.dpatch, 0, (size_t)n_obj * 16 * 2 * kDim * 4, s));
    HIP_TRY(hipMemsetAsync(ws.dlc, 0, (size_t)n_obj * 2 * 2 * kDim * 4, s));
    HIP_TRY(launch_assemble_backward(ws.dx, ws.subj, ws.obj, ws.lc, ws.dpatch, ws.dlc, n_pair, s));
  }

  // ---- patch projection: patch_tab = PA . Wcat^T + bias_cat (bias only on the subject half) ------------------------
  {
    const int R = n_obj * 16;
    if (patch_w || want_maps) HIP_TRY(launch_split_rows(ws.dpatch, ws.dsplit, (size_t)R, 2 * kDim, s));
    // dWcat^T [2048, 1152] = PA^T . dpatch: "dy" = PA (split rows), "x" = dpatch (fp32) in run_wgrad's roles swapped,
    // so that the output width (1152) is a multiple of 192
    if (patch_w) {
      const int N = 2048, K = 2 * kDim;
      const int ks = wgrad_splits(N, K, R, 0, 8);      // (few object rows: tiles of 8 k-steps already)
      const size_t mp = wgrad_mp(R, ks);
      if (!ordered) HIP_TRY(hipMemsetAsync(ws.dwcat_t, 0, (size_t)N * K * 4, s));
      GemmArgs g{};
      g.a = ws.pa; g.w = ws.dsplit; g.c = ordered ? ws.planes : ws.dwcat_t;
      g.M = N; g.N = K; g.K = (int)mp; g.ldc = K; g.k_splits = ks;
      g.tn = 1; g.lda = 2 * (long)N; g.ldw = 2 * (long)K; g.k_valid = R; g.zero = ws.zero;
      HIP_TRY(launch_gemm_split(g, ordered ? EPI_PLANES : EPI_ATOMIC, 0, s));
      if (ordered) HIP_TRY(launch_fold_rows(ws.planes, (long)N * K, ks, (long)N * K, ws.dwcat_t, s));
      HIP_TRY(launch_patch_weight_grad(ws.dwcat_t, G(pe + "proj_d.weight"), G(pe + "proj_v.weight"), s));
    }
    // biases: column sums of the subject half of dpatch: columns 0..511 -> proj_d.bias, 512..575 -> proj_v.bias
    if (patch_b) {
      HIP_TRY(launch_column_sums(ws.dpatch, 2 * kDim, R, kDim, ws.dgb, ws.col_partial, column_sums_chunks(), s));
      HIP_TRY(copy_grad(pe + "proj_d.bias", ws.dgb, 512));
      HIP_TRY(copy_grad(pe + "proj_v.bias", ws.dgb + 512, 64));
    }
    // input gradient (optional): dPA = dpatch . Wcat, i.e. the forward GEMM kernel on split(dpatch) (still in ws.dsplit) and
    // Wcat^T as the weight operand; then the inverse of patchify onto the ROI maps.  The reference's depth backbone is
    // trained through roi_depth_features (tools/relation_train_net.py:166-170).
    if (want_maps) {
      HIP_TRY(launch_build_patch_weight_t(h->p(pe + "proj_d.weight"), h->p(pe + "proj_v.weight"), ws.wcat_t, s));
      GemmArgs g{};
      g.a = ws.dsplit; g.w = ws.wcat_t; g.c = ws.dpa;
      g.M = R; g.N = kPatchTRows; g.K = 2 * kDim; g.ldc = kPatchTRows;
      HIP_TRY(launch_gemm_split(g, EPI_F32, 0, s));
      HIP_TRY(launch_unpatchify(ws.dpa, kPatchTRows, opts->d_roi_depth, opts->d_roi_rgb, n_obj, s));
    }
  }

  // ---- location / class projections and what feeds them -----------------------------------------------------------
  if (lc_side) {
    const long ldlc = 2 * 2 * kDim;   // dlc row n = [location 1152 | class 1152]
    // biases sit on the subject half
    if (float* g = G("location_projection.0.bias")) HIP_TRY(launch_column_sums(ws.dlc, ldlc, n_obj, kDim, g, ws.col_partial, column_sums_chunks(), s));
    if (float* g = G("class_projection.0.bias")) HIP_TRY(launch_column_sums(ws.dlc + 2 * kDim, ldlc, n_obj, kDim, g, ws.col_partial, column_sums_chunks(), s));
    const DropSite dpos_site = drop_site(opts, 1);   // Dropout(0.1) behind the ReLU of pos_embed
    if (pos_side || loc_w) {      // (the location projection's weight gradient reads bn_out, which obj_pos_backward recomputes)
      // position branch: recompute pos (post-ReLU) through the masked gradient path
      //   dpos = dlc_loc . loc_wt^T ; obj_pos_backward -> dpre (ReLU'), BatchNorm affine gradients
      HIP_TRY(launch_sgemm_nt(ws.dlc, ldlc, h->loc_wt, 2 * kDim, ws.dpos, kPosDim, n_obj, kPosDim, 2 * kDim, s));
      if (dpos_site.thresh) HIP_TRY(launch_dropout_apply(ws.dpos, ws.dpos, (size_t)n_obj, kPosDim, dpos_site.seed, dpos_site.thresh, dpos_site.scale, s));
      // (what the forward normalised with: this batch's statistics, or the running ones of an eval-mode pos_embed.0)
      const float* bn_mean = sch.bn_eval ? h->p("pos_embed.0.running_mean") : in->bn_batch_stats;
      const float* bn_var = sch.bn_eval ? h->p("pos_embed.0.running_var") : in->bn_batch_stats + 4;
      HIP_TRY(launch_obj_pos_backward(in->boxes, in->box_mode, bn_mean, bn_var, h->p("pos_embed.0.weight"), h->p("pos_embed.0.bias"),
                                      h->p("pos_embed.1.weight"), h->p("pos_embed.1.bias"), ws.dpos, ws.dpre, ws.xhat, ws.bn_out, ws.dbn_out,
                                      G("pos_embed.0.weight"), G("pos_embed.0.bias"), n_obj, s));
    }
    // pos_embed.1: Linear(4, 128): dW[k, c] = sum_n dpre[n, k] bn_out[n, c]; db = column sums of dpre
    if (float* g = G("pos_embed.1.weight")) HIP_TRY(launch_sgemm_tn(ws.dpre, kPosDim, ws.bn_out, 4, g, 4, n_obj, kPosDim, 4, s));
    if (float* g = G("pos_embed.1.bias")) HIP_TRY(launch_column_sums(ws.dpre, kPosDim, n_obj, kPosDim, g, ws.col_partial, column_sums_chunks(), s));
    if (loc_w) {
      // location_projection weight: d loc_wt[k, j] = sum_n pos[n, k] dlc_loc[n, j], pos = relu(pre): recompute pos = the
      // forward's value; it equals (dpre != 0 ? ... ) no -- recompute it from bn_out
      // pos[n, k] = relu(pos_b[k] + sum_c pos_w[k, c] bn_out[n, c]): one small product + ReLU, done by reusing dpos as storage
      HIP_TRY(launch_sgemm_nt(ws.bn_out, 4, h->p("pos_embed.1.weight"), 4, ws.dpos, kPosDim, n_obj, kPosDim, 4, s));
      HIP_TRY(launch_bias_relu(ws.dpos, h->p("pos_embed.1.bias"), n_obj, kPosDim, s));
      if (dpos_site.thresh) HIP_TRY(launch_dropout_apply(ws.dpos, ws.dpos, (size_t)n_obj, kPosDim, dpos_site.seed, dpos_site.thresh, dpos_site.scale, s));
      HIP_TRY(launch_sgemm_tn(ws.dpos, kPosDim, ws.dlc, ldlc, ws.dloc_wt, 2 * kDim, n_obj, kPosDim, 2 * kDim, s));
      HIP_TRY(launch_untranspose_pair_proj(ws.dloc_wt, G("location_projection.0.weight"), kPosDim, s));
    }
    // class branch: emb = E[label] (hard labels) or softmax(logits) . E (sgcls, :4092-4095);
    // d cls_wt[k, j] = sum_n emb[n, k] dlc_cls[n, j]; demb = dlc_cls . cls_wt^T
    const int C_obj = h->cfg.num_obj_cls;
    if (in->obj_logits && (cls_w || emb_w)) HIP_TRY(launch_softmax_rows(in->obj_logits, ws.prob, n_obj, C_obj, s));
    if (cls_w) {
      if (in->obj_logits) HIP_TRY(launch_sgemm_nn(ws.prob, C_obj, h->p("obj_embed.weight"), E, ws.emb, E, n_obj, E, C_obj, s));
      else HIP_TRY(launch_gather_rows(h->p("obj_embed.weight"), in->obj_labels, E, ws.emb, n_obj, s));
      HIP_TRY(launch_sgemm_tn(ws.emb, E, ws.dlc + 2 * kDim, ldlc, ws.dcls_wt, 2 * kDim, n_obj, E, 2 * kDim, s));
      HIP_TRY(launch_untranspose_pair_proj(ws.dcls_wt, G("class_projection.0.weight"), E, s));
    }
    if (float* g = G("obj_embed.weight")) {
      HIP_TRY(launch_sgemm_nt(ws.dlc + 2 * kDim, ldlc, h->cls_wt, 2 * kDim, ws.demb, E, n_obj, E, 2 * kDim, s));
      if (in->obj_logits) HIP_TRY(launch_sgemm_tn(ws.prob, C_obj, ws.demb, E, g, E, n_obj, C_obj, E, s));
      else if (ordered) HIP_TRY(launch_scatter_rows_ordered(ws.demb, in->obj_labels, E, g, n_obj, C_obj, s));
      else HIP_TRY(launch_scatter_rows(ws.demb, in->obj_labels, E, g, n_obj, s));
    }
  }
  return VETO_OK;
}

int veto_backward(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, void* workspace,
                  size_t workspace_bytes, const float* dlogits, float* grads) {
  return backward_impl(h, stream, in, opts, Sched(), workspace, workspace_bytes, dlogits, grads);
}

int veto_backward_plan(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, const veto_train_plan_t* plan,
                       void* workspace, size_t workspace_bytes, const float* dlogits, float* grads) {
  if (!plan) return veto_backward(h, stream, in, opts, workspace, workspace_bytes, dlogits, grads);
  if (!h) return fail(VETO_ERR_INVALID, "null argument");
  ABI_TRY(check_train_opts(opts));
  Sched sch;
  ABI_TRY(make_sched(h, opts, plan, &sch));
  return backward_impl(h, stream, in, opts, sch, workspace, workspace_bytes, dlogits, grads);
}

// workspace: lse | nll_w | w_row | inv_wsum
static size_t carve_ce_loss(Carver c, size_t n, CeLossArgs* a) {
  a->lse = c.take<float>(n * 4);
  a->nll_w = c.take<float>(n * 4);
  a->w_row = c.take<float>(n * 4);
  a->inv_wsum = c.take<float>(256);
  return c.off;
}

size_t veto_ce_loss_workspace_bytes(int32_t n) {
  if (n <= 0) return 0;
  CeLossArgs a{};
  return carve_ce_loss(Carver{nullptr}, n, &a);
}

int veto_ce_loss(void* stream, const float* logits, int64_t ld, const int64_t* labels, const float* weight,
                 const int64_t* rows, int32_t n, int32_t n_cls, float* loss, float* grad, void* workspace,
                 size_t workspace_bytes) {
  if (!logits || !labels || !loss || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (n <= 0 || n_cls < 2 || ld < n_cls) return fail(VETO_ERR_INVALID, "bad sizes (n %d, n_cls %d, ld %lld)", n, n_cls, (long long)ld);
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_ce_loss_workspace_bytes(n), false));
  CeLossArgs a{};
  a.logits = logits; a.ld = ld; a.labels = labels; a.weight = weight; a.rows = rows; a.n = n; a.C = n_cls;
  carve_ce_loss(Carver{(char*)workspace}, n, &a);
  a.loss = loss; a.grad = grad;
  HIP_TRY(launch_ce_loss(a, (hipStream_t)stream));
  return VETO_OK;
}

int veto_meet_sample(void* stream, const int64_t* labels, int32_t n, const uint32_t* words, int32_t n_words,
                     const int32_t* incre_idx_list, const int32_t* pos_in_group, const int32_t* group_size,
                     const double* sample_rates, int32_t n_groups, int32_t n_cls, int64_t* chosen,
                     int64_t* group_labels, int32_t* counts, int32_t* words_used) {
  if (!labels || !words || !incre_idx_list || !pos_in_group || !group_size || !sample_rates || !chosen || !group_labels ||
      !counts || !words_used)
    return fail(VETO_ERR_INVALID, "null argument");
  if (n <= 0 || n_words <= 0 || n_groups < 1 || n_groups > 64 || n_cls < 2) return fail(VETO_ERR_INVALID, "bad sizes");
  MeetSampleArgs a{};
  a.labels = labels; a.n = n; a.n_groups = n_groups; a.n_cls = n_cls; a.n_words = n_words; a.words = words;
  a.incre = incre_idx_list; a.pos_in_group = pos_in_group; a.group_size = group_size; a.rates = sample_rates;
  a.chosen = chosen; a.group_labels = group_labels; a.counts = counts; a.words_used = words_used;
  HIP_TRY(launch_meet_sample(a, (hipStream_t)stream));
  return VETO_OK;
}

// n % 32 == 0 (every Linear of the transformer): the row-major form, both operands as the split rows the backward holds
// anyway, transposed on their way out of LDS (GemmArgs::tn), one row more than m each (partial tiles read, never use, the row behind
// the last) and the zero row of GemmArgs::zero.  Otherwise: explicit transposed split copies, dy's padded to whole row tiles.
// ordered: behind the operands, the k_splits partial planes [n, k] fp32 of the ordered form (operand bytes: the size of the default form)
struct WgradWs { __bf16 *a, *w, *zero; size_t operand_bytes; float* planes; size_t total; };
static WgradWs carve_wgrad(Carver c, int m, int n, int k, int k_splits, bool ordered = false) {      // (a braced list evaluates left to right)
  const int ks = wgrad_splits(n, k, m, k_splits);
  const size_t plane_bytes = ordered ? (size_t)ks * n * k * 4 : 0;
  if (n % 32 == 0) return WgradWs{c.take<__bf16>(((size_t)m + 1) * n * 4), c.take<__bf16>(((size_t)m + 1) * k * 4), c.take<__bf16>(1024), c.off,
                                  ordered ? c.take<float>(plane_bytes) : nullptr, c.off};
  const size_t mp = wgrad_mp(m, ks);
  return WgradWs{c.take<__bf16>((size_t)gemm_rows_padded(n) * mp * 4), c.take<__bf16>((size_t)k * mp * 4), nullptr, c.off,
                 ordered ? c.take<float>(plane_bytes) : nullptr, c.off};
}

static int debug_wgrad(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k, int32_t k_splits,
                       void* workspace, size_t workspace_bytes, bool ordered);

size_t veto_debug_wgrad_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t k_splits) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return carve_wgrad(Carver{nullptr}, m, n, k, k_splits).total;
}

size_t veto_debug_wgrad_ordered_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t k_splits) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return carve_wgrad(Carver{nullptr}, m, n, k, k_splits, true).total;
}

int veto_debug_wgrad(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k,
                     int32_t k_splits, void* workspace, size_t workspace_bytes) {
  return debug_wgrad(stream, dy, x, dw, m, n, k, k_splits, workspace, workspace_bytes, false);
}

int veto_debug_wgrad_ordered(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k,
                             int32_t k_splits, void* workspace, size_t workspace_bytes) {
  return debug_wgrad(stream, dy, x, dw, m, n, k, k_splits, workspace, workspace_bytes, true);
}

static int debug_wgrad(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k, int32_t k_splits,
                       void* workspace, size_t workspace_bytes, bool ordered) {
  if (!dy || !x || !dw || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (m <= 0 || n <= 0 || k <= 0 || k % 192 != 0) return fail(VETO_ERR_INVALID, "k must be a positive multiple of 192");
  const WgradWs ws = carve_wgrad(Carver{(char*)workspace}, m, n, k, k_splits, ordered);
  ABI_TRY(check_workspace(workspace, workspace_bytes, ws.total, false));
  hipStream_t s = (hipStream_t)stream;
  const int ks = wgrad_splits(n, k, m, k_splits);
  const size_t mp = wgrad_mp(m, ks);
  if (!ordered) HIP_TRY(hipMemsetAsync(dw, 0, (size_t)n * k * 4, s));
  GemmArgs g{};
  g.a = ws.a; g.w = ws.w; g.c = ordered ? ws.planes : dw;
  g.M = n; g.N = k; g.K = (int)mp; g.ldc = k; g.k_splits = ks;
  if (n % 32 == 0) {
    HIP_TRY(hipMemsetAsync(ws.a, 0, ws.operand_bytes, s));   // the row behind the last one is read (never used) by partial tiles
    HIP_TRY(launch_split_rows(dy, ws.a, (size_t)m, n, s));
    HIP_TRY(launch_split_rows(x, ws.w, (size_t)m, k, s));
    g.tn = 1; g.lda = 2 * (long)n; g.ldw = 2 * (long)k; g.k_valid = m;
    g.zero = ws.zero;
  } else {
    HIP_TRY(hipMemsetAsync(ws.a, 0, (char*)ws.w - (char*)ws.a, s));   // rows n..padded stay zero
    HIP_TRY(launch_transpose_split(dy, n, m, n, ws.a, (int)mp, s));
    HIP_TRY(launch_transpose_split(x, k, m, k, ws.w, (int)mp, s));
  }
  hipError_t e = launch_gemm_split(g, ordered ? EPI_PLANES : EPI_ATOMIC, 0, s);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "wgrad gemm launch failed: %s", hipGetErrorString(e));
  if (ordered) HIP_TRY(launch_fold_rows(ws.planes, (long)n * k, ks, (long)n * k, dw, s));
  return VETO_OK;
}

int veto_debug_attention_backward(void* stream, const float* qkv, const float* dout, float* dqkv, int32_t n_pair, int32_t heads) {
  if (!qkv || !dout || !dqkv || n_pair <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  hipError_t e = launch_attention_backward(qkv, dout, dqkv, nullptr, n_pair, heads, 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "attention backward: %s (heads must give a head width of 72, 96 or 144)", hipGetErrorString(e));
  return VETO_OK;
}

int veto_debug_attention_backward_forms(void* stream, const void* qkv, const float* dout, void* dqkv, float* qkv_unpacked, int32_t n_pair,
                                        int32_t heads, uint32_t flags) {
  if (!qkv || !dout || !dqkv || n_pair <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  if (flags & ~(uint32_t)(VETO_ATTN_BWD_CLS_ONLY | VETO_ATTN_BWD_QKV_F24 | VETO_ATTN_BWD_SPLIT_OUT)) return fail(VETO_ERR_INVALID, "unknown flag");
  const bool f24 = (flags & VETO_ATTN_BWD_QKV_F24) != 0, split = (flags & VETO_ATTN_BWD_SPLIT_OUT) != 0;
  hipStream_t s = (hipStream_t)stream;
  if (qkv_unpacked) {
    if (!f24) return fail(VETO_ERR_INVALID, "qkv_unpacked goes with VETO_ATTN_BWD_QKV_F24");
    HIP_TRY(launch_unpack_f24(qkv, qkv_unpacked, (size_t)n_pair * kTokens * 3 * kDim, s));
  }
  hipError_t e = launch_attention_backward((const float*)qkv, dout, split ? nullptr : (float*)dqkv, split ? (__bf16*)dqkv : nullptr, n_pair, heads,
                                           (flags & VETO_ATTN_BWD_CLS_ONLY) ? 1 : 0, s, f24);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "attention backward: %s (head width 72, 96 or 144; 3-byte q / k / v with 72 or 96 only)", hipGetErrorString(e));
  return VETO_OK;
}

size_t veto_debug_layernorm_backward_workspace_bytes(int32_t rows) { return rows > 0 ? layernorm_backward_partial_floats(rows) * 4 : 0; }

int veto_debug_layernorm_backward(void* stream, const float* x, const float* dy, const float* gamma, const float* dres,
                                  float* dx, float* dgamma_dbeta, int32_t rows, void* workspace, size_t workspace_bytes) {
  if (!x || !dy || !gamma || !dx || !dgamma_dbeta || !workspace || rows <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  if (workspace_bytes < veto_debug_layernorm_backward_workspace_bytes(rows)) return fail(VETO_ERR_WORKSPACE, "workspace too small");
  HIP_TRY(launch_layernorm_backward(x, dy, gamma, dres, dx, dgamma_dbeta, (float*)workspace, rows, (hipStream_t)stream));
  return VETO_OK;
}

int32_t veto_debug_layernorm_backward_col_partial_rows(int32_t rows) { return rows > 0 ? layernorm_backward_col_partials(rows) : 0; }

int veto_debug_layernorm_backward_split(void* stream, const float* x, const float* dy, const float* gamma, const float* dres, float* dx,
                                        float* dgamma_dbeta, void* split_rows, float* col_partials, int32_t rows, uint64_t drop_seed,
                                        uint32_t drop_thresh, float drop_scale, void* workspace, size_t workspace_bytes) {
  if (!x || !dy || !gamma || !dx || !dgamma_dbeta || !split_rows || !col_partials || !workspace || rows <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  if (drop_thresh >= (1u << 24)) return fail(VETO_ERR_INVALID, "drop_thresh is p * 2^24 with p < 1");
  if (workspace_bytes < veto_debug_layernorm_backward_workspace_bytes(rows)) return fail(VETO_ERR_WORKSPACE, "workspace too small");
  HIP_TRY(launch_layernorm_backward(x, dy, gamma, dres, dx, dgamma_dbeta, (float*)workspace, rows, (hipStream_t)stream, (__bf16*)split_rows,
                                    col_partials, (unsigned long long)drop_seed, drop_thresh, drop_scale));
  return VETO_OK;
}

int veto_debug_layernorm_backward_ordered(void* stream, const float* x, const float* dy, const float* gamma, const float* dres, float* dx,
                                          float* dgamma_dbeta, void* split_rows, float* col_partials, int32_t rows, uint64_t drop_seed,
                                          uint32_t drop_thresh, float drop_scale, void* workspace, size_t workspace_bytes) {
  if (!x || !dy || !gamma || !dx || !dgamma_dbeta || !workspace || rows <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  if (!split_rows != !col_partials) return fail(VETO_ERR_INVALID, "split_rows and col_partials go together");
  if (drop_thresh >= (1u << 24)) return fail(VETO_ERR_INVALID, "drop_thresh is p * 2^24 with p < 1");
  if (workspace_bytes < veto_debug_layernorm_backward_workspace_bytes(rows)) return fail(VETO_ERR_WORKSPACE, "workspace too small");
  HIP_TRY(launch_layernorm_backward(x, dy, gamma, dres, dx, dgamma_dbeta, (float*)workspace, rows, (hipStream_t)stream, (__bf16*)split_rows,
                                    col_partials, (unsigned long long)drop_seed, drop_thresh, drop_scale, 1, true));
  return VETO_OK;
}

int veto_debug_assemble_backward_ordered(void* stream, const float* dx, const int32_t* subj, const int32_t* obj, const float* lc,
                                         const int32_t* img_obj_offset, const int32_t* img_pair_offset, int32_t n_img, int32_t n_obj,
                                         float* dpatch, float* dlc) {
  if (!dx || !subj || !obj || !lc || !img_obj_offset || !img_pair_offset || !dpatch || !dlc || n_img <= 0 || n_obj <= 0)
    return fail(VETO_ERR_INVALID, "bad argument");
  HIP_TRY(launch_assemble_backward_ordered(dx, subj, obj, lc, img_obj_offset, img_pair_offset, n_img, dpatch, dlc, n_obj, (hipStream_t)stream));
  return VETO_OK;
}

int veto_debug_scatter_rows_ordered(void* stream, const float* demb, const int64_t* labels, int32_t n, int32_t dim, int32_t n_table_rows,
                                    float* dtable) {
  if (!demb || !labels || !dtable || n <= 0 || dim <= 0 || n_table_rows <= 0) return fail(VETO_ERR_INVALID, "bad argument");
  HIP_TRY(launch_scatter_rows_ordered(demb, labels, dim, dtable, n, n_table_rows, (hipStream_t)stream));
  return VETO_OK;
}

int veto_debug_gelu_backward(void* stream, const float* pre, const float* dh, float* dpre, size_t n) {
  if (!pre || !dh || !dpre || n == 0 || n % 4 != 0) return fail(VETO_ERR_INVALID, "bad argument (n must be a positive multiple of 4)");
  HIP_TRY(launch_gelu_backward(pre, dh, dpre, n, (hipStream_t)stream));
  return VETO_OK;
}

int veto_debug_column_sums(void* stream, const float* dy, int64_t ld, int32_t rows, int32_t n_cols, float* out, void* workspace,
                           size_t workspace_bytes) {
  if (!dy || !out || !workspace || rows <= 0 || n_cols <= 0 || ld < n_cols) return fail(VETO_ERR_INVALID, "bad argument");
  if (workspace_bytes < (size_t)column_sums_chunks() * n_cols * 4) return fail(VETO_ERR_WORKSPACE, "workspace too small (256 * n_cols floats)");
  HIP_TRY(launch_column_sums(dy, ld, rows, n_cols, out, (float*)workspace, column_sums_chunks(), (hipStream_t)stream));
  return VETO_OK;
}

// ---- veto_optim_step ------------------------------------------------------------------------------------------------------
static_assert(VETO_OPTIM_CHUNK == kOptimChunk, "the header's chunk size is the kernels'");

// Does the tensor take part in this call?
static bool optim_active(const veto_optim_tensor_t& t) { return t.grad != nullptr && t.numel > 0; }

// the host fields every mode checks; *n_chunks: the rows of the chunk table
static int optim_check_shapes(const veto_optim_args_t* a, long long* n_chunks) {
  if (a->tensor_size != (int32_t)sizeof(veto_optim_tensor_t)) return fail(VETO_ERR_INVALID, "veto_optim_tensor_t size mismatch");
  if (a->n_tensors < 1 || a->n_tensors > kOptimMaxTensors) return fail(VETO_ERR_INVALID, "n_tensors %d outside 1..%d", a->n_tensors, kOptimMaxTensors);
  if (a->mode < VETO_OPTIM_NORMS || a->mode > VETO_OPTIM_CLIP_STEP) return fail(VETO_ERR_INVALID, "unknown mode %d", a->mode);
  if (!a->tensors) return fail(VETO_ERR_INVALID, "missing pointer: tensors");
  long long chunks = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    if (t.numel < 0 || t.numel >= (1ll << 31)) return fail(VETO_ERR_INVALID, "tensor %d: numel %lld outside 0..2^31 - 1", i, (long long)t.numel);
    if (optim_active(t)) chunks += (t.numel + kOptimChunk - 1) / kOptimChunk;
  }
  if (chunks > kOptimMaxChunks) return fail(VETO_ERR_INVALID, "%lld chunks of %d elements, the limit is %d", chunks, kOptimChunk, kOptimMaxChunks);
  *n_chunks = chunks;
  return VETO_OK;
}

// The tables as the device reads them: [counter, 256 bytes][OptimTensor x n_tensors][OptimChunk x n_chunks], each part at a multiple
// of 256 bytes; this prefix of the workspace is what the call uploads.  Behind it: partial [n_chunks] and tensor_sq [n_tensors] doubles.
// (offsets, not pointers: the pinned staging copy of the prefix has the same layout)
struct OptimLayout { size_t tensors, chunks, upload, partial, tensor_sq, total; };
static OptimLayout optim_layout(int n_tensors, long long n_chunks) {
  OptimLayout l;
  Carver c{nullptr};
  c.take_offset(256);      // the counter
  l.tensors = c.take_offset((size_t)n_tensors * sizeof(OptimTensor));
  l.chunks = c.take_offset((size_t)n_chunks * sizeof(OptimChunk));
  l.upload = l.chunks + (size_t)n_chunks * sizeof(OptimChunk);      // (the upload ends with the table's last row, not with its region)
  l.partial = c.take_offset((size_t)n_chunks * 8);
  l.tensor_sq = c.take_offset((size_t)n_tensors * 8);
  l.total = c.off;
  return l;
}

size_t veto_optim_step_workspace_bytes(const veto_optim_args_t* a) {
  if (!a || a->struct_size != (int32_t)sizeof(veto_optim_args_t)) return 0;
  long long n_chunks = 0;
  if (optim_check_shapes(a, &n_chunks) != VETO_OK) return 0;
  return optim_layout(a->n_tensors, n_chunks).total;
}

// Pinned staging for the tables, one buffer per call in flight.  A buffer is taken again only when the event recorded behind the
// call that used it has completed, so rewriting it cannot reach a copy that has not run yet.
struct OptimStage { void* host = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; int device = -1; };
static std::mutex g_optim_mutex;
static std::vector<OptimStage> g_optim_stages;
constexpr size_t kOptimMaxStages = 256;

static int optim_stage_acquire(size_t need, int device, OptimStage** out) {
  OptimStage* idle_small = nullptr;
  for (OptimStage& st : g_optim_stages) {
    if (st.device != device || hipEventQuery(st.done) != hipSuccess) continue;
    if (st.bytes >= need) { *out = &st; return VETO_OK; }
    idle_small = &st;
  }
  (void)hipGetLastError();   // hipErrorNotReady of a busy buffer is no error
  OptimStage* st = idle_small;
  if (!st && g_optim_stages.size() >= kOptimMaxStages) {   // 256 calls in flight on this device: wait for the oldest buffer
    for (OptimStage& o : g_optim_stages)
      if (o.device == device) { st = &o; break; }
    if (!st) return fail(VETO_ERR_HIP, "no staging buffer left for device %d", device);
    HIP_TRY(hipEventSynchronize(st->done));
    if (st->bytes >= need) { *out = st; return VETO_OK; }
  }
  if (st) {   // idle and too small: the parameter set grew
    HIP_TRY(hipHostFree(st->host));
    st->host = nullptr; st->bytes = 0;
  } else {
    g_optim_stages.emplace_back();
    st = &g_optim_stages.back();
    st->device = device;
    HIP_TRY(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
  }
  size_t bytes = 64 << 10;
  while (bytes < need) bytes *= 2;
  HIP_TRY(hipHostMalloc(&st->host, bytes, hipHostMallocDefault));
  st->bytes = bytes;
  *out = st;
  return VETO_OK;
}

int veto_optim_step(void* stream, const veto_optim_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_optim_args_t, a);
  long long n_chunks = 0;
  ABI_TRY(optim_check_shapes(a, &n_chunks));
  const bool norms = a->mode != VETO_OPTIM_STEP, steps = a->mode == VETO_OPTIM_STEP || a->mode == VETO_OPTIM_CLIP_STEP;
  const bool clips = a->mode == VETO_OPTIM_CLIP || a->mode == VETO_OPTIM_CLIP_STEP;
  if (clips && !(a->max_norm > 0.0)) return fail(VETO_ERR_INVALID, "max_norm %g must be > 0 in a mode that clips", a->max_norm);
  if (norms && (!a->norms || !a->total_norm || !a->coef)) return fail(VETO_ERR_INVALID, "missing pointer: norms, total_norm and coef are required");
  if (norms && (((uintptr_t)a->norms | (uintptr_t)a->total_norm | (uintptr_t)a->coef) & 3) != 0) return fail(VETO_ERR_INVALID, "misaligned norms, total_norm or coef");
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    if (!optim_active(t)) continue;
    if (((uintptr_t)t.grad & 3) != 0) return fail(VETO_ERR_INVALID, "tensor %d: misaligned grad", i);
    if (!steps) continue;
    if (t.step < 1) return fail(VETO_ERR_INVALID, "tensor %d: step %lld must be >= 1 (the count including this update)", i, (long long)t.step);
    if (!t.param || !t.exp_avg || !t.exp_avg_sq) return fail(VETO_ERR_INVALID, "tensor %d: missing pointer: param, exp_avg and exp_avg_sq are required", i);
    if ((((uintptr_t)t.param | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 3) != 0) return fail(VETO_ERR_INVALID, "tensor %d: misaligned param, exp_avg or exp_avg_sq", i);
    if (!(t.lr >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: lr %g must be >= 0", i, t.lr);
    if (!(t.eps >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: eps %g must be >= 0", i, t.eps);
    if (!(t.weight_decay >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: weight_decay %g must be >= 0", i, t.weight_decay);
    if (!(t.beta1 >= 0.0 && t.beta1 < 1.0)) return fail(VETO_ERR_INVALID, "tensor %d: beta1 %g outside [0, 1)", i, t.beta1);
    if (!(t.beta2 >= 0.0 && t.beta2 < 1.0)) return fail(VETO_ERR_INVALID, "tensor %d: beta2 %g outside [0, 1)", i, t.beta2);
  }
  const OptimLayout lay = optim_layout(a->n_tensors, n_chunks);
  ABI_TRY(check_workspace(workspace, workspace_bytes, lay.total, true));

  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_optim_mutex);
  OptimStage* st = nullptr;
  ABI_TRY(optim_stage_acquire(lay.upload, device, &st));
  char* host = (char*)st->host;
  memset(host, 0, 256);   // the counter
  OptimTensor* rows = (OptimTensor*)(host + lay.tensors);
  OptimChunk* chunk_rows = (OptimChunk*)(host + lay.chunks);
  int next = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    OptimTensor r{};
    r.numel = (int)t.numel; r.chunk0 = next;
    if (optim_active(t)) {
      r.p = t.param; r.g = t.grad; r.m = t.exp_avg; r.v = t.exp_avg_sq;
      r.n_chunks = (int)((t.numel + kOptimChunk - 1) / kOptimChunk);
      for (int k = 0; k < r.n_chunks; ++k) chunk_rows[next++] = OptimChunk{i, k};
      if (steps) {
        const double bc1 = 1.0 - pow(t.beta1, (double)t.step), bc2 = 1.0 - pow(t.beta2, (double)t.step);
        r.wd = (float)t.weight_decay; r.beta1 = (float)t.beta1; r.omb1 = (float)(1.0 - t.beta1);
        r.beta2 = (float)t.beta2; r.omb2 = (float)(1.0 - t.beta2); r.eps = (float)t.eps;
        r.step_size = (float)(t.lr / bc1); r.bc2_sqrt = (float)sqrt(bc2);
      }
    }
    rows[i] = r;
  }
  char* ws = (char*)workspace;
  OptimArgs p{};
  p.tensors = (const OptimTensor*)(ws + lay.tensors); p.chunks = (const OptimChunk*)(ws + lay.chunks); p.counter = (unsigned*)ws;
  p.partial = (double*)(ws + lay.partial); p.tensor_sq = (double*)(ws + lay.tensor_sq);
  p.n_tensors = a->n_tensors; p.n_chunks = (int)n_chunks; p.max_norm = a->max_norm;
  p.norms = a->norms; p.total = a->total_norm; p.coef = a->coef;
  HIP_TRY(hipMemcpyAsync(ws, host, lay.upload, hipMemcpyHostToDevice, (hipStream_t)stream));
  const hipError_t e = launch_optim(p, norms, a->mode == VETO_OPTIM_CLIP ? 1 : steps ? 2 : 0, clips, (hipStream_t)stream);
  HIP_TRY(hipEventRecord(st->done, (hipStream_t)stream));   // behind the copy, whatever became of the launches
  if (e != hipSuccess) return fail(VETO_ERR_HIP, "launch_optim failed: %s", hipGetErrorString(e));
  return VETO_OK;
}

}  // extern "C"
