// ================================================================================================================
// Training path: the forward that keeps every activation the backward needs, and the backward itself.
// One pass over all pairs (no chunking) on split-bf16 operands.  Layers 0 .. L-2 run on all 19 tokens; the last layer's attention
// reads the 19 keys / values but only the CLS query of each pair, and everything behind it (out projection, FeedForward, head) runs
// on the compact CLS rows, as at inference.  Dropout runs on the device (drop_site: masks from a counter-based hash that forward and
// backward both evaluate); veto_train_opts_t.deterministic selects the ordered mode (every gradient sum in a fixed order); a
// veto_train_plan_t (Sched) leaves out what frozen tensors and an eval-mode pos_embed.0 do not need.
// A step is a TrainStep: one method per stage, which forward_train_impl and backward_impl call in order.
// ================================================================================================================
#include "abi_internal.h"

#include <algorithm>

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
  __bf16* wcat_t;   // Wcat^T [patch_t_rows(p), 2*1152] split rows: weight operand of the patch projection's input gradient
  float* dpa;       // dPA [prow, patch_t_rows(p)] fp32: gradient w.r.t. the patch rows
  size_t mp2;    // padded reduction length of the weight-gradient GEMMs
  // the frozen-fused step (Sched::fused) only: the workspace of the frozen region's inference forward (abi_forward.hip, frozen_forward)
  char* infer;
  size_t infer_bytes;
  // ordered mode (veto_train_opts_t.deterministic) only, behind everything else so that the default layout and size stay what they were:
  // the split-K partial planes of the weight-gradient GEMMs, [k_splits][N][K] fp32 of the largest call; nullptr = the default (atomic) path
  float* planes;
  size_t total;
};

// q / k / v of the training path as 3-byte floats (common.h) between the QKV projection, the attention and the attention backward: 1.7 KB
// per token row and layer less to keep and to move (round 6).  They carry 16 significant bits by default: what the backward, which splits
// them into bf16 hi + lo, would have kept anyway -- but 6 fewer than the forward's attention (fp16 hi + lo planes) keeps of fp32 rows;
// VETO_TRAIN_QKV_F24=0 (fp32 rows) restores the forward's 22.  MFMA head widths only.
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

// The split of the weight-gradient GEMMs of the step (abi_internal.h, wgrad_split): a layer's Linear [n, k] over m rows, and the patch
// projection's dWcat^T [patch_feats(p), 1152] over the object rows
WgradSplit linear_wgrad_split(int n, int k, int m) { return wgrad_split(n, k, m, 0, kWgradLinearKsteps, kWgradLinearCap); }
WgradSplit patch_wgrad_split(int patch, int rows) { return wgrad_split(patch_feats(patch), 2 * kDim, rows, 0, kWgradPatchKsteps, 0); }

// the ordered mode's planes hold the largest of them
size_t wgrad_plane_floats(int patch, int m_tokens, int patch_rows) {
  size_t most = patch_wgrad_split(patch, patch_rows).plane_floats;
  for (const LayerLinear& q : kLayerLinears) most = std::max(most, linear_wgrad_split(q.N, q.K, m_tokens).plane_floats);      // (the last layer's compact rows are fewer: no more splits)
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
  // veto_train_plan_t.frozen_fused: the prelude and layers < keep_from run as the inference forward in a workspace region of its own
  // and keep nothing; layer keep_from's input rows are its hand-off (keep_from == layers: the CLS rows in xout)
  bool fused = false;
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
  // (the frozen-fused step: the prelude runs in the frozen region's own workspace, and nothing under layer keep_from is differentiated)
  const auto prelude = [&](size_t bytes) { return sch.fused ? (size_t)0 : bytes; };
  w.subj = c.take<int32_t>(prelude((size_t)n_pair * 4));
  w.obj = c.take<int32_t>(prelude((size_t)n_pair * 4));
  w.lc = c.take<float>(prelude((size_t)n_obj * 2 * 2 * kDim * 4));
  const int patch = h->cfg.patch;
  w.pa = c.take<__bf16>(prelude(prow * 2 * patch_feats(patch) * 2));
  w.patch_tab = c.take<float>(prelude((size_t)n_obj * 16 * 2 * kDim * 4));
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
    if (sch.fused && l < sch.keep_from) {      // a layer of the frozen region: no buffers here
      t = TrainLayer{};
      continue;
    }
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
  w.dwcat_t = c.take<float>((size_t)patch_feats(patch) * 2 * kDim * 4);
  w.wcat_t = c.take<__bf16>((size_t)patch_t_rows(patch) * 2 * 2 * kDim * 2);
  w.dpa = c.take<float>((size_t)gemm_rows_padded(n_obj * 16) * patch_t_rows(patch) * 4);
  w.planes = ordered ? c.take<float>(wgrad_plane_floats(patch, (int)M, n_obj * 16) * 4) : nullptr;
  w.infer_bytes = sch.fused ? frozen_forward_workspace_bytes(h, n_obj, n_pair, sch.keep_from) : 0;
  w.infer = sch.fused ? c.take(w.infer_bytes) : nullptr;
  w.total = c.off;
  return w;
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
  std::vector<std::string> prelude;      // the tensors under layer 0
  for (const char* name : {"pos_embed.0.weight", "pos_embed.0.bias", "pos_embed.1.weight", "pos_embed.1.bias", "obj_embed.weight",
                           "location_projection.0.weight", "location_projection.0.bias", "class_projection.0.weight", "class_projection.0.bias"})
    prelude.push_back(name);
  for (const char* name : {"pos_embedding", "cls_token", "patch_embed.proj_d.weight", "patch_embed.proj_d.bias", "patch_embed.proj_v.weight",
                           "patch_embed.proj_v.bias"})
    prelude.push_back(T + name);
  for (const std::string& name : prelude) sch.below = sch.below || sch.want(h, name);
  sch.fused = plan->frozen_fused != 0;
  if (sch.fused) {      // what the frozen-fused step refuses, part 1 (include/veto_amd.h): what would make the chain reach under layer 0
    for (const std::string& name : prelude)
      if (sch.want(h, name)) return fail(VETO_ERR_INVALID, "frozen_fused: '%s' is trainable inside the frozen prelude", name.c_str());
    if (sch.maps) return fail(VETO_ERR_INVALID, "frozen_fused: d_roi != 0 (the map gradients run through the frozen prelude)");
    if (!sch.bn_eval) return fail(VETO_ERR_INVALID, "frozen_fused: bn_eval == 0 (the frozen prelude normalises with the running statistics of pos_embed.0)");
  }
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
  sch.key.push_back(sch.fused ? 'F' : '-');
  if (sch.fused) {      // part 2: the frozen region is layers < k = keep_from (nothing under layer 0 has a consumer), the inference forward
    const int k = sch.keep_from;
    if (k == 0) return fail(VETO_ERR_INVALID, "frozen_fused: layer 0 has a trainable tensor (k = 0: there is no frozen layer to run fused)");
    if (opts && opts->p_pos > 0.f) return fail(VETO_ERR_INVALID, "frozen_fused: p_pos = %g, the frozen prelude runs without dropout", opts->p_pos);
    if (opts && opts->p_emb > 0.f) return fail(VETO_ERR_INVALID, "frozen_fused: p_emb = %g, the frozen prelude runs without dropout", opts->p_emb);
    for (int l = 0; l < k; ++l) {
      const float p = !sch.p_attn.empty() ? sch.p_attn[l] : opts ? opts->p_attn : 0.f;
      if (p > 0.f) return fail(VETO_ERR_INVALID, "frozen_fused: attention dropout rate %g in frozen layer %d (p_attn_layer), the frozen layers run without dropout", p, l);
    }
    if (h->cfg.precision == VETO_FAST)
      return fail(VETO_ERR_INVALID, "frozen_fused: a VETO_FAST handle (its logit error is above the 1e-3 bar of a training step's forward)");
    if (env_knob_is("VETO_X_F24", "1")) return fail(VETO_ERR_INVALID, "frozen_fused: VETO_X_F24=1 (the hand-off takes fp32 residual rows)");
  }
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

// One training step on its way through the stages: what every stage needs, and one method per stage -- the forward's in the order
// forward_train_impl calls them, then the backward's in the order of the chain (Sched)
struct TrainStep {
  veto_handle_t h;
  hipStream_t s;
  const veto_inputs_t* in;
  const veto_train_opts_t* opts;
  const Sched& sch;
  float* grads;      // (backward only) laid out like the weight arena
  const bool ordered;
  const TrainWs ws;
  const int n_obj, n_pair, M, L, H;
  const bool q24, recompute;
  const std::string T = kT, pe = T + "patch_embed.";
  int dx_presplit = 0;      // > 0: ws.dsplit / ws.colp already hold the split rows / that many rows of column partials of ws.dx

  TrainStep(veto_handle_t h_, void* stream, const veto_inputs_t* in_, const veto_train_opts_t* opts_, const Sched& sch_, void* workspace,
            float* grads_ = nullptr)
      : h(h_), s((hipStream_t)stream), in(in_), opts(opts_), sch(sch_), grads(grads_), ordered(opts_ordered(opts_)),
        ws(carve_train((char*)workspace, h_, in_->n_obj, in_->n_pair, ordered, sch_)), n_obj(in_->n_obj), n_pair(in_->n_pair),
        M(in_->n_pair * kTokens), L(h_->cfg.layers), H(h_->cfg.heads), q24(train_qkv_f24(h_)), recompute(train_recompute()) {}

  // (a frozen tensor has no gradient pointer: every launch of the backward that would only write it is left out)
  bool W(const std::string& name) const { return sch.want(h, name); }
  float* G(const std::string& name) const { return W(name) ? grads + h->params[h->index.at(name)].offset : nullptr; }
  hipError_t copy_grad(const std::string& name, const float* src, size_t n) const {
    float* g = G(name);
    return g ? hipMemcpyAsync(g, src, n * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
  }
  struct LinGrad { const float* w; float *dw, *db; int N, K; };      // a layer's Linear (kLayerLinears): weight, its and the bias's gradient
  LinGrad lin(int l, int i) const {
    const LayerLinear& q = kLayerLinears[i];
    return LinGrad{h->p(lname(l, q.weight)), G(lname(l, q.weight)), q.bias ? G(lname(l, q.bias)) : nullptr, q.N, q.K};
  }
  // the dropout behind the out projection of layer l (the last layer: on its compact CLS rows)
  DropSite attn_site(int l) const { return drop_site(opts, 3 + l, l == L - 1 ? kTokens : 1, &sch); }

  // ---- forward -----------------------------------------------------------------------------------------------------------
  // pair indices, BatchNorm statistics and the per-object embeddings
  int object_side() {
    HIP_TRY(launch_pair_indices(in->rel_pairs, in->img_obj_offset, in->img_pair_offset, in->n_img, n_pair, ws.subj, ws.obj, nullptr, nullptr, s));
    veto_inputs_t in_bn = *in;      // (an eval-mode pos_embed.0: the running statistics, as the inference forward reads them)
    if (sch.bn_eval) in_bn.bn_batch_stats = nullptr;
    else HIP_TRY(launch_bn_batch_stats(in->boxes, in->box_mode, n_obj, in->bn_batch_stats, s));
    ObjPrepArgs a = obj_prep_args(h, &in_bn, ws.lc);
    set_drop(a, drop_site(opts, 1));
    HIP_TRY(launch_obj_prep(a, s));
    return VETO_OK;
  }

  // The frozen-fused step: the prelude and layers < k = sch.keep_from as the inference forward.  k == L: that is the whole forward, and
  // it leaves the logits and the CLS rows (ws.xout); else layer k's input rows, and here their LayerNorm1 rows as the layer below
  // would have left them
  int frozen_region(float* out_logits) {
    const int k = sch.keep_from;
    ABI_TRY(frozen_forward(h, s, in, ws.infer, ws.infer_bytes, k, k < L ? ws.layers[k].xin : nullptr, out_logits, k < L ? nullptr : ws.xout));
    if (k < L) HIP_TRY(launch_layernorm(ws.layers[k].xin, kDim, h->layers[k].ln1_w, h->layers[k].ln1_b, ws.layers[k].a1, M, s));
    return VETO_OK;
  }

  int patch_projection() {
    HIP_TRY(launch_patchify(in->roi_depth, in->roi_rgb, ws.pa, n_obj, h->cfg.patch, s));
    return run_gemm(h, s, "gemm_patch", ws.pa, h->patch_w, h->patch_bias, nullptr, 0, ws.patch_tab, nullptr, 2 * kDim, n_obj * 16, 2 * kDim, patch_feats(h->cfg.patch),
                    EPI_F32);
  }

  // the token rows of layer 0 and their LayerNorm1 rows
  int assemble_tokens() {
    AssembleArgs a = assemble_args(h, ws.patch_tab, ws.lc, ws.subj, ws.obj, ws.layers[0].xin, ws.layers[0].a1, n_pair);
    set_drop(a, drop_site(opts, 2));
    HIP_TRY(launch_assemble(a, s));
    return VETO_OK;
  }

  int attention(const TrainLayer& t, int cls_only) {
    AttnArgs a{};
    a.qkv = t.qkv; a.n_pair = n_pair; a.heads = H; a.cls_only = cls_only; a.o = t.ao; a.qkv_f24 = q24 ? 1 : 0;
    HIP_TRY(launch_attention(a, s));
    return VETO_OK;
  }

  // a layer but the last, on all token rows; it leaves the LayerNorm1 rows of the next
  int layer(int l) {
    const LayerW& w = h->layers[l];
    const TrainLayer &t = ws.layers[l], &next = ws.layers[l + 1];
    ABI_TRY(run_gemm(h, s, "gemm_qkv", t.a1, w.qkv, nullptr, nullptr, 0, t.qkv, nullptr, 3 * kDim, M, 3 * kDim, kDim, q24 ? EPI_F24 : EPI_F32));
    ABI_TRY(attention(t, 0));
    ABI_TRY(run_gemm(h, s, "gemm_out", t.ao, w.out, w.out_b, t.xin, kDim, t.xmid, nullptr, kDim, M, kDim, kDim, EPI_RESID, 0, 0, attn_site(l)));
    HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, M, s));
    // (the epilogue writes the fp32 pre-activation -- gelu' needs it -- AND its exact-erf GELU as fc2's split rows: round 6; before, a pass
    // of its own read the pre-activation back, 0.55 ms per layer)
    ABI_TRY(run_gemm(h, s, "gemm_fc1", t.a2, w.fc1, w.fc1_b, nullptr, 0, t.pre, t.hid, 4 * kDim, M, 2 * kDim, kDim, EPI_PRE_GELU));
    ABI_TRY(run_gemm(h, s, "gemm_fc2", t.hid, w.fc2, w.fc2_b, t.xmid, kDim, next.xin, nullptr, kDim, M, kDim, 2 * kDim, EPI_RESID));
    HIP_TRY(launch_layernorm(next.xin, kDim, h->layers[l + 1].ln1_w, h->layers[l + 1].ln1_b, next.a1, M, s));
    return VETO_OK;
  }

  // Last layer: only x[:, 0] reaches the loss (model_veto.py:23), so -- as at inference -- keys / values cover the 19
  // tokens, everything behind the attention runs on the CLS row of each pair.  The saved activations of this layer
  // (ao, xmid, a2, pre, hid, ws.xout) are COMPACT: row p = pair p.  The backward mirrors this.
  int last_layer() {
    const int l = L - 1, qepi = q24 ? EPI_F24 : EPI_F32;
    const LayerW& w = h->layers[l];
    const TrainLayer& t = ws.layers[l];
    ABI_TRY(run_gemm(h, s, "gemm_kv_last", t.a1, w.qkv, nullptr, nullptr, 0, q24 ? (float*)((char*)t.qkv + 3 * kDim) : t.qkv + kDim, nullptr,
                     3 * kDim, M, 2 * kDim, kDim, qepi, 0, kDim));
    ABI_TRY(run_gemm(h, s, "gemm_q_cls", t.a1, w.qkv, nullptr, nullptr, 0, t.qkv, nullptr, (long)kTokens * 3 * kDim, n_pair, kDim, kDim, qepi,
                     (long)kTokens * 2 * kDim, 0));
    ABI_TRY(attention(t, 1));
    ABI_TRY(run_gemm(h, s, "gemm_out_cls", t.ao, w.out, w.out_b, t.xin, (long)kTokens * kDim, t.xmid, nullptr, kDim, n_pair, kDim, kDim, EPI_RESID,
                     0, 0, attn_site(l)));
    HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, n_pair, s));
    ABI_TRY(run_gemm(h, s, "gemm_fc1_cls", t.a2, w.fc1, w.fc1_b, nullptr, 0, t.pre, t.hid, 4 * kDim, n_pair, 2 * kDim, kDim, EPI_PRE_GELU));
    return run_gemm(h, s, "gemm_fc2_cls", t.hid, w.fc2, w.fc2_b, t.xmid, kDim, ws.xout, nullptr, kDim, n_pair, kDim, 2 * kDim, EPI_RESID);
  }

  int head(float* out_logits) {
    HIP_TRY(launch_head(ws.xout, h->head_wt, h->p("rel_out.bias"), out_logits, n_pair, h->cfg.num_out, s, (long)kDim));
    return VETO_OK;
  }

  // ---- backward ----------------------------------------------------------------------------------------------------------
  // Backward of y = x W^T (+ b) over `rows` token rows: dW[N, K] = dY^T x, db[N] = column sums of dY (if q.db), dX[rows, K] = dY W.
  // One pass over dY (prep_grad_kernel) produces its split rows -- the A operand of the input-gradient GEMM AND, read through
  // transposing LDS loads, of the weight-gradient GEMM (launch_wgrad; the saved activation x_split is its other operand as it
  // is) -- and the bias partials.  No transposed copies of dY or x exist.
  // dy == nullptr: the producer (attention backward) has already written the split rows into ws.dsplit; no bias then.
  // presplit / presplit_partials: the producer wrote the split rows itself (to `presplit`; nullptr = ws.dsplit) together with
  // `presplit_partials` rows of column sums in ws.colp (0 = none: no bias gradient then).
  // gelu_pre (fc2 only): the input gradient is not written as fp32 rows: the GEMM's epilogue multiplies it by gelu'(gelu_pre) and writes the
  // split rows of fc1's backward to ws.dsplit_b and their column-sum partials to ws.colp (*next_partials rows): the pass that read dH and the
  // pre-activation back (0.9 ms per layer) is gone.
  // Partial training: q.dw == nullptr (a frozen weight) leaves out the weight-gradient GEMM with its zero-fill or fold, q.db == nullptr the
  // bias sums, dx == nullptr without gelu_pre (nothing below this Linear has a consumer) the weight transpose and the input-gradient GEMM.
  int linear_backward(const float* dy, int rows, const LinGrad& q, const __bf16* x_split, float* dx, const GradXform& xf = GradXform(),
                      const __bf16* presplit = nullptr, int presplit_partials = 0, const float* gelu_pre = nullptr, int* next_partials = nullptr) {
    const int N = q.N, K = q.K;
    if (!dy && q.db && presplit_partials <= 0) return fail(VETO_ERR_INVALID, "a pre-split gradient without column partials cannot feed a bias gradient");
    const __bf16* gsplit = !dy && presplit ? presplit : ws.dsplit;
    const WgradSplit sp = linear_wgrad_split(N, K, rows);
    if (sp.mp > ws.mp2) return fail(VETO_ERR_WORKSPACE, "weight-gradient partial buffer too small");
    if (dy) HIP_TRY(launch_prep_grad(dy, N, rows, N, ws.dsplit, (int)sp.mp, q.db ? ws.colp : nullptr, xf, s));
    if (q.db) HIP_TRY(launch_column_sums(ws.colp, N, dy ? (int)(sp.mp / 32) : presplit_partials, N, q.db, ws.col_partial, column_sums_chunks(), s));
    if (q.dw) HIP_TRY(launch_wgrad(h, s, "bwd_wgrad", gsplit, x_split, ws.zero, rows, N, K, sp, q.dw, ws.planes));
    if (!dx && !gelu_pre) return VETO_OK;
    HIP_TRY(launch_transpose_split(q.w, K, N, K, ws.wdg, N, s));     // W [N, K] -> W^T split rows [K, 2N]
    GemmArgs g{};
    g.a = gsplit; g.w = ws.wdg; g.c = dx;
    g.M = rows; g.N = K; g.K = N; g.ldc = K;
    ProfScope ps(h, s, "bwd_dgrad", 2.0 * rows * (double)N * K, 0);
    if (!gelu_pre) {
      HIP_TRY(launch_gemm_split(g, EPI_F32, 0, s));
      return VETO_OK;
    }
    if (gsplit == ws.dsplit_b || !next_partials) return fail(VETO_ERR_INVALID, "internal: the fused gelu' epilogue writes w.dsplit_b");
    g.c = nullptr; g.c_split = ws.dsplit_b; g.ldc = 2L * K; g.resid = gelu_pre; g.ldr = K; g.col_partial = ws.colp;
    *next_partials = (rows + 255) / 256 * 4;      // one partial row per 64-row slice of every 256-row tile
    HIP_TRY(launch_gemm_split(g, EPI_GELU_BWD, 0, s));
    return VETO_OK;
  }

  // the whole buffer, or under a plan the regions of the trainable tensors only, neighbours in one fill (tensors lie in index order,
  // padded to 64 floats); and the zero row of the weight-gradient GEMMs
  int zero_grads() {
    if (sch.full) HIP_TRY(hipMemsetAsync(grads, 0, veto_grad_floats(h) * 4, s));
    for (size_t i = 0; !sch.full && i < h->params.size();) {
      if (!sch.on[i]) { ++i; continue; }
      size_t j = i;
      while (j + 1 < h->params.size() && sch.on[j + 1]) ++j;
      HIP_TRY(hipMemsetAsync(grads + h->params[i].offset, 0, (h->params[j].offset + h->params[j].numel - h->params[i].offset) * 4, s));
      i = j + 1;
    }
    HIP_TRY(hipMemsetAsync(ws.zero, 0, 1024, s));
    return VETO_OK;
  }

  // classifier head: gradient of the compact CLS rows (not written when nothing under the head has a consumer)
  int head_backward(const float* dlogits) {
    HIP_TRY(launch_head_backward(dlogits, h->p("rel_out.weight"), ws.xout, sch.keep_from < L ? ws.dx : nullptr, G("rel_out.weight"),
                                 G("rel_out.bias"), ws.head_partial, n_pair, h->cfg.num_out, (long)kDim, s));
    return VETO_OK;
  }

  // A layer's stages in chain order: fc2, fc1, LayerNorm2, out, attention, qkv, LayerNorm1.  own[i]: stage i has a trainable tensor;
  // deeper[i]: something behind it (in this layer, a lower one or under layer 0) has a consumer, so its input gradient is computed.
  enum { S_FC2, S_FC1, S_LN2, S_OUT, S_ATTN, S_QKV, S_LN1, S_COUNT };
  struct LayerPass {
    int l;
    bool last;
    int R;      // rows behind the attention: the CLS rows only in the last layer (compact buffers)
    LinGrad qkv, out, fc1, fc2;
    bool ln1, ln2;
    bool deeper[S_COUNT];
    DropSite site;      // x_mid = x_in + dropout(attention(LN1(x_in) Wqkv^T) Wo^T + bo): the projection sees the masked gradient
  };

  // The walk ends behind the first stage with deeper[i] == false: every later stage of this and of every lower layer is without a
  // consumer too (so that layer is sch.keep_from, the last one backward_impl visits).
  int layer_backward(int l) {
    LayerPass p{l, l == L - 1, l == L - 1 ? n_pair : M, lin(l, LIN_QKV), lin(l, LIN_OUT), lin(l, LIN_FC1), lin(l, LIN_FC2)};
    p.ln1 = W(lname(l, "0.norm.weight")) || W(lname(l, "0.norm.bias"));
    p.ln2 = W(lname(l, "1.norm.weight")) || W(lname(l, "1.norm.bias"));
    p.site = attn_site(l);
    const bool own[S_COUNT] = {p.fc2.dw || p.fc2.db, p.fc1.dw || p.fc1.db, p.ln2, p.out.dw || p.out.db, false, p.qkv.dw != nullptr, p.ln1};
    for (int i = S_COUNT - 1, acc = sch.need(l); i >= 0; --i) {
      p.deeper[i] = acc;
      acc = acc || own[i];
    }
    const struct { int (TrainStep::*run)(const LayerPass&); int stage; } chain[] = {
        {&TrainStep::ffn_backward, S_FC1},        {&TrainStep::ln2_backward, S_LN2}, {&TrainStep::out_backward, S_OUT},
        {&TrainStep::attention_backward, S_ATTN}, {&TrainStep::qkv_backward, S_QKV}, {&TrainStep::ln1_backward, S_LN1}};
    for (const auto& c : chain) {
      ABI_TRY((this->*c.run)(p));
      if (!p.deeper[c.stage]) break;
    }
    return VETO_OK;
  }

  // x_out = x_mid + gelu(LN2(x_mid) W1^T + b1) W2^T + b2: fc2, then fc1 (not when fc2's input gradient has no consumer)
  // dpre = dh * gelu'(pre): in the epilogue of fc2's input-gradient GEMM (round 6; VETO_TRAIN_GELU_EPI=0: a pass of its own inside the
  // operand preparation of the fc1 backward, rounds 1-5)
  // (the gradient of this layer's output: compact CLS rows from the head in the last layer, else the rows the LayerNorm1 backward of the
  // layer above left -- with their split rows and bias partials when it emitted them)
  int ffn_backward(const LayerPass& p) {
    const LayerW& w = h->layers[p.l];
    const TrainLayer& t = ws.layers[p.l];
    const bool epi = train_gelu_epilogue(), d2 = p.deeper[S_FC2];
    const float* dy2 = dx_presplit ? nullptr : ws.dx;
    float* dx1 = p.deeper[S_FC1] ? ws.dtmp : nullptr;
    int partials = 0;
    if (recompute && p.fc2.dw) HIP_TRY(launch_gelu_split(t.pre, t.hid, (size_t)p.R, 2 * kDim, s));      // gelu(pre): fc2's operand, as the forward's epilogue wrote it
    if (epi) ABI_TRY(linear_backward(dy2, p.R, p.fc2, t.hid, nullptr, GradXform(), nullptr, dx_presplit, d2 ? t.pre : nullptr, &partials));
    else ABI_TRY(linear_backward(dy2, p.R, p.fc2, t.hid, d2 ? ws.dbig : nullptr, GradXform(), nullptr, dx_presplit));
    if (!d2) return VETO_OK;
    if (recompute && p.fc1.dw) HIP_TRY(launch_layernorm(t.xmid, kDim, w.ln2_w, w.ln2_b, t.a2, p.R, s));      // LayerNorm2 rows: fc1's operand
    if (epi) return linear_backward(nullptr, p.R, p.fc1, t.a2, dx1, GradXform(), ws.dsplit_b, partials);
    GradXform gelu;              // dpre = dh * gelu'(pre), folded into the operand preparation of the fc1 backward
    gelu.mode = XF_GELU;
    gelu.pre = t.pre;
    return linear_backward(ws.dbig, p.R, p.fc1, t.a2, dx1, gelu);
  }

  // (VETO_TRAIN_LN_SPLIT=1: it also emits the masked split rows and bias partials of the out projection's backward)
  int ln2_backward(const LayerPass& p) {
    const bool emit = train_ln_emits_split();
    HIP_TRY(launch_layernorm_backward(ws.layers[p.l].xmid, ws.dtmp, h->layers[p.l].ln2_w, ws.dx, ws.dmid, p.ln2 ? ws.dgb : nullptr, ws.ln_partial, p.R, s,
                                      emit ? ws.dsplit : nullptr, emit ? ws.colp : nullptr, emit ? p.site : DropSite(), ordered));
    HIP_TRY(copy_grad(lname(p.l, "1.norm.weight"), ws.dgb, kDim));
    HIP_TRY(copy_grad(lname(p.l, "1.norm.bias"), ws.dgb + kDim, kDim));
    return VETO_OK;
  }

  int out_backward(const LayerPass& p) {
    const bool presplit = train_ln_emits_split();
    return linear_backward(presplit ? nullptr : ws.dmid, p.R, p.out, ws.layers[p.l].ao, p.deeper[S_OUT] ? ws.dtmp : nullptr, drop_xform(p.site), nullptr,
                           presplit ? layernorm_backward_col_partials(p.R) : 0);
  }

  int attention_backward(const LayerPass& p) {
    HIP_TRY(launch_attention_backward(ws.layers[p.l].qkv, ws.dtmp, nullptr, ws.dsplit, n_pair, H, p.last ? 1 : 0, s, q24));
    return VETO_OK;
  }

  int qkv_backward(const LayerPass& p) {
    const LayerW& w = h->layers[p.l];
    const TrainLayer& t = ws.layers[p.l];
    if (recompute && p.qkv.dw) HIP_TRY(launch_layernorm(t.xin, kDim, w.ln1_w, w.ln1_b, t.a1, M, s));      // LayerNorm1 rows: the QKV projection's operand
    return linear_backward(nullptr, M, p.qkv, t.a1, p.deeper[S_QKV] ? ws.dtmp : nullptr);
  }

  // its result, ws.dx, is the gradient of the layer's input: of the output of the layer below
  int ln1_backward(const LayerPass& p) {
    const float* dres = ws.dmid;
    if (p.last) {
      // the residual gradient d x_mid lives on the CLS rows only: spread the compact rows over a zeroed token matrix
      HIP_TRY(hipMemsetAsync(ws.dx, 0, (size_t)M * kDim * 4, s));
      HIP_TRY(hipMemcpy2DAsync(ws.dx, (size_t)kTokens * kDim * 4, ws.dmid, (size_t)kDim * 4, (size_t)kDim * 4, (size_t)n_pair, hipMemcpyDeviceToDevice, s));
      dres = ws.dx;
    }
    // (in the last layer dres == ws.dx is also the output: every element is read and written by the same thread)
    const bool emit = train_ln_emits_split() && p.l > 0;      // (the split rows and bias partials of fc2 of the layer below)
    HIP_TRY(launch_layernorm_backward(ws.layers[p.l].xin, ws.dtmp, h->layers[p.l].ln1_w, dres, ws.dx, p.ln1 ? ws.dgb : nullptr, ws.ln_partial, M, s,
                                      emit ? ws.dsplit : nullptr, emit ? ws.colp : nullptr, DropSite(), ordered));
    dx_presplit = emit ? layernorm_backward_col_partials(M) : 0;
    HIP_TRY(copy_grad(lname(p.l, "0.norm.weight"), ws.dgb, kDim));
    HIP_TRY(copy_grad(lname(p.l, "0.norm.bias"), ws.dgb + kDim, kDim));
    return VETO_OK;
  }

  // What under layer 0 has a consumer
  struct Below { bool maps, patch_w, patch_b, pos_side, loc_w, cls_w, emb_w, lc_side; };
  Below below() const {
    Below b;
    b.maps = opts && (opts->d_roi_rgb || opts->d_roi_depth);
    b.patch_w = W(pe + "proj_d.weight") || W(pe + "proj_v.weight");
    b.patch_b = W(pe + "proj_d.bias") || W(pe + "proj_v.bias");
    b.pos_side = W("pos_embed.0.weight") || W("pos_embed.0.bias") || W("pos_embed.1.weight") || W("pos_embed.1.bias");
    b.loc_w = W("location_projection.0.weight"), b.cls_w = W("class_projection.0.weight"), b.emb_w = W("obj_embed.weight");
    b.lc_side = b.pos_side || b.loc_w || b.cls_w || b.emb_w || W("location_projection.0.bias") || W("class_projection.0.bias");
    return b;
  }

  // Token assembly: x0[p, t] = token + pos_embedding (ONE 576-vector broadcast over all tokens, model_veto.py:43,62): its gradient is
  // the sum over every token row; the cls_token's is the sum over row 0 of every pair; then (objects: anything under the tokens has a
  // consumer) the gradients of the per-object tables, dpatch and dlc
  int assemble_backward(bool objects) {
    const DropSite d = drop_site(opts, 2);   // pos_drop sits between (token + pos_embedding) and the first layer
    if (d.thresh) HIP_TRY(launch_dropout_apply(ws.dx, ws.dx, (size_t)M, kDim, d, s));
    if (float* g = G(T + "pos_embedding")) HIP_TRY(launch_column_sums(ws.dx, kDim, M, kDim, g, ws.col_partial, column_sums_chunks(), s));
    if (float* g = G(T + "cls_token")) HIP_TRY(launch_column_sums(ws.dx, (long)kTokens * kDim, n_pair, kDim, g, ws.col_partial, column_sums_chunks(), s));
    if (!objects) return VETO_OK;
    if (ordered) {
      HIP_TRY(launch_assemble_backward_ordered(ws.dx, ws.subj, ws.obj, ws.lc, in->img_obj_offset, in->img_pair_offset, in->n_img, ws.dpatch, ws.dlc, n_obj, s));
    } else {
      HIP_TRY(hipMemsetAsync(ws.dpatch, 0, (size_t)n_obj * 16 * 2 * kDim * 4, s));
      HIP_TRY(hipMemsetAsync(ws.dlc, 0, (size_t)n_obj * 2 * 2 * kDim * 4, s));
      HIP_TRY(launch_assemble_backward(ws.dx, ws.subj, ws.obj, ws.lc, ws.dpatch, ws.dlc, n_pair, s));
    }
    return VETO_OK;
  }

  // Patch projection: patch_tab = PA . Wcat^T + bias_cat (bias only on the subject half)
  int patch_backward(const Below& b) {
    const int R = n_obj * 16, patch = h->cfg.patch, TR = patch_t_rows(patch);
    if (b.patch_w || b.maps) HIP_TRY(launch_split_rows(ws.dpatch, ws.dsplit, (size_t)R, 2 * kDim, s));
    // dWcat^T [patch_feats(p), 1152] = PA^T . dpatch: "dy" = PA (split rows), "x" = dpatch in the roles of linear_backward swapped,
    // so that the output width (1152) is a multiple of 192
    if (b.patch_w) {
      HIP_TRY(launch_wgrad(h, s, nullptr, ws.pa, ws.dsplit, ws.zero, R, patch_feats(patch), 2 * kDim, patch_wgrad_split(patch, R), ws.dwcat_t, ws.planes));
      HIP_TRY(launch_patch_weight_grad(ws.dwcat_t, G(pe + "proj_d.weight"), G(pe + "proj_v.weight"), patch, s));
    }
    // biases: column sums of the subject half of dpatch: columns 0..511 -> proj_d.bias, 512..575 -> proj_v.bias
    if (b.patch_b) {
      HIP_TRY(launch_column_sums(ws.dpatch, 2 * kDim, R, kDim, ws.dgb, ws.col_partial, column_sums_chunks(), s));
      HIP_TRY(copy_grad(pe + "proj_d.bias", ws.dgb, 512));
      HIP_TRY(copy_grad(pe + "proj_v.bias", ws.dgb + 512, 64));
    }
    // input gradient (optional): dPA = dpatch . Wcat, i.e. the forward GEMM kernel on split(dpatch) (still in ws.dsplit) and
    // Wcat^T as the weight operand; then the inverse of patchify onto the ROI maps.  The reference's depth backbone is
    // trained through roi_depth_features (tools/relation_train_net.py:166-170).
    if (b.maps) {
      HIP_TRY(launch_build_patch_weight_t(h->p(pe + "proj_d.weight"), h->p(pe + "proj_v.weight"), ws.wcat_t, patch, s));
      GemmArgs g{};
      g.a = ws.dsplit; g.w = ws.wcat_t; g.c = ws.dpa;
      g.M = R; g.N = TR; g.K = 2 * kDim; g.ldc = TR;
      HIP_TRY(launch_gemm_split(g, EPI_F32, 0, s));
      HIP_TRY(launch_unpatchify(ws.dpa, TR, opts->d_roi_depth, opts->d_roi_rgb, n_obj, patch, s));
    }
    return VETO_OK;
  }

  static constexpr long kLdLc = 2 * 2 * kDim;   // dlc row n = [location 1152 | class 1152]

  // the biases of the location / class projections: they sit on the subject half
  int lc_bias_backward() {
    if (float* g = G("location_projection.0.bias")) HIP_TRY(launch_column_sums(ws.dlc, kLdLc, n_obj, kDim, g, ws.col_partial, column_sums_chunks(), s));
    if (float* g = G("class_projection.0.bias")) HIP_TRY(launch_column_sums(ws.dlc + 2 * kDim, kLdLc, n_obj, kDim, g, ws.col_partial, column_sums_chunks(), s));
    return VETO_OK;
  }

  // Position branch: pos_embed.0 (BatchNorm), pos_embed.1 and the location projection's weight
  int position_backward(const Below& b) {
    const DropSite site = drop_site(opts, 1);   // Dropout(0.1) behind the ReLU of pos_embed
    if (b.pos_side || b.loc_w) {      // (the location projection's weight gradient reads bn_out, which obj_pos_backward recomputes)
      // recompute pos (post-ReLU) through the masked gradient path
      //   dpos = dlc_loc . loc_wt^T ; obj_pos_backward -> dpre (ReLU'), BatchNorm affine gradients
      HIP_TRY(launch_sgemm_nt(ws.dlc, kLdLc, h->loc_wt, 2 * kDim, ws.dpos, kPosDim, n_obj, kPosDim, 2 * kDim, s));
      if (site.thresh) HIP_TRY(launch_dropout_apply(ws.dpos, ws.dpos, (size_t)n_obj, kPosDim, site, s));
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
    if (!b.loc_w) return VETO_OK;
    // location_projection weight: d loc_wt[k, j] = sum_n pos[n, k] dlc_loc[n, j] with the forward's pos, recomputed from bn_out:
    // pos[n, k] = dropout(relu(pos_b[k] + sum_c pos_w[k, c] bn_out[n, c])): one small product + ReLU, with dpos as its storage
    HIP_TRY(launch_sgemm_nt(ws.bn_out, 4, h->p("pos_embed.1.weight"), 4, ws.dpos, kPosDim, n_obj, kPosDim, 4, s));
    HIP_TRY(launch_bias_relu(ws.dpos, h->p("pos_embed.1.bias"), n_obj, kPosDim, s));
    if (site.thresh) HIP_TRY(launch_dropout_apply(ws.dpos, ws.dpos, (size_t)n_obj, kPosDim, site, s));
    HIP_TRY(launch_sgemm_tn(ws.dpos, kPosDim, ws.dlc, kLdLc, ws.dloc_wt, 2 * kDim, n_obj, kPosDim, 2 * kDim, s));
    HIP_TRY(launch_untranspose_pair_proj(ws.dloc_wt, G("location_projection.0.weight"), kPosDim, s));
    return VETO_OK;
  }

  // Class branch: emb = E[label] (hard labels) or softmax(logits) . E (sgcls, :4092-4095);
  // d cls_wt[k, j] = sum_n emb[n, k] dlc_cls[n, j]; demb = dlc_cls . cls_wt^T
  int class_backward(const Below& b) {
    const int C_obj = h->cfg.num_obj_cls, E = h->cfg.embed_dim;
    if (in->obj_logits && (b.cls_w || b.emb_w)) HIP_TRY(launch_softmax_rows(in->obj_logits, ws.prob, n_obj, C_obj, s));
    if (b.cls_w) {
      if (in->obj_logits) HIP_TRY(launch_sgemm_nn(ws.prob, C_obj, h->p("obj_embed.weight"), E, ws.emb, E, n_obj, E, C_obj, s));
      else HIP_TRY(launch_gather_rows(h->p("obj_embed.weight"), in->obj_labels, E, ws.emb, n_obj, s));
      HIP_TRY(launch_sgemm_tn(ws.emb, E, ws.dlc + 2 * kDim, kLdLc, ws.dcls_wt, 2 * kDim, n_obj, E, 2 * kDim, s));
      HIP_TRY(launch_untranspose_pair_proj(ws.dcls_wt, G("class_projection.0.weight"), E, s));
    }
    if (float* g = G("obj_embed.weight")) {
      HIP_TRY(launch_sgemm_nt(ws.dlc + 2 * kDim, kLdLc, h->cls_wt, 2 * kDim, ws.demb, E, n_obj, E, 2 * kDim, s));
      if (in->obj_logits) HIP_TRY(launch_sgemm_tn(ws.prob, C_obj, ws.demb, E, g, E, n_obj, C_obj, E, s));
      else if (ordered) HIP_TRY(launch_scatter_rows_ordered(ws.demb, in->obj_labels, E, g, n_obj, C_obj, s));
      else HIP_TRY(launch_scatter_rows(ws.demb, in->obj_labels, E, g, n_obj, s));
    }
    return VETO_OK;
  }
};

}  // namespace

// ---- the weight-gradient GEMM (abi_internal.h) -----------------------------------------------------------------------------
WgradSplit wgrad_split(int n, int k, int m, int k_splits, int min_ksteps, int cap) {
  int ks = k_splits;
  if (ks <= 0) {
    const int out_tiles = ((n + 255) / 256) * (k / 192);
    const int max_ks = (m + 32 * min_ksteps - 1) / (32 * min_ksteps);     // at least min_ksteps k-steps per tile
    ks = std::max(1, std::min(2 * 256 / out_tiles, max_ks));              // just under 2 full rounds of the 256 persistent workgroups
  }
  if (cap > 0 && ks > cap) ks = cap;
  const size_t step = 32 * (size_t)ks;
  return WgradSplit{ks, ((size_t)m + step - 1) / step * step, (size_t)ks * n * k};
}

hipError_t launch_wgrad(veto_handle_t h, hipStream_t s, const char* scope, const __bf16* a, const __bf16* b, const __bf16* zero, int m, int n,
                        int k, const WgradSplit& sp, float* dw, float* planes) {
  hipError_t e = planes ? hipSuccess : hipMemsetAsync(dw, 0, (size_t)n * k * 4, s);
  if (e != hipSuccess) return e;
  GemmArgs g{};
  g.a = a; g.w = b; g.c = planes ? planes : dw;
  g.M = n; g.N = k; g.K = (int)sp.mp; g.ldc = k; g.k_splits = sp.ks;
  if (zero) { g.tn = 1; g.lda = 2 * (long)n; g.ldw = 2 * (long)k; g.k_valid = m; g.zero = zero; }
  ProfScope ps(scope ? h : nullptr, s, scope, 2.0 * m * (double)n * k, 0);
  e = launch_gemm_split(g, planes ? EPI_PLANES : EPI_ATOMIC, 0, s);
  if (e == hipSuccess && planes) e = launch_fold_rows(planes, (long)n * k, sp.ks, (long)n * k, dw, s);      // the planes in split order
  return e;
}

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
  HIP_TRY(hipSetDevice(h->cfg.device));
  // (the frozen region's forward refreshes the operands itself: the training side's and the inference side's of its own layers)
  if (h->dirty && !sch.fused) ABI_TRY(finalize_weights(h, (hipStream_t)stream, true));
  h->train_gen.erase(workspace);     // (stamped at the end: a failed forward leaves no workspace that veto_backward would accept)
  h->train_plan.erase(workspace);
  TrainStep st(h, stream, in, opts, sch, workspace);
  if (sch.fused) {
    ABI_TRY(st.frozen_region(out_logits));
  } else {
    ABI_TRY(st.object_side());
    ABI_TRY(st.patch_projection());
    ABI_TRY(st.assemble_tokens());
  }
  if (!sch.fused || sch.keep_from < st.L) {
    for (int l = sch.fused ? sch.keep_from : 0; l < st.L - 1; ++l) ABI_TRY(st.layer(l));
    ABI_TRY(st.last_layer());
    ABI_TRY(st.head(out_logits));
  }
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
  HIP_TRY(hipSetDevice(h->cfg.device));
  // the backward reads the derived operands the matching forward used: a weight upload in between would pair this
  // workspace's activations with different weights
  if (h->dirty) return fail(VETO_ERR_WEIGHTS, "weights were reloaded between veto_forward_train and veto_backward");
  {
    auto it = h->train_gen.find(workspace);
    if (it == h->train_gen.end()) return fail(VETO_ERR_INVALID, "veto_backward: this workspace holds no veto_forward_train activations");
    if (it->second != h->weight_gen)
      return fail(VETO_ERR_WEIGHTS, "veto_backward: the weights were refreshed (by a later forward) since this workspace's veto_forward_train");
    auto pl = h->train_plan.find(workspace);      // (before any launch)
    if (sch.full ? pl != h->train_plan.end() : pl == h->train_plan.end() || pl->second != sch.key)
      return fail(VETO_ERR_INVALID, "veto_backward: this workspace's forward ran under another plan (veto_train_plan_t) than this backward");
  }
  TrainStep st(h, stream, in, opts, sch, workspace, grads);
  ABI_TRY(st.zero_grads());
  ABI_TRY(st.head_backward(dlogits));
  for (int l = st.L - 1; l >= sch.keep_from; --l) ABI_TRY(st.layer_backward(l));      // last to first
  if (!sch.below) return VETO_OK;      // (the walk above ended inside a layer, or behind layer keep_from)
  const TrainStep::Below b = st.below();
  const bool objects = b.patch_w || b.patch_b || b.maps || b.lc_side;
  ABI_TRY(st.assemble_backward(objects));      // pos_embedding, cls_token; objects: the per-object tables' dpatch / dlc
  if (!objects) return VETO_OK;
  ABI_TRY(st.patch_backward(b));      // (the split rows of dpatch in ws.dsplit feed both its weight and its map gradients)
  if (!b.lc_side) return VETO_OK;
  ABI_TRY(st.lc_bias_backward());
  ABI_TRY(st.position_backward(b));
  return st.class_backward(b);
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

// workspace: log_sum | nll_w | w_row | inv_wsum
static size_t carve_ce_loss(Carver c, size_t n, CeLossArgs* a) {
  a->log_sum = c.take<float>(n * 4);
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

int veto_meet_sample_parallel_limits(int32_t* tile, int32_t* window, int32_t* chunk) {
  if (tile) *tile = meet_parallel_tile();
  if (window) *window = meet_parallel_window();
  if (chunk) *chunk = meet_parallel_chunk();
  return VETO_OK;
}

static_assert((int)MEET_RAND_INSERT == VETO_MEET_RAND_INSERT && (int)MEET_RAND_CHOOSE == VETO_MEET_RAND_CHOOSE &&
              (int)MEET_ALL_INCLUDE == VETO_MEET_ALL_INCLUDE, "veto_meet_pad_mode is passed to the kernels as it is");

// workspace: fg_mask | acc_mask | pos | span | tile_count
static size_t carve_meet_parallel(Carver c, size_t n, size_t n_words, MeetParallelArgs* p) {
  p->fg_mask = c.take<unsigned long long>((n + 63) / 64 * 8);
  p->acc_mask = c.take<unsigned long long>((n_words + 63) / 64 * 8);
  p->pos = c.take<int32_t>(n * 4);
  p->span = c.take<uint16_t>(n * 2);
  p->tile_count = c.take<int32_t>((size_t)meet_parallel_tiles((long long)n) * 64 * 4);
  return c.off;
}

size_t veto_meet_sample_parallel_workspace_bytes(int32_t n, int32_t n_words) {
  if (n <= 0 || n_words < 0) return 0;
  MeetParallelArgs p{};
  return carve_meet_parallel(Carver{nullptr}, (size_t)n, (size_t)n_words, &p);
}

int veto_meet_sample_parallel(void* stream, const veto_meet_sample_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_meet_sample_args_t, a);
  if (a->mode != VETO_MEET_RAND_INSERT && a->mode != VETO_MEET_RAND_CHOOSE && a->mode != VETO_MEET_ALL_INCLUDE)
    return fail(VETO_ERR_INVALID, "mode %d is none of rand_insert (0), rand_choose (1), all_include (2)", a->mode);
  if (a->n <= 0 || a->n_words < 0 || a->n_groups < 1 || a->n_groups > 64 || a->n_cls < 2)
    return fail(VETO_ERR_INVALID, "bad sizes (n %d, n_words %d, n_groups %d, n_cls %d)", a->n, a->n_words, a->n_groups, a->n_cls);
  if (!a->labels || (a->n_words > 0 && !a->words) || !a->incre_idx_list || !a->pos_in_group || !a->group_size || !a->sample_rates ||
      !a->chosen || !a->group_labels || !a->counts || !a->words_used)
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_meet_sample_parallel_workspace_bytes(a->n, a->n_words), true));
  MeetParallelArgs p{};
  p.s.labels = a->labels; p.s.n = a->n; p.s.n_groups = a->n_groups; p.s.n_cls = a->n_cls; p.s.n_words = a->n_words; p.s.words = a->words;
  p.s.incre = a->incre_idx_list; p.s.pos_in_group = a->pos_in_group; p.s.group_size = a->group_size; p.s.rates = a->sample_rates;
  p.s.chosen = a->chosen; p.s.group_labels = a->group_labels; p.s.counts = a->counts; p.s.words_used = a->words_used;
  p.mode = a->mode;
  carve_meet_parallel(Carver{(char*)workspace}, (size_t)a->n, (size_t)a->n_words, &p);
  HIP_TRY(launch_meet_sample_parallel(p, (hipStream_t)stream));
  return VETO_OK;
}

}  // extern "C"
