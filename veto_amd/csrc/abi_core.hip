// Core of the C ABI (include/veto_amd.h): the environment knobs, the handle and its weight store (create / destroy, upload, the derived
// operands finalize_weights builds), the GEMM launch helper, the profiler and the last-error call.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "abi_internal.h"

thread_local std::string g_abi_err;

namespace veto {
bool env_knob_is(const char* name, const char* value) {
  const char* v = getenv(name);
  return v && !strcmp(v, value);
}
int device_cu_count() {
  static std::atomic<int> cache[64];      // per device ordinal; 0 = not queried yet (a benign race: every thread stores the same value)
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -1;
  if (dev < 64 && (cus = cache[dev].load(std::memory_order_relaxed)) > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return -1;
  if (dev < 64) cache[dev].store(cus, std::memory_order_relaxed);
  return cus;
}
int env_knob_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
}  // namespace veto

// Padded head width of the block form of the folded last layer, or 0 when the products are used instead: the head width rounded up
// to 32 k's must divide a 192-column GEMM tile (heads 12 / 8 / 6 / 3 of the 576 columns), and the form can be switched off
// (VETO_FOLD_BLOCKS=0, A/B knob).
static int fold_block_width(int heads) {
  static const bool off = env_knob_is("VETO_FOLD_BLOCKS", "0");
  if (off || heads <= 0 || kDim % heads != 0) return 0;
  const int dhp = (kDim / heads + 31) / 32 * 32;
  return 192 % dhp == 0 && (heads * dhp) % 192 == 0 ? dhp : 0;
}

// THE dependency table of the per-tensor refresh (include/veto_amd.h, veto_load_weights): the derived operands that read the
// state-dict tensor `name`.  A tensor that is read in place (biases, obj_embed, pos_embed.*, LayerNorm2 gains, ...) has none.
static std::vector<int> operands_of(veto_handle_t h, const std::string& name) {
  const int L = h->cfg.layers;
  const std::string T = kT;
  std::vector<int> ops;
  for (int l = 0; l < L; ++l)
    for (int i = 0; i < 4; ++i)
      if (name == lname(l, kLayerLinears[i].weight)) ops.push_back(OP_LINEAR0 + 4 * l + i);
  for (const std::string& q : {lname(0, "0.norm.weight"), lname(0, "0.norm.bias"), lname(0, "0.fn.to_qkv.weight"), T + "pos_embedding", T + "cls_token"})
    if (name == q) ops.push_back(OP_QKV0);
  for (const std::string& q : {lname(L - 1, "0.fn.to_qkv.weight"), lname(L - 1, "0.fn.to_out.0.weight")})
    if (name == q) ops.push_back(OP_FOLD);
  if (name.compare(0, T.size() + 12, T + "patch_embed.") == 0) ops.push_back(OP_PATCH);
  if (name == "location_projection.0.weight") ops.push_back(OP_LOC_T);
  if (name == "class_projection.0.weight") ops.push_back(OP_CLS_T);
  if (name == "rel_out.weight") ops.push_back(OP_HEAD_T);
  return ops;
}

// the builds operand `op` has: the four re-layouts are the training path's too, the layer-0 constants and the fold the inference forward's alone
static uint8_t builds_of(int op) {
  return op >= OP_LINEAR0 ? STALE_TRAIN | STALE_INFER : op == OP_QKV0 || op == OP_FOLD ? STALE_INFER : STALE_TRAIN;
}

int finalize_weights(veto_handle_t h, hipStream_t s, bool train_only, int infer_layers) {
  for (const Param& q : h->params)
    if (!q.loaded) return fail(VETO_ERR_WEIGHTS, "weight '%s' was never loaded", q.name.c_str());
  const int L = h->cfg.layers;
  const bool uploaded = h->dirty;      // (false: only inference-side operands are missing)
  const bool mixed = h->cfg.precision != VETO_PRECISE;      // (VETO_FAST runs VETO_MIXED's launches, with the correction stages of the fused ones skipped)
  const int infer_upto = infer_layers < 0 ? L : infer_layers;
  for (int32_t& n : h->built) n = 0;
  // does build `bit` of operand `op` run now?  It is then current.
  auto take = [&](int op, int bit) {
    if (!(h->stale[op] & bit)) return false;
    h->stale[op] &= ~bit;
    return true;
  };
  for (int l = 0; l < L; ++l) {
    LayerW& w = h->layers[l];
    for (int i = 0; i < 4; ++i) {
      const LayerLinear& q = kLayerLinears[i];
      if (take(OP_LINEAR0 + 4 * l + i, STALE_TRAIN)) {
        HIP_TRY(launch_split_rows(h->p(lname(l, q.weight)), w.split(i), q.N, q.K, s));
        ++h->built[VETO_BUILD_SPLIT_ROWS];
      }
      if (!mixed) h->stale[OP_LINEAR0 + 4 * l + i] &= ~STALE_INFER;      // (a VETO_PRECISE handle has no mixed rows)
      else if (!train_only && l < infer_upto && take(OP_LINEAR0 + 4 * l + i, STALE_INFER)) {
        HIP_TRY(launch_mixed_weight_rows(h->p(lname(l, q.weight)), w.mixed_rows(i), q.N, q.K, w.exp_m + i, s));
        ++h->built[VETO_BUILD_MIXED_ROWS];
      }
    }
  }
  const std::string pe = std::string(kT) + "patch_embed.";
  if (take(OP_PATCH, STALE_TRAIN)) {
    HIP_TRY(launch_build_patch_weight(h->p(pe + "proj_d.weight"), h->p(pe + "proj_d.bias"), h->p(pe + "proj_v.weight"),
                                      h->p(pe + "proj_v.bias"), h->patch_w, h->patch_bias, h->cfg.patch, s));
    ++h->built[VETO_BUILD_PATCH];
  }
  if (take(OP_LOC_T, STALE_TRAIN)) {
    HIP_TRY(launch_transpose_pair_proj(h->p("location_projection.0.weight"), h->loc_wt, kPosDim, s));
    ++h->built[VETO_BUILD_LOC_T];
  }
  if (take(OP_CLS_T, STALE_TRAIN)) {
    HIP_TRY(launch_transpose_pair_proj(h->p("class_projection.0.weight"), h->cls_wt, h->cfg.embed_dim, s));
    ++h->built[VETO_BUILD_CLS_T];
  }
  if (take(OP_HEAD_T, STALE_TRAIN)) {
    HIP_TRY(launch_transpose_head(h->p("rel_out.weight"), h->head_wt, h->cfg.num_out, s));
    ++h->built[VETO_BUILD_HEAD_T];
  }
  if (!train_only && infer_upto >= 1 && take(OP_QKV0, STALE_INFER)) {
    // layer 0: Wqkv diag(gamma) and the weight-only vectors of the per-object form (fold_tmp holds >= 1728 x 576 floats)
    const std::string T0 = kT;
    HIP_TRY(launch_qkv0_consts(h->p(lname(0, "0.fn.to_qkv.weight")), h->layers[0].ln1_w, h->layers[0].ln1_b, h->p(T0 + "pos_embedding"),
                               h->p(T0 + "cls_token"), h->fold_tmp, h->q0_vec, s));
    HIP_TRY(launch_split_rows(h->fold_tmp, h->q0_w, 3 * kDim, kDim, s));
    ++h->built[VETO_BUILD_QKV0];
  }
  if (h->cfg.heads > cls_fold_max_heads()) h->stale[OP_FOLD] = 0;      // (no folded last layer at this head count)
  else if (!train_only && infer_upto >= L && take(OP_FOLD, STALE_INFER)) {
    // last layer: M_h = W_q,h^T W_k,h and N_h = W_o,h W_v,h (products over the head width, fp32), as GEMM weight operands
    const int H = h->cfg.heads, dh = kDim / H;
    const float* qkv = h->p(lname(L - 1, "0.fn.to_qkv.weight"));      // [1728, 576]: q rows, k rows, v rows
    const float* wo = h->p(lname(L - 1, "0.fn.to_out.0.weight"));     // [576, 576]
    if (h->fold_dhp > 0) {   // block form: the four factors themselves, padded / block-diagonal, as split rows
      const int np = H * h->fold_dhp;
      HIP_TRY(launch_fold_blocks(qkv, wo, h->fold_tmp, 0, H, h->fold_dhp, s));
      HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_q, (size_t)np, kDim, s));
      HIP_TRY(launch_fold_blocks(qkv, wo, h->fold_tmp, 1, H, h->fold_dhp, s));
      HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_k, (size_t)H * kDim, np, s));
      HIP_TRY(launch_fold_blocks(qkv, wo, h->fold_tmp, 2, H, h->fold_dhp, s));
      HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_v, (size_t)np, H * kDim, s));
      HIP_TRY(launch_fold_blocks(qkv, wo, h->fold_tmp, 3, H, h->fold_dhp, s));
      HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_o, (size_t)kDim, np, s));
    } else {
    for (int hd = 0; hd < H; ++hd)   // Mcat row (hd, c), column c' = sum_d Wk[hd*dh + d, c] Wq[hd*dh + d, c']
      HIP_TRY(launch_sgemm_tn(qkv + ((size_t)kDim + hd * dh) * kDim, kDim, qkv + (size_t)hd * dh * kDim, kDim,
                              h->fold_tmp + (size_t)hd * kDim * kDim, kDim, dh, kDim, kDim, s));
    HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_m, (size_t)H * kDim, kDim, s));
    for (int hd = 0; hd < H; ++hd)   // Ncat row r, column (hd, c) = sum_d Wo[r, hd*dh + d] Wv[hd*dh + d, c]
      HIP_TRY(launch_sgemm_nn(wo + hd * dh, kDim, qkv + ((size_t)2 * kDim + hd * dh) * kDim, kDim, h->fold_tmp + (size_t)hd * kDim,
                              (long)H * kDim, kDim, kDim, dh, s));
    HIP_TRY(launch_split_rows(h->fold_tmp, h->fold_n, (size_t)kDim, H * kDim, s));
    }
    ++h->built[VETO_BUILD_FOLD];
  }
  // an upload changes what a training workspace was computed with (a tensor read in place included); completing the inference side of
  // an earlier upload does not
  if (uploaded) ++h->weight_gen;
  h->dirty = false;
  h->infer_dirty = false;
  for (uint8_t f : h->stale) h->infer_dirty = h->infer_dirty || (f & STALE_INFER);
  return VETO_OK;
}

int run_gemm(veto_handle_t h, hipStream_t s, const char* name, const __bf16* a, SplitW w, const float* bias,
             const float* resid, long ldr, float* c, __bf16* c_split, long ldc, int M, int N, int K, int epi,
             long lda, int w_row0, DropSite drop, const int* w_exp, int kb_tiles, int kb_steps) {
  GemmArgs g{};
  g.kb_tiles = kb_tiles; g.kb_steps = kb_steps;   // block-diagonal weights (kernels.h): flops / bytes below count the blocks only
  if (w_exp) { g.fmt = FMT_MIXED; g.w_exp = w_exp; }   // a, w (and an EPI_GELU_SPLIT output) are mixed rows
  if (drop.thresh) {
    if (epi != EPI_RESID) return fail(VETO_ERR_INVALID, "dropout is fused into the residual epilogue only");
    epi = EPI_RESID_DROP;
    g.drop_seed = drop.seed; g.drop_thresh = drop.thresh; g.drop_scale = drop.scale; g.drop_row_step = drop.row_step;
  }
  g.a = a; g.lda = lda;
  g.w = w + (size_t)w_row0 * 2 * K;
  g.bias = bias; g.resid = resid; g.c = c; g.c_split = c_split;
  g.M = M; g.N = N; g.K = K; g.ldr = ldr; g.ldc = ldc;
  if (epi == EPI_PRE_GELU) g.ldc_f32 = N;      // (c = the fp32 pre-activation rows, contiguous; ldc is the split rows')
  const double kk = kb_tiles > 0 ? 32.0 * kb_steps : (double)K;
  const double flops = 2.0 * M * (double)N * kk;
  const double bytes = 4.0 * ((double)M * K + (double)N * kk) + (double)M * N * (epi == EPI_RESID ? 8.0 : epi == EPI_F24 ? 3.0 : 4.0);
  ProfScope ps(h, s, name, flops, bytes);
  HIP_TRY(launch_gemm_split(g, epi, 0, s));      // (the per-object and CLS-row GEMMs of a VETO_FAST handle are VETO_MIXED's)
  return VETO_OK;
}

// The derived operands of the handle (split planes, mixed rows, transposes, folded tables) in one allocation: points them into `base`,
// or with base == nullptr only sizes it; h->layers has its L entries
static size_t carve_derived(veto_handle_t h, char* base) {
  Carver c{base};
  const veto_config_t& cfg = h->cfg;
  const int L = cfg.layers, E = cfg.embed_dim;
  const bool mixed = cfg.precision != VETO_PRECISE;
  for (LayerW& w : h->layers) {
    w.qkv = c.take<__bf16>((size_t)3 * kDim * kDim * 4);
    w.out = c.take<__bf16>((size_t)kDim * kDim * 4);
    w.fc1 = c.take<__bf16>((size_t)2 * kDim * kDim * 4);
    w.fc2 = c.take<__bf16>((size_t)2 * kDim * kDim * 4);
    if (!mixed) continue;
    w.qkv_m = c.take<__bf16>((size_t)3 * kDim * kDim * 4);
    w.out_m = c.take<__bf16>((size_t)kDim * kDim * 4);
    w.fc1_m = c.take<__bf16>((size_t)2 * kDim * kDim * 4);
    w.fc2_m = c.take<__bf16>((size_t)2 * kDim * kDim * 4);
  }
  int* exps = c.take<int>((size_t)L * 4 * sizeof(int));
  for (int l = 0; l < L && mixed && exps; ++l) h->layers[l].exp_m = exps + 4 * l;
  h->patch_w = c.take<__bf16>((size_t)2 * kDim * patch_feats(cfg.patch) * 4);
  h->patch_bias = c.take<float>((size_t)2 * kDim * 4);
  h->loc_wt = c.take<float>((size_t)kPosDim * 2 * kDim * 4);
  h->cls_wt = c.take<float>((size_t)E * 2 * kDim * 4);
  h->head_wt = c.take<float>((size_t)kDim * cfg.num_out * 4);
  const int fold_dhp = h->fold_dhp = fold_block_width(cfg.heads);
  const size_t fold_np = (size_t)cfg.heads * (fold_dhp > 0 ? fold_dhp : 0);
  const size_t fold_el = fold_dhp > 0 ? (size_t)cfg.heads * kDim * fold_np : (size_t)cfg.heads * kDim * kDim;   // largest staged matrix
  h->fold_m = c.take<__bf16>(fold_dhp > 0 ? 256 : fold_el * 4);
  h->fold_n = c.take<__bf16>(fold_dhp > 0 ? 256 : fold_el * 4);
  h->fold_tmp = c.take<float>(fold_el * 4);
  h->fold_q = c.take<__bf16>(fold_np * kDim * 4 + 256);
  h->fold_k = c.take<__bf16>((size_t)cfg.heads * kDim * fold_np * 4 + 256);
  h->fold_v = c.take<__bf16>((size_t)cfg.heads * kDim * fold_np * 4 + 256);
  h->fold_o = c.take<__bf16>(fold_np * kDim * 4 + 256);
  h->q0_w = c.take<__bf16>((size_t)3 * kDim * kDim * 4);
  h->q0_vec = c.take<float>((size_t)3 * 3 * kDim * 4);
  return c.off;
}

extern "C" {

const char* veto_last_error(void) { return g_abi_err.c_str(); }
const char* veto_version(void) { return "veto_amd 0.1 (gfx950)"; }

int veto_create(const veto_config_t* cfg, veto_handle_t* out) {
  CHECK_STRUCT_AND(veto_config_t, cfg, out != nullptr);
  if (cfg->dim != kDim) return fail(VETO_ERR_INVALID, "T_INPUT_DIM must be 576 (proj_d 512 + proj_v 64), got %d", cfg->dim);
  // (the fused launches hold 19 tokens per pair: CLS, location, class and a 4 x 4 grid of patches)
  if (cfg->patch < 1 || cfg->patch > 4 || cfg->resolution != 4 * cfg->patch || cfg->channels != 256)
    return fail(VETO_ERR_INVALID, "POOLER_RESOLUTION %d / PATCH_SIZE %d / %d channels: supported are (4, 1), (8, 2), (12, 3), (16, 4) with 256 "
                "channels -- the fused launches hold 19 tokens per pair, i.e. a 4 x 4 patch grid (resolution == 4 * patch)",
                cfg->resolution, cfg->patch, cfg->channels);
  if (cfg->layers < 1 || cfg->layers > 64) return fail(VETO_ERR_INVALID, "bad ENC_LAYERS %d", cfg->layers);
  if (cfg->heads < 1 || kDim % cfg->heads != 0 || (kDim / cfg->heads) % 4 != 0)
    return fail(VETO_ERR_INVALID, "NHEADS %d must divide 576 with head dim %% 4 == 0", cfg->heads);
  if (cfg->num_obj_cls < 2 || cfg->num_obj_cls > 256 || cfg->embed_dim < 1 || cfg->embed_dim > 256)
    return fail(VETO_ERR_INVALID, "num_obj_cls/embed_dim out of range");
  if (cfg->num_out < 1 || cfg->num_out > 4096) return fail(VETO_ERR_INVALID, "bad num_out %d", cfg->num_out);
  if (cfg->precision != VETO_PRECISE && cfg->precision != VETO_FAST && cfg->precision != VETO_MIXED) return fail(VETO_ERR_INVALID, "bad precision");
  HIP_TRY(hipSetDevice(cfg->device));

  veto_handle_t h = new veto_handle_s();
  h->cfg = *cfg;
  h->dh = kDim / cfg->heads;
  h->chunk = cfg->max_chunk_pairs > 0 ? cfg->max_chunk_pairs : 32768;
  const int E = cfg->embed_dim, L = cfg->layers;
  h->add("obj_embed.weight", (size_t)cfg->num_obj_cls * E);
  h->add("class_projection.0.weight", (size_t)kDim * 2 * E);
  h->add("class_projection.0.bias", kDim);
  h->add("pos_embed.0.weight", 4);
  h->add("pos_embed.0.bias", 4);
  h->add("pos_embed.0.running_mean", 4);
  h->add("pos_embed.0.running_var", 4);
  h->add("pos_embed.1.weight", (size_t)kPosDim * 4);
  h->add("pos_embed.1.bias", kPosDim);
  h->add("location_projection.0.weight", (size_t)kDim * 2 * kPosDim);
  h->add("location_projection.0.bias", kDim);
  h->add(std::string(kT) + "cls_token", kDim);
  h->add(std::string(kT) + "pos_embedding", kDim);
  const size_t KP = patch_feats(cfg->patch);      // 512 p^2: cat(subject, object) x p^2 x 256 channels
  h->add(std::string(kT) + "patch_embed.proj_d.weight", (size_t)512 * KP);
  h->add(std::string(kT) + "patch_embed.proj_d.bias", 512);
  h->add(std::string(kT) + "patch_embed.proj_v.weight", (size_t)64 * KP);
  h->add(std::string(kT) + "patch_embed.proj_v.bias", 64);
  for (int l = 0; l < L; ++l) {
    h->add(lname(l, "0.norm.weight"), kDim);
    h->add(lname(l, "0.norm.bias"), kDim);
    h->add(lname(l, "0.fn.to_qkv.weight"), (size_t)3 * kDim * kDim);
    h->add(lname(l, "0.fn.to_out.0.weight"), (size_t)kDim * kDim);
    h->add(lname(l, "0.fn.to_out.0.bias"), kDim);
    h->add(lname(l, "1.norm.weight"), kDim);
    h->add(lname(l, "1.norm.bias"), kDim);
    h->add(lname(l, "1.fn.net.0.weight"), (size_t)2 * kDim * kDim);
    h->add(lname(l, "1.fn.net.0.bias"), 2 * kDim);
    h->add(lname(l, "1.fn.net.3.weight"), (size_t)2 * kDim * kDim);
    h->add(lname(l, "1.fn.net.3.bias"), kDim);
  }
  h->add("rel_out.weight", (size_t)cfg->num_out * kDim);
  h->add("rel_out.bias", cfg->num_out);
  for (Param& q : h->params) {
    q.offset = h->raw_floats;
    h->raw_floats += align_up(q.numel, 64);
  }
  for (const Param& q : h->params) h->deps.push_back(operands_of(h, q.name));
  for (int op = 0; op < OP_LINEAR0 + 4 * L; ++op) h->stale.push_back(builds_of(op));      // (nothing is built yet)
  hipError_t e = hipMalloc((void**)&h->raw, h->raw_floats * sizeof(float));
  if (e != hipSuccess) { delete h; return fail(VETO_ERR_HIP, "hipMalloc(raw weights): %s", hipGetErrorString(e)); }

  // derived weights
  h->layers.resize(L);
  e = hipMalloc((void**)&h->derived, carve_derived(h, nullptr));
  if (e != hipSuccess) { (void)hipFree(h->raw); delete h; return fail(VETO_ERR_HIP, "hipMalloc(derived weights): %s", hipGetErrorString(e)); }
  carve_derived(h, h->derived);
  for (int l = 0; l < L; ++l) {
    LayerW& w = h->layers[l];
    w.ln1_w = h->p(lname(l, "0.norm.weight")); w.ln1_b = h->p(lname(l, "0.norm.bias"));
    w.ln2_w = h->p(lname(l, "1.norm.weight")); w.ln2_b = h->p(lname(l, "1.norm.bias"));
    w.out_b = h->p(lname(l, "0.fn.to_out.0.bias"));
    w.fc1_b = h->p(lname(l, "1.fn.net.0.bias"));
    w.fc2_b = h->p(lname(l, "1.fn.net.3.bias"));
  }
  if (cfg->precision == VETO_MIXED) {
    e = hipMalloc((void**)&h->sat_buf, (size_t)L * VETO_SAT_SITES * 4 * sizeof(unsigned long long));
    if (e != hipSuccess) { (void)hipFree(h->raw); (void)hipFree(h->derived); delete h; return fail(VETO_ERR_HIP, "hipMalloc(saturation counters): %s", hipGetErrorString(e)); }
  }
  *out = h;
  return VETO_OK;
}

int veto_destroy(veto_handle_t h) {
  if (!h) return VETO_OK;
  // teardown: nothing useful can be done with a failure here
  for (ProfRec& r : h->prof_recs) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
  for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
  (void)hipFree(h->raw);
  (void)hipFree(h->derived);
  if (h->sat_buf) (void)hipFree(h->sat_buf);
  delete h;
  return VETO_OK;
}

int veto_num_weights(veto_handle_t h) { return h ? (int)h->params.size() : fail(VETO_ERR_INVALID, "null handle"); }

int veto_weight_info(veto_handle_t h, int index, const char** name, size_t* numel) {
  if (!h || index < 0 || index >= (int)h->params.size()) return fail(VETO_ERR_INVALID, "bad weight index");
  if (name) *name = h->params[index].name.c_str();
  if (numel) *numel = h->params[index].numel;
  return VETO_OK;
}

int veto_load_weights(veto_handle_t h, const char* name, const float* src, size_t numel, void* stream) {
  if (!h || !name || !src) return fail(VETO_ERR_INVALID, "null argument");
  auto it = h->index.find(name);
  if (it == h->index.end()) return fail(VETO_ERR_INVALID, "unknown weight '%s'", name);
  Param& q = h->params[it->second];
  if (q.numel != numel) return fail(VETO_ERR_INVALID, "weight '%s': expected %zu elements, got %zu", name, q.numel, numel);
  HIP_TRY(hipMemcpyAsync(h->raw + q.offset, src, numel * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
  q.loaded = true;
  h->dirty = true;
  for (int op : h->deps[it->second]) h->stale[op] = builds_of(op);
  h->train_plan.clear();
  h->train_gen.clear();   // (no workspace's saved activations match the weights any more; also bounds the map)
  return VETO_OK;
}

int veto_debug_last_finalize(veto_handle_t h, int32_t* counts, int32_t capacity) {
  if (!h || !counts) return fail(VETO_ERR_INVALID, "null argument");
  if (capacity < VETO_BUILD_KINDS) return fail(VETO_ERR_INVALID, "counts holds %d entries, need VETO_BUILD_KINDS = %d", capacity, (int)VETO_BUILD_KINDS);
  for (int i = 0; i < VETO_BUILD_KINDS; ++i) counts[i] = h->built[i];
  return VETO_BUILD_KINDS;
}

size_t veto_grad_floats(veto_handle_t h) { return h ? h->raw_floats : 0; }

int veto_weight_offset(veto_handle_t h, int index, size_t* offset_floats) {
  if (!h || index < 0 || index >= (int)h->params.size() || !offset_floats) return fail(VETO_ERR_INVALID, "bad weight index");
  *offset_floats = h->params[index].offset;
  return VETO_OK;
}

int veto_profile_enable(veto_handle_t h, int32_t on) {
  if (!h) return fail(VETO_ERR_INVALID, "null handle");
  h->prof_on = on != 0;
  return VETO_OK;
}

int veto_profile_collect(veto_handle_t h) {
  if (!h) return fail(VETO_ERR_INVALID, "null handle");
  for (ProfRec& r : h->prof_recs) {
    HIP_TRY(hipEventSynchronize(r.stop));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.start, r.stop));
    auto& a = h->prof_agg[r.name_id];
    a.ms += ms;
    a.n += 1;
    a.flops = r.flops;
    a.bytes = r.bytes;
    h->event_pool.push_back(r.start);
    h->event_pool.push_back(r.stop);
  }
  h->prof_recs.clear();
  return (int)h->prof_names.size();
}

int veto_profile_entry(veto_handle_t h, int index, const char** name, double* total_ms, int64_t* launches,
                       double* flops_per_launch, double* bytes_per_launch) {
  if (!h || index < 0 || index >= (int)h->prof_names.size()) return fail(VETO_ERR_INVALID, "bad profile index");
  if (name) *name = h->prof_names[index].c_str();
  if (total_ms) *total_ms = h->prof_agg[index].ms;
  if (launches) *launches = h->prof_agg[index].n;
  if (flops_per_launch) *flops_per_launch = h->prof_agg[index].flops;
  if (bytes_per_launch) *bytes_per_launch = h->prof_agg[index].bytes;
  return VETO_OK;
}

int veto_profile_reset(veto_handle_t h) {
  if (!h) return fail(VETO_ERR_INVALID, "null handle");
  for (ProfRec& r : h->prof_recs) { h->event_pool.push_back(r.start); h->event_pool.push_back(r.stop); }
  h->prof_recs.clear();
  for (auto& a : h->prof_agg) a = veto_handle_s::Agg();
  return VETO_OK;
}

}  // extern "C"
