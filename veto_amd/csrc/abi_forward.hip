// The inference forward of the C ABI: workspace carving and the launch sequence of one eval forward of VETOPredictor / the MEET
// Ensemble trunk (roi_relation_predictors.py:4074-4139, :3752-3853; model_veto.py:15-26), as a plan of the path every stage takes
// plus one short function per stage.
#include "abi_internal.h"

namespace {

struct Workspace {
  int32_t *subj, *obj;
  float* lc;
  __bf16* pa;       // patch rows, split [prow, 2*patch_feats(p)]
  float* patch_tab;
  float* x;
  __bf16* a;        // LN(x) / attention output, split [mpad, 2*576]
  char* big;        // qkv fp32 [mpad,1728]; later the MLP hidden, split [mpad, 2*1152]
  float* xc;
  __bf16* ptab_split;   // layer 0, per-object form: patch_tab as split rows [prow, 2*1152]
  float *sw, *ow;       // ... its products with Wqkv diag(gamma), fp32 [prow, 1728] each
  float* stats;         // ... (mean, rstd) of the layer-0 token rows [mpad, 2]
  __bf16 *ac, *hc;  // CLS-compact operands, split [cpad, 2*576] / [cpad, 2*1152]
  size_t total;
};

// Carves (or, with base == nullptr, just sizes) the workspace.  fold_heads: the head count the folded last layer's region is sized
// for (veto_forward: the most the fold supports, whatever the handle's); cls_rows false: a forward that stops below the last layer
// (frozen_forward) has neither that region nor the compact CLS-row buffers.
Workspace carve(char* base, int n_obj, int n_pair, int chunk, int patch, int fold_heads = cls_fold_max_heads(), bool cls_rows = true) {
  Workspace w;
  Carver c{base};
  const size_t prow = (size_t)gemm_rows_padded(n_obj * 16);
  // (the fused QKV + attention launch reads whole tiles of 16 pairs: the activation rows are padded to those too)
  const size_t tile_rows = qkv_attn_rows_padded(chunk);
  const size_t mpad = (size_t)gemm_rows_padded((int)(tile_rows > (size_t)chunk * kTokens ? tile_rows : (size_t)chunk * kTokens));
  const size_t cpad = (size_t)gemm_rows_padded(chunk);
  w.subj = c.take<int32_t>((size_t)n_pair * 4);
  w.obj = c.take<int32_t>((size_t)n_pair * 4);
  w.lc = c.take<float>((size_t)n_obj * 2 * 2 * kDim * 4);
  w.pa = c.take<__bf16>(prow * 2 * patch_feats(patch) * 2);
  w.patch_tab = c.take<float>((size_t)n_obj * 16 * 2 * kDim * 4);
  w.x = c.take<float>(mpad * kDim * 4);
  w.a = c.take<__bf16>(mpad * 2 * kDim * 2);
  {   // qkv of a chunk; in the last layer instead u [cpad, H*576] fp32 + abar [cpad, 2*H*576] split (folded CLS attention)
    const size_t qkv_bytes = mpad * 3 * kDim * 4, fold_bytes = cls_rows ? 2 * (align_up(cpad * (size_t)fold_heads * kDim * 4, 256)) : 0;
    w.big = c.take(qkv_bytes > fold_bytes ? qkv_bytes : fold_bytes);
  }
  w.xc = c.take<float>(cls_rows ? cpad * kDim * 4 : 0);
  w.ptab_split = c.take<__bf16>(prow * 2 * 2 * kDim * 2);
  w.sw = c.take<float>(prow * 3 * kDim * 4);
  w.ow = c.take<float>(prow * 3 * kDim * 4);
  w.stats = c.take<float>(mpad * 2 * 4);
  w.ac = c.take<__bf16>(cls_rows ? cpad * 2 * kDim * 2 : 0);
  w.hc = c.take<__bf16>(cls_rows ? cpad * 4 * kDim * 2 : 0);
  w.total = c.off;
  return w;
}

// the head count a frozen region's workspace holds the folded last layer for: the handle's own (0: it has no folded form)
int frozen_fold_heads(veto_handle_t h) { return h->cfg.heads <= cls_fold_max_heads() ? h->cfg.heads : 0; }

// Which form every stage of the forward takes: resolved once per call from the handle and from whether the saturation audit runs.
struct ForwardPlan {
  int L, H, dhp;      // layers, heads, padded head width of the folded last layer's block form (0: the products)
  bool qkv0_tables, fold_last, mixed, fast, mixed_out, cls_mixed, tail_fused, panel, qkv_f24, qa_fused, x_f24;
  // ... and the LayerNorm in front of the next layer's QKV GEMM in the FeedForward epilogue, when that GEMM takes mixed rows
  bool ffn_ln_next(int l) const { return mixed && panel && l + 1 < L - 1; }
};

ForwardPlan make_plan(veto_handle_t h, bool sat) {
  ForwardPlan p;
  const int L = p.L = h->cfg.layers, H = p.H = h->cfg.heads;
  p.dhp = h->fold_dhp;
  // Layer 0 in the per-object form: LayerNorm + QKV of the 16 patch tokens of every pair come from two
  // per-object tables SW = S W'^T, OW = O W'^T (S | O = the halves of patch_tab, W' = Wqkv diag(gamma)) -- a GEMM over the
  // n_obj*16 object rows instead of the n_pair*19 token rows.  Needs a layer behind it that reads LN1 rows as usual (L >= 2).
  static const bool tables_off = env_knob_is("VETO_QKV0_TABLES", "0");   // A/B knob of the parity tests
  p.qkv0_tables = L >= 2 && !tables_off;
  static const bool fold_off = env_knob_is("VETO_CLS_FOLD", "0");         // A/B knob of the parity tests
  p.fold_last = !fold_off && H <= cls_fold_max_heads();   // last layer in the folded CLS form (attention.hip)
  // VETO_MIXED: the four token-row Linears of every layer but the last, and layer 0's QKV launches of the location / class token
  // rows, take fp16 + e4m3 operands (common.h); the other per-object and
  // CLS-row GEMMs (8 % of the GEMM work) stay on split-bf16 operands.  The out projection only behind the MFMA attention kernel.
  // VETO_FAST = VETO_MIXED's launches with the correction stages of the two fused token-row launches skipped (fp16 main product only:
  // what the schedule costs with the precision terms free; logit error ~2e-3, reported, never parity-grade)
  p.mixed = h->cfg.precision != VETO_PRECISE;
  p.fast = h->cfg.precision == VETO_FAST;
  p.mixed_out = p.mixed && attention_reads_tables(H);
  // the CLS rows' FeedForward of the last layer on mixed operands too (round 5; rounds 2-4 kept it on split-bf16 because those rows ARE the
  // classifier's input): 0.141 -> 0.119 ms for the two launches, logit error against the CPU oracle 6.2e-5 -> 6.6e-5 on the bench batch -- inside
  // the 3e-4 the parity tests hold the mode to
  p.cls_mixed = p.mixed;
  // VETO_MIXED runs everything of a layer behind its attention as ONE panel launch (ffn_fused.hip MODE 2); VETO_TAIL_FUSED=0 (a knob
  // the parity tests compare against) splits it into the out projection + LayerNorm2 launch and the FeedForward + LayerNorm1 launch
  // of the same kernel.  VETO_PRECISE takes the launch-per-Linear GEMMs and LayerNorm launches; VETO_FAST is VETO_MIXED's launches.
  static const bool tail_off = env_knob_is("VETO_TAIL_FUSED", "0");
  p.tail_fused = !tail_off && !sat;
  p.panel = !sat;        // (the saturation audit needs the LayerNorm2 rows and the hidden activation in memory)
  // q / k / v as 3-byte floats between the QKV GEMM of a mixed layer and the attention kernel (common.h; VETO_QKV_F24=0: fp32)
  static const bool qkv_f24_off = env_knob_is("VETO_QKV_F24", "0");
  p.qkv_f24 = !qkv_f24_off && attention_reads_tables(H);
  // middle layers: QKV projection + attention as ONE launch (qkv_attn_fused.hip): q / k / v never reach memory.  The attention output
  // then lives in ws.big (every head's tile reads all rows of ws.a), the layer tail takes it from there and writes the next layer's
  // LayerNorm1 rows back to ws.a.  VETO_QKV_ATTN_FUSED=0 (a knob the parity tests compare against): the two launches.
  static const bool qa_off = env_knob_is("VETO_QKV_ATTN_FUSED", "0");
  p.qa_fused = p.mixed && p.mixed_out && p.tail_fused && !qa_off && qkv_attn_fused_supports(H);
  // VETO_X_F24=1 (off by default; round 6, measured null): the residual stream BETWEEN the layers as 3-byte floats (common.h: a 16-bit
  // significand) -- token assembly writes them, every layer tail reads them, every tail but the last writes them: a quarter fewer bytes in
  // the two bursts of a panel boundary.  The last tail writes fp32 rows for the last layer's CLS-row kernels, into the buffer that held
  // the LayerNorm1 rows (dead by then: rows of another pitch cannot go over 3-byte rows that other workgroups have yet to read; the
  // folded last layer keeps its own operands in ws.big), so the form needs a fused QKV + attention launch in front of the last tail
  // (L >= 3).  Same-box A/B on the bench batch: 10.99 / 11.03 ms with, 10.98 / 11.02 ms without (profiles/r06_tail_variants.txt) -- the
  // bursts are bound by their request count (16 row pieces per wave instruction either way), not by their bytes -- at a logit error of
  // 1.0-1.4e-4 instead of 5-7e-5.  Kept as a tested variant, not as the default.
  static const bool x_f24_on = env_knob_is("VETO_X_F24", "1");
  p.x_f24 = x_f24_on && !p.fast && p.mixed && p.mixed_out && p.tail_fused && p.fold_last && p.qkv0_tables && p.qa_fused && L >= 3;
  return p;
}

// ---- stage 0: pair indices + per-object partial products (once per call, before the chunks) --------------------------------
int object_side(veto_handle_t h, hipStream_t s, const Workspace& ws, const ForwardPlan& p, const veto_inputs_t* in,
                const veto_debug_outputs_t* dbg) {
  const int n_obj = in->n_obj, n_pair = in->n_pair;
  {
    ProfScope ps(h, s, "pair_indices", 0, (double)n_pair * 24);
    HIP_TRY(launch_pair_indices(in->rel_pairs, in->img_obj_offset, in->img_pair_offset, in->n_img, n_pair, ws.subj,
                                ws.obj, dbg ? dbg->subj_inds : nullptr, dbg ? dbg->obj_inds : nullptr, s));
  }
  {
    // training-mode BatchNorm: this batch's statistics (biased variance)
    if (in->bn_batch_stats) HIP_TRY(launch_bn_batch_stats(in->boxes, in->box_mode, n_obj, in->bn_batch_stats, s));
    const ObjPrepArgs a = obj_prep_args(h, in, ws.lc);
    ProfScope ps(h, s, "obj_prep", 2.0 * n_obj * 2 * kDim * (kPosDim + h->cfg.embed_dim), (double)n_obj * 2 * 2 * kDim * 4);
    HIP_TRY(launch_obj_prep(a, s));
  }
  {
    ProfScope ps(h, s, "patchify", 0, (double)n_obj * patch_feats(h->cfg.patch) * 16 * (4 + 4));
    HIP_TRY(launch_patchify(in->roi_depth, in->roi_rgb, ws.pa, n_obj, h->cfg.patch, s));
  }
  int rc = run_gemm(h, s, "gemm_patch", ws.pa, h->patch_w, h->patch_bias, nullptr, 0, ws.patch_tab, nullptr, 2 * kDim,
                    n_obj * 16, 2 * kDim, patch_feats(h->cfg.patch), EPI_F32);
  if (rc || !p.qkv0_tables) return rc;
  const int R = n_obj * 16;
  HIP_TRY(launch_centre_split(ws.patch_tab, ws.ptab_split, R, s));
  ABI_TRY(run_gemm(h, s, "gemm_qkv0_tab", ws.ptab_split, h->q0_w, h->q0_vec + 3 * kDim, nullptr, 0, ws.sw, nullptr, 3 * kDim, R, 3 * kDim, kDim,
                   EPI_F32, (long)2 * 2 * kDim, 0));
  return run_gemm(h, s, "gemm_qkv0_tab", ws.ptab_split + 2 * kDim, h->q0_w, nullptr, nullptr, 0, ws.ow, nullptr, 3 * kDim, R, 3 * kDim, kDim,
                  EPI_F32, (long)2 * 2 * kDim, 0);
}

// One chunk of pairs [c0, c0 + np) on its way through the layers: M = np * 19 token rows in ws.x / ws.a / ws.big
struct Chunk {
  veto_handle_t h;
  hipStream_t s;
  const Workspace& ws;
  const ForwardPlan& p;
  int c0, np, M;
  unsigned long long* sat;      // veto_forward_saturation: device counters [layers][VETO_SAT_SITES][4]
  const float* xlast;           // the residual stream the last layer reads (x_f24: the fp32 rows the last tail wrote)
  float* qkv() const { return (float*)ws.big; }
  __bf16* hid() const { return (__bf16*)ws.big; }  // MLP hidden, split rows [M, 2*1152] (qkv is dead by then)
  hipError_t count_sat(int layer, int site, const void* rows, long stride_bytes, int n_rows, int K) const {
    if (!sat) return hipSuccess;
    return launch_count_saturation(rows, stride_bytes, n_rows, K, sat + ((size_t)layer * VETO_SAT_SITES + site) * 4, s);
  }

  int assemble_tokens(float* dbg_tokens) {
    {
      AssembleArgs a = assemble_args(h, ws.patch_tab, ws.lc, ws.subj + c0, ws.obj + c0, ws.x, ws.a, np);
      a.stats = p.qkv0_tables ? ws.stats : nullptr;
      a.x_f24 = p.x_f24 ? 1 : 0;
      a.a_fmt = p.mixed && p.qkv0_tables ? FMT_MIXED : FMT_SPLIT;   // (the rows of tokens 17 / 18: the A operand of gemm_qkv0_lc below)
      // bytes = what the kernel WRITES (its HBM stream; the per-object rows it gathers are cache-resident): the fp32 token rows
      // plus either their LayerNorm'ed split copy, or -- per-object layer 0 -- the row statistics and the split rows of tokens 17, 18
      ProfScope ps(h, s, "assemble_tokens", 0, (double)M * kDim * (p.x_f24 ? 3 : 4) + (p.qkv0_tables ? (double)M * 8 + 2.0 * np * kDim * 4 : (double)M * kDim * 4));
      HIP_TRY(launch_assemble(a, s));
    }
    if (dbg_tokens) {
      float* dst = dbg_tokens + (size_t)c0 * kTokens * kDim;
      if (p.x_f24) HIP_TRY(launch_unpack_f24(ws.x, dst, (size_t)M * kDim, s));
      else HIP_TRY(hipMemcpyAsync(dst, ws.x, (size_t)M * kDim * 4, hipMemcpyDeviceToDevice, s));
    }
    return VETO_OK;
  }

  // Layer 0, table form: q / k / v of the 17 CLS / patch tokens come from the per-object tables (formed on load by the MFMA attention
  // kernel, or materialised here); only the two location / class rows of every pair go through a QKV GEMM
  int qkv0_from_tables() {
    const LayerW& w = h->layers[0];
    const bool mixed = p.mixed;
    if (!attention_reads_tables(p.H)) {   // head widths without an MFMA attention: materialise the rows of tokens 0..16
      ProfScope ps(h, s, "qkv0_combine", 0, (double)np * 17 * 3 * kDim * 4 * 3);
      HIP_TRY(launch_qkv0_combine(ws.sw, ws.ow, ws.stats, h->q0_vec, ws.subj + c0, ws.obj + c0, qkv(), np, s));
    }
    for (int t = kTokens - 2; t < kTokens; ++t) {   // the ReLU'd location / class rows: LayerNorm'ed rows x Wqkv as usual (VETO_MIXED: mixed operands)
      if (mixed) HIP_TRY(count_sat(0, VETO_SAT_QKV_IN, ws.a + (size_t)t * 2 * kDim, (long)kTokens * kDim * 4, np, kDim));
      ABI_TRY(run_gemm(h, s, "gemm_qkv0_lc", ws.a + (size_t)t * 2 * kDim, mixed ? w.qkv_m : w.qkv, nullptr, nullptr, 0,
                       qkv() + (size_t)t * 3 * kDim, nullptr, (long)kTokens * 3 * kDim, np, 3 * kDim, kDim, EPI_F32, (long)kTokens * 2 * kDim, 0,
                       DropSite(), mixed ? w.exp_m + LIN_QKV : nullptr));
    }
    return VETO_OK;
  }

  // The attention launch on q / k / v rows in ws.big (layer 0 in table form: formed on load from the tables); the last layer's covers
  // the CLS query of every pair only and writes compact rows
  int attention(int l, bool qkv_f24) {
    const bool last = l == p.L - 1;
    AttnArgs a{};
    a.qkv = qkv(); a.n_pair = np; a.heads = p.H; a.cls_only = last ? 1 : 0;
    a.qkv_f24 = qkv_f24 ? 1 : 0;
    a.o = last ? ws.ac : ws.a;
    a.o_fmt = (!last && p.mixed_out) ? FMT_MIXED : FMT_SPLIT;
    if (l == 0 && p.qkv0_tables && attention_reads_tables(p.H)) {   // q / k / v of the patch tokens are formed on load
      a.sw = ws.sw; a.ow = ws.ow; a.stats = ws.stats; a.vec = h->q0_vec; a.subj = ws.subj + c0; a.obj = ws.obj + c0;
    }
    const double nq = last ? 1 : kTokens;
    ProfScope ps(h, s, last ? "attention_cls" : "attention", 4.0 * np * nq * kTokens * kDim,
                 (double)M * 3 * kDim * (qkv_f24 ? 3 : 4) + (double)np * nq * kDim * 4);
    HIP_TRY(launch_attention(a, s));
    if (a.o_fmt == FMT_MIXED) HIP_TRY(count_sat(l, VETO_SAT_ATTN_OUT, ws.a, (long)kDim * 4, M, kDim));
    return VETO_OK;
  }

  // QKV projection + attention of a layer that is neither in table form nor the last: one launch, whose output is in ws.big
  // (*attn_in_big), or the QKV GEMM and the attention launch
  int qkv_attention(int l, bool* attn_in_big) {
    const LayerW& w = h->layers[l];
    if (p.qa_fused && l > 0) {
      QkvAttnArgs q{};
      q.a = (const char*)ws.a; q.w = (const char*)w.qkv_m; q.w_exp = w.exp_m + LIN_QKV; q.o = ws.big; q.n_pair = np; q.heads = p.H; q.fast = p.fast ? 1 : 0;
      ProfScope ps(h, s, "qkv_attn_fused", 2.0 * M * 3.0 * kDim * kDim + 4.0 * np * kTokens * kTokens * kDim,
                   (double)M * kDim * 8 + 3.0 * kDim * kDim * 4);
      HIP_TRY(launch_qkv_attn_fused(q, s));
      *attn_in_big = true;
      return VETO_OK;
    }
    const bool mq = p.mixed && l > 0;   // layer 0's LayerNorm'ed rows come from token assembly (split rows)
    const bool qkv_f24 = mq && p.qkv_f24;
    if (mq) HIP_TRY(count_sat(l, VETO_SAT_QKV_IN, ws.a, (long)kDim * 4, M, kDim));
    int rc = run_gemm(h, s, "gemm_qkv", ws.a, mq ? w.qkv_m : w.qkv, nullptr, nullptr, 0, qkv(), nullptr, 3 * kDim, M, 3 * kDim, kDim,
                      qkv_f24 ? EPI_F24 : EPI_F32, 0, 0, DropSite(), mq ? w.exp_m + LIN_QKV : nullptr);
    return rc ? rc : attention(l, qkv_f24);
  }

  // Everything of the layer behind its attention in ONE launch (ffn_fused.hip, MODE 2): x1 = x + a Wo^T + bo stays in
  // registers, LayerNorm2(x1) is written in place over the attention output and streamed back as the FeedForward's
  // input, fc2 accumulates on top of x1, the epilogue stores x (and the next layer's LayerNorm1 rows)
  int layer_tail_one_launch(int l, bool attn_in_big) {
    const LayerW& w = h->layers[l];
    const LayerW& nx = h->layers[l + 1];
    const bool ln_next = p.ffn_ln_next(l);
    char* rows = attn_in_big ? ws.big : (char*)ws.a;      // the attention output; the LayerNorm2 rows go over it in place ...
    // ... and the next layer's LayerNorm1 rows too, unless ws.a is free for them (fused QKV + attention launch)
    const RowNorm next{ln_next ? nx.ln1_w : nullptr, ln_next ? nx.ln1_b : nullptr, attn_in_big ? ws.a : nullptr};
    FfnArgs f = layer_tail_args(rows, w.mixed(LIN_OUT), RowNorm{w.ln2_w, w.ln2_b, rows}, w.mixed(LIN_FC1), w.mixed(LIN_FC2), ws.x, M, next);
    f.fast = p.fast ? 1 : 0;
    if (p.x_f24) {
      f.resid_f24 = 1;
      if (l + 1 < p.L - 1) f.out_f24 = 1;
      else {      // the last tail: fp32 rows for the folded last layer, into a buffer that is dead by now (rows of another pitch
                  // cannot go over the 3-byte rows other workgroups have yet to read)
        if (!attn_in_big) return fail(VETO_ERR_INVALID, "internal: 3-byte residual rows without a free buffer for the last tail's fp32 rows");
        f.out = (float*)ws.a;
        xlast = (const float*)ws.a;
      }
    }
    ProfScope ps(h, s, "layer_tail_fused", 2.0 * M * (double)kDim * kDim + 2.0 * 2.0 * M * (double)kDim * 2 * kDim,
                 (double)M * kDim * (p.x_f24 ? (f.out_f24 ? 14 : 15) : 16) + 5.0 * kDim * kDim * 4);
    HIP_TRY(launch_layer_tail(f, s));
    return VETO_OK;
  }

  // x <- x + a Wo^T + bo, then a <- LayerNorm2(x): one panel launch, or the GEMM and a LayerNorm launch
  int out_projection(int l) {
    const LayerW& w = h->layers[l];
    if (p.mixed_out && p.panel) {
      // out projection + residual + LayerNorm2 in one launch on full rows (ffn_fused.hip, MODE 1): x <- x + a Wo^T + bo, then
      // a <- LayerNorm2(x) as mixed rows in place over the attention output
      const FfnArgs f = out_panel_args(ws.a, w.mixed(LIN_OUT), ws.x, M, RowNorm{w.ln2_w, w.ln2_b, ws.a});
      ProfScope ps(h, s, "out_ln_fused", 2.0 * M * (double)kDim * kDim, (double)M * kDim * 16 + (double)kDim * kDim * 4);
      HIP_TRY(launch_out_fused(f, s));
      return VETO_OK;
    }
    ABI_TRY(run_gemm(h, s, "gemm_out", ws.a, p.mixed_out ? w.out_m : w.out, w.out_b, ws.x, kDim, ws.x, nullptr, kDim, M, kDim, kDim, EPI_RESID,
                     0, 0, DropSite(), p.mixed_out ? w.exp_m + LIN_OUT : nullptr));
    {
      ProfScope ps(h, s, "layernorm", 0, (double)M * kDim * 8);
      HIP_TRY(launch_layernorm(ws.x, kDim, w.ln2_w, w.ln2_b, ws.a, M, s, p.mixed ? FMT_MIXED : FMT_SPLIT));
    }
    if (p.mixed) HIP_TRY(count_sat(l, VETO_SAT_FFN_IN, ws.a, (long)kDim * 4, M, kDim));
    return VETO_OK;
  }

  // x <- x + fc2(gelu(fc1(a))): one panel launch (which can write the next layer's LayerNorm1 rows too), or the two GEMMs
  int feed_forward(int l) {
    const LayerW& w = h->layers[l];
    const bool mixed = p.mixed;
    if (mixed && p.panel) {
      // FeedForward in one launch (ffn_fused.hip): the hidden activation never leaves the CU
      const LayerW& nx = h->layers[l + 1];
      // the next layer's LayerNorm1 in the epilogue (mixed rows, in place over this launch's input rows)
      const FfnArgs f = ffn_panel_args(ws.a, w.mixed(LIN_FC1), w.mixed(LIN_FC2), ws.x, M,
                                       p.ffn_ln_next(l) ? RowNorm{nx.ln1_w, nx.ln1_b, ws.a} : RowNorm());
      // bytes: the LayerNorm'ed rows in, the residual stream in and out, the two weight matrices
      ProfScope ps(h, s, "ffn_fused", 2.0 * 2.0 * M * (double)kDim * 2 * kDim, (double)M * kDim * 12 + 2.0 * 2 * kDim * kDim * 4);
      HIP_TRY(launch_ffn_fused(f, s));
      return VETO_OK;
    }
    ABI_TRY(run_gemm(h, s, "gemm_fc1", ws.a, mixed ? w.fc1_m : w.fc1, w.fc1_b, nullptr, 0, nullptr, hid(), 4 * kDim, M, 2 * kDim, kDim,
                     EPI_GELU_SPLIT, 0, 0, DropSite(), mixed ? w.exp_m + LIN_FC1 : nullptr));
    if (mixed) HIP_TRY(count_sat(l, VETO_SAT_HIDDEN, hid(), (long)2 * kDim * 4, M, 2 * kDim));
    return run_gemm(h, s, "gemm_fc2", hid(), mixed ? w.fc2_m : w.fc2, w.fc2_b, ws.x, kDim, ws.x, nullptr, kDim, M, kDim, 2 * kDim, EPI_RESID,
                    0, 0, DropSite(), mixed ? w.exp_m + LIN_FC2 : nullptr);
  }

  // Everything behind the attention of a layer that is not the last: ONE launch, two panel launches, or a launch per Linear
  int layer_tail(int l, bool attn_in_big) {
    if (p.mixed_out && p.tail_fused) return layer_tail_one_launch(l, attn_in_big);
    const int rc = out_projection(l);
    return rc ? rc : feed_forward(l);
  }

  // The LayerNorm1 rows of layer l + 1, unless something else writes them
  int layernorm_next(int l) {
    const LayerW& nx = h->layers[l + 1];
    if (l + 1 == p.L - 1 && p.fold_last) return VETO_OK;      // the folded last layer LayerNorms its token rows itself
    if (p.ffn_ln_next(l)) return VETO_OK;                     // written by the fused FeedForward launch
    ProfScope ps(h, s, "layernorm", 0, (double)M * kDim * 8);
    // the next layer's QKV GEMM takes mixed rows unless it is the (unfolded) last layer
    HIP_TRY(launch_layernorm(ws.x, kDim, nx.ln1_w, nx.ln1_b, ws.a, M, s, (p.mixed && l + 1 < p.L - 1) ? FMT_MIXED : FMT_SPLIT));
    return VETO_OK;
  }

  // Last layer, folded (attention.hip): u = a_0 . Mcat on the CLS rows, per-pair scores / softmax / weighted token means,
  // then out = abar . Ncat^T + b_o + x_0 -- no key / value projection of the 19 tokens.  Leaves x_mid of the CLS rows in ws.xc
  int last_layer_folded() {
    const LayerW& w = h->layers[p.L - 1];
    const int H = p.H;
    int rc;
    Carver fold{ws.big};      // u fp32 [rows, H*576] | abar split [rows, 2*H*576]: carve() reserved both for cls_fold_max_heads() heads
    float* u = fold.take<float>((size_t)gemm_rows_padded(np) * H * kDim * 4);
    __bf16* abar = fold.take<__bf16>((size_t)gemm_rows_padded(np) * 2 * H * kDim * 2);
    {   // LayerNorm1 of the CLS rows (row p*19 of x -> compact split row p): the A operand of the u GEMM
      ProfScope ps(h, s, "layernorm_cls", 0, (double)np * kDim * 8);
      HIP_TRY(launch_layernorm(xlast, (long)kTokens * kDim, w.ln1_w, w.ln1_b, ws.ac, np, s));
    }
    const int dhp = p.dhp, npad = H * dhp;   // block form: padded width of the per-head q / v rows
    bool u24 = false;
    if (dhp > 0) {
      // q0 = a0 Wq_pad^T as split rows (every head's dh columns padded to dhp), then u = q0 . blockdiag(Wk): column tile n of u
      // belongs to head n / 3 and multiplies that head's dhp / 32 k-steps only
      ABI_TRY(run_gemm(h, s, "gemm_q_cls", ws.ac, h->fold_q, nullptr, nullptr, 0, nullptr, ws.hc, 2L * npad, np, npad, kDim, EPI_SPLIT));
      u24 = cls_fold_reads_f24();      // u as 3-byte floats: its consumer splits it into bf16 hi + lo, a 16-bit significand
      rc = run_gemm(h, s, "gemm_u_cls", ws.hc, h->fold_k, nullptr, nullptr, 0, u, nullptr, (long)H * kDim, np, H * kDim, npad,
                    u24 ? EPI_F24 : EPI_F32, 0, 0, DropSite(), nullptr, 3, dhp / 32);
    } else {
      rc = run_gemm(h, s, "gemm_u_cls", ws.ac, h->fold_m, nullptr, nullptr, 0, u, nullptr, (long)H * kDim, np, H * kDim, kDim, EPI_F32);
    }
    if (rc) return rc;
    {
      ProfScope ps(h, s, "attention_cls", 4.0 * np * H * kTokens * kDim, (double)M * kDim * 4 + (double)np * H * kDim * 8);
      HIP_TRY(launch_cls_fold_attention(xlast, w.ln1_w, w.ln1_b, u, abar, np, H, s, u24));
    }
    if (dhp > 0) {
      // vbar = abar . blockdiag(Wv)^T as split rows (column tile n covers the 192 / dhp heads whose 576-wide k blocks it needs),
      // then out = vbar Wo_pad^T + b_o + x_0
      const int hpt = 192 / dhp;
      ABI_TRY(run_gemm(h, s, "gemm_v_cls", abar, h->fold_v, nullptr, nullptr, 0, nullptr, ws.hc, 2L * npad, np, npad, H * kDim, EPI_SPLIT,
                       0, 0, DropSite(), nullptr, 1, hpt * kDim / 32));
      return run_gemm(h, s, "gemm_out_cls", ws.hc, h->fold_o, w.out_b, xlast, (long)kTokens * kDim, ws.xc, nullptr, kDim, np, kDim, npad,
                      EPI_RESID);
    }
    return run_gemm(h, s, "gemm_out_cls", abar, h->fold_n, w.out_b, xlast, (long)kTokens * kDim, ws.xc, nullptr, kDim, np, kDim,
                    H * kDim, EPI_RESID);
  }

  // Last layer, plain: keys/values for all 19 tokens, the query for the CLS row of each pair only; the attention and the out
  // projection + residual on the CLS rows (row p*19 of x -> compact row p) leave x_mid in ws.xc
  int last_layer_plain() {
    const LayerW& w = h->layers[p.L - 1];
    ABI_TRY(run_gemm(h, s, "gemm_kv_last", ws.a, w.qkv, nullptr, nullptr, 0, qkv() + kDim, nullptr, 3 * kDim, M, 2 * kDim,
                     kDim, EPI_F32, 0, kDim));
    ABI_TRY(run_gemm(h, s, "gemm_q_cls", ws.a, w.qkv, nullptr, nullptr, 0, qkv(), nullptr, (long)kTokens * 3 * kDim, np, kDim,
                     kDim, EPI_F32, (long)kTokens * 2 * kDim, 0));
    ABI_TRY(attention(p.L - 1, false));
    return run_gemm(h, s, "gemm_out_cls", ws.ac, w.out, w.out_b, ws.x, (long)kTokens * kDim, ws.xc, nullptr, kDim, np,
                    kDim, kDim, EPI_RESID);
  }

  // Only x[:, 0] of the last layer is consumed (model_veto.py:23): FeedForward and its residual run on the CLS row of each pair
  // (compact rows in ws.xc), behind either form of the last layer's attention
  int cls_feed_forward() {
    const int l = p.L - 1;
    const LayerW& w = h->layers[l];
    const bool cls_mixed = p.cls_mixed;
    {
      ProfScope ps(h, s, "layernorm_cls", 0, (double)np * kDim * 8);
      HIP_TRY(launch_layernorm(ws.xc, kDim, w.ln2_w, w.ln2_b, ws.ac, np, s, cls_mixed ? FMT_MIXED : FMT_SPLIT));
    }
    // (the CLS rows' FeedForward takes mixed operands too, and those rows are the classifier's input: audited like every other site)
    if (cls_mixed) HIP_TRY(count_sat(l, VETO_SAT_FFN_IN, ws.ac, (long)kDim * 4, np, kDim));
    ABI_TRY(run_gemm(h, s, "gemm_fc1_cls", ws.ac, cls_mixed ? w.fc1_m : w.fc1, w.fc1_b, nullptr, 0, nullptr, ws.hc, 4 * kDim, np, 2 * kDim, kDim,
                     EPI_GELU_SPLIT, 0, 0, DropSite(), cls_mixed ? w.exp_m + LIN_FC1 : nullptr));
    if (cls_mixed) HIP_TRY(count_sat(l, VETO_SAT_HIDDEN, ws.hc, (long)2 * kDim * 4, np, 2 * kDim));
    return run_gemm(h, s, "gemm_fc2_cls", ws.hc, cls_mixed ? w.fc2_m : w.fc2, w.fc2_b, ws.xc, kDim, ws.xc, nullptr, kDim, np, kDim, 2 * kDim,
                    EPI_RESID, 0, 0, DropSite(), cls_mixed ? w.exp_m + LIN_FC2 : nullptr);
  }

  int head(float* out_logits, float* dbg_cls) {
    const int n_out = h->cfg.num_out;
    {
      ProfScope ps(h, s, "head", 2.0 * np * kDim * n_out, (double)np * (kDim + n_out) * 4);
      HIP_TRY(launch_head(ws.xc, h->head_wt, h->p("rel_out.bias"), out_logits + (size_t)c0 * n_out, np, n_out, s));
    }
    if (dbg_cls) HIP_TRY(hipMemcpyAsync(dbg_cls + (size_t)c0 * kDim, ws.xc, (size_t)np * kDim * 4, hipMemcpyDeviceToDevice, s));
    return VETO_OK;
  }
};

// The frozen region of a training step (frozen_forward): the forward covers layers < k; k < layers: it ends behind layer k - 1's tail
// with the residual rows copied to handoff
struct FrozenRegion {
  int k;
  float* handoff;
};

// sat != nullptr (veto_forward_saturation): device counters [layers][VETO_SAT_SITES][4]
int forward_impl(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace, size_t workspace_bytes, float* out_logits,
                 const veto_debug_outputs_t* dbg, unsigned long long* sat, const FrozenRegion* fz = nullptr) {
  CHECK_STRUCT_AND(veto_inputs_t, in, h && out_logits);
  if (dbg) CHECK_STRUCT(veto_debug_outputs_t, dbg);
  if (in->n_obj <= 0 || in->n_pair <= 0 || in->n_img <= 0) return fail(VETO_ERR_INVALID, "empty batch (n_obj=%d n_pair=%d n_img=%d)", in->n_obj, in->n_pair, in->n_img);
  if (!in->roi_rgb || !in->roi_depth || !in->boxes || !in->rel_pairs || !in->img_obj_offset || !in->img_pair_offset)
    return fail(VETO_ERR_INVALID, "missing input pointer");
  if (!in->obj_labels && !in->obj_logits) return fail(VETO_ERR_INVALID, "need obj_labels or obj_logits");
  if ((size_t)in->n_obj * 16 > (size_t)1 << 30 || (size_t)in->n_pair * kTokens > (size_t)1 << 30)
    return fail(VETO_ERR_INVALID, "batch too large");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int n_obj = in->n_obj, n_pair = in->n_pair;
  const int chunk = n_pair < h->chunk ? n_pair : h->chunk;
  const int stop = fz && fz->k < h->cfg.layers ? fz->k : 0;      // > 0: the forward ends behind the tail of layer stop - 1
  if (fz && (fz->k < 1 || fz->k > h->cfg.layers || (stop && !fz->handoff))) return fail(VETO_ERR_INVALID, "internal: bad frozen region");
  // (a frozen region: the step's own trainable layers have no use for their inference operands)
  if (h->dirty || h->infer_dirty) ABI_TRY(finalize_weights(h, s, false, fz ? fz->k : -1));
  const Workspace ws = fz ? carve((char*)workspace, n_obj, n_pair, chunk, h->cfg.patch, frozen_fold_heads(h), stop == 0)
                          : carve((char*)workspace, n_obj, n_pair, chunk, h->cfg.patch);
  ABI_TRY(check_workspace(workspace, workspace_bytes, ws.total, true));
  const ForwardPlan p = make_plan(h, sat != nullptr);
  if (fz && p.x_f24) return fail(VETO_ERR_INVALID, "internal: the frozen region hands over fp32 residual rows (VETO_X_F24=1)");

  ABI_TRY(object_side(h, s, ws, p, in, dbg));
  // ---- pairs, in chunks that bound the workspace ----------------------------------------------
  for (int c0 = 0; c0 < n_pair; c0 += chunk) {
    const int np = (n_pair - c0 < chunk) ? n_pair - c0 : chunk;
    Chunk c{h, s, ws, p, c0, np, np * kTokens, sat, ws.x};
    int rc = c.assemble_tokens(dbg ? dbg->tokens : nullptr);
    for (int l = 0; l < (stop ? stop : p.L - 1) && !rc; ++l) {
      bool attn_in_big = false;      // this layer's attention output is in ws.big (fused QKV + attention launch)
      if (l == 0 && p.qkv0_tables) {
        if (!(rc = c.qkv0_from_tables())) rc = c.attention(0, false);
      } else {
        rc = c.qkv_attention(l, &attn_in_big);
      }
      if (!rc) rc = c.layer_tail(l, attn_in_big);
      if (!rc && l + 1 != stop) rc = c.layernorm_next(l);      // (the training forward of layer `stop` LayerNorms its input rows itself)
    }
    if (stop) {      // hand the chunk's residual rows to the training forward
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(fz->handoff + (size_t)c0 * kTokens * kDim, ws.x, (size_t)c.M * kDim * 4, hipMemcpyDeviceToDevice, s));
      continue;
    }
    if (!rc) rc = p.fold_last ? c.last_layer_folded() : c.last_layer_plain();
    if (!rc) rc = c.cls_feed_forward();
    if (!rc) rc = c.head(out_logits, dbg ? dbg->cls : nullptr);
    if (rc) return rc;
  }
  return VETO_OK;
}

}  // namespace

// ---- the frozen region of a training step (abi_internal.h) -----------------------------------------------------------------
size_t frozen_forward_workspace_bytes(veto_handle_t h, int n_obj, int n_pair, int k) {
  const int chunk = n_pair < h->chunk ? n_pair : h->chunk;
  return carve(nullptr, n_obj, n_pair, chunk, h->cfg.patch, frozen_fold_heads(h), k >= h->cfg.layers).total;
}

int frozen_forward(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace, size_t workspace_bytes, int k, float* handoff,
                   float* out_logits, float* cls_rows) {
  veto_inputs_t eval_in = *in;      // (an eval-mode pos_embed.0: the running statistics)
  eval_in.bn_batch_stats = nullptr;
  veto_debug_outputs_t dbg{};
  dbg.struct_size = (int32_t)sizeof(dbg);
  dbg.cls = cls_rows;
  const FrozenRegion fz{k, handoff};
  return forward_impl(h, stream, &eval_in, workspace, workspace_bytes, out_logits, &dbg, nullptr, &fz);
}

extern "C" {

size_t veto_workspace_bytes(veto_handle_t h, int32_t n_obj, int32_t n_pair) {
  if (!h || n_obj <= 0 || n_pair <= 0) return 0;
  const int chunk = n_pair < h->chunk ? n_pair : h->chunk;
  return carve(nullptr, n_obj, n_pair, chunk, h->cfg.patch).total;
}

int veto_forward(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace,
                 size_t workspace_bytes, float* out_logits, const veto_debug_outputs_t* dbg) {
  return forward_impl(h, stream, in, workspace, workspace_bytes, out_logits, dbg, nullptr);
}

int veto_forward_saturation(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace, size_t workspace_bytes,
                            float* out_logits, veto_saturation_t* counts, int32_t capacity) {
  if (!h || !counts) return fail(VETO_ERR_INVALID, "null argument");
  if (h->cfg.precision != VETO_MIXED) return fail(VETO_ERR_INVALID, "veto_forward_saturation audits the VETO_MIXED operands; this handle computes in another mode");
  const int n = h->cfg.layers * VETO_SAT_SITES;
  if (capacity < n) return fail(VETO_ERR_INVALID, "counts holds %d entries, need layers * VETO_SAT_SITES = %d", capacity, n);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (!h->sat_buf) return fail(VETO_ERR_INVALID, "no saturation counters (handle not created in VETO_MIXED)");
  HIP_TRY(hipMemsetAsync(h->sat_buf, 0, (size_t)n * 4 * sizeof(unsigned long long), s));
  ABI_TRY(forward_impl(h, stream, in, workspace, workspace_bytes, out_logits, nullptr, h->sat_buf));
  std::vector<unsigned long long> host((size_t)n * 4);
  HIP_TRY(hipMemcpyAsync(host.data(), h->sat_buf, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) {
    counts[i].elements = (int64_t)host[i * 4 + 0];
    counts[i].f16_saturated = (int64_t)host[i * 4 + 1];
    counts[i].value_saturated = (int64_t)host[i * 4 + 2];
    counts[i].resid_saturated = (int64_t)host[i * 4 + 3];
  }
  return VETO_OK;
}

}  // extern "C"
