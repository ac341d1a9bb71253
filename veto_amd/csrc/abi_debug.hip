// Test and measurement hooks of the inference path's GEMM and fused launches (include/veto_amd.h, veto_debug_*): each builds its
// operands from fp32 inputs and makes the launch with the argument set the forward builds (abi_internal.h); and of the training
// step's backward blocks, where veto_debug_wgrad makes its launch through the helper the step itself uses (launch_wgrad).
#include "abi_internal.h"

namespace {

// Optional device timing of a hook's launches from a hipEvent pair on its stream; without init() every call does nothing
struct EventTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = nullptr;
  float total_ms = 0.f;      // over every start() .. stop() span so far
  hipError_t init(hipStream_t stream) {
    s = stream;
    hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  hipError_t start() { return e1 ? hipEventRecord(e0, s) : hipSuccess; }
  hipError_t stop() {      // waits for the span to finish
    if (!e1) return hipSuccess;
    float ms = 0.f;
    hipError_t e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    total_ms += ms;
    return e;
  }
  ~EventTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// ---- the hooks' workspaces: operand rows built from the fp32 inputs (activation rows padded to whole GEMM tiles), then 256 bytes for the
// mixed weights' exponents.  (A braced list evaluates left to right: the members are carved in their order.)
const size_t kW = (size_t)kDim * kDim * 4;      // bytes of a 576 x 576 weight as split or mixed rows
size_t act_bytes(size_t rows, size_t k) { return (size_t)gemm_rows_padded((int)rows) * k * 4; }

struct GemmWs { __bf16 *a, *w; int* w_exp; size_t total; };       // veto_debug_gemm, veto_debug_gemm_forms
GemmWs carve_gemm(Carver c, int m, int n, int k) {
  return GemmWs{c.take<__bf16>(act_bytes(m, k)), c.take<__bf16>((size_t)n * k * 4), c.take<int>(256), c.off};
}

struct FfnWs { __bf16 *a, *hid, *w1, *w2; int* exps; size_t total; };
FfnWs carve_ffn(Carver c, int m) {
  return FfnWs{c.take<__bf16>(act_bytes(m, kDim)), c.take<__bf16>(act_bytes(m, 2 * kDim)), c.take<__bf16>(2 * kW), c.take<__bf16>(2 * kW),
               c.take<int>(256), c.off};
}

struct OutprojWs { __bf16 *a, *w; int* exps; size_t total; };
OutprojWs carve_outproj(Carver c, int m) {
  return OutprojWs{c.take<__bf16>(act_bytes(m, kDim)), c.take<__bf16>(kW), c.take<int>(256), c.off};
}

struct LayerTailWs { __bf16 *a, *wo, *w1, *w2; int* exps; size_t total; };
LayerTailWs carve_layer_tail(Carver c, int m) {
  return LayerTailWs{c.take<__bf16>(act_bytes(m, kDim)), c.take<__bf16>(kW), c.take<__bf16>(2 * kW), c.take<__bf16>(2 * kW), c.take<int>(256),
                     c.off};
}

struct QkvAttnWs { __bf16* a; char *o, *qkv; __bf16* w; int* exps; size_t total; };
QkvAttnWs carve_qkv_attn(Carver c, int n_pair) {
  // (the fused launch reads whole tiles of 16 pairs: the rows are padded to those too; q / k / v are 3-byte floats)
  const size_t tile_rows = qkv_attn_rows_padded(n_pair), m = (size_t)n_pair * kTokens, rows = tile_rows > m ? tile_rows : m;
  return QkvAttnWs{c.take<__bf16>(act_bytes(rows, kDim)), c.take(act_bytes(rows, kDim)), c.take((size_t)gemm_rows_padded((int)rows) * 3 * kDim * 3),
                   c.take<__bf16>(3 * kW), c.take<int>(256), c.off};
}

// veto_debug_wgrad.  n % 32 == 0 (every Linear of the transformer): the row-major form, both operands as the split rows the backward holds
// anyway, transposed on their way out of LDS (GemmArgs::tn), one row more than m each (partial tiles read, never use, the row behind
// the last) and the zero row of GemmArgs::zero.  Otherwise: explicit transposed split copies, dy's padded to whole row tiles.
// ordered: behind the operands, the partial planes of the ordered form (operand bytes: the size of the default form)
struct WgradWs { WgradSplit split; __bf16 *a, *w, *zero; size_t operand_bytes; float* planes; size_t total; };
WgradWs carve_wgrad(Carver c, int m, int n, int k, int k_splits, bool ordered) {
  const WgradSplit sp = wgrad_split(n, k, m, k_splits, kWgradLinearKsteps, 0);
  const size_t plane_bytes = ordered ? sp.plane_floats * 4 : 0;
  if (n % 32 == 0) return WgradWs{sp, c.take<__bf16>(((size_t)m + 1) * n * 4), c.take<__bf16>(((size_t)m + 1) * k * 4), c.take<__bf16>(1024), c.off,
                                  ordered ? c.take<float>(plane_bytes) : nullptr, c.off};
  return WgradWs{sp, c.take<__bf16>((size_t)gemm_rows_padded(n) * sp.mp * 4), c.take<__bf16>((size_t)k * sp.mp * 4), nullptr, c.off,
                 ordered ? c.take<float>(plane_bytes) : nullptr, c.off};
}

}  // namespace

extern "C" {

size_t veto_debug_gemm_workspace_bytes(int32_t m, int32_t n, int32_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return carve_gemm(Carver{nullptr}, m, n, k).total;
}

int veto_debug_gemm(void* stream, const float* a, const float* w, const float* bias, float* c, int32_t m, int32_t n,
                    int32_t k, int32_t precision, void* workspace, size_t workspace_bytes) {
  if (!a || !w || !c || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_gemm_workspace_bytes(m, n, k), false));
  hipStream_t s = (hipStream_t)stream;
  const auto [a_s, w_s, w_exp, ws_bytes] = carve_gemm(Carver{(char*)workspace}, m, n, k);
  HIP_TRY(hipMemsetAsync(a_s, 0, (char*)w_s - (char*)a_s, s));      // (the rows m..padded stay zero)
  GemmArgs g{};
  if (precision == VETO_MIXED) {
    if (k % 64 != 0) return fail(VETO_ERR_INVALID, "mixed rows need K %% 64 == 0");
    HIP_TRY(launch_mixed_act_rows(a, a_s, (size_t)m, k, s));
    HIP_TRY(launch_mixed_weight_rows(w, w_s, (size_t)n, k, w_exp, s));
    g.fmt = FMT_MIXED; g.w_exp = w_exp;
  } else {
    HIP_TRY(launch_split_rows(a, a_s, (size_t)m, k, s));
    HIP_TRY(launch_split_rows(w, w_s, (size_t)n, k, s));
  }
  g.a = a_s; g.w = w_s; g.bias = bias; g.c = c;
  g.M = m; g.N = n; g.K = k; g.ldc = n;
  hipError_t e = launch_gemm_split(g, EPI_F32, precision == VETO_FAST ? 1 : 0, s);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP,
                                   "gemm launch failed (N must be a multiple of 192, K of 32): %s", hipGetErrorString(e));
  return VETO_OK;
}

// Test hook of the round-3 forms of the split-row GEMM: block-diagonal weights (kb_tiles > 0: column tile n multiplies only the
// k-steps [(n / kb_tiles) * kb_steps, + kb_steps) -- everything outside those blocks of w is ignored) and the output forms:
// out_form 0 = fp32 rows [m, n], 1 = split rows (m x 2n bf16: per 32 columns 32 hi then 32 lo), 2 = 3-byte floats (m x 3n bytes).
// Workspace as for veto_debug_gemm.
int veto_debug_gemm_forms(void* stream, const float* a, const float* w, void* c, int32_t m, int32_t n, int32_t k, int32_t kb_tiles,
                          int32_t kb_steps, int32_t out_form, void* workspace, size_t workspace_bytes) {
  if (!a || !w || !c || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (out_form < 0 || out_form > 2) return fail(VETO_ERR_INVALID, "out_form must be 0, 1 or 2");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_gemm_workspace_bytes(m, n, k), false));
  hipStream_t s = (hipStream_t)stream;
  const auto [a_s, w_s, w_exp, ws_bytes] = carve_gemm(Carver{(char*)workspace}, m, n, k);
  HIP_TRY(hipMemsetAsync(a_s, 0, (char*)w_s - (char*)a_s, s));
  HIP_TRY(launch_split_rows(a, a_s, (size_t)m, k, s));
  HIP_TRY(launch_split_rows(w, w_s, (size_t)n, k, s));
  GemmArgs g{};
  g.a = a_s; g.w = w_s; g.M = m; g.N = n; g.K = k;
  g.kb_tiles = kb_tiles; g.kb_steps = kb_steps;
  if (out_form == 1) { g.c_split = (__bf16*)c; g.ldc = 2L * n; }
  else { g.c = (float*)c; g.ldc = n; }
  hipError_t e = launch_gemm_split(g, out_form == 1 ? EPI_SPLIT : out_form == 2 ? EPI_F24 : EPI_F32, 0, s);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP,
                                   "gemm launch failed (N a multiple of 192, K of 32, the blocks must tile K): %s", hipGetErrorString(e));
  return VETO_OK;
}

// Test / measurement hook of the FeedForward block (model_veto.py:137-143 + the residual of :21) on VETO_MIXED operands:
// x <- x + W2 . gelu(W1 . a + b1) + b2 for m token rows.  mode 0 = the two GEMM launches (fc1 with the GELU epilogue writing
// the hidden activation as mixed rows, fc2 with the residual epilogue), mode 1 = the fused kernel (ffn_fused.hip).
// flags & 1: (re)build the mixed operands from a / w1 / w2 first.  The block runs `reps` times (x accumulates: timing only when
// reps > 1); *ms_per_rep (host, optional) receives the mean device time of one run from hipEvents on `stream`.
size_t veto_debug_ffn_workspace_bytes(int32_t m) {
  return m > 0 ? carve_ffn(Carver{nullptr}, m).total : 0;
}

int veto_debug_ffn(void* stream, const float* a, const float* w1, const float* b1, const float* w2, const float* b2, float* x,
                   int32_t m, int32_t mode, int32_t flags, int32_t reps, float* ms_per_rep, void* workspace, size_t workspace_bytes,
                   const float* ln_w, const float* ln_b, void* ln_rows) {
  if (!a || !w1 || !b1 || !w2 || !b2 || !x || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (m <= 0 || reps <= 0 || (mode != 0 && mode != 1)) return fail(VETO_ERR_INVALID, "bad m / reps / mode");
  if (ln_rows && (!ln_w || !ln_b)) return fail(VETO_ERR_INVALID, "ln_rows needs ln_w and ln_b");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_ffn_workspace_bytes(m), false));
  hipStream_t s = (hipStream_t)stream;
  const auto [a_m, hid, w1_m, w2_m, exps, ws_bytes] = carve_ffn(Carver{(char*)workspace}, m);
  if (flags & 1) {
    HIP_TRY(hipMemsetAsync(a_m, 0, (char*)hid - (char*)a_m, s));
    HIP_TRY(launch_mixed_act_rows(a, a_m, (size_t)m, kDim, s));
    HIP_TRY(launch_mixed_weight_rows(w1, w1_m, (size_t)2 * kDim, kDim, exps + 0, s));
    HIP_TRY(launch_mixed_weight_rows(w2, w2_m, (size_t)kDim, 2 * kDim, exps + 1, s));
  }
  EventTimer timer;      // the whole rep loop
  if (ms_per_rep) HIP_TRY(timer.init(s));
  HIP_TRY(timer.start());
  for (int r = 0; r < reps; ++r) {
    if (mode == 1) {
      HIP_TRY(launch_ffn_fused(ffn_panel_args(a_m, MixedLinear{w1_m, b1, exps + 0}, MixedLinear{w2_m, b2, exps + 1}, x, m,
                                              ln_rows ? RowNorm{ln_w, ln_b, ln_rows} : RowNorm()), s));
    } else {
      GemmArgs g1{};
      g1.fmt = FMT_MIXED; g1.w_exp = exps + 0; g1.a = a_m; g1.w = w1_m; g1.bias = b1; g1.c_split = hid;
      g1.M = m; g1.N = 2 * kDim; g1.K = kDim; g1.ldc = 4 * kDim;
      HIP_TRY(launch_gemm_split(g1, EPI_GELU_SPLIT, 0, s));
      GemmArgs g2{};
      g2.fmt = FMT_MIXED; g2.w_exp = exps + 1; g2.a = hid; g2.w = w2_m; g2.bias = b2; g2.resid = x; g2.c = x;
      g2.M = m; g2.N = kDim; g2.K = 2 * kDim; g2.ldr = kDim; g2.ldc = kDim;
      HIP_TRY(launch_gemm_split(g2, EPI_RESID, 0, s));
      if (ln_rows) HIP_TRY(launch_layernorm(x, kDim, ln_w, ln_b, (__bf16*)ln_rows, m, s, FMT_MIXED));
    }
  }
  HIP_TRY(timer.stop());
  if (ms_per_rep) *ms_per_rep = timer.total_ms / reps;
  return VETO_OK;
}

// Test / measurement hook of the attention out projection + residual (model_veto.py:96 `to_out`, :20) on VETO_MIXED operands:
// x <- x + a W^T + b for m token rows, optionally followed by LayerNorm rows (the FeedForward PreNorm, :125-132).  mode 0 = the GEMM
// launch with the residual epilogue (+ a LayerNorm launch), mode 1 = the full-row panel kernel (ffn_fused.hip, MODE 1).
size_t veto_debug_outproj_workspace_bytes(int32_t m) {
  return m > 0 ? carve_outproj(Carver{nullptr}, m).total : 0;
}

int veto_debug_outproj(void* stream, const float* a, const float* w, const float* b, float* x, int32_t m, int32_t mode, int32_t flags,
                       int32_t reps, float* ms_per_rep, void* workspace, size_t workspace_bytes, const float* ln_w, const float* ln_b,
                       void* ln_rows) {
  if (!a || !w || !b || !x || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (m <= 0 || reps <= 0 || (mode != 0 && mode != 1)) return fail(VETO_ERR_INVALID, "bad m / reps / mode");
  if (ln_rows && (!ln_w || !ln_b)) return fail(VETO_ERR_INVALID, "ln_rows needs ln_w and ln_b");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_outproj_workspace_bytes(m), false));
  hipStream_t s = (hipStream_t)stream;
  const auto [a_m, w_m, exps, ws_bytes] = carve_outproj(Carver{(char*)workspace}, m);
  if (flags & 1) HIP_TRY(launch_mixed_weight_rows(w, w_m, (size_t)kDim, kDim, exps, s));
  EventTimer timer;      // every rep by itself
  if (ms_per_rep) HIP_TRY(timer.init(s));
  for (int r = 0; r < reps; ++r) {
    // the fused form writes its LayerNorm rows over its input rows: rebuild them for every run (outside the timed span)
    HIP_TRY(hipMemsetAsync(a_m, 0, (char*)w_m - (char*)a_m, s));
    HIP_TRY(launch_mixed_act_rows(a, a_m, (size_t)m, kDim, s));
    HIP_TRY(timer.start());
    if (mode == 1) {
      HIP_TRY(launch_out_fused(out_panel_args(a_m, MixedLinear{w_m, b, exps}, x, m, ln_rows ? RowNorm{ln_w, ln_b, ln_rows} : RowNorm()), s));
    } else {
      GemmArgs g{};
      g.fmt = FMT_MIXED; g.w_exp = exps; g.a = a_m; g.w = w_m; g.bias = b; g.resid = x; g.c = x;
      g.M = m; g.N = kDim; g.K = kDim; g.ldr = kDim; g.ldc = kDim;
      HIP_TRY(launch_gemm_split(g, EPI_RESID, 0, s));
      if (ln_rows) HIP_TRY(launch_layernorm(x, kDim, ln_w, ln_b, (__bf16*)ln_rows, m, s, FMT_MIXED));
    }
    HIP_TRY(timer.stop());
  }
  if (ms_per_rep) *ms_per_rep = timer.total_ms / reps;
  return VETO_OK;
}

// Test / measurement hook of everything behind the attention of one layer (model_veto.py:96, :20-21, :125-143): x1 = x + a Wo^T +
// bo, h = LayerNorm2(x1), x2 = x1 + W2 gelu(W1 h + b1) + b2 (+ LayerNorm rows of x2) on VETO_MIXED operands.  mode 0 = the
// out-projection panel launch + the FeedForward panel launch, mode 1 = ONE launch (ffn_fused.hip MODE 2).
size_t veto_debug_layer_tail_workspace_bytes(int32_t m) {
  return m > 0 ? carve_layer_tail(Carver{nullptr}, m).total : 0;
}

int veto_debug_layer_tail(void* stream, const float* a, const float* wo, const float* bo, const float* ln2_w, const float* ln2_b,
                          const float* w1, const float* b1, const float* w2, const float* b2, float* x, int32_t m, int32_t mode,
                          int32_t reps, float* ms_per_rep, void* workspace, size_t workspace_bytes, const float* ln_w, const float* ln_b,
                          void* ln_rows) {
  if (!a || !wo || !bo || !ln2_w || !ln2_b || !w1 || !b1 || !w2 || !b2 || !x || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (m <= 0 || reps <= 0 || (mode != 0 && mode != 1)) return fail(VETO_ERR_INVALID, "bad m / reps / mode");
  if (ln_rows && (!ln_w || !ln_b)) return fail(VETO_ERR_INVALID, "ln_rows needs ln_w and ln_b");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_layer_tail_workspace_bytes(m), false));
  hipStream_t s = (hipStream_t)stream;
  const auto [a_m, wo_m, w1_m, w2_m, exps, ws_bytes] = carve_layer_tail(Carver{(char*)workspace}, m);
  HIP_TRY(launch_mixed_weight_rows(wo, wo_m, (size_t)kDim, kDim, exps + 0, s));
  HIP_TRY(launch_mixed_weight_rows(w1, w1_m, (size_t)2 * kDim, kDim, exps + 1, s));
  HIP_TRY(launch_mixed_weight_rows(w2, w2_m, (size_t)kDim, 2 * kDim, exps + 2, s));
  EventTimer timer;      // every rep by itself
  if (ms_per_rep) HIP_TRY(timer.init(s));
  for (int r = 0; r < reps; ++r) {
    HIP_TRY(hipMemsetAsync(a_m, 0, (char*)wo_m - (char*)a_m, s));       // the activation rows are overwritten in place: rebuilt per run, untimed
    HIP_TRY(launch_mixed_act_rows(a, a_m, (size_t)m, kDim, s));
    HIP_TRY(timer.start());
    // (every LayerNorm goes over the activation rows in place, as in the forward)
    const MixedLinear out{wo_m, bo, exps + 0}, fc1{w1_m, b1, exps + 1}, fc2{w2_m, b2, exps + 2};
    const RowNorm ln2{ln2_w, ln2_b, a_m};
    if (mode == 1) {
      HIP_TRY(launch_layer_tail(layer_tail_args(a_m, out, ln2, fc1, fc2, x, m, ln_rows ? RowNorm{ln_w, ln_b, nullptr} : RowNorm()), s));
    } else {
      HIP_TRY(launch_out_fused(out_panel_args(a_m, out, x, m, ln2), s));
      HIP_TRY(launch_ffn_fused(ffn_panel_args(a_m, fc1, fc2, x, m, ln_rows ? RowNorm{ln_w, ln_b, a_m} : RowNorm()), s));
    }
    HIP_TRY(timer.stop());
  }
  if (ln_rows) HIP_TRY(hipMemcpyAsync(ln_rows, a_m, (size_t)m * kDim * 4, hipMemcpyDeviceToDevice, s));
  if (ms_per_rep) *ms_per_rep = timer.total_ms / reps;
  return VETO_OK;
}

// Test / bench hook of the fused QKV + attention launch: a = LayerNorm1 rows fp32 [19 n_pair, 576], wqkv fp32 [1728, 576]; out_rows receives
// the attention output as mixed rows [19 n_pair, 4*576 B].  mode 1 = qkv_attn_fused.hip, mode 0 = the two launches it replaces (QKV GEMM
// with 3-byte q / k / v + attention_mfma_kernel).
size_t veto_debug_qkv_attn_workspace_bytes(int32_t n_pair) {
  return n_pair > 0 ? carve_qkv_attn(Carver{nullptr}, n_pair).total : 0;
}

int veto_debug_qkv_attn(void* stream, const float* a, const float* wqkv, int32_t n_pair, int32_t heads, int32_t mode, int32_t reps,
                        float* ms_per_rep, void* workspace, size_t workspace_bytes, void* out_rows) {
  if (!a || !wqkv || !workspace || !out_rows) return fail(VETO_ERR_INVALID, "null argument");
  if (n_pair <= 0 || reps <= 0 || (mode != 0 && mode != 1) || !qkv_attn_fused_supports(heads)) return fail(VETO_ERR_INVALID, "bad n_pair / reps / mode / heads");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_debug_qkv_attn_workspace_bytes(n_pair), false));
  hipStream_t s = (hipStream_t)stream;
  const size_t m = (size_t)n_pair * kTokens;
  const auto [a_m, o_m, qkv, w_m, exps, ws_bytes] = carve_qkv_attn(Carver{(char*)workspace}, n_pair);
  HIP_TRY(hipMemsetAsync(a_m, 0, o_m - (char*)a_m, s));      // (the rows m..padded stay zero)
  HIP_TRY(launch_mixed_act_rows(a, a_m, m, kDim, s));
  HIP_TRY(launch_mixed_weight_rows(wqkv, w_m, (size_t)3 * kDim, kDim, exps, s));
  EventTimer timer;      // the whole rep loop
  if (ms_per_rep) HIP_TRY(timer.init(s));
  HIP_TRY(timer.start());
  for (int r = 0; r < reps; ++r) {
    if (mode == 1) {
      QkvAttnArgs q{};
      q.a = (const char*)a_m; q.w = (const char*)w_m; q.w_exp = exps; q.o = o_m; q.n_pair = n_pair; q.heads = heads;
      HIP_TRY(launch_qkv_attn_fused(q, s));
    } else {
      GemmArgs g{};
      g.fmt = FMT_MIXED; g.w_exp = exps; g.a = a_m; g.w = w_m; g.c = (float*)qkv; g.M = (int)m; g.N = 3 * kDim; g.K = kDim; g.ldc = 3 * kDim;
      HIP_TRY(launch_gemm_split(g, EPI_F24, 0, s));
      AttnArgs t{};
      t.qkv = (const float*)qkv; t.o = (__bf16*)o_m; t.n_pair = n_pair; t.heads = heads; t.cls_only = 0; t.qkv_f24 = 1; t.o_fmt = FMT_MIXED;
      HIP_TRY(launch_attention(t, s));
    }
  }
  HIP_TRY(timer.stop());
  if (ms_per_rep) *ms_per_rep = timer.total_ms / reps;
  HIP_TRY(hipMemcpyAsync(out_rows, o_m, m * kDim * 4, hipMemcpyDeviceToDevice, s));
  return VETO_OK;
}

// ---- the backward blocks of the training step (backward.hip, train.hip), one by one -------------------------------------------
static int debug_wgrad(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k, int32_t k_splits,
                       void* workspace, size_t workspace_bytes, bool ordered) {
  if (!dy || !x || !dw || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  if (m <= 0 || n <= 0 || k <= 0 || k % 192 != 0) return fail(VETO_ERR_INVALID, "k must be a positive multiple of 192");
  const WgradWs ws = carve_wgrad(Carver{(char*)workspace}, m, n, k, k_splits, ordered);
  ABI_TRY(check_workspace(workspace, workspace_bytes, ws.total, false));
  hipStream_t s = (hipStream_t)stream;
  if (n % 32 == 0) {
    HIP_TRY(hipMemsetAsync(ws.a, 0, ws.operand_bytes, s));   // the row behind the last one is read (never used) by partial tiles
    HIP_TRY(launch_split_rows(dy, ws.a, (size_t)m, n, s));
    HIP_TRY(launch_split_rows(x, ws.w, (size_t)m, k, s));
  } else {
    HIP_TRY(hipMemsetAsync(ws.a, 0, (char*)ws.w - (char*)ws.a, s));   // rows n..padded stay zero
    HIP_TRY(launch_transpose_split(dy, n, m, n, ws.a, (int)ws.split.mp, s));
    HIP_TRY(launch_transpose_split(x, k, m, k, ws.w, (int)ws.split.mp, s));
  }
  const hipError_t e = launch_wgrad(nullptr, s, nullptr, ws.a, ws.w, ws.zero, m, n, k, ws.split, dw, ws.planes);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "wgrad gemm launch failed: %s", hipGetErrorString(e));
  return VETO_OK;
}

size_t veto_debug_wgrad_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t k_splits) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return carve_wgrad(Carver{nullptr}, m, n, k, k_splits, false).total;
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
  HIP_TRY(launch_layernorm_backward(x, dy, gamma, dres, dx, dgamma_dbeta, (float*)workspace, rows, (hipStream_t)stream, nullptr, nullptr, DropSite(), false));
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
                                    col_partials, DropSite{drop_seed, drop_thresh, drop_scale, 1}, false));
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
                                    col_partials, DropSite{drop_seed, drop_thresh, drop_scale, 1}, true));
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

// ---- the forward attention kernels (attention.hip) and qkv0_combine_kernel (rowops.hip), each alone on caller-given buffers --------
// Everything launch_attention / launch_cls_fold_attention answer with hipErrorInvalidValue is refused here first, with its reason.
int veto_debug_attention(void* stream, const void* qkv, void* o, int32_t n_pair, int32_t heads, int32_t cls_only, int32_t o_fmt,
                         int32_t qkv_f24, const float* sw, const float* ow, const float* stats, const float* vec, const int32_t* subj,
                         const int32_t* obj) {
  if (!qkv || !o) return fail(VETO_ERR_INVALID, "null argument");
  if (n_pair <= 0) return fail(VETO_ERR_INVALID, "n_pair must be positive");
  if ((cls_only != 0 && cls_only != 1) || (qkv_f24 != 0 && qkv_f24 != 1) || (o_fmt != FMT_SPLIT && o_fmt != FMT_MIXED))
    return fail(VETO_ERR_INVALID, "cls_only and qkv_f24 are 0 or 1, o_fmt is 0 (split rows) or 1 (mixed rows)");
  if (heads <= 0 || kDim % heads != 0) return fail(VETO_ERR_INVALID, "heads %d does not divide 576", heads);
  const int dh = kDim / heads;
  const bool mfma = dh == 72 || dh == 96;
  const bool any_tab = sw || ow || stats || vec || subj || obj, all_tab = sw && ow && stats && vec && subj && obj;
  if (any_tab && !all_tab) return fail(VETO_ERR_INVALID, "the table operands sw, ow, stats, vec, subj, obj go together");
  if (any_tab && cls_only) return fail(VETO_ERR_INVALID, "the per-object form has no cls_only instance");
  if (any_tab && qkv_f24) return fail(VETO_ERR_INVALID, "the per-object form reads fp32 rows for tokens 17 / 18");
  if (!mfma) {
    if (any_tab || qkv_f24) return fail(VETO_ERR_INVALID, "tables and 3-byte q / k / v need a head width of 72 or 96 (heads %d: %d)", heads, dh);
    if (o_fmt != FMT_SPLIT) return fail(VETO_ERR_INVALID, "the generic kernel (head width %d) writes split rows only", dh);
    if (dh % 4 != 0) return fail(VETO_ERR_INVALID, "head width %d is no multiple of 4", dh);
    if (attention_generic_lds_bytes(dh) > kAttentionGenericLdsMax)
      return fail(VETO_ERR_INVALID, "head width %d needs %zu bytes of LDS (limit %zu)", dh, attention_generic_lds_bytes(dh), kAttentionGenericLdsMax);
  }
  AttnArgs a{};
  a.qkv = (const float*)qkv; a.o = (__bf16*)o; a.n_pair = n_pair; a.heads = heads; a.cls_only = cls_only; a.qkv_f24 = qkv_f24; a.o_fmt = o_fmt;
  a.sw = sw; a.ow = ow; a.stats = stats; a.vec = vec; a.subj = subj; a.obj = obj;
  const hipError_t e = launch_attention(a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "attention launch: %s", hipGetErrorString(e));
  return VETO_OK;
}

int veto_debug_cls_fold_attention(void* stream, const float* x, const float* ln_w, const float* ln_b, const void* u, void* abar,
                                  int32_t n_pair, int32_t heads, int32_t u_f24) {
  if (!x || !ln_w || !ln_b || !u || !abar) return fail(VETO_ERR_INVALID, "null argument");
  if (n_pair <= 0) return fail(VETO_ERR_INVALID, "n_pair must be positive");
  if (u_f24 != 0 && u_f24 != 1) return fail(VETO_ERR_INVALID, "u_f24 is 0 or 1");
  if (heads <= 0 || kDim % heads != 0) return fail(VETO_ERR_INVALID, "heads %d does not divide 576", heads);
  if (heads > cls_fold_max_heads()) return fail(VETO_ERR_INVALID, "the folded kernels take at most %d heads", cls_fold_max_heads());
  if (u_f24 && cls_fold_on_vector_alu()) return fail(VETO_ERR_INVALID, "the vector-ALU folded kernel (VETO_CLS_MFMA=0) reads u as fp32 only");
  const hipError_t e = launch_cls_fold_attention(x, ln_w, ln_b, (const float*)u, (__bf16*)abar, n_pair, heads, (hipStream_t)stream, u_f24 != 0);
  if (e != hipSuccess) return fail(e == hipErrorInvalidValue ? VETO_ERR_INVALID : VETO_ERR_HIP, "folded attention launch: %s", hipGetErrorString(e));
  return VETO_OK;
}

int veto_debug_qkv0_combine(void* stream, const float* sw, const float* ow, const float* stats, const float* vec, const int32_t* subj,
                            const int32_t* obj, float* qkv, int32_t n_pair) {
  if (!sw || !ow || !stats || !vec || !subj || !obj || !qkv) return fail(VETO_ERR_INVALID, "null argument");
  if (n_pair <= 0) return fail(VETO_ERR_INVALID, "n_pair must be positive");
  HIP_TRY(launch_qkv0_combine(sw, ow, stats, vec, subj, obj, qkv, n_pair, (hipStream_t)stream));
  return VETO_OK;
}

}  // extern "C"
