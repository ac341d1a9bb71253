// Internal launch interface between the C-ABI host code (abi_*.hip) and the kernels.
#pragma once
#include "common.h"

namespace veto {

enum Epi { EPI_F32 = 0, EPI_RESID = 1, EPI_GELU_SPLIT = 2, EPI_ATOMIC = 3, EPI_RESID_DROP = 4, EPI_F24 = 5, EPI_SPLIT = 6, EPI_PRE_GELU = 7, EPI_GELU_BWD = 8, EPI_PLANES = 9 };   // EPI_F24: EPI_F32 written as 3-byte floats (common.h); EPI_SPLIT: split rows, no activation; EPI_PRE_GELU (training, split rows): the fp32 pre-activation to c (row stride ldc_f32) AND exact-erf gelu of it as split rows to c_split

// C[M,N] = A[M,K] . W[N,K]^T with A and W in the split-row format (common.h): rows of 2K bf16.
struct GemmArgs {
  const __bf16* a;     // row r at a + r*lda; rows padded to a multiple of 256 when lda == 2K
  const __bf16* w;     // [N, 2K]
  const float* bias;   // [N] or nullptr
  const float* resid;  // EPI_RESID: row r at resid + r*ldr
  float* c;            // EPI_F32 / EPI_RESID: row r at c + r*ldc; EPI_F24: row r at (char*)c + 3*r*ldc, 3 bytes per element
  __bf16* c_split;     // EPI_GELU_SPLIT / EPI_SPLIT: split-row output, row r at c_split + r*ldc (ldc = 2N)
  int M, N, K;
  long lda;            // A row stride in bf16 elements (0 = 2K)
  long ldr;
  long ldc;
  long ldc_f32;        // EPI_PRE_GELU: row stride of c in floats (ldc is c_split's)
  // EPI_GELU_BWD (training, split rows): the input gradient of fc2 times gelu'(pre) -- resid = the fp32 pre-activation (row stride ldr) --
  // written straight as the split rows of fc1's backward (c_split, ldc), with the column sums of every 64-row slice of a tile (the rows of
  // one wave row) to col_partial[(tile_m * 4 + wave row) * N + column]: the bias gradient's partials, folded by launch_column_sums
  float* col_partial;
  int k_splits;          // EPI_ATOMIC: the reduction K is cut into this many equal ranges (K/32 % k_splits == 0), each a
                         // tile of its own that ADDS into c with fp32 atomics (c zero-initialised); 0/1 = one range
                         // EPI_PLANES (the ordered weight gradient): the same ranges, but range j WRITES its tile with plain stores to
                         // plane j = c + j * M * ldc; every element of all k_splits planes is written; launch_fold_rows adds them in order
  // EPI_RESID_DROP (training only): EPI_RESID with dropout on (A.W^T + bias) before the residual is added; element (row, col) uses index
  // (row * drop_row_step) * N + col of site drop_seed.  drop_thresh = p * 2^24 (0 = off), drop_scale = 1 / (1 - p); drop_row_step: 1, or 19
  // where the rows are the compact CLS rows of the last layer (row p = token row 19 p: the numbering of include/veto_amd.h)
  unsigned long long drop_seed;
  unsigned drop_thresh;
  float drop_scale;
  int drop_row_step;
  int tiles_m, tiles_n;  // filled by the launcher
  // tn (EPI_ATOMIC / EPI_PLANES only, weight gradients): C[M, N] += A^T B with BOTH operands row-major in the reduction index, i.e. the
  // split rows the backward already holds: a = dY split rows [k_valid, lda] (M = its column count), w = X split rows
  // [k_valid, ldw] (N = its column count), K = the reduction length rounded up to 32 * k_splits.  Reduction rows >= k_valid
  // are read from `zero` (>= 1 KiB of zeros).  The operands are transposed on their way out of LDS (ds_read_b64_tr_b16).
  // fmt == FMT_MIXED (common.h): a and w are mixed rows (fp16 + e4m3), w_exp points to the weight tensor's e4m3 exponent
  // on the device, and an EPI_GELU_SPLIT output is written as mixed rows too.  Inference forms only (no tn / split-K).
  int fmt;
  // Block-diagonal weights (kb_tiles > 0; split rows, no split-K, not tn): column tile n multiplies only the k-steps
  // [(n / kb_tiles) * kb_steps, + kb_steps) of the rows -- the products of the folded last layer (abi_core.hip) are block-diagonal
  // over the heads, and the zero blocks are skipped instead of multiplied.
  int kb_tiles, kb_steps;
  const int* w_exp;
  int tn;
  long ldw;
  int k_valid;
  const __bf16* zero;
};

// Environment knobs (abi_core.hip): every one selects a path that a parity test compares against the default (INTEGRATION.md
// lists them); call sites cache the answer in a function-local static.
bool env_knob_is(const char* name, const char* value);   // the variable is set to exactly `value`
int env_knob_int(const char* name, int dflt);
int gemm_rows_padded(int m);
// compute units of the CURRENT device (hipGetDevice), cached per device ordinal: the persistent kernels size their grids with it
// (a process-wide cache of the first device's count would be wrong on a node with unlike devices); <= 0 on error
int device_cu_count();
// precision: 0 = three split-bf16 terms, 1 = one; g.fmt == FMT_MIXED selects the fp16 + e4m3 kernel regardless
hipError_t launch_gemm_split(GemmArgs g, int epi, int precision, hipStream_t s);
hipError_t launch_gemm_split_ps(GemmArgs g, int epi, int precision, hipStream_t s);

// Fused FeedForward (ffn_fused.hip), VETO_MIXED operands: out = resid + W2 . gelu(W1 . a + b1) + b2 on `M` token rows.
// a: mixed activation rows [rows padded to ffn_panel_rows(), 4*576 B]; w1 [1152, 4*576 B], w2 [576, 4*1152 B]: mixed weight
// rows with their e4m3 exponents exp1 / exp2 (device ints); resid / out fp32 rows (may alias).
struct FfnArgs {
  const char* a;
  const char* w1;
  const char* w2;
  const float* b1;
  const float* b2;
  const float* resid;
  float* out;
  long ldr, ldo;         // row strides of resid / out in floats
  int M;
  const int* exp1;
  const int* exp2;
  // optional: LayerNorm (eps 1e-5) of the result rows with ln_w / ln_b, written as mixed activation rows to ln_out (row pitch
  // 4*576 B; may be the buffer `a` points to: a panel's rows are written after its last read) -- the next layer's PreNorm
  const float* ln_w;
  const float* ln_b;
  char* ln_out;
  char* ln1_out;         // launch_layer_tail only, optional: where the final LayerNorm rows (ln_w / ln_b) go instead of ln_out -- with the
                         // fused QKV + attention launch the attention output (a) and the next layer's LayerNorm1 rows live in different buffers
  // launch_layer_tail only: the attention out projection in front of the FeedForward -- x1 = resid + a . wo^T + bo stays in
  // registers, lnm_w / lnm_b (LayerNorm2) turn it into the FeedForward's input rows, written to ln_out (= a, in place)
  const char* wo;        // [576, 4*576 B] mixed weight rows, exponent expo
  const float* bo;
  const int* expo;
  const float* lnm_w;
  const float* lnm_b;
  // launch_layer_tail only: resid / out are rows of 576 3-byte floats (common.h, pack_f24x4; ldr / ldo unused) instead of fp32 rows.  out_f24
  // needs resid_f24; with different formats the two must be different buffers
  int resid_f24, out_f24;
  int fast;              // launch_layer_tail only (VETO_FAST): the fp16 main product alone -- the correction stages are neither loaded nor multiplied
  int n_panels;          // filled by the launcher
  int late;              // filled by the launcher (speed only): start delay (~us) of the workgroups that have one panel fewer than the others
};
int ffn_panel_rows();
hipError_t launch_ffn_fused(FfnArgs g, hipStream_t s);
// the same skeleton as ONE GEMM: out = resid + a . w2^T + b2 (K = 576: the attention out projection + residual), optional LayerNorm rows
hipError_t launch_out_fused(FfnArgs g, hipStream_t s);
// out projection + residual + LayerNorm2 + FeedForward + residual (+ the next layer's LayerNorm1) in ONE launch: everything of a
// transformer layer behind its attention (model_veto.py:96, :20-21, :125-143).  a = attention output rows (mixed), resid = x in,
// out = x out, ln_out = a (the LayerNorm2 rows, then the next layer's LayerNorm1 rows, in place); wo / bo / expo / lnm_* as above
hipError_t launch_layer_tail(FfnArgs g, hipStream_t s);

// ---- weight preparation (once per weight upload) ---------------------------------------------
// src [rows, K] fp32 -> dst [rows, 2K] split rows
hipError_t launch_split_rows(const float* src, __bf16* dst, size_t rows, int K, hipStream_t s);
// block-form weights of the folded last layer (rowops.hip), fp32: which = 0 Wq padded, 1 Wk^T block-diagonal, 2 Wv block-diagonal, 3 Wo padded
hipError_t launch_fold_blocks(const float* qkv, const float* wo, float* out, int which, int heads, int dhp, hipStream_t s);
// src [rows, K] fp32 -> dst [rows, 4K bytes] mixed WEIGHT rows (common.h); *exp_out (device) receives the tensor's e4m3 exponent e:
// the largest e in [0, 24] with 2^e max|w| <= 448
hipError_t launch_mixed_act_rows(const float* src, __bf16* dst, size_t rows, int K, hipStream_t s);
hipError_t launch_mixed_weight_rows(const float* src, __bf16* dst, size_t rows, int K, int* exp_out, hipStream_t s);
// src [M, ld] fp32 (N columns used) -> dst [N, 2*Mp] split rows of the TRANSPOSE, Mp = M rounded up to 32*mult
// (zero padded): the operand layout of a GEMM that reduces over M (weight gradients)
hipError_t launch_transpose_split(const float* src, long ld, int M, int N, __bf16* dst, int Mp, hipStream_t s);
// PATCH_SIZE p in 1..4 on maps of 4p x 4p (always a 4 x 4 patch grid: 16 patch tokens).  The patch features of one object row,
// K of the patch projection: [depth 256 p^2 | rgb 256 p^2], 512 / 2048 / 4608 / 8192; and that count as GEMM output columns
// (a multiple of the 192-column tile): 576 / 2112 / 4608 / 8256
constexpr int patch_feats(int p) { return 512 * p * p; }
constexpr int patch_t_rows(int p) { return (patch_feats(p) + 191) / 192 * 192; }
// W_cat [1152, 2*K] split rows + bias_cat [1152] from proj_d [512, K], proj_v [64, K], K = patch_feats(p)
hipError_t launch_build_patch_weight(const float* wd, const float* bd, const float* wv, const float* bv,
                                     __bf16* dst, float* bias_cat, int p, hipStream_t s);
// dst[k][half*576 + j] = src[j][half*kin + k]   (src is [576, 2*kin])
hipError_t launch_transpose_pair_proj(const float* src, float* dst, int kin, hipStream_t s);
// dst[k][c] = src[c][k]  (src [n_out, 576])
hipError_t launch_transpose_head(const float* src, float* dst, int n_out, hipStream_t s);

// ---- per-object stage --------------------------------------------------------------------------
struct ObjPrepArgs {
  const float* boxes;        // [n_obj, 4]
  int box_mode;              // 0 xyxy, 1 xywh
  const int64_t* labels;     // predcls / MEET: embedding lookup
  const float* obj_logits;   // sgcls: softmax(logits) @ E
  const float* embed;        // [num_obj_cls, embed_dim]
  int num_obj_cls, embed_dim;
  const float* bn_w; const float* bn_b; const float* bn_mean; const float* bn_var;  // [4]
  const float* pos_w; const float* pos_b;   // [128,4], [128]
  const float* loc_wt; const float* loc_b;  // [128][1152] transposed, [576]
  const float* cls_wt; const float* cls_b;  // [embed_dim][1152] transposed, [576]
  float* lc;                 // out [n_obj, 2, 1152]: (location | class) x (subj(+bias) | obj)
  float* pos_out;            // optional debug [n_obj,128]
  int n_obj;
  // training only: Dropout(0.1) behind the position embedding's ReLU; element (n, k) -> index n*128 + k
  unsigned long long drop_seed;
  unsigned drop_thresh;
  float drop_scale;
};
hipError_t launch_obj_prep(const ObjPrepArgs& a, hipStream_t s);
// training-mode BatchNorm1d(4) statistics of the box features center_xywh(boxes): out[0..3] mean, [4..7] biased
// variance (what the batch is normalised with), [8..11] unbiased variance (what running_var is updated with)
hipError_t launch_bn_batch_stats(const float* boxes, int box_mode, int n_obj, float* out, hipStream_t s);
// rgb/depth [n_obj, 256, 4p, 4p] -> patch rows [n_obj*16, 2*patch_feats(p)] split rows (depth features first)
hipError_t launch_patchify(const float* depth, const float* rgb, __bf16* dst, int n_obj, int p, hipStream_t s);

// ---- pair stage --------------------------------------------------------------------------------
hipError_t launch_pair_indices(const int64_t* rel_pairs, const int32_t* img_obj_off,
                               const int32_t* img_pair_off, int n_img, int n_pair, int32_t* subj,
                               int32_t* obj, int64_t* subj64, int64_t* obj64, hipStream_t s);
hipError_t launch_enumerate_pairs(int n, int64_t* out, hipStream_t s);

struct AssembleArgs {
  const float* patch_tab;   // [n_obj*16, 1152]
  const float* lc;          // [n_obj, 2, 1152]
  const float* cls_token;   // [576]
  const float* pos_embedding;  // [576]
  const float* ln_w; const float* ln_b;  // layer-0 attention PreNorm
  const int32_t* subj; const int32_t* obj;  // this chunk's pairs
  float* x;                 // [n_pair*19, 576]
  __bf16* a;                // LN(x), split rows [n_pair*19, 2*576]
  float* stats;             // optional [n_pair*19, 2]: (mean, rstd) of every row; then `a` is written for tokens 17 / 18 only
  int a_fmt;                // ... in this operand format (FMT_SPLIT / FMT_MIXED; with stats only)
  int x_f24;                // (with stats only) x is written as rows of 576 3-byte floats (common.h) instead of fp32
  int n_pair;
  // training only: pos_drop (EMB_DROPOUT) on the assembled tokens; element (row, col) -> index row*576 + col
  unsigned long long drop_seed;
  unsigned drop_thresh;
  float drop_scale;
};
hipError_t launch_assemble(const AssembleArgs& a, hipStream_t s);
// layer 0 in the per-object form (rowops.hip): qkv rows of tokens 0..16 from the per-object tables sw / ow [n_obj*16, 1728],
// the row statistics and the weight-only vectors vec = [c2 | b0 | qkv_cls]; the kernel that builds vec and Wqkv diag(gamma);
// and the row-centred split rows of the two halves of patch_tab [rows, 1152] -> [rows, 2*1152]
hipError_t launch_centre_split(const float* patch_tab, __bf16* dst, int rows, hipStream_t s);
hipError_t launch_qkv0_combine(const float* sw, const float* ow, const float* stats, const float* vec, const int32_t* subj,
                               const int32_t* obj, float* qkv, int n_pair, hipStream_t s);
hipError_t launch_qkv0_consts(const float* wq, const float* gamma, const float* beta, const float* pos, const float* cls, float* wp,
                              float* vec, hipStream_t s);

// LayerNorm(eps 1e-5) of `rows` rows (row r at x + r*ldx) -> split rows [rows, 2*576]
// dst row r at dst + r*ldd (bf16 elements; 0 = contiguous rows of 2*576)
// counters[4] += {elements, fp16 values at +-65504, e4m3 value-plane bytes at +-448, e4m3 residual-plane bytes at +-448} of mixed rows
hipError_t launch_count_saturation(const void* base, long stride_bytes, int rows, int K, unsigned long long* counters, hipStream_t s);
// x_f24: the source rows are 3-byte floats (common.h); ldx still counts elements
hipError_t launch_layernorm(const float* x, long ldx, const float* w, const float* b, __bf16* dst, int rows,
                            hipStream_t s, int fmt = FMT_SPLIT, long ldd = 0, bool x_f24 = false);
// n 3-byte floats (n % 4 == 0) -> fp32
hipError_t launch_unpack_f24(const void* src, float* dst, size_t n, hipStream_t s);

struct AttnArgs {
  const float* qkv;        // [n_pair*19, 1728]; qkv_f24: the same matrix as 3-byte floats (rows of 5184 bytes)
  __bf16* o;               // split rows [rows, 2*576]; rows = n_pair*19, or n_pair when cls_only
  int n_pair, heads, cls_only;
  int qkv_f24 = 0;         // MFMA head widths, not the per-object form
  int o_fmt = FMT_SPLIT;   // operand format of o (MFMA head widths; the generic kernel writes split rows only)
  // layer 0, per-object form (rowops.hip): when sw != nullptr the rows of tokens 1..16 are formed on load as
  // rstd * (sw[subj*16 + t-1] + ow[obj*16 + t-1]) + c2, token 0 is the constant row vec + 2*1728, and only the rows of tokens
  // 17 / 18 are read from qkv.  MFMA head widths (72, 96) only: launch_attention returns hipErrorInvalidValue otherwise.
  const float* sw = nullptr;
  const float* ow = nullptr;
  const float* stats = nullptr;   // [n_pair*19, 2]: (mean, rstd)
  const float* vec = nullptr;     // [c2 | b0 | qkv_cls], each [1728]
  const int32_t* subj = nullptr;
  const int32_t* obj = nullptr;
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);
bool attention_reads_tables(int heads);   // whether launch_attention takes the per-object form for this head count
// the generic (vector-ALU) kernel's dynamic LDS at head width dh, and the most launch_attention accepts
constexpr size_t kAttentionGenericLdsMax = 160 * 1024;
size_t attention_generic_lds_bytes(int dh);

// QKV projection + attention of a middle layer in one launch (qkv_attn_fused.hip; VETO_MIXED, head widths 72 / 96): a = LayerNorm1 rows
// (mixed, [rows padded to qkv_attn_rows_padded(n_pair), 4*576 B]), w = Wqkv as mixed weight rows [1728, 4*576 B] with its e4m3 exponent
// w_exp (device int), o = attention output rows (mixed, row = 19 * pair + token; NOT the buffer a points to: every head's tile reads all
// of a pair group's rows)
struct QkvAttnArgs {
  const char* a;
  const char* w;
  const int* w_exp;
  char* o;
  int n_pair, heads;
  int fast;      // VETO_FAST: the fp16 main product alone (the correction stages are neither loaded nor multiplied)
};
bool qkv_attn_fused_supports(int heads);
size_t qkv_attn_rows_padded(int n_pair);
hipError_t launch_qkv_attn_fused(const QkvAttnArgs& g, hipStream_t s);
// Folded CLS-only attention of the last layer: x = residual stream [n_pair*19, 576] (LayerNorm1 with ln_w / ln_b is applied
// inside), u fp32 [n_pair, heads*576] (= LN1(x_0) . Mcat), abar split rows [n_pair, 2*heads*576] (probability-weighted
// token means per head)
int cls_fold_max_heads();
hipError_t launch_cls_fold_attention(const float* x, const float* ln_w, const float* ln_b, const float* u, __bf16* abar, int n_pair, int heads,
                                     hipStream_t s, bool u_f24 = false);
bool cls_fold_on_vector_alu();   // VETO_CLS_MFMA=0 (read once per process): the fp32 vector-ALU kernel, which takes u as fp32 only
bool cls_fold_reads_f24();   // whether the kernel takes u as 3-byte floats (the MFMA form; VETO_QKV_F24=0 / VETO_CLS_MFMA=0: fp32)

// cls row p at cls + p*ld (ld = 576 for compact CLS rows, 19*576 to read row 0 of every pair of a token matrix)
hipError_t launch_head(const float* cls, const float* wt, const float* bias, float* out, int n_pair,
                       int n_out, hipStream_t s, long ld = kDim);

// ---- post-processing (inference.py:398-453, GT-box branch; the MEET merge :284-397 and the expert vote :93-283) ----------------
// `rows` below: n_pair for the vanilla branch, n_groups * n_pair for the merge and the vote
struct PostArgs {
  const float* rel_logits;       // vanilla: [n_pair, n_rel_cls]
  const float* obj_logits;       // [n_obj, n_obj_cls]; nullptr (sgdet): obj_scores / obj_pred are inputs
  const int64_t* rel_pairs;      // [n_pair, 2] image-local
  const int32_t* img_obj_off;    // [n_img + 1]; both offset arrays nullptr: ONE image that owns every pair and object
  const int32_t* img_pair_off;   // [n_img + 1]
  int n_img, n_obj, n_pair, n_rel_cls, n_obj_cls;
  float* obj_scores;             // out [n_obj]
  int64_t* obj_pred;             // out [n_obj]
  float* out_prob;               // out [rows, n_rel_cls], sorted
  int64_t* out_pairs;            // out [rows, 2], sorted
  int64_t* out_labels;           // out [rows], sorted
  float* out_triple;             // optional out [rows], sorted
  float* prob_tmp;               // workspace [rows, n_rel_cls]
  float* triple;                 // workspace [rows]
  int32_t* label_tmp;            // workspace [rows]
  int32_t* perm;                 // workspace [rows]
  int32_t* kept_count;           // optional out [n_img]: rows of each image's sorted block with score >= 0 (expert voting)
};
constexpr int kPostMaxGroups = 16;
constexpr int kPostMaxRelCls = 256;
struct PostGroupTables {         // passed by value: the heads and the class -> group list; a wave derives its group's columns
  const float* logits[3 * kPostMaxGroups];   // [experts * k + e]: [n_pair, width[k]]
  int width[kPostMaxGroups];     // g_k + 2
  uint8_t cls_group[kPostMaxRelCls];         // 1-based group of class c, 0 = background (255: no group)
  int n_groups, experts;         // experts: 1 (merge) or 3 (vote)
  int voting;                    // vote: 0 = consensus ('C', two of three experts agree), 1 = unanimous ('U')
};
int postprocess_max_pairs_per_image();
// Four launches (object scores, row scores, one sort workgroup per image, gather) whatever n_img and n_groups.  t == nullptr: the
// vanilla branch on a.rel_logits.  Else the MEET merge / expert vote of t's heads: image i owns rows n_groups * img_pair_off[i] .. of
// n_groups * P_i rows, ordered (group, pair) before the sort.
hipError_t launch_postprocess(const PostArgs& a, const PostGroupTables* t, hipStream_t s);

// ---- sgdet: object decoding and test pairs on detected boxes (sgdet.hip) ----------------------------
struct ObjDecodeArgs {
  const float* logits;           // [n_obj, n_cls] (mode 0; and for obj_scores)
  const int64_t* labels;         // [n_obj] (mode 1: the one-hot's labels)
  const float* boxes_per_cls;    // [n_obj, n_cls, 4] xyxy
  const int32_t* img_off;        // [n_img + 1]
  int n_img, n_cls;
  int mode;                      // 0: obj_prediction_nms (PostProcessor), 1: Ensemble.nms_per_cls (MEET decoder)
  float thr;
  float* prob_ws;                // [n_obj, n_cls]: the probability matrix of images that exceed the LDS tile
  int64_t* obj_pred;             // out [n_obj]
  float* obj_scores;             // optional out [n_obj]
  float* out_boxes;              // optional out [n_obj, 4]
};
int obj_decode_max_objects();
hipError_t launch_obj_decode(const ObjDecodeArgs& a, hipStream_t s);
struct PairArgs {
  const float* boxes;            // [n_obj, 4] xyxy
  const float* scores;           // [n_obj] pred_scores
  const int32_t* img_off;        // [n_img + 1]
  const int32_t* out_off;        // [n_img + 1]: image i writes from row out_off[i]
  int n_img, max_pairs, require_overlap;
  int64_t* pairs;                // out [out_off[n_img], 2]
  int32_t* counts;               // out [n_img]
};
int prepare_pairs_max_pairs();
hipError_t launch_prepare_pairs(const PairArgs& a, hipStream_t s);

// ---- sgdet box decoder: segmented greedy NMS and the box head's PostProcessor (nms.hip) -----------------
struct NmsArgs {
  const float* boxes;            // [n_box, 4] xyxy, 16-byte aligned
  const float* scores;           // [n_box]
  const int32_t* seg_off;        // [n_seg + 1]
  int n_seg, max_keep;           // max_keep <= 0: no cap
  float thr;
  int64_t* keep;                 // out [n_box]: segment s writes counts[s] local indices from seg_off[s]
  int32_t* counts;               // out [n_seg]
};
int nms_max_segment();
hipError_t launch_nms(const NmsArgs& a, int max_seg, hipStream_t s);
struct BoxPostArgs {
  const float* logits;           // [n_box, n_cls]
  const float* regression;       // [n_box, reg_cols]
  const float* proposals;        // [n_box, 4] xyxy
  const float* image_sizes;      // [n_img, 2] (width, height)
  const int32_t* img_off;        // [n_img + 1]
  const int32_t* out_off;        // [n_img + 1]: image i writes its detections from row out_off[i]
  int n_img, n_box, n_cls, reg_cols, cls_agnostic, topn, filter_dup, det_per_img;
  float score_thresh, nms_thresh, wx, wy, ww, wh, xform_clip;
  float* prob;                   // workspace [n_box, n_cls]: softmax, then dist_scores
  float* dec;                    // workspace [n_box, n_cls, 4]: decoded, clipped boxes
  float* row_score;              // workspace [n_box] (filter_dup)
  int32_t* row_label;            // workspace [n_box] (filter_dup)
  float* list_score;             // workspace: the detection list before the cut, [n_box] or [n_box * (n_cls - 1)]
  int32_t* list_row;
  int32_t* list_label;
  int64_t* orig_inds;            // out [out_off[n_img]]
  int64_t* labels;               // out
  float* scores;                 // out
  float* boxes;                  // out [.., 4]
  float* boxes_per_cls;          // optional out [.., n_cls, 4]
  int32_t* counts;               // out [n_img]; -count when an image's rows do not hold its detections
};
hipError_t launch_box_postprocess(const BoxPostArgs& a, int max_per_img, hipStream_t s);
// The same NMS for fixed-capacity segments: segment s owns rows s * capacity .. + capacity, of which the first live[s]
// (device memory, clamped to the capacity) count.  The instantiation is picked from the capacity.
struct NmsFixedArgs {
  const float* boxes;            // [n_seg * capacity, 4] xyxy, 16-byte aligned
  const float* scores;           // [n_seg * capacity]
  const int32_t* live;           // [n_seg]
  int n_seg, capacity, max_keep;
  float thr;
  int32_t* keep;                 // out [n_seg * capacity]: segment s writes counts[s] local indices from s * capacity
  int32_t* counts;               // out [n_seg]
};
hipError_t launch_nms_fixed(const NmsFixedArgs& a, hipStream_t s);

// ---- RPN proposal selection: top-k, decode, clip, small boxes, NMS, merge over the levels (rpn.hip) -----------------
constexpr int kRpnMaxLevels = 8;
constexpr int kRpnSortCap = 8192;   // 64-bit keys one workgroup sorts in LDS
struct RpnLevel {
  const float* objectness;       // [n_img, A, H, W]
  const float* regression;       // [n_img, 4A, H, W]
  const float* anchors;          // [A * H * W, 4] xyxy, anchor (h * W + w) * A + a
  int A, HW, N, k;               // N = A * HW, k = min(pre_nms_top_n, N)
};
struct RpnArgs {
  RpnLevel lvl[kRpnMaxLevels];   // the per-level descriptor table: every kernel serves all levels from one grid
  const float* image_sizes;      // [n_img, 2] (width, height)
  const int32_t* out_off;        // [n_img + 1]
  int n_img, n_lvl, capacity;    // capacity = max k over the levels: rows of a segment (image x level) in the workspace
  int post_top_n, fpn_top_n, per_batch, nms_on;
  float nms_thresh, min_size, wx, wy, ww, wh, xform_clip;
  float* cand_box;               // workspace [n_seg * capacity, 4]: decoded, clipped, filtered candidates, best first
  float* cand_logit;             // workspace [n_seg * capacity]
  int32_t* cand_anchor;          // workspace [n_seg * capacity]
  int32_t* live;                 // workspace [n_seg]: candidates behind the small-box filter
  int32_t* keep;                 // workspace [n_seg * capacity]: NMS survivors (candidate rows), ascending
  int32_t* kept;                 // workspace [n_seg]
  int32_t* cut;                  // workspace [4 + n_img] (per-batch mode): cut on, key, need, -, equal keys in earlier images
  float* boxes;                  // out [.., 4]
  float* objectness;             // out
  int32_t* level;                // out
  int64_t* anchor_index;         // out
  int32_t* counts;               // out [n_img]
};
int rpn_batch_cut_max_images();
hipError_t launch_rpn_proposals(const RpnArgs& a, hipStream_t s);

// ---- the RPN's anchor generator: the grid of every level and the per-image visibility plane (rpn.hip) ----------------
struct AnchorLevel {
  const float* cell;             // [A, 4] xyxy, 16-byte aligned
  int A, W, stride;
  int row0;                      // first row of the level in the concatenated buffer
};
struct AnchorArgs {
  AnchorLevel lvl[kRpnMaxLevels];
  int n_lvl, total;              // total = sum of A H W
  float* anchors;                // out [total, 4], or null: the rows are read from anchors_in
  const float* anchors_in;       // [total, 4]
  const float* image_sizes;      // [n_img, 2] (width, height); not read when straddle < 0
  int n_img;
  float straddle;
  uint8_t* visibility;           // out [n_img, total], or null
};
hipError_t launch_anchor_grid(const AnchorArgs& a, hipStream_t s);

// ---- sgdet training: detected-box relation sampling (relsample.hip) ---------------------------------
struct RelSampleArgs {
  const float* prp_boxes;        // [n_prp, 4] xyxy
  const int64_t* prp_labels;     // [n_prp]
  const float* prp_scores;       // [n_prp] pred_scores
  const float* tgt_boxes;        // [n_tgt, 4] xyxy
  const int64_t* tgt_labels;     // [n_tgt]
  const int64_t* relation;       // image i: [T_i, T_i] row-major from rel_off[i]
  const int64_t* relation_nm;    // optional, same layout ('relation_non_masked')
  const int32_t* prp_off;        // [n_img + 1]
  const int32_t* tgt_off;        // [n_img + 1]
  const int32_t* rel_off;        // [n_img + 1]: prefix sums of T_i^2
  const int32_t* bin_off;        // [n_img + 1]: prefix sums of P_i^2
  int n_img, require_overlap, per_rel, max_fg, batch, out_rows;
  float fg_thres;
  uint64_t seed;
  int64_t* ws_nm;                // [rel_off[n_img]]: labels of relation_nm's nonzeros in row-major order
  uint32_t* ws_fg;               // [rel_off[n_img] * per_rel]: foreground triplets before the cap
  int64_t* pairs;                // out [n_img * out_rows, 2]
  int64_t* labels;               // out [n_img * out_rows]
  int64_t* labels_all;           // optional out: image i from rel_off[i] * per_rel + i * out_rows
  int64_t* binary;               // out: image i [P_i, P_i] from bin_off[i]
  float* locating;               // out [n_prp]
  int32_t* counts;               // out [n_img, 4]: rows, foreground before the cap, foreground kept, status
};
int relsample_max_objects();
int relsample_max_batch();
int relsample_max_per_rel();
hipError_t launch_detect_relsample(const RelSampleArgs& a, hipStream_t s);

// ---- predcls / sgcls training: GT-box relation sampling (gtbox_relsample.hip) -------------------------
struct GtboxRelSampleArgs {
  const int64_t* relation;       // image i: [n_i, n_i] row-major from rel_off[i]
  const int32_t* obj_off;        // [n_img + 1]: prefix sums of n_i
  const int32_t* rel_off;        // [n_img + 1]: prefix sums of n_i^2
  int n_img, batch, num_pos;
  uint64_t seed;
  int64_t* pairs;                // out [n_img * batch, 2]
  int64_t* labels;               // out [n_img * batch]
  int64_t* binary;               // out: image i [n_i, n_i] from rel_off[i]
  int32_t* counts;               // out [n_img, 2]: foreground rows, background rows
};
int gtbox_relsample_max_objects();
int gtbox_relsample_max_batch();
hipError_t launch_gtbox_relsample(const GtboxRelSampleArgs& a, hipStream_t s);

// ---- sgdet training: the box head's proposal matching and fg/bg sampling (boxsample.hip) ---------------
struct BoxMatchArgs {
  const float* prp_boxes;        // [n_prp, 4] xyxy, 16-byte aligned
  const float* tgt_boxes;        // [n_tgt, 4] xyxy, 16-byte aligned
  const int64_t* tgt_labels;     // [n_tgt]
  const int32_t* prp_off;        // [n_img + 1]
  const int32_t* tgt_off;        // [n_img + 1]
  int n_img, mode;               // mode 0: assign_label_to_proposals' labels, 1: prepare_targets'
  float high, low, wx, wy, ww, wh;
  int64_t* matched;              // out [n_prp]: GT index, -1 below low, -2 in [low, high)
  int64_t* labels;               // out [n_prp]
  int64_t* matched_rows;         // optional out [n_prp]: tgt_off[img] + max(matched, 0)
  float* targets;                // optional out [n_prp, 4], 16-byte aligned
};
struct BoxSubsampleArgs {
  const int64_t* labels;         // [n_prp]: >= 1 positive, 0 negative, anything else ignored
  const int32_t* prp_off;        // [n_img + 1]
  int n_img, batch, num_pos;
  uint64_t seed;
  int64_t* sampled;              // out [n_img, batch]: proposal indices inside the image, ascending
  int32_t* counts;               // out [n_img]
};
int box_match_max_gt();
int box_subsample_max_proposals();
int box_subsample_max_batch();
hipError_t launch_box_match(const BoxMatchArgs& a, int largest_prp, hipStream_t s);
hipError_t launch_box_subsample(const BoxSubsampleArgs& a, hipStream_t s);

// ---- detector training: the RPN loss -- anchor matching, sampling, both losses and their gradients (rpnloss.hip) ------
struct RpnLossLevel {
  const float* objectness;       // [n_img, A, H, W]; read by the loss stage only
  const float* regression;       // [n_img, 4A, H, W]
  const float* anchors;          // [A * H * W, 4] xyxy, anchor (h * W + w) * A + a, 16-byte aligned
  float* d_objectness;           // optional out, the shape of objectness
  float* d_regression;           // optional out, the shape of regression
  int A, HW, N, off;             // N = A * HW; off = the image-anchor index of the level's first anchor
};
struct RpnLossArgs {
  RpnLossLevel lvl[kRpnMaxLevels];
  const float* image_sizes;      // [n_img, 2] (width, height)
  const float* tgt_boxes;        // [n_tgt, 4] xyxy, 16-byte aligned
  const int32_t* tgt_off;        // [n_img + 1]
  int n_img, n_lvl, n_anchor, batch, num_pos, allow_lowq;
  float high, low, straddle, wx, wy, ww, wh;
  double beta;
  uint64_t seed;
  uint32_t* gtmax;               // workspace [n_tgt]: highest_quality_foreach_gt as bit patterns, zeroed by the call
  float* labels_ws;              // [n_img, n_anchor]: the labels output when it is given, else workspace
  int32_t* matched_ws;           // workspace [n_img, n_anchor]
  int32_t* hist;                 // workspace [n_img, 2, 256]: per class the histogram of the sampler keys' top 8 bits, zeroed by the call
  int32_t* sampled_ws;           // workspace [n_img, batch]
  int32_t* counts_ws;            // workspace [n_img, 2]
  double* partial;               // workspace [n_img, 2]: the image's two sums
  float* losses;                 // out [2]: objectness_loss, box_loss
  int64_t* matched;              // optional out [n_img, n_anchor]
  float* targets;                // optional out [n_img, n_anchor, 4], 16-byte aligned
  int64_t* sampled;              // optional out [n_img, batch]: anchor indices inside the image, ascending
  int32_t* counts;               // optional out [n_img, 2]: sampled positives, sampled negatives
};
struct RpnFillArgs {             // the tensors the call zeroes first, as floats
  float* ptr[2 * kRpnMaxLevels + 2];
  long long n[2 * kRpnMaxLevels + 2];
  int n_seg;
};
enum { kRpnLossMatch = 0, kRpnLossSample = 1, kRpnLossLoss = 2 };   // the stage a call stops after
int rpn_loss_max_gt();
int rpn_loss_max_anchors();
int rpn_loss_max_batch();
hipError_t launch_rpn_loss(const RpnLossArgs& a, const RpnFillArgs& fill, int last_stage, hipStream_t s);

// ---- detector training: the box head's loss -- both losses and their gradients (boxloss.hip) ------
struct BoxLossArgs {
  const float* logits;           // [n_rows, n_cls], row stride ld_logits elements: read in place
  const float* reg;              // [n_rows, n_reg_cols], row stride ld_reg elements: read in place
  const int64_t* labels;         // [n_rows]; outside [0, n_cls): the row is NaN
  const float* targets;          // [n_rows, 4], 16-byte aligned
  int n_rows, n_cls, n_reg_cols, cls_agnostic;
  long long ld_logits, ld_reg;
  double* partial;               // workspace [n_rows, 2]: the row's cross-entropy term and its box terms
  float* losses;                 // out [2]: classification_loss, box_loss
  float* d_logits;               // optional out [n_rows, n_cls], contiguous
  float* d_reg;                  // with d_logits: out [n_rows, n_reg_cols], contiguous, 16-byte aligned
};
int box_loss_max_cls();
int box_loss_max_rows();
hipError_t launch_box_loss(const BoxLossArgs& a, hipStream_t s);

// ---- the optimizer: global-norm clip and the Adam step over many tensors (optim.hip) ---------------
constexpr int kOptimChunk = 8192;        // elements of one tensor that one workgroup handles (a multiple of 4)
constexpr int kOptimMaxTensors = 4096;
constexpr int kOptimMaxChunks = 1 << 20;
struct OptimTensor {             // one row of the device table, as the host builds it for every call
  float* p;                      // [numel]
  const float* g;                // [numel]; NULL: the tensor has no chunk and takes no part
  float* m;                      // exp_avg
  float* v;                      // exp_avg_sq
  int numel;
  int chunk0, n_chunks;          // its rows of the chunk table
  int reserved;
  float wd, beta1, omb1, beta2, omb2, eps;   // omb = 1 - beta, rounded once from double
  float step_size;               // lr / (1 - beta1^step), rounded once from double
  float bc2_sqrt;                // sqrt(1 - beta2^step), rounded once from double
};
struct OptimChunk { int tensor, index; };   // elements [index * kOptimChunk, min(numel, (index + 1) * kOptimChunk)) of the tensor
struct OptimArgs {
  const OptimTensor* tensors;    // device [n_tensors]
  const OptimChunk* chunks;      // device [n_chunks]
  unsigned* counter;             // device, zero when the call starts: the norm pass's workgroups count themselves out on it
  double* partial;               // workspace [n_chunks]: the sum of g^2 of the chunk
  double* tensor_sq;             // workspace [n_tensors]
  int n_tensors, n_chunks;
  double max_norm;
  float* norms;                  // out [n_tensors]
  float* total;                  // out [1]
  float* coef;                   // out [1]: the applied coefficient
};
// norms: the norm pass.  apply: 0 nothing more, 1 scale the gradients in place by coef[0], 2 the Adam step.  use_coef: the step
// scales each gradient in registers by coef[0] (written by the norm pass of the same call); otherwise by exactly 1.
hipError_t launch_optim(const OptimArgs& a, bool norms, int apply, bool use_coef, hipStream_t s);

// ---- ROI feature extraction (roialign.hip) ----------------------------------------------------------
struct RoiLevel {
  const void* feat;              // [n_img, C, H, W] (NCHW) or [n_img, H, W, C] (NHWC) of the map group's element type
  int H, W;
  float scale;
};
enum RoiDtype { kRoiF32 = 0, kRoiF16 = 1, kRoiBF16 = 2 };      // veto_roi_pool_args_t.level_dtype / depth_dtype
enum RoiLayout { kRoiNCHW = 0, kRoiNHWC = 1 };                 // veto_roi_pool_args_t.level_layout / depth_layout
struct RoiPoolArgs {
  RoiLevel lv[4];                // FPN levels of the RGB pyramid, finest first
  RoiLevel depth;                // depth map (feat == nullptr: none)
  int lv_dtype, lv_layout;       // of all pyramid levels (the gradient maps are float32 in lv_layout)
  int depth_dtype, depth_layout; // of the depth map
  int z0;                        // set by the launchers: blockIdx.z + z0 == 1 is the depth map (a launch of one map group)
  int n_levels, k_min, k_max;    // LevelMapper range: -log2(first scale) .. -log2(last scale)
  int n_roi, channels, depth_channels;
  int pooled, sampling_ratio;
  const float* rois;             // [n_roi, 5] (image index, x1, y1, x2, y2)
  float* out_rgb;                // [n_roi, channels, pooled, pooled]
  float* out_depth;              // [n_roi, depth_channels, pooled, pooled]
  int32_t* out_levels;           // optional [n_roi]
  // backward only: gradients of the pooled outputs in, gradients of the maps out (accumulated atomically)
  const float* gout_rgb;         // [n_roi, channels, pooled, pooled]
  const float* gout_depth;       // [n_roi, depth_channels, pooled, pooled] or nullptr
  float* lv_grad[4];             // per level, same shape as lv[l].feat, zero-initialised by the caller
  float* depth_grad;
};
hipError_t launch_roi_pool(const RoiPoolArgs& a, hipStream_t s);
hipError_t launch_roi_pool_backward(const RoiPoolArgs& a, hipStream_t s);
// the ordered (gather) form: every element of every gradient map is written, in the summation order include/veto_amd.h states
hipError_t launch_roi_pool_backward_ordered(const RoiPoolArgs& a, int n_img, hipStream_t s);
// the adaptive sampling grid (sampling_ratio == 0: ceil(roi_size / pooled) samples per bin and axis, per ROI); NCHW maps only
hipError_t launch_roi_pool_adaptive(const RoiPoolArgs& a, hipStream_t s);
hipError_t launch_roi_pool_adaptive_backward(const RoiPoolArgs& a, hipStream_t s);

// ---- relation evaluators (sgg_eval.hip) ---------------------------------------------------------------
struct SggEvalArgs {
  int n_img, n_rel_cls, n_zeroshot;
  float iou_thres;
  const int32_t* gt_off;         // [n_img + 1] prefix sum of GT relations
  const int32_t* obj_off;        // [n_img + 1] prefix sum of objects
  const int32_t* pred_obj_off;   // [n_img + 1] prefix sum of predicted objects, or nullptr = obj_off (GT-box modes)
  int mode;                      // 0 = GT boxes, 1 = sgdet (no pair-accuracy hits)
  const int32_t* pair_off;       // [n_img + 1] prefix sum of predicted pairs
  const int64_t* gt_rels;        // [sum G, 3] (subject, object, predicate), image-local indices
  const int64_t* gt_classes;     // [sum N]
  const float* gt_boxes;         // [sum N, 4] xyxy
  const int64_t* pred_pairs;     // [sum P, 2], in ranking order per image
  const float* rel_scores;       // [sum P, n_rel_cls]
  const int64_t* pred_classes;   // [sum N]
  const float* pred_boxes;       // [sum N, 4]
  const float* obj_scores;       // [sum N]
  const int64_t* zeroshot;       // [n_zeroshot, 3] (subject class, object class, predicate)
  int32_t *gc_rank, *ng_rank, *acc_rank, *zeroshot_flag;   // out [sum G]
  int32_t *ng_rows, *ng_cols;    // out [n_img, 100]
  int32_t* ng_count;             // out [n_img]
  double* metrics;               // out [18 + 6 * (n_rel_cls - 1) + 2]
  int32_t *label_tmp, *flag_tmp, *flag_before;             // workspace [sum P]
  float* pair_score;             // workspace [sum P]
  uint32_t* row_key;             // workspace [sum P]: sortable key of the row's largest cell
  int32_t* acc_first;            // workspace [sum G]
  int32_t* cls_table;            // workspace [n_img, 7, n_rel_cls]
};
hipError_t launch_sgg_eval(const SggEvalArgs& a, hipStream_t s);

// The split-level fold over the per-relation records that launch_sgg_eval leaves (ranks, zero-shot flags) and the GT predicates
struct SggEvalFoldArgs {
  int n_img, n_rel_cls, mode;    // mode 0 = GT boxes, 1 = sgdet (A@K = NaN)
  int n_gt_total;                // rows of the record arrays
  const int32_t* img_gt_off;     // [n_img + 1] prefix sum of GT relations
  const int32_t* img_pair_cnt;   // [n_img] predicted pairs: an image with G == 0 or P == 0 contributes nothing
  const int32_t *gt_predicate, *gc_rank, *ng_rank, *acc_rank, *zeroshot_flag;   // [n_gt_total]
  double* metrics;               // out [18 + 6 * (n_rel_cls - 1) + 2], the layout of SggEvalArgs::metrics
  double* per_image;             // out [n_img, 12] or nullptr
  double* partial;               // workspace [chunks, sgg_eval_fold_partial_doubles(n_rel_cls)]
};
hipError_t launch_sgg_eval_fold(const SggEvalFoldArgs& a, hipStream_t s);
int sgg_eval_fold_images_per_chunk();   // images one workgroup folds, in image order
int sgg_eval_fold_max_rel_cls();        // predicate classes with the background: the per-image table lives in LDS
inline size_t sgg_eval_fold_chunks(size_t n_img) { return (n_img + sgg_eval_fold_images_per_chunk() - 1) / sgg_eval_fold_images_per_chunk(); }
__host__ __device__ inline size_t sgg_eval_fold_partial_doubles(int n_rel_cls) { return 16 + 7 * (size_t)n_rel_cls; }

// ---- detection (box mAP) evaluator (det_eval.hip) -------------------------------------------------------
constexpr int kDetEvalThrs = 10;       // IoU thresholds
constexpr int kDetEvalAreas = 4;       // area ranges
constexpr int kDetEvalRecThrs = 101;   // recall thresholds
struct DetEvalMatchArgs {
  int n_img, n_cls;
  long long first_gt_id;         // annotation id of this batch's first GT box
  long long row_offset;          // record row of this batch's first detection
  double iou_thrs[kDetEvalThrs];
  double area_rngs[2 * kDetEvalAreas];   // lo, hi per range
  const int32_t* gt_off;         // [n_img + 1] prefix sum of GT boxes
  const int32_t* det_off;        // [n_img + 1] prefix sum of detections
  const float* gt_boxes;         // [sum G, 4] xyxy
  const int64_t* gt_labels;      // [sum G]
  const float* det_boxes;        // [sum D, 4] xyxy
  const float* det_scores;       // [sum D]
  const int64_t* det_labels;     // [sum D]
  unsigned long long* rec_key;   // out [row_offset + sum D ..): class << 32 | inverted score key (class 0: not counted)
  unsigned long long* rec_match; // out: 40 matched bits (threshold * 4 + area) | rank << 40
  unsigned long long* rec_ignore;// out: 40 ignored bits
  unsigned long long* npig;      // in/out [n_cls - 1, 4]: non-ignored GT boxes, added to
  int32_t* label_errors;         // in/out [1] or nullptr: labels outside 1..n_cls-1 met (they are not counted), added to
  uint8_t* gtm;                  // workspace [sum G, 40]: "GT taken" per (threshold, area)
};
hipError_t launch_det_eval_match(const DetEvalMatchArgs& a, hipStream_t s);

struct DetEvalAccumArgs {
  int n_cls;
  long long n_rec;
  double iou_thrs[kDetEvalThrs];
  double rec_thrs[kDetEvalRecThrs];
  const unsigned long long *rec_key, *rec_match, *rec_ignore;   // [n_rec]
  const unsigned long long* npig;                               // [n_cls - 1, 4]
  double* precision;             // out [10, 101, n_cls - 1, 4, 3]
  double* recall;                // out [10, n_cls - 1, 4, 3]
  double* stats;                 // out [12]
  double* recall50_100;          // out [1]
  unsigned long long *key_a, *key_b;   // workspace [n_rec] each
  uint32_t *idx_a, *idx_b;             // workspace [n_rec] each
  uint32_t* hist;                      // workspace [256, tiles]
  int32_t* seg_start;                  // workspace [n_cls + 1]: first sorted record of class c (entry n_cls: n_rec)
};
hipError_t launch_det_eval_accumulate(const DetEvalAccumArgs& a, hipStream_t s);
int det_eval_max_gt();           // GT boxes per image
int det_eval_max_det();          // detections per image
int det_eval_scan_chunk();       // records per step of the accumulate pass over a class segment
int det_eval_sort_tile();        // records per workgroup of the radix sort
inline long long det_eval_sort_tiles(long long n_rec) { return n_rec > 0 ? (n_rec + det_eval_sort_tile() - 1) / det_eval_sort_tile() : 1; }

// ---- training losses / MEET sampling (losses.hip) ----------------------------------------------------------
struct CeLossArgs {
  const float* logits;           // row r at logits + r*ld
  long ld;
  const int64_t* labels;         // [n], aligned with the selected rows
  const float* weight;           // [C] or nullptr
  const int64_t* rows;           // [n] row indices into logits, or nullptr = rows 0..n-1
  int n, C;
  float *log_sum, *nll_w, *w_row;   // workspace [n] each; log_sum = logf(sum exp(z - max z)), the row maximum is NOT folded in
  float* inv_wsum;               // workspace [1]
  float* loss;                   // out [1]
  float* grad;                   // optional out [n, C]
};
hipError_t launch_ce_loss(const CeLossArgs& a, hipStream_t s);

struct MeetSampleArgs {
  const int64_t* labels;         // [n] relation labels
  int n, n_groups, n_cls, n_words;
  const uint32_t* words;         // [n_words] raw MT19937 outputs of Python's random, in order
  const int32_t* incre;          // [n_cls] 1-based group of each class
  const int32_t* pos_in_group;   // [n_cls] 1-based position of the class inside its group
  const int32_t* group_size;     // [n_groups]
  const double* rates;           // [n_groups, n_cls] sample_rate_matrix
  int64_t* chosen;               // out [n_groups, n] row indices per group (first counts[k] valid)
  int64_t* group_labels;         // out [n_groups, n] remapped labels of those rows
  int32_t* counts;               // out [n_groups]
  int32_t* words_used;           // out [1]; -1 = the word block was too short
};
hipError_t launch_meet_sample(const MeetSampleArgs& a, hipStream_t s);

// The same sampling for all three ZERO_LABEL_PADDING_MODEs, with only the rand_insert word chain left serial (losses.hip).
enum MeetPadMode { MEET_RAND_INSERT = 0, MEET_RAND_CHOOSE = 1, MEET_ALL_INCLUDE = 2 };
struct MeetParallelArgs {
  MeetSampleArgs s;              // labels, words, tables and outputs: the serial sampler's
  int mode;                      // MeetPadMode
  unsigned long long* fg_mask;   // workspace [ceil(n / 64)]: bit i % 64 of word i / 64 = relation i is foreground
  unsigned long long* acc_mask;  // workspace [ceil(n_words / 64)], rand_insert: the same for "randint accepts word j"
  int32_t* pos;                  // workspace [n]: rand_insert: the word a relation decides on (foreground: its first; background: the
                                 // accepted one); all_include: entry b = foreground relations in front of relation 64 b
  uint16_t* span;                // workspace [n]: lo | hi << 8, the relation goes to groups lo .. hi-1
  int32_t* tile_count;           // workspace [tiles, 64]: rows of a tile per group, then (in place) rows in front of the tile
};
hipError_t launch_meet_sample_parallel(const MeetParallelArgs& a, hipStream_t s);
int meet_parallel_tile();        // relations per workgroup of the decision and of the compaction
int meet_parallel_window();      // words per register window of the rand_insert walk (64 mask words)
int meet_parallel_chunk();       // relations per mask word: the walk flushes its positions once per chunk
inline long long meet_parallel_tiles(long long n) { return (n + meet_parallel_tile() - 1) / meet_parallel_tile(); }

// ---- dropout sites of the training path, and the elementwise backward in front of a Linear's gradient GEMMs ---------------------
struct DropSite {   // one dropout site: threshold p * 2^24 (0 = off), scale 1 / (1 - p).  Host side only: what goes into a kernel by value
                    // (GemmArgs, ObjPrepArgs, AssembleArgs, GradXform) keeps fields of its own, filled from the site
  unsigned long long seed = 0;
  unsigned thresh = 0;
  float scale = 1.f;
  int row_step = 1;   // row r of the matrix the site is applied to is token row r * row_step (the last layer's compact CLS rows: 19)
};
enum GradXformMode { XF_NONE = 0, XF_GELU = 1, XF_DROP = 2 };
struct GradXform {
  int mode = XF_NONE;
  const float* pre = nullptr;           // XF_GELU: pre-activation [M, ld]
  unsigned long long seed = 0;          // XF_DROP: element (m, n) -> index (m * row_step) * N + n
  unsigned thresh = 0;
  float scale = 1.f;
  int row_step = 1;
};
// y = the mask of `site` applied to x ([rows, n_cols], index row*n_cols + col; row_step 1), scaled by site.scale; in place allowed
hipError_t launch_dropout_apply(const float* x, float* y, size_t rows, int n_cols, const DropSite& site, hipStream_t s);

// ---- backward building blocks (backward.hip) -----------------------------------------------------------------
// qkv, dqkv: [n_pair*19, 1728]; dout: [n_pair*19, 576] (gradient of the attention output before the out projection)
// exactly one of dqkv (fp32 [n_pair*19, 1728]) and dqkv_split (split rows [n_pair*19, 2*1728]) is written
// cls_only: dout is compact [n_pair, 576] (gradient of the CLS query's output only), q rows 1..18 of qkv are not read
// qkv_f24 (head widths 72 / 96): qkv holds 3-byte floats (common.h), rows of 1728 x 3 bytes
hipError_t launch_attention_backward(const float* qkv, const float* dout, float* dqkv, __bf16* dqkv_split, int n_pair, int heads, int cls_only,
                                     hipStream_t s, bool qkv_f24 = false);
// dx = LayerNorm backward of dy w.r.t. x (+ dres if given); dgamma_dbeta [2, 576]; partial: workspace of
// layernorm_backward_partial_floats(rows) floats (dgamma_dbeta == nullptr: not wanted, the fold of the partial rows is left out)
size_t layernorm_backward_partial_floats(int rows);
// split_out / colp (both or neither): also write the result's split rows [rows, 2 * 576] (with the dropout mask of `site` applied
// when site.thresh != 0: element (row, col) -> index (row * site.row_step) * 576 + col) and layernorm_backward_col_partials(rows) rows of column sums [*, 576]
// of those rows -- what launch_prep_grad would produce from dx, for the Linear behind this LayerNorm in the backward chain
int layernorm_backward_col_partials(int rows);
hipError_t launch_layernorm_backward(const float* x, const float* dy, const float* gamma, const float* dres, float* dx,
                                     float* dgamma_dbeta, float* partial, int rows, hipStream_t s, __bf16* split_out, float* colp,
                                     const DropSite& site, bool ordered);
// out[c] = (float) of the double sum over rows r = 0 .. n_rows - 1 of src[r * ld + c], rows in a fixed order (fold_rows_kernel): the fold of
// the split-K partial planes of the ordered weight gradient
hipError_t launch_fold_rows(const float* src, long ld, int n_rows, long n_cols, float* out, hipStream_t s);
// out[c] = sum_r dy[r][c]; partial: workspace [n_chunks, n_cols]; column_sums_chunks() chunks keep every stage short
int column_sums_chunks();
hipError_t launch_column_sums(const float* dy, long ld, int rows, int n_cols, float* out, float* partial, int n_chunks, hipStream_t s);
hipError_t launch_gelu_backward(const float* pre, const float* dh, float* dpre, size_t n, hipStream_t s);

// ---- training path around the GEMMs (train.hip) ---------------------------------------------------------------
// dY fp32 [M, N] -> split rows [M, 2N] (the operand of BOTH gradient GEMMs) and (optional) per-32-row column sums
// col_partial [Mp/32, N] (Mp = M rounded up to 32, >= M) in one pass.  GradXform: the elementwise backward that precedes this Linear, applied on load
// (dY itself is not rewritten): gelu'(pre) or the forward's dropout mask.
hipError_t launch_prep_grad(const float* src, long ld, int M, int N, __bf16* rows_out, int Mp, float* col_partial,
                            const GradXform& xf, hipStream_t s);
hipError_t launch_gelu_split(const float* pre, __bf16* dst, size_t rows, int n_cols, hipStream_t s);
// dx row p = dlogits[p] . W; dw [n_out, 576], db [n_out]; row p of x and of dx at + p * ld floats (the CLS rows)
// partial: workspace of head_backward_partial_floats(n_out) floats.  dx / dw / db == nullptr: that output and its launches are left out
size_t head_backward_partial_floats(int n_out);
hipError_t launch_head_backward(const float* dlogits, const float* w, const float* x, float* dx, float* dw, float* db, float* partial,
                                int n_pair, int n_out, long ld, hipStream_t s);
hipError_t launch_assemble_backward(const float* dx, const int32_t* subj, const int32_t* obj, const float* lc, float* dpatch, float* dlc,
                                    int n_pair, hipStream_t s);
// the ordered form (include/veto_amd.h, "ordered mode"): per object, token and half the float32 sum over the image's pair rows in
// ascending order; writes every element of dpatch / dlc.  subj / obj: batch-wide object rows; img_*_off: device [n_img + 1]
hipError_t launch_assemble_backward_ordered(const float* dx, const int32_t* subj, const int32_t* obj, const float* lc,
                                            const int32_t* img_obj_off, const int32_t* img_pair_off, int n_img, float* dpatch, float* dlc,
                                            int n_obj, hipStream_t s);
hipError_t launch_sgemm_tn(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int n, int ka, int kb, hipStream_t s);
hipError_t launch_sgemm_nt(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int n, int ki, int kj, hipStream_t s);
// mean / var [4]: what the forward's BatchNorm normalised with (the batch statistics, or the running ones of an eval-mode pos_embed.0);
// dgamma / dbeta == nullptr: that affine gradient is not written (both: its kernel is not launched)
hipError_t launch_obj_pos_backward(const float* boxes, int box_mode, const float* mean, const float* var, const float* bn_w, const float* bn_b,
                                   const float* pos_w, const float* pos_b, const float* dpos, float* dpre, float* xhat, float* bn_out,
                                   float* dbn_out, float* dgamma, float* dbeta, int n_obj, hipStream_t s);
hipError_t launch_sgemm_nn(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int n, int ki, int kj, hipStream_t s);
hipError_t launch_softmax_rows(const float* x, float* y, int n, int c, hipStream_t s);
hipError_t launch_bias_relu(float* x, const float* b, int n, int k, hipStream_t s);
hipError_t launch_gather_rows(const float* table, const int64_t* labels, int dim, float* out, int n, hipStream_t s);
hipError_t launch_scatter_rows(const float* demb, const int64_t* labels, int dim, float* dtable, int n, hipStream_t s);
// the ordered form: dtable [n_table_rows, dim] written whole, row r = the float32 sum over the object rows labelled r in ascending order
hipError_t launch_scatter_rows_ordered(const float* demb, const int64_t* labels, int dim, float* dtable, int n, int n_table_rows,
                                       hipStream_t s);
hipError_t launch_untranspose_pair_proj(const float* dwt, float* dw, int kin, hipStream_t s);
hipError_t launch_patch_weight_grad(const float* dwcat_t, float* dwd, float* dwv, int p, hipStream_t s);      // (dwd / dwv == nullptr: not written)
// Input gradient of the patch projection (training): the TRANSPOSE of the combined patch weight as a GEMM weight operand,
// dst [patch_t_rows(p), 2*1152] split rows (rows patch_feats(p).. are zero; p = 2: 2112 = 2048 padded to 11 x 192 output columns), and
// the scatter of dPA [n_obj*16, ld] fp32 (patch rows x patch features, depth features first) back onto the ROI maps [n_obj, 256, 4p, 4p]
hipError_t launch_build_patch_weight_t(const float* wd, const float* wv, __bf16* dst, int p, hipStream_t s);
hipError_t launch_unpatchify(const float* dpa, long ld, float* d_depth, float* d_rgb, int n_obj, int p, hipStream_t s);

}  // namespace veto
