/*
 * veto_amd.h -- C ABI of the MI355X-native VETO relation-prediction hot path.
 *
 * The reference has NO FFI on this path: VETOPredictor is pure Python/PyTorch
 * (pysgg/modeling/roi_heads/relation_head/roi_relation_predictors.py:3997-4139 and
 * model_veto.py:6-146).  The boundary a maintainer binds is therefore the predictor's own
 * forward, flattened to raw device pointers:
 *
 *   veto_create            <- VETOPredictor.__init__            roi_relation_predictors.py:3999-4071
 *   veto_load_weights      <- nn.Module.load_state_dict keys    SURVEY.md section 8(b) key list
 *   veto_forward           <- VETOPredictor.forward (eval)      roi_relation_predictors.py:4074-4139
 *                             Ensemble.forward (MEET, eval)     roi_relation_predictors.py:3752-3853
 *   veto_enumerate_pairs   <- RelationSampling.prepare_test_pairs   sampling.py:31-52 (GT-box branch)
 *   veto_prepare_test_pairs <- the same, sgdet branch (box-overlap filter, capped pair order)   sampling.py:31-52
 *   veto_detect_relsample  <- RelationSampling.detect_relsample (sgdet training)   sampling.py:109-309
 *   veto_gtbox_relsample   <- RelationSampling.gtbox_relsample (predcls / sgcls training)   sampling.py:54-107
 *   veto_obj_decode        <- obj_prediction_nms (PostProcessor)    utils_relation.py:94-128, inference.py:410-429
 *                             Ensemble.nms_per_cls (MEET decoder)   roi_relation_predictors.py:3855-3874
 *   veto_nms               <- pysgg._C.nms / boxlist_nms            csrc/cuda/nms.cu, structures/boxlist_ops.py:10-32
 *   veto_box_postprocess   <- PostProcessor (box head)              roi_heads/box_head/inference.py:51-238
 *   veto_rpn_proposals     <- RPNPostProcessor                      rpn/inference.py:13-183
 *   veto_anchor_grid       <- AnchorGenerator.forward (grid_anchors, add_visibility_to)   rpn/anchor_generator.py:73-125
 *   veto_box_match         <- FastRCNNSampling.assign_label_to_proposals / prepare_targets   roi_heads/box_head/sampling.py:34-82, 118-133
 *   veto_box_subsample     <- BalancedPositiveNegativeSampler + FastRCNNSampling.subsample    balanced_positive_negative_sampler.py:37-66
 *   veto_rpn_loss          <- RPNLossComputation (prepare_targets, __call__) and its backward   rpn/loss.py:21-157
 *   veto_box_loss          <- FastRCNNLossComputation.__call__ and its backward   roi_heads/box_head/loss.py:42-84
 *   veto_optim_step        <- clip_grad_norm and the step of make_optimizer's Adam   utils/checkpoint.py:180-219, solver/build.py:7-34
 *
 * Conventions: every pointer marked "device" is a HIP device pointer valid on cfg.device;
 * `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on that
 * stream and nothing synchronises it.  Functions return 0 on success, a negative veto_status
 * otherwise; veto_last_error() gives a thread-local message.  No exceptions cross the boundary.
 * A handle is not thread-safe; use one handle per stream/thread.
 */
#ifndef VETO_AMD_H_
#define VETO_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct veto_handle_s* veto_handle_t;

enum veto_status {
  VETO_OK = 0,
  VETO_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
  VETO_ERR_HIP = -2,          /* a HIP runtime call failed */
  VETO_ERR_WEIGHTS = -3,      /* forward called before every weight was loaded */
  VETO_ERR_WORKSPACE = -4     /* workspace too small */
};

enum veto_precision {
  VETO_PRECISE = 0,  /* 3-term split-bf16 MFMA on every Linear, meets the 1e-3 logit tolerance (2-3e-5 measured).  Range: the Linears'
                        operands keep the fp32 exponent range; the ATTENTION products (every mode, the training path included) split
                        q / k / v and the probabilities into fp16 hi + fp16 lo planes (22 significant bits; on the training path q / k / v
                        are stored as 3-byte floats by default and so carry 16, VETO_TRAIN_QKV_F24=0 restores 22): each plane saturates at
                        +-65504, so of |q|, |k|, |v| beyond 65504 the lo plane keeps the excess with its own 11 bits and the operand clamps
                        only beyond +-131008; components below ~2^-24 are dropped -- both far outside what LayerNorm'ed rows times
                        weights produce (O(10)); no audit counts them */
  VETO_FAST = 1,     /* single-pass form of VETO_MIXED (round 6; rounds 1-5: a single bf16 pass of every GEMM): the same launches
                        on the same operand rows, but the two fused token-row launches of a layer (QKV + attention, layer tail) skip the
                        correction stages -- the fp16 main product alone, neither loading nor multiplying the e4m3 planes.  The measured
                        floor of the schedule with the precision terms free; logit error ~2e-3 (over the 1e-3 bar): reported, never
                        parity-grade.  Inference only. */
  VETO_MIXED = 2     /* fp16 MFMA main product + e4m3 K=128 MFMA correction terms on the token-row Linears: 2/3 of the
                        matrix-pipe time of VETO_PRECISE, logit error 4-9e-5 measured (1e-3 tolerance); what the Python
                        plugin selects by default (VETO_AMD.PRECISION = "mixed").  Supported activation range: the e4m3
                        planes keep full precision for |activation| <= 448 (an element beyond degrades to the fp16
                        class, 2^-11; fp16 overflows at 65504); 6.3e-5 on trained-like activations
                        (tests/test_gpu_parity.py::test_parity_on_trained_like_activations).  In this mode everything
                        of a full layer behind its attention runs as ONE launch (ffn_fused.hip: out projection, both
                        residuals, both LayerNorms, FeedForward), and q / k / v travel from the QKV projection to the
                        attention kernel as 3-byte floats (a 16-bit significand: what the attention's bf16 hi + lo
                        operands keep anyway); logit error 5.7e-5 measured in round 3.  The inference path uses the
                        one-exponential GELU (|error| <= 1e-6) in every mode; the training path keeps the erf form */
};

/* MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.* (config/defaults.py:331-338) + class counts.
 *
 * Patch grids.  (resolution, patch) = (POOLER_RESOLUTION, PATCH_SIZE) is one of (4, 1), (8, 2), (12, 3), (16, 4): resolution == 4 * patch, so
 * that an object's map always cuts into a 4 x 4 grid of patches and a pair into 19 tokens (CLS, location, class, 16 patches), which is
 * what the fused launches hold; veto_create refuses every other pair with a message that names these four, before it allocates
 * anything.  With p = patch, R = 4 p, K = 512 p^2 (512 / 2048 / 4608 / 8192):
 *   ROI maps (inputs and their gradients)       [n_obj, 256, R, R]
 *   patch_embed.proj_d.weight / .proj_v.weight  [512, K] / [64, K]; input feature (p1 p2 c) of cat(subject, object) = (p1 p + p2) 512 +
 *                                               half 256 + c, as einops 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' leaves them
 *   patch rows (workspaces)                     [n_obj * 16 padded to 256, 2 K] bf16 split rows: depth features 0 .. K/2 - 1, then
 *                                               rgb, feature (p1 p + p2) 256 + c
 *   staged patch weight                         [1152, 2 K] split rows;  its transpose for the map gradients [K padded to a multiple
 *                                               of 192 (576 / 2112 / 4608 / 8256), 2 * 1152], the padding rows zero
 * veto_workspace_bytes and veto_train_workspace_bytes* size these from the handle's patch.  Everything behind the patch
 * projection (token assembly, layers, head) is the same for the four. */
typedef struct veto_config {
  int32_t struct_size;     /* sizeof(veto_config_t), for ABI evolution */
  int32_t dim;             /* T_INPUT_DIM; must be 576 (model_veto.py:105-113 force it) */
  int32_t layers;          /* ENC_LAYERS */
  int32_t heads;           /* NHEADS; must divide 576 with 576/heads % 4 == 0 */
  int32_t patch;           /* PATCH_SIZE p: 1, 2, 3 or 4 */
  int32_t channels;        /* ROI channels per modality; must be 256 */
  int32_t resolution;      /* POOLER_RESOLUTION; must be 4 * patch (4, 8, 12 or 16) */
  int32_t num_obj_cls;     /* 151 (VG) / 201 (GQA); <= 256 */
  int32_t embed_dim;       /* 200 */
  int32_t num_out;         /* head width: num_rel_cls (51/101) or sum_k (g_k + 2) for MEET */
  int32_t precision;       /* enum veto_precision */
  int32_t device;          /* HIP device ordinal */
  int32_t max_chunk_pairs; /* pairs processed per pass (bounds the workspace); 0 = default */
} veto_config_t;

typedef struct veto_inputs {
  int32_t struct_size;        /* sizeof(veto_inputs_t) */
  int32_t n_obj;              /* total objects over the batch */
  int32_t n_pair;             /* total pairs over the batch */
  int32_t n_img;              /* images in the batch */
  const float* roi_rgb;       /* device [n_obj, 256, R, R]  roi_features        (relation_head.py:140-141); R = the handle's resolution */
  const float* roi_depth;     /* device [n_obj, 256, R, R]  roi_depth_features                              */
  const float* boxes;         /* device [n_obj, 4]  BoxList.bbox */
  int32_t box_mode;           /* 0 = xyxy, 1 = xywh (BoxList.mode) */
  int32_t reserved0;
  const int64_t* obj_labels;  /* device [n_obj]; predcls GT labels, or MEET sgcls argmax labels; or NULL */
  const float* obj_logits;    /* device [n_obj, num_obj_cls]; vanilla sgcls soft embedding; or NULL */
  const int64_t* rel_pairs;   /* device [n_pair, 2] image-local (subj, obj), images concatenated */
  const int32_t* img_obj_offset;   /* device [n_img + 1] exclusive prefix sum of objects per image */
  const int32_t* img_pair_offset;  /* device [n_img + 1] exclusive prefix sum of pairs per image */
  float* bn_batch_stats;      /* NULL: BatchNorm1d(4) of pos_embed in eval mode (running statistics).  Non-NULL device [12]:
                                 TRAINING-mode BatchNorm (roi_relation_predictors.py:4042-4047, module.train()): the four box
                                 features are normalised with the statistics of THIS batch, which are also written here as
                                 mean[4], biased variance[4], unbiased variance[4] for the caller's running-statistics update */
} veto_inputs_t;

/* Optional extra outputs (all may be NULL); used by the parity tests. */
typedef struct veto_debug_outputs {
  int32_t struct_size;
  int32_t reserved0;
  int64_t* subj_inds;   /* device [n_pair] global subject index  (roi_relation_predictors.py:4112) */
  int64_t* obj_inds;    /* device [n_pair] global object index   (:4113) */
  float* tokens;        /* device [n_pair, 19, 576] transformer input (model_veto.py:52-64) */
  float* cls;           /* device [n_pair, 576] final CLS feature (model_veto.py:23) */
} veto_debug_outputs_t;

const char* veto_last_error(void);
const char* veto_version(void);

int veto_create(const veto_config_t* cfg, veto_handle_t* out);
int veto_destroy(veto_handle_t h);

/* Number of weight tensors the handle expects and the i-th expected name/numel. Names are the
 * reference state-dict keys relative to the predictor, e.g.
 * "fusion_transformer.transformer.layers.0.0.fn.to_qkv.weight"; for MEET the K heads are passed
 * row-concatenated as "rel_out.weight"/"rel_out.bias". */
int veto_num_weights(veto_handle_t h);
int veto_weight_info(veto_handle_t h, int index, const char** name, size_t* numel);
/* Copies `numel` fp32 values from `src` (device or host pointer) on `stream`.
 * The next forward rebuilds the derived operands that read this tensor, and only those:
 *   a layer Linear (to_qkv / to_out.0 / net.0 / net.3 .weight)                     its own split rows and mixed rows
 *   layer 0's 0.norm.weight / .bias, to_qkv.weight, pos_embedding, cls_token       the layer-0 constants (Wqkv diag(gamma), vectors)
 *   the last layer's to_qkv.weight / to_out.0.weight                               the folded last layer's factors
 *   patch_embed.*                                                                  the staged patch weight and bias
 *   location_projection.0.weight, class_projection.0.weight, rel_out.weight       their transposes
 *   every other tensor (biases, obj_embed, pos_embed.*, LayerNorm2 gains, ...)     nothing: it is read in place
 * A rebuilt operand has the bytes a rebuild of everything gives it. */
int veto_load_weights(veto_handle_t h, const char* name, const float* src, size_t numel, void* stream);

/* Test hook: what the last rebuild of derived operands (at the head of a forward that found uploaded weights) launched, as a count
 * of rebuilt operands per kind.  counts: host array of `capacity` >= VETO_BUILD_KINDS entries.  Returns VETO_BUILD_KINDS. */
enum veto_build_kind {
  VETO_BUILD_SPLIT_ROWS = 0,   /* split rows of a layer Linear */
  VETO_BUILD_MIXED_ROWS = 1,   /* mixed rows of a layer Linear (VETO_MIXED / VETO_FAST handles) */
  VETO_BUILD_PATCH = 2,        /* the staged patch weight and bias */
  VETO_BUILD_LOC_T = 3,        /* location_projection.0.weight transposed */
  VETO_BUILD_CLS_T = 4,        /* class_projection.0.weight transposed */
  VETO_BUILD_HEAD_T = 5,       /* rel_out.weight transposed */
  VETO_BUILD_QKV0 = 6,         /* the layer-0 constants */
  VETO_BUILD_FOLD = 7,         /* the folded last layer's factors */
  VETO_BUILD_KINDS = 8
};
int veto_debug_last_finalize(veto_handle_t h, int32_t* counts, int32_t capacity);

size_t veto_workspace_bytes(veto_handle_t h, int32_t n_obj, int32_t n_pair);

/* Eval forward.  out_logits: device [n_pair, num_out] fp32. */
int veto_forward(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace,
                 size_t workspace_bytes, float* out_logits, const veto_debug_outputs_t* dbg);

/* ---- saturation audit of the VETO_MIXED operands (diagnostic) ---------------------------------
 * VETO_MIXED stores every activation that feeds a token-row Linear as fp16 + two e4m3 planes (value, residual x 2^11).  The
 * conversions SATURATE (MODE.FP16_OVFL is set in every kernel that writes such rows): |a| > 448 clamps both e4m3 planes of that
 * element at +-448 -- it then carries fp16 precision (2^-11) instead of 2^-16 -- and |a| > 65504 clamps its fp16 at +-65504, i.e.
 * an Inf or an overflow becomes a FINITE wrong value where the fp32 reference would propagate Inf (a NaN stays a NaN).  Both
 * happen silently in veto_forward.  This call makes them visible: it runs the same forward in its launch-per-stage form (every
 * mixed-row operand exists in memory; logits equal to veto_forward's up to the rounding order of the fused kernels) and counts,
 * behind every producer, the elements that sit AT the clamp values.  counts[layer * VETO_SAT_SITES + site] (host memory,
 * capacity >= layers * VETO_SAT_SITES entries); the last layer runs its attention on split-bf16 operands (its qkv_in / attn_out
 * sites report zeros) and its FeedForward on the pairs' CLS rows only -- mixed rows all the same, and the classifier's input: its
 * ffn_in / hidden sites count n_pair rows --, layer 0 feeds only the location / class token rows through a mixed QKV projection.  Non-zero value_saturated / resid_saturated: those elements lost
 * the correction terms (harmless in small numbers: the 1e-3 logit tolerance holds with 3 % of the hidden units at x 30 and some at
 * x 300, tests/test_gpu_parity.py::test_parity_on_trained_like_activations).  Non-zero f16_saturated: the result is wrong; use
 * VETO_PRECISE for this checkpoint. */
enum veto_saturation_site {
  VETO_SAT_QKV_IN = 0,    /* LayerNorm1 rows: the QKV projection's operand (model_veto.py:125-132 -> :85) */
  VETO_SAT_ATTN_OUT = 1,  /* attention output: the out projection's operand (:94-96) */
  VETO_SAT_FFN_IN = 2,    /* LayerNorm2 rows: fc1's operand (:137-139) */
  VETO_SAT_HIDDEN = 3,    /* gelu(fc1): fc2's operand (:140-143) */
  VETO_SAT_SITES = 4
};
typedef struct veto_saturation {
  int64_t elements;          /* operand elements scanned at this site (0: the site does not exist in this layer) */
  /* upper bounds: an encoding at the clamp also holds values that merely round to it, and NaN / Inf encodings are counted too */
  int64_t f16_saturated;     /* fp16 values at or beyond +-65504 (incl. Inf / NaN) */
  int64_t value_saturated;   /* e4m3 value-plane bytes at +-448 (incl. the NaN encoding) */
  int64_t resid_saturated;   /* e4m3 residual-plane bytes at +-448 (incl. the NaN encoding) */
} veto_saturation_t;
int veto_forward_saturation(veto_handle_t h, void* stream, const veto_inputs_t* in, void* workspace, size_t workspace_bytes,
                            float* out_logits, veto_saturation_t* counts, int32_t capacity);

/* out: device [max(n*(n-1), 1), 2] int64, row-major (i, j), i != j; [[0,0]] when n <= 1. */
int veto_enumerate_pairs(void* stream, int32_t n, int64_t* out);

/* ---- relation post-processing ---------------------------------------
 * The vanilla GT-box branch of PostProcessor.forward, pysgg/modeling/roi_heads/relation_head/
 * inference.py:398-453: softmax of object and predicate logits, max over the foreground classes,
 * triple score rel*obj_s*obj_o, descending sort per image (ties: lower original index first), and the
 * pair indices / probabilities / labels emitted in that order. */
typedef struct veto_post_args {
  int32_t struct_size;            /* sizeof(veto_post_args_t) */
  int32_t n_img, n_obj, n_pair;
  int32_t n_rel_cls, n_obj_cls;   /* 51 / 151 (VG) */
  int32_t max_pairs_per_image;    /* host-side maximum of the per-image pair counts; must be <= 16384 */
  int32_t reserved0;
  const float* rel_logits;        /* device [n_pair, n_rel_cls] */
  const float* obj_logits;        /* device [n_obj, n_obj_cls]  (refine logits / predict_logits); NULL (sgdet): obj_scores and
                                     obj_pred are INPUTS, filled by veto_obj_decode */
  const int64_t* rel_pairs;       /* device [n_pair, 2] image-local */
  const int32_t* img_obj_offset;  /* device [n_img + 1] */
  const int32_t* img_pair_offset; /* device [n_img + 1] */
  float* obj_scores;              /* out device [n_obj]   -> BoxList field pred_scores */
  int64_t* obj_pred;              /* out device [n_obj]   -> pred_labels */
  float* rel_prob_sorted;         /* out device [n_pair, n_rel_cls] -> pred_rel_scores */
  int64_t* rel_pairs_sorted;      /* out device [n_pair, 2]         -> rel_pair_idxs */
  int64_t* rel_labels_sorted;     /* out device [n_pair]            -> pred_rel_labels */
  float* triple_sorted;           /* optional out device [n_pair] (the sort keys) */
} veto_post_args_t;

size_t veto_postprocess_workspace_bytes(int32_t n_pair, int32_t n_rel_cls);
int veto_postprocess(void* stream, const veto_post_args_t* args, void* workspace, size_t workspace_bytes);

/* MEET merge branch (ENSEMBLE_LEARNING.ENABLED, EXPERT_GROUP False), inference.py:284-397, for ONE image
 * (the reference zips the group logits with the first image only).  Each of the n_groups heads is
 * soft-maxed over its g_k+2 logits, the last column dropped, the arg-max over columns 1..g_k taken as a
 * GROUP-LOCAL label; all n_groups*n_pair rows are merged and sorted by triple score; row probabilities are
 * scattered into n_rel_cls-wide rows at columns [0] + {c : incre_idx_list[c] == k+1}.
 * This is veto_postprocess_groups_batch (below) with n_img = 1 and experts_per_group = 1: the same kernels, limits (n_rel_cls <= 256
 * and n_groups <= 16 among them) and refusals; the row limit's message reads "n_groups * n_pair = ... exceeds 16384". */
typedef struct veto_post_meet_args {
  int32_t struct_size;
  int32_t n_obj, n_pair, n_groups;
  int32_t n_rel_cls, n_obj_cls;
  const float* const* group_logits;   /* HOST array of n_groups device pointers [n_pair, group_widths[k]] */
  const int32_t* group_widths;        /* HOST array [n_groups]: g_k + 2 */
  const int32_t* incre_idx_list;      /* HOST array [n_rel_cls]: 1-based group of each class, 0 = background */
  const float* obj_logits;            /* device [n_obj, n_obj_cls]; NULL (sgdet): obj_scores / obj_pred are inputs */
  const int64_t* rel_pairs;           /* device [n_pair, 2] */
  float* obj_scores;                  /* out device [n_obj] */
  int64_t* obj_pred;                  /* out device [n_obj] */
  float* rel_prob_sorted;             /* out device [n_groups*n_pair, n_rel_cls] */
  int64_t* rel_pairs_sorted;          /* out device [n_groups*n_pair, 2] */
  int64_t* rel_labels_sorted;         /* out device [n_groups*n_pair] (group-local labels, as the reference) */
  float* triple_sorted;               /* optional out device [n_groups*n_pair] */
} veto_post_meet_args_t;

/* workspace: veto_postprocess_workspace_bytes(n_groups * n_pair, n_rel_cls) */
int veto_postprocess_meet(void* stream, const veto_post_meet_args_t* args, void* workspace, size_t workspace_bytes);

/* EXPERT_GROUP voting branch (ENSEMBLE_LEARNING.EXPERT_GROUP True, the defaults.py:864 default),
 * inference.py:93-283, for ONE image: every group has three expert heads ('group_<k>1..3'); a pair's row
 * for group k is kept when two experts ('C', consensus) or all three ('U', unanimous) pick the same
 * class; kept rows carry the averaged score / probabilities of the agreeing experts.  Outputs are sized
 * for n_groups*n_pair rows; the first *kept_count rows (score order) are the result, the rest is padding.
 * This is veto_postprocess_groups_batch (below) with n_img = 1 and experts_per_group = 3: the same kernels, limits (n_rel_cls <= 256
 * and n_groups <= 16 among them) and refusals. */
typedef struct veto_post_vote_args {
  int32_t struct_size;
  int32_t n_obj, n_pair, n_groups;
  int32_t n_rel_cls, n_obj_cls;
  int32_t voting;                     /* 0 = 'C' (two of three agree), 1 = 'U' (all agree): ENSEMBLE_LEARNING.VOTING */
  int32_t reserved0;
  const float* const* expert_logits;  /* HOST array of 3*n_groups device pointers, [3*k + e] = 'group_<k><e+1>' */
  const int32_t* group_widths;        /* HOST array [n_groups]: g_k + 2 */
  const int32_t* incre_idx_list;      /* HOST array [n_rel_cls] */
  const float* obj_logits;            /* device [n_obj, n_obj_cls]; NULL (sgdet): obj_scores / obj_pred are inputs */
  const int64_t* rel_pairs;           /* device [n_pair, 2] */
  float* obj_scores;                  /* out device [n_obj] */
  int64_t* obj_pred;                  /* out device [n_obj] */
  float* rel_prob_sorted;             /* out device [n_groups*n_pair, n_rel_cls] */
  int64_t* rel_pairs_sorted;          /* out device [n_groups*n_pair, 2] */
  int64_t* rel_labels_sorted;         /* out device [n_groups*n_pair] (group-local labels) */
  float* triple_sorted;               /* optional out device [n_groups*n_pair]; -1 marks padding rows */
  int32_t* kept_count;                /* out device [1] */
} veto_post_vote_args_t;

/* workspace: veto_postprocess_workspace_bytes(n_groups * n_pair, n_rel_cls) */
int veto_postprocess_vote(void* stream, const veto_post_vote_args_t* args, void* workspace, size_t workspace_bytes);

/* The MEET merge (experts_per_group 1) and the EXPERT_GROUP vote (experts_per_group 3) for a WHOLE ragged batch: image i gets exactly
 * what this call (or veto_postprocess_meet / veto_postprocess_vote) returns for image i alone, bit for bit, in at most four launches per call
 * (object scores, group scores, one sort workgroup per image, gather) whatever n_img and n_groups.
 * Row layout of the four relation outputs (n_groups * n_pair rows, P_i = pairs of image i): image i owns the contiguous block of
 * n_groups * P_i rows that starts at row n_groups * img_pair_offset[i].  Before the sort a block is ordered (group, pair) -- row
 * k * P_i + p -- as the one-image merged list, and it is sorted by (score descending, that index ascending).  Vote: the first
 * kept_count[i] rows of block i are the result; rows kept_count[i] .. of a block are padding with unspecified content.
 * The group heads are batch-wide: row p of every head is pair p of the concatenated pair list.
 * Refused before any launch: n_groups * P_i > 16384 (the message names the image), a group width outside 3..105 or not its class
 * count + 2, n_rel_cls > 256, n_groups > 16, voting not 0 / 1, n_groups * n_pair beyond int32, pairs_per_image that do not add up to
 * n_pair or whose maximum is not max_pairs_per_image, null pointers, a workspace below
 * veto_postprocess_workspace_bytes(n_groups * n_pair, n_rel_cls). */
typedef struct veto_post_groups_batch_args {
  int32_t struct_size;
  int32_t n_img, n_obj, n_pair;       /* images; objects and pairs over the batch */
  int32_t n_groups, experts_per_group;/* experts_per_group: 1 = MEET merge, 3 = expert vote */
  int32_t n_rel_cls, n_obj_cls;
  int32_t voting;                     /* vote: 0 = 'C', 1 = 'U'; merge: 0 */
  int32_t max_pairs_per_image;        /* host-side maximum of pairs_per_image; n_groups * max_pairs_per_image <= 16384 */
  const float* const* head_logits;    /* HOST array of experts_per_group * n_groups device pointers, [experts_per_group * k + e],
                                         each [n_pair, group_widths[k]] */
  const int32_t* group_widths;        /* HOST array [n_groups]: g_k + 2 */
  const int32_t* incre_idx_list;      /* HOST array [n_rel_cls]: 1-based group of each class, 0 = background */
  const int32_t* pairs_per_image;     /* HOST array [n_img]: P_i >= 0, the differences of img_pair_offset */
  const float* obj_logits;            /* device [n_obj, n_obj_cls]; NULL (sgdet): obj_scores / obj_pred are inputs */
  const int64_t* rel_pairs;           /* device [n_pair, 2] image-local, images concatenated */
  const int32_t* img_obj_offset;      /* device [n_img + 1] */
  const int32_t* img_pair_offset;     /* device [n_img + 1] */
  float* obj_scores;                  /* out device [n_obj] */
  int64_t* obj_pred;                  /* out device [n_obj] */
  float* rel_prob_sorted;             /* out device [n_groups*n_pair, n_rel_cls] */
  int64_t* rel_pairs_sorted;          /* out device [n_groups*n_pair, 2] */
  int64_t* rel_labels_sorted;         /* out device [n_groups*n_pair] (group-local labels) */
  float* triple_sorted;               /* optional out device [n_groups*n_pair]; vote: -1 marks padding rows */
  int32_t* kept_count;                /* vote: out device [n_img]; merge: NULL */
} veto_post_groups_batch_args_t;

/* workspace: veto_postprocess_workspace_bytes(n_groups * n_pair, n_rel_cls) */
int veto_postprocess_groups_batch(void* stream, const veto_post_groups_batch_args_t* args, void* workspace, size_t workspace_bytes);

/* ---- sgdet: the relation head on the detector's own boxes (USE_GT_BOX False) ------------------------
 * veto_obj_decode: greedy class-aware NMS over softmax(logits), for a ragged batch (one workgroup per image).
 *   mode 0 = obj_prediction_nms (utils_relation.py:94-128) as the PostProcessor uses it (inference.py:410-429, the
 *            MEET branch :317-341 and the voting branch :123-147): prob[:, 0] = 0, a row keeps its first label;
 *   mode 1 = Ensemble.nms_per_cls (roi_relation_predictors.py:3855-3874), the MEET decoder's labels (:3776-3784):
 *            prob[:, 0] = -1, a re-picked row takes the new label.  Input: the labels of the one-hot; every row is
 *            built from the same two probabilities, so ties between rows are exact and go to the lower row.
 *   N times: (b, c) = first row-major arg-max; label; prob[j, c] = 0 where IoU(boxes_per_cls[b, c], boxes_per_cls[j, c])
 *   >= nms_thres (nms_overlaps, :56-92, TO_REMOVE 1); prob[b, :] = -1.
 *   obj_scores[i] = softmax(logits)[i, label_i] with the background column zeroed; boxes[i] = boxes_per_cls[i, label_i]. */
typedef struct veto_obj_decode_args {
  int32_t struct_size;
  int32_t n_img, n_obj, n_cls;        /* n_cls 151 (VG) / 201 (GQA); 2..1024 */
  int32_t max_obj_per_image;          /* host-side maximum of the per-image counts, 1..256 (DETECTIONS_PER_IMG) */
  int32_t mode;                       /* 0 = PostProcessor, 1 = MEET decoder */
  float nms_thres;                    /* TEST.RELATION.LATER_NMS_PREDICTION_THRES */
  int32_t reserved0;
  const float* logits;                /* device [n_obj, n_cls] ('predict_logits'); mode 0, and whenever obj_scores is wanted */
  const int64_t* labels;              /* device [n_obj] ('pred_labels'); mode 1 */
  const float* boxes_per_cls;         /* device [n_obj, n_cls, 4] xyxy ('boxes_per_cls') */
  const int32_t* img_obj_offset;      /* device [n_img + 1] */
  int64_t* obj_pred;                  /* out device [n_obj] */
  float* obj_scores;                  /* optional out device [n_obj] */
  float* boxes;                       /* optional out device [n_obj, 4]: the regressed boxes */
} veto_obj_decode_args_t;

size_t veto_obj_decode_workspace_bytes(int32_t n_obj, int32_t n_cls);
int veto_obj_decode(void* stream, const veto_obj_decode_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_prepare_test_pairs: RelationSampling.prepare_test_pairs (sampling.py:31-52) with detected boxes, per image:
 * every ordered pair i != j, AND boxlist_iou > 0 (boxlist_ops.py:54-89) when require_overlap (REQUIRE_BOX_OVERLAP), in
 * row-major order; above max_pairs the max_pairs best by scores[i] * scores[j], emitted in the total order
 * (quality desc, row-major index asc) = torch.sort(stable=True, descending=True); [[0, 0]] when no pair is left.
 * Image i writes rows img_out_offset[i] .. + counts[i]; its capacity must be min(max(n(n-1), 1), max_pairs). */
typedef struct veto_pair_args {
  int32_t struct_size;
  int32_t n_img, n_obj;
  int32_t max_obj_per_image;          /* 0..256 */
  int32_t max_pairs;                  /* MAX_PROPOSAL_PAIR, 1..4096 */
  int32_t require_overlap;
  const float* boxes;                 /* device [n_obj, 4] xyxy (the proposals' bbox) */
  const float* scores;                /* device [n_obj] ('pred_scores') */
  const int32_t* img_obj_offset;      /* device [n_img + 1] */
  const int32_t* img_out_offset;      /* device [n_img + 1] */
  int64_t* pairs;                     /* out device [img_out_offset[n_img], 2] */
  int32_t* counts;                    /* out device [n_img]: pairs written per image */
} veto_pair_args_t;

int veto_prepare_test_pairs(void* stream, const veto_pair_args_t* args);

/* ---- sgdet box decoder: what produces predict_logits / pred_labels / pred_scores / boxes_per_cls ------------------
 * veto_nms: pysgg._C.nms (csrc/cuda/nms.cu) for n_seg segments (one image x class, or one image x pyramid level) in ONE
 * launch, nothing copied to the host.  Semantics of the reference's GPU kernel:
 *   IoU = devIoU (nms.cu:13-21, +1 pixel convention, same operation order); a box is suppressed by an earlier kept box at
 *   IoU STRICTLY GREATER than `threshold` (nms.cu:60 -- the reference's CPU twin, nms_cpu.cpp:60, uses >=; the GPU
 *   results are what users have, so > it is); boxes are visited in the total order (score desc, index asc) -- the
 *   reference's sort is unstable, equal scores are decided here; keep = the kept indices, LOCAL to the segment, in
 *   ASCENDING index order (nms.cu:127-130) from keep[seg_offset[s]]; max_keep > 0 keeps the first max_keep of that
 *   ascending list (boxlist_ops.py:29-30), not the best-scoring ones; an empty segment gives count 0.
 * A segment may hold up to veto_nms_max_segment() = 6144 boxes (MODEL.RPN.PRE_NMS_TOP_N_TEST is 6000).  The host copy of the
 * offsets is what the sizes are checked against before anything is launched. */
typedef struct veto_nms_args {
  int32_t struct_size;
  int32_t n_box, n_seg;
  int32_t max_keep;                   /* <= 0: no cap */
  float threshold;
  int32_t reserved0;
  const float* boxes;                 /* device [n_box, 4] xyxy, 16-byte aligned */
  const float* scores;                /* device [n_box] */
  const int32_t* seg_offset;          /* device [n_seg + 1] */
  const int32_t* seg_offset_host;     /* HOST [n_seg + 1], the same values: 0 = first, non-decreasing, last = n_box */
  int64_t* keep;                      /* out device [n_box] */
  int32_t* counts;                    /* out device [n_seg] */
} veto_nms_args_t;

int veto_nms_max_segment(void);
int veto_nms(void* stream, const veto_nms_args_t* args);

/* veto_box_postprocess: the box head's PostProcessor.forward + filter_results (box_head/inference.py:51-238) for a batch.
 *   per proposal: softmax(class_logits); BoxCoder.decode (box_coder.py:62-95: reg_weights, dw / dh clamped at
 *   bbox_xform_clip, the - 1 on x2 / y2) of every class -- cls_agnostic: the LAST four regression columns for every class;
 *   clip_to_image(remove_empty=False): every coordinate clamped to [0, size - 1].
 *   per image x class j >= 1: candidates prob > score_thresh, veto_nms at nms_thresh, at most post_nms_per_cls_topn.
 *   per image: filter_duplicates -- a row survives when any class survived, score / label = its best surviving class (first
 *   column on ties), box = its box of that class, rows ascending (:191-211); else class-major, rows ascending, a row
 *   once per surviving class (:212-214).  With more than detections_per_img (> 0) detections: keep score >= the
 *   (count - detections_per_img + 1)-th smallest; ties at that value stay, as in the reference (:216-226).
 * Image i writes counts[i] rows from img_out_offset[i]; when its capacity img_out_offset[i + 1] - img_out_offset[i] is too
 * small nothing is written for it and counts[i] = -(rows needed).  The decoded [n_box, n_cls, 4] lives in the workspace. */
typedef struct veto_box_post_args {
  int32_t struct_size;
  int32_t n_img, n_box, n_cls;        /* n_cls 2..1024, background = class 0 */
  int32_t reg_cols;                   /* columns of box_regression: 4 * n_cls, or any multiple of 4 with cls_agnostic */
  int32_t cls_agnostic;               /* MODEL.CLS_AGNOSTIC_BBOX_REG */
  int32_t post_nms_per_cls_topn;      /* MODEL.ROI_HEADS.POST_NMS_PER_CLS_TOPN, <= 0: none */
  int32_t filter_duplicates;          /* MODEL.ROI_HEADS.NMS_FILTER_DUPLICATES */
  int32_t detections_per_img;         /* MODEL.ROI_HEADS.DETECTIONS_PER_IMG, <= 0: none */
  float score_thresh;                 /* MODEL.ROI_HEADS.SCORE_THRESH, >= 0 */
  float nms_thresh;                   /* MODEL.ROI_HEADS.NMS */
  float bbox_xform_clip;              /* log(1000 / 16) */
  float reg_weights[4];               /* MODEL.ROI_HEADS.BBOX_REG_WEIGHTS */
  const float* class_logits;          /* device [n_box, n_cls] */
  const float* box_regression;        /* device [n_box, reg_cols], 16-byte aligned */
  const float* proposals;             /* device [n_box, 4] xyxy, 16-byte aligned */
  const float* image_sizes;           /* device [n_img, 2]: (width, height) */
  const int32_t* img_offset;          /* device [n_img + 1]: proposals per image, at most veto_nms_max_segment() each */
  const int32_t* img_offset_host;     /* HOST copy, checked before anything is launched */
  const int32_t* img_out_offset;      /* device [n_img + 1] */
  int64_t* orig_inds;                 /* out device [img_out_offset[n_img]]: proposal row, local to the image */
  int64_t* pred_labels;               /* out device, same rows */
  float* pred_scores;                 /* out device */
  float* boxes;                       /* out device [.., 4], 16-byte aligned */
  float* boxes_per_cls;               /* optional out device [.., n_cls, 4] = decoded[orig_inds] */
  int32_t* counts;                    /* out device [n_img] */
} veto_box_post_args_t;

size_t veto_box_postprocess_workspace_bytes(int32_t n_box, int32_t n_cls, int32_t filter_duplicates);
int veto_box_postprocess(void* stream, const veto_box_post_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_rpn_proposals: RPNPostProcessor.forward (rpn/inference.py:78-183) for a batch of n_img images and n_lvl pyramid levels,
 * three launches (four in per-batch mode) whatever n_img and n_lvl are, nothing copied to the host.  The RPN head's outputs are
 * read in place: objectness[l] [n_img, A, H, W] logits, box_regression[l] [n_img, 4A, H, W], anchors[l] [A H W, 4] xyxy with
 * anchor (h W + w) A + a (permute_and_flatten, rpn/utils.py:10-14) whose regression of coordinate c is channel 4a + c.
 *   per image x level: the k = min(pre_nms_top_n, A H W) best anchors in the total order (logit desc, anchor index asc) -- one
 *   of the orders sigmoid().topk(sorted=True) may give; BoxCoder.decode (box_coder.py:62-95: reg_weights, dw / dh clamped at
 *   bbox_xform_clip, the - 1 on x2 / y2); every coordinate clamped to [0, size - 1]; candidates with x2 - x1 + 1 < min_size or
 *   y2 - y1 + 1 < min_size dropped (remove_small_boxes); veto_nms at nms_thresh over the rest, the first post_nms_top_n (> 0)
 *   survivors kept, best first.  nms_thresh <= 0: no NMS and no cap (boxlist_ops.py:22-23).
 *   per image, n_lvl > 1 (select_over_all_levels, :156-183): per_batch 0 -- the min(fpn_post_nms_top_n, count) best of all
 *   levels in the order (logit desc, level asc, rank asc); per_batch 1 (training with FPN_POST_NMS_PER_BATCH) -- one
 *   top-fpn_post_nms_top_n over the whole batch (ties: image, level, rank), each image keeping its members level-major, rank
 *   ascending.  n_lvl == 1: the level's survivors.
 * objectness out = 1 / (1 + exp(-logit)).  Image i writes counts[i] rows from img_out_offset[i]; when its capacity
 * img_out_offset[i + 1] - img_out_offset[i] is too small nothing is written for it and counts[i] = -(rows needed).
 * Limits, checked before anything is launched: n_lvl 1..VETO_RPN_MAX_LEVELS; pre_nms_top_n 1..veto_nms_max_segment() (the
 * reference default PRE_NMS_TOP_N_TRAIN = 12000 is above it, the VETO configuration's 6000 is not); per_batch 0 with
 * n_lvl > 1: the levels' survivor bounds (min(post_nms_top_n, k), or k without NMS or cap) add up to at most 8192; per_batch 1:
 * n_img <= 1024.  A level may hold up to 2^31 - 1 anchors. */
#define VETO_RPN_MAX_LEVELS 8
typedef struct veto_rpn_args {
  int32_t struct_size;
  int32_t n_img, n_lvl;
  int32_t pre_nms_top_n;              /* MODEL.RPN.PRE_NMS_TOP_N_{TRAIN,TEST} */
  int32_t post_nms_top_n;             /* MODEL.RPN.POST_NMS_TOP_N_*, <= 0: none */
  int32_t fpn_post_nms_top_n;         /* MODEL.RPN.FPN_POST_NMS_TOP_N_*, > 0 when n_lvl > 1 */
  int32_t per_batch;                  /* training && MODEL.RPN.FPN_POST_NMS_PER_BATCH */
  float nms_thresh;                   /* MODEL.RPN.NMS_THRESH */
  float min_size;                     /* MODEL.RPN.MIN_SIZE */
  float bbox_xform_clip;              /* log(1000 / 16) */
  float reg_weights[4];               /* (1, 1, 1, 1) */
  int32_t level_a[VETO_RPN_MAX_LEVELS];   /* HOST: anchors per location, height and width of every level */
  int32_t level_h[VETO_RPN_MAX_LEVELS];
  int32_t level_w[VETO_RPN_MAX_LEVELS];
  const float* objectness[VETO_RPN_MAX_LEVELS];      /* device [n_img, A, H, W] */
  const float* box_regression[VETO_RPN_MAX_LEVELS];  /* device [n_img, 4A, H, W] */
  const float* anchors[VETO_RPN_MAX_LEVELS];         /* device [A H W, 4] xyxy, 16-byte aligned */
  const float* image_sizes;           /* device [n_img, 2]: (width, height) */
  const int32_t* img_out_offset;      /* device [n_img + 1] */
  float* boxes;                       /* out device [img_out_offset[n_img], 4], 16-byte aligned */
  float* objectness_out;              /* out device, same rows */
  int32_t* level;                     /* out device: pyramid level of the row */
  int64_t* anchor_index;              /* out device: anchor index inside that level */
  int32_t* counts;                    /* out device [n_img] */
} veto_rpn_args_t;

/* reads the host fields of `args` only (n_img, n_lvl, pre_nms_top_n, level_a / level_h / level_w); 0 when they are out of range */
size_t veto_rpn_proposals_workspace_bytes(const veto_rpn_args_t* args);
int veto_rpn_proposals(void* stream, const veto_rpn_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_anchor_grid: AnchorGenerator.forward (rpn/anchor_generator.py:73-125) for n_lvl pyramid levels and n_img images, ONE launch
 * whatever n_img and n_lvl are (the contract allows two), no workspace, nothing copied to the host and nothing synchronised.
 *   anchors (grid_anchors, :73-95): every level in one buffer [sum_l A_l H_l W_l, 4] float32 xyxy, level l starting at row
 *   sum_{j<l} A_j H_j W_j.  Row (h W + w) A + a of a level is cell_anchors[l][a] + (w stride, h stride, w stride, h stride): the
 *   order of veto_rpn_proposals and veto_rpn_loss.  Bit-equal to the reference: its shifts are arange(0, W stride, stride) in
 *   float32, integers below 2^24 and so exact, and each coordinate is one float32 addition of a cell anchor and a shift, which is
 *   what the kernel computes (the product w stride is formed in int32 and converted, the sum is never contracted).  The cell
 *   anchors (generate_anchors, :220-289, float64 numpy rounded to float32) are the caller's, computed on the host.
 *   visibility (add_visibility_to, :97-110; optional): a byte plane [n_img, total]; byte (i, r) is
 *   x1 >= -t && y1 >= -t && x2 < width_i + t && y2 < height_i + t of row r, evaluated in float32 on the float32 anchors as the
 *   reference's tensor-scalar comparisons are (the sums width + t, height + t are formed in float32: exact for the integers a
 *   configuration holds); t = straddle_thresh < 0: every byte is 1 (:107-109) and image_sizes is not read.
 *   anchors == NULL with visibility given: the rows are read from anchors_in (a buffer an earlier call wrote) and only the
 *   plane is written -- the call of a caller that caches the anchors per grid shape.
 * Limits, checked on the host fields before anything is launched: n_lvl 1..VETO_RPN_MAX_LEVELS; A, H, W, stride >= 1;
 * (W - 1) stride and (H - 1) stride below 2^24; at most 1 048 576 rows in all (what veto_rpn_loss accepts per image); anchors or
 * visibility given; with visibility n_img 1..65535 and, for t >= 0, image_sizes; cell_anchors, anchors and anchors_in 16-byte
 * aligned.  Left out: the cell anchors themselves (host), and BoxLists (veto_amd.rpn.AnchorGenerator wraps the buffers). */
typedef struct veto_anchor_args {
  int32_t struct_size;
  int32_t n_img;                      /* rows of the visibility plane; not read when visibility is NULL */
  int32_t n_lvl;
  float straddle_thresh;              /* MODEL.RPN.STRADDLE_THRESH; < 0: every anchor is visible */
  int32_t level_a[VETO_RPN_MAX_LEVELS];   /* HOST: anchors per location, height, width and stride of every level */
  int32_t level_h[VETO_RPN_MAX_LEVELS];
  int32_t level_w[VETO_RPN_MAX_LEVELS];
  int32_t level_stride[VETO_RPN_MAX_LEVELS];
  const float* cell_anchors[VETO_RPN_MAX_LEVELS];   /* device [A, 4] xyxy, 16-byte aligned; not read when anchors is NULL */
  const float* image_sizes;           /* device [n_img, 2]: (width, height) */
  float* anchors;                     /* out device [total, 4], 16-byte aligned; NULL: read anchors_in instead */
  const float* anchors_in;            /* device [total, 4], 16-byte aligned; read only when anchors is NULL */
  uint8_t* visibility;                /* optional out device [n_img, total] */
} veto_anchor_args_t;

int veto_anchor_grid(void* stream, const veto_anchor_args_t* args);

/* veto_detect_relsample: RelationSampling.detect_relsample (sampling.py:109-176) with motif_rel_fg_bg_sampling (:179-309),
 * the training-time relation sampler on detected boxes, for a ragged batch (one workgroup per image).  Per image:
 *   ious = boxlist_iou(target, proposal) (TO_REMOVE 1); is_match = same label & iou > fg_thres; locating_match[p] = 1 if
 *   any target has iou > fg_thres.  Candidates: every ordered pair i != j, or 0 < boxlist_iou(p_i, p_j) < 1 with
 *   require_overlap (REQUIRE_BOX_OVERLAP); rows and columns of proposals labelled 0 cleared.
 *   Foreground, GT relations in nonzero(relation) order: (matches of h) x (matches of t), head-major, self-pairs removed,
 *   all of them removed from the candidates; above num_sample_per_gt_rel that many drawn without replacement with
 *   probability proportional to iou[h, p_h] * iou[t, p_t], in draw order (npr.choice).  binary_rel (symmetric, self
 *   entries included) gets (head matches) x (tail matches).  Above max_fg_per_image triplets, a uniformly random
 *   max_fg_per_image of them in random order.
 *   Background: num_neg = min(batch_size_per_image - n_fg, n_bg) of the window of the first 2 * num_neg remaining
 *   candidates by (pred_scores[s] * pred_scores[o] desc, row-major index asc), uniformly at random, in random order.
 *   No foreground and no background: two (0, 0, 0) rows.
 *   labels_all (with relation_non_masked, :160-167): for each triplet relation i before the cap, the label of
 *   nonzero(relation_non_masked)[i]; then zeros for the background rows.  counts[4 * img + 3] bit 0 reports an index i
 *   past the end of that list.
 * Randomness: a counter-based hash of (seed, image index, purpose, element): an image's rows depend only on the seed,
 * its index and its own inputs.  The draws follow the reference's distributions, not its RNG streams.
 * Rows: image i writes pairs / labels from row i * R, R = max(batch_size_per_image, 2), counts[4 * i] rows of them,
 * foreground first; labels_all from row img_rel_offset[i] * num_sample_per_gt_rel + i * R, counts[4 * i + 1] foreground
 * entries then counts[4 * i] - counts[4 * i + 2] zeros. */
typedef struct veto_detect_relsample_args {
  int32_t struct_size;
  int32_t n_img, n_prp, n_tgt;
  int32_t n_rel_cells;                /* sum of T_i^2: img_rel_offset[n_img] */
  int32_t max_prp_per_image;          /* host-side maxima of the per-image counts, 0..256 (DETECTIONS_PER_IMG) */
  int32_t max_tgt_per_image;          /* 0..256 */
  int32_t require_overlap;            /* MODEL.ROI_RELATION_HEAD.REQUIRE_BOX_OVERLAP */
  int32_t num_sample_per_gt_rel;      /* NUM_SAMPLE_PER_GT_REL, 1..16 */
  int32_t batch_size_per_image;       /* BATCH_SIZE_PER_IMAGE, 1..2048 */
  int32_t max_fg_per_image;           /* int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION), 0..batch_size_per_image */
  float fg_thres;                     /* MODEL.ROI_HEADS.FG_IOU_THRESHOLD */
  uint64_t seed;
  const float* prp_boxes;             /* device [n_prp, 4] xyxy */
  const int64_t* prp_labels;          /* device [n_prp] ('labels') */
  const float* prp_scores;            /* device [n_prp] ('pred_scores') */
  const float* tgt_boxes;             /* device [n_tgt, 4] xyxy */
  const int64_t* tgt_labels;          /* device [n_tgt] */
  const int64_t* relation;            /* device: image i [T_i, T_i] row-major from img_rel_offset[i] */
  const int64_t* relation_non_masked; /* optional, same layout; NULL: labels_all is not written */
  const int32_t* img_prp_offset;      /* device [n_img + 1] */
  const int32_t* img_tgt_offset;      /* device [n_img + 1] */
  const int32_t* img_rel_offset;      /* device [n_img + 1]: prefix sums of T_i^2 */
  const int32_t* img_binary_offset;   /* device [n_img + 1]: prefix sums of P_i^2 */
  int64_t* pairs;                     /* out device [n_img * R, 2] */
  int64_t* labels;                    /* out device [n_img * R] */
  int64_t* labels_all;                /* optional out device [n_rel_cells * num_sample_per_gt_rel + n_img * R] */
  int64_t* binary_rel;                /* out device: image i [P_i, P_i] from img_binary_offset[i] */
  float* locating_match;              /* out device [n_prp] */
  int32_t* counts;                    /* out device [n_img, 4]: rows, foreground before the cap, foreground kept, status */
} veto_detect_relsample_args_t;

size_t veto_detect_relsample_workspace_bytes(int32_t n_rel_cells, int32_t num_sample_per_gt_rel);
int veto_detect_relsample(void* stream, const veto_detect_relsample_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_gtbox_relsample: RelationSampling.gtbox_relsample (sampling.py:54-107), the training-time relation sampler on GT
 * boxes (predcls, sgcls), for a ragged batch (one workgroup per image, one launch).  Per image, n objects:
 *   Foreground candidates: the entries relation > 0 in row-major (torch.nonzero) order, label = the entry.  At most
 *   num_pos_per_img of them: all, in that order.  More: a uniformly random num_pos_per_img of them in random order.
 *   Background candidates: every ordered pair (i, j), i != j, whose relation[i, j] is not > 0.
 *   min(candidates, batch_size_per_image - foreground rows) of them, a uniformly random subset in random order, label 0.
 *   binary_rel: 1 at (head, tail) and (tail, head) of every entry relation > 0, before the cap.
 * Randomness: every candidate gets the upper 32 bits of a counter-based hash of (seed, image index, purpose, row-major
 * cell index); a random subset of size k is the k smallest (hash, cell index), written in ascending order.  An image's rows
 * depend only on the seed, its index and its own matrix.  The draws follow the reference's distributions, not its RNG
 * streams.
 * Rows: image i writes pairs / labels from row i * batch_size_per_image: counts[2 * i] foreground rows, then
 * counts[2 * i + 1] background rows.  No workspace; the call runs on `stream` and never synchronises. */
typedef struct veto_gtbox_relsample_args {
  int32_t struct_size;
  int32_t n_img;
  int32_t n_rel_cells;                /* sum of n_i^2: img_rel_offset[n_img] */
  int32_t max_obj_per_image;          /* host-side maximum of n_i, 0..256 */
  int32_t batch_size_per_image;       /* BATCH_SIZE_PER_IMAGE, 1..2048 */
  int32_t num_pos_per_img;            /* int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION), 0..batch_size_per_image */
  uint64_t seed;
  const int64_t* relation;            /* device: image i [n_i, n_i] row-major from img_rel_offset[i] */
  const int32_t* img_obj_offset;      /* device [n_img + 1]: prefix sums of n_i */
  const int32_t* img_rel_offset;      /* device [n_img + 1]: prefix sums of n_i^2 */
  int64_t* pairs;                     /* out device [n_img * batch_size_per_image, 2] */
  int64_t* labels;                    /* out device [n_img * batch_size_per_image] */
  int64_t* binary_rel;                /* out device: image i [n_i, n_i] from img_rel_offset[i] */
  int32_t* counts;                    /* out device [n_img, 2]: foreground rows, background rows */
} veto_gtbox_relsample_args_t;

int veto_gtbox_relsample(void* stream, const veto_gtbox_relsample_args_t* args);

/* veto_box_match: the matching half of FastRCNNSampling (roi_heads/box_head/sampling.py:34-82 and :118-133) for a ragged
 * batch, one launch.  Per proposal of image i: the maximum of boxlist_iou(target, proposal) (TO_REMOVE 1, fp32, bit-equal to
 * the reference's matrix, which is never stored) over the image's GT boxes and the lowest GT index that reaches it; Matcher
 * (matcher.py:66-76, allow_low_quality_matches False): matched_idxs = that index when the maximum >= high_threshold, -2 when it
 * lies in [low_threshold, high_threshold), -1 below.
 *   labels, mode 0 (assign_label_to_proposals): tgt_labels of the matched box, 0 for every negative match.
 *   labels, mode 1 (prepare_targets): the same, but -2 gives -1 (ignored by the sampler).
 *   regression_targets (optional): BoxCoder.encode (box_coder.py:22-50) of the proposal against GT box max(matched_idxs, 0).
 *   matched_rows (optional): img_tgt_offset[i] + max(matched_idxs, 0), the row of that box in the concatenated targets.
 * Limits, checked on the host offsets before the launch: 1..256 GT boxes and 1..6144 proposals per image.  No workspace; the
 * call runs on `stream` and never synchronises. */
typedef struct veto_box_match_args {
  int32_t struct_size;
  int32_t n_img, n_prp, n_tgt;
  int32_t mode;                       /* 0: assign_label_to_proposals, 1: prepare_targets */
  float high_threshold;               /* MODEL.ROI_HEADS.FG_IOU_THRESHOLD */
  float low_threshold;                /* MODEL.ROI_HEADS.BG_IOU_THRESHOLD, <= high_threshold */
  float reg_weights[4];               /* MODEL.ROI_HEADS.BBOX_REG_WEIGHTS; read with regression_targets only */
  int32_t reserved0;
  const float* prp_boxes;             /* device [n_prp, 4] xyxy, 16-byte aligned */
  const float* tgt_boxes;             /* device [n_tgt, 4] xyxy, 16-byte aligned */
  const int64_t* tgt_labels;          /* device [n_tgt] */
  const int32_t* img_prp_offset;      /* device [n_img + 1] */
  const int32_t* img_tgt_offset;      /* device [n_img + 1] */
  const int32_t* img_prp_offset_host; /* HOST copies of the two offset arrays: the limits are checked on them */
  const int32_t* img_tgt_offset_host;
  int64_t* matched_idxs;              /* out device [n_prp] */
  int64_t* labels;                    /* out device [n_prp] */
  int64_t* matched_rows;              /* optional out device [n_prp] */
  float* regression_targets;          /* optional out device [n_prp, 4], 16-byte aligned */
} veto_box_match_args_t;

int veto_box_match(void* stream, const veto_box_match_args_t* args);

/* veto_box_subsample: BalancedPositiveNegativeSampler (balanced_positive_negative_sampler.py:37-66) and the
 * nonzero(pos | neg) of FastRCNNSampling.subsample (sampling.py:111-114) for a ragged batch, one workgroup per image, one
 * launch.  Per image: positives are labels >= 1, negatives labels == 0, everything else is ignored;
 * num_pos = min(positives, num_pos_per_img), num_neg = min(negatives, batch_size_per_image - num_pos).  A class above its
 * quota keeps a uniformly random subset of that size: the members with the smallest (hash, proposal index), hash = the upper
 * 32 bits of a counter-based hash of (seed, image index, class, proposal index).  An image's rows depend only on the seed,
 * its index and its own labels.  The draws follow the reference's distribution (randperm(m)[:k] as a set), not its RNG stream.
 * Rows: image i writes counts[i] = num_pos + num_neg proposal indices (inside the image, ascending) from
 * sampled_inds[i * batch_size_per_image].  Limits, checked before the launch: 1..6144 proposals per image,
 * batch_size_per_image 1..2048.  No workspace; never synchronises. */
typedef struct veto_box_subsample_args {
  int32_t struct_size;
  int32_t n_img, n_prp;
  int32_t batch_size_per_image;       /* MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE, 1..2048 */
  int32_t num_pos_per_img;            /* int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION), 0..batch_size_per_image */
  int32_t reserved0;
  uint64_t seed;
  const int64_t* labels;              /* device [n_prp]: the labels of veto_box_match, mode 1 */
  const int32_t* img_prp_offset;      /* device [n_img + 1] */
  const int32_t* img_prp_offset_host; /* HOST copy: the limits are checked on it */
  int64_t* sampled_inds;              /* out device [n_img, batch_size_per_image] */
  int32_t* counts;                    /* out device [n_img] */
} veto_box_subsample_args_t;

int veto_box_subsample(void* stream, const veto_box_subsample_args_t* args);

/* veto_rpn_loss: RPNLossComputation (rpn/loss.py:21-157) for a batch of n_img images over n_lvl pyramid levels: anchor matching,
 * fg/bg sampling, both losses and their gradients w.r.t. the RPN head's outputs.  Seven launches whatever n_img and n_lvl are, three
 * when only the per-anchor outputs are asked for; nothing is copied to the host and nothing synchronises.  The [n_gt, n_anchor] IoU
 * matrix is never stored and nothing is permuted or concatenated.  Levels as in veto_rpn_proposals: anchors[l] [A H W, 4] xyxy with
 * anchor (h W + w) A + a, shared by the images; an image's anchor index is the level's offset plus the index in the level (the
 * order of cat_boxlist, loss.py:104, and concat_box_prediction_layers, rpn/utils.py:17-45); n_anchor = the sum of A H W.
 *   Matching (match_targets_to_anchors, loss.py:42-54; matcher.py:42-112): per anchor the maximum of boxlist_iou(target, anchor)
 *   (TO_REMOVE 1, fp32, bit-equal to the reference's matrix) over the image's GT boxes and the lowest GT index that reaches it;
 *   matched_idxs = that index when the maximum >= high_threshold, -2 in [low_threshold, high_threshold), -1 below.  With
 *   allow_low_quality_matches (set_low_quality_matches_, :83-112) an anchor whose IoU with any GT j equals the largest IoU any
 *   anchor has with j gets its argmax back; a GT that overlaps no anchor (largest IoU 0) restores every anchor that has IoU 0
 *   with it, as the reference's equality mask does.
 *   labels (loss.py:65-79, generate_rpn_labels): 1 where matched_idxs >= 0, 0 where -1, then -1 where the anchor is not visible,
 *   then -1 where -2.  Visible (anchor_generator.py:97-110): x1 >= -straddle_thresh, y1 >= -straddle_thresh,
 *   x2 < width + straddle_thresh, y2 < height + straddle_thresh with the image's own size; straddle_thresh < 0: every anchor.
 *   regression_targets: BoxCoder.encode (box_coder.py:22-50) of the anchor against GT box max(matched_idxs, 0).
 *   Sampling (balanced_positive_negative_sampler.py:37-66), the convention of veto_box_subsample: positives are labels >= 1,
 *   negatives labels == 0; num_pos = min(positives, num_pos_per_img), num_neg = min(negatives, batch_size_per_image - num_pos);
 *   a class above its quota keeps the members with the smallest (hash, anchor index), hash = the upper 32 bits of a counter-based
 *   hash of (seed, image index, class, anchor index).  For one label vector, this call and veto_box_subsample pick the same rows
 *   from the same seed.  An image's rows depend only on the seed, its index and its own labels.  Image i writes counts[2 i] +
 *   counts[2 i + 1] anchor indices (inside the image, ascending) from sampled_inds[i * batch_size_per_image].
 *   Losses (loss.py:107-131), S = the sampled anchors of the batch, P its sampled positives: losses[0] = objectness_loss = the
 *   mean over S of max(x, 0) - x y + log1p(exp(-|x|)); losses[1] = box_loss = the sum over P and the four coordinates of
 *   smooth-L1 (layers/smooth_l1_loss.py: 0.5 d^2 / beta below beta, |d| - 0.5 beta from beta on) divided by S.  The logit of anchor
 *   (h W + w) A + a of level l is objectness[l][img, a, h, w], its deltas box_regression[l][img, 4 a + c, h, w].  The terms are
 *   evaluated in double from the fp32 inputs and summed in a fixed order: two calls give the same bits.  P = 0: box_loss 0;
 *   S = 0: both NaN (the mean of nothing).
 *   Gradients for an upstream gradient of 1, into tensors of the head outputs' own shapes, which the call fills itself:
 *   (sigmoid(x) - y) / S at the sampled logits, the smooth-L1 derivative / S at the sampled positives' deltas, 0 elsewhere.
 * The call stops after the last stage a requested output needs: losses or gradients -> all of it; else sampled_inds or counts ->
 * matching and sampling; else matching alone (prepare_targets).  At least one output must be given.
 * Limits, checked on the host fields before anything is launched: n_lvl 1..VETO_RPN_MAX_LEVELS; 1..256 GT boxes per image (an
 * empty image is refused with the reference's message); 1..1048576 anchors per image; batch_size_per_image 1..2048. */
typedef struct veto_rpn_loss_args {
  int32_t struct_size;
  int32_t n_img, n_lvl, n_tgt;
  int32_t batch_size_per_image;       /* MODEL.RPN.BATCH_SIZE_PER_IMAGE, 1..2048 */
  int32_t num_pos_per_img;            /* int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION), 0..batch_size_per_image */
  int32_t allow_low_quality_matches;  /* Matcher(..., allow_low_quality_matches): True in make_rpn_loss_evaluator */
  int32_t reserved0;
  float high_threshold;               /* MODEL.RPN.FG_IOU_THRESHOLD */
  float low_threshold;                /* MODEL.RPN.BG_IOU_THRESHOLD, <= high_threshold */
  float straddle_thresh;              /* MODEL.RPN.STRADDLE_THRESH; < 0: every anchor is visible */
  float reserved1;
  float reg_weights[4];               /* the RPN's BoxCoder weights, (1, 1, 1, 1) */
  double beta;                        /* smooth-L1 beta, 1 / 9 (loss.py:123) */
  uint64_t seed;
  int32_t level_a[VETO_RPN_MAX_LEVELS];   /* HOST: anchors per location, height and width of every level */
  int32_t level_h[VETO_RPN_MAX_LEVELS];
  int32_t level_w[VETO_RPN_MAX_LEVELS];
  const float* objectness[VETO_RPN_MAX_LEVELS];      /* device [n_img, A, H, W]; read by the loss stage only */
  const float* box_regression[VETO_RPN_MAX_LEVELS];  /* device [n_img, 4A, H, W]; read by the loss stage only */
  const float* anchors[VETO_RPN_MAX_LEVELS];         /* device [A H W, 4] xyxy, 16-byte aligned */
  float* d_objectness[VETO_RPN_MAX_LEVELS];          /* optional out device, the shape of objectness[l]; all levels or none */
  float* d_box_regression[VETO_RPN_MAX_LEVELS];      /* optional out device, the shape of box_regression[l]; with d_objectness */
  const float* image_sizes;           /* device [n_img, 2]: (width, height) */
  const float* tgt_boxes;             /* device [n_tgt, 4] xyxy, 16-byte aligned */
  const int32_t* img_tgt_offset;      /* device [n_img + 1] */
  const int32_t* img_tgt_offset_host; /* HOST copy: the limits are checked on it */
  float* losses;                      /* out device [2]: objectness_loss, box_loss; required with the gradients */
  float* labels;                      /* optional out device [n_img, n_anchor] */
  int64_t* matched_idxs;              /* optional out device [n_img, n_anchor] */
  float* regression_targets;          /* optional out device [n_img, n_anchor, 4], 16-byte aligned */
  int64_t* sampled_inds;              /* optional out device [n_img, batch_size_per_image] */
  int32_t* counts;                    /* optional out device [n_img, 2]: sampled positives, sampled negatives */
} veto_rpn_loss_args_t;

/* reads the host fields of `args` only (n_img, n_lvl, n_tgt, batch_size_per_image, level_a / level_h / level_w); 0 when they are
 * out of range */
size_t veto_rpn_loss_workspace_bytes(const veto_rpn_loss_args_t* args);
int veto_rpn_loss(void* stream, const veto_rpn_loss_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_box_loss: FastRCNNLossComputation.__call__ (roi_heads/box_head/loss.py:42-84) over the n_rows proposals that
 * FastRCNNSampling.subsample kept, all images concatenated: both losses and their gradients w.r.t. the predictor's outputs.  Two
 * launches whatever n_rows, n_cls and the number of images; nothing is copied to the host and nothing synchronises (the
 * reference's nonzero over labels > 0 reads its count back).  class_logits and box_regression are read in place through a row
 * stride in elements (ld_logits, ld_reg), so a column slice of a wider tensor needs no copy; the outputs are contiguous.
 *   losses[0] = classification_loss = F.cross_entropy(class_logits, labels): the mean over the rows of logsumexp(z) - z[y], the
 *   row maximum subtracted before any exponential.
 *   losses[1] = box_loss = the sum over the rows with y > 0 and the four coordinates of smooth-L1 with beta 1
 *   (layers/smooth_l1_loss.py: n = |input - target|; 0.5 n^2 below 1, n - 0.5 from 1 on) between box_regression[r, 4y .. 4y+3]
 *   (columns 4 .. 7 with cls_agnostic, MODEL.CLS_AGNOSTIC_BBOX_REG) and regression_targets[r], divided by n_rows -- by every
 *   row, not by the positives (loss.py:82).  No row with y > 0: exactly 0.
 *   The terms are evaluated in double from the fp32 inputs; each row leaves two doubles, and one workgroup folds them in row order
 *   (thread t the rows [t ceil(n_rows / 256), (t + 1) ceil(n_rows / 256)), then the 256 sums in thread order): two calls give
 *   the same bits.
 *   Gradients for an upstream gradient of 1, written by the same pass, every element of both outputs:
 *   d_class_logits[r, :] = (softmax(z) - onehot(y)) / n_rows; d_box_regression[r, :] = 0 except clamp(d, -1, 1) / n_rows at the
 *   row's four columns when y > 0 (d = input - target; d / beta and sign(d) agree at |d| = beta).
 *   NaN: n_rows = 0 gives both losses NaN (the mean of nothing; the reference gives NaN and 0 / 0).  A label outside [0, n_cls)
 *   reads nothing out of bounds; it makes both losses NaN and the row's two gradient rows NaN, other rows' gradients are
 *   unaffected (veto_ce_loss does the same for a label >= n_cls; torch raises).  That includes -100: the box head never
 *   produces an ignored row, so no label is an ignore_index here.
 * Limits, refused with a message before anything is launched: n_cls 2..1024 (the decoder's limit); n_rows 0..1048576;
 * n_reg_cols a multiple of 4 and >= 4 n_cls (>= 8 with cls_agnostic); ld_logits >= n_cls, ld_reg >= n_reg_cols; the gradient
 * outputs both or neither; regression_targets and the gradient outputs 16-byte aligned. */
typedef struct veto_box_loss_args {
  int32_t struct_size;
  int32_t n_rows;                     /* labels.numel(), 0..1048576 */
  int32_t n_cls;                      /* columns of class_logits, 2..1024 */
  int32_t n_reg_cols;                 /* columns of box_regression: 4 n_cls, or 8 with cls_agnostic (more are allowed) */
  int32_t cls_agnostic;               /* MODEL.CLS_AGNOSTIC_BBOX_REG */
  int32_t reserved0;
  int64_t ld_logits;                  /* row stride of class_logits in elements, >= n_cls */
  int64_t ld_reg;                     /* row stride of box_regression in elements, >= n_reg_cols */
  const float* class_logits;          /* device [n_rows, n_cls], read in place */
  const float* box_regression;        /* device [n_rows, n_reg_cols], read in place */
  const int64_t* labels;              /* device [n_rows] */
  const float* regression_targets;    /* device [n_rows, 4], 16-byte aligned */
  float* losses;                      /* out device [2]: classification_loss, box_loss */
  float* d_class_logits;              /* optional out device [n_rows, n_cls], contiguous, 16-byte aligned; with d_box_regression */
  float* d_box_regression;            /* optional out device [n_rows, n_reg_cols], contiguous, 16-byte aligned */
} veto_box_loss_args_t;

/* reads the host fields of `args` only (n_rows, n_cls, n_reg_cols, cls_agnostic, ld_logits, ld_reg); 0 when they are out of
 * range */
size_t veto_box_loss_workspace_bytes(const veto_box_loss_args_t* args);
int veto_box_loss(void* stream, const veto_box_loss_args_t* args, void* workspace, size_t workspace_bytes);

/* veto_optim_step: the optimizer side of a training iteration over every parameter tensor at once: clip_grad_norm
 * (pysgg/utils/checkpoint.py:180-219) and the step of the torch.optim.Adam that make_optimizer returns (solver/build.py:7-34,
 * one param group, so one lr and weight_decay, per tensor).  Four modes through this one entry point; nothing is copied to the
 * host and nothing synchronises in any of them (the reference's `if clip_coef < 1` reads the coefficient back).
 *   VETO_OPTIM_NORMS      the norms, the total and the coefficient; gradients are not written.                    1 launch
 *   VETO_OPTIM_CLIP       ... and every gradient is multiplied IN PLACE by the applied coefficient.  When that is exactly 1 the
 *                         gradients are not touched, as the reference skips its mul_.                              2 launches
 *   VETO_OPTIM_STEP       the Adam step alone; norms, total_norm, coef and max_norm are not read or written.        1 launch
 *   VETO_OPTIM_CLIP_STEP  norms, clip and step fused: gradients are READ-ONLY, each is scaled in registers by the
 *                         coefficient, which the step reads from device memory, and stays unscaled in memory.      2 launches
 *   The launch counts hold whatever n_tensors is; each call also makes one host-to-device copy of its tables (below).
 * The norm: a tensor is cut into chunks of VETO_OPTIM_CHUNK elements.  A chunk's sum of g^2 is taken by 256 threads, thread t the
 * 16-byte groups t, t + 256, ... (the elements t, t + 256, ... where the gradient is only 4-byte aligned, and of the tail) in
 * that order, every g converted to double BEFORE it is squared and every add in double; then a butterfly over each 64-lane wave
 * and the four wave sums in wave order.  A tensor's sum is its chunks' in chunk order; the total is the tensors' sums, thread t
 * the tensors [t ceil(n / 256), (t + 1) ceil(n / 256)), then the 256 sums in thread order.  No floating-point atomic: two calls
 * on the same inputs and addresses give the same bits.  norms[i] = sqrt(sum_i) and total_norm = sqrt(total), rounded to fp32
 * once; a tensor without a gradient or with no element has norms[i] = 0 and adds nothing.
 * The coefficient: max_norm / (total + 1e-6) in double, rounded to fp32 once (checkpoint.py:207); coef[0], the APPLIED
 * coefficient, is that value where it is < 1 and exactly 1.0f otherwise (checkpoint.py:208).
 * The step, per element (torch.optim.Adam's single-tensor form without amsgrad, maximize, capturable, differentiable); g', m and v
 * are formed in double from the fp32 operands and rounded to fp32 once each, the last line is fp32 arithmetic on those fp32 values:
 *   g' = coef g + weight_decay p   (the second term only where weight_decay != 0, as torch skips the add)
 *   m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2
 *   p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),  bc_i = 1 - beta_i^step
 *   1 - beta_i, lr / bc1 and sqrt(bc2) are formed on the host in double from this tensor's own step and rounded to fp32 once.
 *   `step` is the count INCLUDING this update (torch increments before it computes); the call does not change it.
 * A tensor whose grad is NULL takes no part: not in the norm, not updated, its state not read (param, exp_avg, exp_avg_sq may be
 * NULL and step may be anything).  numel 0 likewise.
 * Non-finite values follow the arithmetic; nothing is skipped or sanitised.  A NaN gradient makes its tensor's norm, the total
 * and the unrounded coefficient NaN; NaN < 1 is false, so the applied coefficient is exactly 1 and only that element's p, m, v
 * become NaN.  An Inf gradient makes the total Inf and the coefficient 0: that element's g' is Inf * 0 = NaN, every other
 * element's g' is weight_decay p (VETO_OPTIM_CLIP: the Inf gradient becomes NaN in memory, the others 0).
 * The tables: `tensors` is a HOST array.  The call copies what it needs of it into pinned staging memory that the library owns
 * before it returns, one buffer per call in flight (a buffer is used again only once the event recorded behind its call has
 * completed; more than 256 calls in flight wait for the oldest), so the caller may rewrite or free the array as soon as the
 * call returns, and gradient pointers may change from call to call.
 * Limits, refused with a message before anything is launched: n_tensors 1..4096; numel 0..2^31 - 1; at most 1 048 576 chunks in
 * all; an unknown mode; in the modes that clip, max_norm not > 0 (NaN included); in the modes that step, for a tensor with a
 * gradient and elements: step < 1, a missing param, exp_avg or exp_avg_sq, lr or eps or weight_decay negative or NaN, a beta
 * outside [0, 1); pointers not 4-byte aligned; in the modes that take norms, a missing norms, total_norm or coef. */
#define VETO_OPTIM_CHUNK 8192
#define VETO_OPTIM_NORMS 0
#define VETO_OPTIM_CLIP 1
#define VETO_OPTIM_STEP 2
#define VETO_OPTIM_CLIP_STEP 3

typedef struct veto_optim_tensor {
  float* param;                       /* device [numel] */
  const float* grad;                  /* device [numel], or NULL: the tensor takes no part */
  float* exp_avg;                     /* device [numel] */
  float* exp_avg_sq;                  /* device [numel] */
  int64_t numel;                      /* 0..2^31 - 1 */
  int64_t step;                       /* >= 1: the number of updates including this one */
  double lr, weight_decay, beta1, beta2, eps;
} veto_optim_tensor_t;

typedef struct veto_optim_args {
  int32_t struct_size;
  int32_t tensor_size;                /* sizeof(veto_optim_tensor_t) */
  int32_t n_tensors;                  /* 1..4096 */
  int32_t mode;                       /* VETO_OPTIM_* */
  double max_norm;                    /* > 0 in the modes that clip; in VETO_OPTIM_NORMS it only enters coef */
  const veto_optim_tensor_t* tensors; /* HOST [n_tensors]; reusable as soon as the call returns */
  float* norms;                       /* out device [n_tensors] */
  float* total_norm;                  /* out device [1] */
  float* coef;                        /* out device [1]: the applied coefficient */
} veto_optim_args_t;

/* reads the host fields of `args` and of its tensors (numel, grad); 0 when they are out of range */
size_t veto_optim_step_workspace_bytes(const veto_optim_args_t* args);
int veto_optim_step(void* stream, const veto_optim_args_t* args, void* workspace, size_t workspace_bytes);

/* ---- ROI feature extraction -------------------------------------------
 * VETOFeatureExtractor.forward -> Pooler.forward with cat_all_levels=False
 * (pysgg/modeling/roi_heads/box_head/roi_box_feature_extractors.py:75-121, pysgg/modeling/poolers.py:109-171)
 * over the legacy ROIAlign of pysgg/csrc/cuda/ROIAlign_cuda.cu:65-125 (layers/roi_align.py:12-61):
 * every ROI is pooled from ITS FPN level (LevelMapper, poolers.py:17-43) at that level's scale, the depth
 * map with the fixed pooler of level 2 (poolers.py:144-153; level 0 when there is one level).  One launch when every map is
 * float32 NCHW; otherwise one launch for the pyramid and one for the depth map.
 *
 * Map forms.  The maps are read in place in the form the four trailing fields name: an element type (level_dtype / depth_dtype:
 * VETO_ROI_F32, VETO_ROI_F16 (IEEE binary16), VETO_ROI_BF16) and a layout (level_layout / depth_layout: VETO_ROI_NCHW, dense
 * [n_img, C, H, W], or VETO_ROI_NHWC, dense [n_img, H, W, C] -- torch.channels_last).  All pyramid levels of one call share a type
 * and a layout; the depth map has its own pair.  Codes outside these ranges are refused with VETO_ERR_INVALID before any launch.
 * A call whose struct_size is offsetof(veto_roi_pool_args_t, level_dtype) -- the struct before these fields existed -- is
 * accepted and means float32 NCHW for every map.  Maps need only the alignment of their element type: the kernels use wider
 * accesses only where the row length in bytes and the base address allow them.
 * Promised: an element is widened to float32 (exact for both 16-bit types) and from there the arithmetic is that of the float32
 * NCHW form, in the same operation order without fused multiply-add.  So the pooled outputs of every form are bit-identical to
 * the call on the float32 NCHW copy of the same values (NaN and Inf travel the same way), and the float32 NCHW form is the code
 * it was before the fields existed.  The pooled outputs are float32, [n_roi, C, pooled, pooled], dense, whatever the map form. */
#define VETO_ROI_F32 0
#define VETO_ROI_F16 1
#define VETO_ROI_BF16 2
#define VETO_ROI_NCHW 0
#define VETO_ROI_NHWC 1

typedef struct veto_roi_pool_args {
  int32_t struct_size;
  int32_t n_levels;               /* 1..4 */
  int32_t n_img, n_roi;
  int32_t channels;               /* of the pyramid maps (256) */
  int32_t depth_channels;         /* of the depth map (256); ignored when depth_feat is NULL */
  int32_t pooled;                 /* POOLER_RESOLUTION (8); 1..16, with pooled * sampling_ratio <= 32 */
  int32_t sampling_ratio;         /* POOLER_SAMPLING_RATIO (2); 1..4 (0 = the adaptive grid: veto_roi_pool_adaptive below, only there) */
  const void* level_feat[4];      /* device [n_img, channels, level_h[l], level_w[l]] (or NHWC), finest level first */
  int32_t level_h[4];
  int32_t level_w[4];
  float level_scale[4];           /* POOLER_SCALES, e.g. 1/4, 1/8, 1/16, 1/32 */
  const void* depth_feat;         /* device [n_img, depth_channels, depth_h, depth_w] (or NHWC) or NULL */
  int32_t depth_h, depth_w;
  const float* rois;              /* device [n_roi, 5]: image index, x1, y1, x2, y2 (Pooler.convert_to_roi_format) */
  float* out_rgb;                 /* out device [n_roi, channels, pooled, pooled]        -> roi_features */
  float* out_depth;               /* out device [n_roi, depth_channels, pooled, pooled]  -> roi_depth_features */
  int32_t* out_levels;            /* optional out device [n_roi]: the level each ROI was pooled from */
  /* ---- the map forms (see above); absent from a struct of the earlier size, which means float32 NCHW ---- */
  int32_t level_dtype;            /* VETO_ROI_F32 / F16 / BF16: element type of every level_feat[l] */
  int32_t depth_dtype;            /* the same for depth_feat */
  int32_t level_layout;           /* VETO_ROI_NCHW / NHWC: layout of every level_feat[l] and of every level_grad[l] */
  int32_t depth_layout;           /* the same for depth_feat and depth_grad */
} veto_roi_pool_args_t;

int veto_roi_pool(void* stream, const veto_roi_pool_args_t* args);

/* Backward of veto_roi_pool (pysgg/csrc/cuda/ROIAlign_cuda.cu:178-262 RoIAlignBackwardFeature behind
 * layers/roi_align.py:27-44): `args` describes the forward call (shapes, scales, rois; its feature / output
 * pointers are not read), grad_rgb / grad_depth are the gradients of the two pooled tensors, level_grad[l] /
 * depth_grad receive the map gradients (same shapes as the maps; ZERO-INITIALISED BY THE CALLER, accumulated
 * with atomic adds, so the summation order -- not the result up to rounding -- varies from run to run;
 * veto_roi_pool_backward_ordered below fixes the order).
 * grad_depth / depth_grad may be NULL.
 * Both backward entry points read only the LAYOUT fields of `args`: the gradient maps are always float32, level_grad[l] in
 * level_layout and depth_grad in depth_layout (for a 16-bit map the caller casts afterwards); grad_rgb / grad_depth are float32
 * [n_roi, C, pooled, pooled] whatever the layout.  The terms are the same (g * w) / count per tap in both layouts. */
int veto_roi_pool_backward(void* stream, const veto_roi_pool_args_t* args, const float* grad_rgb, const float* grad_depth,
                           float* const* level_grad, float* depth_grad);

/* The ordered sibling (the "ordered mode" of the training path, see veto_train_opts_t.deterministic): the same arguments and the
 * same terms, gathered per map pixel instead of scattered, so the result is a pure function of the input bits, the library build
 * and the device model.  EVERY element of every gradient map is written by the call (a pixel nothing touches gets +0): the
 * caller zeroes nothing, and what the maps held before does not matter.
 * For the pixel (image b, channel c, y, x) of a map the result is the float32 sequential sum, starting from +0, of
 *     term = (g * w) / count       g = the pooled gradient of (ROI r, channel c, bin row ph, bin column pw),
 *                                  w = the tap's bilinear weight (hy*hx, hy*lx, ly*hx, ly*lx for taps 0..3), count = sampling_ratio^2,
 *                                  each operation rounded to float32 (no fused multiply-add), as in veto_roi_pool_backward,
 * over (r, ph, pw, iy, ix, tap) in lexicographic order, restricted to the valid samples' taps that land on (y, x) and -- for a pyramid
 * map -- to the ROIs of image b that the float32 LevelMapper of veto_roi_pool assigns to that level (the depth map takes every ROI of
 * image b).  Taps that coincide at the far edge (low index == high index) both count, in tap order.  pooled 9..16 changes nothing in
 * this: ph and pw run over 0 .. pooled - 1 in the same lexicographic order, whichever lane of veto_roi_pool computed the bin.
 * The order is stated per pixel and does not depend on the layout: the VETO_ROI_NHWC result is the VETO_ROI_NCHW result bit for bit,
 * permuted to [n_img, H, W, C], and every element is written in that layout too.
 * Not promised: the bits of veto_roi_pool_backward (whose order varies), equality across library builds or device models. */
int veto_roi_pool_backward_ordered(void* stream, const veto_roi_pool_args_t* args, const float* grad_rgb, const float* grad_depth,
                                   float* const* level_grad, float* depth_grad);

/* The adaptive sampling grid, POOLER_SAMPLING_RATIO = 0 (the default of pysgg/config/defaults.py; ROIAlign_cuda.cu:103-104): the
 * same pooling with a grid chosen per ROI.  Entry points of their own: the three above keep every check, message and bit.
 * `args` is the veto_roi_pool_args_t of veto_roi_pool at either accepted struct_size, with sampling_ratio == 0 REQUIRED.
 * Accepted: pooled 1..16 (there is no axis table, so no pooled * ratio condition), 1..4 levels with the float32 LevelMapper, the
 * depth map on its fixed level, out_levels, maps of VETO_ROI_F32 / F16 / BF16 in VETO_ROI_NCHW.
 * Refused with VETO_ERR_INVALID before any launch: VETO_ROI_NHWC in either layout field, sampling_ratio != 0, and everything
 * veto_roi_pool refuses (one shared argument check).
 * Per ROI and map, in float32 with every operation rounded (no fused multiply-add), for the y axis and the x axis separately:
 *     len = max(hi * scale - lo * scale, 1)      bin = len / pooled      g = (int)ceil(len / pooled)       (gh for y, gw for x)
 *     sample i of bin p lies at  v = (lo * scale + p * bin) + ((i + 0.5) * bin) / g,   i = 0 .. g - 1,
 * valid when !(v < -1 || v > size), with the clamping, tap indices and weights of veto_roi_pool.  Per bin and channel the sum starts
 * at +0 and adds  ((w0*v0 + w1*v1) + w2*v2) + w3*v3  of every valid sample, iy outer and ix inner, sequentially; an invalid sample
 * adds +0; the output is sum / (float)(gh * gw).  One bin's sum is never split, so the result is bit-identical to the reference's
 * kernel and, on ROIs whose grid is (g, g), g = 1..4, to veto_roi_pool at sampling_ratio = g.
 * Work bound: v is non-decreasing in i, so an axis of a bin has ONE contiguous range of valid samples; it is found by bisection on
 * the same float32 expression and only the product of the two ranges is visited.  The sample spacing bin / g lies in (0.5, 1] once
 * len >= pooled (g = 1 below that), so an axis holds at most 2 * size + 3 valid samples whatever the box: the work per ROI is bounded
 * by the map, not by the ROI's coordinates.  Outside the contract (the call still ends within that bound): ROIs with gh * gw >= 2^31,
 * whose count overflows in the reference too, non-finite coordinates, and coordinates so large (beyond 2^22 map pixels) that
 * float32 cannot tell neighbouring samples apart -- an axis range longer than 2 * size + 3 samples is treated as empty.
 * veto_roi_pool_adaptive_backward: the arguments and conventions of veto_roi_pool_backward (float32 NCHW gradient maps,
 * ZERO-INITIALISED BY THE CALLER, atomic adds, order not fixed); per valid sample and tap it adds (g * w) / count with
 * count = (float)(gh * gw), the terms of veto_roi_pool_backward.
 * Not built: an ordered (bit-repeatable) backward for the adaptive grid -- veto_roi_pool_backward_ordered refuses sampling_ratio 0
 * and the ordered mode must not fall back to this one --, VETO_ROI_NHWC maps in place, and rectangular outputs. */
int veto_roi_pool_adaptive(void* stream, const veto_roi_pool_args_t* args);
int veto_roi_pool_adaptive_backward(void* stream, const veto_roi_pool_args_t* args, const float* grad_rgb, const float* grad_depth,
                                    float* const* level_grad, float* depth_grad);

/* ---- relation evaluators -----------------------------------------------
 * evaluate_relation_of_one_image (pysgg/data/datasets/evaluation/vg/vg_eval.py:459-566) over the evaluator
 * classes of sgg_eval.py for the GT-box modes and sgdet (see reserved0 / pred_obj_offset): SGRecall (:121-187), SGNoGraphConstraintRecall (:195-255),
 * SGZeroShotRecall (:263-313), SGPairAccuracy (:322-369), SGMeanRecall (:377-466), SGNGMeanRecall (:470-546),
 * and their accumulation over the data set, K = 20 / 50 / 100.  Images are concatenated; the *_off arrays
 * are exclusive prefix sums.  For predcls pass the GT classes / boxes as the predicted ones and obj_scores = 1
 * (vg_eval.py:517-520).  Images without GT relations or without predictions contribute nothing (:474, :544). */
typedef struct veto_sgg_eval_args {
  int32_t struct_size;
  int32_t n_img;
  int32_t n_rel_cls;               /* 51 */
  int32_t n_zeroshot;
  float iou_thres;                 /* TEST.RELATION.IOU_THRESHOLD (0.5) */
  int32_t reserved0;               /* mode: 0 = GT boxes (predcls / sgcls), 1 = sgdet (SGPairAccuracy records nothing,
                                      sgg_eval.py:356: acc_rank is all 0x3fffffff and A@K is to be read as NaN) */
  const int32_t* gt_offset;        /* device [n_img + 1] GT relations */
  const int32_t* obj_offset;       /* device [n_img + 1] objects */
  const int32_t* pair_offset;      /* device [n_img + 1] predicted pairs */
  const int64_t* gt_rels;          /* device [sum G, 3]: subject, object (image-local), predicate  ('relation_tuple') */
  const int64_t* gt_classes;       /* device [sum N]  ('labels') */
  const float* gt_boxes;           /* device [sum N, 4] xyxy */
  const int64_t* pred_pairs;       /* device [sum P, 2] in ranking order  ('rel_pair_idxs') */
  const float* rel_scores;         /* device [sum P, n_rel_cls]           ('pred_rel_scores') */
  const int64_t* pred_classes;     /* device [sum N]  ('pred_labels') */
  const float* pred_boxes;         /* device [sum N, 4] */
  const float* obj_scores;         /* device [sum N]  ('pred_scores') */
  const int64_t* zeroshot;         /* device [n_zeroshot, 3]: subject class, object class, predicate */
  int32_t* gc_rank;                /* out device [sum G]: index of the first matching prediction, 0x3fffffff = none */
  int32_t* ng_rank;                /* out device [sum G]: the same in the no-graph-constraint top-100 list */
  int32_t* acc_rank;               /* out device [sum G]: the same, counted among the predictions on GT pairs */
  int32_t* zeroshot_flag;          /* out device [sum G] */
  int32_t* ng_rows;                /* out device [n_img, 100]: pair index of the i-th no-graph-constraint entry */
  int32_t* ng_cols;                /* out device [n_img, 100]: its predicate */
  int32_t* ng_count;               /* out device [n_img]: entries in that list (min(100, P * (n_rel_cls - 1))) */
  double* metrics;                 /* out device [18 + 6 * (n_rel_cls - 1) + 2]: R@20/50/100, ngR, zR, A, mR, ng-mR,
                                      per-class recall lists [2 kinds][3 K][n_rel_cls - 1], images evaluated,
                                      images with a zero-shot relation */
  const int32_t* pred_obj_offset;  /* device [n_img + 1] predicted objects (pred_classes / pred_boxes / obj_scores); NULL =
                                      obj_offset.  sgdet: the detector's boxes, whose count differs from the GT count
                                      (vg_eval.py:491-495).  A caller built against the struct without this field passes
                                      its shorter struct_size and gets NULL. */
} veto_sgg_eval_args_t;

size_t veto_sgg_eval_workspace_bytes(int32_t n_img, int32_t n_pair_total, int32_t n_gt_total, int32_t n_rel_cls);
int veto_sgg_eval(void* stream, const veto_sgg_eval_args_t* args, int32_t n_pair_total, int32_t n_gt_total,
                  void* workspace, size_t workspace_bytes);

/* The same accumulation over a whole split, from per-relation records that stay on the device.  veto_sgg_eval, called batch by
 * batch with gc_rank / ng_rank / acc_rank / zeroshot_flag pointing into caller-owned arrays at the batch's first row, leaves the
 * records; the caller adds each GT relation's predicate (column 2 of gt_rels) and keeps, per image, its GT-relation and pair
 * counts.  veto_sgg_eval_fold, once per split, restates sgg_eval.py:133-136, :209, :331-336, :420-466 over them; neither call
 * copies anything to the host, and the fold makes two launches whatever the number of images.
 *
 * Image i owns rows img_gt_offset[i] .. img_gt_offset[i+1]-1 (G of them) and is evaluated iff G > 0 and img_pair_count[i] > 0
 * (vg_eval.py:474, :548).  Ranks are compared as rank < K, K = 20 / 50 / 100; 0x3fffffff = no match.  Per evaluated image:
 *   R@K = #(gc_rank < K) / G,  ngR@K = #(ng_rank < K) / G,  zR@K = #(gc_rank < K and zeroshot) / #zeroshot if that is > 0,
 *   A@K hits = #(acc_rank < K), count = G,
 *   per predicate c in 1..n_rel_cls-1 with count_c > 0 relations in the image: #(rank < K among them) / count_c.
 * A GT predicate outside 1..n_rel_cls-1 counts for R, ngR, zR and A and for no class.  Over the split: R, ngR = the mean of the
 * quotients over the evaluated images, zR over those with a zero-shot relation (NaN without any), A@K = mean(hits) /
 * mean(counts) (NaN for mode 1), the per-class lists = the mean over the images that HAVE the class (0.0 for a class no image
 * has), mR / ng-mR = their sum in class order / (n_rel_cls - 1).
 *
 * Summation order, in double: workgroup b adds the images [b * images_per_chunk, (b+1) * images_per_chunk) in image order from
 * 0.0; the per-chunk sums are added in chunk order from 0.0.  No floating-point atomics: the same records give the same bits
 * whatever batches, buffer capacities or ranks produced them.  The per-image predicate counts live in LDS.
 *
 * Limits, refused before any launch: n_rel_cls 2..max_rel_cls (1024); n_img >= 0 and n_gt_total >= 0, so fewer than 2^31 images
 * and GT relations per split (n_img = 0 gives NaN recalls, mean recalls of 0.0 and counts of 0); the workspace, 256-byte aligned.
 * An image whose offsets leave 0..n_gt_total is treated as not evaluated. */
typedef struct veto_sgg_eval_fold_args {
  int32_t struct_size;
  int32_t n_img;
  int32_t n_rel_cls;
  int32_t mode;                    /* 0 = GT boxes (predcls / sgcls), 1 = sgdet: the A@K slots are NaN */
  int32_t n_gt_total;              /* rows of the five record arrays = img_gt_offset[n_img] */
  int32_t reserved0;
  const int32_t* img_gt_offset;    /* device [n_img + 1] */
  const int32_t* img_pair_count;   /* device [n_img] predicted pairs P of each image (NULL allowed when n_img = 0) */
  const int32_t* gt_predicate;     /* device [n_gt_total] each (NULL allowed when n_gt_total = 0) */
  const int32_t* gc_rank;
  const int32_t* ng_rank;
  const int32_t* acc_rank;
  const int32_t* zeroshot_flag;
  double* metrics;                 /* out device [18 + 6 * (n_rel_cls - 1) + 2], the layout of veto_sgg_eval_args_t.metrics */
  double* per_image;               /* out device [n_img, 12], optional: R@20/50/100, ngR, zR (NaN without a zero-shot relation),
                                      A hits / G (NaN for mode 1) of each image; all NaN for an image that is not evaluated */
} veto_sgg_eval_fold_args_t;

size_t veto_sgg_eval_fold_workspace_bytes(int32_t n_img, int32_t n_rel_cls);
int veto_sgg_eval_fold(void* stream, const veto_sgg_eval_fold_args_t* args, void* workspace, size_t workspace_bytes);

/* The sizes the fold is built with: images per workgroup (the unit of the summation order) and the largest n_rel_cls (either
 * pointer may be NULL). */
int veto_sgg_eval_fold_limits(int32_t* images_per_chunk, int32_t* max_rel_cls);

/* ---- detection (box mAP) evaluator ------------------------------------------------------------------
 * The "bbox" branch of do_vg_evaluation (pysgg/data/datasets/evaluation/vg/vg_eval.py:67-182): COCOeval.evaluate()
 * and accumulate() as that code drives them -- iouType 'bbox', no crowd boxes, the ten IoU thresholds
 * np.linspace(.5, .95, 10), the 101 recall thresholds np.linspace(0, 1, 101), maxDets [1, 10, 100], the area ranges
 * [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10], categories 1 .. n_cls-1 -- and summarize()'s twelve numbers.
 * A split is fed batch by batch: veto_det_eval_match appends one record per detection to three caller-owned device
 * buffers and adds the batch's non-ignored GT counts into a caller-owned table; veto_det_eval_accumulate, once per
 * split, sorts the records and forms precision / recall / stats.  Neither call copies anything to the host, and each
 * makes a number of launches that does not depend on the number of images, classes or records.
 *
 * Arithmetic is the reference's, in double: a detection's w, h are x2 - x1 + 1 rounded in float32 (BoxList.convert('xywh'))
 * and then widened, a GT box's are formed in double from its float32 coordinates (vg_eval.py:72-76); areas are w * h;
 * IoU is maskUtils.bbIou's (iw = min(dx+dw, gx+gw) - max(dx, gx), likewise ih, 0 if either is <= 0, else
 * i = iw*ih, u = dw*dh + gw*gh - i, i / u).  The thresholds and the area ranges are given as doubles so that they are numpy's bits.
 *
 * Per image the detections of each class are ordered by score descending, ties by index ascending (np.argsort(-score,
 * kind='mergesort')) and cut at 100.  For each (threshold, area range) COCOeval's greedy matching runs in that order over the
 * class's GT boxes, non-ignored ones (area inside the range) first, then ignored ones, each group in the given order: a GT box
 * already taken is skipped, the ignored group is not visited once a non-ignored match is held, a candidate needs
 * iou >= min(threshold, 1 - 1e-10) and then >= the best so far (of two equal IoUs the later GT box wins).  A detection
 * inherits its GT box's ignore flag; an unmatched detection whose area is outside the range is ignored.
 *
 * first_gt_id: vg_eval.py:78 numbers the annotations of the split from 0, and COCOeval tests the stored id for truth, so a
 * detection matched to annotation 0 occupies that GT box but counts as unmatched (a false positive, or ignored when its own
 * area is outside the range).  Pass the annotation id of THIS batch's first GT box: 0 for the first batch of a split
 * reproduces the reference, 1 gives the COCO-correct count; later batches add the GT boxes seen so far.
 *
 * Limits, refused before any launch: n_cls 2..1024; veto_det_eval_limits() GT boxes and detections per image (1024 and 1024);
 * row_offset + n_det below 2^31.  Preconditions: scores are finite; boxes are finite.  A label outside 1..n_cls-1 cannot be
 * seen from the host: such a box is left out of every count and *label_errors is incremented (a caller holding the labels
 * on the host refuses them there, as veto_amd.DetectionEvaluator does).  n_det = 0 with n_gt > 0 is allowed (the GT boxes are
 * counted, no record is written, the record pointers may be NULL).
 * Time: one workgroup matches an image, a thread per (class, threshold, area), so the boxes of one class are walked serially:
 * 0.2 ms per batch of 12 images x 80 detections; at the per-image limits with every box in ONE class (100 kept detections
 * against 1024 GT boxes) about 34 ms per batch, whatever the number of images (MI355X, profiles/det_eval_bench.txt).
 *
 * Record r = row_offset + det_offset[image] + (position in the image's (class, score desc, index) order):
 *   rec_key    class << 32 | ~order(score)   (order: larger score -> larger key, -0.0 and +0.0 share one);
 *              class 0 = not counted (beyond the 100 per (image, class), or a label out of range)
 *   rec_match  bit (threshold * 4 + area) = matched, bits 40..46 = rank within the (image, class) list
 *   rec_ignore bit (threshold * 4 + area) = ignored */
typedef struct veto_det_eval_match_args {
  int32_t struct_size;
  int32_t n_img;
  int32_t n_cls;                   /* object classes with the background (151) */
  int32_t n_gt;                    /* GT boxes of the batch */
  int32_t n_det;                   /* detections of the batch */
  int32_t reserved0;
  int64_t first_gt_id;             /* see above */
  int64_t row_offset;              /* records appended by the earlier batches of the split */
  double iou_thrs[10];             /* np.linspace(.5, .95, 10) */
  double area_rngs[8];             /* lo, hi of the four ranges */
  const int32_t* gt_offset;        /* device [n_img + 1] */
  const int32_t* det_offset;       /* device [n_img + 1] */
  const int32_t* gt_offset_host;   /* host copies of the two: the per-image limits are checked on them */
  const int32_t* det_offset_host;
  const float* gt_boxes;           /* device [n_gt, 4] xyxy */
  const int64_t* gt_labels;        /* device [n_gt] */
  const float* det_boxes;          /* device [n_det, 4] xyxy */
  const float* det_scores;         /* device [n_det], finite */
  const int64_t* det_labels;       /* device [n_det] */
  uint64_t* rec_key;               /* in/out device, at least row_offset + n_det rows each */
  uint64_t* rec_match;
  uint64_t* rec_ignore;
  int64_t* gt_counts;              /* in/out device [n_cls - 1, 4]: non-ignored GT boxes per (class, area range), added to
                                      (zeroed by the caller before the first batch) */
  int32_t* label_errors;           /* in/out device [1], optional: added to */
} veto_det_eval_match_args_t;

size_t veto_det_eval_match_workspace_bytes(int32_t n_img, int32_t n_gt, int32_t n_det);
int veto_det_eval_match(void* stream, const veto_det_eval_match_args_t* args, void* workspace, size_t workspace_bytes);

/* Once per split.  A device-wide stable LSD radix sort of the records by (class ascending, score descending) -- stability keeps
 * the append order among ties, i.e. image order and then the in-image order, which is what COCOeval's mergesort over its
 * concatenated per-image lists keeps -- then per (class k, area a, maxDets m) one pass over the class's records of rank < m with
 * running counts TP (matched, not ignored) and FP (not matched, not ignored) for the ten thresholds:
 *   rc = tp / npig,  pr = tp / (fp + tp + np.spacing(1)),
 *   recall[t,k,a,m] = the last rc (0 without records),
 *   precision[t,r,k,a,m] = max pr[i] over the i with rc[i] >= rec_thrs[r] (0 if none): COCOeval's backward envelope read at
 *   np.searchsorted(rc, rec_thrs, side='left').
 * Cells of a (class, area) without a non-ignored GT box stay -1.  stats[0..11] are summarize()'s: AP, AP50, AP75, APs, APm, APl,
 * AR@1, AR@10, AR@100, ARs, ARm, ARl, each the mean over the entries > -1 or -1 without any, summed in double in a fixed order;
 * recall50_100 is vg_eval.py:177's recall@100 at IoU 0.5.  n_rec = 0 is allowed.
 * Time: measured up to 400 000 records.  Each of the six radix passes scans its 256 * ceil(n_rec / 2048) histogram entries with a
 * single workgroup, so beyond a few million records the time of this call is unmeasured and dominated by that scan (about 2.7e8
 * entries a pass at the limit of 2^31). */
typedef struct veto_det_eval_accumulate_args {
  int32_t struct_size;
  int32_t n_cls;
  int64_t n_rec;                   /* records appended over the split, below 2^31 */
  double iou_thrs[10];
  double rec_thrs[101];            /* np.linspace(0, 1, 101) */
  const uint64_t* rec_key;         /* device [n_rec] each (not written) */
  const uint64_t* rec_match;
  const uint64_t* rec_ignore;
  const int64_t* gt_counts;        /* device [n_cls - 1, 4] */
  double* precision;               /* out device [10, 101, n_cls - 1, 4, 3] */
  double* recall;                  /* out device [10, n_cls - 1, 4, 3] */
  double* stats;                   /* out device [12] */
  double* recall50_100;            /* out device [1] */
} veto_det_eval_accumulate_args_t;

size_t veto_det_eval_accumulate_workspace_bytes(int64_t n_rec, int32_t n_cls);
int veto_det_eval_accumulate(void* stream, const veto_det_eval_accumulate_args_t* args, void* workspace, size_t workspace_bytes);

/* The sizes the evaluator is built with: GT boxes and detections per image, the records per step of the accumulate pass over a
 * class segment, the records per workgroup of the radix sort (any of the pointers may be NULL). */
int veto_det_eval_limits(int32_t* max_gt_per_image, int32_t* max_det_per_image, int32_t* scan_chunk, int32_t* sort_tile);

/* ---- measurement hooks (bench.py): per-kernel device time from hipEvents on `stream` ---------- */
int veto_profile_enable(veto_handle_t h, int32_t on);
/* Synchronises the recorded events; returns the number of distinct kernels. */
int veto_profile_collect(veto_handle_t h);
int veto_profile_entry(veto_handle_t h, int index, const char** name, double* total_ms, int64_t* launches,
                       double* flops_per_launch, double* bytes_per_launch);
int veto_profile_reset(veto_handle_t h);

/* ---- test hook: C[M,N] = A[M,K] . W[N,K]^T (+bias) through the production split-bf16 GEMM ------ */
int veto_debug_gemm(void* stream, const float* a, const float* w, const float* bias, float* c, int32_t m,
                    int32_t n, int32_t k, int32_t precision, void* workspace, size_t workspace_bytes);
size_t veto_debug_gemm_workspace_bytes(int32_t m, int32_t n, int32_t k);
/* ---- test hook: the same GEMM (3-term split-bf16) in its other forms: block-diagonal weights -- column tile j (192 columns) of C
 * multiplies only the k-steps (32 k's each) [(j / kb_tiles) * kb_steps, + kb_steps) of the rows, the rest of w is ignored;
 * kb_tiles = 0: dense -- and the output forms out_form 0 = fp32 [m, n], 1 = split rows (m x 2n bf16: per 32 columns 32 hi, then
 * 32 lo), 2 = 3-byte floats (m x 3n bytes: the top three bytes of the fp32 rounded to nearest even).  The folded last layer of the
 * predictor is built from these (roi_relation_predictors.py:4118-4131 -> model_veto.py:85-96 for the CLS query). */
int veto_debug_gemm_forms(void* stream, const float* a, const float* w, void* c, int32_t m, int32_t n, int32_t k,
                          int32_t kb_tiles, int32_t kb_steps, int32_t out_form, void* workspace, size_t workspace_bytes);

/* ---- test / measurement hook: the FeedForward block of one layer, x <- x + W2 . gelu(W1 . a + b1) + b2 (model_veto.py:137-143
 * with the residual of :21) on VETO_MIXED operands; mode 0 = two GEMM launches with the hidden activation in HBM, mode 1 = the
 * fused kernel (hidden activation stays on the CU).  a [m, 576] (the LayerNorm'ed rows), w1 [1152, 576], w2 [576, 1152],
 * x [m, 576] in / out.  flags & 1: rebuild the mixed operands in the workspace first.  Runs `reps` times; *ms_per_rep (host,
 * optional) = mean device time of one run.  ln_rows (optional, m x 2304 bytes): LayerNorm(x_out; ln_w, ln_b) as mixed activation
 * rows -- the next layer's PreNorm -- from the fused kernel's epilogue (mode 1) or a LayerNorm launch (mode 0). */
int veto_debug_ffn(void* stream, const float* a, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* x, int32_t m, int32_t mode, int32_t flags, int32_t reps, float* ms_per_rep, void* workspace,
                   size_t workspace_bytes, const float* ln_w, const float* ln_b, void* ln_rows);
size_t veto_debug_ffn_workspace_bytes(int32_t m);

/* ---- test / measurement hook: the attention out projection + residual, x <- x + a W^T + b (model_veto.py:96 `to_out`, :20) on
 * VETO_MIXED operands, optionally followed by LayerNorm rows (ln_rows, m x 2304 bytes of mixed activation rows: the FeedForward
 * PreNorm).  mode 0 = the GEMM launch (+ a LayerNorm launch), mode 1 = the full-row panel kernel (one launch).  a [m, 576],
 * w [576, 576], x [m, 576] in / out. */
int veto_debug_outproj(void* stream, const float* a, const float* w, const float* b, float* x, int32_t m, int32_t mode,
                       int32_t flags, int32_t reps, float* ms_per_rep, void* workspace, size_t workspace_bytes,
                       const float* ln_w, const float* ln_b, void* ln_rows);
size_t veto_debug_outproj_workspace_bytes(int32_t m);

/* ---- test / measurement hook: everything of one layer behind its attention (model_veto.py:96, :20-21, :125-143) on VETO_MIXED
 * operands: x1 = x + a Wo^T + bo, h = LayerNorm(x1; ln2_w, ln2_b), x = x1 + W2 gelu(W1 h + b1) + b2, and optionally ln_rows =
 * LayerNorm(x; ln_w, ln_b) as mixed activation rows (m x 2304 bytes).  mode 0 = the out-projection panel launch + the FeedForward
 * panel launch, mode 1 = one launch.  a [m, 576] (attention output), wo [576, 576], w1 [1152, 576], w2 [576, 1152], x in / out. */
int veto_debug_layer_tail(void* stream, const float* a, const float* wo, const float* bo, const float* ln2_w, const float* ln2_b,
                          const float* w1, const float* b1, const float* w2, const float* b2, float* x, int32_t m, int32_t mode,
                          int32_t reps, float* ms_per_rep, void* workspace, size_t workspace_bytes, const float* ln_w,
                          const float* ln_b, void* ln_rows);
size_t veto_debug_layer_tail_workspace_bytes(int32_t m);

/* ---- test / measurement hook: QKV projection + per-pair attention of a middle layer (model_veto.py:78-96) on VETO_MIXED operands:
 * a [19 n_pair, 576] = LayerNorm1 rows, wqkv [1728, 576] (no bias); out_rows receives the merged-heads attention output as mixed
 * activation rows (19 n_pair x 2304 bytes: the operand of the out projection).  mode 1 = ONE launch (qkv_attn_fused.hip: q / k / v never
 * reach memory), mode 0 = the two launches it replaces (QKV GEMM writing 3-byte q / k / v + the attention launch).  heads 8 or 6. */
int veto_debug_qkv_attn(void* stream, const float* a, const float* wqkv, int32_t n_pair, int32_t heads, int32_t mode, int32_t reps,
                        float* ms_per_rep, void* workspace, size_t workspace_bytes, void* out_rows);
size_t veto_debug_qkv_attn_workspace_bytes(int32_t n_pair);

/* ---- training losses and MEET expert sampling (partial) -------------------------
 * veto_ce_loss: nn.CrossEntropyLoss(weight)(logits[rows], labels), mean reduction -- the relation loss of
 * VETOPredictor.forward (roi_relation_predictors.py:4133, BETA_LOSS weights :4057-4068) and, on a row subset with
 * group-local labels, the per-group losses of Ensemble.forward (:3842-3846).  Writes the loss (device float) and,
 * if grad is non-NULL, d loss / d logits for the selected rows [n, n_cls].
 * Shift invariance: the loss term and the gradient's exponent are both formed as (z - max z) - logf(sum exp(z - max z)), the row
 * maximum and the log of the shifted sum kept apart, so the result does not depend on the offset of a row's logits (rows whose
 * logits differ by an exactly representable shift give the same gradient bits).  Labels: a negative label is an ignored row --
 * weight 0 in the loss, a gradient of exactly 0 whatever the weight sum (with every row ignored the loss is NaN, as torch's, and
 * the gradient all 0); a label >= n_cls makes the loss and its gradient row NaN; valid rows under a weight sum of 0 are NaN, as in
 * torch.  The workspace holds floats only and need not be 256-byte aligned. */
size_t veto_ce_loss_workspace_bytes(int32_t n);
int veto_ce_loss(void* stream, const float* logits, int64_t ld, const int64_t* labels, const float* weight,
                 const int64_t* rows, int32_t n, int32_t n_cls, float* loss, float* grad, void* workspace,
                 size_t workspace_bytes);

/* MEET expert sampling: the loop of VETOPredictor_MEET.forward in training (:3940-3969) followed by the per-group label
 * remap of Ensemble.forward (:3812-3821).  `words` are the next raw 32-bit outputs of Python's `random` generator
 * (MT19937), consumed exactly as random.randint / random.random would, relation by relation in index order;
 * *words_used tells the host how far to advance its generator (-1: the block was too short; the other outputs of such a
 * call are unspecified).  sample_rates is the [n_groups, n_cls] matrix of extra_function_utils.py:185-257 in double
 * precision.  random() takes two words, u = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53; randint(0, G-1) takes one word per
 * attempt, r = w >> (32 - G.bit_length()), again while r >= G.
 *
 * A foreground relation (label != 0) draws u = random() in every mode and joins groups 0..act-1 for the first act = G..1
 * with u <= sample_rates[act-1][label] or act < incre_idx_list[label] (no group if there is none).  A background relation
 * follows GCL_SETTING.ZERO_LABEL_PADDING_MODE:
 *   'rand_insert'   one word per attempt of randint(0, G-1); it joins the one drawn group
 *   'rand_choose'   two words, u = random(); u >= 0.4 (the double 0.4, inclusive): every group, otherwise none
 *   'all_include'   no word; every group
 * In each group the rows stand in ascending relation index, each at most once.
 *
 * veto_meet_sample is 'rand_insert' on one device thread.  veto_meet_sample_parallel computes the same bits for all three
 * modes: a relation's first word is a prefix sum of what the relations in front of it consume (fixed by the labels in
 * 'rand_choose' and 'all_include'; in 'rand_insert' a chain over the words, walked by one wave on bit masks held in
 * registers), every relation then decides by itself, and the lists are a stable compaction (no atomics: repeatable bit for
 * bit).  Limits of both: n >= 1, 1 <= n_groups <= 64, n_cls >= 2; the parallel call also takes n_words = 0 (words may then be
 * NULL) and needs a 256-byte aligned workspace. */
int veto_meet_sample(void* stream, const int64_t* labels, int32_t n, const uint32_t* words, int32_t n_words,
                     const int32_t* incre_idx_list, const int32_t* pos_in_group, const int32_t* group_size,
                     const double* sample_rates, int32_t n_groups, int32_t n_cls, int64_t* chosen,
                     int64_t* group_labels, int32_t* counts, int32_t* words_used);

enum veto_meet_pad_mode { VETO_MEET_RAND_INSERT = 0, VETO_MEET_RAND_CHOOSE = 1, VETO_MEET_ALL_INCLUDE = 2 };

typedef struct veto_meet_sample_args {
  int32_t struct_size;
  int32_t mode;                    /* enum veto_meet_pad_mode */
  int32_t n;                       /* relations */
  int32_t n_words;
  int32_t n_groups;
  int32_t n_cls;
  const int64_t* labels;           /* device [n] */
  const uint32_t* words;           /* device [n_words] */
  const int32_t* incre_idx_list;   /* device [n_cls]: 1-based group of each class */
  const int32_t* pos_in_group;     /* device [n_cls]: 1-based position of the class inside its group */
  const int32_t* group_size;       /* device [n_groups] */
  const double* sample_rates;      /* device [n_groups, n_cls] */
  int64_t* chosen;                 /* out device [n_groups, n]: row k holds counts[k] relation indices; the rest is not written */
  int64_t* group_labels;           /* out device [n_groups, n]: the group-local labels of those rows */
  int32_t* counts;                 /* out device [n_groups] */
  int32_t* words_used;             /* out device [1] */
} veto_meet_sample_args_t;

size_t veto_meet_sample_parallel_workspace_bytes(int32_t n, int32_t n_words);
int veto_meet_sample_parallel(void* stream, const veto_meet_sample_args_t* args, void* workspace, size_t workspace_bytes);

/* The sizes the parallel sampler is built with (any pointer may be NULL): relations per workgroup of the decision and the
 * compaction (tile), words per register window of the 'rand_insert' walk (window), relations per mask word (chunk). */
int veto_meet_sample_parallel_limits(int32_t* tile, int32_t* window, int32_t* chunk);

/* ---- training path: forward that keeps the activations + backward --------------
 * The backward of VETOPredictor.forward's computation graph (roi_relation_predictors.py:4074-4133, model_veto.py)
 * w.r.t. every parameter, for hard object labels (predcls, MEET), precise mode.  veto_forward_train runs all pairs in one pass, every layer on all 19 tokens, BatchNorm on batch
 * statistics (in->bn_batch_stats is mandatory), and leaves the activations in `workspace`
 * (veto_train_workspace_bytes, ~28 KB per token row and layer); veto_backward takes d loss / d logits
 * [n_pair, num_out] and writes d loss / d parameter for every state-dict tensor into `grads`, a flat float buffer of
 * veto_grad_floats(h) elements in which tensor i starts at veto_weight_offset(h, i) (buffers such as running
 * statistics get zeros).  Both calls must see the same inputs and workspace. */
/* Dropout of the training path (NULL = none): pos_embed's Dropout(0.1) (roi_relation_predictors.py:4042-4047), the
 * transformer's pos_drop (EMB_DROPOUT, model_veto.py:44,63) and the Dropout behind every attention out projection
 * (T_DROPOUT, model_veto.py:80-83).  Masks come from a counter-based hash of (seed, site, element index), recomputed in
 * the backward: the same opts must be given to both calls.  The masks are this library's own (the reference draws from
 * torch's generator), i.e. equal in distribution, not bit for bit.
 *
 * The contract, element by element (oracle/dropout.py restates it on the host; tests/test_train_dropout_gpu.py holds the step to it):
 *   y = keep ? x * (1.f / (1.f - p)) : 0 in float32; a site with p == 0 is the identity (no mask, no scale).
 *   keep(element) = (splitmix64(site_seed + index * 0x9E3779B97F4A7C15) >> 40) >= (uint32_t)(p * 16777216.0f),
 *   site_seed = seed + site * 0x632BE59BD9B4E019 (mod 2^64), with
 *     site 1      p_pos,  behind the ReLU of pos_embed:            element (n, k) of [n_obj, 128]  -> index n * 128 + k
 *     site 2      p_emb,  pos_drop on the tokens, after the positional embedding is added:
 *                                                                  element (row, col) of [n_pair * 19, 576] -> index row * 576 + col,
 *                                                                  row = pair * 19 + token, pair = the row of the batch's pair list
 *     site 3 + l  p_attn, on (attn_out Wo^T + bo) of layer l, before the residual add:          numbered as site 2
 *   The numbering is by token row whatever rows the implementation computes: the last layer runs on the CLS rows only, and its
 *   CLS row of pair p uses the elements of token row 19 p. */
typedef struct veto_train_opts {
  int32_t struct_size;
  float p_pos, p_emb, p_attn;
  uint64_t seed;
  /* veto_backward only, optional (NULL = not wanted): gradients of the loss w.r.t. the ROI maps, device [n_obj, 256, R, R]
   * (R = the handle's resolution) fp32 each.  The reference trains its depth backbone through roi_depth_features (tools/relation_train_net.py:166-170). */
  float* d_roi_rgb;
  float* d_roi_depth;
  /* Ordered mode (0 = off: the default kernels, workspace and bits).  Read only when struct_size covers it: a caller built against
   * the struct without this field passes the shorter struct_size and gets 0.  Both calls of a step must agree on it.
   *
   * With it on, every output of veto_forward_train and veto_backward (the logits, `grads`, d_roi_rgb / d_roi_depth) -- and of
   * veto_roi_pool_backward_ordered for the map gradients -- is a pure function of
   *     the input bits, the opts, the library build, and the device model:
   * repeated calls give the same bits whatever the workspace held before and whatever runs on other streams.
   * NOT promised: equality with the default path's bits, equality across library builds, equality across devices with another
   * compute-unit count.
   *
   * Every float32 sum of the backward that the default path leaves to atomics has a stated order instead:
   *   token assembly   dpatch[n, t, half] (and dlc, with the ReLU gate lc[subject] + lc[object] > 0 per term) = the float32 sequential
   *                    sum, from +0, of the token-gradient rows dx[p * 19 + t] over the pairs p, in ascending row of the batch's pair
   *                    list, whose subject (first half) / object (second half) is object n.  A pair listed twice counts twice; an object in
   *                    no pair gets +0.
   *   obj_embed        dE[label] = the float32 sequential sum, from +0, of the embedding-gradient rows over the object rows that carry the
   *                    label, in ascending row.
   *   LayerNorm        per block of 64 rows, the 8 row slots (slot s holds rows s, s + 8, ... of the block, added in that order) are added
   *                    in slot order 0..7 from +0 -- dgamma / dbeta and, where the kernel emits them, the column sums of rows 0..31 and
   *                    32..63 of the block; the per-block rows are folded in block order in double.
   *   weight gradients split j of the reduction writes its float32 tile to partial plane j; the planes are added in split order in
   *                    double and rounded once.  The split count is a function of the GEMM's shape (M, N, K) alone.
   *   ROI pooling      see veto_roi_pool_backward_ordered.
   * The workspace grows by the partial planes: size it with veto_train_workspace_bytes_opts. */
  int32_t deterministic;
} veto_train_opts_t;

/* veto_train_workspace_bytes: the default path's need (unchanged by the ordered mode's existence); veto_train_workspace_bytes_opts: the
 * need under `opts` (NULL = the default path) -- larger with opts->deterministic != 0. */
size_t veto_train_workspace_bytes(veto_handle_t h, int32_t n_obj, int32_t n_pair);
size_t veto_train_workspace_bytes_opts(veto_handle_t h, int32_t n_obj, int32_t n_pair, const veto_train_opts_t* opts);
size_t veto_grad_floats(veto_handle_t h);
int veto_weight_offset(veto_handle_t h, int index, size_t* offset_floats);
int veto_forward_train(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, void* workspace,
                       size_t workspace_bytes, float* out_logits);
int veto_backward(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts, void* workspace,
                  size_t workspace_bytes, const float* dlogits, float* grads);

/* ---- partial training: a step that computes only the gradients somebody reads, and honours eval-mode sub-modules -----------------
 * A plan rides beside the opts.  plan == NULL in any of the three entry points below is the entry point above it: same launches,
 * workspace and bits.  With a plan, veto_backward_plan launches nothing whose every output is unused:
 *   the chain  head -> layers L-1 .. 0 (fc2, fc1, LayerNorm2, out, attention, qkv, LayerNorm1) -> pos_embedding / cls_token
 *              -> patch projection and the map gradients -> location / class projections -> pos_embed.1, pos_embed.0, obj_embed
 *   is walked down to the deepest stage with a consumer (a trainable tensor, or d_roi_rgb / d_roi_depth) and ends there; a frozen
 *   Linear above that stage loses its weight-gradient GEMM, its zero-fill or fold and its bias sums, the deepest Linear with nothing
 *   below it its input-gradient GEMM as well; a heads-only plan is the head's weight and bias gradient alone.
 * Only the regions of `grads` that belong to trainable tensors are zeroed or written: a frozen tensor's region is left as the caller
 * gave it.  A computed gradient has the bits the unplanned step gives it in the ordered mode (the stated orders are per sum).
 * The forward keeps the activations of the layers the backward will read; the layers below the lowest consumer (the last layer
 * excepted: its buffers are the compact ones) alternate between two sets of buffers, so veto_train_workspace_bytes_plan shrinks with
 * the frozen prefix.  Both calls of a step must see the same plan: the forward stamps it with the workspace and the backward refuses
 * another one, as it refuses a plan on the workspace of a veto_forward_train and the other way round. */
typedef struct veto_train_plan {
  int32_t struct_size;
  /* pos_embed.0 (the BatchNorm) normalises with its running statistics: in->bn_batch_stats is neither needed nor written.  Refused
   * while pos_embed.0.weight or pos_embed.0.bias is trainable. */
  int32_t bn_eval;
  /* host array of veto_num_weights(h) bytes, indexed like veto_weight_info: nonzero = the tensor's gradient is wanted.  The
   * row-concatenated rel_out.weight / rel_out.bias take one flag each. */
  const uint8_t* trainable;
  /* host array [layers] of the dropout rates behind the attention out projections (site 3 + l), each in [0, 1); NULL: opts->p_attn
   * for every layer. */
  const float* p_attn_layer;
  /* nonzero: veto_backward_plan will be given opts->d_roi_rgb and / or opts->d_roi_depth, so the chain runs down to the patch
   * projection whatever is frozen (the pointers themselves are read by the backward only; asking for them there with 0 here is
   * refused). */
  int32_t d_roi;
  /* nonzero: the frozen-fused step (opt-in; 0 leaves every launch, workspace size and bit as it was).  The frozen region -- the
   * prelude (pair indices, object side, patch GEMM, token assembly) and layers 0 .. k-1, k the lowest layer with a trainable tensor
   * (k = layers when only rel_out.* is trainable) -- is the inference forward: veto_forward's stages in the handle's own precision,
   * chunk by chunk, on operands that are rebuilt per changed tensor (veto_load_weights).
   *   k == layers: the whole forward is veto_forward's (logits bit-equal to it); the CLS rows [n_pair, 576] stay in the workspace
   *                and the backward is the head's weight and bias gradient.
   *   k <  layers: behind layer k-1's tail the chunk's fp32 residual rows are copied to the buffer the training forward of layer k
   *                reads; layers k .. L-1 and the head run on the training path as under the same plan without this flag (saved
   *                activations, the step seed's dropout masks in those layers, the plain last layer).
   * The backward is the planned step's: it ends at layer k.  The workspace holds the inference forward's regions, the hand-off or CLS
   * rows and the saved activations of layers >= k.
   * Refused (VETO_ERR_INVALID by the forward and the backward, 0 by the size query, before any launch): a trainable tensor inside
   * the prelude; k == 0; bn_eval == 0; d_roi != 0; a non-zero opts->p_pos or opts->p_emb, or a non-zero attention dropout rate
   * in a layer < k; a VETO_FAST handle (its logit error is above the 1e-3 bar); VETO_X_F24=1.  Both calls of a step must agree on the
   * flag as on the rest of the plan. */
  int32_t frozen_fused;
} veto_train_plan_t;

size_t veto_train_workspace_bytes_plan(veto_handle_t h, int32_t n_obj, int32_t n_pair, const veto_train_opts_t* opts,
                                       const veto_train_plan_t* plan);
int veto_forward_train_plan(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts,
                            const veto_train_plan_t* plan, void* workspace, size_t workspace_bytes, float* out_logits);
int veto_backward_plan(veto_handle_t h, void* stream, const veto_inputs_t* in, const veto_train_opts_t* opts,
                       const veto_train_plan_t* plan, void* workspace, size_t workspace_bytes, const float* dlogits, float* grads);

/* ---- test hook: dw[N,K] = dy[M,N]^T . x[M,K], the weight-gradient GEMM (reduction over the M rows) through the
 * production split-bf16 kernel in its split-K / atomic-add form.  k must be a multiple of 192; k_splits 0 = auto. */
int veto_debug_wgrad(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k,
                     int32_t k_splits, void* workspace, size_t workspace_bytes);
size_t veto_debug_wgrad_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t k_splits);
/* The ordered form of the same GEMM: split j writes partial plane j (inside the workspace; every slot that is read is written by the
 * call), the planes are folded in split order.  Same arguments; the workspace is larger by k_splits planes of [n, k] fp32. */
int veto_debug_wgrad_ordered(void* stream, const float* dy, const float* x, float* dw, int32_t m, int32_t n, int32_t k,
                             int32_t k_splits, void* workspace, size_t workspace_bytes);
size_t veto_debug_wgrad_ordered_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t k_splits);

/* ---- test hooks: backward building blocks of the transformer (chained by veto_backward) ----------------------
 * veto_debug_attention_backward: qkv, dqkv device [n_pair*19, 1728], dout device [n_pair*19, 576]   (model_veto.py:85-96)
 * veto_debug_layernorm_backward: x, dy, dx device [rows, 576] (dres optional, added to dx), gamma [576],
 *                                dgamma_dbeta device [2, 576]; workspace of veto_debug_layernorm_backward_workspace_bytes
 * veto_debug_gelu_backward:      dpre = dh * gelu'(pre), n elements (n % 4 == 0)                       (model_veto.py:140)
 * veto_debug_column_sums:        out[c] = sum_r dy[r, c] (bias gradients); workspace 256 * n_cols floats */
int veto_debug_attention_backward(void* stream, const float* qkv, const float* dout, float* dqkv, int32_t n_pair, int32_t heads);
size_t veto_debug_layernorm_backward_workspace_bytes(int32_t rows);
int veto_debug_layernorm_backward(void* stream, const float* x, const float* dy, const float* gamma, const float* dres,
                                  float* dx, float* dgamma_dbeta, int32_t rows, void* workspace, size_t workspace_bytes);
int veto_debug_gelu_backward(void* stream, const float* pre, const float* dh, float* dpre, size_t n);
int veto_debug_column_sums(void* stream, const float* dy, int64_t ld, int32_t rows, int32_t n_cols, float* out,
                           void* workspace, size_t workspace_bytes);

/* ---- test hooks: the same blocks in the forms veto_backward runs ------------------------------------------------
 * veto_debug_attention_backward_forms: `flags` selects
 *   VETO_ATTN_BWD_CLS_ONLY   the last layer's form: dout is compact [n_pair, 576] (the CLS query's row); dq of token rows 1..18 is
 *                            written as zero
 *   VETO_ATTN_BWD_QKV_F24    qkv holds 3-byte floats (the top three bytes of the fp32 value rounded to nearest even, low address
 *                            first; rows of 1728 x 3 bytes); head widths 72 and 96 only.  qkv_unpacked (optional, fp32
 *                            [n_pair*19, 1728]) receives the values the kernel sees
 *   VETO_ATTN_BWD_SPLIT_OUT  dqkv is written as split rows instead of fp32: per row 2 x 1728 bf16, in blocks of 32 columns
 *                            [hi(c0..c0+31) | lo(c0..c0+31)], value = hi + lo
 * veto_debug_layernorm_backward_split: veto_debug_layernorm_backward that also writes what the Linear behind the LayerNorm takes:
 *   split_rows [rows, 2 x 576] bf16 (layout above) of dx with the dropout mask of site drop_seed applied (element (r, c) has index
 *   r * 576 + c; kept iff the top 24 bits of its splitmix64 hash are >= drop_thresh = p * 2^24, scaled by drop_scale; 0 = no mask),
 *   and col_partials [veto_debug_layernorm_backward_col_partial_rows(rows), 576]: the column sums of those rows per 32 rows. */
#define VETO_ATTN_BWD_CLS_ONLY 1u
#define VETO_ATTN_BWD_QKV_F24 2u
#define VETO_ATTN_BWD_SPLIT_OUT 4u
int veto_debug_attention_backward_forms(void* stream, const void* qkv, const float* dout, void* dqkv, float* qkv_unpacked,
                                        int32_t n_pair, int32_t heads, uint32_t flags);
int32_t veto_debug_layernorm_backward_col_partial_rows(int32_t rows);
int veto_debug_layernorm_backward_split(void* stream, const float* x, const float* dy, const float* gamma, const float* dres,
                                        float* dx, float* dgamma_dbeta, void* split_rows, float* col_partials, int32_t rows,
                                        uint64_t drop_seed, uint32_t drop_thresh, float drop_scale, void* workspace,
                                        size_t workspace_bytes);


/* ---- test hooks: the ordered forms (veto_train_opts_t.deterministic) of the backward's order-dependent sums, alone on caller-given buffers --
 * veto_debug_assemble_backward_ordered: dx device [n_pair * 19, 576]; subj / obj device int32 [n_pair], batch-wide object rows; lc device
 *   [n_obj, 2, 1152]; img_obj_offset / img_pair_offset device [n_img + 1] (the pairs of an image name objects of that image); out dpatch
 *   [n_obj, 16, 1152] and dlc [n_obj, 2, 1152], every element written.
 * veto_debug_scatter_rows_ordered: demb device [n, dim], labels device int64 [n]; out dtable [n_table_rows, dim], every element written.
 * veto_debug_layernorm_backward_ordered: veto_debug_layernorm_backward_split in the ordered form; split_rows and col_partials may both be
 *   NULL (the form without them). */
int veto_debug_assemble_backward_ordered(void* stream, const float* dx, const int32_t* subj, const int32_t* obj, const float* lc,
                                         const int32_t* img_obj_offset, const int32_t* img_pair_offset, int32_t n_img, int32_t n_obj,
                                         float* dpatch, float* dlc);
int veto_debug_scatter_rows_ordered(void* stream, const float* demb, const int64_t* labels, int32_t n, int32_t dim, int32_t n_table_rows,
                                    float* dtable);
int veto_debug_layernorm_backward_ordered(void* stream, const float* x, const float* dy, const float* gamma, const float* dres,
                                          float* dx, float* dgamma_dbeta, void* split_rows, float* col_partials, int32_t rows,
                                          uint64_t drop_seed, uint32_t drop_thresh, float drop_scale, void* workspace,
                                          size_t workspace_bytes);

/* ---- test hooks: the forward attention kernels and the layer-0 row combiner, each alone on caller-given device buffers ----------
 * (model_veto.py:85-96 per pair and head over the 19 tokens; tests/attention_cases.py states the contracts in float64.)
 * veto_debug_attention: qkv [19 n_pair, 1728] fp32 (q | k | v, heads side by side), or with qkv_f24 = 1 the same matrix as 3-byte
 *   floats (rows of 5184 bytes).  o receives the merged-heads output rows: split rows (o_fmt 0: 2 x 576 bf16 per row) or mixed
 *   activation rows (o_fmt 1: 2304 bytes per row), 19 n_pair of them, or n_pair (the CLS query's row of every pair) with cls_only = 1.
 *   Per-object form of layer 0 (all six of sw .. obj non-NULL, else all NULL): sw / ow fp32 [n_obj * 16, 1728], stats fp32
 *   [19 n_pair, 2] = (mean, rstd) per token row, vec fp32 [3, 1728] = c2 | b0 | the CLS row, subj / obj int32 [n_pair]: the row of
 *   token t = 1..16 of pair p is rstd[p, t] (sw[subj[p] * 16 + t - 1] + ow[obj[p] * 16 + t - 1]) + c2, token 0 is vec's third row,
 *   and only the rows of tokens 17 / 18 are read from qkv.
 *   Refused with VETO_ERR_INVALID before any launch: a NULL qkv or o, n_pair <= 0, heads that do not divide 576, table operands
 *   given in part, tables with cls_only or qkv_f24, tables / qkv_f24 / o_fmt 1 at a head width other than 72 or 96, a generic head
 *   width that is no multiple of 4 or needs more than 160 KB of LDS (heads 1, 2, 3).
 * veto_debug_cls_fold_attention: the folded CLS-query attention of the last layer.  x fp32 [19 n_pair, 576] (the residual stream;
 *   a_j = LayerNorm(x_j; ln_w, ln_b, eps 1e-5) is formed inside), u [n_pair, heads * 576] fp32 or (u_f24 = 1) 3-byte floats;
 *   score[h][j] = dh^-0.5 u_h . a_j, p = softmax over j, abar_h = sum_j p[h][j] a_j; abar = split rows [n_pair, 2 x heads x 576].
 *   Refused: NULL pointers, n_pair <= 0, heads that do not divide 576 or exceed 12, u_f24 with the vector-ALU form (VETO_CLS_MFMA=0).
 * veto_debug_qkv0_combine: writes the rows of tokens 0..16 of qkv fp32 [19 n_pair, 1728] from the per-object operands above (the
 *   rows of tokens 17 / 18 are left alone). */
int veto_debug_attention(void* stream, const void* qkv, void* o, int32_t n_pair, int32_t heads, int32_t cls_only, int32_t o_fmt,
                         int32_t qkv_f24, const float* sw, const float* ow, const float* stats, const float* vec, const int32_t* subj,
                         const int32_t* obj);
int veto_debug_cls_fold_attention(void* stream, const float* x, const float* ln_w, const float* ln_b, const void* u, void* abar,
                                  int32_t n_pair, int32_t heads, int32_t u_f24);
int veto_debug_qkv0_combine(void* stream, const float* sw, const float* ow, const float* stats, const float* vec, const int32_t* subj,
                            const int32_t* obj, float* qkv, int32_t n_pair);

#ifdef __cplusplus
}
#endif
#endif /* VETO_AMD_H_ */
