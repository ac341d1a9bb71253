// Detection-side entry points of the C ABI: pair enumeration / preparation, the relation post-processors, object decoding, NMS,
// box-head and RPN post-processing, the RPN's anchor generator, the relation samplers, the box head's proposal sampler, the RPN loss, the box head's loss, ROI pooling and
// the relation and detection evaluators.
// Each checks its argument struct (the checks several of them make are in abi_internal.h), fills the launch struct and makes one
// launch call (kernels.h).  An entry point with a workspace has ONE carve_*() that walks the layout and sets the launch struct's
// workspace pointers: veto_X_workspace_bytes runs it on a null base, veto_X on the caller's buffer.
#include <cmath>

#include "abi_internal.h"

extern "C" {

int veto_enumerate_pairs(void* stream, int32_t n, int64_t* out) {
  if (n < 0 || !out) return fail(VETO_ERR_INVALID, "bad argument");
  HIP_TRY(launch_enumerate_pairs(n, out, (hipStream_t)stream));
  return VETO_OK;
}

// workspace of the three relation post-processors over `rows` (merged) rows: prob_tmp | triple | label_tmp | perm
static size_t carve_post(Carver c, size_t rows, int n_rel_cls, PostArgs* p) {
  p->prob_tmp = c.take<float>(rows * n_rel_cls * 4);
  p->triple = c.take<float>(rows * 4);
  p->label_tmp = c.take<int32_t>(rows * 4);
  p->perm = c.take<int32_t>(rows * 4);
  return c.off;
}

size_t veto_postprocess_workspace_bytes(int32_t n_pair, int32_t n_rel_cls) {
  if (n_pair <= 0 || n_rel_cls <= 0) return 0;
  PostArgs p{};
  return carve_post(Carver{nullptr}, n_pair, n_rel_cls, &p);
}

int veto_postprocess(void* stream, const veto_post_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT_AND(veto_post_args_t, a, workspace != nullptr);
  if (a->n_img <= 0 || a->n_obj <= 0 || a->n_pair <= 0 || a->n_rel_cls < 2 || a->n_obj_cls < 2)
    return fail(VETO_ERR_INVALID, "bad sizes");
  if (!a->rel_logits || !a->rel_pairs || !a->img_obj_offset || !a->img_pair_offset || !a->obj_scores ||
      !a->obj_pred || !a->rel_prob_sorted || !a->rel_pairs_sorted || !a->rel_labels_sorted)
    return fail(VETO_ERR_INVALID, "missing pointer");
  if (a->max_pairs_per_image < 1 || a->max_pairs_per_image > postprocess_max_pairs_per_image())
    return fail(VETO_ERR_INVALID, "max_pairs_per_image %d outside 1..%d (MAX_PROPOSAL_PAIR is 2048 at test time)",
                a->max_pairs_per_image, postprocess_max_pairs_per_image());
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_postprocess_workspace_bytes(a->n_pair, a->n_rel_cls), false));
  PostArgs p = post_args(a);
  p.rel_logits = a->rel_logits; p.img_obj_off = a->img_obj_offset; p.img_pair_off = a->img_pair_offset; p.n_img = a->n_img;
  carve_post(Carver{(char*)workspace}, a->n_pair, a->n_rel_cls, &p);
  HIP_TRY(launch_postprocess(p, nullptr, (hipStream_t)stream));
  return VETO_OK;
}

// The MEET merge / expert vote of veto_postprocess_groups_batch and of the two one-image entry points, which are that call with
// n_img = 1: every check, the group tables, the workspace and the launch.  one_image: `a` was filled by one_image_groups() -- null
// offsets, pairs_per_image = {n_pair} -- and the row limit's message names no image.
static int post_groups(void* stream, const veto_post_groups_batch_args_t* a, bool one_image, void* workspace, size_t workspace_bytes) {
  if (a->n_img <= 0 || a->n_obj <= 0 || a->n_pair <= 0 || a->n_groups <= 0 || a->n_groups > kPostMaxGroups || a->n_rel_cls < 2 ||
      a->n_rel_cls > kPostMaxRelCls || a->n_obj_cls < 2)
    return fail(VETO_ERR_INVALID, "bad sizes (n_groups 1..%d, n_rel_cls 2..%d)", kPostMaxGroups, kPostMaxRelCls);
  if (a->experts_per_group != 1 && a->experts_per_group != 3)
    return fail(VETO_ERR_INVALID, "experts_per_group must be 1 (merge) or 3 (vote)");
  const bool vote = a->experts_per_group == 3;
  if (vote ? (a->voting != 0 && a->voting != 1) : a->voting != 0)
    return fail(VETO_ERR_INVALID, "%s", vote ? "voting must be 0 ('C') or 1 ('U')" : "voting must be 0 for the merge");
  if (!a->head_logits || !a->group_widths || !a->incre_idx_list || !a->pairs_per_image || !a->rel_pairs ||
      (!one_image && (!a->img_obj_offset || !a->img_pair_offset)) || !a->obj_scores || !a->obj_pred || !a->rel_prob_sorted ||
      !a->rel_pairs_sorted || !a->rel_labels_sorted || vote != (a->kept_count != nullptr))
    return fail(VETO_ERR_INVALID, "missing pointer");
  const long total = (long)a->n_groups * a->n_pair;
  if (total > INT32_MAX) return fail(VETO_ERR_INVALID, "n_groups * n_pair = %ld exceeds int32", total);
  long sum = 0;
  int largest = 0;
  for (int i = 0; i < a->n_img; ++i) {
    const long rows = (long)a->n_groups * a->pairs_per_image[i];
    if (a->pairs_per_image[i] < 0) return fail(VETO_ERR_INVALID, "image %d: %d pairs", i, a->pairs_per_image[i]);
    if (rows > postprocess_max_pairs_per_image())
      return one_image ? fail(VETO_ERR_INVALID, "n_groups * n_pair = %ld exceeds %d", rows, postprocess_max_pairs_per_image())
                       : fail(VETO_ERR_INVALID, "image %d: n_groups * pairs = %ld exceeds %d", i, rows, postprocess_max_pairs_per_image());
    sum += a->pairs_per_image[i];
    if (a->pairs_per_image[i] > largest) largest = a->pairs_per_image[i];
  }
  if (sum != a->n_pair || largest != a->max_pairs_per_image)
    return fail(VETO_ERR_INVALID, "pairs_per_image: sum %ld, maximum %d; n_pair %d, max_pairs_per_image %d", sum, largest, a->n_pair,
                a->max_pairs_per_image);
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_postprocess_workspace_bytes((int32_t)total, a->n_rel_cls), false));
  PostGroupTables t{};
  t.n_groups = a->n_groups; t.experts = a->experts_per_group; t.voting = a->voting;
  for (int c = 0; c < a->n_rel_cls; ++c)
    t.cls_group[c] = a->incre_idx_list[c] >= 0 && a->incre_idx_list[c] <= a->n_groups ? (uint8_t)a->incre_idx_list[c] : 255;
  for (int k = 0; k < a->n_groups; ++k) {
    ABI_TRY(check_group_width(a->group_widths[k], k, a->incre_idx_list, a->n_rel_cls));   // the kernel derives the columns itself
    t.width[k] = a->group_widths[k];
    for (int e = 0; e < a->experts_per_group; ++e) {
      t.logits[a->experts_per_group * k + e] = a->head_logits[a->experts_per_group * k + e];
      if (!t.logits[a->experts_per_group * k + e]) return fail(VETO_ERR_INVALID, "group %d head %d: null logits", k, e + 1);
    }
  }
  PostArgs p = post_args(a);
  p.n_img = a->n_img; p.img_obj_off = a->img_obj_offset; p.img_pair_off = a->img_pair_offset; p.kept_count = a->kept_count;
  carve_post(Carver{(char*)workspace}, total, a->n_rel_cls, &p);
  HIP_TRY(launch_postprocess(p, &t, (hipStream_t)stream));
  return VETO_OK;
}

int veto_postprocess_meet(void* stream, const veto_post_meet_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT_AND(veto_post_meet_args_t, a, workspace != nullptr);
  const veto_post_groups_batch_args_t b = one_image_groups(a, a->group_logits, 1, 0, nullptr);
  return post_groups(stream, &b, true, workspace, workspace_bytes);
}

int veto_postprocess_vote(void* stream, const veto_post_vote_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT_AND(veto_post_vote_args_t, a, workspace != nullptr);
  const veto_post_groups_batch_args_t b = one_image_groups(a, a->expert_logits, 3, a->voting, a->kept_count);
  return post_groups(stream, &b, true, workspace, workspace_bytes);
}

int veto_postprocess_groups_batch(void* stream, const veto_post_groups_batch_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT_AND(veto_post_groups_batch_args_t, a, workspace != nullptr);
  return post_groups(stream, a, false, workspace, workspace_bytes);
}

static size_t carve_obj_decode(Carver c, int n_obj, int n_cls, ObjDecodeArgs* p) {
  p->prob_ws = c.take<float>((size_t)n_obj * n_cls * 4);
  return c.off;
}

size_t veto_obj_decode_workspace_bytes(int32_t n_obj, int32_t n_cls) {
  if (n_obj <= 0 || n_cls <= 0) return 0;
  ObjDecodeArgs p{};
  return carve_obj_decode(Carver{nullptr}, n_obj, n_cls, &p);
}

int veto_obj_decode(void* stream, const veto_obj_decode_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_obj_decode_args_t, a);
  if (a->n_img <= 0 || a->n_obj <= 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_obj %d)", a->n_img, a->n_obj);
  if (a->n_cls < 2 || a->n_cls > 1024) return fail(VETO_ERR_INVALID, "n_cls %d outside 2..1024", a->n_cls);
  if (a->max_obj_per_image < 1 || a->max_obj_per_image > obj_decode_max_objects())
    return fail(VETO_ERR_INVALID, "max_obj_per_image %d outside 1..%d (DETECTIONS_PER_IMG)", a->max_obj_per_image,
                obj_decode_max_objects());
  if (a->mode != 0 && a->mode != 1) return fail(VETO_ERR_INVALID, "mode must be 0 (PostProcessor) or 1 (MEET decoder)");
  if (!a->boxes_per_cls || !a->img_obj_offset || !a->obj_pred || (a->mode == 0 && !a->logits) || (a->mode == 1 && !a->labels) ||
      (a->obj_scores && !a->logits))
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_obj_decode_workspace_bytes(a->n_obj, a->n_cls), false));
  ObjDecodeArgs p{};
  p.logits = a->logits; p.labels = a->labels; p.boxes_per_cls = a->boxes_per_cls; p.img_off = a->img_obj_offset;
  p.n_img = a->n_img; p.n_cls = a->n_cls; p.mode = a->mode; p.thr = a->nms_thres;
  carve_obj_decode(Carver{(char*)workspace}, a->n_obj, a->n_cls, &p);
  p.obj_pred = a->obj_pred; p.obj_scores = a->obj_scores; p.out_boxes = a->boxes;
  HIP_TRY(launch_obj_decode(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_prepare_test_pairs(void* stream, const veto_pair_args_t* a) {
  CHECK_STRUCT(veto_pair_args_t, a);
  if (a->n_img <= 0 || a->n_obj < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_obj %d)", a->n_img, a->n_obj);
  if (a->max_obj_per_image < 0 || a->max_obj_per_image > obj_decode_max_objects())
    return fail(VETO_ERR_INVALID, "max_obj_per_image %d outside 0..%d", a->max_obj_per_image, obj_decode_max_objects());
  if (a->max_pairs < 1 || a->max_pairs > prepare_pairs_max_pairs())
    return fail(VETO_ERR_INVALID, "max_pairs %d outside 1..%d (MAX_PROPOSAL_PAIR)", a->max_pairs, prepare_pairs_max_pairs());
  if ((a->n_obj > 0 && (!a->boxes || !a->scores)) || !a->img_obj_offset || !a->img_out_offset || !a->pairs || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  PairArgs p{};
  p.boxes = a->boxes; p.scores = a->scores; p.img_off = a->img_obj_offset; p.out_off = a->img_out_offset;
  p.n_img = a->n_img; p.max_pairs = a->max_pairs; p.require_overlap = a->require_overlap != 0;
  p.pairs = a->pairs; p.counts = a->counts;
  HIP_TRY(launch_prepare_pairs(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_nms_max_segment(void) { return nms_max_segment(); }

// host offsets: 0 = first, non-decreasing, last = total, no segment above `limit`; returns the largest segment or -1 (error set)
static int check_host_offsets(const int32_t* off, int n_seg, int total, int limit, const char* name, const char* total_name) {
  if (off[0] != 0) return fail(VETO_ERR_INVALID, "%s[0] must be 0, got %d", name, off[0]);
  int largest = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int n = off[s + 1] - off[s];
    if (n < 0) return fail(VETO_ERR_INVALID, "%s is not monotone: entry %d is %d after %d", name, s + 1, off[s + 1], off[s]);
    if (n > limit) return fail(VETO_ERR_INVALID, "%s: segment %d holds %d boxes, the limit is %d", name, s, n, limit);
    if (n > largest) largest = n;
  }
  if (off[n_seg] != total) return fail(VETO_ERR_INVALID, "%s ends at %d, %s is %d", name, off[n_seg], total_name, total);
  return largest;
}

int veto_nms(void* stream, const veto_nms_args_t* a) {
  CHECK_STRUCT(veto_nms_args_t, a);
  if (a->n_seg <= 0 || a->n_box < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_seg %d, n_box %d)", a->n_seg, a->n_box);
  if (!a->seg_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: seg_offset_host");
  const int largest = check_host_offsets(a->seg_offset_host, a->n_seg, a->n_box, nms_max_segment(), "seg_offset_host", "n_box");
  if (largest < 0) return largest;
  if ((a->n_box > 0 && (!a->boxes || !a->scores || !a->keep)) || !a->seg_offset || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  if (((uintptr_t)a->boxes & 15) != 0) return fail(VETO_ERR_INVALID, "boxes must be 16-byte aligned");
  NmsArgs p{};
  p.boxes = a->boxes; p.scores = a->scores; p.seg_off = a->seg_offset; p.n_seg = a->n_seg; p.max_keep = a->max_keep;
  p.thr = a->threshold; p.keep = a->keep; p.counts = a->counts;
  HIP_TRY(launch_nms(p, largest, (hipStream_t)stream));
  return VETO_OK;
}

// workspace: prob | dec | row_score | row_label | list_score | list_row | list_label
static size_t carve_box_post(Carver c, size_t n_box, int n_cls, bool filter_dup, BoxPostArgs* p) {
  const size_t list_rows = filter_dup ? n_box : n_box * (n_cls - 1);
  p->prob = c.take<float>(n_box * n_cls * 4);
  p->dec = c.take<float>(n_box * n_cls * 16);
  p->row_score = c.take<float>(n_box * 4);
  p->row_label = c.take<int32_t>(n_box * 4);
  p->list_score = c.take<float>(list_rows * 4);
  p->list_row = c.take<int32_t>(list_rows * 4);
  p->list_label = c.take<int32_t>(list_rows * 4);
  return c.off;
}

size_t veto_box_postprocess_workspace_bytes(int32_t n_box, int32_t n_cls, int32_t filter_duplicates) {
  if (n_box <= 0 || n_cls < 2) return 256;
  BoxPostArgs p{};
  return carve_box_post(Carver{nullptr}, n_box, n_cls, filter_duplicates != 0, &p);
}

int veto_box_postprocess(void* stream, const veto_box_post_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_box_post_args_t, a);
  if (a->n_img <= 0 || a->n_box <= 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_box %d)", a->n_img, a->n_box);
  if (a->n_img > 65535) return fail(VETO_ERR_INVALID, "n_img %d above 65535", a->n_img);
  if (a->n_cls < 2 || a->n_cls > 1024) return fail(VETO_ERR_INVALID, "n_cls %d outside 2..1024", a->n_cls);
  if (a->reg_cols < 4 || a->reg_cols % 4 != 0 || (!a->cls_agnostic && a->reg_cols != 4 * a->n_cls))
    return fail(VETO_ERR_INVALID, "reg_cols %d: must be 4 * n_cls (%d), or a multiple of 4 with cls_agnostic", a->reg_cols, 4 * a->n_cls);
  if (!(a->score_thresh >= 0.f)) return fail(VETO_ERR_INVALID, "score_thresh %g must be >= 0 (SCORE_THRESH)", a->score_thresh);
  if (!(a->nms_thresh > 0.f)) return fail(VETO_ERR_INVALID, "nms_thresh %g must be > 0 (ROI_HEADS.NMS)", a->nms_thresh);
  ABI_TRY(check_reg_weights(a->reg_weights, true, " (BBOX_REG_WEIGHTS)"));
  if (!a->img_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: img_offset_host");
  const int largest = check_host_offsets(a->img_offset_host, a->n_img, a->n_box, nms_max_segment(), "img_offset_host", "n_box");
  if (largest < 0) return largest;
  if (!a->class_logits || !a->box_regression || !a->proposals || !a->image_sizes || !a->img_offset || !a->img_out_offset ||
      !a->orig_inds || !a->pred_labels || !a->pred_scores || !a->boxes || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  if ((((uintptr_t)a->box_regression | (uintptr_t)a->proposals | (uintptr_t)a->boxes | (uintptr_t)a->boxes_per_cls) & 15) != 0)
    return fail(VETO_ERR_INVALID, "box_regression, proposals, boxes and boxes_per_cls must be 16-byte aligned");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_box_postprocess_workspace_bytes(a->n_box, a->n_cls, a->filter_duplicates), true));
  BoxPostArgs p{};
  p.logits = a->class_logits; p.regression = a->box_regression; p.proposals = a->proposals; p.image_sizes = a->image_sizes;
  p.img_off = a->img_offset; p.out_off = a->img_out_offset;
  p.n_img = a->n_img; p.n_box = a->n_box; p.n_cls = a->n_cls; p.reg_cols = a->reg_cols; p.cls_agnostic = a->cls_agnostic != 0;
  p.topn = a->post_nms_per_cls_topn; p.filter_dup = a->filter_duplicates != 0; p.det_per_img = a->detections_per_img;
  p.score_thresh = a->score_thresh; p.nms_thresh = a->nms_thresh;
  p.wx = a->reg_weights[0]; p.wy = a->reg_weights[1]; p.ww = a->reg_weights[2]; p.wh = a->reg_weights[3];
  p.xform_clip = a->bbox_xform_clip;
  carve_box_post(Carver{(char*)workspace}, a->n_box, a->n_cls, p.filter_dup, &p);
  p.orig_inds = a->orig_inds; p.labels = a->pred_labels; p.scores = a->pred_scores; p.boxes = a->boxes;
  p.boxes_per_cls = a->boxes_per_cls; p.counts = a->counts;
  HIP_TRY(launch_box_postprocess(p, largest, (hipStream_t)stream));
  return VETO_OK;
}

// the host fields of the RPN arguments: capacity = the largest k of a level, or -1 (error set)
static int rpn_check_shapes(const veto_rpn_args_t* a) {
  ABI_TRY(check_rpn_counts(a));
  if (a->pre_nms_top_n <= 0 || a->pre_nms_top_n > nms_max_segment())
    return fail(VETO_ERR_INVALID, "pre_nms_top_n %d outside 1..%d (MODEL.RPN.PRE_NMS_TOP_N; the limit is veto_nms_max_segment())",
                a->pre_nms_top_n, nms_max_segment());
  int capacity = 0;
  for (int l = 0; l < a->n_lvl; ++l) {
    ABI_TRY(check_rpn_level(a, l));
    const int64_t n = (int64_t)a->level_a[l] * a->level_h[l] * a->level_w[l];
    if (n > INT32_MAX) return fail(VETO_ERR_INVALID, "level %d holds %lld anchors, the limit is %d", l, (long long)n, INT32_MAX);
    const int k = n < a->pre_nms_top_n ? (int)n : a->pre_nms_top_n;
    if (k > capacity) capacity = k;
  }
  return capacity;
}

// workspace: cand_box | cand_logit | cand_anchor | keep | live | kept | cut
static size_t carve_rpn(Carver c, size_t n_img, size_t n_lvl, size_t capacity, RpnArgs* p) {
  const size_t n_seg = n_img * n_lvl, rows = n_seg * capacity;
  p->cand_box = c.take<float>(rows * 16);
  p->cand_logit = c.take<float>(rows * 4);
  p->cand_anchor = c.take<int32_t>(rows * 4);
  p->keep = c.take<int32_t>(rows * 4);
  p->live = c.take<int32_t>(n_seg * 4);
  p->kept = c.take<int32_t>(n_seg * 4);
  p->cut = c.take<int32_t>((4 + n_img) * 4);
  return c.off;
}

size_t veto_rpn_proposals_workspace_bytes(const veto_rpn_args_t* a) {
  if (!a || a->struct_size != (int32_t)sizeof(veto_rpn_args_t)) return 0;
  const int capacity = rpn_check_shapes(a);
  if (capacity < 0) return 0;
  RpnArgs p{};
  return carve_rpn(Carver{nullptr}, a->n_img, a->n_lvl, capacity, &p);
}

int veto_rpn_proposals(void* stream, const veto_rpn_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_rpn_args_t, a);
  const int capacity = rpn_check_shapes(a);
  if (capacity < 0) return capacity;
  const bool nms_on = a->nms_thresh > 0.f, merge = a->n_lvl > 1;
  if (merge && a->fpn_post_nms_top_n <= 0) return fail(VETO_ERR_INVALID, "fpn_post_nms_top_n %d must be > 0 with %d levels", a->fpn_post_nms_top_n, a->n_lvl);
  ABI_TRY(check_reg_weights(a->reg_weights, true, ""));
  if (merge && a->per_batch) {
    if (a->n_img > rpn_batch_cut_max_images())
      return fail(VETO_ERR_INVALID, "per_batch: n_img %d above %d", a->n_img, rpn_batch_cut_max_images());
  } else if (merge) {   // the per-image merge sorts every survivor of the image in one workgroup
    int64_t bound = 0;
    for (int l = 0; l < a->n_lvl; ++l) {
      const int64_t n = (int64_t)a->level_a[l] * a->level_h[l] * a->level_w[l];
      const int64_t k = n < a->pre_nms_top_n ? n : a->pre_nms_top_n;
      bound += nms_on && a->post_nms_top_n > 0 && a->post_nms_top_n < k ? a->post_nms_top_n : k;
    }
    if (bound > kRpnSortCap)
      return fail(VETO_ERR_INVALID, "the levels may leave %lld proposals per image, the merge takes %d (lower post_nms_top_n)", (long long)bound,
                  kRpnSortCap);
  }
  for (int l = 0; l < a->n_lvl; ++l) {
    if (!a->objectness[l] || !a->box_regression[l] || !a->anchors[l]) return fail(VETO_ERR_INVALID, "missing pointer: level %d", l);
    if (((uintptr_t)a->anchors[l] & 15) != 0) return fail(VETO_ERR_INVALID, "anchors[%d] must be 16-byte aligned", l);
    if ((((uintptr_t)a->objectness[l] | (uintptr_t)a->box_regression[l]) & 3) != 0) return fail(VETO_ERR_INVALID, "level %d: misaligned floats", l);
  }
  if (!a->image_sizes || !a->img_out_offset || !a->boxes || !a->objectness_out || !a->level || !a->anchor_index || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  if (((uintptr_t)a->boxes & 15) != 0) return fail(VETO_ERR_INVALID, "boxes must be 16-byte aligned");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_rpn_proposals_workspace_bytes(a), true));
  RpnArgs p{};
  for (int l = 0; l < a->n_lvl; ++l) {
    RpnLevel& v = p.lvl[l];
    v.objectness = a->objectness[l]; v.regression = a->box_regression[l]; v.anchors = a->anchors[l];
    v.A = a->level_a[l]; v.HW = a->level_h[l] * a->level_w[l]; v.N = v.A * v.HW;
    v.k = v.N < a->pre_nms_top_n ? v.N : a->pre_nms_top_n;
  }
  p.image_sizes = a->image_sizes; p.out_off = a->img_out_offset;
  p.n_img = a->n_img; p.n_lvl = a->n_lvl; p.capacity = capacity;
  p.post_top_n = a->post_nms_top_n; p.fpn_top_n = a->fpn_post_nms_top_n; p.per_batch = a->per_batch != 0; p.nms_on = nms_on;
  p.nms_thresh = a->nms_thresh; p.min_size = a->min_size;
  p.wx = a->reg_weights[0]; p.wy = a->reg_weights[1]; p.ww = a->reg_weights[2]; p.wh = a->reg_weights[3];
  p.xform_clip = a->bbox_xform_clip;
  carve_rpn(Carver{(char*)workspace}, a->n_img, a->n_lvl, capacity, &p);
  p.boxes = a->boxes; p.objectness = a->objectness_out; p.level = a->level; p.anchor_index = a->anchor_index; p.counts = a->counts;
  HIP_TRY(launch_rpn_proposals(p, (hipStream_t)stream));
  return VETO_OK;
}

// the host fields of the anchor generator's arguments: rows of the concatenated levels, or a negative status (error set)
static int anchor_check_shapes(const veto_anchor_args_t* a) {
  if (a->n_lvl <= 0 || a->n_lvl > VETO_RPN_MAX_LEVELS) return fail(VETO_ERR_INVALID, "n_lvl %d outside 1..%d", a->n_lvl, VETO_RPN_MAX_LEVELS);
  int64_t total = 0;
  for (int l = 0; l < a->n_lvl; ++l) {
    ABI_TRY(check_rpn_level(a, l));
    if (a->level_stride[l] < 1) return fail(VETO_ERR_INVALID, "level %d: stride %d must be >= 1 (ANCHOR_STRIDE)", l, a->level_stride[l]);
    const int64_t sx = (int64_t)(a->level_w[l] - 1) * a->level_stride[l], sy = (int64_t)(a->level_h[l] - 1) * a->level_stride[l];
    if (sx >= (1 << 24) || sy >= (1 << 24))
      return fail(VETO_ERR_INVALID, "level %d: the largest shift (%lld, %lld) must stay below 2^24 to be exact in float32", l, (long long)sx,
                  (long long)sy);
    total += (int64_t)a->level_a[l] * a->level_h[l] * a->level_w[l];
    if (total > rpn_loss_max_anchors())
      return fail(VETO_ERR_INVALID, "levels 0..%d: an image holds %lld anchors, the limit is %d", l, (long long)total, rpn_loss_max_anchors());
  }
  return (int)total;
}

int veto_anchor_grid(void* stream, const veto_anchor_args_t* a) {
  CHECK_STRUCT(veto_anchor_args_t, a);
  const int total = anchor_check_shapes(a);
  if (total < 0) return total;
  if (!a->anchors && !a->visibility) return fail(VETO_ERR_INVALID, "missing pointer: anchors and visibility are both NULL, nothing to write");
  if (!a->anchors && !a->anchors_in) return fail(VETO_ERR_INVALID, "missing pointer: anchors_in (anchors is NULL, so the plane is computed from it)");
  if ((((uintptr_t)a->anchors | (uintptr_t)a->anchors_in) & 15) != 0) return fail(VETO_ERR_INVALID, "anchors and anchors_in must be 16-byte aligned");
  if (a->anchors)
    for (int l = 0; l < a->n_lvl; ++l) {
      if (!a->cell_anchors[l]) return fail(VETO_ERR_INVALID, "missing pointer: cell_anchors[%d]", l);
      if (((uintptr_t)a->cell_anchors[l] & 15) != 0) return fail(VETO_ERR_INVALID, "cell_anchors[%d] must be 16-byte aligned", l);
    }
  if (a->visibility) {
    if (a->n_img < 1 || a->n_img > 65535) return fail(VETO_ERR_INVALID, "n_img %d outside 1..65535 (visibility is asked for)", a->n_img);
    if (a->straddle_thresh >= 0.f && !a->image_sizes) return fail(VETO_ERR_INVALID, "missing pointer: image_sizes (straddle_thresh >= 0)");
    if (!(a->straddle_thresh == a->straddle_thresh)) return fail(VETO_ERR_INVALID, "straddle_thresh is NaN");
  }
  AnchorArgs p{};
  int row0 = 0;
  for (int l = 0; l < a->n_lvl; ++l) {
    AnchorLevel& v = p.lvl[l];
    v.cell = a->cell_anchors[l]; v.A = a->level_a[l]; v.W = a->level_w[l]; v.stride = a->level_stride[l]; v.row0 = row0;
    row0 += a->level_a[l] * a->level_h[l] * a->level_w[l];
  }
  p.n_lvl = a->n_lvl; p.total = total;
  p.anchors = a->anchors; p.anchors_in = a->anchors_in; p.image_sizes = a->image_sizes;
  p.n_img = a->n_img; p.straddle = a->straddle_thresh; p.visibility = a->visibility;
  HIP_TRY(launch_anchor_grid(p, (hipStream_t)stream));
  return VETO_OK;
}

// workspace: ws_nm | ws_fg
static size_t carve_relsample(Carver c, size_t n_rel_cells, int per_rel, RelSampleArgs* p) {
  p->ws_nm = c.take<int64_t>(n_rel_cells * 8);
  p->ws_fg = c.take<uint32_t>(n_rel_cells * per_rel * 4);
  return c.off;
}

size_t veto_detect_relsample_workspace_bytes(int32_t n_rel_cells, int32_t num_sample_per_gt_rel) {
  if (n_rel_cells <= 0 || num_sample_per_gt_rel <= 0) return 256;
  RelSampleArgs p{};
  return carve_relsample(Carver{nullptr}, n_rel_cells, num_sample_per_gt_rel, &p);
}

int veto_detect_relsample(void* stream, const veto_detect_relsample_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_detect_relsample_args_t, a);
  if (a->n_img <= 0 || a->n_prp < 0 || a->n_tgt < 0 || a->n_rel_cells < 0)
    return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_prp %d, n_tgt %d, n_rel_cells %d)", a->n_img, a->n_prp, a->n_tgt,
                a->n_rel_cells);
  const int lim = relsample_max_objects();
  if (a->max_prp_per_image < 0 || a->max_prp_per_image > lim)
    return fail(VETO_ERR_INVALID, "max_prp_per_image %d outside 0..%d (detections per image, DETECTIONS_PER_IMG)",
                a->max_prp_per_image, lim);
  if (a->max_tgt_per_image < 0 || a->max_tgt_per_image > lim)
    return fail(VETO_ERR_INVALID, "max_tgt_per_image %d outside 0..%d (GT boxes per image)", a->max_tgt_per_image, lim);
  ABI_TRY(check_batch_size(a->batch_size_per_image, relsample_max_batch(), "BATCH_SIZE_PER_IMAGE"));
  if (a->num_sample_per_gt_rel < 1 || a->num_sample_per_gt_rel > relsample_max_per_rel())
    return fail(VETO_ERR_INVALID, "num_sample_per_gt_rel %d outside 1..%d (NUM_SAMPLE_PER_GT_REL)", a->num_sample_per_gt_rel,
                relsample_max_per_rel());
  ABI_TRY(check_positives("max_fg_per_image", a->max_fg_per_image, a->batch_size_per_image));
  if ((a->n_prp > 0 && (!a->prp_boxes || !a->prp_labels || !a->prp_scores || !a->locating_match)) ||
      (a->n_tgt > 0 && (!a->tgt_boxes || !a->tgt_labels)) || (a->n_rel_cells > 0 && !a->relation) ||
      (a->relation_non_masked && !a->labels_all) || !a->img_prp_offset || !a->img_tgt_offset || !a->img_rel_offset ||
      !a->img_binary_offset || !a->pairs || !a->labels || !a->binary_rel || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_detect_relsample_workspace_bytes(a->n_rel_cells, a->num_sample_per_gt_rel), true));
  RelSampleArgs p{};
  p.prp_boxes = a->prp_boxes; p.prp_labels = a->prp_labels; p.prp_scores = a->prp_scores;
  p.tgt_boxes = a->tgt_boxes; p.tgt_labels = a->tgt_labels;
  p.relation = a->relation; p.relation_nm = a->relation_non_masked;
  p.prp_off = a->img_prp_offset; p.tgt_off = a->img_tgt_offset; p.rel_off = a->img_rel_offset; p.bin_off = a->img_binary_offset;
  p.n_img = a->n_img; p.require_overlap = a->require_overlap != 0; p.per_rel = a->num_sample_per_gt_rel;
  p.max_fg = a->max_fg_per_image; p.batch = a->batch_size_per_image;
  p.out_rows = a->batch_size_per_image > 2 ? a->batch_size_per_image : 2;
  p.fg_thres = a->fg_thres; p.seed = a->seed;
  carve_relsample(Carver{(char*)workspace}, a->n_rel_cells, a->num_sample_per_gt_rel, &p);
  p.pairs = a->pairs; p.labels = a->labels; p.labels_all = a->relation_non_masked ? a->labels_all : nullptr;
  p.binary = a->binary_rel; p.locating = a->locating_match; p.counts = a->counts;
  HIP_TRY(launch_detect_relsample(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_gtbox_relsample(void* stream, const veto_gtbox_relsample_args_t* a) {
  CHECK_STRUCT(veto_gtbox_relsample_args_t, a);
  if (a->n_img <= 0 || a->n_rel_cells < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_rel_cells %d)", a->n_img, a->n_rel_cells);
  if (a->max_obj_per_image < 0 || a->max_obj_per_image > gtbox_relsample_max_objects())
    return fail(VETO_ERR_INVALID, "max_obj_per_image %d outside 0..%d (GT boxes per image)", a->max_obj_per_image,
                gtbox_relsample_max_objects());
  ABI_TRY(check_batch_size(a->batch_size_per_image, gtbox_relsample_max_batch(), "BATCH_SIZE_PER_IMAGE"));
  ABI_TRY(check_positives("num_pos_per_img", a->num_pos_per_img, a->batch_size_per_image));
  if ((a->n_rel_cells > 0 && (!a->relation || !a->binary_rel)) || !a->img_obj_offset || !a->img_rel_offset || !a->pairs ||
      !a->labels || !a->counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  GtboxRelSampleArgs p{};
  p.relation = a->relation; p.obj_off = a->img_obj_offset; p.rel_off = a->img_rel_offset;
  p.n_img = a->n_img; p.batch = a->batch_size_per_image; p.num_pos = a->num_pos_per_img; p.seed = a->seed;
  p.pairs = a->pairs; p.labels = a->labels; p.binary = a->binary_rel; p.counts = a->counts;
  HIP_TRY(launch_gtbox_relsample(p, (hipStream_t)stream));
  return VETO_OK;
}

// check_host_offsets for the box-head sampler, which also refuses an empty image as the reference does (matcher.py:53-62)
static int check_box_sample_offsets(const int32_t* off, int n_img, int total, int limit, const char* name, const char* total_name,
                                    const char* empty_message) {
  const int largest = check_host_offsets(off, n_img, total, limit, name, total_name);
  for (int i = 0; largest >= 0 && i < n_img; ++i)
    if (off[i + 1] == off[i]) return fail(VETO_ERR_INVALID, "%s (image %d)", empty_message, i);
  return largest;
}

static const char* const kNoGtBoxes = "No ground-truth boxes available for one of the images during training";
static const char* const kNoProposals = "No proposal boxes available for one of the images during training";

int veto_box_match(void* stream, const veto_box_match_args_t* a) {
  CHECK_STRUCT(veto_box_match_args_t, a);
  if (a->n_img <= 0 || a->n_img > 65535 || a->n_prp < 0 || a->n_tgt < 0)
    return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_prp %d, n_tgt %d)", a->n_img, a->n_prp, a->n_tgt);
  if (a->mode != 0 && a->mode != 1) return fail(VETO_ERR_INVALID, "mode must be 0 (assign_label_to_proposals) or 1 (prepare_targets)");
  if (!(a->low_threshold <= a->high_threshold))
    return fail(VETO_ERR_INVALID, "low_threshold %g must be <= high_threshold %g (BG_IOU_THRESHOLD, FG_IOU_THRESHOLD)", a->low_threshold,
                a->high_threshold);
  if (!a->img_prp_offset_host || !a->img_tgt_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: host offsets");
  // the reference meets the empty GT list first (matcher.py:55)
  if (check_box_sample_offsets(a->img_tgt_offset_host, a->n_img, a->n_tgt, box_match_max_gt(), "img_tgt_offset_host", "n_tgt",
                               kNoGtBoxes) < 0)
    return VETO_ERR_INVALID;
  const int largest = check_box_sample_offsets(a->img_prp_offset_host, a->n_img, a->n_prp, box_subsample_max_proposals(),
                                               "img_prp_offset_host", "n_prp", kNoProposals);
  if (largest < 0) return largest;
  if (a->regression_targets) ABI_TRY(check_reg_weights(a->reg_weights, false, " (BBOX_REG_WEIGHTS)"));
  if (!a->prp_boxes || !a->tgt_boxes || !a->tgt_labels || !a->img_prp_offset || !a->img_tgt_offset || !a->matched_idxs || !a->labels)
    return fail(VETO_ERR_INVALID, "missing pointer");
  if ((((uintptr_t)a->prp_boxes | (uintptr_t)a->tgt_boxes | (uintptr_t)a->regression_targets) & 15) != 0)
    return fail(VETO_ERR_INVALID, "prp_boxes, tgt_boxes and regression_targets must be 16-byte aligned");
  BoxMatchArgs p{};
  p.prp_boxes = a->prp_boxes; p.tgt_boxes = a->tgt_boxes; p.tgt_labels = a->tgt_labels;
  p.prp_off = a->img_prp_offset; p.tgt_off = a->img_tgt_offset;
  p.n_img = a->n_img; p.mode = a->mode; p.high = a->high_threshold; p.low = a->low_threshold;
  p.wx = a->reg_weights[0]; p.wy = a->reg_weights[1]; p.ww = a->reg_weights[2]; p.wh = a->reg_weights[3];
  p.matched = a->matched_idxs; p.labels = a->labels; p.matched_rows = a->matched_rows; p.targets = a->regression_targets;
  HIP_TRY(launch_box_match(p, largest, (hipStream_t)stream));
  return VETO_OK;
}

int veto_box_subsample(void* stream, const veto_box_subsample_args_t* a) {
  CHECK_STRUCT(veto_box_subsample_args_t, a);
  if (a->n_img <= 0 || a->n_prp < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_prp %d)", a->n_img, a->n_prp);
  ABI_TRY(check_batch_size(a->batch_size_per_image, box_subsample_max_batch(), "BATCH_SIZE_PER_IMAGE"));
  ABI_TRY(check_positives("num_pos_per_img", a->num_pos_per_img, a->batch_size_per_image));
  if (!a->img_prp_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: img_prp_offset_host");
  if (check_box_sample_offsets(a->img_prp_offset_host, a->n_img, a->n_prp, box_subsample_max_proposals(), "img_prp_offset_host", "n_prp",
                               kNoProposals) < 0)
    return VETO_ERR_INVALID;
  if (!a->labels || !a->img_prp_offset || !a->sampled_inds || !a->counts) return fail(VETO_ERR_INVALID, "missing pointer");
  BoxSubsampleArgs p{};
  p.labels = a->labels; p.prp_off = a->img_prp_offset;
  p.n_img = a->n_img; p.batch = a->batch_size_per_image; p.num_pos = a->num_pos_per_img; p.seed = a->seed;
  p.sampled = a->sampled_inds; p.counts = a->counts;
  HIP_TRY(launch_box_subsample(p, (hipStream_t)stream));
  return VETO_OK;
}

// the host fields of the RPN loss arguments: anchors per image, or -1 (error set)
static int rpn_loss_check_shapes(const veto_rpn_loss_args_t* a) {
  ABI_TRY(check_rpn_counts(a));
  if (a->n_tgt < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_tgt %d)", a->n_tgt);
  ABI_TRY(check_batch_size(a->batch_size_per_image, rpn_loss_max_batch(), "MODEL.RPN.BATCH_SIZE_PER_IMAGE"));
  int64_t n_anchor = 0;
  for (int l = 0; l < a->n_lvl; ++l) {
    ABI_TRY(check_rpn_level(a, l));
    n_anchor += (int64_t)a->level_a[l] * a->level_h[l] * a->level_w[l];
    if (n_anchor > rpn_loss_max_anchors())
      return fail(VETO_ERR_INVALID, "levels 0..%d: an image holds %lld anchors, the limit is %d", l, (long long)n_anchor, rpn_loss_max_anchors());
  }
  return (int)n_anchor;
}

// workspace: gtmax | labels | matched | sampled | counts | partial | hist
static size_t carve_rpn_loss(Carver c, const veto_rpn_loss_args_t* a, size_t n_anchor, RpnLossArgs* p) {
  const size_t n_img = a->n_img, rows = n_img * n_anchor;
  p->gtmax = c.take<uint32_t>((size_t)a->n_tgt * 4 + 4);
  p->labels_ws = c.take<float>(rows * 4);      // (reserved also when the caller's `labels` takes its place)
  p->matched_ws = c.take<int32_t>(rows * 4);
  p->sampled_ws = c.take<int32_t>(n_img * a->batch_size_per_image * 4);
  p->counts_ws = c.take<int32_t>(n_img * 8);
  p->partial = c.take<double>(n_img * 16);
  p->hist = c.take<int32_t>(n_img * 2048);
  return c.off;
}

size_t veto_rpn_loss_workspace_bytes(const veto_rpn_loss_args_t* a) {
  if (!a || a->struct_size != (int32_t)sizeof(veto_rpn_loss_args_t)) return 0;
  const int n_anchor = rpn_loss_check_shapes(a);
  if (n_anchor < 0) return 0;
  RpnLossArgs p{};
  return carve_rpn_loss(Carver{nullptr}, a, n_anchor, &p);
}

int veto_rpn_loss(void* stream, const veto_rpn_loss_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_rpn_loss_args_t, a);
  const int n_anchor = rpn_loss_check_shapes(a);
  if (n_anchor < 0) return n_anchor;
  ABI_TRY(check_positives("num_pos_per_img", a->num_pos_per_img, a->batch_size_per_image));
  if (!(a->low_threshold <= a->high_threshold))
    return fail(VETO_ERR_INVALID, "low_threshold %g must be <= high_threshold %g (BG_IOU_THRESHOLD, FG_IOU_THRESHOLD)", a->low_threshold,
                a->high_threshold);
  if (!a->img_tgt_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: img_tgt_offset_host");
  if (check_box_sample_offsets(a->img_tgt_offset_host, a->n_img, a->n_tgt, rpn_loss_max_gt(), "img_tgt_offset_host", "n_tgt", kNoGtBoxes) < 0)
    return VETO_ERR_INVALID;
  int n_grad = 0;
  for (int l = 0; l < a->n_lvl; ++l) n_grad += (a->d_objectness[l] != nullptr) + (a->d_box_regression[l] != nullptr);
  if (n_grad != 0 && n_grad != 2 * a->n_lvl)
    return fail(VETO_ERR_INVALID, "d_objectness and d_box_regression: every level of both or none (%d of %d given)", n_grad, 2 * a->n_lvl);
  if (n_grad && !a->losses) return fail(VETO_ERR_INVALID, "missing pointer: losses (required with the gradients)");
  const int last_stage = a->losses ? kRpnLossLoss : (a->sampled_inds || a->counts) ? kRpnLossSample : kRpnLossMatch;
  if (last_stage == kRpnLossMatch && !a->labels && !a->matched_idxs && !a->regression_targets)
    return fail(VETO_ERR_INVALID, "no output requested");
  if (last_stage == kRpnLossLoss || a->regression_targets) {
    if (!(a->beta > 0.0) && last_stage == kRpnLossLoss) return fail(VETO_ERR_INVALID, "beta %g must be > 0", a->beta);
    ABI_TRY(check_reg_weights(a->reg_weights, false, ""));
  }
  for (int l = 0; l < a->n_lvl; ++l) {
    if (!a->anchors[l] || (last_stage == kRpnLossLoss && (!a->objectness[l] || !a->box_regression[l])))
      return fail(VETO_ERR_INVALID, "missing pointer: level %d", l);
    if (((uintptr_t)a->anchors[l] & 15) != 0) return fail(VETO_ERR_INVALID, "anchors[%d] must be 16-byte aligned", l);
    if ((((uintptr_t)a->objectness[l] | (uintptr_t)a->box_regression[l] | (uintptr_t)a->d_objectness[l] | (uintptr_t)a->d_box_regression[l]) & 3) != 0)
      return fail(VETO_ERR_INVALID, "level %d: misaligned floats", l);
  }
  if (!a->image_sizes || !a->tgt_boxes || !a->img_tgt_offset) return fail(VETO_ERR_INVALID, "missing pointer");
  if ((((uintptr_t)a->tgt_boxes | (uintptr_t)a->regression_targets) & 15) != 0)
    return fail(VETO_ERR_INVALID, "tgt_boxes and regression_targets must be 16-byte aligned");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_rpn_loss_workspace_bytes(a), true));
  RpnLossArgs p{};
  RpnFillArgs fill{};
  carve_rpn_loss(Carver{(char*)workspace}, a, n_anchor, &p);
  if (a->labels) p.labels_ws = a->labels;
  fill.ptr[0] = (float*)p.gtmax; fill.n[0] = a->n_tgt; fill.n_seg = 1;
  if (last_stage >= kRpnLossSample) { fill.ptr[1] = (float*)p.hist; fill.n[1] = (long long)a->n_img * 512; fill.n_seg = 2; }
  int off = 0;
  for (int l = 0; l < a->n_lvl; ++l) {
    RpnLossLevel& v = p.lvl[l];
    v.objectness = a->objectness[l]; v.regression = a->box_regression[l]; v.anchors = a->anchors[l];
    v.d_objectness = a->d_objectness[l]; v.d_regression = a->d_box_regression[l];
    v.A = a->level_a[l]; v.HW = a->level_h[l] * a->level_w[l]; v.N = v.A * v.HW; v.off = off;
    off += v.N;
    if (n_grad) {
      fill.ptr[fill.n_seg] = v.d_objectness; fill.n[fill.n_seg++] = (long long)a->n_img * v.N;
      fill.ptr[fill.n_seg] = v.d_regression; fill.n[fill.n_seg++] = (long long)a->n_img * v.N * 4;
    }
  }
  p.image_sizes = a->image_sizes; p.tgt_boxes = a->tgt_boxes; p.tgt_off = a->img_tgt_offset;
  p.n_img = a->n_img; p.n_lvl = a->n_lvl; p.n_anchor = n_anchor; p.batch = a->batch_size_per_image; p.num_pos = a->num_pos_per_img;
  p.allow_lowq = a->allow_low_quality_matches != 0;
  p.high = a->high_threshold; p.low = a->low_threshold; p.straddle = a->straddle_thresh;
  p.wx = a->reg_weights[0]; p.wy = a->reg_weights[1]; p.ww = a->reg_weights[2]; p.wh = a->reg_weights[3];
  p.beta = a->beta; p.seed = a->seed;
  p.losses = a->losses; p.matched = a->matched_idxs; p.targets = a->regression_targets; p.sampled = a->sampled_inds; p.counts = a->counts;
  HIP_TRY(launch_rpn_loss(p, fill, last_stage, (hipStream_t)stream));
  return VETO_OK;
}

// the host fields of the box loss arguments: 0, or an error (set)
static int box_loss_check_shapes(const veto_box_loss_args_t* a) {
  if (a->n_cls < 2 || a->n_cls > box_loss_max_cls()) return fail(VETO_ERR_INVALID, "n_cls %d outside 2..%d", a->n_cls, box_loss_max_cls());
  if (a->n_rows < 0 || a->n_rows > box_loss_max_rows()) return fail(VETO_ERR_INVALID, "n_rows %d outside 0..%d", a->n_rows, box_loss_max_rows());
  const int need_cols = a->cls_agnostic ? 8 : 4 * a->n_cls;
  if (a->n_reg_cols < need_cols || a->n_reg_cols % 4 != 0)
    return fail(VETO_ERR_INVALID, "n_reg_cols %d must be a multiple of 4 and >= %d (%s)", a->n_reg_cols, need_cols,
                a->cls_agnostic ? "cls_agnostic: columns 4..7" : "4 n_cls");
  if (a->ld_logits < a->n_cls) return fail(VETO_ERR_INVALID, "ld_logits %lld is below the row width %d", (long long)a->ld_logits, a->n_cls);
  if (a->ld_reg < a->n_reg_cols) return fail(VETO_ERR_INVALID, "ld_reg %lld is below the row width %d", (long long)a->ld_reg, a->n_reg_cols);
  return VETO_OK;
}

// workspace: the rows' partial pairs
static size_t carve_box_loss(Carver c, size_t n_rows, BoxLossArgs* p) {
  p->partial = c.take<double>(n_rows * 16 + 16);
  return c.off;
}

size_t veto_box_loss_workspace_bytes(const veto_box_loss_args_t* a) {
  if (!a || a->struct_size != (int32_t)sizeof(veto_box_loss_args_t)) return 0;
  if (box_loss_check_shapes(a) != VETO_OK) return 0;
  BoxLossArgs p{};
  return carve_box_loss(Carver{nullptr}, a->n_rows, &p);
}

int veto_box_loss(void* stream, const veto_box_loss_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_box_loss_args_t, a);
  ABI_TRY(box_loss_check_shapes(a));
  if (!a->losses) return fail(VETO_ERR_INVALID, "missing pointer: losses");
  if (a->n_rows > 0 && (!a->class_logits || !a->box_regression || !a->labels || !a->regression_targets))
    return fail(VETO_ERR_INVALID, "missing pointer: class_logits, box_regression, labels and regression_targets are required");
  if ((a->d_class_logits != nullptr) != (a->d_box_regression != nullptr))
    return fail(VETO_ERR_INVALID, "d_class_logits and d_box_regression: both or neither");
  if (((uintptr_t)a->regression_targets & 15) != 0) return fail(VETO_ERR_INVALID, "regression_targets must be 16-byte aligned");
  if ((((uintptr_t)a->d_class_logits | (uintptr_t)a->d_box_regression) & 15) != 0)
    return fail(VETO_ERR_INVALID, "d_class_logits and d_box_regression must be 16-byte aligned");
  if ((((uintptr_t)a->class_logits | (uintptr_t)a->box_regression | (uintptr_t)a->losses) & 3) != 0 || ((uintptr_t)a->labels & 7) != 0)
    return fail(VETO_ERR_INVALID, "misaligned class_logits, box_regression, losses or labels");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_box_loss_workspace_bytes(a), true));
  BoxLossArgs p{};
  p.logits = a->class_logits; p.reg = a->box_regression; p.labels = a->labels; p.targets = a->regression_targets;
  p.n_rows = a->n_rows; p.n_cls = a->n_cls; p.n_reg_cols = a->n_reg_cols; p.cls_agnostic = a->cls_agnostic != 0;
  p.ld_logits = a->ld_logits; p.ld_reg = a->ld_reg;
  carve_box_loss(Carver{(char*)workspace}, a->n_rows, &p);
  p.losses = a->losses; p.d_logits = a->d_class_logits; p.d_reg = a->d_box_regression;
  HIP_TRY(launch_box_loss(p, (hipStream_t)stream));
  return VETO_OK;
}

// shared argument check / conversion of veto_roi_pool, veto_roi_pool_backward and their adaptive-grid siblings (adaptive: the
// sampling ratio must be 0 and the maps NCHW; everything else is checked the same way, with the same messages)
static int roi_pool_args(const veto_roi_pool_args_t* a, bool forward, RoiPoolArgs* out, bool adaptive = false) {
  // two sizes: the struct before the map-form fields (float32 NCHW) and the current one, as veto_sgg_eval does for pred_obj_offset
  if (!a) return fail(VETO_ERR_INVALID, "veto_roi_pool_args_t is null");
  const bool has_forms = a->struct_size == (int32_t)sizeof(veto_roi_pool_args_t);
  if (!has_forms && a->struct_size != (int32_t)offsetof(veto_roi_pool_args_t, level_dtype))
    return fail(VETO_ERR_INVALID, "veto_roi_pool_args_t size mismatch");
  const int lv_dtype = has_forms ? a->level_dtype : VETO_ROI_F32, dp_dtype = has_forms ? a->depth_dtype : VETO_ROI_F32;
  const int lv_layout = has_forms ? a->level_layout : VETO_ROI_NCHW, dp_layout = has_forms ? a->depth_layout : VETO_ROI_NCHW;
  if (lv_dtype < VETO_ROI_F32 || lv_dtype > VETO_ROI_BF16 || dp_dtype < VETO_ROI_F32 || dp_dtype > VETO_ROI_BF16)
    return fail(VETO_ERR_INVALID, "level_dtype / depth_dtype must be 0 (float32), 1 (float16) or 2 (bfloat16), got %d / %d", lv_dtype, dp_dtype);
  if (lv_layout < VETO_ROI_NCHW || lv_layout > VETO_ROI_NHWC || dp_layout < VETO_ROI_NCHW || dp_layout > VETO_ROI_NHWC)
    return fail(VETO_ERR_INVALID, "level_layout / depth_layout must be 0 (NCHW) or 1 (NHWC), got %d / %d", lv_layout, dp_layout);
  if (a->n_levels < 1 || a->n_levels > 4) return fail(VETO_ERR_INVALID, "n_levels must be 1..4, got %d", a->n_levels);
  if (a->n_img <= 0 || a->n_roi <= 0 || a->channels <= 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_roi %d, channels %d)", a->n_img, a->n_roi, a->channels);
  if (a->pooled < 1 || a->pooled > 16) return fail(VETO_ERR_INVALID, "pooled must be 1..16, got %d", a->pooled);
  if (adaptive) {
    if (a->sampling_ratio != 0)
      return fail(VETO_ERR_INVALID, "sampling_ratio must be 0 for the adaptive entry points (veto_roi_pool takes 1..4), got %d", a->sampling_ratio);
    if (lv_layout == VETO_ROI_NHWC || dp_layout == VETO_ROI_NHWC)
      return fail(VETO_ERR_INVALID, "VETO_ROI_NHWC is not built for the adaptive grid: level_layout / depth_layout must be VETO_ROI_NCHW, got %d / %d",
                  lv_layout, dp_layout);
  } else {
    if (a->sampling_ratio < 1 || a->sampling_ratio > 4)
      return fail(VETO_ERR_INVALID, "sampling_ratio must be 1..4 (adaptive sampling is not built), got %d", a->sampling_ratio);
    if (a->pooled * a->sampling_ratio > 32)
      return fail(VETO_ERR_INVALID, "pooled * sampling_ratio must be at most 32 (the per-ROI axis tables), got %d x %d", a->pooled, a->sampling_ratio);
  }
  if (!a->rois || (forward && !a->out_rgb))
    return fail(VETO_ERR_INVALID, "missing pointer:%s%s", !a->rois ? " rois [n_roi, 5]" : "",
                forward && !a->out_rgb ? " out_rgb [n_roi, channels, pooled, pooled]" : "");
  const bool has_depth = forward ? a->depth_feat != nullptr : a->depth_h > 0;
  if (has_depth && ((forward && !a->out_depth) || a->depth_channels <= 0 || a->depth_h <= 0 || a->depth_w <= 0))
    return fail(VETO_ERR_INVALID, "depth map given without out_depth / sizes");
  RoiPoolArgs p{};
  // the backward reads the layouts only: its gradient maps are float32
  p.lv_dtype = forward ? lv_dtype : kRoiF32; p.depth_dtype = forward ? dp_dtype : kRoiF32;
  p.lv_layout = lv_layout; p.depth_layout = dp_layout;
  const uintptr_t lv_mask = p.lv_dtype == kRoiF32 ? 3 : 1, dp_mask = p.depth_dtype == kRoiF32 ? 3 : 1;
  if (forward && has_depth && ((uintptr_t)a->depth_feat & dp_mask) != 0) return fail(VETO_ERR_INVALID, "depth_feat is not aligned to its element type");
  for (int l = 0; l < a->n_levels; ++l) {
    if (forward && ((uintptr_t)a->level_feat[l] & lv_mask) != 0) return fail(VETO_ERR_INVALID, "level_feat[%d] is not aligned to its element type", l);
    if ((forward && !a->level_feat[l]) || a->level_h[l] <= 0 || a->level_w[l] <= 0 || !(a->level_scale[l] > 0.f))
      return fail(VETO_ERR_INVALID, "bad pyramid level %d", l);
    p.lv[l] = RoiLevel{a->level_feat[l], a->level_h[l], a->level_w[l], a->level_scale[l]};
  }
  p.n_levels = a->n_levels;
  // poolers.py:86-88: the level range follows from the first and last scale
  p.k_min = (int)lroundf(-log2f(a->level_scale[0]));
  p.k_max = (int)lroundf(-log2f(a->level_scale[a->n_levels - 1]));
  if (has_depth) {
    const int dl = a->n_levels > 1 ? 2 : 0;  // poolers.py:146-149
    if (dl >= a->n_levels) return fail(VETO_ERR_INVALID, "the depth pooler is level 2; need at least 3 levels or exactly 1");
    p.depth = RoiLevel{a->depth_feat, a->depth_h, a->depth_w, a->level_scale[dl]};
  }
  p.n_roi = a->n_roi; p.channels = a->channels; p.depth_channels = has_depth ? a->depth_channels : 0;
  p.pooled = a->pooled; p.sampling_ratio = a->sampling_ratio;
  p.rois = a->rois; p.out_rgb = a->out_rgb; p.out_depth = a->out_depth; p.out_levels = a->out_levels;
  *out = p;
  return VETO_OK;
}

int veto_roi_pool(void* stream, const veto_roi_pool_args_t* a) {
  RoiPoolArgs p{};
  ABI_TRY(roi_pool_args(a, true, &p));
  HIP_TRY(launch_roi_pool(p, (hipStream_t)stream));
  return VETO_OK;
}

static int roi_pool_backward(void* stream, const veto_roi_pool_args_t* a, const float* grad_rgb, const float* grad_depth,
                             float* const* level_grad, float* depth_grad, bool ordered, bool adaptive = false) {
  RoiPoolArgs p{};
  ABI_TRY(roi_pool_args(a, false, &p, adaptive));
  if (!grad_rgb || !level_grad) return fail(VETO_ERR_INVALID, "missing gradient pointer");
  for (int l = 0; l < p.n_levels; ++l) {
    if (!level_grad[l]) return fail(VETO_ERR_INVALID, "level_grad[%d] is null", l);
    p.lv_grad[l] = level_grad[l];
  }
  if ((grad_depth != nullptr) != (depth_grad != nullptr)) return fail(VETO_ERR_INVALID, "grad_depth and depth_grad go together");
  if (grad_depth && p.depth.H <= 0) return fail(VETO_ERR_INVALID, "depth gradient without depth sizes in args");
  if (grad_depth) p.depth.feat = grad_depth;   // only its non-null-ness and the sizes are used
  else p.depth.feat = nullptr;
  p.gout_rgb = grad_rgb; p.gout_depth = grad_depth; p.depth_grad = depth_grad;
  if (adaptive) HIP_TRY(launch_roi_pool_adaptive_backward(p, (hipStream_t)stream));
  else if (ordered) HIP_TRY(launch_roi_pool_backward_ordered(p, a->n_img, (hipStream_t)stream));
  else HIP_TRY(launch_roi_pool_backward(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_roi_pool_backward(void* stream, const veto_roi_pool_args_t* a, const float* grad_rgb, const float* grad_depth,
                           float* const* level_grad, float* depth_grad) {
  return roi_pool_backward(stream, a, grad_rgb, grad_depth, level_grad, depth_grad, false);
}

int veto_roi_pool_backward_ordered(void* stream, const veto_roi_pool_args_t* a, const float* grad_rgb, const float* grad_depth,
                                   float* const* level_grad, float* depth_grad) {
  return roi_pool_backward(stream, a, grad_rgb, grad_depth, level_grad, depth_grad, true);
}

int veto_roi_pool_adaptive(void* stream, const veto_roi_pool_args_t* a) {
  RoiPoolArgs p{};
  ABI_TRY(roi_pool_args(a, true, &p, true));
  HIP_TRY(launch_roi_pool_adaptive(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_roi_pool_adaptive_backward(void* stream, const veto_roi_pool_args_t* a, const float* grad_rgb, const float* grad_depth,
                                    float* const* level_grad, float* depth_grad) {
  return roi_pool_backward(stream, a, grad_rgb, grad_depth, level_grad, depth_grad, false, true);
}

// workspace: label_tmp | flag_tmp | flag_before | pair_score | row_key | acc_first | cls_table
static size_t carve_sgg_eval(Carver c, size_t n_img, size_t n_pair_total, size_t n_gt_total, int n_rel_cls, SggEvalArgs* p) {
  const size_t per_pair = n_pair_total * 4 + 4;
  p->label_tmp = c.take<int32_t>(per_pair);
  p->flag_tmp = c.take<int32_t>(per_pair);
  p->flag_before = c.take<int32_t>(per_pair);
  p->pair_score = c.take<float>(per_pair);
  p->row_key = c.take<uint32_t>(per_pair);
  p->acc_first = c.take<int32_t>(n_gt_total * 4 + 4);
  p->cls_table = c.take<int32_t>(n_img * 7 * n_rel_cls * 4);
  return c.off;
}

size_t veto_sgg_eval_workspace_bytes(int32_t n_img, int32_t n_pair_total, int32_t n_gt_total, int32_t n_rel_cls) {
  if (n_img <= 0 || n_pair_total < 0 || n_gt_total < 0 || n_rel_cls < 2) return 0;
  SggEvalArgs p{};
  return carve_sgg_eval(Carver{nullptr}, n_img, n_pair_total, n_gt_total, n_rel_cls, &p);
}

int veto_sgg_eval(void* stream, const veto_sgg_eval_args_t* a, int32_t n_pair_total, int32_t n_gt_total, void* workspace,
                  size_t workspace_bytes) {
  if (!a || !workspace) return fail(VETO_ERR_INVALID, "null argument");
  // the struct before pred_obj_offset was appended is still accepted (GT-box modes, pred_obj_offset = NULL)
  const bool has_pred_off = a->struct_size == (int32_t)sizeof(veto_sgg_eval_args_t);
  if (!has_pred_off && a->struct_size != (int32_t)offsetof(veto_sgg_eval_args_t, pred_obj_offset))
    return fail(VETO_ERR_INVALID, "veto_sgg_eval_args_t size mismatch");
  if (a->reserved0 != 0 && a->reserved0 != 1) return fail(VETO_ERR_INVALID, "mode (reserved0) must be 0 (GT boxes) or 1 (sgdet)");
  const int32_t* pred_off = has_pred_off ? a->pred_obj_offset : nullptr;
  if (a->reserved0 == 1 && !pred_off) return fail(VETO_ERR_INVALID, "sgdet needs pred_obj_offset");
  if (a->n_img <= 0 || a->n_rel_cls < 2 || a->n_rel_cls > 4096 || a->n_zeroshot < 0 || n_pair_total < 0 || n_gt_total < 0)
    return fail(VETO_ERR_INVALID, "bad sizes");
  if (!(a->iou_thres >= 0.f && a->iou_thres <= 1.f)) return fail(VETO_ERR_INVALID, "iou_thres must be in [0, 1]");
  if (!a->gt_offset || !a->obj_offset || !a->pair_offset || !a->gt_rels || !a->gt_classes || !a->gt_boxes || !a->pred_pairs ||
      !a->rel_scores || !a->pred_classes || !a->pred_boxes || !a->obj_scores || (a->n_zeroshot > 0 && !a->zeroshot) ||
      !a->gc_rank || !a->ng_rank || !a->acc_rank || !a->zeroshot_flag || !a->ng_rows || !a->ng_cols || !a->ng_count || !a->metrics)
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_sgg_eval_workspace_bytes(a->n_img, n_pair_total, n_gt_total, a->n_rel_cls), false));
  SggEvalArgs p{};
  p.n_img = a->n_img; p.n_rel_cls = a->n_rel_cls; p.n_zeroshot = a->n_zeroshot; p.iou_thres = a->iou_thres;
  p.gt_off = a->gt_offset; p.obj_off = a->obj_offset; p.pair_off = a->pair_offset;
  p.pred_obj_off = pred_off; p.mode = a->reserved0;
  p.gt_rels = a->gt_rels; p.gt_classes = a->gt_classes; p.gt_boxes = a->gt_boxes;
  p.pred_pairs = a->pred_pairs; p.rel_scores = a->rel_scores; p.pred_classes = a->pred_classes;
  p.pred_boxes = a->pred_boxes; p.obj_scores = a->obj_scores; p.zeroshot = a->zeroshot;
  p.gc_rank = a->gc_rank; p.ng_rank = a->ng_rank; p.acc_rank = a->acc_rank; p.zeroshot_flag = a->zeroshot_flag;
  p.ng_rows = a->ng_rows; p.ng_cols = a->ng_cols; p.ng_count = a->ng_count; p.metrics = a->metrics;
  carve_sgg_eval(Carver{(char*)workspace}, a->n_img, n_pair_total, n_gt_total, a->n_rel_cls, &p);
  HIP_TRY(launch_sgg_eval(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_sgg_eval_fold_limits(int32_t* images_per_chunk, int32_t* max_rel_cls) {
  if (images_per_chunk) *images_per_chunk = sgg_eval_fold_images_per_chunk();
  if (max_rel_cls) *max_rel_cls = sgg_eval_fold_max_rel_cls();
  return VETO_OK;
}

// workspace: one row of partial sums per image chunk
static size_t carve_sgg_eval_fold(Carver c, size_t n_img, int n_rel_cls, SggEvalFoldArgs* p) {
  p->partial = c.take<double>((sgg_eval_fold_chunks(n_img) * sgg_eval_fold_partial_doubles(n_rel_cls) + 1) * 8);
  return c.off;
}

size_t veto_sgg_eval_fold_workspace_bytes(int32_t n_img, int32_t n_rel_cls) {
  if (n_img < 0 || n_rel_cls < 2 || n_rel_cls > sgg_eval_fold_max_rel_cls()) return 0;
  SggEvalFoldArgs p{};
  return carve_sgg_eval_fold(Carver{nullptr}, (size_t)n_img, n_rel_cls, &p);
}

int veto_sgg_eval_fold(void* stream, const veto_sgg_eval_fold_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_sgg_eval_fold_args_t, a);
  if (a->n_rel_cls < 2 || a->n_rel_cls > sgg_eval_fold_max_rel_cls())
    return fail(VETO_ERR_INVALID, "n_rel_cls %d outside 2..%d", a->n_rel_cls, sgg_eval_fold_max_rel_cls());
  if (a->mode != 0 && a->mode != 1) return fail(VETO_ERR_INVALID, "mode must be 0 (GT boxes) or 1 (sgdet)");
  if (a->n_img < 0 || a->n_gt_total < 0) return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_gt_total %d)", a->n_img, a->n_gt_total);
  if (!a->img_gt_offset || (a->n_img > 0 && !a->img_pair_count) || !a->metrics ||
      (a->n_gt_total > 0 && (!a->gt_predicate || !a->gc_rank || !a->ng_rank || !a->acc_rank || !a->zeroshot_flag)))
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_sgg_eval_fold_workspace_bytes(a->n_img, a->n_rel_cls), true));
  SggEvalFoldArgs p{};
  p.n_img = a->n_img; p.n_rel_cls = a->n_rel_cls; p.mode = a->mode; p.n_gt_total = a->n_gt_total;
  p.img_gt_off = a->img_gt_offset; p.img_pair_cnt = a->img_pair_count;
  p.gt_predicate = a->gt_predicate; p.gc_rank = a->gc_rank; p.ng_rank = a->ng_rank; p.acc_rank = a->acc_rank;
  p.zeroshot_flag = a->zeroshot_flag; p.metrics = a->metrics; p.per_image = a->per_image;
  carve_sgg_eval_fold(Carver{(char*)workspace}, (size_t)a->n_img, a->n_rel_cls, &p);
  HIP_TRY(launch_sgg_eval_fold(p, (hipStream_t)stream));
  return VETO_OK;
}

int veto_det_eval_limits(int32_t* max_gt_per_image, int32_t* max_det_per_image, int32_t* scan_chunk, int32_t* sort_tile) {
  if (max_gt_per_image) *max_gt_per_image = det_eval_max_gt();
  if (max_det_per_image) *max_det_per_image = det_eval_max_det();
  if (scan_chunk) *scan_chunk = det_eval_scan_chunk();
  if (sort_tile) *sort_tile = det_eval_sort_tile();
  return VETO_OK;
}

// workspace: the "GT taken" flags
static size_t carve_det_eval_match(Carver c, size_t n_gt, DetEvalMatchArgs* p) {
  p->gtm = c.take<uint8_t>(n_gt * kDetEvalThrs * kDetEvalAreas + 1);
  return c.off;
}

size_t veto_det_eval_match_workspace_bytes(int32_t n_img, int32_t n_gt, int32_t n_det) {
  if (n_img <= 0 || n_gt < 0 || n_det < 0) return 0;
  DetEvalMatchArgs p{};
  return carve_det_eval_match(Carver{nullptr}, n_gt, &p);
}

int veto_det_eval_match(void* stream, const veto_det_eval_match_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_det_eval_match_args_t, a);
  if (a->n_cls < 2 || a->n_cls > 1024) return fail(VETO_ERR_INVALID, "n_cls %d outside 2..1024", a->n_cls);
  if (a->n_img <= 0 || a->n_gt < 0 || a->n_det < 0)
    return fail(VETO_ERR_INVALID, "bad sizes (n_img %d, n_gt %d, n_det %d)", a->n_img, a->n_gt, a->n_det);
  if (a->row_offset < 0 || a->row_offset + (int64_t)a->n_det >= ((int64_t)1 << 31))
    return fail(VETO_ERR_INVALID, "row_offset %lld + n_det %d: the record total must stay below 2^31", (long long)a->row_offset, a->n_det);
  if (!a->gt_offset_host || !a->det_offset_host) return fail(VETO_ERR_INVALID, "missing pointer: host offsets");
  if (check_host_offsets(a->gt_offset_host, a->n_img, a->n_gt, det_eval_max_gt(), "gt_offset_host", "n_gt") < 0) return VETO_ERR_INVALID;
  if (check_host_offsets(a->det_offset_host, a->n_img, a->n_det, det_eval_max_det(), "det_offset_host", "n_det") < 0) return VETO_ERR_INVALID;
  for (int t = 0; t < kDetEvalThrs; ++t)
    if (!(a->iou_thrs[t] > 0.0 && a->iou_thrs[t] <= 1.0)) return fail(VETO_ERR_INVALID, "iou_thrs[%d] = %g outside (0, 1]", t, a->iou_thrs[t]);
  for (int r = 0; r < kDetEvalAreas; ++r)
    if (!(a->area_rngs[2 * r] <= a->area_rngs[2 * r + 1])) return fail(VETO_ERR_INVALID, "area_rngs[%d]: lo above hi (or NaN)", r);
  if ((a->n_gt > 0 && (!a->gt_boxes || !a->gt_labels)) || (a->n_det > 0 && (!a->det_boxes || !a->det_scores || !a->det_labels || !a->rec_key ||
      !a->rec_match || !a->rec_ignore)) || !a->gt_offset || !a->det_offset || !a->gt_counts)
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_det_eval_match_workspace_bytes(a->n_img, a->n_gt, a->n_det), true));
  DetEvalMatchArgs p{};
  p.n_img = a->n_img; p.n_cls = a->n_cls; p.first_gt_id = a->first_gt_id; p.row_offset = a->row_offset;
  for (int t = 0; t < kDetEvalThrs; ++t) p.iou_thrs[t] = a->iou_thrs[t];
  for (int r = 0; r < 2 * kDetEvalAreas; ++r) p.area_rngs[r] = a->area_rngs[r];
  p.gt_off = a->gt_offset; p.det_off = a->det_offset;
  p.gt_boxes = a->gt_boxes; p.gt_labels = a->gt_labels;
  p.det_boxes = a->det_boxes; p.det_scores = a->det_scores; p.det_labels = a->det_labels;
  p.rec_key = (unsigned long long*)a->rec_key; p.rec_match = (unsigned long long*)a->rec_match; p.rec_ignore = (unsigned long long*)a->rec_ignore;
  p.npig = (unsigned long long*)a->gt_counts; p.label_errors = a->label_errors;
  carve_det_eval_match(Carver{(char*)workspace}, a->n_gt, &p);
  HIP_TRY(launch_det_eval_match(p, (hipStream_t)stream));
  return VETO_OK;
}

// workspace: key_a | key_b | idx_a | idx_b | hist | seg_start
static size_t carve_det_eval_accumulate(Carver c, size_t n_rec, int n_cls, DetEvalAccumArgs* p) {
  p->key_a = c.take<unsigned long long>(n_rec * 8 + 8);
  p->key_b = c.take<unsigned long long>(n_rec * 8 + 8);
  p->idx_a = c.take<uint32_t>(n_rec * 4 + 4);
  p->idx_b = c.take<uint32_t>(n_rec * 4 + 4);
  p->hist = c.take<uint32_t>((size_t)det_eval_sort_tiles((long long)n_rec) * 256 * 4);
  p->seg_start = c.take<int32_t>(((size_t)n_cls + 1) * 4);
  return c.off;
}

size_t veto_det_eval_accumulate_workspace_bytes(int64_t n_rec, int32_t n_cls) {
  if (n_rec < 0 || n_rec >= ((int64_t)1 << 31) || n_cls < 2 || n_cls > 1024) return 0;
  DetEvalAccumArgs p{};
  return carve_det_eval_accumulate(Carver{nullptr}, (size_t)n_rec, n_cls, &p);
}

int veto_det_eval_accumulate(void* stream, const veto_det_eval_accumulate_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_det_eval_accumulate_args_t, a);
  if (a->n_cls < 2 || a->n_cls > 1024) return fail(VETO_ERR_INVALID, "n_cls %d outside 2..1024", a->n_cls);
  if (a->n_rec < 0 || a->n_rec >= ((int64_t)1 << 31)) return fail(VETO_ERR_INVALID, "n_rec %lld outside 0..2^31-1", (long long)a->n_rec);
  for (int r = 1; r < kDetEvalRecThrs; ++r)
    if (!(a->rec_thrs[r - 1] <= a->rec_thrs[r])) return fail(VETO_ERR_INVALID, "rec_thrs must be non-decreasing (entry %d)", r);
  if ((a->n_rec > 0 && (!a->rec_key || !a->rec_match || !a->rec_ignore)) || !a->gt_counts || !a->precision || !a->recall || !a->stats ||
      !a->recall50_100)
    return fail(VETO_ERR_INVALID, "missing pointer");
  ABI_TRY(check_workspace(workspace, workspace_bytes, veto_det_eval_accumulate_workspace_bytes(a->n_rec, a->n_cls), true));
  DetEvalAccumArgs p{};
  p.n_cls = a->n_cls; p.n_rec = a->n_rec;
  for (int t = 0; t < kDetEvalThrs; ++t) p.iou_thrs[t] = a->iou_thrs[t];
  for (int r = 0; r < kDetEvalRecThrs; ++r) p.rec_thrs[r] = a->rec_thrs[r];
  p.rec_key = (const unsigned long long*)a->rec_key; p.rec_match = (const unsigned long long*)a->rec_match;
  p.rec_ignore = (const unsigned long long*)a->rec_ignore; p.npig = (const unsigned long long*)a->gt_counts;
  p.precision = a->precision; p.recall = a->recall; p.stats = a->stats; p.recall50_100 = a->recall50_100;
  carve_det_eval_accumulate(Carver{(char*)workspace}, (size_t)a->n_rec, a->n_cls, &p);
  HIP_TRY(launch_det_eval_accumulate(p, (hipStream_t)stream));
  return VETO_OK;
}

}  // extern "C"
