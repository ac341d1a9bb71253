"""ctypes binding of the C ABI declared in include/veto_amd.h (libveto_amd.so), and the one call path the wrappers share
(Launch, device_offsets).

There is no fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import itertools
import os

# PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be
# mapped BEFORE libveto_amd.so so that the library's NEEDED libamdhip64.so.7 resolves to that same copy;
# the other order maps two runtimes into the process and the second one finds no device.
import torch  # noqa: F401
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64,
                    c_size_t, c_uint32, c_uint64, c_void_p)

_LIB = None

VETO_PRECISE, VETO_FAST, VETO_MIXED = 0, 1, 2
VETO_ATTN_BWD_CLS_ONLY, VETO_ATTN_BWD_QKV_F24, VETO_ATTN_BWD_SPLIT_OUT = 1, 2, 4   # veto_debug_attention_backward_forms flags


class VetoConfig(Structure):
    _fields_ = [(n, c_int32) for n in (
        "struct_size", "dim", "layers", "heads", "patch", "channels", "resolution", "num_obj_cls",
        "embed_dim", "num_out", "precision", "device", "max_chunk_pairs")]


class VetoInputs(Structure):
    _fields_ = [
        ("struct_size", c_int32), ("n_obj", c_int32), ("n_pair", c_int32), ("n_img", c_int32),
        ("roi_rgb", c_void_p), ("roi_depth", c_void_p), ("boxes", c_void_p),
        ("box_mode", c_int32), ("reserved0", c_int32),
        ("obj_labels", c_void_p), ("obj_logits", c_void_p), ("rel_pairs", c_void_p),
        ("img_obj_offset", c_void_p), ("img_pair_offset", c_void_p), ("bn_batch_stats", c_void_p),
    ]


class VetoDebugOutputs(Structure):
    _fields_ = [
        ("struct_size", c_int32), ("reserved0", c_int32),
        ("subj_inds", c_void_p), ("obj_inds", c_void_p), ("tokens", c_void_p), ("cls", c_void_p),
    ]


class VetoSaturation(Structure):
    _fields_ = [(n, c_int64) for n in ("elements", "f16_saturated", "value_saturated", "resid_saturated")]


SATURATION_SITES = ("qkv_in", "attn_out", "ffn_in", "hidden")       # enum veto_saturation_site


class VetoPostArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_obj", "n_pair", "n_rel_cls", "n_obj_cls",
                                       "max_pairs_per_image", "reserved0")] + \
               [(n, c_void_p) for n in ("rel_logits", "obj_logits", "rel_pairs", "img_obj_offset", "img_pair_offset",
                                        "obj_scores", "obj_pred", "rel_prob_sorted", "rel_pairs_sorted",
                                        "rel_labels_sorted", "triple_sorted")]


class VetoObjDecodeArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_obj", "n_cls", "max_obj_per_image", "mode")] + \
               [("nms_thres", ctypes.c_float), ("reserved0", c_int32)] + \
               [(n, c_void_p) for n in ("logits", "labels", "boxes_per_cls", "img_obj_offset", "obj_pred", "obj_scores", "boxes")]


class VetoPairArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_obj", "max_obj_per_image", "max_pairs",
                                       "require_overlap")] + \
               [(n, c_void_p) for n in ("boxes", "scores", "img_obj_offset", "img_out_offset", "pairs", "counts")]


class VetoNmsArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_box", "n_seg", "max_keep")] + \
               [("threshold", ctypes.c_float), ("reserved0", c_int32)] + \
               [(n, c_void_p) for n in ("boxes", "scores", "seg_offset", "seg_offset_host", "keep", "counts")]


class VetoBoxPostArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_box", "n_cls", "reg_cols", "cls_agnostic",
                                       "post_nms_per_cls_topn", "filter_duplicates", "detections_per_img")] + \
               [(n, ctypes.c_float) for n in ("score_thresh", "nms_thresh", "bbox_xform_clip")] + \
               [("reg_weights", ctypes.c_float * 4)] + \
               [(n, c_void_p) for n in ("class_logits", "box_regression", "proposals", "image_sizes", "img_offset",
                                        "img_offset_host", "img_out_offset", "orig_inds", "pred_labels", "pred_scores",
                                        "boxes", "boxes_per_cls", "counts")]


RPN_MAX_LEVELS = 8   # VETO_RPN_MAX_LEVELS


class VetoRpnArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_lvl", "pre_nms_top_n", "post_nms_top_n", "fpn_post_nms_top_n",
                                       "per_batch")] + \
               [(n, ctypes.c_float) for n in ("nms_thresh", "min_size", "bbox_xform_clip")] + \
               [("reg_weights", ctypes.c_float * 4)] + \
               [(n, c_int32 * RPN_MAX_LEVELS) for n in ("level_a", "level_h", "level_w")] + \
               [(n, c_void_p * RPN_MAX_LEVELS) for n in ("objectness", "box_regression", "anchors")] + \
               [(n, c_void_p) for n in ("image_sizes", "img_out_offset", "boxes", "objectness_out", "level", "anchor_index",
                                        "counts")]


class VetoAnchorArgs(Structure):
    _fields_ = [("struct_size", c_int32), ("n_img", c_int32), ("n_lvl", c_int32), ("straddle_thresh", ctypes.c_float)] + \
               [(n, c_int32 * RPN_MAX_LEVELS) for n in ("level_a", "level_h", "level_w", "level_stride")] + \
               [("cell_anchors", c_void_p * RPN_MAX_LEVELS)] + \
               [(n, c_void_p) for n in ("image_sizes", "anchors", "anchors_in", "visibility")]


class VetoDetectRelsampleArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_prp", "n_tgt", "n_rel_cells", "max_prp_per_image",
                                       "max_tgt_per_image", "require_overlap", "num_sample_per_gt_rel",
                                       "batch_size_per_image", "max_fg_per_image")] + \
               [("fg_thres", ctypes.c_float), ("seed", ctypes.c_uint64)] + \
               [(n, c_void_p) for n in ("prp_boxes", "prp_labels", "prp_scores", "tgt_boxes", "tgt_labels", "relation",
                                        "relation_non_masked", "img_prp_offset", "img_tgt_offset", "img_rel_offset",
                                        "img_binary_offset", "pairs", "labels", "labels_all", "binary_rel",
                                        "locating_match", "counts")]


class VetoGtboxRelsampleArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_rel_cells", "max_obj_per_image", "batch_size_per_image",
                                       "num_pos_per_img")] + \
               [("seed", ctypes.c_uint64)] + \
               [(n, c_void_p) for n in ("relation", "img_obj_offset", "img_rel_offset", "pairs", "labels", "binary_rel",
                                        "counts")]


class VetoBoxMatchArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_prp", "n_tgt", "mode")] + \
               [("high_threshold", ctypes.c_float), ("low_threshold", ctypes.c_float), ("reg_weights", ctypes.c_float * 4),
                ("reserved0", c_int32)] + \
               [(n, c_void_p) for n in ("prp_boxes", "tgt_boxes", "tgt_labels", "img_prp_offset", "img_tgt_offset",
                                        "img_prp_offset_host", "img_tgt_offset_host", "matched_idxs", "labels", "matched_rows",
                                        "regression_targets")]


class VetoBoxSubsampleArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_prp", "batch_size_per_image", "num_pos_per_img", "reserved0")] + \
               [("seed", ctypes.c_uint64)] + \
               [(n, c_void_p) for n in ("labels", "img_prp_offset", "img_prp_offset_host", "sampled_inds", "counts")]


class VetoRpnLossArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_lvl", "n_tgt", "batch_size_per_image", "num_pos_per_img",
                                       "allow_low_quality_matches", "reserved0")] + \
               [(n, ctypes.c_float) for n in ("high_threshold", "low_threshold", "straddle_thresh", "reserved1")] + \
               [("reg_weights", ctypes.c_float * 4), ("beta", c_double), ("seed", ctypes.c_uint64)] + \
               [(n, c_int32 * RPN_MAX_LEVELS) for n in ("level_a", "level_h", "level_w")] + \
               [(n, c_void_p * RPN_MAX_LEVELS) for n in ("objectness", "box_regression", "anchors", "d_objectness",
                                                         "d_box_regression")] + \
               [(n, c_void_p) for n in ("image_sizes", "tgt_boxes", "img_tgt_offset", "img_tgt_offset_host", "losses", "labels",
                                        "matched_idxs", "regression_targets", "sampled_inds", "counts")]


class VetoBoxLossArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_rows", "n_cls", "n_reg_cols", "cls_agnostic", "reserved0")] + \
               [("ld_logits", c_int64), ("ld_reg", c_int64)] + \
               [(n, c_void_p) for n in ("class_logits", "box_regression", "labels", "regression_targets", "losses",
                                        "d_class_logits", "d_box_regression")]


class VetoOptimTensor(Structure):
    _fields_ = [(n, c_void_p) for n in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("numel", c_int64), ("step", c_int64)] + \
               [(n, c_double) for n in ("lr", "weight_decay", "beta1", "beta2", "eps")]


class VetoOptimArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "tensor_size", "n_tensors", "mode")] + [("max_norm", c_double)] + \
               [("tensors", POINTER(VetoOptimTensor))] + [(n, c_void_p) for n in ("norms", "total_norm", "coef")]


VETO_OPTIM_NORMS, VETO_OPTIM_CLIP, VETO_OPTIM_STEP, VETO_OPTIM_CLIP_STEP = 0, 1, 2, 3   # veto_optim_args_t.mode
VETO_OPTIM_CHUNK = 8192


class VetoPostMeetArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_obj", "n_pair", "n_groups", "n_rel_cls", "n_obj_cls")] + \
               [(n, c_void_p) for n in ("group_logits", "group_widths", "incre_idx_list", "obj_logits", "rel_pairs",
                                        "obj_scores", "obj_pred", "rel_prob_sorted", "rel_pairs_sorted",
                                        "rel_labels_sorted", "triple_sorted")]


class VetoPostVoteArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_obj", "n_pair", "n_groups", "n_rel_cls", "n_obj_cls",
                                       "voting", "reserved0")] + \
               [(n, c_void_p) for n in ("expert_logits", "group_widths", "incre_idx_list", "obj_logits", "rel_pairs",
                                        "obj_scores", "obj_pred", "rel_prob_sorted", "rel_pairs_sorted",
                                        "rel_labels_sorted", "triple_sorted", "kept_count")]


class VetoPostGroupsBatchArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_obj", "n_pair", "n_groups", "experts_per_group", "n_rel_cls",
                                       "n_obj_cls", "voting", "max_pairs_per_image")] + \
               [(n, c_void_p) for n in ("head_logits", "group_widths", "incre_idx_list", "pairs_per_image", "obj_logits",
                                        "rel_pairs", "img_obj_offset", "img_pair_offset", "obj_scores", "obj_pred",
                                        "rel_prob_sorted", "rel_pairs_sorted", "rel_labels_sorted", "triple_sorted", "kept_count")]


class VetoRoiPoolArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_levels", "n_img", "n_roi", "channels", "depth_channels",
                                       "pooled", "sampling_ratio")] + \
               [("level_feat", c_void_p * 4), ("level_h", c_int32 * 4), ("level_w", c_int32 * 4),
                ("level_scale", ctypes.c_float * 4), ("depth_feat", c_void_p), ("depth_h", c_int32),
                ("depth_w", c_int32), ("rois", c_void_p), ("out_rgb", c_void_p), ("out_depth", c_void_p),
                ("out_levels", c_void_p)] + \
               [(n, c_int32) for n in ("level_dtype", "depth_dtype", "level_layout", "depth_layout")]


VETO_ROI_F32, VETO_ROI_F16, VETO_ROI_BF16 = 0, 1, 2   # veto_roi_pool_args_t.level_dtype / depth_dtype
VETO_ROI_NCHW, VETO_ROI_NHWC = 0, 1                    # veto_roi_pool_args_t.level_layout / depth_layout
ROI_POOL_ARGS_SIZE_V1 = VetoRoiPoolArgs.level_dtype.offset   # the struct before the map-form fields: means float32 NCHW


class VetoSggEvalArgs(Structure):
    _fields_ = [("struct_size", c_int32), ("n_img", c_int32), ("n_rel_cls", c_int32), ("n_zeroshot", c_int32),
                ("iou_thres", ctypes.c_float), ("reserved0", c_int32)] + \
               [(n, c_void_p) for n in ("gt_offset", "obj_offset", "pair_offset", "gt_rels", "gt_classes", "gt_boxes",
                                        "pred_pairs", "rel_scores", "pred_classes", "pred_boxes", "obj_scores", "zeroshot",
                                        "gc_rank", "ng_rank", "acc_rank", "zeroshot_flag", "ng_rows", "ng_cols", "ng_count",
                                        "metrics", "pred_obj_offset")]


class VetoSggEvalFoldArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_rel_cls", "mode", "n_gt_total", "reserved0")] + \
               [(n, c_void_p) for n in ("img_gt_offset", "img_pair_count", "gt_predicate", "gc_rank", "ng_rank", "acc_rank",
                                        "zeroshot_flag", "metrics", "per_image")]


class VetoDetEvalMatchArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "n_img", "n_cls", "n_gt", "n_det", "reserved0")] + \
               [("first_gt_id", c_int64), ("row_offset", c_int64), ("iou_thrs", c_double * 10), ("area_rngs", c_double * 8)] + \
               [(n, c_void_p) for n in ("gt_offset", "det_offset", "gt_offset_host", "det_offset_host", "gt_boxes", "gt_labels",
                                        "det_boxes", "det_scores", "det_labels", "rec_key", "rec_match", "rec_ignore",
                                        "gt_counts", "label_errors")]


class VetoDetEvalAccumulateArgs(Structure):
    _fields_ = [("struct_size", c_int32), ("n_cls", c_int32), ("n_rec", c_int64), ("iou_thrs", c_double * 10),
                ("rec_thrs", c_double * 101)] + \
               [(n, c_void_p) for n in ("rec_key", "rec_match", "rec_ignore", "gt_counts", "precision", "recall", "stats",
                                        "recall50_100")]


class VetoTrainOpts(Structure):
    _fields_ = [("struct_size", c_int32), ("p_pos", ctypes.c_float), ("p_emb", ctypes.c_float), ("p_attn", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("d_roi_rgb", c_void_p), ("d_roi_depth", c_void_p), ("deterministic", c_int32)]


class VetoTrainPlan(Structure):
    _fields_ = [("struct_size", c_int32), ("bn_eval", c_int32), ("trainable", c_void_p), ("p_attn_layer", c_void_p),
                ("d_roi", c_int32), ("frozen_fused", c_int32)]


BUILD_KINDS = ("split_rows", "mixed_rows", "patch", "loc_t", "cls_t", "head_t", "qkv0", "fold")   # enum veto_build_kind


class VetoMeetSampleArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("struct_size", "mode", "n", "n_words", "n_groups", "n_cls")] + \
               [(n, c_void_p) for n in ("labels", "words", "incre_idx_list", "pos_in_group", "group_size", "sample_rates",
                                        "chosen", "group_labels", "counts", "words_used")]


VETO_MEET_RAND_INSERT, VETO_MEET_RAND_CHOOSE, VETO_MEET_ALL_INCLUDE = 0, 1, 2   # enum veto_meet_pad_mode
MEET_PAD_MODES = {"rand_insert": VETO_MEET_RAND_INSERT, "rand_choose": VETO_MEET_RAND_CHOOSE, "all_include": VETO_MEET_ALL_INCLUDE}


STRUCTS = {   # C typedef name in include/veto_amd.h -> its mirror (tests/test_abi_symbols.py compares every field's offset and size)
    "veto_config_t": VetoConfig, "veto_inputs_t": VetoInputs, "veto_debug_outputs_t": VetoDebugOutputs,
    "veto_saturation_t": VetoSaturation, "veto_post_args_t": VetoPostArgs, "veto_post_meet_args_t": VetoPostMeetArgs,
    "veto_post_vote_args_t": VetoPostVoteArgs, "veto_post_groups_batch_args_t": VetoPostGroupsBatchArgs, "veto_obj_decode_args_t": VetoObjDecodeArgs, "veto_pair_args_t": VetoPairArgs,
    "veto_nms_args_t": VetoNmsArgs, "veto_box_post_args_t": VetoBoxPostArgs, "veto_rpn_args_t": VetoRpnArgs,
    "veto_anchor_args_t": VetoAnchorArgs,
    "veto_detect_relsample_args_t": VetoDetectRelsampleArgs, "veto_gtbox_relsample_args_t": VetoGtboxRelsampleArgs,
    "veto_box_match_args_t": VetoBoxMatchArgs, "veto_box_subsample_args_t": VetoBoxSubsampleArgs,
    "veto_rpn_loss_args_t": VetoRpnLossArgs, "veto_box_loss_args_t": VetoBoxLossArgs,
    "veto_optim_tensor_t": VetoOptimTensor, "veto_optim_args_t": VetoOptimArgs,
    "veto_roi_pool_args_t": VetoRoiPoolArgs, "veto_sgg_eval_args_t": VetoSggEvalArgs, "veto_train_opts_t": VetoTrainOpts,
    "veto_train_plan_t": VetoTrainPlan,
    "veto_det_eval_match_args_t": VetoDetEvalMatchArgs, "veto_det_eval_accumulate_args_t": VetoDetEvalAccumulateArgs,
    "veto_sgg_eval_fold_args_t": VetoSggEvalFoldArgs, "veto_meet_sample_args_t": VetoMeetSampleArgs,
}

_P, _I, _Z = c_void_p, c_int32, c_size_t


def _sig(*argtypes, ret=c_int):
    return ret, list(argtypes)


SIGNATURES = {   # entry point -> (restype, argtypes): load_library() applies all of it, so no export goes without a signature
    "veto_last_error": _sig(ret=c_char_p),
    "veto_version": _sig(ret=c_char_p),
    "veto_create": _sig(POINTER(VetoConfig), POINTER(_P)),
    "veto_destroy": _sig(_P),
    "veto_num_weights": _sig(_P),
    "veto_weight_info": _sig(_P, _I, POINTER(c_char_p), POINTER(_Z)),
    "veto_load_weights": _sig(_P, c_char_p, _P, _Z, _P),
    "veto_debug_last_finalize": _sig(_P, POINTER(_I), _I),
    "veto_workspace_bytes": _sig(_P, _I, _I, ret=_Z),
    "veto_forward": _sig(_P, _P, POINTER(VetoInputs), _P, _Z, _P, POINTER(VetoDebugOutputs)),
    "veto_forward_saturation": _sig(_P, _P, POINTER(VetoInputs), _P, _Z, _P, POINTER(VetoSaturation), _I),
    "veto_enumerate_pairs": _sig(_P, _I, _P),
    "veto_profile_enable": _sig(_P, _I),
    "veto_profile_collect": _sig(_P),
    "veto_profile_entry": _sig(_P, _I, POINTER(c_char_p), POINTER(c_double), POINTER(c_int64), POINTER(c_double), POINTER(c_double)),
    "veto_profile_reset": _sig(_P),
    "veto_debug_gemm": _sig(_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z),
    "veto_debug_gemm_workspace_bytes": _sig(_I, _I, _I, ret=_Z),
    "veto_debug_gemm_forms": _sig(_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _Z),
    "veto_debug_ffn": _sig(_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, POINTER(c_float), _P, _Z, _P, _P, _P),
    "veto_debug_ffn_workspace_bytes": _sig(_I, ret=_Z),
    "veto_debug_outproj": _sig(_P, _P, _P, _P, _P, _I, _I, _I, _I, POINTER(c_float), _P, _Z, _P, _P, _P),
    "veto_debug_outproj_workspace_bytes": _sig(_I, ret=_Z),
    "veto_debug_layer_tail": _sig(_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, POINTER(c_float), _P, _Z, _P, _P, _P),
    "veto_debug_layer_tail_workspace_bytes": _sig(_I, ret=_Z),
    "veto_debug_qkv_attn": _sig(_P, _P, _P, _I, _I, _I, _I, POINTER(c_float), _P, _Z, _P),
    "veto_debug_qkv_attn_workspace_bytes": _sig(_I, ret=_Z),
    "veto_postprocess": _sig(_P, POINTER(VetoPostArgs), _P, _Z),
    "veto_postprocess_workspace_bytes": _sig(_I, _I, ret=_Z),
    "veto_postprocess_meet": _sig(_P, POINTER(VetoPostMeetArgs), _P, _Z),
    "veto_postprocess_vote": _sig(_P, POINTER(VetoPostVoteArgs), _P, _Z),
    "veto_postprocess_groups_batch": _sig(_P, POINTER(VetoPostGroupsBatchArgs), _P, _Z),
    "veto_obj_decode": _sig(_P, POINTER(VetoObjDecodeArgs), _P, _Z),
    "veto_obj_decode_workspace_bytes": _sig(_I, _I, ret=_Z),
    "veto_prepare_test_pairs": _sig(_P, POINTER(VetoPairArgs)),
    "veto_detect_relsample": _sig(_P, POINTER(VetoDetectRelsampleArgs), _P, _Z),
    "veto_detect_relsample_workspace_bytes": _sig(_I, _I, ret=_Z),
    "veto_gtbox_relsample": _sig(_P, POINTER(VetoGtboxRelsampleArgs)),
    "veto_box_match": _sig(_P, POINTER(VetoBoxMatchArgs)),
    "veto_box_subsample": _sig(_P, POINTER(VetoBoxSubsampleArgs)),
    "veto_nms": _sig(_P, POINTER(VetoNmsArgs)),
    "veto_nms_max_segment": _sig(),
    "veto_box_postprocess": _sig(_P, POINTER(VetoBoxPostArgs), _P, _Z),
    "veto_box_postprocess_workspace_bytes": _sig(_I, _I, _I, ret=_Z),
    "veto_rpn_proposals": _sig(_P, POINTER(VetoRpnArgs), _P, _Z),
    "veto_rpn_proposals_workspace_bytes": _sig(POINTER(VetoRpnArgs), ret=_Z),
    "veto_anchor_grid": _sig(_P, POINTER(VetoAnchorArgs)),
    "veto_rpn_loss": _sig(_P, POINTER(VetoRpnLossArgs), _P, _Z),
    "veto_rpn_loss_workspace_bytes": _sig(POINTER(VetoRpnLossArgs), ret=_Z),
    "veto_box_loss": _sig(_P, POINTER(VetoBoxLossArgs), _P, _Z),
    "veto_box_loss_workspace_bytes": _sig(POINTER(VetoBoxLossArgs), ret=_Z),
    "veto_optim_step": _sig(_P, POINTER(VetoOptimArgs), _P, _Z),
    "veto_optim_step_workspace_bytes": _sig(POINTER(VetoOptimArgs), ret=_Z),
    "veto_train_workspace_bytes": _sig(_P, _I, _I, ret=_Z),
    "veto_train_workspace_bytes_opts": _sig(_P, _I, _I, POINTER(VetoTrainOpts), ret=_Z),
    "veto_grad_floats": _sig(_P, ret=_Z),
    "veto_weight_offset": _sig(_P, _I, POINTER(_Z)),
    "veto_forward_train": _sig(_P, _P, POINTER(VetoInputs), POINTER(VetoTrainOpts), _P, _Z, _P),
    "veto_backward": _sig(_P, _P, POINTER(VetoInputs), POINTER(VetoTrainOpts), _P, _Z, _P, _P),
    "veto_train_workspace_bytes_plan": _sig(_P, _I, _I, POINTER(VetoTrainOpts), POINTER(VetoTrainPlan), ret=_Z),
    "veto_forward_train_plan": _sig(_P, _P, POINTER(VetoInputs), POINTER(VetoTrainOpts), POINTER(VetoTrainPlan), _P, _Z, _P),
    "veto_backward_plan": _sig(_P, _P, POINTER(VetoInputs), POINTER(VetoTrainOpts), POINTER(VetoTrainPlan), _P, _Z, _P, _P),
    "veto_debug_attention_backward": _sig(_P, _P, _P, _P, _I, _I),
    "veto_debug_layernorm_backward": _sig(_P, _P, _P, _P, _P, _P, _P, _I, _P, _Z),
    "veto_debug_layernorm_backward_workspace_bytes": _sig(_I, ret=_Z),
    "veto_debug_gelu_backward": _sig(_P, _P, _P, _P, _Z),
    "veto_debug_column_sums": _sig(_P, _P, c_int64, _I, _I, _P, _P, _Z),
    "veto_debug_attention_backward_forms": _sig(_P, _P, _P, _P, _P, _I, _I, c_uint32),
    "veto_debug_layernorm_backward_split": _sig(_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, c_uint64, c_uint32, c_float, _P, _Z),
    "veto_debug_layernorm_backward_col_partial_rows": _sig(_I, ret=_I),
    "veto_debug_wgrad": _sig(_P, _P, _P, _P, _I, _I, _I, _I, _P, _Z),
    "veto_debug_wgrad_workspace_bytes": _sig(_I, _I, _I, _I, ret=_Z),
    "veto_debug_wgrad_ordered": _sig(_P, _P, _P, _P, _I, _I, _I, _I, _P, _Z),
    "veto_debug_wgrad_ordered_workspace_bytes": _sig(_I, _I, _I, _I, ret=_Z),
    "veto_debug_assemble_backward_ordered": _sig(_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P),
    "veto_debug_scatter_rows_ordered": _sig(_P, _P, _P, _I, _I, _I, _P),
    "veto_debug_layernorm_backward_ordered": _sig(_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, c_uint64, c_uint32, c_float, _P, _Z),
    "veto_debug_attention": _sig(_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P),
    "veto_debug_cls_fold_attention": _sig(_P, _P, _P, _P, _P, _P, _I, _I, _I),
    "veto_debug_qkv0_combine": _sig(_P, _P, _P, _P, _P, _P, _P, _P, _I),
    "veto_ce_loss": _sig(_P, _P, c_int64, _P, _P, _P, _I, _I, _P, _P, _P, _Z),
    "veto_ce_loss_workspace_bytes": _sig(_I, ret=_Z),
    "veto_meet_sample": _sig(_P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P),
    "veto_meet_sample_parallel": _sig(_P, POINTER(VetoMeetSampleArgs), _P, _Z),
    "veto_meet_sample_parallel_workspace_bytes": _sig(_I, _I, ret=_Z),
    "veto_meet_sample_parallel_limits": _sig(POINTER(_I), POINTER(_I), POINTER(_I)),
    "veto_roi_pool": _sig(_P, POINTER(VetoRoiPoolArgs)),
    "veto_roi_pool_backward": _sig(_P, POINTER(VetoRoiPoolArgs), _P, _P, POINTER(_P), _P),
    "veto_roi_pool_backward_ordered": _sig(_P, POINTER(VetoRoiPoolArgs), _P, _P, POINTER(_P), _P),
    "veto_roi_pool_adaptive": _sig(_P, POINTER(VetoRoiPoolArgs)),
    "veto_roi_pool_adaptive_backward": _sig(_P, POINTER(VetoRoiPoolArgs), _P, _P, POINTER(_P), _P),
    "veto_sgg_eval": _sig(_P, POINTER(VetoSggEvalArgs), _I, _I, _P, _Z),
    "veto_sgg_eval_workspace_bytes": _sig(_I, _I, _I, _I, ret=_Z),
    "veto_sgg_eval_fold": _sig(_P, POINTER(VetoSggEvalFoldArgs), _P, _Z),
    "veto_sgg_eval_fold_workspace_bytes": _sig(_I, _I, ret=_Z),
    "veto_sgg_eval_fold_limits": _sig(POINTER(_I), POINTER(_I)),
    "veto_det_eval_match": _sig(_P, POINTER(VetoDetEvalMatchArgs), _P, _Z),
    "veto_det_eval_match_workspace_bytes": _sig(_I, _I, _I, ret=_Z),
    "veto_det_eval_accumulate": _sig(_P, POINTER(VetoDetEvalAccumulateArgs), _P, _Z),
    "veto_det_eval_accumulate_workspace_bytes": _sig(c_int64, _I, ret=_Z),
    "veto_det_eval_limits": _sig(POINTER(_I), POINTER(_I), POINTER(_I), POINTER(_I)),
}
EXPORTS = list(SIGNATURES)   # what include/veto_amd.h declares


class VetoError(RuntimeError):
    pass


_ENV_DETERMINISTIC = None


def ordered_mode(knob=False):
    """Does the training path run in the ordered mode (include/veto_amd.h, veto_train_opts_t.deterministic)?  `knob` is the caller's
    cfg.VETO_AMD.DETERMINISTIC; torch.use_deterministic_algorithms(True) and VETO_DETERMINISTIC=1 (read once per process, like the
    library's VETO_TRAIN_* knobs) switch it on as well."""
    global _ENV_DETERMINISTIC
    if _ENV_DETERMINISTIC is None:
        _ENV_DETERMINISTIC = os.environ.get("VETO_DETERMINISTIC") == "1"
    return bool(knob) or _ENV_DETERMINISTIC or torch.are_deterministic_algorithms_enabled()


def library_path():
    # VETO_AMD_LIB: A/B a differently built copy of the same library (tools/ only; never a fallback)
    return os.environ.get("VETO_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                          "libveto_amd.so")


def load_library():
    """Loads libveto_amd.so (building it with hipcc first if it is absent). Raises if impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        from .build import build_native
        build_native()
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = lib
    return lib


def check(rc):
    if rc < 0:
        raise VetoError("veto_amd native call failed (%d): %s" % (rc, load_library().veto_last_error().decode()))
    return rc


_OFFSETS = {}      # (device, size lists) -> the rows of an int32 [len(size_lists), n + 1] device tensor
_PLAIN = (int, float, type(None))
_WORKSPACES = {}   # (device index, stream) -> uint8 scratch tensor, grow-only: calls on different streams never share one


def device_offsets(*size_lists, device):
    """Exclusive prefix sums of equally long per-image size lists: the rows of ONE int32 [len(size_lists), n + 1] device tensor,
    as a tuple (row r belongs to size_lists[r]; the row views are made once, a slice per call costs microseconds).
    torch.tensor(list, device=...) is a synchronous pageable H2D copy that stalls the host behind all queued GPU work, so
    batch shapes seen before (the common case in an eval or training loop) re-use their tensor.  The one offset cache of the
    package; it is emptied when it reaches 256 shapes."""
    key = (str(device),) + tuple(tuple(sizes) for sizes in size_lists)
    hit = _OFFSETS.get(key)
    if hit is None:
        if len(_OFFSETS) >= 256:
            _OFFSETS.clear()
        rows = [[0] + list(itertools.accumulate(sizes)) for sizes in key[1:]]
        hit = _OFFSETS[key] = torch.tensor(rows, dtype=torch.int32, device=device).unbind(0)
    return hit


class Launch:
    """One stream-ordered C-ABI call from a wrapper: the device check, the library, the current stream, the struct's pointer
    fields, the scratch workspace and, after the call, record_stream on every tensor the call was handed."""

    def __init__(self, device, what):
        """what: the refusal for a non-HIP device, e.g. 'veto_amd.PostProcessor runs only on a HIP device'."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s (got %s)" % (what, device))
        self.lib = load_library()
        self.stream = torch.cuda.current_stream(self.device)
        self._tensors = []

    def ptr(self, t):
        """NULL for None or an empty tensor, else the tensor's address; the tensor is kept for record_stream."""
        if t is None or t.numel() == 0:
            return None
        self._tensors.append(t)
        return t.data_ptr()

    def args(self, struct_cls, **fields):
        """A struct_cls with struct_size set; tensor (or None) fields go through ptr(), everything else as it is."""
        a = struct_cls(struct_size=ctypes.sizeof(struct_cls))
        keep = self._tensors.append
        for name, v in fields.items():   # (ptr() inlined: this loop is the host cost of a call)
            if type(v) not in _PLAIN and isinstance(v, torch.Tensor):   # (isinstance on Tensor's metaclass is slow for an int)
                if v.numel():
                    keep(v)
                    v = v.data_ptr()
                else:
                    v = None
            setattr(a, name, v)
        return a

    def workspace(self, need):
        """The scratch tensor of this (device, stream), at least `need` bytes."""
        key = (self.stream.device_index, self.stream.cuda_stream)
        ws = _WORKSPACES.get(key)
        if ws is None or ws.numel() < need:
            ws = _WORKSPACES[key] = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return ws

    def run(self, name, *tail, handle=None):
        """check(lib.<name>([handle,] stream, *tail)), then record()."""
        head = (c_void_p(self.stream.cuda_stream),) if handle is None else (handle, c_void_p(self.stream.cuda_stream))
        rc = check(getattr(self.lib, name)(*head, *tail))
        self.record()
        return rc

    def record(self):
        """The tensors handed to ptr() are referenced by enqueued kernels: keep them alive on this stream."""
        for t in self._tensors:
            t.record_stream(self.stream)


class Engine:
    """Owns one veto_handle_t. Thin: every method maps 1:1 onto a C-ABI call."""

    def __init__(self, layers, heads, num_obj_cls, num_out, precision=VETO_PRECISE, device=0, dim=576,
                 embed_dim=200, max_chunk_pairs=0, patch=2, resolution=8):
        self.lib = load_library()
        cfg = VetoConfig(ctypes.sizeof(VetoConfig), dim, layers, heads, patch, 256, resolution, num_obj_cls, embed_dim,
                         num_out, precision, device, max_chunk_pairs)
        self.cfg = cfg
        h = c_void_p()
        check(self.lib.veto_create(byref(cfg), byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.veto_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def weight_specs(self):
        out = []
        for i in range(check(self.lib.veto_num_weights(self.handle))):
            name, numel = c_char_p(), c_size_t()
            check(self.lib.veto_weight_info(self.handle, i, byref(name), byref(numel)))
            out.append((name.value.decode(), numel.value))
        return out

    def load_weight(self, name, ptr, numel, stream=0):
        check(self.lib.veto_load_weights(self.handle, name.encode(), c_void_p(ptr), numel, c_void_p(stream)))

    def last_finalize(self):
        """veto_debug_last_finalize: {build kind: operands rebuilt} of the last rebuild of derived operands (BUILD_KINDS)."""
        counts = (c_int32 * len(BUILD_KINDS))()
        check(self.lib.veto_debug_last_finalize(self.handle, counts, len(BUILD_KINDS)))
        return dict(zip(BUILD_KINDS, (int(c) for c in counts)))

    def workspace_bytes(self, n_obj, n_pair):
        return self.lib.veto_workspace_bytes(self.handle, n_obj, n_pair)

    def forward(self, stream, inputs, workspace_ptr, workspace_bytes, out_ptr, dbg=None):
        check(self.lib.veto_forward(self.handle, c_void_p(stream), byref(inputs), c_void_p(workspace_ptr),
                                    workspace_bytes, c_void_p(out_ptr), byref(dbg) if dbg is not None else None))

    def forward_saturation(self, stream, inputs, workspace_ptr, workspace_bytes, out_ptr):
        """veto_forward_saturation: the forward in its launch-per-stage form plus, per layer and operand site, the count of mixed-row
        elements that sit at the clamp values.  Returns [{site: dict(elements, f16_saturated, value_saturated, resid_saturated)}]
        with one entry per layer (synchronises the stream)."""
        n = self.cfg.layers * len(SATURATION_SITES)
        counts = (VetoSaturation * n)()
        check(self.lib.veto_forward_saturation(self.handle, c_void_p(stream), byref(inputs), c_void_p(workspace_ptr), workspace_bytes,
                                               c_void_p(out_ptr), counts, n))
        out = []
        for layer in range(self.cfg.layers):
            out.append({site: {f: int(getattr(counts[layer * len(SATURATION_SITES) + i], f)) for f, _ in VetoSaturation._fields_}
                        for i, site in enumerate(SATURATION_SITES)})
        return out

    def weight_offsets(self):
        """{weight name: (offset, numel)} in floats into the flat gradient buffer of veto_backward."""
        if getattr(self, "_offsets", None) is None:
            out = {}
            for i in range(check(self.lib.veto_num_weights(self.handle))):
                name, numel, off = c_char_p(), c_size_t(), c_size_t()
                check(self.lib.veto_weight_info(self.handle, i, byref(name), byref(numel)))
                check(self.lib.veto_weight_offset(self.handle, i, byref(off)))
                out[name.value.decode()] = (off.value, numel.value)
            self._offsets = out
        return self._offsets

    def profile_enable(self, on):
        check(self.lib.veto_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.veto_profile_reset(self.handle))

    def profile(self):
        """Returns {kernel: dict(total_ms, launches, flops_per_launch, bytes_per_launch)}."""
        n = check(self.lib.veto_profile_collect(self.handle))
        out = {}
        for i in range(n):
            name, ms, cnt, fl, by = c_char_p(), c_double(), c_int64(), c_double(), c_double()
            check(self.lib.veto_profile_entry(self.handle, i, byref(name), byref(ms), byref(cnt), byref(fl), byref(by)))
            if cnt.value:
                out[name.value.decode()] = dict(total_ms=ms.value, launches=cnt.value,
                                                flops_per_launch=fl.value, bytes_per_launch=by.value)
        return out
