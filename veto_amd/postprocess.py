"""MI355X-native relation PostProcessor.

Mirrors the vanilla, GT-box branch of the reference's PostProcessor
(pysgg/modeling/roi_heads/relation_head/inference.py:9-92,398-453): same constructor arguments, same
`forward(x, rel_pair_idxs, boxes)` call, and the same BoxList fields on the results
(`pred_labels`, `pred_scores`, `rel_pair_idxs`, `pred_rel_scores`, `pred_rel_labels`).  The
arithmetic (softmax, foreground max, triple score, per-image descending sort, gather) runs in
libveto_amd.so (veto_postprocess).  When the relation logits are the MEET dict of group heads
(ENSEMBLE_LEARNING.ENABLED with EXPERT_GROUP False), the MEET merge branch (inference.py:284-397) runs
with the reference's quirks kept: group-local labels, float pair indices.  With
EXPERT_GROUP True (three expert heads per group, keys 'group_<k><e>') the voting branch (inference.py:93-283,
ENSEMBLE_LEARNING.VOTING 'C' or 'U') runs; its row counts are data dependent, so that
branch reads one int32 per image back from the device.  The reference zips the batch-wide group logits with the first image only
(inference.py:114-116, :302-306); here both MEET branches take any number of images, one included, through
veto_postprocess_groups_batch in at most four launches (plus the object
decoding in sgdet), every image getting exactly the result of a call on it alone, the vote reading kept_count[n_img] back
once per call.  With detected boxes
(sgdet, use_gt_box False) every branch first decodes the objects with the class-aware NMS of inference.py:413-429
(veto_obj_decode, LATER_NMS_PREDICTION_THRES) and returns NEW BoxLists holding the regressed boxes
boxes_per_cls[i, label_i]; the relation kernels then read those labels / scores (obj_logits = NULL).  Attributes
are not built; they raise."""
import ctypes

import torch
from torch import nn

from . import native


class PostProcessor(nn.Module):
    def __init__(self, attribute_on, use_gt_box=False, later_nms_pred_thres=0.3, cfg=None):
        super().__init__()
        self.cfg = cfg
        self.attribute_on = attribute_on
        self.use_gt_box = use_gt_box
        self.later_nms_pred_thres = later_nms_pred_thres

    def forward(self, x, rel_pair_idxs, boxes, custom_rel_labels=None, cur_chosen_matrix=None, incre_idx_list=None,
                ensemble=False):
        relation_logits, refine_logits = x
        if self.attribute_on:
            raise NotImplementedError("veto_amd.PostProcessor: attribute head is outside the VETO path")
        if isinstance(relation_logits, dict):
            if "group_01" in relation_logits:   # inference.py:93: three experts per group
                return self._forward_vote(relation_logits, refine_logits, rel_pair_idxs, boxes, incre_idx_list)
            return self._forward_meet(relation_logits, refine_logits, rel_pair_idxs, boxes, incre_idx_list)
        rel = torch.cat(list(relation_logits), 0) if isinstance(relation_logits, (list, tuple)) else relation_logits
        obj = torch.cat(list(refine_logits), 0) if isinstance(refine_logits, (list, tuple)) else refine_logits
        device = rel.device
        call = native.Launch(device, "veto_amd.PostProcessor runs only on a HIP device")
        n_objs = [len(b) for b in boxes]
        n_pairs = [int(p.shape[0]) for p in rel_pair_idxs]
        n_obj, n_pair = sum(n_objs), sum(n_pairs)
        rel = rel.detach().to(device=device, dtype=torch.float32).contiguous()
        obj = obj.detach().to(device=device, dtype=torch.float32).contiguous()
        if rel.shape[0] != n_pair or obj.shape[0] != n_obj:
            raise ValueError("logit rows (%d, %d) do not match pairs/objects (%d, %d)" % (rel.shape[0], obj.shape[0], n_pair, n_obj))
        pairs = torch.cat([p.reshape(-1, 2) for p in rel_pair_idxs], 0).to(device=device, dtype=torch.int64).contiguous()
        off = native.device_offsets(n_objs, n_pairs, device=device)   # no host-blocking H2D copy in the steady state
        out, reg_boxes = self._outputs(obj, boxes, n_pair, rel.shape[1])
        a = call.args(native.VetoPostArgs, n_img=len(boxes), n_obj=n_obj, n_pair=n_pair, n_rel_cls=rel.shape[1],
                      n_obj_cls=obj.shape[1], max_pairs_per_image=max(n_pairs), rel_logits=rel, rel_pairs=pairs,
                      img_obj_offset=off[0], img_pair_offset=off[1], **self._shared_fields(obj, out, reg_boxes))
        ws = call.workspace(call.lib.veto_postprocess_workspace_bytes(n_pair, rel.shape[1]))
        call.run("veto_postprocess", ctypes.byref(a), ws.data_ptr(), ws.numel())
        self.last_triple_scores = out["triple"].split(n_pairs)
        regs = reg_boxes.split(n_objs) if reg_boxes is not None else [None] * len(boxes)
        return [self._fill(box, reg, sc, pr, pidx, prob, lab)    # inference.py:431-432 (the GT-box branch re-uses `box`), :450-452
                for box, reg, sc, pr, pidx, prob, lab in zip(boxes, regs, out["obj_scores"].split(n_objs), out["obj_pred"].split(n_objs),
                                                             out["pairs"].split(n_pairs), out["prob"].split(n_pairs),
                                                             out["labels"].split(n_pairs))]

    def _forward_meet(self, relation_logits, refine_logits, rel_pair_idxs, boxes, incre_idx_list):
        if incre_idx_list is None:
            raise ValueError("the MEET merge needs incre_idx_list (4th element of the predictor's return tuple)")
        keys = ["group_%d" % k for k in range(len(relation_logits))]
        return self._forward_groups(relation_logits, keys, 1, refine_logits, rel_pair_idxs, boxes, incre_idx_list)

    def _forward_vote(self, relation_logits, refine_logits, rel_pair_idxs, boxes, incre_idx_list):
        if incre_idx_list is None:
            raise ValueError("expert voting needs incre_idx_list (4th element of the predictor's return tuple)")
        voting = str(self.cfg.ENSEMBLE_LEARNING.VOTING) if self.cfg is not None else "C"
        if voting not in ("C", "U"):
            raise ValueError("ENSEMBLE_LEARNING.VOTING must be 'C' or 'U', got %r" % voting)
        if len(relation_logits) % 3:
            raise ValueError("expected three expert heads per group, got %d heads" % len(relation_logits))
        keys = ["group_%d%d" % (k, e + 1) for k in range(len(relation_logits) // 3) for e in range(3)]
        return self._forward_groups(relation_logits, keys, 3, refine_logits, rel_pair_idxs, boxes, incre_idx_list,
                                    voting=0 if voting == "C" else 1)

    def _forward_groups(self, relation_logits, keys, per_group, refine_logits, rel_pair_idxs, boxes, incre_idx_list, voting=None):
        """The MEET merge (per_group 1) and the expert vote (per_group 3, `voting` set): K groups of per_group heads each, one
        image or a batch in ONE call: the batch-wide head logits as they are, the concatenated image-local pair lists and
        refine logits (one image: its own tensors, no copy).  Image i owns the K * P_i rows from K * (pairs before it) on
        (include/veto_amd.h).  The merge reads nothing back; the vote's row counts are data dependent: kept_count[n_img] is
        read back once, to cut the blocks."""
        if len(boxes) == 0:
            raise ValueError("the MEET post-processor needs at least one image")
        device = relation_logits[keys[0]].device
        call = native.Launch(device, "veto_amd.PostProcessor runs only on a HIP device")
        heads = [relation_logits[k].detach().to(device=device, dtype=torch.float32).contiguous() for k in keys]
        obj = _cat(list(refine_logits)) if isinstance(refine_logits, (list, tuple)) else refine_logits
        obj = obj.detach().to(device=device, dtype=torch.float32).contiguous()
        n_objs = [len(b) for b in boxes]
        pair_lists = [p.reshape(-1, 2) for p in rel_pair_idxs]
        n_pairs = [int(p.shape[0]) for p in pair_lists]
        n_obj, n_pair = sum(n_objs), sum(n_pairs)
        if len(n_pairs) != len(boxes) or obj.shape[0] != n_obj or any(h.shape[0] != n_pair for h in heads):
            raise ValueError("head rows %s / object rows %d do not match the batch's pairs %s / objects %s"
                             % (sorted({int(h.shape[0]) for h in heads}), obj.shape[0], n_pairs, n_objs))
        pairs = _cat(pair_lists).to(device=device, dtype=torch.int64).contiguous()
        off = native.device_offsets(n_objs, n_pairs, device=device)   # no host-blocking H2D copy in the steady state
        K, n_rel = len(heads) // per_group, len(incre_idx_list)
        total = K * n_pair
        out, reg_boxes = self._outputs(obj, boxes, total, n_rel)
        fields = self._shared_fields(obj, out, reg_boxes)
        kept = None
        if voting is not None:
            kept = torch.zeros(len(boxes), dtype=torch.int32, device=device)
            fields.update(voting=voting, kept_count=kept)
        # host arrays: the ABI reads them before it returns
        ptrs = (ctypes.c_void_p * len(heads))(*[call.ptr(h) for h in heads])
        widths = (ctypes.c_int32 * K)(*[heads[per_group * k].shape[1] for k in range(K)])
        incre = (ctypes.c_int32 * n_rel)(*[int(x) for x in incre_idx_list])
        counts = (ctypes.c_int32 * len(n_pairs))(*n_pairs)
        a = call.args(native.VetoPostGroupsBatchArgs, n_img=len(boxes), n_obj=n_obj, n_pair=n_pair, n_groups=K,
                      experts_per_group=per_group, n_rel_cls=n_rel, n_obj_cls=obj.shape[1], max_pairs_per_image=max(n_pairs),
                      head_logits=ctypes.cast(ptrs, ctypes.c_void_p), group_widths=ctypes.cast(widths, ctypes.c_void_p),
                      incre_idx_list=ctypes.cast(incre, ctypes.c_void_p), pairs_per_image=ctypes.cast(counts, ctypes.c_void_p),
                      rel_pairs=pairs, img_obj_offset=off[0], img_pair_offset=off[1], **fields)
        ws = call.workspace(call.lib.veto_postprocess_workspace_bytes(total, n_rel))
        call.run("veto_postprocess_groups_batch", ctypes.byref(a), ws.data_ptr(), ws.numel())
        blocks = [K * p for p in n_pairs]
        if kept is None:
            cut = lambda t: _split(t, blocks)
        else:
            keep = kept.tolist()   # the vote's one device read-back: the row counts are data dependent
            cut = lambda t: [b[:n] for b, n in zip(_split(t, blocks), keep)]
        self.last_triple_scores = cut(out["triple"])
        regs = _split(reg_boxes, n_objs) if reg_boxes is not None else [None] * len(boxes)
        # float pair indices (torch.zeros(total, 2) in the reference, inference.py:381 / :267) and group-local labels (:388)
        # (one conversion for the batch, not one per image)
        return [self._fill(box, reg, sc, pr, pidx, prob, lab)
                for box, reg, sc, pr, pidx, prob, lab in zip(boxes, regs, _split(out["obj_scores"], n_objs), _split(out["obj_pred"], n_objs),
                                                             cut(out["pairs"].to(torch.float32)), cut(out["prob"]), cut(out["labels"]))]

    def _outputs(self, obj, boxes, rows, n_rel):
        """(the output tensors of `rows` relation rows, the regressed boxes or None)."""
        device = obj.device
        obj_pred, obj_scores, reg_boxes = self._decode_objects(obj, boxes)
        return {"obj_scores": obj_scores, "obj_pred": obj_pred,
                "prob": torch.empty((rows, n_rel), dtype=torch.float32, device=device),
                "pairs": torch.empty((rows, 2), dtype=torch.int64, device=device),
                "labels": torch.empty(rows, dtype=torch.int64, device=device),
                "triple": torch.empty(rows, dtype=torch.float32, device=device)}, reg_boxes

    @staticmethod
    def _shared_fields(obj, out, reg_boxes):
        """The struct fields the three entry points have in common.  sgdet: labels / scores are the decoder's (obj_logits NULL)."""
        return dict(obj_logits=obj if reg_boxes is None else None, obj_scores=out["obj_scores"], obj_pred=out["obj_pred"],
                    rel_prob_sorted=out["prob"], rel_pairs_sorted=out["pairs"], rel_labels_sorted=out["labels"],
                    triple_sorted=out["triple"])

    def _fill(self, box, reg, obj_scores, obj_pred, pair_idxs, prob, labels):
        box = self._result_box(box, reg)
        box.add_field("pred_labels", obj_pred)
        box.add_field("pred_scores", obj_scores)
        box.add_field("rel_pair_idxs", pair_idxs)
        box.add_field("pred_rel_scores", prob)
        box.add_field("pred_rel_labels", labels)
        return box

    def _decode_objects(self, obj_logits, boxes):
        """(obj_pred, obj_scores, regressed boxes) of the concatenated images.  GT boxes: two empty outputs that the
        relation kernel fills from obj_logits, no boxes.  Detected boxes: the class-aware NMS decoding of
        inference.py:413-429 on the device (veto_obj_decode), whose labels / scores the relation kernel then reads."""
        device, n_obj = obj_logits.device, obj_logits.shape[0]
        if self.use_gt_box:
            return (torch.empty(n_obj, dtype=torch.int64, device=device), torch.empty(n_obj, dtype=torch.float32, device=device),
                    None)
        from .sgdet import decode_objects
        for b in boxes:
            if not b.has_field("boxes_per_cls"):
                raise ValueError("sgdet post-processing needs the detector's 'boxes_per_cls' field on every proposal")
        boxes_per_cls = torch.cat([b.get_field("boxes_per_cls").reshape(len(b), -1, 4) for b in boxes], 0).to(device)
        return decode_objects(obj_logits, boxes_per_cls, [len(b) for b in boxes], self.later_nms_pred_thres, mode="post")

    @staticmethod
    def _result_box(box, reg):
        """GT boxes: the proposal itself (inference.py:421-422).  sgdet: a new BoxList of the regressed boxes, xyxy, with
        the proposal's size (:424-428)."""
        if reg is None:
            return box
        return type(box)(reg, box.size, "xyxy")


def _cat(tensors):
    """torch.cat along rows; a single tensor as it is, without the copy."""
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, 0)


def _split(t, sizes):
    """t.split(sizes); one size: the tensor as it is (a call on one image pays for no views)."""
    return [t] if len(sizes) == 1 else t.split(sizes)


def make_roi_relation_post_processor(cfg):
    """inference.py:456-468."""
    return PostProcessor(getattr(cfg.MODEL, "ATTRIBUTE_ON", False), cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX,
                         cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES, cfg)
