"""The box head's PostProcessor (pysgg/modeling/roi_heads/box_head/inference.py:12-267) on the HIP device.

It is the one producer of the fields the sgdet relation head starts from -- `predict_logits`, `pred_labels`, `pred_scores`
and `boxes_per_cls`.  `PostProcessor.forward` runs veto_box_postprocess once per batch: softmax, BoxCoder.decode of every
class, clipping, the per-class NMS, duplicate filtering and the DETECTIONS_PER_IMG cut, four launches whatever the number
of classes or images.  The per-image counts are read back once (the only device->host copy) to split the outputs; the
decoded [N, C, 4] boxes stay in the workspace.  The decoder has no backward (the reference runs it under no_grad)."""
import ctypes
import math

import numpy as np
import torch
from torch import nn

from . import native

_SIZES = {}       # (device, image sizes) -> device tensor [n_img, 2]


class BoxCoder:
    """The two attributes of pysgg.modeling.box_coder.BoxCoder that decoding reads."""

    def __init__(self, weights, bbox_xform_clip=math.log(1000. / 16)):
        self.weights = tuple(float(w) for w in weights)
        self.bbox_xform_clip = bbox_xform_clip


def _image_sizes(sizes, device):
    key = (str(device), tuple(sizes))
    hit = _SIZES.get(key)
    if hit is None:
        if len(_SIZES) >= 256:
            _SIZES.clear()
        hit = _SIZES[key] = torch.tensor(sizes, dtype=torch.float32).reshape(-1, 2).to(device)
    return hit


def box_postprocess(class_logits, box_regression, proposals, n_per_img, image_sizes, score_thresh=0.05, nms=0.5,
                    post_nms_per_cls_topn=300, nms_filter_duplicates=True, detections_per_img=100,
                    reg_weights=(10., 10., 5., 5.), bbox_xform_clip=math.log(1000. / 16), cls_agnostic_bbox_reg=False,
                    want_boxes_per_cls=True):
    """veto_box_postprocess for a batch.  class_logits [N, C], box_regression [N, 4C] (or [N, 4k] with
    cls_agnostic_bbox_reg), proposals [N, 4] xyxy on the HIP device; n_per_img and image_sizes ((width, height)) per image.
    Returns per image a dict of device tensors: orig_inds int64 [K], pred_labels int64 [K], pred_scores [K], boxes [K, 4],
    boxes_per_cls [K, C, 4]."""
    device = class_logits.device
    call = native.Launch(device, "veto_amd box-head post-processing runs on a HIP device only")
    f32 = dict(device=device, dtype=torch.float32)
    n_box, n_cls = int(class_logits.shape[0]), int(class_logits.shape[1])
    n_per_img = [int(n) for n in n_per_img]
    if sum(n_per_img) != n_box:
        raise ValueError("per-image counts %s do not add up to %d rows" % (n_per_img, n_box))
    if n_box == 0:
        e = torch.empty(0, **f32)
        return [dict(orig_inds=torch.empty(0, dtype=torch.int64, device=device), pred_labels=torch.empty(0, dtype=torch.int64, device=device),
                     pred_scores=e, boxes=e.reshape(0, 4), boxes_per_cls=e.reshape(0, n_cls, 4)) for _ in n_per_img]
    class_logits = class_logits.detach().to(**f32).contiguous()
    box_regression = box_regression.detach().to(**f32).reshape(n_box, -1).contiguous()
    proposals = proposals.detach().to(**f32).reshape(n_box, 4).contiguous()
    sizes = _image_sizes([(float(w), float(h)) for w, h in image_sizes], device)
    host_off = np.concatenate([[0], np.cumsum(n_per_img)]).astype(np.int32)
    ws = call.workspace(call.lib.veto_box_postprocess_workspace_bytes(n_box, n_cls, int(bool(nms_filter_duplicates))))
    # rows reserved per image: every detection when there is no cut, else the cut plus as many ties again (a batch whose
    # ties exceed that reports the rows it needs and is run once more with exactly those)
    bound = [n if nms_filter_duplicates else
             (min(n, post_nms_per_cls_topn) if post_nms_per_cls_topn > 0 else n) * (n_cls - 1) for n in n_per_img]
    caps = [min(b, 2 * detections_per_img) if detections_per_img > 0 else b for b in bound]
    for attempt in range(2):
        off = native.device_offsets(n_per_img, caps, device=device)
        rows = sum(caps)
        orig = torch.empty(rows, dtype=torch.int64, device=device)
        labels = torch.empty(rows, dtype=torch.int64, device=device)
        scores = torch.empty(rows, **f32)
        boxes = torch.empty((rows, 4), **f32)
        bpc = torch.empty((rows, n_cls, 4), **f32) if want_boxes_per_cls else None
        counts = torch.empty(len(n_per_img), dtype=torch.int32, device=device)
        a = call.args(native.VetoBoxPostArgs, n_img=len(n_per_img), n_box=n_box, n_cls=n_cls, reg_cols=int(box_regression.shape[1]),
                      cls_agnostic=int(bool(cls_agnostic_bbox_reg)), post_nms_per_cls_topn=int(post_nms_per_cls_topn),
                      filter_duplicates=int(bool(nms_filter_duplicates)), detections_per_img=int(detections_per_img),
                      score_thresh=float(score_thresh), nms_thresh=float(nms), bbox_xform_clip=float(bbox_xform_clip),
                      reg_weights=(ctypes.c_float * 4)(*[float(w) for w in reg_weights]), class_logits=class_logits,
                      box_regression=box_regression, proposals=proposals, image_sizes=sizes, img_offset=off[0],
                      img_offset_host=host_off.ctypes.data, img_out_offset=off[1], orig_inds=orig, pred_labels=labels,
                      pred_scores=scores, boxes=boxes, boxes_per_cls=bpc, counts=counts)
        call.run("veto_box_postprocess", ctypes.byref(a), ws.data_ptr(), ws.numel())
        kept = counts.tolist()   # the one device->host copy of the batch: the counts decide the split
        if min(kept) >= 0:
            break
        if attempt:
            raise native.VetoError("veto_box_postprocess: detections %s do not fit the rows %s" % (kept, caps))
        caps = [max(c, -k) for c, k in zip(caps, kept)]
    out, row = [], 0
    for cap, k in zip(caps, kept):
        sl = slice(row, row + k)
        out.append(dict(orig_inds=orig[sl], pred_labels=labels[sl], pred_scores=scores[sl], boxes=boxes[sl],
                        boxes_per_cls=bpc[sl] if bpc is not None else None))
        row += cap
    return out


class PostProcessor(nn.Module):
    """inference.py:12-238 with the reference's constructor and forward contract."""

    def __init__(self, score_thresh=0.05, nms=0.5, post_nms_per_cls_topn=300, nms_filter_duplicates=True,
                 detections_per_img=100, box_coder=None, cls_agnostic_bbox_reg=False, bbox_aug_enabled=False,
                 save_proposals=False):
        super().__init__()
        if bbox_aug_enabled:
            raise NotImplementedError("TEST.BBOX_AUG.ENABLED is not supported (the reference asserts it off, inference.py:93)")
        self.score_thresh = score_thresh
        self.nms = nms
        self.post_nms_per_cls_topn = post_nms_per_cls_topn
        self.nms_filter_duplicates = nms_filter_duplicates
        self.detections_per_img = detections_per_img
        self.box_coder = box_coder if box_coder is not None else BoxCoder(weights=(10., 10., 5., 5.))
        self.cls_agnostic_bbox_reg = cls_agnostic_bbox_reg
        self.bbox_aug_enabled = bbox_aug_enabled
        self.save_proposals = save_proposals

    @torch.no_grad()
    def forward(self, x, boxes, relation_mode=False):
        """x = (features, class_logits, box_regression); boxes = the proposals, one BoxList per image with the field
        'predict_logits'.  Returns (nms_features, results) as inference.py:51-104."""
        features, class_logits, box_regression = x
        n_per_img = [len(b) for b in boxes]
        concat = torch.cat([b.bbox.reshape(-1, 4) for b in boxes], 0)
        outs = box_postprocess(class_logits, box_regression, concat, n_per_img, [b.size for b in boxes],
                               score_thresh=self.score_thresh, nms=self.nms, post_nms_per_cls_topn=self.post_nms_per_cls_topn,
                               nms_filter_duplicates=bool(self.nms_filter_duplicates or self.save_proposals),
                               detections_per_img=self.detections_per_img, reg_weights=self.box_coder.weights,
                               bbox_xform_clip=self.box_coder.bbox_xform_clip, cls_agnostic_bbox_reg=self.cls_agnostic_bbox_reg)
        results, nms_features = [], []
        for o, b, feat in zip(outs, boxes, features.split(n_per_img, dim=0)):
            inds = o["orig_inds"]
            res = type(b)(o["boxes"], b.size, mode="xyxy")
            res.add_field("pred_scores", o["pred_scores"])
            res.add_field("pred_labels", o["pred_labels"])
            if relation_mode and self.training:   # add_important_fields, :106-120
                assert b.has_field("labels")
                res.add_field("labels", b.get_field("labels")[inds])
            res.add_field("boxes_per_cls", o["boxes_per_cls"])
            res.add_field("predict_logits", b.get_field("predict_logits")[inds])
            results.append(res)
            nms_features.append(feat[inds])
        return torch.cat(nms_features, dim=0), results


def make_roi_box_post_processor(cfg):
    """inference.py:241-267: the keys it reads."""
    if cfg.TEST.BBOX_AUG.ENABLED:
        raise NotImplementedError("TEST.BBOX_AUG.ENABLED is not supported (the reference asserts it off, inference.py:93)")
    rh = cfg.MODEL.ROI_HEADS
    return PostProcessor(rh.SCORE_THRESH, rh.NMS, rh.POST_NMS_PER_CLS_TOPN, rh.NMS_FILTER_DUPLICATES, rh.DETECTIONS_PER_IMG,
                         BoxCoder(weights=rh.BBOX_REG_WEIGHTS), cfg.MODEL.CLS_AGNOSTIC_BBOX_REG, cfg.TEST.BBOX_AUG.ENABLED,
                         cfg.TEST.SAVE_PROPOSALS)
