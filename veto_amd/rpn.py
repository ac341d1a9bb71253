"""The RPN's proposal selection (pysgg/modeling/rpn/inference.py:13-210) on the HIP device.

`rpn_proposals` runs veto_rpn_proposals once per batch: per image and pyramid level the top-k of the objectness logits,
BoxCoder.decode of the selected anchors, clipping, the small-box filter and NMS, then the merge over the levels -- three
launches (four in per-batch mode) whatever the number of images or levels, reading the RPN head's NCHW outputs in place.  The
per-image counts are read back once (the only device->host copy) to split the outputs.  `RPNPostProcessor` wraps it in the
reference's constructor and forward contract; it has no backward (the reference's proposals carry no gradient either)."""
import ctypes
import math

import torch
from torch import nn

from . import native
from .boxhead import BoxCoder, _image_sizes


def _check_shapes(objectness, box_regression, anchors, image_sizes, pre_nms_top_n):
    """The argument checks that need neither the device nor the library.  Returns (n_img, [(A, H, W)])."""
    n_lvl = len(objectness)
    if n_lvl == 0 or n_lvl > native.RPN_MAX_LEVELS:
        raise ValueError("%d pyramid levels: 1..%d are supported" % (n_lvl, native.RPN_MAX_LEVELS))
    if len(box_regression) != n_lvl or len(anchors) != n_lvl:
        raise ValueError("objectness, box_regression and anchors must hold one entry per level (%d, %d, %d)"
                         % (n_lvl, len(box_regression), len(anchors)))
    if int(pre_nms_top_n) <= 0:
        raise ValueError("pre_nms_top_n must be positive, got %s" % (pre_nms_top_n,))
    n_img, shapes = len(image_sizes), []
    for l, (o, r, a) in enumerate(zip(objectness, box_regression, anchors)):
        if o.dim() != 4 or int(o.shape[0]) != n_img:
            raise ValueError("objectness[%d] must be [%d, A, H, W], got %s" % (l, n_img, tuple(o.shape)))
        A, H, W = (int(v) for v in o.shape[1:])
        if tuple(r.shape) != (n_img, 4 * A, H, W):
            raise ValueError("box_regression[%d] must be %s, got %s" % (l, (n_img, 4 * A, H, W), tuple(r.shape)))
        if tuple(a.shape) != (A * H * W, 4):
            raise ValueError("anchors[%d] must be %s, got %s" % (l, (A * H * W, 4), tuple(a.shape)))
        shapes.append((A, H, W))
    return n_img, shapes


def _row_bound(shapes, pre_nms_top_n, post_nms_top_n, nms_thresh, fpn_post_nms_top_n):
    """Rows an image can emit at most."""
    per_level = []
    for A, H, W in shapes:
        k = min(int(pre_nms_top_n), A * H * W)
        per_level.append(min(k, int(post_nms_top_n)) if nms_thresh > 0 and post_nms_top_n > 0 else k)
    total = sum(per_level)
    return min(total, int(fpn_post_nms_top_n)) if len(shapes) > 1 else total


def rpn_proposals_padded(objectness, box_regression, anchors, image_sizes, *, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size,
                         fpn_post_nms_top_n=None, per_batch=False, weights=(1., 1., 1., 1.), bbox_xform_clip=math.log(1000. / 16),
                         rows_per_image=None, out=None):
    """One veto_rpn_proposals call.  Image i owns rows_per_image[i] output rows (default: the most it can emit).  Returns
    (rows_per_image, dict of padded device tensors boxes / objectness / level / anchor_index, counts as a host list); an image
    whose rows are too few reports -(rows needed) and leaves its rows as they were (`out`: the tensors to write into)."""
    n_img, shapes = _check_shapes(objectness, box_regression, anchors, image_sizes, pre_nms_top_n)
    device = objectness[0].device
    call = native.Launch(device, "veto_amd RPN proposal selection runs on a HIP device only")
    if fpn_post_nms_top_n is None:
        fpn_post_nms_top_n = post_nms_top_n
    f32 = dict(device=device, dtype=torch.float32)
    objectness = [o.detach().to(**f32).contiguous() for o in objectness]
    box_regression = [r.detach().to(**f32).contiguous() for r in box_regression]
    anchors = [a.detach().to(**f32).contiguous() for a in anchors]
    sizes = _image_sizes([(float(w), float(h)) for w, h in image_sizes], device)
    if rows_per_image is None:
        rows_per_image = [_row_bound(shapes, pre_nms_top_n, post_nms_top_n, nms_thresh, fpn_post_nms_top_n)] * n_img
    rows_per_image = [int(r) for r in rows_per_image]
    rows = sum(rows_per_image)
    if out is None:
        out = dict(boxes=torch.empty((rows, 4), **f32), objectness=torch.empty(rows, **f32),
                   level=torch.empty(rows, dtype=torch.int32, device=device),
                   anchor_index=torch.empty(rows, dtype=torch.int64, device=device))
    counts = torch.empty(n_img, dtype=torch.int32, device=device)
    a = call.args(native.VetoRpnArgs, n_img=n_img, n_lvl=len(shapes), pre_nms_top_n=int(pre_nms_top_n),
                  post_nms_top_n=int(post_nms_top_n), fpn_post_nms_top_n=int(fpn_post_nms_top_n), per_batch=int(bool(per_batch)),
                  nms_thresh=float(nms_thresh), min_size=float(min_size), bbox_xform_clip=float(bbox_xform_clip),
                  reg_weights=(ctypes.c_float * 4)(*[float(w) for w in weights]), image_sizes=sizes,
                  img_out_offset=native.device_offsets(rows_per_image, device=device)[0], boxes=out["boxes"],
                  objectness_out=out["objectness"], level=out["level"], anchor_index=out["anchor_index"], counts=counts)
    for l, (A, H, W) in enumerate(shapes):
        a.level_a[l], a.level_h[l], a.level_w[l] = A, H, W
        a.objectness[l], a.box_regression[l], a.anchors[l] = call.ptr(objectness[l]), call.ptr(box_regression[l]), call.ptr(anchors[l])
    need = call.lib.veto_rpn_proposals_workspace_bytes(ctypes.byref(a))   # (0: the shapes are out of range, the call says which)
    ws = call.workspace(need)
    call.run("veto_rpn_proposals", ctypes.byref(a), ws.data_ptr(), ws.numel())
    kept = counts.tolist()   # the one device->host copy of the batch: the counts decide the split
    return rows_per_image, out, kept


def rpn_proposals(objectness, box_regression, anchors, image_sizes, *, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size,
                  fpn_post_nms_top_n=None, per_batch=False, weights=(1., 1., 1., 1.), bbox_xform_clip=math.log(1000. / 16)):
    """RPNPostProcessor.forward without the BoxLists.  Per level l: objectness[l] [n_img, A, H, W] logits, box_regression[l]
    [n_img, 4A, H, W], anchors[l] [A H W, 4] xyxy (anchor (h W + w) A + a), all on the HIP device; image_sizes = (width, height)
    per image.  Returns per image a dict of device tensors: boxes [K, 4], objectness [K], level int32 [K], anchor_index int64
    [K] (inside the level)."""
    caps, out, kept = rpn_proposals_padded(objectness, box_regression, anchors, image_sizes, pre_nms_top_n=pre_nms_top_n,
                                           post_nms_top_n=post_nms_top_n, nms_thresh=nms_thresh, min_size=min_size,
                                           fpn_post_nms_top_n=fpn_post_nms_top_n, per_batch=per_batch, weights=weights,
                                           bbox_xform_clip=bbox_xform_clip)
    if min(kept) < 0:
        raise native.VetoError("veto_rpn_proposals: proposals %s do not fit the rows %s" % (kept, caps))
    res, row = [], 0
    for cap, k in zip(caps, kept):
        res.append({name: t[row:row + k] for name, t in out.items()})
        row += cap
    return res


class RPNPostProcessor(nn.Module):
    """inference.py:13-183 with the reference's constructor and forward contract."""

    def __init__(self, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, box_coder=None, fpn_post_nms_top_n=None,
                 fpn_post_nms_per_batch=True, add_gt=True):
        super().__init__()
        self.pre_nms_top_n = pre_nms_top_n
        self.post_nms_top_n = post_nms_top_n
        self.nms_thresh = nms_thresh
        self.min_size = min_size
        self.add_gt = add_gt
        self.box_coder = box_coder if box_coder is not None else BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.fpn_post_nms_top_n = post_nms_top_n if fpn_post_nms_top_n is None else fpn_post_nms_top_n
        self.fpn_post_nms_per_batch = fpn_post_nms_per_batch

    @torch.no_grad()
    def forward(self, anchors, objectness, box_regression, targets=None):
        """anchors: list[list[BoxList]], image-major (the boxes are taken from the first image's lists, the sizes from every
        image's); objectness / box_regression: one tensor per level.  Returns one BoxList per image, mode xyxy, with the
        field 'objectness'."""
        first = anchors[0]
        outs = rpn_proposals(objectness, box_regression, [lvl.bbox for lvl in first], [per_img[0].size for per_img in anchors],
                             pre_nms_top_n=self.pre_nms_top_n, post_nms_top_n=self.post_nms_top_n, nms_thresh=self.nms_thresh,
                             min_size=self.min_size, fpn_post_nms_top_n=self.fpn_post_nms_top_n,
                             per_batch=bool(self.training and self.fpn_post_nms_per_batch), weights=self.box_coder.weights,
                             bbox_xform_clip=self.box_coder.bbox_xform_clip)
        add_gt = self.training and targets is not None and self.add_gt   # add_gt_proposals, :55-76
        boxlists = []
        for i, (o, per_img) in enumerate(zip(outs, anchors)):
            boxes, scores = o["boxes"], o["objectness"]
            if add_gt:
                gt = targets[i].convert("xyxy").bbox.to(boxes)
                boxes = torch.cat([boxes, gt], 0)
                scores = torch.cat([scores, torch.ones(len(gt), dtype=scores.dtype, device=scores.device)], 0)
            res = type(first[0])(boxes, per_img[0].size, mode="xyxy")
            res.add_field("objectness", scores)
            boxlists.append(res)
        return boxlists


def make_rpn_postprocessor(config, rpn_box_coder, is_train):
    """inference.py:186-210: the keys it reads."""
    rpn = config.MODEL.RPN
    return RPNPostProcessor(pre_nms_top_n=rpn.PRE_NMS_TOP_N_TRAIN if is_train else rpn.PRE_NMS_TOP_N_TEST,
                            post_nms_top_n=rpn.POST_NMS_TOP_N_TRAIN if is_train else rpn.POST_NMS_TOP_N_TEST,
                            nms_thresh=rpn.NMS_THRESH, min_size=rpn.MIN_SIZE, box_coder=rpn_box_coder,
                            fpn_post_nms_top_n=rpn.FPN_POST_NMS_TOP_N_TRAIN if is_train else rpn.FPN_POST_NMS_TOP_N_TEST,
                            fpn_post_nms_per_batch=rpn.FPN_POST_NMS_PER_BATCH,
                            add_gt=config.MODEL.ROI_RELATION_HEAD.ADD_GTBOX_TO_PROPOSAL_IN_TRAIN)
