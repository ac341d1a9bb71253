"""The RPN's training loss, RPNLossComputation (pysgg/modeling/rpn/loss.py:21-157), on the HIP device: the caller side of
veto_rpn_loss.

`rpn_loss_call` is the one ABI call: anchor matching (Matcher with or without allow_low_quality_matches), the labels with the
anchors' visibility, BoxCoder.encode, the balanced fg/bg sampling, both losses and their gradients w.r.t. the RPN head's NCHW
outputs, seven launches whatever the batch or the pyramid and no device->host copy.  The reference's per-image loop (a
[n_gt, n_anchor] boxlist_iou matrix, max over both axes, a nonzero over an equality mask, two nonzero / randperm pairs) and its
permute + concatenate of every level's outputs do not exist here.  Matching is bit-equal to the reference's (see
include/veto_amd.h); the draws have its distribution (randperm(m)[:k] as a set) from the counter-based hash of
veto_box_subsample, so they are not its draws for a given torch seed.

`RPNLossComputation` wraps the call in the reference's constructor, `prepare_targets` and `__call__`; the two losses come out of
one torch.autograd.Function over the lists of head outputs, whose backward scales the gradients the forward call already wrote."""
import ctypes

import numpy as np
import torch

from . import native
from .boxhead import BoxCoder, _image_sizes  # noqa: F401  (BoxCoder: what make_rpn_loss_evaluator is handed)
from .boxsampling import MAX_BATCH_SIZE_PER_IMAGE, NO_GT_BOXES, BalancedPositiveNegativeSampler

MAX_GT_PER_IMAGE = 256            # veto_rpn_loss
MAX_ANCHORS_PER_IMAGE = 1 << 20
SMOOTH_L1_BETA = 1.0 / 9          # loss.py:123


class Matcher:
    """matcher.py:5-40: the thresholds and the low-quality switch veto_rpn_loss matches by.  The matching itself, the
    low-quality step included, runs inside the kernels."""
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        assert low_threshold <= high_threshold
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches


def generate_rpn_labels(matched_targets):
    """loss.py:134-137.  RPNLossComputation takes this function as the name of the labelling the kernels implement
    (matched_idxs >= 0); it is never called on the device path."""
    return matched_targets.get_field("matched_idxs") >= 0


def _check_shapes(anchors, n_gt, batch_size_per_image, objectness=None, box_regression=None):
    """The argument checks that need neither the device nor the library.  Returns [(A, H, W)] when the head outputs are given."""
    n_lvl, n_img = len(anchors), len(n_gt)
    if n_lvl == 0 or n_lvl > native.RPN_MAX_LEVELS:
        raise ValueError("%d pyramid levels: 1..%d are supported" % (n_lvl, native.RPN_MAX_LEVELS))
    B = int(batch_size_per_image)
    if not 1 <= B <= MAX_BATCH_SIZE_PER_IMAGE:
        raise ValueError("batch_size_per_image %d outside 1..%d (MODEL.RPN.BATCH_SIZE_PER_IMAGE)" % (B, MAX_BATCH_SIZE_PER_IMAGE))
    if n_img == 0:
        raise ValueError("the RPN loss needs at least one image")
    for i, m in enumerate(n_gt):
        if m == 0:
            raise ValueError(NO_GT_BOXES)                                  # matcher.py:55-58
        if m > MAX_GT_PER_IMAGE:
            raise ValueError("image %d holds %d GT boxes, the limit is %d" % (i, m, MAX_GT_PER_IMAGE))
    for l, a in enumerate(anchors):
        if a.dim() != 2 or a.shape[1] != 4 or a.shape[0] == 0:
            raise ValueError("anchors[%d] must be [A H W, 4], got %s" % (l, tuple(a.shape)))
    n_anchor = sum(int(a.shape[0]) for a in anchors)
    if n_anchor > MAX_ANCHORS_PER_IMAGE:
        raise ValueError("an image holds %d anchors, the limit is %d" % (n_anchor, MAX_ANCHORS_PER_IMAGE))
    if objectness is None:
        return None
    if len(objectness) != n_lvl or len(box_regression) != n_lvl:
        raise ValueError("objectness, box_regression and anchors must hold one entry per level (%d, %d, %d)"
                         % (len(objectness), len(box_regression), n_lvl))
    shapes = []
    for l, (o, r, a) in enumerate(zip(objectness, box_regression, anchors)):
        if o.dim() != 4 or int(o.shape[0]) != n_img:
            raise ValueError("objectness[%d] must be [%d, A, H, W], got %s" % (l, n_img, tuple(o.shape)))
        A, H, W = (int(v) for v in o.shape[1:])
        if tuple(r.shape) != (n_img, 4 * A, H, W):
            raise ValueError("box_regression[%d] must be %s, got %s" % (l, (n_img, 4 * A, H, W), tuple(r.shape)))
        if int(a.shape[0]) != A * H * W:
            raise ValueError("anchors[%d] must be %s, got %s" % (l, (A * H * W, 4), tuple(a.shape)))
        shapes.append((A, H, W))
    return shapes


def rpn_loss_call(anchors, image_sizes, tgt_boxes, *, high_threshold, low_threshold, allow_low_quality_matches=True,
                  straddle_thresh=0, weights=(1., 1., 1., 1.), batch_size_per_image=256, positive_fraction=0.5, seed=None,
                  objectness=None, box_regression=None, want=("losses", "grads"), level_shapes=None):
    """One veto_rpn_loss call.  anchors: per level [A H W, 4] xyxy (anchor (h W + w) A + a); image_sizes: (width, height) per
    image; tgt_boxes: per image [n_gt, 4] xyxy; objectness / box_regression: per level [n_img, A, H, W] / [n_img, 4A, H, W], read
    in place (needed for 'losses' and 'grads' only).  want: any of 'losses', 'grads', 'labels', 'matched_idxs',
    'regression_targets', 'sampled_inds', 'counts'; the call stops after the stage the last of them needs.  Returns a dict of
    device tensors: losses float [2] (objectness_loss, box_loss); d_objectness / d_box_regression, lists in the head outputs'
    shapes, for an upstream gradient of 1; labels float [n_img, n_anchor]; matched_idxs int64; regression_targets
    [n_img, n_anchor, 4]; sampled_inds int64 [n_img, batch_size_per_image] (image i keeps the first counts[i].sum() entries, anchor
    indices inside the image, ascending); counts int32 [n_img, 2] (positives, negatives).  No device->host copy.
    seed: 64-bit; None draws one from torch's default CPU generator, so torch.manual_seed makes a run reproducible.
    level_shapes: [(A, H, W)] when no head outputs are given (A H W must equal the level's anchors)."""
    want = set(want)
    unknown = want - {"losses", "grads", "labels", "matched_idxs", "regression_targets", "sampled_inds", "counts"}
    if unknown or not want:
        raise ValueError("want: unknown or no outputs %s" % sorted(unknown))
    if "grads" in want:
        want.add("losses")
    n_gt = [int(t.shape[0]) for t in tgt_boxes]
    if len(image_sizes) != len(n_gt):
        raise ValueError("one image size per target list (got %d and %d)" % (len(image_sizes), len(n_gt)))
    with_head = "losses" in want
    if with_head and (objectness is None or box_regression is None):
        raise ValueError("the losses need objectness and box_regression")
    shapes = _check_shapes(anchors, n_gt, batch_size_per_image, objectness if with_head else None, box_regression)
    if shapes is None:
        shapes = level_shapes if level_shapes is not None else [(1, 1, int(a.shape[0])) for a in anchors]
        if len(shapes) != len(anchors) or any(A * H * W != int(a.shape[0]) for (A, H, W), a in zip(shapes, anchors)):
            raise ValueError("level_shapes %s do not match the anchors" % (shapes,))
    device = anchors[0].device
    call = native.Launch(device, "veto_amd RPN loss runs on a HIP device only")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
    n_img, n_anchor, B = len(n_gt), sum(int(a.shape[0]) for a in anchors), int(batch_size_per_image)
    f32 = dict(device=device, dtype=torch.float32)
    anchors = [a.detach().to(**f32).contiguous() for a in anchors]
    tgt = tgt_boxes[0].reshape(-1, 4) if len(tgt_boxes) == 1 else torch.cat([t.reshape(-1, 4) for t in tgt_boxes])   # (cat of one copies)
    tgt = tgt.detach().to(**f32).contiguous()
    host_tgt = np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int32)
    out = {}
    if "losses" in want:
        objectness = [o.detach().to(**f32).contiguous() for o in objectness]
        box_regression = [r.detach().to(**f32).contiguous() for r in box_regression]
        out["losses"] = torch.empty(2, **f32)
    if "grads" in want:
        out["d_objectness"] = [torch.empty_like(o) for o in objectness]
        out["d_box_regression"] = [torch.empty_like(r) for r in box_regression]
    if "labels" in want:
        out["labels"] = torch.empty((n_img, n_anchor), **f32)
    if "matched_idxs" in want:
        out["matched_idxs"] = torch.empty((n_img, n_anchor), dtype=torch.int64, device=device)
    if "regression_targets" in want:
        out["regression_targets"] = torch.empty((n_img, n_anchor, 4), **f32)
    if "sampled_inds" in want:
        out["sampled_inds"] = torch.empty((n_img, B), dtype=torch.int64, device=device)
    if "counts" in want:
        out["counts"] = torch.empty((n_img, 2), dtype=torch.int32, device=device)
    a = call.args(native.VetoRpnLossArgs, n_img=n_img, n_lvl=len(anchors), n_tgt=sum(n_gt), batch_size_per_image=B,
                  num_pos_per_img=int(B * positive_fraction),   # balanced_positive_negative_sampler.py:41
                  allow_low_quality_matches=int(bool(allow_low_quality_matches)), high_threshold=float(high_threshold),
                  low_threshold=float(low_threshold), straddle_thresh=float(straddle_thresh),
                  reg_weights=(ctypes.c_float * 4)(*[float(w) for w in weights]), beta=SMOOTH_L1_BETA, seed=seed & (2 ** 64 - 1),
                  image_sizes=_image_sizes([(float(w), float(h)) for w, h in image_sizes], device), tgt_boxes=tgt,
                  img_tgt_offset=native.device_offsets(n_gt, device=device)[0], img_tgt_offset_host=host_tgt.ctypes.data,
                  losses=out.get("losses"), labels=out.get("labels"), matched_idxs=out.get("matched_idxs"),
                  regression_targets=out.get("regression_targets"), sampled_inds=out.get("sampled_inds"), counts=out.get("counts"))
    for l, (A, H, W) in enumerate(shapes):
        a.level_a[l], a.level_h[l], a.level_w[l] = A, H, W
        a.anchors[l] = call.ptr(anchors[l])
        if "losses" in want:
            a.objectness[l], a.box_regression[l] = call.ptr(objectness[l]), call.ptr(box_regression[l])
        if "grads" in want:
            a.d_objectness[l], a.d_box_regression[l] = call.ptr(out["d_objectness"][l]), call.ptr(out["d_box_regression"][l])
    need = call.lib.veto_rpn_loss_workspace_bytes(ctypes.byref(a))   # (0: the shapes are out of range, the call says which)
    ws = call.workspace(need)
    call.run("veto_rpn_loss", ctypes.byref(a), ws.data_ptr(), ws.numel())
    return out


class _RPNLossFn(torch.autograd.Function):
    """(objectness_loss, box_loss) over the lists of head outputs; the forward's one call has already written both gradients."""

    @staticmethod
    def forward(ctx, settings, n_lvl, *head):
        out = rpn_loss_call(objectness=list(head[:n_lvl]), box_regression=list(head[n_lvl:]), want=("losses", "grads"), **settings)
        ctx.save_for_backward(*out["d_objectness"], *out["d_box_regression"])
        ctx.n_lvl = n_lvl
        return out["losses"][0], out["losses"][1]

    @staticmethod
    def backward(ctx, g_obj, g_box):
        saved = ctx.saved_tensors
        return (None, None) + tuple(d * g_obj for d in saved[:ctx.n_lvl]) + tuple(d * g_box for d in saved[ctx.n_lvl:])


class RPNLossComputation(object):
    """loss.py:21-131 with the reference's constructor, prepare_targets and __call__."""

    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, generate_labels_func):
        if getattr(generate_labels_func, "__name__", None) != "generate_rpn_labels":
            raise NotImplementedError("only generate_rpn_labels (matched_idxs >= 0, loss.py:134-137) is built on the device, got %r; "
                                      "RetinaNet's label function is not" % (generate_labels_func,))
        self.proposal_matcher = proposal_matcher
        self.fg_bg_sampler = fg_bg_sampler
        self.box_coder = box_coder
        self.copied_fields = []
        self.generate_labels_func = generate_labels_func
        self.discard_cases = ['not_visibility', 'between_thresholds']
        self.straddle_thresh = 0   # MODEL.RPN.STRADDLE_THRESH: the reference keeps it in the anchors' 'visibility' field

    def _settings(self, anchors, targets, seed=None):
        """anchors: list[list[BoxList]], image-major (the boxes are taken from the first image's lists, the sizes from every
        image's); targets: one BoxList per image."""
        if len(anchors) != len(targets) or not len(anchors):
            raise ValueError("the RPN loss needs one target per image (got %d anchor lists and %d targets)" % (len(anchors), len(targets)))
        for per_img, t in zip(anchors, targets):   # boxlist_iou, boxlist_ops.py:68-70
            if tuple(per_img[0].size) != tuple(t.size):
                raise RuntimeError("boxlists should have same image size, got {}, {}".format(t.size, per_img[0].size))
        m = self.proposal_matcher
        return dict(anchors=[lvl.convert("xyxy").bbox for lvl in anchors[0]], image_sizes=[per_img[0].size for per_img in anchors],
                    tgt_boxes=[t.convert("xyxy").bbox.reshape(-1, 4) for t in targets], high_threshold=m.high_threshold,
                    low_threshold=m.low_threshold, allow_low_quality_matches=bool(getattr(m, "allow_low_quality_matches", False)),
                    straddle_thresh=self.straddle_thresh, weights=self.box_coder.weights,
                    batch_size_per_image=self.fg_bg_sampler.batch_size_per_image,
                    positive_fraction=self.fg_bg_sampler.positive_fraction, seed=seed)

    def prepare_targets(self, anchors, targets):
        """(labels, regression_targets), one tensor per image each ([n_anchor] float, [n_anchor, 4]).  Three launches, no
        device->host copy."""
        out = rpn_loss_call(want=("labels", "regression_targets"), **self._settings(anchors, targets, seed=0))
        return list(out["labels"].unbind(0)), list(out["regression_targets"].unbind(0))

    def __call__(self, anchors, objectness, box_regression, targets, seed=None):
        """(objectness_loss, box_loss): two device scalars, differentiable when a head output requires grad (the gradients are
        asked of the call only then).
        seed: 64-bit; None draws one from torch's default generator, so torch.manual_seed makes a run reproducible."""
        settings = self._settings(anchors, targets, seed)
        objectness, box_regression = list(objectness), list(box_regression)
        if torch.is_grad_enabled() and any(t.requires_grad for t in objectness + box_regression):
            return _RPNLossFn.apply(settings, len(objectness), *objectness, *box_regression)
        losses = rpn_loss_call(objectness=objectness, box_regression=box_regression, want=("losses",), **settings)["losses"]
        return losses[0], losses[1]


def make_rpn_loss_evaluator(cfg, box_coder):
    """loss.py:140-157: the keys it reads, plus MODEL.RPN.STRADDLE_THRESH (anchor_generator.py:132; the reference's anchors carry
    it as their 'visibility' field)."""
    rpn = cfg.MODEL.RPN
    loss = RPNLossComputation(Matcher(rpn.FG_IOU_THRESHOLD, rpn.BG_IOU_THRESHOLD, allow_low_quality_matches=True),
                              BalancedPositiveNegativeSampler(rpn.BATCH_SIZE_PER_IMAGE, rpn.POSITIVE_FRACTION), box_coder,
                              generate_rpn_labels)
    loss.straddle_thresh = rpn.STRADDLE_THRESH
    return loss
