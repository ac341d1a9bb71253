"""The box head's training loss, FastRCNNLossComputation (pysgg/modeling/roi_heads/box_head/loss.py:15-92), on the HIP device:
the caller side of veto_box_loss.

`box_loss_call` is the one ABI call: the cross entropy over every sampled row, the smooth-L1 box loss (beta 1) over the rows with
a positive label, both divided by labels.numel(), and their gradients w.r.t. class_logits and box_regression, two launches
whatever the batch and no device->host copy.  The reference's nonzero (whose count is read back), its advanced-index gather of
[P, 4] out of [R, 4C] and its backward's scatter into a zero-filled [R, 4C] do not exist here.  Semantics, the order of summation
and the NaN cases: include/veto_amd.h.

`FastRCNNLossComputation` wraps the call in the reference's constructor and `__call__`; the two losses come out of one
torch.autograd.Function whose backward scales the gradients the forward call already wrote."""
import ctypes

import torch

from . import native

MAX_CLASSES = 1024          # veto_box_loss; the decoder's limit
MAX_ROWS = 1 << 20
_WANT = {"losses", "grads"}


def _check_shapes(class_logits, box_regression, labels, regression_targets, cls_agnostic_bbox_reg):
    """The argument checks that need neither the device nor the library.  Returns (R, C, reg_cols)."""
    if class_logits.dim() != 2:
        raise ValueError("class_logits must be [R, C], got %s" % (tuple(class_logits.shape),))
    R, C = (int(v) for v in class_logits.shape)
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError("%d classes: 2..%d are supported" % (C, MAX_CLASSES))
    if R > MAX_ROWS:
        raise ValueError("%d rows, the limit is %d" % (R, MAX_ROWS))
    cols = 8 if cls_agnostic_bbox_reg else 4 * C
    got = tuple(box_regression.shape)
    if cls_agnostic_bbox_reg:   # the reference's predictor makes 8 columns; a wider tensor is read at columns 4..7 all the same
        if box_regression.dim() != 2 or got[0] != R or got[1] < 8 or got[1] % 4:
            raise ValueError("box_regression must be [%d, >= 8] with a multiple of 4 columns, got %s" % (R, got))
    elif got != (R, cols):
        raise ValueError("box_regression must be [%d, %d], got %s" % (R, cols, got))
    if labels.dim() != 1 or int(labels.shape[0]) != R:
        raise ValueError("labels must be [%d], got %s" % (R, tuple(labels.shape)))
    if tuple(regression_targets.shape) != (R, 4):
        raise ValueError("regression_targets must be [%d, 4], got %s" % (R, tuple(regression_targets.shape)))
    return R, C, int(box_regression.shape[1])


def _in_place(t):
    """t as the call reads it: fp32 rows of unit column stride behind a non-negative row stride, else a contiguous fp32 copy."""
    t = t.detach()
    if t.dtype != torch.float32 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.to(torch.float32).contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def box_loss_call(class_logits, box_regression, labels, regression_targets, *, cls_agnostic_bbox_reg=False, want=("losses", "grads")):
    """One veto_box_loss call.  class_logits [R, C] and box_regression [R, 4C] ([R, 8] or wider when class-agnostic) are read in
    place when they are fp32 with unit column stride, a column slice of a wider tensor included; labels [R] (converted to
    int64); regression_targets [R, 4].  want: 'losses', 'grads' or both ('grads' implies 'losses').  Returns a dict of device
    tensors: losses float [2] (classification_loss, box_loss); d_class_logits [R, C] and d_box_regression in box_regression's
    shape, contiguous, for an upstream gradient of 1, every element written by the call.  R = 0: both losses NaN.  A label outside
    [0, C) makes both losses and its two gradient rows NaN.  No device->host copy."""
    want = set(want)
    if not want or want - _WANT:
        raise ValueError("want: unknown or no outputs %s" % sorted(want - _WANT))
    R, C, cols = _check_shapes(class_logits, box_regression, labels, regression_targets, cls_agnostic_bbox_reg)
    device = class_logits.device
    for name, t in (("box_regression", box_regression), ("labels", labels), ("regression_targets", regression_targets)):
        if t.device != device:
            raise ValueError("%s is on %s, class_logits on %s" % (name, t.device, device))
    call = native.Launch(device, "veto_amd box loss runs on a HIP device only")
    logits, ld_logits = _in_place(class_logits)
    reg, ld_reg = _in_place(box_regression)
    labels = labels.detach().to(torch.int64).contiguous()          # loss.py:64, labels.long()
    targets = regression_targets.detach().to(torch.float32).contiguous()
    out = {"losses": torch.empty(2, dtype=torch.float32, device=device)}
    if "grads" in want:
        out["d_class_logits"] = torch.empty((R, C), dtype=torch.float32, device=device)
        out["d_box_regression"] = torch.empty((R, cols), dtype=torch.float32, device=device)
    a = call.args(native.VetoBoxLossArgs, n_rows=R, n_cls=C, n_reg_cols=cols, cls_agnostic=int(bool(cls_agnostic_bbox_reg)),
                  ld_logits=int(ld_logits), ld_reg=int(ld_reg), class_logits=logits, box_regression=reg, labels=labels,
                  regression_targets=targets, losses=out["losses"], d_class_logits=out.get("d_class_logits"),
                  d_box_regression=out.get("d_box_regression"))
    need = call.lib.veto_box_loss_workspace_bytes(ctypes.byref(a))   # (0: the shapes are out of range, the call says which)
    ws = call.workspace(need)
    call.run("veto_box_loss", ctypes.byref(a), ws.data_ptr(), ws.numel())
    return out


class _BoxLossFn(torch.autograd.Function):
    """(classification_loss, box_loss); the forward's one call has already written both gradients."""

    @staticmethod
    def forward(ctx, class_logits, box_regression, labels, regression_targets, cls_agnostic_bbox_reg):
        out = box_loss_call(class_logits, box_regression, labels, regression_targets, cls_agnostic_bbox_reg=cls_agnostic_bbox_reg,
                            want=("losses", "grads"))
        ctx.save_for_backward(out["d_class_logits"], out["d_box_regression"])
        ctx.dtypes = (class_logits.dtype, box_regression.dtype)
        return out["losses"][0], out["losses"][1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        d_logits, d_reg = ctx.saved_tensors
        return (d_logits * g_cls).to(ctx.dtypes[0]), (d_reg * g_box).to(ctx.dtypes[1]), None, None, None


def _cat(tensors):
    """modeling/utils.py:9-16: a list of one tensor is that tensor, no copy."""
    tensors = list(tensors)
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=0)


class FastRCNNLossComputation(object):
    """loss.py:15-84 with the reference's constructor and __call__.  The reference's assign_label_to_proposals on this class reads
    a proposal_matcher the class never sets: it is dead code and is not carried over; the labelling that runs is
    boxsampling.FastRCNNSampling.assign_label_to_proposals."""

    def __init__(self, cls_agnostic_bbox_reg=False):
        self.cls_agnostic_bbox_reg = cls_agnostic_bbox_reg

    def __call__(self, class_logits, box_regression, proposals):
        """class_logits, box_regression: lists of tensors (one entry, as box_head.py:133 passes, is used in place; more are
        concatenated); proposals: BoxLists carrying 'labels' and 'regression_targets' (subsample has run).  Returns
        (classification_loss, box_loss): two 0-dim device tensors, differentiable when an input requires grad (the gradients
        are asked of the call only then)."""
        class_logits, box_regression, proposals = list(class_logits), list(box_regression), list(proposals)
        if not class_logits or len(class_logits) != len(box_regression):
            raise ValueError("class_logits and box_regression must be equally long, non-empty lists (got %d and %d)"
                             % (len(class_logits), len(box_regression)))
        if not proposals:
            raise ValueError("the box loss needs the sampled proposals of at least one image")
        logits, reg = _cat(class_logits), _cat(box_regression)
        labels = _cat([p.get_field("labels").reshape(-1) for p in proposals])
        targets = _cat([p.get_field("regression_targets").reshape(-1, 4) for p in proposals])
        _check_shapes(logits, reg, labels, targets, self.cls_agnostic_bbox_reg)
        if torch.is_grad_enabled() and (logits.requires_grad or reg.requires_grad):
            return _BoxLossFn.apply(logits, reg, labels, targets, bool(self.cls_agnostic_bbox_reg))
        losses = box_loss_call(logits, reg, labels, targets, cls_agnostic_bbox_reg=self.cls_agnostic_bbox_reg, want=("losses",))["losses"]
        return losses[0], losses[1]


def make_roi_box_loss_evaluator(cfg):
    """loss.py:87-92: the one key it reads."""
    return FastRCNNLossComputation(cfg.MODEL.CLS_AGNOSTIC_BBOX_REG)
