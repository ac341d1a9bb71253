"""Object decoding on detected boxes (sgdet), shared by the PostProcessor and the MEET predictor.

`decode_objects` runs veto_obj_decode: the reference's greedy class-aware NMS over the object class probabilities,
  mode "post": obj_prediction_nms (relation_head/utils_relation.py:94-128) as the PostProcessor applies it
               (inference.py:410-429), returning labels, scores softmax(logits)[i, label_i] and the regressed boxes
               boxes_per_cls[i, label_i];
  mode "meet": Ensemble.nms_per_cls (roi_relation_predictors.py:3855-3874), the MEET decoder's labels, from the
               labels of its one-hot input (pass them as `logits`, int64 [sum N]).
One workgroup per image, all on the device: no host copy."""
import ctypes

import torch

from . import native

MODES = {"post": 0, "meet": 1}


def decode_objects(logits, boxes_per_cls, n_objs, nms_thres, mode="post", want_scores=True, want_boxes=True):
    """logits [sum N, C] and boxes_per_cls [sum N, C, 4] (xyxy) on the HIP device; n_objs = per-image counts.
    Returns (labels int64 [sum N], scores fp32 [sum N] or None, boxes fp32 [sum N, 4] or None)."""
    device = logits.device
    n_obj = int(logits.shape[0])
    n_cls = int(boxes_per_cls.shape[1])
    if tuple(boxes_per_cls.shape) != (n_obj, n_cls, 4):
        raise ValueError("boxes_per_cls must be [%d, %d, 4], got %s" % (n_obj, n_cls, tuple(boxes_per_cls.shape)))
    if sum(n_objs) != n_obj:
        raise ValueError("per-image counts %s do not add up to %d rows" % (list(n_objs), n_obj))
    call = native.Launch(device, "veto_amd sgdet decoding runs on a HIP device only")
    f32 = dict(device=device, dtype=torch.float32)
    meet = mode == "meet"
    logits = logits.detach().to(device=device, dtype=torch.int64 if meet else torch.float32).contiguous()
    if meet and want_scores:
        raise ValueError("the MEET decoder's labels come without scores")
    boxes_per_cls = boxes_per_cls.detach().to(**f32).contiguous()
    pred = torch.empty(n_obj, dtype=torch.int64, device=device)
    scores = torch.empty(n_obj, **f32) if want_scores else None
    boxes = torch.empty((n_obj, 4), **f32) if want_boxes else None
    a = call.args(native.VetoObjDecodeArgs, n_img=len(n_objs), n_obj=n_obj, n_cls=n_cls, max_obj_per_image=max(n_objs),
                  mode=MODES[mode], nms_thres=float(nms_thres), labels=logits if meet else None, logits=None if meet else logits,
                  boxes_per_cls=boxes_per_cls, img_obj_offset=native.device_offsets(n_objs, device=device)[0], obj_pred=pred,
                  obj_scores=scores, boxes=boxes)
    ws = call.workspace(call.lib.veto_obj_decode_workspace_bytes(n_obj, n_cls))
    call.run("veto_obj_decode", ctypes.byref(a), ws.data_ptr(), ws.numel())
    return pred, scores, boxes
