"""Detector-side layers on the HIP device: the drop-in for `pysgg.layers.nms` (pysgg._C.nms, csrc/cuda/nms.cu).

`batched_nms` runs veto_nms: greedy NMS of any number of segments (one image x class, one image x pyramid level) in one
launch, with the reference GPU kernel's semantics -- devIoU with the +1 pixel convention, suppression at IoU strictly
greater than the threshold, boxes visited by (score desc, index asc), kept indices returned in ascending index order, a cap
that keeps the first `max_keep` of that ascending list.  Nothing is copied to the host and nothing synchronises.

`nms` is the one-segment form with the reference's signature.  It returns a tensor whose LENGTH is the result, so it reads
one int32 back (the reference copies the whole n x n/64 mask to the host at the same point)."""
import ctypes

import numpy as np
import torch

from . import native


def max_segment():
    """Largest segment veto_nms takes (6144; MODEL.RPN.PRE_NMS_TOP_N_TEST is 6000)."""
    return int(native.load_library().veto_nms_max_segment())


def batched_nms(boxes, scores, offsets, threshold, max_keep=-1):
    """boxes [M, 4] xyxy and scores [M] on the HIP device; offsets = the S + 1 segment boundaries (a host sequence: 0, ...,
    M).  Returns (keep int64 [M], counts int32 [S]) on the device: segment s kept counts[s] boxes, whose indices LOCAL to
    the segment are keep[offsets[s] : offsets[s] + counts[s]], ascending."""
    device = boxes.device
    call = native.Launch(device, "veto_amd.layers.nms runs on a HIP device only")
    host = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1))
    if host.size < 2:
        raise ValueError("offsets must hold at least two boundaries, got %d" % host.size)
    n_box = int(boxes.shape[0])
    boxes = boxes.detach().to(dtype=torch.float32).reshape(n_box, 4).contiguous()
    scores = scores.detach().to(device=device, dtype=torch.float32).reshape(n_box).contiguous()
    sizes = np.diff(host).tolist()
    if min(sizes) < 0:   # (the ABI checks again; a prefix sum of these sizes would hide it)
        raise native.VetoError("veto_amd native call failed (-1): seg_offset_host is not monotone: %s" % host.tolist())
    keep = torch.empty(n_box, dtype=torch.int64, device=device)
    counts = torch.empty(len(sizes), dtype=torch.int32, device=device)
    a = call.args(native.VetoNmsArgs, n_box=n_box, n_seg=len(sizes), max_keep=int(max_keep), threshold=float(threshold), boxes=boxes,
                  scores=scores, seg_offset=native.device_offsets(sizes, device=device)[0], seg_offset_host=host.ctypes.data,
                  keep=keep, counts=counts)
    call.run("veto_nms", ctypes.byref(a))
    return keep, counts


def nms(boxes, scores, threshold):
    """Drop-in for pysgg.layers.nms(boxes, scores, threshold): the kept indices, int64, ascending, on the boxes' device."""
    n = int(boxes.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    keep, counts = batched_nms(boxes, scores, (0, n), threshold)
    return keep[:int(counts.item())]
