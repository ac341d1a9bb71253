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
from .predictor import cached_offsets


def max_segment():
    """Largest segment veto_nms takes (6144; MODEL.RPN.PRE_NMS_TOP_N_TEST is 6000)."""
    return int(native.load_library().veto_nms_max_segment())


def batched_nms(boxes, scores, offsets, threshold, max_keep=-1):
    """boxes [M, 4] xyxy and scores [M] on the HIP device; offsets = the S + 1 segment boundaries (a host sequence: 0, ...,
    M).  Returns (keep int64 [M], counts int32 [S]) on the device: segment s kept counts[s] boxes, whose indices LOCAL to
    the segment are keep[offsets[s] : offsets[s] + counts[s]], ascending."""
    device = boxes.device
    if device.type != "cuda":
        raise RuntimeError("veto_amd.layers.nms runs on a HIP device only (got %s)" % device)
    lib = native.load_library()
    host = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1))
    if host.size < 2:
        raise ValueError("offsets must hold at least two boundaries, got %d" % host.size)
    n_box = int(boxes.shape[0])
    boxes = boxes.detach().to(dtype=torch.float32).reshape(n_box, 4).contiguous()
    scores = scores.detach().to(device=device, dtype=torch.float32).reshape(n_box).contiguous()
    sizes = np.diff(host).tolist()
    if min(sizes) < 0:   # (the ABI checks again; a prefix sum of these sizes would hide it)
        raise native.VetoError("veto_amd native call failed (-1): seg_offset_host is not monotone: %s" % host.tolist())
    dev_off, _ = cached_offsets(sizes, [0] * len(sizes), device)
    keep = torch.empty(n_box, dtype=torch.int64, device=device)
    counts = torch.empty(len(sizes), dtype=torch.int32, device=device)
    a = native.VetoNmsArgs()
    a.struct_size = ctypes.sizeof(native.VetoNmsArgs)
    a.n_box, a.n_seg, a.max_keep, a.threshold = n_box, len(sizes), int(max_keep), float(threshold)
    a.boxes, a.scores = boxes.data_ptr(), scores.data_ptr()
    a.seg_offset, a.seg_offset_host = dev_off.data_ptr(), host.ctypes.data
    a.keep, a.counts = keep.data_ptr(), counts.data_ptr()
    stream = torch.cuda.current_stream(device)
    native.check(lib.veto_nms(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a)))
    for t in (boxes, scores, dev_off):
        t.record_stream(stream)
    return keep, counts


def nms(boxes, scores, threshold):
    """Drop-in for pysgg.layers.nms(boxes, scores, threshold): the kept indices, int64, ascending, on the boxes' device."""
    n = int(boxes.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    keep, counts = batched_nms(boxes, scores, (0, n), threshold)
    return keep[:int(counts.item())]
