"""Test-time pair enumeration, the caller-side contract of the hot path.

Mirrors `RelationSampling.prepare_test_pairs` (sampling.py:31-52).  GT-box modes (predcls / sgcls, the
benchmarked path): every ordered pair (i, j), i != j, in the row-major order of `torch.nonzero(ones - eye)`,
or the `[[0, 0]]` placeholder when an image has no candidate pair; the enumeration runs on the device through
the C ABI (veto_enumerate_pairs) and the MAX_PROPOSAL_PAIR cap is a host-issued torch.sort.

Detected boxes (sgdet, `use_gt_box=False`): one veto_prepare_test_pairs launch for the batch does the optional
box-overlap filter (REQUIRE_BOX_OVERLAP, `boxlist_iou(p, p) > 0`), the row-major enumeration and the cap, whose
survivors come in the total order (quality desc, row-major index asc) -- what torch.sort(stable=True,
descending=True) gives; the reference's unstable sort leaves the order of tied pairs, e.g. (i, j) and (j, i),
unspecified.  Without the filter every image's pair count is known on the host.  With it, the counts are data
dependent: the batch's int32 counts are read back once (one device->host copy per batch) to split the list."""
import ctypes

import torch

from . import native


def prepare_test_pairs(device, proposals, max_proposal_pairs=2048, require_overlap=False, use_gt_box=True):
    call = native.Launch(device, "veto_amd.prepare_test_pairs runs on a HIP device only")
    device = call.device
    if not use_gt_box:
        return _prepare_detected_pairs(call, proposals, max_proposal_pairs, require_overlap)
    out = []
    for p in proposals:
        n = len(p)
        total = n * (n - 1) if n > 1 else 1
        idxs = torch.empty((total, 2), dtype=torch.int64, device=device)
        call.run("veto_enumerate_pairs", n, idxs.data_ptr())
        if total > max_proposal_pairs:
            # sampling.py:41-45: keep the MAX_PROPOSAL_PAIR best pairs by pred_scores product
            q = p.get_field("pred_scores").to(device)
            q = q[idxs[:, 0]] * q[idxs[:, 1]]
            idxs = idxs[torch.sort(q, descending=True)[1][:max_proposal_pairs]]
        out.append(idxs)
    return out


def pair_capacity(n, max_proposal_pairs):
    """Rows reserved for an image of n detections: all ordered pairs (or the placeholder), at most the cap."""
    return min(max(n * (n - 1), 1), max_proposal_pairs)


def _prepare_detected_pairs(call, proposals, max_proposal_pairs, require_overlap):
    device = call.device
    n_objs = [len(p) for p in proposals]
    caps = [pair_capacity(n, max_proposal_pairs) for n in n_objs]
    f32 = dict(device=device, dtype=torch.float32)
    boxes = torch.cat([p.convert("xyxy").bbox.reshape(-1, 4) for p in proposals], 0).to(**f32).contiguous()
    scores = torch.cat([p.get_field("pred_scores").reshape(-1) for p in proposals], 0).to(**f32).contiguous()
    off = native.device_offsets(n_objs, caps, device=device)
    pairs = torch.empty((sum(caps), 2), dtype=torch.int64, device=device)
    counts = torch.empty(len(proposals), dtype=torch.int32, device=device)
    a = call.args(native.VetoPairArgs, n_img=len(proposals), n_obj=sum(n_objs), max_obj_per_image=max(n_objs),
                  max_pairs=int(max_proposal_pairs), require_overlap=int(bool(require_overlap)), boxes=boxes, scores=scores,
                  img_obj_offset=off[0], img_out_offset=off[1], pairs=pairs, counts=counts)
    call.run("veto_prepare_test_pairs", ctypes.byref(a))
    rows = pairs.split(caps)
    if not require_overlap:
        return list(rows)
    kept = counts.tolist()   # the one device->host copy of the batch: the filtered counts decide the split
    return [r[:k] for r, k in zip(rows, kept)]
