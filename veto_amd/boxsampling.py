"""The box head's training-time sampler, FastRCNNSampling (pysgg/modeling/roi_heads/box_head/sampling.py:14-156), on the HIP
device: the caller side of veto_box_match and veto_box_subsample.

`assign_label_to_proposals` is what sgdet training calls (box_head.py:92-94): it gives every proposal the label of the GT box it
matches, the field `labels` that `boxhead.PostProcessor` carries over and `DetectRelationSampler` reads.  It and
`prepare_targets` make one launch for the batch and no device->host copy.  `subsample` makes two launches, reads the per-image
counts back once and gathers every field of the sampled proposals with one index per field.

The reference's per-image loop (a boxlist_iou matrix, Matcher, clamp, gather, masked writes) does not exist here.  Matching is
bit-equal to it (see include/veto_amd.h); the draws of `subsample` have its distribution (randperm(m)[:k] as a set), from a
counter-based hash instead of torch's generator, so they are not its draws for a given torch seed.  Boxes are matched and
encoded as xyxy (the reference encodes `.bbox` as it is, which is the same for the xyxy lists the detector passes)."""
import ctypes

import numpy as np
import torch

from . import native
from .boxhead import BoxCoder

MAX_BATCH_SIZE_PER_IMAGE = 2048   # veto_box_subsample
NO_GT_BOXES = "No ground-truth boxes available for one of the images during training"        # matcher.py:56-58
NO_PROPOSALS = "No proposal boxes available for one of the images during training"           # matcher.py:60-62


class Matcher:
    """matcher.py:5-40: the thresholds veto_box_match stratifies by.  The matching itself runs inside the kernel."""
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        assert low_threshold <= high_threshold
        if allow_low_quality_matches:
            raise NotImplementedError("allow_low_quality_matches=True is the RPN loss's setting and is not built on the device "
                                      "(the box head's make_roi_box_samp_processor passes False, sampling.py:137-141)")
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = False


class BalancedPositiveNegativeSampler:
    """balanced_positive_negative_sampler.py:10-17: the two numbers veto_box_subsample samples by."""

    def __init__(self, batch_size_per_image, positive_fraction):
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction


def _host_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _check_batch(batch_size_per_image):
    B = int(batch_size_per_image)
    if not 1 <= B <= MAX_BATCH_SIZE_PER_IMAGE:
        raise ValueError("batch_size_per_image %d outside 1..%d (BATCH_SIZE_PER_IMAGE)" % (B, MAX_BATCH_SIZE_PER_IMAGE))
    return B


def box_subsample(labels, n_per_img, batch_size_per_image, positive_fraction, seed=None):
    """veto_box_subsample for a batch: labels int64 [sum n_per_img] on the HIP device (>= 1 positive, 0 negative, anything else
    ignored).  Returns (sampled_inds int64 [n_img, batch_size_per_image], counts int32 [n_img]) on the device: image i keeps the
    proposals sampled_inds[i, :counts[i]], indices inside the image, ascending.  No device->host copy.
    seed: 64-bit; None draws one from torch's default generator, so torch.manual_seed makes a run reproducible."""
    B = _check_batch(batch_size_per_image)
    n_per_img = [int(n) for n in n_per_img]
    if sum(n_per_img) != labels.numel():
        raise ValueError("per-image counts %s do not add up to %d labels" % (n_per_img, labels.numel()))
    if not n_per_img or min(n_per_img) == 0:
        raise ValueError(NO_PROPOSALS)
    device = labels.device
    call = native.Launch(device, "veto_amd subsample runs on a HIP device only")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
    labels = labels.to(dtype=torch.int64).contiguous()
    host_prp = _host_offsets(n_per_img)
    sampled = torch.empty((len(n_per_img), B), dtype=torch.int64, device=device)
    counts = torch.empty(len(n_per_img), dtype=torch.int32, device=device)
    a = call.args(native.VetoBoxSubsampleArgs, n_img=len(n_per_img), n_prp=sum(n_per_img), batch_size_per_image=B,
                  num_pos_per_img=int(B * positive_fraction),   # balanced_positive_negative_sampler.py:41
                  seed=seed & (2 ** 64 - 1), labels=labels, img_prp_offset=native.device_offsets(n_per_img, device=device)[0],
                  img_prp_offset_host=host_prp.ctypes.data, sampled_inds=sampled, counts=counts)
    call.run("veto_box_subsample", ctypes.byref(a))
    return sampled, counts


class FastRCNNSampling(object):
    """sampling.py:14-133 with the reference's constructor, methods, return values and field names."""

    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder):
        if getattr(proposal_matcher, "allow_low_quality_matches", False):
            raise NotImplementedError("allow_low_quality_matches=True is not built on the device")
        self.proposal_matcher = proposal_matcher
        self.fg_bg_sampler = fg_bg_sampler
        self.box_coder = box_coder

    # ---- the one launch the three public methods share ------------------------------------------------------------------
    def _match(self, proposals, targets, mode, want_targets, want_rows, what):
        """veto_box_match for the batch: (matched_idxs, labels, matched_rows or None, regression_targets or None, per-image
        proposal counts), the tensors concatenated over the images."""
        if len(proposals) != len(targets) or not len(proposals):
            raise ValueError("%s needs one target per proposal list (got %d and %d)" % (what, len(proposals), len(targets)))
        n_prp = [len(p) for p in proposals]
        n_tgt = [len(t) for t in targets]
        for p, t in zip(proposals, targets):   # boxlist_iou, boxlist_ops.py:68-70, then Matcher, matcher.py:53-62
            if tuple(p.size) != tuple(t.size):
                raise RuntimeError("boxlists should have same image size, got {}, {}".format(t.size, p.size))
            if len(t) == 0:
                raise ValueError(NO_GT_BOXES)
            if len(p) == 0:
                raise ValueError(NO_PROPOSALS)
        device = proposals[0].bbox.device
        call = native.Launch(device, "veto_amd %s runs on a HIP device only" % what)
        f32 = dict(device=device, dtype=torch.float32)
        i64 = dict(device=device, dtype=torch.int64)
        prp_boxes = torch.cat([p.convert("xyxy").bbox.reshape(-1, 4) for p in proposals]).to(**f32).contiguous()
        tgt_boxes = torch.cat([t.convert("xyxy").bbox.reshape(-1, 4) for t in targets]).to(**f32).contiguous()
        tgt_labels = torch.cat([t.get_field("labels").reshape(-1) for t in targets]).to(**i64).contiguous()
        off = native.device_offsets(n_prp, n_tgt, device=device)
        host_prp, host_tgt = _host_offsets(n_prp), _host_offsets(n_tgt)
        total = sum(n_prp)
        matched = torch.empty(total, **i64)
        labels = torch.empty(total, **i64)
        rows = torch.empty(total, **i64) if want_rows else None
        reg = torch.empty((total, 4), **f32) if want_targets else None
        weights = [float(w) for w in self.box_coder.weights] if want_targets else [1.0] * 4
        a = call.args(native.VetoBoxMatchArgs, n_img=len(n_prp), n_prp=total, n_tgt=sum(n_tgt), mode=mode,
                      high_threshold=float(self.proposal_matcher.high_threshold),
                      low_threshold=float(self.proposal_matcher.low_threshold), reg_weights=(ctypes.c_float * 4)(*weights),
                      prp_boxes=prp_boxes, tgt_boxes=tgt_boxes, tgt_labels=tgt_labels, img_prp_offset=off[0], img_tgt_offset=off[1],
                      img_prp_offset_host=host_prp.ctypes.data, img_tgt_offset_host=host_tgt.ctypes.data, matched_idxs=matched,
                      labels=labels, matched_rows=rows, regression_targets=reg)
        call.run("veto_box_match", ctypes.byref(a))
        return matched, labels, rows, reg, n_prp

    @staticmethod
    def _attributes(targets, matched, rows):
        """sampling.py:59-66 for the batch: the matched boxes' 'attributes', zero where the match is below the low threshold; None
        when the targets do not carry the field."""
        has = [t.has_field("attributes") for t in targets]
        if not all(has):
            if any(has):
                raise ValueError("'attributes' must be on every target or on none")
            return None
        attrs = torch.cat([t.get_field("attributes") for t in targets]).to(dtype=torch.int64)[rows]   # the one batched index
        return attrs * (matched != Matcher.BELOW_LOW_THRESHOLD).reshape((-1,) + (1,) * (attrs.dim() - 1)).to(attrs.dtype)

    # ---- sampling.py:34-45 --------------------------------------------------------------------------------------------
    def match_targets_to_proposals(self, proposal, target):
        """One image: the matched GT boxes as a box list with 'labels' (and 'attributes' when the target has them), taken at
        matched_idxs.clamp(min=0), and the field 'matched_idxs'."""
        matched, _, rows, _, _ = self._match([proposal], [target], 0, False, True, "match_targets_to_proposals")
        out = type(target)(target.bbox[rows], target.size, target.mode)
        out.add_field("labels", target.get_field("labels")[rows])
        if target.has_field("attributes"):
            out.add_field("attributes", target.get_field("attributes")[rows])
        out.add_field("matched_idxs", matched)
        return out

    # ---- sampling.py:47-82 --------------------------------------------------------------------------------------------
    def prepare_targets(self, proposals, targets):
        """(labels, attributes, regression_targets, matched_idxs), one tensor per image each; `attributes` holds None per image
        when the targets carry no such field.  One launch, no device->host copy."""
        return self._prepare(proposals, targets, "prepare_targets")[:4]

    def _prepare(self, proposals, targets, what):
        want_rows = any(t.has_field("attributes") for t in targets)
        matched, labels, rows, reg, n_prp = self._match(proposals, targets, 1, True, want_rows, what)
        attrs = self._attributes(targets, matched, rows) if want_rows else None
        split = (lambda x: list(x.split(n_prp)))
        return (split(labels), split(attrs) if attrs is not None else [None] * len(n_prp), split(reg), split(matched),
                (labels, attrs, reg, matched, n_prp))

    # ---- sampling.py:84-116 -------------------------------------------------------------------------------------------
    def subsample(self, proposals, targets, seed=None):
        """Adds 'labels', 'regression_targets', 'matched_idxs' (and 'attributes') to the proposals and returns, per image, the
        box list of the sampled ones in ascending proposal order, every field gathered.
        seed: 64-bit; None draws one from torch's default generator, so torch.manual_seed makes a run reproducible."""
        B = _check_batch(self.fg_bg_sampler.batch_size_per_image)   # refused here, before the matching is launched
        per_l, per_a, per_r, per_m, (labels, attrs, reg, matched, n_prp) = self._prepare(proposals, targets, "subsample")
        proposals = list(proposals)
        for p, l, at, r, m in zip(proposals, per_l, per_a, per_r, per_m):
            p.add_field("labels", l)
            if at is not None:
                p.add_field("attributes", at)
            p.add_field("regression_targets", r)
            p.add_field("matched_idxs", m)
        sampled, counts = box_subsample(labels, n_prp, B, self.fg_bg_sampler.positive_fraction, seed)
        cnt = counts.tolist()   # the one device->host copy: the per-image counts split the outputs
        glob = sampled + native.device_offsets(n_prp, device=labels.device)[0][:-1, None]   # rows of the concatenated batch
        rows = torch.cat([glob[i, :c] for i, c in enumerate(cnt)])
        made = {"labels": labels, "regression_targets": reg, "matched_idxs": matched}
        if attrs is not None:
            made["attributes"] = attrs
        names = [k for k in proposals[0].fields() if all(p.has_field(k) for p in proposals)]
        picked = {"bbox": torch.cat([p.bbox for p in proposals])[rows].split(cnt)}
        for k in names:   # one batched gather per field
            whole = made[k] if k in made else torch.cat([p.get_field(k) for p in proposals])
            picked[k] = whole[rows].split(cnt)
        out = []
        for i, p in enumerate(proposals):
            q = type(p)(picked["bbox"][i], p.size, p.mode)
            for k in names:
                q.add_field(k, picked[k][i])
            out.append(q)
        return out

    # ---- sampling.py:118-133 ------------------------------------------------------------------------------------------
    def assign_label_to_proposals(self, proposals, targets):
        """Adds 'labels' to every proposal: the label of the matched GT box, 0 where the match is negative.  One launch, no
        device->host copy."""
        _, labels, _, _, n_prp = self._match(proposals, targets, 0, False, False, "assign_label_to_proposals")
        for p, l in zip(proposals, labels.split(n_prp)):
            p.add_field("labels", l)
        return proposals


def make_roi_box_samp_processor(cfg):
    """sampling.py:136-156: the keys it reads."""
    rh = cfg.MODEL.ROI_HEADS
    return FastRCNNSampling(Matcher(rh.FG_IOU_THRESHOLD, rh.BG_IOU_THRESHOLD, allow_low_quality_matches=False),
                            BalancedPositiveNegativeSampler(rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION),
                            BoxCoder(weights=rh.BBOX_REG_WEIGHTS))
