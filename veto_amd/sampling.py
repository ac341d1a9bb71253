"""Training-time relation sampling, the caller side of veto_detect_relsample (sgdet) and veto_gtbox_relsample (predcls, sgcls).

`RelationSampling` has the reference's interface (sampling.py:13-309) and delegates each method to the device path:
prepare_test_pairs -> pairs.prepare_test_pairs, gtbox_relsample -> GTBoxRelationSampler, detect_relsample ->
DetectRelationSampler.

`GTBoxRelationSampler.gtbox_relsample` mirrors `RelationSampling.gtbox_relsample` (sampling.py:54-107): one launch for the
batch picks the foreground rows (all of them in torch.nonzero order, or a random subset above the positive budget), the random
background rows and `binary_rel`.  The only device->host copy is the batch's per-image counts.

`DetectRelationSampler.detect_relsample` mirrors `RelationSampling.detect_relsample`
(pysgg/modeling/roi_heads/relation_head/sampling.py:109-176) with `motif_rel_fg_bg_sampling` (:179-309): one launch for the
batch does the IoU matching, the per-GT-relation foreground draws, the foreground cap, the background window and its
random subset, `binary_rel` and `locating_match` (see include/veto_amd.h).  The draws have the reference's distributions;
they are not the reference's draws for a given seed (it mixes numpy's and torch's generators).  The only device->host copy
is the batch's per-image counts, which decide how the outputs are split.  The same holds for the GT-box sampler: its subsets
and orders are uniform like torch.randperm's, from a counter-based hash instead of torch's generator."""
import ctypes

import torch

from . import native

class DetectRelationSampler:
    def __init__(self, fg_thres, require_overlap, num_sample_per_gt_rel, batch_size_per_image, positive_fraction):
        self.fg_thres = float(fg_thres)
        self.require_overlap = bool(require_overlap)
        self.num_sample_per_gt_rel = int(num_sample_per_gt_rel)
        self.batch_size_per_image = int(batch_size_per_image)
        self.positive_fraction = float(positive_fraction)
        self.num_pos_per_img = int(self.batch_size_per_image * self.positive_fraction)   # sampling.py:120

    @classmethod
    def from_config(cls, cfg):
        """The arguments make_roi_relation_samp_processor (sampling.py:312-323) passes for detect_relsample."""
        rh = cfg.MODEL.ROI_RELATION_HEAD
        return cls(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, rh.REQUIRE_BOX_OVERLAP, rh.NUM_SAMPLE_PER_GT_REL,
                   rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION)

    def detect_relsample(self, proposals, targets, seed=None):
        """proposals: BoxLists with 'labels' and 'pred_scores'; targets: BoxLists with 'labels', 'relation' [T, T] and
        optionally 'relation_non_masked' (all targets or none).  Adds 'locating_match' to every proposal and returns
        (proposals, rel_labels, rel_labels_all, rel_pair_idxs, rel_sym_binarys) as the reference does.
        seed: 64-bit; None draws one from torch's default generator, so torch.manual_seed makes a run reproducible."""
        if len(proposals) != len(targets) or not proposals:
            raise ValueError("detect_relsample needs one target per proposal list (got %d and %d)" % (len(proposals), len(targets)))
        has_nm = [t.has_field("relation_non_masked") for t in targets]
        if any(has_nm) and not all(has_nm):
            raise ValueError("'relation_non_masked' must be on every target or on none")
        has_nm = all(has_nm)
        device = proposals[0].bbox.device
        call = native.Launch(device, "veto_amd detect_relsample runs on a HIP device only")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
        n_prp = [len(p) for p in proposals]
        n_tgt = [len(t) for t in targets]
        n_img, k, B = len(proposals), self.num_sample_per_gt_rel, self.batch_size_per_image
        rows = max(B, 2)
        n_cells = sum(t * t for t in n_tgt)
        f32 = dict(device=device, dtype=torch.float32)
        i64 = dict(device=device, dtype=torch.int64)

        def cat(parts, **kw):
            parts = [x.reshape(-1).to(**kw) for x in parts]
            return torch.cat(parts).contiguous() if parts else torch.empty(0, **kw)

        prp_boxes = cat([p.convert("xyxy").bbox for p in proposals], **f32)
        prp_labels = cat([p.get_field("labels") for p in proposals], **i64)
        prp_scores = cat([p.get_field("pred_scores") for p in proposals], **f32)
        tgt_boxes = cat([t.convert("xyxy").bbox for t in targets], **f32)
        tgt_labels = cat([t.get_field("labels") for t in targets], **i64)
        relation = cat([t.get_field("relation") for t in targets], **i64)
        rel_nm = cat([t.get_field("relation_non_masked") for t in targets], **i64) if has_nm else None
        for t, n in zip(targets, n_tgt):
            if tuple(t.get_field("relation").shape) != (n, n):
                raise ValueError("a target's 'relation' must be [%d, %d], got %s" % (n, n, tuple(t.get_field("relation").shape)))
            if has_nm and tuple(t.get_field("relation_non_masked").shape) != (n, n):
                raise ValueError("a target's 'relation_non_masked' must be [%d, %d]" % (n, n))
        # prefix sums of P_i, T_i, T_i^2, P_i^2
        off = native.device_offsets(n_prp, n_tgt, [t * t for t in n_tgt], [p * p for p in n_prp], device=device)
        pairs = torch.empty((n_img * rows, 2), **i64)
        labels = torch.empty(n_img * rows, **i64)
        labels_all = torch.empty(n_cells * k + n_img * rows, **i64) if has_nm else None
        binary = torch.empty(sum(p * p for p in n_prp), **i64)
        locating = torch.empty(sum(n_prp), **f32)
        counts = torch.empty((n_img, 4), dtype=torch.int32, device=device)
        a = call.args(native.VetoDetectRelsampleArgs, n_img=n_img, n_prp=sum(n_prp), n_tgt=sum(n_tgt), n_rel_cells=n_cells,
                      max_prp_per_image=max(n_prp), max_tgt_per_image=max(n_tgt), require_overlap=int(self.require_overlap),
                      num_sample_per_gt_rel=k, batch_size_per_image=B, max_fg_per_image=self.num_pos_per_img,
                      fg_thres=self.fg_thres, seed=seed & (2 ** 64 - 1), prp_boxes=prp_boxes, prp_labels=prp_labels,
                      prp_scores=prp_scores, tgt_boxes=tgt_boxes, tgt_labels=tgt_labels, relation=relation,
                      relation_non_masked=rel_nm, img_prp_offset=off[0], img_tgt_offset=off[1], img_rel_offset=off[2],
                      img_binary_offset=off[3], pairs=pairs, labels=labels, labels_all=labels_all,
                      binary_rel=binary if binary.numel() else pairs, locating_match=locating, counts=counts)
        ws = call.workspace(call.lib.veto_detect_relsample_workspace_bytes(n_cells, k))
        call.run("veto_detect_relsample", ctypes.byref(a), ws.data_ptr(), ws.numel())
        cnt = counts.tolist()   # the one device->host copy: the per-image counts split the outputs
        bad = [i for i, c in enumerate(cnt) if c[3] & 1]
        if bad:
            raise IndexError("detect_relsample: relation_non_masked has fewer nonzero entries than the relation index of a "
                             "foreground triplet (images %s; sampling.py:162 indexes nonzero(relation_non_masked))" % bad)
        rel_labels, rel_labels_all, rel_pair_idxs, rel_sym_binarys = [], [], [], []
        boff = loff = poff = 0
        for i, (p, n, t) in enumerate(zip(proposals, n_prp, n_tgt)):
            r, f_all, n_fg, _ = cnt[i]
            rel_pair_idxs.append(pairs[i * rows:i * rows + r])
            rel_labels.append(labels[i * rows:i * rows + r])
            if has_nm:
                start = loff * k + i * rows
                rel_labels_all.append(labels_all[start:start + f_all + r - n_fg])
            rel_sym_binarys.append(binary[boff:boff + n * n].view(n, n))
            p.add_field("locating_match", locating[poff:poff + n])
            boff, loff, poff = boff + n * n, loff + t * t, poff + n
        if not has_nm:
            rel_labels_all = rel_labels   # sampling.py:173-174
        return proposals, rel_labels, rel_labels_all, rel_pair_idxs, rel_sym_binarys


class GTBoxRelationSampler:
    def __init__(self, batch_size_per_image, positive_fraction):
        self.batch_size_per_image = int(batch_size_per_image)
        self.positive_fraction = float(positive_fraction)
        self.num_pos_per_img = int(self.batch_size_per_image * self.positive_fraction)   # sampling.py:56

    @classmethod
    def from_config(cls, cfg):
        rh = cfg.MODEL.ROI_RELATION_HEAD
        return cls(rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION)

    def gtbox_relsample(self, proposals, targets, seed=None):
        """proposals: BoxLists of the GT boxes; targets: BoxLists with 'relation' [n, n].  Adds 'locating_match' (ones,
        sampling.py:71-73) to every proposal and returns (proposals, rel_labels, rel_idx_pairs, rel_sym_binarys) as the
        reference does.  seed: 64-bit; None draws one from torch's default generator, so torch.manual_seed makes a run
        reproducible."""
        if len(proposals) != len(targets) or not proposals:
            raise ValueError("gtbox_relsample needs one target per proposal list (got %d and %d)" % (len(proposals), len(targets)))
        n_obj = [len(p) for p in proposals]
        for i, (n, t) in enumerate(zip(n_obj, targets)):
            if len(t) != n:
                raise ValueError("image %d: %d proposals but %d targets (GT-box sampling pairs them one to one, "
                                 "sampling.py:66)" % (i, n, len(t)))
            if tuple(t.get_field("relation").shape) != (n, n):
                raise ValueError("a target's 'relation' must be [%d, %d], got %s" % (n, n, tuple(t.get_field("relation").shape)))
        device = proposals[0].bbox.device
        call = native.Launch(device, "veto_amd gtbox_relsample runs on a HIP device only")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
        n_img, B = len(proposals), self.batch_size_per_image
        n_cells = sum(n * n for n in n_obj)
        i64 = dict(device=device, dtype=torch.int64)
        parts = [t.get_field("relation").reshape(-1).to(**i64) for t in targets]
        relation = torch.cat(parts).contiguous()
        off = native.device_offsets(n_obj, [n * n for n in n_obj], device=device)
        pairs = torch.empty((n_img * B, 2), **i64)
        labels = torch.empty(n_img * B, **i64)
        binary = torch.empty(n_cells, **i64)
        counts = torch.empty((n_img, 2), dtype=torch.int32, device=device)
        a = call.args(native.VetoGtboxRelsampleArgs, n_img=n_img, n_rel_cells=n_cells, max_obj_per_image=max(n_obj),
                      batch_size_per_image=B, num_pos_per_img=self.num_pos_per_img, seed=seed & (2 ** 64 - 1), relation=relation,
                      img_obj_offset=off[0], img_rel_offset=off[1], pairs=pairs, labels=labels, binary_rel=binary, counts=counts)
        call.run("veto_gtbox_relsample", ctypes.byref(a))
        cnt = counts.tolist()   # the one device->host copy: the per-image counts split the outputs
        ones = torch.ones(sum(n_obj), device=device)
        rel_labels, rel_idx_pairs, rel_sym_binarys = [], [], []
        boff = ooff = 0
        for i, (p, n) in enumerate(zip(proposals, n_obj)):
            r = cnt[i][0] + cnt[i][1]
            rel_idx_pairs.append(pairs[i * B:i * B + r])
            rel_labels.append(labels[i * B:i * B + r])
            rel_sym_binarys.append(binary[boff:boff + n * n].view(n, n))
            p.add_field("locating_match", ones[ooff:ooff + n])
            boff, ooff = boff + n * n, ooff + n
        return proposals, rel_labels, rel_idx_pairs, rel_sym_binarys


class RelationSampling(object):
    """The reference's sampler interface (sampling.py:13-29) on the device paths of this package."""

    def __init__(self, fg_thres, require_overlap, num_sample_per_gt_rel, batch_size_per_image, positive_fraction, max_proposal_pairs,
                 use_gt_box, test_overlap):
        self.fg_thres = fg_thres
        self.require_overlap = require_overlap
        self.num_sample_per_gt_rel = num_sample_per_gt_rel
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.use_gt_box = use_gt_box
        self.max_proposal_pairs = max_proposal_pairs
        self.test_overlap = test_overlap
        self._gtbox = GTBoxRelationSampler(batch_size_per_image, positive_fraction)
        self._detect = DetectRelationSampler(fg_thres, require_overlap, num_sample_per_gt_rel, batch_size_per_image, positive_fraction)

    def prepare_test_pairs(self, device, proposals):
        from .pairs import prepare_test_pairs
        return prepare_test_pairs(device, proposals, self.max_proposal_pairs,
                                  require_overlap=bool(self.test_overlap) and not self.use_gt_box, use_gt_box=bool(self.use_gt_box))

    def gtbox_relsample(self, proposals, targets):
        assert self.use_gt_box
        return self._gtbox.gtbox_relsample(proposals, targets)

    def detect_relsample(self, proposals, targets):
        return self._detect.detect_relsample(proposals, targets)


def make_roi_relation_samp_processor(cfg):
    """sampling.py:312-324."""
    rh = cfg.MODEL.ROI_RELATION_HEAD
    return RelationSampling(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, rh.REQUIRE_BOX_OVERLAP, rh.NUM_SAMPLE_PER_GT_REL,
                            rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION, rh.MAX_PROPOSAL_PAIR, rh.USE_GT_BOX,
                            cfg.TEST.RELATION.REQUIRE_OVERLAP)
