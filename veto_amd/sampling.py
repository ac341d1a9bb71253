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

_OFFSETS = {}     # batch shape -> int32 offset tensor on the device
_WORKSPACE = {}   # (device, stream) -> workspace: launches on different streams never share one


def _prefix_sums(sizes):
    acc, row = 0, [0]
    for v in sizes:
        acc += v
        row.append(acc)
    return row


def _offsets(n_prp, n_tgt, device):
    """[4, n_img + 1] int32 prefix sums of P_i, T_i, T_i^2, P_i^2, cached per batch shape (a pageable H2D copy stalls the
    host behind the queued GPU work, as predictor.cached_offsets notes)."""
    key = (tuple(n_prp), tuple(n_tgt), str(device))
    hit = _OFFSETS.get(key)
    if hit is None:
        if len(_OFFSETS) >= 256:
            _OFFSETS.clear()
        rows = [_prefix_sums(sizes) for sizes in (n_prp, n_tgt, [t * t for t in n_tgt], [p * p for p in n_prp])]
        hit = _OFFSETS[key] = torch.tensor(rows, dtype=torch.int32, device=device)
    return hit


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
        device = proposals[0].bbox.device
        if device.type != "cuda":
            raise RuntimeError("veto_amd detect_relsample runs on a HIP device only (got %s)" % device)
        has_nm = [t.has_field("relation_non_masked") for t in targets]
        if any(has_nm) and not all(has_nm):
            raise ValueError("'relation_non_masked' must be on every target or on none")
        has_nm = all(has_nm)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
        lib = native.load_library()
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
        off = _offsets(n_prp, n_tgt, device)
        pairs = torch.empty((n_img * rows, 2), **i64)
        labels = torch.empty(n_img * rows, **i64)
        labels_all = torch.empty(n_cells * k + n_img * rows, **i64) if has_nm else None
        binary = torch.empty(sum(p * p for p in n_prp), **i64)
        locating = torch.empty(sum(n_prp), **f32)
        counts = torch.empty((n_img, 4), dtype=torch.int32, device=device)
        need = lib.veto_detect_relsample_workspace_bytes(n_cells, k)
        stream = torch.cuda.current_stream(device)
        key = (str(device), stream.cuda_stream)
        ws = _WORKSPACE.get(key)
        if ws is None or ws.numel() < need:
            ws = _WORKSPACE[key] = torch.empty(need, dtype=torch.uint8, device=device)

        a = native.VetoDetectRelsampleArgs()
        a.struct_size = ctypes.sizeof(native.VetoDetectRelsampleArgs)
        a.n_img, a.n_prp, a.n_tgt, a.n_rel_cells = n_img, sum(n_prp), sum(n_tgt), n_cells
        a.max_prp_per_image, a.max_tgt_per_image = max(n_prp), max(n_tgt)
        a.require_overlap, a.num_sample_per_gt_rel = int(self.require_overlap), k
        a.batch_size_per_image, a.max_fg_per_image = B, self.num_pos_per_img
        a.fg_thres, a.seed = self.fg_thres, seed & (2 ** 64 - 1)

        def ptr(t):
            return t.data_ptr() if t is not None and t.numel() else None

        a.prp_boxes, a.prp_labels, a.prp_scores = ptr(prp_boxes), ptr(prp_labels), ptr(prp_scores)
        a.tgt_boxes, a.tgt_labels, a.relation, a.relation_non_masked = ptr(tgt_boxes), ptr(tgt_labels), ptr(relation), ptr(rel_nm)
        a.img_prp_offset, a.img_tgt_offset = off[0].data_ptr(), off[1].data_ptr()
        a.img_rel_offset, a.img_binary_offset = off[2].data_ptr(), off[3].data_ptr()
        a.pairs, a.labels, a.labels_all = pairs.data_ptr(), labels.data_ptr(), ptr(labels_all)
        a.binary_rel, a.locating_match, a.counts = ptr(binary) or pairs.data_ptr(), ptr(locating), counts.data_ptr()
        native.check(lib.veto_detect_relsample(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()),
                                               ws.numel()))
        for t in (prp_boxes, prp_labels, prp_scores, tgt_boxes, tgt_labels, relation, rel_nm, off, ws):
            if t is not None:
                t.record_stream(stream)
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


_GT_OFFSETS = {}  # batch shape -> [2, n_img + 1] int32 offset tensor on the device


def _gt_offsets(n_obj, device):
    """[2, n_img + 1] int32 prefix sums of n_i and n_i^2, cached per batch shape like _offsets."""
    key = (tuple(n_obj), str(device))
    hit = _GT_OFFSETS.get(key)
    if hit is None:
        if len(_GT_OFFSETS) >= 256:
            _GT_OFFSETS.clear()
        rows = [_prefix_sums(sizes) for sizes in (n_obj, [n * n for n in n_obj])]
        hit = _GT_OFFSETS[key] = torch.tensor(rows, dtype=torch.int32, device=device)
    return hit


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
        if device.type != "cuda":
            raise RuntimeError("veto_amd gtbox_relsample runs on a HIP device only (got %s)" % device)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # the CPU generator: no device synchronisation
        lib = native.load_library()
        n_img, B = len(proposals), self.batch_size_per_image
        n_cells = sum(n * n for n in n_obj)
        i64 = dict(device=device, dtype=torch.int64)
        parts = [t.get_field("relation").reshape(-1).to(**i64) for t in targets]
        relation = torch.cat(parts).contiguous()
        off = _gt_offsets(n_obj, device)
        pairs = torch.empty((n_img * B, 2), **i64)
        labels = torch.empty(n_img * B, **i64)
        binary = torch.empty(n_cells, **i64)
        counts = torch.empty((n_img, 2), dtype=torch.int32, device=device)
        stream = torch.cuda.current_stream(device)

        a = native.VetoGtboxRelsampleArgs()
        a.struct_size = ctypes.sizeof(native.VetoGtboxRelsampleArgs)
        a.n_img, a.n_rel_cells, a.max_obj_per_image = n_img, n_cells, max(n_obj)
        a.batch_size_per_image, a.num_pos_per_img = B, self.num_pos_per_img
        a.seed = seed & (2 ** 64 - 1)
        a.relation = relation.data_ptr() if n_cells else None
        a.img_obj_offset, a.img_rel_offset = off[0].data_ptr(), off[1].data_ptr()
        a.pairs, a.labels, a.counts = pairs.data_ptr(), labels.data_ptr(), counts.data_ptr()
        a.binary_rel = binary.data_ptr() if n_cells else None
        native.check(lib.veto_gtbox_relsample(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a)))
        relation.record_stream(stream)
        off.record_stream(stream)
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
