"""The RPN's proposal selection (pysgg/modeling/rpn/inference.py:13-210) on the HIP device.

`rpn_proposals` runs veto_rpn_proposals once per batch: per image and pyramid level the top-k of the objectness logits,
BoxCoder.decode of the selected anchors, clipping, the small-box filter and NMS, then the merge over the levels -- three
launches (four in per-batch mode) whatever the number of images or levels, reading the RPN head's NCHW outputs in place.  The
per-image counts are read back once (the only device->host copy) to split the outputs.  `RPNPostProcessor` wraps it in the
reference's constructor and forward contract; it has no backward (the reference's proposals carry no gradient either).

`AnchorGenerator` (pysgg/modeling/rpn/anchor_generator.py:34-166) feeds it: veto_anchor_grid writes the anchors of every level
and the visibility plane of every image in one launch, and the anchors are cached per grid shape."""
import collections
import ctypes
import math

import torch
from torch import nn

from . import native
from .boxhead import BoxCoder, _image_sizes
from .synth import _cell_anchors


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


ANCHOR_CACHE_SIZE = 4   # grid shapes an AnchorGenerator keeps anchors for (a training loop sees a handful of padded batch shapes)


class BufferList(nn.Module):
    """anchor_generator.py:11-31: buffers named "0", "1", ... (the state dict's `cell_anchors.0` ...)."""

    def __init__(self, buffers=None):
        super().__init__()
        if buffers is not None:
            self.extend(buffers)

    def extend(self, buffers):
        offset = len(self)
        for i, buffer in enumerate(buffers):
            self.register_buffer(str(offset + i), buffer)
        return self

    def __len__(self):
        return len(self._buffers)

    def __iter__(self):
        return iter(self._buffers.values())


def _boxlist_class():
    try:
        from pysgg.structures.bounding_box import BoxList  # type: ignore
    except Exception:     # not installed / its own imports fail outside the host code base
        from .structures import BoxList
    return BoxList


def generate_anchors(stride=16, sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1, 2)):
    """anchor_generator.py:220-289: the [len(aspect_ratios) * len(sizes), 4] float64 cell anchors, ratio-major (host)."""
    return torch.from_numpy(_cell_anchors(stride, sizes, aspect_ratios))


def _anchor_call(device, levels, cells, *, anchors=None, anchors_in=None, image_sizes=None, straddle_thresh=0, visibility=None):
    """One veto_anchor_grid call.  levels: (A, H, W, stride) per level; image_sizes: (width, height) per image."""
    call = native.Launch(device, "veto_amd AnchorGenerator runs on a HIP device only")
    n_img = 0 if visibility is None else len(image_sizes)
    sizes = None
    if visibility is not None and straddle_thresh >= 0:
        sizes = _image_sizes([(float(w), float(h)) for w, h in image_sizes], device)
    a = call.args(native.VetoAnchorArgs, n_img=n_img, n_lvl=len(levels), straddle_thresh=float(straddle_thresh), image_sizes=sizes,
                  anchors=anchors, anchors_in=anchors_in, visibility=visibility)
    for l, (A, H, W, stride) in enumerate(levels[:native.RPN_MAX_LEVELS]):   # (more levels: the call refuses n_lvl)
        a.level_a[l], a.level_h[l], a.level_w[l], a.level_stride[l] = A, H, W, stride
        if cells is not None:
            a.cell_anchors[l] = call.ptr(cells[l])
    call.run("veto_anchor_grid", ctypes.byref(a))


class AnchorGenerator(nn.Module):
    """anchor_generator.py:34-125 with the reference's constructor, attributes, methods and state dict, on the HIP device.

    forward makes one veto_anchor_grid launch: the anchors of all levels go into one buffer, the visibility of all images into one
    byte plane, and the BoxLists hold views of the two.  The anchor buffer is cached per (device, grid sizes, current stream), the
    ANCHOR_CACHE_SIZE most recently used of them (per stream, because the buffer is written on the stream of its miss and nothing
    would order a hit on another stream behind that write); a forward that finds its shape writes the visibility plane only.  The cached
    tensors are handed out as they are, to every image and every call: they must not be written in place (the reference shares
    one tensor among the images of a batch in the same way).  Moving the module or changing a cell_anchors buffer empties the cache."""

    def __init__(self, sizes=(128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(8, 16, 32), straddle_thresh=0):
        super().__init__()
        if len(anchor_strides) == 1:
            cell_anchors = [generate_anchors(anchor_strides[0], sizes, aspect_ratios).float()]
        else:
            if len(anchor_strides) != len(sizes):
                raise RuntimeError("FPN should have #anchor_strides == #sizes")
            cell_anchors = [generate_anchors(anchor_stride, size if isinstance(size, (tuple, list)) else (size,), aspect_ratios).float()
                            for anchor_stride, size in zip(anchor_strides, sizes)]
        self.strides = anchor_strides
        self.cell_anchors = BufferList(cell_anchors)
        self.straddle_thresh = straddle_thresh
        self._boxlist = _boxlist_class()
        self._cache = collections.OrderedDict()   # (device, grid sizes, stream) -> (buffer [total, 4], its per-level views)
        self._cache_of = None                     # the cell_anchors buffers the cache was computed from

    def num_anchors_per_location(self):
        return [len(cell_anchors) for cell_anchors in self.cell_anchors]

    def _apply(self, fn, *args, **kwargs):
        self._cache.clear()
        return super()._apply(fn, *args, **kwargs)

    def _levels(self, grid_sizes):
        """((A, H, W, stride) per level, the cell anchors): as many levels as the shortest of the three lists (the reference zips)."""
        cells = list(self.cell_anchors)
        levels = tuple((len(c), int(h), int(w), int(s)) for (h, w), s, c in zip(grid_sizes, self.strides, cells))
        return levels, cells[:len(levels)]

    def _cached(self, levels, cells):
        """(buffer, views, hit?) of these levels; on a miss the buffer is allocated and not yet written."""
        stamp = tuple((c.data_ptr(), c._version, str(c.device), c.dtype) for c in cells)
        if stamp != self._cache_of:
            self._cache.clear()
            self._cache_of = stamp
        # the stream is part of the key: a buffer is written on the stream of its miss, and a hit on another stream would read it
        # with nothing ordering the two
        key = (str(cells[0].device), tuple((h, w) for _, h, w, _ in levels), torch.cuda.current_stream(cells[0].device).cuda_stream)
        hit = self._cache.get(key)
        if hit is not None:
            self._cache.move_to_end(key)
            return hit[0], hit[1], True
        rows = [A * H * W for A, H, W, _ in levels]
        buf = torch.empty((sum(rows), 4), dtype=torch.float32, device=cells[0].device)
        views = list(buf.split(rows, 0))
        self._cache[key] = (buf, views)
        while len(self._cache) > ANCHOR_CACHE_SIZE:
            self._cache.popitem(last=False)
        return buf, views, False

    def _check(self, levels, cells):
        if not levels:
            raise ValueError("AnchorGenerator: no pyramid level (grid sizes, strides or cell anchors are empty)")
        for c in cells:
            if c.dtype != torch.float32 or not c.is_contiguous():
                raise TypeError("cell_anchors must be contiguous float32 buffers, got %s" % (c.dtype,))

    def grid_anchors(self, grid_sizes):
        """The [A H W, 4] anchors of every level, on the cell anchors' device: views of one cached buffer (one launch when the
        grid sizes are new, none otherwise)."""
        levels, cells = self._levels(grid_sizes)
        self._check(levels, cells)
        native.Launch(cells[0].device, "veto_amd AnchorGenerator runs on a HIP device only")
        buf, views, hit = self._cached(levels, cells)
        if not hit:
            try:
                _anchor_call(buf.device, levels, cells, anchors=buf)
            except Exception:
                self._cache.clear()
                raise
        return list(views)

    def add_visibility_to(self, boxlist):
        """Adds the field 'visibility' to one BoxList (one launch): bool for straddle_thresh >= 0, uint8 ones below."""
        image_width, image_height = boxlist.size
        anchors = boxlist.bbox
        native.Launch(anchors.device, "veto_amd AnchorGenerator runs on a HIP device only")
        rows = anchors.to(torch.float32).reshape(-1, 4).contiguous()
        if rows.data_ptr() % 16:
            rows = rows.clone()
        vis = torch.empty(len(rows), dtype=torch.uint8, device=anchors.device)
        if len(rows):
            _anchor_call(anchors.device, ((len(rows), 1, 1, 1),), None, anchors_in=rows, image_sizes=[(image_width, image_height)],
                         straddle_thresh=self.straddle_thresh, visibility=vis)
        boxlist.add_field("visibility", vis.view(torch.bool) if self.straddle_thresh >= 0 else vis)

    def forward(self, image_list, feature_maps):
        """image_list.image_sizes: (height, width) per image; feature_maps: one [N, C, H, W] tensor per level, on the HIP device.
        Returns list[list[BoxList]], image-major, mode xyxy, size (width, height), with the field 'visibility'; the BoxLists of
        all images share each level's (cached, read-only) anchor tensor and the visibility fields are views of one plane."""
        device = feature_maps[0].device
        native.Launch(device, "veto_amd AnchorGenerator runs on a HIP device only")
        levels, cells = self._levels([feature_map.shape[-2:] for feature_map in feature_maps])
        self._check(levels, cells)
        if cells[0].device != device:
            raise RuntimeError("AnchorGenerator: cell_anchors are on %s, the feature maps on %s (move the module with .to())"
                               % (cells[0].device, device))
        image_sizes = [(image_width, image_height) for image_height, image_width in image_list.image_sizes]
        if not image_sizes:
            return []
        buf, views, hit = self._cached(levels, cells)
        plane = torch.empty((len(image_sizes), len(buf)), dtype=torch.uint8, device=device)
        try:
            _anchor_call(device, levels, None if hit else cells, anchors=None if hit else buf, anchors_in=buf, image_sizes=image_sizes,
                         straddle_thresh=self.straddle_thresh, visibility=plane)
        except Exception:
            if not hit:
                self._cache.clear()
            raise
        if self.straddle_thresh >= 0:
            plane = plane.view(torch.bool)
        rows = [len(v) for v in views]
        anchors = []
        for size, visible in zip(image_sizes, plane.unbind(0)):
            anchors_in_image = []
            for level_anchors, level_visible in zip(views, visible.split(rows, 0)):
                boxlist = self._boxlist(level_anchors, size, mode="xyxy")
                boxlist.add_field("visibility", level_visible)
                anchors_in_image.append(boxlist)
            anchors.append(anchors_in_image)
        return anchors


def make_anchor_generator(config):
    """anchor_generator.py:128-143: the keys it reads and its asserts."""
    anchor_sizes = config.MODEL.RPN.ANCHOR_SIZES
    aspect_ratios = config.MODEL.RPN.ASPECT_RATIOS
    anchor_stride = config.MODEL.RPN.ANCHOR_STRIDE
    straddle_thresh = config.MODEL.RPN.STRADDLE_THRESH
    if config.MODEL.RPN.USE_FPN:
        assert len(anchor_stride) == len(anchor_sizes), "FPN should have len(ANCHOR_STRIDE) == len(ANCHOR_SIZES)"
    else:
        assert len(anchor_stride) == 1, "Non-FPN should have a single ANCHOR_STRIDE"
    return AnchorGenerator(anchor_sizes, aspect_ratios, anchor_stride, straddle_thresh)


def make_anchor_generator_retinanet(config):
    """anchor_generator.py:146-166: per level SCALES_PER_OCTAVE sizes, OCTAVE ** (i / SCALES_PER_OCTAVE) apart."""
    anchor_sizes = config.MODEL.RETINANET.ANCHOR_SIZES
    aspect_ratios = config.MODEL.RETINANET.ASPECT_RATIOS
    anchor_strides = config.MODEL.RETINANET.ANCHOR_STRIDES
    straddle_thresh = config.MODEL.RETINANET.STRADDLE_THRESH
    octave = config.MODEL.RETINANET.OCTAVE
    scales_per_octave = config.MODEL.RETINANET.SCALES_PER_OCTAVE
    assert len(anchor_strides) == len(anchor_sizes), "Only support FPN now"
    new_anchor_sizes = []
    for size in anchor_sizes:
        new_anchor_sizes.append(tuple(octave ** (i / float(scales_per_octave)) * size for i in range(scales_per_octave)))
    return AnchorGenerator(tuple(new_anchor_sizes), aspect_ratios, anchor_strides, straddle_thresh)
