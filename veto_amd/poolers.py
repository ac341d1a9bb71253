"""MI355X-native ROI feature extraction for the VETO relation head.

Host-side mirror of the reference's
  * `ROIAlign` module          pysgg/layers/roi_align.py:49-68
  * `LevelMapper`, `Pooler`    pysgg/modeling/poolers.py:12-171 (cat_all_levels=False, the way VETO builds it:
                               relation_head.py:53)
  * `VETOFeatureExtractor`     pysgg/modeling/roi_heads/box_head/roi_box_feature_extractors.py:75-121
with the same constructor arguments, call signatures and return values.  All arithmetic runs in
libveto_amd.so (veto_roi_pool; veto_roi_pool_adaptive for sampling_ratio 0, the reference's default, whose grid is
chosen per ROI): one launch pools every ROI from its own FPN level and the depth map with the fixed 1/16 pooler; dense NCHW or channels_last maps of float32, float16 or bfloat16 are read in place (anything else is
first copied to float32 NCHW), and their gradients come back in the leaf's dtype and memory format; differentiable w.r.t. the maps (veto_roi_pool_backward, the atomic-add scatter of
ROIAlign_cuda.cu:178-262).  Union pooling
(7x7, Pooler.forward(union=True)) and cat_all_levels=True are not used by VETO and raise."""
import ctypes
import math

import torch
from torch import nn

from . import native


def _pool_args(call, feats, scales, rois, n_img, pooled, sampling_ratio, depth_shape, **pointers):
    """feats: per level the map or its shape (the backward has only the shapes)."""
    shapes = [tuple(getattr(f, "shape", f)) for f in feats]
    a = call.args(native.VetoRoiPoolArgs, n_levels=len(shapes), n_img=n_img, n_roi=rois.shape[0], channels=shapes[0][1], pooled=pooled,
                  sampling_ratio=sampling_ratio, rois=rois, **pointers)
    for l, (f, shape, sc) in enumerate(zip(feats, shapes, scales)):
        a.level_h[l], a.level_w[l], a.level_scale[l] = shape[2], shape[3], float(sc)
        if isinstance(f, torch.Tensor):
            a.level_feat[l] = call.ptr(f)
    if depth_shape is not None:
        a.depth_channels, a.depth_h, a.depth_w = depth_shape[1], depth_shape[2], depth_shape[3]
    return a


_DTYPE_CODES = {torch.float32: native.VETO_ROI_F32, torch.float16: native.VETO_ROI_F16, torch.bfloat16: native.VETO_ROI_BF16}
_NCHW, _NHWC = native.VETO_ROI_NCHW, native.VETO_ROI_NHWC
# Which map forms (dtype code, layout code) each entry point takes in place; every other form goes through the float32 NCHW copy.
# Decided per form by measurement against copy-then-pool (profiles/roi_layouts.txt states the times and what follows from them).
IN_PLACE = {
    "forward": {(d, l) for d in _DTYPE_CODES.values() for l in (_NCHW, _NHWC)},
    "backward": {_NCHW, _NHWC},            # the gradient maps' layout (they are float32 whatever the maps were)
    "backward_ordered": {_NCHW, _NHWC},
    # the adaptive grid (sampling_ratio 0, veto_roi_pool_adaptive): NCHW maps of the three dtypes in place; channels_last maps take the
    # float32 NCHW copy (the same bits), and their gradients go back through autograd's own conversion.  No ordered backward.
    "adaptive_forward": {(d, _NCHW) for d in _DTYPE_CODES.values()},
    "adaptive_backward": {_NCHW},
}
_ADAPTIVE_ORDERED = ("veto_amd ROI pooling: sampling_ratio = 0 (the adaptive grid) has no ordered backward, and the ordered mode "
                     "(VETO_AMD.DETERMINISTIC, torch.use_deterministic_algorithms(True) or VETO_DETERMINISTIC=1) is on; it does not "
                     "fall back to atomic adds.  Use POOLER_SAMPLING_RATIO 1-4, which veto_roi_pool_backward_ordered supports, or "
                     "switch the ordered mode off")


def _map_form(maps):
    """(dtype code, layout code) when every map of the group is dense in one and the same memory format and of one dtype the
    kernels read; None otherwise (strided views, mixed formats, float64, ...).  Where both formats hold (C == 1 or
    H == W == 1) this is NCHW."""
    code = _DTYPE_CODES.get(maps[0].dtype)
    if code is None or any(m.dtype != maps[0].dtype or m.dim() != 4 for m in maps):
        return None
    if all(m.is_contiguous() for m in maps):
        return code, _NCHW
    if all(m.is_contiguous(memory_format=torch.channels_last) for m in maps):
        return code, _NHWC
    return None


def _in_place(maps, device, key="forward"):
    """(the maps as the call reads them, (dtype code, layout code)): in place when their form is dispatched that way (IN_PLACE[key]),
    else the dense float32 NCHW copies."""
    form = _map_form(maps)
    if form is not None and form in IN_PLACE[key] and all(m.device == device for m in maps):
        return [m.detach() for m in maps], form
    return [m.detach().to(device=device, dtype=torch.float32).contiguous() for m in maps], (native.VETO_ROI_F32, _NCHW)


def _roi_pool(level_feats, scales, rois, n_img, pooled, sampling_ratio, depth=None, want_levels=False):
    device = rois.device
    call = native.Launch(device, "veto_amd ROI pooling runs only on a HIP device")
    f32 = dict(device=device, dtype=torch.float32)
    adaptive = sampling_ratio == 0      # the grid chosen per ROI: entry points of its own
    key = "adaptive_forward" if adaptive else "forward"
    feats, (level_dtype, level_layout) = _in_place(list(level_feats), device, key)
    rois = rois.detach().to(**f32).contiguous()
    n_roi, C = rois.shape[0], feats[0].shape[1]
    for l, f in enumerate(feats):
        if f.shape[0] != n_img or f.shape[1] != C:
            raise ValueError("pyramid level %d has shape %s, expected [%d, %d, H, W]" % (l, tuple(f.shape), n_img, C))
    depth_dtype, depth_layout = native.VETO_ROI_F32, _NCHW
    if depth is not None:
        (depth,), (depth_dtype, depth_layout) = _in_place([depth], device, key)
    out_rgb = torch.empty((n_roi, C, pooled, pooled), **f32)
    out_depth = None
    if depth is not None:
        out_depth = torch.empty((n_roi, depth.shape[1], pooled, pooled), **f32)
    levels = torch.empty(n_roi, dtype=torch.int32, device=device) if want_levels else None
    a = _pool_args(call, feats, scales, rois, n_img, pooled, sampling_ratio, tuple(depth.shape) if depth is not None else None,
                   depth_feat=depth, out_rgb=out_rgb, out_depth=out_depth, out_levels=levels, level_dtype=level_dtype,
                   level_layout=level_layout, depth_dtype=depth_dtype, depth_layout=depth_layout)
    call.run("veto_roi_pool_adaptive" if adaptive else "veto_roi_pool", ctypes.byref(a))
    return out_rgb, out_depth, levels


def _roi_pool_backward(shapes, scales, rois, n_img, pooled, sampling_ratio, grad_rgb, depth_shape, grad_depth, ordered=False,
                       level_layout=_NCHW, depth_layout=_NCHW):
    """Map gradients of one veto_roi_pool call: (list of per-level gradients, depth gradient or None), float32 and dense in
    level_layout / depth_layout (NHWC: torch.channels_last).  ordered: through veto_roi_pool_backward_ordered, which fixes the
    summation order and writes every element itself.  sampling_ratio 0: veto_roi_pool_adaptive_backward (atomic, NCHW only)."""
    if sampling_ratio == 0 and ordered:
        raise NotImplementedError(_ADAPTIVE_ORDERED)
    device = rois.device
    call = native.Launch(device, "veto_amd ROI pooling runs only on a HIP device")
    f32 = dict(device=device, dtype=torch.float32)
    rois = rois.detach().to(**f32).contiguous()
    a = _pool_args(call, shapes, scales, rois, n_img, pooled, sampling_ratio, depth_shape if grad_depth is not None else None,
                   level_layout=level_layout, depth_layout=depth_layout)
    grad_rgb = grad_rgb.detach().to(**f32).contiguous()
    formats = {_NCHW: torch.contiguous_format, _NHWC: torch.channels_last}

    def make(shape, memory_format):      # (torch.zeros takes no memory_format)
        g = torch.empty(shape, memory_format=memory_format, **f32)
        return g if ordered else g.zero_()

    level_grads = [make(shape, memory_format=formats[level_layout]) for shape in shapes]
    ptrs = (ctypes.c_void_p * 4)(*[g.data_ptr() for g in level_grads])
    depth_grad = None
    if grad_depth is not None:
        grad_depth = grad_depth.detach().to(**f32).contiguous()
        depth_grad = make(depth_shape, memory_format=formats[depth_layout])
    entry = "veto_roi_pool_adaptive_backward" if sampling_ratio == 0 else "veto_roi_pool_backward_ordered" if ordered else "veto_roi_pool_backward"
    call.run(entry, ctypes.byref(a), call.ptr(grad_rgb), call.ptr(grad_depth), ptrs, call.ptr(depth_grad))
    return level_grads, depth_grad


_TORCH_DTYPES = {code: dtype for dtype, code in _DTYPE_CODES.items()}


def _as_leaf(grad, form):
    """The float32 gradient in its leaf's dtype and memory format: one cast in torch (a no-op for a float32 gradient that is
    already in the leaf's layout).  form None: the leaf went through the conversion path and autograd does the rest, as before."""
    if grad is None or form is None:
        return grad
    return grad.to(dtype=_TORCH_DTYPES[form[0]], memory_format=torch.channels_last if form[1] == _NHWC else torch.contiguous_format)


class _RoiPoolFn(torch.autograd.Function):
    """layers/roi_align.py:12-44 (_ROIAlign) for the fused multi-level + depth call: differentiable w.r.t. the maps."""

    @staticmethod
    def forward(ctx, rois, scales, n_img, pooled, sampling_ratio, want_levels, n_levels, ordered, *maps):
        feats, depth = list(maps[:n_levels]), (maps[n_levels] if len(maps) > n_levels else None)
        rgb, dep, levels = _roi_pool(feats, scales, rois, n_img, pooled, sampling_ratio, depth=depth, want_levels=want_levels)
        ctx.save_for_backward(rois)
        ctx.meta = ([tuple(f.shape) for f in feats], list(scales), n_img, pooled, sampling_ratio,
                    tuple(depth.shape) if depth is not None else None)
        ctx.ordered = ordered
        # the leaves' forms: a group of one readable form gets its gradient back in that dtype and memory format
        ctx.forms = (_map_form(feats), _map_form([depth]) if depth is not None else None)
        ctx.mark_non_differentiable(*([levels] if levels is not None else []))
        outs = (rgb,) + ((dep,) if dep is not None else ()) + ((levels,) if levels is not None else ())
        return outs

    @staticmethod
    def backward(ctx, *grads):
        (rois,) = ctx.saved_tensors
        shapes, scales, n_img, pooled, sampling_ratio, depth_shape = ctx.meta
        grad_rgb = grads[0]
        grad_dep = grads[1] if depth_shape is not None else None
        if grad_rgb is None:
            grad_rgb = torch.zeros((rois.shape[0], shapes[0][1], pooled, pooled), device=rois.device)
        ordered = native.ordered_mode(ctx.ordered)
        if ordered and sampling_ratio == 0:
            raise NotImplementedError(_ADAPTIVE_ORDERED)
        in_place = IN_PLACE["adaptive_backward" if sampling_ratio == 0 else "backward_ordered" if ordered else "backward"]
        layouts = [form[1] if form is not None and form[1] in in_place else _NCHW for form in ctx.forms]
        level_grads, depth_grad = _roi_pool_backward(shapes, scales, rois, n_img, pooled, sampling_ratio, grad_rgb,
                                                     depth_shape, grad_dep, ordered=ordered, level_layout=layouts[0], depth_layout=layouts[1])
        level_grads = [_as_leaf(g, ctx.forms[0]) for g in level_grads]
        depth_grad = _as_leaf(depth_grad, ctx.forms[1])
        return (None,) * 8 + tuple(level_grads) + ((depth_grad,) if depth_shape is not None else ())


def _roi_pool_autograd(level_feats, scales, rois, n_img, pooled, sampling_ratio, depth=None, want_levels=False, ordered=False):
    """_roi_pool, recorded on the autograd tape when a map requires grad."""
    maps = list(level_feats) + ([depth] if depth is not None else [])
    if not (torch.is_grad_enabled() and any(m.requires_grad for m in maps)):
        return _roi_pool(level_feats, scales, rois, n_img, pooled, sampling_ratio, depth=depth, want_levels=want_levels)
    outs = _RoiPoolFn.apply(rois, tuple(scales), n_img, pooled, sampling_ratio, want_levels, len(level_feats), ordered, *maps)
    rgb = outs[0]
    dep = outs[1] if depth is not None else None
    levels = outs[-1] if want_levels else None
    return rgb, dep, levels


class ROIAlign(nn.Module):
    """layers/roi_align.py:49-68: ROIAlign(output_size, spatial_scale, sampling_ratio)(input, rois)."""

    def __init__(self, output_size, spatial_scale, sampling_ratio):
        super().__init__()
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio
        if self.output_size[0] != self.output_size[1]:
            raise NotImplementedError("veto_amd ROIAlign: square outputs only (VETO pools 8x8)")

    def forward(self, input, rois):
        return _roi_pool_autograd([input], [self.spatial_scale], rois, input.shape[0], self.output_size[0], self.sampling_ratio)[0]

    def __repr__(self):
        return "%s(output_size=%s, spatial_scale=%s, sampling_ratio=%s)" % (
            self.__class__.__name__, self.output_size, self.spatial_scale, self.sampling_ratio)


class LevelMapper(object):
    """poolers.py:12-43.  Kept for callers that want the levels; Pooler.forward computes them in the kernel."""

    def __init__(self, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
        self.k_min, self.k_max, self.s0, self.lvl0, self.eps = k_min, k_max, canonical_scale, canonical_level, eps

    def __call__(self, boxlists):
        s = torch.sqrt(torch.cat([b.area() for b in boxlists]))
        lv = torch.floor(self.lvl0 + torch.log2(s / self.s0 + self.eps))
        return torch.clamp(lv, min=self.k_min, max=self.k_max).to(torch.int64) - self.k_min


class Pooler(nn.Module):
    """poolers.py:46-171 with cat_all_levels=False."""

    def __init__(self, output_size, scales, sampling_ratio, in_channels=512, cat_all_levels=False):
        super().__init__()
        if cat_all_levels:
            raise NotImplementedError("veto_amd Pooler: cat_all_levels=True (reduce_channel conv) is not the VETO path "
                                      "(relation_head.py:53 builds the extractor without it)")
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        self.scales = [float(s) for s in scales]
        self.sampling_ratio = sampling_ratio
        self.cat_all_levels = False
        self.poolers = nn.ModuleList(ROIAlign(self.output_size, s, sampling_ratio) for s in self.scales)
        lvl_min = -math.log2(self.scales[0])
        lvl_max = -math.log2(self.scales[-1])
        self.map_levels = LevelMapper(lvl_min, lvl_max)
        if not 1 <= len(self.scales) <= 4:
            raise ValueError("1 to 4 pooler scales are supported, got %d" % len(self.scales))

    def convert_to_roi_format(self, boxes):
        """poolers.py:96-107: rows (image index, x1, y1, x2, y2)."""
        concat = torch.cat([b.bbox for b in boxes], dim=0)
        ids = torch.cat([torch.full((len(b), 1), i, dtype=concat.dtype, device=concat.device) for i, b in enumerate(boxes)], dim=0)
        return torch.cat([ids, concat], dim=1)

    def forward(self, x, boxes, depth_features=None, union=False):
        if union:
            raise NotImplementedError("veto_amd Pooler: union pooling (7x7) is not used by the VETO predictors")
        for b in boxes:
            if b.mode != "xyxy":
                raise ValueError("Pooler expects xyxy boxes (poolers.py:96-107 passes BoxList.bbox through), got %s" % b.mode)
        rois = self.convert_to_roi_format(boxes)
        assert rois.size(0) > 0
        if len(x) != len(self.scales):
            raise ValueError("%d feature levels for %d pooler scales" % (len(x), len(self.scales)))
        rgb, depth, levels = _roi_pool_autograd(list(x), self.scales, rois, x[0].shape[0], self.output_size[0],
                                                self.sampling_ratio, depth=depth_features,
                                                want_levels=getattr(self, "keep_levels", False),
                                                ordered=getattr(self, "deterministic", False))
        self.last_levels = levels
        if depth_features is not None:
            return rgb, depth
        return rgb


class VETOFeatureExtractor(nn.Module):
    """roi_box_feature_extractors.py:75-121: forward(x, proposals, depth_features) ->
    (x_2d, d_2d, None, None), the pooled [sum N, 256, R, R] RGB / depth ROI maps (R = POOLER_RESOLUTION, 1..16)."""

    def __init__(self, cfg, in_channels, half_out=False, cat_all_levels=False, for_relation=False):
        super().__init__()
        resolution = cfg.MODEL.ROI_RELATION_HEAD.POOLER_RESOLUTION
        scales = cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES
        sampling_ratio = cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO
        self.pooler = Pooler(output_size=(resolution, resolution), scales=scales, sampling_ratio=sampling_ratio,
                             in_channels=in_channels, cat_all_levels=cat_all_levels)
        # VETO_AMD.DETERMINISTIC: the map gradients through veto_roi_pool_backward_ordered (fixed summation order)
        self.pooler.deterministic = bool(getattr(getattr(cfg, "VETO_AMD", None), "DETERMINISTIC", False))
        self.out_channels = 256

    def forward(self, x, proposals, depth_features=None):
        x_2d = d_2d = None
        if depth_features is not None:
            x_2d, d_2d = self.pooler(x, proposals, depth_features=depth_features)
        else:
            x = self.pooler(x, proposals, depth_features=depth_features)   # :112 (result unused by the reference too)
        return x_2d, d_2d, None, None


def make_roi_box_feature_extractor(cfg, in_channels, half_out=False, cat_all_levels=False, for_relation=False):
    """roi_box_feature_extractors.py:315-323: the relation head asks with for_relation=True and gets
    ROI_RELATION_HEAD.FEATURE_EXTRACTOR_MINI ("VETOFeatureExtractor", VETO_final.yaml:71) when depth is on."""
    if for_relation and getattr(cfg.MODEL.ROI_RELATION_HEAD, "FEATURE_EXTRACTOR_MINI", None) is not None \
            and cfg.DATASETS.USE_DEPTH:
        name = cfg.MODEL.ROI_RELATION_HEAD.FEATURE_EXTRACTOR_MINI
    else:
        name = cfg.MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR
    if name != "VETOFeatureExtractor":
        raise ValueError("veto_amd only provides VETOFeatureExtractor, got %r" % (name,))
    return VETOFeatureExtractor(cfg, in_channels, half_out, cat_all_levels, for_relation)
