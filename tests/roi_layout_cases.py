"""Inputs of the ROI pooling map-form suite (tests/test_roi_layouts_gpu.py on the device, tests/test_roi_layouts_host.py for their
premises): the same values as dense NCHW float32 and as the NCHW / NHWC, float32 / float16 / bfloat16 buffers that veto_roi_pool reads
in place, and the deliberately WRONG readings of those buffers (layout flag ignored, bfloat16 read as float16) that the expected
results must be able to tell from the right one.

Plain module, no test in it.  Everything is numpy on the CPU.  The cases are those of tests/roi_pool_cases.py and
tests/deterministic_cases.py, which this module imports and does not change."""
import functools

import numpy as np

import deterministic_cases as dc
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
F32, F16, BF16 = 0, 1, 2                # veto_roi_pool_args_t.level_dtype / depth_dtype
NCHW, NHWC = 0, 1                       # veto_roi_pool_args_t.level_layout / depth_layout
DTYPE_NAMES = {F32: "float32", F16: "float16", BF16: "bfloat16"}
LAYOUT_NAMES = {NCHW: "NCHW", NHWC: "NHWC"}
ITEMSIZE = {F32: 4, F16: 2, BF16: 2}

# the five forms the float32 NCHW kernels did not read, as (dtype, layout)
FORMS = [(F16, NCHW), (BF16, NCHW), (F32, NHWC), (F16, NHWC), (BF16, NHWC)]
WALK_INSTANCES = [(9, 3), (12, 1), (16, 2)]                                     # pooled 9..16: a lane owns several bins
FORWARD_INSTANCES = rc.FORWARD_INSTANCES + [(8, 2)] + WALK_INSTANCES            # C = 40
CHANNELS = [1, 3, 31, 32, 33, 40, 65]                                           # at (8, 2)
ORDERED_CASES = ["ratio2", "channels32", "channels65", "levels4_depth", "level_boundaries", "far_edge", "contention_64_copies",
                 "exact_contention"]


def form_id(form):
    return "%s-%s" % (LAYOUT_NAMES[form[1]], DTYPE_NAMES[form[0]])


# ---- bfloat16, written twice ---------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the upper 16 bits after round-to-nearest-even on the lower 16 (uint16).  NaN becomes the quiet NaN 0x7FC0 with
    the sign kept: rounding a NaN's payload could carry into the exponent and make it an infinity."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=F))
    return np.where(nan, ((u >> 16) & 0x8000 | 0x7FC0).astype(np.uint16), r)


def bf16_bits_torch(x):
    """The same through torch.bfloat16 on the CPU."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F)


def quantise(a, dtype):
    """The float32 values that `dtype` holds for `a`: what every reference is computed on."""
    a = np.asarray(a, dtype=F)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(F)
    if dtype == BF16:
        return bf16_to_f32(bf16_bits(a))
    return a.copy()


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def pack(a, form):
    """The dense buffer of the NCHW float32 array `a` in `form`: float32 / float16 storage, or the uint16 bit patterns of bfloat16,
    shaped [N, C, H, W] or [N, H, W, C]."""
    dtype, layout = form
    a = np.asarray(a, dtype=F)
    if layout == NHWC:
        a = a.transpose(0, 2, 3, 1)
    a = np.ascontiguousarray(a)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return a.astype(np.float16)
    if dtype == BF16:
        return bf16_bits(a)
    return a


def unpack(buf, form, shape):
    """The NCHW float32 array that a buffer of `form` holds for a map of the logical shape [N, C, H, W]: the inverse of pack, and
    with a wrong `form` the misreading of a kernel that ignores a flag."""
    dtype, layout = form
    N, C, H, W = shape
    flat = np.ascontiguousarray(buf).reshape(-1)
    if dtype == BF16:
        vals = bf16_to_f32(flat.view(np.uint16))
    elif dtype == F16:
        vals = flat.view(np.float16).astype(F)
    else:
        vals = flat.view(F)
    if layout == NHWC:
        return np.ascontiguousarray(vals.reshape(N, H, W, C).transpose(0, 3, 1, 2))
    return vals.reshape(N, C, H, W).copy()


def off_boundary(flat, lead=1):
    """A copy of the 1-d array `flat` that starts `lead` elements past a 16-byte boundary: (the view, the buffer that owns it)."""
    item = flat.dtype.itemsize
    buf = np.empty(flat.size + 16 // item + lead + 1, dtype=flat.dtype)
    start = (-buf.ctypes.data % 16) // item + lead
    view = buf[start:start + flat.size]
    view[...] = flat
    return view, buf


# ---- forward references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_forward(pooled, ratio, channels, dtype):
    """(values the map holds in `dtype` as NCHW float32, rois, oracle output on those values)."""
    feat, rois = rc.single(pooled, ratio, channels)
    q = quantise(feat, dtype)
    return q, rois, ro.roi_align(q, rois, rc.SCALE, pooled, ratio)


@functools.lru_cache(maxsize=None)
def depth_forward(channels, dtype, pyramid_channels):
    """A second map on the grid of rc.single(8, 2, pyramid_channels) with its own channel count (8: narrower than most pyramids
    here, 70: wider): the depth map of a one-level call, pooled at the same scale from the same ROIs (rc.single draws them after
    the map, so they depend on its channel count)."""
    _, rois = rc.single(8, 2, pyramid_channels)
    q = quantise(np.random.RandomState(500 + channels).randn(2, channels, 50, 84).astype(F), dtype)
    return q, ro.roi_align(q, rois, rc.SCALE, 8, 2)


@functools.lru_cache(maxsize=None)
def pyramid_forward(n_levels, level_dtype, depth_dtype):
    """rc.pyramid(40, 8) in the n-level form: (maps, scales, depth, rois, oracle rgb, oracle depth, oracle levels)."""
    feats, depth, boxes = rc.pyramid(channels=40, depth_channels=8)
    maps, scales = rc.level_form(feats, n_levels)
    maps, depth = [quantise(m, level_dtype) for m in maps], quantise(depth, depth_dtype)
    rgb, dep, lv = ro.pooler_forward(maps, boxes, depth, scales=scales, return_levels=True)
    return maps, scales, depth, ro.to_rois(boxes), rgb, dep, lv


# ---- backward references -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_backward(pooled=8, ratio=2, channels=33):
    feat, rois = rc.single(pooled, ratio, channels)
    gout = rc.cotangent((len(rois), channels, pooled, pooled), 600 + channels)
    return feat.shape, rois, gout, ro.roi_align_backward(gout, rois, rc.SCALE, feat.shape, pooled, ratio, stats=True)


@functools.lru_cache(maxsize=None)
def pyramid_backward(depth_channels=8):
    feats, depth, boxes = rc.pyramid(channels=40, depth_channels=depth_channels)
    n = sum(len(b) for b in boxes)
    g_rgb, g_dep = rc.cotangent((n, 40, 8, 8), 31), rc.cotangent((n, depth_channels, 8, 8), 32)
    per_level, dep = rc.pyramid_backward(g_rgb, g_dep, boxes, [f.shape for f in feats], rc.SCALES4, depth.shape)
    return feats, depth, boxes, g_rgb, g_dep, per_level, dep


@functools.lru_cache(maxsize=None)
def ordered_reference(name):
    case = dc.ROI_CASES[name]()
    levels, dep = dc.pooler_backward_ordered(case)
    return case, levels, dep
