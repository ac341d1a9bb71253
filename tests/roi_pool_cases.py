"""Inputs of the ROI pooling suite (tests/test_roi_pool_gpu.py on the device, tests/test_roi_pool_cases_host.py for their premises)
and deliberately WRONG restatements of oracle/roi_align_oracle.py that those inputs must be able to tell from the right one.

Plain module, no test in it.  Everything is numpy on the CPU; nothing here touches the device."""
import numpy as np

from oracle import roi_align_oracle as ro
from veto_amd import synth

F = np.float32
U = 2.0 ** -24                                   # unit roundoff of float32
SCALE = 1.0 / 16
SCALES4 = (0.25, 0.125, 0.0625, 0.03125)

# ---- section 1: every forward instance and lane layout -------------------------------------------------------------
FORWARD_INSTANCES = [(8, 3), (8, 4), (5, 3), (3, 4), (2, 1), (1, 1), (1, 4)]     # C = 40
FORWARD_CHANNELS = [1, 31, 32, 33, 40, 65]                                       # at (8, 2)
# ---- section 6: every backward instance ----------------------------------------------------------------------------
BACKWARD_INSTANCES = [(8, 1), (7, 2), (8, 3), (4, 4), (8, 4), (1, 1)]            # C = 33


def single(pooled, ratio, channels):
    """synth.synthetic_roi_single: one [2, channels, 50, 84] map at scale 1/16, 23 ROI rows with the four fixed corner boxes."""
    return synth.synthetic_roi_single(pooled, ratio, channels=channels)


def cotangent(shape, seed):
    return np.random.RandomState(seed).randn(*shape).astype(F)


# ---- section 2: a small pyramid with unequal channel counts --------------------------------------------------------
PYR_W, PYR_H = 1024, 640
SEED_PYRAMID, SEED_EMPTY = 121, 44     # chosen so that the boxes reach every level they can (asserted by the host test)


def pyramid(channels=40, depth_channels=8, num_objs=(11, 12), W=PYR_W, H=PYR_H, seed=SEED_PYRAMID):
    """Four levels (strides 4..32) and a stride-16 depth map with its own channel count.  The boxes (one synth.roi_test_boxes draw,
    dealt to the images in order) are drawn before the maps, so they do not depend on the channel counts.
    Returns (feats, depth, boxes per image)."""
    rng = np.random.RandomState(seed)
    boxes = np.split(synth.roi_test_boxes(rng, sum(num_objs), W, H), np.cumsum(num_objs)[:-1])
    B = len(num_objs)
    feats = [rng.randn(B, channels, H >> (2 + l), W >> (2 + l)).astype(F) for l in range(4)]
    depth = rng.randn(B, depth_channels, H >> 4, W >> 4).astype(F)
    return feats, depth, boxes


def level_form(feats, n_levels):
    """(maps, scales) of the 4-, 3- and 1-level forms: the first n levels, or the stride-16 map alone."""
    if n_levels == 1:
        return [feats[2]], (SCALES4[2],)
    return feats[:n_levels], SCALES4[:n_levels]


# ---- section 3: level boundaries ------------------------------------------------------------------------------------
BOUNDARY_SIDES = (112, 224, 448)
BOUNDARY_MAP_SIZES = (116, 58, 29, 15)           # H = W per level: holds x2 * scale of every box below


def boundary_sweep(s):
    """Boxes [3, 5, x2, 5 + s - 1] with x2 in single float32 steps from 128 below 3 + s - 1 to 64 above: sqrt(area) walks
    across s, where LevelMapper's floor(4 + log2(sqrt(area) / 224 + 1e-6)) steps up."""
    x2 = F(3 + s - 1)
    for _ in range(128):
        x2 = np.nextafter(x2, F(-np.inf), dtype=F)
    rows = []
    for _ in range(128 + 64 + 1):
        rows.append([3.0, 5.0, x2, 5.0 + s - 1])
        x2 = np.nextafter(x2, F(np.inf), dtype=F)
    return np.array(rows, dtype=F)


def boundary_boxes():
    return np.concatenate([boundary_sweep(s) for s in BOUNDARY_SIDES])     # 579 boxes


def boundary_maps(channels=2):
    """Level l is the constant l + 1: whatever is pooled from it is l + 1, so the output names the level that was read."""
    return [np.full((1, channels, n, n), l + 1, dtype=F) for l, n in enumerate(BOUNDARY_MAP_SIZES)]


def map_levels_f64(boxes, k_min=2, k_max=5):
    """WRONG variant 5: LevelMapper evaluated in float64 on the float32 boxes."""
    b = np.asarray(boxes, dtype=np.float64)
    s = np.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))
    lv = np.floor(4 + np.log2(s / 224 + 1e-6))
    return np.clip(lv, k_min, k_max).astype(np.int64) - k_min


# ---- section 4: samples exactly on the validity edge ---------------------------------------------------------------
def edge_map():
    return np.arange(1, 31, dtype=F).reshape(1, 1, 6, 5)       # H = 6, W = 5


def _next(v, up):
    return float(np.nextafter(F(v), F(np.inf if up else -np.inf), dtype=F))


def edge_rois():
    """Scale 1, pooled 2, ratio 1 on the 6 x 5 map: boxes four wide, so bin = 2 and the sample centres are start + 1, start + 3.
    Rows 0-1: a centre exactly at -1 / exactly at W and H (valid, clamped).  Rows 2-5: one float32 step further out in x or in y
    (that sample is invalid and contributes 0)."""
    W, H = 5, 6
    return np.array([
        [0, -2, -2, 2, 2],
        [0, W - 1, H - 1, W + 3, H + 3],
        [0, _next(-2, False), -2, 2, 2],
        [0, -2, _next(-2, False), 2, 2],
        [0, _next(W - 1, True), H - 1, W + 3, H + 3],
        [0, W - 1, _next(H - 1, True), W + 3, H + 3],
    ], dtype=F)


# test_roi_align.py::test_hand_computed_border_and_out_of_map_samples: arange(16) as 4 x 4 (+1 for the last), pooled 2, ratio 1, scale 1
HAND_ROIS = np.array([[0, 1, 1, 3, 3], [0, 2, 2, 6, 6], [0, -3, -3, 1, 1], [0, -1.5, -1.5, 0.5, 0.5]], dtype=F)
HAND_WANT = [[7.5, 8.5, 11.5, 12.5], [15.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
HAND_WANT_PLUS1 = [[8.5, 9.5, 12.5, 13.5], [16.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]]


def hand_map():
    return np.arange(16, dtype=F).reshape(1, 1, 4, 4)


# ---- section 5: masked samples must not leak -------------------------------------------------------------------------
def roi_tables(roi, scale, pooled, ratio, H, W):
    """The two axis tables of one ROI row, as oracle.roi_align builds them: ((vy, ylo, yhi, ly, hy), (vx, xlo, xhi, lx, hx))."""
    sc = F(scale)
    x1, y1, x2, y2 = F(roi[1] * sc), F(roi[2] * sc), F(roi[3] * sc), F(roi[4] * sc)
    roi_w, roi_h = max(F(x2 - x1), F(1.0)), max(F(y2 - y1), F(1.0))
    return (ro._axis_samples(y1, F(roi_h / F(pooled)), pooled, ratio, H), ro._axis_samples(x1, F(roi_w / F(pooled)), pooled, ratio, W))


def touched_pixels(rois, scale, pooled, ratio, shape):
    """touched [B, H, W] bool: the pixels that a tap of a VALID sample of some ROI reads (whatever its weight: 0 * Inf is NaN);
    n_invalid [R]: the number of invalid samples per ROI."""
    B, _, H, W = shape
    touched = np.zeros((B, H, W), dtype=bool)
    n_invalid = np.zeros(len(rois), dtype=np.int64)
    for r, roi in enumerate(rois):
        (vy, ylo, yhi, _, _), (vx, xlo, xhi, _, _) = roi_tables(roi, scale, pooled, ratio, H, W)
        ys = np.unique(np.concatenate([ylo[vy], yhi[vy]]))
        xs = np.unique(np.concatenate([xlo[vx], xhi[vx]]))
        touched[int(roi[0])][np.ix_(ys, xs)] = True
        n_invalid[r] = len(vy) * len(vx) - int(vy.sum()) * int(vx.sum())
    return touched, n_invalid


def leak_case(pooled=8, ratio=2, channels=40):
    """The clean single-map case with every ROI whose valid samples read pixel (0, 0) moved 40 px down and right until they do not,
    and a poisoned copy of the map: NaN at pixel (0, 0) of every plane (what the kernel reads for an invalid sample) and +Inf at
    every pixel that no valid sample touches.  Returns (feat, poisoned, rois)."""
    feat, rois = single(pooled, ratio, channels)
    rois = rois.copy()
    for r in range(len(rois)):
        for _ in range(8):
            if not touched_pixels(rois[r:r + 1], SCALE, pooled, ratio, feat.shape)[0][:, 0, 0].any():
                break
            rois[r, 1:] += F(40)
    touched, _ = touched_pixels(rois, SCALE, pooled, ratio, feat.shape)
    poisoned = feat.copy()
    poisoned[np.broadcast_to(~touched[:, None], feat.shape)] = np.inf
    poisoned[:, :, 0, 0] = np.nan
    return feat, poisoned, rois


def leak_backward_case(pooled=8, ratio=2, channels=33):
    """The single-map case plus one ROI with every sample outside the map; its grad_out rows are NaN.
    Returns (feat_shape, rois, grad_out, index of the outside ROI)."""
    feat, rois = single(pooled, ratio, channels)
    H, W = feat.shape[2:]
    outside = np.array([[1, (W + 2) * 16, (H + 2) * 16, (W + 9) * 16, (H + 7) * 16]], dtype=F)
    rois = np.concatenate([rois[:11], outside, rois[11:]])
    gout = cotangent((len(rois), channels, pooled, pooled), 77)
    gout[11] = np.nan
    return feat.shape, rois, gout, 11


# ---- section 6: the backward bound ------------------------------------------------------------------------------------
def backward_bound(want, K, A):
    """|device - want| per pixel for a float32 accumulation of K float32 terms in ANY order, the terms themselves bit-equal to the
    oracle's: gamma_K * sum |term| with gamma_K = K u / (1 - K u), plus one rounding of the result.  Where K = 0 the bound is 0."""
    Ku = K.astype(np.float64)[:, None] * U
    return Ku / (1.0 - Ku) * A + U * np.abs(want)


def check_backward(got, want, K, A):
    """Returns (largest error / bound over the pixels with K > 0, K max); asserts exact zeros where K = 0."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    zero = np.broadcast_to((K == 0)[:, None], want.shape)
    assert not got[zero].any(), "a pixel no sample touches holds %r" % got[zero][np.nonzero(got[zero])[0][:4]]
    err, bound = np.abs(got - want), backward_bound(want, K, A)
    live = ~zero & (bound > 0)
    assert not err[~zero & (bound == 0)].any()          # every contribution is exactly 0: so is the sum
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    return ratio, int(K.max())


CONTENTION_ROI = [30.2, 40.7, 30.3, 40.8]


def contention_case(copies=64, channels=33):
    """`copies` times one sub-pixel ROI at (8, 2): every add of a channel plane lands in the same 3 x 3 pixels (the ROI is widened to
    one map pixel and straddles a pixel border on both axes), 896 to 16 384 adds per pixel with 64 copies.  Under the bound of
    backward_bound one lost update of average size is A / K against gamma_K A ~ K u A: it shows where K^2 u < 1, i.e. K < 4 096 (the
    three lightest pixels here); at the 16 384-add pixel it takes about K^2 u = 16 of them.  exact_contention_case is the case in
    which a single lost update shows at every pixel."""
    rois = np.array([[0] + CONTENTION_ROI] * copies, dtype=F)
    return (2, channels, 50, 84), rois, cotangent((copies, channels, 8, 8), 78)


EXACT_CONTENTION_ROI = [32.0, 48.0, 48.0, 64.0]


def exact_contention_case(copies=64, channels=33):
    """Contention with an order-free answer.  The ROI is exactly one map pixel, (2, 3) .. (3, 4) at scale 1/16: every sample
    coordinate is a multiple of 1/32 strictly inside that pixel, so all adds of a plane land on the SAME FOUR pixels (256 per pixel
    and copy) and every weight is a multiple of 2^-10.  The cotangent holds integers in [-3, 3], so every term g * w / 4 is a
    multiple of 2^-12 and the absolute sum per pixel stays below 2^12 (16 per copy and unit of |g|: at most 3 072 with 64 copies).
    Every partial sum of such terms, in any order, is a multiple of 2^-12 below 2^12 and therefore a float32: the float32
    accumulation is exact whatever the order, and the device must equal the oracle EXACTLY -- one lost nonzero update is visible at
    every pixel, the 16 384-add ones included."""
    rois = np.array([[0] + EXACT_CONTENTION_ROI] * copies, dtype=F)
    gout = np.random.RandomState(79).randint(-3, 4, size=(copies, channels, 8, 8)).astype(F)
    return (2, channels, 50, 84), rois, gout


# ---- section 7: a batch with empty images -----------------------------------------------------------------------------
EMPTY_COUNTS = (3, 0, 7, 0, 2)


def empty_image_case():
    return pyramid(channels=40, depth_channels=8, num_objs=EMPTY_COUNTS, W=512, H=320, seed=SEED_EMPTY)


def to_rois(boxes):
    """ro.to_rois for lists that hold empty images."""
    return ro.to_rois([np.asarray(b, dtype=F).reshape(-1, 4) for b in boxes])


def pyramid_backward(g_rgb, g_dep, boxes, shapes, scales, depth_shape, pooled=8, ratio=2):
    """Oracle gradients of a Pooler call with their stats: ([(grad, K, A) per level], (grad, K, A) of the depth map or None)."""
    rois = to_rois(boxes)
    if len(scales) == 1:
        lv = np.zeros(len(rois), dtype=np.int64)
    else:
        lv = ro.map_levels(rois[:, 1:], int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1]))))
    per_level = []
    for l, (shape, sc) in enumerate(zip(shapes, scales)):
        idx = np.nonzero(lv == l)[0]
        per_level.append(ro.roi_align_backward(g_rgb[idx], rois[idx], sc, shape, pooled, ratio, stats=True))
    dep = None
    if g_dep is not None:
        dep = ro.roi_align_backward(g_dep, rois, scales[2] if len(scales) > 1 else scales[0], depth_shape, pooled, ratio, stats=True)
    return per_level, dep


# ---- section 8: wrong restatements ------------------------------------------------------------------------------------
def _axis(start, bin_size, pooled, grid, size, far_ge):
    """ro._axis_samples with the far-edge comparison selectable; invalid entries carry what the kernel reads for them:
    index 0 and the weights of the clamped coordinate."""
    n = pooled * grid
    valid, low, high = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    l, h = np.zeros(n, dtype=F), np.ones(n, dtype=F)
    for p in range(pooled):
        for i in range(grid):
            v = F(F(start + F(F(p) * bin_size)) + F(F(F(i + 0.5) * bin_size) / F(grid)))
            k = p * grid + i
            if v < F(-1.0) or (v >= F(size) if far_ge else v > F(size)):
                continue
            valid[k] = True
            if v <= 0:
                v = F(0)
            lo = int(v)
            if lo >= size - 1:
                hi = lo = size - 1
                v = F(lo)
            else:
                hi = lo + 1
            low[k], high[k] = lo, hi
            l[k] = F(v - F(lo))
            h[k] = F(F(1.0) - l[k])
    return valid, low, high, l, h


VARIANTS_FORWARD = ("aligned", "far_ge", "mask_mul", "fused")


def variant_roi_align(feat, rois, spatial_scale, pooled, ratio, variant=None):
    """ro.roi_align (variant None: bit-identical, asserted by the host test) or one of its wrong forms:
      aligned   the -0.5 pixel shift of the "aligned" ROIAlign;
      far_ge    a sample exactly at `size` treated as outside (>= for >);
      mask_mul  an invalid sample read at plane[0] and multiplied by 0 instead of being dropped;
      fused     each sample's four-term sum evaluated exactly (float64) and rounded once, as FMA contraction does."""
    assert variant in (None,) + VARIANTS_FORWARD
    feat = np.ascontiguousarray(feat, dtype=F)
    rois = np.asarray(rois, dtype=F)
    _, C, H, W = feat.shape
    out = np.zeros((len(rois), C, pooled, pooled), dtype=F)
    scale = F(spatial_scale)
    shift = F(0.5) if variant == "aligned" else F(0)
    for r in range(len(rois)):
        plane = feat[int(rois[r, 0])]
        x1, y1, x2, y2 = (F(F(rois[r, k] * scale) - shift) for k in (1, 2, 3, 4))
        roi_w, roi_h = max(F(x2 - x1), F(1.0)), max(F(y2 - y1), F(1.0))
        vy, ylo, yhi, ly, hy = _axis(y1, F(roi_h / F(pooled)), pooled, ratio, H, variant == "far_ge")
        vx, xlo, xhi, lx, hx = _axis(x1, F(roi_w / F(pooled)), pooled, ratio, W, variant == "far_ge")
        count = F(ratio * ratio)
        for ph in range(pooled):
            for pw in range(pooled):
                acc = np.zeros(C, dtype=F)
                for ky in range(ph * ratio, (ph + 1) * ratio):
                    for kx in range(pw * ratio, (pw + 1) * ratio):
                        ok = vy[ky] and vx[kx]
                        if not ok and variant != "mask_mul":
                            continue
                        if not ok:
                            with np.errstate(invalid="ignore"):
                                acc = acc + plane[:, 0, 0] * F(0)
                            continue
                        w = (F(hy[ky] * hx[kx]), F(hy[ky] * lx[kx]), F(ly[ky] * hx[kx]), F(ly[ky] * lx[kx]))
                        v = (plane[:, ylo[ky], xlo[kx]], plane[:, ylo[ky], xhi[kx]], plane[:, yhi[ky], xlo[kx]], plane[:, yhi[ky], xhi[kx]])
                        if variant == "fused":
                            val = sum(np.float64(wk) * vk.astype(np.float64) for wk, vk in zip(w, v)).astype(F)
                        else:
                            val = ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3]
                        acc = acc + val
                out[r, :, ph, pw] = acc / count
    return out


def backward_without_count(grad_out, rois, spatial_scale, feat_shape, pooled, ratio):
    """WRONG variant 6: the scatter without the division by the sample count.  The scatter is linear in grad_out and `count` is a
    power of two or 9, so this is the oracle on grad_out * count up to one rounding per term."""
    return ro.roi_align_backward(np.asarray(grad_out, dtype=F) * F(ratio * ratio), rois, spatial_scale, feat_shape, pooled, ratio)
