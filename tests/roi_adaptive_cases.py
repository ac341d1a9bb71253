"""Inputs of the adaptive-grid ROI pooling tests (sampling_ratio = 0: tests/test_roi_adaptive_gpu.py on the device,
tests/test_roi_adaptive_host.py for their premises), an explicit restatement of the kernel as a list of taps, and deliberately WRONG
restatements that the inputs must be able to tell from the right one.  Plain module, no test in it; numpy on the CPU only.

np_adaptive_taps lists, in the kernel's order (ROI, bin row, bin column, sample iy, sample ix), every valid sample as four
(pixel, float32 weight) taps, with the count gh * gw and the number of skipped samples per output cell.  Two things follow from it:
apply_taps, the forward (held to oracle/roi_align_oracle.py::roi_align bit for bit by the host test), and taps_backward, the
backward reference -- per pixel the float64 sum of the float32 terms (g * w) / count, their number K and the sum of their absolute
values, what roi_align_backward(stats=True) gives for the fixed ratios."""
import functools

import numpy as np

import roi_pool16_cases as c16
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
U = 2.0 ** -24
SCALE = rc.SCALE                       # 1 / 16: the [2, C, 50, 84] map of synth.synthetic_roi_single
H, W = 50, 84
POOLED = [1, 6, 7, 8, 14, 16]
CHANNELS = [1, 33, 65]                 # part of a wave's planes, a slab + 1, two slabs + 1
VARIANTS = ("floor", "unclamped", "square", "count_gh2", "f64grid")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def axis_grid(lo, hi, scale, pooled, variant=None):
    """(start, bin, g) of one ROI axis: ROIAlign_cuda.cu:84-104 in float32."""
    lo_c, hi_c = F(F(lo) * F(scale)), F(F(hi) * F(scale))
    raw = F(hi_c - lo_c)
    ln = max(raw, F(1.0))
    bin_size = F(ln / F(pooled))
    q = F(ln / F(pooled))
    if variant == "floor":
        g = int(np.floor(q))
    elif variant == "unclamped":
        g = int(np.ceil(F(raw / F(pooled))))
    elif variant == "f64grid":
        s64 = float(F(scale))      # the float32 scale the kernel is handed, then everything in float64
        g = int(np.ceil(max(float(hi) * s64 - float(lo) * s64, 1.0) / pooled))
    else:
        g = int(np.ceil(q))
    return lo_c, bin_size, g


def axis_coords(start, bin_size, p, g, i=None):
    """float32 sample coordinates v(i) of bin p, i = 0 .. g - 1 (or the given indices): the expression of axis_coord in roialign.hip"""
    i = np.arange(g, dtype=F) if i is None else np.asarray(i, dtype=F)
    return (F(start + F(F(p) * bin_size)) + ((i + F(0.5)) * bin_size) / F(g)).astype(F)


def axis_valid(v, size):
    return ~((v < F(-1.0)) | (v > F(size)))


def axis_taps(v, size):
    """(lo, hi, l, h) of valid coordinates: ROIAlign_cuda.cu:31-57"""
    v = np.where(v <= 0, F(0), v).astype(F)
    lo = v.astype(np.int64)
    edge = lo >= size - 1
    lo = np.where(edge, size - 1, lo)
    hi = np.where(edge, size - 1, lo + 1)
    v = np.where(edge, lo.astype(F), v).astype(F)
    l = (v - lo.astype(F)).astype(F)
    return lo, hi, l, (F(1.0) - l).astype(F)


def bisect_valid_range(start, bin_size, p, g, size):
    """(first valid index, number of valid samples) by the two bisections of axis_valid_range in roialign.hip: never more than
    2 * ceil(log2(g + 1)) evaluations of v."""
    def first(pred):
        lo, hi = 0, g
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if pred(axis_coords(start, bin_size, p, g, [mid])[0]):
                hi = mid
            else:
                lo = mid + 1
        return lo
    i0 = first(lambda v: not v < F(-1.0))
    n = first(lambda v: v > F(size)) - i0
    if n < 0 or n > 2 * size + 3:
        n = 0
    return i0, n


class Taps(object):
    """cell [N] flat output cell (r * P * P + ph * P + pw) of each valid sample, ascending in the kernel's order; pix [N, 4] flat pixel
    (b * H * W + y * W + x) and w [N, 4] float32 weight of its four taps; count [R * P * P] float32; grid [R, 2] (gh, gw);
    skipped [R * P * P] samples left out; shape, pooled."""


def np_adaptive_taps(rois, scale, shape, pooled, variant=None):
    rois = np.asarray(rois, dtype=F)
    B, _, Hm, Wm = shape
    P = pooled
    cells, pix, wts = [], [], []
    count = np.zeros(len(rois) * P * P, dtype=F)
    skipped = np.zeros(len(rois) * P * P, dtype=np.int64)
    grid = np.zeros((len(rois), 2), dtype=np.int64)
    for r, roi in enumerate(rois):
        b = int(roi[0])
        sy, bin_h, gh = axis_grid(roi[2], roi[4], scale, P, variant)
        sx, bin_w, gw = axis_grid(roi[1], roi[3], scale, P, variant)
        if variant == "square":
            gh = gw = max(gh, gw)
        grid[r] = gh, gw
        cnt = F(gh * gh) if variant == "count_gh2" else F(gh * gw)
        ys, xs = [], []
        for p in range(P):
            vy, vx = axis_coords(sy, bin_h, p, gh), axis_coords(sx, bin_w, p, gw)
            oky, okx = axis_valid(vy, Hm), axis_valid(vx, Wm)
            ys.append((oky,) + axis_taps(vy[oky], Hm))
            xs.append((okx,) + axis_taps(vx[okx], Wm))
        for ph in range(P):
            oky, ylo, yhi, ly, hy = ys[ph]
            for pw in range(P):
                okx, xlo, xhi, lx, hx = xs[pw]
                cell = (r * P + ph) * P + pw
                count[cell] = cnt
                ny, nx = len(ylo), len(xlo)
                skipped[cell] = gh * gw - ny * nx
                if ny == 0 or nx == 0:
                    continue
                Y = lambda a: np.repeat(a, nx)      # noqa: E731  iy outer
                X = lambda a: np.tile(a, ny)        # noqa: E731  ix inner
                w = np.stack([Y(hy) * X(hx), Y(hy) * X(lx), Y(ly) * X(hx), Y(ly) * X(lx)], 1).astype(F)
                base = b * Hm * Wm
                px = np.stack([base + Y(ylo) * Wm + X(xlo), base + Y(ylo) * Wm + X(xhi), base + Y(yhi) * Wm + X(xlo), base + Y(yhi) * Wm + X(xhi)], 1)
                cells.append(np.full(ny * nx, cell, dtype=np.int64))
                pix.append(px)
                wts.append(w)
    t = Taps()
    t.cell = np.concatenate(cells) if cells else np.zeros(0, dtype=np.int64)
    t.pix = np.concatenate(pix) if pix else np.zeros((0, 4), dtype=np.int64)
    t.w = np.concatenate(wts) if wts else np.zeros((0, 4), dtype=F)
    t.count, t.skipped, t.grid, t.shape, t.pooled, t.n_roi = count, skipped, grid, tuple(shape), P, len(rois)
    return t


def apply_taps(t, feat, plus_zero=True):
    """The forward from the tap list: per cell acc = +0, acc = acc + (((w0*v0 + w1*v1) + w2*v2) + w3*v3) sample by sample, + 0 once
    when a sample was skipped (plus_zero=False: the restatement without it), / count.  [R, C, P, P] float32."""
    feat = np.ascontiguousarray(feat, dtype=F)
    B, C, Hm, Wm = feat.shape
    flat = feat.transpose(1, 0, 2, 3).reshape(C, B * Hm * Wm)
    P = t.pooled
    out = np.zeros((C, t.n_roi * P * P), dtype=F)
    if len(t.cell):
        v = flat[:, t.pix]                                                    # [C, N, 4]
        val = ((t.w[:, 0] * v[:, :, 0] + t.w[:, 1] * v[:, :, 1]) + t.w[:, 2] * v[:, :, 2]) + t.w[:, 3] * v[:, :, 3]
        val = val.astype(F)
        ends = np.nonzero(np.diff(t.cell, append=-1))[0] + 1
        start = 0
        for e in ends:
            acc = np.zeros(C, dtype=F)
            for k in range(start, e):
                acc = acc + val[:, k]
            out[:, t.cell[start]] = acc
            start = e
    if plus_zero:
        out[:, t.skipped > 0] = out[:, t.skipped > 0] + F(0)
    out = (out / t.count[None, :]).astype(F)
    return np.ascontiguousarray(out.reshape(C, t.n_roi, P, P).transpose(1, 0, 2, 3))


def taps_backward(t, grad_out):
    """(grad [B, C, H, W] float64, K [B, H, W] int64, A [B, C, H, W] float64): per pixel the float64 sum of the float32 terms
    (g * w) / count of every tap of every valid sample, their number and the sum of their absolute values."""
    g = np.asarray(grad_out, dtype=F)
    B, C, Hm, Wm = t.shape
    assert g.shape == (t.n_roi, C, t.pooled, t.pooled)
    gc = g.transpose(1, 0, 2, 3).reshape(C, -1)
    grad = np.zeros((C, B * Hm * Wm), dtype=np.float64)
    A = np.zeros((C, B * Hm * Wm), dtype=np.float64)
    K = np.zeros(B * Hm * Wm, dtype=np.int64)
    if len(t.cell):
        gs, cnt = gc[:, t.cell], t.count[t.cell]
        term = ((gs[:, :, None] * t.w[None]).astype(F) / cnt[None, :, None]).astype(F).astype(np.float64)      # [C, N, 4]
        where = t.pix.ravel()      # (sample, tap) order: bincount adds in input order, the order of roi_align_backward
        for c in range(C):
            grad[c] = np.bincount(where, weights=term[c].ravel(), minlength=grad.shape[1])
            A[c] = np.bincount(where, weights=np.abs(term[c]).ravel(), minlength=grad.shape[1])
        K = np.bincount(where, minlength=len(K))
    shape4 = lambda a: np.ascontiguousarray(a.reshape(C, B, Hm, Wm).transpose(1, 0, 2, 3))      # noqa: E731
    return shape4(grad), K.reshape(B, Hm, Wm), shape4(A)


def adaptive_bound(K, A):
    """|device - float64 sum| per pixel for a float32 accumulation of K terms in any order: K u / (1 - K u) * sum |term|"""
    Ku = K.astype(np.float64)[:, None] * U
    return Ku / (1.0 - Ku) * A


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------
def feature_map(channels=65, seed=5, shape=(2, H, W)):
    """Multiples of 1/8 in [-8, 8]: exact in float32, float16 and bfloat16, so one oracle output serves the three map dtypes; the
    channel counts of CHANNELS are its leading planes."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-64, 65, size=(shape[0], channels) + tuple(shape[1:])) / 8.0).astype(F)


WHOLE_MAP = [0.0, 0.0, W * 16.0, H * 16.0]                       # pooled 1: a 50 x 84 grid
FAR_AROUND = [-4000.0, -4000.0, W * 16 + 4000.0, H * 16 + 4000.0]
NAMED = {
    "tall": [100.0, 50.0, 160.0, 700.0], "wide": [90.0, 300.0, 1200.0, 340.0],
    "sub_pixel": [30.2, 40.7, 30.3, 40.8], "zero_size": [100.0, 100.0, 100.0, 100.0], "malformed": [50.0, 60.0, 40.0, 30.0],
    "grid_3x2": [200.0, 100.0, 200.0 + 7 * 1.5 * 16, 100.0 + 7 * 2.5 * 16],      # pooled 7: gh 3, gw 2, count 6
    "whole_map": WHOLE_MAP, "far_around": FAR_AROUND,
    "off_top_left": [-100.0, -100.0, 300.0, 300.0], "off_bottom_right": [1100.0, 600.0, 1500.0, 1000.0],
    "outside": [(W + 2) * 16.0, (H + 2) * 16.0, (W + 9) * 16.0, (H + 7) * 16.0],
}
NAMES = list(NAMED)


def single_rois():
    """The named boxes, alternating over the two images, then six random ones"""
    rng = np.random.RandomState(21)
    xy = rng.uniform(-20, [W * 14.0, H * 14.0], size=(6, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(900), size=(6, 2)))
    boxes = np.concatenate([np.array([NAMED[n] for n in NAMES]), np.concatenate([xy, xy + wh], 1)]).astype(F)
    img = (np.arange(len(boxes)) % 2).astype(F)[:, None]
    return np.concatenate([img, boxes], 1)


@functools.lru_cache(maxsize=None)
def single_reference(pooled):
    """(feat [2, 65, 50, 84], rois, ro.roi_align at sampling_ratio 0): computed once per pooled size and shared, read-only"""
    feat, rois = feature_map(), single_rois()
    want = ro.roi_align(feat, rois, SCALE, pooled, 0)
    for a in (feat, rois, want):
        a.setflags(write=False)
    return feat, rois, want


def axis_events(rois, scale, size_hw, pooled):
    """How many (ROI, bin, axis) have their skipped samples in front only, behind only, on both sides, or no valid sample at all."""
    ev = dict(prefix=0, suffix=0, both=0, nothing=0)
    for roi in np.asarray(rois, dtype=F):
        for lo, hi, size in ((roi[2], roi[4], size_hw[0]), (roi[1], roi[3], size_hw[1])):
            s, b, g = axis_grid(lo, hi, scale, pooled)
            for p in range(pooled):
                ok = axis_valid(axis_coords(s, b, p, g), size)
                if not ok.any():
                    ev["nothing"] += 1
                elif not ok[0] and not ok[-1]:
                    ev["both"] += 1
                elif not ok[0]:
                    ev["prefix"] += 1
                elif not ok[-1]:
                    ev["suffix"] += 1
    return ev


# ---- boxes on which float64 arithmetic picks another grid ------------------------------------------------------------------------------------
QUARTER = 0.25
QUARTER_HW = (128, 128)      # a [1, C, 128, 128] map at scale 1/4


def grid_rounding_draw(rng):
    """One box side drawn as y2 = y1 + 4 * 7k +- 2e-5, k = 10..16: (y1, y2, float32 grid, float64 grid) at scale 1/4 and pooled 7"""
    k = int(rng.randint(10, 17))
    y1 = F(rng.uniform(2, 30))
    y2 = F(float(y1) + 28.0 * k + (2e-5 if rng.rand() < 0.5 else -2e-5))
    return y1, y2, axis_grid(y1, y2, QUARTER, 7)[2], axis_grid(y1, y2, QUARTER, 7, "f64grid")[2]


def grid_rounding_rois(n=6):
    """Boxes on which float64 arithmetic picks another grid.  len / 7 lies within a few float32 steps of the integer k: the float32
    difference hi*scale - lo*scale rounds a length just above 7k down to 7k (one step there is 7.6e-6), so float32 takes k samples
    where float64, which keeps the excess, takes k + 1.  Only this way round AT THIS SCALE: it is a power of two, so both products
    are exact, and a monotone rounding of the difference and of the quotient cannot carry a value at or below k above it
    (tests/test_roi_adaptive_host.py counts both directions over a draw).  odd_scale_rois below has boxes that go each way.
    Returns (rois, float32 gh, float64 gh)."""
    rng = np.random.RandomState(75)
    pick = []
    while len(pick) < n:
        y1, y2, g32, g64 = grid_rounding_draw(rng)
        if g32 != g64:
            pick.append(([0.0, 8.0, float(y1), 64.0, float(y2)], g32, g64))
    return np.array([p[0] for p in pick], dtype=F), np.array([p[1] for p in pick]), np.array([p[2] for p in pick])


ODD_SCALE = 0.3              # not a power of two: lo * scale and hi * scale round in float32
ODD_HW = (72, 72)            # a [1, C, 72, 72] map at that scale


def odd_scale_draw(rng):
    """One box side drawn as y2 = y1 + 7k / 0.3 +- 5e-6, k = 1..8: (y1, y2, float32 grid, float64 grid) at scale 0.3 and pooled 7"""
    k = int(rng.randint(1, 9))
    y1 = F(rng.uniform(2, 30))
    y2 = F(float(y1) + 7.0 * k / ODD_SCALE + (5e-6 if rng.rand() < 0.5 else -5e-6))
    return y1, y2, axis_grid(y1, y2, ODD_SCALE, 7)[2], axis_grid(y1, y2, ODD_SCALE, 7, "f64grid")[2]


def odd_scale_rois(each_way=3):
    """Boxes at a scale that is no power of two, on which float64 arithmetic (on the same float32 boxes and the same float32 scale)
    picks another grid, EACH WAY: hi*scale and lo*scale are rounded in float32, each by up to half a step in either direction, so
    their difference lands on either side of 7k whatever side the exact one lies on.  Here (hi - lo) * scale, or hi*scale - lo*scale
    contracted into a fused multiply-add, are other numbers than the reference's two rounded products: at a power-of-two scale all
    these forms give the same bits.  Returns (rois, float32 gh, float64 gh): `each_way` boxes where float32 takes the larger grid,
    then as many where it takes the smaller."""
    rng = np.random.RandomState(76)
    up, down = [], []
    while len(up) < each_way or len(down) < each_way:
        y1, y2, g32, g64 = odd_scale_draw(rng)
        if g32 != g64:
            (up if g32 > g64 else down).append(([0.0, 20.0, float(y1), 200.0, float(y2)], g32, g64))
    pick = up[:each_way] + down[:each_way]
    return np.array([p[0] for p in pick], dtype=F), np.array([p[1] for p in pick]), np.array([p[2] for p in pick])


# ---- boxes whose grid is (g, g) for every ROI ------------------------------------------------------------------------------------------------
def square_grid_rois(g, pooled=7, n=6, seed=31):
    """Sides of pooled * (g - 1 + t) map pixels, t in (0.1, 0.9): ceil gives g on both axes"""
    rng = np.random.RandomState(seed + g)
    xy = rng.uniform(0, 300, size=(n, 2))
    wh = pooled * (g - 1 + rng.uniform(0.1, 0.9, size=(n, 2))) * 16.0
    img = (np.arange(n) % 2)[:, None]
    return np.concatenate([img, xy, xy + wh], 1).astype(F)


# ---- contention with an order-free answer -------------------------------------------------------------------------------------------------------
def exact_contention_case(copies=64, channels=33):
    """64 copies of [48, 32, 304, 544] at scale 1/16 and pooled 8: len 32 x 16 map pixels, bins 4 x 2, grid (4, 2), count 8, sample
    spacing exactly 1 with every coordinate at an integer + 1/2.  Every weight is 1/4 and the cotangent holds integers in [-3, 3],
    so every term (g * w) / 8 is a multiple of 2^-5 and a pixel's absolute sum stays below 2^12 (at most 4 samples x 64 copies x
    3 / 32 = 24): the float32 accumulation is exact in any order, and one lost update shows at every pixel."""
    rois = np.array([[0, 48.0, 32.0, 304.0, 544.0]] * copies, dtype=F)
    gout = np.random.RandomState(79).randint(-3, 4, size=(copies, channels, 8, 8)).astype(F)
    return (2, channels, H, W), rois, gout


# ---- four levels and the depth map; images with no ROI -----------------------------------------------------------------------------------------
def pyramid_maps(channels, depth_channels, n_img=2, seed=160):
    rng = np.random.RandomState(seed)
    feats = [(rng.randint(-64, 65, size=(n_img, channels, c16.H >> (2 + l), c16.W >> (2 + l))) / 8.0).astype(F) for l in range(4)]
    depth = (rng.randint(-64, 65, size=(n_img, depth_channels, c16.H >> 4, c16.W >> 4)) / 8.0).astype(F)
    return feats, depth


@functools.lru_cache(maxsize=None)
def pyramid_reference(pooled, channels=33, depth_channels=65):
    """roi_pool16_cases.boxes() (sub-pixel, hanging over the edges, the whole image, larger than the image, either side of every
    level boundary) through ro.pooler_forward at sampling_ratio 0"""
    feats, depth = pyramid_maps(channels, depth_channels)
    boxes = c16.boxes()
    rgb, dep, lv = ro.pooler_forward(feats, boxes, depth, scales=rc.SCALES4, pooled=pooled, sampling_ratio=0, return_levels=True)
    return feats, depth, boxes, rgb, dep, lv


EMPTY_COUNTS = (3, 0, 7, 0, 2)


@functools.lru_cache(maxsize=None)
def empty_image_reference(pooled=7):
    feats, depth = pyramid_maps(33, 1, n_img=len(EMPTY_COUNTS), seed=44)
    rng = np.random.RandomState(45)
    n = sum(EMPTY_COUNTS)
    xy = rng.uniform(-10, [c16.W * 0.8, c16.H * 0.8], size=(n, 2))
    wh = np.exp(rng.uniform(np.log(3), np.log(400), size=(n, 2)))
    boxes = np.split(np.concatenate([xy, xy + wh], 1).astype(F), np.cumsum(EMPTY_COUNTS)[:-1])
    rgb, dep, lv = ro.pooler_forward(feats, boxes, depth, scales=rc.SCALES4, pooled=pooled, sampling_ratio=0, return_levels=True)
    return feats, depth, boxes, rgb, dep, lv


def pyramid_taps_backward(g_rgb, g_dep, boxes, shapes, depth_shape, pooled):
    """taps_backward per level (the ROIs the float32 LevelMapper sends there) and for the depth map (every ROI, level 2)"""
    rois = rc.to_rois(boxes)
    lv = ro.map_levels(rois[:, 1:], 2, 5)
    per_level = []
    for l, (shape, sc) in enumerate(zip(shapes, rc.SCALES4)):
        idx = np.nonzero(lv == l)[0]
        per_level.append(taps_backward(np_adaptive_taps(rois[idx], sc, shape, pooled), g_rgb[idx]))
    dep = taps_backward(np_adaptive_taps(rois, rc.SCALES4[2], depth_shape, pooled), g_dep) if g_dep is not None else None
    return per_level, dep
