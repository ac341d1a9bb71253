"""The ordered mode's summation orders (include/veto_amd.h, veto_train_opts_t.deterministic and veto_roi_pool_backward_ordered) restated in
numpy as float32 sequential sums, and the inputs on which tests/test_deterministic_gpu.py compares the device with them bit for bit.

Plain module, no test in it.  Everything is numpy on the CPU.  tests/test_deterministic_host.py proves what the comparison rests on: each
restatement lies within the any-order bound of the existing oracles; on every input below that is not marked exact, walking the pairs /
ROIs / object rows in DESCENDING order changes at least one bit (so a bit match on the device means the stated order and no other, and
the atomic path cannot pass by luck); and the inputs marked exact have order-free float32 answers.

`reverse=True` is that descending walk: the same terms, the outermost index (pair row, ROI, object row) from last to first."""
import numpy as np

import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
DIM, TOK = 576, 19


# ---- site 5: ROI pooling backward ------------------------------------------------------------------------------------------------
def roi_backward_ordered(grad_out, rois, spatial_scale, feat_shape, pooled, ratio, reverse=False):
    """Per map pixel the float32 sequential sum, from +0, of (g * w) / count over (ROI, bin row, bin column, sample iy, sample ix,
    tap 0..3) in lexicographic order, over the taps of valid samples that land on the pixel.  The terms are the oracle's
    (ro.roi_align_backward); only the accumulation differs: float32, in this order.  All channels at once: they do not interact."""
    grad_out = np.asarray(grad_out, dtype=F)
    rois = np.asarray(rois, dtype=F)
    B, C, H, W = feat_shape
    grad = np.zeros((B, C, H, W), dtype=F)
    count = F(ratio * ratio)
    order = range(len(rois) - 1, -1, -1) if reverse else range(len(rois))
    for r in order:
        b = int(rois[r, 0])
        (vy, ylo, yhi, ly, hy), (vx, xlo, xhi, lx, hx) = rc.roi_tables(rois[r], spatial_scale, pooled, ratio, H, W)
        for ph in range(pooled):
            for pw in range(pooled):
                g = grad_out[r, :, ph, pw]
                for iy in range(ratio):
                    ky = ph * ratio + iy
                    for ix in range(ratio):
                        kx = pw * ratio + ix
                        if not (vy[ky] and vx[kx]):
                            continue
                        w = (F(hy[ky] * hx[kx]), F(hy[ky] * lx[kx]), F(ly[ky] * hx[kx]), F(ly[ky] * lx[kx]))
                        taps = ((ylo[ky], xlo[kx]), (ylo[ky], xhi[kx]), (yhi[ky], xlo[kx]), (yhi[ky], xhi[kx]))
                        for wk, (yy, xx) in zip(w, taps):      # coinciding taps (low == high) both count, in tap order
                            grad[b, :, yy, xx] = grad[b, :, yy, xx] + (g * wk) / count
    return grad


def pooler_levels(rois, scales):
    if len(scales) == 1:
        return np.zeros(len(rois), dtype=np.int64)
    return ro.map_levels(rois[:, 1:], int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1]))))


def pooler_backward_ordered(case, reverse=False):
    """The ordered map gradients of a RoiCase: ([per level], depth or None).  A level sees the ROIs the float32 LevelMapper gives it,
    in their order; the depth map sees every ROI at scale[2] (scale[0] with one level)."""
    lv = pooler_levels(case.rois, case.scales)
    per_level = []
    for l, (shape, sc) in enumerate(zip(case.shapes, case.scales)):
        idx = np.nonzero(lv == l)[0]
        per_level.append(roi_backward_ordered(case.g_rgb[idx], case.rois[idx], sc, shape, case.pooled, case.ratio, reverse))
    dep = None
    if case.g_dep is not None:
        sc = case.scales[2] if len(case.scales) > 1 else case.scales[0]
        dep = roi_backward_ordered(case.g_dep, case.rois, sc, case.depth_shape, case.pooled, case.ratio, reverse)
    return per_level, dep


class RoiCase:
    def __init__(self, shapes, scales, rois, pooled, ratio, g_rgb, depth_shape=None, g_dep=None, exact=False):
        self.shapes, self.scales, self.rois = [tuple(s) for s in shapes], tuple(scales), np.asarray(rois, dtype=F)
        self.pooled, self.ratio, self.g_rgb, self.depth_shape, self.g_dep, self.exact = pooled, ratio, g_rgb, depth_shape, g_dep, exact


def _single_case(pooled, ratio, channels, seed):
    feat, rois = rc.single(pooled, ratio, channels)
    return RoiCase([feat.shape], (rc.SCALE,), rois, pooled, ratio, rc.cotangent((len(rois), channels, pooled, pooled), seed))


def _pyramid_case(n_levels, with_depth, num_objs=(11, 12), seed=rc.SEED_PYRAMID, W=512, H=320, channels=5, depth_channels=3):
    feats, depth, boxes = rc.pyramid(channels=channels, depth_channels=depth_channels, num_objs=num_objs, W=W, H=H, seed=seed)
    maps, scales = rc.level_form(feats, n_levels)
    rois = rc.to_rois(boxes)
    g_rgb = rc.cotangent((len(rois), channels, 8, 8), 300 + n_levels)
    g_dep = rc.cotangent((len(rois), depth_channels, 8, 8), 310 + n_levels) if with_depth else None
    return RoiCase([m.shape for m in maps], scales, rois, 8, 2, g_rgb, depth.shape if with_depth else None, g_dep)


def _boundary_case():
    """24 boxes around each of the three float32 level boundaries (tests/roi_pool_cases.py, section 3): of every sweep the 12 single-float32
    steps below the box at which the float32 LevelMapper steps up, and 12 from it on."""
    parts = []
    for side in rc.BOUNDARY_SIDES:
        sweep = rc.boundary_sweep(side)
        step = int(np.nonzero(np.diff(ro.map_levels(sweep)))[0][0]) + 1
        parts.append(sweep[step - 12:step + 12])
    boxes = np.concatenate(parts)
    rois = ro.to_rois([boxes])
    shapes = [(1, 2, n, n) for n in rc.BOUNDARY_MAP_SIZES]
    return RoiCase(shapes, rc.SCALES4, rois, 8, 2, rc.cotangent((len(rois), 2, 8, 8), 320))


def _far_edge_case():
    """The 6 x 5 map of rc.edge_map at scale 1, pooled 2, ratio 1: boxes whose sample centres sit at and beyond the last row and
    column, where the low and the high index are both size - 1 (taps 0..3 coincide pairwise or all four)."""
    W, H = 5, 6
    rois = np.array([[0, W - 1, H - 1, W + 3, H + 3], [0, W - 3, H - 3, W + 1, H + 1], [0, W - 2.5, H - 1, W + 1.5, H + 3],
                     [0, W - 1, H - 2.25, W + 3, H + 1.75], [0, W - 3, H - 3, W + 1, H + 1]], dtype=F)
    return RoiCase([(1, 3, H, W)], (1.0,), rois, 2, 1, rc.cotangent((len(rois), 3, 2, 2), 321))


def _contention(exact):
    shape, rois, gout = rc.exact_contention_case() if exact else rc.contention_case()
    return RoiCase([shape], (rc.SCALE,), rois, 8, 2, gout, exact=exact)


ROI_CASES = {
    "contention_64_copies": lambda: _contention(False),
    "exact_contention": lambda: _contention(True),
    "ratio1": lambda: _single_case(8, 1, 33, 201), "ratio2": lambda: _single_case(8, 2, 33, 202),
    "ratio3": lambda: _single_case(8, 3, 33, 203), "ratio4": lambda: _single_case(8, 4, 33, 204),
    "pooled1": lambda: _single_case(1, 2, 33, 205), "pooled7": lambda: _single_case(7, 2, 33, 206),
    "channels1": lambda: _single_case(8, 2, 1, 207), "channels32": lambda: _single_case(8, 2, 32, 208),
    "channels65": lambda: _single_case(8, 2, 65, 209),
    "levels4_depth": lambda: _pyramid_case(4, True), "levels3_depth": lambda: _pyramid_case(3, True),
    "levels1_depth": lambda: _pyramid_case(1, True), "levels4": lambda: _pyramid_case(4, False),
    "levels3": lambda: _pyramid_case(3, False), "levels1": lambda: _pyramid_case(1, False),
    "empty_image": lambda: _pyramid_case(4, True, num_objs=rc.EMPTY_COUNTS, seed=rc.SEED_EMPTY),
    "level_boundaries": _boundary_case,
    "far_edge": _far_edge_case,
}
# ("ratio2" is also pooled 8 and 33 channels: the far side of the 32-channel slab)


# ---- site 1: token-assembly backward -------------------------------------------------------------------------------------------------
def assemble_backward_ordered(dx, subj, obj, lc, n_obj, reverse=False):
    """dpatch [n_obj, 16, 1152], dlc [n_obj, 2, 1152]: per object row, token and half (subject | object) the float32 sequential sum, from
    +0, of the token-gradient rows of the pairs, in ascending pair row, whose subject / object it is; dlc with the ReLU gate
    lc[subject, w, :576] + lc[object, w, 576:] > 0 per element.  dx [n_pair, 19, 576]; subj / obj: batch-wide object rows."""
    dx = np.asarray(dx, dtype=F).reshape(-1, TOK, DIM)
    lc = np.asarray(lc, dtype=F).reshape(n_obj, 2, 2 * DIM)
    dpatch = np.zeros((n_obj, 16, 2 * DIM), dtype=F)
    dlc = np.zeros((n_obj, 2, 2 * DIM), dtype=F)
    order = range(len(subj) - 1, -1, -1) if reverse else range(len(subj))
    for p in order:
        s, o = int(subj[p]), int(obj[p])
        g = dx[p, 1:17]
        dpatch[s, :, :DIM] = dpatch[s, :, :DIM] + g
        dpatch[o, :, DIM:] = dpatch[o, :, DIM:] + g
        gate = (lc[s, :, :DIM] + lc[o, :, DIM:]) > 0
        g = np.where(gate, dx[p, 17:19], F(0))      # (x + 0 == x in float32, -0 aside: a sum that starts from +0 never holds -0)
        dlc[s, :, :DIM] = dlc[s, :, :DIM] + g
        dlc[o, :, DIM:] = dlc[o, :, DIM:] + g
    return dpatch, dlc


class AssembleCase:
    def __init__(self, num_objs, pairs, seed, single_term=False):
        """pairs: per image [P_i, 2] image-local object indices.  single_term: no destination receives more than two terms, so every order
        gives the same bits (a + b == b + a) and the descending walk cannot differ."""
        self.num_objs, self.pairs, self.single_term = list(num_objs), [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs], single_term
        self.obj_off = np.concatenate([[0], np.cumsum(self.num_objs)]).astype(np.int32)
        self.pair_off = np.concatenate([[0], np.cumsum([len(p) for p in self.pairs])]).astype(np.int32)
        self.subj = np.concatenate([p[:, 0] + o for p, o in zip(self.pairs, self.obj_off)]).astype(np.int32)
        self.obj = np.concatenate([p[:, 1] + o for p, o in zip(self.pairs, self.obj_off)]).astype(np.int32)
        self.n_obj, self.n_pair = int(self.obj_off[-1]), int(self.pair_off[-1])
        rng = np.random.RandomState(seed)
        self.dx = rng.randn(self.n_pair, TOK, DIM).astype(F)
        self.lc = rng.randn(self.n_obj, 2, 2 * DIM).astype(F)


def _drawn_pairs(n_obj, n_pair, seed):
    rng = np.random.RandomState(seed)
    s = rng.randint(0, n_obj, size=n_pair)
    o = (s + 1 + rng.randint(0, n_obj - 1, size=n_pair)) % n_obj
    return np.stack([s, o], 1)


def _one_subject_pairs(n_pair):
    """Object 0 is the subject of every pair; the objects 1..7 take turns on the other side."""
    return np.stack([np.zeros(n_pair, dtype=np.int64), 1 + np.arange(n_pair) % 7], 1)


def _hand_case():
    from train_dropout_cases import HAND_OBJS, HAND_PAIRS
    return AssembleCase(HAND_OBJS, HAND_PAIRS, 401)


# seeds: the first tried; tests/test_deterministic_host.py asserts that the descending walk differs on each (those with three terms somewhere)
ASSEMBLE_CASES = {
    "hand_pairs": _hand_case,                                                            # gaps, a one-sided object, a repeated pair, two images
    "pairs1": lambda: AssembleCase([3], [[[2, 0]]], 402, single_term=True),
    "pairs15": lambda: AssembleCase([4], [_drawn_pairs(4, 15, 1)], 403),                 # one side and the other of the scatter kernel's
    "pairs16": lambda: AssembleCase([4], [_drawn_pairs(4, 16, 2)], 404),                 # 16 token rows per workgroup
    "pairs17": lambda: AssembleCase([4], [_drawn_pairs(4, 17, 3)], 405),
    "one_subject_1024": lambda: AssembleCase([8], [_one_subject_pairs(1024)], 406),
    "two_images": lambda: AssembleCase([5, 6], [_drawn_pairs(5, 23, 4), _drawn_pairs(6, 31, 5)], 407),      # offsets that are not zero
}


# ---- site 2: embedding scatter -----------------------------------------------------------------------------------------------------
def scatter_rows_ordered(demb, labels, n_table_rows, reverse=False):
    """dE[label] = the float32 sequential sum, from +0, over the object rows that carry the label, in ascending row."""
    demb = np.asarray(demb, dtype=F)
    out = np.zeros((n_table_rows, demb.shape[1]), dtype=F)
    order = range(len(labels) - 1, -1, -1) if reverse else range(len(labels))
    for n in order:
        out[labels[n]] = out[labels[n]] + demb[n]
    return out


class ScatterCase:
    def __init__(self, labels, n_table_rows, dim, seed, single_term=False):
        self.labels, self.n_table_rows, self.dim, self.single_term = np.asarray(labels, dtype=np.int64), n_table_rows, dim, single_term
        self.demb = np.random.RandomState(seed).randn(len(self.labels), dim).astype(F)


SCATTER_CASES = {
    "one_label_432_rows": lambda: ScatterCase(np.full(432, 17), 151, 200, 501),
    "all_distinct": lambda: ScatterCase(np.random.RandomState(502).permutation(151)[:120], 151, 200, 502, single_term=True),
    "drawn_labels": lambda: ScatterCase(np.random.RandomState(503).randint(0, 151, size=432), 151, 200, 503),
}
