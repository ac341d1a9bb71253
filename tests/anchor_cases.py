"""What the anchor-generator tests and tests/golden/make_golden_anchors.py share: the cases, the fixture loader, the yardsticks --
`np_anchors` (synth.anchor_grid, pinned to the reference's AnchorGenerator by make_golden_rpn.check_anchors and again by the
fixtures here) and `np_visibility_plane`, a numpy restatement of anchor_generator.py:97-110 -- and the wrong restatements of the
mutation check.  No test lives here.

A case: sizes (one entry per level, a number or a tuple; with one stride: every size of the one level), strides, ratios, grids
((H, W) per level), images ((width, height) per image), thresholds (the straddle thresholds its visibility is stored for).  `big`
cases are stored as SHA-256 checksums only."""
import hashlib
import os

import numpy as np

from veto_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchors")
CLASSIC = (0.5, 1.0, 2.0)
VETO_RATIOS = (0.23232838, 0.63365731, 1.28478321, 3.15089189)        # configs/VETO_final.yaml:21
FPN_SIZES, FPN_STRIDES = (32, 64, 128, 256, 512), (4, 8, 16, 32, 64)
RETINA_STRIDES = (8, 16, 32, 64, 128)
RETINA_SIZES = tuple(tuple(2.0 ** (i / 3.0) * s for i in range(3)) for s in FPN_SIZES)      # OCTAVE 2, SCALES_PER_OCTAVE 3
OFFSET_GRIDS = ((7, 11), (4, 6), (2, 3), (1, 2), (1, 1))
# thirteen sizes that all differ; (20, 20) is smaller than every anchor of the coarsest level, (1, 1) than every anchor
THIRTEEN = ((176, 112), (200, 160), (192, 150), (44, 28), (20, 20), (1, 1), (300, 40), (40, 300), (64, 64), (65, 64), (64, 65),
            (1000, 1000), (87, 59))
THRESHOLDS = (0, 16, -1)
VETO_GRIDS = ((200, 336), (100, 168), (50, 84), (25, 42), (13, 21))
TWELVE = tuple((1344 - 16 * i, 800 - 8 * i) for i in range(12))

CASES = {
    # the classic stride-16 set of the generator's own comment (anchor_generator.py:197-207)
    "classic": dict(sizes=(128, 256, 512), strides=(16,), ratios=CLASSIC, grids=((3, 5),), images=((80, 48), (100, 56)),
                    thresholds=(0, 16)),
    "veto4": dict(sizes=FPN_SIZES, strides=FPN_STRIDES, ratios=VETO_RATIOS, grids=OFFSET_GRIDS, images=THIRTEEN[:2],
                  thresholds=THRESHOLDS),
    "retina": dict(sizes=RETINA_SIZES, strides=RETINA_STRIDES, ratios=CLASSIC, grids=((5, 7), (3, 4), (2, 3), (1, 2), (1, 1)),
                   images=((60, 44),), thresholds=(0, 16)),
    # level offsets that are no multiple of anything: 231, 72, 18, 6, 3 rows
    "offsets5": dict(sizes=FPN_SIZES, strides=FPN_STRIDES, ratios=CLASSIC, grids=OFFSET_GRIDS, images=THIRTEEN, thresholds=THRESHOLDS),
    "levels8": dict(sizes=(16, 32, 64, 128, 256, 512, 1024, 2048), strides=(2, 4, 8, 16, 32, 64, 128, 256), ratios=CLASSIC,
                    grids=OFFSET_GRIDS + ((5, 3), (2, 5), (3, 1)), images=THIRTEEN[:2], thresholds=(0,)),
    # far-edge and near-edge equalities: cells (-8, -8, 23, 23) and (-16, -16, 31, 31); see EDGE_EXPECT
    "edges": dict(sizes=(32, 48), strides=(16,), ratios=(1.0,), grids=((3, 4),),
                  images=((39, 64), (40, 64), (64, 39), (64, 40), (15, 64), (16, 64), (64, 15), (64, 16), (1, 1)), thresholds=(0, 16)),
    "wide15": dict(sizes=(32, 64, 128, 256, 512), strides=(16,), ratios=CLASSIC, grids=((38, 50),), images=((800, 608), (790, 600)),
                   thresholds=(0,), big=True),
    "retina9": dict(sizes=RETINA_SIZES, strides=RETINA_STRIDES, ratios=CLASSIC, grids=((19, 25), (10, 13), (5, 7), (3, 4), (2, 1)),
                    images=((200, 152),), thresholds=(0,), big=True),
    # VETO's geometry: 12 images padded to 800 x 1344, A = 4, 358 092 anchors
    "veto_big": dict(sizes=FPN_SIZES, strides=FPN_STRIDES, ratios=VETO_RATIOS, grids=VETO_GRIDS, images=TWELVE, thresholds=(0,), big=True),
}
# one level, A = 1: the wave and workgroup edges of a flat index
for _h, _w in ((1, 1), (1, 63), (1, 64), (1, 65), (3, 85), (16, 16), (257, 1)):
    CASES["flat_%dx%d" % (_h, _w)] = dict(sizes=(32,), strides=(8,), ratios=(1.0,), grids=((_h, _w),), images=((_w * 8, _h * 8),),
                                          thresholds=(0,))
SMALL = tuple(n for n, c in CASES.items() if not c.get("big"))

# "edges": (threshold, image, anchor row) -> visible.  Row (h W + w) A + a with W = 4, A = 2.
_R = (1 * 4 + 1) * 2          # cell (1, 1), a = 0: (8, 8, 39, 39)
EDGE_EXPECT = {
    (0, 0, _R): 0, (0, 1, _R): 1,      # x2 == width (not visible), x2 == width - 1
    (0, 2, _R): 0, (0, 3, _R): 1,      # y2 == height, y2 == height - 1
    (16, 4, 1): 0, (16, 5, 1): 1,      # cell (0, 0), a = 1: (-16, -16, 31, 31), x1 == -t exactly; x2 == width + t, then one below
    (16, 6, 1): 0, (16, 7, 1): 1,
    (0, 5, 1): 0, (0, 5, 0): 0,        # t = 0: x1 < 0
}


def generator_args(c):
    """The (sizes, aspect_ratios, anchor_strides) an AnchorGenerator takes for a case."""
    return tuple(c["sizes"]), tuple(c["ratios"]), tuple(c["strides"])


def level_sizes(c):
    """The size tuple of every level, as the generator's constructor reads `sizes`."""
    if len(c["strides"]) == 1:
        return [tuple(c["sizes"])]
    return [s if isinstance(s, tuple) else (s,) for s in c["sizes"]]


def np_anchors(c, order="hwa", stride_shift=0):
    """synth.anchor_grid for a case.  order / stride_shift: the wrong restatements of the mutation check ("wha": h and w swapped in
    the row order; "ahw": a slowest; stride_shift 1: the neighbouring level's stride)."""
    sizes, strides = level_sizes(c), list(c["strides"])
    if stride_shift:
        strides = [strides[(l + stride_shift) % len(strides)] if len(strides) > 1 else strides[0] * 2 for l in range(len(strides))]
    if order == "hwa" and not stride_shift:
        return synth.anchor_grid(sizes, strides, c["ratios"], c["grids"])
    out = []
    for size, stride, true_stride, (H, W) in zip(sizes, strides, c["strides"], c["grids"]):
        cell = synth._cell_anchors(true_stride, size, c["ratios"]).astype(np.float32)
        A = len(cell)
        h, w, a = np.meshgrid(np.arange(H), np.arange(W), np.arange(A), indexing="ij")
        shift = np.stack([w, h, w, h], -1).astype(np.float32) * np.float32(stride)
        full = shift + cell[a]                                                    # [H, W, A, 4]
        if order == "wha":
            full = full.transpose(1, 0, 2, 3)
        elif order == "ahw":
            full = full.transpose(2, 0, 1, 3)
        out.append(np.ascontiguousarray(full).reshape(-1, 4).astype(np.float32))
    return out


def np_visibility_plane(anchors, images, t, far="<", swap_size=False):
    """anchor_generator.py:97-110 per image on the float32 anchors of all levels: uint8 [n_img, total].  far / swap_size: wrong
    restatements of the mutation check (`<=` at the far edge; the image's (height, width) swapped)."""
    a = np.concatenate([np.asarray(x, np.float32) for x in anchors])
    plane = np.ones((len(images), len(a)), np.uint8)
    if t < 0:
        return plane
    lo = np.float32(-t)
    for i, (w, h) in enumerate(images):
        if swap_size:
            w, h = h, w
        xmax, ymax = np.float32(w + t), np.float32(h + t)
        near = (a[:, 0] >= lo) & (a[:, 1] >= lo)
        plane[i] = near & ((a[:, 2] <= xmax) & (a[:, 3] <= ymax) if far == "<=" else (a[:, 2] < xmax) & (a[:, 3] < ymax))
    return plane


def sha256(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def fixture_anchors(z, c):
    return [z["anchors_%d" % l] for l in range(len(c["grids"]))]
