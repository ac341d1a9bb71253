"""Inputs of the ROI pooling tests for outputs of 9 x 9 to 16 x 16 (tests/test_roi_pool16_gpu.py on the device,
tests/test_roi_pool16_cases_host.py for their premises).  Plain module; numpy on the CPU only.

A lane of roi_pool_kernel walks ceil(P*P / 64) bins for P > 8: 2 at P = 9..11, 3 at P = 12, 13, 4 at P = 14..16; the last pass is
partial except at P = 16.  The per-ROI axis tables hold P * G <= 32 entries: (16, 2), (10, 3) and (16, 1) fill 32, 30 and 16 of them."""
import numpy as np

import deterministic_cases as dc
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
# (pooled, sampling_ratio): the four the issue names, then the partial last pass at four passes (15, 2) and the largest ratio-3 table (10, 3)
INSTANCES = [(16, 2), (12, 2), (9, 3), (16, 1), (15, 2), (10, 3)]
CHANNELS = [1, 33, 65]                      # one wave's worth, a slab + 1, two slabs + 1
REFUSED = [(17, 1), (17, 2), (11, 3), (9, 4), (16, 3)]      # P = 17; P * G = 33, 36, 48
W, H = 512, 320                             # image; maps 128 x 80, 64 x 40, 32 x 20, 16 x 10, depth 32 x 20


def boxes():
    """Two images.  Image 0: sub-pixel boxes (one inside a pixel, one straddling pixel borders), a box hanging out of the image at the
    top left and one at the bottom right (samples below -1 and beyond the map size: the validity edge, on every level they map to),
    the whole image, and a box far larger than it (level 3).  Image 1: pairs of boxes at and 128 float32 steps below the level
    boundaries sqrt(area) = 112, 224, 448, and four random boxes."""
    def below(v, steps=128):      # (LevelMapper's 1e-6 and the float32 sqrt / log2 blur the boundary by a few steps: roi_pool_cases.boundary_sweep)
        v = F(v)
        for _ in range(steps):
            v = np.nextafter(v, F(-np.inf), dtype=F)
        return float(v)
    img0 = [[30.2, 40.7, 30.3, 40.8], [31.9, 47.9, 32.1, 48.1], [-40.0, -25.0, 30.0, 22.0], [470.0, 290.0, 560.0, 350.0],
            [0.0, 0.0, 511.0, 319.0], [-100.0, -100.0, 700.0, 500.0], [5.0, 7.0, 11.0, 9.0]]
    img1 = []
    for s in rc.BOUNDARY_SIDES:
        img1.append([3.0, 5.0, 3.0 + s - 1, 5.0 + s - 1])
        img1.append([3.0, 5.0, below(3.0 + s - 1), 5.0 + s - 1])
    rng = np.random.RandomState(16)
    xy = rng.uniform(0, 300, (4, 2))
    wh = rng.uniform(8, 200, (4, 2))
    img1 += np.concatenate([xy, xy + wh], axis=1).tolist()
    return [np.array(img0, dtype=F), np.array(img1, dtype=F)]


def pyramid(channels, depth_channels, seed=160):
    rng = np.random.RandomState(seed)
    feats = [rng.randn(2, channels, H >> (2 + l), W >> (2 + l)).astype(F) for l in range(4)]
    depth = rng.randn(2, depth_channels, H >> 4, W >> 4).astype(F)
    return feats, depth


def depth_channels_for(channels):
    return {1: 33, 33: 65, 65: 1}[channels]      # never the pyramid's count: the two launch halves have grids of their own


def roi_case(pooled, ratio, channels, seed=7):
    """deterministic_cases.RoiCase of the pyramid: shapes, rois and the two cotangents"""
    dch = depth_channels_for(channels)
    bx = boxes()
    n = sum(len(b) for b in bx)
    shapes = [(2, channels, H >> (2 + l), W >> (2 + l)) for l in range(4)]
    return dc.RoiCase(shapes, rc.SCALES4, ro.to_rois(bx), pooled, ratio, rc.cotangent((n, channels, pooled, pooled), seed),
                      depth_shape=(2, dch, H >> 4, W >> 4), g_dep=rc.cotangent((n, dch, pooled, pooled), seed + 1))
