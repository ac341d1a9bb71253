"""Premises of tests/roi_pool16_cases.py, on the CPU: the boxes reach what they are there for, and oracle/roi_align_oracle.py at
outputs of 9 x 9 to 16 x 16 equals the reference's compiled CPU kernel (tests/golden/patchgrid/roialign16.npz, made by
tests/golden/make_golden_patchgrid.py) bit for bit -- the oracle is then what the device is held to."""
import os

import numpy as np
import pytest

import roi_pool16_cases as c16
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro
from veto_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchgrid", "roialign16.npz")


def test_every_instance_fits_the_axis_tables_and_walks_more_than_one_bin():
    for p, g in c16.INSTANCES:
        assert 9 <= p <= 16 and p * g <= 32
    assert {(p * p + 63) // 64 for p, _ in c16.INSTANCES} == {2, 3, 4}
    assert max(p * g for p, g in c16.INSTANCES) == 32
    for p, g in c16.REFUSED:
        assert p > 16 or p * g > 32


def test_boxes_reach_every_level_both_sides_of_every_boundary_and_the_validity_edge():
    bx = c16.boxes()
    lv = [ro.map_levels(b) for b in bx]
    assert set(np.concatenate(lv).tolist()) == {0, 1, 2, 3}
    for i in range(3):            # the boundary pairs of image 1: the box at the boundary one level above the one a step below it
        assert lv[1][2 * i] == lv[1][2 * i + 1] + 1 == i + 1
    # sub-pixel: narrower than one pixel of their level's map, so the width is widened to 1 (:84-98)
    for b, l in zip(bx[0][:2], lv[0][:2]):
        assert (b[2] - b[0]) * rc.SCALES4[l] < 1 and (b[3] - b[1]) * rc.SCALES4[l] < 1
    # the two boxes hanging out of the image have invalid samples on their level and on the depth map, but not only invalid ones
    rois = ro.to_rois(bx)
    for r in (2, 3):
        for scale, shape in ((rc.SCALES4[lv[0][r]], (2, 1, c16.H >> (2 + lv[0][r]), c16.W >> (2 + lv[0][r]))), (rc.SCALES4[2], (2, 1, c16.H >> 4, c16.W >> 4))):
            _, n_invalid = rc.touched_pixels(rois[r:r + 1], scale, 16, 2, shape)
            assert 0 < n_invalid[0] < 32 * 32, (r, scale, n_invalid)


@pytest.mark.parametrize("pooled,ratio", c16.INSTANCES)
def test_oracle_equals_the_reference_kernel_bit_for_bit(pooled, ratio):
    want = np.load(FIXTURE)["out_p%d_r%d" % (pooled, ratio)]
    feat, rois = synth.synthetic_roi_single(pooled, ratio, channels=want.shape[1])
    got = ro.roi_align(feat, rois, rc.SCALE, pooled, ratio)
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
