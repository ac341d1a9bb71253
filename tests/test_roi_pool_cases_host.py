"""Premises of the inputs of tests/test_roi_pool_gpu.py (CPU): what each case is built to reach is asserted here against the oracle
alone, and every wrong restatement of the oracle kept in tests/roi_pool_cases.py must differ from the right one on the inputs that
are meant to catch it -- so a device that computes the wrong form cannot pass the GPU module."""
import os

import numpy as np
import pytest

import roi_pool_cases as rc
from oracle import roi_align_oracle as ro
from veto_amd import synth

F = np.float32


# ---- section 1: the oracle at the new (pooled, ratio) pairs is the executed reference, bit for bit ---------------------------------
@pytest.mark.parametrize("pooled,ratio", synth.ROI_SINGLE_CASES_MORE)
def test_oracle_matches_the_reference_kernel_at_the_new_pairs(pooled, ratio):
    """tests/golden/roialign_single.npz holds the reference's own compiled CPU kernel on these inputs (make_golden.py::run_roialign)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roialign_single.npz"))
    feat, rois = synth.synthetic_roi_single(pooled, ratio, channels=6)
    assert np.array_equal(rois, g["rois_p%d_r%d" % (pooled, ratio)])
    want = g["out_p%d_r%d" % (pooled, ratio)]
    got = ro.roi_align(feat, rois, rc.SCALE, pooled, ratio)
    assert got.shape == want.shape == (23, 6, pooled, pooled) and np.array_equal(got, want)
    assert (want[1] == 0).any()      # the mostly-outside ROI exercises the out-of-map branch


def test_the_new_pairs_are_the_forward_instances_of_the_device_module():
    assert synth.ROI_SINGLE_CASES_MORE == rc.FORWARD_INSTANCES and not set(synth.ROI_SINGLE_CASES_MORE) & set(synth.ROI_SINGLE_CASES)


# ---- sections 1 / 8: the variant machinery restates the oracle exactly ------------------------------------------------------------
@pytest.mark.parametrize("pooled,ratio", [(8, 2), (5, 3), (1, 4)])
def test_variant_none_is_the_oracle(pooled, ratio):
    feat, rois = rc.single(pooled, ratio, 3)
    assert np.array_equal(rc.variant_roi_align(feat, rois, rc.SCALE, pooled, ratio), ro.roi_align(feat, rois, rc.SCALE, pooled, ratio))
    assert np.array_equal(rc.variant_roi_align(rc.edge_map(), rc.edge_rois(), 1.0, 2, 1), ro.roi_align(rc.edge_map(), rc.edge_rois(), 1.0, 2, 1))


def test_forward_instances_fill_the_axis_tables_and_idle_most_lanes():
    assert max(p * r for p, r in rc.FORWARD_INSTANCES) == 32 and (8, 4) in rc.FORWARD_INSTANCES      # kMaxAxis, last entry
    assert {r for _, r in rc.FORWARD_INSTANCES} | {2} == {1, 2, 3, 4}                                 # every template instance
    assert min(p * p for p, _ in rc.FORWARD_INSTANCES) == 1                                           # 63 of 64 lanes return early
    assert {c % 32 for c in rc.FORWARD_CHANNELS} >= {0, 1, 31} and max(rc.FORWARD_CHANNELS) > 64      # slab tails, three slabs
    assert {r for _, r in rc.BACKWARD_INSTANCES} == {1, 2, 3, 4}
    for pooled, ratio in rc.FORWARD_INSTANCES:      # the fixed boxes keep their roles at every shape: ROI 1 has samples outside
        feat, rois = rc.single(pooled, ratio, 1)
        _, n_invalid = rc.touched_pixels(rois, rc.SCALE, pooled, ratio, feat.shape)
        assert n_invalid[1] > 0 and (n_invalid == 0).any()


# ---- section 2 ------------------------------------------------------------------------------------------------------------------------
def test_pyramid_reaches_every_level_and_the_clamp_at_three_levels():
    feats, depth, boxes = rc.pyramid(channels=3, depth_channels=2)
    allb = np.concatenate(boxes)
    lv4 = ro.map_levels(allb)
    assert np.bincount(lv4, minlength=4).min() >= 3
    lv3 = ro.map_levels(allb, 2, 4)
    assert (lv3[lv4 == 3] == 2).all() and (lv3[lv4 < 3] == lv4[lv4 < 3]).all()       # the large boxes land on level index 2
    rois = ro.to_rois(boxes)
    for n_levels in (4, 3, 1):
        maps, scales = rc.level_form(feats, n_levels)
        rgb, dep, lv = ro.pooler_forward(maps, boxes, depth, scales=scales, return_levels=True)
        want_lv = {4: lv4, 3: lv3, 1: np.zeros(len(rois), dtype=np.int64)}[n_levels]
        assert np.array_equal(lv, want_lv)
        for r in range(len(rois)):
            assert np.array_equal(rgb[r], ro.roi_align(maps[lv[r]], rois[r:r + 1], scales[lv[r]])[0])
        assert np.array_equal(dep, ro.roi_align(depth, rois, scales[2] if n_levels > 1 else scales[0]))
    with pytest.raises(ValueError, match="depth pooler is level 2"):
        ro.pooler_forward(feats[:2], boxes, depth, scales=rc.SCALES4[:2])
    # the channel counts do not move the boxes
    assert all(np.array_equal(a, b) for a, b in zip(boxes, rc.pyramid(channels=5, depth_channels=9)[2]))


# ---- section 3 ------------------------------------------------------------------------------------------------------------------------
def test_boundary_sweeps_cross_their_level_step_and_separate_float32_from_float64():
    boxes = rc.boundary_boxes()
    assert boxes.shape == (579, 4)
    lv32, lv64 = ro.map_levels(boxes), rc.map_levels_f64(boxes)
    differ = 0
    for i, s in enumerate(rc.BOUNDARY_SIDES):
        sl = slice(193 * i, 193 * (i + 1))
        x2 = boxes[sl, 2]
        assert (np.diff(x2) > 0).all() and x2[128] == F(3 + s - 1)
        assert np.array_equal(x2[1:], np.nextafter(x2[:-1], F(np.inf)))                  # single float32 steps
        assert set(lv32[sl].tolist()) == {i, i + 1}                                       # both neighbouring levels
        assert (np.diff(lv32[sl]) >= 0).all()                                             # monotone in x2
        differ += int((lv32[sl] != lv64[sl]).sum())
    assert differ >= 1, "no box tells the float32 level from the float64 one"              # here: 5 + 3 + 7
    # the boxes lie inside the map of EVERY level at that level's scale, so every sample is valid and reads the constant
    for n, sc in zip(rc.BOUNDARY_MAP_SIZES, rc.SCALES4):
        assert float(boxes[:, 2:].max()) * sc <= n and float(boxes[:, :2].min()) * sc >= 0      # valid is [-1, size]
    for l, m in enumerate(rc.boundary_maps()):
        assert m.shape == (1, 2, rc.BOUNDARY_MAP_SIZES[l], rc.BOUNDARY_MAP_SIZES[l]) and (m == l + 1).all()
    # ... and the oracle pooler agrees that the output names the level (a sample of the sweep: the full sweep runs on the device)
    pick = np.r_[0:579:37, 128, 321, 514]
    rgb, _ = ro.pooler_forward(rc.boundary_maps(), [boxes[pick]])
    assert np.array_equal(rgb, np.broadcast_to((lv32[pick] + 1).astype(F)[:, None, None, None], rgb.shape))


# ---- section 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_edge_samples_literal_values():
    out = ro.roi_align(rc.edge_map(), rc.edge_rois(), 1.0, pooled=2, sampling_ratio=1).reshape(6, 4)
    rois = rc.edge_rois()
    assert rois[2, 1] == F(-2.0000002) and rois[2, 1] < -2 and rois[4, 1] > 4 and rois[5, 2] > 5
    assert out[0].tolist() == [1.0, 2.0, 6.0, 7.0]                        # centre at exactly -1: valid, clamped to index 0
    assert out[1].tolist() == [30.0, 0.0, 0.0, 0.0]                       # centre at exactly W and H: valid, last row and column
    assert np.array_equal(out[2], np.array([0, 1.9999998, 0, 6.9999995], dtype=F))      # x centre below -1: column 0 contributes 0
    assert np.array_equal(out[3], np.array([0, 0, 5.999999, 6.9999986], dtype=F))       # y centre below -1: row 0 contributes 0
    assert out[4].tolist() == [0.0] * 4 and out[5].tolist() == [0.0] * 4  # one step past W / past H: nothing is left
    hand = ro.roi_align(rc.hand_map(), rc.HAND_ROIS, 1.0, pooled=2, sampling_ratio=1).reshape(4, 4)
    assert hand.tolist() == rc.HAND_WANT
    hand1 = ro.roi_align(rc.hand_map() + F(1), rc.HAND_ROIS, 1.0, pooled=2, sampling_ratio=1).reshape(4, 4)
    assert hand1.tolist() == rc.HAND_WANT_PLUS1


# ---- section 5 ------------------------------------------------------------------------------------------------------------------------
def test_leak_case_premises():
    feat, poisoned, rois = rc.leak_case()
    touched, n_invalid = rc.touched_pixels(rois, rc.SCALE, 8, 2, feat.shape)
    assert (n_invalid > 0).sum() >= 2                       # plane[0] is really read
    assert not touched[:, 0, 0].any()                       # ... and by no valid sample
    assert np.isnan(poisoned[:, :, 0, 0]).all()
    free = ~touched
    free[:, 0, 0] = False
    assert np.isinf(poisoned[np.broadcast_to(free[:, None], feat.shape)]).all() and free.sum() > 100
    assert np.array_equal(poisoned[np.broadcast_to(touched[:, None], feat.shape)], feat[np.broadcast_to(touched[:, None], feat.shape)])
    clean = ro.roi_align(feat, rois, rc.SCALE, 8, 2)
    assert np.isfinite(clean).all() and np.array_equal(ro.roi_align(poisoned, rois, rc.SCALE, 8, 2), clean)
    shape, brois, gout, k = rc.leak_backward_case()
    _, inv = rc.touched_pixels(brois[k:k + 1], rc.SCALE, 8, 2, shape)
    assert inv[0] == 16 * 16 and np.isnan(gout[k]).all() and int(brois[k, 0]) in (0, 1)
    keep = np.arange(len(brois)) != k
    with_nan = ro.roi_align_backward(gout, brois, rc.SCALE, shape, 8, 2)
    assert np.array_equal(with_nan, ro.roi_align_backward(gout[keep], brois[keep], rc.SCALE, shape, 8, 2))


# ---- section 6 ------------------------------------------------------------------------------------------------------------------------
def test_backward_stats_and_bound():
    pooled, ratio = 7, 2
    feat, rois = rc.single(pooled, ratio, 4)
    g = rc.cotangent((23, 4, pooled, pooled), 1)
    want, K, A = ro.roi_align_backward(g, rois, rc.SCALE, feat.shape, pooled, ratio, stats=True)
    assert np.array_equal(want, ro.roi_align_backward(g, rois, rc.SCALE, feat.shape, pooled, ratio))
    _, n_invalid = rc.touched_pixels(rois, rc.SCALE, pooled, ratio, feat.shape)
    assert K.sum() == 4 * (23 * (pooled * ratio) ** 2 - n_invalid.sum())           # four taps per valid sample
    touched, _ = rc.touched_pixels(rois, rc.SCALE, pooled, ratio, feat.shape)
    assert np.array_equal(K > 0, touched) and (K == 0).mean() > 0.5
    zero = np.broadcast_to((K == 0)[:, None], want.shape)
    assert not want[zero].any() and not A[zero].any() and (np.abs(want) <= A * (1 + 1e-12)).all()
    # the right answer rounded to float32 passes, below the bound
    ratio_ok, kmax = rc.check_backward(want.astype(F), want, K, A)
    assert ratio_ok <= 1.0 and kmax == K.max() > 100
    # a float32 accumulation in another order passes as well: here every map pixel summed ROI by ROI, last ROI first
    acc = np.zeros(want.shape, dtype=F)
    for r in range(22, -1, -1):
        acc = acc + ro.roi_align_backward(g[r:r + 1], rois[r:r + 1], rc.SCALE, feat.shape, pooled, ratio).astype(F)
    # (the per-ROI partial sums were rounded once more each: K + 23 roundings at most, so twice the bound covers it)
    err, bound = np.abs(acc.astype(np.float64) - want), rc.backward_bound(want, K, A)
    assert (err <= 2 * bound).all()
    # one lost update on the most lightly loaded pixel, and one stray write on a pixel nothing touches, are both caught
    b, y, x = np.argwhere(K == K[K > 0].min())[0]
    lost = want.copy()
    lost[b, 0, y, x] -= A[b, 0, y, x] / K[b, y, x]
    assert rc.check_backward(lost.astype(F), want, K, A)[0] > 1000
    b, y, x = np.argwhere(K == 0)[0]
    stray = want.astype(F)
    stray[b, 1, y, x] = F(1e-7)
    with pytest.raises(AssertionError, match="no sample touches"):
        rc.check_backward(stray, want, K, A)


def test_contention_case_piles_its_adds_on_nine_pixels_and_what_the_bound_can_see_there():
    shape, rois, g = rc.contention_case(channels=2)
    want, K, A = ro.roi_align_backward(g, rois, rc.SCALE, shape, 8, 2, stats=True)
    # per copy: 64 bins x 4 samples x 4 taps = 1024 adds per plane, all of them into 3 x 3 pixels, 256 into the middle one
    assert (K > 0).sum() == 9 and K.sum() == 64 * 1024 and K[0, 2:5, 1:4].sum() == K.sum()
    assert sorted(K[K > 0].tolist()) == [896, 1152, 2048, 6272, 7168, 8064, 9216, 14336, 16384]
    # What the derived bound can see of ONE lost update of average size (A / K) at a pixel: A / K against gamma_K A ~ K u A, a ratio of
    # 1 / (K^2 u).  It exceeds the bound at the three pixels with K <= 2 048 (4 x, 13 x, 21 x) and stays below it at the other six:
    # 0.06 at the 16 384-add pixel, where about K^2 u = 16 lost updates are needed.  This case therefore holds the kernel to the
    # any-order rounding bound under contention and catches a lost update at the lightly loaded pixels only; a single lost update
    # at EVERY pixel is what the exact case below catches.
    bound = rc.backward_bound(want, K, A)
    for y, x in np.argwhere(K[0] > 0):
        one_lost = (A[0, :, y, x] / K[0, y, x]) / bound[0, :, y, x]
        k = int(K[0, y, x])
        assert (one_lost > 3.9).all() if k <= 2048 else (one_lost < 0.5).all(), (k, one_lost)
        assert np.allclose(one_lost, 1.0 / (k * k * rc.U), rtol=0.01)
    assert 64 * 256 * 64 * 256 * rc.U == 16.0


def test_exact_contention_case_has_an_order_free_float32_answer():
    shape, rois, g = rc.exact_contention_case(channels=3)
    want, K, A = ro.roi_align_backward(g, rois, rc.SCALE, shape, 8, 2, stats=True)
    assert (K > 0).sum() == 4 and (K[0, 3:5, 2:4] == 16384).all()                      # the same four pixels, 16 384 adds each
    assert set(np.unique(g).tolist()) == {-3, -2, -1, 0, 1, 2, 3}
    # every term is a multiple of 2^-12 and the absolute sum at a pixel is below 2^12: every partial sum, in any order, is a float32
    (vy, _, _, ly, hy), (vx, _, _, lx, hx) = rc.roi_tables(rois[0], rc.SCALE, 8, 2, shape[2], shape[3])
    assert vy.all() and vx.all()
    for t in (ly, hy, lx, hx):
        assert np.array_equal(t * 32, np.rint(t * 32)) and (t > 0).all() and (t < 1).all()
    assert A.max() < 2.0 ** 12 and A.max() <= 64 * 16 * 3
    assert np.array_equal(want * 2.0 ** 12, np.rint(want * 2.0 ** 12)) and np.array_equal(want.astype(F).astype(np.float64), want)
    # ... shown on the 4 x 3 x 16 384 terms themselves: float32 running sums in three orders all equal the float64 sum
    terms = []
    for r in range(len(rois)):
        for ky in range(16):
            for kx in range(16):
                gg = g[r, :, ky // 2, kx // 2]
                terms.append([gg * F(hy[ky] * hx[kx]) / F(4), gg * F(hy[ky] * lx[kx]) / F(4), gg * F(ly[ky] * hx[kx]) / F(4), gg * F(ly[ky] * lx[kx]) / F(4)])
    terms = np.array(terms, dtype=F)                                                      # [16384, 4 taps, C]
    assert terms.dtype == np.float32 and np.array_equal(terms * 4096, np.rint(terms * 4096))
    exact = terms.astype(np.float64).sum(0)                                                # [4, C]
    assert np.array_equal(exact.T.reshape(3, 2, 2), want[0, :, 3:5, 2:4])
    order = np.random.RandomState(0).permutation(len(terms))
    for seq in (terms, terms[::-1], terms[order]):
        assert np.array_equal(np.cumsum(seq, axis=0, dtype=F)[-1].astype(np.float64), exact)
    # one lost update of the smallest nonzero term moves the answer
    nz = np.abs(terms[terms != 0]).min()
    assert nz >= 2.0 ** -12 and (exact - nz != exact).all()


# ---- section 7 ------------------------------------------------------------------------------------------------------------------------
def test_empty_image_case_skips_the_empty_images_in_the_roi_rows():
    feats, depth, boxes = rc.empty_image_case()
    assert tuple(len(b) for b in boxes) == rc.EMPTY_COUNTS and feats[0].shape[0] == 5
    rois = rc.to_rois(boxes)
    assert rois[:, 0].tolist() == [0] * 3 + [2] * 7 + [4] * 2
    lv = ro.map_levels(rois[:, 1:])
    assert np.bincount(lv, minlength=4).tolist()[3] == 0 and np.bincount(lv, minlength=4)[:3].min() >= 2     # level 3 gets no ROI


# ---- section 8 ------------------------------------------------------------------------------------------------------------------------
def test_every_wrong_variant_differs_on_the_inputs_meant_for_it():
    # 1 (aligned) and 4 (fused four-term sum): the random single-map case at the shapes of section 1
    for pooled, ratio in [(8, 3), (5, 3), (1, 1)]:
        feat, rois = rc.single(pooled, ratio, 4)
        right = ro.roi_align(feat, rois, rc.SCALE, pooled, ratio)
        for v in ("aligned", "fused"):
            wrong = rc.variant_roi_align(feat, rois, rc.SCALE, pooled, ratio, v)
            assert (wrong != right).mean() > 0.05, (v, pooled, ratio)
    # 2 (>= at the far edge): the exact-edge box, and only the far-edge rows of it
    right = ro.roi_align(rc.edge_map(), rc.edge_rois(), 1.0, 2, 1)
    wrong = rc.variant_roi_align(rc.edge_map(), rc.edge_rois(), 1.0, 2, 1, "far_ge")
    assert (wrong != right).reshape(6, 4).any(1).tolist() == [False, True, False, False, False, False] and wrong[1].max() == 0
    wrong = rc.variant_roi_align(rc.hand_map(), rc.HAND_ROIS, 1.0, 2, 1, "far_ge")
    assert np.array_equal(wrong, ro.roi_align(rc.hand_map(), rc.HAND_ROIS, 1.0, 2, 1))      # the older hand cases cannot see it
    # 3 (mask by multiplication): the poisoned map
    feat, poisoned, rois = rc.leak_case(channels=4)
    right = ro.roi_align(poisoned, rois, rc.SCALE, 8, 2)
    wrong = rc.variant_roi_align(poisoned, rois, rc.SCALE, 8, 2, "mask_mul")
    assert np.isnan(wrong).any() and not np.isnan(right).any()
    assert np.array_equal(rc.variant_roi_align(feat, rois, rc.SCALE, 8, 2, "mask_mul"), right)  # the clean map cannot see it
    # 5 (level in float64): the boundary sweeps
    boxes = rc.boundary_boxes()
    assert (rc.map_levels_f64(boxes) != ro.map_levels(boxes)).any()
    # 6 (backward without / count): beyond the bound of section 6 at every ratio above 1
    for pooled, ratio in [pr for pr in rc.BACKWARD_INSTANCES if pr[1] > 1]:      # (count = 1 at ratio 1: nothing to leave out)
        feat, rois = rc.single(pooled, ratio, 2)
        g = rc.cotangent((23, 2, pooled, pooled), 6)
        want, K, A = ro.roi_align_backward(g, rois, rc.SCALE, feat.shape, pooled, ratio, stats=True)
        wrong = rc.backward_without_count(g, rois, rc.SCALE, feat.shape, pooled, ratio)
        assert rc.check_backward(wrong, want, K, A)[0] > 1e6, (pooled, ratio)
