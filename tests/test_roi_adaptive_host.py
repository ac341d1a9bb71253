"""The adaptive-grid ROI pooling tests' own ground, on the CPU: the tap-list restatement of tests/roi_adaptive_cases.py is held to
oracle/roi_align_oracle.py (forward bit for bit on every case; backward bit for bit against the fixed ratio 2 where every grid is
(2, 2)), the kernel's bisection selects exactly the samples the per-sample validity test selects, every case contains the event it is
named for, and five wrong restatements each change an expected output.  tests/test_roi_adaptive_gpu.py runs the same inputs on the
device."""
import numpy as np
import pytest

import roi_adaptive_cases as ac
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ---- the restatement is proved ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", ac.POOLED)
def test_tap_list_forward_equals_the_oracle_bit_for_bit(pooled):
    feat, rois, want = ac.single_reference(pooled)
    got = ac.apply_taps(ac.np_adaptive_taps(rois, ac.SCALE, feat.shape, pooled), feat[:, :5])
    assert np.array_equal(_bits(got), _bits(want[:, :5]))


def test_tap_list_forward_equals_the_oracle_on_the_other_cases():
    rois, _, _ = ac.grid_rounding_rois()
    feat = ac.feature_map(3, seed=6, shape=(1,) + ac.QUARTER_HW)
    got = ac.apply_taps(ac.np_adaptive_taps(rois, ac.QUARTER, feat.shape, 7), feat)
    assert np.array_equal(_bits(got), _bits(ro.roi_align(feat, rois, ac.QUARTER, 7, 0)))
    rois, _, _ = ac.odd_scale_rois()
    feat = ac.feature_map(3, seed=8, shape=(1,) + ac.ODD_HW)
    got = ac.apply_taps(ac.np_adaptive_taps(rois, ac.ODD_SCALE, feat.shape, 7), feat)
    assert np.array_equal(_bits(got), _bits(ro.roi_align(feat, rois, ac.ODD_SCALE, 7, 0)))
    feat = ac.feature_map(3)
    for g in (1, 2, 3, 4):
        rois = ac.square_grid_rois(g)
        got = ac.apply_taps(ac.np_adaptive_taps(rois, ac.SCALE, feat.shape, 7), feat)
        assert np.array_equal(_bits(got), _bits(ro.roi_align(feat, rois, ac.SCALE, 7, 0))), g
        assert np.array_equal(_bits(got), _bits(ro.roi_align(feat, rois, ac.SCALE, 7, g))), g      # and the fixed ratio g
    shape, rois, _ = ac.exact_contention_case(copies=2, channels=3)
    got = ac.apply_taps(ac.np_adaptive_taps(rois, ac.SCALE, shape, 8), feat)
    assert np.array_equal(_bits(got), _bits(ro.roi_align(feat, rois, ac.SCALE, 8, 0)))


def test_tap_list_backward_equals_the_fixed_ratio_2_where_every_grid_is_2x2():
    rois = ac.square_grid_rois(2)
    shape = (2, 3, ac.H, ac.W)
    t = ac.np_adaptive_taps(rois, ac.SCALE, shape, 7)
    assert (t.grid == 2).all() and (t.count == 4).all()
    gout = rc.cotangent((len(rois), 3, 7, 7), 9)
    grad, K, A = ac.taps_backward(t, gout)
    want, wK, wA = ro.roi_align_backward(gout, rois, ac.SCALE, shape, 7, 2, stats=True)
    assert np.array_equal(K, wK) and K.max() > 1
    assert np.array_equal(grad.view(np.int64), want.view(np.int64)) and np.array_equal(A.view(np.int64), wA.view(np.int64))


def _all_axes():
    """(start, bin, g, size, pooled) of every ROI axis of every single-map case"""
    for pooled in ac.POOLED:
        for roi in ac.single_rois():
            for lo, hi, size in ((roi[2], roi[4], ac.H), (roi[1], roi[3], ac.W)):
                yield ac.axis_grid(lo, hi, ac.SCALE, pooled) + (size, pooled)
    for roi in ac.grid_rounding_rois()[0]:
        for lo, hi in ((roi[2], roi[4]), (roi[1], roi[3])):
            yield ac.axis_grid(lo, hi, ac.QUARTER, 7) + (ac.QUARTER_HW[0], 7)
    for roi in ac.odd_scale_rois()[0]:
        for lo, hi in ((roi[2], roi[4]), (roi[1], roi[3])):
            yield ac.axis_grid(lo, hi, ac.ODD_SCALE, 7) + (ac.ODD_HW[0], 7)


def test_bisection_selects_exactly_the_valid_samples():
    n_axes = n_partial = 0
    for start, bin_size, g, size, pooled in _all_axes():
        for p in range(pooled):
            v = ac.axis_coords(start, bin_size, p, g)
            assert (np.diff(v) >= 0).all()                      # the premise of the bisection: v is non-decreasing in i
            ok = ac.axis_valid(v, size)
            i0, n = ac.bisect_valid_range(start, bin_size, p, g, size)
            want = np.zeros(g, dtype=bool)
            want[i0:i0 + n] = True
            assert np.array_equal(ok, want), (start, bin_size, g, p)
            assert n <= 2 * size + 3
            n_axes += 1
            n_partial += 0 < n < g
    assert n_axes > 1000 and n_partial >= 20      # bins with some, not all, samples valid: where a wrong bisection would show


# ---- each case holds the event it is named for ------------------------------------------------------------------------------------------
def _grid(name, pooled):
    roi = np.array([[0] + ac.NAMED[name]], dtype=F)
    return tuple(ac.np_adaptive_taps(roi, ac.SCALE, (2, 1, ac.H, ac.W), pooled).grid[0])


def test_premises_of_the_named_boxes():
    gh, gw = _grid("tall", 7)
    assert gh > gw >= 1
    gh, gw = _grid("wide", 7)
    assert gw > gh >= 1
    t = ac.np_adaptive_taps(ac.single_rois(), ac.SCALE, (2, 1, ac.H, ac.W), 7)
    assert (t.grid[:, 0] != t.grid[:, 1]).sum() >= 4
    # grid 1 through the max(., 1) clamp: the raw size is below one map pixel, zero, negative
    for name in ("sub_pixel", "zero_size", "malformed"):
        for pooled in ac.POOLED:
            assert _grid(name, pooled) == (1, 1), name
        roi = ac.NAMED[name]
        assert F(F(roi[2]) * F(ac.SCALE)) - F(F(roi[0]) * F(ac.SCALE)) < 1 and F(F(roi[3]) * F(ac.SCALE)) - F(F(roi[1]) * F(ac.SCALE)) < 1
    assert ac.NAMED["malformed"][2] < ac.NAMED["malformed"][0] and ac.NAMED["zero_size"][2] == ac.NAMED["zero_size"][0]
    assert _grid("grid_3x2", 7) == (3, 2)                       # a count that is no power of two
    assert _grid("whole_map", 1) == (ac.H, ac.W)                 # 50 x 84 samples in one bin
    t = ac.np_adaptive_taps(np.array([[0] + ac.WHOLE_MAP], dtype=F), ac.SCALE, (2, 1, ac.H, ac.W), 1)
    assert len(t.cell) == ac.H * ac.W and t.skipped[0] == 0


@pytest.mark.parametrize("pooled", ac.POOLED)
def test_far_around_roi_is_bounded_by_the_map(pooled):
    t = ac.np_adaptive_taps(np.array([[0] + ac.FAR_AROUND], dtype=F), ac.SCALE, (2, 1, ac.H, ac.W), pooled)
    gh, gw = t.grid[0]
    assert gh * gw * pooled * pooled > 300000 and (t.count == F(gh * gw)).all()      # count stays gh * gw ...
    n_valid = len(t.cell)
    assert 0 < n_valid <= (2 * ac.H + 3) * (2 * ac.W + 3)                            # ... while the samples inside are bounded by the map
    assert t.skipped.sum() == gh * gw * pooled * pooled - n_valid and t.skipped.sum() > 40 * n_valid
    assert np.bincount(t.cell).max() <= (2 * ac.H + 3) * (2 * ac.W + 3)


def test_skipped_prefix_suffix_both_and_nothing_valid_all_occur():
    total = dict(prefix=0, suffix=0, both=0, nothing=0)
    for pooled in ac.POOLED:
        for k, n in ac.axis_events(ac.single_rois()[:, :], ac.SCALE, (ac.H, ac.W), pooled).items():
            total[k] += n
    assert all(n > 0 for n in total.values()), total
    one = ac.axis_events(np.array([[0] + ac.FAR_AROUND], dtype=F), ac.SCALE, (ac.H, ac.W), 1)
    assert one == dict(prefix=0, suffix=0, both=2, nothing=0)
    seven = ac.axis_events(np.array([[0] + ac.FAR_AROUND], dtype=F), ac.SCALE, (ac.H, ac.W), 7)
    assert seven["nothing"] >= 8      # most bins of a +-4000 px box lie wholly outside the map
    assert ac.axis_events(np.array([[0] + ac.NAMED["off_top_left"]], dtype=F), ac.SCALE, (ac.H, ac.W), 2)["prefix"] == 2
    assert ac.axis_events(np.array([[0] + ac.NAMED["off_bottom_right"]], dtype=F), ac.SCALE, (ac.H, ac.W), 2)["suffix"] >= 1
    assert ac.axis_events(np.array([[0] + ac.NAMED["outside"]], dtype=F), ac.SCALE, (ac.H, ac.W), 7)["nothing"] == 14


def test_float64_picks_another_grid():
    """About one box in five of the draw gets another grid from float64 arithmetic, always the larger one: with power-of-two scales
    hi*scale and lo*scale are exact, so float32 differs from float64 by two monotone roundings (the difference, the quotient), which
    can bring a length just above 7k down to 7k but never one at or below 7k above it.  Both directions are counted."""
    rois, g32, g64 = ac.grid_rounding_rois()
    assert len(rois) == 6 and (g32 == g64 - 1).all()
    assert (rois[:, 4] * F(ac.QUARTER) <= ac.QUARTER_HW[0]).all()
    t = ac.np_adaptive_taps(rois, ac.QUARTER, (1, 1) + ac.QUARTER_HW, 7)
    assert np.array_equal(t.grid[:, 0], g32)
    rng = np.random.RandomState(3)
    draws = [ac.grid_rounding_draw(rng) for _ in range(500)]
    smaller = sum(g32 < g64 for _, _, g32, g64 in draws)
    larger = sum(g32 > g64 for _, _, g32, g64 in draws)
    assert 25 <= smaller <= 250 and larger == 0, (smaller, larger)


def test_float64_picks_another_grid_each_way_at_a_scale_that_is_no_power_of_two():
    """At scale 0.3 the two products round, and float32 lands on either side: three boxes where it takes the larger grid, three
    where it takes the smaller, and both directions occur in number over a draw.  On these boxes (hi - lo) * scale differs from
    hi*scale - lo*scale in float32 too, which no power-of-two scale can show."""
    rois, g32, g64 = ac.odd_scale_rois()
    assert len(rois) == 6 and (g32[:3] == g64[:3] + 1).all() and (g32[3:] == g64[3:] - 1).all()
    assert np.log2(float(F(ac.ODD_SCALE))) % 1 != 0
    assert (rois[:, 4] * F(ac.ODD_SCALE) <= ac.ODD_HW[0]).all() and (rois[:, 3] * F(ac.ODD_SCALE) <= ac.ODD_HW[1]).all()
    t = ac.np_adaptive_taps(rois, ac.ODD_SCALE, (1, 1) + ac.ODD_HW, 7)
    assert np.array_equal(t.grid[:, 0], g32)
    sc = F(ac.ODD_SCALE)
    other = [int(np.ceil(max(F(F(r[4] - r[2]) * sc), F(1.0)) / F(7))) for r in rois]      # the grid of (hi - lo) * scale
    assert (np.array(other) != g32).any()
    rng = np.random.RandomState(4)
    draws = [ac.odd_scale_draw(rng) for _ in range(2000)]
    larger = sum(a > b for _, _, a, b in draws)
    smaller = sum(a < b for _, _, a, b in draws)
    assert larger > 0 and smaller > 0, (larger, smaller)


def test_pyramid_and_empty_image_premises():
    feats, depth, boxes, rgb, dep, lv = ac.pyramid_reference(7)
    assert set(lv.tolist()) == {0, 1, 2, 3} and depth.shape[1] != feats[0].shape[1]
    feats, depth, boxes, rgb, dep, lv = ac.empty_image_reference()
    assert [len(b) for b in boxes] == list(ac.EMPTY_COUNTS) and 0 in ac.EMPTY_COUNTS
    assert ac.CHANNELS == [1, 33, 65] and ac.feature_map().shape[1] == 65
    # the map values are exact in float16 and bfloat16: one oracle output serves the three map dtypes
    import torch
    m = torch.from_numpy(ac.feature_map())
    assert torch.equal(m.half().float(), m) and torch.equal(m.bfloat16().float(), m)


def test_exact_contention_premise():
    shape, rois, gout = ac.exact_contention_case()
    t = ac.np_adaptive_taps(rois, ac.SCALE, shape, 8)
    assert (t.grid == (4, 2)).all() and (t.count == 8).all() and (t.skipped == 0).all()
    assert (t.w == F(0.25)).all()
    grad, K, A = ac.taps_backward(t, gout)
    assert K.max() == 4 * 64 and A.max() < 2.0 ** 12 and (A > 0).sum() > 0
    assert np.array_equal(grad * 32, np.round(grad * 32))      # every sum is a multiple of 2^-5


# ---- wrong restatements change an expected output -------------------------------------------------------------------------------------------
def _out(rois, scale, feat, pooled, variant=None):
    with np.errstate(all="ignore"):      # (a grid of 0 divides 0 by 0)
        return ac.apply_taps(ac.np_adaptive_taps(rois, scale, feat.shape, pooled, variant), feat)


def _changed(got, want):
    return (_bits(got) != _bits(want)).reshape(len(want), -1).any(axis=1)


@pytest.mark.parametrize("variant", ac.VARIANTS)
def test_a_wrong_restatement_changes_an_expected_output(variant):
    feat = ac.feature_map()[:, :3]
    rois = ac.single_rois()
    idx = {n: i for i, n in enumerate(ac.NAMES)}
    want = _out(rois, ac.SCALE, feat, 7)
    assert np.array_equal(_bits(want), _bits(ac.single_reference(7)[2][:, :3]))
    if variant == "f64grid":
        rois, g32, g64 = ac.grid_rounding_rois()
        feat = ac.feature_map(3, seed=6, shape=(1,) + ac.QUARTER_HW)
        changed = _changed(_out(rois, ac.QUARTER, feat, 7, variant), _out(rois, ac.QUARTER, feat, 7))
        assert changed.all()                                    # every box (float32 takes the smaller grid on all of them)
        rois, g32, g64 = ac.odd_scale_rois()                    # and each way, at a scale that is no power of two
        feat = ac.feature_map(3, seed=8, shape=(1,) + ac.ODD_HW)
        changed = _changed(_out(rois, ac.ODD_SCALE, feat, 7, variant), _out(rois, ac.ODD_SCALE, feat, 7))
        assert changed[:3].all() and changed[3:].all() and (g32[:3] > g64[:3]).all() and (g32[3:] < g64[3:]).all()
        return
    changed = _changed(_out(rois, ac.SCALE, feat, 7, variant), want)
    if variant == "floor":
        assert changed[idx["tall"]] and changed[idx["wide"]] and changed[idx["grid_3x2"]]
    elif variant == "unclamped":                                # a size of zero or below gives a grid of 0
        assert changed[idx["zero_size"]] and changed[idx["malformed"]]
    elif variant == "square":
        assert changed[idx["tall"]] and changed[idx["wide"]] and not changed[idx["sub_pixel"]]
    elif variant == "count_gh2":
        assert changed[idx["tall"]] and changed[idx["wide"]] and changed[idx["grid_3x2"]] and not changed[idx["sub_pixel"]]


def test_dropping_invalid_samples_without_plus_zero_cannot_change_an_output():
    """The kernel adds + 0.f once to a bin that left samples out, as the reference adds the 0 that bilinear_interpolate returns.
    A restatement without it would differ only on a bin whose running sum is -0 when the 0 is added.  There is no such bin: the sum
    starts at +0, and in round-to-nearest x + y is -0 only when both are -0, so no prefix of the sum is ever -0 -- the oracle itself
    drops those samples.  The nearest case is a map of -0 (every valid term is -0): both forms give +0 there, bit for bit, and on
    every other case."""
    rois = ac.single_rois()
    feat = np.full((2, 2, ac.H, ac.W), -0.0, dtype=F)
    t = ac.np_adaptive_taps(rois, ac.SCALE, feat.shape, 7)
    assert (t.skipped > 0).sum() > 50
    with_zero, without = ac.apply_taps(t, feat), ac.apply_taps(t, feat, plus_zero=False)
    assert np.signbit(feat).all() and not np.signbit(with_zero).any() and not np.signbit(without).any()
    assert np.array_equal(_bits(with_zero), _bits(ro.roi_align(feat, rois, ac.SCALE, 7, 0)))
    feat = ac.feature_map(3)
    assert np.array_equal(_bits(ac.apply_taps(t, feat)), _bits(ac.apply_taps(t, feat, plus_zero=False)))
