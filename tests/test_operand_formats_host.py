"""CPU proof of tests/operand_cases.py: the restated formats against torch's casts and against each other, every probe construction
with the count of the event it is named for, the derived per-product bounds, and the mutation check (eleven wrong restatements must
each change an expected output of the probe set)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operand_cases as oc  # noqa: E402
from operand_cases import FAST, MIXED, PRECISE  # noqa: E402


@pytest.fixture(scope="module")
def classes():
    return oc.activation_classes()


@pytest.fixture(scope="module")
def all_values(classes):
    """every probe value that any plane converts: activations, weights, and the scaled residuals of both"""
    acts = np.concatenate(list(classes.values()) + [oc.NONFINITE])
    vals = [acts]
    with np.errstate(invalid="ignore", over="ignore"):
        vals.append(oc._scaled(acts - oc.fp16_sat(acts), oc.ACT_RES_EXP))
        for w in oc.weight_sets().values():
            e = oc.weight_exp(np.abs(w).max())
            h = oc.fp16_sat(w)
            vals += [w, oc._scaled(h, e), oc._scaled(w - h, e + oc.ACT_RES_EXP)]
    return oc.f32(np.concatenate(vals))


def _is_tie(v, mant_bits, emin):
    v = np.asarray(v, dtype=np.float64)
    return np.abs(v - oc._grid_round(v, mant_bits, emin, False)) == oc._half_ulp(v, mant_bits, emin)


def test_the_two_e4m3_restatements_agree(all_values):
    sweep = oc.from_bits(np.arange(0, 2 ** 32, 2048, dtype=np.uint64).astype(np.uint32))     # every binade, 4096 mantissas each
    edge = oc.from_bits(np.concatenate([oc.bits(oc.E4M3_VALUE[np.isfinite(oc.E4M3_VALUE)]) + np.uint32(d) for d in (0, 1, 0xffffffff)]))
    mids = oc.f32((oc.E4M3_VALUE[:0x7e] + oc.E4M3_VALUE[1:0x7f]) / 2)                         # every tie of the positive half
    for v in (all_values, sweep, edge, mids, -mids):
        hand, th = oc.e4m3_sat_bits(v), oc.e4m3_sat_bits_torch(v)
        nan = np.isnan(v)
        assert np.array_equal(hand[~nan], th[~nan])
        assert ((hand[nan] & 0x7f) == 0x7f).all() and ((th[nan] & 0x7f) == 0x7f).all()       # a NaN stays a NaN in both
    # the documented points: 464 is the 448 / 480 tie and goes to the even 448; everything above saturates; 2^-10 ties to zero
    pts = oc.f32([448, 464, float(oc._next_up(464.0)), 480, 1000, np.inf, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, -1e9])
    assert oc.e4m3_sat_bits(pts).tolist() == [0x7e, 0x7e, 0x7e, 0x7e, 0x7e, 0x7e, 0x00, 0x02, 0x01, 0xfe]
    assert np.array_equal(oc.e4m3_sat_bits(oc.f32(oc.E4M3_VALUE[:0x7f])), np.arange(0x7f, dtype=np.uint8))    # every code is a fixed point


def test_fp16_and_bf16_agree_with_torch(all_values):
    v = all_values[np.isfinite(all_values)]
    t = torch.from_numpy(v.copy())
    bf = t.to(torch.bfloat16).to(torch.float32).numpy()
    ok = np.isfinite(bf)
    assert np.array_equal(oc.bits(oc.bf16_rne(v))[ok], oc.bits(bf)[ok])
    h = t.to(torch.float16).to(torch.float32).numpy()
    ok = np.isfinite(h)                                                   # torch overflows to Inf where the format saturates
    assert np.array_equal(oc.bits(oc.fp16_sat(v))[ok], oc.bits(h)[ok]) and (~ok).sum() > 0
    assert (np.abs(oc.fp16_sat(v)[~ok]) == oc.FP16_MAX).all()
    assert np.isnan(oc.fp16_sat(oc.NONFINITE[2:])).all() and np.isnan(oc.bf16_rne(oc.NONFINITE[2:])).all()
    hi, lo = oc.split(v)
    assert np.array_equal(lo, oc.bf16_rne(v - hi))


def test_f24_rounds_to_nearest_even_at_bit_8():
    x = oc.from_bits(np.uint32([0x3f800080, 0x3f800180, 0x3f800081, 0x3f80007f, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xffffffff,
                                0x80000000]))
    want = [0x3f800000, 0x3f800200, 0x3f800100, 0x3f800000, 0x7f800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffffff00, 0x80000000]
    assert oc.bits(oc.f24(x)).tolist() == want
    rows = oc.f24_rows(x.reshape(2, 5))
    assert rows.shape == (2, 15) and rows[0, :3].tolist() == [0x00, 0x80, 0x3f]
    assert np.array_equal(oc.bits(oc.decode_f24_rows(rows)).ravel(), np.uint32(want))


def test_weight_exponent_boundaries():
    sets = oc.weight_sets()
    got = {k: oc.weight_exp(np.abs(v).max()) for k, v in sets.items()}
    assert got == {"zeros": 24, "tiny": 24, "boundary_e10": 10, "boundary_e9": 9, "max_448": 0, "above_448": 0, "ordinary": got["ordinary"]}
    assert 10 <= got["ordinary"] <= 12 and np.abs(sets["tiny"]).max() < 448 * 2.0 ** -24
    assert np.abs(sets["boundary_e10"]).max() == np.float32(448 * 2.0 ** -10)
    assert oc.bits(np.abs(sets["boundary_e9"]).max()) == oc.bits(np.float32(448 * 2.0 ** -10)) + 1     # the exponent boundary: one float apart
    for e in range(0, 25):
        assert oc.weight_exp(448 * 2.0 ** -e) == e and oc.weight_exp(float(oc._next_up(448 * 2.0 ** -e))) == max(e - 1, 0)
    # X = e4m3(2^e h) saturates only in the tensor whose maximum exceeds 448
    for name, w in sets.items():
        e = got[name]
        sat = int((np.abs(oc._scaled(oc.fp16_sat(w), e)) > 448).sum())
        assert (sat > 0) == (name == "above_448"), (name, sat)


def test_layouts():
    k = np.arange(1152)
    assert oc.split_index(k[:70]).tolist()[:34] == list(range(32)) + [64, 65] and oc.split_index(33) + 32 == 97
    s = np.concatenate([oc.split_index(k), oc.split_index(k) + 32])
    assert np.array_equal(np.sort(s), np.arange(2304))                  # hi and lo slots tile the row
    b = np.concatenate([oc.mixed_h_offset(k), oc.mixed_h_offset(k) + 1, oc.mixed_x_offset(k), oc.mixed_x_offset(k) + 4])
    assert np.array_equal(np.sort(b), np.arange(4608))
    assert oc.mixed_h_offset(65) == 258 and oc.mixed_x_offset(0) == 128 and oc.mixed_x_offset(5) == 137 and oc.mixed_x_offset(64) == 384
    a = oc.f32(np.arange(128).reshape(2, 64) / 8)
    rows = oc.mixed_act_rows(a)
    assert rows.shape == (2, 256) and oc.E4M3_VALUE[rows[0, 128 + 8 + 4 + 1]] == a[0, 5] == 0.625    # Y of column 5: group 1, byte 4 + 1


def test_every_class_holds_the_event_it_is_named_for(classes, capsys):
    c = {k: v.astype(np.float64) for k, v in classes.items()}
    count = {}
    h = {k: oc.fp16_sat(classes[k]).astype(np.float64) for k in c}
    up16 = lambda k: np.abs(h[k]) > np.abs(c[k])                           # noqa: E731
    count["fp16_tie_down"] = int((_is_tie(c["fp16_tie_down"], 10, -14) & ~up16("fp16_tie_down")).sum())
    count["fp16_tie_up"] = int((_is_tie(c["fp16_tie_up"], 10, -14) & up16("fp16_tie_up")).sum())
    assert count["fp16_tie_down"] == len(c["fp16_tie_down"]) and count["fp16_tie_up"] == len(c["fp16_tie_up"])
    for k, up in (("bf16_hi_tie_down", False), ("bf16_hi_tie_up", True)):
        hi, lo = oc.split(classes[k])
        went_up = np.abs(hi) > np.abs(classes[k])
        count[k] = int((_is_tie(c[k], 7, -126) & (went_up == up) & (lo != 0)).sum())
        assert count[k] == len(c[k])
    hi, lo = oc.split(classes["bf16_lo_tie"])
    res = c["bf16_lo_tie"] - hi
    count["bf16_lo_tie"] = int((_is_tie(res, 7, -126) & (lo != 0)).sum())
    assert count["bf16_lo_tie"] >= 32
    count["f24_tie"] = int(((oc.bits(hi + lo) & 0xff) == 0x80).sum())      # the 16-bit form ties again at bit 8
    assert count["f24_tie"] >= 4
    for plane in (oc.split(classes["zero_residual"])[1], c["zero_residual"] - h["zero_residual"]):
        assert (plane == 0).all()
    count["zero_residual"] = len(c["zero_residual"])
    # residual planes that must be non-zero: X of the classes that exercise it, Y of all non-zero values
    for k in ("fp16_tie_down", "fp16_tie_up", "max_residual", "e4m3_subnormal_residual", "normal", "outlier"):
        _, x, y = oc.mixed_act_planes(classes[k])
        nz = (x & 0x7f) != 0
        assert nz.sum() >= (0.6 * len(x) if k == "e4m3_subnormal_residual" else 0.9 * len(x)), k
        assert ((y & 0x7f) != 0).all() or k in ("normal",)
    l = c["max_residual"] - h["max_residual"]
    count["max_residual"] = int((np.abs(l) > 0.999 * oc._half_ulp(c["max_residual"], 10, -14)).sum())
    assert count["max_residual"] == len(l)
    xs = (c["e4m3_tie"] - h["e4m3_tie"]) * 2.0 ** 11
    count["e4m3_tie_X"] = int((_is_tie(xs, 3, -6) & (xs != 0)).sum())
    count["e4m3_tie_Y"] = int(_is_tie(c["e4m3_tie"], 3, -6).sum())
    assert count["e4m3_tie_X"] == 72 and count["e4m3_tie_Y"] == 36
    for name, v in (("X", xs[xs != 0]), ("Y", c["e4m3_tie"][_is_tie(c["e4m3_tie"], 3, -6)])):       # both directions
        up = np.abs(oc.e4m3_sat(oc.f32(v))) > np.abs(v)
        assert up.sum() > 0 and (~up).sum() > 0, name
    a = np.abs(c["clamp_448"])
    count["e4m3_saturations"] = int((a > 448).sum())
    count["e4m3_tie_at_464"] = int((a == 464).sum())
    assert count["e4m3_saturations"] >= 12 and count["e4m3_tie_at_464"] == 2 and (a == 448).sum() == 2 and (a == 480).sum() == 2
    assert ((oc.e4m3_sat_bits(classes["clamp_448"][a >= 447.95]) & 0x7f) == 0x7e).all()
    a = np.abs(c["clamp_65504"])
    count["fp16_saturations"] = int((a > 65504).sum())
    assert count["fp16_saturations"] >= 10 and (np.abs(h["clamp_65504"]) <= 65504).all() and (a == 65520).sum() == 2
    assert (np.abs(h["clamp_65504"][a >= 65504]) == 65504).all()
    a = np.abs(h["fp16_subnormal"])
    count["fp16_subnormals"] = int(((a < 2.0 ** -14) & (a > 0)).sum())
    count["fp16_subnormal_ties"] = int(_is_tie(c["fp16_subnormal"], 10, -14).sum())
    assert count["fp16_subnormals"] >= 8 and count["fp16_subnormal_ties"] >= 6 and (a == 2.0 ** -14).sum() >= 2 and (a == 0).sum() >= 2
    xs = np.abs(c["e4m3_subnormal_residual"] - h["e4m3_subnormal_residual"]) * 2.0 ** 11
    count["e4m3_subnormal_X"] = int(((xs >= 2.0 ** -9) & (xs < 2.0 ** -6)).sum())
    ys = np.abs(c["e4m3_subnormal_residual"])
    count["e4m3_subnormal_Y"] = int(((ys >= 2.0 ** -9) & (ys < 2.0 ** -6)).sum())
    assert count["e4m3_subnormal_X"] >= 12 and count["e4m3_subnormal_Y"] >= 6
    assert _is_tie(xs[xs > 0], 3, -6).sum() >= 4
    xs = np.abs(c["e4m3_below_subnormal"] - h["e4m3_below_subnormal"]) * 2.0 ** 11
    count["e4m3_below_half_subnormal_X"] = int(((xs > 0) & (xs <= 2.0 ** -10)).sum())
    _, x, y = oc.mixed_act_planes(classes["e4m3_below_subnormal"])
    assert count["e4m3_below_half_subnormal_X"] >= 8 and ((x & 0x7f)[(xs > 0) & (xs <= 2.0 ** -10)] == 0).all()
    assert ((y & 0x7f) == 0).sum() >= 4                                     # |a| <= 2^-10: Y rounds to zero too
    a = np.abs(c["zero_and_fp32_subnormal"])
    count["fp32_subnormals"] = int(((a > 0) & (a < 2.0 ** -126)).sum())
    count["zeros"] = int((a == 0).sum())
    assert count["fp32_subnormals"] >= 5 and count["zeros"] >= 3 and np.signbit(classes["zero_and_fp32_subnormal"][1])
    assert len(classes["normal"]) == 256 and np.abs(classes["outlier"]).max() > 60
    with capsys.disabled():
        print("\n[operand probes] events per class: %s" % count)


def test_weight_values_carry_residuals_in_every_plane():
    for name, w in oc.weight_sets().items():
        if name == "zeros":
            continue
        e = oc.weight_exp(np.abs(w).max())
        hi, lo = oc.split(w)
        h, x, y = oc.mixed_weight_planes(w, e)
        assert (lo != 0).sum() >= 3 and ((x & 0x7f) != 0).sum() >= 3 and ((y & 0x7f) != 0).sum() >= (1 if name == "tiny" else 3), name
    w = oc.weight_sets()["ordinary"]
    assert _is_tie(w.astype(np.float64), 10, -14).sum() >= 2 and _is_tie(w.astype(np.float64), 7, -126).sum() >= 1


def test_layout_meets_every_slot_and_swizzle_class():
    for M, K in ((513, 576), (255, 64)):
        _, cls = oc.activation_matrix(M, K)
        m, k = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
        seen = np.zeros((oc.N_CLASSES, 64, 8), dtype=bool)
        seen[cls, k & 63, (m >> 1) & 7] = True
        assert seen.all(), (M, K)
    a, cls = oc.activation_matrix(513, 576)
    names = list(oc.activation_classes())
    for ci, name in enumerate(names):            # every value of every class is in the matrix
        assert set(oc.bits(oc.activation_classes()[name]).tolist()) == set(oc.bits(a[cls == ci]).tolist()), name
    for name in oc.SIGMAS:
        for N, K in ((576, 576), (192, 64), (192, 32), (1152, 1152), (1728, 64)):
            s = oc.sigma(name, N, K)
            assert s.min() == 0 and s.max() == K - 1 and len(set(s.tolist())) == K
    assert len(oc.wgrad_rows(1000, 1)) <= 100 and {0, 31, 32, 255, 256, 767, 768, 991, 992, 999} <= set(oc.wgrad_rows(1000, 1))
    assert {1439, 1440, 8639, 8640, 9998, 9983, 9984} <= set(oc.wgrad_rows(9999, 7))


@pytest.mark.parametrize("mode", [PRECISE, FAST, MIXED])
def test_restatement_stays_inside_the_derived_bound(mode, classes, capsys):
    """|product - a w| against float64 on every finite probe pair; the bound comes from half-ulps of the planes (product_bound)."""
    a = np.concatenate(list(classes.values()))
    worst = 0.0
    for name, w in oc.weight_sets().items():
        e = oc.weight_exp(np.abs(w).max())
        p = oc.product(a[:, None], w[None, :], mode, e).astype(np.float64)
        ref = a[:, None].astype(np.float64) * w[None, :].astype(np.float64)
        b = oc.product_bound(a[:, None], w[None, :], mode, e)
        assert np.isfinite(p).all()
        frac = np.abs(p - ref) / b
        assert frac.max() <= 1.0, (name, frac.max())
        worst = max(worst, frac.max())
    # the class the formats claim, where nothing saturates and nothing is subnormal: a few 2^-16 (precise), 2^-13 worst case (mixed:
    # four e4m3 half-steps of 2^-4 on residuals of 2^-11), 2^-7 (fast)
    a1, w1 = classes["normal"], oc.weight_sets()["ordinary"]
    e = oc.weight_exp(np.abs(w1).max())
    rel = oc.product_bound(a1[:, None], w1[None, :], mode, e) / np.abs(a1[:, None].astype(np.float64) * w1[None, :])
    big = (np.abs(a1[:, None]) >= 2.0 ** -5) & (np.abs(w1[None, :]) >= np.abs(w1).max() / 8)      # every plane in its normal range
    assert big.sum() > 1000 and rel[big].max() <= {PRECISE: 3.1 * 2.0 ** -16, FAST: 2.0 ** -7 * 1.01, MIXED: 1.1 * 2.0 ** -13}[mode]
    with capsys.disabled():
        print("\n[operand probes] %s: restatement reaches %.3f of the derived bound" % (oc.MODE_NAMES[mode], worst))


def _expected_outputs(W):
    """every kind of expected output of the device test, on 128 rows of the probe matrix: products per weight set and mode, the
    operand row images, and the split-row / f24 bytes of the precise products"""
    M, K = 128, 576
    a, _ = oc.activation_matrix(M, K)
    sig = oc.sigma("permutation", K, K)
    out = {"act_rows_mixed": oc.mixed_act_rows(a, W), "act_rows_split": oc.split_rows(a, W)}
    for name, vals in oc.weight_sets().items():
        w, wv = oc.selector_weight(K, K, vals, sig)
        rows, e = oc.mixed_weight_rows(w, W)
        out["weight_rows_" + name], out["weight_exp_" + name] = rows, np.int32(e)
        for mode in (PRECISE, FAST, MIXED):
            out["product_%s_%s" % (name, oc.MODE_NAMES[mode])] = oc.product(a[:, sig], wv[None, :], mode, e, W)
    c = oc.product(a[:, sig], oc.selector_weight(K, K, oc.weight_sets()["max_448"], sig)[1][None, :], PRECISE)    # the formats' own input
    out["split_epilogue"], out["f24_epilogue"] = oc.split_rows(c, W), oc.f24_rows(c, W)
    return out


def test_every_wrong_restatement_changes_an_expected_output(capsys):
    right = _expected_outputs(oc.RIGHT)
    again = _expected_outputs(oc.Wrong())
    assert all(right[k].tobytes() == again[k].tobytes() for k in right)
    log = []
    for name, kw in oc.MUTATIONS.items():
        wrong = _expected_outputs(oc.Wrong(**kw))
        changed = {k: int((np.atleast_1d(right[k]).view(np.uint8) != np.atleast_1d(wrong[k]).view(np.uint8)).sum()) for k in right}
        changed = {k: v for k, v in changed.items() if v}
        assert changed, name
        kinds = sorted({k.split("_")[0] + "_" + k.split("_")[1] if not k.startswith("product") else "product_" + k.rsplit("_", 1)[1] for k in changed})
        log.append("%-42s changes %9d bytes in %2d outputs: %s" % (name, sum(changed.values()), len(changed), ", ".join(kinds)))
    assert len(log) == 11
    with capsys.disabled():
        print("\n[operand probes] mutation log\n" + "\n".join(log))
