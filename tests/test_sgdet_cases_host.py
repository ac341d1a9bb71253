"""The premises of the sgdet parity suite, on the CPU: every case of tests/sgdet_cases.py reaches the branch, limit or tie it is
named for (a count above zero from the instrumented restatements, not merely a run), its random parts pass the draw conditions,
np_pairs equals a direct torch.sort(descending=True, stable=True) formulation, and the restatements reproduce what the
reference computed on the hand-built cases (tests/golden/sgdet/decode_cases.npz and pairs_cases.npz, written by
`tests/golden/make_golden_sgdet.py cases`).  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgdet_cases as sc  # noqa: E402
from test_sgdet_host import load_golden, np_decode_scores, np_overlap, np_pairs, pair_qualities  # noqa: E402

F = np.float32


def _summaries(name):
    """[(launch index, image index, mode, image, counters)] of a decode case, empty images left out."""
    out = []
    for li, (imgs, thr) in enumerate(sc.decode_case(name)):
        for mode in sc.decode_modes(name):
            for ii, d in enumerate(imgs):
                if len(d["predict_logits"]):
                    out.append((li, ii, mode, d, sc.decode_summary(d, thr, mode)))
    return out


# ---- the instrumented restatements are the restatements ---------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.DECODE_CASE_NAMES)
def test_decode_trace_equals_np_decode(name):
    for (imgs, thr) in sc.decode_case(name):
        for mode in sc.decode_modes(name):
            for d in imgs:
                if len(d["predict_logits"]):
                    np.testing.assert_array_equal(sc.decode_summary(d, thr, mode)["labels"], sc.expected_decode(d, thr, mode))


@pytest.mark.parametrize("name", sc.PAIR_CASE_NAMES)
def test_np_pairs_equals_a_stable_descending_torch_sort(name):
    for imgs, cap, overlap in sc.pair_case(name):
        for d in imgs:
            mine = np_pairs(d["boxes"], d["pred_scores"], cap, overlap)
            np.testing.assert_array_equal(mine, sc.torch_pairs(d["boxes"], d["pred_scores"], cap, overlap))
            t = sc.pairs_trace(d["boxes"], d["pred_scores"], cap, overlap)
            assert len(mine) == max(1, min(t["total"], cap))
            if t["capped"]:       # the trace's cut describes np_pairs' output: everything above T, then `need` of the group
                q = pair_qualities(mine, d["pred_scores"])
                assert (q > F(t["T"])).sum() == t["above"] and (q == F(t["T"])).sum() == t["need"] and 0 < t["need"] <= t["group"]


# ---- decode premises ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["post", "meet"])
def test_zero_max_cases_reach_the_zero_maximum_branches(mode):
    rows = _summaries("zero_max_" + mode)
    shapes = {d["predict_logits"].shape for _, _, _, d, _ in rows}
    assert shapes == {(n, C) for n in (4, 8, 70) for C in (2, 3, 5)}
    for li, ii, _, d, s in rows:
        n, C = d["predict_logits"].shape
        if n > C + 1:        # C - 1 foreground columns go in C - 1 steps; the steps after them have maximum 0
            assert s["zero_steps"] > 0 and s["repicks"] > 0 and s["never_picked"] > 0 and s["revived"] > 0, (li, ii, s)
            if mode == "meet":
                assert s["overwritten"] > 0, (li, ii, s)
    assert any(70 in (d["predict_logits"].shape[0],) and s["never_picked"] > 64 for _, _, _, d, s in rows)   # rows of two waves
    total = {k: sum(s[k] for *_, s in rows) for k in ("changed", "kept", "lower_col")}
    if mode == "meet":
        assert total["changed"] > 0          # a re-pick that gives the row another label
    else:
        assert total["kept"] > 0             # a re-pick of a labelled row at another column: "post" keeps the first label
    descending = [s for li, _, _, _, s in rows if li == 3]
    assert len(descending) == 1 and descending[0]["lower_col"] > 0 and descending[0]["repicks"] > 0
    never = [s["labels"][i] for *_, d, s in rows for i in range(len(s["labels"]))]
    assert 0 in never


def test_descending_variant_comes_back_at_the_lower_column():
    (imgs, thr), = sc.zero_max()[3:]
    d, = imgs
    C = d["predict_logits"].shape[1]
    label, steps, never = sc.decode_trace(sc.np_onehot_prob(d["pred_labels"], C), d["boxes_per_cls"], thr, "meet")
    assert [(s["row"], s["col"]) for s in steps[:4]] == [(0, 4), (1, 3), (2, 2), (3, 1)]
    assert steps[1]["revived"] == 1 and steps[2]["lower_col"] >= 1 and steps[3]["lower_col"] >= 1   # columns 3, 2, 1 of the picked row 0
    assert steps[4]["max"] == 0 and (steps[4]["row"], steps[4]["col"]) == (0, 1) and steps[4]["changed"]
    assert label[0] == 1 and list(never) == [4, 5, 6, 7] and not label[4:].any()


def test_row_ties_are_exact_and_of_every_kind():
    (imgs, thr), = sc.row_ties_post()
    loose, tight = imgs
    x = loose["predict_logits"]
    assert x.shape == (140, 201)
    np.testing.assert_array_equal(x[0], x[65]); np.testing.assert_array_equal(x[0], x[130])
    np.testing.assert_array_equal(x[1], x[66]); np.testing.assert_array_equal(x[1], x[131])
    assert x[0, 9] == x[0, 73] == x[0, 137] == x[0].max() and x[1, 5] == x[1, 8] == x[1, 72] == x[1].max()
    s = sc.decode_summary(loose, thr, "post")
    assert s["row_ties"] == 6 and s["col_ties"] == 6 and s["lane_ties"] == 3
    assert list(s["labels"][[0, 65, 130, 1, 66, 131]]) == [9, 9, 9, 5, 5, 5]
    t = sc.decode_summary(tight, thr, "post")       # one cluster: the second and third of identical rows fall to the next tied column
    assert list(t["labels"][[0, 2, 4]]) == [9, 73, 137] and list(t["labels"][[1, 3, 5]]) == [5, 8, 72]
    # the step that picks row 0 sees nine equal cells (three rows x three columns) and takes the first in row-major order
    _, steps, _ = sc.decode_trace(sc.np_softmax(x), loose["boxes_per_cls"], thr, "post")
    k = [st["row"] for st in steps].index(0)
    assert [(st["row"], st["col"], st["at_max"]) for st in steps[k:k + 3]] == [(0, 9, 9), (65, 9, 6), (130, 9, 3)]
    k = [st["row"] for st in steps].index(1)
    assert [(st["row"], st["col"], st["at_max"]) for st in steps[k:k + 3]] == [(1, 5, 9), (66, 5, 6), (131, 5, 3)]


def test_class_edges_and_homes():
    shapes = [[d["predict_logits"].shape for d in imgs] for imgs, _ in sc.class_edges()]
    assert shapes == [[(n, C) for n in (1, 5, 30)] for C in (2, 63, 64, 65, 128, 129, 1024)]
    homes = [[(d["predict_logits"].size, d["predict_logits"].size <= sc.LDS_CELLS) for d in imgs] for imgs, _ in sc.lds_boundary()]
    assert homes == [[(30720, True)], [(30855, False), (30613, True), (30976, False)], [(30720, True), (30848, False)]]
    assert 254 * 121 > sc.LDS_CELLS                  # 253 x 121 is the nearest LDS neighbour of 255 x 121
    (imgs, _), (far, _) = sc.mixed_homes()
    assert [len(d["predict_logits"]) for d in imgs] == [256, 10, 0, 1, 200]
    assert [d["predict_logits"].size > sc.LDS_CELLS for d in imgs] == [True, False, False, False, True]
    ws = [i for i, d in enumerate(far) if d["predict_logits"].size > sc.LDS_CELLS]
    assert ws == [0, 8, 16]                          # workspace images eight workgroups apart, LDS and empty images between


@pytest.mark.parametrize("name", sc.DECODE_CASE_NAMES)
def test_decode_cases_pass_the_draw_conditions(name):
    for li, ii, mode, d, s in _summaries(name):
        thr = sc.decode_case(name)[li][1]
        assert sc.robust(d, thr, sc.MIN_GAP if name in sc.HAND_MADE else None), (name, li, ii, mode, s["gap"], s["iou_margin"])   # both modes
        assert s["iou_margin"] >= sc.IOU_MARGIN
        if name in sc.HAND_MADE:
            assert s["gap"] >= sc.MIN_GAP


# ---- pair premises ------------------------------------------------------------------------------------------------------------

def _traces(name):
    return [[sc.pairs_trace(d["boxes"], d["pred_scores"], cap, ov) for d in imgs] for imgs, cap, ov in sc.pair_case(name)]


def test_caps_case_covers_the_bitonic_paddings():
    case = sc.caps()
    assert [cap for _, cap, _ in case] == [1, 2, 3, 100, 1000, 2047, 2049, 4095, 4096]
    for (t,), (_, cap, _) in zip(_traces("caps"), case):
        assert t["total"] == 4830 and t["capped"] and t["above"] + t["need"] == cap


def test_cap_edges_sit_on_both_sides_of_the_split():
    tr = [t for t, in _traces("cap_edges")]
    caps = [cap for _, cap, _ in sc.cap_edges()]
    overlap = [ov for _, _, ov in sc.cap_edges()]
    at = [(t["total"] == cap, ov) for t, cap, ov in zip(tr, caps, overlap)]
    above = [(t["total"] == cap + 1, ov) for t, cap, ov in zip(tr, caps, overlap)]
    for ov in (False, True):
        assert at.count((True, ov)) >= 1 and above.count((True, ov)) >= 1
    assert [t["capped"] for t in tr] == [False, True, False, True, False, True, False]
    assert tr[4]["total"] == 78 and tr[0]["total"] == 2070 and tr[2]["total"] == 6


def test_straddling_tie_groups():
    (a,), (b,), (c,) = _traces("straddle")
    for t in (a, b, c):
        assert t["T"] == 0.5 and t["above"] == 90 and t["group"] == 800 and len(t["waves"]) >= 3
    assert 0 < a["need"] < a["group"] and a["need"] == 410 and len(a["taken_waves"]) >= 2
    assert set(a["waves"]) - set(a["taken_waves"])          # members in waves from which nothing is taken
    assert b["need"] == b["group"] and c["need"] == 1
    assert (a["qualities"] > F(0.5)).sum() == 90 and (a["qualities"] < F(0.5)).sum() > 0


def test_zero_and_subnormal_products():
    tr = [t for t, in _traces("zero_scores")]
    assert tr[0]["T"] == 0 and tr[0]["above"] == 2450 and 0 < tr[0]["need"] < tr[0]["group"] == 7450
    assert tr[1]["T"] > 0 and tr[1]["above"] + tr[1]["need"] == 2450 and tr[2]["above"] + tr[2]["need"] == 2449   # the last non-zero product
    tiny = float(np.finfo(F).tiny)
    assert 0 < tr[3]["T"] < tiny and tr[3]["above"] == 600 and tr[3]["group"] == 1250 and tr[3]["need"] == 400
    q = tr[4]["qualities"]
    assert tr[4]["T"] == 0 and tr[4]["above"] == 1850 and ((q > 0) & (q < tiny)).sum() == 1850 and tr[4]["need"] == 150
    s = sc.zero_scores()[3][0][0]["pred_scores"]
    assert F(1e-23) * F(1e-23) == 0 and F(1e-22) * F(1e-23) > 0 and (s == 0).sum() == 50


def test_touching_boxes_overlap_and_boxes_a_pixel_apart_do_not():
    (imgs, cap, ov) = sc.touching()[0]
    a, nothing, gap1 = imgs
    m = np_overlap(a["boxes"])
    assert sorted(map(tuple, np.argwhere(m & ~np.eye(5, dtype=bool)))) == sorted(sc.TOUCHING_PAIRS)
    b = a["boxes"]
    assert b[0, 2] == b[1, 0] and m[0, 1] and b[1, 2] + 1 == b[2, 0] and not m[1, 2]         # x: shared column / next column
    assert b[0, 3] == b[3, 1] and m[0, 3] and b[3, 3] + 1 == b[4, 1] and not m[3, 4]         # y
    for d in (nothing, gap1):
        assert not (np_overlap(d["boxes"]) & ~np.eye(len(d["boxes"]), dtype=bool)).any()
        np.testing.assert_array_equal(np_pairs(d["boxes"], d["pred_scores"], cap, True), [[0, 0]])   # the placeholder, count 1
    assert sc.pairs_trace(a["boxes"], a["pred_scores"], 4, True)["capped"]


def test_word_edges_mix_the_mask_word_sizes_in_one_batch():
    case = sc.word_edges()
    assert [len(d["boxes"]) for d in case[0][0]] == [0, 1, 2, 31, 32, 33, 255, 256, 0, 64]
    assert [(cap, ov) for _, cap, ov in case] == [(2048, True), (2048, False)]
    tr = _traces("word_edges")
    assert any(t["capped"] for t in tr[0]) and any(t["capped"] for t in tr[1]) and any(not t["capped"] and t["total"] for t in tr[0])


# ---- the reference on the hand-built cases --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.GOLDEN_DECODE)
def test_decode_restatement_reproduces_the_reference_on_the_cases(name):
    g = load_golden("decode_cases")
    mode, = sc.decode_modes(name)
    imgs = [(d, thr) for ims, thr in sc.decode_case(name) for d in ims]
    got = [sc.expected_decode(d, thr, mode) for d, thr in imgs]
    np.testing.assert_array_equal(np.concatenate(got), g[name + "__labels"])          # bit for bit, re-picks and never-picked rows included
    if mode == "post":
        scores = np.concatenate([np_decode_scores(d["predict_logits"], l) for (d, _), l in zip(imgs, got)])
        np.testing.assert_allclose(scores, g[name + "__scores"], rtol=1e-6, atol=0)
        assert (scores == 0).sum() == (np.concatenate(got) == 0).sum()


@pytest.mark.parametrize("name", sc.GOLDEN_PAIRS)
def test_pair_restatement_reproduces_the_reference_on_the_cases(name):
    g = load_golden("pairs_cases")
    case = sc.pair_case(name)
    for k in sc.golden_pair_instances(name):
        imgs, cap, overlap = case[k]
        counts = g["%s__%d__counts" % (name, k)]
        ref = np.split(g["%s__%d__pairs" % (name, k)].astype(np.int64), np.cumsum(counts)[:-1])
        assert len(ref) == len(imgs)
        for d, r in zip(imgs, ref):
            mine = np_pairs(d["boxes"], d["pred_scores"], cap, overlap)
            assert mine.shape == r.shape, (name, k)
            if not sc.pairs_trace(d["boxes"], d["pred_scores"], cap, overlap)["capped"]:
                np.testing.assert_array_equal(mine, r, err_msg="%s %d" % (name, k))      # at or below the cap: row-major, exact
            else:                                                                         # the reference's sort is unstable
                q_ref, q_mine = pair_qualities(r, d["pred_scores"]), pair_qualities(mine, d["pred_scores"])
                np.testing.assert_array_equal(q_mine, q_ref)
                t = q_ref[-1]
                assert set(map(tuple, r[q_ref > t])) == set(map(tuple, mine[q_mine > t]))
