"""Premises of the detector-side parity inputs (tests/detect_cases.py), on the CPU: the closed forms equal the restatements, every
"only this wave / this bit sees it" input has its suppressor where it says, the seeded cases are decision-robust, the exact cases
are exact, every kernel instance has a case, and each wrong restatement changes the expected result of at least one case -- so a
device that computed the wrong form would fail tests/test_detect_parity_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_cases as dc  # noqa: E402
from test_boxhead_host import np_nms  # noqa: E402

F = np.float32


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


_all_nms_launches = dc.all_nms_launches


def test_the_name_lists_are_the_cases():
    assert tuple(_all_nms_launches()) == dc.NMS_LAUNCH_NAMES
    assert tuple(dc.box_cases()) == dc.BOX_CASE_NAMES and tuple(dc.rpn_cases()) == dc.RPN_CASE_NAMES


# ---- the restatements with switches ----------------------------------------------------------------------------------------

def test_the_variants_with_every_switch_off_are_the_restatements():
    for name, launch in _all_nms_launches().items():
        assert _same(dc.expected_nms(launch), dc.expected_nms(launch, dc.nms_variant)), name
    for name, case in dc.box_cases().items():
        for d, (r32, _, _, _) in zip(case["imgs"], dc.expected_box(name)):
            got = dc.box_variant(d, case["prm"])
            assert np.array_equal(got["orig_inds"], r32["orig_inds"]) and np.array_equal(got["pred_labels"], r32["pred_labels"]), name
    for name, case in dc.rpn_cases().items():
        if len(case["d"]["objectness"]) == 1:
            for got, want in zip(dc.rpn_variant(case["d"], case["c"]), dc.expected_rpn(name)[0]):
                assert np.array_equal(got["anchor_index"], want["anchor_index"]), name


def test_closed_forms_equal_np_nms():
    """The ladder keeps the even ranks, the disjoint boxes all stay, the copies leave one, the caps cut the ascending list."""
    n = 0
    for name, launch in _all_nms_launches().items():
        if "closed_form" in launch:
            assert _same(dc.expected_nms(launch), launch["closed_form"]), name
            n += 1
    assert n >= 14
    lad = dc.ladder_boxes(8)
    assert dc.iou_form("dev", lad[0], lad[1]) == F(70) / F(130) and dc.iou_form("dev", lad[0], lad[2]) == F(40) / F(160)
    for mode in ("perm", "equal"):   # the permuted ladder really permutes; 6144 needs the whole uint16 order[]
        boxes, scores, keep = dc.ladder_segment(6144, mode)
        assert len(keep) == 3072 and (mode == "equal" or not np.array_equal(keep, np.arange(0, 6144, 2)))
    assert [len(k) for k in dc.nms_launches()["cap_33"]["closed_form"]] == [33, 33, 1]
    assert [len(k) for k in dc.nms_launches()["cap_32"]["closed_form"]] == [32, 32, 1]
    assert [len(k) for k in dc.expected_nms(dict(dc.nms_launches()["cap_33"], max_keep=-1))] == [33, 64, 1]   # 33 = the survivor count


# ---- where the suppressor sits ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(dc.SUPPRESSOR_FORMS))
def test_one_suppressor_sits_at_the_stated_kept_position(name):
    """Replay of the greedy pass: all n boxes are kept in index order, the last candidate starts a 64-block of its own and exactly
    one kept box suppresses it, at kept position p -- which only wave p mod (NT / 64) reads."""
    launch = dc.nms_launches()["suppressor_" + name]
    n, ps = launch["n"], launch["ps"]
    waves = 16 if name.startswith("w16") else 4
    assert n % 64 == 0 and len(launch["segs"][0][0]) == n + 1
    assert {p % waves for p in ps if p < 17} == set(range(waves)) == {p % waves for p in ps if p >= n - 16}
    assert max(ps) == n - 1 and min(ps) == 0
    for (boxes, scores), p in zip(launch["segs"], ps):
        order, kept, by = dc.nms_replay(boxes, scores, launch["thr"])
        assert np.array_equal(order, np.arange(n + 1)) and kept == list(range(n)) and by == {n: [p]}


def test_in_block_pairs_sit_at_the_stated_bits():
    launch = dc.nms_launches()["inblock_bits"]
    assert {(a, b) for _, a, b in launch["pairs"]} == {(0, 1), (0, 63), (62, 63), (31, 32)}
    for (boxes, scores), (blk, a, b) in zip(launch["segs"], launch["pairs"]):
        order, kept, by = dc.nms_replay(boxes, scores, launch["thr"])
        base = 64 * blk
        assert np.array_equal(order, np.arange(base + 64))
        assert by == {base + b: [base + a]} and kept[base + a] == base + a   # nothing before lane a is removed: position = rank
        assert (base + a) // 64 == (base + b) // 64 == blk                   # suppressor and candidate share the 64-block
    boxes, scores = launch["segs"][-1]                                         # the chain across the 63 | 64 boundary
    order, kept, by = dc.nms_replay(boxes, scores, launch["thr"])
    assert np.array_equal(order, np.arange(128)) and by == {64: [63]} and 65 in kept
    assert dc.iou_form("dev", boxes[64], boxes[65]) > F(0.5) >= dc.iou_form("dev", boxes[63], boxes[65])


# ---- robustness and exactness ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["instances_%d" % n for n in sorted(dc.NMS_SEEDS)])
def test_seeded_nms_launches_are_decision_robust(name):
    launch = dc.nms_launches()[name]
    assert dc.nms_launch_robust(launch)
    sizes = [len(s[0]) for s in launch["segs"]]
    assert sizes[1:] == [0, 1, 63, 64, 65] and sizes[0] in (256, 257, 1024, 1025, 6144)
    kept = len(dc.expected_nms(launch)[0])
    assert 0.1 * sizes[0] <= kept <= 0.9 * sizes[0]   # the NMS removes a good part and keeps a good part


@pytest.mark.parametrize("name", sorted(dc.BOX_SHAPES))
def test_seeded_decoder_cases_are_decision_robust(name):
    assert dc.box_case_robust(name)
    C, sizes = dc.BOX_SHAPES[name]
    assert 3 <= C <= 5 and [len(d["proposals"]) for d in dc.box_cases()[name]["imgs"]] == list(sizes)
    r32, _, d32, _ = dc.expected_box(name)[0]
    assert 0 < len(r32["orig_inds"]) and len(d32["consulted"]) > sizes[0]


def test_rpn_cases_are_decision_robust_or_exact():
    for name, case in dc.rpn_cases().items():
        r32, r64, diag = dc.expected_rpn(name)
        if name.startswith("pairs_") and name != "pairs_half":   # (built so that float64 decides the other way)
            continue
        for a, b in zip(r32, r64):
            assert np.array_equal(a["level"], b["level"]) and np.array_equal(a["anchor_index"], b["anchor_index"]), name
        if case["c"]["thr"] > 0 and not name.startswith("pairs_"):   # (the pairs sit on the threshold on purpose)
            assert not np.any(np.abs(diag["consulted"].astype(np.float64) - case["c"]["thr"]) < 1e-5), name
        if not any(name.startswith(p) for p in ("ties_", "signed_zero", "merge_")):   # (those cut inside a tie on purpose)
            assert all(float(hi) - float(lo) >= 1e-6 for hi, lo in diag["cuts"]), name


def test_exact_cases_are_exact():
    """Zero regressions return the anchor / proposal bit for bit (float32 == float64 == input); equal logits give exactly 1 / C."""
    for name, case in dc.rpn_cases().items():
        if name.startswith("k_") or name == "shift_only" or (name.startswith("pairs_") and name != "pairs_half"):
            continue   # (anchor_grid's anchors reach over the image: clipped, still exact; the form pairs: float64 keeps other rows)
        anchors = case["d"]["anchors"]
        for a, b in zip(*dc.expected_rpn(name)[:2]):
            assert np.array_equal(a["boxes"], b["boxes"].astype(F)), name
            if "instances" not in name and "post_cap" not in name and name != "min_size_exact":   # (those clip)
                for l in np.unique(a["level"]):
                    m = a["level"] == l
                    assert np.array_equal(a["boxes"][m], anchors[l][a["anchor_index"][m]]), name
    for name, case in dc.box_cases().items():
        if case.get("seeded"):
            continue
        for d, (r32, r64, d32, _) in zip(case["imgs"], dc.expected_box(name)):
            assert np.array_equal(d32["dec"], np.repeat(d["proposals"][:, None], d["class_logits"].shape[1], 1)), name
            if not name.startswith("pairs_") or name == "pairs_half":
                assert np.array_equal(r32["boxes"], r64["boxes"].astype(F)), name
    for C in (2, 4):
        for r32, r64, d32, d64 in dc.expected_box("score_thresh_C%d_at" % C):
            assert np.all(d32["prob"] == F(1.0 / C)) and np.all(d64["prob"] == 1.0 / C)
    for name, case in dc.box_cases().items():
        if "n_det" in case:
            assert [len(r[0]["orig_inds"]) for r in dc.expected_box(name)] == [case["n_det"]] * len(case["imgs"]), name
    case = dc.box_cases()["row_max_ties"]
    assert dc.expected_box("row_max_ties")[0][0]["pred_labels"].tolist() == case["labels"]


def test_threshold_pairs_separate_the_forms():
    forms = dc.form_pairs()
    a, b = dc.drawn_pairs()
    assert np.all(a * 256 == np.round(a * 256)) and np.all(b * 256 == np.round(b * 256)) and a.min() >= 0 and b.min() >= 0   # the 1 / 256 grid
    sides = np.concatenate([a[:, 2:] - a[:, :2] + 1, b[:, 2:] - b[:, :2] + 1])
    assert sides.min() >= 8 and sides.max() <= 300 and max(a.max(), b.max()) < 1000
    dev = dc.iou_form("dev", a, b)
    for form in dc.IOU_FORMS:
        v = forms[form]
        frac = float(np.mean(dc.iou_form(form, a, b) != dev))
        print("%s differs from devIoU in the last bit on %.1f %% of %d pairs" % (form, 100 * frac, len(a)))
        assert len(v["a"]) == 4 and np.all(v["dev"] != v["other"])
        thr = F(v["thr"])
        assert float(thr) == v["thr"] and thr == min(v["dev"][0], v["other"][0])
        assert (v["dev"][0] > thr) != (v["other"][0] > thr)            # under `>` exactly one of the two forms suppresses
    ha, hb = dc.half_pairs()
    assert len(ha) == 16 and np.all(dc.iou_form("dev", ha, hb) == F(0.5)) and np.all(ha == np.round(ha)) and np.all(hb == np.round(hb))
    ua, ub = dc.above_half_pairs()
    assert len(ua) == 16 and np.all(dc.iou_form("dev", ua, ub) == dc.UP_HALF)
    assert np.all(ua * 4 == np.round(ua * 4)) and np.all(ub * 4 == np.round(ub * 4))
    # translated by the pitch of the RPN / decoder cases the pairs keep their IoU bits, and pairs do not meet
    for case in (dc.rpn_cases()["pairs_half"]["d"]["anchors"][0], dc.box_cases()["pairs_half"]["imgs"][0]["proposals"]):
        ba, bb, sup = dc.bulk_pairs()
        assert np.array_equal(dc.iou_form("dev", case[0::2], case[1::2]), dc.iou_form("dev", ba, bb))
        assert np.all(case[2::2, 0] > case[0:-2:2, 2]) and np.all(case[2::2, 0] > case[1:-2:2, 2])


# ---- every kernel instance, every stated size ------------------------------------------------------------------------------

_instance = dc.nms_instance


def test_every_instance_and_boundary_has_a_case():
    nms = {max(len(s[0]) for s in l["segs"]) for l in dc.nms_launches().values()}
    assert {256, 257, 1024, 1025, 6144} <= nms and {_instance(n) for n in nms} == {256, 1024, 6144}
    rpn = {c["capacity"] for c in dc.rpn_cases().values() if "capacity" in c}
    assert rpn == {256, 257, 1024, 1025, 6144}
    for name, c in dc.rpn_cases().items():
        if "capacity" in c:
            A, H, W = c["d"]["objectness"][0].shape[1:]
            assert c["capacity"] == min(c["c"]["pre"], A * H * W)
            live = [n for n in dc.expected_rpn(name)[2]["nms_in"]]
            assert live == [c["capacity"], 0, 1, 63, 64, 65], (name, live)
    for case in (dc.box_cases()["shift_only"], dc.rpn_cases()["shift_only"]):   # shifts, no scaling: expf(0) == 1 is the only expf
        reg = case["imgs"][0]["box_regression"].reshape(64, 3, 4) if "imgs" in case else case["d"]["box_regression"][0].reshape(2, 3, 4, 10, 12).transpose(0, 1, 3, 4, 2)
        assert case["bitwise"] and np.all(reg[..., 2:] == 0) and np.count_nonzero(reg[..., :2]) > 0.9 * reg[..., :2].size
    box = {len(d["proposals"]) for c in dc.box_cases().values() for d in c["imgs"]}
    assert {256, 257, 1024, 1025, 2000, 6144} <= box
    assert {_instance(max(len(d["proposals"]) for d in c["imgs"])) for c in dc.box_cases().values()} == {256, 1024, 6144}
    for name in ("instances_256", "instances_1024", "instances_6144"):
        assert 0 in [len(d["proposals"]) for d in dc.box_cases()[name]["imgs"][1:-1]]   # an empty image between two others
    assert dc.box_cases()["agnostic_6144"]["imgs"][0]["box_regression"].shape[1] == 8
    assert _instance(max(dc.BOX_SHAPES["agnostic_6144"][1])) == 6144


# ---- the selection's paths ---------------------------------------------------------------------------------------------------

def test_rpn_selection_cases_enter_the_stated_paths():
    cases = dc.rpn_cases()
    for pre, path in ((106, "copy"), (105, "copy"), (104, "radix")):
        c = cases["k_%d_of_105" % pre]
        assert c["d"]["objectness"][0].shape == (3, 3, 5, 7) and (pre >= 105) == (path == "copy")
    assert [(105 * 4 * i) % 16 for i in range(3)] == [0, 4, 8]   # where images 1 and 2 start, relative to image 0's alignment
    fit = cases["ties_fit"]
    for i, n_gt in enumerate(fit["n_gt"]):
        x = fit["d"]["objectness"][0][i].reshape(-1)
        assert (x > 1).sum() == n_gt and (x == 1).sum() == 300 and n_gt + 300 <= 8192 and 0 < 100 - n_gt < 300
        tied = np.nonzero(fit["d"]["objectness"][0][i] == 1)
        assert len(np.unique(tied[0])) == 3 and len(np.unique(tied[1])) > 5   # spread over every A and over the cells
        got = dc.expected_rpn("ties_fit")[0][i]["anchor_index"]
        anchor_logit = fit["d"]["objectness"][0][i].transpose(1, 2, 0).reshape(-1)
        assert np.array_equal(got[n_gt:], np.nonzero(anchor_logit == 1)[0][:100 - n_gt])   # the lowest tied anchors win
    over = cases["ties_overflow"]
    N, per = 12261, -(-12261 // 256)
    assert over["d"]["objectness"][0].shape[1:] == (3, 67, 61) and per * 256 != N and N % per != 0   # uneven thread ranges
    for i, n_gt in enumerate((3000, 2999)):
        x = over["d"]["objectness"][0][i].transpose(1, 2, 0).reshape(-1)
        assert (x > 1).sum() == n_gt and (x == 1).sum() == 9000 and n_gt + 9000 > 8192
        last = np.nonzero(x == 1)[0][6000 - n_gt - 1]   # the last tied anchor taken: inside a thread's range, not at its end
        assert last % per not in (0, per - 1) and x[last + 1:(last // per + 1) * per].tolist().count(1.0) > 0
    for name in ("signed_zero_fit", "signed_zero_overflow"):
        c = cases[name]
        x = c["d"]["objectness"][0]
        assert np.all(x == 0) and np.signbit(x).sum() * 2 == x.size and np.signbit(x[0]).reshape(-1)[:4].tolist() == [True, False, True, False]
        for r in dc.expected_rpn(name)[0]:
            assert np.array_equal(r["anchor_index"], np.arange(c["first_k"])) and np.all(r["objectness"] == F(0.5))
    want = {24: 24, 23: 23, 8: 8, 13: 13}
    for fpn, k in want.items():
        r32, _, diag = dc.expected_rpn("merge_image_%d" % fpn)
        assert [len(r["boxes"]) for r in r32] == [k, k]
        assert fpn == 24 or any(hi == lo for hi, lo in diag["cuts"])   # the cut lies inside a tie
    r = dc.expected_rpn("merge_image_8")[0][0]   # 5, 4.5, 4, 3, then four of the five logits 2: level 0's three, level 1's first
    assert r["level"].tolist() == [0, 1, 0, 0, 0, 0, 0, 1] and r["anchor_index"].tolist() == [0, 0, 1, 2, 3, 4, 5, 1]
    r32, _, diag = dc.expected_rpn("merge_batch_11")
    assert [len(r["boxes"]) for r in r32] == [6, 3, 2] and any(hi == lo == 2 for hi, lo in diag["cuts"])
    assert r32[1]["level"].tolist() == [0, 0, 1] and r32[1]["anchor_index"].tolist() == [0, 1, 0]   # need = 5 ends inside image 1, level 0
    assert [len(r["boxes"]) for r in dc.expected_rpn("merge_batch_100")[0]] == [24, 24, 24]          # total 72 <= fpn: no cut
    r32, _, diag = dc.expected_rpn("min_size_exact")
    assert r32[0]["anchor_index"].tolist() == [5, 0, 3, 6] and sorted(set(diag["sides"].tolist())) [:2] == [7.0, 8.0]


def test_decoder_cases_enter_the_stated_paths():
    cases = dc.box_cases()
    flood = dc.expected_box("tie_flood")[0][0]
    cap = cases["tie_flood"]["prm"]["det_per_img"]
    assert len(flood["orig_inds"]) == 17 > 2 * cap and np.array_equal(flood["orig_inds"], np.arange(17))   # above the 2 x cap rows reserved
    assert len(np.unique(flood["pred_scores"][2:])) == 1
    for name in ("topn_bind", "topn_bind_nodup"):
        r = dc.expected_box(name)[0][0]
        d = cases[name]["imgs"][0]
        assert r["orig_inds"].tolist() == [0, 1, 2] and int(np.argmax(d["class_logits"][:, 1])) == 9
    r = dc.expected_box("class_major_wide")[0][0]
    assert r["pred_labels"].tolist() == [1, 1, 255, 256, 257, 257, 299, 299] and r["orig_inds"].tolist() == [4, 5, 3, 2, 1, 5, 0, 5]
    assert dc.expected_box("class_major_wide_cut")[0][0]["pred_labels"].tolist() == [1, 255, 256, 257]
    big = cases["instances_6144"]
    assert big["prm"]["topn"] == 300 and max(len(d["proposals"]) for d in big["imgs"]) == 2000


# ---- the wrong restatements ------------------------------------------------------------------------------------------------

def _nms_differs(launch_name, **switches):
    launch = _all_nms_launches()[launch_name]
    return not _same(dc.expected_nms(launch), dc.expected_nms(launch, lambda b, s, t: dc.nms_variant(b, s, t, **switches)))


def _box_differs(name, **switches):
    case = dc.box_cases()[name]
    for d, (r32, _, _, _) in zip(case["imgs"], dc.expected_box(name)):
        got = dc.box_variant(d, case["prm"], **switches)
        if not (np.array_equal(got["orig_inds"], r32["orig_inds"]) and np.array_equal(got["pred_labels"], r32["pred_labels"])):
            return True
    return False


def _rpn_differs(name, **switches):
    case = dc.rpn_cases()[name]
    return any(not np.array_equal(g["anchor_index"], w["anchor_index"])
               for g, w in zip(dc.rpn_variant(case["d"], case["c"], **switches), dc.expected_rpn(name)[0]))


def test_every_wrong_restatement_changes_an_expected_result():
    assert _nms_differs("threshold_half", ge=True)                              # `>=` at the threshold
    for form in dc.IOU_FORMS:                                                   # each of the four IoU forms, at its own threshold
        assert _nms_differs("threshold_" + form, form=form), form
    for name in ("ladder_perm_128", "ladder_equal_6144", "inblock_bits"):       # suppression by a removed box
        assert _nms_differs(name, skip_removed=False), name
    launch = dc.nms_launches()["cap_by_index"]                                  # a cap by score instead of by index
    for (boxes, scores), want in zip(launch["segs"], dc.expected_nms(launch)):
        keep = np_nms(boxes, scores, launch["thr"])
        assert not np.array_equal(np.sort(keep[dc.score_order(scores[keep])[:launch["max_keep"]]]), want)
    assert _box_differs("topn_bind", topn_by_score=True) and _box_differs("topn_bind_nodup", topn_by_score=True)
    for C in (2, 4):
        assert _box_differs("score_thresh_C%d_at" % C, ge_score=True)          # `>=` at SCORE_THRESH
    assert _box_differs("row_max_ties", last_col=True)                          # last column on row_max ties
    assert _nms_differs("signed_zero_ladder", signed_zero=True)                 # signed zeros ordered
    assert _rpn_differs("signed_zero_fit", signed_zero=True) and _rpn_differs("signed_zero_overflow", signed_zero=True)
    assert _rpn_differs("ties_fit", highest_anchor=True) and _rpn_differs("ties_overflow", highest_anchor=True)
    assert _rpn_differs("min_size_exact", gt_min_size=True)                     # `>` at min_size
    # the threshold pairs decide the same way through the RPN's and the decoder's NMS
    _, _, sup = dc.bulk_pairs()
    kept = set(dc.expected_rpn("pairs_half")[0][0]["anchor_index"].tolist())
    assert [2 * i + 1 not in kept for i in range(len(sup))] == sup.tolist() and all(2 * i in kept for i in range(len(sup)))
    rows = set(dc.expected_box("pairs_half")[0][0]["orig_inds"].tolist())
    assert [2 * i + 1 not in rows for i in range(len(sup))] == sup.tolist()
