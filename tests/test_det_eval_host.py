"""CPU premises of the detection-evaluator tests: the two numpy restatements of COCOeval (tests/det_eval_cases.py) agree bit for
bit on every case, both give the hand-derived numbers below, every wrong variant changes a result on the case built for it, and
the geometric premises of the threshold cases hold in double.  The restatements have never been run against pycocotools."""
import numpy as np
import pytest

import det_eval_cases as dc
from det_eval_cases import EPS, IOU_THRS, REC_THRS

P1 = 1.0 / (1.0 + EPS)          # the precision of "one TP, no FP": 0.9999999999999998, not 1
ALL, SMALL, MEDIUM, LARGE = range(4)
HAND = ("perfect_id1", "perfect_id0", "two_on_one", "between_two", "prefer_nonignored", "unmatched_outside", "iou_at_threshold",
        "iou_below_threshold", "f32_width", "score_ties", "maxdets", "empties", "gt_only_first_batch", "gt_only_split", "no_updates")


@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_the_two_restatements_agree_bit_for_bit(name):
    case = dc.cases()[name]
    lit = dc.expected(name)
    flat = dc.np_coco_eval_flat(dc.flat_images(case), case["num_classes"], case["first_gt_id"])
    assert np.array_equal(lit["precision"], flat["precision"])
    assert np.array_equal(lit["recall"], flat["recall"])
    assert np.array_equal(lit["stats"], flat["stats"]) and lit["recall50_100"] == flat["recall50_100"]


def test_thresholds_are_the_values_the_cases_assume():
    assert IOU_THRS[0] == 0.5 and IOU_THRS[5] == 0.75 and len(IOU_THRS) == 10
    assert REC_THRS[0] == 0.0 and REC_THRS[50] == 0.5 and REC_THRS[100] == 1.0 and len(REC_THRS) == 101
    assert 0.81 < IOU_THRS[7] <= 1.0 and IOU_THRS[1] > 0.5 and 0.6 < IOU_THRS[3] < 2.0 / 3.0
    assert 2.0 + EPS == 2.0 and 10.0 + EPS == 10.0 and P1 == 1.0 - 2.0 ** -52


def test_perfect_detections_and_the_annotation_id_quirk():
    one, zero = dc.expected("perfect_id1"), dc.expected("perfect_id0")
    p, r = one["precision"], one["recall"]
    # class 1: a 10 x 10 box (all, small) in image 0 and a 110 x 110 one (all, large) in image 1; class 2: a 50 x 50 box (all, medium)
    populated = np.zeros((2, 4), bool)
    populated[0, [ALL, SMALL, LARGE]] = True
    populated[1, [ALL, MEDIUM]] = True
    assert np.all(r[:, populated] == 1.0) and np.all(r[:, ~populated] == -1.0)
    assert np.all(p[:, :, ~populated] == -1.0)
    # class 1 / all: tp = [1, 2], pr = [1/(1+eps), 2/(2+eps) = 1]: the maximum over rc >= thr always includes the last -> exactly 1.
    # every other populated cell ends at one TP (the other detection is matched to an ignored GT box): 1/(1+eps)
    assert np.all(p[:, :, 0, ALL, :] == 1.0)
    assert np.all(p[:, :, 0, [SMALL, LARGE], :] == P1) and np.all(p[:, :, 1, [ALL, MEDIUM], :] == P1)
    # first_gt_id = 0: the 0.9 detection of class 1 sits on annotation 0 and counts as unmatched.
    #   all:   records FP, TP: tp = [0, 1], fp = [1, 1], rc = [0, .5], pr = [0, 1/(2+eps) = .5] -> .5 up to recall .5, then 0
    #   small: the FP alone (the other detection is ignored): precision 0, recall 0
    #   large: its GT box is ignored there, so is the detection: as before
    p0, r0 = zero["precision"], zero["recall"]
    assert np.all(p0[:, :51, 0, ALL, :] == 0.5) and np.all(p0[:, 51:, 0, ALL, :] == 0.0) and np.all(r0[:, 0, ALL, :] == 0.5)
    assert np.all(p0[:, :, 0, SMALL, :] == 0.0) and np.all(r0[:, 0, SMALL, :] == 0.0)
    differs = np.zeros(p.shape, bool)
    differs[:, :, 0, [ALL, SMALL], :] = True
    assert np.array_equal(p != p0, differs)
    assert np.array_equal(r != r0, differs[:, 0])


def test_two_detections_on_one_gt_box():
    e = dc.expected("two_on_one")
    # by score: 0.9 takes the box (TP), 0.6 is a FP: tp = [1, 1], fp = [0, 1], rc = [1, 1], pr = [1/(1+eps), .5]
    assert np.all(e["precision"][:, :, 0, [ALL, SMALL], :] == P1) and np.all(e["recall"][:, 0, [ALL, SMALL], :] == 1.0)


def test_one_detection_between_two_gt_boxes():
    e = dc.expected("between_two")
    dets = dc.flat_images(dc.cases()["between_two"])[0]
    d1, g10, g11 = dc.det_xywh(dets["pred_boxes"][0]), dc.gt_xywh(dets["gt_boxes"][0]), dc.gt_xywh(dets["gt_boxes"][1])
    assert dc.bb_iou(d1, g10) == dc.bb_iou(d1, g11) == 150.0 / 250.0
    d2, g20, g21 = dc.det_xywh(dets["pred_boxes"][2]), dc.gt_xywh(dets["gt_boxes"][2]), dc.gt_xywh(dets["gt_boxes"][3])
    assert dc.bb_iou(d2, g20) == 160.0 / 240.0 > dc.bb_iou(d2, g21) == 140.0 / 260.0 > 0.5
    # class 1, threshold .5: equal IoU -> the LATER box; the second detection sits on that box (IoU 1/3 with the other): FP.
    # tp = [1, 1], fp = [0, 1], npig = 2 -> recall .5, precision 1/(1+eps) up to recall .5.  (The earlier box: recall 1.)
    assert e["recall"][0, 0, ALL, 2] == 0.5 and e["precision"][0, 0, 0, ALL, 2] == P1 and e["precision"][0, 51, 0, ALL, 2] == 0.0
    # threshold .65: the first detection (IoU .6) is a FP, the second a TP: tp = [0, 1], fp = [1, 1] -> pr = [0, .5]
    assert e["recall"][3, 0, ALL, 2] == 0.5 and e["precision"][3, 0, 0, ALL, 2] == 0.5
    # class 2: IoU 2/3 with the first box, 7/13 with the second -> the first; the second detection sits on the first box: FP
    assert e["recall"][0, 1, ALL, 2] == 0.5 and e["precision"][0, 0, 1, ALL, 2] == P1


def test_ignored_gt_boxes():
    e = dc.expected("prefer_nonignored")
    # medium, threshold .5: the 90 x 90 box (IoU .81, not ignored) is taken although the ignored 100 x 100 one has IoU 1: two TPs of two
    assert e["recall"][0, 0, MEDIUM, 2] == 1.0 and np.all(e["precision"][0, :, 0, MEDIUM, 2] == 1.0)
    # medium, threshold .85: only the ignored box matches -> the detection is neither TP nor FP; the 0.3 detection of image 1 is the
    # one TP of two GT boxes: tp = [0, 1], fp = [0, 0] -> pr = [0, 1/(1+eps)] (a FP in front would give .5)
    assert e["recall"][7, 0, MEDIUM, 2] == 0.5 and e["precision"][7, 0, 0, MEDIUM, 2] == P1
    # all: the 100 x 100 box first (IoU 1), the .81 does not beat it: 2 TPs of 3 GT boxes
    assert e["recall"][0, 0, ALL, 2] == 2.0 / 3.0
    e = dc.expected("unmatched_outside")
    # the unmatched 5 x 5 detection of score .9: FP for "all" (pr = [0, .5]), ignored for "medium" (pr = [0, 1/(1+eps)])
    assert np.all(e["precision"][:, :, 0, ALL, 2] == 0.5) and np.all(e["precision"][:, :, 0, MEDIUM, 2] == P1)
    assert np.all(e["recall"][:, 0, [ALL, MEDIUM], 2] == 1.0) and np.all(e["precision"][:, :, 0, SMALL, :] == -1.0)


def test_iou_at_and_just_below_a_threshold():
    at, below = dc.cases()["iou_at_threshold"]["batches"][0][0], dc.cases()["iou_below_threshold"]["batches"][0][0]
    for j, thr in ((0, IOU_THRS[0]), (1, IOU_THRS[5])):
        assert dc.bb_iou(dc.det_xywh(at["pred_boxes"][j]), dc.gt_xywh(at["gt_boxes"][j])) == thr
        assert dc.bb_iou(dc.det_xywh(below["pred_boxes"][j]), dc.gt_xywh(below["gt_boxes"][j])) == np.nextafter(thr, 0.0)
    e = dc.expected("iou_at_threshold")          # >= : a match at the threshold itself, none above it
    assert np.array_equal(e["recall"][:, 0, ALL, 2], [1.0] + [0.0] * 9) and np.array_equal(e["recall"][:, 1, ALL, 2], [1.0] * 6 + [0.0] * 4)
    e = dc.expected("iou_below_threshold")       # one double below: no match at that threshold
    assert np.array_equal(e["recall"][:, 0, ALL, 2], [0.0] * 10) and np.array_equal(e["recall"][:, 1, ALL, 2], [1.0] * 5 + [0.0] * 5)


def test_float32_width_changes_a_decision():
    im = dc.cases()["f32_width"]["batches"][0][0]
    g = dc.gt_xywh(im["gt_boxes"][0])
    assert dc.det_xywh(im["pred_boxes"][0])[2] == 2.0 ** 21 and dc.det_xywh(im["pred_boxes"][0], double_width=True)[2] == 2.0 ** 21 - 2.0 ** -5
    assert dc.bb_iou(dc.det_xywh(im["pred_boxes"][0]), g) == 0.5 > dc.bb_iou(dc.det_xywh(im["pred_boxes"][0], double_width=True), g)
    assert dc.expected("f32_width")["recall"][0, 0, ALL, 2] == 1.0
    assert dc.np_coco_eval([im], 3, 1, mut="double_width")["recall"][0, 0, ALL, 2] == 0.0


def test_score_ties_keep_image_then_index_order():
    case = dc.cases()["score_ties"]
    e = dc.expected("score_ties")
    # records TP FP | TP TP, npig = 3: tp = [1, 1, 2, 3], fp = [0, 1, 1, 1], rc = [1/3, 1/3, 2/3, 1], pr = [1/(1+eps), .5, 2/3, .75]
    assert e["precision"][0, 0, 0, ALL, 2] == P1 and e["precision"][0, 34, 0, ALL, 2] == 0.75 and e["precision"][0, 100, 0, ALL, 2] == 0.75
    assert REC_THRS[33] <= 1.0 / 3.0 < REC_THRS[34] and e["precision"][0, 33, 0, ALL, 2] == P1
    # the zeros of both signs are equal scores: class 2 reads as class 1
    assert np.array_equal(e["precision"][:, :, 1], e["precision"][:, :, 0]) and np.array_equal(e["recall"][:, 1], e["recall"][:, 0])
    for tie in dc.TIE_ORDERS:
        wrong = dc.np_coco_eval(dc.flat_images(case), 3, 1, tie=tie)
        for k in (0, 1):
            assert not np.array_equal(wrong["precision"][:, :, k], e["precision"][:, :, k]), (tie, k)


def test_max_dets_cut_per_image_and_class():
    e = dc.expected("maxdets")
    # rank 0 a FP, rank 9 a TP, rank 50 a TP, rank 110 beyond the cut: recall 0, 1/3, 2/3 of 3 GT boxes; at 10: pr[9] = 1/(10+eps) = .1
    assert np.array_equal(e["recall"][0, 0, ALL, :], [0.0, 1.0 / 3.0, 2.0 / 3.0])
    assert e["precision"][0, 0, 0, ALL, 0] == 0.0 and e["precision"][0, 0, 0, ALL, 1] == 1.0 / 10.0 and e["precision"][0, 34, 0, ALL, 1] == 0.0


def test_empty_things():
    e = dc.expected("empties")
    # class 1: a GT box (all, small), no detection -> 0; class 2: detections, no GT box -> -1
    assert np.all(e["precision"][:, :, 0, [ALL, SMALL], :] == 0.0) and np.all(e["recall"][:, 0, [ALL, SMALL], :] == 0.0)
    assert np.all(e["precision"][:, :, 0, [MEDIUM, LARGE], :] == -1.0) and np.all(e["precision"][:, :, 1] == -1.0) and np.all(e["recall"][:, 1] == -1.0)
    # class 3: two medium GT boxes; a FAR 10 x 10 FP of score .8 (ignored for medium), a TP of score .7
    assert np.all(e["precision"][:, :51, 2, ALL, 2] == 0.5) and np.all(e["precision"][:, 51:, 2, ALL, 2] == 0.0)
    assert np.all(e["precision"][:, :51, 2, MEDIUM, 2] == P1) and np.all(e["recall"][:, 2, [ALL, MEDIUM], 2] == 0.5)
    e = dc.expected("no_updates")
    assert np.all(e["precision"] == -1.0) and np.all(e["recall"] == -1.0) and np.all(e["stats"] == -1.0) and e["recall50_100"] == -1.0


def test_batches_and_splits_without_a_detection():
    e = dc.expected("gt_only_first_batch")
    # class 1: two 10 x 10 GT boxes (all, small), the first in the batch without detections.  Records TP (.9), FP (.4, a 10 x 10 box):
    # tp = [1, 1], fp = [0, 1], rc = [.5, .5], pr = [1/(1+eps), .5] -> 1/(1+eps) up to recall .5, then 0; at maxDets 1 the TP alone: the same
    assert np.all(e["precision"][:, :51, 0, [ALL, SMALL], :] == P1) and np.all(e["precision"][:, 51:, 0, [ALL, SMALL], :] == 0.0)
    assert np.all(e["recall"][:, 0, [ALL, SMALL], :] == 0.5) and np.all(e["recall"][:, 0, [MEDIUM, LARGE], :] == -1.0)
    # class 2: a 50 x 50 GT box (all, medium) of that batch, never detected
    assert np.all(e["precision"][:, :, 1, [ALL, MEDIUM], :] == 0.0) and np.all(e["recall"][:, 1, [ALL, MEDIUM], :] == 0.0)
    assert np.all(e["precision"][:, :, 1, [SMALL, LARGE], :] == -1.0)
    e = dc.expected("gt_only_split")
    # no detection anywhere: 0 where the (class, area) has a GT box, -1 elsewhere; every mean is over zeros
    populated = np.zeros((2, 4), bool)
    populated[0, [ALL, SMALL, LARGE]] = True
    populated[1, [ALL, MEDIUM]] = True
    assert np.all(e["precision"][:, :, populated] == 0.0) and np.all(e["precision"][:, :, ~populated] == -1.0)
    assert np.all(e["recall"][:, populated] == 0.0) and np.all(e["recall"][:, ~populated] == -1.0)
    assert np.all(e["stats"] == 0.0) and e["recall50_100"] == 0.0
    for name in ("gt_only_first_batch", "gt_only_split"):
        assert not any(len(im["obj_scores"]) for im in dc.cases()[name]["batches"][0])


MUTATION_CASES = {"gt_strict": "iou_at_threshold", "double_width": "f32_width", "no_break": "prefer_nonignored", "unstable": "score_ties",
                  "side_right": "two_on_one", "no_envelope": "score_ties", "ignore_first_id": "perfect_id0", "late_cut": "perfect_id1"}


def test_every_wrong_restatement_changes_an_expected_result():
    assert set(MUTATION_CASES) == set(dc.MUTATIONS)
    for mut, name in MUTATION_CASES.items():
        case = dc.cases()[name]
        wrong = dc.np_coco_eval(dc.flat_images(case), case["num_classes"], case["first_gt_id"], mut=mut)
        good = dc.expected(name)
        changed = int((wrong["precision"] != good["precision"]).sum() + (wrong["recall"] != good["recall"]).sum())
        print("mutation %-16s on %-18s changes %d cells" % (mut, name, changed))
        assert changed > 0, mut


def test_segment_cases_have_the_segment_lengths_and_totals_they_are_named_for():
    B = dc.SCAN_CHUNK
    for total in (dc.SORT_TILE - 1, dc.SORT_TILE, dc.SORT_TILE + 1):
        case = dc.cases()["segments_%d" % total]
        assert len(case["batches"]) == 2
        images = dc.flat_images(case)
        assert sum(len(im["obj_scores"]) for im in images) == total
        counted = np.zeros(9, np.int64)
        for im in images:
            counted += np.minimum(np.bincount(im["pred_classes"], minlength=9), 100)
        assert counted[1:].tolist() == [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7]
    real = dc.cases()["realistic"]
    assert [len(b) for b in real["batches"]] == [16] * 4 and real["num_classes"] == 151
    scores = np.concatenate([im["obj_scores"] for im in dc.flat_images(real)])
    assert len(np.unique(scores)) < len(scores)          # ties occur
