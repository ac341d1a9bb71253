"""The detector's inference side on the MI355X, every instance, edge and tie: nms.hip (nms_kernel through layers.batched_nms,
nms_fixed_kernel through rpn_proposals, class_nms_kernel through box_postprocess, each in its 256 / 1024 / 6144 instance; the box
decoder, row_max_kernel, select_kernel), rpn.hip (select, batch cut, emit) and the shared selection.h, on the inputs of
tests/detect_cases.py (premises: tests/test_detect_cases_host.py).

Exact, compared with ==: keep lists and counts of veto_nms; orig_inds, labels and counts of the decoder; counts, level and
anchor_index of the RPN -- against np_nms / np_box_postprocess / np_rpn_proposals in float32, and against the closed form where
the case has one.  Boxes, scores and objectness: within 4x the float32 restatement's own error against its float64 form on the
same inputs, computed here and printed; on the exact cases (zero regressions, equal logits) that error is 0 and the comparison
is bit for bit, and so it is on the `shift_only` cases (regressions that shift and do not scale: every expf result is 1).  No
case is left out.  Every figure is printed before it is asserted (pytest -s: "detect_parity:" lines)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


_instance = dc.nms_instance


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _paired_error(got, want32, want64, keys, fields):
    """Largest |got - float32 restatement| and |float32 - float64 restatement| per field.  got and the float32 restatement hold
    the same rows (asserted before); the float64 restatement may hold others (the threshold pairs are built for that): its rows
    are matched by `keys`."""
    idx64 = {tuple(int(want64[k][r]) for k in keys): r for r in range(len(want64[keys[0]]))}
    rows = [(r, idx64[t]) for r, t in enumerate(zip(*[want32[k].tolist() for k in keys])) if t in idx64]
    a, b = [r for r, _ in rows], [r for _, r in rows]
    out = {}
    for f in fields:
        dev_err = float(np.abs(got[f].astype(np.float64) - want32[f]).max(initial=0))
        ref_err = float(np.abs(want32[f][a].astype(np.float64) - want64[f][b]).max(initial=0))
        out[f] = (dev_err, ref_err)
    return out


# ---- veto_nms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.NMS_LAUNCH_NAMES)
def test_nms_launch_keeps_what_the_restatement_keeps(name):
    from veto_amd.layers import batched_nms
    launch = dc.all_nms_launches()[name]
    boxes, scores, off = dc.pack(launch)
    keep, counts = batched_nms(_dev(boxes), _dev(scores), off.tolist(), launch["thr"], max_keep=launch["max_keep"])
    keep, counts = keep.cpu().numpy(), counts.cpu().numpy()
    want = dc.expected_nms(launch)
    got = [keep[off[s]:off[s] + counts[s]] for s in range(len(want))]
    bad = [s for s in range(len(want)) if not np.array_equal(got[s], want[s])]
    largest = int(np.diff(off).max())
    print("detect_parity: nms %-24s nms_kernel<%d> thr %.9g cap %d: %d segments, largest %d, %d boxes, kept %d (expected %d), "
          "segments that differ: %s" % (name, _instance(largest), launch["thr"], launch["max_keep"], len(want), largest, len(boxes),
                                        int(counts.sum()), sum(len(w) for w in want), bad))
    assert counts.tolist() == [len(w) for w in want]
    assert not bad
    if "closed_form" in launch:
        for g, c in zip(got, launch["closed_form"]):
            np.testing.assert_array_equal(g, c)


# ---- veto_box_postprocess ---------------------------------------------------------------------------------------------------

def _run_box(case):
    from veto_amd.boxhead import box_postprocess
    imgs, prm = case["imgs"], case["prm"]
    cat = lambda k: _dev(np.concatenate([d[k] for d in imgs]))   # noqa: E731
    return box_postprocess(cat("class_logits"), cat("box_regression"), cat("proposals"), [len(d["proposals"]) for d in imgs],
                           [d["image_size"] for d in imgs], score_thresh=prm["score_thresh"], nms=prm["nms"],
                           post_nms_per_cls_topn=prm["topn"], nms_filter_duplicates=prm["filter_dup"],
                           detections_per_img=prm["det_per_img"], reg_weights=prm["weights"], cls_agnostic_bbox_reg=prm["cls_agnostic"])


@pytest.mark.parametrize("name", dc.BOX_CASE_NAMES)
def test_decoder_case_matches_the_restatement(name):
    case = dc.box_cases()[name]
    outs = _run_box(case)
    want = dc.expected_box(name)
    assert len(outs) == len(want)
    largest = max(len(d["proposals"]) for d in case["imgs"])
    err = {"pred_scores": [0.0, 0.0], "boxes": [0.0, 0.0], "boxes_per_cls": [0.0, 0.0]}
    counts, bad = [], []
    for i, (o, (r32, r64, _, _)) in enumerate(zip(outs, want)):
        got = {k: v.cpu().numpy() for k, v in o.items()}
        counts.append(len(got["orig_inds"]))
        if not (np.array_equal(got["orig_inds"], r32["orig_inds"]) and np.array_equal(got["pred_labels"], r32["pred_labels"])):
            bad.append(i)
            continue
        for f, (d, r) in _paired_error(got, r32, r64, ("orig_inds", "pred_labels"), tuple(err)).items():
            err[f] = [max(err[f][0], d), max(err[f][1], r)]
    print("detect_parity: box %-28s class_nms_kernel<%d> C %d: images %s -> detections %s (expected %s), images that differ: %s; "
          "device error / float32 restatement's own: scores %.3e / %.3e, boxes %.3e / %.3e, boxes_per_cls %.3e / %.3e"
          % (name, _instance(largest), case["imgs"][0]["class_logits"].shape[1], [len(d["proposals"]) for d in case["imgs"]], counts,
             [len(w[0]["orig_inds"]) for w in want], bad, err["pred_scores"][0], err["pred_scores"][1], err["boxes"][0], err["boxes"][1],
             err["boxes_per_cls"][0], err["boxes_per_cls"][1]))
    assert not bad
    for f, (d, r) in err.items():
        assert d <= 4 * r, (name, f, d, r)
    if case.get("bitwise"):   # no expf result other than 1: BoxCoder.decode operation for operation
        assert err["boxes"][0] == 0 and err["boxes_per_cls"][0] == 0, (name, err)
    if "labels" in case:
        assert outs[0]["pred_labels"].tolist() == case["labels"]


# ---- veto_rpn_proposals -----------------------------------------------------------------------------------------------------

def _run_rpn(case):
    from veto_amd.rpn import rpn_proposals
    d, c = case["d"], case["c"]
    return rpn_proposals([_dev(o) for o in d["objectness"]], [_dev(r) for r in d["box_regression"]], [_dev(a) for a in d["anchors"]],
                         list(c["images"]), pre_nms_top_n=c["pre"], post_nms_top_n=c["post"], nms_thresh=c["thr"], min_size=c["min_size"],
                         fpn_post_nms_top_n=c["fpn"], per_batch=bool(c.get("training") and c.get("per_batch")))


@pytest.mark.parametrize("name", dc.RPN_CASE_NAMES)
def test_rpn_case_matches_the_restatement(name):
    case = dc.rpn_cases()[name]
    outs = _run_rpn(case)
    r32, r64, _ = dc.expected_rpn(name)
    assert len(outs) == len(r32)
    shapes = [tuple(o.shape[1:]) for o in case["d"]["objectness"]]
    capacity = max(min(case["c"]["pre"], a * h * w) for a, h, w in shapes)
    err = {"boxes": [0.0, 0.0], "objectness": [0.0, 0.0]}
    counts, bad = [], []
    for i, (o, a, b) in enumerate(zip(outs, r32, r64)):
        got = {k: v.cpu().numpy() for k, v in o.items()}
        counts.append(len(got["boxes"]))
        if not (np.array_equal(got["level"], a["level"]) and np.array_equal(got["anchor_index"], a["anchor_index"])):
            bad.append(i)
            continue
        for f, (d, r) in _paired_error(got, a, b, ("level", "anchor_index"), tuple(err)).items():
            err[f] = [max(err[f][0], d), max(err[f][1], r)]
    print("detect_parity: rpn %-22s nms_fixed_kernel<%s> planes %s x %d images, k %d: rows %s (expected %s), images that differ: %s; "
          "device error / float32 restatement's own: boxes %.3e / %.3e, objectness %.3e / %.3e"
          % (name, _instance(capacity) if case["c"]["thr"] > 0 else "-", shapes, len(outs), case["c"]["pre"], counts,
             [len(a["boxes"]) for a in r32], bad, err["boxes"][0], err["boxes"][1], err["objectness"][0], err["objectness"][1]))
    assert not bad
    for f, (d, r) in err.items():
        assert d <= 4 * r, (name, f, d, r)
    if case.get("bitwise"):   # no expf result other than 1: BoxCoder.decode operation for operation
        assert err["boxes"][0] == 0, (name, err)


def test_signed_zeros_are_one_logit():
    """+0.0 and -0.0 are equal in every documented order (and in the reference's sort): the selection falls through to the
    anchor index, the NMS to the box index; the objectness of either is 0.5."""
    for name in ("signed_zero_fit", "signed_zero_overflow"):
        case = dc.rpn_cases()[name]
        for i, o in enumerate(_run_rpn(case)):
            got = o["anchor_index"].cpu().numpy()
            print("detect_parity: signed zeros %-22s image %d: first anchors %s" % (name, i, got[:8].tolist()))
            np.testing.assert_array_equal(got, np.arange(case["first_k"]))
            assert bool((o["objectness"] == 0.5).all())
