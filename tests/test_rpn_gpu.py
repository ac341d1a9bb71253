"""RPN proposal selection on the MI355X: veto_rpn_proposals against the reference's fixtures (tests/golden/rpn/) through
rpn_proposals and through RPNPostProcessor, batch independence, workspace reuse, the hand-over to the box head's decoder, the
capacity rule and the refusals.

Exact: the per-image counts, the pyramid level and the anchor index of every row.  Toleranced (results of exp): boxes and
objectness, at 4x the error of the reference's own fp32 arithmetic against fp64, which the generator measured and stored per
fixture (ref_fp32_err_boxes ~5e-5 px, ref_fp32_err_objectness ~8e-8; 0 for the boxes of `ties`, which are exact).  Every figure
is printed before it is asserted (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rpn_host import CASES, GOLDEN, case_inputs, fixture_rows, np_rpn_proposals, rpn_targets  # noqa: E402

from veto_amd import native, synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def _case(name):
    """(fixture, case settings, device inputs), loaded once and left unchanged."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        d = case_inputs(name, int(z["seed"]))
        _CACHE[name] = (z, CASES[name], {k: [torch.from_numpy(x).to(DEV) for x in v] for k, v in d.items()})
    return _CACHE[name]


def _settings(c):
    return dict(pre_nms_top_n=c["pre"], post_nms_top_n=c["post"], nms_thresh=c["thr"], min_size=c["min_size"],
                fpn_post_nms_top_n=c["fpn"], per_batch=bool(c.get("training") and c.get("per_batch")))


def _run(name, images=None):
    from veto_amd.rpn import rpn_proposals
    _, c, t = _case(name)
    idx = list(range(len(c["images"]))) if images is None else list(images)
    return rpn_proposals([o[idx] for o in t["objectness"]], [r[idx] for r in t["box_regression"]], t["anchors"],
                         [c["images"][i] for i in idx], **_settings(c))


def _compare(name, outs, z, n_gt=0, gt_present=False):
    tol_b, tol_o = 4 * float(z["ref_fp32_err_boxes"]), 4 * float(z["ref_fp32_err_objectness"])
    err_b = err_o = 0.0
    want_rows = fixture_rows(z)
    assert len(outs) == len(want_rows)
    for i, (o, want) in enumerate(zip(outs, want_rows)):
        k = len(want["boxes"]) - (0 if gt_present else n_gt)
        got = {key: v.cpu().numpy() for key, v in o.items()}
        assert len(got["boxes"]) == k, (name, i, len(got["boxes"]), k)
        if "level" in got:
            m = k - (n_gt if gt_present else 0)
            assert got["level"].dtype == np.int32 and got["anchor_index"].dtype == np.int64
            np.testing.assert_array_equal(got["level"], want["level"][:m], err_msg="%s image %d" % (name, i))
            np.testing.assert_array_equal(got["anchor_index"], want["anchor_index"][:m], err_msg="%s image %d" % (name, i))
        err_b = max(err_b, np.abs(got["boxes"] - want["boxes"][:k]).max(initial=0))
        err_o = max(err_o, np.abs(got["objectness"] - want["objectness"][:k]).max(initial=0))
    print("%s: device error boxes %.3e (allowed %.3e), objectness %.3e (allowed %.3e)" % (name, err_b, tol_b, err_o, tol_o))
    assert err_b <= tol_b, (name, err_b, tol_b)
    assert err_o <= tol_o, (name, err_o, tol_o)


@pytest.mark.parametrize("name", sorted(CASES))
def test_functional_entry_matches_every_fixture(name):
    z, c, _ = _case(name)
    outs = _run(name)
    _compare(name, outs, z, n_gt=c.get("add_gt", 0))
    second = np_rpn_proposals(case_inputs(name, int(z["seed"])), c)   # the second yardstick agrees on the exact quantities too
    for o, s in zip(outs, second):
        np.testing.assert_array_equal(o["level"].cpu().numpy(), s["level"])
        np.testing.assert_array_equal(o["anchor_index"].cpu().numpy(), s["anchor_index"])


@pytest.mark.parametrize("name", ["small5", "per_batch", "add_gt"])
def test_module_forward_matches_the_fixture(name):
    from veto_amd.rpn import RPNPostProcessor
    z, c, t = _case(name)
    n_gt = c.get("add_gt", 0)
    post = RPNPostProcessor(c["pre"], c["post"], c["thr"], c["min_size"], None, c["fpn"], bool(c.get("per_batch", False)), bool(n_gt))
    post.train(bool(c.get("training", False)))
    anchors = [[BoxList(a, size, "xyxy") for a in t["anchors"]] for size in c["images"]]
    targets = [BoxList(torch.from_numpy(b).to(DEV), size, "xyxy") for b, size in
               zip(rpn_targets(int(z["seed"]), c["images"], n_gt), c["images"])] if n_gt else None
    res = post(anchors, t["objectness"], t["box_regression"], targets)
    for r, size in zip(res, c["images"]):
        assert type(r) is BoxList and r.mode == "xyxy" and r.size == size and r.bbox.device.type == "cuda"
        assert r.get_field("objectness").shape == (len(r),)
    _compare(name + "/module", [dict(boxes=r.bbox, objectness=r.get_field("objectness")) for r in res], z, n_gt=n_gt, gt_present=True)
    if n_gt:   # eval mode appends nothing
        res = post.eval()(anchors, t["objectness"], t["box_regression"], targets)
        assert [len(r) for r in res] == [int(k) - n_gt for k in z["counts"]]


def _equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for key in x:
            assert torch.equal(x[key], y[key]), key


def test_a_batch_equals_its_images_one_at_a_time():
    batch = _run("small5")
    for i in range(3):
        _equal(_run("small5", [i]), batch[i:i + 1])


def test_workspace_reuse_across_larger_and_smaller_batches():
    first = _run("small5", [1])
    _run("full_level")                      # a larger workspace on the same stream
    z, c, _ = _case("one_level")
    _compare("one_level after full_level", _run("one_level"), z)
    _equal(_run("small5", [1]), first)      # and a smaller batch again
    z, c, _ = _case("small5")
    _compare("small5 after the others", _run("small5"), z)


def test_many_ties_at_the_cut_take_the_lowest_anchors():
    """More equal logits at the pre-NMS cut than the select can sort (8 400 zeros, 300 wanted): the lowest anchor indices win,
    as the total order (logit desc, anchor asc) says.  Expected values from that order alone: NMS is off, the anchors pass
    through the decoder unchanged (zero regression), so row r is anchor r."""
    from veto_amd.rpn import rpn_proposals
    H, W, A = 40, 70, 3
    anchors = synth.anchor_grid((64,), (8,), (0.5, 1.0, 2.0), ((H, W),))[0]
    obj = torch.zeros((1, A, H, W), device=DEV)
    obj[0, 1, 0, 0] = 1.0                   # anchor 1 is the one logit above the tie
    out = rpn_proposals([obj], [torch.zeros((1, 4 * A, H, W), device=DEV)], [torch.from_numpy(anchors).to(DEV)], [(10000, 10000)],
                        pre_nms_top_n=300, post_nms_top_n=0, nms_thresh=0.0, min_size=-1e9)[0]
    want = np.array([1, 0] + list(range(2, 300)))
    np.testing.assert_array_equal(out["anchor_index"].cpu().numpy(), want)
    np.testing.assert_array_equal(out["level"].cpu().numpy(), np.zeros(300, np.int32))
    assert float(out["objectness"][1]) == 0.5 and float(out["objectness"][0]) > 0.73


def test_proposals_feed_the_box_head_decoder_unchanged():
    """small5's proposals go into boxhead.box_postprocess with synthetic head outputs; the result equals the same call fed with
    the fixture's proposals (the decoder rounds its inputs' last bits away in nothing it decides: same rows, same labels)."""
    from veto_amd.boxhead import box_postprocess
    z, c, _ = _case("small5")
    outs = _run("small5")
    n_per_img = [len(o["boxes"]) for o in outs]
    assert n_per_img == [int(k) for k in z["counts"]]
    n, C = sum(n_per_img), 21
    logits = torch.from_numpy(synth.uniform(7, "rpn.handover.logits", (n, C), -3.0, 3.0)).to(DEV)
    reg = torch.from_numpy(synth.normal(7, "rpn.handover.reg", (n, 4 * C), 0.0, 0.3)).to(DEV)
    kw = dict(score_thresh=0.05, nms=0.5, post_nms_per_cls_topn=300, nms_filter_duplicates=True, detections_per_img=100)
    mine = box_postprocess(logits, reg, torch.cat([o["boxes"] for o in outs]), n_per_img, c["images"], **kw)
    ref = box_postprocess(logits, reg, torch.from_numpy(z["boxes"]).to(DEV), n_per_img, c["images"], **kw)
    tol = 4 * float(z["ref_fp32_err_boxes"]) * 4   # a decoded side is at most exp(dw) ~ 3x the proposal's error, plus the centre's
    for a, b in zip(mine, ref):
        assert len(a["orig_inds"]) > 0
        assert torch.equal(a["orig_inds"], b["orig_inds"]) and torch.equal(a["pred_labels"], b["pred_labels"])
        assert torch.equal(a["pred_scores"], b["pred_scores"])
        err = float((a["boxes"] - b["boxes"]).abs().max())
        print("hand-over: decoded boxes differ by %.3e (allowed %.3e)" % (err, tol))
        assert err <= tol


def test_too_few_rows_report_the_count_and_leave_the_rows_untouched():
    from veto_amd.rpn import rpn_proposals_padded
    z, c, t = _case("small5")
    rows = [150, 10, 150]
    out = dict(boxes=torch.full((310, 4), -7.0, device=DEV), objectness=torch.full((310,), -7.0, device=DEV),
               level=torch.full((310,), -7, dtype=torch.int32, device=DEV), anchor_index=torch.full((310,), -7, dtype=torch.int64, device=DEV))
    caps, out, kept = rpn_proposals_padded(t["objectness"], t["box_regression"], t["anchors"], c["images"], rows_per_image=rows, out=out,
                                           **_settings(c))
    assert caps == rows and kept == [150, -150, 150]
    for v in out.values():
        assert bool((v[150:160] == -7).all())
    want = fixture_rows(z)
    np.testing.assert_array_equal(out["anchor_index"][:150].cpu().numpy(), want[0]["anchor_index"])
    np.testing.assert_array_equal(out["anchor_index"][160:].cpu().numpy(), want[2]["anchor_index"])


def test_refusals_come_before_any_launch():
    from veto_amd.layers import max_segment
    from veto_amd.rpn import rpn_proposals
    _, c, t = _case("small5")
    limit = max_segment()
    with pytest.raises(native.VetoError, match=str(limit)):
        rpn_proposals(t["objectness"], t["box_regression"], t["anchors"], c["images"], **dict(_settings(c), pre_nms_top_n=limit + 1))
    with pytest.raises(native.VetoError, match="pre_nms_top_n"):
        rpn_proposals(t["objectness"], t["box_regression"], t["anchors"], c["images"], **dict(_settings(c), pre_nms_top_n=12000))
    torch.cuda.synchronize()   # nothing was launched: nothing can have failed
    with pytest.raises(RuntimeError, match="HIP device only"):
        rpn_proposals([o.cpu() for o in t["objectness"]], [r.cpu() for r in t["box_regression"]], [a.cpu() for a in t["anchors"]],
                      c["images"], **_settings(c))
