"""sgdet box decoder on the MI355X: veto_nms and veto_box_postprocess against the reference's fixtures (tests/golden/boxhead/)
through the C-ABI wrappers and through PostProcessor, the hand-over to VETORelationHead, and workspace reuse.

Exact: keep / counts of veto_nms; orig_inds, pred_labels and the per-image counts of the decoder.  Toleranced (results of exp):
pred_scores, final boxes and boxes_per_cls, at 4x the error of the reference's own fp32 arithmetic against fp64, which the
generator measured and stored per fixture (ref_fp32_err_boxes ~1e-4 px, ref_fp32_err_scores ~2e-8).  Every figure is printed
before it is asserted (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_boxhead_host import (GOLDEN, decoder_fixtures, fixture_images, fixture_params, nms_fixture_inputs, np_box_postprocess,  # noqa: E402
                               np_nms)

from veto_amd import synth, testing  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- veto_nms -----------------------------------------------------------------------------------------------------------

def _nms_cases():
    z = np.load(os.path.join(GOLDEN, "nms.npz"))
    out = []
    for name in [str(s) for s in z["cases"]]:
        seed, n, thr = int(z[name + "__seed"]), int(z[name + "__n"]), float(z[name + "__thr"])
        boxes, scores = nms_fixture_inputs(seed, n)
        out.append((name, boxes[:n], scores[:n], thr, z[name + "__keep"]))
    return out


def test_nms_matches_every_fixture_one_segment_at_a_time():
    from veto_amd.layers import nms
    for name, boxes, scores, thr, want in _nms_cases():
        keep = nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), thr)
        assert keep.dtype == torch.int64 and keep.device.type == "cuda"
        np.testing.assert_array_equal(keep.cpu().numpy(), want, err_msg=name)


@pytest.mark.parametrize("thr", [0.7, 0.3, 0.5])
def test_nms_matches_every_fixture_as_segments_of_one_launch(thr):
    """All fixture segments of one threshold (the empty one included) in a single veto_nms launch, without and with a cap."""
    from veto_amd.layers import batched_nms
    cases = [c for c in _nms_cases() if c[3] == thr]
    assert cases
    sizes = [len(c[1]) for c in cases]
    off = np.concatenate([[0], np.cumsum(sizes)])
    boxes = torch.from_numpy(np.concatenate([c[1] for c in cases])).to(DEV)
    scores = torch.from_numpy(np.concatenate([c[2] for c in cases])).to(DEV)
    for cap in (-1, 5):
        keep, counts = batched_nms(boxes, scores, off.tolist(), thr, max_keep=cap)
        keep, counts = keep.cpu().numpy(), counts.cpu().numpy()
        for s, c in enumerate(cases):
            want = c[4] if cap < 0 else c[4][:cap]   # boxlist_ops.py:29-30: the first max_keep of the ascending list
            assert counts[s] == len(want), (c[0], cap)
            np.testing.assert_array_equal(keep[off[s]:off[s] + counts[s]], want, err_msg="%s cap %d" % (c[0], cap))


def test_nms_rejects_a_segment_above_the_limit_before_launching():
    from veto_amd import native
    from veto_amd.layers import batched_nms, max_segment
    n = max_segment() + 1
    with pytest.raises(native.VetoError, match="seg_offset_host"):
        batched_nms(torch.zeros((n, 4), device=DEV), torch.zeros(n, device=DEV), (0, n), 0.5)


# ---- veto_box_postprocess -------------------------------------------------------------------------------------------------

def _run_abi(imgs, prm):
    from veto_amd.boxhead import box_postprocess
    cat = lambda k: torch.from_numpy(np.concatenate([d[k] for d in imgs])).to(DEV)   # noqa: E731
    return box_postprocess(cat("class_logits"), cat("box_regression"), cat("proposals"), [len(d["proposals"]) for d in imgs],
                           [d["image_size"] for d in imgs], score_thresh=prm["score_thresh"], nms=prm["nms"],
                           post_nms_per_cls_topn=prm["topn"], nms_filter_duplicates=prm["filter_dup"],
                           detections_per_img=prm["det_per_img"], reg_weights=prm["weights"], cls_agnostic_bbox_reg=prm["cls_agnostic"])


def _run_module(imgs, prm):
    from veto_amd.boxhead import BoxCoder, PostProcessor
    post = PostProcessor(prm["score_thresh"], prm["nms"], prm["topn"], prm["filter_dup"], prm["det_per_img"],
                         BoxCoder(prm["weights"]), prm["cls_agnostic"]).eval()
    props = []
    for d in imgs:
        b = BoxList(torch.from_numpy(d["proposals"]).to(DEV), d["image_size"], "xyxy")
        b.add_field("predict_logits", torch.from_numpy(d["class_logits"]).to(DEV))
        props.append(b)
    total = sum(len(d["proposals"]) for d in imgs)
    feats = torch.arange(total, dtype=torch.float32, device=DEV).reshape(total, 1)
    cat = lambda k: torch.from_numpy(np.concatenate([d[k] for d in imgs])).to(DEV)   # noqa: E731
    nms_feats, results = post((feats, cat("class_logits"), cat("box_regression")), props)
    outs, row, base = [], 0, 0
    for r, d in zip(results, imgs):
        k = len(r)
        assert r.mode == "xyxy" and r.size == d["image_size"]
        inds = (nms_feats[row:row + k, 0] - base).long()   # nms_features = features[orig_inds]: recovers orig_inds
        assert torch.equal(r.get_field("predict_logits"), props[len(outs)].get_field("predict_logits")[inds])
        outs.append(dict(orig_inds=inds, pred_labels=r.get_field("pred_labels"), pred_scores=r.get_field("pred_scores"),
                         boxes=r.bbox, boxes_per_cls=r.get_field("boxes_per_cls")))
        row += k
        base += len(d["proposals"])
    assert row == nms_feats.shape[0]
    return outs


def _compare(name, outs, z, imgs, prm):
    tol_b, tol_s = 4 * float(z["ref_fp32_err_boxes"]), 4 * float(z["ref_fp32_err_scores"])
    row, err_b, err_s = 0, 0.0, 0.0
    for i, (o, d) in enumerate(zip(outs, imgs)):
        k = int(z["counts"][i])
        sl = slice(row, row + k)
        got = {key: v.cpu().numpy() for key, v in o.items()}
        assert got["orig_inds"].dtype == np.int64 and got["pred_labels"].dtype == np.int64
        assert len(got["orig_inds"]) == k, (name, i, len(got["orig_inds"]), k)
        np.testing.assert_array_equal(got["orig_inds"], z["orig_inds"][sl], err_msg="%s image %d" % (name, i))
        np.testing.assert_array_equal(got["pred_labels"], z["pred_labels"][sl], err_msg="%s image %d" % (name, i))
        second = np_box_postprocess(d, prm)   # the second yardstick agrees on the exact quantities too
        np.testing.assert_array_equal(got["orig_inds"], second["orig_inds"])
        np.testing.assert_array_equal(got["pred_labels"], second["pred_labels"])
        assert got["boxes_per_cls"].shape == (k, int(z["n_cls"]), 4)
        err_s = max(err_s, np.abs(got["pred_scores"] - z["pred_scores"][sl]).max(initial=0))
        err_b = max(err_b, np.abs(got["boxes"] - z["boxes"][sl]).max(initial=0),
                    np.abs(got["boxes_per_cls"] - z["boxes_per_cls"][sl]).max(initial=0))
        if "dec_full" in z.files:   # every proposal of this fixture survives: boxes_per_cls IS the full decode
            assert k == len(d["proposals"]) and np.array_equal(got["orig_inds"], np.arange(k))
            err_b = max(err_b, np.abs(got["boxes_per_cls"] - z["dec_full"]).max())
        row += k
    assert row == len(z["orig_inds"])
    print("%s: device error boxes %.3e (allowed %.3e), scores %.3e (allowed %.3e)" % (name, err_b, tol_b, err_s, tol_s))
    assert err_b <= tol_b, (name, err_b, tol_b)
    assert err_s <= tol_s, (name, err_s, tol_s)


@pytest.mark.parametrize("via", ["abi", "module"])
@pytest.mark.parametrize("path", decoder_fixtures(), ids=lambda p: os.path.basename(p)[:-4])
def test_decoder_matches_every_fixture(path, via):
    z = np.load(path)
    prm, imgs = fixture_params(z), fixture_images(z)
    outs = (_run_abi if via == "abi" else _run_module)(imgs, prm)
    _compare(os.path.basename(path)[:-4] + "/" + via, outs, z, imgs, prm)


def test_training_relation_mode_carries_the_labels():
    from veto_amd.boxhead import PostProcessor
    d = synth.synthetic_box_head_outputs(1700, 30)
    b = BoxList(torch.from_numpy(d["proposals"]).to(DEV), d["image_size"], "xyxy")
    b.add_field("predict_logits", torch.from_numpy(d["class_logits"]).to(DEV))
    gt = torch.arange(30, device=DEV) + 100
    b.add_field("labels", gt)
    post = PostProcessor(0.01, 0.3, 300, True, 80).train()
    feats = torch.zeros((30, 2), device=DEV)
    _, res = post((feats, b.get_field("predict_logits"), torch.from_numpy(d["box_regression"]).to(DEV)), [b], relation_mode=True)
    want = np_box_postprocess(d, dict(score_thresh=0.01, nms=0.3, topn=300, filter_dup=True, det_per_img=80,
                                      weights=(10., 10., 5., 5.), cls_agnostic=False))
    np.testing.assert_array_equal(res[0].get_field("labels").cpu().numpy(), want["orig_inds"] + 100)
    _, res = post.eval()((feats, b.get_field("predict_logits"), torch.from_numpy(d["box_regression"]).to(DEV)), [b], relation_mode=True)
    assert not res[0].has_field("labels")


def test_post_processor_output_feeds_the_relation_head_unchanged():
    """The detections of the vg1000 fixture's image (80 after the cut: inside veto_obj_decode's 256 rows) and of below_cap's go
    straight into VETORelationHead.forward_pooled in sgdet mode."""
    from veto_amd import predictor
    from veto_amd.boxhead import PostProcessor
    from veto_amd.relation_head import VETORelationHead
    imgs = [synth.synthetic_box_head_outputs(s, n) for s, n in ((1102, 1000), (1700, 30))]
    post = PostProcessor(0.01, 0.3, 300, True, 80).eval()
    props = []
    for d in imgs:
        b = BoxList(torch.from_numpy(d["proposals"]).to(DEV), d["image_size"], "xyxy")
        b.add_field("predict_logits", torch.from_numpy(d["class_logits"]).to(DEV))
        props.append(b)
    total = sum(len(b) for b in props)
    cat = lambda k: torch.from_numpy(np.concatenate([d[k] for d in imgs])).to(DEV)   # noqa: E731
    feats = torch.from_numpy(synth.normal(3, "boxhead.roi", (total, 8), 0.0, 1.0)).to(DEV)
    nms_feats, dets = post((feats, cat("class_logits"), cat("box_regression")), props)
    assert [len(r) for r in dets] == [80, 30] and nms_feats.shape == (110, 8)
    for r in dets:
        n = len(r)
        assert r.bbox.dtype == torch.float32 and r.bbox.shape == (n, 4)
        assert r.get_field("pred_labels").dtype == torch.int64 and r.get_field("pred_scores").dtype == torch.float32
        assert r.get_field("boxes_per_cls").shape == (n, 151, 4) and r.get_field("predict_logits").shape == (n, 151)
        assert all(r.get_field(k).device.type == "cuda" for k in ("pred_labels", "pred_scores", "boxes_per_cls", "predict_logits"))
        assert int(r.get_field("pred_labels").min()) >= 1
    cfg = testing.make_config(2, 8, mode="sgcls")
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = 0.5
    cfg.TEST.RELATION.REQUIRE_OVERLAP = True
    predictor.set_embedding_provider(lambda names, w, k: torch.zeros(len(names), k))
    predictor.set_statistics_provider(lambda c: {"obj_classes": ["o%d" % i for i in range(151)],
                                                 "rel_classes": ["r%d" % i for i in range(51)]})
    head = VETORelationHead(cfg).to(DEV).eval()
    sd = synth.predictor_state_dict(0, layers=2)
    head.predictor.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    head.predictor.eval()
    roi = torch.from_numpy(synth.normal(3, "sgdet.roi", (110, 256, 8, 8), 0.0, 1.0)).to(DEV)
    depth = torch.from_numpy(synth.normal(4, "sgdet.depth", (110, 256, 8, 8), 0.0, 1.0)).to(DEV)
    with torch.no_grad():
        _, result, _ = head.forward_pooled(dets, roi, depth)
    torch.cuda.synchronize()
    for r, det in zip(result, dets):
        assert len(r) == len(det)
        assert torch.isfinite(r.get_field("pred_rel_scores")).all()
        assert r.get_field("rel_pair_idxs").shape[1] == 2


_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_boxhead_gpu import _run_abi
from test_boxhead_host import fixture_images, fixture_params
z = np.load(%r)
o = _run_abi(fixture_images(z), fixture_params(z))
np.savez(%r, **{k: np.concatenate([x[k].cpu().numpy() for x in o]) for k in o[0]})
"""


def test_second_call_with_other_shapes_matches_a_fresh_process(tmp_path):
    """Workspace reuse: vg1000 (a large workspace) first, then ragged12 on the same stream; ragged12's results must be
    bit-identical to those of a process that ran nothing before."""
    here = os.path.dirname(os.path.abspath(__file__))
    small, big = os.path.join(GOLDEN, "ragged12.npz"), os.path.join(GOLDEN, "vg1000.npz")
    out = str(tmp_path / "fresh.npz")
    subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here, small, out)], check=True, timeout=600)
    fresh = np.load(out)
    zb, zs = np.load(big), np.load(small)
    _run_abi(fixture_images(zb), fixture_params(zb))
    again = _run_abi(fixture_images(zs), fixture_params(zs))
    for k in fresh.files:
        np.testing.assert_array_equal(np.concatenate([x[k].cpu().numpy() for x in again]), fresh[k], err_msg=k)
