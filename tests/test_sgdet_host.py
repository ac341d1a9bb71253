"""sgdet (detected boxes), host side: a numpy restatement of the reference's object decoding and test-pair
preparation, checked against the fixtures the reference produced (tests/golden/sgdet/, written by
tests/golden/make_golden_sgdet.py), the C-ABI argument checks, and the config plumbing.  No GPU needed.

Restated from the cited semantics:
  decode, mode "post": obj_prediction_nms (relation_head/utils_relation.py:94-128) -- prob = softmax, prob[:, 0] = 0;
      N times: first row-major arg-max (b, c); label[b] = c unless already > 0; prob[j, c] = 0 for every j with
      nms_overlaps(...)[b, j, c] >= thr; prob[b, :] = -1.
  decode, mode "meet": Ensemble.nms_per_cls (roi_relation_predictors.py:3855-3874) -- the same with prob[:, 0] = -1 and
      label[b] = c unconditionally, on softmax(one_hot(pred_labels)).
  pairs: RelationSampling.prepare_test_pairs (sampling.py:31-52) -- ones - eye, AND boxlist_iou > 0 when the overlap
      filter is on, row-major; above the cap the best by pred_scores[s] * pred_scores[o], in the stable descending order."""
import ctypes
import os

import numpy as np
import pytest
import torch

from veto_amd import native, synth, testing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgdet")


# ---- the restatement --------------------------------------------------------------------------------

def np_softmax(logits):
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def np_nms_iou(bb, bj):
    """nms_overlaps for box b against boxes j of one class, fp32, in the reference's operation order."""
    f = np.float32
    iw = np.maximum((np.minimum(bb[2], bj[:, 2]) - np.maximum(bb[0], bj[:, 0])) + f(1), f(0))
    ih = np.maximum((np.minimum(bb[3], bj[:, 3]) - np.maximum(bb[1], bj[:, 1])) + f(1), f(0))
    inter = iw * ih
    area_b = ((bb[2] - bb[0]) + f(1)) * ((bb[3] - bb[1]) + f(1))
    area_j = ((bj[:, 2] - bj[:, 0]) + f(1)) * ((bj[:, 3] - bj[:, 1]) + f(1))
    return inter / ((-inter + area_j) + area_b)


def np_decode(prob, boxes_per_cls, thr, mode="post", consulted=None):
    """Greedy class-aware NMS on a probability matrix (softmax already applied).  consulted: optional list that
    receives every IoU the loop compares with the threshold."""
    p = np.array(prob, np.float32, copy=True)
    bpc = np.asarray(boxes_per_cls, np.float32)
    n = p.shape[0]
    p[:, 0] = 0.0 if mode == "post" else -1.0
    label = np.zeros(n, np.int64)
    thr32 = np.float32(thr)
    for _ in range(n):
        b, c = np.unravel_index(int(p.argmax()), p.shape)
        if mode == "meet" or label[b] == 0:
            label[b] = c
        iou = np_nms_iou(bpc[b, c], bpc[:, c])
        if consulted is not None:
            consulted.extend(iou.tolist())
        p[iou >= thr32, c] = 0.0
        p[b] = -1.0
    return label


def np_onehot_prob(labels, n_cls):
    """softmax(one_hot(labels)) with every row built from the same two values: the MEET decoder's ties between rows are
    exact, broken by the first row-major index.  (The reference's softmax sums each row in an order that depends on
    where its 1 sits, which can move a row's cold values by an ulp; the fixtures hold only images where that does not
    change a label.)"""
    e = np.float32(np.e)
    hot, cold = e / (e + np.float32(n_cls - 1)), np.float32(1) / (e + np.float32(n_cls - 1))
    p = np.full((len(labels), n_cls), cold, np.float32)
    p[np.arange(len(labels)), labels] = hot
    return p


def np_decode_scores(logits, labels):
    prob = np_softmax(logits)
    prob[:, 0] = 0.0
    return prob[np.arange(len(labels)), labels]


def np_overlap(boxes):
    """boxlist_iou(p, p) > 0, fp32, TO_REMOVE = 1."""
    b = np.asarray(boxes, np.float32)
    f = np.float32
    lt = np.maximum(b[:, None, :2], b[None, :, :2])
    rb = np.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = np.maximum((rb - lt) + f(1), f(0))
    inter = wh[..., 0] * wh[..., 1]
    area = ((b[:, 2] - b[:, 0]) + f(1)) * ((b[:, 3] - b[:, 1]) + f(1))
    return inter / ((area[:, None] + area[None, :]) - inter) > 0


def np_pairs(boxes, scores, cap, require_overlap):
    """Pairs of one image in the kernel's (and torch.sort(stable=True, descending=True)'s) order."""
    n = len(boxes)
    cand = ~np.eye(n, dtype=bool)
    if require_overlap and n:
        cand &= np_overlap(boxes)
    idx = np.argwhere(cand).astype(np.int64).reshape(-1, 2)
    if len(idx) > cap:
        s = np.asarray(scores, np.float32)
        q = s[idx[:, 0]] * s[idx[:, 1]]
        idx = idx[np.argsort(-q, kind="stable")[:cap]]
    if len(idx) == 0:
        idx = np.zeros((1, 2), np.int64)
    return idx


def pair_qualities(pairs, scores):
    s = np.asarray(scores, np.float32)
    return s[pairs[:, 0]] * s[pairs[:, 1]]


# ---- fixtures -----------------------------------------------------------------------------------------

def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def case_names(g):
    return sorted({k.split("__")[0] for k in g})


def case_images(g, case):
    """The case's images regenerated from their synth seeds (seed -1: the hand-built IoU-tie image)."""
    C = int(g[case + "__n_cls"])
    out = []
    for seed, n in zip(g[case + "__seeds"], g[case + "__n_objs"]):
        if seed < 0:
            out.append(synth.synthetic_detections_iou_tie(C))
        else:
            out.append(synth.synthetic_detections(int(seed), int(n), C, spread=float(g[case + "__spread"])))
    return out


def test_decode_restatement_reproduces_the_reference():
    g = load_golden("decode")
    assert len(case_names(g)) >= 10
    for case in case_names(g):
        thr = float(g[case + "__thr"])
        imgs = case_images(g, case)
        for mode in ("post", "meet"):
            got = []
            for d in imgs:
                if mode == "post":
                    prob = np_softmax(d["predict_logits"])
                else:
                    prob = np_onehot_prob(d["pred_labels"], d["predict_logits"].shape[1])
                got.append(np_decode(prob, d["boxes_per_cls"], thr, mode))
            np.testing.assert_array_equal(np.concatenate(got), g["%s__labels_%s" % (case, mode)], err_msg="%s %s" % (case, mode))
        scores = np.concatenate([np_decode_scores(d["predict_logits"], l) for d, l in
                                 zip(imgs, np.split(g[case + "__labels_post"], np.cumsum(g[case + "__n_objs"])[:-1]))])
        np.testing.assert_allclose(scores, g[case + "__scores_post"], rtol=1e-6, atol=0)


def test_the_iou_tie_case_suppresses_at_equality():
    d = synth.synthetic_detections_iou_tie()
    bpc = d["boxes_per_cls"]
    assert np_nms_iou(bpc[0, 5], bpc[1:2, 5])[0] == np.float32(0.5)
    lab = np_decode(np_softmax(d["predict_logits"]), bpc, 0.5, "post")
    assert lab[0] == 5 and lab[1] != 5 and lab[2] != 5      # IoU == thr suppresses (>=)
    lab = np_decode(np_softmax(d["predict_logits"]), bpc, 0.500001, "post")
    assert list(lab) == [5, 5, 5]


def test_pair_restatement_reproduces_the_reference():
    g = load_golden("pairs")
    seen_cap = seen_placeholder = 0
    for case in case_names(g):
        cap = int(g[case + "__cap"])
        overlap = bool(g[case + "__overlap"])
        ref = np.split(g[case + "__pairs"], np.cumsum(g[case + "__counts"])[:-1])
        for d, r in zip(case_images(g, case), ref):
            mine = np_pairs(d["boxes"], d["pred_scores"], cap, overlap)
            assert mine.shape == r.shape, case
            if len(r) < cap or (len(d["boxes"]) * (len(d["boxes"]) - 1) <= cap and not overlap):
                np.testing.assert_array_equal(mine, r, err_msg=case)   # below the cap: row-major, exact
            else:
                seen_cap += 1
                q_ref, q_mine = pair_qualities(r, d["pred_scores"]), pair_qualities(mine, d["pred_scores"])
                np.testing.assert_array_equal(q_mine, q_ref)          # same qualities in the same (descending) order
                t = q_ref[-1]                                          # the cap-th score: ties at it may differ
                assert set(map(tuple, r[q_ref > t])) == set(map(tuple, mine[q_mine > t]))
            seen_placeholder += int(len(r) == 1 and not r.any())
    assert seen_cap and seen_placeholder


# ---- C ABI and config, no GPU ------------------------------------------------------------------------------

def test_sgdet_abi_rejects_bad_arguments_without_a_gpu():
    lib = native.load_library()
    a = native.VetoObjDecodeArgs()
    assert lib.veto_obj_decode(None, ctypes.byref(a), ctypes.c_void_p(8), 1 << 20) == -1
    assert b"size mismatch" in lib.veto_last_error()
    a.struct_size = ctypes.sizeof(native.VetoObjDecodeArgs)
    a.n_img, a.n_obj, a.n_cls, a.max_obj_per_image, a.mode, a.nms_thres = 1, 300, 151, 300, 0, 0.3
    a.logits = a.labels = a.boxes_per_cls = a.img_obj_offset = a.obj_pred = 8
    assert lib.veto_obj_decode(None, ctypes.byref(a), ctypes.c_void_p(8), 1 << 30) == -1
    assert b"max_obj_per_image 300" in lib.veto_last_error()
    a.max_obj_per_image = 80
    for field, value, needle in (("n_cls", 1, b"n_cls"), ("n_cls", 5000, b"n_cls"), ("mode", 2, b"mode"),
                                 ("obj_pred", None, b"missing pointer")):
        old = getattr(a, field)
        setattr(a, field, value)
        assert lib.veto_obj_decode(None, ctypes.byref(a), ctypes.c_void_p(8), 1 << 30) == -1, field
        assert needle in lib.veto_last_error(), (field, lib.veto_last_error())
        setattr(a, field, old)
    assert lib.veto_obj_decode(None, ctypes.byref(a), ctypes.c_void_p(8), 16) == -4   # workspace too small
    assert lib.veto_obj_decode_workspace_bytes(80, 151) >= 80 * 151 * 4

    p = native.VetoPairArgs()
    assert lib.veto_prepare_test_pairs(None, ctypes.byref(p)) == -1
    p.struct_size = ctypes.sizeof(native.VetoPairArgs)
    p.n_img, p.n_obj, p.max_obj_per_image, p.max_pairs = 1, 257, 257, 2048
    p.boxes = p.scores = p.img_obj_offset = p.img_out_offset = p.pairs = p.counts = 8
    assert lib.veto_prepare_test_pairs(None, ctypes.byref(p)) == -1
    assert b"max_obj_per_image 257" in lib.veto_last_error()
    p.max_obj_per_image, p.max_pairs = 80, 0
    assert lib.veto_prepare_test_pairs(None, ctypes.byref(p)) == -1
    assert b"max_pairs" in lib.veto_last_error()
    p.max_pairs, p.counts = 2048, None
    assert lib.veto_prepare_test_pairs(None, ctypes.byref(p)) == -1
    assert b"missing pointer" in lib.veto_last_error()


def test_struct_layouts_of_the_sgdet_entries():
    assert ctypes.sizeof(native.VetoObjDecodeArgs) == 8 * 4 + 7 * 8
    assert ctypes.sizeof(native.VetoPairArgs) == 6 * 4 + 6 * 8


def _sgdet_config(meet=False, thr=0.5, overlap=True):
    cfg = testing.make_config(2, 8, mode="sgcls", meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = thr
    cfg.TEST.RELATION.REQUIRE_OVERLAP = overlap
    return cfg


def test_relation_head_and_post_processor_accept_detected_boxes():
    from veto_amd import predictor
    from veto_amd.relation_head import VETORelationHead
    predictor.set_embedding_provider(lambda names, d, k: torch.zeros(len(names), k))
    head = VETORelationHead(_sgdet_config(thr=0.5, overlap=True))
    assert head.mode == "sgdet" and head.require_overlap and not head.use_gt_box
    assert head.post_processor.later_nms_pred_thres == 0.5 and not head.post_processor.use_gt_box
    cfg = _sgdet_config(thr=0.3, overlap=False)
    cfg.MODEL.ROI_RELATION_HEAD.REQUIRE_BOX_OVERLAP = True   # the training-time key does not drive the test pairs
    head = VETORelationHead(cfg)
    assert not head.require_overlap and head.post_processor.later_nms_pred_thres == 0.3
    head.train()
    with pytest.raises(NotImplementedError, match="detect_relsample"):
        head.forward([torch.zeros(1, 256, 8, 8)], [], depth_features=torch.zeros(1, 256, 4, 4), targets=[])
    cfg = _sgdet_config(meet=True, thr=0.4)
    m = predictor.VETOPredictor_MEET(cfg, 512)
    assert m.mode == "sgdet" and m.nms_thresh == pytest.approx(0.4)
    gt = testing.make_config(2, 8, mode="sgcls")     # GT boxes: no overlap filter whatever the config says
    gt.TEST.RELATION.REQUIRE_OVERLAP = True
    assert not VETORelationHead(gt).require_overlap


def test_sgg_evaluator_accepts_sgdet_and_the_abi_checks_its_mode():
    from veto_amd.evaluation import SGGEvaluator
    with pytest.raises(RuntimeError, match="HIP device"):      # past the mode check: only the device is missing here
        SGGEvaluator("sgdet", 51, np.zeros((0, 3), np.int64), device="cpu")
    with pytest.raises(NotImplementedError):
        SGGEvaluator("phrdet", 51, np.zeros((0, 3), np.int64), device="cpu")
    lib = native.load_library()
    a = native.VetoSggEvalArgs()
    assert ctypes.sizeof(native.VetoSggEvalArgs) == 6 * 4 + 21 * 8
    a.struct_size = ctypes.sizeof(native.VetoSggEvalArgs)
    a.n_img, a.n_rel_cls, a.iou_thres = 1, 51, 0.5
    for f in ("gt_offset", "obj_offset", "pair_offset", "gt_rels", "gt_classes", "gt_boxes", "pred_pairs", "rel_scores",
              "pred_classes", "pred_boxes", "obj_scores", "gc_rank", "ng_rank", "acc_rank", "zeroshot_flag", "ng_rows",
              "ng_cols", "ng_count", "metrics"):
        setattr(a, f, 8)
    a.reserved0 = 2
    assert lib.veto_sgg_eval(None, ctypes.byref(a), 1, 1, ctypes.c_void_p(8), 1 << 30) == -1
    assert b"mode" in lib.veto_last_error()
    a.reserved0 = 1
    assert lib.veto_sgg_eval(None, ctypes.byref(a), 1, 1, ctypes.c_void_p(8), 1 << 30) == -1
    assert b"pred_obj_offset" in lib.veto_last_error()
    a.struct_size = 8
    assert lib.veto_sgg_eval(None, ctypes.byref(a), 1, 1, ctypes.c_void_p(8), 1 << 30) == -1
    assert b"size mismatch" in lib.veto_last_error()
