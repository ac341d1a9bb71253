"""sgdet (detected boxes) on the MI355X: veto_obj_decode and veto_prepare_test_pairs against the reference's fixtures
(tests/golden/sgdet/) and the numpy restatement of tests/test_sgdet_host.py, the PostProcessor's three branches and
VETORelationHead end to end on detected boxes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sgdet_host import (case_images, case_names, load_golden, np_decode, np_decode_scores, np_onehot_prob,  # noqa: E402
                             np_pairs, np_softmax, pair_qualities)

from veto_amd import synth, testing  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _decode(imgs, thr, mode):
    from veto_amd.sgdet import decode_objects
    n_objs = [len(d["boxes"]) for d in imgs]
    bpc = torch.from_numpy(np.concatenate([d["boxes_per_cls"] for d in imgs])).to(DEV)
    if mode == "post":
        x = torch.from_numpy(np.concatenate([d["predict_logits"] for d in imgs])).to(DEV)
        lab, sc, bx = decode_objects(x, bpc, n_objs, thr, mode="post")
        return lab.cpu().numpy(), sc.cpu().numpy(), bx.cpu().numpy()
    x = torch.from_numpy(np.concatenate([d["pred_labels"] for d in imgs])).to(DEV)
    lab, _, _ = decode_objects(x, bpc, n_objs, thr, mode="meet", want_scores=False, want_boxes=False)
    return lab.cpu().numpy(), None, None


def _regressed(imgs, labels):
    bpc = np.concatenate([d["boxes_per_cls"] for d in imgs])
    return bpc[np.arange(len(labels)), labels]


def test_decode_matches_the_reference_fixtures():
    g = load_golden("decode")
    for case in case_names(g):
        thr = float(g[case + "__thr"])
        imgs = case_images(g, case)
        lab, sc, bx = _decode(imgs, thr, "post")
        np.testing.assert_array_equal(lab, g[case + "__labels_post"], err_msg=case)
        np.testing.assert_allclose(sc, g[case + "__scores_post"], rtol=1e-6, atol=0, err_msg=case)
        np.testing.assert_array_equal(bx, _regressed(imgs, lab))
        lab, _, _ = _decode(imgs, thr, "meet")
        np.testing.assert_array_equal(lab, g[case + "__labels_meet"], err_msg=case + " meet")


def _robust_detections(seed, n, n_cls, thr):
    """synthetic_detections for the first seed (seed, seed + 50, ...) whose post-processor decode does not hinge on the last
    ulp of the softmax -- the fp32 and fp64 restatements agree on every label -- as the fixture generator requires."""
    for s in range(seed, seed + 50 * 40, 50):
        d = synth.synthetic_detections(s, n, n_cls)
        want = np_decode(np_softmax(d["predict_logits"]), d["boxes_per_cls"], thr, "post")
        want64 = np_decode(np_softmax(d["predict_logits"].astype(np.float64)), d["boxes_per_cls"].astype(np.float64), thr, "post")
        if np.array_equal(want, want64):
            return d, want
    raise AssertionError("no seed without a softmax-ulp decision near %d" % seed)


@pytest.mark.parametrize("seed", range(50))
def test_decode_matches_the_restatement_at_256_by_201(seed):
    """N = 256, C = 201: the probability matrix does not fit in LDS and lives in the workspace.  Every label compared."""
    thr = 0.3 if seed % 2 else 0.5
    d, want = _robust_detections(1000 + seed, 256, 201, thr)
    lab, sc, bx = _decode([d], thr, "post")
    np.testing.assert_array_equal(lab, want)
    np.testing.assert_allclose(sc, np_decode_scores(d["predict_logits"], lab), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(bx, _regressed([d], lab))
    lab, _, _ = _decode([d], thr, "meet")
    np.testing.assert_array_equal(lab, np_decode(np_onehot_prob(d["pred_labels"], 201), d["boxes_per_cls"], thr, "meet"))


def _props(imgs, with_logits=True):
    props = []
    for d in imgs:
        b = BoxList(torch.from_numpy(d["boxes"]).to(DEV), d["image_size"], "xyxy")
        b.add_field("pred_scores", torch.from_numpy(d["pred_scores"]).to(DEV))
        b.add_field("pred_labels", torch.from_numpy(d["pred_labels"]).to(DEV))
        b.add_field("boxes_per_cls", torch.from_numpy(d["boxes_per_cls"]).to(DEV))
        if with_logits:
            b.add_field("predict_logits", torch.from_numpy(d["predict_logits"]).to(DEV))
        props.append(b)
    return props


def test_pairs_match_the_reference_fixtures():
    from veto_amd.pairs import prepare_test_pairs
    g = load_golden("pairs")
    capped = 0
    for case in case_names(g):
        cap, overlap = int(g[case + "__cap"]), bool(g[case + "__overlap"])
        imgs = case_images(g, case)
        got = prepare_test_pairs(DEV, _props(imgs), cap, require_overlap=overlap, use_gt_box=False)
        ref = np.split(g[case + "__pairs"], np.cumsum(g[case + "__counts"])[:-1])
        for d, r, p in zip(imgs, ref, got):
            p = p.cpu().numpy()
            np.testing.assert_array_equal(p, np_pairs(d["boxes"], d["pred_scores"], cap, overlap), err_msg=case)
            assert p.shape == r.shape
            q_ref, q = pair_qualities(r, d["pred_scores"]), pair_qualities(p, d["pred_scores"])
            if len(r) < cap:
                np.testing.assert_array_equal(p, r, err_msg=case)
            else:
                capped += 1
                np.testing.assert_array_equal(q, q_ref)
                t = q_ref[-1]
                assert set(map(tuple, r[q_ref > t])) == set(map(tuple, p[q > t])), case
    assert capped


@pytest.mark.parametrize("seed", range(6))
def test_pairs_match_the_restatement_at_256(seed):
    from veto_amd.pairs import prepare_test_pairs
    imgs = [synth.synthetic_detections(2000 + seed, n, 151) for n in (256, 200, 46, 3)]
    if seed % 3 == 0:   # heavy ties: every quality equal
        for d in imgs:
            d["pred_scores"] = np.full_like(d["pred_scores"], 0.5)
    for overlap in (False, True):
        got = prepare_test_pairs(DEV, _props(imgs), 2048, require_overlap=overlap, use_gt_box=False)
        for d, p in zip(imgs, got):
            np.testing.assert_array_equal(p.cpu().numpy(), np_pairs(d["boxes"], d["pred_scores"], 2048, overlap))


def _post_cfg(thr, meet=False, expert=False):
    cfg = testing.make_config(2, 8, mode="sgcls", meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = thr
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = expert
    return cfg


def _check_objects(res, d, thr):
    lab = np_decode(np_softmax(d["predict_logits"]), d["boxes_per_cls"], thr, "post")
    np.testing.assert_array_equal(res.get_field("pred_labels").cpu().numpy(), lab)
    np.testing.assert_allclose(res.get_field("pred_scores").cpu().numpy(), np_decode_scores(d["predict_logits"], lab),
                               rtol=1e-5, atol=0)
    np.testing.assert_array_equal(res.bbox.cpu().numpy(), d["boxes_per_cls"][np.arange(len(lab)), lab])
    assert res.size == d["image_size"] and res.mode == "xyxy"
    return lab


def test_post_processor_vanilla_branch_on_detected_boxes():
    from veto_amd.postprocess import make_roi_relation_post_processor
    g = load_golden("decode")
    imgs = case_images(g, "ragged12")
    thr = float(g["ragged12__thr"])
    props = _props(imgs)
    pairs = [torch.from_numpy(np_pairs(d["boxes"], d["pred_scores"], 2048, False)).to(DEV) for d in imgs]
    rel = [torch.from_numpy(synth.normal(5, "sgdet.rel.%d" % i, (len(p), 51), 0.0, 2.0)).to(DEV) for i, p in enumerate(pairs)]
    pp = make_roi_relation_post_processor(_post_cfg(thr))
    res = pp((rel, [p.get_field("predict_logits") for p in props]), pairs, props)
    off = 0
    for r, pr, d, p, x, t in zip(res, props, imgs, pairs, rel, pp.last_triple_scores):
        assert r is not pr      # sgdet returns new BoxLists (inference.py:424-428)
        lab = _check_objects(r, d, thr)
        np.testing.assert_array_equal(lab, g["ragged12__labels_post"][off:off + len(lab)])
        off += len(lab)
        sc = np_decode_scores(d["predict_logits"], lab)
        prob = np_softmax(x.cpu().numpy())
        pn = p.cpu().numpy()
        triple = prob[:, 1:].max(1) * sc[pn[:, 0]] * sc[pn[:, 1]]
        out_pairs = r.get_field("rel_pair_idxs").cpu().numpy()
        row = {tuple(q): i for i, q in enumerate(pn)}
        src = np.array([row[tuple(q)] for q in out_pairs])
        assert sorted(src.tolist()) == list(range(len(pn)))                       # a permutation of the input pairs
        t = t.cpu().numpy()
        assert np.all(t[:-1] >= t[1:])                                           # in descending triple score
        np.testing.assert_allclose(t, triple[src], rtol=1e-5, atol=0)
        np.testing.assert_allclose(r.get_field("pred_rel_scores").cpu().numpy(), prob[src], rtol=1e-5, atol=1e-7)
        np.testing.assert_array_equal(r.get_field("pred_rel_labels").cpu().numpy(), prob[src][:, 1:].argmax(1) + 1)


@pytest.mark.parametrize("expert", [False, True])
def test_post_processor_meet_and_voting_branches_on_detected_boxes(expert):
    from veto_amd import meet_tables
    from veto_amd.postprocess import make_roi_relation_post_processor
    d = synth.synthetic_detections(77, 10, 151)
    thr = 0.5
    props = _props([d])
    pairs = torch.from_numpy(np_pairs(d["boxes"], d["pred_scores"], 2048, False)).to(DEV)
    sizes = meet_tables.group_sizes("VG", "divide4")
    incre = meet_tables.incre_idx_list(sizes)
    rel = {}
    for k, gk in enumerate(sizes):
        for e in range(3 if expert else 1):
            key = "group_%d%d" % (k, e + 1) if expert else "group_%d" % k
            rel[key] = torch.from_numpy(synth.normal(9, "sgdet." + key, (len(pairs), gk + 2), 0.0, 2.0)).to(DEV)
    pp = make_roi_relation_post_processor(_post_cfg(thr, meet=True, expert=expert))
    res = pp((rel, [props[0].get_field("predict_logits")]), [pairs], props, incre_idx_list=incre)
    assert len(res) == 1 and res[0] is not props[0]
    _check_objects(res[0], d, thr)
    t = pp.last_triple_scores[0]
    assert torch.all(t[:-1] >= t[1:]) and torch.isfinite(t).all()


@pytest.mark.parametrize("meet", [False, True])
def test_relation_head_end_to_end_from_pooled_features(meet):
    from veto_amd import predictor
    from veto_amd.relation_head import VETORelationHead
    imgs = [synth.synthetic_detections(300 + i, n, 151) for i, n in enumerate((12, 9))]
    cfg = _post_cfg(0.5, meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.ENC_LAYERS = 2
    cfg.TEST.RELATION.REQUIRE_OVERLAP = True
    predictor.set_embedding_provider(lambda names, w, k: torch.zeros(len(names), k))
    n_obj, n_rel = 151, 51
    predictor.set_statistics_provider(lambda c: {"obj_classes": ["o%d" % i for i in range(n_obj)],
                                                 "rel_classes": ["r%d" % i for i in range(n_rel)]})
    head = VETORelationHead(cfg).to(DEV).eval()
    sd = synth.meet_state_dict(0, head.predictor.max_group_element_number_list, layers=2) if meet \
        else synth.predictor_state_dict(0, layers=2)
    head.predictor.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    head.predictor.eval()
    total = sum(len(d["boxes"]) for d in imgs)
    feats = torch.from_numpy(synth.normal(3, "sgdet.roi", (total, 256, 8, 8), 0.0, 1.0)).to(DEV)
    depth = torch.from_numpy(synth.normal(4, "sgdet.depth", (total, 256, 8, 8), 0.0, 1.0)).to(DEV)
    props = _props(imgs[:1] if meet else imgs)   # the MEET post-processor takes one image per batch
    nf = sum(len(p) for p in props)
    with torch.no_grad():
        _, result, _ = head.forward_pooled(props, feats[:nf], depth[:nf])
    torch.cuda.synchronize()
    for r, d in zip(result, imgs):
        _check_objects(r, d, 0.5)
        pairs = r.get_field("rel_pair_idxs").long().cpu().numpy()
        want = np_pairs(d["boxes"], d["pred_scores"], 2048, True)
        assert set(map(tuple, pairs)) == set(map(tuple, want))
        assert torch.isfinite(r.get_field("pred_rel_scores")).all()


# ---- evaluator in sgdet ------------------------------------------------------------------------------------------------

def _sgdet_eval_golden():
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgdet", "sggeval_sgdet.npz")))
    images, zeroshot = synth.synthetic_eval_images_sgdet(int(g["seed"]), [int(x) for x in g["num_objs"]],
                                                         num_rel_cls=int(g["num_rel"]))
    return g, images, zeroshot


def _check_sgdet_eval(res, g):
    KS = (20, 50, 100)
    for k in KS:
        for key in ("recall", "recall_nogc", "zeroshot_recall"):
            ref = g["%s_%d" % (key, k)]
            if key + "_list" in res:
                np.testing.assert_allclose(res[key + "_list"][k], ref, rtol=0, atol=1e-12, err_msg="%s %d" % (key, k))
            assert abs(res[key][k] - float(np.mean(ref))) < 1e-12, (key, k)
        for key in ("mean_recall", "ng_mean_recall"):
            assert abs(res[key][k] - float(g["%s_%d" % (key, k)])) < 1e-12, (key, k)
            np.testing.assert_allclose(res[key + "_list"][k], g["%s_list_%d" % (key, k)], rtol=0, atol=1e-12)
        assert len(g["accuracy_hit_%d" % k]) == 0 and np.isnan(res["accuracy"][k])   # the reference's A@K: mean of []


def test_evaluator_sgdet_matches_the_reference_evaluators():
    from veto_amd.evaluation import SGGEvaluator
    g, images, zeroshot = _sgdet_eval_golden()
    assert any(len(im["pred_classes"]) != len(im["gt_classes"]) for im in images)
    ev = SGGEvaluator("sgdet", int(g["num_rel"]), zeroshot, iou_thres=0.5, device=DEV)
    res = ev.evaluate(images)
    _check_sgdet_eval(res, g)
    assert 0.0 < res["recall"][100] < 1.0 and len(res["zeroshot_recall_list"][100]) >= 1
    assert all(r is None or np.all(r["acc_rank"] >= 0x3fffffff) for r in res["per_image"])
    for i in range(0, len(images), 3):                     # accumulated over batches like the reference over the split
        ev.update(images[i:i + 3])
    _check_sgdet_eval(ev.finalize(), g)
    assert "A @ 20: nan" in ev.generate_print_string(res)
    assert "A @ 20: nan" in str(g["print_accuracy"])


# ---- predictor logits in sgdet -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pred_vanilla_n12_l4h8", "pred_vanilla_n10_l6h6", "pred_meet_n12_l4h8", "pred_meet_n10_l6h6"])
def test_predictor_sgdet_logits_match_the_reference(name):
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgdet", name + ".npz")))
    seed, n, thr, layers, heads, meet = (int(g["seed"]), int(g["n"]), float(g["thr"]), int(g["layers"]), int(g["heads"]),
                                         bool(g["meet"]))
    d = synth.synthetic_detections(seed, n, 151)
    b = synth.synthetic_batch(seed, 1, [n], num_obj_cls=151)
    cfg = testing.make_config(layers, heads, mode="sgcls", meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = thr
    sd = synth.meet_state_dict(0, __import__("veto_amd").meet_tables.group_sizes("VG", "divide4"), layers=layers) if meet \
        else synth.predictor_state_dict(0, layers=layers)
    model = testing.make_predictor(cfg, sd, DEV)
    assert model.mode == "sgdet"
    props = _props([d])
    pairs = [torch.from_numpy(g["pair_idx"]).to(DEV)]
    with torch.no_grad():
        out = model(props, pairs, None, None, roi_features=torch.from_numpy(b["roi_features"]).to(DEV),
                    roi_depth_features=torch.from_numpy(b["roi_depth_features"]).to(DEV))
    if meet:
        # the decoder's NMS labels differ from the clamped pred_labels on this image: the logits pin the decode
        assert not np.array_equal(g["decoder_labels"], np.where(d["pred_labels"] > 0, d["pred_labels"], 1))
        keys = sorted(k[4:] for k in g if k.startswith("rel_group_"))
        assert keys and sorted(out[1]) == keys
        for k in keys:
            err = float(np.abs(out[1][k].cpu().numpy() - g["rel_" + k]).max())
            assert err <= 1e-3, (k, err)
    else:
        err = float(np.abs(torch.cat(list(out[1]), 0).cpu().numpy() - g["rel_dists"]).max())
        assert err <= 1e-3, err
