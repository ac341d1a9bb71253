"""Writes tests/golden/sgdet/{decode,pairs}.npz: what the reference computes on detected boxes.

Runs the reference itself (pysgg, imported with make_golden's stubs) on inputs regenerated from
veto_amd.synth seeds, and stores outputs only (plus the seeds that regenerate the inputs):
  decode.npz  obj_prediction_nms (utils_relation.py:94-128) labels and the PostProcessor's scores
              (inference.py:410-420), Ensemble.nms_per_cls (roi_relation_predictors.py:3855-3874) labels
  pairs.npz   RelationSampling.prepare_test_pairs (sampling.py:31-52), use_gt_box False, with and without
              test_overlap, MAX_PROPOSAL_PAIR 2048
  pred_*.npz  VETOPredictor / VETOPredictor_MEET (roi_relation_predictors.py:4074-4139, :3752-3853, :3905-) in sgdet
              eval mode: relation logits for detected proposals, the MEET decoder's nms_per_cls labels included
  sggeval_sgdet.npz  the reference's evaluators through evaluate_relation_of_one_image (vg_eval.py:459-566) in
              mode 'sgdet' on veto_amd.synth.synthetic_eval_images_sgdet (#pred boxes != #GT boxes)
A seed is rejected (the next one is tried) when the reference's labels change under an fp64 recomputation or a
consulted same-class IoU lies within 1e-6 of the threshold, or when a MEET-decoder tie between rows is decided by the
last ulp of the reference's softmax (its row sums depend on where the one-hot's 1 sits) rather than by the row-major
order that identical rows give; the hand-built image of synth.synthetic_detections_iou_tie
is the one deliberate exact equality.  Usage: python tests/golden/make_golden_sgdet.py

`python tests/golden/make_golden_sgdet.py cases` writes only decode_cases.npz and pairs_cases.npz: the same three reference
functions on the hand-built cases of tests/sgdet_cases.py (GOLDEN_DECODE, GOLDEN_PAIRS; prepare_test_pairs with its
max_proposal_pairs argument set to the instance's cap), outputs only -- the inputs are rebuilt by the case builders."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import configure, import_reference, load_sd  # noqa: E402
from veto_amd import synth  # noqa: E402
from test_sgdet_host import np_decode, np_onehot_prob, np_softmax  # noqa: E402

OUT = os.path.join(HERE, "sgdet")


def ref_decode(d, thr, dtype):
    from pysgg.modeling.roi_heads.relation_head.utils_relation import obj_prediction_nms
    from pysgg.modeling.roi_heads.relation_head.roi_relation_predictors import Ensemble
    import torch.nn.functional as F
    bpc = torch.from_numpy(d["boxes_per_cls"]).to(dtype)
    logits = torch.from_numpy(d["predict_logits"]).to(dtype)
    post = obj_prediction_nms(bpc, logits, thr).numpy()
    C = logits.shape[1]
    onehot = F.one_hot(torch.from_numpy(d["pred_labels"]), C).to(dtype)
    meet = Ensemble.nms_per_cls(types.SimpleNamespace(nms_thresh=thr), onehot, [bpc], [len(post)]).numpy()
    prob = F.softmax(logits, 1)
    prob[:, 0] = 0
    scores = prob[torch.arange(len(post)), torch.from_numpy(post)].numpy()
    return post, meet, scores


def robust(d, thr):
    p32, m32, _ = ref_decode(d, thr, torch.float32)
    p64, m64, _ = ref_decode(d, thr, torch.float64)
    if not (np.array_equal(p32, p64) and np.array_equal(m32, m64)):
        return False
    for mode, prob in (("post", np_softmax(d["predict_logits"])),
                       ("meet", np_onehot_prob(d["pred_labels"], d["predict_logits"].shape[1]))):
        iou = []
        lab = np_decode(prob, d["boxes_per_cls"], thr, mode, consulted=iou)
        if mode == "meet" and not np.array_equal(lab, m32):   # a tie decided by the reference's summation order
            return False
        if np.any(np.abs(np.asarray(iou, np.float64) - np.float32(thr)) < 1e-6):
            return False
    return True


def pick_seed(seed, n, C, thr, spread):
    for s in range(seed, seed + 200):
        d = synth.synthetic_detections(s, n, C, spread=spread)
        if robust(d, thr):
            return s, d
    raise RuntimeError("no robust seed near %d" % seed)


PRED_CASES = {   # name: (predictor, layers, heads, seed, n, thr)
    "pred_vanilla_n12_l4h8": ("VETOPredictor", 4, 8, 600, 12, 0.5),
    "pred_vanilla_n10_l6h6": ("VETOPredictor", 6, 6, 610, 10, 0.5),
    "pred_meet_n12_l4h8": ("VETOPredictor_MEET", 4, 8, 620, 12, 0.5),
    "pred_meet_n10_l6h6": ("VETOPredictor_MEET", 6, 6, 630, 10, 0.3),
}


def predictor_inputs(seed, n):
    """Detections of synth.synthetic_detections plus ROI maps of synth.synthetic_batch(seed, 1, [n])."""
    d = synth.synthetic_detections(seed, n, 151)
    b = synth.synthetic_batch(seed, 1, [n], num_obj_cls=151)
    d["roi_features"], d["roi_depth_features"] = b["roi_features"], b["roi_depth_features"]
    return d


def meet_decodes_differently(d, thr):
    """True when the MEET decoder's labels differ from the clamped pred_labels on some row (the case worth pinning)."""
    lab = np_decode(np_onehot_prob(d["pred_labels"], 151), d["boxes_per_cls"], thr, "meet")
    return not np.array_equal(lab, np.where(d["pred_labels"] > 0, d["pred_labels"], 1))


def run_predictor(P, cfg, BoxList, name):
    kind, layers, heads, seed, n, thr = PRED_CASES[name]
    meet = kind == "VETOPredictor_MEET"
    configure(P, cfg, "sgcls", layers, heads, kind, "VG")
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = thr
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
    for s in range(seed, seed + 200):
        d = predictor_inputs(s, n)
        if robust(d, thr) and (not meet or meet_decodes_differently(d, thr)):
            break
    else:
        raise RuntimeError("no usable seed for %s" % name)
    torch.manual_seed(0)
    model = getattr(P, kind)(cfg, 512)
    assert model.mode == "sgdet"
    sd = synth.meet_state_dict(0, list(model.max_group_element_number_list), layers=layers) if meet \
        else synth.predictor_state_dict(0, layers=layers)
    load_sd(model, sd)
    model.eval()
    b = BoxList(torch.from_numpy(d["boxes"]), d["image_size"], "xyxy")
    for k in ("predict_logits", "pred_labels", "pred_scores", "boxes_per_cls"):
        b.add_field(k, torch.from_numpy(d[k]))
    pairs = [torch.from_numpy(np.argwhere(~np.eye(n, dtype=bool)).astype(np.int64))]
    with torch.no_grad():
        res = model([b], pairs, None, None, roi_features=torch.from_numpy(d["roi_features"]),
                    roi_depth_features=torch.from_numpy(d["roi_depth_features"]))
    out = {"seed": np.int64(s), "n": np.int64(n), "thr": np.float64(thr), "layers": np.int64(layers), "heads": np.int64(heads),
           "meet": np.int64(meet), "pair_idx": pairs[0].numpy()}
    if meet:
        for k, v in res[1].items():
            out["rel_" + k] = v.numpy()
        out["decoder_labels"] = np_decode(np_onehot_prob(d["pred_labels"], 151), d["boxes_per_cls"], thr, "meet")
    else:
        out["rel_dists"] = torch.cat(list(res[1]), 0).numpy()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "seed", s, "logits", {k: v.shape for k, v in out.items() if k.startswith("rel")})


SGDET_EVAL = (33, [6, 9, 12, 3, 15, 20, 2, 8])


def run_sgg_eval_sgdet(cfg, BoxList):
    import pysgg.data.datasets.evaluation.vg.vg_eval as ve
    from pysgg.data.datasets.evaluation.vg.sgg_eval import (SGMeanRecall, SGNGMeanRecall, SGNoGraphConstraintRecall,
                                                             SGPairAccuracy, SGRecall, SGZeroShotRecall)
    seed, num_objs = SGDET_EVAL
    mode, num_rel = "sgdet", 51
    images, zeroshot = synth.synthetic_eval_images_sgdet(seed, num_objs, num_rel_cls=num_rel)
    rd = {}
    names = ["r%d" % i for i in range(num_rel)]
    evaluator = {"eval_recall": SGRecall(rd), "eval_nog_recall": SGNoGraphConstraintRecall(rd),
                 "eval_zeroshot_recall": SGZeroShotRecall(rd), "eval_pair_accuracy": SGPairAccuracy(rd),
                 "eval_mean_recall": SGMeanRecall(rd, num_rel, names, print_detail=True),
                 "eval_ng_mean_recall": SGNGMeanRecall(rd, num_rel, names, print_detail=True)}
    for e in evaluator.values():
        e.register_container(mode)
    gc = {"zeroshot_triplet": zeroshot, "result_dict": rd, "mode": mode, "multiple_preds": False,
          "num_rel_category": num_rel, "iou_thres": 0.5, "attribute_on": False, "num_attributes": 201}
    for img in images:
        gt = BoxList(torch.from_numpy(img["gt_boxes"]), (800, 600), mode="xyxy")
        gt.add_field("relation_tuple", torch.from_numpy(img["gt_rels"]))
        gt.add_field("labels", torch.from_numpy(img["gt_classes"]))
        pr = BoxList(torch.from_numpy(img["pred_boxes"]), (800, 600), mode="xyxy")
        pr.add_field("rel_pair_idxs", torch.from_numpy(img["pred_rel_inds"]))
        pr.add_field("pred_rel_scores", torch.from_numpy(img["rel_scores"]))
        pr.add_field("pred_labels", torch.from_numpy(img["pred_classes"]))
        pr.add_field("pred_scores", torch.from_numpy(img["obj_scores"]))
        ve.evaluate_relation_of_one_image(gt, pr, gc, evaluator)
    evaluator["eval_mean_recall"].calculate_mean_recall(mode)
    evaluator["eval_ng_mean_recall"].calculate_mean_recall(mode)
    out = {"seed": np.int64(seed), "num_objs": np.array(num_objs), "num_rel": np.int64(num_rel)}
    for key in ("recall", "recall_nogc", "zeroshot_recall", "accuracy_hit", "accuracy_count"):
        for k in (20, 50, 100):
            out["%s_%d" % (key, k)] = np.array(rd["%s_%s" % (mode, key)][k], dtype=np.float64)
    for key in ("mean_recall", "ng_mean_recall"):
        for k in (20, 50, 100):
            out["%s_%d" % (key, k)] = np.array(rd["%s_%s" % (mode, key)][k], dtype=np.float64)
            out["%s_list_%d" % (key, k)] = np.array(rd["%s_%s_list" % (mode, key)][k], dtype=np.float64)
    out["print_accuracy"] = np.array(evaluator["eval_pair_accuracy"].generate_print_string(mode))
    np.savez_compressed(os.path.join(OUT, "sggeval_sgdet.npz"), **out)
    print("sggeval_sgdet R@100 per image", out["recall_100"], "mR@100", out["mean_recall_100"],
          "A lists", len(out["accuracy_hit_100"]))


def run_cases(BoxList):
    """decode_cases.npz: <case>__labels (the case's mode; launches and images concatenated) and, in "post", <case>__scores.
    pairs_cases.npz: <case>__<instance>__pairs / __counts for the instances sgdet_cases.golden_pair_instances names."""
    import sgdet_cases as sc
    from pysgg.modeling.roi_heads.relation_head.sampling import RelationSampling
    dec, pairs = {}, {}
    for name in sc.GOLDEN_DECODE:
        mode, = sc.decode_modes(name)
        labels, scores = [], []
        for imgs, thr in sc.decode_case(name):
            for d in imgs:
                post, meet, sco = ref_decode(d, thr, torch.float32)
                p64, m64, _ = ref_decode(d, thr, torch.float64)
                ref, ref64 = (post, p64) if mode == "post" else (meet, m64)
                if mode == "post":     # (MEET: the fp64 softmax of a one-hot row has its own last-ulp pattern; the labels below decide)
                    assert np.array_equal(ref, ref64), (name, "the reference's labels change in fp64")
                labels.append(ref)
                scores.append(sco)
        dec[name + "__labels"] = np.concatenate(labels).astype(np.int64)
        if mode == "post":
            dec[name + "__scores"] = np.concatenate(scores).astype(np.float32)
        print(name, dec[name + "__labels"][:24])
    for name in sc.GOLDEN_PAIRS:
        case = sc.pair_case(name)
        for k in sc.golden_pair_instances(name):
            imgs, cap, overlap = case[k]
            samp = RelationSampling(0.5, False, 4, 1024, 0.25, cap, False, overlap)
            props = []
            for d in imgs:
                b = BoxList(torch.from_numpy(d["boxes"]), d["image_size"], "xyxy")
                b.add_field("pred_scores", torch.from_numpy(d["pred_scores"]))
                props.append(b)
            got = samp.prepare_test_pairs("cpu", props)
            pairs["%s__%d__pairs" % (name, k)] = torch.cat(got).numpy().astype(np.int16)
            pairs["%s__%d__counts" % (name, k)] = np.array([len(x) for x in got], np.int64)
            print(name, k, "cap", cap, "overlap", overlap, "counts", [len(x) for x in got])
    np.savez_compressed(os.path.join(OUT, "decode_cases.npz"), **dec)
    np.savez_compressed(os.path.join(OUT, "pairs_cases.npz"), **pairs)
    for f in ("decode_cases.npz", "pairs_cases.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


def main():
    P, cfg, BoxList = import_reference()
    if sys.argv[1:] == ["cases"]:
        return run_cases(BoxList)
    os.makedirs(OUT, exist_ok=True)
    run_sgg_eval_sgdet(cfg, BoxList)
    for name in PRED_CASES:
        run_predictor(P, cfg, BoxList, name)
    if os.environ.get("SGDET_GOLDEN_ONLY") == "extra":
        return
    from pysgg.modeling.roi_heads.relation_head.sampling import RelationSampling
    os.makedirs(OUT, exist_ok=True)
    # name: ([(seed, n), ...], n_cls, thr, spread)
    cases = {
        "n1": ([(100, 1)], 151, 0.3, 1.0), "n2": ([(110, 2)], 151, 0.5, 1.0), "n10": ([(120, 10)], 151, 0.3, 1.0),
        "n45": ([(130, 45)], 151, 0.5, 1.0), "n46": ([(140, 46)], 151, 0.3, 1.0), "n80": ([(150, 80)], 151, 0.5, 1.0),
        "n80_t03": ([(160, 80)], 151, 0.3, 1.0), "n100": ([(170, 100)], 151, 0.3, 1.0),
        "ragged12": ([(200 + 10 * i, 80 - 3 * (i % 4)) for i in range(12)], 151, 0.5, 1.0),
        "gqa_n80": ([(400, 80)], 201, 0.5, 1.0),
        "apart": ([(500, 6)], 151, 0.3, 40.0),
        "tie": ([(-1, 3)], 151, 0.5, 1.0),
    }
    dec, pairs = {}, {}
    for name, (imgs, C, thr, spread) in cases.items():
        seeds, ds = [], []
        for seed, n in imgs:
            if seed < 0:
                s, d = -1, synth.synthetic_detections_iou_tie(C)
            else:
                s, d = pick_seed(seed, n, C, thr, spread)
            seeds.append(s)
            ds.append(d)
        meta = {"seeds": np.array(seeds, np.int64), "n_objs": np.array([len(d["boxes"]) for d in ds], np.int64),
                "n_cls": np.int64(C), "spread": np.float64(spread)}
        outs = [ref_decode(d, thr, torch.float32) for d in ds]
        for k, v in meta.items():
            dec["%s__%s" % (name, k)] = v
        dec[name + "__thr"] = np.float64(thr)
        dec[name + "__labels_post"] = np.concatenate([o[0] for o in outs]).astype(np.int64)
        dec[name + "__labels_meet"] = np.concatenate([o[1] for o in outs]).astype(np.int64)
        dec[name + "__scores_post"] = np.concatenate([o[2] for o in outs]).astype(np.float32)
        for overlap in (False, True):
            samp = RelationSampling(0.5, False, 4, 1024, 0.25, 2048, False, overlap)
            props = []
            for d in ds:
                b = BoxList(torch.from_numpy(d["boxes"]), d["image_size"], "xyxy")
                b.add_field("pred_scores", torch.from_numpy(d["pred_scores"]))
                props.append(b)
            got = samp.prepare_test_pairs("cpu", props)
            key = "%s_%s" % (name, "ov" if overlap else "all")
            for k, v in meta.items():
                pairs["%s__%s" % (key, k)] = v
            pairs[key + "__cap"] = np.int64(2048)
            pairs[key + "__overlap"] = np.bool_(overlap)
            pairs[key + "__pairs"] = torch.cat(got).numpy().astype(np.int64)
            pairs[key + "__counts"] = np.array([len(x) for x in got], np.int64)
        print(name, "seeds", seeds, "labels", dec[name + "__labels_post"][:12])
    np.savez_compressed(os.path.join(OUT, "decode.npz"), **dec)
    np.savez_compressed(os.path.join(OUT, "pairs.npz"), **pairs)
    for f in ("decode.npz", "pairs.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
