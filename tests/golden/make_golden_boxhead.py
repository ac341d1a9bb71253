"""Writes tests/golden/boxhead/*.npz: what the reference's box-head PostProcessor computes from the box head's raw outputs.

Runs the reference itself (pysgg, imported with make_golden's stubs): PostProcessor.forward / filter_results
(box_head/inference.py:51-238), BoxCoder.decode, BoxList.clip_to_image and boxlist_nms, on inputs regenerated from
veto_amd.synth seeds, and stores OUTPUTS AND SEEDS ONLY.

The one gap: pysgg._C.nms (csrc/cuda/nms.cu) is a CUDA extension that cannot be built where the fixtures are made.  Behind
`pysgg.layers.nms` / `boxlist_ops._box_nms` this generator therefore puts a numpy restatement of that kernel
(test_boxhead_host.np_nms: score-descending greedy :73-75 and :112-123, devIoU :13-21, suppression at IoU > threshold :60,
ascending keep :127-130).  The fixtures are the reference's decoder around a restated NMS primitive.  nms.npz (NMS alone)
is that restatement's output, in fp32 arithmetic.

A seed is rejected (the next one is tried, at most 200 per case) when a ulp of difference in exp / softmax could change a
decision: the fp32 and fp64 results differ in any index, label or count; an IoU the greedy pass consults lies within 1e-5
of the threshold; a probability lies within 1e-6 of SCORE_THRESH; two scores inside one NMS segment are equal; the scores
on either side of the DETECTIONS_PER_IMG cut are closer than 1e-6.  The deliberate exact cases are hand-built, not seeded
(test_boxhead_host.hand_built_image, nms_fixture_inputs): two boxes at IoU exactly 0.5 with threshold 0.5 -- both kept under
`>` -- and two equal scores at the cut -- both kept.

Per decoder fixture, ref_fp32_err_boxes / ref_fp32_err_scores = the largest absolute difference between the reference's fp32
outputs and the fp64 recomputation (test_boxhead_host.np_box_postprocess in float64): the GPU tests allow 4x that.
Usage: python tests/golden/make_golden_boxhead.py [case ... | nms]   (no argument: every fixture)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference  # noqa: E402
from veto_amd import synth  # noqa: E402
from test_boxhead_host import hand_built_image, nms_fixture_inputs, np_box_postprocess, np_nms  # noqa: E402

OUT = os.path.join(HERE, "boxhead")
VETO = dict(score_thresh=0.01, nms=0.3, topn=300, filter_dup=True, det_per_img=80, weights=(10., 10., 5., 5.), cls_agnostic=False)
# name: (n_cls, [(seed, n, kind)], parameter overrides, store the full decode)
CASES = {
    "n20_full": (151, [(1000, 20, "synth")], {}, True),
    "vg1000": (151, [(1100, 1000, "synth")], {}, False),
    "vg1000_nodup": (151, [(1100, 1000, "synth")], dict(filter_dup=False, det_per_img=256), False),
    "ragged12": (151, [(1200 + 10 * i, n, "synth") for i, n in enumerate((12, 40, 25, 8, 33, 20, 15, 38, 10, 28, 22, 30))], {}, False),
    "gqa": (201, [(1400, 300, "synth")], {}, False),
    "agnostic": (151, [(1500, 200, "synth")], dict(cls_agnostic=True), False),
    "nothing": (151, [(1600, 30, "synth"), (-1, 10, "nothing")], {}, False),
    "below_cap": (151, [(1700, 30, "synth")], {}, False),
    "tie_cap": (151, [(-1, 3, "tie_cap")], dict(det_per_img=1), False),
    # branches of filter_results no seeded case enters: a binding POST_NMS_PER_CLS_TOPN, and the class-major list at 300 classes
    "topn_bind": (2, [(-1, 10, "topn_bind")], dict(topn=3, det_per_img=0), False),
    "topn_bind_nodup": (2, [(-1, 10, "topn_bind")], dict(topn=3, det_per_img=0, filter_dup=False), False),
    "class_major_wide": (300, [(-1, 6, "class_major")], dict(filter_dup=False, det_per_img=0), False),
    "class_major_wide_cut": (300, [(-1, 6, "class_major")], dict(filter_dup=False, det_per_img=4), False),
}
NMS_SIZES = (0, 1, 2, 63, 64, 65, 1000, 6000)


def torch_nms(boxes, scores, thr):
    """What stands behind pysgg.layers.nms here: the numpy restatement of nms.cu, in the dtype of the boxes."""
    dtype = np.float64 if boxes.dtype == torch.float64 else np.float32
    return torch.from_numpy(np_nms(boxes.numpy(), scores.numpy(), thr, dtype))


def ref_postprocess(BoxList, d, prm):
    from pysgg.modeling.box_coder import BoxCoder
    from pysgg.modeling.roi_heads.box_head.inference import PostProcessor
    post = PostProcessor(prm["score_thresh"], prm["nms"], prm["topn"], prm["filter_dup"], prm["det_per_img"],
                         BoxCoder(weights=prm["weights"]), prm["cls_agnostic"], False, False)
    post.eval()
    n = len(d["proposals"])
    b = BoxList(torch.from_numpy(d["proposals"]), d["image_size"], "xyxy")
    b.add_field("predict_logits", torch.from_numpy(d["class_logits"]))
    feats = torch.arange(n, dtype=torch.float32).reshape(n, 1)
    with torch.no_grad():
        nms_feats, res = post((feats, torch.from_numpy(d["class_logits"]), torch.from_numpy(d["box_regression"])), [b])
    r = res[0]
    reg = torch.from_numpy(d["box_regression"])
    dec = post.box_coder.decode(reg[:, -4:] if prm["cls_agnostic"] else reg, torch.from_numpy(d["proposals"]))
    if prm["cls_agnostic"]:
        dec = dec.repeat(1, d["class_logits"].shape[1])
    dec = BoxList(dec.reshape(-1, 4), d["image_size"], "xyxy").clip_to_image(remove_empty=False).bbox.reshape(n, -1, 4).numpy()
    return {"dec_full": dec, "orig_inds": nms_feats.reshape(-1).long().numpy(), "pred_labels": r.get_field("pred_labels").numpy().astype(np.int64),
            "pred_scores": r.get_field("pred_scores").numpy(), "boxes": r.bbox.numpy(),
            "boxes_per_cls": r.get_field("boxes_per_cls").numpy()}


def check(BoxList, d, prm):
    """(reference outputs, fp32-vs-fp64 errors of boxes and scores, robust?)."""
    ref = ref_postprocess(BoxList, d, prm)
    diag32, diag64 = {}, {}
    mine = np_box_postprocess(d, prm, np.float32, diag32)
    f64 = np_box_postprocess(d, prm, np.float64, diag64)
    for other in (mine, f64):
        if not (np.array_equal(ref["orig_inds"], other["orig_inds"]) and np.array_equal(ref["pred_labels"], other["pred_labels"])):
            return ref, 0.0, 0.0, False
    robust = not (np.any(np.abs(diag64["consulted"] - prm["nms"]) < 1e-5) or
                  np.any(np.abs(diag32["consulted"].astype(np.float64) - prm["nms"]) < 1e-5) or
                  np.any(np.abs(diag64["prob"] - prm["score_thresh"]) < 1e-6) or diag32["seg_ties"] or diag64["cut_gap"] < 1e-6)
    err_b = max(np.abs(ref["boxes"] - f64["boxes"]).max(initial=0), np.abs(ref["boxes_per_cls"] - f64["boxes_per_cls"]).max(initial=0),
                np.abs(ref["dec_full"] - diag64["dec"]).max(initial=0))
    err_s = np.abs(ref["pred_scores"] - f64["pred_scores"]).max(initial=0)
    return ref, float(err_b), float(err_s), robust


def main():
    _, _, BoxList = import_reference()
    import pysgg.layers
    import pysgg.structures.boxlist_ops as ops
    pysgg.layers.nms = ops._box_nms = torch_nms
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    for name, (C, images, over, full) in CASES.items():
        if only and name not in only:
            continue
        prm = dict(VETO, **over)
        seeds, outs, err_b, err_s, dec_full = [], [], 0.0, 0.0, None
        for seed, n, kind in images:
            if seed < 0:
                got = check(BoxList, hand_built_image(kind, C), prm)
                if kind == "nothing":   # every probability is 1 / C: not near the threshold, nothing to consult
                    assert got[3] and len(got[0]["orig_inds"]) == 0
                elif kind == "topn_bind":   # rows 0, 1, 2 although row 9 scores best
                    assert got[3] and got[0]["orig_inds"].tolist() == [0, 1, 2]
                elif kind == "class_major":   # class-major, rows ascending; the cut of 4 drops row 0 and the three entries of row 5
                    assert got[3] and got[0]["pred_labels"].tolist() == ([1, 1, 255, 256, 257, 257, 299, 299] if prm["det_per_img"] == 0
                                                                         else [1, 255, 256, 257])
                else:                   # the tie at the cut is the point of this image: exempt from the cut-gap rule only
                    assert len(got[0]["orig_inds"]) == 2 and prm["det_per_img"] == 1
                s = -1
            else:
                for s in range(seed, seed + 200):
                    got = check(BoxList, synth.synthetic_box_head_outputs(s, n, C, cls_agnostic=prm["cls_agnostic"]), prm)
                    if got[3]:
                        break
                else:
                    raise RuntimeError("no robust seed near %d for %s" % (seed, name))
            seeds.append(s)
            outs.append(got[0])
            err_b, err_s = max(err_b, got[1]), max(err_s, got[2])
            dec_full = got[0]["dec_full"]
        z = {"n_cls": np.int64(C), "seeds": np.array(seeds, np.int64), "n_per_img": np.array([n for _, n, _ in images], np.int64),
             "kinds": np.array([k for _, _, k in images]), "counts": np.array([len(o["orig_inds"]) for o in outs], np.int64),
             "score_thresh": np.float64(prm["score_thresh"]), "nms": np.float64(prm["nms"]), "topn": np.int64(prm["topn"]),
             "filter_dup": np.bool_(prm["filter_dup"]), "det_per_img": np.int64(prm["det_per_img"]),
             "weights": np.array(prm["weights"], np.float64), "cls_agnostic": np.bool_(prm["cls_agnostic"]),
             "ref_fp32_err_boxes": np.float64(err_b), "ref_fp32_err_scores": np.float64(err_s)}
        for k in ("orig_inds", "pred_labels", "pred_scores", "boxes", "boxes_per_cls"):
            z[k] = np.concatenate([o[k] for o in outs], 0)
        if full:
            z["dec_full"] = dec_full
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, "seeds", seeds, "counts", z["counts"].tolist(), "err boxes %.3g scores %.3g" % (err_b, err_s),
              os.path.getsize(path), "bytes")
    if only and "nms" not in only:
        return
    z = {}
    cases = []
    for thr in (0.7, 0.3):
        for n in NMS_SIZES:
            name = "n%d_t%02d" % (n, int(thr * 10))
            for s in range(2000 + n, 2000 + n + 200):
                boxes, scores = nms_fixture_inputs(s, n)
                c32, c64 = [], []
                k32, k64 = np_nms(boxes, scores, thr, np.float32, c32), np_nms(boxes, scores, thr, np.float64, c64)
                near = any(np.any(np.abs(c.astype(np.float64) - thr) < 1e-5) for c in c32 + c64)
                if np.array_equal(k32, k64) and not near and len(np.unique(scores)) == len(scores):
                    break
            else:
                raise RuntimeError("no robust seed for %s" % name)
            cases.append(name)
            z[name + "__seed"], z[name + "__n"], z[name + "__thr"], z[name + "__keep"] = np.int64(s), np.int64(n), np.float64(thr), k32
            print(name, "seed", s, "kept", len(k32))
    boxes, scores = nms_fixture_inputs(-1, 2)
    cases.append("iou_tie")
    z["iou_tie__seed"], z["iou_tie__n"], z["iou_tie__thr"] = np.int64(-1), np.int64(2), np.float64(0.5)
    z["iou_tie__keep"] = np_nms(boxes, scores, 0.5)
    z["cases"] = np.array(cases)
    np.savez_compressed(os.path.join(OUT, "nms.npz"), **z)
    print("nms.npz", os.path.getsize(os.path.join(OUT, "nms.npz")), "bytes; iou_tie keep", z["iou_tie__keep"])


if __name__ == "__main__":
    main()
