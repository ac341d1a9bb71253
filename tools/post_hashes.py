"""sha256 of everything veto_amd.postprocess.PostProcessor returns -- the bytes of every result field, the triple scores and the
kept row counts -- on the post-processor cases of tests/: every batch of post_batch_cases.py as a batch and image by image, its
sgdet merge and vote batches, and the MEET, vote and vanilla cases of post_eval_cases.py.  One line per call and image; two trees
that print the same lines compute the same bits.  Only the public call is used, so the file runs unchanged in another checkout.
Usage: python tools/post_hashes.py > FILE"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import post_batch_cases as bc  # noqa: E402
import post_eval_cases as pc  # noqa: E402
from veto_amd import testing  # noqa: E402
from veto_amd.postprocess import PostProcessor  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

DEV = torch.device("cuda:0")
FIELDS = ("rel_pair_idxs", "pred_rel_scores", "pred_rel_labels", "pred_labels", "pred_scores")
to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(label, rel, objs, pairs, boxes, incre=None, voting=None, use_gt_box=True):
    cfg = None
    if voting:
        cfg = testing.make_config(1, 8, meet=True, dataset="VG")
        cfg.ENSEMBLE_LEARNING.EXPERT_GROUP, cfg.ENSEMBLE_LEARNING.VOTING = True, voting
    post = PostProcessor(False, use_gt_box=use_gt_box, later_nms_pred_thres=bc.SGDET_THR, cfg=cfg)
    rel = {k: to(v) for k, v in rel.items()} if isinstance(rel, dict) else [to(r) for r in rel]
    kw = dict(incre_idx_list=incre, ensemble=True) if incre is not None else {}
    res = post((rel, [to(o) for o in objs]), [to(p) for p in pairs], boxes, **kw)
    for i, (r, t) in enumerate(zip(res, post.last_triple_scores)):
        named = [(k, r.get_field(k)) for k in FIELDS] + [("triple", t)] + ([] if use_gt_box else [("bbox", r.bbox)])
        print("%s image %d kept %d %s" % (label, i, t.shape[0], " ".join(
            "%s=%s" % (k, hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]) for k, v in named)))


def gt_boxes(ns):
    return [BoxList(torch.zeros(n, 4), (800, 600)).to(DEV) for n in ns]


def main():
    for b in bc.BATCH_NAMES:
        x = bc.inputs(b)
        run("batch " + b, x["rel"], x["obj"], x["pairs"], gt_boxes(x["n_objs"]), x["incre"], bc.voting(b))
        for i, n in enumerate(x["n_objs"]):
            s = bc.image_slices(b, i)
            run("alone %s[%d]" % (b, i), s["rel"], [s["obj"]], [s["pairs"]], gt_boxes([n]), x["incre"], bc.voting(b))
    for expert in (False, True):
        s = bc.sgdet_batch(expert)
        props = []
        for d in s["dets"]:
            props.append(BoxList(to(d["boxes"]), d["image_size"], "xyxy"))
            props[-1].add_field("boxes_per_cls", to(d["boxes_per_cls"]))
        run("sgdet " + ("vote_C" if expert else "merge"), s["rel"], [d["predict_logits"] for d in s["dets"]], s["pairs"], props,
            s["incre"], "C" if expert else None, use_gt_box=False)
    for kind, names in (("meet", ("vg36", "gqa_limit", "capped_ties")), ("vote", ("vg36_C", "vg36_U", "capped_ties_C", "none_U", "all_U"))):
        for name in names:
            c = getattr(pc, kind + "_case")(name)
            run("%s %s" % (kind, name), c["rel"], [c["obj"]], [c["pairs"]], gt_boxes([c["n"]]), c["incre"], c.get("voting"))
    for name in ("random", "ties"):      # pair counts [0, 1, 1260, 0, 2, 16384, 90] in one batch
        c = pc.vanilla_case(name)
        run("vanilla " + name, np.split(c["rel"], np.cumsum([len(p) for p in c["pairs"]])[:-1]),
            np.split(c["obj"], np.cumsum(c["num_objs"])[:-1]), c["pairs"], gt_boxes(c["num_objs"]))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
