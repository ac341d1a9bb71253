"""Writes tests/golden/sgdet/relsample.npz: what the reference's RelationSampling.detect_relsample
(pysgg/modeling/roi_heads/relation_head/sampling.py:109-176, with motif_rel_fg_bg_sampling :179-309) returns on synthetic
training images (veto_amd.synth.synthetic_relsample_image), one image per case, run on CPU tensors.

Per case: the inputs, the config (FG_IOU_THRESHOLD, REQUIRE_BOX_OVERLAP, NUM_SAMPLE_PER_GT_REL, BATCH_SIZE_PER_IMAGE,
POSITIVE_FRACTION), the returned pairs, labels, rel_labels_all (when the target has relation_non_masked), binary_rel and
locating_match, the IoUs boxlist_iou(target, proposal), and rel_possibility after the foreground removal -- the bound
motif_rel_fg_bg_sampling is wrapped and its mutated argument cloned after the call (the reference stays untouched).
The reference draws from numpy's and torch's generators, seeded per case here.

With `large` it writes tests/golden/sgdet/relsample_large.npz instead: the same arrays for the cases of
tests/relsample_cases.py (LARGE_CASES), one image each at the sizes sgdet training has and at the sampler's limits of 256
proposals and 256 GT boxes.  relsample.npz is left alone then.
Usage: python tests/golden/make_golden_relsample_sgdet.py [large]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402
import relsample_cases  # noqa: E402
from veto_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "sgdet")

# name: (image seed, n_gt, n_det, n_rel, synth options, (fg_thres, overlap, per_rel, batch, fraction), non_masked)
CASES = {
    "many": (11, 8, 40, 10, dict(), (0.5, False, 4, 1024, 0.25), True),
    "many_overlap": (11, 8, 40, 10, dict(), (0.5, True, 4, 1024, 0.25), False),
    "twin": (12, 6, 30, 8, dict(twin=True), (0.5, False, 4, 1024, 0.25), True),
    "cap": (13, 10, 60, 20, dict(), (0.5, False, 4, 64, 0.25), True),
    "cap_overlap": (13, 10, 60, 20, dict(), (0.5, True, 4, 64, 0.25), False),
    "small": (14, 4, 10, 3, dict(max_copies=2), (0.5, False, 4, 1024, 0.25), True),
    "small_overlap": (14, 4, 10, 3, dict(max_copies=2), (0.5, True, 4, 1024, 0.25), False),
    "degenerate": (15, 2, 3, 1, dict(max_copies=0, clutter_bg=1.0), (0.5, False, 4, 1024, 0.25), True),
}


def run_case(BoxList, RelationSampling, seed, d, cfg, non_masked):
    fg_thres, overlap, per_rel, batch, frac = cfg
    samp = RelationSampling(fg_thres, overlap, per_rel, batch, frac, 2048, False, False)   # use_gt_box False
    captured = []
    orig = samp.motif_rel_fg_bg_sampling

    def wrapped(device, tgt_rel_matrix, ious, is_match, rel_possibility, quality):
        out = orig(device, tgt_rel_matrix, ious, is_match, rel_possibility, quality)
        captured.append((ious.clone(), rel_possibility.clone()))
        return out

    samp.motif_rel_fg_bg_sampling = wrapped
    size = d["image_size"]
    p = BoxList(torch.from_numpy(d["prp_boxes"]), size, mode="xyxy")
    p.add_field("labels", torch.from_numpy(d["prp_labels"]))
    p.add_field("pred_scores", torch.from_numpy(d["pred_scores"]))
    t = BoxList(torch.from_numpy(d["tgt_boxes"]), size, mode="xyxy")
    t.add_field("labels", torch.from_numpy(d["tgt_labels"]))
    t.add_field("relation", torch.from_numpy(d["relation"]))
    if non_masked:
        t.add_field("relation_non_masked", torch.from_numpy(d["relation_non_masked"]))
    np.random.seed(seed)
    torch.manual_seed(seed)
    props, labels, labels_all, pairs, binary = samp.detect_relsample([p], [t])
    ious, poss = captured[0]
    out = {"pairs": pairs[0].numpy(), "labels": labels[0].numpy(), "binary_rel": binary[0].numpy(),
           "locating_match": props[0].get_field("locating_match").numpy().astype(np.float32), "ious": ious.numpy(),
           "rel_possibility": poss.numpy().astype(np.int64)}
    if non_masked:
        out["labels_all"] = labels_all[0].numpy()
    return out


def store(arrays, name, d, out, cfg, non_masked):
    for k in ("prp_boxes", "prp_labels", "pred_scores", "tgt_boxes", "tgt_labels", "relation"):
        arrays[name + "__" + k] = d[k]
    if non_masked:
        arrays[name + "__relation_non_masked"] = d["relation_non_masked"]
    arrays[name + "__config"] = np.array([cfg[0], float(cfg[1]), cfg[2], cfg[3], cfg[4]], np.float64)
    for k, v in out.items():
        arrays[name + "__" + k] = v
    print(name, "rows", len(out["pairs"]), "fg", int((out["labels"] > 0).sum()))


def main(large=False):
    _, _, BoxList = import_reference()
    from pysgg.modeling.roi_heads.relation_head.sampling import RelationSampling
    arrays = {}
    if large:
        for name, case in relsample_cases.LARGE_CASES.items():
            d, cfg, non_masked = relsample_cases.large_case_inputs(name)
            store(arrays, name, d, run_case(BoxList, RelationSampling, case[0], d, cfg, non_masked), cfg, non_masked)
    else:
        for name, (seed, n_gt, n_det, n_rel, opts, cfg, non_masked) in CASES.items():
            d = synth.synthetic_relsample_image(seed, n_gt, n_det, n_rel, **opts)
            store(arrays, name, d, run_case(BoxList, RelationSampling, seed, d, cfg, non_masked), cfg, non_masked)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "relsample_large.npz" if large else "relsample.npz"), **arrays)


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["large"]):
        sys.exit(__doc__)
    main(large=sys.argv[1:] == ["large"])
