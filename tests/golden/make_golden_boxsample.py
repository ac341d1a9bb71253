"""Writes tests/golden/boxsample/*.npz: what the reference's own FastRCNNSampling (roi_heads/box_head/sampling.py:14-156) with
its Matcher, BoxCoder and BalancedPositiveNegativeSampler returns on CPU tensors, one fixture per case, one batch per fixture.

Seeded cases regenerate their inputs from veto_amd.synth.synthetic_box_sampling_image (GT boxes, clustered detections, the GT
boxes appended to the proposals), so a fixture stores the seeds, the sizes, the settings and the outputs only.  The hand-built
cases store their few boxes as well: IoU exactly 0.5 and exactly 0.25, each sitting on a threshold, and duplicated GT boxes
with proposals equal to them, on which this generator asserts that the reference's max(dim=0) returns the lowest GT index.

Per image: matched_idxs, the labels of assign_label_to_proposals and of prepare_targets, attributes, regression_targets, and
the indices subsample kept (an `orig_index` field rides through its BoxList indexing) for torch.manual_seed(case number).
A seed is rejected (the next one is tried) when the fp64 recomputation of the matching (test_boxsample_host.np_box_match in
float64) changes any matched_idx, i.e. an IoU lies within rounding of a threshold; the hand-built cases are exact in both.
Per fixture, ref_fp32_err_targets = the largest absolute difference between the reference's fp32 regression_targets and that
fp64 recomputation: the GPU tests allow 4x that.
Usage: python tests/golden/make_golden_boxsample.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402
from test_boxsample_host import np_box_match  # noqa: E402
from veto_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "boxsample")
WEIGHTS = (10., 10., 5., 5.)

# name: ([(first seed, n_gt, n_det)], high, low, BATCH_SIZE_PER_IMAGE, POSITIVE_FRACTION)
SEEDED = {
    "vg": ([(101, 8, 60), (121, 5, 40)], 0.5, 0.3, 32, 0.25),
    "equal": ([(141, 6, 50)], 0.5, 0.5, 256, 0.25),
    "ragged": ([(161, 3, 10), (181, 12, 300), (201, 1, 5), (221, 7, 250)], 0.5, 0.3, 64, 0.25),
    "one_gt": ([(241, 1, 30)], 0.5, 0.3, 16, 0.5),
    "gt256": ([(261, 256, 300)], 0.5, 0.3, 256, 0.25),
    "under_quota": ([(281, 4, 20), (301, 2, 9)], 0.5, 0.3, 512, 0.25),
}

A, B, C, D = [10, 10, 109, 109], [200, 50, 299, 199], [400, 300, 519, 419], [50, 400, 149, 499]
HAND = {
    "threshold": (dict(tgt_boxes=[[0, 0, 9, 9]], tgt_labels=[4],
                       prp_boxes=[[0, 0, 9, 4], [0, 0, 4, 4], [0, 0, 9, 9], [100, 100, 120, 120], [0, 0, 9, 5], [0, 0, 3, 4]]),
                  0.5, 0.25, 4, 0.5),
    "ties": (dict(tgt_boxes=[A, A, B, C, D, C], tgt_labels=[5, 9, 7, 11, 13, 17],
                  prp_boxes=[A, B, C, [14, 12, 113, 111], D, [600, 20, 700, 90], C, [10, 10, 109, 80]]),
             0.5, 0.3, 8, 0.25),
}


def hand_image(spec):
    n = len(spec["tgt_boxes"])
    return {"prp_boxes": np.asarray(spec["prp_boxes"], np.float32), "tgt_boxes": np.asarray(spec["tgt_boxes"], np.float32),
            "tgt_labels": np.asarray(spec["tgt_labels"], np.int64), "image_size": (800, 600),
            "attributes": (np.arange(n * 3, dtype=np.int64).reshape(n, 3) % 7) + 1}


def run_reference(ref, images, high, low, batch, fraction, torch_seed):
    BoxList, FastRCNNSampling, Matcher, BoxCoder, Sampler = ref
    samp = FastRCNNSampling(Matcher(high, low, allow_low_quality_matches=False), Sampler(batch, fraction), BoxCoder(weights=WEIGHTS))

    def lists():
        props, targets = [], []
        for d in images:
            p = BoxList(torch.from_numpy(d["prp_boxes"]), d["image_size"], mode="xyxy")
            p.add_field("orig_index", torch.arange(len(p)))
            t = BoxList(torch.from_numpy(d["tgt_boxes"]), d["image_size"], mode="xyxy")
            t.add_field("labels", torch.from_numpy(d["tgt_labels"]))
            t.add_field("attributes", torch.from_numpy(d["attributes"]))
            props.append(p)
            targets.append(t)
        return props, targets

    props, targets = lists()
    assign = [p.get_field("labels").numpy() for p in samp.assign_label_to_proposals(props, targets)]
    props, targets = lists()
    labels, attributes, reg, matched = samp.prepare_targets(props, targets)
    torch.manual_seed(torch_seed)
    sampled = samp.subsample(props, targets)
    out = []
    for i, p in enumerate(props):
        assert torch.equal(p.get_field("labels"), labels[i]) and torch.equal(p.get_field("matched_idxs"), matched[i])
        assert reg[i].dtype == torch.float32 and labels[i].dtype == matched[i].dtype == torch.int64
        out.append({"matched": matched[i].numpy(), "labels_assign": assign[i], "labels_prepare": labels[i].numpy(),
                    "attributes": attributes[i].numpy(), "targets": reg[i].numpy(),
                    "sampled": sampled[i].get_field("orig_index").numpy().astype(np.int64)})
    return out


def fp64_check(d, o, high, low):
    """(matching unchanged in fp64, the reference's fp32 error of the regression targets)."""
    matched, assign, prepare, targets = np_box_match(d["prp_boxes"], d["tgt_boxes"], d["tgt_labels"], high, low, WEIGHTS, np.float64)
    same = np.array_equal(matched, o["matched"])
    return same, float(np.abs(targets - o["targets"].astype(np.float64)).max()) if same else 0.0


def main():
    import_reference()
    from pysgg.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from pysgg.modeling.box_coder import BoxCoder
    from pysgg.modeling.matcher import Matcher
    from pysgg.modeling.roi_heads.box_head.sampling import FastRCNNSampling
    from pysgg.structures.bounding_box import BoxList
    ref = (BoxList, FastRCNNSampling, Matcher, BoxCoder, BalancedPositiveNegativeSampler)
    os.makedirs(OUT, exist_ok=True)
    for case_no, (name, (specs, high, low, batch, fraction)) in enumerate(SEEDED.items()):
        seeds, images = [], []
        for first, n_gt, n_det in specs:
            for s in range(first, first + 20):
                d = synth.synthetic_box_sampling_image(s, n_gt, n_det)
                o = run_reference(ref, [d], high, low, batch, fraction, 0)[0]
                if fp64_check(d, o, high, low)[0]:
                    break
            else:
                raise RuntimeError("no robust seed near %d for %s" % (first, name))
            seeds.append(s)
            images.append(d)
        outs = run_reference(ref, images, high, low, batch, fraction, case_no)
        save(name, images, outs, high, low, batch, fraction, seeds=np.array(seeds, np.int64),
             n_gt=np.array([g for _, g, _ in specs], np.int64), n_det=np.array([n for _, _, n in specs], np.int64))
    for case_no, (name, (spec, high, low, batch, fraction)) in enumerate(HAND.items()):
        d = hand_image(spec)
        outs = run_reference(ref, [d], high, low, batch, fraction, 100 + case_no)
        extra = {"in_%s_0" % k: d[k] for k in ("prp_boxes", "tgt_boxes", "tgt_labels", "attributes")}
        save(name, [d], outs, high, low, batch, fraction, n_gt=np.array([len(d["tgt_boxes"])], np.int64), **extra)
        if name == "ties":      # CPU max(dim=0) returns the lowest GT index among equal maxima
            m = outs[0]["matched"]
            assert m[0] == 0 and m[2] == 3 and m[6] == 3 and m[1] == 2 and 1 not in m and 5 not in m, m
        if name == "threshold":
            assert outs[0]["matched"].tolist()[:3] == [0, -2, 0], outs[0]["matched"]


def save(name, images, outs, high, low, batch, fraction, **extra):
    err = 0.0
    for d, o in zip(images, outs):
        same, e = fp64_check(d, o, high, low)
        assert same, name
        err = max(err, e)
    z = {"high": np.float64(high), "low": np.float64(low), "batch": np.int64(batch), "fraction": np.float64(fraction),
         "weights": np.array(WEIGHTS, np.float64), "n_prp": np.array([len(d["prp_boxes"]) for d in images], np.int64),
         "ref_fp32_err_targets": np.float64(err)}
    z.update(extra)
    for i, o in enumerate(outs):
        for k, v in o.items():
            z["%s_%d" % (k, i)] = v
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **z)
    print(name, "seeds", extra.get("seeds", "-"), "proposals", z["n_prp"].tolist(), "matched >= 0:",
          [int((o["matched"] >= 0).sum()) for o in outs], "between:", [int((o["matched"] == -2).sum()) for o in outs],
          "sampled:", [len(o["sampled"]) for o in outs], "ref fp32 err %.3g" % err)


if __name__ == "__main__":
    main()
