"""Writes tests/golden/rpnloss/*.npz: what the reference's own RPNLossComputation (pysgg/modeling/rpn/loss.py:21-157) with its
Matcher, BoxCoder, BalancedPositiveNegativeSampler and AnchorGenerator computes on CPU tensors, one batch per fixture.

The inputs are regenerated from tests/rpnloss_cases.py (synth.anchor_grid, asserted equal to the reference's AnchorGenerator, and
synth.synthetic_rpn_training_batch; the hand-built cases keep their few boxes in that module), so a fixture stores the seed and
the outputs only.  Per image: labels (int8), matched_idxs (int16), regression_targets, the anchors the reference sampled for
torch.manual_seed(case number) and, at those anchors, the gradients of a second run on float64 head outputs; per fixture the two
losses in fp32 and in float64, ref_fp32_err_targets (the largest absolute difference between the reference's fp32 targets and a
float64 recomputation) and ref_fp32_err_loss (the largest relative difference between its fp32 and float64 losses).

A seed is rejected (the next one is tried) when the float64 recomputation of the matching moves any anchor across a threshold;
the tie sets of the low-quality step are fp32 facts and are not part of that check.  It is also rejected when any sampled |d|
lies within 1e-5 of beta.  Asserted per hand-built case: lowq -- every positive comes from the low-quality step, two anchors tie
for one GT, one anchor is best for two; zero_gt -- the GT that overlaps nothing restores every anchor; thresholds -- IoU exactly
on `high` matches, exactly on `low` is ignored; no_pos -- no positive.
Usage: python tests/golden/make_golden_rpnloss.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402
import rpnloss_cases as rc  # noqa: E402


def reference_anchor_lists(BoxList, c, d, seeded):
    from pysgg.modeling.rpn.anchor_generator import AnchorGenerator
    if not hasattr(np, "float"):
        np.float = float   # the reference predates numpy 1.24
    if seeded:
        sizes = tuple((s,) for s in c["sizes"]) if len(c["strides"]) > 1 else tuple(c["sizes"][0])
        gen = AnchorGenerator(sizes, rc.RATIOS, c["strides"], c["straddle"])
        ref = gen.grid_anchors([tuple(g) for g in c["grids"]])
        assert len(ref) == len(d["anchors"])
        for r, m in zip(ref, d["anchors"]):
            assert np.array_equal(r.numpy(), m), "synth.anchor_grid differs from the reference's AnchorGenerator"
    else:
        gen = AnchorGenerator(straddle_thresh=c["straddle"])
    lists = []
    for size in d["image_sizes"]:
        per_level = []
        for a in d["anchors"]:
            b = BoxList(torch.from_numpy(a), size, mode="xyxy")
            gen.add_visibility_to(b)
            per_level.append(b)
        lists.append(per_level)
    return lists


def run_reference(BoxList, name, c, d, torch_seed):
    from pysgg.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from pysgg.modeling.box_coder import BoxCoder
    from pysgg.modeling.matcher import Matcher
    from pysgg.modeling.rpn.loss import RPNLossComputation, generate_rpn_labels
    from pysgg.structures.boxlist_ops import cat_boxlist
    loss = RPNLossComputation(Matcher(c["high"], c["low"], allow_low_quality_matches=c["lowq"]),
                              BalancedPositiveNegativeSampler(c["batch"], c["fraction"]), BoxCoder(weights=rc.WEIGHTS), generate_rpn_labels)
    anchors = reference_anchor_lists(BoxList, c, d, name in rc.SEEDED)
    targets = [BoxList(torch.from_numpy(t), size, mode="xyxy") for t, size in zip(d["tgt_boxes"], d["image_sizes"])]
    cat = [cat_boxlist(per_img) for per_img in anchors]
    matched = [loss.match_targets_to_anchors(a, t).get_field("matched_idxs").numpy() for a, t in zip(cat, targets)]
    labels, reg = loss.prepare_targets(cat, targets)
    torch.manual_seed(torch_seed)
    pos, neg = loss.fg_bg_sampler(labels)
    sampled = [torch.nonzero(p | n).squeeze(1).numpy().astype(np.int64) for p, n in zip(pos, neg)]
    out = {}
    for dtype in (torch.float32, torch.float64):
        obj = [torch.tensor(o, dtype=dtype, requires_grad=True) for o in d["objectness"]]
        box = [torch.tensor(r, dtype=dtype, requires_grad=True) for r in d["box_regression"]]
        torch.manual_seed(torch_seed)   # prepare_targets draws nothing: the sampler repeats the draws above
        if dtype == torch.float64:      # binary_cross_entropy_with_logits wants the labels in the logits' dtype
            prepare = loss.prepare_targets
            loss.prepare_targets = lambda a, t: ([l.double() for l in prepare(a, t)[0]], prepare(a, t)[1])
        lo, lb = loss(anchors, obj, box, targets)
        (lo + lb).backward()
        out[dtype] = (float(lo.detach()), float(lb.detach()), [o.grad.numpy() for o in obj], [b.grad.numpy() for b in box])
    return matched, [l.numpy() for l in labels], [r.numpy() for r in reg], sampled, out[torch.float32], out[torch.float64]


def attempt(BoxList, name, seed, case_no):
    """(fixture dict, robust?)"""
    c, d = rc.case_inputs(name, seed)
    shapes = d["level_shapes"]
    matched, labels, reg, sampled, r32, r64 = run_reference(BoxList, name, c, d, case_no)
    all_anchors = np.concatenate(d["anchors"])
    robust, err_t = True, 0.0
    z = {"seed": np.int64(seed), "losses_fp32": np.array(r32[:2], np.float32), "losses_fp64": np.array(r64[:2], np.float64)}
    for i, (t, size) in enumerate(zip(d["tgt_boxes"], d["image_sizes"])):
        m32, l32, t32, plain32 = rc.np_rpn_match(all_anchors, t, size, c["high"], c["low"], c["lowq"], c["straddle"])
        plain64 = rc.np_rpn_match(all_anchors, t, size, c["high"], c["low"], c["lowq"], c["straddle"], dtype=np.float64)[3]
        robust &= np.array_equal(plain32, plain64)
        assert np.array_equal(m32, matched[i]) and np.array_equal(l32, labels[i]), "%s: np_rpn_match differs from the reference" % name
        t64 = rc.np_encode(all_anchors, t[np.maximum(matched[i], 0)], rc.WEIGHTS, np.float64)
        err_t = max(err_t, float(np.abs(reg[i].astype(np.float64) - t64).max()))
        pos = sampled[i][labels[i][sampled[i]] >= 1]
        resid = np.abs(rc.gather_nchw(d["box_regression"], shapes, i, pos, 4).astype(np.float64) - reg[i][pos])
        robust &= not np.any(np.abs(resid - rc.BETA) < 1e-5)
        z["labels_%d" % i] = labels[i].astype(np.int8)
        z["matched_%d" % i] = matched[i].astype(np.int16)
        z["targets_%d" % i] = reg[i]
        z["sampled_%d" % i] = sampled[i]
        z["grad_objectness_%d" % i] = rc.gather_nchw(r64[2], shapes, i, sampled[i], 1)[:, 0]
        z["grad_box_regression_%d" % i] = rc.gather_nchw(r64[3], shapes, i, sampled[i], 4)
    rel = [abs(a - b) / abs(b) for a, b in zip(r32[:2], r64[:2]) if b != 0]
    z["ref_fp32_err_targets"] = np.float64(err_t)
    z["ref_fp32_err_loss"] = np.float64(max(rel))
    check_named_for(name, c, d, matched, labels, all_anchors)
    return z, bool(robust)


def check_named_for(name, c, d, matched, labels, anchors):
    if name not in rc.HAND:
        return
    tgt, m, lab = d["tgt_boxes"][0], matched[0], labels[0]
    iou = rc.np_iou(tgt, anchors)
    plain = rc.np_rpn_match(anchors, tgt, d["image_sizes"][0], c["high"], c["low"], False, c["straddle"])[0]
    if name == "lowq":
        assert (iou.max(1) < c["high"]).all() and (lab == 1).any() and not (plain >= 0).any(), "every positive comes from the low-quality step"
        assert iou[0, 0] == iou[0, 1] == iou[0].max() and m[0] == m[1] == 0                       # two anchors tie for GT 0
        assert iou[1].argmax() == iou[2].argmax() == 2 and iou[1, 2] == iou[2, 2] and m[2] == 1  # one anchor best for GT 1 and 2
        assert m.tolist() == [0, 0, 1, -1, -1, -2, -1], m
    if name == "zero_gt":
        assert iou[1].max() == 0 and (m >= 0).all() and (plain < 0).any(), m                     # restore-everything
        assert lab.tolist() == [1, 1, 1, -1, 1], lab                                             # anchor 3 leaves the image
    if name == "thresholds":
        assert iou[0, 0] == c["high"] and iou[0, 1] == c["low"] and m.tolist() == [0, -2, 0, -1, 0, -1], m
    if name == "no_pos":
        assert not (lab == 1).any() and (lab == 0).any()


def main():
    _, _, BoxList = import_reference()
    os.makedirs(rc.GOLDEN, exist_ok=True)
    for case_no, name in enumerate(rc.ALL):
        first = rc.SEEDED[name]["first_seed"] if name in rc.SEEDED else rc.HAND[name]["seed"]
        for seed in range(first, first + (50 if name in rc.SEEDED else 20)):
            z, robust = attempt(BoxList, name, seed, case_no)
            if robust:
                break
        else:
            raise RuntimeError("no robust seed for %s" % name)
        path = os.path.join(rc.GOLDEN, name + ".npz")
        np.savez_compressed(path, **z)
        n_img = len([k for k in z if k.startswith("labels_")])
        print(name, "seed", seed, "positives", [int((z["labels_%d" % i] == 1).sum()) for i in range(n_img)],
              "sampled", [len(z["sampled_%d" % i]) for i in range(n_img)], "losses", z["losses_fp32"].tolist(),
              "err targets %.3g loss %.3g" % (z["ref_fp32_err_targets"], z["ref_fp32_err_loss"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
