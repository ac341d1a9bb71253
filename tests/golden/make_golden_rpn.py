"""Writes tests/golden/rpn/*.npz: what the reference's RPNPostProcessor (pysgg/modeling/rpn/inference.py:13-210) computes from
the RPN head's raw outputs.

Runs the reference itself (pysgg, imported with make_golden's stubs) on BoxList anchors, in eval or training mode as the case
says, on inputs regenerated from veto_amd.synth seeds, and stores OUTPUTS AND SEEDS ONLY.  As in make_golden_boxhead.py,
the numpy restatement test_boxhead_host.np_nms stands behind `pysgg.layers.nms` / `boxlist_ops._box_nms` (pysgg._C.nms is a
CUDA extension that cannot be built where the fixtures are made).  synth.anchor_grid is asserted equal to the reference's
AnchorGenerator for every fixture's geometry; the fixtures keep a checksum of the anchors.

The reference does not emit pyramid levels or anchor indices: they come from test_rpn_host.np_rpn_proposals (float32 and
float64), which is accepted only when its counts equal the reference's and its boxes and objectness agree with the reference's
row by row (1e-3 px, 1e-6).

A seed is rejected (the next one is tried, at most 200 per case) when a ulp could change a decision: float32 and float64
disagree in any level, anchor index or count; an IoU the greedy pass consults lies within 1e-5 of the threshold; a side length
lies within 1e-4 of min_size (when min_size > 0 can bind); the two logits that meet at a cut -- the pre-NMS k, the
POST_NMS_TOP_N cap, the cut across the levels -- are equal or map to equal float32 sigmoid values.  Asserted per seeded case: the
NMS of at least one segment removes at least a tenth of its candidates and keeps at least a tenth; min_size: the filter removes
at least one candidate and leaves at least one; small5: the POST_NMS_TOP_N cap binds in a segment; per_batch: the images end with
different counts.

`ties` is hand-built (test_rpn_host.ties_inputs); its expected output is the restatement's, i.e. the orders this project fixes
where the reference's topk leaves ties open.  It is checked against the reference only as a set, on the rows whose membership
the reference determines (everything but the tied logits).  `min_size_exact` is hand-built too (min_size_exact_inputs: sides
exactly min_size and one below it), with distinct logits: the reference determines every row and is compared row by row.

Per fixture, ref_fp32_err_boxes / ref_fp32_err_objectness = the largest absolute difference between the reference's float32
outputs and the float64 restatement: the GPU tests allow 4x that.
Usage: python tests/golden/make_golden_rpn.py [case ...]   (no case: all of them)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference  # noqa: E402
from make_golden_boxhead import torch_nms  # noqa: E402
from veto_amd import synth  # noqa: E402
from test_rpn_host import CASES, RATIOS, anchor_checksum, case_inputs, np_rpn_proposals, np_sigmoid, rpn_targets  # noqa: E402

OUT = os.path.join(HERE, "rpn")
FIRST_SEED = {"small5": 3000, "below_cap": 3100, "min_size": 3200, "one_level": 3300, "per_batch": 3400, "add_gt": 3500,
              "full_level": 3600, "ties": -1, "min_size_exact": -1}


def ref_forward(BoxList, d, c, targets):
    from pysgg.modeling.rpn.inference import RPNPostProcessor
    post = RPNPostProcessor(c["pre"], c["post"], c["thr"], c["min_size"], None, c["fpn"], bool(c.get("per_batch", False)),
                            bool(c.get("add_gt", 0)))
    post.train(bool(c.get("training", False)))
    anchors = [[BoxList(torch.from_numpy(a), size, "xyxy") for a in d["anchors"]] for size in c["images"]]
    tg = [BoxList(torch.from_numpy(t), size, "xyxy") for t, size in zip(targets, c["images"])] if targets else None
    with torch.no_grad():
        res = post(anchors, [torch.from_numpy(o) for o in d["objectness"]], [torch.from_numpy(r) for r in d["box_regression"]], tg)
    return [dict(boxes=r.bbox.numpy(), objectness=r.get_field("objectness").numpy()) for r in res]


def check_anchors(c):
    from pysgg.modeling.rpn.anchor_generator import AnchorGenerator
    if not hasattr(np, "float"):
        np.float = float   # the reference predates numpy 1.24
    gen = AnchorGenerator(tuple((s,) for s in c["sizes"]) if len(c["strides"]) > 1 else tuple(c["sizes"]), RATIOS, c["strides"])
    ref = gen.grid_anchors([tuple(g) for g in c["grids"]])
    mine = synth.anchor_grid(c["sizes"], c["strides"], RATIOS, c["grids"])
    assert len(ref) == len(mine)
    for r, m in zip(ref, mine):
        assert np.array_equal(r.numpy(), m), "synth.anchor_grid differs from the reference's AnchorGenerator"


def attempt(BoxList, name, seed):
    """(fixture dict, robust?)"""
    c = CASES[name]
    d = case_inputs(name, seed)
    n_gt = c.get("add_gt", 0)
    targets = rpn_targets(seed, c["images"], n_gt) if n_gt else None
    ref = ref_forward(BoxList, d, c, targets)
    diag32, diag64 = {}, {}
    m32, m64 = np_rpn_proposals(d, c, np.float32, diag32), np_rpn_proposals(d, c, np.float64, diag64)
    hand = bool(c.get("hand_built")) and not c.get("determinate")   # (a determinate hand-built case is compared row by row)
    for r, a, b in zip(ref, m32, m64):
        k = len(r["boxes"]) - n_gt
        if len(a["boxes"]) != k or len(b["boxes"]) != k:
            return None, False
        if not (np.array_equal(a["level"], b["level"]) and np.array_equal(a["anchor_index"], b["anchor_index"])):
            return None, False
        if hand:   # the reference leaves the tied rows open: compare as sets, and only the rows above the tied logit
            sure = a["logit"] > np.float32(1.52)
            got = {tuple(x) for x in r["boxes"][:k][r["objectness"][:k] > np_sigmoid(np.float32([1.52]), np.float32)[0]].tolist()}
            assert got == {tuple(x) for x in a["boxes"][sure].tolist()}, "ties: the determinate rows differ from the reference's"
        elif np.abs(r["boxes"][:k] - a["boxes"]).max(initial=0) > 1e-3 or np.abs(r["objectness"][:k] - a["objectness"]).max(initial=0) > 1e-6:
            return None, False
    robust = True
    if not c.get("hand_built"):
        for dg in (diag32, diag64):
            robust &= not np.any(np.abs(dg["consulted"].astype(np.float64) - c["thr"]) < 1e-5)
            if c["min_size"] > 0:
                robust &= not np.any(np.abs(dg["sides"].astype(np.float64) - c["min_size"]) < 1e-4)
        for hi, lo in diag32["cuts"]:
            robust &= hi != lo and np_sigmoid(np.float32([hi]), np.float32)[0] != np_sigmoid(np.float32([lo]), np.float32)[0]
        nin, nout = np.array(diag32["nms_in"]), np.array(diag32["nms_out"])
        robust &= bool(np.any((nin - nout >= 0.1 * nin) & (nout >= 0.1 * nin) & (nin > 0)))
        if name == "min_size":
            removed = sum(int((s.reshape(2, -1) < c["min_size"]).any(0).sum()) for s in [diag32["sides"]])
            robust &= 0 < removed < diag32["sides"].size // 2
        if name == "small5":
            robust &= bool(np.any(nout > c["post"]))
        if name == "per_batch":
            robust &= len({len(a["boxes"]) for a in m32}) == len(m32)
    err_b = err_o = 0.0
    rows = []
    for i, (r, a, b) in enumerate(zip(ref, m32, m64)):
        k = len(r["boxes"]) - n_gt
        src = a if hand else dict(a, boxes=r["boxes"][:k], objectness=r["objectness"][:k])
        err_b = max(err_b, float(np.abs(src["boxes"].astype(np.float64) - b["boxes"]).max(initial=0)))
        err_o = max(err_o, float(np.abs(src["objectness"].astype(np.float64) - b["objectness"]).max(initial=0)))
        row = dict(boxes=src["boxes"], objectness=src["objectness"], level=a["level"], anchor_index=a["anchor_index"])
        if n_gt:
            assert np.array_equal(r["boxes"][k:], targets[i]) and np.all(r["objectness"][k:] == 1)
            row = dict(boxes=np.concatenate([row["boxes"], targets[i]]), objectness=np.concatenate([row["objectness"], np.ones(n_gt, np.float32)]),
                       level=np.concatenate([row["level"], np.full(n_gt, -1, np.int32)]),
                       anchor_index=np.concatenate([row["anchor_index"], np.full(n_gt, -1, np.int64)]))
        rows.append(row)
    z = {"seed": np.int64(seed), "counts": np.array([len(r["boxes"]) for r in rows], np.int64),
         "ref_fp32_err_boxes": np.float64(err_b), "ref_fp32_err_objectness": np.float64(err_o),
         "anchor_sha256": np.array(anchor_checksum(d["anchors"]))}
    for key in ("boxes", "objectness", "level", "anchor_index"):
        z[key] = np.concatenate([r[key] for r in rows])
    return z, robust


def main():
    _, _, BoxList = import_reference()
    import pysgg.layers
    import pysgg.structures.boxlist_ops as ops
    pysgg.layers.nms = ops._box_nms = torch_nms
    os.makedirs(OUT, exist_ok=True)
    for name, c in CASES.items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        if c.get("hand_built"):
            z, _ = attempt(BoxList, name, -1)
            assert z is not None
            if name == "min_size_exact":   # the kept anchors are those of min_size_exact_inputs' docstring, best logit first
                assert z["anchor_index"].tolist() == [5, 0, 3, 6] and float(z["ref_fp32_err_boxes"]) == 0.0
        else:
            check_anchors(c)
            for seed in range(FIRST_SEED[name], FIRST_SEED[name] + 200):
                z, robust = attempt(BoxList, name, seed)
                if robust:
                    break
            else:
                raise RuntimeError("no robust seed for %s" % name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, "seed", int(z["seed"]), "counts", z["counts"].tolist(), "err boxes %.3g objectness %.3g" %
              (z["ref_fp32_err_boxes"], z["ref_fp32_err_objectness"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
