"""Writes tests/golden/boxloss/*.npz: what the reference's own FastRCNNLossComputation (pysgg/modeling/roi_heads/box_head/loss.py:
15-84) computes on CPU tensors, in fp32 and in float64, one batch per fixture, given as per-image lists.

The inputs are regenerated from tests/boxloss_cases.py, so a fixture stores outputs only: the two losses in both precisions; the
float64 gradients of `rows` (every row where R * 4C <= 65 536, otherwise 64 seeded rows and every hand-set row); and the
reference's own fp32-against-float64 errors in the metrics of boxloss_cases (ref_fp32_err_loss, ref_fp32_err_dlogits,
ref_fp32_err_dbox), from which the device tests take their bounds.  Asserted per case: box_loss_fp64 reproduces the float64 run,
and the case holds what it is named for.
Usage: python tests/golden/make_golden_boxloss.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402
import boxloss_cases as bc  # noqa: E402


def run_reference(BoxList, d, dtype):
    from pysgg.modeling.roi_heads.box_head.loss import FastRCNNLossComputation
    logits = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in d["class_logits"]]
    reg = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in d["box_regression"]]
    proposals = []
    for lab, tgt in zip(d["labels"], d["regression_targets"]):
        p = BoxList(torch.zeros((len(lab), 4)), (640, 480), mode="xyxy")
        p.add_field("labels", torch.from_numpy(lab))
        p.add_field("regression_targets", torch.tensor(tgt, dtype=dtype))
        proposals.append(p)
    cls_loss, box_loss = FastRCNNLossComputation(d["agnostic"])(logits, reg, proposals)
    g_logits = torch.autograd.grad(cls_loss, logits, retain_graph=True)
    if box_loss.requires_grad:
        g_reg = torch.autograd.grad(box_loss, reg, allow_unused=True)
        g_reg = [torch.zeros_like(r) if g is None else g for g, r in zip(g_reg, reg)]
    else:
        g_reg = [torch.zeros_like(r) for r in reg]
    return (np.array([float(cls_loss.detach()), float(box_loss.detach())], np.float64), torch.cat(g_logits).numpy().astype(np.float64),
            torch.cat(g_reg).numpy().astype(np.float64))


def check_named_for(name, d, o):
    """The case holds what it is named for (tests/test_boxloss_host.py repeats these on the committed fixtures)."""
    labels = np.concatenate(d["labels"])
    C = d["class_logits"][0].shape[1]
    if name == "no_pos":
        assert not (labels > 0).any() and o["losses"][1] == 0 and not o["d_box_regression"].any()
    if name == "all_pos":
        assert (labels > 0).all()
    if name in ("vg", "agnostic", "ragged"):
        assert 0.1 < (labels > 0).mean() < 0.45
    if name.startswith("lanes") or name == "two_cls":
        assert {0, C - 1, min(63, C - 1)} <= set(labels.tolist())
    if name == "wide":
        assert {1023, 960} <= set(labels.tolist())
    if name == "kink":
        _, x, y, t = bc.concatenated(d)
        got = sorted({float(np.float64(x[r, 4 + c]) - np.float64(t[r, c])) for r in np.nonzero(y > 0)[0] for c in range(4)})
        assert set(bc.KINK_D) <= set(got), got


def main():
    _, _, BoxList = import_reference()
    os.makedirs(bc.GOLDEN, exist_ok=True)
    for name in bc.ALL:
        d = bc.case_inputs(name)
        l32, gl32, gr32 = run_reference(BoxList, d, torch.float32)
        l64, gl64, gr64 = run_reference(BoxList, d, torch.float64)
        o = bc.box_loss_fp64(*bc.concatenated(d), agnostic=d["agnostic"])
        assert bc.loss_err(o["losses"], l64) <= 1e-12, (name, o["losses"], l64)
        assert bc.dlogits_err(o["d_class_logits"], gl64, o["p"], o["onehot"]) <= 1e-12, name
        assert bc.dbox_err(o["d_box_regression"], gr64) <= 1e-12, name
        check_named_for(name, d, o)
        rows = bc.grad_rows(name, d)
        z = {"losses_fp32": l32.astype(np.float32), "losses_fp64": l64, "rows": rows.astype(np.int64),
             "d_class_logits_fp64": gl64[rows], "d_box_regression_fp64": gr64[rows],
             "ref_fp32_err_loss": np.float64(bc.loss_err(l32, l64)),
             "ref_fp32_err_dlogits": np.float64(bc.dlogits_err(gl32, gl64, o["p"], o["onehot"])),
             "ref_fp32_err_dbox": np.float64(bc.dbox_err(gr32, gr64))}
        path = os.path.join(bc.GOLDEN, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, "R", len(gl64), "C", gl64.shape[1], "positives", int((np.concatenate(d["labels"]) > 0).sum()), "losses", l32.tolist(),
              "err loss %.3g dlogits %.3g dbox %.3g" % (z["ref_fp32_err_loss"], z["ref_fp32_err_dlogits"], z["ref_fp32_err_dbox"]),
              "rows kept", len(rows), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
