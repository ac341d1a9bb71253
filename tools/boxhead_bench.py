"""Times the sgdet box decoder on the device.

  decoder    veto_amd.boxhead.PostProcessor at 12 images x 1000 proposals x 151 classes (VETO_final.yaml settings)
  torch-loop a plain torch restatement of the reference's per-class loop (inference.py:157-238) around veto_amd.layers.nms,
             on the same inputs: what install_detector_ops() without the device PostProcessor would run
  nms-6000   veto_amd.layers.batched_nms on one segment of 6000 boxes (the RPN's PRE_NMS_TOP_N_TEST) at 0.7

Wall-clock per call (the calls end in their one read-back, so they are synchronous), median and spread over --iters calls
after --warmup; --kernels-only runs a few decoder and NMS calls and nothing else, for a kernel trace.
Usage: python tools/boxhead_bench.py [--iters 30] [--warmup 5] [--loop-iters 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import synth  # noqa: E402
from veto_amd.boxhead import PostProcessor  # noqa: E402
from veto_amd.layers import batched_nms, nms  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

DEV = "cuda"


def torch_loop(class_logits, box_regression, props, thr=0.01, nms_thr=0.3, topn=300, cap=80, weights=(10., 10., 5., 5.)):
    """The reference's PostProcessor in plain torch (duplicates filtered), one nms call per image x class."""
    prob = torch.softmax(class_logits, -1)
    boxes = torch.cat([b.bbox for b in props])
    w = boxes[:, 2] - boxes[:, 0] + 1
    h = boxes[:, 3] - boxes[:, 1] + 1
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    r = box_regression.reshape(len(boxes), -1, 4)
    dx, dy = r[..., 0] / weights[0], r[..., 1] / weights[1]
    dw = (r[..., 2] / weights[2]).clamp(max=float(np.log(1000. / 16)))
    dh = (r[..., 3] / weights[3]).clamp(max=float(np.log(1000. / 16)))
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    dec = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], -1)
    out, row = [], 0
    for b in props:
        n = len(b)
        d, p = dec[row:row + n].clone(), prob[row:row + n]
        d[..., 0::2].clamp_(0, b.size[0] - 1)
        d[..., 1::2].clamp_(0, b.size[1] - 1)
        alive = torch.zeros_like(p, dtype=torch.bool)
        cand = p > thr
        for j in range(1, p.shape[1]):
            inds = cand[:, j].nonzero().squeeze(1)
            if len(inds) == 0:
                continue
            keep = nms(d[inds, j].contiguous(), p[inds, j].contiguous(), nms_thr)[:topn]
            alive[inds[keep], j] = True
        scores, labels = (p * alive).max(1)
        rows = scores.nonzero().squeeze(1)
        scores, labels = scores[rows], labels[rows]
        if len(rows) > cap > 0:
            cut = torch.kthvalue(scores, len(rows) - cap + 1)[0]
            sel = (scores >= cut).nonzero().squeeze(1)
            rows, scores, labels = rows[sel], scores[sel], labels[sel]
        out.append((rows, labels, scores, d[rows, labels], d[rows]))
        row += n
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    imgs = [synth.synthetic_box_head_outputs(900 + i, 1000) for i in range(12)]
    props = []
    for d in imgs:
        b = BoxList(torch.from_numpy(d["proposals"]).to(DEV), d["image_size"], "xyxy")
        b.add_field("predict_logits", torch.from_numpy(d["class_logits"]).to(DEV))
        props.append(b)
    logits = torch.cat([b.get_field("predict_logits") for b in props])
    reg = torch.from_numpy(np.concatenate([d["box_regression"] for d in imgs])).to(DEV)
    feats = torch.zeros((len(logits), 16), device=DEV)
    post = PostProcessor(0.01, 0.3, 300, True, 80).eval()
    nb, ns = synth.synthetic_nms_boxes(7, 6000)
    nb, ns = torch.from_numpy(nb).to(DEV), torch.from_numpy(ns).to(DEV)
    run_post = lambda: post((feats, logits, reg), props)   # noqa: E731
    run_nms = lambda: batched_nms(nb, ns, (0, 6000), 0.7)[1].tolist()   # noqa: E731
    if a.kernels_only:
        for _ in range(5):
            run_post()
            run_nms()
        torch.cuda.synchronize()
        return
    lines = []
    got, want = run_post()[1], torch_loop(logits, reg, props)
    same = all(torch.equal(g.get_field("pred_labels"), w[1]) and len(g) == len(w[0]) for g, w in zip(got, want))
    lines.append("decoder vs torch-loop: same detections per image: %s (%s)" % (same, [len(g) for g in got]))
    for name, fn, it in (("decoder 12 x 1000 x 151", run_post, a.iters), ("nms-6000 @0.7", run_nms, a.iters),
                         ("torch-loop 12 x 1000 x 151", lambda: torch_loop(logits, reg, props), a.loop_iters)):
        med, lo, hi = timed(fn, it, a.warmup if it == a.iters else 1)
        lines.append("%-28s median %9.3f ms  (min %9.3f, max %9.3f, %d calls)" % (name, med, lo, hi, it))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
