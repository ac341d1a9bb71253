"""Times the RPN proposal selection of the VETO workload on the device: 12 images of 800 x 608, pyramid levels 152 x 200,
76 x 100, 38 x 50, 19 x 25 and 10 x 13 with 3 anchors per cell, PRE_NMS_TOP_N 6000, POST_NMS_TOP_N 1000, FPN_POST_NMS_TOP_N 1000,
NMS 0.7, per image.

Two paths in the same process on the same inputs: veto_amd.rpn.rpn_proposals (one C-ABI call per batch), and the baseline a
user has after install_detector_ops(): the reference's algorithm (rpn/inference.py:78-183) written in torch on the device,
calling veto_amd.layers.nms once per image and level.  Wall clock per batch includes the read-back that ends each path
(host clock around a call that ends in a device synchronise), after a warm-up, over --reps repetitions, the two paths
alternating: minimum and median.  Per-kernel device time of one batch of each path comes from torch.profiler in a pass of its
own.  Usage: python tools/rpn_bench.py [--reps 7] [--out profiles/rpn_bench.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import layers, rpn, synth  # noqa: E402

GRIDS = ((152, 200), (76, 100), (38, 50), (19, 25), (10, 13))
SET = dict(pre_nms_top_n=6000, post_nms_top_n=1000, nms_thresh=0.7, min_size=0, fpn_post_nms_top_n=1000)
CLIP = math.log(1000. / 16)


def baseline(objectness, box_regression, anchors, image_sizes):
    """RPNPostProcessor.forward in torch, eval mode, NMS through veto_amd.layers.nms per image and level."""
    per_img = [[] for _ in image_sizes]
    for obj, reg, anc in zip(objectness, box_regression, anchors):
        N, A, H, W = obj.shape
        obj = obj.view(N, -1, 1, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1).sigmoid()
        reg = reg.view(N, -1, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, 4)
        k = min(SET["pre_nms_top_n"], A * H * W)
        obj, idx = obj.topk(k, dim=1, sorted=True)
        batch = torch.arange(N, device=obj.device)[:, None]
        reg, a = reg[batch, idx], anc[idx]
        w, h = a[..., 2] - a[..., 0] + 1, a[..., 3] - a[..., 1] + 1
        cx, cy = a[..., 0] + 0.5 * w, a[..., 1] + 0.5 * h
        dw, dh = reg[..., 2].clamp(max=CLIP), reg[..., 3].clamp(max=CLIP)
        pcx, pcy, pw, ph = reg[..., 0] * w + cx, reg[..., 1] * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
        boxes = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], -1)
        for i, (iw, ih) in enumerate(image_sizes):
            b, s = boxes[i].clone(), obj[i]
            b[:, 0::2].clamp_(min=0, max=iw - 1)
            b[:, 1::2].clamp_(min=0, max=ih - 1)
            keep = ((b[:, 2] - b[:, 0] + 1 >= SET["min_size"]) & (b[:, 3] - b[:, 1] + 1 >= SET["min_size"])).nonzero().squeeze(1)
            b, s = b[keep], s[keep]
            keep = layers.nms(b, s, SET["nms_thresh"])[:SET["post_nms_top_n"]]
            per_img[i].append((b[keep], s[keep]))
    out = []
    for parts in per_img:
        b, s = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        _, order = torch.topk(s, min(SET["fpn_post_nms_top_n"], len(s)), dim=0, sorted=True)
        out.append((b[order], s[order]))
    return out


def kernel_times(fn):
    """(name, total us, calls) of the device kernels of one call, by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = [(e.key, getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0), e.count) for e in prof.key_averages()
            if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    return sorted(rows, key=lambda r: -r[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rpn_bench needs a HIP device")
    dev = "cuda"
    d = synth.synthetic_rpn_outputs(11, args.images, GRIDS)
    objectness = [torch.from_numpy(x).to(dev) for x in d["objectness"]]
    box_regression = [torch.from_numpy(x).to(dev) for x in d["box_regression"]]
    anchors = [torch.from_numpy(a).to(dev) for a in synth.anchor_grid((32, 64, 128, 256, 512), (4, 8, 16, 32, 64), (0.5, 1.0, 2.0), GRIDS)]
    sizes = [(800, 608)] * args.images

    def device_path():
        return rpn.rpn_proposals(objectness, box_regression, anchors, sizes, **SET)

    def torch_path():
        out = baseline(objectness, box_regression, anchors, sizes)
        torch.cuda.synchronize()
        return out

    mine, base = device_path(), torch_path()   # warm-up, and the two paths agree on what they keep
    # the baseline's topk orders equal fp32 sigmoid values its own way (distinct logits saturate to ties), so the two paths may
    # resolve a few near-ties differently: compare as sets of boxes rounded to 0.01 px
    as_set = lambda b: {tuple(r) for r in (b.cpu().numpy() * 100).round().astype("int64").tolist()}   # noqa: E731
    shared = [len(as_set(m["boxes"]) & as_set(b[0])) / max(len(m["boxes"]), 1) for m, b in zip(mine, base)]
    for _ in range(2):
        device_path(), torch_path()
    t_dev, t_base = [], []
    for _ in range(max(5, args.reps)):
        for fn, acc in ((device_path, t_dev), (torch_path, t_base)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    lines = ["RPN proposal selection, %d images of 800 x 608, 5 levels, A = 3, pre 6000 / post 1000 / fpn 1000, NMS 0.7" % args.images,
             "device: %s; %d timed repetitions after 3 warm-up batches, the paths alternating; wall clock per batch, read-back included"
             % (torch.cuda.get_device_name(0), len(t_dev)),
             "proposals per image %s; share of the device path's boxes that the baseline keeps too: min %.4f, mean %.4f"
             % (sorted({len(m["boxes"]) for m in mine}), min(shared), sum(shared) / len(shared)),
             "veto_rpn_proposals          min %8.3f ms   median %8.3f ms   max %8.3f ms" % (min(t_dev), statistics.median(t_dev), max(t_dev)),
             "torch + layers.nms per seg  min %8.3f ms   median %8.3f ms   max %8.3f ms" % (min(t_base), statistics.median(t_base), max(t_base))]
    for title, fn in (("veto_rpn_proposals", device_path), ("torch + layers.nms per segment", torch_path)):
        try:
            rows = kernel_times(fn)
            lines.append("kernels of one batch, %s: %d launches, %.1f us of device time" % (title, sum(r[2] for r in rows), sum(r[1] for r in rows)))
            lines += ["  %10.1f us  x%-4d %s" % (us, n, name[:110]) for name, us, n in rows[:12]]
        except Exception as e:   # the profiler is optional equipment: the wall-clock figures above stand on their own
            lines.append("kernels of one batch, %s: not measured (%s: %s)" % (title, type(e).__name__, e))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
