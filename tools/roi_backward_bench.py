"""Times the ROI pooling backward at the training shape: 12 images x 36 boxes, 256 channels, 4 pyramid levels of a 1216 x 800 image + the
stride-16 depth map, pooled 8, ratio 2.  Default entry (the caller's zero fill + the atomic scatter) against veto_roi_pool_backward_ordered
(the gather, which writes every element), alternating; profiles/train_deterministic.txt section 3.

With --layout / --dtype the leaves are taken to have that form and, per entry point, two paths to their gradients are timed against each
other in this process, alternating, `--rounds` windows of `--reps` calls each: IN PLACE -- float32 gradient maps in the leaves' layout, then
one cast to the leaves' dtype -- and COPY -- float32 NCHW gradient maps, then the cast and re-stride into the leaves' dtype and memory
format, which is what autograd did for such leaves before.  (For an NCHW leaf the two are the same code; nothing to compare.)  Prints per
path the median window and the spread (min .. max), and whether the ordered results are bit-equal.
usage: tools/roi_backward_bench.py [--layout nhwc] [--dtype float32|float16|bfloat16] [--rounds 5] [--reps 5]"""
import argparse
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from veto_amd import native, poolers, synth

ap = argparse.ArgumentParser()
ap.add_argument("--layout", choices=["nchw", "nhwc"], default=None)
ap.add_argument("--dtype", choices=["float32", "float16", "bfloat16"], default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
opt = ap.parse_args()

dev = torch.device("cuda:0")
W, H, B, C = 1216, 800, 12, 256
rng = np.random.RandomState(5)
boxes = [synth.roi_test_boxes(rng, 36, W, H) for _ in range(B)]
rois = torch.from_numpy(np.concatenate([np.concatenate([np.full((36, 1), i, dtype=np.float32), b], 1) for i, b in enumerate(boxes)])).to(dev)
shapes = [(B, C, H >> (2 + l), W >> (2 + l)) for l in range(4)]
dshape = (B, C, H >> 4, W >> 4)
scales = (0.25, 0.125, 0.0625, 0.03125)
g_rgb = torch.randn(len(rois), C, 8, 8, device=dev)
g_dep = torch.randn(len(rois), C, 8, 8, device=dev)
map_bytes = sum(int(np.prod(s)) for s in shapes + [dshape]) * 4


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


if opt.layout is None and opt.dtype is None:
    for ordered in (False, True, False, True):
        window(lambda: poolers._roi_pool_backward(shapes, scales, rois, B, 8, 2, g_rgb, dshape, g_dep, ordered=ordered), 3)
        ms, out = window(lambda: poolers._roi_pool_backward(shapes, scales, rois, B, 8, 2, g_rgb, dshape, g_dep, ordered=ordered), 10)
        print("%s entry, map allocation and fill included: %.3f ms per call (map bytes %.2f GB)"
              % ("ordered" if ordered else "default", ms, map_bytes / 2 ** 30))
        del out
    sys.exit(0)

if opt.layout != "nhwc":
    sys.exit("an NCHW leaf's gradient is computed by the same code on both paths: nothing to compare (use --layout nhwc)")
form = (poolers._DTYPE_CODES[getattr(torch, opt.dtype or "float32")], native.VETO_ROI_NHWC)


def grads(ordered, layout):
    lv, dp = poolers._roi_pool_backward(shapes, scales, rois, B, 8, 2, g_rgb, dshape, g_dep, ordered=ordered, level_layout=layout,
                                        depth_layout=layout)
    return [poolers._as_leaf(g, form) for g in lv + [dp]]


for ordered in (False, True):
    paths = {"in place": lambda: grads(ordered, native.VETO_ROI_NHWC), "copy": lambda: grads(ordered, native.VETO_ROI_NCHW)}
    times, outs = {k: [] for k in paths}, {}
    for fn in paths.values():
        window(fn, 2)
    for _ in range(opt.rounds):
        for name, fn in paths.items():
            ms, outs[name] = window(fn, opt.reps)
            times[name].append(ms)
    for a, b in zip(outs["in place"], outs["copy"]):
        assert a.dtype == b.dtype and a.stride() == b.stride()
    same = all(torch.equal(a, b) for a, b in zip(outs["in place"], outs["copy"]))
    del outs
    print("roi_pool backward, %s entry, leaves nhwc %s: %d ROIs, float32 map bytes %.2f GB, %d windows x %d calls, allocation and fill included%s"
          % ("ordered" if ordered else "atomic", opt.dtype or "float32", len(rois), map_bytes / 2 ** 30, opt.rounds, opt.reps,
             ", results bit-equal: %s" % same if ordered else ""))
    for name, ts in times.items():
        ts = sorted(ts)
        print("  %-9s median %.3f ms per call   spread %.3f .. %.3f ms" % (name, ts[len(ts) // 2], ts[0], ts[-1]))
