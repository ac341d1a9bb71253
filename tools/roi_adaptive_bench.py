"""Times ROI pooling on the adaptive grid (sampling_ratio = 0, veto_roi_pool_adaptive) against sampling_ratio = 2 on the same ROIs, at
the box head's shape: 8 images x 1000 clipped proposals of a 1216 x 800 image, 7 x 7, 256 channels, four pyramid levels, float32 NCHW;
and the same ROIs grown by 4000 px on every side, whose sample grids are hundreds of times larger while the samples inside the maps
are bounded by the maps.  profiles/roi_adaptive.txt keeps one run.

Measured: device time per call (HIP events around `--reps` calls through the C ABI with preallocated outputs and argument structs built
once, outside the window; the two ratios alternate, `--rounds` windows each; median and spread).  The backward is timed on gradient maps that are zeroed once, outside the window.
Counted on the host from the float32 grid arithmetic (not measured): mean gh * gw and the number of valid samples per batch.
Derived: time per valid sample = median time / valid samples (a sample serves all 256 channels).
usage: tools/roi_adaptive_bench.py [--rounds 5] [--reps 20]"""
import argparse
import ctypes
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from veto_amd import native, poolers

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
opt = ap.parse_args()

F = np.float32
dev = torch.device("cuda:0")
W, H, B, C, P, N = 1216, 800, 8, 256, 7, 1000
scales = (0.25, 0.125, 0.0625, 0.03125)
shapes = [(B, C, H >> (2 + l), W >> (2 + l)) for l in range(4)]


def proposals(rng):
    """log-uniform sizes, clipped to the image as the RPN's are"""
    cxy = rng.uniform(0, [W, H], size=(N, 2))
    wh = np.exp(rng.uniform(np.log(8), np.log(900), size=(N, 2)))
    b = np.concatenate([cxy - wh / 2, cxy + wh / 2], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W - 1)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, H - 1)
    return b.astype(F)


def sample_counts(rois, levels, ratio):
    """(sum of gh * gw over the ROIs, valid samples of the batch) from the float32 grid arithmetic of include/veto_amd.h"""
    grid_sum = valid = 0
    for roi, lv in zip(rois, levels):
        sc, (_, _, Hm, Wm) = F(scales[lv]), shapes[lv]
        per_axis = []
        for lo, hi, size in ((roi[2], roi[4], Hm), (roi[1], roi[3], Wm)):
            start = F(lo * sc)
            ln = max(F(F(hi * sc) - start), F(1.0))
            bin_size = F(ln / F(P))
            g = ratio if ratio > 0 else int(np.ceil(F(ln / F(P))))
            i = np.arange(g, dtype=F)
            n = 0
            for p in range(P):
                v = (F(start + F(F(p) * bin_size)) + ((i + F(0.5)) * bin_size) / F(g)).astype(F)
                n += int((~((v < F(-1.0)) | (v > F(size)))).sum())
            per_axis.append((g, n))
        grid_sum += per_axis[0][0] * per_axis[1][0]
        valid += per_axis[0][1] * per_axis[1][1]
    return grid_sum, valid


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


rng = np.random.RandomState(7)
maps = [torch.randn(s, device=dev) for s in shapes]
boxes = [proposals(rng) for _ in range(B)]
clipped = np.concatenate([np.concatenate([np.full((N, 1), i, dtype=F), b], 1) for i, b in enumerate(boxes)])
far = clipped.copy()
far[:, 1:3] -= F(4000)
far[:, 3:5] += F(4000)

for name, rois_np in (("8 x 1000 clipped proposals", clipped), ("the same, +-4000 px on every side", far)):
    rois = torch.from_numpy(rois_np).to(dev)
    out = torch.empty((len(rois), C, P, P), device=dev)
    levels = torch.empty(len(rois), dtype=torch.int32, device=dev)
    gout = torch.randn((len(rois), C, P, P), device=dev)
    grads = [torch.zeros(s, device=dev) for s in shapes]
    ptrs = (ctypes.c_void_p * 4)(*[g.data_ptr() for g in grads])

    # the argument structs are built once, outside the timed windows: a window holds nothing but the C-ABI calls
    call = native.Launch(dev, "ROI pooling runs only on a HIP device")
    fargs = {r: poolers._pool_args(call, maps, scales, rois, B, P, r, None, out_rgb=out, out_levels=levels) for r in (0, 2)}
    bargs = {r: poolers._pool_args(call, shapes, scales, rois, B, P, r, None) for r in (0, 2)}
    stream = ctypes.c_void_p(call.stream.cuda_stream)
    gptr = ctypes.c_void_p(gout.data_ptr())

    def forward(ratio):
        native.check(getattr(call.lib, "veto_roi_pool_adaptive" if ratio == 0 else "veto_roi_pool")(stream, ctypes.byref(fargs[ratio])))

    def backward(ratio):
        entry = "veto_roi_pool_adaptive_backward" if ratio == 0 else "veto_roi_pool_backward"
        native.check(getattr(call.lib, entry)(stream, ctypes.byref(bargs[ratio]), gptr, None, ptrs, None))

    forward(0)
    torch.cuda.synchronize()
    lv = levels.cpu().numpy()
    counts = {r: sample_counts(rois_np, lv, r) for r in (0, 2)}
    print("%s: %d ROIs, levels %s" % (name, len(rois), np.bincount(lv, minlength=4).tolist()))
    for r in (0, 2):
        print("  ratio %d: mean gh * gw %.1f, valid samples %d of %d (counted on the host)"
              % (r, counts[r][0] / len(rois), counts[r][1], counts[r][0] * P * P))
    for what, fn in (("forward", forward), ("backward", backward)):
        times = {0: [], 2: []}
        for r in times:
            window(lambda: fn(r), 3)
        for _ in range(opt.rounds):
            for r in times:
                times[r].append(window(lambda: fn(r), opt.reps))
        for r, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            print("  %-8s ratio %d: median %.3f ms per call (spread %.3f .. %.3f, %d windows x %d calls, measured); %.3f ns per valid sample (derived)"
                  % (what, r, med, ts[0], ts[-1], opt.rounds, opt.reps, med * 1e6 / max(counts[r][1], 1)))
