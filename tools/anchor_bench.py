"""The RPN's anchor generator on VETO's geometry: images padded to 800 x 1344, five levels (200 x 336, 100 x 168, 50 x 84, 25 x 42,
13 x 21), four aspect ratios (A = 4, 358 092 anchors per image), for 12 images and for 1.  Three arrangements in one process:

  torch   the reference's arrangement (pysgg/modeling/rpn/anchor_generator.py:73-125) restated here in torch on the device: per level
          two arange, a meshgrid, two reshapes, a stack, a broadcast add and a reshape; per (image, level) four comparisons and
          three `&`
  miss    veto_amd.rpn.AnchorGenerator.forward with an empty cache: anchors and visibility, one launch
  hit     the same with the grid shape cached: the visibility plane only, one launch

Timing (default): the three alternate call by call inside a round, `--rounds` rounds of `--calls` calls; each call starts on an idle
device, `host` is the time until the call returns (the enqueue), `wall` until the device is idle again.  Reported: the median round
(a round = the mean of its calls) with the smallest and largest round.  No speed-up is asserted.

Launch counts: `--trace` runs `--calls` calls of each arrangement and nothing else that launches a kernel; run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/anchor_bench.py --trace --images N`, then `--summarise DIR --images N`
counts the dispatches of the run per arrangement (the device module's two kernel instances are told from ATen's by name).
Every mode appends JSON lines to --out when given.
Usage: python tools/anchor_bench.py [--images 12] [--rounds 9] [--calls 20] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd.config import default_config  # noqa: E402
from veto_amd.rpn import make_anchor_generator  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

GRIDS = ((200, 336), (100, 168), (50, 84), (25, 42), (13, 21))
PADDED = (800, 1344)      # (height, width)


def reference_forward(cells, strides, straddle_thresh, image_sizes, grid_sizes):
    """The launch pattern of the reference's AnchorGenerator.forward, written out here: the grid of every level from arange /
    meshgrid / stack / add, then per image and level a BoxList whose visibility is four comparisons joined by three `&`."""
    per_level = []
    for (gh, gw), stride, cell in zip(grid_sizes, strides, cells):
        xs = torch.arange(0, gw * stride, step=stride, dtype=torch.float32, device=cell.device)
        ys = torch.arange(0, gh * stride, step=stride, dtype=torch.float32, device=cell.device)
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        xx, yy = xx.reshape(-1), yy.reshape(-1)
        shifts = torch.stack((xx, yy, xx, yy), dim=1)
        per_level.append((shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4))
    out = []
    for height, width in image_sizes:
        lists = []
        for a in per_level:
            b = BoxList(a, (width, height), mode="xyxy")
            if straddle_thresh >= 0:
                vis = ((a[..., 0] >= -straddle_thresh) & (a[..., 1] >= -straddle_thresh) & (a[..., 2] < width + straddle_thresh)
                       & (a[..., 3] < height + straddle_thresh))
            else:
                vis = torch.ones(a.shape[0], dtype=torch.uint8, device=a.device)
            b.add_field("visibility", vis)
            lists.append(b)
        out.append(lists)
    return out


def arrangements(n_img, dev):
    gen = make_anchor_generator(default_config()).to(dev)
    cells = list(gen.cell_anchors)      # (shared with the module, read only: a clone would be a kernel in the trace)
    images = types.SimpleNamespace(image_sizes=[(PADDED[0] - 8 * i, PADDED[1] - 16 * i) for i in range(n_img)])
    maps = [torch.empty((n_img, 1, h, w), device=dev) for h, w in GRIDS]

    def miss():
        gen._cache.clear()
        return gen(images, maps)

    return {"torch": lambda: reference_forward(cells, gen.strides, gen.straddle_thresh, images.image_sizes, GRIDS),
            "miss": miss, "hit": lambda: gen(images, maps)}, gen


def check(arr):
    """The three arrangements return the same bits."""
    want = arr["torch"]()
    for name in ("miss", "hit"):
        got = arr[name]()
        for per_w, per_g in zip(want, got):
            for w, g in zip(per_w, per_g):
                assert torch.equal(w.bbox, g.bbox) and torch.equal(w.get_field("visibility"), g.get_field("visibility")), name
                assert w.size == g.size and w.get_field("visibility").dtype == g.get_field("visibility").dtype


def timed(arr, rounds, calls):
    per = {name: {"host": [], "wall": []} for name in arr}
    for _ in range(rounds):
        acc = {name: [0.0, 0.0] for name in arr}
        for _ in range(calls):
            for name, fn in arr.items():      # interleaved: the three see the same machine state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                del out
                acc[name][0] += t1 - t0
                acc[name][1] += t2 - t0
        for name in arr:
            per[name]["host"].append(acc[name][0] / calls * 1e3)
            per[name]["wall"].append(acc[name][1] / calls * 1e3)
    return per


def summarise(directory, n_img, calls):
    """Dispatches per call from the run's *kernel_stats.csv (Name, Calls; what --stats writes), else from its *kernel_trace.csv.  The
    runtime's own copy kernels (__amd_rocclr_*: the set-up's host->device copies) belong to no arrangement and are listed apart."""
    counts = {}
    stats = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    for path in stats or glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("Kernel_Name") or ""
                counts[name] = counts.get(name, 0) + (int(r["Calls"]) if stats else 1)
    if not counts:
        raise SystemExit("no kernel statistics or trace under %s" % directory)
    miss = sum(n for k, n in counts.items() if "anchor_grid_kernel<true>" in k)
    hit = sum(n for k, n in counts.items() if "anchor_grid_kernel<false>" in k)
    runtime = sum(n for k, n in counts.items() if k.startswith("__amd_rocclr_"))
    other = {k: n for k, n in counts.items() if "anchor_grid_kernel" not in k and not k.startswith("__amd_rocclr_")}
    return {"setting": "%d images, launches per call (rocprofv3 --kernel-trace --stats, %d calls of each arrangement)" % (n_img, calls),
            "torch": sum(other.values()) / calls, "miss": miss / calls, "hit": hit / calls, "dispatches_in_run": sum(counts.values()),
            "runtime_copy_kernels_in_run": runtime, "torch_distinct_kernels": len(other)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.summarise:
        lines.append(summarise(args.summarise, args.images, args.calls))
    else:
        dev = torch.device("cuda:0")
        arr, gen = arrangements(args.images, dev)
        if args.trace:      # nothing here but the calls launches a kernel (the set-up above is allocations and host->device copies)
            for name in ("torch", "miss", "hit"):
                for _ in range(args.calls):
                    arr[name]()
            torch.cuda.synchronize()
            return
        check(arr)
        timed(arr, 1, 5)      # warm-up
        per = timed(arr, args.rounds, args.calls)
        total = sum(a * h * w for a, (h, w) in zip(gen.num_anchors_per_location(), GRIDS))
        for name in arr:
            lines.append({"setting": "%d images %s" % (args.images, name), "anchors_per_image": total,
                          "wall_ms_per_call": round(statistics.median(per[name]["wall"]), 4),
                          "host_ms_per_call": round(statistics.median(per[name]["host"]), 4),
                          "wall_ms_min_max": [round(min(per[name]["wall"]), 4), round(max(per[name]["wall"]), 4)],
                          "host_ms_min_max": [round(min(per[name]["host"]), 4), round(max(per[name]["host"]), 4)],
                          "rounds": args.rounds, "calls": args.calls})
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
