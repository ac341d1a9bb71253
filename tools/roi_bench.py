"""Times the fused ROI pooling launch (veto_roi_pool: 4 FPN levels + depth map -> two [N, 256, 8, 8] tensors)
at the BASELINE cfg-2 batch shape: 12 images (608 x 1024 after padding) x 36 boxes.  Prints ms per launch and
the write-side bandwidth (the 2 x N x 256 x 64 x 4 output bytes are the algorithmic minimum; the reads are the
ROIs' footprints of the maps, at most that much again for 8x8 outputs with 2x2 samples).

With --layout / --dtype the maps are built in that form and two paths are timed against each other in this process,
alternating, `--rounds` windows of `--reps` calls each: the form read IN PLACE, and COPY-THEN-POOL -- `.float().contiguous()`
of every map followed by the float32 NCHW call, which is what the pooler did for such maps before it read them in place.
Prints per path the median window and the spread (min .. max) over the windows, and whether the outputs are bit-equal.
usage: tools/roi_bench.py [--layout nchw|nhwc] [--dtype float32|float16|bfloat16] [--rounds 7] [--reps 20]"""
import argparse
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from veto_amd import poolers, synth, testing
from veto_amd.poolers import make_roi_box_feature_extractor
from veto_amd.structures import BoxList

ap = argparse.ArgumentParser()
ap.add_argument("--layout", choices=["nchw", "nhwc"], default=None)
ap.add_argument("--dtype", choices=["float32", "float16", "bfloat16"], default=None)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
opt = ap.parse_args()

dev = torch.device("cuda:0")
n_img, n_obj, W, H = 12, 36, 1024, 608
torch.manual_seed(0)
feats = [torch.randn(n_img, 256, H >> (2 + l), W >> (2 + l), device=dev) for l in range(4)]
depth = torch.randn(n_img, 256, H >> 4, W >> 4, device=dev)
batch = synth.synthetic_batch(7, n_img, n_obj)
boxes = torch.from_numpy(batch["boxes"]).to(dev)
boxes[:, 2:] = torch.minimum(boxes[:, 2:] * 1.6, torch.tensor([W - 1.0, H - 1.0], device=dev))
props = [BoxList(boxes[i * n_obj:(i + 1) * n_obj], (W, H)) for i in range(n_img)]
ext = make_roi_box_feature_extractor(testing.make_config(4, 8), 256, for_relation=True)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


if opt.layout is None and opt.dtype is None:
    for _ in range(3):
        x2d, d2d, _, _ = ext(feats, props, depth_features=depth)
    torch.cuda.synchronize()
    ms, (x2d, d2d, _, _) = window(lambda: ext(feats, props, depth_features=depth), 50)
    out_bytes = 2 * x2d.numel() * 4
    print("roi_pool: %d ROIs x 2 maps, %.4f ms per call (host enqueue included), output %.1f MB -> %.0f GB/s written" %
          (n_img * n_obj, ms, out_bytes / 1e6, out_bytes / (ms * 1e-3) / 1e9))
    sys.exit(0)

dtype = getattr(torch, opt.dtype or "float32")
fmt = torch.channels_last if opt.layout == "nhwc" else torch.contiguous_format
maps = [m.to(dtype).contiguous(memory_format=fmt) for m in feats + [depth]]
del feats, depth
form = poolers._map_form(maps[:4])
assert form is not None and form == poolers._map_form(maps[4:])
rois = ext.pooler.convert_to_roi_format(props)
scales = ext.pooler.scales
poolers.IN_PLACE["forward"].add(form)      # time the in-place kernels whatever the dispatch table says


def in_place():
    return poolers._roi_pool(maps[:4], scales, rois, n_img, 8, 2, depth=maps[4])


def copy_then_pool():
    return poolers._roi_pool([m.float().contiguous() for m in maps[:4]], scales, rois, n_img, 8, 2, depth=maps[4].float().contiguous())


paths = {"in place": in_place, "copy then pool": copy_then_pool}
times = {k: [] for k in paths}
outs = {}
for fn in paths.values():
    window(fn, 3)
for _ in range(opt.rounds):
    for name, fn in paths.items():
        ms, outs[name] = window(fn, opt.reps)
        times[name].append(ms)
same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["in place"][:2], outs["copy then pool"][:2]))
map_elems = sum(m.numel() for m in maps)
print("roi_pool forward %s %s: %d ROIs, %d map elements (%.0f MB as stored, %.0f MB as a float32 copy), %d windows x %d calls, outputs bit-equal: %s"
      % (opt.layout or "nchw", opt.dtype or "float32", len(rois), map_elems, map_elems * maps[0].element_size() / 1e6, map_elems * 4 / 1e6,
         opt.rounds, opt.reps, same))
for name, ts in times.items():
    ts = sorted(ts)
    print("  %-15s median %.4f ms per call   spread %.4f .. %.4f ms" % (name, ts[len(ts) // 2], ts[0], ts[-1]))
