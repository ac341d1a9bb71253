"""Relation evaluation over a whole split, two ways: SGGEvaluator.update() per batch + the host finalize() (read-back per batch,
fold in Python) against accumulate() per batch + the device finalize() (records resident, veto_sgg_eval_fold, one copy).

  python tools/sgg_eval_split_bench.py [--images 5000] [--fold-images 5000,26000] [--passes 3] [--way both|update|accumulate]
                                       [--tree DIR] [--out profiles/sgg_eval_split_bench.txt]
      (a) host clock per batch and of finalize(), each pass over the split ending in a synchronise;
      (b) device time (events around the C call) of veto_sgg_eval_fold at the given split sizes.
      --tree DIR imports veto_amd from another checkout (the parent commit, for its update() figures on the same box).
  rocprofv3 --memory-copy-trace --kernel-trace --output-format csv -d DIR -- python tools/sgg_eval_split_bench.py --copies
      three accumulate() calls and one finalize(), each phase fenced by an enumerate_pairs_kernel launch as a marker;
  python tools/sgg_eval_split_bench.py --summarise-trace DIR [--out FILE]
      (c) the device-to-host copies of that trace per phase, and the device time of the kernels it saw.

The batch is the one of tools/eval_bench.py: 12 images x 36 objects (1260 ranked pairs each), predcls, inputs on the device."""
import argparse
import csv
import ctypes
import glob
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=5000)
ap.add_argument("--fold-images", default="5000,26000")
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--way", default="both", choices=("both", "update", "accumulate"))
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--copies", action="store_true")
ap.add_argument("--summarise-trace", default=None)
opt = ap.parse_args()
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def flush_out():
    if opt.out:
        with open(opt.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


def summarise_trace(root):
    def rows(pattern):
        out = []
        for path in glob.glob(os.path.join(root, "**", pattern), recursive=True):
            out += list(csv.DictReader(open(path)))
        return out
    kernels, copies = rows("*kernel_trace.csv"), rows("*memory_copy_trace.csv")
    marks = sorted(int(r["Start_Timestamp"]) for r in kernels if "enumerate_pairs_kernel" in r["Kernel_Name"])
    assert len(marks) == 3, "expected the three marker launches of --copies, found %d" % len(marks)
    say("(c) device-to-host copies, rocprofv3 --memory-copy-trace --kernel-trace on `--copies` (3 x accumulate() of 12 images, then finalize()):")
    for name, lo, hi in (("first accumulate() .. before finalize()", marks[0], marks[1]), ("inside finalize()", marks[1], marks[2])):
        inside = [r for r in copies if lo <= int(r["Start_Timestamp"]) < hi]
        kinds = {}
        for r in inside:
            kinds[r["Direction"]] = kinds.get(r["Direction"], 0) + 1
        d2h = sum(n for k, n in kinds.items() if k.endswith("DEVICE_TO_HOST"))
        say("  %-42s device-to-host copies: %d   (all copies by direction: %s)" % (name, d2h, ", ".join("%s %d" % kv for kv in sorted(kinds.items())) or "none"))
    # small pageable copies may run as the runtime's blit kernel instead of a copy-engine transfer: then the kernel trace has them
    # and the copy trace does not.  A read-back of results can only follow the kernels that produce them, so each is shown in place.
    order = sorted(kernels, key=lambda r: int(r["Start_Timestamp"]))
    ours = ("sgg_eval_image_kernel", "sgg_eval_reduce_kernel", "sgg_eval_fold_chunk_kernel", "sgg_eval_fold_combine_kernel")
    for name, lo, hi in (("first accumulate() .. before finalize()", marks[0], marks[1]), ("inside finalize()", marks[1], marks[2])):
        seq = []
        for r in order:
            if lo < int(r["Start_Timestamp"]) < hi:
                hit = [k for k in ours if k in r["Kernel_Name"]]
                if hit:
                    seq.append(hit[0])
                elif "__amd_rocclr_copy" in r["Kernel_Name"] or "__amd_rocclr_fill" in r["Kernel_Name"]:
                    seq.append("[BLIT " + r["Kernel_Name"].strip('"') + "]")
        say("  %-42s blit-kernel copies: %d; in launch order among the evaluator's kernels: %s" %
            (name, sum(x.startswith("[BLIT") for x in seq), " > ".join(seq) or "none"))
    say("  device time of the kernels in that trace (us):")
    for key in ours:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in kernels if key in r["Kernel_Name"]]
        say("    %-30s %d launches: %s" % (key, len(us), " ".join("%.1f" % u for u in us)))


if opt.summarise_trace:
    summarise_trace(opt.summarise_trace)
    flush_out()
    sys.exit(0)

sys.path.insert(0, os.path.abspath(opt.tree))
import numpy as np
import torch
from veto_amd import native, synth
from veto_amd.evaluation import SGGEvaluator

dev = torch.device("cuda:0")
images, zeroshot = synth.synthetic_eval_images(77, [36] * 12, "predcls")
batch = [{k: torch.as_tensor(v).to(dev) for k, v in im.items()} for im in images]
n_batches = (opt.images + len(batch) - 1) // len(batch)
has_accumulate = hasattr(SGGEvaluator, "accumulate")


def marker():
    torch.cuda.synchronize()
    out = torch.empty((2, 2), dtype=torch.int64, device=dev)
    native.check(native.load_library().veto_enumerate_pairs(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), 2, ctypes.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()


if opt.copies:
    ev = SGGEvaluator("predcls", 51, zeroshot, device=dev)
    marker()
    for _ in range(3):
        ev.accumulate(batch)
    marker()
    res = ev.finalize()
    marker()
    print("copies run: %d images evaluated, R@100 %.4f" % (res["images_evaluated"], res["recall"][100]))
    sys.exit(0)


def one_pass(ev, feed):
    ev.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_batches):
        feed(batch)
    t1 = time.perf_counter()      # everything enqueued (update(): and read back)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = ev.finalize()
    t3 = time.perf_counter()
    return (t1 - t0) / n_batches * 1e3, (t2 - t0) / n_batches * 1e3, (t3 - t2) * 1e3, res


def fold_device_ms(ev, reps=7):
    """Events around veto_sgg_eval_fold alone, on the evaluator's resident records."""
    n_img, C = len(ev._img_g), ev.num_rel
    counts = np.zeros((2, n_img + 1), dtype=np.int64)
    np.cumsum(np.asarray(ev._img_g, dtype=np.int64), out=counts[0, 1:])
    counts[1, :n_img] = ev._img_p
    counts = torch.from_numpy(counts.astype(np.int32)).to(dev)
    n_m = 18 + 6 * (C - 1) + 2
    out = torch.empty(n_m + 12 * n_img, dtype=torch.float64, device=dev)
    call = native.Launch(dev, "needs a HIP device")
    a = call.args(native.VetoSggEvalFoldArgs, n_img=n_img, n_rel_cls=C, mode=0, n_gt_total=ev._rows, img_gt_offset=counts[0],
                  img_pair_count=counts[1], gt_predicate=ev._rec[4], gc_rank=ev._rec[0], ng_rank=ev._rec[1], acc_rank=ev._rec[2],
                  zeroshot_flag=ev._rec[3], metrics=out, per_image=out[n_m:])
    ws = call.workspace(call.lib.veto_sgg_eval_fold_workspace_bytes(n_img, C))
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call.run("veto_sgg_eval_fold", ctypes.byref(a), ws.data_ptr(), ws.numel())
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


say("sgg_eval_split_bench: tree %s; %d images as %d repeats of one 12 x 36-object predcls batch (%d GT relations), %d passes" %
    ("with accumulate()" if has_accumulate else "WITHOUT accumulate() (the parent commit)", n_batches * 12, n_batches,
     sum(len(im["gt_rels"]) for im in images), opt.passes))
ways = [w for w in ("update", "accumulate") if opt.way in ("both", w) and (w == "update" or has_accumulate)]
results = {}
for way in ways:
    ev = SGGEvaluator("predcls", 51, zeroshot, device=dev)
    feed = ev.update if way == "update" else ev.accumulate
    for _ in range(5):
        feed(batch)      # warm: the batch shape's offsets, the workspace, the first buffers
    say("(a) %s() per batch, then finalize() [%s]" % (way, "read-back per batch, host fold" if way == "update" else "resident records, device fold, one copy"))
    say("    pass | enqueue per batch (ms) | per batch incl. final synchronise (ms) | finalize (ms)")
    rows = []
    for p in range(opt.passes):
        enq, per, fin, res = one_pass(ev, feed)
        rows.append((enq, per, fin))
        say("    %4d | %10.4f | %10.4f | %10.3f" % (p, enq, per, fin))
    med = [float(np.median([r[i] for r in rows])) for i in range(3)]
    say("  median | %10.4f | %10.4f | %10.3f     -> split total %.1f ms" % (med[0], med[1], med[2], med[1] * n_batches + med[2]))
    results[way] = res
if len(results) == 2:
    a, b = results["update"], results["accumulate"]
    worst = max(abs(a[n][k] - b[n][k]) for n in ("recall", "recall_nogc", "zeroshot_recall", "accuracy", "mean_recall", "ng_mean_recall") for k in (20, 50, 100))
    say("    the two ways agree within %.1e on the eighteen split-level numbers; %d images evaluated" % (worst, b["images_evaluated"]))

if has_accumulate and opt.way in ("both", "accumulate"):
    say("(b) device time of veto_sgg_eval_fold (events around the C call: both launches), first call then 7:")
    ev = SGGEvaluator("predcls", 51, zeroshot, device=dev)
    ev.accumulate(batch)
    one = {k: v for k, v in ev.state().items()}
    per_chunk = ctypes.c_int32()
    native.check(native.load_library().veto_sgg_eval_fold_limits(ctypes.byref(per_chunk), None))
    for n in [int(x) for x in opt.fold_images.split(",") if x]:
        reps = (n + 11) // 12
        big = {k: v.repeat(reps) for k, v in one.items()}
        ev.load_state([big])
        ms = fold_device_ms(ev)
        say("    %6d images, %8d GT relations, %4d chunks: %s ms   (median of the 7: %.4f ms)" %
            (reps * 12, ev._rows, (reps * 12 + per_chunk.value - 1) // per_chunk.value, " ".join("%.4f" % m for m in ms), float(np.median(ms[1:]))))
flush_out()
