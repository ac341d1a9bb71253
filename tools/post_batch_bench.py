"""MEET post-processing of a whole batch in one call (veto_postprocess_groups_batch) against the loop of one-image calls
(the same entry point with n_img = 1) on the same inputs: 12 images x 36 objects (1 260 pairs each, 15 120 pairs), VG
(5 groups, 51 classes) and GQA (4 groups, 101 classes), the merge and both votes, through veto_amd.postprocess.PostProcessor.
One more setting, vg_vanilla, times the vanilla branch (one [15 120, 51] logit matrix) on the same 12 images, the batch call only.

  batch   one PostProcessor call on the 12 images: at most 4 launches, the vote reads kept_count[12] back once
  loop    12 PostProcessor calls on one image each, on slices of the same tensors: 12 x 4 launches, the vote reads back 12 x

Both forms are timed in the same process, alternating, after a warm-up; per repetition the device time is taken with device events
around the call(s) and the host time with a host clock from the call to its return on an idle stream.  The report is the median
of `--reps` repetitions of each and their ratio, one JSON line per setting, after a line that says whether the two forms gave
equal results.  --kernels-only FORM makes `--reps` calls of one form on one setting and nothing else, for a kernel trace.
Usage: python tools/post_batch_bench.py [--reps 30] [--out FILE] [--kernels-only batch|loop --setting vg_merge]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import meet_tables, testing  # noqa: E402
from veto_amd.postprocess import PostProcessor  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

N_IMG, N_OBJ = 12, 36
DATASETS = {"vg": ([4, 6, 9, 19, 12], 151), "gqa": ([5, 10, 20, 65], 201)}      # MEET group sizes (divide4 / divide4 of GQA), object classes
SETTINGS = [d + "_" + m for d in DATASETS for m in ("merge", "vote_C", "vote_U")] + ["vg_vanilla"]


def build(setting, dev):
    dataset, mode = setting.split("_", 1)
    groups, n_objc = DATASETS[dataset]
    incre = meet_tables.incre_idx_list(groups)
    P = N_OBJ * (N_OBJ - 1)
    gen = torch.Generator(device="cpu").manual_seed(7)
    idx = torch.arange(N_OBJ)
    pairs = torch.stack(torch.meshgrid(idx, idx, indexing="ij"), -1).reshape(-1, 2)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]].contiguous().to(dev)
    rel = {}
    for k, g in enumerate(groups if mode != "vanilla" else []):
        if mode == "merge":
            rel["group_%d" % k] = (2.0 * torch.randn(N_IMG * P, g + 2, generator=gen)).to(dev)
        else:       # three experts that share a part, so that they often agree
            base = 1.5 * torch.randn(N_IMG * P, g + 2, generator=gen)
            for e in range(3):
                rel["group_%d%d" % (k, e + 1)] = (base + torch.randn(N_IMG * P, g + 2, generator=gen)).to(dev)
    obj = (3.0 * torch.randn(N_IMG * N_OBJ, n_objc, generator=gen)).to(dev)
    cfg = None
    if mode.startswith("vote"):
        cfg = testing.make_config(1, 8, meet=True, dataset="VG")
        cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = True
        cfg.ENSEMBLE_LEARNING.VOTING = mode[-1]
    post = PostProcessor(False, use_gt_box=True, cfg=cfg)
    boxes = [BoxList(torch.zeros(N_OBJ, 4), (800, 600)).to(dev) for _ in range(N_IMG)]
    objs, pair_lists = list(obj.split(N_OBJ)), [pairs] * N_IMG
    if mode == "vanilla":
        logits = list((2.0 * torch.randn(N_IMG * P, len(incre), generator=gen)).to(dev).split(P))

        def vanilla():
            res = post((logits, objs), pair_lists, boxes)
            return res, post.last_triple_scores

        return {"batch": vanilla}, 1
    slices = [{k: v[i * P:(i + 1) * P] for k, v in rel.items()} for i in range(N_IMG)]

    def batch():
        res = post((rel, objs), pair_lists, boxes, incre_idx_list=incre, ensemble=True)
        return res, post.last_triple_scores

    def loop():
        res, triples = [], []
        for i in range(N_IMG):
            res += post((slices[i], [objs[i]]), [pairs], [boxes[i]], incre_idx_list=incre, ensemble=True)
            triples += post.last_triple_scores
        return res, triples

    return {"batch": batch, "loop": loop}, len(groups)


def snapshot(out):
    res, triples = out
    keys = ("rel_pair_idxs", "pred_rel_scores", "pred_rel_labels", "pred_labels", "pred_scores")
    return [[r.get_field(k).clone() for k in keys] + [t.clone()] for r, t in zip(res, triples)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--kernels-only", choices=["batch", "loop"], default=None)
    ap.add_argument("--setting", choices=SETTINGS, default="vg_merge")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("post_batch_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    if args.kernels_only:
        calls, _ = build(args.setting, dev)
        for _ in range(args.reps):
            calls[args.kernels_only]()
        torch.cuda.synchronize()
        return
    if args.reps < 20:
        raise SystemExit("at least 20 timed repetitions")
    lines = []
    for setting in SETTINGS:
        calls, K = build(setting, dev)
        for _ in range(3):          # warm-up: code objects, allocator, workspace, the cached offsets
            got = {name: snapshot(call()) for name, call in calls.items()}
        torch.cuda.synchronize()
        equal = all(torch.equal(x, y) for a, b in zip(got["batch"], got.get("loop", got["batch"])) for x, y in zip(a, b))
        rows = [int(a[-1].shape[0]) for a in got["batch"]]
        dev_ms, host_ms = {n: [] for n in calls}, {n: [] for n in calls}
        for _ in range(args.reps):
            for name, call in calls.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                start.record()
                call()
                stop.record()
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                dev_ms[name].append(start.elapsed_time(stop))
        med = lambda xs: round(statistics.median(xs), 4)
        out = {"setting": setting, "images": N_IMG, "objects_per_image": N_OBJ, "groups": K, "rows": sum(rows), "rows_min": min(rows),
               "rows_max": max(rows), "batch_equals_loop": equal, "reps": args.reps}
        for name in calls:
            out.update({name + "_device_ms": med(dev_ms[name]), name + "_device_ms_min": round(min(dev_ms[name]), 4),
                        name + "_device_ms_max": round(max(dev_ms[name]), 4), name + "_host_ms": med(host_ms[name])})
        if "loop" in calls:
            out.update(loop_over_batch_device=round(out["loop_device_ms"] / out["batch_device_ms"], 2),
                       loop_over_batch_host=round(out["loop_host_ms"] / out["batch_host_ms"], 2))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
