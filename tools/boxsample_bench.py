"""Latency of the box head's training-time sampler on the device (veto_amd.boxsampling.FastRCNNSampling) against the reference's
per-image algorithm in plain torch on the same device tensors, on 12 images x (1000 proposals + 25 appended GT boxes) with 25 GT
boxes each, at FG / BG thresholds 0.5 / 0.3 and BATCH_SIZE_PER_IMAGE 256 / POSITIVE_FRACTION 0.25 (the reference's defaults).

  device assign      assign_label_to_proposals: one veto_box_match launch, no device->host copy
  device subsample   subsample: veto_box_match + veto_box_subsample, one read-back of the counts, one gather per field
  host assign        per image: the boxlist_iou matrix, max over the GT boxes, the two threshold masks, clamp, gather, masked write
  host subsample     per image: the same plus BoxCoder.encode, two nonzero, two randperm, two masks, nonzero and the field gathers

The two sides are timed in the same process in alternating rounds of `--reps` calls, each round ending in a synchronise (the calls
that read back block by themselves); the report is the median round of each and their ratio.  The launches and device->host
copies of one device call are counted with the torch profiler, after the timing.  --kernels-only makes a few device calls and
nothing else, for a kernel trace.  Prints one JSON line per setting.
Usage: python tools/boxsample_bench.py [--reps 20] [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import boxsampling as bs  # noqa: E402
from veto_amd import synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

HIGH, LOW, BATCH, FRACTION, WEIGHTS = 0.5, 0.3, 256, 0.25, (10., 10., 5., 5.)
N_IMG, N_DET, N_GT = 12, 1000, 25


def batch(dev):
    props, targets = [], []
    for i in range(N_IMG):
        d = synth.synthetic_box_sampling_image(900 + i, N_GT, N_DET)
        props.append(BoxList(torch.from_numpy(d["prp_boxes"]).to(dev), d["image_size"], "xyxy"))
        t = BoxList(torch.from_numpy(d["tgt_boxes"]).to(dev), d["image_size"], "xyxy")
        t.add_field("labels", torch.from_numpy(d["tgt_labels"]).to(dev))
        targets.append(t)
    return props, targets


def fresh(props):
    return [BoxList(p.bbox, p.size, p.mode) for p in props]


def host_match(p, t):
    """One image of the reference's matching in torch: (matched_idxs, the matched boxes' labels)."""
    a, b = t.bbox, p.bbox
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2]) + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    vals, matched = (inter / (area_a[:, None] + area_b - inter)).max(dim=0)
    below, between = vals < LOW, (vals >= LOW) & (vals < HIGH)
    matched[below] = -1
    matched[between] = -2
    return matched, t.get_field("labels")[matched.clamp(min=0)].to(torch.int64)


def host_assign(props, targets):
    for p, t in zip(props, targets):
        matched, labels = host_match(p, t)
        labels[matched < 0] = 0
        p.add_field("labels", labels)
    return props


def host_subsample(props, targets):
    out = []
    for p, t in zip(props, targets):
        matched, labels = host_match(p, t)
        labels[matched == -1] = 0
        labels[matched == -2] = -1
        g, b = t.bbox[matched.clamp(min=0)], p.bbox
        ew, eh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
        gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
        reg = torch.stack([WEIGHTS[0] * (g[:, 0] + 0.5 * gw - b[:, 0] - 0.5 * ew) / ew, WEIGHTS[1] * (g[:, 1] + 0.5 * gh - b[:, 1] - 0.5 * eh) / eh,
                           WEIGHTS[2] * torch.log(gw / ew), WEIGHTS[3] * torch.log(gh / eh)], 1)
        pos, neg = torch.nonzero(labels >= 1).squeeze(1), torch.nonzero(labels == 0).squeeze(1)
        num_pos = min(pos.numel(), int(BATCH * FRACTION))
        num_neg = min(neg.numel(), BATCH - num_pos)
        mask = torch.zeros_like(labels, dtype=torch.bool)
        mask[pos[torch.randperm(pos.numel(), device=pos.device)[:num_pos]]] = True
        mask[neg[torch.randperm(neg.numel(), device=neg.device)[:num_neg]]] = True
        inds = torch.nonzero(mask).squeeze(1)
        q = BoxList(b[inds], p.size, p.mode)
        for k, v in (("labels", labels), ("regression_targets", reg), ("matched_idxs", matched)):
            q.add_field(k, v[inds])
        out.append(q)
    return out


def profile_call(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    on_device = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA]
    ours = sum(1 for n in on_device if "box_match" in n or "box_subsample" in n)
    d2h = sum(1 for e in ev if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    return ours, len([n for n in on_device if "Memcpy" not in n and "Memset" not in n]), d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boxsample_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    props, targets = batch(dev)
    s = bs.FastRCNNSampling(bs.Matcher(HIGH, LOW), bs.BalancedPositiveNegativeSampler(BATCH, FRACTION), bs.BoxCoder(WEIGHTS))
    calls = {"device_assign": lambda: s.assign_label_to_proposals(fresh(props), targets),
             "host_assign": lambda: host_assign(fresh(props), targets),
             "device_subsample": lambda: s.subsample(fresh(props), targets, seed=1),
             "host_subsample": lambda: host_subsample(fresh(props), targets)}
    if args.kernels_only:
        for _ in range(5):
            calls["device_assign"]()
            calls["device_subsample"]()
        torch.cuda.synchronize()
        return
    lines = []
    for _ in range(3):          # warm-up: code objects, allocator, the cached offsets
        got = {name: call() for name, call in calls.items()}
    torch.cuda.synchronize()
    same = all(torch.equal(a.get_field("labels"), b.get_field("labels")) for a, b in zip(got["device_assign"], got["host_assign"]))
    rows = {name: [len(q) for q in got[name]] for name in ("device_subsample", "host_subsample")}
    lines.append(json.dumps({"setting": "agreement", "assign_labels_equal": same, "device_subsample_rows": rows["device_subsample"],
                             "host_subsample_rows": rows["host_subsample"]}))
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.reps)
    med = {name: statistics.median(t) for name, t in times.items()}
    for name in calls:
        out = {"setting": name, "images": N_IMG, "proposals_per_image": N_DET + N_GT, "gt_boxes": N_GT, "batch_size_per_image": BATCH,
               "positive_fraction": FRACTION, "ms_per_call": round(med[name], 4), "ms_min": round(min(times[name]), 4),
               "ms_max": round(max(times[name]), 4), "rounds": args.rounds, "reps": args.reps}
        ours, kernels, d2h = profile_call(calls[name])
        out.update(kernel_launches=kernels, device_to_host_copies=d2h)
        if name.startswith("device"):
            out.update(veto_launches=ours)
        lines.append(json.dumps(out))
    lines.append(json.dumps({"setting": "ratio", "host_over_device_assign": round(med["host_assign"] / med["device_assign"], 2),
                             "host_over_device_subsample": round(med["host_subsample"] / med["device_subsample"], 2)}))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
