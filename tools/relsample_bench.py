"""Latency of the sgdet training sampler: DetectRelationSampler.detect_relsample (one veto_detect_relsample launch and one
read-back of the per-image counts) on 12 images x 80 detections with 25 GT boxes and 20 relations each, at
BATCH_SIZE_PER_IMAGE 1024 / POSITIVE_FRACTION 0.25 (VETO_final.yaml), with and without REQUIRE_BOX_OVERLAP.
Reports ms per call (wall time over `--reps` calls; each call ends in its blocking read-back), the kernel launches and
device->host copies of one call (torch profiler).  When the reference code base is importable (pysgg on sys.path, or
--reference DIR), also times its RelationSampling.detect_relsample on CPU tensors, labelled as a CPU number; otherwise that
leg is reported as skipped.  Prints one JSON line per setting.  Usage: python tools/relsample_bench.py [--reps 50]

--gtbox times the GT-box training sampler instead (predcls / sgcls): GTBoxRelationSampler.gtbox_relsample (one
veto_gtbox_relsample launch and one read-back) against the stand-in host sampler of tests/relation_sampling.py (the reference's
per-image loop of ATen calls, on the same device tensors) on 12 images of 36 objects at 1024 / 0.25.  The two are timed in the
same process in alternating rounds of `--reps` calls, each round ending in a synchronise; the report is the median round of
each, their ratio, and the device sampler's launches and device->host copies."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import synth  # noqa: E402
from veto_amd.sampling import DetectRelationSampler  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402


def batch(dev, box_cls=BoxList):
    props, targets = [], []
    for i in range(12):
        d = synth.synthetic_relsample_image(900 + i, 25, 80, 20)
        p = box_cls(torch.from_numpy(d["prp_boxes"]).to(dev), d["image_size"], mode="xyxy")
        p.add_field("labels", torch.from_numpy(d["prp_labels"]).to(dev))
        p.add_field("pred_scores", torch.from_numpy(d["pred_scores"]).to(dev))
        t = box_cls(torch.from_numpy(d["tgt_boxes"]).to(dev), d["image_size"], mode="xyxy")
        t.add_field("labels", torch.from_numpy(d["tgt_labels"]).to(dev))
        t.add_field("relation", torch.from_numpy(d["relation"]).to(dev))
        props.append(p)
        targets.append(t)
    return props, targets


def profile_call(fn, kernel="detect_relsample"):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    kernels = sum(1 for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and kernel in e.name)
    d2h = sum(1 for e in ev if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    return kernels, d2h


def reference_sampler(reference):
    """The reference's RelationSampling class, or None when it cannot be imported here."""
    try:
        if reference:
            here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            sys.path.insert(0, os.path.join(here, "tests", "golden"))
            from make_golden import REF, import_reference   # stubs for the reference's optional imports
            if os.path.abspath(reference) != os.path.abspath(REF):
                sys.path.insert(0, reference)
            _, _, box_cls = import_reference()
        else:
            from pysgg.structures.bounding_box import BoxList as box_cls
        from pysgg.modeling.roi_heads.relation_head.sampling import RelationSampling
        return RelationSampling, box_cls
    except Exception as e:   # absent on this machine: the CPU leg is skipped
        return None, repr(e)


def reference_leg(reference, reps):
    RelationSampling, box_cls = reference_sampler(reference)
    if RelationSampling is None:
        print(json.dumps({"setting": "reference_cpu", "skipped": "reference not importable: %s" % box_cls}), flush=True)
        return
    import numpy as np
    cpu_props, cpu_targets = batch(torch.device("cpu"), box_cls)
    for overlap in (False, True):
        ref = RelationSampling(0.5, overlap, 4, 1024, 0.25, 2048, False, False)
        np.random.seed(0)
        torch.manual_seed(0)
        t0 = time.perf_counter()
        for _ in range(reps):
            ref.detect_relsample(cpu_props, cpu_targets)
        ms = (time.perf_counter() - t0) * 1e3 / reps
        print(json.dumps({"setting": "reference_cpu", "require_overlap": overlap, "device": "cpu", "images": 12,
                          "ms_per_call": round(ms, 3)}), flush=True)


def gtbox_batch(dev, n_img=12, n_obj=36):
    props, targets = [], []
    for boxes, rel in synth.synthetic_relation_targets(seed=77, num_objs=(n_obj,) * n_img):
        props.append(BoxList(torch.from_numpy(boxes).to(dev), (800, 600), mode="xyxy"))
        t = BoxList(torch.from_numpy(boxes.copy()).to(dev), (800, 600), mode="xyxy")
        t.add_field("relation", torch.from_numpy(rel).to(dev))
        targets.append(t)
    return props, targets


def gtbox_leg(reps, rounds=9):
    import statistics
    from veto_amd.sampling import GTBoxRelationSampler
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from relation_sampling import RelationSampling as HostSampling
    if not torch.cuda.is_available():
        raise SystemExit("relsample_bench --gtbox needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    props, targets = gtbox_batch(dev)
    device = GTBoxRelationSampler(1024, 0.25)
    host = HostSampling(0.5, False, 4, 1024, 0.25, 2048, True, False)
    calls = {"device_sampler": lambda: device.gtbox_relsample(props, targets, seed=1),
             "host_sampler": lambda: host.gtbox_relsample(props, targets)}
    rows = {}
    for name, call in calls.items():          # warm-up: code objects, allocator, the cached offsets
        for _ in range(5):
            _, labels, pairs, _ = call()
        torch.cuda.synchronize()
        rows[name] = (sum(len(p) for p in pairs), int(sum(int((l > 0).sum()) for l in labels)))
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()                        # the device sampler ends in its blocking read-back, the host one in nonzero's
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    kernels, d2h = profile_call(calls["device_sampler"], "gtbox_relsample")
    med = {name: statistics.median(t) for name, t in times.items()}
    for name in calls:
        out = {"setting": "gtbox_" + name, "images": 12, "objects": 36, "batch_size_per_image": 1024, "positive_fraction": 0.25,
               "ms_per_call": round(med[name], 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
               "rounds": rounds, "reps": reps, "rows": rows[name][0], "fg_rows": rows[name][1]}
        if name == "device_sampler":
            out.update(kernel_launches=kernels, device_to_host_copies=d2h)
        print(json.dumps(out), flush=True)
    print(json.dumps({"setting": "gtbox_ratio", "host_over_device": round(med["host_sampler"] / med["device_sampler"], 2),
                      "device_share_of_62ms_step": round(med["device_sampler"] / 62.0, 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--gtbox", action="store_true", help="time the GT-box sampler against the stand-in host sampler")
    ap.add_argument("--reference", default="", help="directory of the reference checkout (for the CPU comparison)")
    args = ap.parse_args()
    if args.gtbox:
        gtbox_leg(args.reps)
        return
    reference_leg(args.reference, max(1, args.reps // 10))
    if not torch.cuda.is_available():
        print(json.dumps({"setting": "device_sampler", "skipped": "no HIP device"}), flush=True)
        return
    dev = torch.device("cuda")
    props, targets = batch(dev)
    for overlap in (False, True):
        s = DetectRelationSampler(0.5, overlap, 4, 1024, 0.25)
        call = lambda: s.detect_relsample(props, targets, seed=1)   # noqa: E731
        call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            _, labels, _, pairs, _ = call()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.reps
        kernels, d2h = profile_call(call)
        print(json.dumps({"setting": "device_sampler", "require_overlap": overlap, "images": 12, "detections": 80,
                          "gt_boxes": 25, "relations": 20, "batch_size_per_image": 1024, "positive_fraction": 0.25,
                          "ms_per_call": round(ms, 4), "kernel_launches": kernels, "device_to_host_copies": d2h,
                          "rows": sum(len(p) for p in pairs), "fg_rows": int(sum(int((l > 0).sum()) for l in labels))}),
              flush=True)


if __name__ == "__main__":
    main()
