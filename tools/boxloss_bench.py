"""Latency of the box head's loss on the device (veto_amd.boxloss.FastRCNNLossComputation: one veto_box_loss call, then the
backward that scales its gradients) against the reference's algorithm restated in plain torch on the same device tensors, forward
and backward: 12 images x 512 sampled rows x 151 classes, class-specific regression ([6144, 604]), a quarter of the rows positive.

  device   both losses and both gradients in two launches; backward = one multiply per input
  host     loss.py:57-84: the concatenation of the per-image fields, F.cross_entropy, a nonzero over labels > 0 (its count is read
           back), the advanced-index gather of [P, 4] out of [R, 4C], smooth-L1 with beta 1, and autograd's backward through the
           gather (a scatter into a zero-filled [R, 4C])

The two sides are timed in the same process in alternating rounds of `--reps` calls (500: some 60 ms per round on the device
side), each round ending in a synchronise; the report is the median round of each and their ratio.  The times are host wall-clock
per call: they include the Python side of a call, not kernel time alone.  The launches and the memcpy calls (of any direction: every read-back is one) of one call of each are
counted with the torch profiler, after the timing.  Prints one JSON line per setting.
Usage: python tools/boxloss_bench.py [--reps 500] [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import boxloss as bl  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

N_IMG, ROWS, N_CLS, POSITIVE = 12, 512, 151, 0.25


def batch(dev):
    gen = torch.Generator(device="cpu").manual_seed(78)
    R = N_IMG * ROWS
    logits = (2.0 * torch.randn((R, N_CLS), generator=gen)).to(dev).requires_grad_()
    reg = (0.5 * torch.randn((R, 4 * N_CLS), generator=gen)).to(dev).requires_grad_()
    proposals = []
    for _ in range(N_IMG):
        p = BoxList(torch.zeros((ROWS, 4), device=dev), (1344, 800), "xyxy")
        pos = torch.rand(ROWS, generator=gen) < POSITIVE
        p.add_field("labels", (torch.randint(1, N_CLS, (ROWS,), generator=gen) * pos).to(dev))
        p.add_field("regression_targets", (0.5 * torch.randn((ROWS, 4), generator=gen)).to(dev))
        proposals.append(p)
    return logits, reg, proposals


def host_loss(class_logits, box_regression, proposals):
    """FastRCNNLossComputation.__call__ (loss.py:57-84) in torch, then backward."""
    device = class_logits.device
    labels = torch.cat([p.get_field("labels") for p in proposals], dim=0)
    regression_targets = torch.cat([p.get_field("regression_targets") for p in proposals], dim=0)
    classification_loss = torch.nn.functional.cross_entropy(class_logits, labels.long())
    sampled_pos_inds_subset = torch.nonzero(labels > 0).squeeze(1)
    labels_pos = labels[sampled_pos_inds_subset]
    map_inds = 4 * labels_pos[:, None] + torch.tensor([0, 1, 2, 3], device=device)
    n = torch.abs(box_regression[sampled_pos_inds_subset[:, None], map_inds] - regression_targets[sampled_pos_inds_subset])
    box_loss = torch.where(n < 1, 0.5 * n ** 2, n - 0.5).sum() / labels.numel()
    (classification_loss + box_loss).backward()
    return classification_loss.detach(), box_loss.detach()


def profile_call(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    on_device = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA]
    # the runtime's memcpy calls of any direction (a read-back through pinned memory, such as nonzero's count, runs as a blit kernel
    # without a direction in its name) or, if more, the activities named as device->host copies
    d2h = max(sum(1 for e in ev if e.name.startswith(("hipMemcpy", "cudaMemcpy"))),
              sum(1 for e in ev if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name))
    return sum(1 for k in on_device if "box_loss_" in k), len([k for k in on_device if "Memcpy" not in k and "Memset" not in k]), d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boxloss_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    logits, reg, proposals = batch(dev)
    loss = bl.FastRCNNLossComputation(False)

    def clear():
        logits.grad = reg.grad = None

    def device_call():
        clear()
        lc, lb = loss([logits], [reg], proposals)
        (lc + lb).backward()
        return lc.detach(), lb.detach()

    def host_call():
        clear()
        return host_loss(logits, reg, proposals)

    calls = {"device": device_call, "host": host_call}
    for _ in range(3):          # warm-up: code objects, allocator, the workspace
        got = {name: [float(v) for v in call()] for name, call in calls.items()}
    torch.cuda.synchronize()
    lines = [json.dumps({"setting": "losses (classification_loss, box_loss)", "device": got["device"], "host": got["host"]})]
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
    for name, call in calls.items():
        ours, kernels, d2h = profile_call(call)
        lines.append(json.dumps({"setting": name + " forward + backward", "images": N_IMG, "rows_per_image": ROWS, "classes": N_CLS,
                                 "box_columns": 4 * N_CLS, "ms_per_call": round(med[name], 4), "ms_min": round(min(times[name]), 4),
                                 "ms_max": round(max(times[name]), 4), "rounds": args.rounds, "reps": args.reps, "kernel_launches": kernels,
                                 "veto_box_loss_launches": ours, "memcpy_calls": d2h}))
    lines.append(json.dumps({"setting": "ratio", "host_over_device": round(med["host"] / med["device"], 2)}))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
