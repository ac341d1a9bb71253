"""Latency of the RPN loss on the device (veto_amd.rpnloss.RPNLossComputation: one veto_rpn_loss call, then the backward that
scales its gradients) against the reference's algorithm restated in plain torch on the same device tensors, forward and backward,
on an FPN pyramid over a 1344 x 800 batch: 12 images x 268 569 anchors (strides 4..64, three ratios) x 20 GT boxes,
BATCH_SIZE_PER_IMAGE 256 at POSITIVE_FRACTION 0.5, thresholds 0.7 / 0.3 with low-quality matches.

  device   anchor matching, sampling, both losses and their gradients in seven launches; backward = one multiply per level tensor
  host     per image: the [20, 268 569] boxlist_iou matrix, max over both axes, the nonzero over the equality mask, the labels,
           BoxCoder.encode, two nonzero / randperm pairs; then concat_box_prediction_layers (permute + reshape + cat of every
           level), smooth-L1 and BCE-with-logits, and autograd's backward through the gathers and the concatenation

The two sides are timed in the same process in alternating rounds of `--reps` calls (50: tens of milliseconds per round on the
device side), each round ending in a synchronise; the report is the median round of each and their ratio.  The times are host
wall-clock per call: they include the Python side of a call, not kernel time alone.  The launches and the memcpy calls (of any
direction: every read-back is one) of one call of each are counted with the torch profiler, after the timing.  Prints one JSON line per setting.
Usage: python tools/rpnloss_bench.py [--reps 50] [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import rpnloss as rl  # noqa: E402
from veto_amd import synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

HIGH, LOW, BATCH, FRACTION, BETA = 0.7, 0.3, 256, 0.5, 1.0 / 9
N_IMG, N_GT, SIZE = 12, 20, (1344, 800)
STRIDES, SIZES, RATIOS = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)
GRIDS = ((200, 336), (100, 168), (50, 84), (25, 42), (13, 21))


def batch(dev):
    anchors = [torch.from_numpy(a).to(dev) for a in synth.anchor_grid(SIZES, STRIDES, RATIOS, GRIDS)]
    gt = synth.synthetic_rpn_training_batch(77, [SIZE] * N_IMG, [(1, 1, 1)], [N_GT] * N_IMG, min_side=32.0)["tgt_boxes"]
    gen = torch.Generator(device="cpu").manual_seed(77)
    obj = [(2.0 * torch.randn((N_IMG, 3, h, w), generator=gen)).to(dev).requires_grad_() for h, w in GRIDS]
    reg = [(0.5 * torch.randn((N_IMG, 12, h, w), generator=gen)).to(dev).requires_grad_() for h, w in GRIDS]
    lists = [[BoxList(a, SIZE, "xyxy") for a in anchors] for _ in range(N_IMG)]
    targets = [BoxList(torch.from_numpy(t).to(dev), SIZE, "xyxy") for t in gt]
    return lists, obj, reg, targets


def host_prepare(anchor, size, tgt):
    """One image of prepare_targets (loss.py:56-89) with Matcher(allow_low_quality_matches=True) in torch."""
    area_t = (tgt[:, 2] - tgt[:, 0] + 1) * (tgt[:, 3] - tgt[:, 1] + 1)
    area_a = (anchor[:, 2] - anchor[:, 0] + 1) * (anchor[:, 3] - anchor[:, 1] + 1)
    wh = (torch.min(tgt[:, None, 2:], anchor[:, 2:]) - torch.max(tgt[:, None, :2], anchor[:, :2]) + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    quality = inter / (area_t[:, None] + area_a - inter)
    vals, matches = quality.max(dim=0)
    all_matches = matches.clone()
    matches[vals < LOW] = -1
    matches[(vals >= LOW) & (vals < HIGH)] = -2
    best, _ = quality.max(dim=1)
    update = torch.nonzero(quality == best[:, None])[:, 1]
    matches[update] = all_matches[update]
    labels = (matches >= 0).to(torch.float32)
    labels[matches == -1] = 0
    visible = (anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] < size[0]) & (anchor[:, 3] < size[1])
    labels[~visible] = -1
    labels[matches == -2] = -1
    g = tgt[matches.clamp(min=0)]
    ew, eh = anchor[:, 2] - anchor[:, 0] + 1, anchor[:, 3] - anchor[:, 1] + 1
    gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    reg = torch.stack([(g[:, 0] + 0.5 * gw - anchor[:, 0] - 0.5 * ew) / ew, (g[:, 1] + 0.5 * gh - anchor[:, 1] - 0.5 * eh) / eh,
                       torch.log(gw / ew), torch.log(gh / eh)], 1)
    return labels, reg


def host_loss(lists, obj, reg, targets):
    """RPNLossComputation.__call__ (loss.py:92-131) in torch, then backward."""
    labels, reg_targets, pos_masks, neg_masks = [], [], [], []
    for per_img, t in zip(lists, targets):
        lab, rt = host_prepare(torch.cat([a.bbox for a in per_img]), per_img[0].size, t.bbox)
        pos, neg = torch.nonzero(lab >= 1).squeeze(1), torch.nonzero(lab == 0).squeeze(1)
        num_pos = min(pos.numel(), int(BATCH * FRACTION))
        num_neg = min(neg.numel(), BATCH - num_pos)
        pm, nm = torch.zeros_like(lab, dtype=torch.uint8), torch.zeros_like(lab, dtype=torch.uint8)
        pm[pos[torch.randperm(pos.numel(), device=pos.device)[:num_pos]]] = 1
        nm[neg[torch.randperm(neg.numel(), device=neg.device)[:num_neg]]] = 1
        labels.append(lab)
        reg_targets.append(rt)
        pos_masks.append(pm)
        neg_masks.append(nm)
    sampled_pos = torch.nonzero(torch.cat(pos_masks)).squeeze(1)
    sampled = torch.cat([sampled_pos, torch.nonzero(torch.cat(neg_masks)).squeeze(1)])
    n = obj[0].shape[0]
    flat_o = torch.cat([o.view(n, -1, 1, o.shape[2], o.shape[3]).permute(0, 3, 4, 1, 2).reshape(n, -1, 1) for o in obj], 1).reshape(-1)
    flat_r = torch.cat([r.view(n, -1, 4, r.shape[2], r.shape[3]).permute(0, 3, 4, 1, 2).reshape(n, -1, 4) for r in reg], 1).reshape(-1, 4)
    labels, reg_targets = torch.cat(labels), torch.cat(reg_targets)
    d = torch.abs(flat_r[sampled_pos] - reg_targets[sampled_pos])
    box_loss = torch.where(d < BETA, 0.5 * d ** 2 / BETA, d - 0.5 * BETA).sum() / sampled.numel()
    obj_loss = torch.nn.functional.binary_cross_entropy_with_logits(flat_o[sampled], labels[sampled])
    (obj_loss + box_loss).backward()
    return obj_loss.detach(), box_loss.detach()


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
    return sum(1 for k in on_device if "rpn_" in k), len([k for k in on_device if "Memcpy" not in k and "Memset" not in k]), d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rpnloss_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    lists, obj, reg, targets = batch(dev)
    rpn = types.SimpleNamespace(FG_IOU_THRESHOLD=HIGH, BG_IOU_THRESHOLD=LOW, BATCH_SIZE_PER_IMAGE=BATCH, POSITIVE_FRACTION=FRACTION,
                                STRADDLE_THRESH=0)
    loss = rl.make_rpn_loss_evaluator(types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN=rpn)), rl.BoxCoder((1., 1., 1., 1.)))

    def clear():
        for t in obj + reg:
            t.grad = None

    def device_call():
        clear()
        lo, lb = loss(lists, obj, reg, targets, seed=1)
        (lo + lb).backward()
        return lo.detach(), lb.detach()

    def host_call():
        clear()
        return host_loss(lists, obj, reg, targets)

    calls = {"device": device_call, "host": host_call}
    for _ in range(3):          # warm-up: code objects, allocator, the cached sizes and offsets
        got = {name: [float(v) for v in call()] for name, call in calls.items()}
    torch.cuda.synchronize()
    lines = [json.dumps({"setting": "losses (the draws differ: the device samples by a counter-based hash, the host by randperm)",
                         "device": got["device"], "host": got["host"]})]
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
        lines.append(json.dumps({"setting": name + " forward + backward", "images": N_IMG, "anchors_per_image": sum(3 * h * w for h, w in GRIDS),
                                 "gt_boxes": N_GT, "batch_size_per_image": BATCH, "positive_fraction": FRACTION,
                                 "ms_per_call": round(med[name], 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                                 "rounds": args.rounds, "reps": args.reps, "kernel_launches": kernels, "veto_rpn_loss_launches": ours,
                                 "memcpy_calls": d2h}))
    lines.append(json.dumps({"setting": "ratio", "host_over_device": round(med["host"] / med["device"], 2)}))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
