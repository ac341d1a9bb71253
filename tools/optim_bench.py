"""The optimizer side of a training iteration on the predictor's parameter sets (L4/H8 and L6/H6, the trainable tensors of
VETOPredictor with seeded gradients), three arrangements timed in one process in alternating rounds:

  torch    the reference's arrangement: torch.optim.Adam with one param group per parameter (pysgg/solver/build.py:7-34) behind a
           restatement of clip_grad_norm(clip=True) (pysgg/utils/checkpoint.py:194-211: one norm per parameter, `if clip_coef < 1`
           on a device tensor, one mul_ per parameter)
  fused    veto_amd.solver.Adam.clip_and_step(max_norm): one call
  pair     the drop-in pair: veto_amd.solver.clip_grad_norm(clip=True), then veto_amd.solver.Adam.step()

Every arrangement works on its own copy of the parameters; before each step, outside the timed span, the gradients are restored
from one master copy (clip=True scales them in place).  Reported per arrangement: device time per step (events around the step,
warm), wall time per step from the call on an idle device until the device is idle again, host time until the call returns, and
from the torch profiler for one step the kernel launches, the time the device spent inside them, the runtime's memcpy calls and how many of them read back (every call
beyond the library's one table upload is a read-back).  The report is the median round.  Prints one JSON line per setting and
says whether both device forms took less device time and less wall time than the torch arrangement of the same run.
Usage: python tools/optim_bench.py [--steps 20] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import solver, synth, testing  # noqa: E402

MAX_NORM = 5.0


class _Log(object):
    def info(self, msg):
        pass


def reference_clip_grad_norm(named_parameters, max_norm, clip=True):
    """The launch pattern of the reference's clip_grad_norm (pysgg/utils/checkpoint.py:194-211), written out here: one 2-norm
    launch per gradient, the squares accumulated one by one from Python, the coefficient formed on the device, ONE host branch
    on that device value (the read-back), and one in-place multiply per gradient when it clips."""
    grads = [p.grad for _, p in named_parameters if p.grad is not None]
    squares = 0
    for g in grads:
        squares = squares + g.norm(2) ** 2
    total = squares ** 0.5
    coef = float(max_norm) / (total + 1e-6)
    if clip and bool(coef < 1):                      # a device tensor: the host waits here for everything queued before
        for g in grads:
            g.mul_(coef)
    return total


def parameter_set(layers, heads, dev):
    """(names, shapes) of the trainable tensors of the predictor, and seeded gradients of norm ~ 4 x MAX_NORM."""
    cfg = testing.make_config(layers, heads)
    model = testing.make_predictor(cfg, synth.predictor_state_dict(0, layers=layers), dev)
    named = [(n, p.detach().clone()) for n, p in model.named_parameters() if p.requires_grad]
    del model
    gen = torch.Generator().manual_seed(1234)
    numel = sum(p.numel() for _, p in named)
    scale = 4.0 * MAX_NORM / np.sqrt(numel)
    grads = [(scale * torch.randn(p.shape, generator=gen)).to(dev) for _, p in named]
    return cfg, named, grads


class Arrangement(object):
    def __init__(self, kind, cfg, named, grads):
        self.kind = kind
        self.params = [torch.nn.Parameter(p.clone()) for _, p in named]
        self.named = [(n, p) for (n, _), p in zip(named, self.params)]
        self.master = grads
        for p, g in zip(self.params, grads):
            p.grad = g.clone()
        self.grads = [p.grad for p in self.params]
        groups = [{"params": [p], "lr": cfg.SOLVER.BASE_LR * (cfg.SOLVER.BIAS_LR_FACTOR if "bias" in n else 1),
                   "weight_decay": cfg.SOLVER.WEIGHT_DECAY_BIAS if "bias" in n else cfg.SOLVER.WEIGHT_DECAY} for n, p in self.named]
        self.opt = torch.optim.Adam(groups, lr=cfg.SOLVER.BASE_LR) if kind == "torch" else solver.Adam(groups, lr=cfg.SOLVER.BASE_LR)
        self.log = _Log()

    def restore(self):
        torch._foreach_copy_(self.grads, self.master)

    def step(self):
        if self.kind == "torch":
            total = reference_clip_grad_norm(self.named, MAX_NORM, clip=True)
            self.opt.step()
        elif self.kind == "fused":
            total = self.opt.clip_and_step(MAX_NORM)
        else:
            total = solver.clip_grad_norm(self.named, MAX_NORM, self.log, clip=True)
            self.opt.step()
        return total

    def round(self, steps):
        """(device ms, wall ms, host ms) per step, each the mean over `steps` steps that each start on an idle device."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        dev_ms = wall = host = 0.0
        for _ in range(steps):
            self.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            self.step()
            ev[1].record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            dev_ms += ev[0].elapsed_time(ev[1])
            host += (t1 - t0) * 1e3
            wall += (t2 - t0) * 1e3
        return dev_ms / steps, wall / steps, host / steps

    def profile(self):
        from torch.profiler import ProfilerActivity, profile
        self.restore()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            self.step()
            torch.cuda.synchronize()
        ev = list(prof.events())
        kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name
                   and "__amd_rocclr_" not in e.name and not e.name.startswith("Optimizer.step#")]
        memcpy = sum(1 for e in ev if e.name.startswith(("hipMemcpy", "cudaMemcpy")))
        uploads = {"torch": 0, "fused": 1, "pair": 2}[self.kind]          # the library's table upload, one per call
        busy = sum(getattr(e, "device_time", 0.0) for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and e.name in set(kernels))
        return len(kernels), memcpy, memcpy - uploads, busy * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    lines = []
    for layers, heads in ((4, 8), (6, 6)):
        cfg, named, grads = parameter_set(layers, heads, dev)
        arr = {kind: Arrangement(kind, cfg, named, grads) for kind in ("torch", "fused", "pair")}
        totals = {}
        for kind, a in arr.items():                 # warm-up: code objects, allocator, workspace, staging; and the three agree
            for _ in range(3):
                a.restore()
                totals[kind] = float(a.step())
        rounds = {kind: [] for kind in arr}
        for _ in range(args.rounds):
            for kind, a in arr.items():
                rounds[kind].append(a.round(args.steps))
        med = {kind: tuple(statistics.median(r[i] for r in rounds[kind]) for i in range(3)) for kind in arr}
        numel = sum(p.numel() for _, p in named)
        for kind, a in arr.items():
            kernels, memcpy, readbacks, busy_ms = a.profile()
            lines.append(json.dumps({"setting": "L%d/H%d %s" % (layers, heads, kind), "tensors": len(named), "elements": numel,
                                     "total_norm": round(totals[kind], 5), "device_ms_per_step": round(med[kind][0], 4),
                                     "wall_ms_per_step": round(med[kind][1], 4), "host_ms_per_step": round(med[kind][2], 4),
                                     "device_ms_min_max": [round(min(r[0] for r in rounds[kind]), 4), round(max(r[0] for r in rounds[kind]), 4)],
                                     "wall_ms_min_max": [round(min(r[1] for r in rounds[kind]), 4), round(max(r[1] for r in rounds[kind]), 4)],
                                     "kernel_launches": kernels, "kernels_busy_ms": round(busy_ms, 4), "memcpy_calls": memcpy, "read_backs": readbacks,
                                     "steps": args.steps, "rounds": args.rounds}))
        # bytes per element: the norm pass reads g (4); the step reads p, g, m, v and writes p, m, v (28); the in-place scaling reads and writes g (8)
        traffic = {"fused": 4 + 28, "pair": 4 + 8 + 28}
        busy = {kind: a.profile()[3] for kind, a in arr.items()}
        for kind in ("fused", "pair"):
            faster = med[kind][0] < med["torch"][0] and med[kind][1] < med["torch"][1]
            lines.append(json.dumps({"setting": "L%d/H%d %s against torch" % (layers, heads, kind),
                                     "device_time_ratio": round(med["torch"][0] / med[kind][0], 2), "wall_time_ratio": round(med["torch"][1] / med[kind][1], 2),
                                     "less_device_and_wall_time_than_torch": bool(faster),
                                     "bytes_per_step_gb": round(numel * traffic[kind] / 1e9, 4),
                                     "gb_per_s_over_device_time": round(numel * traffic[kind] / 1e9 / (med[kind][0] * 1e-3), 1),
                                     "gb_per_s_over_kernel_time": round(numel * traffic[kind] / 1e9 / (busy[kind] * 1e-3), 1) if busy[kind] else None}))
        del arr
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
