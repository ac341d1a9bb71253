"""MEET expert sampling on the device: the serial veto_meet_sample ('rand_insert', one device thread) against
veto_meet_sample_parallel in the three GCL_SETTING.ZERO_LABEL_PADDING_MODEs, on seeded labels and words.

  device time   device events around `--reps` back-to-back calls of the entry point on prepared device buffers (no read-back);
                the arms alternate inside every round, in one process; the report is the median round with its min and max
  host time     time.perf_counter around MeetTrainingSampler.sample (word generation, upload, the call, the read-back of the list
                lengths, the generator's advance); the parent arm is the same host path around the serial entry

n in 1 024 / 12 288 / 49 152 relations, foreground fractions 0.25 and 1.0, the VG and GQA tables.  Before anything is timed the
parallel 'rand_insert' result is compared with the serial one at every size (lists, labels, counts, words used).  `step_share` is the
device time over --step-ms (default 62.6: the measured L4 / H8 training step of tools/train_bench.py).
Prints one JSON line per setting.  Usage: python tools/meet_sample_bench.py [--reps 20] [--rounds 7] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import losses, meet_tables, native  # noqa: E402

GROUPS = {"VG": [4, 6, 9, 19, 12], "GQA": [5, 10, 20, 65]}
SIZES, FG = (1024, 12288, 49152), (0.25, 1.0)
ARMS = ("serial", "rand_insert", "rand_choose", "all_include")


class Setting:
    def __init__(self, sampler, n, fg, seed, dev):
        rng = np.random.RandomState(seed)
        labels = np.where(rng.random_sample(n) < fg, rng.randint(1, sampler.n_cls, size=n), 0)
        self.sampler, self.n, self.G = sampler, n, len(sampler.sizes)
        self.labels = torch.from_numpy(labels).to(dev)
        self.n_words = 4 * n + 64
        self.words = torch.from_numpy(rng.randint(0, 1 << 32, size=self.n_words, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
        self.out = {arm: (torch.empty((self.G, n), dtype=torch.int64, device=dev), torch.empty((self.G, n), dtype=torch.int64, device=dev),
                          torch.empty(self.G + 1, dtype=torch.int32, device=dev)) for arm in ARMS}
        self.lib = native.load_library()
        self.ws = torch.empty(max(self.lib.veto_meet_sample_parallel_workspace_bytes(n, self.n_words), 256), dtype=torch.uint8, device=dev)
        self.args = {}
        s = sampler
        for arm in ARMS[1:]:
            chosen, glabels, meta = self.out[arm]
            self.args[arm] = native.VetoMeetSampleArgs(
                struct_size=ctypes.sizeof(native.VetoMeetSampleArgs), mode=native.MEET_PAD_MODES[arm], n=n, n_words=self.n_words, n_groups=self.G,
                n_cls=s.n_cls, labels=self.labels.data_ptr(), words=self.words.data_ptr(), incre_idx_list=s.incre.data_ptr(),
                pos_in_group=s.pos_in_group.data_ptr(), group_size=s.group_size.data_ptr(), sample_rates=s.rates.data_ptr(),
                chosen=chosen.data_ptr(), group_labels=glabels.data_ptr(), counts=meta.data_ptr(), words_used=meta[self.G:].data_ptr())

    def call(self, arm):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if arm == "serial":
            s = self.sampler
            chosen, glabels, meta = self.out[arm]
            native.check(self.lib.veto_meet_sample(stream, self.labels.data_ptr(), self.n, self.words.data_ptr(), self.n_words, s.incre.data_ptr(),
                                                   s.pos_in_group.data_ptr(), s.group_size.data_ptr(), s.rates.data_ptr(), self.G, s.n_cls,
                                                   chosen.data_ptr(), glabels.data_ptr(), meta.data_ptr(), meta[self.G:].data_ptr()))
        else:
            native.check(self.lib.veto_meet_sample_parallel(stream, ctypes.byref(self.args[arm]), self.ws.data_ptr(), self.ws.numel()))

    def results_equal(self):
        """Serial against parallel rand_insert: counts, words used, and the valid part of every list."""
        for arm in ("serial", "rand_insert"):
            self.out[arm][0].fill_(-1)
            self.out[arm][1].fill_(-1)
            self.call(arm)
        torch.cuda.synchronize()
        a, b = self.out["serial"], self.out["rand_insert"]
        return bool(torch.equal(a[2], b[2]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])) and int(a[2][self.G]) > 0


def serial_sample(sampler, rel_labels):
    """MeetTrainingSampler.sample as it was around the serial entry: the parent arm of the host-side time."""
    dev, G = sampler.device, len(sampler.sizes)
    call = native.Launch(dev, "bench")
    labels = rel_labels.to(device=dev, dtype=torch.int64).contiguous()
    n = int(labels.shape[0])
    n_words = 4 * n + 64
    bg, st = losses._numpy_generator_from_python_random()
    words = torch.from_numpy(bg.random_raw(n_words).astype(np.uint32).view(np.int32)).to(dev)
    chosen = torch.empty((G, n), dtype=torch.int64, device=dev)
    glabels = torch.empty((G, n), dtype=torch.int64, device=dev)
    meta = torch.empty(G + 1, dtype=torch.int32, device=dev)
    call.run("veto_meet_sample", call.ptr(labels), n, call.ptr(words), n_words, sampler.incre.data_ptr(), sampler.pos_in_group.data_ptr(),
             sampler.group_size.data_ptr(), sampler.rates.data_ptr(), G, sampler.n_cls, chosen.data_ptr(), glabels.data_ptr(), meta.data_ptr(),
             meta[G:].data_ptr())
    host = meta.cpu().tolist()
    bg2, st = losses._numpy_generator_from_python_random()
    bg2.random_raw(host[G])
    s2 = bg2.state["state"]
    random.setstate((st[0], tuple(int(x) for x in s2["key"]) + (int(s2["pos"]),), st[2]))
    return [chosen[k, :host[k]] for k in range(G)], [glabels[k, :host[k]] for k in range(G)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-ms", type=float, default=62.6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meet_sample_bench needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"setting": "box", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "step_ms": args.step_ms})
    for dataset, sizes in GROUPS.items():
        samplers = {arm: losses.MeetTrainingSampler(dataset, sizes, device=dev, zero_label_padding_mode=arm) for arm in ARMS[1:]}
        for n in SIZES:
            for fg in FG:
                st = Setting(samplers["rand_insert"], n, fg, 1000 + n, dev)
                equal = st.results_equal()
                for arm in ARMS:          # warm-up: code objects, the allocator
                    for _ in range(3):
                        st.call(arm)
                torch.cuda.synchronize()
                dev_ms = {arm: [] for arm in ARMS}
                host_ms = {arm: [] for arm in ARMS}
                for rnd in range(args.rounds):
                    order = ARMS if rnd % 2 == 0 else ARMS[::-1]
                    for arm in order:
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(args.reps):
                            st.call(arm)
                        b.record()
                        b.synchronize()
                        dev_ms[arm].append(a.elapsed_time(b) / args.reps)
                    for arm in order:
                        random.seed(rnd)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(3):
                            serial_sample(samplers["rand_insert"], st.labels) if arm == "serial" else samplers[arm].sample(st.labels)
                        host_ms[arm].append((time.perf_counter() - t0) * 1e3 / 3)
                med = {arm: statistics.median(dev_ms[arm]) for arm in ARMS}
                for arm in ARMS:
                    emit({"setting": arm, "dataset": dataset, "n": n, "fg_fraction": fg, "device_ms": round(med[arm], 4),
                          "device_ms_min": round(min(dev_ms[arm]), 4), "device_ms_max": round(max(dev_ms[arm]), 4),
                          "host_sample_ms": round(statistics.median(host_ms[arm]), 3), "step_share": round(med[arm] / args.step_ms, 5)})
                emit({"setting": "rand_insert_vs_serial", "dataset": dataset, "n": n, "fg_fraction": fg, "results_equal": equal,
                      "serial_over_parallel": round(med["serial"] / med["rand_insert"], 2),
                      "parallel_max_below_serial_min": max(dev_ms["rand_insert"]) <= min(dev_ms["serial"])})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
