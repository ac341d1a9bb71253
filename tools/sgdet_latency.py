"""sgdet latency on the MI355X: 12 images x 80 detections (VG, L4/H8, MAX_PROPOSAL_PAIR 2048), with and without the
test-time overlap filter.  Reports the time per CALL of veto_amd.pairs.prepare_test_pairs and veto_amd.sgdet.decode_objects
(hipEvents around `--reps` back-to-back calls: the kernel plus the wrapper's host work -- concatenations, offsets, the ctypes
set-up and, with the overlap filter, the blocking read-back of the counts -- including the GPU idle time it causes; the
kernels alone come from a `rocprofv3 --kernel-trace --stats` run of this script), the wall time of
VETORelationHead.forward_pooled, and the device->host copies one forward issues (torch profiler).  Prints one JSON line per setting.  Usage: python tools/sgdet_latency.py [--reps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import predictor, synth, testing  # noqa: E402
from veto_amd.pairs import prepare_test_pairs  # noqa: E402
from veto_amd.relation_head import VETORelationHead  # noqa: E402
from veto_amd.sgdet import decode_objects  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402


def device_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def d2h_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return sum(1 for n in names if "DtoH" in n or "Device -> Host" in n or "DeviceToHost" in n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda")
    imgs = [synth.synthetic_detections(700 + i, 80, 151) for i in range(12)]
    props = []
    for d in imgs:
        b = BoxList(torch.from_numpy(d["boxes"]).to(dev), d["image_size"], "xyxy")
        for k in ("pred_scores", "pred_labels", "boxes_per_cls", "predict_logits"):
            b.add_field(k, torch.from_numpy(d[k]).to(dev))
        props.append(b)
    logits = torch.cat([p.get_field("predict_logits") for p in props])
    bpc = torch.cat([p.get_field("boxes_per_cls") for p in props])
    n_objs = [len(p) for p in props]
    predictor.set_embedding_provider(lambda names, w, k: torch.zeros(len(names), k))
    predictor.set_statistics_provider(lambda c: {"obj_classes": ["o%d" % i for i in range(151)],
                                                 "rel_classes": ["r%d" % i for i in range(51)]})
    total = sum(n_objs)
    feats = torch.from_numpy(synth.normal(3, "lat.roi", (total, 256, 8, 8), 0.0, 1.0)).to(dev)
    depth = torch.from_numpy(synth.normal(4, "lat.depth", (total, 256, 8, 8), 0.0, 1.0)).to(dev)
    for overlap in (False, True):
        cfg = testing.make_config(4, 8, mode="sgcls")
        cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
        cfg.TEST.RELATION.REQUIRE_OVERLAP = overlap
        cfg.TEST.RELATION.LATER_NMS_PREDICTION_THRES = 0.5
        head = VETORelationHead(cfg).to(dev).eval()
        sd = synth.predictor_state_dict(0, layers=4)
        head.predictor.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
        head.predictor.eval()
        pairs_us = device_us(lambda: prepare_test_pairs(dev, props, 2048, require_overlap=overlap, use_gt_box=False), args.reps)
        decode_us = device_us(lambda: decode_objects(logits, bpc, n_objs, 0.5), args.reps)
        fwd = lambda: head.forward_pooled(props, feats, depth)   # noqa: E731
        with torch.no_grad():
            fwd()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                _, res, _ = fwd()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / 10
            copies = d2h_copies(fwd)
        n_pairs = sum(len(r.get_field("rel_pair_idxs")) for r in res)
        print(json.dumps({"images": 12, "detections": 80, "overlap_filter": overlap, "pairs": n_pairs,
                          "prepare_test_pairs_call_us": round(pairs_us, 1), "decode_objects_call_us": round(decode_us, 1),
                          "forward_pooled_ms": round(ms, 3), "pairs_per_s": round(n_pairs / ms * 1e3),
                          "d2h_copies_per_forward": copies}))


if __name__ == "__main__":
    main()
