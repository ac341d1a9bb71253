"""Times the device detection (box mAP) evaluator at a VG-validation-like size: 5 000 images x 80 detections, 151 classes, fed in
batches of 12 images with the inputs already on the device (where veto_amd.boxhead.PostProcessor leaves them).

  update    per batch: device events around DetectionEvaluator.update (torch's concatenations + veto_det_eval_match), and the
            host clock over the whole split ending in a synchronise
  finalize  the host clock around DetectionEvaluator.finalize (veto_det_eval_accumulate + the read-back, which synchronises)

Every shape is warmed by one untimed pass over the split; the timed pass is repeated and the spread printed.  There is no speed
criterion: the reference's own path (pycocotools) is not installed and cannot be timed.  --restatement N also times the numpy
restatement of COCOeval the tests compare with (tests/det_eval_cases.py) on the first N images, on the host, as context only."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from veto_amd.evaluation import DetectionEvaluator  # noqa: E402


def make_split(n_img, n_det, n_cls, seed):
    """Per image 10-40 GT boxes; detections are jittered GT boxes (85 % with the GT class) or noise; scores rounded to 1/64."""
    rng = np.random.RandomState(seed)
    images = []
    for _ in range(n_img):
        n_gt = rng.randint(10, 41)
        xy = rng.uniform(0, 580, (n_gt, 2))
        wh = rng.choice([8., 24., 60., 150.], (n_gt, 2)) * rng.uniform(.6, 1.4, (n_gt, 2))
        gt = np.concatenate([xy, xy + wh], 1).round().astype(np.float32)
        gcls = rng.randint(1, n_cls, n_gt)
        src = rng.randint(0, n_gt, n_det)
        db = gt[src] + rng.normal(0, 1, (n_det, 4)) * (wh[src].mean(1, keepdims=True) * rng.choice([.02, .1, .3], (n_det, 1)))
        noise = rng.uniform(0, 1, n_det) < .3
        nxy = rng.uniform(0, 580, (n_det, 2))
        db[noise] = np.concatenate([nxy, nxy + rng.uniform(5, 200, (n_det, 2))], 1)[noise]
        db[:, 2:] = np.maximum(db[:, 2:], db[:, :2])
        dcls = np.where(rng.uniform(0, 1, n_det) < .85, gcls[src], rng.randint(1, n_cls, n_det))
        images.append({"gt_boxes": gt, "gt_classes": gcls.astype(np.int64), "pred_boxes": db.astype(np.float32),
                       "pred_classes": dcls.astype(np.int64), "obj_scores": (np.round(rng.uniform(0, 1, n_det) * 64) / 64).astype(np.float32)})
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--detections", type=int, default=80)
    ap.add_argument("--classes", type=int, default=151)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restatement", type=int, default=0, help="also time the numpy restatement on the first N images (host, context only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_eval_bench needs the GPU: a host run measures nothing")
    dev = torch.device("cuda:0")
    images = make_split(args.images, args.detections, args.classes, 2024)
    on_dev = [{k: torch.as_tensor(v).to(dev) for k, v in im.items()} for im in images]
    batches = [on_dev[i:i + args.batch] for i in range(0, len(on_dev), args.batch)]
    ev = DetectionEvaluator(args.classes, device=dev)

    def one_pass(timed):
        ev.reset()
        events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            if timed:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
            ev.update(b)
            if timed:
                stop.record()
                events.append((start, stop))
        torch.cuda.synchronize()
        t_update = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = ev.finalize()
        t_final = time.perf_counter() - t0
        dev_ms = [s.elapsed_time(e) for s, e in events]
        return t_update, t_final, dev_ms, res

    one_pass(False)                                    # warm-up: every batch shape, the buffer growth, the accumulate workspace
    rows = []
    for _ in range(args.repeats):
        t_update, t_final, dev_ms, res = one_pass(True)
        rows.append((t_update * 1e3 / len(batches), float(np.median(dev_ms)), float(np.sum(dev_ms)), t_final * 1e3))
    print("det_eval_bench: %d images x %d detections, %d classes, %d batches of %d; %d records; mAp %.4f, recall@100 IOU:0.5 %.4f"
          % (args.images, args.detections, args.classes, len(batches), args.batch, args.images * args.detections, res["mAp"],
             res["recall@100_iou0.5"]))
    print("repeat | update: host clock per batch (ms) | update: device events per batch, median (ms) | update: device events, split total (ms) | finalize: host clock incl. read-back (ms)")
    for i, r in enumerate(rows):
        print("%6d | %10.4f | %10.4f | %10.2f | %10.3f" % ((i,) + r))
    med = np.median(np.array(rows), axis=0)
    print("median | %10.4f | %10.4f | %10.2f | %10.3f" % tuple(med))
    if args.restatement:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import det_eval_cases as dc
        n = min(args.restatement, len(images))
        t0 = time.perf_counter()
        want = dc.np_coco_eval(images[:n], args.classes, 0)
        t_host = time.perf_counter() - t0
        got = DetectionEvaluator(args.classes, device=dev).evaluate(on_dev[:n])
        print("context only: the numpy restatement (np_coco_eval, never run against pycocotools) on the first %d images: %.1f s on the host; "
              "the device result on the same %d images equals it in %d of %d precision cells"
              % (n, t_host, n, int((got["precision"] == want["precision"]).sum()), want["precision"].size))


if __name__ == "__main__":
    main()
