"""Inputs and the yardstick of the detection (box mAP) evaluator tests (test_det_eval_host.py, test_det_eval_gpu.py).

The reference computes these numbers with pycocotools (vg_eval.py:67-182), which is installed neither here nor in the reference
tree, so the yardstick is a numpy restatement of COCOeval.evaluate() / accumulate() / summarize() as vg_eval.py drives them.
NOBODY HAS RUN pycocotools AGAINST IT.  To keep it honest without the original it is written twice, independently:

  np_coco_eval       the literal loop form: per (image, class, area) evaluateImg with its gtm / dtm / dtIg arrays and its
                     break / continue rules, then concatenate, mergesort argsort, cumsum, backward envelope, searchsorted
  np_coco_eval_flat  flat sorted records, greedy matching by masked argmax, precision as "maximum of pr over rc >= threshold"

test_det_eval_host.py requires the two to agree bit for bit on every case and pins both to hand-derived numbers.
np_coco_eval takes `mut`, a deliberately wrong variant (MUTATIONS), and `tie`, a wrong order among equal scores (TIE_ORDERS):
each must change a result on the cases built for it.
"""
import functools
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNGS), len(MAX_DETS)
EPS = float(np.spacing(1))

MUTATIONS = ("gt_strict", "double_width", "no_break", "unstable", "side_right", "no_envelope", "ignore_first_id", "late_cut")
TIE_ORDERS = ("reverse", "image_reverse", "inimage_reverse")


def bb_iou(d, g):
    """maskApi.c bbIou for one pair of xywh boxes, in double (Python floats)."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3] - i
    return i / u


def gt_xywh(box):
    """vg_eval.py:72-76: the float32 coordinates widened (tolist), w and h formed in double."""
    b = [float(v) for v in np.asarray(box, np.float32)]
    return [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]


def det_xywh(box, double_width=False):
    """BoxList.convert('xywh'): x2 - x1 + 1 in float32, widened afterwards by np.column_stack (vg_eval.py:97-108)."""
    b = np.asarray(box, np.float32)
    if double_width:
        return gt_xywh(b)
    one = np.float32(1)
    return [float(b[0]), float(b[1]), float((b[2] - b[0]) + one), float((b[3] - b[1]) + one)]


def _desc_order(scores, tie, image=None):
    """np.argsort(-scores, kind='mergesort'), or a wrong order among equal scores."""
    s = -np.asarray(scores, np.float64)
    n = len(s)
    pos = np.arange(n)
    if tie == "stable" or (tie == "image_reverse" and image is None) or (tie == "inimage_reverse" and image is not None):
        return np.argsort(s, kind="mergesort")
    if tie == "reverse" or tie == "inimage_reverse":
        return np.lexsort((-pos, s))
    if tie == "image_reverse":
        return np.lexsort((pos, -np.asarray(image), s))
    raise ValueError(tie)


# ---------------------------------------------------------------------------------------------------------------------------
# the literal form
# ---------------------------------------------------------------------------------------------------------------------------
def np_coco_eval(images, num_classes, first_gt_id=0, mut=None, tie="stable"):
    assert mut is None or mut in MUTATIONS
    if mut == "unstable":
        tie = "reverse"
    K = num_classes - 1
    gts, dts = defaultdict(list), defaultdict(list)
    ann_id = 1 if mut == "ignore_first_id" else first_gt_id
    det_id = 1                                             # loadRes numbers the results from 1
    for img, im in enumerate(images):
        for cls, box in zip(np.asarray(im["gt_classes"]).reshape(-1).tolist(), np.asarray(im["gt_boxes"], np.float32).reshape(-1, 4)):
            bb = gt_xywh(box)
            gts[img, int(cls)].append({"area": bb[3] * bb[2], "bbox": bb, "id": ann_id, "ignore": 0})
            ann_id += 1
        boxes = np.asarray(im["pred_boxes"], np.float32).reshape(-1, 4)
        for cls, score, box in zip(np.asarray(im["pred_classes"]).reshape(-1).tolist(), np.asarray(im["obj_scores"]).reshape(-1).tolist(), boxes):
            bb = det_xywh(box, double_width=mut == "double_width")
            dts[img, int(cls)].append({"area": bb[2] * bb[3], "bbox": bb, "score": float(score), "id": det_id})
            det_id += 1
    n_img = len(images)
    cat_ids = list(range(1, num_classes))
    max_det = MAX_DETS[-1]

    def compute_iou(img, cat):
        gt, dt = gts[img, cat], dts[img, cat]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = _desc_order([d["score"] for d in dt], tie)
        dt = [dt[i] for i in inds]
        if len(dt) > max_det:
            dt = dt[0:max_det]
        ious = np.zeros((len(dt), len(gt)))
        for di, d in enumerate(dt):
            for gi, g in enumerate(gt):
                ious[di, gi] = bb_iou(d["bbox"], g["bbox"])
        return ious

    all_ious = {(img, cat): compute_iou(img, cat) for img in range(n_img) for cat in cat_ids}

    def evaluate_img(img, cat, a_rng):
        gt, dt = gts[img, cat], dts[img, cat]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = _desc_order([d["score"] for d in dt], tie)
        dt = [dt[i] for i in dtind[0:max_det]]
        ious = all_ious[img, cat][:, gtind] if len(all_ious[img, cat]) > 0 else all_ious[img, cat]
        G, D = len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([g["_ignore"] for g in gt])
        dt_ig = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1 and mut != "no_break":
                            break
                        if (ious[dind, gind] <= iou) if mut == "gt_strict" else (ious[dind, gind] < iou):
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig, "image": img}

    eval_imgs = [evaluate_img(img, cat, a_rng) for cat in cat_ids for a_rng in AREA_RNGS for img in range(n_img)]

    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        nk = k * A * n_img
        for a in range(A):
            na = a * n_img
            for m, max_d in enumerate(MAX_DETS):
                E = [eval_imgs[nk + na + i] for i in range(n_img)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                cut = MAX_DETS[-1] if mut == "late_cut" else max_d
                dt_scores = np.concatenate([e["dtScores"][0:cut] for e in E])
                image = np.concatenate([[e["image"]] * len(e["dtScores"][0:cut]) for e in E])
                inds = _desc_order(dt_scores, tie, image)
                if mut == "late_cut":
                    inds = inds[0:max_d]
                dtm = np.concatenate([e["dtMatches"][:, 0:cut] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:cut] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,)).tolist()
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    if mut != "no_envelope":
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="right" if mut == "side_right" else "left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return _summarize(precision, recall)


def _summarize(precision, recall):
    """COCOeval.summarize()'s twelve numbers and vg_eval.py:177's recall@100 at IoU 0.5."""
    def one(ap, iou_thr=None, a=0, m=2):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    stats = np.array([one(1), one(1, .5), one(1, .75), one(1, a=1), one(1, a=2), one(1, a=3),
                      one(0, m=0), one(0, m=1), one(0, m=2), one(0, a=1), one(0, a=2), one(0, a=3)])
    return {"precision": precision, "recall": recall, "stats": stats, "recall50_100": one(0, .5)}


# ---------------------------------------------------------------------------------------------------------------------------
# the flat form, written independently of the above
# ---------------------------------------------------------------------------------------------------------------------------
def np_coco_eval_flat(images, num_classes, first_gt_id=0):
    K = num_classes - 1
    lo = np.array([r[0] for r in AREA_RNGS], np.float64)
    hi = np.array([r[1] for r in AREA_RNGS], np.float64)
    thr = np.minimum(IOU_THRS, 1 - 1e-10)
    npig = np.zeros((K, A), np.int64)
    rec_cls, rec_score, rec_rank, rec_match, rec_ign = [], [], [], [], []
    gt_seen = 0
    for im in images:
        gb = np.asarray(im["gt_boxes"], np.float32).reshape(-1, 4).astype(np.float64)
        gc = np.asarray(im["gt_classes"]).reshape(-1).astype(np.int64)
        gw, gh = gb[:, 2] - gb[:, 0] + 1, gb[:, 3] - gb[:, 1] + 1
        g_area = gh * gw
        g_out = (g_area[:, None] < lo[None]) | (g_area[:, None] > hi[None])         # [G, A]
        g_id = first_gt_id + gt_seen + np.arange(len(gc))
        gt_seen += len(gc)
        np.add.at(npig, (np.repeat(gc - 1, A), np.tile(np.arange(A), len(gc))), (~g_out).reshape(-1).astype(np.int64))
        db32 = np.asarray(im["pred_boxes"], np.float32).reshape(-1, 4)
        dc = np.asarray(im["pred_classes"]).reshape(-1).astype(np.int64)
        ds = np.asarray(im["obj_scores"]).reshape(-1).astype(np.float64)
        dw = ((db32[:, 2] - db32[:, 0]) + np.float32(1)).astype(np.float64)
        dh = ((db32[:, 3] - db32[:, 1]) + np.float32(1)).astype(np.float64)
        dx, dy = db32[:, 0].astype(np.float64), db32[:, 1].astype(np.float64)
        d_area = dw * dh
        d_out = (d_area[:, None] < lo[None]) | (d_area[:, None] > hi[None])         # [D, A]
        order = np.lexsort((np.arange(len(dc)), -ds, dc))                            # class, score descending, index
        for c in np.unique(dc):
            sel = order[dc[order] == c][:MAX_DETS[-1]]
            gsel = np.nonzero(gc == c)[0]
            n, G = len(sel), len(gsel)
            iw = np.minimum((dw + dx)[sel, None], (gw + gb[:, 0])[None, gsel]) - np.maximum(dx[sel, None], gb[None, gsel, 0])
            ih = np.minimum((dh + dy)[sel, None], (gh + gb[:, 1])[None, gsel]) - np.maximum(dy[sel, None], gb[None, gsel, 1])
            inter = iw * ih
            union = (dw * dh)[sel, None] + (gw * gh)[None, gsel] - inter
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.where((iw > 0) & (ih > 0), inter / union, 0.0)              # [n, G]
            match = np.zeros((n, T, A), bool)
            ign = np.zeros((n, T, A), bool)
            for t in range(T):
                for a in range(A):
                    free = np.ones(G, bool)
                    for d in range(n):
                        cand = free & (iou[d] >= thr[t])
                        m = -1
                        for group in (cand & ~g_out[gsel, a], cand & g_out[gsel, a]):  # non-ignored GT first; the ignored only without a match
                            idx = np.nonzero(group)[0]
                            if len(idx):
                                best = iou[d, idx].max()
                                m = idx[iou[d, idx] == best][-1]                        # of equal IoUs the later GT wins
                                break
                        if m < 0:
                            ign[d, t, a] = d_out[sel[d], a]
                            continue
                        free[m] = False
                        counted = g_id[gsel[m]] != 0                                    # annotation id 0 is falsy in accumulate
                        match[d, t, a] = counted
                        ign[d, t, a] = g_out[gsel[m], a] or (not counted and d_out[sel[d], a])
            rec_cls.append(np.full(n, c)); rec_score.append(ds[sel]); rec_rank.append(np.arange(n))
            rec_match.append(match); rec_ign.append(ign)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    if rec_cls:
        cls, score, rank = np.concatenate(rec_cls), np.concatenate(rec_score), np.concatenate(rec_rank)
        match, ign = np.concatenate(rec_match), np.concatenate(rec_ign)
        # within an image the classes were appended one after the other, so sorting by (class, -score) stably over the append
        # order gives image order and then in-image rank among equal scores
        order = np.lexsort((np.arange(len(cls)), -score, cls))
        cls, rank, match, ign = cls[order], rank[order], match[order], ign[order]
    for k in range(K):
        for a in range(A):
            if npig[k, a] == 0:
                continue
            seg = np.nonzero(cls == k + 1)[0] if rec_cls else np.zeros(0, np.int64)
            for m, max_d in enumerate(MAX_DETS):
                s = seg[rank[seg] < max_d] if len(seg) else seg
                for t in range(T):
                    if len(s) == 0:
                        precision[t, :, k, a, m] = 0
                        recall[t, k, a, m] = 0
                        continue
                    tp = np.cumsum(match[s, t, a] & ~ign[s, t, a]).astype(np.float64)
                    fp = np.cumsum(~match[s, t, a] & ~ign[s, t, a]).astype(np.float64)
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + EPS)
                    reach = rc[None, :] >= REC_THRS[:, None]                           # [R, n]
                    precision[t, :, k, a, m] = np.where(reach, pr[None, :], 0.0).max(axis=1)
                    recall[t, k, a, m] = rc[-1]
    return _summarize(precision, recall)


# ---------------------------------------------------------------------------------------------------------------------------
# cases: name -> dict(batches=[[image, ...], ...], num_classes, first_gt_id)
# ---------------------------------------------------------------------------------------------------------------------------
def image(gt=(), det=()):
    """gt: (class, x1, y1, x2, y2) rows; det: (class, score, x1, y1, x2, y2) rows."""
    gt = np.asarray(gt, np.float64).reshape(-1, 5)
    det = np.asarray(det, np.float64).reshape(-1, 6)
    return {"gt_boxes": gt[:, 1:].astype(np.float32), "gt_classes": gt[:, 0].astype(np.int64),
            "pred_boxes": det[:, 2:].astype(np.float32), "pred_classes": det[:, 0].astype(np.int64),
            "obj_scores": det[:, 1].astype(np.float32)}


FAR = (5000., 5000., 5009., 5009.)     # a 10 x 10 box that touches nothing


def _hand_cases():
    c = {}
    # every detection equals its GT box; annotation 0 is the class-1 box of image 0
    perfect = [[image(gt=[(1, 0, 0, 9, 9), (2, 0, 0, 49, 49)], det=[(1, .9, 0, 0, 9, 9), (2, .8, 0, 0, 49, 49)]),
                image(gt=[(1, 10, 10, 119, 119)], det=[(1, .7, 10, 10, 119, 119)])]]
    c["perfect_id1"] = dict(batches=perfect, num_classes=3, first_gt_id=1)
    c["perfect_id0"] = dict(batches=perfect, num_classes=3, first_gt_id=0)
    # two detections on one GT box: the higher score (listed second) takes it
    c["two_on_one"] = dict(batches=[[image(gt=[(1, 0, 0, 9, 9)], det=[(1, .6, 0, 0, 9, 9), (1, .9, 0, 0, 9, 9)])]], num_classes=3, first_gt_id=1)
    # one detection between two GT boxes.  Class 1: IoU 0.6 with both -> the later; class 2: 2/3 with the first, 7/13 with the
    # second -> the first.  A second detection on the box that was taken shows which one it was.
    c["between_two"] = dict(batches=[[image(gt=[(1, 0, 0, 19, 9), (1, 10, 0, 29, 9), (2, 0, 0, 19, 9), (2, 10, 0, 29, 9)],
                                            det=[(1, .9, 5, 0, 24, 9), (1, .5, 10, 0, 29, 9), (2, .9, 4, 0, 23, 9), (2, .5, 0, 0, 19, 9)])]],
                            num_classes=3, first_gt_id=1)
    # area "medium": the detection's best GT box (100 x 100, IoU 1) is ignored there, a 90 x 90 one (IoU 0.81) is not -> takes the
    # latter up to threshold 0.80; from 0.85 on it matches only the ignored box and is neither TP nor FP.  Image 1: a plain TP of
    # lower score, whose precision shows whether the first detection counted as a false positive.
    c["prefer_nonignored"] = dict(batches=[[image(gt=[(1, 0, 0, 99, 99), (1, 0, 0, 89, 89)], det=[(1, .9, 0, 0, 99, 99)]),
                                            image(gt=[(1, 200, 200, 259, 259)], det=[(1, .3, 200, 200, 259, 259)])]],
                                  num_classes=3, first_gt_id=1)
    # an unmatched 5 x 5 detection: a false positive for "all", ignored for "medium"
    c["unmatched_outside"] = dict(batches=[[image(gt=[(1, 0, 0, 59, 59)], det=[(1, .9, 300, 300, 304, 304), (1, .5, 0, 0, 59, 59)])]],
                                  num_classes=3, first_gt_id=1)
    # IoU exactly 0.5 (class 1: 10 x 10 inside 20 x 10) and exactly 0.75 (class 2: 15 x 10 inside 20 x 10)
    c["iou_at_threshold"] = dict(batches=[[image(gt=[(1, 0, 0, 19, 9), (2, 0, 0, 19, 9)], det=[(1, .9, 0, 0, 9, 9), (2, .9, 0, 0, 14, 9)])]],
                                 num_classes=3, first_gt_id=1)
    # the next double below each.  The detection is the unit box (0, 0, 0, 0): w = h = 1.  The GT box has x1 = 2^-53 > x2 = 0, so
    # gw = (0 - 2^-53) + 1 = 1 - 2^-53 exactly and gx + gw = 1; y1 = 0.5 (0.25) > y2 = 0, so gh = 0.5 (0.75) and gy + gh = 1: the GT
    # box lies inside the detection, i = gw * gh = 0.5 - 2^-54 (0.75 - 2^-53 after rounding), u = (1 + i) - i rounds to 1.
    c["iou_below_threshold"] = dict(batches=[[image(gt=[(1, 2. ** -53, .5, 0, 0), (2, 2. ** -53, .25, 0, 0)],
                                                    det=[(1, .9, 0, 0, 0, 0), (2, .9, 0, 0, 0, 0)])]], num_classes=3, first_gt_id=1)
    # float32 width: x1 = 2^-5, x2 = 2^21 - 1.  x2 - x1 = 2097150.96875 rounds in float32 (grid 1/8) to 2097151, so w = 2^21 and
    # the IoU with the GT box of width 2^22 is exactly 0.5; formed in double, w = 2^21 - 2^-5 and the IoU is below 0.5
    c["f32_width"] = dict(batches=[[image(gt=[(1, 0, 0, 2. ** 22 - 1, 0)], det=[(1, .9, 2. ** -5, 0, 2. ** 21 - 1, 0)])]],
                          num_classes=3, first_gt_id=1)
    # equal scores: class 1 all 0.5, class 2 zeros of both signs.  TP = the GT box, FP = FAR.  In (image, index) order the
    # records read TP FP | TP TP; reversed TP TP FP TP; images swapped TP TP TP FP; in-image swapped FP TP TP TP
    def tie_image(s, pattern, x0, cls):
        gts = [(cls, x0 + 100 * j, 0, x0 + 100 * j + 9, 9) for j, p in enumerate(pattern) if p]
        dets = [((cls, s[j], x0 + 100 * j, 0, x0 + 100 * j + 9, 9) if p else (cls, s[j]) + FAR) for j, p in enumerate(pattern)]
        return gts, dets
    g1a, d1a = tie_image([.5, .5], [1, 0], 0, 1)
    g1b, d1b = tie_image([.5, .5], [1, 1], 0, 1)
    g2a, d2a = tie_image([-0., 0.], [1, 0], 1000, 2)
    g2b, d2b = tie_image([0., -0.], [1, 1], 1000, 2)
    c["score_ties"] = dict(batches=[[image(gt=g1a + g2a, det=d1a + d2a), image(gt=g1b + g2b, det=d1b + d2b)]], num_classes=3, first_gt_id=1)
    # 130 detections of one class in one image, listed in a shuffled order; by score rank: 0 a false positive, 9 on GT box A,
    # 50 on B, 110 (beyond the cut of 100) on C, every other one FAR
    rng = np.random.RandomState(5)
    boxes = {9: (0, 0, 9, 9), 50: (100, 0, 109, 9), 110: (200, 0, 209, 9)}
    dets = [(1, 1.0 - rank / 256.) + tuple(boxes.get(rank, FAR)) for rank in range(130)]
    dets = [dets[i] for i in rng.permutation(130)]
    c["maxdets"] = dict(batches=[[image(gt=[(1,) + boxes[9], (1,) + boxes[50], (1,) + boxes[110]], det=dets)]], num_classes=3, first_gt_id=1)
    # class 1: GT but no detection; class 2: detections but no GT anywhere; class 3: ordinary.  Image 0 (first of batch 0) is empty,
    # image 1 has no GT, image 2 no detection, image 3 (first of batch 1) is empty again
    c["empties"] = dict(batches=[[image(), image(det=[(2, .9, 0, 0, 9, 9), (3, .8) + FAR]), image(gt=[(1, 0, 0, 9, 9), (3, 0, 0, 49, 49)])],
                                 [image(), image(gt=[(3, 0, 0, 39, 39)], det=[(3, .7, 0, 0, 39, 39), (2, .2, 0, 0, 9, 9)])]],
                        num_classes=4, first_gt_id=0)
    # the first batch after reset() holds GT boxes and not one detection (nothing above the score threshold, early in
    # pre-training); annotation 0 is its undetected class-1 box.  Batch 1, class 1: a TP of score .9 and a FAR FP of score .4
    c["gt_only_first_batch"] = dict(batches=[[image(gt=[(1, 0, 0, 9, 9)]), image(gt=[(2, 0, 0, 49, 49)])],
                                             [image(gt=[(1, 100, 0, 109, 9)], det=[(1, .9, 100, 0, 109, 9), (1, .4) + FAR])]],
                                    num_classes=3, first_gt_id=0)
    # a split with GT boxes and no detection at all, in two batches, the last image empty
    c["gt_only_split"] = dict(batches=[[image(gt=[(1, 0, 0, 9, 9)])], [image(gt=[(2, 0, 0, 49, 49), (1, 0, 0, 119, 119)]), image()]],
                              num_classes=3, first_gt_id=0)
    c["no_updates"] = dict(batches=[], num_classes=4, first_gt_id=0)
    return c


def _jittered(rng, n_gt, n_det, n_cls, size=600.):
    """GT boxes of random classes; detections = jittered GT boxes (sometimes of another class) plus noise boxes; scores in 1/64."""
    xy = rng.uniform(0, size - 20, (n_gt, 2))
    wh = rng.choice([8., 24., 60., 150.], (n_gt, 2)) * rng.uniform(.6, 1.4, (n_gt, 2))
    gt = np.concatenate([xy, xy + wh], 1).round()
    gcls = rng.randint(1, n_cls, n_gt)
    src = rng.randint(0, max(n_gt, 1), n_det)
    noise = rng.uniform(0, 1, n_det) < .3
    db = gt[src] + rng.normal(0, 1, (n_det, 4)) * (wh[src].mean(1, keepdims=True) * rng.choice([.02, .1, .3], (n_det, 1)))
    nxy = rng.uniform(0, size - 20, (n_det, 2))
    db[noise] = np.concatenate([nxy, nxy + rng.uniform(5, 200, (n_det, 2))], 1)[noise]
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2])
    dcls = np.where(rng.uniform(0, 1, n_det) < .85, gcls[src], rng.randint(1, n_cls, n_det))
    score = np.round(rng.uniform(0, 1, n_det) * 64) / 64
    return image(gt=np.concatenate([gcls[:, None], gt], 1), det=np.concatenate([dcls[:, None], score[:, None], db], 1))


def segment_case(chunk, tile, total):
    """Class c = 1..8 holds 1, 63, 64, 65, chunk-1, chunk, chunk+1, 3 chunk+7 counted records (chunk: the accumulate scan's step);
    the last image adds detections of class 8 beyond the cut of 100, which become uncounted records, until the record total is
    `total` (tile - 1, tile, tile + 1 for the radix sort's tile).  Two batches."""
    lengths = [1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]
    rng = np.random.RandomState(11)
    filler = total - sum(lengths)
    assert 0 < filler <= 900
    n_img = (max(lengths) - 100 + 99) // 100 + 1
    per_image = [[] for _ in range(n_img)]          # (class, count)
    for c, n in enumerate(lengths, 1):
        left = n
        if c == 8:
            per_image[n_img - 1].append((c, 100 + filler))
            left -= 100
        i = 0
        while left > 0:
            take = min(100, left)
            per_image[i].append((c, take))
            left -= take
            i += 1
    images = []
    for plan in per_image:
        gts, dets = [], []
        for c, n in plan:
            n_gt = min(max(n // 3, 1), 60)
            xy = rng.uniform(0, 900, (n_gt, 2)).round()
            wh = rng.choice([10., 40., 120.], (n_gt, 2))
            g = np.concatenate([xy, xy + wh], 1)
            gts += [(c,) + tuple(b) for b in g]
            src = rng.randint(0, n_gt, n)
            d = g[src] + rng.normal(0, 1, (n, 4)) * wh[src].mean(1, keepdims=True) * rng.choice([0., .05, .25], (n, 1))
            d[:, 2:] = np.maximum(d[:, 2:], d[:, :2])
            score = np.round(rng.uniform(0, 1, n) * 64) / 64
            dets += [(c, s) + tuple(b) for s, b in zip(score, d)]
        order = rng.permutation(len(dets))
        images.append(image(gt=gts, det=[dets[i] for i in order]))
    half = len(images) // 2
    return dict(batches=[images[:half], images[half:]], num_classes=9, first_gt_id=0)


def realistic_case():
    """64 images, 151 classes, 10-40 GT boxes and 80 detections per image, in four batches."""
    rng = np.random.RandomState(2024)
    images = [_jittered(rng, rng.randint(10, 41), 80, 151) for _ in range(64)]
    return dict(batches=[images[i:i + 16] for i in range(0, 64, 16)], num_classes=151, first_gt_id=0)


SCAN_CHUNK, SORT_TILE = 256, 2048       # det_eval.hip's kChunk and kSortTile (test_det_eval_gpu.py checks them against the library)


@functools.lru_cache(maxsize=None)
def cases():
    c = _hand_cases()
    for total in (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1):
        c["segments_%d" % total] = segment_case(SCAN_CHUNK, SORT_TILE, total)
    c["realistic"] = realistic_case()
    return c


def flat_images(case):
    return [im for batch in case["batches"] for im in batch]


@functools.lru_cache(maxsize=None)
def expected(name):
    """np_coco_eval of the case, computed once and shared (read-only)."""
    case = cases()[name]
    out = np_coco_eval(flat_images(case), case["num_classes"], case["first_gt_id"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
