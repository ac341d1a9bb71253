"""Portable synthetic inputs and weights for the VETO relation-prediction path.

Everything here is produced by a counter-based integer hash (splitmix64) with
exact IEEE arithmetic on top, so the same tensors are regenerated bit-for-bit on
any machine (this container, the GPU box) from a (seed, name) pair alone.  The
golden fixtures in tests/golden/ only hold the *outputs* the reference produced
for these tensors; the 70 MB of weights never need to be committed.

Shapes and ranges follow SURVEY.md section 8(d) ("Synthetic inputs").
"""
import hashlib
import math

import numpy as np

_MASK = (1 << 64) - 1


def _name_key(seed, name):
    h = hashlib.sha256(("%d/%s" % (seed, name)).encode()).digest()
    return int.from_bytes(h[:8], "little")


def _splitmix64(x):
    """Vectorised splitmix64 finaliser on uint64 arrays (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform01(seed, name, n, stream=0):
    """n doubles in [0,1): (hash >> 11) * 2**-53, exact."""
    key = np.uint64((_name_key(seed, name) + 0x632BE59BD9B4E019 * stream) & _MASK)
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + key
    bits = _splitmix64(ctr)
    return (bits >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def uniform(seed, name, shape, lo, hi):
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, name, n)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def normal(seed, name, shape, mean=0.0, std=1.0):
    """Approximate N(mean, std): centred sum of four uniforms (Irwin-Hall), which
    needs no libm call and is therefore bit-portable."""
    n = int(np.prod(shape)) if len(shape) else 1
    s = np.zeros(n, dtype=np.float64)
    for k in range(4):
        s += uniform01(seed, name, n, stream=k + 1)
    z = (s - 2.0) * 1.7320508075688772  # var(sum of 4 U) = 1/3
    return (mean + std * z).astype(np.float32).reshape(shape)


def integers(seed, name, shape, lo, hi):
    """Integers in [lo, hi)."""
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, name, n)
    return (lo + np.floor(u * (hi - lo))).astype(np.int64).reshape(shape)


# ---------------------------------------------------------------------------
# Weights: one entry per state-dict key of the reference VETOPredictor
# (roi_relation_predictors.py:3999-4071; key list in SURVEY.md section 8b).
# ---------------------------------------------------------------------------

def _linear(sd, seed, prefix, out_f, in_f, bias=True):
    b = 1.0 / math.sqrt(in_f)
    sd[prefix + ".weight"] = uniform(seed, prefix + ".weight", (out_f, in_f), -b, b)
    if bias:
        sd[prefix + ".bias"] = uniform(seed, prefix + ".bias", (out_f,), -b, b)


def transformer_state_dict(seed, prefix, dim=576, layers=6, in_channels=256, patch=2):
    """Keys of VETOTransformer (model_veto.py:6-146) under `prefix`."""
    sd = {}
    t = prefix + "transformer."
    sd[t + "cls_token"] = normal(seed, t + "cls_token", (1, 1, dim))
    sd[t + "pos_embedding"] = normal(seed, t + "pos_embedding", (1, 1, dim))
    pdim = in_channels * 2 * patch * patch
    _linear(sd, seed, t + "patch_embed.proj_d", 512, pdim)
    _linear(sd, seed, t + "patch_embed.proj_v", 64, pdim)
    for l in range(layers):
        a = t + "layers.%d.0." % l
        f = t + "layers.%d.1." % l
        sd[a + "norm.weight"] = normal(seed, a + "norm.weight", (dim,), 1.0, 0.1)
        sd[a + "norm.bias"] = normal(seed, a + "norm.bias", (dim,), 0.0, 0.1)
        _linear(sd, seed, a + "fn.to_qkv", 3 * dim, dim, bias=False)
        _linear(sd, seed, a + "fn.to_out.0", dim, dim)
        sd[f + "norm.weight"] = normal(seed, f + "norm.weight", (dim,), 1.0, 0.1)
        sd[f + "norm.bias"] = normal(seed, f + "norm.bias", (dim,), 0.0, 0.1)
        _linear(sd, seed, f + "fn.net.0", 2 * dim, dim)
        _linear(sd, seed, f + "fn.net.3", dim, 2 * dim)
    return sd


def trunk_state_dict(seed, prefix="", dim=576, layers=6, num_obj_cls=151, embed_dim=200, patch=2):
    """Everything VETOPredictor and the MEET Ensemble share (all keys but rel_out)."""
    sd = {}
    sd[prefix + "obj_embed2.weight"] = normal(seed, prefix + "obj_embed2.weight", (num_obj_cls, embed_dim))
    sd[prefix + "obj_embed.weight"] = normal(seed, prefix + "obj_embed.weight", (num_obj_cls, embed_dim), 0.0, 0.5)
    _linear(sd, seed, prefix + "class_projection.0", dim, 2 * embed_dim)
    _linear(sd, seed, prefix + "bbox_embed.0", 32, 9)
    _linear(sd, seed, prefix + "bbox_embed.3", 128, 32)
    p = prefix + "pos_embed.0."
    sd[p + "weight"] = normal(seed, p + "weight", (4,), 1.0, 0.1)
    sd[p + "bias"] = normal(seed, p + "bias", (4,), 0.0, 0.1)
    # running statistics in pixel units (boxes are un-normalised)
    sd[p + "running_mean"] = (np.array([250.0, 200.0, 110.0, 110.0], dtype=np.float32)
                              + normal(seed, p + "running_mean", (4,), 0.0, 5.0))
    sd[p + "running_var"] = (np.array([20000.0, 15000.0, 3500.0, 3500.0], dtype=np.float32)
                             * uniform(seed, p + "running_var", (4,), 0.8, 1.2))
    sd[p + "num_batches_tracked"] = np.array(1000, dtype=np.int64)
    _linear(sd, seed, prefix + "pos_embed.1", 128, 4)
    _linear(sd, seed, prefix + "location_projection.0", dim, 256)
    sd.update(transformer_state_dict(seed, prefix + "fusion_transformer.", dim=dim, layers=layers, patch=patch))
    return sd


def predictor_state_dict(seed, dim=576, layers=6, num_obj_cls=151, num_rel_cls=51, patch=2):
    """Full state dict of the vanilla VETOPredictor."""
    sd = trunk_state_dict(seed, "", dim, layers, num_obj_cls, patch=patch)
    std = math.sqrt(2.0 / (dim + num_rel_cls))  # xavier_normal_, utils/miscellaneous.py
    sd["rel_out.weight"] = normal(seed, "rel_out.weight", (num_rel_cls, dim), 0.0, std)
    sd["rel_out.bias"] = uniform(seed, "rel_out.bias", (num_rel_cls,), -0.04, 0.04)
    sd["criterion_loss_rel.weight"] = np.ones((num_rel_cls,), dtype=np.float32)
    return sd


def meet_state_dict(seed, group_sizes, dim=576, layers=6, num_obj_cls=151, experts=0, patch=2):
    """State dict of VETOPredictor_MEET (everything lives under `model.`).  experts=3 gives the
    ENSEMBLE_LEARNING.EXPERT_GROUP layout: `model.rel_out_group.{e}.{k}` for 3 experts x K groups, with
    `model.rel_out.{k}` the same tensors as the LAST expert's (roi_relation_predictors.py:3717-3723
    leaves `self.rel_out` bound to the last list it appended)."""
    sd = trunk_state_dict(seed, "model.", dim, layers, num_obj_cls, patch=patch)
    del sd["model.obj_embed2.weight"]  # Ensemble has no obj_embed2 (roi_relation_predictors.py:3676)

    def head(name, g):
        std = math.sqrt(2.0 / (dim + g + 2))
        sd[name + ".weight"] = normal(seed, name + ".weight", (g + 2, dim), 0.0, std)
        sd[name + ".bias"] = uniform(seed, name + ".bias", (g + 2,), -0.04, 0.04)

    if experts:
        for e in range(experts):
            for k, g in enumerate(group_sizes):
                head("model.rel_out_group.%d.%d" % (e, k), g)
        for k in range(len(group_sizes)):
            for part in (".weight", ".bias"):
                sd["model.rel_out.%d%s" % (k, part)] = sd["model.rel_out_group.%d.%d%s" % (experts - 1, k, part)]
    else:
        for k, g in enumerate(group_sizes):
            head("model.rel_out.%d" % k, g)
    return sd


# ---------------------------------------------------------------------------
# Inputs: B images x N boxes.
# ---------------------------------------------------------------------------

def synthetic_batch(seed, num_images, num_objs, num_obj_cls=151, channels=256, res=8,
                    relu_like=False, patch=None, resolution=None):
    """Returns a dict of numpy arrays; `num_objs` may be an int or a per-image list.  The ROI maps are res x res; `resolution=`
    (POOLER_RESOLUTION) overrides `res`, and `patch=` (PATCH_SIZE) alone asks for the 4 x 4 patch grid's 4 * patch."""
    if resolution is None and patch is not None:
        resolution = 4 * patch
    if resolution is not None:
        res = int(resolution)
    if isinstance(num_objs, int):
        num_objs = [num_objs] * num_images
    total = int(sum(num_objs))
    xy = uniform(seed, "boxes.xy", (total, 2), 0.0, 400.0)
    wh = uniform(seed, "boxes.wh", (total, 2), 10.0, 210.0)
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)  # xyxy
    labels = integers(seed, "labels", (total,), 1, num_obj_cls)
    pred_labels = integers(seed, "pred_labels", (total,), 1, num_obj_cls)
    predict_logits = normal(seed, "predict_logits", (total, num_obj_cls))
    rgb = normal(seed, "roi_features", (total, channels, res, res))
    depth = normal(seed, "roi_depth_features", (total, channels, res, res))
    if relu_like:
        rgb = (0.5 * np.abs(rgb)).astype(np.float32)
        depth = (0.5 * np.abs(depth)).astype(np.float32)
    return {
        "num_objs": list(num_objs), "image_size": (800, 600), "boxes": boxes, "labels": labels,
        "pred_labels": pred_labels, "predict_logits": predict_logits,
        "roi_features": rgb, "roi_depth_features": depth,
    }


# ---------------------------------------------------------------------------
# Evaluation inputs: ground truth + sorted predictions per image.
# ---------------------------------------------------------------------------

def synthetic_eval_images(seed, num_objs, mode="predcls", num_rel_cls=51, num_obj_cls=21):
    """Per image: GT boxes / classes / relation tuples and a PostProcessor-shaped prediction (pairs sorted by
    triple score, [P, num_rel_cls] probabilities, object labels / scores).  Division-only arithmetic (no
    libm), so the arrays are bit-portable.  Near-duplicate boxes with equal classes make some predictions
    match a GT relation through a DIFFERENT box index (IoU >= 0.5), and a fraction of the GT predicates is
    boosted so that recall is neither 0 nor 1.  Also returns a zero-shot triplet table [Z, 3]
    (subject class, object class, predicate) that holds part of the GT triplets."""
    images, zs_rows = [], []
    for i, n in enumerate(num_objs):
        tag = "eval.%d." % i
        xy = uniform(seed, tag + "xy", (n, 2), 0.0, 300.0)
        wh = uniform(seed, tag + "wh", (n, 2), 30.0, 160.0)
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        classes = integers(seed, tag + "cls", (n,), 1, num_obj_cls)
        dup = uniform01(seed, tag + "dup", n)
        src = integers(seed, tag + "dupsrc", (n,), 0, max(n, 1))
        jit = uniform(seed, tag + "jit", (n, 4), -6.0, 6.0)
        for k in range(1, n):                     # ~30 %: a jittered copy of an earlier box, same class
            if dup[k] < 0.3:
                j = int(src[k]) % k
                boxes[k] = boxes[j] + jit[k]
                classes[k] = classes[j]
        pairs = np.array([(a, b) for a in range(n) for b in range(n) if a != b], dtype=np.int64).reshape(-1, 2)
        P = len(pairs)
        n_gt = int(min(P, 3 + integers(seed, tag + "ngt", (1,), 0, 22)[0] + (40 if n >= 15 else 0)))
        order = np.argsort(uniform01(seed, tag + "gtsel", P), kind="stable")[:n_gt]
        u = uniform01(seed, tag + "gtpred", n_gt)
        gt_pred = (1 + np.floor((u * u * np.sqrt(u)) * (num_rel_cls - 1))).astype(np.int64)   # skewed towards the head classes
        gt_rels = np.concatenate([pairs[order], gt_pred[:, None]], 1)
        if n_gt > 2:                              # a repeated pair with another predicate
            extra = gt_rels[:1].copy()
            extra[0, 2] = 1 + (extra[0, 2] % (num_rel_cls - 1))
            gt_rels = np.concatenate([gt_rels, extra], 0)
        w = uniform01(seed, tag + "w", P * num_rel_cls).reshape(P, num_rel_cls)
        w = w * w * w
        boost = uniform01(seed, tag + "boost", len(gt_rels))
        row_of = {(int(a), int(b)): r for r, (a, b) in enumerate(pairs)}
        for g, (s, o, r) in enumerate(gt_rels):
            if boost[g] < 0.65:
                w[row_of[(int(s), int(o))], int(r)] += 1.0 + 2.0 * boost[g]
        rel_scores = (w / w.sum(1, keepdims=True)).astype(np.float32)
        if mode == "predcls":
            pred_classes = classes.copy()
            obj_scores = np.ones(n, dtype=np.float32)
        else:
            flip = uniform01(seed, tag + "flip", n) < 0.2
            alt = integers(seed, tag + "alt", (n,), 1, num_obj_cls)
            pred_classes = np.where(flip, alt, classes)
            obj_scores = uniform(seed, tag + "objs", (n,), 0.3, 1.0)
        triple = rel_scores[:, 1:].max(1) * obj_scores[pairs[:, 0]] * obj_scores[pairs[:, 1]]
        srt = np.argsort(-triple, kind="stable")
        images.append({
            "gt_rels": gt_rels.astype(np.int64), "gt_classes": classes.astype(np.int64), "gt_boxes": boxes,
            "pred_rel_inds": pairs[srt], "rel_scores": rel_scores[srt], "pred_classes": pred_classes.astype(np.int64),
            "pred_boxes": boxes.copy(), "obj_scores": obj_scores,
        })
        zsel = uniform01(seed, tag + "zs", len(gt_rels)) < 0.35
        for (s, o, r) in gt_rels[zsel]:
            zs_rows.append((classes[s], classes[o], r))
    filler = integers(seed, "eval.zs_filler", (40, 3), 1, num_obj_cls)
    filler[:, 2] = 1 + filler[:, 2] % (num_rel_cls - 1)
    zeroshot = np.concatenate([np.array(zs_rows, dtype=np.int64).reshape(-1, 3), filler.astype(np.int64)], 0)
    return images, zeroshot


def synthetic_relation_targets(seed=41, num_objs=(6, 40, 3, 1), num_rel_cls=51):
    """(boxes [n, 4], relation matrix [n, n]) per image for the training-time relation sampler: random predicate matrices,
    one image with more foreground pairs than the positive budget, one with a single object (no candidate pair)."""
    out = []
    for i, n in enumerate(num_objs):
        boxes = uniform(seed, "rs.boxes.%d" % i, (n, 4), 0.0, 300.0)
        u = uniform01(seed, "rs.rel.%d" % i, n * n).reshape(n, n)
        lab = integers(seed, "rs.lab.%d" % i, (n, n), 1, num_rel_cls)
        rel = np.where(u < (0.5 if n >= 30 else 0.15), lab, 0)
        np.fill_diagonal(rel, 0)
        out.append((boxes, rel.astype(np.int64)))
    return out


# ---- ROI feature extraction fixtures ------------------------------------------------
def roi_test_boxes(rng, n, W, H):
    """n xyxy boxes on a W x H image: log-uniform sizes, some starting outside, and four fixed corner cases
    (the whole image, mostly outside, sub-pixel, malformed x2 < x1)."""
    xy = rng.uniform(-20, [W * 0.9, H * 0.9], size=(n, 2))
    wh = np.exp(rng.uniform(np.log(2), np.log(max(W, H) * 1.2), size=(n, 2)))
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    b[0] = [0, 0, W - 1, H - 1]
    b[1] = [W - 3, H - 3, W + 40, H + 40]
    b[2] = [30.2, 40.7, 30.3, 40.8]
    b[3] = [50, 60, 40, 30]
    return b


ROI_SINGLE_CASES = [(8, 2), (7, 2), (8, 1), (4, 4), (6, 0)]   # (pooled, sampling_ratio); 0 = adaptive grid (veto_roi_pool_adaptive)
# the pairs the ROI pooling suite added to the same fixture file (every kernel instance, full axis tables, mostly idle waves); a list of
# its own, so that a test written against ROI_SINGLE_CASES keeps reading the keys it was written for
ROI_SINGLE_CASES_MORE = [(8, 3), (8, 4), (5, 3), (3, 4), (2, 1), (1, 1), (1, 4)]


def synthetic_roi_single(pooled, ratio, channels=37):
    """One feature map [2, channels, 50, 84] at scale 1/16 and 23 ROI rows (image index, x1, y1, x2, y2)."""
    rng = np.random.RandomState(pooled * 10 + ratio)
    feat = rng.randn(2, channels, 50, 84).astype(np.float32)
    boxes = roi_test_boxes(rng, 23, 84 * 16, 50 * 16)
    rois = np.concatenate([rng.randint(0, 2, size=(23, 1)).astype(np.float32), boxes], 1)
    return feat, rois


def synthetic_roi_pyramid(channels=256, num_objs=(9, 17, 5), W=1024, H=640, seed=11):
    """Four FPN levels (strides 4..32) + a stride-16 depth map for 3 images, and per-image xyxy boxes that cover all four levels."""
    rng = np.random.RandomState(seed)
    feats = [rng.randn(len(num_objs), channels, H >> (2 + l), W >> (2 + l)).astype(np.float32) for l in range(4)]
    depth = rng.randn(len(num_objs), channels, H >> 4, W >> 4).astype(np.float32)
    boxes = [roi_test_boxes(rng, n, W, H) for n in num_objs]
    return feats, depth, boxes, (W, H)


# ---------------------------------------------------------------------------
# sgdet: detector outputs for the detected-box path (object decoding, test pairs)
# ---------------------------------------------------------------------------

def synthetic_detections(seed, n, num_obj_cls=151, W=800, H=600, spread=1.0):
    """One image of n detections in clusters, as a detector hands them to the relation head: per-class regressed boxes
    `boxes_per_cls` [n, C, 4] xyxy (the detection's box plus a small per-class jitter), `predict_logits` [n, C] that favour
    the cluster's class (so the class-aware NMS really suppresses), `pred_labels`, `pred_scores` and the proposal `boxes`.
    spread > 1 gives every detection a cluster of its own and pulls the clusters apart (no overlaps)."""
    tag = "sgdet.%d.%d" % (n, num_obj_cls)
    k = n if spread > 1 else max(1, n // 6)
    cl = np.arange(n) if spread > 1 else integers(seed, tag + ".cluster", (n,), 0, k)
    cx = uniform(seed, tag + ".cx", (k,), 0.1 * W, 0.9 * W).astype(np.float64) * spread
    cy = uniform(seed, tag + ".cy", (k,), 0.1 * H, 0.9 * H).astype(np.float64) * spread
    bw = uniform(seed, tag + ".w", (k,), 40.0, 260.0).astype(np.float64)
    bh = uniform(seed, tag + ".h", (k,), 40.0, 220.0).astype(np.float64)
    jit = normal(seed, tag + ".jit", (n, 4), 0.0, 12.0).astype(np.float64)
    x1 = cx[cl] - bw[cl] / 2 + jit[:, 0]
    y1 = cy[cl] - bh[cl] / 2 + jit[:, 1]
    x2 = cx[cl] + bw[cl] / 2 + jit[:, 2]
    y2 = cy[cl] + bh[cl] / 2 + jit[:, 3]
    det = np.stack([x1, y1, x2, y2], 1)
    per_cls = normal(seed, tag + ".cls_jit", (n, num_obj_cls, 4), 0.0, 5.0).astype(np.float64)
    bpc = det[:, None, :] + per_cls
    lo = np.minimum(bpc[..., 0:2], bpc[..., 2:4] - 8.0)
    bpc = np.concatenate([np.maximum(lo, 0.0), np.maximum(bpc[..., 2:4], lo + 8.0)], -1)
    logits = normal(seed, tag + ".logits", (n, num_obj_cls), 0.0, 1.5).astype(np.float64)
    main = integers(seed, tag + ".main", (k,), 1, num_obj_cls)
    alt = integers(seed, tag + ".alt", (k,), 1, num_obj_cls)
    logits[np.arange(n), main[cl]] += uniform(seed, tag + ".boost", (n,), 2.0, 6.0)
    logits[np.arange(n), alt[cl]] += uniform(seed, tag + ".boost2", (n,), 1.0, 5.0)
    logits = logits.astype(np.float32)
    pred_labels = logits[:, 1:].argmax(1).astype(np.int64) + 1
    return {"boxes_per_cls": bpc.astype(np.float32), "predict_logits": logits, "pred_labels": pred_labels,
            "pred_scores": uniform(seed, tag + ".score", (n,), 0.05, 1.0),
            "boxes": bpc[np.arange(n), pred_labels].astype(np.float32), "image_size": (W, H)}


def synthetic_detections_iou_tie(num_obj_cls=151):
    """Three detections whose class-5 boxes overlap at IoU exactly 0.5 and 0.25 (nms_overlaps arithmetic, +1 convention):
    box 0 = [0, 0, 9, 9] (area 100), box 1 = [0, 0, 9, 4] (inter 50, union 100), box 2 = [0, 5, 9, 9] (IoU 0.5 with box 0,
    0 with box 1).  Class 5 wins every row, rows in decreasing order of confidence."""
    n, C = 3, num_obj_cls
    base = np.array([[0, 0, 9, 9], [0, 0, 9, 4], [0, 5, 9, 9]], np.float64)
    bpc = np.repeat(base[:, None, :], C, 1) + np.arange(C)[None, :, None] * 100.0 * (np.arange(C) != 5)[None, :, None]
    logits = np.zeros((n, C), np.float64)
    logits[:, 5] = [6.0, 5.0, 4.0]
    logits[:, 7] = 3.0
    return {"boxes_per_cls": bpc.astype(np.float32), "predict_logits": logits.astype(np.float32),
            "pred_labels": np.full(n, 5, np.int64), "pred_scores": np.array([0.9, 0.8, 0.7], np.float32),
            "boxes": base.astype(np.float32), "image_size": (16, 16)}


def synthetic_eval_images_sgdet(seed, num_objs, num_rel_cls=51):
    """sgdet evaluator inputs: the GT side of synthetic_eval_images(seed, num_objs, 'sgcls') with predictions on the
    detector's OWN objects -- a jittered copy of most GT boxes (shifts of up to a quarter of the box, so the IoUs with
    their GT box spread around 0.5), in shuffled order, plus a few spurious boxes; their count differs from the GT count.
    Pairs are all ordered pairs of predicted objects sorted by triple score."""
    base, zeroshot = synthetic_eval_images(seed, num_objs, "sgcls", num_rel_cls=num_rel_cls)
    images = []
    for i, im in enumerate(base):
        tag = "eval_sgdet.%d." % i
        gtb, gtc = im["gt_boxes"].astype(np.float64), im["gt_classes"]
        n = len(gtb)
        keep = np.nonzero(uniform01(seed, tag + "keep", n) < 0.8)[0]
        n_extra = int(integers(seed, tag + "extra", (1,), 1, 4)[0])
        wh = np.concatenate([gtb[:, 2:] - gtb[:, :2]] * 2, 1)
        shift = (uniform(seed, tag + "shift", (n, 4), -0.25, 0.25).astype(np.float64) * wh)[keep]
        boxes = gtb[keep] + shift
        xy = uniform(seed, tag + "xy", (n_extra, 2), 0.0, 300.0).astype(np.float64)
        ewh = uniform(seed, tag + "wh", (n_extra, 2), 30.0, 160.0).astype(np.float64)
        boxes = np.concatenate([boxes, np.concatenate([xy, xy + ewh], 1)], 0)
        src = np.concatenate([keep, -np.ones(n_extra, np.int64)])
        flip = uniform01(seed, tag + "flip", len(src)) < 0.15
        alt = integers(seed, tag + "alt", (len(src),), 1, 21)
        classes = np.where((src >= 0) & ~flip, gtc[np.maximum(src, 0)], alt)
        perm = np.argsort(uniform01(seed, tag + "perm", len(src)), kind="stable")
        boxes, classes, src = boxes[perm], classes[perm], src[perm]
        m = len(src)
        pairs = np.array([(a, b) for a in range(m) for b in range(m) if a != b], dtype=np.int64).reshape(-1, 2)
        w = uniform01(seed, tag + "w", len(pairs) * num_rel_cls).reshape(len(pairs), num_rel_cls) ** 3
        boost = uniform01(seed, tag + "boost", len(im["gt_rels"]))
        where = {int(s): k for k, s in enumerate(src) if s >= 0}
        row_of = {(int(a), int(b)): r for r, (a, b) in enumerate(pairs)}
        for g, (s, o, r) in enumerate(im["gt_rels"]):
            if boost[g] < 0.7 and int(s) in where and int(o) in where:
                w[row_of[(where[int(s)], where[int(o)])], int(r)] += 1.0 + 2.0 * boost[g]
        rel_scores = (w / w.sum(1, keepdims=True)).astype(np.float32)
        obj_scores = uniform(seed, tag + "objs", (m,), 0.3, 1.0)
        triple = rel_scores[:, 1:].max(1) * obj_scores[pairs[:, 0]] * obj_scores[pairs[:, 1]]
        srt = np.argsort(-triple, kind="stable")
        images.append({"gt_rels": im["gt_rels"], "gt_classes": gtc, "gt_boxes": im["gt_boxes"],
                       "pred_rel_inds": pairs[srt], "rel_scores": rel_scores[srt], "pred_classes": classes.astype(np.int64),
                       "pred_boxes": boxes.astype(np.float32), "obj_scores": obj_scores})
    return images, zeroshot


def synthetic_relsample_image(seed, n_gt, n_det, n_rel, num_obj_cls=151, num_rel_cls=51, max_copies=5, twin=False,
                              clutter_bg=0.6, n_extra_non_masked=3, W=800, H=600):
    """One training image for the detected-box relation sampler (detect_relsample): `n_gt` GT boxes with labels and a
    relation matrix of `n_rel` distinct ordered pairs, `relation_non_masked` = that matrix plus `n_extra_non_masked` more
    nonzero entries, and `n_det` detections: 0..max_copies jittered copies of every GT box (mostly with its label, so they
    match it at IoU > 0.5), then clutter anywhere, labelled 0 with probability `clutter_bg`; shuffled.  twin=True makes GT
    box 1 a shifted copy of box 0 with its label, so the copies of box 0 match both."""
    tag = "relsample.%d.%d.%d" % (n_gt, n_det, n_rel)
    cx = uniform(seed, tag + ".cx", (n_gt,), 0.1 * W, 0.9 * W).astype(np.float64)
    cy = uniform(seed, tag + ".cy", (n_gt,), 0.1 * H, 0.9 * H).astype(np.float64)
    bw = uniform(seed, tag + ".w", (n_gt,), 40.0, 260.0).astype(np.float64)
    bh = uniform(seed, tag + ".h", (n_gt,), 40.0, 220.0).astype(np.float64)
    gt = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    gt_lab = integers(seed, tag + ".gt_lab", (n_gt,), 1, num_obj_cls)
    if twin and n_gt > 1:
        gt[1] = gt[0] + np.array([6.0, 4.0, 6.0, 4.0])
        gt_lab[1] = gt_lab[0]
    copies = integers(seed, tag + ".copies", (n_gt,), 0, max_copies + 1)
    src = np.repeat(np.arange(n_gt), copies)[:n_det]
    m = len(src)
    jit = normal(seed, tag + ".jit", (m, 4), 0.0, 6.0).astype(np.float64)
    det = gt[src] + jit
    relabel = uniform01(seed, tag + ".relabel", m) < 0.15
    det_lab = np.where(relabel, integers(seed, tag + ".wrong", (m,), 0, num_obj_cls), gt_lab[src])
    k = n_det - m
    ccx = uniform(seed, tag + ".ccx", (k,), 0.0, W).astype(np.float64)
    ccy = uniform(seed, tag + ".ccy", (k,), 0.0, H).astype(np.float64)
    cw = uniform(seed, tag + ".cw", (k,), 20.0, 300.0).astype(np.float64)
    ch = uniform(seed, tag + ".ch", (k,), 20.0, 300.0).astype(np.float64)
    clutter = np.stack([ccx - cw / 2, ccy - ch / 2, ccx + cw / 2, ccy + ch / 2], 1)
    clutter_lab = np.where(uniform01(seed, tag + ".bg", k) < clutter_bg, 0, integers(seed, tag + ".clab", (k,), 1, num_obj_cls))
    boxes = np.concatenate([det, clutter], 0)
    labels = np.concatenate([det_lab, clutter_lab]).astype(np.int64)
    order = np.argsort(uniform01(seed, tag + ".shuffle", n_det), kind="stable")
    boxes, labels = boxes[order], labels[order]
    x1y1 = np.maximum(boxes[:, :2], 0.0)
    boxes = np.concatenate([x1y1, np.maximum(boxes[:, 2:], x1y1 + 4.0)], 1)

    def pick_pairs(name, count, exclude=()):
        flat = [f for f in np.argsort(uniform01(seed, name, n_gt * n_gt), kind="stable")
                if f // n_gt != f % n_gt and f not in exclude]
        return np.asarray(flat[:count], np.int64)

    rel = np.zeros(n_gt * n_gt, np.int64)
    chosen = pick_pairs(tag + ".rel", n_rel)
    rel[chosen] = integers(seed, tag + ".rel_lab", (len(chosen),), 1, num_rel_cls)
    non_masked = rel.copy()
    extra = pick_pairs(tag + ".extra", n_extra_non_masked, exclude=set(chosen.tolist()))
    non_masked[extra] = integers(seed, tag + ".extra_lab", (len(extra),), 1, num_rel_cls)
    return {"prp_boxes": boxes.astype(np.float32), "prp_labels": labels,
            "pred_scores": uniform(seed, tag + ".score", (n_det,), 0.05, 1.0),
            "tgt_boxes": gt.astype(np.float32), "tgt_labels": gt_lab.astype(np.int64),
            "relation": rel.reshape(n_gt, n_gt), "relation_non_masked": non_masked.reshape(n_gt, n_gt), "image_size": (W, H)}


def synthetic_box_sampling_image(seed, n_gt, n_det, num_obj_cls=151, n_attr=3, W=800, H=600):
    """One training image for the box head's sampler (FastRCNNSampling): the GT boxes and clustered detections of
    synthetic_relsample_image with the GT boxes appended to the proposals (as ADD_GTBOX_TO_PROPOSAL_IN_TRAIN does), GT labels
    and an `attributes` matrix [n_gt, n_attr]."""
    d = synthetic_relsample_image(seed, n_gt, n_det, min(2, n_gt * (n_gt - 1)), num_obj_cls=num_obj_cls, W=W, H=H)
    return {"prp_boxes": np.concatenate([d["prp_boxes"], d["tgt_boxes"]], 0), "tgt_boxes": d["tgt_boxes"],
            "tgt_labels": d["tgt_labels"], "image_size": (W, H),
            "attributes": integers(seed, "boxsample.attr.%d.%d" % (n_gt, n_det), (n_gt, n_attr), 0, 20)}


# ---------------------------------------------------------------------------
# sgdet box decoder: the box head's raw outputs, and boxes + scores for NMS alone
# ---------------------------------------------------------------------------

def _clustered_boxes(seed, tag, n, W, H, per_cluster=8):
    """n xyxy boxes in clusters on a jittered grid: boxes of one cluster overlap heavily (IoU mostly above 0.5), boxes of
    neighbouring clusters barely (what a detector's proposals around objects look like, scaled to the grid)."""
    k = max(1, n // per_cluster)
    gx = max(1, int(math.ceil(math.sqrt(k * W / float(H)))))
    gy = max(1, int(math.ceil(k / float(gx))))
    cw, ch = W / float(gx), H / float(gy)
    cell = np.arange(k)
    cx = (cell % gx + 0.5) * cw + uniform(seed, tag + ".cx", (k,), -0.15, 0.15).astype(np.float64) * cw
    cy = (cell // gx + 0.5) * ch + uniform(seed, tag + ".cy", (k,), -0.15, 0.15).astype(np.float64) * ch
    bw = uniform(seed, tag + ".w", (k,), 0.55, 0.95).astype(np.float64) * cw
    bh = uniform(seed, tag + ".h", (k,), 0.55, 0.95).astype(np.float64) * ch
    cl = integers(seed, tag + ".cluster", (n,), 0, k)
    jit = normal(seed, tag + ".jit", (n, 4), 0.0, 0.04).astype(np.float64)
    x1 = cx[cl] - bw[cl] / 2 + jit[:, 0] * bw[cl]
    y1 = cy[cl] - bh[cl] / 2 + jit[:, 1] * bh[cl]
    x2 = cx[cl] + bw[cl] / 2 + jit[:, 2] * bw[cl]
    y2 = cy[cl] + bh[cl] / 2 + jit[:, 3] * bh[cl]
    x1, y1 = np.clip(x1, 0.0, W - 3.0), np.clip(y1, 0.0, H - 3.0)
    x2, y2 = np.clip(np.maximum(x2, x1 + 2.0), 0.0, W - 1.0), np.clip(np.maximum(y2, y1 + 2.0), 0.0, H - 1.0)
    return np.stack([x1, y1, x2, y2], 1).astype(np.float32), cl


def synthetic_nms_boxes(seed, n, W=1333, H=800):
    """(boxes [n, 4] xyxy, scores [n]) for NMS alone: clustered boxes, scores distinct by construction (a random permutation
    of n slots of width 1/n, each with a jitter of less than half a slot)."""
    tag = "nms.%d" % n
    boxes, _ = _clustered_boxes(seed, tag, n, W, H)
    rank = np.argsort(np.argsort(uniform01(seed, tag + ".perm", n), kind="stable"), kind="stable")
    scores = ((rank + 0.25 + 0.5 * uniform01(seed, tag + ".u", n)) / max(n, 1)).astype(np.float32)
    return boxes, scores


def synthetic_box_head_outputs(seed, n, num_obj_cls=151, W=800, H=600, on_classes=(12, 36), marginal=2, cls_agnostic=False):
    """What the box head's predictor hands the PostProcessor for one image of n proposals: `proposals` [n, 4] xyxy in clusters,
    `class_logits` [n, C] and `box_regression` [n, 4C] ([n, 8] with cls_agnostic).  Per row, on_classes[0]..on_classes[1]
    classes (the cluster's favourites among them) carry logits in [3.2, 5], `marginal` more sit around the usual score
    threshold of 0.01 and the rest, the background included, lie below -1: a few dozen classes per row pass the threshold and
    the probabilities in between are sparse.  Regressions are of the size a trained head emits: shifts of ~6 % of the box,
    log-scale changes of ~8 % (after BBOX_REG_WEIGHTS (10, 10, 5, 5))."""
    C = num_obj_cls
    tag = "boxhead.%d.%d" % (n, C)
    proposals, cl = _clustered_boxes(seed, tag, n, W, H)
    k = int(cl.max()) + 1 if n else 1
    logits = uniform(seed, tag + ".off", (n, C), -6.0, -1.0).astype(np.float64)
    n_on = integers(seed, tag + ".n_on", (n,), on_classes[0], on_classes[1] + 1)
    # a class is "on" for a row when its (cluster, class) or (row, class) draw is small enough: clusters share favourites
    shared = uniform01(seed, tag + ".shared", k * C).reshape(k, C)[cl]
    own = uniform01(seed, tag + ".own", n * C).reshape(n, C)
    pick = np.minimum(shared, own * 2.0)
    pick[:, 0] = 2.0
    order = np.argsort(pick, axis=1, kind="stable")
    rank = np.argsort(order, axis=1, kind="stable")
    on = rank < n_on[:, None]
    marg = (rank >= n_on[:, None]) & (rank < n_on[:, None] + marginal)
    logits = np.where(on, uniform(seed, tag + ".on", (n, C), 3.2, 5.0).astype(np.float64), logits)
    logits = np.where(marg, uniform(seed, tag + ".marg", (n, C), 2.0, 3.6).astype(np.float64), logits)
    cols = 8 if cls_agnostic else 4 * C
    reg = normal(seed, tag + ".reg", (n, cols // 4, 4), 0.0, 1.0).astype(np.float64) * np.array([0.6, 0.6, 0.4, 0.4])
    return {"proposals": proposals, "class_logits": logits.astype(np.float32),
            "box_regression": reg.reshape(n, cols).astype(np.float32), "image_size": (W, H)}


# ---------------------------------------------------------------------------
# RPN proposal selection: anchors and the RPN head's raw outputs
# ---------------------------------------------------------------------------

def _cell_anchors(stride, sizes, aspect_ratios):
    """The A = len(aspect_ratios) * len(sizes) anchors of one cell, ratio-major: windows around the centre of the
    (0, 0, stride - 1, stride - 1) cell whose area is about size^2, with integer-rounded sides before scaling."""
    ctr = 0.5 * (stride - 1)
    out = []
    for ratio in aspect_ratios:
        w = float(np.round(np.sqrt(stride * stride / float(ratio))))
        h = float(np.round(w * ratio))
        for size in sizes:
            scale = float(size) / stride
            ws, hs = w * scale, h * scale
            out.append([ctr - 0.5 * (ws - 1), ctr - 0.5 * (hs - 1), ctr + 0.5 * (ws - 1), ctr + 0.5 * (hs - 1)])
    return np.asarray(out, np.float64)


def anchor_grid(sizes, strides, aspect_ratios, grid_sizes):
    """Per level l the [A * H * W, 4] xyxy float32 anchors of a (H, W) = grid_sizes[l] feature map with stride strides[l] and
    anchor size(s) sizes[l]: anchor (h * W + w) * A + a is cell anchor a shifted by (w, h) * stride."""
    out = []
    for size, stride, (H, W) in zip(sizes, strides, grid_sizes):
        cell = _cell_anchors(stride, size if isinstance(size, (tuple, list)) else (size,), aspect_ratios).astype(np.float32)
        sx = (np.arange(W, dtype=np.float32) * np.float32(stride))[None, :].repeat(H, 0).reshape(-1)
        sy = (np.arange(H, dtype=np.float32) * np.float32(stride))[:, None].repeat(W, 1).reshape(-1)
        shifts = np.stack([sx, sy, sx, sy], 1)
        out.append((shifts[:, None, :] + cell[None, :, :]).reshape(-1, 4).astype(np.float32))
    return out


def synthetic_rpn_outputs(seed, n_img, grid_sizes, A=3, W=800, H=608, peaks=6, background=-4.0, delta=(0.25, 0.25, 0.2, 0.2)):
    """What the RPN head hands its post-processor: per level `objectness` [n_img, A, H_l, W_l] logits and `box_regression`
    [n_img, 4A, H_l, W_l].  Every image has `peaks` objects; a cell's logits rise towards the nearest of them on every level (so
    anchors of neighbouring cells and of several levels compete in NMS) over a noisy background, and the regression deltas
    are small (shifts of a quarter of the anchor, log-scale changes of a fifth).  W, H: the image extent the peaks live in."""
    objectness, regression = [], []
    for l, (gh, gw) in enumerate(grid_sizes):
        tag = "rpn.%d.%dx%d" % (l, gh, gw)
        px = uniform(seed, "rpn.px", (n_img, peaks), 0.1, 0.9).astype(np.float64) * gw
        py = uniform(seed, "rpn.py", (n_img, peaks), 0.1, 0.9).astype(np.float64) * gh
        rad = uniform(seed, "rpn.rad", (n_img, peaks), 0.08, 0.2).astype(np.float64) * max(gw, gh) + 0.7
        ys, xs = np.mgrid[0:gh, 0:gw]
        d2 = (xs[None, None] + 0.5 - px[:, :, None, None]) ** 2 + (ys[None, None] + 0.5 - py[:, :, None, None]) ** 2
        bump = (7.0 / (1.0 + d2 / rad[:, :, None, None] ** 2)).max(1)                           # [n_img, gh, gw]
        noise = normal(seed, tag + ".noise", (n_img, A, gh, gw), 0.0, 1.0).astype(np.float64)
        objectness.append((background + bump[:, None] + noise).astype(np.float32))
        reg = normal(seed, tag + ".reg", (n_img, A, 4, gh, gw), 0.0, 1.0).astype(np.float64) * np.asarray(delta)[None, None, :, None, None]
        regression.append(reg.reshape(n_img, 4 * A, gh, gw).astype(np.float32))
    return {"objectness": objectness, "box_regression": regression}


# ---------------------------------------------------------------------------
# RPN training: GT boxes per image and the RPN head's raw outputs per level
# ---------------------------------------------------------------------------

def synthetic_rpn_training_batch(seed, image_sizes, level_shapes, n_gt, min_side=24.0, logit_std=2.0, delta_std=0.5):
    """What one RPN training step is given besides its anchors (anchor_grid): per image `tgt_boxes` [n_gt[i], 4] xyxy inside
    the image ((width, height) = image_sizes[i]; sides between min_side and 0.6 of the image's), per level (A, H, W) =
    level_shapes[l] `objectness` [n_img, A, H, W] logits and `box_regression` [n_img, 4A, H, W].  The deltas are of the size of
    the regression targets of matched anchors, so the smooth-L1 residuals fall on both sides of beta."""
    n_img = len(image_sizes)
    tgt = []
    for i, ((W, H), m) in enumerate(zip(image_sizes, n_gt)):
        tag = "rpntrain.%d.%d" % (i, m)
        w = uniform(seed, tag + ".w", (m,), min_side, 0.6 * W).astype(np.float64)
        h = uniform(seed, tag + ".h", (m,), min_side, 0.6 * H).astype(np.float64)
        x1 = uniform01(seed, tag + ".x", m) * (W - 1 - w)
        y1 = uniform01(seed, tag + ".y", m) * (H - 1 - h)
        tgt.append(np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32))
    objectness, regression = [], []
    for l, (A, H, W) in enumerate(level_shapes):
        tag = "rpntrain.%d.%dx%dx%d" % (l, A, H, W)
        objectness.append(normal(seed, tag + ".obj", (n_img, A, H, W), 0.0, logit_std))
        regression.append(normal(seed, tag + ".reg", (n_img, 4 * A, H, W), 0.0, delta_std))
    return {"tgt_boxes": tgt, "objectness": objectness, "box_regression": regression}
