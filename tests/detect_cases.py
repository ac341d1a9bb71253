"""Inputs of the detector-side parity suite (tests/test_detect_parity_gpu.py, premises in tests/test_detect_cases_host.py): every
NMS kernel instance and its boundaries, the IoU threshold to the last bit, the box decoder's branches and the RPN's selection
and merge, and the wrong restatements that must differ on them.  numpy only; seeded through veto_amd.synth or closed-form.

Expected values come from test_boxhead_host.np_nms / np_box_postprocess and test_rpn_host.np_rpn_proposals (float32, operation
for operation, pinned to the reference's fixtures).  Almost every case is exact by construction: zero regressions (expf(0) == 1),
integer or quarter-pixel coordinates, hand-chosen logits.  The seeded ones are decision-robust (the host test asserts it for the
seeds chosen here): no consulted IoU within 1e-5 of the NMS threshold, no probability within 1e-6 of SCORE_THRESH, no cut
between scores closer than 1e-6."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_boxhead_host import hand_built_image, np_box_postprocess, np_decode_boxes, np_nms, np_softmax  # noqa: E402
from test_rpn_host import CASES as RPN_FIXTURE_CASES, min_size_exact_inputs, np_rpn_proposals  # noqa: E402

from veto_amd import synth  # noqa: E402

F = np.float32
UP_HALF = np.nextafter(F(0.5), F(1))          # the float32 above 0.5
IOU_FORMS = ("contracted", "reassociated", "reciprocal", "float64")


# the names of the cases below, as literals: parametrising over them builds nothing at collection time
NMS_LAUNCH_NAMES = ("instances_256", "instances_257", "instances_1024", "instances_1025", "instances_6144", "ladder_perm_128",
                    "ladder_perm_1024", "ladder_perm_6144", "ladder_equal_128", "ladder_equal_1024", "ladder_equal_6144", "suppressor_w4_256",
                    "suppressor_w4_1024", "suppressor_w16_6144", "inblock_bits", "extremes_6144", "cap_33", "cap_32", "cap_1", "cap_by_index",
                    "signed_zero_ladder", "threshold_contracted", "threshold_reassociated", "threshold_reciprocal", "threshold_float64",
                    "threshold_half")
BOX_CASE_NAMES = ("instances_256", "instances_1024", "instances_1024_full", "instances_6144", "instances_6144_full", "agnostic_6144",
                  "shift_only", "pairs_half", "pairs_contracted", "pairs_reassociated", "pairs_reciprocal", "pairs_float64", "score_thresh_C2_at",
                  "score_thresh_C2_below", "score_thresh_C2_nodup_at", "score_thresh_C2_nodup_below", "score_thresh_C4_at",
                  "score_thresh_C4_below", "score_thresh_C4_nodup_at", "score_thresh_C4_nodup_below", "topn_bind", "topn_bind_nodup",
                  "class_major_wide", "class_major_wide_cut", "row_max_ties", "tie_flood")
RPN_CASE_NAMES = ("instances_256", "instances_257", "instances_1024", "instances_1025", "instances_6144", "post_cap_equal", "post_cap_below",
                  "post_cap_one", "pairs_half", "pairs_contracted", "pairs_reassociated", "pairs_reciprocal", "pairs_float64", "k_106_of_105",
                  "k_105_of_105", "k_104_of_105", "shift_only", "ties_fit", "ties_overflow", "signed_zero_fit", "signed_zero_overflow", "min_size_exact",
                  "merge_image_24", "merge_image_23", "merge_image_8", "merge_image_13", "merge_batch_11", "merge_batch_100")


def nms_instance(n):
    """The capacity instance launch_nms, launch_nms_fixed and launch_box_postprocess (nms.hip) choose for a largest segment,
    capacity or image of n boxes.  The one restatement of that rule in the tests."""
    return 256 if n <= 256 else 1024 if n <= 1024 else 6144


def all_nms_launches():
    return dict(nms_launches(), **threshold_launches())


# ---- boxes --------------------------------------------------------------------------------------------------------------

def grid_boxes(n, per_row=128, side=10, pitch=20):
    """n pairwise disjoint side x side boxes on a pitch-pixel grid (integer coordinates)."""
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side - 1, y + side - 1], 1).astype(F)


def ladder_boxes(n):
    """10 x 10 boxes 3 pixels apart: neighbours meet at IoU 70 / 130 > 0.5, second neighbours at 40 / 160 < 0.5."""
    x = 3.0 * np.arange(n)
    return np.stack([x, 0 * x, x + 9, 0 * x + 9], 1).astype(F)


def shifted(box, dx):
    return box + np.array([dx, 0, dx, 0], F)


def permutation(seed, tag, n):
    return np.argsort(synth.uniform01(seed, tag, n), kind="stable")


# ---- IoU in devIoU's order and in the four wrong forms --------------------------------------------------------------------

def iou_form(form, a, b):
    """IoU of the float32 boxes a [.., 4] (the kept one) and b [.., 4] -> float32.  'dev': nms.cu:13-21 operation for operation.
    'contracted': the denominator's product fused into the subtraction, fma(-w, h, sa + sb).  'reassociated': sa + (sb - inter).
    'reciprocal': inter * (1 / denominator).  'float64': everything in float64, rounded once at the end."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if form == "float64":
        a, b = a.astype(np.float64), b.astype(np.float64)
    t = a.dtype.type
    one, zero = t(1), t(0)
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + one, zero)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + one, zero)
    inter = w * h
    sa = (a[..., 2] - a[..., 0] + one) * (a[..., 3] - a[..., 1] + one)
    sb = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
    if form in ("dev", "float64"):
        return (inter / ((sa + sb) - inter)).astype(F)
    if form == "contracted":   # (the float64 product of two float32 is exact)
        den = ((sa + sb).astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(F)
        return inter / den
    if form == "reassociated":
        return inter / (sa + (sb - inter))
    assert form == "reciprocal"
    return inter * (one / ((sa + sb) - inter))


def score_order(scores, signed_zero=False):
    """Visiting order (score desc, index asc).  signed_zero: the wrong order that puts +0.0 before -0.0."""
    s = np.asarray(scores).astype(np.float64)
    if signed_zero:
        s = np.where((s == 0) & np.signbit(s), -1e-300, s)
    return np.lexsort((np.arange(len(s)), -s))


def nms_variant(boxes, scores, thr, form="dev", ge=False, skip_removed=True, signed_zero=False):
    """np_nms with switches; all off it IS np_nms (the host test asserts that on every case).  ge: suppress at IoU >= thr.
    skip_removed=False: a removed box still suppresses.  form: see iou_form."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    n = len(boxes)
    order = score_order(scores, signed_zero)
    b = boxes[order]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            if skip_removed:
                continue
        else:
            keep.append(order[i])
        iou = iou_form(form, b[i], b[i + 1:])
        removed[i + 1:] |= (iou >= F(thr)) if ge else (iou > F(thr))
    return np.sort(np.asarray(keep, np.int64))


def nms_replay(boxes, scores, thr):
    """The greedy pass once more, recording what the kernel's structure depends on: (order, the sorted ranks of the kept boxes in
    kept order, {rank of a suppressed box: [positions in the kept list of every kept box that suppresses it]})."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    order = score_order(scores)
    b = boxes[order]
    kept, by = [], {}
    for i in range(len(b)):
        hits = np.nonzero(iou_form("dev", b[np.asarray(kept, np.int64)], b[i]) > F(thr))[0].tolist() if kept else []
        if hits:
            by[i] = hits
        else:
            kept.append(i)
    return order, kept, by


# ---- 1. greedy NMS: launches of veto_nms ---------------------------------------------------------------------------------
# A launch: name, segs = [(boxes, scores), ...], thr, max_keep.  launch_nms picks the kernel instance by the largest segment.

NMS_SEEDS = {256: 5000, 257: 5100, 1024: 5200, 1025: 5300, 6144: 5400}   # first seed of a launch; segment j uses seed + j


def pack(launch):
    """(boxes [M, 4], scores [M], offsets [S + 1]) of a launch."""
    sizes = [len(s[0]) for s in launch["segs"]]
    boxes = np.concatenate([s[0].reshape(-1, 4) for s in launch["segs"]]).astype(F)
    scores = np.concatenate([s[1].reshape(-1) for s in launch["segs"]]).astype(F)
    return boxes, scores, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def seeded_segment(seed, n):
    if n == 0:
        return np.zeros((0, 4), F), np.zeros(0, F)
    return synth.synthetic_nms_boxes(seed, n)


def ladder_segment(n, mode, seed=77):
    """mode 'perm': index = a seeded permutation of the rank, scores distinct and falling with the rank.  'equal': one score, the
    index order is the visiting order.  'zeros': the same with scores alternating -0.0 / +0.0 (equal, as every documented order
    has it).  Returns (boxes, scores, the closed-form keep list: the even ranks)."""
    lad = ladder_boxes(n)
    if mode == "perm":
        perm = permutation(seed, "detect.ladder.%d" % n, n)
        boxes, scores = np.empty((n, 4), F), np.empty(n, F)
        boxes[perm], scores[perm] = lad, (n - np.arange(n)).astype(F)
        return boxes, scores, np.sort(perm[0::2]).astype(np.int64)
    scores = np.ones(n, F) if mode == "equal" else np.where(np.arange(n) % 2 == 0, F(-0.0), F(0.0)).astype(F)
    return lad, scores, np.arange(0, n, 2, dtype=np.int64)


def one_suppressor_segment(n, p):
    """n disjoint boxes with falling scores (all kept: kept position = index) and one last candidate that overlaps box p alone."""
    boxes = grid_boxes(n)
    scores = (n + 1 - np.arange(n)).astype(F)
    return np.concatenate([boxes, shifted(boxes[p], 3)[None]]), np.concatenate([scores, [F(0.5)]]).astype(F)


def inblock_segment(blocks_before, a, b):
    """64 (blocks_before + 1) disjoint boxes, falling scores; the box at lane b of the last 64-block overlaps the one at lane a."""
    n = 64 * (blocks_before + 1)
    boxes = grid_boxes(n)
    boxes[n - 64 + b] = shifted(boxes[n - 64 + a], 3)
    return boxes, (n + 1 - np.arange(n)).astype(F)


def chain_segment():
    """128 boxes; ranks 63, 64, 65 are a ladder across the block boundary: 63 kills 64, 64 would kill 65, 63 does not: 65 stays."""
    boxes = grid_boxes(128)
    boxes[64], boxes[65] = shifted(boxes[63], 3), shifted(boxes[63], 6)
    return boxes, (200 - np.arange(128)).astype(F)


SUPPRESSOR_FORMS = {"w4_256": (128, list(range(17)) + list(range(112, 128))),       # nms_kernel<256, 256>: 4 waves
                    "w4_1024": (320, list(range(17)) + list(range(304, 320))),      # nms_kernel<1024, 256>: 4 waves
                    "w16_6144": (1088, list(range(17)) + list(range(1072, 1088)))}  # nms_kernel<6144, 1024>: 16 waves
INBLOCK_BITS = ((0, 1), (0, 63), (62, 63), (31, 32))


@functools.lru_cache(None)
def nms_launches():
    out = {}
    for big in (256, 257, 1024, 1025, 6144):
        thr = 0.7 if big in (256, 1024) else 0.3
        segs = [seeded_segment(NMS_SEEDS[big] + j, n) for j, n in enumerate((big, 0, 1, 63, 64, 65))]
        out["instances_%d" % big] = dict(segs=segs, thr=thr, max_keep=-1, seeded=True)
    for mode in ("perm", "equal"):
        for sizes in ((64, 65, 128), (1024, 64), (6144, 65)):
            lad = [ladder_segment(n, mode) for n in sizes]
            out["ladder_%s_%d" % (mode, sizes[0] if sizes[0] > 64 else 128)] = dict(
                segs=[l[:2] for l in lad], thr=0.5, max_keep=-1, closed_form=[l[2] for l in lad])
    for name, (n, ps) in SUPPRESSOR_FORMS.items():
        out["suppressor_" + name] = dict(segs=[one_suppressor_segment(n, p) for p in ps], thr=0.5, max_keep=-1,
                                         closed_form=[np.arange(n, dtype=np.int64)] * len(ps), n=n, ps=ps)
    pairs = [(blk, a, b) for blk in (0, 1) for a, b in INBLOCK_BITS]
    out["inblock_bits"] = dict(segs=[inblock_segment(*p) for p in pairs] + [chain_segment()], thr=0.5, max_keep=-1, pairs=pairs,
                               closed_form=[np.delete(np.arange(64 * (blk + 1)), 64 * blk + b) for blk, a, b in pairs]
                               + [np.delete(np.arange(128), 64)])
    one = np.tile(np.array([[5, 7, 104, 86]], F), (6144, 1))
    out["extremes_6144"] = dict(segs=[(grid_boxes(6144), (7000 - np.arange(6144)).astype(F)), (one, np.ones(6144, F))], thr=0.5,
                                max_keep=-1, closed_form=[np.arange(6144, dtype=np.int64), np.zeros(1, np.int64)])
    lad = ladder_segment(65, "equal")
    for cap in (33, 32, 1):   # the ladder keeps 33, the disjoint grid 64, the single box 1
        out["cap_%d" % cap] = dict(segs=[lad[:2], (grid_boxes(64), np.ones(64, F)), (grid_boxes(1), np.ones(1, F))], thr=0.5, max_keep=cap,
                                   closed_form=[lad[2][:cap], np.arange(64)[:cap], np.zeros(1, np.int64)])
    # the cap is by index, not by score: survivors whose scores do not follow their indices (a permuted ladder, a permuted grid)
    lad = ladder_segment(65, "perm")
    grid_scores = (1 + permutation(78, "detect.cap.grid", 64)).astype(F)
    out["cap_by_index"] = dict(segs=[lad[:2], (grid_boxes(64), grid_scores)], thr=0.5, max_keep=10,
                               closed_form=[lad[2][:10], np.arange(10, dtype=np.int64)])
    z = [ladder_segment(n, "zeros") for n in (65, 300)]
    out["signed_zero_ladder"] = dict(segs=[s[:2] for s in z], thr=0.5, max_keep=-1, closed_form=[s[2] for s in z])
    return out


def expected_nms(launch, nms=np_nms):
    """Per segment the keep list (the cap applied: the first max_keep of the ascending list, boxlist_ops.py:29-30)."""
    out = []
    for boxes, scores in launch["segs"]:
        keep = nms(boxes, scores, launch["thr"])
        out.append(keep[:launch["max_keep"]] if launch["max_keep"] > 0 else keep)
    return out


# ---- 2. the threshold, to the last bit -----------------------------------------------------------------------------------

@functools.lru_cache(None)
def drawn_pairs(seed=91, n=4000):
    """n overlapping box pairs with coordinates on a 1 / 256-pixel grid in [0, 700) and sides of 8 .. 300 pixels: (a [n, 4],
    b [n, 4]).  Every coordinate, difference and translation by a multiple of 1024 below 2^14 is exact in float32; the products
    are not (on a quarter-pixel grid at these sizes they would be -- 21 bits -- and no form could differ from devIoU except
    through the division)."""
    G = 256.0
    q = lambda tag, lo, hi: synth.integers(seed, "detect.pairs." + tag, (n,), int(lo * G), int(hi * G) + 1).astype(np.float64) / G   # noqa: E731
    ax, ay, aw, ah = q("ax", 150, 400), q("ay", 150, 400), q("aw", 8, 300), q("ah", 8, 300)
    bw, bh = q("bw", 8, 300), q("bh", 8, 300)
    fx, fy = synth.uniform01(seed, "detect.pairs.fx", n), synth.uniform01(seed, "detect.pairs.fy", n)
    bx = np.round((ax - 0.5 * bw + (0.1 + 0.8 * fx) * 0.5 * (aw + bw)) * G) / G
    by = np.round((ay - 0.5 * bh + (0.1 + 0.8 * fy) * 0.5 * (ah + bh)) * G) / G
    a = np.stack([ax, ay, ax + aw - 1, ay + ah - 1], 1).astype(F)
    b = np.stack([bx, by, bx + bw - 1, by + bh - 1], 1).astype(F)
    return a, b


@functools.lru_cache(None)
def form_pairs(per_form=4):
    """Per wrong IoU form the first per_form drawn pairs on which it differs from devIoU, and the threshold that separates them
    on the first: the smaller of the two float32 values, so that under `>` exactly one of the two forms suppresses."""
    a, b = drawn_pairs()
    dev = iou_form("dev", a, b)
    out = {}
    for form in IOU_FORMS:
        other = iou_form(form, a, b)
        idx = np.nonzero((other != dev) & (dev > 0.05) & (dev < 0.95))[0][:per_form]
        out[form] = dict(a=a[idx], b=b[idx], dev=dev[idx], other=other[idx], thr=float(min(dev[idx[0]], other[idx[0]])))
    return out


def pair_segments(a, b):
    """Every pair its own 2-box segment, the first box scoring higher."""
    return [(np.stack([x, y]), np.array([0.9, 0.8], F)) for x, y in zip(a, b)]


@functools.lru_cache(None)
def half_pairs():
    """Integer pairs at IoU exactly 0.5: a 2a x h box against an a x h box inside it, and two 3a x h boxes overlapping by 2a."""
    a, b = [], []
    for i, (w, h, k) in enumerate(((5, 10, 0), (5, 10, 5), (7, 3, 2), (16, 16, 9), (1, 1, 1), (33, 21, 0), (100, 50, 37), (2, 9, 1))):
        ox, oy = 3.0 * i, 11.0 * i
        a.append([ox, oy, ox + 2 * w - 1, oy + h - 1])
        b.append([ox + k, oy, ox + k + w - 1, oy + h - 1])
        a.append([ox, oy, ox + 3 * w - 1, oy + h - 1])
        b.append([ox + w, oy, ox + 4 * w - 1, oy + h - 1])
    return np.asarray(a, F), np.asarray(b, F)


@functools.lru_cache(None)
def above_half_pairs(count=16):
    """Quarter-pixel pairs whose devIoU is the float32 just above 0.5.  The inner box lies inside the outer one, so IoU = I / U
    with the areas I = r s / 16 and U = p q / 16 (sides in quarter pixels); 2 r s = p q + 1 puts the quotient 1 / (2 p q) above
    one half, which rounds to 0.5 + 2^-24 for p q in (2^24 / 3, 2^24); p q + r s < 2^24 keeps every sum exact."""
    a, b = [], []
    for p in range(2401, 3300, 14):
        for q in range(p + 2, 3300, 2):
            m = (p * q + 1) // 2
            r = np.arange(-(-m // q), p + 1)
            r = r[m % r == 0]
            if len(r):
                r = int(r[len(r) // 2])
                s = m // r
                x0, y0 = float(len(a) % 7), float(len(a) % 5)
                dx, dy = ((p - r) // 2) / 4.0, ((q - s) // 2) / 4.0
                a.append([x0, y0, x0 + p / 4.0 - 1, y0 + q / 4.0 - 1])
                b.append([x0 + dx, y0 + dy, x0 + dx + r / 4.0 - 1, y0 + dy + s / 4.0 - 1])
                break
        if len(a) == count:
            break
    return np.asarray(a, F), np.asarray(b, F)


@functools.lru_cache(None)
def bulk_pairs():
    """(a, b, suppressed): the exact-0.5 pairs (both kept at threshold 0.5) followed by the just-above pairs (second suppressed)."""
    (ha, hb), (ua, ub) = half_pairs(), above_half_pairs()
    return np.concatenate([ha, ua]), np.concatenate([hb, ub]), np.concatenate([np.zeros(len(ha), bool), np.ones(len(ua), bool)])


@functools.lru_cache(None)
def threshold_launches():
    forms = form_pairs()
    a = np.concatenate([forms[f]["a"] for f in IOU_FORMS])
    b = np.concatenate([forms[f]["b"] for f in IOU_FORMS])
    out = {"threshold_" + f: dict(segs=pair_segments(a, b), thr=forms[f]["thr"], max_keep=-1) for f in IOU_FORMS}
    ba, bb, sup = bulk_pairs()
    out["threshold_half"] = dict(segs=pair_segments(ba, bb), thr=0.5, max_keep=-1,
                                 closed_form=[np.array([0] if s else [0, 1], np.int64) for s in sup])
    return out


# ---- the decoder (veto_box_postprocess) -------------------------------------------------------------------------------------

BOX_PRM = dict(score_thresh=0.05, nms=0.5, topn=300, filter_dup=True, det_per_img=100, weights=(10., 10., 5., 5.), cls_agnostic=False)
BOX_SEEDS = {"instances_256": 6000, "instances_1024": 6100, "instances_1024_full": 6200, "instances_6144": 6300,
             "instances_6144_full": 6450, "agnostic_6144": 6500, "shift_only": 6600}
BOX_SHAPES = {"instances_256": (3, (256, 0, 65)), "instances_1024": (4, (257, 0, 64, 63, 1)), "instances_1024_full": (3, (1024, 0, 1)),
              "instances_6144": (5, (1025, 0, 2000, 1)), "instances_6144_full": (3, (6144,)), "agnostic_6144": (4, (1100, 0, 300)),
              "shift_only": (3, (64, 200))}   # regressions that shift and do not scale: no expf result other than 1, compared bit for bit


def empty_image(C, cols):
    return {"proposals": np.zeros((0, 4), F), "class_logits": np.zeros((0, C), F), "box_regression": np.zeros((0, cols), F),
            "image_size": (800, 600)}


def seeded_box_case(name):
    C, sizes = BOX_SHAPES[name]
    agn = name.startswith("agnostic")
    imgs = []
    for j, n in enumerate(sizes):
        if n == 0:
            imgs.append(empty_image(C, 8 if agn else 4 * C))
            continue
        seed = BOX_SEEDS[name] + j
        d = synth.synthetic_box_head_outputs(seed, n, C, on_classes=(1, 1), marginal=0, cls_agnostic=agn)
        # clustered proposals and regressions as the box head emits them; logits uniform in [-2, 2], so that most rows are
        # candidates of every class (NMS segments of almost the image's size) with probabilities spread over (0.01, 0.96)
        d["class_logits"] = synth.uniform(seed, "detect.box.logits.%d.%d" % (n, C), (n, C), -2.0, 2.0)
        if name == "shift_only":
            d["box_regression"] = d["box_regression"].reshape(n, C, 4) * np.array([1, 1, 0, 0], F)
            d["box_regression"] = np.ascontiguousarray(d["box_regression"].reshape(n, 4 * C))
        imgs.append(d)
    return dict(imgs=imgs, prm=dict(BOX_PRM, cls_agnostic=agn), seeded=True, bitwise=name == "shift_only")


def exact_image(proposals, logits, size=(4000, 3000)):
    """Zero regressions: the decoder returns the proposals bit for bit (for every class)."""
    n, C = logits.shape
    return {"proposals": np.asarray(proposals, F), "class_logits": np.asarray(logits, F), "box_regression": np.zeros((n, 4 * C), F),
            "image_size": size}


def pairs_box_case(a, b, thr, pitch=1024.0):
    """The pairs as one image of C = 2: pair i translated by i * pitch pixels (exact: quarter pixels below 2^17), so that pairs do
    not meet; the first box of a pair scores higher.  SCORE_THRESH is far from every probability."""
    n = len(a)
    t = (np.arange(n) * pitch)[:, None] * np.array([1, 0, 1, 0])
    prop = np.stack([a + t, b + t], 1).reshape(-1, 4).astype(F)
    logits = np.zeros((2 * n, 2), F)
    logits[0::2, 1], logits[1::2, 1] = 2.0, 1.0
    return dict(imgs=[exact_image(prop, logits, (int(n * pitch + 2000), 4000))], prm=dict(BOX_PRM, nms=thr, det_per_img=0))


@functools.lru_cache(None)
def box_cases():
    out = {name: seeded_box_case(name) for name in BOX_SHAPES}
    ba, bb, _ = bulk_pairs()
    out["pairs_half"] = pairs_box_case(ba, bb, 0.5)
    for f, v in form_pairs().items():
        out["pairs_" + f] = pairs_box_case(v["a"], v["b"], v["thr"])
    # SCORE_THRESH exactly: equal logits, every probability exactly 1 / C on both sides
    for C in (2, 4):
        img = exact_image(grid_boxes(12, pitch=40, side=30), np.zeros((12, C), F))
        below = float(np.nextafter(F(1.0 / C), F(0)))
        for dup in (True, False):
            tag = "score_thresh_C%d%s" % (C, "" if dup else "_nodup")
            out[tag + "_at"] = dict(imgs=[img], prm=dict(BOX_PRM, score_thresh=1.0 / C, filter_dup=dup, det_per_img=0), n_det=0)
            out[tag + "_below"] = dict(imgs=[img], prm=dict(BOX_PRM, score_thresh=below, filter_dup=dup, det_per_img=0),
                                       n_det=12 if dup else 12 * (C - 1))
    # the reference-pinned branches (tests/golden/boxhead/topn_bind*.npz, class_major_wide*.npz), here inside a batch
    for dup in (True, False):
        out["topn_bind" + ("" if dup else "_nodup")] = dict(imgs=[hand_built_image("topn_bind", 2)] * 2,
                                                            prm=dict(BOX_PRM, score_thresh=0.01, nms=0.3, topn=3, filter_dup=dup, det_per_img=0))
    for cut in (0, 4):
        out["class_major_wide" + ("_cut" if cut else "")] = dict(imgs=[hand_built_image("class_major", 300), hand_built_image("class_major", 300)],
                                                                 prm=dict(BOX_PRM, score_thresh=0.01, nms=0.3, filter_dup=False, det_per_img=cut))
    # row_max ties, C = 151: rows whose two best columns carry the same logit; row 3 sits on row 4's box and loses column 5 to it
    C = 151
    prop = grid_boxes(6, pitch=60, side=40)
    prop[3] = prop[4]
    logits = np.full((6, C), -3.0, F)
    for r, (c1, c2) in enumerate(((5, 69), (70, 71), (1, 150), (5, 69))):
        logits[r, c1] = logits[r, c2] = 3.0
    logits[4, 5] = 4.0
    logits[5, 150] = 3.0
    out["row_max_ties"] = dict(imgs=[exact_image(prop, logits)], prm=dict(BOX_PRM, score_thresh=0.01, nms=0.3, det_per_img=0),
                               labels=[5, 70, 1, 69, 5, 150])
    # tie flood at the cut: DETECTIONS_PER_IMG = 5; rows 0-1 score higher, rows 2-16 share the cut score, rows 17-19 score lower
    logits = np.zeros((20, 3), F)
    logits[:2, 1], logits[2:17, 2], logits[17:, 1] = (3.0, 2.5), 2.0, 1.0
    out["tie_flood"] = dict(imgs=[exact_image(grid_boxes(20, pitch=40, side=30), logits)] * 2, prm=dict(BOX_PRM, det_per_img=5), n_det=17)
    return out


def box_variant(d, prm, topn_by_score=False, ge_score=False, last_col=False, dtype=F):
    """np_box_postprocess with switches; all off it IS np_box_postprocess (exact quantities; the host test asserts that on every
    case).  topn_by_score: POST_NMS_PER_CLS_TOPN keeps the best-scored survivors.  ge_score: candidates at prob >= SCORE_THRESH.
    last_col: the last of the tied best columns of a row."""
    C = d["class_logits"].shape[1]
    prob = np_softmax(d["class_logits"].astype(dtype)).astype(dtype)
    dec = np_decode_boxes(d["box_regression"], d["proposals"], d["image_size"], prm["weights"], C, prm["cls_agnostic"], dtype)
    thr = dtype(prm["score_thresh"])
    alive = np.zeros(prob.shape, bool)
    for j in range(1, C):
        inds = np.nonzero(prob[:, j] >= thr if ge_score else prob[:, j] > thr)[0]
        if len(inds) == 0:
            continue
        keep = np_nms(dec[inds, j], prob[inds, j], prm["nms"], dtype)
        if prm["topn"] > 0:
            keep = np.sort(keep[score_order(prob[inds[keep], j])[:prm["topn"]]]) if topn_by_score else keep[:prm["topn"]]
        alive[inds[keep], j] = True
    if prm["filter_dup"]:
        dist = np.where(alive, prob, dtype(0))
        scores = dist.max(1)
        labels = C - 1 - dist[:, ::-1].argmax(1) if last_col else dist.argmax(1)
        rows = np.nonzero(scores)[0]
        scores, labels = scores[rows], labels[rows]
    else:
        labels, rows = np.nonzero(alive[:, 1:].T)
        labels = labels + 1
        scores = prob[rows, labels]
    cap = prm["det_per_img"]
    if 0 < cap < len(rows):
        keep = np.nonzero(scores >= np.sort(scores)[len(rows) - cap])[0]
        rows, labels = rows[keep], labels[keep]
    return {"orig_inds": rows.astype(np.int64), "pred_labels": labels.astype(np.int64)}


@functools.lru_cache(None)
def expected_box(name):
    """Per image (float32 restatement, float64 restatement, diag32, diag64), computed once and left unchanged."""
    case = box_cases()[name]
    out = []
    for d in case["imgs"]:
        d32, d64 = {}, {}
        out.append((np_box_postprocess(d, case["prm"], F, d32), np_box_postprocess(d, case["prm"], np.float64, d64), d32, d64))
    return out


def box_case_robust(name):
    """The generators' rule for a seeded decoder case: float32 and float64 agree on every exact quantity, and no decision is
    within rounding: consulted IoUs 1e-5 off the threshold, probabilities 1e-6 off SCORE_THRESH, no equal scores inside an NMS
    segment, 1e-6 between the scores on either side of the cut."""
    prm = box_cases()[name]["prm"]
    for r32, r64, d32, d64 in expected_box(name):
        ok = np.array_equal(r32["orig_inds"], r64["orig_inds"]) and np.array_equal(r32["pred_labels"], r64["pred_labels"])
        for dg in (d32, d64):
            ok &= not np.any(np.abs(dg["consulted"].astype(np.float64) - prm["nms"]) < 1e-5)
            ok &= not np.any(np.abs(dg["prob"].astype(np.float64) - prm["score_thresh"]) < 1e-6)
            ok &= not dg["seg_ties"] and dg["cut_gap"] >= 1e-6
        if not ok:
            return False
    return True


def nms_launch_robust(launch):
    """The same rule for a seeded veto_nms launch."""
    for boxes, scores in launch["segs"]:
        c32, c64 = [], []
        k32, k64 = np_nms(boxes, scores, launch["thr"], F, c32), np_nms(boxes, scores, launch["thr"], np.float64, c64)
        near = any(np.any(np.abs(c.astype(np.float64) - launch["thr"]) < 1e-5) for c in c32 + c64)
        if near or not np.array_equal(k32, k64) or len(np.unique(scores)) != len(scores):
            return False
    return True


# ---- the RPN (veto_rpn_proposals) -------------------------------------------------------------------------------------------
# A case: d = anchors / objectness / box_regression (lists over the levels, as test_rpn_host.case_inputs), c = the settings.

def plane(values, A, H, W):
    """[n_img, A H W] logits in anchor order ((h W + w) A + a) -> the RPN head's [n_img, A, H, W]."""
    v = np.asarray(values, F).reshape(-1, H, W, A)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def one_level(anchors, values, A, H, W):
    n_img = np.asarray(values).reshape(-1, A * H * W).shape[0]
    return {"anchors": [np.asarray(anchors, F)], "objectness": [plane(values, A, H, W)],
            "box_regression": [np.zeros((n_img, 4 * A, H, W), F)]}


def settings(images, pre, post, thr, min_size=0, fpn=None, **kw):
    return dict(images=tuple(images), pre=pre, post=post, fpn=fpn if fpn is not None else max(post, 1), thr=thr, min_size=min_size, **kw)


def paired_row_anchors(n):
    """Anchor j = 10 x 10 at x = 20 (j // 2) + 3 (j % 2): the two anchors of a pair meet at IoU 70 / 130, pairs are disjoint."""
    j = np.arange(n)
    x = 20.0 * (j // 2) + 3.0 * (j % 2)
    return np.stack([x, 0 * x, x + 9, 0 * x + 9], 1).astype(F)


RPN_INSTANCES = {256: ((1, 16, 16), 300), 257: ((1, 1, 257), 6000), 1024: ((3, 23, 16), 1024), 1025: ((3, 23, 16), 1025),
                 6144: ((3, 64, 32), 6144)}


def rpn_instance_case(cap, post=2000):
    """nms_fixed_kernel at capacity `cap` = min(pre, A H W).  One level of paired anchors, zero regressions, distinct logits in a
    seeded permutation, min_size 10 = the anchors' side: an image's width decides how many anchors lie inside it untouched; the
    clipped ones fall below min_size.  Live counts per image: the capacity, then 0, 1, 63, 64, 65.  Where pre < A H W (capacities
    1024 and 1025: the radix path) the narrow images lift the logits of their first 66 anchors by 4, above everything else of the
    plane, so that every anchor inside the image is among the pre selected; among themselves they stay permuted."""
    (A, H, W), pre = RPN_INSTANCES[cap]
    N = A * H * W
    anchors = paired_row_anchors(N)
    x2 = anchors[:, 2]
    assert np.all(np.diff(x2) > 0)   # anchor j is the j-th from the left: an image of m anchors holds anchors 0 .. m - 1
    lives = (N, 0, 1, 63, 64, 65)
    images = [(int(x2[m - 1]) + 1 if m else 5, 10) for m in lives]
    values = np.stack([(permutation(300 + i, "detect.rpn.inst.%d" % cap, N) - N // 2) / 512.0 for i in range(len(lives))])
    if pre < N:
        values[1:, :66] += 4.0
    return dict(d=one_level(anchors, values, A, H, W), c=settings(images, pre, post, 0.5, min_size=10), capacity=min(pre, N))


def pairs_rpn_case(a, b, thr, pitch=1024.0):
    """The pairs as one level of 2 n anchors (A = 1, one row of cells), pair i translated by i * pitch; zero regressions."""
    n = len(a)
    t = (np.arange(n) * pitch)[:, None] * np.array([1, 0, 1, 0])
    anchors = np.stack([a + t, b + t], 1).reshape(-1, 4).astype(F)
    values = (2 * n - np.arange(2 * n)).astype(F)[None]
    return dict(d=one_level(anchors, values, 1, 1, 2 * n), c=settings([(int(n * pitch + 2000), 4000)], 2 * n, 2 * n, thr))


def tie_plane(seed, N, n_gt, n_eq, tie=1.0):
    """N logits in anchor order: n_gt distinct values above `tie`, n_eq equal to it, the rest distinct below, at seeded places."""
    perm = permutation(seed, "detect.rpn.tie.%d" % N, N)
    v = np.empty(N, F)
    v[perm[:n_gt]] = tie + 1 + np.arange(n_gt) / 8.0
    v[perm[n_gt:n_gt + n_eq]] = tie
    v[perm[n_gt + n_eq:]] = tie - 1 - np.arange(N - n_gt - n_eq) / 8.0
    return v


def merge_levels(n_img, logits0, logits1):
    """Two levels of 12 disjoint anchors (A = 1, 3 x 4 cells; level 1 lies 200 pixels lower), zero regressions."""
    a0 = grid_boxes(12, per_row=4, side=20, pitch=40)
    a1 = a0 + np.array([0, 200, 0, 200], F)
    return {"anchors": [a0, a1], "objectness": [plane(logits0, 1, 3, 4), plane(logits1, 1, 3, 4)],
            "box_regression": [np.zeros((n_img, 4, 3, 4), F)] * 2}


@functools.lru_cache(None)
def rpn_cases():
    out = {}
    for cap in RPN_INSTANCES:
        out["instances_%d" % cap] = rpn_instance_case(cap)
    full = np_rpn_proposals(out["instances_256"]["d"], out["instances_256"]["c"])
    survivors = len(full[0]["boxes"])
    for post in (survivors, survivors - 1, 1):   # POST_NMS_TOP_N equal to the survivor count of image 0, one below it, and 1
        out["post_cap_%s" % ("equal" if post == survivors else "below" if post > 1 else "one")] = rpn_instance_case(256, post)
    ba, bb, _ = bulk_pairs()
    out["pairs_half"] = pairs_rpn_case(ba, bb, 0.5)
    for f, v in form_pairs().items():
        out["pairs_" + f] = pairs_rpn_case(v["a"], v["b"], v["thr"])
    # both sides of k >= N: A H W = 3 * 5 * 7 = 105 is no multiple of 4, images 1 and 2 start 4 and 8 bytes off alignment
    anchors = synth.anchor_grid((32,), (8,), (0.5, 1.0, 2.0), ((5, 7),))[0]
    values = np.stack([(permutation(400 + i, "detect.rpn.kn", 105) - 52) / 4.0 for i in range(3)])
    for pre in (106, 105, 104):
        out["k_%d_of_105" % pre] = dict(d=one_level(anchors, values, 3, 5, 7), c=settings([(64, 48)] * 3, pre, 1000, 0.7))
    # regressions that shift and do not scale (dw = dh = 0): BoxCoder.decode without an expf result other than 1, bit for bit
    anchors = synth.anchor_grid((32,), (8,), (0.5, 1.0, 2.0), ((10, 12),))[0]
    values = np.stack([(permutation(450 + i, "detect.rpn.shift", 360) - 180) / 8.0 for i in range(2)])
    d = one_level(anchors, values, 3, 10, 12)
    reg = synth.normal(451, "detect.rpn.shift.reg", (2, 3, 4, 10, 12), 0.0, 0.25) * np.array([1, 1, 0, 0], F)[None, None, :, None, None]
    d["box_regression"] = [np.ascontiguousarray(reg.reshape(2, 12, 10, 12).astype(F))]
    out["shift_only"] = dict(d=d, c=settings([(96, 80)] * 2, 200, 100, 0.7), bitwise=True)
    # ties at the pre-NMS cut that fit the LDS sort: 600 anchors, k = 100, 300 tied, n_gt = 0 / 50 / 99 (one image each)
    values = np.stack([tie_plane(500 + i, 600, n_gt, 300) for i, n_gt in enumerate((0, 50, 99))])
    out["ties_fit"] = dict(d=one_level(grid_boxes(600), values, 3, 10, 20), c=settings([(4000, 4000)] * 3, 100, 0, 0.0), n_gt=(0, 50, 99))
    # ties that overflow it: 3 * 67 * 61 = 12 261 anchors (48 per thread, the last threads short), 3000 / 2999 above 9000 tied, k = 6000
    values = np.stack([tie_plane(600, 12261, 3000, 9000), tie_plane(601, 12261, 2999, 9000)])
    out["ties_overflow"] = dict(d=one_level(grid_boxes(12261), values, 3, 67, 61), c=settings([(4000, 4000)] * 2, 6000, 0, 0.0))
    # signed zeros: planes alternating -0.0 / +0.0 with the cut inside (fits the sort; overflows it)
    for name, (A, H, W), k in (("signed_zero_fit", (3, 8, 8), 50), ("signed_zero_overflow", (3, 67, 61), 6000)):
        N = A * H * W
        z = np.where(np.arange(N) % 2 == 0, F(-0.0), F(0.0)).astype(F)   # alternating in plane order; image 1 the other way round
        d = one_level(grid_boxes(N), np.zeros((2, N), F), A, H, W)
        d["objectness"] = [np.stack([z, -z]).reshape(2, A, H, W).astype(F)]
        out[name] = dict(d=d, c=settings([(4000, 4000)] * 2, k, 0, 0.0), first_k=k)
    out["min_size_exact"] = dict(d=min_size_exact_inputs(), c=dict(RPN_FIXTURE_CASES["min_size_exact"]))
    # the merge over the levels, per image: equal logits across the levels on either side of FPN_POST_NMS_TOP_N
    l0 = [5, 4, 3, 2, 2, 2, 1, 1, 1, .5, .25, -7]   # (the two -7 meet at the cut of 23)
    l1 = [4.5, 2, 2, 1, 1, -1, -2, -3, -4, -5, -6, -7]
    d = merge_levels(2, [l0, l1[::-1]], [l1, l0[::-1]])
    for fpn in (24, 23, 8, 13):
        out["merge_image_%d" % fpn] = dict(d=d, c=settings([(400, 400)] * 2, 12, 12, 0.5, fpn=fpn))
    # ... and per batch (training): 6 distinct logits above 12 equal ones spread over 3 images x 2 levels, need = 5 of them
    lv = lambda hi: [hi, 2, 2] + [-1 - i for i in range(9)]   # noqa: E731
    d = merge_levels(3, [lv(9), lv(7), lv(5)], [lv(8), lv(6), lv(4)])
    for fpn in (11, 100):
        out["merge_batch_%d" % fpn] = dict(d=d, c=settings([(400, 400)] * 3, 12, 12, 0.5, fpn=fpn, training=True, per_batch=True))
    return out


@functools.lru_cache(None)
def expected_rpn(name):
    """(float32 restatement, float64 restatement, diag32), computed once and left unchanged."""
    case = rpn_cases()[name]
    diag = {}
    return np_rpn_proposals(case["d"], case["c"], F, diag), np_rpn_proposals(case["d"], case["c"], np.float64), diag


def rpn_variant(d, c, signed_zero=False, highest_anchor=False, gt_min_size=False):
    """np_rpn_proposals for one level with switches; all off it IS np_rpn_proposals (level and anchor_index; the host test asserts
    that on every one-level case).  signed_zero: +0.0 before -0.0.  highest_anchor: ties at the pre-NMS cut go to the highest
    anchor index.  gt_min_size: remove_small_boxes keeps sides > min_size."""
    assert len(d["objectness"]) == 1
    obj, reg, anc = d["objectness"][0], d["box_regression"][0], d["anchors"][0]
    A, H, W = obj.shape[1:]
    out = []
    for i, size in enumerate(c["images"]):
        x = obj[i].transpose(1, 2, 0).reshape(-1)
        k = min(c["pre"], len(x))
        s = x.astype(np.float64)
        if signed_zero:
            s = np.where((s == 0) & np.signbit(s), -1e-300, s)
        idx = np.arange(len(x))
        order = np.lexsort((-idx if highest_anchor else idx, -s))[:k]
        r = reg[i].reshape(A, 4, H, W).transpose(2, 3, 0, 1).reshape(-1, 4)[order]
        box = np_decode_boxes(r, anc[order], size, (1., 1., 1., 1.), 1, False, F)[:, 0]
        ws, hs = box[:, 2] - box[:, 0] + F(1), box[:, 3] - box[:, 1] + F(1)
        m = F(c["min_size"])
        ok = np.nonzero((ws > m) & (hs > m) if gt_min_size else (ws >= m) & (hs >= m))[0]
        box, order = box[ok], order[ok]
        if c["thr"] > 0:
            keep = np_nms(box, x[order], c["thr"])
            if c["post"] > 0:
                keep = keep[:c["post"]]
            order = order[keep]
        out.append(dict(anchor_index=order.astype(np.int64)))
    return out
