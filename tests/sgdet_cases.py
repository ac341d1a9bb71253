"""Inputs of the sgdet parity suite (tests/test_sgdet_parity_gpu.py, premises in tests/test_sgdet_cases_host.py): the branches,
limits and ties of obj_decode_kernel and prepare_pairs_kernel (veto_amd/csrc/sgdet.hip) that the reference fixtures and the
random 256 x 201 images never reach, and instrumented restatements that count the events each case is named for.

Expected values come from test_sgdet_host.np_decode / np_pairs (float32, operation for operation, pinned to the reference's
fixtures).  decode_trace and pairs_trace are those two loops again with counters; the host test holds them equal to the originals.

Decode cases (a case is a list of launches; a launch is (images, thr)):
  zero_max_post / zero_max_meet  one tight cluster, C in {2, 3, 5}, n in {4, 8, 70}: steps whose global maximum is 0, re-picks of
                      picked rows, MEET labels overwritten by a re-pick, never-picked rows; a variant zeroes two columns of a
                      picked row in descending column order
  row_ties_post       identical logit rows (0, 65, 130 of 140) and equal logits inside a row (c, c + 64, c + 128; c, c + 3, c + 67)
  class_edges         C in {2, 63, 64, 65, 128, 129, 1024}, n in {1, 5, 30}
  lds_boundary        n * C on both sides of the 30720 cells that fit in LDS
  mixed_homes         one launch: workspace image, LDS image, empty image, n = 1, second workspace image; a second launch with
                      workspace images eight workgroups apart
Random parts are drawn as test_sgdet_gpu._robust_detections draws them: a draw is rejected when the fp32 and fp64 restatements
disagree on a label or a consulted IoU lies within 1e-6 of the threshold.  The hand-made tie cases must also keep every step's
maximum at least 1e-4 (relative) above the largest strictly smaller cell: 100 times the 1e-6 to which the device softmax is
held, so only exact ties -- identical inputs -- can be decided by rounding.

Pair cases (a case is a list of (images, cap, require_overlap)):
  caps, cap_edges, straddle, zero_scores, touching, word_edges -- see the builders.

`python tests/sgdet_cases.py` prints the premises and gaps recorded in profiles/sgdet_parity.txt."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sgdet_host import np_decode, np_nms_iou, np_onehot_prob, np_overlap, np_softmax  # noqa: E402

from veto_amd import synth  # noqa: E402

F = np.float32
LDS_CELLS = 30720                 # kProbLds of sgdet.hip: the probability matrix lives in LDS up to this many cells
MIN_GAP = 1e-4
IOU_MARGIN = 1e-6

MODES = ("post", "meet")
DECODE_CASE_NAMES = ("zero_max_post", "zero_max_meet", "row_ties_post", "class_edges", "lds_boundary", "mixed_homes")
HAND_MADE = ("zero_max_post", "zero_max_meet", "row_ties_post")
PAIR_CASE_NAMES = ("caps", "cap_edges", "straddle", "zero_scores", "touching", "word_edges")
GOLDEN_DECODE = ("zero_max_post", "zero_max_meet", "row_ties_post")          # cases with reference outputs in tests/golden/sgdet/
GOLDEN_PAIRS = ("caps", "cap_edges", "straddle", "touching")


# ---- instrumented restatements ----------------------------------------------------------------------------------------

def decode_trace(prob, boxes_per_cls, thr, mode="post"):
    """np_decode with counters.  Returns (labels, steps, never_picked): a step holds the global maximum `max`, the largest
    strictly smaller cell `second` (None when there is none), `at_max` cells equal to the maximum, `row`, `col`, `repick` (the
    row had been picked before), `overwritten` (a re-pick wrote the label), `changed` (to another value) and `kept` ("post": a
    re-pick at another column left a non-zero label alone), `revived` (picked
    rows whose -1 row got its first 0) and `lower_col` (picked rows at maximum 0 that got a 0 in an earlier column), and the
    consulted IoUs `iou`."""
    p = np.array(prob, F, copy=True)
    bpc = np.asarray(boxes_per_cls, F)
    n = p.shape[0]
    p[:, 0] = 0.0 if mode == "post" else -1.0
    label = np.zeros(n, np.int64)
    picked = np.zeros(n, bool)
    thr32 = F(thr)
    steps = []
    for _ in range(n):
        b, c = np.unravel_index(int(p.argmax()), p.shape)
        m = p[b, c]
        below = p[p < m]
        st = {"max": float(m), "second": float(below.max()) if below.size else None, "at_max": int((p == m).sum()),
              "row": int(b), "col": int(c), "repick": bool(picked[b]), "overwritten": False, "changed": False,
              "kept": bool(picked[b]) and mode == "post" and label[b] != 0 and label[b] != c}
        if mode == "meet" or label[b] == 0:
            st["overwritten"] = bool(picked[b])
            st["changed"] = bool(picked[b]) and label[b] != c
            label[b] = c
        iou = np_nms_iou(bpc[b, c], bpc[:, c])
        hit = iou >= thr32
        others = hit & picked & (np.arange(n) != b) & (p[:, c] != 0)
        rmax = p.max(1)
        st["revived"] = int((others & (rmax == -1)).sum())
        st["lower_col"] = int((others & (rmax == 0) & (p.argmax(1) > c)).sum())
        st["iou"] = iou
        p[hit, c] = 0.0
        p[b] = -1.0
        picked[b] = True
        steps.append(st)
    return label, steps, np.flatnonzero(~picked)


def step_gap(st):
    """Relative distance of a step's maximum to the largest strictly smaller cell; inf for a maximum <= 0 (exact values)."""
    if st["max"] <= 0 or st["second"] is None:
        return np.inf
    return (st["max"] - st["second"]) / st["max"]


def decode_summary(d, thr, mode):
    """The counters of one image in one mode, summed over its steps."""
    C = d["predict_logits"].shape[1]
    prob = np_softmax(d["predict_logits"]) if mode == "post" else np_onehot_prob(d["pred_labels"], C)
    label, steps, never = decode_trace(prob, d["boxes_per_cls"], thr, mode)
    iou = np.concatenate([s["iou"] for s in steps]) if steps else np.zeros(0)
    out = {"labels": label, "zero_steps": sum(s["max"] == 0 for s in steps), "repicks": sum(s["repick"] for s in steps),
           "overwritten": sum(s["overwritten"] for s in steps), "changed": sum(s["changed"] for s in steps),
           "revived": sum(s["revived"] for s in steps), "lower_col": sum(s["lower_col"] for s in steps),
           "never_picked": len(never), "gap": min([step_gap(s) for s in steps], default=np.inf),
           "kept": sum(s["kept"] for s in steps),
           "iou_margin": float(np.abs(iou.astype(np.float64) - F(thr)).min()) if iou.size else np.inf,
           # exact ties at a positive maximum: between rows, inside the picked row, and inside it across lanes (col % 64 differs)
           "row_ties": 0, "col_ties": 0, "lane_ties": 0}
    p = np.array(prob, F, copy=True)
    p[:, 0] = 0.0 if mode == "post" else -1.0
    for s in steps:     # ties of the first pick of every row, on the unsuppressed matrix: exact by construction or not at all
        if s["max"] <= 0 or s["repick"]:
            continue
        cols = np.flatnonzero(p[s["row"]] == F(s["max"]))
        if len(cols) > 1 and cols[0] == s["col"]:
            out["col_ties"] += 1
            out["lane_ties"] += int(len(set(cols % 64)) > 1)
        out["row_ties"] += int(((p == F(s["max"])).any(1)).sum() > 1)
    return out


def pairs_trace(boxes, scores, cap, require_overlap):
    """np_pairs with counters: total, and above the cap the cut quality T, the count above it, the tie group's size, `need`
    (how many of the group are taken), and the rows and waves (row // 64) of the group's members."""
    n = len(boxes)
    cand = ~np.eye(n, dtype=bool)
    if require_overlap and n:
        cand &= np_overlap(boxes)
    idx = np.argwhere(cand).astype(np.int64).reshape(-1, 2)
    out = {"total": len(idx), "capped": len(idx) > cap}
    if out["capped"]:
        s = np.asarray(scores, F)
        q = s[idx[:, 0]] * s[idx[:, 1]]
        order = np.argsort(-q, kind="stable")
        T = q[order[cap - 1]]
        rows = idx[q == T][:, 0]
        out.update(T=float(T), above=int((q > T).sum()), group=int((q == T).sum()), rows=rows,
                   waves=sorted(set((rows // 64).tolist())), qualities=q)
        out["need"] = cap - out["above"]
        out["taken_waves"] = sorted(set((rows[:out["need"]] // 64).tolist()))
    return out


# ---- decode: images ---------------------------------------------------------------------------------------------------

def _image(bpc, logits, size=(800, 600)):
    logits = np.asarray(logits, F)
    bpc = np.asarray(bpc, F)
    n = len(logits)
    lab = logits[:, 1:].argmax(1).astype(np.int64) + 1 if n else np.zeros(0, np.int64)
    return {"boxes_per_cls": bpc, "predict_logits": logits, "pred_labels": lab,
            "pred_scores": np.full(n, 0.5, F), "boxes": bpc[np.arange(n), lab], "image_size": size}


def empty_image(C):
    return _image(np.zeros((0, C, 4), F), np.zeros((0, C), F))


def cluster_boxes(seed, tag, n, C):
    """One tight cluster: a 201 x 201 box moved by at most 3 pixels per (row, class) -- every same-class IoU is above 0.9."""
    j = synth.uniform(seed, tag + ".jit", (n, C, 4), -3.0, 3.0)
    return np.array([100, 100, 300, 300], F)[None, None, :] + j


def apart_boxes(n, C):
    """Pairwise disjoint boxes, the same for every class: nothing is suppressed."""
    i = np.arange(n)
    b = np.stack([(i % 16) * 40, (i // 16) * 40, (i % 16) * 40 + 19, (i // 16) * 40 + 19], 1).astype(F)
    return np.repeat(b[:, None, :], C, 1)


def robust(d, thr, gap=None, modes=("post", "meet")):
    """The draw conditions: fp32 and fp64 restatements agree on every label, no consulted IoU within 1e-6 of the threshold,
    and with `gap` every step's maximum at least that far (relative) above the largest strictly smaller cell."""
    C = d["predict_logits"].shape[1]
    if not len(d["predict_logits"]):
        return True
    for mode in modes:
        s = decode_summary(d, thr, mode)
        if mode == "post":
            l64 = np_decode(np_softmax(d["predict_logits"].astype(np.float64)), d["boxes_per_cls"].astype(np.float64), thr, mode)
            if not np.array_equal(s["labels"], l64):
                return False
        if s["iou_margin"] < IOU_MARGIN or (gap is not None and s["gap"] < gap):
            return False
    return True


def robust_detections(seed, n, C, thr):
    """synth.synthetic_detections of the first seed (seed, seed + 50, ...) that passes robust()."""
    for s in range(seed, seed + 50 * 40, 50):
        d = synth.synthetic_detections(s, n, C)
        if robust(d, thr):
            return d
    raise AssertionError("no robust seed near %d for %d x %d" % (seed, n, C))


def cluster_image(seed, n, C, thr):
    """A tight cluster with seeded logits; drawn again until robust, in both modes, with the hand-made cases' gap."""
    for s in range(seed, seed + 50 * 40, 50):
        tag = "sgdet_cases.cluster.%d.%d" % (n, C)
        d = _image(cluster_boxes(s, tag, n, C), synth.normal(s, tag + ".logits", (n, C), 0.0, 2.0))
        if robust(d, thr, MIN_GAP):
            return d
    raise AssertionError("no robust cluster near %d for %d x %d" % (seed, n, C))


def descending_image(n=8):
    """C = 5: row 0 is picked at column 4, then rows 1, 2 and 3 at columns 3, 2 and 1 zero those columns of the picked row 0 in
    descending order, and every later step has maximum 0: row 0 comes back at column 1 (`c < rc`, twice).  MEET labels: the
    reference's softmax of a one-hot row gives a 1 in column 1 a hot value one ulp above a 1 elsewhere (its row sum adds in
    another order), so no row is labelled 1 and the rows still unpicked at step 4 all carry label 4 -- equal cold values."""
    C = 5
    logits = np.full((n, C), -2.0, F)
    logits[0, 4], logits[1, 3], logits[2, 2] = 6.0, 5.0, 4.0
    logits[3:, 1] = 3.0 - 0.25 * np.arange(n - 3)
    logits[3:, 4] = 1.0
    d = _image(cluster_boxes(7, "sgdet_cases.descending", n, C), logits)
    d["pred_labels"] = np.array([4, 3, 2] + [4] * (n - 3), np.int64)
    d["boxes"] = d["boxes_per_cls"][np.arange(n), d["pred_labels"]]
    return d


@functools.lru_cache(None)
def zero_max():
    """[(images, thr)]: one launch per C holding the n = 4, 8, 70 clusters, and the descending-column variant.  zero_max_post and
    zero_max_meet are these images in the two modes (logits in one, their arg-max labels in the other)."""
    out = []
    for C in (2, 3, 5):
        out.append(([cluster_image(9000 + C, n, C, 0.5) for n in (4, 8, 70)], 0.5))
    out.append(([descending_image(8)], 0.5))
    return out


@functools.lru_cache(None)
def row_ties_post():
    """n = 140, C = 201, disjoint boxes (nothing suppressed, every row keeps its first maximum).  Rows 0, 65 and 130 are one
    logit row; rows 1, 66 and 131 another.  Rows 0.. tie at columns 9, 73 and 137 (one lane, three strides); rows 1.. at
    columns 5, 8 and 72 (three lanes: a butterfly without the column rule would answer 8).  A second image of the same rows
    sits in one tight cluster, so a suppressed row falls to its next tied column."""
    n, C = 140, 201
    for seed in range(31, 71):
        base = synth.normal(seed, "sgdet_cases.row_ties", (n, C), 0.0, 1.0)
        logits = base.copy()
        a = base[0].copy()
        a[[9, 73, 137]] = 5.0
        b = base[1].copy()
        b[[5, 8, 72]] = 5.0
        logits[[0, 65, 130]] = a
        logits[[1, 66, 131]] = b
        for r in range(2, n):                              # every other row: its own distinct winner, well below the tied rows
            if r not in (65, 66, 130, 131):
                logits[r, 1 + (r * 7) % (C - 1)] = 3.0 + 0.01 * r
        loose = _image(apart_boxes(n, C), logits)
        tight = _image(cluster_boxes(seed, "sgdet_cases.row_ties.tight", 20, C), logits[[0, 1, 65, 66, 130, 131] + list(range(2, 16))])
        if robust(loose, 0.5, MIN_GAP) and robust(tight, 0.5, MIN_GAP):
            return [([loose, tight], 0.5)]
    raise AssertionError("no robust row-tie draw")


@functools.lru_cache(None)
def class_edges():
    return [([robust_detections(9100 + C + n, n, C, 0.5) for n in (1, 5, 30)], 0.5) for C in (2, 63, 64, 65, 128, 129, 1024)]


LDS_BOUNDARY_SHAPES = (((256, 120),), ((255, 121), (253, 121), (256, 121)), ((240, 128), (241, 128)))


@functools.lru_cache(None)
def lds_boundary():
    """One launch per C.  256 x 120 and 240 x 128 are exactly 30720 cells (LDS); 255 x 121, 256 x 121 and 241 x 128 are their
    nearest neighbours in the workspace, 253 x 121 the nearest LDS neighbour of 255 x 121 (254 x 121 = 30734 is still outside)."""
    return [([robust_detections(9300 + n + C, n, C, 0.3) for n, C in launch], 0.3) for launch in LDS_BOUNDARY_SHAPES]


MIXED_HOMES_N = (256, 10, 0, 1, 200)
SAME_XCD_N = (200, 1, 2, 0, 3, 1, 2, 1, 256, 4, 1, 0, 2, 1, 3, 1, 230)


@functools.lru_cache(None)
def mixed_homes():
    """Launch 0: workspace, LDS, empty, n = 1, workspace.  Launch 1: workspace images at workgroups 0, 8 and 16 with small LDS
    images between them -- workgroups go round the chip's eight XCDs in turn, each with an L2 of its own, so only images
    eight workgroups apart see each other's stores if they are handed the same workspace rows."""
    C = 201
    return [([robust_detections(9500 + 10 * k + n, n, C, 0.5) if n else empty_image(C) for n in sizes], 0.5)
            for k, sizes in enumerate((MIXED_HOMES_N, SAME_XCD_N))]


def decode_case(name):
    return zero_max() if name.startswith("zero_max_") else globals()[name]()


def decode_modes(name):
    """The mode a case is named for -- its premises and its reference fixture; the device runs every case in both modes."""
    return ("post",) if name.endswith("_post") else ("meet",) if name.endswith("_meet") else MODES


def expected_decode(d, thr, mode):
    C = d["predict_logits"].shape[1]
    if not len(d["predict_logits"]):
        return np.zeros(0, np.int64)
    prob = np_softmax(d["predict_logits"]) if mode == "post" else np_onehot_prob(d["pred_labels"], C)
    return np_decode(prob, d["boxes_per_cls"], thr, mode)


# ---- pairs ------------------------------------------------------------------------------------------------------------

def _pimage(boxes, scores, size=(4000, 3000)):
    return {"boxes": np.asarray(boxes, F).reshape(-1, 4), "pred_scores": np.asarray(scores, F).reshape(-1), "image_size": size}


def seeded_pimage(seed, n):
    if n == 0:
        return _pimage(np.zeros((0, 4), F), np.zeros(0, F))
    d = synth.synthetic_detections(seed, n, 151)
    return _pimage(d["boxes"], d["pred_scores"], d["image_size"])


def chain_boxes(n):
    """Box i overlaps boxes i - 1 and i + 1 only: 2 * (n - 1) ordered pairs pass the filter."""
    x = np.arange(n) * 10.0
    return np.stack([x, np.zeros(n), x + 12.0, np.full(n, 9.0)], 1).astype(F)


CAPS = (1, 2, 3, 100, 1000, 2047, 2049, 4095, 4096)
STRADDLE_ONES = (0, 1, 2, 70, 71, 72, 140, 141, 142, 200)
STRADDLE_HALVES = tuple(range(3, 14)) + tuple(range(73, 83)) + tuple(range(143, 153)) + tuple(range(201, 210))
STRADDLE_CAPS = (500, 890, 91)     # 90 products of 1 above T = 0.5, 800 products of 0.5: need 410, 800 (all) and 1


@functools.lru_cache(None)
def caps():
    d = seeded_pimage(9700, 70)
    return [([d], cap, False) for cap in CAPS]


@functools.lru_cache(None)
def cap_edges():
    """total == cap and total == cap + 1, unfiltered (n * (n - 1)) and filtered (a chain of 40 boxes: 78 pairs; cap 79 too)."""
    a, b, c = seeded_pimage(9710, 46), seeded_pimage(9711, 3), _pimage(chain_boxes(40), synth.uniform(9712, "sgdet_cases.chain", (40,), 0.05, 1.0))
    return [([a], 2070, False), ([a], 2069, False), ([b], 6, False), ([b], 5, False),
            ([c], 78, True), ([c], 77, True), ([c], 79, True)]


@functools.lru_cache(None)
def straddle():
    n = 210
    s = np.full(n, 0.25, F)
    s[list(STRADDLE_ONES)] = 1.0
    s[list(STRADDLE_HALVES)] = 0.5
    d = _pimage(apart_boxes(n, 1)[:, 0], s)
    return [([d], cap, False) for cap in STRADDLE_CAPS]


@functools.lru_cache(None)
def zero_scores():
    """Half the detections decoded as background (score 0): 2450 non-zero products of 9900, the cap inside the zero group; and
    scores 1e-22 / 1e-23 whose products are subnormal (600 of 1e-44, 1250 of 1e-45) or underflow to 0 (1e-46)."""
    n = 100
    s = synth.uniform(9720, "sgdet_cases.zero_scores", (n,), 0.05, 1.0)
    s[1::2] = 0.0
    t = np.zeros(n, F)
    t[0::4], t[2::4] = F(1e-22), F(1e-23)
    boxes = seeded_pimage(9721, n)["boxes"]
    return [([_pimage(boxes, s)], 3000, False), ([_pimage(boxes, s)], 2450, False), ([_pimage(boxes, s)], 2449, False),
            ([_pimage(boxes, t)], 1000, False), ([_pimage(boxes, t)], 2000, False)]


TOUCHING_BOXES = ((0, 0, 10, 10),      # 0
                  (10, 0, 20, 10),     # 1: x1 == x2 of box 0 -- one shared pixel column, overlaps 0
                  (21, 0, 30, 10),     # 2: x1 == x2 of box 1 + 1 -- apart from 1
                  (0, 10, 10, 20),     # 3: y1 == y2 of box 0 -- overlaps 0 (and 1 in the corner pixel)
                  (0, 21, 10, 30))     # 4: y1 == y2 of box 3 + 1 -- apart from 3
TOUCHING_PAIRS = ((0, 1), (0, 3), (1, 0), (1, 3), (3, 0), (3, 1))


@functools.lru_cache(None)
def touching():
    a = _pimage(np.array(TOUCHING_BOXES, F), np.array([0.9, 0.8, 0.7, 0.6, 0.5], F))
    nothing = _pimage(apart_boxes(6, 1)[:, 0], np.full(6, 0.5, F))
    gap1 = _pimage(np.array([(0, 0, 10, 10), (11, 0, 20, 10), (0, 11, 10, 20)], F), np.full(3, 0.5, F))   # all one pixel apart
    return [([a, nothing, gap1], 2048, True), ([a, nothing, gap1], 2048, False), ([a], 4, True)]


WORD_EDGE_N = (0, 1, 2, 31, 32, 33, 255, 256, 0, 64)


@functools.lru_cache(None)
def word_edges():
    imgs = [seeded_pimage(9800 + i, n) for i, n in enumerate(WORD_EDGE_N)]
    return [(imgs, 2048, True), (imgs, 2048, False)]


def pair_case(name):
    return globals()[name]()


def golden_pair_instances(name):
    """The instances of a pair case whose reference output is stored (tests/golden/sgdet/pairs_cases.npz)."""
    return {"caps": (3, 6), "cap_edges": (2, 3, 4, 5, 6), "straddle": (0,), "touching": (0, 1, 2)}[name]


def torch_pairs(boxes, scores, cap, require_overlap):
    """prepare_test_pairs written directly: nonzero of the candidate matrix, then torch.sort(descending=True, stable=True)."""
    import torch
    n = len(boxes)
    cand = torch.ones(n, n, dtype=torch.bool) & ~torch.eye(n, dtype=torch.bool)
    if require_overlap and n:
        cand &= torch.from_numpy(np_overlap(boxes))
    idx = torch.nonzero(cand).reshape(-1, 2)
    if len(idx) > cap:
        s = torch.from_numpy(np.asarray(scores, F))
        q = s[idx[:, 0]] * s[idx[:, 1]]
        idx = idx[torch.sort(q, descending=True, stable=True)[1][:cap]]
    if len(idx) == 0:
        idx = torch.zeros((1, 2), dtype=torch.int64)
    return idx.numpy()


# ---- the recorded premises ----------------------------------------------------------------------------------------------

def report():
    lines = []
    for name in DECODE_CASE_NAMES:
        for li, (imgs, thr) in enumerate(decode_case(name)):
            for mode in decode_modes(name):
                for d in imgs:
                    n, C = d["predict_logits"].shape
                    if not n:
                        continue
                    s = decode_summary(d, thr, mode)
                    lines.append("%-14s launch %d %-4s %3d x %-4d %s zero-max %3d re-picks %3d overwritten %3d (changed %3d) kept %3d revived %3d "
                                 "lower-col %2d never-picked %3d row-ties %3d col-ties %3d (lanes %3d) gap %.3g iou-margin %.3g"
                                 % (name, li, mode, n, C, "lds" if n * C <= LDS_CELLS else "ws ", s["zero_steps"], s["repicks"],
                                    s["overwritten"], s["changed"], s["kept"], s["revived"], s["lower_col"], s["never_picked"], s["row_ties"],
                                    s["col_ties"], s["lane_ties"], s["gap"], s["iou_margin"]))
    for name in PAIR_CASE_NAMES:
        for imgs, cap, ov in pair_case(name):
            for d in imgs:
                t = pairs_trace(d["boxes"], d["pred_scores"], cap, ov)
                tail = "T %.9g above %d group %d need %d waves %s taken from %s" % (
                    t["T"], t["above"], t["group"], t["need"], t["waves"], t["taken_waves"]) if t["capped"] else "row-major"
                lines.append("%-12s n %3d cap %4d filter %d total %5d %s" % (name, len(d["boxes"]), cap, ov, t["total"], tail))
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
