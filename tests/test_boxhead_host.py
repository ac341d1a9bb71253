"""sgdet box decoder, host side: the numpy restatements of the reference's NMS kernel and box-head PostProcessor (the GPU tests'
second yardstick) reproduce every fixture of tests/golden/boxhead/, and the new C-ABI entries reject bad arguments without
a GPU.  The fixtures come from tests/golden/make_golden_boxhead.py (the reference's own PostProcessor around a restated
NMS primitive: see its docstring)."""
import ctypes
import glob
import os
import sys
import types

import numpy as np
import pytest

from veto_amd import native, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxhead")
XFORM_CLIP = float(np.log(1000.0 / 16))


# ---- numpy restatements -----------------------------------------------------------------------------------------------

def np_nms(boxes, scores, thr, dtype=np.float32, consulted=None):
    """pysgg._C.nms as the GPU computes it (csrc/cuda/nms.cu): boxes visited by descending score (:73-75; ties: index asc),
    devIoU with the +1 convention in its operation order (:13-21), suppression at IoU > thr (:60), greedy resolution
    (:112-123), kept indices ascending (:127-130).  `consulted` collects every IoU a kept box was compared at."""
    boxes = np.asarray(boxes, dtype).reshape(-1, 4)
    n = len(boxes)
    order = np.lexsort((np.arange(n), -np.asarray(scores, np.float64)))
    b = boxes[order]
    one, zero, thr = dtype(1), dtype(0), dtype(thr)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(order[i])
        r = b[i + 1:]
        w = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]) + one, zero)
        h = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]) + one, zero)
        inter = w * h
        iou = inter / (area[i] + area[i + 1:] - inter)
        if consulted is not None:
            consulted.append(iou[~removed[i + 1:]])
        removed[i + 1:] |= iou > thr
    return np.sort(np.asarray(keep, np.int64))


def np_softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def np_decode_boxes(reg, proposals, size, weights, n_cls, cls_agnostic, dtype):
    """BoxCoder.decode (box_coder.py:62-95) + clip_to_image(remove_empty=False) (bounding_box.py:237-247) -> [n, C, 4]."""
    p = proposals.astype(dtype)
    reg = reg.astype(dtype)
    if cls_agnostic:
        reg = np.tile(reg[:, -4:], (1, n_cls))
    reg = reg.reshape(len(p), n_cls, 4)
    half, one = dtype(0.5), dtype(1)
    w = (p[:, 2] - p[:, 0] + one)[:, None]
    h = (p[:, 3] - p[:, 1] + one)[:, None]
    cx, cy = p[:, 0:1] + half * w, p[:, 1:2] + half * h
    wx, wy, ww, wh = (dtype(v) for v in weights)
    dx, dy = reg[..., 0] / wx, reg[..., 1] / wy
    dw, dh = np.minimum(reg[..., 2] / ww, dtype(XFORM_CLIP)), np.minimum(reg[..., 3] / wh, dtype(XFORM_CLIP))
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    out = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw - one, pcy + half * ph - one], -1)
    out[..., 0::2] = np.clip(out[..., 0::2], dtype(0), dtype(size[0] - 1))
    out[..., 1::2] = np.clip(out[..., 1::2], dtype(0), dtype(size[1] - 1))
    return out.astype(dtype)


def np_box_postprocess(d, prm, dtype=np.float32, diag=None):
    """PostProcessor.forward + filter_results (box_head/inference.py:51-238) for one image d (synth.synthetic_box_head_outputs
    keys).  diag (a dict) receives what the fixture generator's robustness checks look at."""
    C = d["class_logits"].shape[1]
    prob = np_softmax(d["class_logits"].astype(dtype)).astype(dtype)
    dec = np_decode_boxes(d["box_regression"], d["proposals"], d["image_size"], prm["weights"], C, prm["cls_agnostic"], dtype)
    thr = dtype(prm["score_thresh"])
    alive = np.zeros(prob.shape, bool)
    consulted, seg_ties = [], False
    for j in range(1, C):
        inds = np.nonzero(prob[:, j] > thr)[0]
        if len(inds) == 0:
            continue
        seg_ties |= len(np.unique(prob[inds, j])) != len(inds)
        keep = np_nms(dec[inds, j], prob[inds, j], prm["nms"], dtype, consulted)
        if prm["topn"] > 0:
            keep = keep[:prm["topn"]]
        alive[inds[keep], j] = True
    if prm["filter_dup"]:
        dist = np.where(alive, prob, dtype(0))
        scores, labels = dist.max(1), dist.argmax(1)
        rows = np.nonzero(scores)[0]
        scores, labels = scores[rows], labels[rows]
    else:
        labels, rows = np.nonzero(alive[:, 1:].T)
        labels = labels + 1
        scores = prob[rows, labels]
    gap = np.inf
    cap = prm["det_per_img"]
    if 0 < cap < len(rows):
        srt = np.sort(scores)
        cut = srt[len(rows) - cap]
        if len(rows) - cap - 1 >= 0:
            gap = float(cut) - float(srt[len(rows) - cap - 1])
        keep = np.nonzero(scores >= cut)[0]
        rows, labels, scores = rows[keep], labels[keep], scores[keep]
    if diag is not None:
        diag.update(consulted=np.concatenate(consulted) if consulted else np.zeros(0, dtype), prob=prob, seg_ties=seg_ties,
                    cut_gap=gap, dec=dec)
    return {"orig_inds": rows.astype(np.int64), "pred_labels": labels.astype(np.int64), "pred_scores": scores.astype(dtype),
            "boxes": dec[rows, labels], "boxes_per_cls": dec[rows]}


# ---- fixtures ---------------------------------------------------------------------------------------------------------

def fixture_params(z):
    return {"score_thresh": float(z["score_thresh"]), "nms": float(z["nms"]), "topn": int(z["topn"]),
            "filter_dup": bool(z["filter_dup"]), "det_per_img": int(z["det_per_img"]), "weights": tuple(float(w) for w in z["weights"]),
            "cls_agnostic": bool(z["cls_agnostic"])}


def hand_built_image(kind, C):
    """The deliberate exact cases (not seeded).  'nothing': equal logits, every probability 1 / C < SCORE_THRESH.
    'tie_cap': rows 0 and 1 are identical (far apart as boxes), row 2 scores lower; with DETECTIONS_PER_IMG = 1 the cut value
    is the shared score of rows 0 and 1 and BOTH stay (score >= cut, inference.py:223).  'topn_bind' and 'class_major': the two
    branches of filter_results that no seeded fixture enters (see below)."""
    if kind == "nothing":
        n = 10
        prop = np.stack([np.arange(n) * 20.0, np.arange(n) * 10.0, np.arange(n) * 20.0 + 50, np.arange(n) * 10.0 + 40], 1)
        return {"proposals": prop.astype(np.float32), "class_logits": np.zeros((n, C), np.float32),
                "box_regression": np.zeros((n, 4 * C), np.float32), "image_size": (800, 600)}
    if kind == "topn_bind":   # C = 2: ten disjoint boxes, all survive the NMS, the score rises with the row (the best is row 9);
        n = 10               # a binding POST_NMS_PER_CLS_TOPN keeps the FIRST rows of the ascending keep list (inference.py:191-193)
        x0 = np.arange(n) * 40.0
        prop = np.stack([x0, x0 * 0 + 10, x0 + 29, x0 * 0 + 39], 1)
        logits = np.zeros((n, C), np.float32)
        logits[:, 1] = 0.25 * np.arange(n)
        return {"proposals": prop.astype(np.float32), "class_logits": logits, "box_regression": np.zeros((n, 4 * C), np.float32),
                "image_size": (800, 600)}
    if kind == "class_major":   # C = 300, duplicates kept: the detection list is class-major; survivors in columns 1, 255, 256, 257, 299
        assert C == 300
        n = 6
        x0 = np.arange(n) * 50.0
        prop = np.stack([x0, x0 * 0 + 20, x0 + 39, x0 * 0 + 59], 1)
        logits = np.full((n, C), -2.0, np.float32)
        for r, (c, v) in enumerate(((299, 4.0), (257, 4.5), (256, 5.0), (255, 5.5), (1, 6.0))):
            logits[r, c] = v
        logits[5, 1], logits[5, 299], logits[5, 257] = 5.25, 4.75, 4.25   # one row in three columns, both rounds of columns
        return {"proposals": prop.astype(np.float32), "class_logits": logits, "box_regression": np.zeros((n, 4 * C), np.float32),
                "image_size": (800, 600)}
    assert kind == "tie_cap"
    prop = np.array([[10, 10, 60, 60], [300, 300, 350, 350], [600, 100, 650, 150]], np.float32)
    logits = np.full((3, C), -4.0, np.float32)
    logits[0, 5] = logits[1, 5] = 4.0
    logits[2, 7] = 3.0
    return {"proposals": prop, "class_logits": logits, "box_regression": np.zeros((3, 4 * C), np.float32), "image_size": (800, 600)}


def fixture_images(z):
    """Regenerates a decoder fixture's inputs from its seeds (seed < 0: a hand-built image)."""
    C = int(z["n_cls"])
    out = []
    for seed, n, kind in zip(z["seeds"], z["n_per_img"], z["kinds"]):
        if seed < 0:
            out.append(hand_built_image(str(kind), C))
        else:
            out.append(synth.synthetic_box_head_outputs(int(seed), int(n), C, cls_agnostic=bool(z["cls_agnostic"])))
    return out


def nms_fixture_inputs(seed, n):
    """Boxes and scores of one NMS segment (seed < 0: the hand-built pair at IoU exactly 0.5: inter 50, union 100)."""
    if seed < 0:
        return np.array([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32), np.array([0.9, 0.8], np.float32)
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    return synth.synthetic_nms_boxes(int(seed), int(n))


def decoder_fixtures():
    return sorted(f for f in glob.glob(os.path.join(GOLDEN, "*.npz")) if os.path.basename(f) != "nms.npz")


def test_fixtures_are_present():
    names = {os.path.basename(f)[:-4] for f in decoder_fixtures()}
    assert {"n20_full", "vg1000", "vg1000_nodup", "ragged12", "gqa", "agnostic", "nothing", "below_cap", "tie_cap"} <= names
    assert os.path.exists(os.path.join(GOLDEN, "nms.npz"))


def test_numpy_nms_reproduces_every_fixture():
    z = np.load(os.path.join(GOLDEN, "nms.npz"))
    sizes = set()
    for name in [str(s) for s in z["cases"]]:
        seed, n, thr = int(z[name + "__seed"]), int(z[name + "__n"]), float(z[name + "__thr"])
        boxes, scores = nms_fixture_inputs(seed, n)
        boxes, scores = boxes[:n], scores[:n]
        keep = np_nms(boxes, scores, thr)
        assert np.array_equal(keep, z[name + "__keep"]), name
        sizes.add(n)
    assert {0, 1, 2, 63, 64, 65, 1000, 6000} <= sizes
    # the deliberate exact case: IoU == threshold keeps both boxes under `>` (nms.cu:60)
    assert np.array_equal(z["iou_tie__keep"], [0, 1]) and float(z["iou_tie__thr"]) == 0.5


@pytest.mark.parametrize("path", decoder_fixtures(), ids=lambda p: os.path.basename(p)[:-4])
def test_numpy_decoder_reproduces_every_fixture(path):
    z = np.load(path)
    prm = fixture_params(z)
    row = 0
    for i, d in enumerate(fixture_images(z)):
        got = np_box_postprocess(d, prm)
        k = int(z["counts"][i])
        sl = slice(row, row + k)
        assert len(got["orig_inds"]) == k
        assert np.array_equal(got["orig_inds"], z["orig_inds"][sl])
        assert np.array_equal(got["pred_labels"], z["pred_labels"][sl])
        tol_b, tol_s = 4 * float(z["ref_fp32_err_boxes"]), 4 * float(z["ref_fp32_err_scores"])
        assert np.abs(got["pred_scores"] - z["pred_scores"][sl]).max(initial=0) <= tol_s
        assert np.abs(got["boxes"] - z["boxes"][sl]).max(initial=0) <= tol_b
        assert np.abs(got["boxes_per_cls"] - z["boxes_per_cls"][sl]).max(initial=0) <= tol_b
        if "dec_full" in z.files:
            diag = {}
            np_box_postprocess(d, prm, diag=diag)
            assert np.abs(diag["dec"] - z["dec_full"]).max() <= tol_b
        row += k
    assert row == len(z["orig_inds"])
    if os.path.basename(path) == "tie_cap.npz":   # both equal scores at the cut are kept: 2 detections with a cap of 1
        assert prm["det_per_img"] == 1 and list(z["counts"]) == [2]
    if os.path.basename(path) == "nothing.npz":
        assert 0 in list(z["counts"])


def test_fixture_files_are_small():
    for f in glob.glob(os.path.join(GOLDEN, "*.npz")):
        assert os.path.getsize(f) < (1 << 20), f


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------

def test_new_entries_are_exported():
    for name in ("veto_nms", "veto_nms_max_segment", "veto_box_postprocess", "veto_box_postprocess_workspace_bytes"):
        assert name in native.EXPORTS
        assert hasattr(native.load_library(), name)
    assert native.load_library().veto_nms_max_segment() >= 6000


def _off(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_nms_rejects_bad_arguments_without_a_gpu():
    lib = native.load_library()
    a = native.VetoNmsArgs()
    assert lib.veto_nms(None, ctypes.byref(a)) == -1
    assert b"veto_nms_args_t size mismatch" in lib.veto_last_error()
    a.struct_size = ctypes.sizeof(native.VetoNmsArgs)
    limit = lib.veto_nms_max_segment()
    a.n_seg, a.n_box, a.threshold = 2, limit + 11, 0.5
    a.boxes = a.scores = a.seg_offset = a.keep = a.counts = 256
    big = _off([0, 10, limit + 11])
    a.seg_offset_host = ctypes.cast(big, ctypes.c_void_p)
    assert lib.veto_nms(None, ctypes.byref(a)) == -1
    msg = lib.veto_last_error()
    assert b"seg_offset_host" in msg and str(limit).encode() in msg and b"segment 1" in msg
    bad = _off([0, 30, 20])
    a.n_box, a.seg_offset_host = 20, ctypes.cast(bad, ctypes.c_void_p)
    assert lib.veto_nms(None, ctypes.byref(a)) == -1
    assert b"seg_offset_host is not monotone" in lib.veto_last_error()
    a.seg_offset_host = None
    assert lib.veto_nms(None, ctypes.byref(a)) == -1
    assert b"seg_offset_host" in lib.veto_last_error()


def test_box_postprocess_rejects_bad_arguments_without_a_gpu():
    lib = native.load_library()
    a = native.VetoBoxPostArgs()
    assert lib.veto_box_postprocess(None, ctypes.byref(a), None, 0) == -1
    assert b"veto_box_post_args_t size mismatch" in lib.veto_last_error()
    a.struct_size = ctypes.sizeof(native.VetoBoxPostArgs)
    a.n_img, a.n_box, a.n_cls, a.reg_cols = 2, 20, 1, 4
    assert lib.veto_box_postprocess(None, ctypes.byref(a), None, 0) == -1
    assert b"n_cls" in lib.veto_last_error()
    a.n_cls, a.reg_cols = 151, 600
    assert lib.veto_box_postprocess(None, ctypes.byref(a), None, 0) == -1
    assert b"reg_cols" in lib.veto_last_error()
    a.reg_cols, a.score_thresh, a.nms_thresh = 604, 0.01, 0.3
    a.reg_weights = (ctypes.c_float * 4)(10, 10, 5, 5)
    bad = _off([0, 30, 20])
    a.img_offset_host = ctypes.cast(bad, ctypes.c_void_p)
    assert lib.veto_box_postprocess(None, ctypes.byref(a), None, 0) == -1
    assert b"img_offset_host is not monotone" in lib.veto_last_error()
    limit = lib.veto_nms_max_segment()
    big = _off([0, limit + 1, limit + 2])
    a.n_box, a.img_offset_host = limit + 2, ctypes.cast(big, ctypes.c_void_p)
    assert lib.veto_box_postprocess(None, ctypes.byref(a), None, 0) == -1
    assert b"img_offset_host" in lib.veto_last_error() and str(limit).encode() in lib.veto_last_error()
    assert lib.veto_box_postprocess_workspace_bytes(1000, 151, 1) >= 1000 * 151 * 20


# ---- the Python surface -----------------------------------------------------------------------------------------------

def test_post_processor_constructor_and_factory():
    from veto_amd import boxhead
    p = boxhead.PostProcessor()
    assert (p.score_thresh, p.nms, p.post_nms_per_cls_topn, p.nms_filter_duplicates, p.detections_per_img) == (0.05, 0.5, 300, True, 100)
    assert p.box_coder.weights == (10., 10., 5., 5.) and abs(p.box_coder.bbox_xform_clip - XFORM_CLIP) < 1e-12
    with pytest.raises(NotImplementedError):
        boxhead.PostProcessor(bbox_aug_enabled=True)
    ns = types.SimpleNamespace
    cfg = ns(MODEL=ns(ROI_HEADS=ns(USE_FPN=True, BBOX_REG_WEIGHTS=(10., 10., 5., 5.), SCORE_THRESH=0.01, NMS=0.3, DETECTIONS_PER_IMG=80,
                                   POST_NMS_PER_CLS_TOPN=300, NMS_FILTER_DUPLICATES=True), CLS_AGNOSTIC_BBOX_REG=False),
             TEST=ns(BBOX_AUG=ns(ENABLED=False), SAVE_PROPOSALS=False))
    p = boxhead.make_roi_box_post_processor(cfg)
    assert (p.score_thresh, p.nms, p.detections_per_img, p.nms_filter_duplicates) == (0.01, 0.3, 80, True)
    cfg.TEST.BBOX_AUG.ENABLED = True
    with pytest.raises(NotImplementedError):
        boxhead.make_roi_box_post_processor(cfg)


def test_install_detector_ops_patches_the_three_names(monkeypatch):
    from veto_amd import boxhead, layers, registry
    names = ["pysgg", "pysgg.layers", "pysgg.structures", "pysgg.structures.boxlist_ops", "pysgg.modeling",
             "pysgg.modeling.roi_heads", "pysgg.modeling.roi_heads.box_head", "pysgg.modeling.roi_heads.box_head.inference",
             "pysgg.modeling.registry"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
        if "." in n:
            setattr(mods[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], m)
    sentinel = object()
    mods["pysgg.layers"].nms = sentinel
    mods["pysgg.structures.boxlist_ops"]._box_nms = sentinel
    mods["pysgg.modeling.roi_heads.box_head.inference"].make_roi_box_post_processor = sentinel
    mods["pysgg.modeling.registry"].ROI_RELATION_PREDICTOR = {}
    registry.install_detector_ops()
    assert mods["pysgg.layers"].nms is layers.nms
    assert mods["pysgg.structures.boxlist_ops"]._box_nms is layers.nms
    assert mods["pysgg.modeling.roi_heads.box_head.inference"].make_roi_box_post_processor is boxhead.make_roi_box_post_processor
    assert mods["pysgg.modeling.registry"].ROI_RELATION_PREDICTOR == {}          # install()'s target is untouched ...
    target = registry.install()                                                   # ... and install() does what it did
    assert target is mods["pysgg.modeling.registry"].ROI_RELATION_PREDICTOR
    assert sorted(target) == ["VETOPredictor", "VETOPredictor_MEET"]
    assert mods["pysgg.layers"].nms is layers.nms


def test_synthetic_box_head_outputs_shape_and_sparsity():
    d = synth.synthetic_box_head_outputs(5, 200)
    assert d["proposals"].shape == (200, 4) and d["class_logits"].shape == (200, 151) and d["box_regression"].shape == (200, 604)
    p = np_softmax(d["class_logits"].astype(np.float64))
    passing = (p[:, 1:] > 0.01).sum(1)
    assert 10 <= passing.mean() <= 40
    assert synth.synthetic_box_head_outputs(5, 50, cls_agnostic=True)["box_regression"].shape == (50, 8)
    again = synth.synthetic_box_head_outputs(5, 200)
    assert all(np.array_equal(d[k], again[k]) for k in ("proposals", "class_logits", "box_regression"))
