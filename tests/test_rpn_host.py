"""RPN proposal selection, host side: the numpy restatement of the reference's RPNPostProcessor (the GPU tests' second
yardstick) reproduces every fixture of tests/golden/rpn/, veto_amd.synth.anchor_grid matches the stored anchor checksums, and
the new Python and C-ABI entries reject bad arguments without a GPU.  The fixtures come from tests/golden/make_golden_rpn.py
(the reference's own RPNPostProcessor around the restated NMS primitive of test_boxhead_host: see its docstring)."""
import ctypes
import glob
import hashlib
import inspect
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_boxhead_host import XFORM_CLIP, np_decode_boxes, np_nms  # noqa: E402

from veto_amd import native, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpn")
RATIOS = (0.5, 1.0, 2.0)
FIVE = ((20, 25), (10, 13), (5, 7), (3, 4), (2, 2))
FIVE_GEOM = dict(strides=(8, 16, 32, 64, 128), sizes=(64, 128, 256, 512, 1024))
# name: geometry, image sizes (width, height), settings
CASES = {
    "small5": dict(grids=FIVE, images=((200, 160), (192, 150), (176, 144)), pre=300, post=100, fpn=150, thr=0.7, min_size=0,
                   **FIVE_GEOM),
    "below_cap": dict(grids=FIVE, images=((200, 160),), pre=300, post=300, fpn=2000, thr=0.7, min_size=0, **FIVE_GEOM),
    "min_size": dict(grids=FIVE[:2], images=((200, 160), (192, 150)), pre=300, post=100, fpn=150, thr=0.7, min_size=12,
                     strides=(8, 16), sizes=(64, 128)),
    "one_level": dict(grids=((32, 40),), images=((640, 512), (600, 500)), pre=1500, post=300, fpn=300, thr=0.7, min_size=0,
                      strides=(16,), sizes=(128,)),
    "per_batch": dict(grids=FIVE, images=((200, 160), (192, 150), (176, 144)), pre=300, post=100, fpn=200, thr=0.7, min_size=0,
                      training=True, per_batch=True, **FIVE_GEOM),
    "add_gt": dict(grids=FIVE, images=((200, 160), (192, 150)), pre=300, post=100, fpn=150, thr=0.7, min_size=0, training=True,
                   per_batch=False, add_gt=4, **FIVE_GEOM),
    "full_level": dict(grids=((152, 200),), images=((800, 608),), pre=6000, post=1000, fpn=1000, thr=0.7, min_size=0,
                       strides=(4,), sizes=(32,)),
    "ties": dict(grids=((4, 4), (4, 4)), images=((200, 240),), pre=10, post=100, fpn=17, thr=0.5, min_size=0, hand_built=True),
    "min_size_exact": dict(grids=((2, 4),), images=((100, 60),), pre=8, post=8, fpn=8, thr=0.7, min_size=8, hand_built=True,
                           determinate=True),
}


# ---- inputs -------------------------------------------------------------------------------------------------------------

def ties_inputs():
    """The deliberate exact case.  Two levels of 48 disjoint 10 x 10 anchors and zero regressions (decode returns the anchor
    bit for bit).  Level 0: anchor 1 is [0, 0, 9, 4] against anchor 0 = [0, 0, 9, 9]: IoU exactly 0.5 at threshold 0.5, both
    kept; anchors 9, 10 and 11 share the logit 1.52 at the pre-NMS cut of 10: anchor 9 alone is taken.  Both levels hold a
    logit 1.52 on either side of the merge cut of 17: level 0's is kept."""
    anchors, obj, reg = [], [], []
    tops = ([3.0, 2.5, 2.0, 1.9, 1.8, 1.7, 1.6, 1.58, 1.56, 1.52, 1.52, 1.52], [2.9, 2.4, 1.95, 1.85, 1.75, 1.65, 1.55, 1.52, 1.3, 1.2, 1.1])
    for l in range(2):
        i = np.arange(48)
        x0, y0 = (i % 8) * 20.0, (i // 8) * 20.0 + 120.0 * l
        a = np.stack([x0, y0, x0 + 9, y0 + 9], 1).astype(np.float32)
        if l == 0:
            a[1] = [0, 0, 9, 4]
        vals = (-2.0 - l - 0.01 * i).astype(np.float32)
        vals[:len(tops[l])] = tops[l]
        anchors.append(a)
        obj.append(np.ascontiguousarray(vals.reshape(4, 4, 3).transpose(2, 0, 1))[None])
        reg.append(np.zeros((1, 12, 4, 4), np.float32))
    return {"anchors": anchors, "objectness": obj, "box_regression": reg}


def min_size_exact_inputs():
    """min_size met exactly (remove_small_boxes keeps a side >= min_size, boxlist_ops.py:35-49).  One level of 8 hand-placed
    anchors (A = 1, 2 x 4 cells), zero regressions, an image 100 wide and 60 high, min_size 8, distinct logits.  Kept: 0 (8 x 8),
    3 (9 x 8), 5 (reaches to x = 110, clipped at 99 to exactly 8 wide), 6 (clipped at y = 59 to exactly 8 high).  Removed: 1 (7
    wide), 2 (7 high), 4 (clipped to 7 wide: narrow only by the clip), 7 (clipped to 7 high)."""
    a = np.array([[0, 0, 7, 7], [20, 0, 26, 7], [40, 0, 47, 6], [60, 0, 68, 7],
                  [93, 20, 110, 30], [92, 40, 110, 50], [0, 52, 10, 70], [20, 53, 30, 70]], np.float32)
    obj = np.array([1.0, 3.0, 2.5, 0.5, 2.0, 1.5, -0.5, 0.75], np.float32).reshape(1, 1, 2, 4)
    return {"anchors": [a], "objectness": [obj], "box_regression": [np.zeros((1, 4, 2, 4), np.float32)]}


HAND_BUILT = {"ties": ties_inputs, "min_size_exact": min_size_exact_inputs}


def rpn_targets(seed, image_sizes, n):
    """n ground-truth boxes per image (xyxy) for the add_gt case."""
    out = []
    for i, (w, h) in enumerate(image_sizes):
        c = synth.uniform(seed, "rpn.gt.%d" % i, (n, 4), 0.0, 1.0).astype(np.float64)
        x1, y1 = c[:, 0] * 0.6 * w, c[:, 1] * 0.6 * h
        out.append(np.stack([x1, y1, x1 + 8 + c[:, 2] * 0.3 * w, y1 + 8 + c[:, 3] * 0.3 * h], 1).astype(np.float32))
    return out


def case_inputs(name, seed):
    """anchors / objectness / box_regression (lists over the levels) of a case, regenerated from its seed."""
    c = CASES[name]
    if c.get("hand_built"):
        return HAND_BUILT[name]()
    d = synth.synthetic_rpn_outputs(int(seed), len(c["images"]), c["grids"], A=len(RATIOS))
    d["anchors"] = synth.anchor_grid(c["sizes"], c["strides"], RATIOS, c["grids"])
    return d


def anchor_checksum(anchors):
    h = hashlib.sha256()
    for a in anchors:
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


# ---- numpy restatement --------------------------------------------------------------------------------------------------

def np_sigmoid(x, dtype):
    return (dtype(1) / (dtype(1) + np.exp(-x.astype(dtype)))).astype(dtype)


def np_rpn_proposals(d, c, dtype=np.float32, diag=None):
    """RPNPostProcessor.forward (rpn/inference.py:78-183) without add_gt_proposals, with the total orders this project fixes:
    (logit desc, anchor asc) at the pre-NMS cut, (logit desc, level asc, rank asc) at the per-image merge, (image, level, rank)
    among equal logits at the per-batch cut.  Returns per image boxes / objectness / level / anchor_index / logit; diag collects
    what the fixture generator's robustness checks look at."""
    per_img, consulted, sides, cuts, nms_in, nms_out = [], [], [], [], [], []
    for i, size in enumerate(c["images"]):
        rows = []
        for l, (obj, reg, anc) in enumerate(zip(d["objectness"], d["box_regression"], d["anchors"])):
            A, H, W = obj.shape[1:]
            x = obj[i].transpose(1, 2, 0).reshape(-1)
            k = min(c["pre"], len(x))
            order = np.lexsort((np.arange(len(x)), -x.astype(np.float64)))
            if k < len(x):
                cuts.append((x[order[k - 1]], x[order[k]]))
            order = order[:k]
            r = reg[i].reshape(A, 4, H, W).transpose(2, 3, 0, 1).reshape(-1, 4)[order]
            box = np_decode_boxes(r, anc[order], size, (1., 1., 1., 1.), 1, False, dtype)[:, 0]
            ws, hs = box[:, 2] - box[:, 0] + dtype(1), box[:, 3] - box[:, 1] + dtype(1)
            sides.append(np.concatenate([ws, hs]))
            ok = np.nonzero((ws >= dtype(c["min_size"])) & (hs >= dtype(c["min_size"])))[0]
            box, order = box[ok], order[ok]
            if c["thr"] > 0:
                keep = np_nms(box, x[order], c["thr"], dtype, consulted)
                nms_in.append(len(order))
                nms_out.append(len(keep))   # (before the cap)
                if c["post"] > 0:
                    if len(keep) > c["post"]:
                        cuts.append((x[order[keep[c["post"] - 1]]], x[order[keep[c["post"]]]]))
                    keep = keep[:c["post"]]
                box, order = box[keep], order[keep]
            rows.append(dict(boxes=box, logit=x[order], level=np.full(len(order), l, np.int32), anchor_index=order.astype(np.int64)))
        per_img.append({k: np.concatenate([r[k] for r in rows]) for k in rows[0]})
    if len(d["objectness"]) > 1:
        if c.get("training") and c.get("per_batch"):
            x = np.concatenate([p["logit"] for p in per_img])
            order = np.lexsort((np.arange(len(x)), -x.astype(np.float64)))
            if c["fpn"] < len(x):
                cuts.append((x[order[c["fpn"] - 1]], x[order[c["fpn"]]]))
            mask = np.zeros(len(x), bool)
            mask[order[:c["fpn"]]] = True
            start = 0
            for p in per_img:
                m = mask[start:start + len(p["logit"])]
                start += len(m)
                for k in p:
                    p[k] = p[k][m]
        else:
            for p in per_img:
                x = p["logit"]
                order = np.lexsort((np.arange(len(x)), -x.astype(np.float64)))
                if c["fpn"] < len(x):
                    cuts.append((x[order[c["fpn"] - 1]], x[order[c["fpn"]]]))
                for k in p:
                    p[k] = p[k][order[:c["fpn"]]]
    for p in per_img:
        p["objectness"] = np_sigmoid(p["logit"], dtype)
    if diag is not None:
        diag.update(consulted=np.concatenate(consulted) if consulted else np.zeros(0, dtype), sides=np.concatenate(sides), cuts=cuts,
                    nms_in=nms_in, nms_out=nms_out)
    return per_img


# ---- fixtures -----------------------------------------------------------------------------------------------------------

def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def fixture_rows(z):
    """Per image the fixture's rows (the appended ground-truth rows of add_gt included: level and anchor_index -1)."""
    out, row = [], 0
    for k in z["counts"]:
        sl = slice(row, row + int(k))
        out.append({key: z[key][sl] for key in ("boxes", "objectness", "level", "anchor_index")})
        row += int(k)
    assert row == len(z["boxes"])
    return out


def test_fixtures_are_present_and_small():
    assert {os.path.basename(f)[:-4] for f in fixtures()} == set(CASES)
    for f in fixtures():
        assert os.path.getsize(f) < (1 << 20), f


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_reproduces_every_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = CASES[name]
    got = np_rpn_proposals(case_inputs(name, int(z["seed"])), c)
    n_gt = c.get("add_gt", 0)
    tol_b, tol_o = 4 * float(z["ref_fp32_err_boxes"]), 4 * float(z["ref_fp32_err_objectness"])
    for g, want in zip(got, fixture_rows(z)):
        k = len(want["boxes"]) - n_gt
        assert len(g["boxes"]) == k
        assert np.array_equal(g["level"], want["level"][:k]) and np.array_equal(g["anchor_index"], want["anchor_index"][:k])
        assert np.abs(g["boxes"] - want["boxes"][:k]).max(initial=0) <= tol_b
        assert np.abs(g["objectness"] - want["objectness"][:k]).max(initial=0) <= tol_o
        if n_gt:
            assert np.all(want["level"][k:] == -1) and np.all(want["objectness"][k:] == 1)
    if n_gt:
        for t, want in zip(rpn_targets(int(z["seed"]), c["images"], n_gt), fixture_rows(z)):
            assert np.array_equal(want["boxes"][-n_gt:], t)


def test_ties_fixture_holds_the_fixed_orders():
    z = np.load(os.path.join(GOLDEN, "ties.npz"))
    lvl, anc = z["level"], z["anchor_index"]
    assert list(z["counts"]) == [17] and float(z["ref_fp32_err_boxes"]) == 0.0
    assert sorted(anc[lvl == 0].tolist()) == list(range(10))   # anchor 9 of the three logits 1.52 at the pre-NMS cut; 0 and 1 (IoU == threshold) both kept
    assert sorted(anc[lvl == 1].tolist()) == list(range(7))    # level 1's 1.52 loses the tie at the merge cut
    assert (int(lvl[-1]), int(anc[-1])) == (0, 9)              # ... to level 0's, the last row


def test_anchor_grid_matches_the_stored_checksums():
    for name, c in CASES.items():
        if c.get("hand_built"):
            continue
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        anchors = synth.anchor_grid(c["sizes"], c["strides"], RATIOS, c["grids"])
        assert [a.shape for a in anchors] == [(3 * h * w, 4) for h, w in c["grids"]]
        assert anchor_checksum(anchors) == str(z["anchor_sha256"]), name
    a = synth.anchor_grid((32,), (4,), RATIOS, ((2, 3),))[0]
    assert a.dtype == np.float32 and np.array_equal(a[3] - a[0], [4, 0, 4, 0]) and np.array_equal(a[9] - a[0], [0, 4, 0, 4])
    assert np.array_equal(a[:3], [[-22., -10., 25., 13.], [-14., -14., 17., 17.], [-10., -22., 13., 25.]])


def test_synthetic_rpn_outputs_shapes_and_determinism():
    d = synth.synthetic_rpn_outputs(3, 2, ((5, 7), (3, 4)))
    assert [o.shape for o in d["objectness"]] == [(2, 3, 5, 7), (2, 3, 3, 4)]
    assert [r.shape for r in d["box_regression"]] == [(2, 12, 5, 7), (2, 12, 3, 4)]
    again = synth.synthetic_rpn_outputs(3, 2, ((5, 7), (3, 4)))
    assert all(np.array_equal(x, y) for x, y in zip(d["objectness"] + d["box_regression"], again["objectness"] + again["box_regression"]))
    assert d["objectness"][0].max() > 0 > d["objectness"][0].min()


# ---- the Python surface -------------------------------------------------------------------------------------------------

def test_post_processor_signatures_and_config_keys():
    from veto_amd import rpn
    assert list(inspect.signature(rpn.RPNPostProcessor.__init__).parameters) == [
        "self", "pre_nms_top_n", "post_nms_top_n", "nms_thresh", "min_size", "box_coder", "fpn_post_nms_top_n", "fpn_post_nms_per_batch",
        "add_gt"]
    assert list(inspect.signature(rpn.RPNPostProcessor.forward).parameters) == ["self", "anchors", "objectness", "box_regression", "targets"]
    assert list(inspect.signature(rpn.make_rpn_postprocessor).parameters) == ["config", "rpn_box_coder", "is_train"]
    p = rpn.RPNPostProcessor(6000, 1000, 0.7, 0)
    assert p.fpn_post_nms_top_n == 1000 and p.fpn_post_nms_per_batch is True and p.add_gt is True
    assert p.box_coder.weights == (1., 1., 1., 1.) and abs(p.box_coder.bbox_xform_clip - XFORM_CLIP) < 1e-12
    ns = types.SimpleNamespace
    cfg = ns(MODEL=ns(RPN=ns(PRE_NMS_TOP_N_TRAIN=2000, PRE_NMS_TOP_N_TEST=6000, POST_NMS_TOP_N_TRAIN=900, POST_NMS_TOP_N_TEST=1000,
                             FPN_POST_NMS_TOP_N_TRAIN=800, FPN_POST_NMS_TOP_N_TEST=700, FPN_POST_NMS_PER_BATCH=False, NMS_THRESH=0.7,
                             MIN_SIZE=0),
                      ROI_RELATION_HEAD=ns(ADD_GTBOX_TO_PROPOSAL_IN_TRAIN=True)))
    coder = object()
    p = rpn.make_rpn_postprocessor(cfg, coder, True)
    assert (p.pre_nms_top_n, p.post_nms_top_n, p.fpn_post_nms_top_n, p.fpn_post_nms_per_batch, p.add_gt) == (2000, 900, 800, False, True)
    assert p.box_coder is coder and (p.nms_thresh, p.min_size) == (0.7, 0)
    p = rpn.make_rpn_postprocessor(cfg, coder, False)
    assert (p.pre_nms_top_n, p.post_nms_top_n, p.fpn_post_nms_top_n) == (6000, 1000, 700)


def _fake_pysgg(monkeypatch, names):
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
        if "." in n:
            setattr(mods[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], m)
    return mods


def test_install_rpn_ops_patches_the_factory_and_its_bound_name(monkeypatch):
    from veto_amd import registry, rpn
    mods = _fake_pysgg(monkeypatch, ["pysgg", "pysgg.modeling", "pysgg.modeling.rpn", "pysgg.modeling.rpn.inference",
                                     "pysgg.modeling.rpn.rpn", "pysgg.layers"])
    sentinel = object()
    mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor = sentinel
    mods["pysgg.modeling.rpn.rpn"].make_rpn_postprocessor = sentinel
    mods["pysgg.layers"].nms = sentinel
    patched = registry.install_rpn_ops()
    assert mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor is rpn.make_rpn_postprocessor
    assert mods["pysgg.modeling.rpn.rpn"].make_rpn_postprocessor is rpn.make_rpn_postprocessor
    assert mods["pysgg.layers"].nms is sentinel   # nothing else is touched
    assert patched == [("pysgg.modeling.rpn.inference", "make_rpn_postprocessor"), ("pysgg.modeling.rpn.rpn", "make_rpn_postprocessor")]


def test_install_rpn_ops_without_the_rpn_module_loaded(monkeypatch):
    from veto_amd import registry, rpn
    mods = _fake_pysgg(monkeypatch, ["pysgg", "pysgg.modeling", "pysgg.modeling.rpn", "pysgg.modeling.rpn.inference"])
    monkeypatch.delitem(sys.modules, "pysgg.modeling.rpn.rpn", raising=False)
    assert registry.install_rpn_ops() == [("pysgg.modeling.rpn.inference", "make_rpn_postprocessor")]
    assert mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor is rpn.make_rpn_postprocessor


def test_install_detector_ops_still_patches_only_what_it_did(monkeypatch):
    from veto_amd import registry
    mods = _fake_pysgg(monkeypatch, ["pysgg", "pysgg.layers", "pysgg.structures", "pysgg.structures.boxlist_ops", "pysgg.modeling",
                                     "pysgg.modeling.roi_heads", "pysgg.modeling.roi_heads.box_head",
                                     "pysgg.modeling.roi_heads.box_head.inference", "pysgg.modeling.rpn", "pysgg.modeling.rpn.inference",
                                     "pysgg.modeling.rpn.rpn"])
    sentinel = object()
    mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor = sentinel
    mods["pysgg.modeling.rpn.rpn"].make_rpn_postprocessor = sentinel
    patched = registry.install_detector_ops()
    assert patched == [("pysgg.layers", "nms"), ("pysgg.structures.boxlist_ops", "_box_nms"),
                       ("pysgg.modeling.roi_heads.box_head.inference", "make_roi_box_post_processor")]
    assert mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor is sentinel
    assert mods["pysgg.modeling.rpn.rpn"].make_rpn_postprocessor is sentinel


def test_python_argument_checks_fail_before_the_library_is_touched(monkeypatch):
    import torch
    from veto_amd import rpn

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(native, "load_library", boom)
    o, r, a = torch.zeros(1, 3, 2, 2), torch.zeros(1, 12, 2, 2), torch.zeros(12, 4)
    kw = dict(pre_nms_top_n=10, post_nms_top_n=5, nms_thresh=0.7, min_size=0)
    with pytest.raises(ValueError, match="levels"):
        rpn.rpn_proposals([], [], [], [(8, 8)], **kw)
    with pytest.raises(ValueError, match="levels"):
        rpn.rpn_proposals([o] * 9, [r] * 9, [a] * 9, [(8, 8)], **kw)
    with pytest.raises(ValueError, match="one entry per level"):
        rpn.rpn_proposals([o], [r, r], [a], [(8, 8)], **kw)
    with pytest.raises(ValueError, match="box_regression"):
        rpn.rpn_proposals([o], [torch.zeros(1, 3, 2, 2)], [a], [(8, 8)], **kw)
    with pytest.raises(ValueError, match="anchors"):
        rpn.rpn_proposals([o], [r], [torch.zeros(11, 4)], [(8, 8)], **kw)
    with pytest.raises(ValueError, match="objectness"):
        rpn.rpn_proposals([o], [r], [a], [(8, 8), (8, 8)], **kw)
    with pytest.raises(ValueError, match="pre_nms_top_n"):
        rpn.rpn_proposals([o], [r], [a], [(8, 8)], **dict(kw, pre_nms_top_n=0))
    with pytest.raises(RuntimeError, match="HIP device only"):   # CPU tensors fail loudly
        rpn.rpn_proposals([o], [r], [a], [(8, 8)], **kw)


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------

def test_new_entries_are_exported():
    for name in ("veto_rpn_proposals", "veto_rpn_proposals_workspace_bytes"):
        assert name in native.EXPORTS
        assert hasattr(native.load_library(), name)


def _args(**kw):
    a = native.VetoRpnArgs()
    a.struct_size = ctypes.sizeof(native.VetoRpnArgs)
    a.n_img, a.n_lvl, a.pre_nms_top_n, a.post_nms_top_n, a.fpn_post_nms_top_n = 2, 2, 300, 100, 150
    a.nms_thresh, a.min_size, a.bbox_xform_clip = 0.7, 0.0, XFORM_CLIP
    a.reg_weights = (ctypes.c_float * 4)(1, 1, 1, 1)
    for l, (h, w) in enumerate(((20, 25), (10, 13))):
        a.level_a[l], a.level_h[l], a.level_w[l] = 3, h, w
        a.objectness[l] = a.box_regression[l] = a.anchors[l] = 256
    a.image_sizes = a.img_out_offset = a.boxes = a.objectness_out = a.level = a.anchor_index = a.counts = 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rpn_proposals_rejects_bad_arguments_without_a_gpu():
    lib = native.load_library()
    limit = lib.veto_nms_max_segment()
    a = native.VetoRpnArgs()
    assert lib.veto_rpn_proposals(None, ctypes.byref(a), None, 0) == -1
    assert b"veto_rpn_args_t size mismatch" in lib.veto_last_error()
    for bad, needle in ((dict(n_lvl=9), b"n_lvl"), (dict(n_img=0), b"n_img"), (dict(pre_nms_top_n=limit + 1), str(limit).encode()),
                        (dict(pre_nms_top_n=12000), b"pre_nms_top_n"), (dict(fpn_post_nms_top_n=0), b"fpn_post_nms_top_n"),
                        (dict(reg_weights=(ctypes.c_float * 4)(1, 1, 0, 1)), b"reg_weights[2]"),
                        (dict(per_batch=1, n_img=1025), b"per_batch"), (dict(boxes=None), b"missing pointer"),
                        (dict(boxes=264), b"16-byte")):
        assert lib.veto_rpn_proposals(None, ctypes.byref(_args(**bad)), ctypes.c_void_p(256), 1 << 30) == -1, bad
        assert needle in lib.veto_last_error(), (bad, lib.veto_last_error())
    a = _args()
    a.level_h[1] = 0
    assert lib.veto_rpn_proposals(None, ctypes.byref(a), ctypes.c_void_p(256), 1 << 30) == -1
    assert b"level 1" in lib.veto_last_error()
    a = _args(pre_nms_top_n=6000, post_nms_top_n=0, n_lvl=2)   # nothing caps the levels: 2 x 1500 and 390 fit, 5 x 6000 would not
    a.n_lvl = 5
    for l in range(5):
        a.level_a[l], a.level_h[l], a.level_w[l] = 3, 152, 200
        a.objectness[l] = a.box_regression[l] = a.anchors[l] = 256
    assert lib.veto_rpn_proposals(None, ctypes.byref(a), ctypes.c_void_p(256), 1 << 30) == -1
    assert b"8192" in lib.veto_last_error()
    good = _args()
    need = lib.veto_rpn_proposals_workspace_bytes(ctypes.byref(good))
    assert need >= 2 * 2 * 300 * 28
    assert lib.veto_rpn_proposals(None, ctypes.byref(good), ctypes.c_void_p(256), need - 1) == -4
    assert b"workspace too small" in lib.veto_last_error()
    assert lib.veto_rpn_proposals_workspace_bytes(ctypes.byref(_args(n_lvl=0))) == 0
