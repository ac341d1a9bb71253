"""sgdet training, the box head's sampler, host side: a numpy restatement of box_match_kernel and box_subsample_kernel
(FastRCNNSampling, roi_heads/box_head/sampling.py:14-156, with the kernels' hash and k-smallest select), pinned to the reference's
own outputs (tests/golden/boxsample/*.npz): matched_idxs and the labels of both conventions exactly, the sampled indices
wherever no draw decides them, regression_targets within the reference's own fp32 error.  Plus the C ABI's refusals, the config
keys, the reference-shaped classes of veto_amd.boxsampling, their argument checks and the registry installer."""
import ctypes
import glob
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_relsample_gtbox_host import np_pick  # noqa: E402

from veto_amd import native, synth, testing  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxsample")
PICK_POS, PICK_NEG = 0, 1     # the kernel's `purpose` of a draw
SEEDED = ("vg", "equal", "ragged", "one_gt", "gt256", "under_quota")
HAND = ("threshold", "ties")


# ---- the numpy restatement ---------------------------------------------------------------------------------------------

def np_iou(tgt, prp, dtype=np.float32):
    """boxlist_iou(target, proposal) [M, N] (boxlist_ops.py:54-89, TO_REMOVE 1) in `dtype` arithmetic."""
    t, p, one = np.asarray(tgt).astype(dtype), np.asarray(prp).astype(dtype), dtype(1)
    area_t = (t[:, 2] - t[:, 0] + one) * (t[:, 3] - t[:, 1] + one)
    area_p = (p[:, 2] - p[:, 0] + one) * (p[:, 3] - p[:, 1] + one)
    wh = np.maximum(np.minimum(t[:, None, 2:], p[None, :, 2:]) - np.maximum(t[:, None, :2], p[None, :, :2]) + one, dtype(0))
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_t[:, None] + area_p[None, :] - inter)


def np_box_match(prp, tgt, tgt_labels, high, low, weights=(10., 10., 5., 5.), dtype=np.float32):
    """One image of box_match_kernel: (matched_idxs, labels of assign_label_to_proposals, labels of prepare_targets,
    regression_targets), the thresholds rounded to fp32 as the kernel (and torch's comparison with a Python scalar) has them."""
    iou = np_iou(tgt, prp, dtype)
    arg = iou.argmax(0)                                    # the first = lowest GT index that reaches the maximum
    best = iou[arg, np.arange(iou.shape[1])]
    matched = np.where(best < dtype(np.float32(low)), -1, np.where(best < dtype(np.float32(high)), -2, arg)).astype(np.int64)
    g = np.maximum(matched, 0)
    lab = np.asarray(tgt_labels, np.int64)[g]
    assign = np.where(matched < 0, 0, lab)
    prepare = np.where(matched == -1, 0, np.where(matched == -2, -1, lab))
    t, p, one, half = np.asarray(tgt).astype(dtype)[g], np.asarray(prp).astype(dtype), dtype(1), dtype(0.5)
    wx, wy, ww, wh = (dtype(w) for w in weights)
    ex_w, ex_h = p[:, 2] - p[:, 0] + one, p[:, 3] - p[:, 1] + one
    ex_cx, ex_cy = p[:, 0] + half * ex_w, p[:, 1] + half * ex_h
    gt_w, gt_h = t[:, 2] - t[:, 0] + one, t[:, 3] - t[:, 1] + one
    gt_cx, gt_cy = t[:, 0] + half * gt_w, t[:, 1] + half * gt_h
    targets = np.stack([wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * np.log(gt_w / ex_w), wh * np.log(gt_h / ex_h)], 1)
    return matched, assign, prepare, targets.astype(dtype)


def np_quota(labels, batch, fraction):
    """(positives, negatives, num_pos, num_neg) of balanced_positive_negative_sampler.py:38-46."""
    labels = np.asarray(labels)
    pos, neg = np.nonzero(labels >= 1)[0], np.nonzero(labels == 0)[0]
    num_pos = min(len(pos), int(batch * fraction))
    return pos, neg, num_pos, min(len(neg), batch - num_pos)


def np_box_subsample(labels, img, seed, batch, fraction):
    """One image of box_subsample_kernel: the sampled proposal indices, ascending."""
    pos, neg, num_pos, num_neg = np_quota(labels, batch, fraction)
    if num_pos < len(pos):
        pos = np_pick(seed, img, PICK_POS, pos, num_pos)
    if num_neg < len(neg):
        neg = np_pick(seed, img, PICK_NEG, neg, num_neg)
    return np.sort(np.concatenate([pos, neg])).astype(np.int64)


def draw_free(labels, batch, fraction):
    """True when both classes are under quota: the sampled set is the same whatever the draws."""
    pos, neg, num_pos, num_neg = np_quota(labels, batch, fraction)
    return num_pos == len(pos) and num_neg == len(neg)


# ---- the fixtures ------------------------------------------------------------------------------------------------------

def load_case(name):
    """(fixture, images): the inputs of a seeded case are regenerated from its seeds, those of a hand-built one are stored."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    images = []
    for i in range(len(z["n_prp"])):
        if "seeds" in z.files:
            d = synth.synthetic_box_sampling_image(int(z["seeds"][i]), int(z["n_gt"][i]), int(z["n_det"][i]))
        else:
            d = {k: z["in_%s_%d" % (k, i)] for k in ("prp_boxes", "tgt_boxes", "tgt_labels", "attributes")}
            d["image_size"] = (800, 600)
        assert len(d["prp_boxes"]) == int(z["n_prp"][i])
        images.append(d)
    return z, images


def case_params(z):
    return float(z["high"]), float(z["low"]), int(z["batch"]), float(z["fraction"]), tuple(float(w) for w in z["weights"])


def box_lists(images, device="cpu"):
    props, targets = [], []
    for d in images:
        props.append(BoxList(torch.from_numpy(d["prp_boxes"]).to(device), d["image_size"], "xyxy"))
        t = BoxList(torch.from_numpy(d["tgt_boxes"]).to(device), d["image_size"], "xyxy")
        t.add_field("labels", torch.from_numpy(d["tgt_labels"]).to(device))
        t.add_field("attributes", torch.from_numpy(d["attributes"]).to(device))
        targets.append(t)
    return props, targets


def check_sampled_against_fixture(z, i, labels, sampled, batch, fraction):
    """What one image's sampled indices must share with the reference's whatever the draws (also used by the GPU tests)."""
    pos, neg, num_pos, num_neg = np_quota(labels, batch, fraction)
    want = z["sampled_%d" % i]
    assert len(sampled) == len(want) == num_pos + num_neg
    assert (np.diff(sampled) > 0).all()
    assert int((labels[sampled] >= 1).sum()) == int((labels[want] >= 1).sum()) == num_pos
    assert int((labels[sampled] == 0).sum()) == num_neg
    if draw_free(labels, batch, fraction):
        np.testing.assert_array_equal(sampled, want)


def test_every_fixture_is_present():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))) == sorted(SEEDED + HAND)


@pytest.mark.parametrize("name", SEEDED + HAND)
def test_numpy_restatement_reproduces_the_reference_fixture(name):
    z, images = load_case(name)
    high, low, batch, fraction, weights = case_params(z)
    worst = 0.0
    for i, d in enumerate(images):
        matched, assign, prepare, targets = np_box_match(d["prp_boxes"], d["tgt_boxes"], d["tgt_labels"], high, low, weights)
        np.testing.assert_array_equal(matched, z["matched_%d" % i])
        np.testing.assert_array_equal(assign, z["labels_assign_%d" % i])
        np.testing.assert_array_equal(prepare, z["labels_prepare_%d" % i])
        worst = max(worst, float(np.abs(targets.astype(np.float64) - z["targets_%d" % i]).max()))
        for seed in (0, 2 ** 63 + 5):
            check_sampled_against_fixture(z, i, prepare, np_box_subsample(prepare, i, seed, batch, fraction), batch, fraction)
    print("%s: restated fp32 regression_targets differ from the reference's by %.3g, its own fp32 error is %.3g"
          % (name, worst, float(z["ref_fp32_err_targets"])))
    assert worst <= float(z["ref_fp32_err_targets"])


def test_fixtures_cover_what_they_are_named_for():
    z, images = load_case("threshold")     # IoU exactly 0.5 and exactly 0.25, each on a threshold: `>=` keeps both sides
    assert case_params(z)[:2] == (0.5, 0.25)
    iou = np_iou(images[0]["tgt_boxes"], images[0]["prp_boxes"])
    assert iou[0, 0] == 0.5 and iou[0, 1] == 0.25
    assert z["matched_0"][0] == 0 and z["matched_0"][1] == -2 and z["labels_prepare_0"][1] == -1 and z["labels_assign_0"][1] == 0
    z, images = load_case("ties")          # duplicated GT boxes: the lowest index wins, with that box's label
    d = images[0]
    assert np.array_equal(d["tgt_boxes"][0], d["tgt_boxes"][1]) and d["tgt_labels"][0] != d["tgt_labels"][1]
    assert np.array_equal(d["prp_boxes"][0], d["tgt_boxes"][0]) and z["matched_0"][0] == 0 and z["labels_assign_0"][0] == d["tgt_labels"][0]
    assert np.array_equal(d["tgt_boxes"][3], d["tgt_boxes"][5]) and set(z["matched_0"].tolist()) >= {0, 2, 3} and 5 not in z["matched_0"]
    z, images = load_case("equal")
    assert case_params(z)[:2] == (0.5, 0.5) and not (z["matched_0"] == -2).any() and (z["matched_0"] == -1).any()
    z, _ = load_case("ragged")
    assert len(set(z["n_prp"].tolist())) == len(z["n_prp"]) > 2
    assert load_case("one_gt")[0]["n_gt"].tolist() == [1] and load_case("gt256")[0]["n_gt"].tolist() == [256]
    z, _ = load_case("under_quota")
    _, _, batch, fraction, _ = case_params(z)
    assert all(draw_free(z["labels_prepare_%d" % i], batch, fraction) for i in range(len(z["n_prp"])))
    z, _ = load_case("vg")                 # and one where the draws do decide, on both classes
    _, _, batch, fraction, _ = case_params(z)
    pos, neg, num_pos, num_neg = np_quota(z["labels_prepare_0"], batch, fraction)
    assert 0 < num_pos < len(pos) and 0 < num_neg < len(neg) and (z["matched_0"] == -2).any()


def test_numpy_subsample_follows_the_quota_formulas_and_the_seed():
    labels = np.array([3, 0, 0, -1, 7, 0, 0, 1, 0, -1, 0, 2, 0, 0, 9, 0], np.int64)
    for batch, fraction, want in ((8, 0.25, (2, 6)), (4, 0.5, (2, 2)), (64, 0.25, (5, 9)), (8, 0.0, (0, 8)), (8, 1.0, (5, 3)), (1, 0.25, (0, 1))):
        got = np_box_subsample(labels, 0, 11, batch, fraction)
        assert (int((labels[got] >= 1).sum()), int((labels[got] == 0).sum())) == want, (batch, fraction)
        assert (np.diff(got) > 0).all()
    a, b = np_box_subsample(labels, 0, 11, 8, 0.25), np_box_subsample(labels, 0, 11, 8, 0.25)
    others = [np_box_subsample(labels, 0, s, 8, 0.25) for s in range(12, 20)] + [np_box_subsample(labels, i, 11, 8, 0.25) for i in range(1, 9)]
    assert np.array_equal(a, b) and any(not np.array_equal(a, o) for o in others[:8]) and any(not np.array_equal(a, o) for o in others[8:])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def _match_args(n_prp=(3,), n_tgt=(2,), **kw):
    a = native.VetoBoxMatchArgs()
    a.struct_size = ctypes.sizeof(native.VetoBoxMatchArgs)
    a.n_img, a.n_prp, a.n_tgt, a.mode, a.high_threshold, a.low_threshold = len(n_prp), sum(n_prp), sum(n_tgt), 0, 0.5, 0.3
    keep = [np.concatenate([[0], np.cumsum(n_prp)]).astype(np.int32), np.concatenate([[0], np.cumsum(n_tgt)]).astype(np.int32)]
    a.img_prp_offset_host, a.img_tgt_offset_host = keep[0].ctypes.data, keep[1].ctypes.data
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep


def test_box_match_abi_rejects_bad_arguments_without_a_gpu():
    """Every check comes before the launch: the device pointers here are null, so a launch would not be survivable."""
    lib = native.load_library()
    for sizes, kw, needle in (((), dict(struct_size=8), b"veto_box_match_args_t size mismatch"),
                              ((), dict(n_img=0), b"bad sizes"),
                              ((), dict(mode=2), b"mode must be 0"),
                              ((), dict(low_threshold=0.7), b"must be <= high_threshold"),
                              ((), dict(img_tgt_offset_host=None), b"host offsets"),
                              (((3, 4), (257, 2)), {}, b"img_tgt_offset_host: segment 0 holds 257 boxes, the limit is 256"),
                              (((3, 6145), (2, 2)), {}, b"img_prp_offset_host: segment 1 holds 6145 boxes, the limit is 6144"),
                              (((3, 4), (2, 0)), {}, b"No ground-truth boxes available for one of the images during training"),
                              (((0, 4), (2, 2)), {}, b"No proposal boxes available for one of the images during training"),
                              (((6144, 1), (256, 1)), {}, b"missing pointer")):
        a, keep = _match_args(*sizes, **kw)
        assert lib.veto_box_match(None, ctypes.byref(a)) == -1, (sizes, kw)      # VETO_ERR_INVALID
        assert needle in lib.veto_last_error(), (sizes, kw, lib.veto_last_error())
    assert lib.veto_box_match(None, None) == -1


def test_box_subsample_abi_rejects_bad_arguments_without_a_gpu():
    lib = native.load_library()

    def args(n_prp=(5,), **kw):
        a = native.VetoBoxSubsampleArgs()
        a.struct_size = ctypes.sizeof(native.VetoBoxSubsampleArgs)
        a.n_img, a.n_prp, a.batch_size_per_image, a.num_pos_per_img = len(n_prp), sum(n_prp), 256, 64
        keep = np.concatenate([[0], np.cumsum(n_prp)]).astype(np.int32)
        a.img_prp_offset_host = keep.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a, keep

    for n_prp, kw, needle in (((5,), dict(struct_size=8), b"veto_box_subsample_args_t size mismatch"),
                              ((5,), dict(n_img=0), b"bad sizes"),
                              ((5,), dict(batch_size_per_image=2049), b"batch_size_per_image 2049 outside 1..2048"),
                              ((5,), dict(batch_size_per_image=0), b"batch_size_per_image 0 outside 1..2048"),
                              ((5,), dict(num_pos_per_img=257), b"num_pos_per_img 257 outside 0..256"),
                              ((5, 6145), {}, b"img_prp_offset_host: segment 1 holds 6145 boxes, the limit is 6144"),
                              ((5, 0), {}, b"No proposal boxes available"),
                              ((6144, 1), dict(batch_size_per_image=2048, num_pos_per_img=2048), b"missing pointer")):
        a, keep = args(n_prp, **kw)
        assert lib.veto_box_subsample(None, ctypes.byref(a)) == -1, (n_prp, kw)
        assert needle in lib.veto_last_error(), (n_prp, kw, lib.veto_last_error())
    assert lib.veto_box_subsample(None, None) == -1


# ---- the classes, the factory, the installer ---------------------------------------------------------------------------

def test_classes_have_the_reference_interface():
    from veto_amd import boxsampling as bs
    assert list(inspect.signature(bs.Matcher.__init__).parameters) == ["self", "high_threshold", "low_threshold", "allow_low_quality_matches"]
    assert (bs.Matcher.BELOW_LOW_THRESHOLD, bs.Matcher.BETWEEN_THRESHOLDS) == (-1, -2)
    assert list(inspect.signature(bs.FastRCNNSampling.__init__).parameters) == ["self", "proposal_matcher", "fg_bg_sampler", "box_coder"]
    assert list(inspect.signature(bs.FastRCNNSampling.match_targets_to_proposals).parameters) == ["self", "proposal", "target"]
    for method in ("prepare_targets", "assign_label_to_proposals"):
        assert list(inspect.signature(getattr(bs.FastRCNNSampling, method)).parameters) == ["self", "proposals", "targets"]
    assert list(inspect.signature(bs.FastRCNNSampling.subsample).parameters) == ["self", "proposals", "targets", "seed"]
    assert list(inspect.signature(bs.make_roi_box_samp_processor).parameters) == ["cfg"]


def test_factory_reads_the_box_heads_keys():
    from veto_amd import boxsampling as bs
    cfg = testing.make_config(2, 8)
    rh = cfg.MODEL.ROI_HEADS
    assert (rh.FG_IOU_THRESHOLD, rh.BG_IOU_THRESHOLD, tuple(rh.BBOX_REG_WEIGHTS), rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION) == \
        (0.5, 0.3, (10., 10., 5., 5.), 256, 0.25)                      # the reference's defaults, defaults.py:202-216
    rh.FG_IOU_THRESHOLD, rh.BG_IOU_THRESHOLD, rh.BBOX_REG_WEIGHTS, rh.BATCH_SIZE_PER_IMAGE, rh.POSITIVE_FRACTION = 0.6, 0.2, (1., 2., 3., 4.), 512, 0.5
    s = bs.make_roi_box_samp_processor(cfg)
    assert isinstance(s, bs.FastRCNNSampling) and isinstance(s.proposal_matcher, bs.Matcher)
    assert (s.proposal_matcher.high_threshold, s.proposal_matcher.low_threshold, s.proposal_matcher.allow_low_quality_matches) == (0.6, 0.2, False)
    assert (s.fg_bg_sampler.batch_size_per_image, s.fg_bg_sampler.positive_fraction, s.box_coder.weights) == (512, 0.5, (1., 2., 3., 4.))


def test_allow_low_quality_matches_is_refused():
    from veto_amd import boxsampling as bs
    with pytest.raises(NotImplementedError, match="allow_low_quality_matches"):
        bs.Matcher(0.7, 0.3, allow_low_quality_matches=True)
    with pytest.raises(NotImplementedError, match="allow_low_quality_matches"):
        bs.FastRCNNSampling(types.SimpleNamespace(high_threshold=0.7, low_threshold=0.3, allow_low_quality_matches=True),
                            bs.BalancedPositiveNegativeSampler(256, 0.25), bs.BoxCoder((10., 10., 5., 5.)))
    with pytest.raises(AssertionError):
        bs.Matcher(0.3, 0.5)                                           # matcher.py:37


def test_sampler_checks_its_arguments_before_touching_the_library(monkeypatch):
    from veto_amd import boxsampling as bs

    def no_library():
        raise AssertionError("the library must not be loaded before the arguments are checked")
    monkeypatch.setattr(native, "load_library", no_library)
    s = bs.make_roi_box_samp_processor(testing.make_config(2, 8))
    props, targets = box_lists(load_case("ragged")[1])
    empty_t = BoxList(torch.zeros((0, 4)), (800, 600))
    empty_t.add_field("labels", torch.zeros(0, dtype=torch.int64))
    for call in (s.assign_label_to_proposals, s.prepare_targets, s.subsample):
        with pytest.raises(ValueError, match="one target per proposal list"):
            call(props, targets[:1])
        with pytest.raises(ValueError, match="one target per proposal list"):
            call([], [])
        with pytest.raises(ValueError, match="No ground-truth boxes available for one of the images during training"):
            call(props[:2], [targets[0], empty_t])
        with pytest.raises(ValueError, match="No proposal boxes available for one of the images during training"):
            call([props[0], BoxList(torch.zeros((0, 4)), (800, 600))], targets[:2])
        with pytest.raises(RuntimeError, match="boxlists should have same image size"):
            call([BoxList(props[0].bbox, (640, 480))], targets[:1])
        with pytest.raises(RuntimeError, match="runs on a HIP device only"):
            call(props, targets)
    with pytest.raises(RuntimeError, match="match_targets_to_proposals runs on a HIP device only"):
        s.match_targets_to_proposals(props[0], targets[0])
    for budget in (0, 2049):
        big = bs.FastRCNNSampling(s.proposal_matcher, bs.BalancedPositiveNegativeSampler(budget, 0.25), s.box_coder)
        with pytest.raises(ValueError, match=r"batch_size_per_image %d outside 1\.\.2048" % budget):
            big.subsample(props, targets)


def test_installer_points_the_reference_factory_at_the_device_sampler(monkeypatch):
    from veto_amd import boxsampling, registry
    names = ["pysgg", "pysgg.modeling", "pysgg.modeling.roi_heads", "pysgg.modeling.roi_heads.box_head",
             "pysgg.modeling.roi_heads.box_head.sampling", "pysgg.modeling.roi_heads.box_head.box_head",
             "pysgg.modeling.roi_heads.box_head.inference", "pysgg.modeling.rpn", "pysgg.modeling.rpn.inference"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
    samp, head = mods["pysgg.modeling.roi_heads.box_head.sampling"], mods["pysgg.modeling.roi_heads.box_head.box_head"]
    samp.make_roi_box_samp_processor = head.make_roi_box_samp_processor = original = object()
    head.make_roi_box_post_processor = post = object()
    patched = registry.install_box_sampling_ops()
    assert patched == [("pysgg.modeling.roi_heads.box_head.sampling", "make_roi_box_samp_processor"),
                       ("pysgg.modeling.roi_heads.box_head.box_head", "make_roi_box_samp_processor")]
    assert samp.make_roi_box_samp_processor is head.make_roi_box_samp_processor is boxsampling.make_roi_box_samp_processor
    assert samp.make_roi_box_samp_processor is not original and head.make_roi_box_post_processor is post   # the others stay
