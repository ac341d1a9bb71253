"""The RPN loss, host side: the numpy restatement of the matching (rpnloss_cases.np_rpn_match) and the float64 oracle of the losses
(rpnloss_cases.rpn_loss_fp64) pinned to the reference's own outputs (tests/golden/rpnloss/*.npz), the negative control of the
low-quality step, the premises the GPU tests rest on, the C ABI's refusals, the reference-shaped classes of veto_amd.rpnloss,
their argument checks and the registry installer."""
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
import rpnloss_cases as rc  # noqa: E402

from veto_amd import native  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402


def _n_img(z):
    return len([k for k in z.files if k.startswith("labels_")])


def test_every_fixture_is_present():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(rc.GOLDEN, "*.npz"))) == sorted(rc.ALL)
    assert all(os.path.getsize(p) < 256 * 1024 for p in glob.glob(os.path.join(rc.GOLDEN, "*.npz")))


@pytest.mark.parametrize("name", rc.ALL)
def test_numpy_restatement_reproduces_the_reference_fixture(name):
    z, c, d = rc.load_case(name)
    anchors = np.concatenate(d["anchors"])
    worst = 0.0
    for i in range(_n_img(z)):
        matched, labels, targets, _ = rc.np_rpn_match(anchors, d["tgt_boxes"][i], d["image_sizes"][i], c["high"], c["low"], c["lowq"], c["straddle"])
        np.testing.assert_array_equal(matched, z["matched_%d" % i])
        np.testing.assert_array_equal(labels, z["labels_%d" % i].astype(np.float32))
        worst = max(worst, float(np.abs(targets.astype(np.float64) - z["targets_%d" % i]).max()))
    print("%s: restated fp32 regression_targets differ from the reference's by %.3g, its own fp32 error is %.3g"
          % (name, worst, float(z["ref_fp32_err_targets"])))
    assert worst <= float(z["ref_fp32_err_targets"])


@pytest.mark.parametrize("name", rc.ALL)
def test_fp64_oracle_reproduces_the_reference_losses_and_gradients(name):
    """rpn_loss_fp64 at the reference's sampled anchors against the reference's own float64 run: the losses to 1e-12 relative, the
    gradients at the sampled positions to 1e-12 of the largest, and zero everywhere else."""
    z, c, d = rc.load_case(name)
    n, shapes = _n_img(z), d["level_shapes"]
    sampled = [z["sampled_%d" % i] for i in range(n)]
    lo, lb, g_obj, g_box = rc.rpn_loss_fp64(d["objectness"], d["box_regression"], shapes, sampled,
                                            [z["labels_%d" % i] for i in range(n)], [z["targets_%d" % i] for i in range(n)])
    want = z["losses_fp64"]
    assert abs(lo - want[0]) <= 1e-12 * abs(want[0]) and abs(lb - want[1]) <= 1e-12 * max(abs(want[1]), 1e-30)
    touched_obj, touched_box = 0, 0
    for i in range(n):
        go, gb = rc.gather_nchw(g_obj, shapes, i, sampled[i], 1)[:, 0], rc.gather_nchw(g_box, shapes, i, sampled[i], 4)
        np.testing.assert_allclose(go, z["grad_objectness_%d" % i], rtol=0, atol=1e-12 * np.abs(z["grad_objectness_%d" % i]).max())
        np.testing.assert_allclose(gb, z["grad_box_regression_%d" % i], rtol=0, atol=1e-12 * max(np.abs(z["grad_box_regression_%d" % i]).max(), 1e-30))
        touched_obj += int((go != 0).sum())
        touched_box += int((gb != 0).sum())
    assert sum(int((g != 0).sum()) for g in g_obj) == touched_obj and sum(int((g != 0).sum()) for g in g_box) == touched_box
    assert abs(float(z["losses_fp32"][0]) - want[0]) <= float(z["ref_fp32_err_loss"]) * abs(want[0]) * (1 + 1e-9)


def test_without_the_low_quality_step_the_restatement_differs():
    """The negative control: with the step switched off, lowq and zero_gt lose the matches they are named for."""
    for name in ("lowq", "zero_gt"):
        z, c, d = rc.load_case(name)
        matched, labels, _, plain = rc.np_rpn_match(d["anchors"][0], d["tgt_boxes"][0], d["image_sizes"][0], c["high"], c["low"], False, c["straddle"])
        assert np.array_equal(matched, plain)
        assert not np.array_equal(matched, z["matched_0"]) and not np.array_equal(labels, z["labels_0"].astype(np.float32)), name
    z, _, _ = rc.load_case("lowq")
    assert z["matched_0"].tolist() == [0, 0, 1, -1, -1, -2, -1]
    z, _, _ = rc.load_case("zero_gt")
    assert (z["matched_0"] >= 0).all() and z["labels_0"].tolist() == [1, 1, 1, -1, 1]


def test_fixtures_cover_what_they_are_named_for():
    z, c, d = rc.load_case("fpn5")
    assert len(d["anchors"]) == 5 and sum(len(a) for a in d["anchors"]) == 12276 and [len(t) for t in d["tgt_boxes"]] == [3, 8]
    assert not np.array_equal(z["labels_0"] == -1, z["labels_1"] == -1)            # the images' sizes differ, so visibility does
    assert all((z["labels_%d" % i] == 1).any() and (z["matched_%d" % i] == -2).any() for i in range(2))
    z, c, d = rc.load_case("one_level")
    assert d["level_shapes"] == [(9, 12, 16)]
    z, c, d = rc.load_case("ragged_gt")
    assert [len(t) for t in d["tgt_boxes"]] == [1, 12, 256, 5] and int(z["matched_2"].max()) > 127
    z, c, d = rc.load_case("thresholds")
    iou = rc.np_iou(d["tgt_boxes"][0], d["anchors"][0])
    assert iou[0, 0] == np.float32(c["high"]) and iou[0, 1] == np.float32(c["low"]) and z["matched_0"].tolist() == [0, -2, 0, -1, 0, -1]
    z, c, d = rc.load_case("no_pos")
    assert not c["lowq"] and not (z["labels_0"] == 1).any() and z["losses_fp32"][1] == 0 and z["losses_fp64"][1] == 0


@pytest.mark.parametrize("name", rc.ALL)
def test_premises_of_the_gpu_inputs(name):
    """What lets the GPU tests ask for bit-equal matching and a tight loss bound: no IoU within rounding of a threshold (the
    float64 matching before the low-quality step equals the fp32 one), and no sampled residual within 1e-5 of the smooth-L1 kink."""
    z, c, d = rc.load_case(name)
    anchors = np.concatenate(d["anchors"])
    for i in range(_n_img(z)):
        args = (anchors, d["tgt_boxes"][i], d["image_sizes"][i], c["high"], c["low"], c["lowq"], c["straddle"])
        np.testing.assert_array_equal(rc.np_rpn_match(*args)[3], rc.np_rpn_match(*args, dtype=np.float64)[3])
        pos = np.nonzero(z["labels_%d" % i] == 1)[0]                                # every positive: whatever a sampler picks
        resid = np.abs(rc.gather_nchw(d["box_regression"], d["level_shapes"], i, pos, 4).astype(np.float64) - z["targets_%d" % i][pos])
        assert not np.any(np.abs(resid - rc.BETA) < 1e-5)
        if len(pos):
            assert (resid < rc.BETA).any() or name in rc.HAND                       # both branches of smooth-L1 are exercised
    assert float(z["ref_fp32_err_loss"]) > 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def _abi_args(n_tgt=(3,), levels=((3, 4, 5),), **kw):
    a = native.VetoRpnLossArgs()
    a.struct_size = ctypes.sizeof(native.VetoRpnLossArgs)
    a.n_img, a.n_lvl, a.n_tgt, a.batch_size_per_image, a.num_pos_per_img = len(n_tgt), len(levels), sum(n_tgt), 256, 128
    a.high_threshold, a.low_threshold, a.beta, a.allow_low_quality_matches = 0.7, 0.3, 1.0 / 9, 1
    for l, (A, H, W) in enumerate(levels[:native.RPN_MAX_LEVELS]):
        a.level_a[l], a.level_h[l], a.level_w[l] = A, H, W
        a.anchors[l] = 4096                                                         # never dereferenced: every refusal comes first
    keep = np.concatenate([[0], np.cumsum(n_tgt)]).astype(np.int32)
    a.img_tgt_offset_host = keep.ctypes.data
    a.labels = 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep


def test_rpn_loss_abi_rejects_bad_arguments_without_a_gpu():
    """Every check comes before the launch: the device pointers here are null or made up, so a launch would not be survivable."""
    lib = native.load_library()
    for sizes, kw, needle in ((dict(), dict(struct_size=8), b"veto_rpn_loss_args_t size mismatch"),
                              (dict(), dict(n_img=0), b"n_img 0 outside 1..65535"),
                              (dict(), dict(n_lvl=9), b"n_lvl 9 outside 1..8"),
                              (dict(), dict(n_lvl=0), b"n_lvl 0 outside 1..8"),
                              (dict(), dict(batch_size_per_image=2049), b"batch_size_per_image 2049 outside 1..2048"),
                              (dict(), dict(batch_size_per_image=0), b"batch_size_per_image 0 outside 1..2048"),
                              (dict(), dict(num_pos_per_img=257), b"num_pos_per_img 257 outside 0..256"),
                              (dict(), dict(low_threshold=0.8), b"must be <= high_threshold"),
                              (dict(levels=((3, 0, 5),)), {}, b"level 0: bad shape"),
                              (dict(levels=((1, 1, 1048576), (1, 1, 1))), {}, b"an image holds 1048577 anchors, the limit is 1048576"),
                              (dict(), dict(img_tgt_offset_host=None), b"img_tgt_offset_host"),
                              (dict(n_tgt=(3, 257)), {}, b"img_tgt_offset_host: segment 1 holds 257 boxes, the limit is 256"),
                              (dict(n_tgt=(3, 0)), {}, b"No ground-truth boxes available for one of the images during training"),
                              (dict(), dict(labels=None), b"no output requested"),
                              (dict(), dict(losses=4096), b"missing pointer: level 0"),
                              (dict(), dict(counts=4096), b"missing pointer"),
                              (dict(n_tgt=(256, 1), levels=((1, 1, 1048576),)), dict(counts=4096), b"missing pointer")):
        a, keep = _abi_args(**sizes, **kw)
        assert lib.veto_rpn_loss(None, ctypes.byref(a), None, 0) == -1, (sizes, kw)          # VETO_ERR_INVALID
        assert needle in lib.veto_last_error(), (sizes, kw, lib.veto_last_error())
    a, keep = _abi_args()
    a.d_objectness[0] = 4096                                                        # half of the gradients
    assert lib.veto_rpn_loss(None, ctypes.byref(a), None, 0) == -1 and b"every level of both or none" in lib.veto_last_error()
    a.d_box_regression[0] = 4096
    assert lib.veto_rpn_loss(None, ctypes.byref(a), None, 0) == -1 and b"losses (required with the gradients)" in lib.veto_last_error()
    a, keep = _abi_args(image_sizes=4096, tgt_boxes=4096, img_tgt_offset=4096)
    assert lib.veto_rpn_loss(None, ctypes.byref(a), None, 0) == -4 and b"workspace too small" in lib.veto_last_error()
    assert lib.veto_rpn_loss(None, None, None, 0) == -1
    # the workspace: gtmax | labels | matched | sampled | counts | partial | hist, each rounded up to 256 bytes
    assert lib.veto_rpn_loss_workspace_bytes(ctypes.byref(a)) == 256 + 2 * 256 + 1024 + 256 + 256 + 2048
    assert lib.veto_rpn_loss_workspace_bytes(ctypes.byref(_abi_args(n_lvl=9)[0])) == 0


# ---- the classes, the factory, the installer ---------------------------------------------------------------------------

def _cfg(**kw):
    rpn = dict(FG_IOU_THRESHOLD=0.7, BG_IOU_THRESHOLD=0.3, BATCH_SIZE_PER_IMAGE=256, POSITIVE_FRACTION=0.5, STRADDLE_THRESH=0)
    rpn.update(kw)
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN=types.SimpleNamespace(**rpn)))


def _lists(name="lowq", device="cpu"):
    _, c, d = rc.load_case(name)
    anchors = [[BoxList(torch.from_numpy(a).to(device), size, "xyxy") for a in d["anchors"]] for size in d["image_sizes"]]
    targets = [BoxList(torch.from_numpy(t).to(device), size, "xyxy") for t, size in zip(d["tgt_boxes"], d["image_sizes"])]
    return anchors, [torch.from_numpy(o).to(device) for o in d["objectness"]], [torch.from_numpy(r).to(device) for r in d["box_regression"]], targets


def test_classes_have_the_reference_interface():
    from veto_amd import rpnloss as rl
    assert list(inspect.signature(rl.RPNLossComputation.__init__).parameters) == ["self", "proposal_matcher", "fg_bg_sampler", "box_coder",
                                                                                  "generate_labels_func"]
    assert list(inspect.signature(rl.RPNLossComputation.prepare_targets).parameters) == ["self", "anchors", "targets"]
    assert list(inspect.signature(rl.RPNLossComputation.__call__).parameters)[:5] == ["self", "anchors", "objectness", "box_regression", "targets"]
    assert list(inspect.signature(rl.make_rpn_loss_evaluator).parameters) == ["cfg", "box_coder"]
    assert list(inspect.signature(rl.Matcher.__init__).parameters) == ["self", "high_threshold", "low_threshold", "allow_low_quality_matches"]
    assert (rl.Matcher.BELOW_LOW_THRESHOLD, rl.Matcher.BETWEEN_THRESHOLDS) == (-1, -2)
    # (the reference is not importable where the tests run: loss.py:26-27, :56, :92 and :140 are restated above)
    assert rl.RPNLossComputation(rl.Matcher(0.7, 0.3, True), rl.BalancedPositiveNegativeSampler(256, 0.5), rl.BoxCoder((1., 1., 1., 1.)),
                                 rl.generate_rpn_labels).discard_cases == ['not_visibility', 'between_thresholds']


def test_factory_reads_the_rpn_keys_and_accepts_both_matcher_settings():
    from veto_amd import rpnloss as rl
    coder = rl.BoxCoder((1., 1., 1., 1.))
    s = rl.make_rpn_loss_evaluator(_cfg(FG_IOU_THRESHOLD=0.6, BG_IOU_THRESHOLD=0.2, BATCH_SIZE_PER_IMAGE=512, POSITIVE_FRACTION=0.25,
                                        STRADDLE_THRESH=-1), coder)
    assert isinstance(s, rl.RPNLossComputation) and isinstance(s.proposal_matcher, rl.Matcher) and s.box_coder is coder
    assert (s.proposal_matcher.high_threshold, s.proposal_matcher.low_threshold, s.proposal_matcher.allow_low_quality_matches) == (0.6, 0.2, True)
    assert (s.fg_bg_sampler.batch_size_per_image, s.fg_bg_sampler.positive_fraction, s.straddle_thresh) == (512, 0.25, -1)
    assert s.generate_labels_func is rl.generate_rpn_labels
    for lowq in (True, False):
        assert rl.RPNLossComputation(rl.Matcher(0.7, 0.3, lowq), s.fg_bg_sampler, coder, rl.generate_rpn_labels).proposal_matcher.allow_low_quality_matches is lowq
    with pytest.raises(AssertionError):
        rl.Matcher(0.3, 0.7)                                                        # matcher.py:37

    def generate_retinanet_labels(matched_targets):
        return matched_targets.get_field("labels")
    with pytest.raises(NotImplementedError, match="only generate_rpn_labels"):
        rl.RPNLossComputation(s.proposal_matcher, s.fg_bg_sampler, coder, generate_retinanet_labels)


def test_loss_checks_its_arguments_before_touching_the_library(monkeypatch):
    from veto_amd import rpnloss as rl

    def no_library():
        raise AssertionError("the library must not be loaded before the arguments are checked")
    monkeypatch.setattr(native, "load_library", no_library)
    s = rl.make_rpn_loss_evaluator(_cfg(), rl.BoxCoder((1., 1., 1., 1.)))
    anchors, obj, reg, targets = _lists()
    size = targets[0].size
    empty = BoxList(torch.zeros((0, 4)), size)
    many = BoxList(torch.tensor([[0., 0., 9., 9.]]).repeat(257, 1), size)
    for call in (lambda a, t: s.prepare_targets(a, t), lambda a, t: s(a, obj, reg, t)):
        with pytest.raises(ValueError, match="No ground-truth boxes available for one of the images during training"):
            call(anchors, [empty])
        with pytest.raises(ValueError, match="image 0 holds 257 GT boxes, the limit is 256"):
            call(anchors, [many])
        with pytest.raises(ValueError, match="one target per image"):
            call(anchors, targets + targets)
        with pytest.raises(RuntimeError, match="boxlists should have same image size"):
            call(anchors, [BoxList(targets[0].bbox, (640, 480))])
        with pytest.raises(ValueError, match=r"9 pyramid levels: 1\.\.8 are supported"):
            call([anchors[0] * 9], targets)
        with pytest.raises(ValueError, match="an image holds 1048577 anchors, the limit is 1048576"):
            call([[BoxList(torch.zeros((1048577, 4)), size)]], targets)
        with pytest.raises(RuntimeError, match="RPN loss runs on a HIP device only"):
            call(anchors, targets)
    for budget in (0, 2049):
        big = rl.RPNLossComputation(s.proposal_matcher, rl.BalancedPositiveNegativeSampler(budget, 0.5), s.box_coder, rl.generate_rpn_labels)
        with pytest.raises(ValueError, match=r"batch_size_per_image %d outside 1\.\.2048" % budget):
            big(anchors, obj, reg, targets)
    with pytest.raises(ValueError, match=r"box_regression\[0\] must be"):
        s(anchors, obj, obj, targets)


def test_installer_points_the_reference_factory_at_the_device_loss(monkeypatch):
    from veto_amd import registry, rpnloss
    names = ["pysgg", "pysgg.modeling", "pysgg.modeling.rpn", "pysgg.modeling.rpn.loss", "pysgg.modeling.rpn.rpn", "pysgg.modeling.rpn.inference"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
    loss, head, inference = mods["pysgg.modeling.rpn.loss"], mods["pysgg.modeling.rpn.rpn"], mods["pysgg.modeling.rpn.inference"]
    loss.make_rpn_loss_evaluator = head.make_rpn_loss_evaluator = original = object()
    inference.make_rpn_postprocessor = head.make_rpn_postprocessor = post = object()
    patched = registry.install_rpn_loss_ops()
    assert patched == [("pysgg.modeling.rpn.loss", "make_rpn_loss_evaluator"), ("pysgg.modeling.rpn.rpn", "make_rpn_loss_evaluator")]
    assert loss.make_rpn_loss_evaluator is head.make_rpn_loss_evaluator is rpnloss.make_rpn_loss_evaluator
    assert loss.make_rpn_loss_evaluator is not original
    assert inference.make_rpn_postprocessor is head.make_rpn_postprocessor is post   # the other installers' targets stay
