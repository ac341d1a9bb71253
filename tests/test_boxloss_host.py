"""The box head's loss without a GPU: the fixtures of tests/golden/boxloss (the reference's own FastRCNNLossComputation on CPU
tensors) against the float64 oracle boxloss_cases.box_loss_fp64, what each fixture is named for, four wrong restatements of the
oracle, the argument checks of veto_box_loss, and the interface, the factory and the installer of veto_amd.boxloss."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxloss_cases as bc  # noqa: E402

from veto_amd import native  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402


# ---- the fixtures and the oracle ---------------------------------------------------------------------------------------------

def test_every_fixture_is_present():
    assert sorted(f[:-4] for f in os.listdir(bc.GOLDEN) if f.endswith(".npz")) == sorted(bc.ALL)
    for name in bc.ALL:
        z, d = bc.load_case(name)
        R = sum(len(x) for x in d["labels"])
        C = d["class_logits"][0].shape[1]
        assert z["losses_fp32"].dtype == np.float32 and z["losses_fp64"].dtype == np.float64
        assert len(z["rows"]) == (R if R * 4 * C <= bc.FULL_GRADS else len(bc.grad_rows(name, d))) and set(d["forced_rows"]) <= set(z["rows"].tolist())
        assert z["d_class_logits_fp64"].shape == (len(z["rows"]), C)
        assert z["d_box_regression_fp64"].shape == (len(z["rows"]), 8 if d["agnostic"] else 4 * C)
        for k in ("ref_fp32_err_loss", "ref_fp32_err_dlogits", "ref_fp32_err_dbox"):
            assert 0 <= float(z[k]) < 1e-4, (name, k, z[k])


@pytest.mark.parametrize("name", bc.ALL)
def test_the_oracle_reproduces_the_reference_float64_run(name):
    """Losses to 1e-12 relative; d_box_regression to 1e-12 relative at its elements, exactly 0 elsewhere; d_class_logits to 1e-12 of
    (p + onehot) / R, the magnitude of its terms before they cancel."""
    z, d = bc.load_case(name)
    o = bc.box_loss_fp64(*bc.concatenated(d), agnostic=d["agnostic"])
    rows = z["rows"]
    assert bc.loss_err(o["losses"], z["losses_fp64"]) <= 1e-12
    assert bc.dbox_err(o["d_box_regression"][rows], z["d_box_regression_fp64"]) <= 1e-12
    p, onehot = o["p"][rows], o["onehot"][rows]
    R = len(o["p"])
    assert bc.dlogits_err(o["d_class_logits"][rows], z["d_class_logits_fp64"], p, onehot, R) <= 1e-12
    assert bc.loss_err(z["losses_fp32"], z["losses_fp64"]) == float(z["ref_fp32_err_loss"])


def test_the_fixtures_cover_what_they_are_named_for():
    def labels(name):
        return np.concatenate(bc.case_inputs(name)["labels"])
    for name in ("vg", "agnostic"):
        d = bc.case_inputs(name)
        assert [len(x) for x in d["labels"]] == [64, 64] and d["class_logits"][0].shape[1] == 151
        assert 0.15 < (labels(name) > 0).mean() < 0.35
    assert bc.case_inputs("agnostic")["box_regression"][0].shape == (64, 8) and bc.case_inputs("agnostic")["agnostic"]
    assert bc.case_inputs("vg")["box_regression"][0].shape == (64, 604)
    assert set(labels("two_cls").tolist()) == {0, 1} and bc.case_inputs("two_cls")["class_logits"][0].shape == (5, 2)
    for C in (63, 64, 65):
        d = bc.case_inputs("lanes%d" % C)
        assert d["class_logits"][0].shape == (7, C) and {0, C - 1, min(63, C - 1)} <= set(labels("lanes%d" % C).tolist())
    assert bc.case_inputs("wide")["class_logits"][0].shape == (9, 1024) and {1023, 960} <= set(labels("wide").tolist())
    z, _ = bc.load_case("no_pos")
    assert not (labels("no_pos") > 0).any() and z["losses_fp64"][1] == 0 and z["losses_fp32"][1] == 0 and not z["d_box_regression_fp64"].any()
    assert (labels("all_pos") > 0).all()
    assert [len(x) for x in bc.case_inputs("ragged")["labels"]] == [1, 0, 130]
    d = bc.case_inputs("sharp")
    logits, _, y, _ = bc.concatenated(d)
    c = bc.SEEDED["sharp"]
    assert logits[c["shifted_row"]].max() > 9000 and logits[c["shifted_row"]].max() > np.log(np.finfo(np.float32).max)
    gone = np.nonzero(np.isneginf(logits[c["inf_row"]]))[0]
    assert len(gone) == 1 and gone[0] != y[c["inf_row"]] and np.abs(logits[np.isfinite(logits)]).max() > 60
    z, _ = bc.load_case("sharp")
    assert np.isfinite(z["losses_fp64"]).all() and np.isfinite(z["losses_fp32"]).all()
    assert z["d_class_logits_fp64"][list(z["rows"]).index(c["inf_row"]), gone[0]] == 0
    d = bc.case_inputs("kink")
    _, x, y, t = bc.concatenated(d)
    got = {float(np.float64(x[r, 4 * y[r] + k]) - np.float64(t[r, k])) for r in np.nonzero(y > 0)[0] for k in range(4)}
    assert set(bc.KINK_D) <= got and len(y) == 16
    z, _ = bc.load_case("kink")
    assert z["losses_fp32"][1] == np.float32(z["losses_fp64"][1]) == np.float32(0.517578125) and float(z["ref_fp32_err_dbox"]) == 0 and float(z["ref_fp32_err_dlogits"]) == 0


@pytest.mark.parametrize("name,wrong", [("vg", dict(beta=1.0 / 9)), ("vg", dict(box_norm="positives")), ("agnostic", "class_columns"),
                                        ("vg", dict(ce_over="positives"))])
def test_a_wrong_restatement_changes_the_result(name, wrong):
    """beta 1/9 (the RPN's), division by the number of positives, class-specific columns under agnostic regression, cross entropy
    averaged over the positives only: each moves a loss far beyond the tolerance of the test above."""
    z, d = bc.load_case(name)
    logits, reg, y, t = bc.concatenated(d)
    if wrong == "class_columns":
        wide = np.zeros((len(reg), 4 * logits.shape[1]), np.float32)
        wide[:, :8] = reg
        o = bc.box_loss_fp64(logits, wide, y, t, agnostic=False)
    else:
        o = bc.box_loss_fp64(logits, reg, y, t, agnostic=d["agnostic"], **wrong)
    rel = np.abs(o["losses"] - z["losses_fp64"]) / np.abs(z["losses_fp64"])
    assert rel.max() > 1e-3, (wrong, rel)


# ---- the ABI's argument checks -------------------------------------------------------------------------------------------------

def _abi_args(**over):
    """Arguments that pass every check up to the workspace: made-up, aligned device addresses (a launch would not be survivable)."""
    kw = dict(n_rows=8, n_cls=151, n_reg_cols=604, cls_agnostic=0, ld_logits=151, ld_reg=604, class_logits=4096, box_regression=8192,
              labels=12288, regression_targets=16384, losses=20480)
    kw.update(over)
    a = native.VetoBoxLossArgs(struct_size=ctypes.sizeof(native.VetoBoxLossArgs))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_box_loss_abi_rejects_bad_arguments_without_a_gpu():
    """Every check comes before the launch."""
    lib = native.load_library()
    for kw, needle in ((dict(struct_size=8), b"veto_box_loss_args_t size mismatch"),
                       (dict(n_cls=1), b"n_cls 1 outside 2..1024"),
                       (dict(n_cls=1025, n_reg_cols=4100, ld_logits=1025, ld_reg=4100), b"n_cls 1025 outside 2..1024"),
                       (dict(n_rows=-1), b"n_rows -1 outside 0..1048576"),
                       (dict(n_rows=1048577), b"n_rows 1048577 outside 0..1048576"),
                       (dict(n_reg_cols=600), b"n_reg_cols 600 must be a multiple of 4 and >= 604 (4 n_cls)"),
                       (dict(n_reg_cols=606, ld_reg=606), b"n_reg_cols 606 must be a multiple of 4 and >= 604"),
                       (dict(n_reg_cols=4, cls_agnostic=1), b"n_reg_cols 4 must be a multiple of 4 and >= 8 (cls_agnostic: columns 4..7)"),
                       (dict(ld_logits=150), b"ld_logits 150 is below the row width 151"),
                       (dict(ld_reg=603), b"ld_reg 603 is below the row width 604"),
                       (dict(losses=None), b"missing pointer: losses"),
                       (dict(class_logits=None), b"missing pointer: class_logits, box_regression, labels and regression_targets"),
                       (dict(box_regression=None), b"missing pointer"),
                       (dict(labels=None), b"missing pointer"),
                       (dict(regression_targets=None), b"missing pointer"),
                       (dict(d_class_logits=4096), b"d_class_logits and d_box_regression: both or neither"),
                       (dict(d_box_regression=4096), b"d_class_logits and d_box_regression: both or neither"),
                       (dict(regression_targets=16388), b"regression_targets must be 16-byte aligned"),
                       (dict(d_class_logits=4096, d_box_regression=8200), b"d_class_logits and d_box_regression must be 16-byte aligned"),
                       (dict(d_class_logits=4100, d_box_regression=8192), b"d_class_logits and d_box_regression must be 16-byte aligned"),
                       (dict(class_logits=4097), b"misaligned"),
                       (dict(labels=12292), b"misaligned")):
        a = _abi_args(**kw)
        assert lib.veto_box_loss(None, ctypes.byref(a), None, 0) == -1, kw            # VETO_ERR_INVALID
        assert needle in lib.veto_last_error(), (kw, lib.veto_last_error())
    assert lib.veto_box_loss(None, None, None, 0) == -1
    a = _abi_args(d_class_logits=4096, d_box_regression=8192)
    assert lib.veto_box_loss(None, ctypes.byref(a), None, 0) == -4 and b"workspace too small" in lib.veto_last_error()
    assert lib.veto_box_loss(None, ctypes.byref(a), ctypes.c_void_p(4100), 1 << 20) == -4 and b"256-byte aligned" in lib.veto_last_error()
    # the workspace: two doubles per row (and one spare pair), rounded up to 256 bytes
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(a)) == 256
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(_abi_args(n_rows=6144))) == 6144 * 16 + 256
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(_abi_args(n_rows=0))) == 256
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(_abi_args(n_cls=1))) == 0
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(_abi_args(struct_size=8))) == 0
    assert lib.veto_box_loss_workspace_bytes(None) == 0
    # agnostic with 8 columns and strides wider than the rows pass the shape checks
    assert lib.veto_box_loss_workspace_bytes(ctypes.byref(_abi_args(n_reg_cols=8, cls_agnostic=1, ld_logits=758, ld_reg=758))) == 256


# ---- the classes, the factory, the installer ---------------------------------------------------------------------------------

def _proposals(d, device="cpu"):
    out = []
    for lab, tgt in zip(d["labels"], d["regression_targets"]):
        p = BoxList(torch.zeros((len(lab), 4), device=device), (640, 480), "xyxy")
        p.add_field("labels", torch.from_numpy(lab).to(device))
        p.add_field("regression_targets", torch.from_numpy(tgt).to(device))
        out.append(p)
    return out


def test_classes_have_the_reference_interface():
    from veto_amd import boxloss as bl
    assert list(inspect.signature(bl.FastRCNNLossComputation.__init__).parameters) == ["self", "cls_agnostic_bbox_reg"]
    assert inspect.signature(bl.FastRCNNLossComputation.__init__).parameters["cls_agnostic_bbox_reg"].default is False
    assert list(inspect.signature(bl.FastRCNNLossComputation.__call__).parameters) == ["self", "class_logits", "box_regression", "proposals"]
    assert list(inspect.signature(bl.make_roi_box_loss_evaluator).parameters) == ["cfg"]
    # (the reference is not importable where the tests run: loss.py:21, :42 and :87 are restated above)
    sig = inspect.signature(bl.box_loss_call)
    assert list(sig.parameters) == ["class_logits", "box_regression", "labels", "regression_targets", "cls_agnostic_bbox_reg", "want"]
    assert sig.parameters["cls_agnostic_bbox_reg"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["want"].default == ("losses", "grads")
    assert not hasattr(bl.FastRCNNLossComputation, "assign_label_to_proposals")     # dead code in the reference: not carried over
    assert "FastRCNNSampling.assign_label_to_proposals" in bl.FastRCNNLossComputation.__doc__
    for flag in (False, True):
        cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(CLS_AGNOSTIC_BBOX_REG=flag))
        s = bl.make_roi_box_loss_evaluator(cfg)
        assert isinstance(s, bl.FastRCNNLossComputation) and s.cls_agnostic_bbox_reg is flag
    assert bl.FastRCNNLossComputation().cls_agnostic_bbox_reg is False


def test_loss_checks_its_arguments_before_touching_the_library(monkeypatch):
    from veto_amd import boxloss as bl

    def no_library():
        raise AssertionError("the library must not be loaded before the arguments are checked")
    monkeypatch.setattr(native, "load_library", no_library)
    d = bc.case_inputs("lanes65")
    logits, reg = [torch.from_numpy(x) for x in d["class_logits"]], [torch.from_numpy(x) for x in d["box_regression"]]
    props = _proposals(d)
    s = bl.FastRCNNLossComputation()
    with pytest.raises(ValueError, match=r"equally long, non-empty lists \(got 1 and 2\)"):
        s(logits, reg + reg, props)
    with pytest.raises(ValueError, match="equally long, non-empty lists"):
        s([], [], props)
    with pytest.raises(ValueError, match="at least one image"):
        s(logits, reg, [])
    with pytest.raises(ValueError, match=r"labels must be \[7\], got \(14,\)"):
        s(logits, reg, props + props)
    with pytest.raises(ValueError, match=r"box_regression must be \[7, 260\], got \(7, 65\)"):
        s(logits, logits, props)
    with pytest.raises(ValueError, match=r"box_regression must be \[7, 260\], got \(6, 260\)"):
        s(logits, [reg[0][:6]], props)
    with pytest.raises(ValueError, match=r"class_logits must be \[R, C\]"):
        s([logits[0][0]], reg, props)
    with pytest.raises(ValueError, match=r"1 classes: 2\.\.1024 are supported"):
        s([logits[0][:, :1]], reg, props)
    with pytest.raises(ValueError, match=r"1025 classes: 2\.\.1024 are supported"):
        s([torch.zeros((7, 1025))], [torch.zeros((7, 4100))], props)
    with pytest.raises(ValueError, match=r"box_regression must be \[7, >= 8\]"):
        bl.FastRCNNLossComputation(True)(logits, [reg[0][:, :4]], props)
    bad = _proposals(d)
    bad[0].add_field("regression_targets", torch.zeros((7, 5)))
    with pytest.raises(ValueError, match=r"regression_targets must be \[7, 4\]"):
        bl.box_loss_call(logits[0], reg[0], bad[0].get_field("labels"), bad[0].get_field("regression_targets"))
    with pytest.raises(ValueError, match="want: unknown or no outputs"):
        bl.box_loss_call(logits[0], reg[0], props[0].get_field("labels"), props[0].get_field("regression_targets"), want=("loss",))
    with pytest.raises(ValueError, match="want: unknown or no outputs"):
        bl.box_loss_call(logits[0], reg[0], props[0].get_field("labels"), props[0].get_field("regression_targets"), want=())
    with pytest.raises(RuntimeError, match="box loss runs on a HIP device only"):
        s(logits, reg, props)
    with pytest.raises(RuntimeError, match="box loss runs on a HIP device only"):
        s([x.requires_grad_() for x in logits], reg, props)


def test_installer_points_the_reference_factory_at_the_device_loss(monkeypatch):
    from veto_amd import boxloss, registry
    pkg = "pysgg.modeling.roi_heads.box_head"
    names = ["pysgg", "pysgg.modeling", "pysgg.modeling.roi_heads", pkg, pkg + ".loss", pkg + ".box_head", pkg + ".sampling", "pysgg.modeling.rpn",
             "pysgg.modeling.rpn.loss"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
    loss, head, sampling, rpn_loss = mods[pkg + ".loss"], mods[pkg + ".box_head"], mods[pkg + ".sampling"], mods["pysgg.modeling.rpn.loss"]
    loss.make_roi_box_loss_evaluator = head.make_roi_box_loss_evaluator = original = object()
    sampling.make_roi_box_samp_processor = head.make_roi_box_samp_processor = samp = object()
    rpn_loss.make_rpn_loss_evaluator = rpn = object()
    patched = registry.install_box_loss_ops()
    assert patched == [(pkg + ".loss", "make_roi_box_loss_evaluator"), (pkg + ".box_head", "make_roi_box_loss_evaluator")]
    assert loss.make_roi_box_loss_evaluator is head.make_roi_box_loss_evaluator is boxloss.make_roi_box_loss_evaluator
    assert loss.make_roi_box_loss_evaluator is not original
    assert sampling.make_roi_box_samp_processor is head.make_roi_box_samp_processor is samp   # the other installers' targets stay
    assert rpn_loss.make_rpn_loss_evaluator is rpn
    # box_head.py not loaded: only the factory's own module is patched
    monkeypatch.delitem(sys.modules, pkg + ".box_head")
    loss.make_roi_box_loss_evaluator = original
    assert registry.install_box_loss_ops() == [(pkg + ".loss", "make_roi_box_loss_evaluator")]
    assert loss.make_roi_box_loss_evaluator is boxloss.make_roi_box_loss_evaluator
