"""The box head's loss on the MI355X: veto_box_loss (veto_amd.boxloss) against the float64 oracle boxloss_cases.box_loss_fp64 on
every case of the fixtures (tests/golden/boxloss), at the edges of the launch shape, on strided inputs and at the real size; the
NaN cases; autograd; the whole sampled path behind FastRCNNSampling.subsample; the launches and copies of a call; the limits.
Every measured figure is printed before it is asserted (pytest -s); the parity figures also go to profiles/boxloss_parity.txt."""
import contextlib
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxloss_cases as bc  # noqa: E402
from test_boxsample_host import box_lists  # noqa: E402

from veto_amd import boxloss as bl  # noqa: E402
from veto_amd import boxsampling as bs  # noqa: E402
from veto_amd import native, synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "boxloss_parity.txt")
EPS = 2.0 ** -23    # one fp32 rounding of the result


def _bounds():
    """(losses, d_class_logits, d_box_regression): each 4 x the largest matching error the reference's own fp32 run has against
    its float64 run, over all fixtures (the maximum, so that one lucky fixture cannot set it; the margin covers a different but
    equally valid fp32 evaluation order), and at least 2^-23."""
    z = [bc.load_case(name)[0] for name in bc.ALL]
    return tuple(max(4 * max(float(f[k]) for f in z), EPS) for k in ("ref_fp32_err_loss", "ref_fp32_err_dlogits", "ref_fp32_err_dbox"))


@contextlib.contextmanager
def _nan_filled_outputs():
    """Every floating tensor the call allocates with torch.empty starts as NaN: an element the call does not write shows."""
    real = torch.empty

    def empty(*size, **kw):
        t = real(*size, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def _call(logits, reg, labels, targets, agnostic=False, want=("losses", "grads")):
    """box_loss_call on numpy or device inputs, the outputs pre-filled with NaN; every output as numpy."""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a for a in (logits, reg, labels, targets)]
    with _nan_filled_outputs():
        out = bl.box_loss_call(*dev, cls_agnostic_bbox_reg=agnostic, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _measure(out, o):
    """(loss, d_class_logits, d_box_regression) errors of a call against the oracle's dict, in the metrics of boxloss_cases."""
    assert out["losses"].dtype == out["d_class_logits"].dtype == out["d_box_regression"].dtype == np.float32
    assert out["d_class_logits"].shape == o["d_class_logits"].shape and out["d_box_regression"].shape == o["d_box_regression"].shape
    assert not np.isnan(out["d_class_logits"]).any() and not np.isnan(out["d_box_regression"]).any()      # every element was written
    return (bc.loss_err(out["losses"], o["losses"]), bc.dlogits_err(out["d_class_logits"], o["d_class_logits"], o["p"], o["onehot"]),
            bc.dbox_err(out["d_box_regression"], o["d_box_regression"]))


def _assert_within(errs, what):
    bounds = _bounds()
    print("%s: losses rel err %.3g (bound %.3g)  d_class_logits err %.3g of (p + onehot) / R (bound %.3g)  d_box_regression rel err %.3g (bound %.3g)"
          % (what, errs[0], bounds[0], errs[1], bounds[1], errs[2], bounds[2]))
    assert errs[0] <= bounds[0] and errs[1] <= bounds[1] and errs[2] <= bounds[2], (what, errs, bounds)


# ---- parity with the float64 oracle on every case ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def parity_report():
    """Collects one line per case; profiles/boxloss_parity.txt is written once, after the last case, and only by a run that
    covered every case (a run of some cases leaves the committed record alone)."""
    lines = {}
    yield lines
    if set(lines) != set(bc.ALL):
        return
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        f.write("Box-head loss on the device against the float64 oracle on the same fp32 inputs; bounds = 4 x the largest ref_fp32_err_* "
                "of the fixtures (at least 2^-23): losses %.3g relative, d_class_logits %.3g of (p + onehot) / R (+ 2^-126), "
                "d_box_regression %.3g relative at the oracle's elements (exactly 0 elsewhere); each figure is the worst element\n" % _bounds())
        for k in bc.ALL:
            f.write(lines[k] + "\n")


@pytest.mark.parametrize("name", bc.ALL)
def test_losses_and_gradients_match_the_fp64_oracle(name, parity_report):
    z, d = bc.load_case(name)
    logits, reg, labels, targets = bc.concatenated(d)
    o = bc.box_loss_fp64(logits, reg, labels, targets, agnostic=d["agnostic"])
    assert bc.loss_err(o["losses"], z["losses_fp64"]) <= 1e-12                   # the oracle is the reference's float64 run
    out = _call(logits, reg, labels, targets, d["agnostic"])
    again = _call(logits, reg, labels, targets, d["agnostic"])
    errs = _measure(out, o)
    line = ("%-9s R %4d C %4d P %3d  classification_loss %.9g  box_loss %.9g  losses rel err %.3g  d_class_logits err %.3g  d_box_regression rel err %.3g"
            % (name, len(labels), logits.shape[1], int((labels > 0).sum()), out["losses"][0], out["losses"][1], errs[0], errs[1], errs[2]))
    print("PARITY " + line)
    parity_report[name] = line
    _assert_within(errs, name)
    for k in ("losses", "d_class_logits", "d_box_regression"):
        assert out[k].tobytes() == again[k].tobytes(), k                           # two calls give the same bits
    only = _call(logits, reg, labels, targets, d["agnostic"], want=("losses",))
    assert sorted(only) == ["losses"] and only["losses"].tobytes() == out["losses"].tobytes()
    if name == "no_pos":
        assert out["losses"][1] == 0 and not out["d_box_regression"].any()
    if name == "sharp":
        c = bc.SEEDED["sharp"]
        gone = int(np.nonzero(np.isneginf(logits[c["inf_row"]]))[0][0])
        assert out["d_class_logits"][c["inf_row"], gone] == 0 and np.isfinite(out["losses"]).all()
    if name == "kink":                                                             # its answers are exact in fp32
        np.testing.assert_array_equal(out["d_box_regression"], o["d_box_regression"].astype(np.float32))
        np.testing.assert_array_equal(out["d_class_logits"], o["d_class_logits"].astype(np.float32))
        assert out["losses"][1] == np.float32(o["losses"][1]) == np.float32(0.517578125)
        assert np.array_equal(o["d_box_regression"].astype(np.float32).astype(np.float64), o["d_box_regression"])
        got = set((out["d_box_regression"][labels > 0][:, 4:] * 16).ravel().tolist())
        assert got == {0.0, 1.0, -1.0, float(np.float32(1 - 2.0 ** -23)), -float(np.float32(1 - 2.0 ** -23)), 0.5, -0.5, 0.25}


# ---- the edges of the launch shape ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3, 4, 5, 255, 256, 257, 1025])
def test_rows_at_the_workgroup_and_fold_edges(R):
    """C = 151; four rows per workgroup (R = 3, 4, 5) and the final fold's per-thread ranges (255, 256, 257: one row per thread
    with and without an idle thread, then two; 1025: five per thread, the last threads empty)."""
    logits, reg, labels, targets = bc.seeded_batch(8000 + R, R, 151, pos=0.4)
    if R >= 3:
        labels[[0, R - 1]] = (150, 7)
    o = bc.box_loss_fp64(logits, reg, labels, targets)
    out = _call(logits, reg, labels, targets)
    _assert_within(_measure(out, o), "R = %d" % R)


def test_the_real_size_and_strided_inputs():
    """R = 6144 at C = 151 (12 images x 512 rows) once; then class_logits and box_regression as column slices of one [R, 5C + 3]
    tensor, read in place: the same bits as from contiguous copies."""
    R, C = 6144, 151
    logits, reg, labels, targets = bc.seeded_batch(8100, R, C)
    o = bc.box_loss_fp64(logits, reg, labels, targets)
    out = _call(logits, reg, labels, targets)
    _assert_within(_measure(out, o), "R = 6144")
    R = 257
    logits, reg, labels, targets = bc.seeded_batch(8101, R, C)
    both = torch.from_numpy(np.concatenate([logits, reg, np.full((R, 3), np.nan, np.float32)], 1)).to(DEV)
    assert both.shape == (R, 5 * C + 3)
    z_view, x_view = both[:, :C], both[:, C:5 * C]
    assert not z_view.is_contiguous() and not x_view.is_contiguous() and x_view.data_ptr() % 16 != 0
    strided = _call(z_view, x_view, labels, targets)
    plain = _call(logits, reg, labels, targets)
    for k in ("losses", "d_class_logits", "d_box_regression"):
        assert strided[k].tobytes() == plain[k].tobytes(), k
    _assert_within(_measure(strided, bc.box_loss_fp64(logits, reg, labels, targets)), "strided, R = 257")
    # in place: the call was handed the views' own addresses and strides
    a = _captured_args(lambda: bl.box_loss_call(z_view, x_view, torch.from_numpy(labels).to(DEV), torch.from_numpy(targets).to(DEV)))
    assert (a["class_logits"], a["box_regression"], a["ld_logits"], a["ld_reg"]) == (z_view.data_ptr(), x_view.data_ptr(), 5 * C + 3, 5 * C + 3)


def _captured_args(fn):
    """The fields of the veto_box_loss_args_t a call passes."""
    seen = {}
    real = native.Launch.run

    def run(self, name, *tail, **kw):
        a = ctypes.cast(tail[0], ctypes.POINTER(native.VetoBoxLossArgs)).contents
        seen.update({f: getattr(a, f) for f, _ in native.VetoBoxLossArgs._fields_})
        return real(self, name, *tail, **kw)
    native.Launch.run = run
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        native.Launch.run = real
    return seen


# ---- the NaN cases -----------------------------------------------------------------------------------------------------------

def test_no_rows_give_nan():
    out = _call(np.zeros((0, 151), np.float32), np.zeros((0, 604), np.float32), np.zeros(0, np.int64), np.zeros((0, 4), np.float32))
    assert math.isnan(out["losses"][0]) and math.isnan(out["losses"][1])
    assert out["d_class_logits"].shape == (0, 151) and out["d_box_regression"].shape == (0, 604)
    out = _call(np.zeros((0, 151), np.float32), np.zeros((0, 604), np.float32), np.zeros(0, np.int64), np.zeros((0, 4), np.float32), want=("losses",))
    assert math.isnan(out["losses"][0]) and math.isnan(out["losses"][1])


@pytest.mark.parametrize("bad", [151, -1, -100, 2 ** 40])
def test_a_label_outside_the_classes_poisons_its_row_and_the_losses_only(bad):
    """Row 5 of 11 carries the label: both losses NaN, its two gradient rows NaN, every other row as without it."""
    logits, reg, labels, targets = bc.seeded_batch(8200, 11, 151, pos=0.5)
    good = _call(logits, reg, labels, targets)
    labels = labels.copy()
    labels[5] = bad
    dev = [torch.from_numpy(a).to(DEV) for a in (logits, reg, labels, targets)]
    out = bl.box_loss_call(*dev)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.isnan(out["losses"]).all()
    assert np.isnan(out["d_class_logits"][5]).all() and np.isnan(out["d_box_regression"][5]).all()
    others = np.arange(11) != 5
    assert out["d_class_logits"][others].tobytes() == good["d_class_logits"][others].tobytes()
    assert out["d_box_regression"][others].tobytes() == good["d_box_regression"][others].tobytes()


# ---- autograd ----------------------------------------------------------------------------------------------------------------

def _proposals(d):
    out = []
    for lab, tgt in zip(d["labels"], d["regression_targets"]):
        p = BoxList(torch.zeros((len(lab), 4), device=DEV), (640, 480), "xyxy")
        p.add_field("labels", torch.from_numpy(lab).to(DEV))
        p.add_field("regression_targets", torch.from_numpy(tgt).to(DEV))
        out.append(p)
    return out


@pytest.mark.parametrize("name", ["vg", "ragged"])
def test_backward_puts_the_scaled_gradients_into_the_leaves(name):
    """(2 classification_loss + 3 box_loss).backward() through FastRCNNLossComputation on per-image lists: the leaves' .grad are
    the call's gradients times 2 and 3, bit for bit; with nothing requiring grad no gradient is asked for and the losses are the
    same bits."""
    _, d = bc.load_case(name)
    loss = bl.FastRCNNLossComputation()
    logits = [torch.from_numpy(x).to(DEV).requires_grad_() for x in d["class_logits"]]
    reg = [torch.from_numpy(x).to(DEV).requires_grad_() for x in d["box_regression"]]
    lc, lb = loss(logits, reg, _proposals(d))
    assert lc.dim() == 0 and lb.dim() == 0 and lc.requires_grad and lb.requires_grad and lc.device.type == "cuda"
    (2 * lc + 3 * lb).backward()
    ref = bl.box_loss_call(*[torch.from_numpy(a).to(DEV) for a in bc.concatenated(d)])
    assert torch.equal(torch.stack([lc.detach(), lb.detach()]), ref["losses"])
    n = [len(x) for x in d["labels"]]
    for leaf, want in zip(logits, ref["d_class_logits"].split(n)):
        assert leaf.grad.shape == want.shape and torch.equal(leaf.grad, want * 2)
    for leaf, want in zip(reg, ref["d_box_regression"].split(n)):
        assert leaf.grad.shape == want.shape and torch.equal(leaf.grad, want * 3)
    assert ref["d_class_logits"].any() and ref["d_box_regression"].any()
    wants = []
    real = bl.box_loss_call

    def spy(*a, **kw):
        wants.append(tuple(kw["want"]))
        return real(*a, **kw)
    bl.box_loss_call = spy
    try:
        plain = loss([x.detach() for x in logits], [x.detach() for x in reg], _proposals(d))
        with torch.no_grad():
            quiet = loss(logits, reg, _proposals(d))
        one = loss([torch.cat(logits).detach().requires_grad_()], [torch.cat(reg).detach()], _proposals(d))   # the shape box_head.py passes
    finally:
        bl.box_loss_call = real
    assert wants == [("losses",), ("losses",), ("losses", "grads")]
    assert not plain[0].requires_grad and torch.equal(torch.stack(plain), ref["losses"]) and torch.equal(torch.stack(quiet), ref["losses"])
    assert one[0].requires_grad and torch.equal(torch.stack([t.detach() for t in one]), ref["losses"])


# ---- the whole sampled path ------------------------------------------------------------------------------------------------------

def test_sampled_proposals_through_a_predictor_pair_and_back():
    """2 images x 300 proposals x 20 GT boxes, budget 64: FastRCNNSampling.subsample on the device, a float64 Linear pair on
    features of the sampled rows (C = 151, 4C box columns), the device loss, backward().  The weights' gradients against float64
    torch autograd through the reference's formulas on the same sampled rows and the same fp32-rounded predictor outputs: the class
    predictor's under the d_class_logits bound, the box predictor's under the d_box_regression bound, each scaled by the
    features: |dW[c, f] - dW64[c, f]| <= sum_r bound_r[c] |feat[r, f]|."""
    C, F = 151, 24
    images = []
    for i in range(2):
        d = synth.synthetic_relsample_image(8300 + i, 20, 300, 2)
        images.append({"prp_boxes": d["prp_boxes"], "tgt_boxes": d["tgt_boxes"], "tgt_labels": d["tgt_labels"], "image_size": d["image_size"],
                       "attributes": synth.integers(8300 + i, "boxloss.attr", (20, 2), 0, 9)})
        assert d["tgt_labels"].max() < C and d["tgt_labels"].min() >= 1
    props, targets = box_lists(images, DEV)
    sampler = bs.FastRCNNSampling(bs.Matcher(0.5, 0.3), bs.BalancedPositiveNegativeSampler(64, 0.25), bs.BoxCoder((10., 10., 5., 5.)))
    sampled = sampler.subsample(props, targets, seed=77)
    R = sum(len(p) for p in sampled)
    labels = torch.cat([p.get_field("labels") for p in sampled])
    assert R == 128 and 0 < int((labels > 0).sum()) < R
    gen = torch.Generator().manual_seed(8300)
    feat = torch.randn((R, F), dtype=torch.float64, generator=gen).to(DEV)

    def predictors():
        g = torch.Generator().manual_seed(8301)
        cls, box = torch.nn.Linear(F, C).double(), torch.nn.Linear(F, 4 * C).double()
        with torch.no_grad():
            for lin in (cls, box):
                lin.weight.copy_(torch.randn(lin.weight.shape, dtype=torch.float64, generator=g) * 0.3)
                lin.bias.copy_(torch.randn(lin.bias.shape, dtype=torch.float64, generator=g) * 0.3)
        return cls.to(DEV), box.to(DEV)

    def rounded(t):   # the value the device reads (fp32), the gradient of the float64 tensor
        return t + (t.float().double() - t).detach()

    cls, box = predictors()
    lc, lb = bl.FastRCNNLossComputation()([rounded(cls(feat))], [rounded(box(feat))], sampled)
    assert lc.dtype == torch.float32 and lc.requires_grad
    (lc.double() + lb.double()).backward()

    cls64, box64 = predictors()
    z, x = rounded(cls64(feat)), rounded(box64(feat))
    t = torch.cat([p.get_field("regression_targets") for p in sampled]).double()
    pos = torch.nonzero(labels > 0).squeeze(1)                                # loss.py:64-82 in float64
    ce = torch.nn.functional.cross_entropy(z, labels)
    n = (x[pos[:, None], 4 * labels[pos][:, None] + torch.arange(4, device=DEV)] - t[pos]).abs()
    sl1 = torch.where(n < 1, 0.5 * n ** 2, n - 0.5).sum() / labels.numel()
    (ce + sl1).backward()
    b_loss, b_logits, b_box = _bounds()
    assert abs(float(lc.detach()) - float(ce.detach())) <= b_loss * abs(float(ce.detach())) and abs(float(lb.detach()) - float(sl1.detach())) <= b_loss * abs(float(sl1.detach()))
    p = torch.softmax(z.detach(), 1)
    onehot = torch.nn.functional.one_hot(labels, C).double()
    mag = b_logits * (p + onehot) / R + bc.TINY                               # per element of d_class_logits
    af = feat.abs()
    err_w, allow_w = (cls.weight.grad - cls64.weight.grad).abs(), mag.t() @ af
    err_b, allow_b = (cls.bias.grad - cls64.bias.grad).abs(), mag.sum(0)
    print("class predictor: weight grad err / allowed %.3g, bias %.3g" % (float((err_w / allow_w).max()), float((err_b / allow_b).max())))
    assert (err_w <= allow_w).all() and (err_b <= allow_b).all()
    # the box predictor: d_box_regression's own float64 values are the gradient of sl1 w.r.t. x
    x2 = x.detach().requires_grad_()
    n2 = (x2[pos[:, None], 4 * labels[pos][:, None] + torch.arange(4, device=DEV)] - t[pos]).abs()
    (torch.where(n2 < 1, 0.5 * n2 ** 2, n2 - 0.5).sum() / labels.numel()).backward()
    mag = b_box * x2.grad.abs()
    err_w, allow_w = (box.weight.grad - box64.weight.grad).abs(), mag.t() @ af
    err_b, allow_b = (box.bias.grad - box64.bias.grad).abs(), mag.sum(0)
    hit = allow_w > 0
    print("box predictor: weight grad err / allowed %.3g over %d elements" % (float((err_w[hit] / allow_w[hit]).max()), int(hit.sum())))
    assert (err_w <= allow_w).all() and (err_b <= allow_b).all() and hit.any() and box64.weight.grad.abs().sum() > 0


# ---- launches and copies of a call ---------------------------------------------------------------------------------------------

def _copies(events):
    """Copies in a profile: the runtime's memcpy calls (hipMemcpy*, of any direction: a read-back through pinned memory, such as
    nonzero's count, is executed by a blit kernel and carries no direction in its name) or, if more, the device activities named as
    device->host copies."""
    runtime = sum(1 for e in events if e.name.startswith(("hipMemcpy", "cudaMemcpy")))
    named = sum(1 for e in events if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    return max(runtime, named)


def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and "box_loss_" in e.name]
    return len(kernels), _copies(ev)


def test_the_copy_count_sees_a_read_back():
    """The positive control of the zero below: a nonzero (its count is read back), an .item() and a .cpu() each count."""
    x = torch.zeros(1000, device=DEV)
    x[3] = 1
    torch.nonzero(x)
    for what, fn in (("nonzero", lambda: torch.nonzero(x)), ("item", lambda: x.sum().item()), ("cpu", lambda: x.cpu())):
        launches, copies = _profile(fn)
        print("%s: %d copies" % (what, copies))
        assert copies >= 1 and launches == 0, what
    assert _profile(lambda: x + 1) == (0, 0)


def test_launches_and_copies_of_a_call():
    """Two launches with the gradients and two without, for 1 and for 3 images and for C = 2 and C = 1024; no memcpy call of any
    direction (test_the_copy_count_sees_a_read_back)."""
    got = {}
    for name in ("vg", "ragged", "two_cls", "wide"):
        _, d = bc.load_case(name)
        if name == "vg":
            d = {k: v[:1] if isinstance(v, list) else v for k, v in d.items()}
        loss = bl.FastRCNNLossComputation()
        props = _proposals(d)
        logits = [torch.from_numpy(x).to(DEV) for x in d["class_logits"]]
        reg = [torch.from_numpy(x).to(DEV) for x in d["box_regression"]]
        leaves = [x.clone().requires_grad_() for x in logits]
        loss(leaves, reg, props)                                                # warm-up: the code objects, the workspace
        loss(logits, reg, props)
        full = _profile(lambda: loss(leaves, reg, props))
        plain = _profile(lambda: loss(logits, reg, props))
        print("%s, %d images, C = %d: %d launches and %d memcpy calls with the gradients, %d and %d without"
              % ((name, len(props), logits[0].shape[1]) + full + plain))
        got[(len(props), logits[0].shape[1])] = (full, plain)
    assert set(got) == {(1, 151), (3, 151), (1, 2), (1, 1024)}
    assert all(v == ((2, 0), (2, 0)) for v in got.values()), got


# ---- limits ------------------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_truncations(monkeypatch):
    calls = []
    real = native.Launch.run

    def run(self, name, *tail, **kw):
        calls.append(name)
        return real(self, name, *tail, **kw)
    monkeypatch.setattr(native.Launch, "run", run)
    f32 = dict(dtype=torch.float32, device=DEV)
    labels, targets = torch.zeros(7, dtype=torch.int64, device=DEV), torch.zeros((7, 4), **f32)
    with pytest.raises(ValueError, match=r"1 classes: 2\.\.1024 are supported"):
        bl.box_loss_call(torch.zeros((7, 1), **f32), torch.zeros((7, 4), **f32), labels, targets)
    with pytest.raises(ValueError, match=r"1025 classes: 2\.\.1024 are supported"):
        bl.box_loss_call(torch.zeros((7, 1025), **f32), torch.zeros((7, 4100), **f32), labels, targets)
    with pytest.raises(ValueError, match="1048577 rows, the limit is 1048576"):
        bl.box_loss_call(torch.zeros((1, 2), **f32).expand(1048577, 2), torch.zeros((1, 8), **f32).expand(1048577, 8),
                         labels[:1].expand(1048577), targets[:1].expand(1048577, 4))
    with pytest.raises(ValueError, match=r"box_regression must be \[7, 604\], got \(7, 600\)"):
        bl.box_loss_call(torch.zeros((7, 151), **f32), torch.zeros((7, 600), **f32), labels, targets)
    with pytest.raises(ValueError, match=r"box_regression must be \[7, >= 8\] with a multiple of 4 columns, got \(7, 4\)"):
        bl.box_loss_call(torch.zeros((7, 151), **f32), torch.zeros((7, 4), **f32), labels, targets, cls_agnostic_bbox_reg=True)
    with pytest.raises(ValueError, match=r"with a multiple of 4 columns, got \(7, 10\)"):
        bl.box_loss_call(torch.zeros((7, 151), **f32), torch.zeros((7, 10), **f32), labels, targets, cls_agnostic_bbox_reg=True)
    with pytest.raises(ValueError, match=r"labels must be \[7\]"):
        bl.box_loss_call(torch.zeros((7, 151), **f32), torch.zeros((7, 604), **f32), labels[:6], targets)
    with pytest.raises(ValueError, match=r"regression_targets must be \[7, 4\]"):
        bl.box_loss_call(torch.zeros((7, 151), **f32), torch.zeros((7, 604), **f32), labels, targets[:, :3])
    assert calls == []                                                          # refused before Launch.run was reached
    # what the Python side cannot produce, at the ABI: refused with a message, nothing launched
    lib = native.load_library()
    z, x = torch.zeros((7, 151), **f32), torch.zeros((7, 604), **f32)
    losses, gz, gx = torch.zeros(2, **f32), torch.zeros((7, 151), **f32), torch.zeros((7, 604), **f32)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)

    def abi(**over):
        kw = dict(n_rows=7, n_cls=151, n_reg_cols=604, cls_agnostic=0, ld_logits=151, ld_reg=604, class_logits=z.data_ptr(),
                  box_regression=x.data_ptr(), labels=labels.data_ptr(), regression_targets=targets.data_ptr(), losses=losses.data_ptr(),
                  d_class_logits=gz.data_ptr(), d_box_regression=gx.data_ptr())
        kw.update(over)
        a = native.VetoBoxLossArgs(struct_size=ctypes.sizeof(native.VetoBoxLossArgs))
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.veto_box_loss(None, ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()), ws.numel())
        return rc, lib.veto_last_error()
    for over, needle in ((dict(struct_size=8), b"size mismatch"), (dict(ld_logits=150), b"ld_logits 150 is below the row width 151"),
                         (dict(ld_reg=600), b"ld_reg 600 is below the row width 604"), (dict(d_box_regression=None), b"both or neither"),
                         (dict(regression_targets=targets.data_ptr() + 4), b"regression_targets must be 16-byte aligned"),
                         (dict(d_box_regression=gx.data_ptr() + 8), b"must be 16-byte aligned"), (dict(labels=None), b"missing pointer"),
                         (dict(n_cls=1025), b"n_cls 1025 outside 2..1024"), (dict(n_rows=1048577), b"n_rows 1048577 outside 0..1048576")):
        rc, msg = abi(**over)
        assert rc == -1 and needle in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert not gz.any() and not gx.any() and not losses.any()                   # nothing ran
    # the limits themselves are fine: C = 2 and C = 1024 are fixtures; the largest row count, class-agnostic so that it stays small
    n = 1 << 20
    rng = np.random.RandomState(8400)
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    reg = (rng.standard_normal((n, 8)) * 0.7).astype(np.float32)
    tg = (rng.standard_normal((n, 4)) * 0.7).astype(np.float32)
    lab = (rng.random_sample(n) < 0.25).astype(np.int64)
    o = bc.box_loss_fp64(logits, reg, lab, tg, agnostic=True)
    out = _call(logits, reg, lab, tg, agnostic=True)
    _assert_within(_measure(out, o), "R = 1048576, C = 2, class-agnostic")
    assert calls == ["veto_box_loss"]
