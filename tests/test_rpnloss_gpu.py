"""The RPN loss on the MI355X: veto_rpn_loss (veto_amd.rpnloss) against the reference's fixtures (tests/golden/rpnloss), the numpy
restatement rpnloss_cases.np_rpn_match at the tile and LDS edges, the sampler against test_boxsample_host.np_box_subsample and
veto_box_subsample, the losses and gradients at the device's own sampled anchors against the float64 oracle
rpnloss_cases.rpn_loss_fp64, autograd, the launches and copies of a call, and the limits.  Every measured figure is printed
before it is asserted (pytest -s); the loss parity figures also go to profiles/rpnloss_parity.txt."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rpnloss_cases as rc  # noqa: E402
from test_boxsample_host import np_box_subsample, np_quota  # noqa: E402
from test_relsample_gtbox_gpu import binomial_bound  # noqa: E402

from veto_amd import boxsampling as bs  # noqa: E402
from veto_amd import native, synth  # noqa: E402
from veto_amd import rpnloss as rl  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rpnloss_parity.txt")


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _call(c, d, want, seed=1, head=True, **over):
    """rpn_loss_call on a case's inputs; every output as numpy (lists per level for the gradients)."""
    kw = dict(high_threshold=c["high"], low_threshold=c["low"], allow_low_quality_matches=c["lowq"], straddle_thresh=c["straddle"],
              weights=rc.WEIGHTS, batch_size_per_image=c["batch"], positive_fraction=c["fraction"], seed=seed, want=want,
              level_shapes=d["level_shapes"])
    if head:
        kw.update(objectness=_dev(d["objectness"]), box_regression=_dev(d["box_regression"]))
    kw.update(over)
    out = rl.rpn_loss_call(_dev(d["anchors"]), d["image_sizes"], _dev(d["tgt_boxes"]), **kw)
    torch.cuda.synchronize()
    return {k: [t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy() for k, v in out.items()}


def _sampled_lists(out):
    return [out["sampled_inds"][i, :int(out["counts"][i].sum())] for i in range(len(out["counts"]))]


# ---- matching against the goldens ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.ALL)
def test_matching_matches_the_reference_fixture(name):
    z, c, d = rc.load_case(name)
    out = _call(c, d, ("labels", "matched_idxs", "regression_targets"), head=False)
    assert out["labels"].dtype == np.float32 and out["matched_idxs"].dtype == np.int64 and out["regression_targets"].dtype == np.float32
    err = 0.0
    for i in range(len(d["tgt_boxes"])):
        np.testing.assert_array_equal(out["matched_idxs"][i], z["matched_%d" % i], err_msg="matched_idxs of image %d" % i)
        np.testing.assert_array_equal(out["labels"][i], z["labels_%d" % i].astype(np.float32), err_msg="labels of image %d" % i)
        err = max(err, float(np.abs(out["regression_targets"][i].astype(np.float64) - z["targets_%d" % i]).max()))
    tol = 4 * float(z["ref_fp32_err_targets"])
    print("%s: regression_targets differ from the reference's by %.3g, allowed %.3g (4x its own fp32 error)" % (name, err, tol))
    assert err <= tol


# ---- the tile and LDS edges ------------------------------------------------------------------------------------------------

def _assert_matches_numpy(c, d, out):
    """labels and matched_idxs bit for bit; dx, dy of the targets bit for bit (the same fp32 operations), dw, dh within 4 ulp of
    max(|t|, 1) (the device's logf and the host libm's each round within an ulp or two of the true logarithm)."""
    anchors = np.concatenate(d["anchors"])
    worst = 0.0
    for i, (t, size) in enumerate(zip(d["tgt_boxes"], d["image_sizes"])):
        matched, labels, targets, _ = rc.np_rpn_match(anchors, t, size, c["high"], c["low"], c["lowq"], c["straddle"])
        np.testing.assert_array_equal(out["matched_idxs"][i], matched, err_msg="matched_idxs of image %d" % i)
        np.testing.assert_array_equal(out["labels"][i], labels, err_msg="labels of image %d" % i)
        got = out["regression_targets"][i]
        np.testing.assert_array_equal(got[:, :2], targets[:, :2], err_msg="dx, dy of image %d" % i)
        ulps = np.abs(got[:, 2:].astype(np.float64) - targets[:, 2:]) / (2.0 ** -23 * np.maximum(np.abs(targets[:, 2:]), 1.0))
        worst = max(worst, float(ulps.max()))
    return worst


EDGE_IMAGES = ((800, 600), (640, 480), (700, 500))
EDGE = dict(high=0.7, low=0.3, lowq=True, straddle=0, batch=64, fraction=0.5)


@pytest.mark.parametrize("n_gt", [1, 255, 256])
@pytest.mark.parametrize("n_anchor", [255, 256, 257, 513])
def test_matching_at_the_tile_and_lds_edges_one_level(n_anchor, n_gt):
    """One level of A = 1 (one thread short of a tile, a full tile, one over, two tiles and one) against 1, 255 or 256 GT boxes, three
    images of different sizes: every output against the numpy restatement."""
    images = [synth.synthetic_relsample_image(7000 + 10 * n_gt + i, n_gt, n_anchor, min(2, n_gt * (n_gt - 1))) for i in range(3)]
    assert len(images[0]["prp_boxes"]) == n_anchor
    d = dict(anchors=[images[0]["prp_boxes"]], tgt_boxes=[im["tgt_boxes"] for im in images], image_sizes=list(EDGE_IMAGES),
             level_shapes=[(1, 1, n_anchor)])
    out = _call(EDGE, d, ("labels", "matched_idxs", "regression_targets"), head=False)
    worst = _assert_matches_numpy(EDGE, d, out)
    print("%d anchors, %d GT boxes: dw, dh differ from the fp32 numpy restatement by %.2f ulp" % (n_anchor, n_gt, worst))
    assert worst <= 4
    assert any((out["labels"][i] == -1).any() for i in range(3)) and any((out["labels"][i] == 1).any() for i in range(3))


def test_matching_over_five_levels_of_three_anchors():
    """Five levels, A = 3, 546 anchors: the level boundaries fall inside tiles; three images of different sizes."""
    grids = ((10, 13), (5, 7), (3, 4), (2, 2), (1, 1))
    shapes = [(3, h, w) for h, w in grids]
    images = [(104, 80), (96, 72), (100, 64)]
    d = synth.synthetic_rpn_training_batch(7100, images, shapes, (2, 9, 4), min_side=12.0)
    d.update(anchors=synth.anchor_grid((16, 32, 64, 128, 256), (8, 16, 32, 64, 128), rc.RATIOS, grids), image_sizes=images, level_shapes=shapes)
    assert sum(len(a) for a in d["anchors"]) == 546
    out = _call(EDGE, d, ("labels", "matched_idxs", "regression_targets"), head=False)
    worst = _assert_matches_numpy(EDGE, d, out)
    print("five levels: dw, dh differ from the fp32 numpy restatement by %.2f ulp" % worst)
    assert worst <= 4 and any((out["labels"][i] == 1).any() for i in range(3))


# ---- the sampler -----------------------------------------------------------------------------------------------------------

def _inputs_for_labels(label_lists):
    """Anchors and per-image GT boxes whose labels (allow_low_quality_matches False, every anchor visible) are the given equally
    long vectors over {1, 0, -1}, for at most 4 images: the anchor of code k = sum 3^i (label_i + 1) is the 20 x 20 box at x = 100 k;
    image i holds an equal GT box (IoU 1) for every code it labels 1, the box's upper half (IoU 0.5, between the thresholds) for
    every code it labels -1, and one GT box far from every anchor."""
    n_img = len(label_lists)
    assert n_img <= 4 or all(np.array_equal(label_lists[0], x) for x in label_lists)
    distinct = label_lists if n_img <= 4 else label_lists[:1]
    code = sum((np.asarray(x, np.int64) + 1) * 3 ** i for i, x in enumerate(distinct))
    x0 = (100 * code).astype(np.float32)
    anchors = np.stack([x0, np.zeros_like(x0), x0 + 19, np.full_like(x0, 19)], 1)
    tgt = []
    for i in range(n_img):
        digit = i if n_img <= 4 else 0
        boxes = [[0, 1000, 19, 1019]]
        for k in range(3 ** len(distinct)):
            lab = (k // 3 ** digit) % 3 - 1
            if lab == 1:
                boxes.append([100 * k, 0, 100 * k + 19, 19])
            elif lab == -1:
                boxes.append([100 * k, 0, 100 * k + 19, 9])
        tgt.append(np.asarray(boxes, np.float32))
    return anchors, tgt


def _sample(label_lists, batch, fraction, seed):
    """The sampler of veto_rpn_loss on given label vectors: (rows per image, counts [n_img, 2])."""
    label_lists = [np.asarray(x, np.int64) for x in label_lists]
    anchors, tgt = _inputs_for_labels(label_lists)
    c = dict(high=0.7, low=0.3, lowq=False, straddle=-1, batch=batch, fraction=fraction)
    d = dict(anchors=[anchors], tgt_boxes=tgt, image_sizes=[(64, 64)] * len(tgt), level_shapes=[(1, 1, len(anchors))])
    out = _call(c, d, ("labels", "sampled_inds", "counts"), seed=seed, head=False)
    for i, want in enumerate(label_lists):
        np.testing.assert_array_equal(out["labels"][i], want.astype(np.float32), err_msg="the labels the inputs were built for, image %d" % i)
    assert out["sampled_inds"].shape == (len(tgt), batch) and out["sampled_inds"].dtype == np.int64 and out["counts"].dtype == np.int32
    return _sampled_lists(out), out["counts"]


def _labels(seed, n, p_pos, p_ignore):
    u = synth.uniform01(seed, "rpnloss.labels.%d" % n, n)
    return np.where(u < p_pos, 1, np.where(u < p_pos + p_ignore, -1, 0)).astype(np.int64)


def _quota_lists():
    """The quota edges of test_boxsample_gpu._quota_batch (labels in {1, 0, -1}), plus one 270 000-anchor image."""
    return [np.zeros(50, np.int64), _labels(2, 300, 0.9, 0.08), _labels(3, 7, 0.4, 0.2), np.full(9, -1, np.int64), np.array([1], np.int64),
            _labels(4, 1000, 0.3, 0.1), _labels(5, 6144, 0.5, 0.05), _labels(6, 270000, 0.01, 0.3)]


@pytest.mark.parametrize("batch,fraction", [(1, 0.25), (2, 0.5), (16, 0.25), (256, 0.5), (512, 0.0), (512, 1.0), (2048, 0.25), (2048, 1.0)])
def test_sampler_quota_edges_and_invariants(batch, fraction):
    seed = 31 + batch
    for labels in _quota_lists():
        (sampled,), counts = _sample([labels], batch, fraction, seed)
        pos, neg, num_pos, num_neg = np_quota(labels, batch, fraction)
        assert num_pos == min(len(pos), int(batch * fraction)) and num_neg == min(len(neg), batch - num_pos)    # the reference's two formulas
        assert counts.tolist() == [[num_pos, num_neg]], len(labels)
        assert (np.diff(sampled) > 0).all() and (len(sampled) == 0 or (0 <= sampled[0] and sampled[-1] < len(labels)))
        assert int((labels[sampled] >= 1).sum()) == num_pos and int((labels[sampled] == 0).sum()) == num_neg
        np.testing.assert_array_equal(sampled, np_box_subsample(labels, 0, seed, batch, fraction), err_msg="%d labels" % len(labels))
        if len(labels) <= 6144:
            rows, cnt = bs.box_subsample(torch.from_numpy(labels).to(DEV), [len(labels)], batch, fraction, seed=seed)
            np.testing.assert_array_equal(sampled, rows[0, :int(cnt[0])].cpu().numpy(), err_msg="veto_box_subsample, %d labels" % len(labels))


def test_same_seed_same_rows_other_seed_other_rows_and_no_dependence_on_the_images_behind():
    a_lab, b_lab = _labels(4, 1000, 0.3, 0.1), _labels(6, 1000, 0.5, 0.0)
    (a, _), (b, _), (c, _) = _sample([a_lab, b_lab], 64, 0.25, 77), _sample([a_lab, b_lab], 64, 0.25, 77), _sample([a_lab, b_lab], 64, 0.25, 78)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    lists = [a_lab, b_lab, _labels(7, 1000, 0.2, 0.2), a_lab]
    more, _ = _sample(lists, 64, 0.25, 77)
    assert np.array_equal(more[0], a[0]) and np.array_equal(more[1], a[1])
    assert not np.array_equal(more[3], more[0])            # the same image at another index draws differently
    rows, cnt = bs.box_subsample(torch.from_numpy(np.concatenate(lists)).to(DEV), [1000] * 4, 64, 0.25, seed=77)
    for i, labels in enumerate(lists):                     # every image index: the numpy restatement and veto_box_subsample
        np.testing.assert_array_equal(more[i], np_box_subsample(labels, i, 77, 64, 0.25), err_msg="image %d" % i)
        np.testing.assert_array_equal(more[i], rows[i, :int(cnt[i])].cpu().numpy(), err_msg="veto_box_subsample, image %d" % i)


def test_subsets_are_uniform():
    """One call over C copies of one image (each copy draws from its own stream): 40 anchors, 12 positive, budget 16 at 0.25:
    4 of the 12 positives and 12 of the 28 negatives.  Every candidate must be included with frequency k / m; the allowed
    deviation is the exact binomial one for a false-failure probability of 1e-6 over all 40 comparisons."""
    C = 2000
    labels = np.zeros(40, np.int64)
    pos = np.array([0, 3, 4, 9, 13, 17, 18, 22, 27, 31, 36, 39])
    labels[pos] = 1
    neg = np.nonzero(labels == 0)[0]
    got, counts = _sample([labels] * C, 16, 0.25, 2024)
    count = np.zeros(40)
    for sampled in got:
        assert len(sampled) == 16 and int((labels[sampled] >= 1).sum()) == 4
        count[sampled] += 1
    for what, idx, p in (("positive inclusion", pos, 4 / 12), ("negative inclusion", neg, 12 / 28)):
        bound = binomial_bound(C, p, 40)
        worst = float(np.abs(count[idx] - C * p).max())
        print("%s: expected %.1f of %d, worst deviation %.1f, bound %.1f" % (what, C * p, C, worst, bound))
        assert worst < bound, (what, count[idx], C * p, bound)


# ---- losses and gradients at the device's own sampled anchors --------------------------------------------------------------

def _loss_bound():
    """4 x the largest relative fp32 error the reference's own losses have against its float64 run, over all fixtures (the
    maximum, so that one lucky fixture cannot set it)."""
    return 4 * max(float(rc.load_case(name)[0]["ref_fp32_err_loss"]) for name in rc.ALL)


@pytest.fixture(scope="module")
def parity_report():
    """Collects one line per fixture; profiles/rpnloss_parity.txt is written once, after the last case, and only by a run that
    covered every fixture (a run of some cases leaves the committed record alone)."""
    lines = {}
    yield lines
    if set(lines) != set(rc.ALL):
        return
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        f.write("RPN loss on the device against the float64 oracle at the device's own sampled anchors; bound = 4 x the largest "
                "ref_fp32_err_loss of the fixtures = %.3g, relative: the losses, and every gradient element at a sampled position "
                "against its own oracle value (the figure is the worst element)\n" % _loss_bound())
        for k in rc.ALL:
            f.write(lines[k] + "\n")


ALL_WANT = ("losses", "grads", "labels", "regression_targets", "sampled_inds", "counts")


def _worst_relative(got_levels, ref_levels):
    """The largest |got - ref| / |ref| over the elements the oracle's gradient touches (the sampled positions); 0 when there are none."""
    worst = 0.0
    for got, ref in zip(got_levels, ref_levels):
        at = ref != 0
        if at.any():
            worst = max(worst, float((np.abs(got[at].astype(np.float64) - ref[at]) / np.abs(ref[at])).max()))
    return worst


@pytest.mark.parametrize("name", rc.ALL)
def test_losses_and_gradients_match_the_fp64_oracle(name, parity_report):
    """Both losses within the bound, relative.  Gradients element by element at the sampled positions under the same relative
    bound, each against its own oracle value (the oracle is given the device's fp32 regression targets and the same fp32 head
    outputs, so every residual is exact in double on both sides), exactly zero everywhere else, and two calls give the same bits."""
    z, c, d = rc.load_case(name)
    bound = _loss_bound()
    out = _call(c, d, ALL_WANT, seed=2025)
    again = _call(c, d, ALL_WANT, seed=2025)
    n, shapes = len(d["tgt_boxes"]), d["level_shapes"]
    sampled = _sampled_lists(out)
    for i in range(n):
        labels = z["labels_%d" % i].astype(np.float32)
        np.testing.assert_array_equal(out["labels"][i], labels)
        np.testing.assert_array_equal(sampled[i], np_box_subsample(labels.astype(np.int64), i, 2025, c["batch"], c["fraction"]))
    lo, lb, g_obj, g_box = rc.rpn_loss_fp64(d["objectness"], d["box_regression"], shapes, sampled, list(out["labels"]),
                                            list(out["regression_targets"]))
    err_o = abs(float(out["losses"][0]) - lo) / abs(lo)
    err_b = abs(float(out["losses"][1]) - lb) / abs(lb) if lb != 0 else abs(float(out["losses"][1]))
    gerr_o, gerr_b = _worst_relative(out["d_objectness"], g_obj), _worst_relative(out["d_box_regression"], g_box)
    line = ("%-10s S %4d P %4d  objectness_loss %.9g (rel err %.3g)  box_loss %.9g (rel err %.3g)  d objectness rel err %.3g  d box_regression rel err %.3g"
            % (name, sum(len(s) for s in sampled), int(out["counts"][:, 0].sum()), out["losses"][0], err_o, out["losses"][1], err_b, gerr_o, gerr_b))
    print("PARITY bound %.3g  %s" % (bound, line))
    parity_report[name] = line
    assert err_o <= bound and err_b <= bound and gerr_o <= bound and gerr_b <= bound
    for got, ref in list(zip(out["d_objectness"], g_obj)) + list(zip(out["d_box_regression"], g_box)):
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert not got[ref == 0].any()                                      # exact zero off the sampled positions
        assert (got[ref != 0] != 0).all()
    for key in ("losses", "sampled_inds", "counts"):
        assert out[key].tobytes() == again[key].tobytes(), key
    for key in ("d_objectness", "d_box_regression"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[key], again[key])), key
    if name == "no_pos":
        assert out["losses"][1] == 0 and int(out["counts"][:, 0].sum()) == 0 and not any(g.any() for g in out["d_box_regression"])


def test_an_all_ignored_batch_gives_nan():
    """Images smaller than every anchor: no anchor is visible, nothing is sampled, both losses are the mean of nothing."""
    _, c, d = rc.load_case("lowq")
    d["image_sizes"] = [(5, 5)]
    out = _call(c, d, ALL_WANT, seed=3)
    assert (out["labels"] == -1).all() and out["counts"].tolist() == [[0, 0]]
    assert math.isnan(out["losses"][0]) and math.isnan(out["losses"][1])
    assert not any(g.any() for g in out["d_objectness"] + out["d_box_regression"])


# ---- autograd --------------------------------------------------------------------------------------------------------------

def _cfg(c):
    rpn = types.SimpleNamespace(FG_IOU_THRESHOLD=c["high"], BG_IOU_THRESHOLD=c["low"], BATCH_SIZE_PER_IMAGE=c["batch"],
                                POSITIVE_FRACTION=c["fraction"], STRADDLE_THRESH=c["straddle"])
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN=rpn))


def _box_lists(d):
    anchors = [[BoxList(torch.from_numpy(a).to(DEV), size, "xyxy") for a in d["anchors"]] for size in d["image_sizes"]]
    targets = [BoxList(torch.from_numpy(t).to(DEV), size, "xyxy") for t, size in zip(d["tgt_boxes"], d["image_sizes"])]
    return anchors, targets


def test_backward_puts_the_scaled_gradients_into_every_levels_grad():
    """(2 objectness_loss + 3 box_loss).backward() through RPNLossComputation on fpn5, the head outputs non-contiguous NCHW views of
    NHWC leaves: the leaves' .grad are the call's gradients times 2 and 3, bit for bit; prepare_targets equals the fixture."""
    z, c, d = rc.load_case("fpn5")
    loss = rl.make_rpn_loss_evaluator(_cfg(c), rl.BoxCoder(rc.WEIGHTS))
    anchors, targets = _box_lists(d)
    leaves_o = [torch.from_numpy(o).to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_() for o in d["objectness"]]
    leaves_r = [torch.from_numpy(r).to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_() for r in d["box_regression"]]
    obj, reg = [t.permute(0, 3, 1, 2) for t in leaves_o], [t.permute(0, 3, 1, 2) for t in leaves_r]
    assert not obj[0].is_contiguous()
    lo, lb = loss(anchors, obj, reg, targets, seed=11)
    assert lo.dim() == 0 and lb.dim() == 0 and lo.requires_grad and lb.requires_grad
    (2 * lo + 3 * lb).backward()
    ref = rl.rpn_loss_call(_dev(d["anchors"]), d["image_sizes"], _dev(d["tgt_boxes"]), high_threshold=c["high"], low_threshold=c["low"],
                           allow_low_quality_matches=True, straddle_thresh=c["straddle"], batch_size_per_image=c["batch"],
                           positive_fraction=c["fraction"], seed=11, objectness=_dev(d["objectness"]), box_regression=_dev(d["box_regression"]))
    assert torch.equal(torch.stack([lo.detach(), lb.detach()]), ref["losses"])
    for leaf, want in zip(leaves_o, ref["d_objectness"]):
        assert torch.equal(leaf.grad.permute(0, 3, 1, 2), want * 2)
    for leaf, want in zip(leaves_r, ref["d_box_regression"]):
        assert torch.equal(leaf.grad.permute(0, 3, 1, 2), want * 3)
    assert any(w.any() for w in ref["d_objectness"]) and any(w.any() for w in ref["d_box_regression"])
    labels, reg_targets = loss.prepare_targets(anchors, targets)
    for i in range(2):
        np.testing.assert_array_equal(labels[i].cpu().numpy(), z["labels_%d" % i].astype(np.float32))
        assert reg_targets[i].shape == (12276, 4)
    plain = loss(anchors, [o.detach() for o in obj], [r.detach() for r in reg], targets, seed=11)    # nothing requires grad: no gradients asked
    assert not plain[0].requires_grad and torch.equal(torch.stack(plain), ref["losses"])
    torch.manual_seed(5)                                                    # seed=None draws from torch's CPU generator
    first = loss(anchors, obj, reg, targets)[0].item()
    torch.manual_seed(5)
    assert loss(anchors, obj, reg, targets)[0].item() == first


# ---- launches and copies of a call -----------------------------------------------------------------------------------------

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
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and "rpn_" in e.name]
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


def test_launches_and_device_to_host_copies_of_a_call():
    """Seven launches for the losses with their gradients and three for prepare_targets, whether the batch has 1 or 4 images and the
    pyramid 1 or 5 levels; no copy of any direction, so no device->host copy (test_the_copy_count_sees_a_read_back)."""
    got = {}
    for name, n_img in (("fpn5", 1), ("ragged_gt", 4), ("one_level", 1), ("fpn5", 2)):
        _, c, d = rc.load_case(name)
        d = dict(d, tgt_boxes=d["tgt_boxes"][:n_img], image_sizes=d["image_sizes"][:n_img], objectness=[o[:n_img] for o in d["objectness"]],
                 box_regression=[r[:n_img] for r in d["box_regression"]])
        loss = rl.make_rpn_loss_evaluator(_cfg(c), rl.BoxCoder(rc.WEIGHTS))
        anchors, targets = _box_lists(d)
        obj, reg = [t.requires_grad_() for t in _dev(d["objectness"])], [t.requires_grad_() for t in _dev(d["box_regression"])]
        loss(anchors, obj, reg, targets, seed=1)                            # warm-up: code objects, the cached sizes and offsets
        loss.prepare_targets(anchors, targets)
        full = _profile(lambda: loss(anchors, obj, reg, targets, seed=1))
        prep = _profile(lambda: loss.prepare_targets(anchors, targets))
        print("%s, %d images, %d levels: %d launches and %d memcpy calls for the losses, %d and %d for prepare_targets"
              % ((name, n_img, len(d["anchors"])) + full + prep))
        got[(n_img, len(d["anchors"]))] = (full, prep)
    assert set(got) == {(1, 5), (4, 3), (1, 1), (2, 5)}
    assert all(v == ((7, 0), (3, 0)) for v in got.values()), got


# ---- limits ----------------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_truncations(monkeypatch):
    calls = []
    real = native.Launch.run

    def run(self, name, *tail, **kw):
        calls.append(name)
        return real(self, name, *tail, **kw)
    monkeypatch.setattr(native.Launch, "run", run)
    _, c, d = rc.load_case("lowq")
    anchors, tgt = _dev(d["anchors"]), _dev(d["tgt_boxes"])
    kw = dict(high_threshold=0.7, low_threshold=0.3, want=("labels", "counts"))
    with pytest.raises(ValueError, match="image 0 holds 257 GT boxes, the limit is 256"):
        rl.rpn_loss_call(anchors, d["image_sizes"], [tgt[0][:1].repeat(257, 1)], **kw)
    with pytest.raises(ValueError, match="an image holds 1048577 anchors, the limit is 1048576"):
        rl.rpn_loss_call([anchors[0][:1].repeat(1048577, 1)], d["image_sizes"], tgt, **kw)
    with pytest.raises(ValueError, match=r"batch_size_per_image 2049 outside 1\.\.2048"):
        rl.rpn_loss_call(anchors, d["image_sizes"], tgt, batch_size_per_image=2049, **kw)
    with pytest.raises(ValueError, match=r"9 pyramid levels: 1\.\.8 are supported"):
        rl.rpn_loss_call(anchors * 9, d["image_sizes"], tgt, **kw)
    with pytest.raises(ValueError, match="No ground-truth boxes available for one of the images during training"):
        rl.rpn_loss_call(anchors, d["image_sizes"], [tgt[0][:0]], **kw)
    assert calls == []                                                      # refused before anything was launched
    # the limits themselves are fine: 1 048 576 anchors (the sampler's streaming path: its cut bin holds some 4000 keys), batch 2048, 8 levels
    n = 1 << 20
    x0 = (np.arange(n, dtype=np.float32) % 4096) * 8
    y0 = (np.arange(n, dtype=np.int64) // 4096).astype(np.float32) * 8
    big = np.stack([x0, y0, x0 + 15, y0 + 15], 1)
    j = np.array([0, 1, 37], np.float32)                                    # (256 GT boxes: the ragged_gt fixture)
    gt = np.stack([j * 64, j * 4, j * 64 + 17, j * 4 + 15], 1)
    cc = dict(high=0.7, low=0.3, lowq=True, straddle=0, batch=2048, fraction=0.5)
    dd = dict(anchors=list(np.split(big, 8)), tgt_boxes=[gt], image_sizes=[(32768, 2000)], level_shapes=[(1, 1, n // 8)] * 8)
    out = _call(cc, dd, ("labels", "matched_idxs", "sampled_inds", "counts"), seed=9, head=False)
    matched, labels, _, _ = rc.np_rpn_match(big, gt, (32768, 2000), 0.7, 0.3, True, 0, chunk=1 << 15)
    np.testing.assert_array_equal(out["labels"][0], labels)
    np.testing.assert_array_equal(out["matched_idxs"][0], matched)
    assert (labels == 1).any() and (labels == -1).any() and (labels == 0).sum() > 2048
    np.testing.assert_array_equal(_sampled_lists(out)[0], np_box_subsample(labels.astype(np.int64), 0, 9, 2048, 0.5))
    assert calls == ["veto_rpn_loss"]
