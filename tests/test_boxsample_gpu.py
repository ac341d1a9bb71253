"""sgdet training on the MI355X, the box head's sampler: veto_box_match and veto_box_subsample (veto_amd.boxsampling) bit for bit
against the reference's fixtures (tests/golden/boxsample) and the numpy restatement of tests/test_boxsample_host.py, at the tile
edges, the quota edges and the limits; the seeds, the distribution of the draws over one launch of many copies of an image, the
launches and copies of a call, and the chain assign_label_to_proposals -> boxhead.PostProcessor -> VETORelationHead training on
detected boxes.  Every measured figure is printed before it is asserted (pytest -s)."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_boxsample_host import (HAND, SEEDED, box_lists, case_params, check_sampled_against_fixture, load_case, np_box_match,  # noqa: E402
                                 np_box_subsample, np_quota)
from test_relsample_gtbox_gpu import binomial_bound  # noqa: E402

from veto_amd import boxsampling as bs  # noqa: E402
from veto_amd import native, synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sampler(high=0.5, low=0.3, batch=256, fraction=0.25, weights=(10., 10., 5., 5.)):
    return bs.FastRCNNSampling(bs.Matcher(high, low), bs.BalancedPositiveNegativeSampler(batch, fraction), bs.BoxCoder(weights))


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


def _match_all(s, images):
    """The three public methods on fresh lists: (assign labels, prepare labels, attributes, targets, matched), numpy per image."""
    props, targets = box_lists(images, DEV)
    assign = _np([p.get_field("labels") for p in s.assign_label_to_proposals(props, targets)])
    props, targets = box_lists(images, DEV)
    labels, attributes, reg, matched = s.prepare_targets(props, targets)
    assert all(not p.has_field("labels") for p in props)          # prepare_targets adds no field (sampling.py:47-82)
    torch.cuda.synchronize()
    return assign, _np(labels), _np(attributes), _np(reg), _np(matched)


def _assert_matches_numpy(images, got, high, low, weights=(10., 10., 5., 5.)):
    assign, prepare, _, reg, matched = got
    worst = 0.0
    for i, d in enumerate(images):
        wm, wa, wp, wt = np_box_match(d["prp_boxes"], d["tgt_boxes"], d["tgt_labels"], high, low, weights)
        np.testing.assert_array_equal(matched[i], wm, err_msg="matched_idxs of image %d" % i)
        np.testing.assert_array_equal(assign[i], wa, err_msg="assign labels of image %d" % i)
        np.testing.assert_array_equal(prepare[i], wp, err_msg="prepare labels of image %d" % i)
        assert matched[i].dtype == assign[i].dtype == prepare[i].dtype == np.int64 and reg[i].dtype == np.float32
        worst = max(worst, float(np.abs(reg[i].astype(np.float64) - wt).max()))
    return worst


# ---- matching and sampling against the goldens ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", SEEDED + HAND)
def test_matching_and_sampling_match_the_reference_fixture(name):
    z, images = load_case(name)
    high, low, batch, fraction, weights = case_params(z)
    s = _sampler(high, low, batch, fraction, weights)
    got = _match_all(s, images)
    assign, prepare, attributes, reg, matched = got
    _assert_matches_numpy(images, got, high, low, weights)
    err = 0.0
    for i in range(len(images)):
        np.testing.assert_array_equal(matched[i], z["matched_%d" % i])
        np.testing.assert_array_equal(assign[i], z["labels_assign_%d" % i])
        np.testing.assert_array_equal(prepare[i], z["labels_prepare_%d" % i])
        np.testing.assert_array_equal(attributes[i], z["attributes_%d" % i])
        err = max(err, float(np.abs(reg[i].astype(np.float64) - z["targets_%d" % i]).max()))
    tol = 4 * float(z["ref_fp32_err_targets"])
    print("%s: regression_targets differ from the reference's by %.3g, allowed %.3g (4x its own fp32 error)" % (name, err, tol))
    assert err <= tol
    # subsample: the fields it adds, and the sampled box lists
    seed = 4242
    props, targets = box_lists(images, DEV)
    for i, p in enumerate(props):
        p.add_field("objectness", torch.arange(len(p), device=DEV, dtype=torch.float32) + 100 * i)
    out = s.subsample(props, targets, seed=seed)
    for i, (p, q) in enumerate(zip(props, out)):
        assert sorted(p.fields()) == sorted(q.fields()) == ["attributes", "labels", "matched_idxs", "objectness", "regression_targets"]
        np.testing.assert_array_equal(p.get_field("labels").cpu().numpy(), prepare[i])
        np.testing.assert_array_equal(p.get_field("matched_idxs").cpu().numpy(), matched[i])
        np.testing.assert_array_equal(p.get_field("regression_targets").cpu().numpy(), reg[i])
        np.testing.assert_array_equal(p.get_field("attributes").cpu().numpy(), attributes[i])
        sampled = (q.get_field("objectness") - 100 * i).long().cpu().numpy()
        np.testing.assert_array_equal(sampled, np_box_subsample(prepare[i], i, seed, batch, fraction), err_msg="sampled_inds of image %d" % i)
        check_sampled_against_fixture(z, i, prepare[i], sampled, batch, fraction)
        assert len(q) == len(sampled) and q.size == p.size and q.mode == p.mode
        np.testing.assert_array_equal(q.bbox.cpu().numpy(), images[i]["prp_boxes"][sampled])
        for k, whole in (("labels", prepare[i]), ("matched_idxs", matched[i]), ("regression_targets", reg[i]), ("attributes", attributes[i])):
            np.testing.assert_array_equal(q.get_field(k).cpu().numpy(), whole[sampled], err_msg=k)


def test_match_targets_to_proposals_returns_the_matched_boxes():
    z, images = load_case("vg")
    high, low, _, _, _ = case_params(z)
    props, targets = box_lists(images[:1], DEV)
    m = _sampler(high, low).match_targets_to_proposals(props[0], targets[0])
    idx = np.maximum(z["matched_0"], 0)
    np.testing.assert_array_equal(m.get_field("matched_idxs").cpu().numpy(), z["matched_0"])
    np.testing.assert_array_equal(m.get_field("labels").cpu().numpy(), images[0]["tgt_labels"][idx])    # the box's own label, also for -1 / -2
    np.testing.assert_array_equal(m.get_field("attributes").cpu().numpy(), images[0]["attributes"][idx])
    np.testing.assert_array_equal(m.bbox.cpu().numpy(), images[0]["tgt_boxes"][idx])


# ---- the size edges ----------------------------------------------------------------------------------------------------

def _edge_image(seed, n_gt, n_prp):
    d = synth.synthetic_relsample_image(seed, n_gt, n_prp, min(2, n_gt * (n_gt - 1)))
    return {"prp_boxes": d["prp_boxes"], "tgt_boxes": d["tgt_boxes"], "tgt_labels": d["tgt_labels"], "image_size": d["image_size"],
            "attributes": synth.integers(seed, "edge.attr", (n_gt, 2), 0, 9)}


@pytest.mark.parametrize("n_gt", [1, 2, 256])
def test_matching_and_sampling_at_the_tile_edges(n_gt):
    """One ragged batch of 1, 255, 256, 257 and 1281 proposals (one thread short of a tile, a full tile, one over, five tiles and
    one) against 1, 2 or 256 GT boxes: every output against the numpy restatement, bit for bit."""
    images = [_edge_image(700 + 10 * n_gt + i, n_gt, n) for i, n in enumerate((1, 255, 256, 257, 1281))]
    s = _sampler(0.5, 0.3, 128, 0.25)
    got = _match_all(s, images)
    worst = _assert_matches_numpy(images, got, 0.5, 0.3)
    print("%d GT boxes: regression_targets differ from the fp32 numpy restatement by %.3g" % (n_gt, worst))
    sampled, counts = bs.box_subsample(torch.from_numpy(np.concatenate(got[1])).to(DEV), [len(d["prp_boxes"]) for d in images], 128, 0.25, seed=9)
    sampled, counts = sampled.cpu().numpy(), counts.cpu().numpy()
    for i in range(len(images)):
        np.testing.assert_array_equal(sampled[i, :counts[i]], np_box_subsample(got[1][i], i, 9, 128, 0.25), err_msg="image %d" % i)


# ---- subsample: quota edges, invariants, seeds -------------------------------------------------------------------------

def _subsample(label_lists, batch, fraction, seed):
    labels = torch.from_numpy(np.concatenate(label_lists).astype(np.int64)).to(DEV)
    sampled, counts = bs.box_subsample(labels, [len(x) for x in label_lists], batch, fraction, seed=seed)
    torch.cuda.synchronize()
    sampled, counts = sampled.cpu().numpy(), counts.cpu().numpy()
    assert sampled.shape == (len(label_lists), batch) and sampled.dtype == np.int64 and counts.dtype == np.int32
    return [sampled[i, :counts[i]] for i in range(len(label_lists))]


def _labels(seed, n, p_pos, p_ignore):
    u = synth.uniform01(seed, "boxsample.labels.%d" % n, n)
    return np.where(u < p_pos, synth.integers(seed, "boxsample.cls.%d" % n, (n,), 1, 151), np.where(u < p_pos + p_ignore, -1, 0)).astype(np.int64)


def _quota_batch():
    """No positive; fewer negatives than their quota; an image smaller than any budget; only ignored proposals; one proposal;
    many of both classes; the largest image."""
    few_neg = _labels(2, 300, 0.9, 0.08)
    return [np.zeros(50, np.int64), few_neg, _labels(3, 7, 0.4, 0.2), np.full(9, -1, np.int64), np.array([5], np.int64),
            _labels(4, 1000, 0.3, 0.1), _labels(5, 6144, 0.5, 0.05)]


@pytest.mark.parametrize("batch,fraction", [(1, 0.25), (2, 0.5), (16, 0.25), (256, 0.25), (512, 0.0), (512, 1.0), (2048, 0.25), (2048, 1.0)])
def test_subsample_quota_edges_and_invariants(batch, fraction):
    lists = _quota_batch()
    got = _subsample(lists, batch, fraction, 31 + batch)
    for i, (labels, sampled) in enumerate(zip(lists, got)):
        pos, neg, num_pos, num_neg = np_quota(labels, batch, fraction)
        assert num_pos == min(len(pos), int(batch * fraction)) and num_neg == min(len(neg), batch - num_pos)    # the reference's two formulas
        assert len(sampled) == num_pos + num_neg, i
        assert (np.diff(sampled) > 0).all() and (len(sampled) == 0 or (0 <= sampled[0] and sampled[-1] < len(labels)))
        assert int((labels[sampled] >= 1).sum()) == num_pos and int((labels[sampled] == 0).sum()) == num_neg
        np.testing.assert_array_equal(sampled, np_box_subsample(labels, i, 31 + batch, batch, fraction), err_msg="image %d" % i)
    assert len(got[3]) == 0 and len(got[0]) == min(50, batch - 0)


def test_same_seed_same_rows_other_seed_other_rows_and_no_dependence_on_the_images_behind():
    lists = [_labels(4, 1000, 0.3, 0.1), _labels(6, 400, 0.5, 0.0)]
    a, b, c = _subsample(lists, 64, 0.25, 77), _subsample(lists, 64, 0.25, 77), _subsample(lists, 64, 0.25, 78)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    more = _subsample(lists + [_labels(7, 90, 0.2, 0.2), lists[0]], 64, 0.25, 77)
    assert np.array_equal(more[0], a[0]) and np.array_equal(more[1], a[1])
    assert not np.array_equal(more[3], more[0])            # the same image at another index draws differently


def test_torch_generator_seeds_the_draws_when_no_seed_is_given():
    _, images = load_case("vg")
    out = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        props, targets = box_lists(images, DEV)
        out.append(_sampler(0.5, 0.3, 16, 0.25).subsample(props, targets)[0].bbox.cpu())
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])


def test_subsets_are_uniform():
    """One launch over C copies of one image (each copy draws from its own stream): 40 proposals, 12 positive, budget 16 at 0.25:
    4 of the 12 positives and 12 of the 28 negatives.  Every candidate must be included with frequency k / m; the allowed
    deviation is the exact binomial one for a false-failure probability of 1e-6 over all 40 comparisons."""
    C = 2000
    labels = np.zeros(40, np.int64)
    pos = np.array([0, 3, 4, 9, 13, 17, 18, 22, 27, 31, 36, 39])
    labels[pos] = 1 + np.arange(12)
    neg = np.nonzero(labels == 0)[0]
    got = _subsample([labels] * C, 16, 0.25, 2024)
    count = np.zeros(40)
    for sampled in got:
        assert len(sampled) == 16 and int((labels[sampled] >= 1).sum()) == 4
        count[sampled] += 1
    for what, idx, p in (("positive inclusion", pos, 4 / 12), ("negative inclusion", neg, 12 / 28)):
        bound = binomial_bound(C, p, 40)
        worst = float(np.abs(count[idx] - C * p).max())
        print("%s: expected %.1f of %d, worst deviation %.1f, bound %.1f" % (what, C * p, C, worst, bound))
        assert worst < bound, (what, count[idx], C * p, bound)


# ---- limits ------------------------------------------------------------------------------------------------------------

def _count_launches(monkeypatch):
    calls = []
    real = native.Launch.run

    def run(self, name, *tail, **kw):
        calls.append(name)
        return real(self, name, *tail, **kw)
    monkeypatch.setattr(native.Launch, "run", run)
    return calls


def _plain_lists(n_prp, n_gt):
    props, targets = [], []
    for i, (n, m) in enumerate(zip(n_prp, n_gt)):
        d = _edge_image(900 + i, max(m, 1), max(n, 1))
        props.append(BoxList(torch.from_numpy(d["prp_boxes"][:n]).to(DEV), d["image_size"], "xyxy"))
        t = BoxList(torch.from_numpy(d["tgt_boxes"][:m]).to(DEV), d["image_size"], "xyxy")
        t.add_field("labels", torch.from_numpy(d["tgt_labels"][:m]).to(DEV))
        targets.append(t)
    return props, targets


def test_limits_are_errors_not_truncations(monkeypatch):
    s = _sampler()
    for method in ("assign_label_to_proposals", "prepare_targets", "subsample"):
        call = getattr(s, method)
        with pytest.raises(native.VetoError, match="img_tgt_offset_host: segment 1 holds 257 boxes, the limit is 256"):
            call(*_plain_lists((20, 30), (5, 257)))
        with pytest.raises(native.VetoError, match="img_prp_offset_host: segment 0 holds 6145 boxes, the limit is 6144"):
            call(*_plain_lists((6145, 30), (5, 3)))
        with pytest.raises(ValueError, match="No ground-truth boxes available for one of the images during training"):
            call(*_plain_lists((20, 30), (5, 0)))
        with pytest.raises(ValueError, match="No proposal boxes available for one of the images during training"):
            call(*_plain_lists((0, 30), (5, 3)))
    calls = _count_launches(monkeypatch)
    big = _sampler(batch=2049)
    with pytest.raises(ValueError, match=r"batch_size_per_image 2049 outside 1\.\.2048"):
        big.subsample(*_plain_lists((20, 30), (5, 3)))
    assert calls == []                                                    # refused before the matching was launched
    with pytest.raises(ValueError, match=r"batch_size_per_image 2049 outside 1\.\.2048"):
        bs.box_subsample(torch.zeros(5, dtype=torch.int64, device=DEV), [5], 2049, 0.25, seed=1)
    with pytest.raises(ValueError, match="No proposal boxes available"):
        bs.box_subsample(torch.zeros(5, dtype=torch.int64, device=DEV), [5, 0], 16, 0.25, seed=1)
    # the limits themselves are fine
    props, targets = _plain_lists((6144, 30), (256, 3))
    out = _sampler(batch=2048, fraction=0.25).subsample(props, targets, seed=1)
    labels = props[0].get_field("labels").cpu().numpy()
    _, _, num_pos, num_neg = np_quota(labels, 2048, 0.25)
    assert len(out[0]) == num_pos + num_neg and len(props[0].get_field("matched_idxs")) == 6144
    assert calls == ["veto_box_match", "veto_box_subsample"]


# ---- launches and copies of a call -------------------------------------------------------------------------------------

def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and ("box_match" in e.name or "box_subsample" in e.name)]
    d2h = sum(1 for e in ev if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    return sum("box_match" in k for k in kernels), sum("box_subsample" in k for k in kernels), d2h


def test_launches_and_device_to_host_copies_of_a_call():
    """assign_label_to_proposals and prepare_targets: one launch and no device->host copy; subsample: two launches and the one
    read-back of the counts."""
    _, images = load_case("ragged")
    s = _sampler(0.5, 0.3, 64, 0.25)
    for method, want in (("assign_label_to_proposals", (1, 0, 0)), ("prepare_targets", (1, 0, 0)), ("subsample", (1, 1, 1))):
        getattr(s, method)(*box_lists(images, DEV))                       # warm-up: code objects, the cached offsets
        props, targets = box_lists(images, DEV)
        got = _profile(lambda: getattr(s, method)(props, targets))
        print("%s: %d box_match launches, %d box_subsample launches, %d device->host copies" % ((method,) + got))
        assert got == want, method


# ---- the chain: box-head labels -> PostProcessor -> relation head training -----------------------------------------------

def test_assigned_labels_carry_sgdet_training_from_the_box_head_to_the_relation_losses():
    """2 images of 30 proposals, L2/H8: assign_label_to_proposals -> boxhead.PostProcessor(relation_mode=True) in training ->
    VETORelationHead with DEVICE_DETECT_RELSAMPLE and a fixed seed.  The losses are finite and bit-equal to those of the same
    chain fed with the numpy restatement's labels."""
    from test_relsample_gpu import _sgdet_head
    from veto_amd.boxhead import PostProcessor
    dev = torch.device("cuda:0")
    n_cls, W, H = 151, 800, 600
    rng = np.random.RandomState(5)
    feats = [torch.from_numpy((0.5 * rng.randn(2, 256, H >> (2 + l), W >> (2 + l))).astype(np.float32)).to(dev) for l in range(4)]
    depth = torch.from_numpy((0.5 * rng.randn(2, 256, H >> 4, W >> 4)).astype(np.float32)).to(dev)
    heads, targets, np_labels = [], [], []
    for i in range(2):
        o = synth.synthetic_box_head_outputs(60 + i, 30, num_obj_cls=n_cls, W=W, H=H)
        gt_rows = np.arange(0, 30, 5)                                      # six GT boxes: every fifth proposal, so its cluster matches it
        tgt_boxes = o["proposals"][gt_rows]
        tgt_labels = synth.integers(60 + i, "chain.labels", (len(gt_rows),), 1, n_cls)
        rel = np.zeros((len(gt_rows), len(gt_rows)), np.int64)
        for h, t in ((0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3)):
            rel[h, t] = 1 + (3 * h + t) % 50
        t = BoxList(torch.from_numpy(tgt_boxes), (W, H), "xyxy").to(dev)
        t.add_field("labels", torch.from_numpy(tgt_labels).to(dev))
        t.add_field("relation", torch.from_numpy(rel).to(dev))
        targets.append(t)
        heads.append(o)
        np_labels.append(np_box_match(o["proposals"], tgt_boxes, tgt_labels, 0.5, 0.3)[1])
    class_logits = torch.from_numpy(np.concatenate([o["class_logits"] for o in heads])).to(dev)
    box_regression = torch.from_numpy(np.concatenate([o["box_regression"] for o in heads])).to(dev)
    cfg, head = _sgdet_head(False, dev)
    post = PostProcessor(score_thresh=0.01, nms=0.5, detections_per_img=80, box_coder=bs.BoxCoder((10., 10., 5., 5.)))
    post.train()
    sampler = bs.make_roi_box_samp_processor(cfg)

    def chain(labels_from_device):
        props = [BoxList(torch.from_numpy(o["proposals"]), (W, H), "xyxy").to(dev) for o in heads]
        if labels_from_device:
            props = sampler.assign_label_to_proposals(props, targets)
        else:
            for p, l in zip(props, np_labels):
                p.add_field("labels", torch.from_numpy(l).to(dev))
        for p, logits in zip(props, class_logits.split([30, 30])):
            p.add_field("predict_logits", logits)
        _, dets = post((torch.zeros(60, 8, device=dev), class_logits, box_regression), props, relation_mode=True)
        assert all(d.has_field("labels") and len(d) > 0 for d in dets)
        torch.manual_seed(11)
        random.seed(11)
        _, out, losses = head(feats, dets, targets=targets, depth_features=depth, logger=None, x=None)
        return [d.get_field("labels").cpu().numpy() for d in dets], {k: float(v.detach()) for k, v in losses.items()}

    for p, l in zip(sampler.assign_label_to_proposals([BoxList(torch.from_numpy(o["proposals"]), (W, H), "xyxy").to(dev) for o in heads], targets),
                    np_labels):
        np.testing.assert_array_equal(p.get_field("labels").cpu().numpy(), l)
        assert (l > 0).sum() >= 6
    det_labels, device_losses = chain(True)
    _, host_losses = chain(False)
    print("losses with the device's labels %s, with the numpy restatement's %s" % (device_losses, host_losses))
    assert any((l > 0).any() for l in det_labels)
    assert device_losses and all(math.isfinite(v) for v in device_losses.values())
    assert device_losses == host_losses
