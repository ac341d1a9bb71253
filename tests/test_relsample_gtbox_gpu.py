"""predcls / sgcls training on the MI355X: veto_gtbox_relsample (GTBoxRelationSampler) bit for bit against the numpy restatement
of tests/test_relsample_gtbox_host.py, its seeds, its distributions over one launch of many copies of an image, its limits,
and VETORelationHead training on GT boxes without a host sampler (predcls and sgcls, vanilla and MEET)."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_relsample_gtbox_host import GOLDEN, check_against_fixture, np_candidates, np_gtbox_relsample  # noqa: E402

from veto_amd import native, synth, testing  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lists(rels):
    props, targets = [], []
    for rel in rels:
        n = rel.shape[0]
        boxes = torch.zeros((n, 4), device=DEV)
        props.append(BoxList(boxes, (800, 600), "xyxy"))
        t = BoxList(boxes.clone(), (800, 600), "xyxy")
        t.add_field("relation", torch.from_numpy(np.ascontiguousarray(rel)).to(DEV))
        targets.append(t)
    return props, targets


def _run(rels, seed, batch=1024, frac=0.25):
    from veto_amd.sampling import GTBoxRelationSampler
    props, targets = _lists(rels)
    props, labels, pairs, binary = GTBoxRelationSampler(batch, frac).gtbox_relsample(props, targets, seed=seed)
    torch.cuda.synchronize()
    assert all(torch.equal(p.get_field("locating_match"), torch.ones(len(p), device=DEV)) for p in props)
    return [x.cpu().numpy() for x in pairs], [x.cpu().numpy() for x in labels], [x.cpu().numpy() for x in binary]


def _assert_matches_numpy(rels, seed, batch, frac):
    pairs, labels, binary = _run(rels, seed, batch, frac)
    for i, rel in enumerate(rels):
        wp, wl, wb, _, _ = np_gtbox_relsample(rel, i, seed, batch, int(batch * frac))
        np.testing.assert_array_equal(pairs[i], wp, err_msg="pairs of image %d" % i)
        np.testing.assert_array_equal(labels[i], wl, err_msg="labels of image %d" % i)
        np.testing.assert_array_equal(binary[i], wb, err_msg="binary_rel of image %d" % i)
    return pairs, labels, binary


def _random_relation(seed, n, density, num_rel_cls=51):
    u = synth.uniform01(seed, "gt.rel.%d" % n, n * n).reshape(n, n)
    rel = np.where(u < density, synth.integers(seed, "gt.lab.%d" % n, (n, n), 1, num_rel_cls), 0)
    np.fill_diagonal(rel, 0)
    return rel.astype(np.int64)


def _ragged_batch():
    """1, 2 and 256 objects, a matrix without a relation, one with every off-diagonal entry set (no background), negative
    entries (not foreground: `relation > 0`), a set diagonal entry (foreground, as torch.nonzero has it)."""
    full = np.full((9, 9), 3, np.int64)
    np.fill_diagonal(full, 0)
    odd = _random_relation(5, 12, 0.3)
    odd[2, 5], odd[7, 7], odd[0, 1] = -4, 9, -1
    return [np.zeros((1, 1), np.int64), _random_relation(1, 2, 0.6), _random_relation(2, 256, 0.4), np.zeros((17, 17), np.int64),
            full, odd, _random_relation(3, 256, 0.001), _random_relation(4, 70, 0.05)]


def test_kernel_matches_the_numpy_restatement_on_the_fixture_batch():
    g = np.load(GOLDEN)
    rels = [rel for _, rel in synth.synthetic_relation_targets()]
    pairs, labels, binary = _assert_matches_numpy(rels, 1234, 1024, 0.25)
    for i, rel in enumerate(rels):
        check_against_fixture(i, rel, pairs[i], labels[i], binary[i], g)
    assert [len(p) for p in pairs] == [30, 1024, 6, 0]


@pytest.mark.parametrize("batch,frac", [(1, 0.25), (256, 0.25), (2048, 0.25), (2048, 1.0), (64, 0.0)])
def test_kernel_matches_the_numpy_restatement_on_a_ragged_batch(batch, frac):
    rels = _ragged_batch()
    pairs, labels, _ = _assert_matches_numpy(rels, 99 + batch, batch, frac)
    assert len(pairs[0]) == 0 and all(len(p) <= batch for p in pairs)
    fg, bg = np_candidates(rels[4])
    assert len(bg) == 0 and len(pairs[4]) == min(len(fg), int(batch * frac)) and (labels[4] == 3).all()


def test_same_seed_same_rows_other_seed_other_rows():
    rels = [rel for _, rel in synth.synthetic_relation_targets()]
    a, b, c = _run(rels, 77), _run(rels, 77), _run(rels, 78)
    for k in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    assert not np.array_equal(a[0][1], c[0][1])
    assert np.array_equal(a[2][1], c[2][1])     # binary_rel does not depend on the draws


def test_rows_do_not_depend_on_the_images_behind():
    rels = [rel for _, rel in synth.synthetic_relation_targets()]
    alone = _run(rels[:2], 5)
    more = _run(rels[:2] + [_random_relation(6, 90, 0.2), rels[1]], 5)
    for k in range(3):
        assert np.array_equal(alone[k][0], more[k][0]) and np.array_equal(alone[k][1], more[k][1])
    assert not np.array_equal(more[0][1], more[0][3])     # the same image at another index draws differently


def test_torch_generator_seeds_the_draws_when_no_seed_is_given():
    from veto_amd.sampling import GTBoxRelationSampler
    rels = [rel for _, rel in synth.synthetic_relation_targets()]
    out = []
    for s in (3, 3, 4):
        torch.manual_seed(s)
        _, _, pairs, _ = GTBoxRelationSampler(1024, 0.25).gtbox_relsample(*_lists(rels))
        out.append(pairs[1].cpu())
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])


# ---- distributions -----------------------------------------------------------------------------------------------------

def binomial_bound(C, p, n_tests, alpha=1e-6):
    """The smallest d with P(|X - C p| >= d) <= alpha / n_tests for X ~ Binomial(C, p), from the exact probabilities: under
    exact uniform sampling, n_tests such comparisons fail with probability at most alpha altogether (union bound)."""
    x = np.arange(C + 1)
    logpmf = np.array([math.lgamma(C + 1) - math.lgamma(k + 1) - math.lgamma(C - k + 1) for k in x]) \
        + x * math.log(p) + (C - x) * math.log1p(-p)
    pmf = np.exp(logpmf)
    dev = np.abs(x - C * p)
    order = np.argsort(-dev, kind="stable")
    tail = np.cumsum(pmf[order])                      # P(deviation >= dev[order[j]])
    ok = tail <= alpha / n_tests
    assert ok.any()
    return float(dev[order][ok].min())


def test_subsets_and_orders_are_uniform():
    """One launch over C copies of one image (each copy draws from its own stream): 5 objects, 8 foreground candidates of
    which k = 4 are kept, 12 background candidates of which 4 are kept.  Every candidate must be included with frequency
    k / m and come first with frequency 1 / m; the allowed deviation is the exact binomial one for a false-failure
    probability of 1e-6 over all 40 comparisons."""
    C = 2000
    rel = np.zeros((5, 5), np.int64)
    for j, (h, t) in enumerate([(0, 1), (0, 3), (1, 0), (2, 4), (3, 1), (3, 2), (4, 0), (4, 3)]):
        rel[h, t] = 1 + j
    fg, bg = np_candidates(rel)
    m_fg, m_bg, k_fg, k_bg = len(fg), len(bg), 4, 4
    assert (m_fg, m_bg) == (8, 12)
    pairs, labels, _ = _run([rel] * C, 2024, batch=8, frac=0.5)
    fg_index = {r[:2]: j for j, r in enumerate(fg)}
    bg_index = {r: j for j, r in enumerate(bg)}
    fg_count, fg_first, bg_count, bg_first = np.zeros(m_fg), np.zeros(m_fg), np.zeros(m_bg), np.zeros(m_bg)
    for pr, lb in zip(pairs, labels):
        rows = [tuple(r) for r in pr.tolist()]
        assert len(rows) == 8 and len(set(rows)) == 8 and (lb[:4] > 0).all() and (lb[4:] == 0).all()
        assert all(rel[h, t] == lab for (h, t), lab in zip(rows[:4], lb[:4]))
        for r in rows[:4]:
            fg_count[fg_index[r]] += 1
        for r in rows[4:]:
            bg_count[bg_index[r]] += 1
        fg_first[fg_index[rows[0]]] += 1
        bg_first[bg_index[rows[4]]] += 1
    n_tests = 2 * (m_fg + m_bg)
    for what, count, p in (("foreground inclusion", fg_count, k_fg / m_fg), ("background inclusion", bg_count, k_bg / m_bg),
                           ("foreground first", fg_first, 1 / m_fg), ("background first", bg_first, 1 / m_bg)):
        bound = binomial_bound(C, p, n_tests)
        worst = float(np.abs(count - C * p).max())
        print("%s: expected %.1f of %d, worst deviation %.1f, bound %.1f" % (what, C * p, C, worst, bound))
        assert worst < bound, (what, count, C * p, bound)


# ---- limits ------------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_truncations():
    small = _random_relation(1, 6, 0.3)
    with pytest.raises(native.VetoError, match="max_obj_per_image 257 outside 0..256"):
        _run([small, np.zeros((257, 257), np.int64)], 1)
    with pytest.raises(native.VetoError, match="batch_size_per_image 2049 outside 1..2048"):
        _run([small], 1, batch=2049)
    assert native.load_library().veto_last_error().startswith(b"batch_size_per_image")
    pairs, _, _ = _run([small, np.zeros((256, 256), np.int64)], 1, batch=2048)      # the limits themselves are fine
    assert len(pairs[1]) == 2048


# ---- the relation head training on GT boxes --------------------------------------------------------------------------------

W, H = 512, 384


def _head_inputs(dev, num_objs, mode, n_cls=151):
    rng = np.random.RandomState(21)
    B = len(num_objs)
    feats = [torch.from_numpy((0.5 * rng.randn(B, 256, H >> (2 + l), W >> (2 + l))).astype(np.float32)).to(dev) for l in range(4)]
    depth = torch.from_numpy((0.5 * rng.randn(B, 256, H >> 4, W >> 4)).astype(np.float32)).to(dev)
    props, targets = [], []
    for i, (boxes, rel) in enumerate(synth.synthetic_relation_targets(num_objs=num_objs)):
        b = torch.from_numpy(boxes)
        b[:, 2:] = b[:, :2] + b[:, 2:].abs() * 0.5 + 8
        labels = torch.from_numpy(synth.integers(3, "head.labels.%d" % i, (len(boxes),), 1, n_cls))
        p = BoxList(b, (W, H)).to(dev)
        p.add_field("labels", labels.to(dev))
        if mode != "predcls":
            logits = torch.from_numpy(synth.normal(50 + i, "head.logits", (len(boxes), n_cls), 0.0, 1.0)).to(dev)
            p.add_field("predict_logits", logits)
            p.add_field("pred_labels", logits[:, 1:].argmax(1) + 1)
        t = BoxList(b.clone(), (W, H)).to(dev)
        t.add_field("relation", torch.from_numpy(rel).to(dev))
        t.add_field("labels", labels.to(dev))
        props.append(p)
        targets.append(t)
    return feats, depth, props, targets


def _clone(p):
    q = BoxList(p.bbox, p.size, p.mode)
    q.extra_fields = dict(p.extra_fields)
    return q


def _head(mode, meet, dev, device_sampler, samp_processor=None):
    from veto_amd import predictor
    from veto_amd.relation_head import VETORelationHead
    predictor.set_embedding_provider(lambda names, w, k: torch.zeros(len(names), k))
    cfg = testing.make_config(2, 8, mode=mode, meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.EMB_DROPOUT = 0.0
    cfg.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.T_DROPOUT = 0.0
    cfg.VETO_AMD.DEVICE_GTBOX_RELSAMPLE = device_sampler
    head = VETORelationHead(cfg, samp_processor=samp_processor)
    sd = synth.meet_state_dict(0, head.predictor.max_group_element_number_list, layers=2) if meet \
        else synth.predictor_state_dict(3, layers=2)
    head.predictor = testing.make_predictor(cfg, sd, dev)
    head.train()
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return cfg, head


def _step(head, feats, depth, props, targets, seed):
    for p in head.predictor.parameters():
        p.grad = None
    depth.grad = None
    torch.manual_seed(seed)
    random.seed(seed)   # the MEET expert sampling draws from Python's random, as the reference's does
    roi, out_props, losses = head(feats, [_clone(p) for p in props], targets=targets, depth_features=depth, logger=None, x=None)
    sum(losses.values()).backward()
    grads = {n: p.grad.clone() for n, p in head.predictor.named_parameters() if p.grad is not None}
    return roi, out_props, {k: float(v.detach()) for k, v in losses.items()}, grads


@pytest.mark.parametrize("mode", ["predcls", "sgcls"])
@pytest.mark.parametrize("meet", [False, True])
def test_relation_head_trains_on_gt_boxes_without_a_host_sampler(mode, meet):
    from relation_sampling import make_roi_relation_samp_processor    # tests/: the stand-in host sampler
    from veto_amd.sampling import GTBoxRelationSampler
    dev = torch.device("cuda:0")
    num_objs = (7, 40)                      # the second image hits both budgets: 256 + 768 rows
    feats, depth, props, targets = _head_inputs(dev, num_objs, mode)
    depth.requires_grad_(True)
    cfg, head = _head(mode, meet, dev, True)
    assert head.samp_processor is None
    roi, out_props, values, grads = _step(head, feats, depth, props, targets, 11)
    assert all(math.isfinite(v) for v in values.values()) and values
    assert all("locating_match" in p.extra_fields for p in out_props)
    assert roi.shape == (sum(num_objs), 256, 8, 8)
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert depth.grad is not None and torch.isfinite(depth.grad).all() and float(depth.grad.abs().max()) > 0
    # "every used parameter": the parameters that get a gradient when the same head trains with the host sampler
    _, host_head = _head(mode, meet, dev, False, samp_processor=make_roi_relation_samp_processor(cfg))
    _, _, _, host_grads = _step(host_head, feats, depth, props, targets, 11)
    used = {n for n, g in host_grads.items() if float(g.abs().max()) > 0}
    assert len(used) >= 20 and used <= set(grads)
    if not meet:     # (which MEET group heads see a row depends on the expert sampling's draws)
        assert used <= {n for n, g in grads.items() if float(g.abs().max()) > 0}
    # a second step with the same generator state repeats the first
    _, _, again, _ = _step(head, feats, depth, props, targets, 11)
    assert again == values
    # the head's loss is the predictor's loss on the rows GTBoxRelationSampler returns for the same generator state
    torch.manual_seed(11)
    random.seed(11)
    fresh = [_clone(p) for p in props]
    head._overload_predcls_fields(fresh, dev)
    with torch.no_grad():
        fresh, rel_labels, rel_pairs, _ = GTBoxRelationSampler.from_config(cfg).gtbox_relsample(fresh, targets)
    assert len(rel_pairs[1]) == 1024 and int((rel_labels[1] > 0).sum()) == 256
    assert len(rel_pairs[0]) == 42
    roi2, d2, _, _ = head.box_feature_extractor(feats, fresh, depth_features=depth)
    _, _, direct, _, _, _ = head.predictor(fresh, rel_pairs, rel_labels, None, roi_features=roi2, roi_depth_features=d2)
    assert {k: float(v.detach()) for k, v in direct.items()} == values
    # without the key the same call raises what it raises today
    _, plain = _head(mode, meet, dev, False)
    with pytest.raises(ValueError, match="training needs a relation sampler"):
        plain(feats, [_clone(p) for p in props], targets=targets, depth_features=depth, logger=None, x=None)


@pytest.mark.parametrize("mode", ["predcls", "sgcls"])
def test_head_loss_equals_the_host_samplers_when_no_draw_decides_the_rows(mode):
    """7 and 5 objects: the foreground fits the positive budget and every background candidate is taken, so both samplers
    return the same rows, the device sampler's background in its own order.  The relation loss is a mean over the rows: it must
    agree to the tolerance tests/test_train_losses.py uses for a loss, 2e-4 * max(1, |loss|) (dropout off)."""
    from relation_sampling import make_roi_relation_samp_processor
    from veto_amd.sampling import GTBoxRelationSampler
    dev = torch.device("cuda:0")
    feats, depth, props, targets = _head_inputs(dev, (7, 5), mode)
    depth.requires_grad_(True)
    cfg, head = _head(mode, False, dev, True)
    _, host_head = _head(mode, False, dev, False, samp_processor=make_roi_relation_samp_processor(cfg))
    _, _, dev_loss, _ = _step(head, feats, depth, props, targets, 5)
    _, _, host_loss, _ = _step(host_head, feats, depth, props, targets, 5)
    assert set(dev_loss) == set(host_loss) == ({"rel_loss"} if mode == "predcls" else {"rel_loss", "obj_loss"})
    # the same rows once both lists are sorted the same way
    _, dl, dp, db = GTBoxRelationSampler.from_config(cfg).gtbox_relsample([_clone(p) for p in props], targets, seed=1)
    _, hl, hp, hb = make_roi_relation_samp_processor(cfg).gtbox_relsample([_clone(p) for p in props], targets)
    for i in range(2):
        drows = sorted(map(tuple, torch.cat([dp[i], dl[i][:, None]], 1).cpu().tolist()))
        hrows = sorted(map(tuple, torch.cat([hp[i], hl[i][:, None]], 1).cpu().tolist()))
        assert drows == hrows and len(drows) == (42, 20)[i]
        n_fg = int((hl[i] > 0).sum())
        assert torch.equal(dp[i][:n_fg], hp[i][:n_fg]) and torch.equal(dl[i][:n_fg], hl[i][:n_fg])
        assert torch.equal(db[i], hb[i])
    for key, ref in host_loss.items():
        print("%s: %s device sampler %.7f, host sampler %.7f" % (mode, key, dev_loss[key], ref))
        assert abs(dev_loss[key] - ref) < 2e-4 * max(1.0, abs(ref)), (key, dev_loss, host_loss)
