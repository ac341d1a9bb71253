"""sgdet training on the MI355X: veto_detect_relsample (DetectRelationSampler) against the reference's outputs
(tests/golden/sgdet/relsample.npz, and relsample_large.npz at the sizes of sgdet training and at the limits of 256 proposals and
256 GT boxes) and the numpy restatement of tests/test_relsample_host.py, an edge sweep over the mask-word and loop-step sizes,
its distributions over one launch of many copies of an image (in the first and in the last mask word), its limits, and
VETORelationHead training on detected boxes (vanilla and MEET)."""
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relsample_cases as rc  # noqa: E402
from test_relsample_host import (case_config, case_image, case_names, deterministic, load_golden,  # noqa: E402
                                 load_golden_large, np_labels_all_fg, np_relsample_parts, rows_multiset)

from veto_amd import native, synth, testing  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lists(d, copies=1, with_nm=None):
    props, targets = [], []
    for _ in range(copies):
        p = BoxList(torch.from_numpy(d["prp_boxes"]).to(DEV), (800, 600), "xyxy")
        p.add_field("labels", torch.from_numpy(d["prp_labels"]).to(DEV))
        p.add_field("pred_scores", torch.from_numpy(d["pred_scores"]).to(DEV))
        t = BoxList(torch.from_numpy(d["tgt_boxes"]).to(DEV), (800, 600), "xyxy")
        t.add_field("labels", torch.from_numpy(d["tgt_labels"]).to(DEV))
        t.add_field("relation", torch.from_numpy(d["relation"]).to(DEV))
        if (with_nm is None and "relation_non_masked" in d) or with_nm:
            t.add_field("relation_non_masked", torch.from_numpy(d["relation_non_masked"]).to(DEV))
        props.append(p)
        targets.append(t)
    return props, targets


def _sampler(cfg):
    from veto_amd.sampling import DetectRelationSampler
    return DetectRelationSampler(*cfg)


def _check_image(d, cfg, s, pairs, labels, labels_all, binary, locating, g=None, case=None):
    """Everything one image's output must satisfy whatever the draws."""
    per_rel = cfg[2]
    n_fg = s["n_fg"]
    rows = 2 if n_fg == 0 and s["num_neg"] == 0 else n_fg + s["num_neg"]
    assert pairs.shape == (rows, 2) and labels.shape == (rows,)
    np.testing.assert_array_equal(locating, s["locating"])
    np.testing.assert_array_equal(binary, s["binary"])
    assert (labels[:n_fg] > 0).all() and (labels[n_fg:] == 0).all()
    per = {}
    cand = {}
    for i, r in enumerate(s["rels"]):
        for c in r["cand"]:
            cand.setdefault((c[0], c[1], r["label"]), set()).add(i)
    fg = [tuple(x) for x in np.concatenate([pairs[:n_fg], labels[:n_fg, None]], 1).tolist()]
    for row in fg:
        assert row in cand, row
    if s["n_pre"] <= s["num_pos"]:   # no cap: at most per_rel per relation, relation after relation
        for row in fg:
            for i in cand[row]:
                per[i] = per.get(i, 0) + 1
        assert sum(min(len(r["cand"]), per_rel) for r in s["rels"]) == len(fg)
        at = 0
        for i, r in enumerate(s["rels"]):   # relation i owns the next min(candidates, per_rel) rows, all different
            mine = fg[at:at + r["n"]]
            at += r["n"]
            assert len(set(mine)) == len(mine) and all(i in cand[row] for row in mine), (i, mine)
            if len(r["cand"]) <= per_rel:
                assert [(a, b) for a, b, _ in mine] == [tuple(map(int, c)) for c in r["cand"]]
    if s["num_neg"]:
        bg = [tuple(x) for x in pairs[n_fg:].tolist()]
        win = {tuple(x) for x in s["bg_sorted"][:s["window"]].tolist()}
        assert len(set(bg)) == len(bg) and set(bg) <= win
        assert not set(bg) & {(a, b) for a, b, _ in fg}
    if labels_all is not None:
        assert len(labels_all) == s["n_pre"] + rows - n_fg
        corr = [i for i, r in enumerate(s["rels"]) for _ in range(r["n"])]
        np.testing.assert_array_equal(labels_all[:s["n_pre"]], np_labels_all_fg(d, corr))
        assert (labels_all[s["n_pre"]:] == 0).all()
    if g is not None and deterministic(s, per_rel):
        assert rows_multiset(pairs, labels) == rows_multiset(g[case + "__pairs"], g[case + "__labels"])


def _run(d, cfg, seed, copies=1):
    props, targets = _lists(d, copies)
    out = _sampler(cfg).detect_relsample(props, targets, seed=seed)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", case_names(load_golden()))
def test_kernel_matches_the_reference_fixtures(case):
    _kernel_matches_the_reference_fixture(load_golden(), case)


@pytest.mark.parametrize("case", sorted(rc.LARGE_CASES))
def test_kernel_matches_the_reference_fixtures_at_real_and_limit_sizes(case):
    g = load_golden_large()
    d, cfg, s = _kernel_matches_the_reference_fixture(g, case)
    print(rc.record_line(case, d, cfg, s, deterministic(s, cfg[2])))


def _kernel_matches_the_reference_fixture(g, case):
    d, cfg = case_image(g, case), case_config(g, case)
    s = np_relsample_parts(d, *cfg)
    props, labels, labels_all, pairs, binary = _run(d, cfg, 1234)
    la = labels_all[0].cpu().numpy() if "relation_non_masked" in d else None
    if la is None:
        assert labels_all is labels
    np.testing.assert_array_equal(props[0].get_field("locating_match").cpu().numpy(), g[case + "__locating_match"])
    np.testing.assert_array_equal(binary[0].cpu().numpy(), g[case + "__binary_rel"])
    assert len(pairs[0]) == len(g[case + "__pairs"])
    if la is not None:
        np.testing.assert_array_equal(la[:s["n_pre"]], g[case + "__labels_all"][:s["n_pre"]])
        assert len(la) == len(g[case + "__labels_all"])
    _check_image(d, cfg, s, pairs[0].cpu().numpy(), labels[0].cpu().numpy(), la, binary[0].cpu().numpy(),
                 props[0].get_field("locating_match").cpu().numpy(), g, case)
    return d, cfg, s


@pytest.mark.parametrize("sweep", sorted(rc.SWEEPS))
def test_edge_sweep_matches_the_restatement(sweep):
    """Every image of a sweep in one launch: proposals at the mask-word edges 31..33, 63..65 and 255/256, GT boxes at the
    loop-step edges 15..17 (225, 256, 289 cells), 32/33 and 256."""
    cfg, images = rc.sweep_images(sweep)
    props, targets = [], []
    for d in images:
        p, t = _lists(d, with_nm=True)
        props += p
        targets += t
    props, labels, labels_all, pairs, binary = _sampler(cfg).detect_relsample(props, targets, seed=4321)
    for i, d in enumerate(images):
        s = np_relsample_parts(d, *cfg)
        pr, lb, la = pairs[i].cpu().numpy(), labels[i].cpu().numpy(), labels_all[i].cpu().numpy()
        n_fg = int((lb > 0).sum())
        rows = 2 if s["n_fg"] == 0 and s["num_neg"] == 0 else s["n_fg"] + s["num_neg"]
        # counts = (rows, F, n_fg, status): the split of the outputs is made from them, and status 0 is the absence of the IndexError
        assert (len(pr), len(la) - (len(pr) - n_fg), n_fg) == (rows, s["n_pre"], s["n_fg"]), (sweep, i)
        corr = [k for k, r in enumerate(s["rels"]) for _ in range(r["n"])]
        np.testing.assert_array_equal(la[:s["n_pre"]], np_labels_all_fg(d, corr))
        _check_image(d, cfg, s, pr, lb, la, binary[i].cpu().numpy(), props[i].get_field("locating_match").cpu().numpy())
        print(rc.record_line("sweep_%s_%d" % (sweep, i), d, cfg, s, False))


def _outputs(out, i):
    props, labels, labels_all, pairs, binary = out
    return [x.cpu().numpy() for x in (pairs[i], labels[i], labels_all[i], binary[i], props[i].get_field("locating_match"))]


def test_an_image_at_the_limits_does_not_depend_on_its_neighbours():
    """Draws depend on the seed, the image index and the image's own inputs: each image of a ragged batch of limit-size,
    real-size, one-proposal and zero-relation images is bit-equal to the same image at the same position among small ones."""
    g, small = load_golden_large(), load_golden()
    cfg = (0.5, False, 4, 1024, 0.25)
    one = rc.seeded_image(61, 17, 1, 30)
    assert len(one["prp_boxes"]) == 1
    none = rc.seeded_image(62, 33, 65, 0, dict(n_extra_non_masked=0))
    assert not none["relation"].any()
    mixed = [case_image(g, "limit"), case_image(g, "real"), one, none, case_image(g, "padded_deterministic")]
    filler = [case_image(small, c) for c in ("many", "twin", "cap", "small", "degenerate")]
    assert all("relation_non_masked" in d for d in mixed + filler)

    def run(images):
        props, targets = [], []
        for d in images:
            p, t = _lists(d, with_nm=True)
            props += p
            targets += t
        return _sampler(cfg).detect_relsample(props, targets, seed=99)

    together = run(mixed)
    for i, d in enumerate(mixed):
        s = np_relsample_parts(d, *cfg)
        got = _outputs(together, i)
        _check_image(d, cfg, s, got[0], got[1], got[2], got[3], got[4])
        alone = _outputs(run(filler[:i] + [d] + filler[i + 1:]), i)
        for a, b in zip(got, alone):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
    assert len(_outputs(together, 3)[0]) == cfg[3] and not _outputs(together, 3)[1].any()


def test_a_batch_of_images_gives_each_image_its_own_result():
    g = load_golden()
    cases = [c for c in case_names(g) if case_config(g, c) == (0.5, False, 4, 1024, 0.25)]
    assert len(cases) >= 3
    imgs = [case_image(g, c) for c in cases]
    props, targets = [], []
    for d in imgs:
        p, t = _lists(d, with_nm=True)
        props += p
        targets += t
    props, labels, labels_all, pairs, binary = _sampler((0.5, False, 4, 1024, 0.25)).detect_relsample(props, targets, seed=9)
    for i, (c, d) in enumerate(zip(cases, imgs)):
        s = np_relsample_parts(d, *case_config(g, c))
        _check_image(d, case_config(g, c), s, pairs[i].cpu().numpy(), labels[i].cpu().numpy(), labels_all[i].cpu().numpy(),
                     binary[i].cpu().numpy(), props[i].get_field("locating_match").cpu().numpy(), g, c)


def test_same_seed_same_rows_other_seed_other_rows():
    g = load_golden()
    d, cfg = case_image(g, "many"), case_config(g, "many")
    a = _run(d, cfg, 77)
    b = _run(d, cfg, 77)
    c = _run(d, cfg, 78)
    for k in (1, 2, 3, 4):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
    assert not torch.equal(a[3][0], c[3][0])


def test_draws_depend_on_the_seed_and_the_image_index_only():
    g = load_golden()
    d, cfg = case_image(g, "cap"), case_config(g, "cap")
    one = _run(d, cfg, 5, copies=3)
    other = _sampler(cfg).detect_relsample(*_lists(case_image(g, "many")), seed=5)
    props, targets = _lists(case_image(g, "many"))
    p2, t2 = _lists(d, copies=3)
    mixed = _sampler(cfg).detect_relsample(props + p2[1:], targets + t2[1:], seed=5)
    assert torch.equal(mixed[3][1], one[3][1]) and torch.equal(mixed[3][2], one[3][2])
    assert torch.equal(mixed[3][0], other[3][0])
    assert not torch.equal(one[3][0], one[3][1])


# ---- distributions -----------------------------------------------------------------------------------------------------

def _image_six_candidates():
    """GT 0 -> GT 1 (label 7); two detections match GT 0 and three match GT 1 at different IoUs: 6 weighted candidates."""
    g0, g1 = np.array([100, 100, 200, 200.]), np.array([300, 100, 400, 220.])
    prp = np.stack([g0, g0 + [0, 0, 30, 20], g1, g1 + [12, 0, 0, 12], g1 + [-20, -10, 15, 0]]).astype(np.float32)
    return {"prp_boxes": prp, "prp_labels": np.array([3, 3, 5, 5, 5], np.int64),
            "pred_scores": np.array([0.9, 0.3, 0.8, 0.5, 0.6], np.float32),
            "tgt_boxes": np.stack([g0, g1]).astype(np.float32), "tgt_labels": np.array([3, 5], np.int64),
            "relation": np.array([[0, 7], [0, 0]], np.int64)}


def _inclusion_exact(w, k):
    p = np.asarray(w, np.float64) / np.sum(w)
    inc = np.zeros(len(p))
    for seq in itertools.permutations(range(len(p)), k):
        pr, rest = 1.0, 1.0
        for j in seq:
            pr *= p[j] / rest
            rest -= p[j]
        for j in seq:
            inc[j] += pr
    return inc


def _assert_freq(count, n, prob, what):
    sigma = np.sqrt(np.maximum(prob * (1 - prob), 1e-12) / n)
    z = np.abs(count / n - prob) / sigma
    assert (z < 5).all(), (what, count / n, prob, z)


def _image_four_candidates():
    """The first four detections of _image_six_candidates: 2 x 2 candidates, so no draws."""
    d = _image_six_candidates()
    d["prp_boxes"] = d["prp_boxes"][[0, 1, 2, 3]]
    d["prp_labels"], d["pred_scores"] = d["prp_labels"][[0, 1, 2, 3]], d["pred_scores"][[0, 1, 2, 3]]
    return d


def _run_copies(d, cfg, seed, copies):
    """`copies` times the same image in one launch, the inputs uploaded once."""
    (p,), (t,) = _lists(d)
    out = _sampler(cfg).detect_relsample([p] * copies, [t] * copies, seed=seed)
    torch.cuda.synchronize()
    return out


def test_foreground_draws_follow_the_weights():
    _foreground_draws_follow_the_weights(_image_six_candidates(), (1, 2))


def test_foreground_draws_follow_the_weights_in_the_last_mask_word():
    """The same image at proposals 251..255 and GT boxes 254 and 255 of a 256 x 256 one (relation cell 65 279)."""
    d = rc.pad_front(_image_six_candidates(), 256, 256)
    s = np_relsample_parts(d, 0.5, False, 4, 1024, 0.25)
    assert (s["rels"][0]["h"], s["rels"][0]["t"]) == (254, 255) and min(min(c) for c in s["rels"][0]["cand"]) == 251
    _foreground_draws_follow_the_weights(d, (1, 2, 5, 6))


def _foreground_draws_follow_the_weights(d, seeds):
    cfg = (0.5, False, 4, 1024, 0.25)
    s = np_relsample_parts(d, *cfg)
    r = s["rels"][0]
    assert len(r["cand"]) == 6 and len(set(r["weight"].tolist())) == 6
    want = _inclusion_exact(r["weight"], 4)
    N = 2000
    first = np.zeros(6)
    count = np.zeros(6)
    for seed in seeds:
        _, labels, _, pairs, _ = _run_copies(d, cfg, seed, N // len(seeds))
        index = {tuple(map(int, c)): j for j, c in enumerate(r["cand"])}
        for pr, lb in zip(pairs, labels):
            fg = [tuple(x) for x in pr[lb > 0].cpu().numpy().tolist()]
            assert len(fg) == 4 and len(set(fg)) == 4
            for x in fg:
                count[index[x]] += 1
            first[index[fg[0]]] += 1
    _assert_freq(count, N, want, "inclusion")
    p = r["weight"].astype(np.float64) / r["weight"].sum()
    _assert_freq(first, N, p, "first draw")   # draw order: the first row is the first draw


def test_foreground_cap_and_background_subset_are_uniform():
    _foreground_cap_and_background_subset_are_uniform(_image_four_candidates(), (3, 4))


def test_foreground_cap_and_background_subset_are_uniform_in_the_last_mask_word():
    """The same image at proposals 252..255 and GT boxes 254 and 255 of a 256 x 256 one."""
    d = rc.pad_front(_image_four_candidates(), 256, 256)
    s = np_relsample_parts(d, 0.5, False, 4, 4, 0.25)
    assert (s["rels"][0]["h"], s["rels"][0]["t"]) == (254, 255) and int(s["bg_sorted"].min()) == 252
    _foreground_cap_and_background_subset_are_uniform(d, (3, 4, 7, 8))


def _foreground_cap_and_background_subset_are_uniform(d, seeds):
    # 4 candidates (2 x 2), so no draws; B = 4 keeps 1 foreground row, then 3 of the 8 remaining pairs, window 6
    cfg = (0.5, False, 4, 4, 0.25)
    s = np_relsample_parts(d, *cfg)
    assert s["n_pre"] == 4 and s["num_pos"] == 1 and s["num_neg"] == 3 and s["window"] == 6 and len(s["bg_sorted"]) == 8
    fg_index = {tuple(map(int, c)): j for j, c in enumerate(s["rels"][0]["cand"])}
    win = [tuple(x) for x in s["bg_sorted"][:6].tolist()]
    N = 2000
    fg_count, bg_count, bg_first = np.zeros(4), np.zeros(6), np.zeros(6)
    for seed in seeds:
        _, labels, _, pairs, _ = _run_copies(d, cfg, seed, N // len(seeds))
        for pr, lb in zip(pairs, labels):
            pr = pr.cpu().numpy()
            assert len(pr) == 4
            fg_count[fg_index[tuple(pr[0])]] += 1
            bg = [tuple(x) for x in pr[1:].tolist()]
            for x in bg:
                bg_count[win.index(x)] += 1
            bg_first[win.index(bg[0])] += 1
    _assert_freq(fg_count, N, np.full(4, 0.25), "foreground cap")
    _assert_freq(bg_count, N, np.full(6, 0.5), "background subset")
    _assert_freq(bg_first, N, np.full(6, 1 / 6), "background order")


# ---- limits ------------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_truncations():
    g = load_golden()
    d = case_image(g, "small")
    big = dict(d)
    big["prp_boxes"] = np.tile(d["prp_boxes"], (26, 1))[:257]
    big["prp_labels"], big["pred_scores"] = np.tile(d["prp_labels"], 26)[:257], np.tile(d["pred_scores"], 26)[:257]
    with pytest.raises(native.VetoError, match="max_prp_per_image 257 outside 0..256"):
        _run(big, (0.5, False, 4, 1024, 0.25), 1)
    with pytest.raises(native.VetoError, match="batch_size_per_image 4096 outside 1..2048"):
        _run(d, (0.5, False, 4, 4096, 0.25), 1)
    with pytest.raises(native.VetoError, match="NUM_SAMPLE_PER_GT_REL"):
        _run(d, (0.5, False, 17, 1024, 0.25), 1)
    short = dict(d)
    short["relation_non_masked"] = np.zeros_like(d["relation"])
    assert np_relsample_parts(d, 0.5, False, 4, 1024, 0.25)["n_pre"] > 0
    with pytest.raises(IndexError, match="relation_non_masked"):
        _run(short, (0.5, False, 4, 1024, 0.25), 1)


def test_relation_non_masked_too_short_in_a_later_step_is_an_error():
    """17 GT boxes: 289 cells, two steps.  relation_non_masked has a nonzero entry for every relation before the first relation
    of the second step that produces triplets, and none from there on: the same IndexError as in the first step, nothing
    clamped; with one more entry that relation is served and the next one fails; with all of them nothing does."""
    cfg = (0.5, False, 4, 1024, 0.25)
    d = rc.seeded_image(21, 17, 80, 30)
    s = np_relsample_parts(d, *cfg)
    cells = rc.relation_cells(s, 17)
    live = [k for k, (c, r) in enumerate(zip(cells, s["rels"])) if r["n"] > 0]
    assert any(cells[k] < rc.STEP for k in live)
    later = [k for k in live if cells[k] >= rc.STEP]
    assert len(later) >= 2 and later[0] >= sum(c < rc.STEP for c in cells)

    def with_entries(count):
        nm = np.zeros(17 * 17, np.int64)
        nm[cells[:count]] = [r["label"] for r in s["rels"][:count]]
        return dict(d, relation_non_masked=nm.reshape(17, 17))

    for count in (later[0], later[-1]):
        with pytest.raises(IndexError, match="relation_non_masked has fewer nonzero entries"):
            _run(with_entries(count), cfg, 1)
    full = with_entries(later[-1] + 1)
    _, labels, labels_all, pairs, _ = _run(full, cfg, 1)
    corr = [k for k, r in enumerate(s["rels"]) for _ in range(r["n"])]
    np.testing.assert_array_equal(labels_all[0].cpu().numpy()[:s["n_pre"]], np_labels_all_fg(full, corr))


# ---- the relation head training on detected boxes ----------------------------------------------------------------------

SMALL_SIZES = ((6, 24, 6), (5, 18, 4))       # (GT boxes, detections, relations) per image
REAL_SIZES = ((35, 80, 60), (50, 80, 90))    # 1225 and 2500 relation cells: 5 and 10 steps, mask words 0..2


def _head_inputs(dev, n_cls=151, sizes=SMALL_SIZES):
    rng = np.random.RandomState(31)
    W, H = 800, 600
    feats = [torch.from_numpy((0.5 * rng.randn(2, 256, H >> (2 + l), W >> (2 + l))).astype(np.float32)).to(dev) for l in range(4)]
    depth = torch.from_numpy((0.5 * rng.randn(2, 256, H >> 4, W >> 4)).astype(np.float32)).to(dev)
    props, targets = [], []
    for i, (n_gt, n_det, n_rel) in enumerate(sizes):
        d = synth.synthetic_relsample_image(40 + i, n_gt, n_det, n_rel, num_obj_cls=n_cls)
        (p,), (t,) = _lists(d, with_nm=False)
        logits = torch.from_numpy(synth.normal(50 + i, "head.logits", (n_det, n_cls), 0.0, 1.0)).to(dev)
        p.add_field("predict_logits", logits)
        p.add_field("pred_labels", logits[:, 1:].argmax(1) + 1)
        props.append(p)
        targets.append(t)
    return feats, depth, props, targets


def _clone(p):
    q = BoxList(p.bbox, p.size, p.mode)
    q.extra_fields = dict(p.extra_fields)
    return q


def _sgdet_head(meet, dev):
    from veto_amd import predictor
    from veto_amd.relation_head import VETORelationHead
    predictor.set_embedding_provider(lambda names, w, k: torch.zeros(len(names), k))
    cfg = testing.make_config(2, 8, mode="sgcls", meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    cfg.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.EMB_DROPOUT = 0.0
    cfg.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.T_DROPOUT = 0.0
    cfg.VETO_AMD.DEVICE_DETECT_RELSAMPLE = True
    head = VETORelationHead(cfg, samp_processor=object())
    sd = synth.meet_state_dict(0, head.predictor.max_group_element_number_list, layers=2) if meet \
        else synth.predictor_state_dict(0, layers=2)
    head.predictor = testing.make_predictor(cfg, sd, dev)
    head.train()
    return cfg, head


@pytest.mark.parametrize("meet", [False, True])
def test_relation_head_trains_on_detected_boxes(meet):
    _relation_head_trains_on_detected_boxes(meet, SMALL_SIZES)


@pytest.mark.parametrize("meet", [False, True])
def test_relation_head_trains_on_detected_boxes_at_real_size(meet):
    """Two images of 80 detections against 35 and 50 GT boxes."""
    _relation_head_trains_on_detected_boxes(meet, REAL_SIZES)


def _relation_head_trains_on_detected_boxes(meet, sizes):
    dev = torch.device("cuda:0")
    cfg, head = _sgdet_head(meet, dev)
    feats, depth, props, targets = _head_inputs(dev, sizes=sizes)
    assert [(len(t), len(p)) for p, t in zip(props, targets)] == [s[:2] for s in sizes]
    depth.requires_grad_(True)

    def step(seed):
        for p in head.predictor.parameters():
            p.grad = None
        depth.grad = None
        torch.manual_seed(seed)
        random.seed(seed)   # the MEET expert sampling draws from Python's random, as the reference's does
        roi, out_props, losses = head(feats, [_clone(p) for p in props], targets=targets,
                                      depth_features=depth, logger=None, x=None)
        return roi, out_props, losses

    roi, out_props, losses = step(11)
    assert all(torch.isfinite(v).all() for v in losses.values())
    assert all("locating_match" in p.extra_fields for p in out_props)
    assert roi.shape == (sum(len(p) for p in props), 256, 8, 8)
    total = sum(losses.values())
    total.backward()
    grads = [p.grad for p in head.predictor.parameters() if p.grad is not None]
    assert len(grads) >= 20 and all(torch.isfinite(g).all() for g in grads)
    assert depth.grad is not None and float(depth.grad.abs().max()) > 0
    values = {k: float(v.detach()) for k, v in losses.items()}
    _, _, again = step(11)
    assert {k: float(v.detach()) for k, v in again.items()} == values
    # the head's loss is the predictor's loss on the pairs DetectRelationSampler returns for the same generator state
    from veto_amd.sampling import DetectRelationSampler
    torch.manual_seed(11)
    random.seed(11)
    fresh = [_clone(p) for p in props]
    with torch.no_grad():
        fresh, rel_labels, _, rel_pairs, _ = DetectRelationSampler.from_config(cfg).detect_relsample(fresh, targets)
    roi2, d2, _, _ = head.box_feature_extractor(feats, fresh, depth_features=depth)
    _, _, direct, _, _, _ = head.predictor(fresh, rel_pairs, rel_labels, None, roi_features=roi2, roi_depth_features=d2)
    assert {k: float(v.detach()) for k, v in direct.items()} == values
