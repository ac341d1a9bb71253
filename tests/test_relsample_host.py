"""sgdet training, host side: a numpy restatement of RelationSampling.detect_relsample (sampling.py:109-176) and
motif_rel_fg_bg_sampling (:179-309) with the randomness factored out, pinned to the reference's own outputs
(tests/golden/sgdet/relsample.npz, and relsample_large.npz at the sizes of sgdet training and at the sampler's limits of 256
proposals and 256 GT boxes); the C ABI of veto_detect_relsample; the config key and the refusal without it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relsample_cases as rc  # noqa: E402
from veto_amd import native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgdet", "relsample.npz")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "veto_amd.h")
FIELDS = ("prp_boxes", "prp_labels", "pred_scores", "tgt_boxes", "tgt_labels", "relation")


def load_golden():
    return np.load(GOLDEN)


def load_golden_large():
    return np.load(rc.GOLDEN_LARGE)


def case_names(g):
    return sorted({k.split("__")[0] for k in g.files})


def case_image(g, case):
    d = {f: g[case + "__" + f] for f in FIELDS}
    if case + "__relation_non_masked" in g.files:
        d["relation_non_masked"] = g[case + "__relation_non_masked"]
    return d


def case_config(g, case):
    """(fg_thres, require_overlap, num_sample_per_gt_rel, batch_size_per_image, positive_fraction)"""
    c = g[case + "__config"]
    return float(c[0]), bool(c[1]), int(c[2]), int(c[3]), float(c[4])


def np_iou(a, b):
    """boxlist_iou(a, b) in fp32, operation for operation (boxlist_ops.py:54-89, TO_REMOVE 1)."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    one, zero = np.float32(1), np.float32(0)
    w = np.maximum((np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])) + one, zero)
    h = np.maximum((np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])) + one, zero)
    inter = w * h
    area_a = ((a[:, 2] - a[:, 0]) + one) * ((a[:, 3] - a[:, 1]) + one)
    area_b = ((b[:, 2] - b[:, 0]) + one) * ((b[:, 3] - b[:, 1]) + one)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((area_a[:, None] + area_b[None, :]) - inter)


def np_relsample_parts(d, fg_thres, require_overlap, per_rel, batch, positive_fraction):
    """Every deterministic quantity of one image: the IoUs, matches, locating_match, the candidates before and after the
    foreground removal, binary_rel, the GT relations with their candidate lists (and draw weights), the foreground count
    before the cap, the budgets and the background candidates in the window's (quality desc, row-major asc) order."""
    pb, pl, q = d["prp_boxes"], d["prp_labels"].astype(np.int64), d["pred_scores"].astype(np.float32)
    tb, tl, rel = d["tgt_boxes"], d["tgt_labels"].astype(np.int64), d["relation"]
    P, thr = len(pb), np.float32(fg_thres)
    ious = np_iou(tb, pb)
    over = ious > thr
    is_match = (tl[:, None] == pl[None, :]) & over
    locating = over.any(0).astype(np.float32)
    if require_overlap:
        self_iou = np_iou(pb, pb)
        poss = (self_iou > 0) & (self_iou < 1)
    else:
        poss = ~np.eye(P, dtype=bool)
    poss[pl == 0] = False
    poss[:, pl == 0] = False
    poss0 = poss.copy()
    binary = np.zeros((P, P), np.int64)
    rels = []
    for h, t in zip(*np.nonzero(rel)):
        H, T = np.nonzero(is_match[h])[0], np.nonzero(is_match[t])[0]
        if len(H) and len(T):
            binary[np.ix_(H, T)] = 1
            binary[np.ix_(T, H)] = 1
        cand = [(a, b) for a in H for b in T if a != b]
        for a, b in cand:
            poss[a, b] = False
        w = np.array([ious[h, a] * ious[t, b] for a, b in cand], np.float32)
        rels.append(dict(h=int(h), t=int(t), label=int(rel[h, t]), cand=cand, weight=w, n=min(len(cand), per_rel)))
    n_pre = sum(r["n"] for r in rels)
    num_pos = int(batch * positive_fraction)
    n_fg = min(n_pre, num_pos)
    bg = np.argwhere(poss)
    quality = q[bg[:, 0]] * q[bg[:, 1]]
    order = np.lexsort((np.arange(len(bg)), -quality.astype(np.float64)))   # quality desc, row-major asc
    num_neg = min(batch - n_fg, len(bg))
    return dict(ious=ious, is_match=is_match, locating=locating, poss0=poss0, poss=poss, binary=binary, rels=rels,
                n_pre=n_pre, num_pos=num_pos, n_fg=n_fg, bg_sorted=bg[order], bg_quality=quality[order], num_neg=num_neg,
                window=min(int(num_neg * 2.0), len(bg)))


def np_relsample(d, cfg, rng):
    """The whole sampler with the draws taken from `rng` (a numpy Generator): (pairs [n, 2], labels [n],
    labels_all or None).  The reference's distribution, not its draws."""
    fg_thres, overlap, per_rel, batch, frac = cfg
    s = np_relsample_parts(d, fg_thres, overlap, per_rel, batch, frac)
    fg, corr = [], []
    for i, r in enumerate(s["rels"]):
        cand = r["cand"]
        if len(cand) > per_rel:
            p = r["weight"].astype(np.float64)
            cand = [cand[j] for j in rng.choice(len(cand), size=per_rel, replace=False, p=p / p.sum())]
        fg += [(a, b, r["label"]) for a, b in cand]
        corr += [i] * len(cand)
    fg = np.array(fg, np.int64).reshape(-1, 3)
    if len(fg) > s["num_pos"]:
        fg = fg[rng.permutation(len(fg))[:s["num_pos"]]]
    win = s["bg_sorted"][:s["window"]]
    bg = win[rng.permutation(len(win))[:s["num_neg"]]]
    bg = np.concatenate([bg, np.zeros((len(bg), 1), np.int64)], 1)
    if len(fg) == 0 and len(bg) == 0:
        bg = np.zeros((2, 3), np.int64)
    out = np.concatenate([fg, bg], 0)
    labels_all = None
    if "relation_non_masked" in d:
        labels_all = np.concatenate([np_labels_all_fg(d, corr), np.zeros(len(bg), np.int64)])
    return out[:, :2], out[:, 2], labels_all


def np_labels_all_fg(d, corr):
    """sampling.py:160-167: nonzero(relation_non_masked) indexed by the relation index of every pre-cap triplet."""
    nm = d["relation_non_masked"]
    idx = np.argwhere(nm != 0)
    return np.array([nm[tuple(idx[i])] for i in corr], np.int64)


def rows_multiset(pairs, labels):
    return sorted(map(tuple, np.concatenate([pairs.reshape(-1, 2), labels.reshape(-1, 1)], 1).tolist()))


def deterministic(s, per_rel):
    """True when the output is fixed up to its order: no relation draws, no foreground cap, the window is all of it."""
    return all(len(r["cand"]) <= per_rel for r in s["rels"]) and s["n_pre"] <= s["num_pos"] and \
        s["num_neg"] == len(s["bg_sorted"])


# ---- the restatement against the reference -------------------------------------------------------------------------

def test_fixture_covers_the_cases_the_sampler_must_handle():
    g = load_golden()
    seen = set()
    for case in case_names(g):
        cfg = case_config(g, case)
        s = np_relsample_parts(case_image(g, case), *cfg)
        if any(len(r["cand"]) > cfg[2] for r in s["rels"]):
            seen.add("draws")
        if (s["is_match"].sum(0) >= 2).any():
            seen.add("two_gt")
        if s["n_pre"] > s["num_pos"]:
            seen.add("cap")
        if deterministic(s, cfg[2]) and s["num_neg"] > 0:
            seen.add("deterministic")
        if len(g[case + "__pairs"]) == 2 and s["n_fg"] == 0 and s["num_neg"] == 0:
            seen.add("degenerate")
        seen.add("overlap" if cfg[1] else "no_overlap")
        seen.add("non_masked" if case + "__relation_non_masked" in g.files else "masked_only")
    assert seen == {"draws", "two_gt", "cap", "deterministic", "degenerate", "overlap", "no_overlap", "non_masked",
                    "masked_only"}


@pytest.mark.parametrize("case", case_names(load_golden()))
def test_restatement_matches_the_reference_deterministic_quantities(case):
    _restatement_matches_the_reference(load_golden(), case)


def _restatement_matches_the_reference(g, case):
    d, cfg = case_image(g, case), case_config(g, case)
    s = np_relsample_parts(d, *cfg)
    np.testing.assert_array_equal(s["ious"], g[case + "__ious"])
    np.testing.assert_array_equal(s["locating"], g[case + "__locating_match"])
    np.testing.assert_array_equal(s["binary"], g[case + "__binary_rel"])
    np.testing.assert_array_equal(s["poss"], g[case + "__rel_possibility"] != 0)
    pairs, labels = g[case + "__pairs"], g[case + "__labels"]
    n_fg = s["n_fg"]
    assert len(pairs) == (2 if n_fg == 0 and s["num_neg"] == 0 else n_fg + s["num_neg"])
    assert (labels[:n_fg] > 0).all() and (labels[n_fg:] == 0).all()
    # every foreground triplet is a candidate of a relation with its label, at most per_rel per relation
    cand = {}
    for r in s["rels"]:
        for c in r["cand"]:
            cand.setdefault((c[0], c[1], r["label"]), 0)
            cand[(c[0], c[1], r["label"])] += 1
    for row in rows_multiset(pairs[:n_fg], labels[:n_fg]):
        assert row in cand, row
    # the background lies in the window, without duplicates; its quality multiset is the window's when it is all of it.
    # The reference's torch.sort (:290) is not stable, so where the window's edge falls inside a run of equal qualities its
    # window holds everything above the run and any window - above members of the run (the restatement, like the kernel, takes
    # the first of them in row-major order); without such a run this is the restatement's window exactly.
    w, bq = s["window"], s["bg_quality"]
    q = d["pred_scores"].astype(np.float32)
    bg = [tuple(p) for p in pairs[n_fg:].tolist()] if s["num_neg"] else []
    if 0 < w < len(bq) and bq[w] == bq[w - 1]:
        above = int((bq > bq[w - 1]).sum())
        win = {tuple(p) for p in s["bg_sorted"][bq >= bq[w - 1]].tolist()}
        assert sum(q[a] * q[b] == bq[w - 1] for a, b in bg) <= w - above
    else:
        win = {tuple(p) for p in s["bg_sorted"][:w].tolist()}
    assert len(set(bg)) == len(bg) and set(bg) <= win
    if s["num_neg"] == s["window"]:
        got = sorted(q[[b[0] for b in bg]] * q[[b[1] for b in bg]])
        np.testing.assert_array_equal(got, sorted(s["bg_quality"][:s["window"]]))
    if "relation_non_masked" in d:
        all_ = g[case + "__labels_all"]
        assert len(all_) == s["n_pre"] + len(pairs) - n_fg
        corr = [i for i, r in enumerate(s["rels"]) for _ in range(r["n"])]
        np.testing.assert_array_equal(all_[:s["n_pre"]], np_labels_all_fg(d, corr))
        assert (all_[s["n_pre"]:] == 0).all()
    if deterministic(s, cfg[2]):
        want_p, want_l, _ = np_relsample(d, cfg, np.random.default_rng(0))
        assert rows_multiset(pairs, labels) == rows_multiset(want_p, want_l)


def test_restatement_draws_respect_the_budgets():
    _restatement_draws_respect_the_budgets(load_golden())


def _restatement_draws_respect_the_budgets(g):
    rng = np.random.default_rng(5)
    for case in case_names(g):
        d, cfg = case_image(g, case), case_config(g, case)
        s = np_relsample_parts(d, *cfg)
        pairs, labels, all_ = np_relsample(d, cfg, rng)
        assert len(pairs) == len(g[case + "__pairs"])
        assert (labels > 0).sum() == s["n_fg"]
        if all_ is not None:
            assert len(all_) == len(g[case + "__labels_all"])


# ---- the same at the sizes of sgdet training and at the limits: 256 proposals, 256 GT boxes, all eight mask words -----------------

def test_large_fixture_holds_the_cases_of_the_case_table():
    g = load_golden_large()
    assert case_names(g) == sorted(rc.LARGE_CASES)
    for case in case_names(g):
        d, cfg, non_masked = rc.large_case_inputs(case)
        assert case_config(g, case) == cfg
        assert (case + "__relation_non_masked" in g.files) == non_masked
        for k, v in case_image(g, case).items():
            assert v.dtype == d[k].dtype and np.array_equal(v, d[k]), (case, k)
    assert os.path.getsize(rc.GOLDEN_LARGE) <= 1 << 20
    sizes = {c: (len(g[c + "__prp_boxes"]), len(g[c + "__tgt_boxes"])) for c in case_names(g)}
    assert sizes == {"real": (80, 17), "word_edge": (65, 33), "limit": (256, 60), "limit_overlap": (256, 256),
                     "over_sort_buffer": (256, 40), "padded_deterministic": (256, 256), "ties": (80, 17)}
    assert case_config(g, "real") == (0.5, False, 4, 1024, 0.25)
    assert case_config(g, "word_edge")[3] == 64 and case_config(g, "limit_overlap") == (0.5, True, 16, 2048, 0.25)
    assert case_config(g, "over_sort_buffer")[2:4] == (16, 2048) and case_config(g, "padded_deterministic")[2:4] == (4, 2048)
    assert int(np.count_nonzero(g["limit__relation"])) == 150
    assert len(np.unique(g["ties__pred_scores"])) == 4


def test_large_fixture_covers_what_the_small_sizes_cannot_reach():
    g = load_golden_large()
    parts = {}
    for case in case_names(g):
        cfg = case_config(g, case)
        parts[case] = (case_image(g, case), cfg, np_relsample_parts(case_image(g, case), *cfg))
    words, seen = set(), set()
    for case, (d, cfg, s) in parts.items():
        P, T, per_rel = len(d["prp_boxes"]), len(d["tgt_boxes"]), cfg[2]
        words |= set(rc.match_words(s))
        cells = rc.relation_cells(s, T)
        live = [(c, r) for c, r in zip(cells, s["rels"]) if r["cand"]]     # relations that produce triplets
        for lo in (256, 32768, 65280):
            if any(c >= lo for c, _ in live):
                seen.add("cell>=%d" % lo)
        if len({c // rc.STEP for c, _ in live}) >= 3:
            seen.add("three_steps")
            if any(c >= rc.STEP and len(r["cand"]) > per_rel for c, r in live):
                seen.add("draws_in_a_later_step")
        if s["n_pre"] > rc.SORT_BUFFER and cfg[3] == 2048 and s["n_pre"] > s["num_pos"]:
            seen.add("F>2048")
        if s["n_pre"] > s["num_pos"] and s["window"] < len(s["bg_sorted"]) and P == 256:
            seen.add("cap_and_window_at_256")
        taken, left = rc.window_tie_run(s)
        if len(taken) and len(left):
            run = np.concatenate([taken, left])
            # the run of equal qualities around the window's edge spans proposal rows and 32-column mask words, and so do the
            # part inside the window and the part outside it
            if min(len({int(x[0]) for x in part}) for part in (taken, left)) >= 3 and \
                    min(len({int(x[1]) // 32 for x in part}) for part in (taken, left)) >= 2 and len(run) > 64:
                seen.add("tie_run_across_words")
        if P == 256 and T >= 17 and deterministic(s, per_rel) and s["num_neg"] > 0 and s["n_fg"] > 0:
            seen.add("deterministic_at_256")
    assert words == set(range(8)), words
    assert seen == {"cell>=256", "cell>=32768", "cell>=65280", "three_steps", "draws_in_a_later_step", "F>2048",
                    "cap_and_window_at_256", "tie_run_across_words", "deterministic_at_256"}, seen
    # the cases the table names have the properties it names them for
    d, cfg, s = parts["padded_deterministic"]
    assert deterministic(s, cfg[2]) and s["num_neg"] == len(s["bg_sorted"]) > 0
    assert rc.match_words(s) == [6, 7] and not s["is_match"][:, :216].any() and (d["prp_labels"][:216] == 0).all()
    assert not d["relation"][:236].any() and not d["relation"][:, :236].any()
    assert max(rc.relation_cells(s, 256)) >= 65280
    d, cfg, s = parts["real"]
    assert rc.steps_of(17) == 2 and {c // rc.STEP for c in rc.relation_cells(s, 17)} == {0, 1}
    d, cfg, s = parts["word_edge"]
    assert s["n_pre"] > s["num_pos"] and 2 in rc.match_words(s)
    d, cfg, s = parts["limit"]
    assert s["n_pre"] > s["num_pos"] and s["window"] < len(s["bg_sorted"])
    d, cfg, s = parts["over_sort_buffer"]
    assert s["n_pre"] > rc.SORT_BUFFER
    d, cfg, s = parts["ties"]
    assert len(d["prp_boxes"]) > 64 and len(rc.window_tie_run(s)[0]) > 0


@pytest.mark.parametrize("case", sorted(rc.LARGE_CASES))
def test_restatement_matches_the_reference_at_real_and_limit_sizes(case):
    _restatement_matches_the_reference(load_golden_large(), case)


def test_restatement_draws_respect_the_budgets_at_real_and_limit_sizes():
    _restatement_draws_respect_the_budgets(load_golden_large())


def test_front_padding_moves_an_image_without_changing_it():
    d = rc.seeded_image(26, 20, 40, 30, dict(max_copies=2))
    cfg = (0.5, False, 4, 2048, 0.25)
    s, big = np_relsample_parts(d, *cfg), np_relsample_parts(rc.pad_front(d, 256, 256), *cfg)
    assert [(r["h"] + 236, r["t"] + 236, r["label"], [(a + 216, b + 216) for a, b in r["cand"]]) for r in s["rels"]] == \
        [(r["h"], r["t"], r["label"], [tuple(map(int, c)) for c in r["cand"]]) for r in big["rels"]]
    np.testing.assert_array_equal(big["bg_sorted"], s["bg_sorted"] + 216)
    np.testing.assert_array_equal(big["binary"][216:, 216:], s["binary"])
    assert not big["binary"][:216].any() and not big["binary"][:, :216].any() and not big["poss0"][:216].any()
    assert not big["locating"][:216].any()
    assert (big["n_pre"], big["n_fg"], big["num_neg"], big["window"]) == (s["n_pre"], s["n_fg"], s["num_neg"], s["window"])


def test_sweep_covers_every_edge_size_and_setting():
    seen_p, seen_t, per_rel, batch, overlap, edge_t = set(), set(), set(), set(), set(), {}
    for name in rc.SWEEPS:
        cfg, images = rc.sweep_images(name)
        per_rel.add(cfg[2])
        batch.add(cfg[3])
        overlap.add(cfg[1])
        for d in images:
            P, T = len(d["prp_boxes"]), len(d["tgt_boxes"])
            assert "relation_non_masked" in d and np_relsample_parts(d, *cfg)["n_pre"] > 0
            seen_p.add(P)
            seen_t.add(T)
            edge_t[P] = max(edge_t.get(P, 0), T)
    assert seen_p == {31, 32, 33, 63, 64, 65, 255, 256} and seen_t == {15, 16, 17, 32, 33, 256}
    assert per_rel == {1, 4, 16} and batch == {2, 64, 2048} and overlap == {False, True}
    assert all(edge_t[P] > 16 for P in (64, 65, 255, 256))


# ---- C ABI, config and the refusal without the key -----------------------------------------------------------------

def test_abi_declares_detect_relsample():
    text = open(HEADER).read()
    for name in ("veto_detect_relsample_args_t", "veto_detect_relsample_workspace_bytes", "veto_detect_relsample"):
        assert re.search(r"\b%s\b" % name, text), name
    assert "veto_detect_relsample" in native.EXPORTS and "veto_detect_relsample_workspace_bytes" in native.EXPORTS
    # 11 int32 + fg_thres + seed (u64) + 17 pointers
    assert ctypes.sizeof(native.VetoDetectRelsampleArgs) == 12 * 4 + 8 + 17 * 8


def _args(**kw):
    a = native.VetoDetectRelsampleArgs()
    a.struct_size = ctypes.sizeof(native.VetoDetectRelsampleArgs)
    a.n_img, a.n_prp, a.n_tgt, a.n_rel_cells = 1, 10, 4, 16
    a.max_prp_per_image, a.max_tgt_per_image = 10, 4
    a.num_sample_per_gt_rel, a.batch_size_per_image, a.max_fg_per_image = 4, 1024, 256
    a.fg_thres = 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("field,value,word", [
    ("max_prp_per_image", 257, b"max_prp_per_image 257 outside 0..256"),
    ("max_tgt_per_image", 300, b"max_tgt_per_image 300 outside 0..256"),
    ("batch_size_per_image", 4096, b"batch_size_per_image 4096 outside 1..2048"),
    ("num_sample_per_gt_rel", 17, b"NUM_SAMPLE_PER_GT_REL"),
    ("max_fg_per_image", 2000, b"max_fg_per_image"),
])
def test_abi_rejects_out_of_range_sizes_without_a_gpu(field, value, word):
    lib = native.load_library()
    a = _args(**{field: value})
    assert lib.veto_detect_relsample(None, ctypes.byref(a), ctypes.c_void_p(256), 1 << 20) == -1   # VETO_ERR_INVALID
    assert word in lib.veto_last_error()


def test_abi_checks_struct_size_and_workspace():
    lib = native.load_library()
    a = _args(struct_size=8)
    assert lib.veto_detect_relsample(None, ctypes.byref(a), None, 0) < 0
    assert b"size mismatch" in lib.veto_last_error()
    assert lib.veto_detect_relsample_workspace_bytes(16, 4) >= 16 * 8 + 16 * 4 * 4


def test_config_default_keeps_sgdet_training_off():
    from veto_amd.config import default_config
    assert default_config().VETO_AMD.DEVICE_DETECT_RELSAMPLE is False


def _sgdet_cfg(meet=False):
    from veto_amd import testing
    cfg = testing.make_config(2, 8, mode="sgcls", meet=meet)
    cfg.MODEL.ROI_RELATION_HEAD.USE_GT_BOX = False
    return cfg


def test_sgdet_training_is_refused_without_the_key_before_any_device_check():
    from veto_amd import predictor
    from veto_amd.relation_head import VETORelationHead
    predictor.set_embedding_provider(lambda names, d, k: torch.zeros(len(names), k))
    head = VETORelationHead(_sgdet_cfg())
    head.train()
    with pytest.raises(NotImplementedError, match="detect_relsample.*DEVICE_DETECT_RELSAMPLE"):
        head.forward([torch.zeros(1, 256, 8, 8)], [], depth_features=torch.zeros(1, 256, 4, 4), targets=[])


def test_sampler_reads_its_config_and_refuses_the_cpu():
    from veto_amd.config import default_config
    from veto_amd.sampling import DetectRelationSampler
    from veto_amd.structures import BoxList
    cfg = default_config()
    cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD = 0.6
    cfg.MODEL.ROI_RELATION_HEAD.REQUIRE_BOX_OVERLAP = True
    s = DetectRelationSampler.from_config(cfg)
    assert (s.fg_thres, s.require_overlap, s.num_sample_per_gt_rel, s.batch_size_per_image, s.num_pos_per_img) == \
        (0.6, True, 4, 1024, 256)
    p = BoxList(torch.zeros(2, 4), (10, 10))
    with pytest.raises(RuntimeError, match="HIP device"):
        s.detect_relsample([p], [p])
