"""Premises of the constructed inputs of tests/test_post_eval_scale_gpu.py, checked against the oracles alone (no GPU): a
fixture that no longer has the sizes, ties, gaps or candidate counts the GPU tests rely on fails here first."""
import numpy as np
import pytest

import post_eval_cases as pc
from oracle import sgg_eval_oracle as so


# ---- post-processor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,n2", [("vg36", 6300, 8192), ("gqa_limit", 16384, 16384), ("capped_ties", 10240, 16384)])
def test_meet_cases_have_the_stated_sizes_and_recoverable_source_rows(name, rows, n2):
    c, ref = pc.meet_case(name), pc.meet_reference(name)
    assert len(c["rel"]) * len(c["pairs"]) == rows and 1 << int(np.ceil(np.log2(rows))) == n2
    # no softmax probability is exactly zero: the group of every row can be read off its probability row
    src = pc.source_rows(ref["rel_pair_idxs"], ref["pred_rel_scores"], c["pairs"], c["incre"])
    assert np.array_equal(np.sort(src), np.arange(rows))
    assert ref["rel_pair_idxs"].dtype == np.float32 and (np.diff(ref["triple_scores"]) <= 0).all()


def test_meet_limit_case_is_the_limit_and_has_a_wide_head():
    c = pc.meet_case("gqa_limit")
    assert len(c["rel"]) * len(c["pairs"]) == pc.MAX_ROWS and c["rel"]["group_3"].shape[1] == 67 and len(c["incre"]) == 101
    over = pc.meet_case("gqa_over")
    assert len(over["rel"]) * len(over["pairs"]) == pc.MAX_ROWS + 4 and len(over["pairs"]) == len(c["pairs"]) + 1


def test_real_size_meet_scores_are_too_close_for_a_position_wise_comparison():
    """Why the comparison is per source row: hundreds of neighbouring oracle scores lie within the tolerance."""
    ts = pc.meet_reference("vg36")["triple_scores"].astype(np.float64)
    assert (np.abs(np.diff(ts)) <= pc.SCORE_TOL).sum() > 300


def test_capped_tie_cases_are_decided_by_the_tie_break_alone():
    c, ref = pc.meet_case("capped_ties"), pc.meet_reference("capped_ties")
    assert (ref["pred_scores"] == 1.0).all()                               # one-hot objects
    n, gap = pc.distinct_score_gaps(ref["triple_scores"])
    assert n == 5 * pc.TIE_PERIOD == 320 and gap > pc.TIE_GAP, (n, gap)
    _, counts = np.unique(ref["triple_scores"], return_counts=True)
    assert counts.min() == 2048 // pc.TIE_PERIOD                            # every score is shared by 32 rows
    # ... and the oracle's order inside a tie is the source order (stable sort)
    src = pc.source_rows(ref["rel_pair_idxs"], ref["pred_rel_scores"], c["pairs"], c["incre"])
    tie = ref["triple_scores"][1:] == ref["triple_scores"][:-1]
    assert tie.sum() == 10240 - 320 and (src[1:][tie] > src[:-1][tie]).all()
    cv, rv = pc.vote_case("capped_ties_C"), pc.vote_reference("capped_ties_C")
    assert pc.expert_top_two_gaps(cv).min() >= pc.ARGMAX_GAP
    n, gap = pc.distinct_score_gaps(rv["triple_scores"])
    kept = len(rv["triple_scores"])
    assert 0 < kept < 10240 and kept % 32 == 0 and n == kept // 32 and gap > pc.TIE_GAP, (kept, n, gap)


@pytest.mark.parametrize("voting", ["C", "U"])
def test_random_vote_cases_keep_a_proper_subset_with_clear_arg_maxes(voting):
    c, ref = pc.vote_case("vg36_" + voting), pc.vote_reference("vg36_" + voting)
    # the premise under which the device's kept set must equal the oracle's exactly: no expert's arg-max hangs on rounding
    assert pc.expert_top_two_gaps(c).min() >= pc.ARGMAX_GAP
    kept = len(ref["triple_scores"])
    assert 0.05 * 6300 < kept < 0.95 * 6300
    src = pc.source_rows(ref["rel_pair_idxs"], ref["pred_rel_scores"], c["pairs"], c["incre"])
    assert len(np.unique(src)) == kept


def test_vote_extremes_keep_nothing_and_everything():
    none = pc.vote_reference("none_U")
    assert none["triple_scores"].shape == (0,) and none["pred_rel_scores"].shape == (0, 51) and none["rel_pair_idxs"].shape == (0, 2)
    assert pc.expert_top_two_gaps(pc.vote_case("none_U")).min() >= pc.ARGMAX_GAP
    full = pc.vote_reference("all_U")
    assert len(full["triple_scores"]) == 6300


def test_vanilla_batch_has_the_stated_shapes():
    c = pc.vanilla_case("random")
    assert [len(p) for p in c["pairs"]] == [0, 1, 1260, 0, 2, 16384, 90] and c["num_objs"] == [1, 2, 36, 1, 2, 129, 10]
    assert all(p.max() < n for p, n in zip(c["pairs"], c["num_objs"]) if len(p))
    assert [len(p) for p in pc.vanilla_case("over")["pairs"]] == [16385]
    ref = pc.vanilla_reference("random")
    assert [len(r["triple_scores"]) for r in ref] == [0, 1, 1260, 0, 2, 16384, 90]
    ties = pc.vanilla_reference("ties")
    for r, cnt in zip(ties, pc.VANILLA_PAIR_COUNTS):
        assert (r["pred_scores"] == 1.0).all()
        n, gap = pc.distinct_score_gaps(r["triple_scores"])
        assert n == min(cnt, pc.TIE_PERIOD) and gap > pc.TIE_GAP, (cnt, n, gap)


def test_compare_rows_catches_a_misplaced_and_a_corrupted_row():
    """The comparison itself: a swap across a clear score gap, a wrong tie order and a changed probability are each refused."""
    c, ref = pc.meet_case("capped_ties"), pc.meet_reference("capped_ties")
    args = (c["pairs"], c["incre"])
    assert pc.compare_rows(ref, ref, *args, expect_all=10240, exact_order=True)["moved"] == 0
    def swapped(i, k):
        out = {key: v.copy() for key, v in ref.items()}
        for key in ("rel_pair_idxs", "pred_rel_scores", "pred_rel_labels", "triple_scores"):
            out[key][[i, k]] = out[key][[k, i]]
        return out
    with pytest.raises(AssertionError, match="non-increasing"):
        pc.compare_rows(swapped(0, 10239), ref, *args)
    with pytest.raises(AssertionError, match="source order"):
        pc.compare_rows(swapped(0, 1), ref, *args)                      # rows 0 and 1 tie: only the tie-break tells them apart
    bad = {key: v.copy() for key, v in ref.items()}
    bad["pred_rel_scores"][5000, 0] += 1e-5
    with pytest.raises(AssertionError, match="prob_err"):
        pc.compare_rows(bad, ref, *args)
    bad = {key: v.copy() for key, v in ref.items()}
    bad["rel_pair_idxs"][7] = bad["rel_pair_idxs"][8]
    bad["pred_rel_scores"][7] = bad["pred_rel_scores"][8]
    with pytest.raises(AssertionError):                                  # a row twice, another one missing
        pc.compare_rows(bad, ref, *args)


# ---- evaluator --------------------------------------------------------------------------------------------------------------
def _evaluated(res):
    return [r for r in res["per_image"] if r is not None]


@pytest.mark.parametrize("mode", ["predcls", "sgcls", "sgdet"])
def test_eval_101_classes_reach_the_second_trip_of_the_row_loops(mode):
    images, zs, _, C = pc.eval_case("c101_" + mode)
    ref = pc.eval_reference("c101_" + mode)
    assert C == 101 and all(im["rel_scores"].shape[1] == 101 for im in images)
    ev = _evaluated(ref)
    assert len(ev) >= 4
    assert max(r["ng_cols"].max() for r in ev) > 64 and max(r["gt_pred"].max() for r in ev) > 64
    # matches whose predicate lies past column 64, in both lists
    assert any(((r["gt_pred"] > 64) & (r["gc_rank"] < so.NO_MATCH)).any() for r in ev)
    assert any(((r["gt_pred"] > 64) & (r["ng_rank"] < so.NO_MATCH)).any() for r in ev)
    assert 0.0 < ref["recall"][100] < 1.0 or mode == "sgdet"
    if mode == "sgdet":
        assert any(len(im["pred_classes"]) != len(im["gt_classes"]) for im in images)


@pytest.mark.parametrize("name,cells", [("small_c51", [50, 100, 150]), ("small_c101", [100, 200])])
def test_eval_small_lists_sit_on_and_around_the_100_cell_branch(name, cells):
    images, zs, mode, C = pc.eval_case(name)
    assert [len(im["pred_rel_inds"]) * (C - 1) for im in images] == cells
    ev = _evaluated(pc.eval_reference(name))
    assert len(ev) == len(cells) and [len(r["ng_rows"]) for r in ev] == [min(c, 100) for c in cells]
    assert any((r["ng_rank"] < so.NO_MATCH).any() for r in ev)           # not vacuous: something matches


@pytest.mark.parametrize("C", [51, 101])
def test_eval_row_switch_case_has_99_100_101_rows(C):
    images, zs, mode, C2 = pc.eval_case("rows_c%d" % C)
    assert C2 == C and [len(im["pred_rel_inds"]) for im in images] == [99, 100, 101]
    ev = _evaluated(pc.eval_reference("rows_c%d" % C))
    assert len(ev) == 3 and all((r["gc_rank"] < so.NO_MATCH).any() for r in ev)


@pytest.mark.parametrize("N", pc.HALF_CELLS)
def test_eval_candidate_switch_case_has_exactly_n_cells_above_the_bound(N):
    images, zs, mode, C = pc.eval_case("half_%d" % N)
    s = images[0]["rel_scores"]
    assert s.shape == (120, 51) and mode == "predcls"                       # predcls: object scores 1.0
    half = s[:, 1:] == 0.5
    assert half.sum() == N and (half.any(1)).sum() >= 100 and (s[:, 0] < 0.4).all()
    rest = s[:, 1:][~half]
    assert rest.max() < 0.4 and len(np.unique(rest)) == len(rest)
    # the 100-th largest row maximum is 0.5, so exactly the N cells lie at or above the pruned path's bound
    assert np.sort(s[:, 1:].max(1))[::-1][99] == 0.5
    r = _evaluated(pc.eval_reference("half_%d" % N))[0]
    flat = np.nonzero(half.ravel())[0][:100]                                 # the first 100 of those cells by flat index
    assert np.array_equal(r["ng_rows"], flat // 50) and np.array_equal(r["ng_cols"], flat % 50 + 1)
