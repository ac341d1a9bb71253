"""CPU side of tests/test_prelude_gpu.py: the premises of its cases (tests/prelude_cases.py) and the power of its bounds.  A case
that does not contain what it is named for, or a bound so wide that a wrong formula fits under it, would let the GPU tests pass
without checking anything."""
import numpy as np
import pytest
import torch

import prelude_cases as pc
from oracle import veto_oracle as vo

TOKEN_CASES = pc.token_cases()
PAIR_INDEX_CASES = pc.pair_index_cases()
BN_CASES = pc.bn_cases()


def _sd(case, layers=1):
    return pc.state_dict(layers, case["num_obj_cls"], 51, case["var0"])


# ---- the restatement the bounds are built on is the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TOKEN_CASES))
def test_restatement_equals_the_oracle(name):
    """The per-object form (prelude_cases.restate) and the reference formulation (oracle/veto_oracle.py), both float64: equal up to
    float64 rounding on every token kind but 0, where restate holds the float32 sum the kernel must produce bit for bit."""
    case = TOKEN_CASES[name]
    sd = _sd(case)
    tok, bound, subj, obj = pc.restate(sd, case)
    ref, s2, o2 = pc.oracle_tokens(sd, case)
    assert np.array_equal(subj, s2) and np.array_equal(obj, o2)
    scale = np.abs(ref[:, 1:]).max(axis=2, keepdims=True)
    assert (np.abs(tok[:, 1:] - ref[:, 1:]) <= 1e-12 * scale).all()
    assert (np.abs(tok[:, 0] - ref[:, 0]) <= pc.U * np.abs(ref[:, 0])).all()
    assert np.isfinite(bound).all() and (bound[:, 1:] > 0).all() and (bound[:, 0] == 0).all()
    # the bound is a float32 bound: the float32 oracle, which rounds the same chain in another order, is inside it
    f32, _, _ = pc.oracle_tokens(sd, case, dtype=torch.float32)
    assert pc.worst_ratio(f32[:, 1:], ref[:, 1:], bound[:, 1:]) <= 1.0


def test_partial_oracle_rows_equal_the_full_ones():
    case = TOKEN_CASES["sgcls_151"]
    sd = _sd(case)
    full, _, _ = pc.oracle_tokens(sd, case)
    part, _, _ = pc.oracle_tokens(sd, case, patch=False)
    assert np.isnan(part[:, 1:17]).all()
    for t in (17, 18):
        assert np.array_equal(full[:, t], part[:, t])
    assert np.abs(full[:, 0] - part[:, 0]).max() == 0


# ---- premises: pair indices ---------------------------------------------------------------------------------------------------------------
def test_pair_index_cases_contain_what_they_are_named_for():
    assert sorted(len(c["num_objs"]) for n, c in PAIR_INDEX_CASES.items() if n.startswith("images_")) == [1, 2, 3, 64, 65, 257]
    for name, c in PAIR_INDEX_CASES.items():
        assert sum(c["num_objs"]) <= 560 and pc.n_pair(c) <= 4000, name
        subj, obj = pc.reference_indices(c)
        s2, o2 = vo.build_pair_indices(c["pairs"], c["num_objs"])
        assert np.array_equal(subj, s2) and np.array_equal(obj, o2)
        assert subj.max() < sum(c["num_objs"]) and obj.max() < sum(c["num_objs"]) and min(subj.min(), obj.min()) >= 0
        for pairs, n in zip(c["pairs"], c["num_objs"]):
            assert len(pairs) == 0 or (pairs.min() >= 0 and pairs.max() < n)
    zero = lambda name: [i for i, p in enumerate(PAIR_INDEX_CASES[name]["pairs"]) if len(p) == 0]      # noqa: E731
    assert zero("zero_pairs_front") == [0]
    assert zero("zero_pairs_middle") == [3] and len(PAIR_INDEX_CASES["zero_pairs_middle"]["pairs"]) == 6
    assert zero("zero_pairs_twice") == [2, 3]
    assert zero("zero_pairs_end") == [4] and len(PAIR_INDEX_CASES["zero_pairs_end"]["pairs"]) == 5
    assert zero("zero_pairs_front_twice_end") == [0, 1, 30, 31, 32, 65] and len(PAIR_INDEX_CASES["zero_pairs_front_twice_end"]["pairs"]) == 66
    for name in PAIR_INDEX_CASES:
        if name.startswith("images_"):
            assert zero(name) == []
    big = PAIR_INDEX_CASES["images_257"]
    placeholders = [i for i, (p, n) in enumerate(zip(big["pairs"], big["num_objs"])) if n == 1 and len(p) == 1 and not p.any()]
    assert placeholders and placeholders[0] == 0
    allp = [p for p in big["pairs"] if len(p) >= 3]
    assert any((p[:, 0] == p[:, 1]).any() for p in allp), "no self-pair"
    assert any(len(np.unique(p, axis=0)) < len(p) for p in allp), "no repeated pair"
    # an image without pairs repeats its offset: the binary search of pair_indices_kernel meets equal neighbours
    off = np.concatenate([[0], np.cumsum([len(p) for p in PAIR_INDEX_CASES["zero_pairs_twice"]["pairs"]])])
    assert off[2] == off[3] == off[4]


# ---- premises: token rows -----------------------------------------------------------------------------------------------------------------
def test_pair_counts_straddle_the_grid_roundings():
    """assemble_kernel: 16 token rows per workgroup, the launcher rounds the workgroup count up to a multiple of 8 (the XCDs)."""
    blocks = {n: (19 * n + 15) // 16 for n in pc.GRID_PAIR_COUNTS}
    grid = {n: (b + 7) // 8 * 8 for n, b in blocks.items()}
    assert blocks == {1: 2, 6: 8, 7: 9, 27: 33, 28: 34}
    assert grid == {1: 8, 6: 8, 7: 16, 27: 40, 28: 40}
    assert blocks[6] == grid[6] and blocks[7] == grid[6] + 1              # 6 fills the eight workgroups, 7 needs a ninth
    assert 19 * 27 == 32 * 16 + 1                                         # one row into the workgroup behind a multiple of 8
    assert grid[1] - blocks[1] == 6                                       # six of eight workgroups have no row at all
    for n in pc.GRID_PAIR_COUNTS + (36,):
        assert pc.n_pair(TOKEN_CASES["pairs_%d" % n]) == n
    # chunks: 6 = 5 + 1, 36 = 7 x 5 + 1 = 5 x 7 + 1 end on one pair; image 0 of pairs_36 has 12 pairs, so both chunkings split it
    assert 6 % 5 == 1 and 36 % 5 == 1 and 36 % 7 == 1
    assert [len(p) for p in TOKEN_CASES["pairs_36"]["pairs"]] == [12, 24] and 12 % 5 and 12 % 7


def test_hard_boxes_are_hard_and_their_xywh_form_is_exact():
    b = pc.HARD_BOXES.astype(np.float64)
    assert (b[:, 2] == b[:, 0]).any() and (b[:, 3] == b[:, 1]).any()
    assert (b < 0).any() and (b.min(axis=1) < 0).sum() >= 3
    assert (np.abs(b) >= 3000).any()
    w = pc.to_xywh(pc.HARD_BOXES).astype(np.float64)
    assert np.array_equal(w[:, 2], b[:, 2] - b[:, 0] + 1) and np.array_equal(w[:, 3], b[:, 3] - b[:, 1] + 1)
    # ... in float32 as well: fl(fl(x2 - x1) + 1) is the exact width, so the two modes must agree bit for bit
    f = pc.HARD_BOXES
    assert np.array_equal(((f[:, 2] - f[:, 0]) + np.float32(1)).astype(np.float64), w[:, 2])
    for a, c in (("hard_boxes_xyxy_outliers", "hard_boxes_xywh_outliers"), ("hard_boxes_xyxy_var0", "hard_boxes_xywh_var0")):
        A, C = TOKEN_CASES[a], TOKEN_CASES[c]
        assert A["box_mode"] == 0 and C["box_mode"] == 1
        assert np.array_equal(pc.box_features(A)[0], pc.box_features(C)[0])
        assert np.array_equal(A["rgb"], C["rgb"]) and np.array_equal(A["labels"], C["labels"])
    assert (pc.state_dict(1, var0=True)["pos_embed.0.running_var"] == 0).all()
    lab = TOKEN_CASES["pairs_28"]["labels"]
    assert lab[0] == 0 and lab[-1] == 150
    assert np.abs(TOKEN_CASES["hard_boxes_xyxy_outliers"]["rgb"]).max() > 300
    assert abs(TOKEN_CASES["hard_boxes_xyxy_offset"]["rgb"].mean() - 15.0) < 0.5


@pytest.mark.parametrize("C", [151, 201])
def test_softmax_rows_contain_what_they_are_named_for(C):
    case = TOKEN_CASES["sgcls_%d" % C]
    names, rows = pc.softmax_logit_rows(C, pc._rng("softmax_%d" % C, 2))
    assert np.array_equal(rows, case["logits"], equal_nan=True) and rows.shape == (len(names), C)
    r = dict(zip(names, rows.astype(np.float64)))
    assert len(np.unique(r["equal"])) == 1 and len(np.unique(r["equal_zero"])) == 1
    with np.errstate(over="ignore"):
        p = torch.softmax(torch.from_numpy(rows).double(), 1).numpy()
    p = dict(zip(names, p))
    assert np.allclose(p["equal"], 1.0 / C, rtol=1e-12)
    assert p["dominant_last"][C - 1] > 1 - 1e-12 and p["dominant_first"][0] > 1 - 1e-9
    assert np.isneginf(r["minus_inf_entries"]).sum() == len(range(0, C, 3)) and np.isfinite(r["minus_inf_entries"]).any()
    assert np.isneginf(r["minus_inf_all_but_one"]).sum() == C - 1 and p["minus_inf_all_but_one"][C // 2] == 1.0
    assert np.abs(r["magnitude_1e4"]).max() > 1e4
    # softmax without the max subtraction overflows float32 AND float64 on these rows
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(r["magnitude_1e4"])).any() and np.isinf(np.exp(r["offset_plus_1e4"])).all()
    assert (np.exp(r["offset_minus_1e4"]) == 0).all()
    assert all(np.isfinite(v).all() and abs(v.sum() - 1) < 1e-12 for v in p.values())
    pairs = case["pairs"][0]
    assert set(pairs.ravel()) == set(range(len(names))), "a softmax row that no pair reads"


# ---- premises: batch statistics -----------------------------------------------------------------------------------------------------------
def test_batch_statistics_cases():
    assert sorted({len(c["boxes"]) for c in BN_CASES.values()}) == [2, 255, 256, 257, 513]      # 256-thread stride: below, at, above, 2 trips + 1
    for name, c in BN_CASES.items():
        ref, bound = pc.batch_statistics(c)
        v, dv = pc.box_features(c)
        if "identical" in name:
            assert (ref[4:] == 0).all() and len(np.unique(c["boxes"], axis=0)) == 1
        if "offset_1e4" in name:
            # features exact in float32 (grid of 1/8 at 1e4), so the bound is the store rounding: 2^-24 relative
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
            assert (v[:, :2] > 1e4).all() and (v[:, :2].max(0) - v[:, :2].min(0) <= 2).all()
            # ... and a one-pass variance in float32, E[x^2] - E[x]^2, misses it by far more than 10 bounds
            x = v[:, 0].astype(np.float32)
            n = np.float32(len(x))
            one_pass = float((x * x).sum(dtype=np.float32) / n - (x.sum(dtype=np.float32) / n) ** 2)
            assert abs(one_pass - ref[4]) > 10 * (bound[4] + pc.U * ref[4]), (name, one_pass, ref[4])
            # even a float64 one-pass loses digits there the two-pass keeps: cancellation of 1e8 against a variance below 1
            assert ref[4] < 1.0 and (v[:, 0] ** 2).mean() > 1e8
        both = BN_CASES[name.replace("xyxy", "xywh")], BN_CASES[name.replace("xywh", "xyxy")]
        assert np.array_equal(pc.box_features(both[0])[0], pc.box_features(both[1])[0])


# ---- premises: head -----------------------------------------------------------------------------------------------------------------------
def test_head_cases_reach_every_trip_of_both_loops():
    trips = {w: (w + 127) // 128 for w in pc.HEAD_WIDTHS}
    assert trips == {51: 1, 101: 1, 60: 1, 108: 1, 128: 1, 129: 2, 257: 3}
    live = set()      # (pairs alive in a workgroup of 4, chunk offset mod 4) over every chunk of every call
    for chunk in pc.HEAD_CHUNKS:
        for count in pc.HEAD_PAIR_COUNTS:
            for c0 in range(0, count, chunk):
                np_ = min(chunk, count - c0)
                for g in range(0, np_, 4):
                    live.add((min(4, np_ - g), c0 % 4))
    assert {k for k, _ in live} == {1, 2, 3, 4} and {o for _, o in live} == {0, 1, 2, 3}
    assert {5 % 4, 2 % 4, 3 % 4} == {1, 2, 3}


# ---- the bounds have teeth ----------------------------------------------------------------------------------------------------------------
WRONG = {      # deliberate mistake -> the cases whose bound it must leave by 10 x
    "xywh_plus_one": ("+1 applied in xywh mode", ["hard_boxes_xywh_outliers", "hard_boxes_xywh_var0"]),
    "halves_swapped": ("subject and object halves swapped", ["pairs_28", "hard_boxes_xyxy_offset"]),
    "relu_per_half": ("ReLU applied per half before the sum", ["pairs_6", "sgcls_201"]),
    "pos_before_relu": ("the positional embedding added before the ReLU", ["pairs_6", "sgcls_151"]),
    "softmax_no_max": ("softmax without the max subtraction", ["sgcls_151", "sgcls_201"]),
}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_token_restatements_leave_the_bound(wrong):
    for name in WRONG[wrong][1]:
        case = TOKEN_CASES[name]
        sd = _sd(case)
        tok, bound, _, _ = pc.restate(sd, case)
        bad, _, _, _ = pc.restate(sd, case, wrong=(wrong,))
        ratio = pc.worst_ratio(bad, tok, bound)
        assert ratio >= 10.0, (wrong, name, ratio)
        # ... in the rows it is about: the location / class rows for everything but the swapped halves, which move the patch rows too
        if wrong == "halves_swapped":
            assert pc.worst_ratio(bad[:, 1:17], tok[:, 1:17], bound[:, 1:17]) >= 10.0


def test_unbiased_variance_for_normalising_leaves_the_bound():
    """n / (n - 1) in the variance BatchNorm normalises with: a factor 2 at two objects, still 10 bounds at 513."""
    for name in ("bn_plain_2_xyxy", "bn_plain_257_xywh", "bn_offset_1e4_513_xyxy"):
        case = BN_CASES[name]
        sd = pc.state_dict(1)
        stats = pc.batch_statistics(case)[0]
        tok, bound, _, _ = pc.restate(sd, case, stats=stats, patch=False)
        bad, _, _, _ = pc.restate(sd, case, stats=stats, wrong=("unbiased_variance",), patch=False)
        assert pc.worst_ratio(bad[:, 17], tok[:, 17], bound[:, 17]) >= 10.0, name
    # ... and the statistics themselves tell the two variances apart
    ref, bound = pc.batch_statistics(BN_CASES["bn_plain_513_xyxy"])
    assert (np.abs(ref[8:] - ref[4:8]) > 10 * bound[4:8]).all()


@pytest.mark.parametrize("wrong", ["next_image_offset", "placeholder_dropped"])
def test_wrong_pair_indices_differ(wrong):
    """The index comparison is bit-exact, so 'leaving the bound' is differing at all: the object offset of the NEXT image, and the
    (0, 0) placeholder of a one-object image dropped."""
    hit = 0
    for name, case in PAIR_INDEX_CASES.items():
        subj, obj = pc.reference_indices(case)
        s2, o2 = pc.reference_indices(case, wrong=(wrong,))
        if len(case["num_objs"]) == 1 and wrong == "next_image_offset":
            assert not np.array_equal(subj, s2)      # even one image: every index moves by its object count
        hit += len(subj) != len(s2) or not np.array_equal(subj, s2) or not np.array_equal(obj, o2)
    assert hit >= len(PAIR_INDEX_CASES) - 1
    # the int32 indices are seen through the token rows: a wrong offset moves the location rows out of their bound
    case = PAIR_INDEX_CASES["zero_pairs_middle"]
    sd = pc.state_dict(1)
    tok, bound, _, _ = pc.restate(sd, case, patch=False)
    if wrong == "next_image_offset":
        shifted = dict(case, num_objs=case["num_objs"] + [3], pairs=case["pairs"] + [pc.NO_PAIRS],
                       boxes=np.concatenate([case["boxes"], case["boxes"][:3]]), labels=np.concatenate([case["labels"], case["labels"][:3]]))
        bad, _, _, _ = pc.restate(sd, shifted, wrong=(wrong,), patch=False)
        assert pc.worst_ratio(bad[:, 17], tok[:, 17], bound[:, 17]) >= 10.0


def test_head_bound_tells_a_dropped_term_apart():
    """gamma(577) (sum |w||cls| + |b|) against the two mistakes head_kernel's loops could make: a class column taken from the
    neighbouring trip (c + 128 for c), and a pair reading the cls row of its neighbour."""
    rng = np.random.default_rng(5)
    sd = pc.state_dict(1, num_out=257)
    cls = rng.standard_normal((5, pc.DIM)).astype(np.float32)
    ref, bound = pc.head_reference(sd, cls)
    assert (np.abs(np.roll(ref, 128, axis=1) - ref) / bound).max() >= 10 and (np.abs(np.roll(ref, 1, axis=0) - ref) / bound).max() >= 10
    f32 = (torch.from_numpy(cls) @ torch.from_numpy(sd["rel_out.weight"]).t() + torch.from_numpy(sd["rel_out.bias"])).numpy()
    assert (np.abs(f32 - ref) / bound).max() <= 1.0
