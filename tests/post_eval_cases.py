"""TEST INFRASTRUCTURE: constructed inputs, oracle results and the order-free row comparison shared by
tests/test_post_eval_scale_host.py (premises of the inputs, CPU) and tests/test_post_eval_scale_gpu.py (the HIP
post-processor and evaluators against the oracle at production sizes, at their limits and on exact ties).

Post-processor rows are compared per SOURCE ROW, so that a rounding-sized swap between near-equal sort keys moves no row
out of the comparison:
  vanilla      source row = index of the output pair in the image's pair list
  MEET / vote  source row = group * n_pair + pair index; the group is read off the probability row, whose non-zero columns
               (c >= 1) are the group's own classes (incre_idx_list[c] = group + 1)
Tolerances are those of tests/test_gpu_parity.py: 2e-6 on relation probabilities and triple scores, 1e-6 on object scores."""
import functools

import numpy as np

from conftest import GQA_MEET_GROUPS, VG_MEET_GROUPS
from oracle import sgg_eval_oracle as so
from oracle import veto_oracle as vo
from veto_amd import synth

SCORE_TOL = 2e-6          # pred_rel_scores, triple scores
OBJ_TOL = 1e-6            # pred_scores
TIE_GAP = 2 * SCORE_TOL   # distinct scores of the tie cases lie further apart than both sides' rounding together
ARGMAX_GAP = 1e-5         # top-two probability gap of every expert in the voting cases
MAX_ROWS = 16384          # postprocess_max_pairs_per_image()
TIE_PERIOD = 64

# seeds chosen on the CPU so that the premises test_post_eval_scale_host.py asserts hold
SEED_GQA, SEED_TIES, SEED_VOTE, SEED_VANILLA, SEED_EVAL = 31, 40, 29, 36, 92


def onehot_obj_logits(seed, n, n_cls):
    """+-1000 logits as conftest.load_post_golden's `onehot`: every object score is exactly 1.0 on both sides."""
    lab = synth.integers(seed, "cases.labels", (n,), 1, n_cls)
    out = np.full((n, n_cls), -1000.0, dtype=np.float32)
    out[np.arange(n), lab] = 1000.0
    return out


def tied_rows(seed, name, n_rows, width, std=2.0):
    """Row i is rows[i % 64]: with one-hot objects every score is shared by n_rows / 64 rows."""
    rows = synth.normal(seed, name, (TIE_PERIOD, width), 0.0, std)
    return rows[np.arange(n_rows) % TIE_PERIOD]


# ---- post-processor inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def meet_case(name):
    """{'rel': {group_k: [P, g_k + 2]}, 'obj': [n, n_obj_cls], 'pairs': [P, 2], 'incre', 'n'}"""
    if name == "vg36":            # 36 objects x 5 groups = 6 300 rows, the logits of conftest.load_postmeet_golden
        groups, n, n_objc, P = VG_MEET_GROUPS, 36, 151, 1260
        rel = {"group_%d" % k: synth.normal(23, "meet.group_%d" % k, (P, g + 2), 0.0, 2.0) for k, g in enumerate(groups)}
        obj = synth.normal(23, "meet.obj_logits", (n, n_objc), 0.0, 3.0)
    elif name in ("gqa_limit", "gqa_over"):   # 65 objects, 4 groups, a width-67 head: 16 384 rows is the limit
        groups, n, n_objc = GQA_MEET_GROUPS, 65, 201
        P = MAX_ROWS // 4 + (name == "gqa_over")
        rel = {"group_%d" % k: synth.normal(SEED_GQA, "meet.group_%d" % k, (4160, g + 2), 0.0, 2.0)[:P] for k, g in enumerate(groups)}
        obj = synth.normal(SEED_GQA, "meet.obj_logits", (n, n_objc), 0.0, 3.0)
    elif name == "capped_ties":   # 64 objects, the 2 048-pair cap, 5 groups = 10 240 rows; the tie-break alone decides the order
        groups, n, n_objc, P = VG_MEET_GROUPS, 64, 151, 2048
        rel = {"group_%d" % k: tied_rows(SEED_TIES, "meet.group_%d" % k, P, g + 2) for k, g in enumerate(groups)}
        obj = onehot_obj_logits(SEED_TIES, n, n_objc)
    else:
        raise KeyError(name)
    return {"rel": rel, "obj": obj, "pairs": vo.enumerate_test_pairs(n)[:P], "incre": vo.meet_incre_idx_list(groups), "n": n}


@functools.lru_cache(maxsize=None)
def vote_case(name):
    """As meet_case with rel = {group_<k><e>: ...}, plus 'voting'."""
    groups, n_objc = VG_MEET_GROUPS, 151
    kind, voting = name.rsplit("_", 1)
    if kind == "capped_ties":
        n, P = 64, 2048
        obj = onehot_obj_logits(SEED_TIES, n, n_objc)
        gen = lambda tag, w, std: tied_rows(SEED_TIES, tag, P, w, std)
    else:
        n, P = 36, 1260
        obj = synth.normal(SEED_VOTE, "vote.obj_logits", (n, n_objc), 0.0, 3.0)
        gen = lambda tag, w, std: synth.normal(SEED_VOTE, tag, (P, w), 0.0, std)
    rel = {}
    for k, g in enumerate(groups):
        base = gen("vote.base_%d" % k, g + 2, 1.5)     # as conftest.load_postvote_golden: a shared part so that experts often agree
        for e in range(3):
            own = gen("vote.group_%d%d" % (k, e + 1), g + 2, 1.0)
            if kind == "none":      # expert e's arg-max is column 1 + e: no two experts agree
                own = own.copy()
                own[:, 1 + e] += 20.0
            elif kind == "all":     # three identical experts: every row survives
                own = gen("vote.group_%d1" % k, g + 2, 1.0)
            rel["group_%d%d" % (k, e + 1)] = (base + own).astype(np.float32)
    return {"rel": rel, "obj": obj, "pairs": vo.enumerate_test_pairs(n)[:P], "incre": vo.meet_incre_idx_list(groups), "n": n,
            "voting": voting}


VANILLA_PAIR_COUNTS = [0, 1, 1260, 0, 2, 16384, 90]
VANILLA_OBJ_COUNTS = [1, 2, 36, 1, 2, 129, 10]


@functools.lru_cache(maxsize=None)
def vanilla_case(name):
    """One batch: {'rel': [sum P, 51], 'obj': [sum n, 151], 'pairs': list of [P_i, 2], 'num_objs'}.  name: 'random' or 'ties'
    (one-hot objects, relation row i of an image = rows[i % 64]); 'over' is one image of 16 385 pairs."""
    if name == "over":
        counts, num_objs = [MAX_ROWS + 1], [129]
    else:
        counts, num_objs = VANILLA_PAIR_COUNTS, VANILLA_OBJ_COUNTS
    pairs = [vo.enumerate_test_pairs(n)[:c] if c else np.zeros((0, 2), dtype=np.int64) for n, c in zip(num_objs, counts)]
    assert [len(p) for p in pairs] == counts
    if name == "ties":
        rel = np.concatenate([tied_rows(SEED_VANILLA, "post.rel.%d" % i, c, 51) for i, c in enumerate(counts)])
        obj = onehot_obj_logits(SEED_VANILLA, sum(num_objs), 151)
    else:
        rel = synth.normal(SEED_VANILLA, "post.rel_logits", (sum(counts), 51), 0.0, 2.0)
        obj = synth.normal(SEED_VANILLA, "post.obj_logits", (sum(num_objs), 151), 0.0, 3.0)
    return {"rel": rel, "obj": obj, "pairs": pairs, "num_objs": num_objs}


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def meet_reference(name):
    c = meet_case(name)
    return _np(vo.postprocess_meet(c["rel"], c["obj"], c["pairs"], c["incre"], len(c["incre"])))


@functools.lru_cache(maxsize=None)
def vote_reference(name):
    c = vote_case(name)
    return _np(vo.postprocess_vote(c["rel"], c["obj"], c["pairs"], c["incre"], len(c["incre"]), voting=c["voting"]))


@functools.lru_cache(maxsize=None)
def vanilla_reference(name):
    c = vanilla_case(name)
    return [_np(r) for r in vo.postprocess(c["rel"], c["obj"], c["pairs"], c["num_objs"])]


def expert_top_two_gaps(case):
    """Per expert head: top-1 minus top-2 probability over the columns the arg-max runs over (1 .. g)."""
    import torch
    gaps = []
    for logit in case["rel"].values():
        prob = torch.softmax(torch.from_numpy(logit), -1)[:, 1:-1]
        top = torch.topk(prob, 2, dim=1)[0]
        gaps.append((top[:, 0] - top[:, 1]).numpy())
    return np.concatenate(gaps)


def distinct_score_gaps(scores):
    """(number of distinct values, smallest gap between two distinct values) of a sorted score list."""
    u = np.unique(np.asarray(scores, dtype=np.float64))
    return len(u), (np.diff(u).min() if len(u) > 1 else np.inf)


# ---- order-free comparison ------------------------------------------------------------------------------------------------
def source_rows(out_pairs, prob, pair_list, incre=None):
    """Source row of every output row (module docstring).  Raises if an output pair is not in the pair list or if a
    probability row's non-zero columns are not exactly one group's classes."""
    pair_list = np.asarray(pair_list, dtype=np.int64).reshape(-1, 2)
    out_pairs = np.asarray(out_pairs)
    n_pair = len(pair_list)
    if len(out_pairs) == 0:
        return np.zeros(0, dtype=np.int64)
    ip = out_pairs.astype(np.int64)
    assert np.array_equal(ip, out_pairs), "pair indices are not whole numbers"
    side = int(max(pair_list.max(), ip.max())) + 1
    lut = np.full(side * side, -1, dtype=np.int64)
    lut[pair_list[:, 0] * side + pair_list[:, 1]] = np.arange(n_pair)
    assert ip.min() >= 0
    pidx = lut[ip[:, 0] * side + ip[:, 1]]
    assert (pidx >= 0).all(), "an output pair that is not in the input pair list"
    if incre is None:
        return pidx
    col_group = np.asarray(incre, dtype=np.int64)[1:] - 1
    nz = np.asarray(prob)[:, 1:] != 0
    assert nz.any(1).all(), "a probability row without a non-zero foreground column"
    group = col_group[nz.argmax(1)]
    assert (nz == (col_group[None, :] == group[:, None])).all(), "non-zero columns are not exactly one group's classes"
    return group * n_pair + pidx


def compare_rows(got, ref, pair_list, incre=None, expect_all=None, exact_order=False):
    """got / ref: dicts of numpy arrays rel_pair_idxs, pred_rel_scores, pred_rel_labels, triple_scores, pred_labels,
    pred_scores.  Asserts the permutation, per-row and order properties on EVERY row; returns the observed figures."""
    src_g = source_rows(got["rel_pair_idxs"], got["pred_rel_scores"], pair_list, incre)
    src_r = source_rows(ref["rel_pair_idxs"], ref["pred_rel_scores"], pair_list, incre)
    n = len(src_r)
    assert len(src_g) == n, "row count %d, oracle %d" % (len(src_g), n)
    assert got["pred_rel_scores"].shape == ref["pred_rel_scores"].shape and got["rel_pair_idxs"].shape == ref["rel_pair_idxs"].shape
    # permutation: the same set of source rows, each once (voting: exactly the oracle's kept set)
    assert np.array_equal(np.sort(src_g), np.sort(src_r)) and len(np.unique(src_g)) == n
    if expect_all is not None:
        assert np.array_equal(np.sort(src_r), np.arange(expect_all))
    assert np.array_equal(got["pred_labels"], ref["pred_labels"])
    fig = {"rows": n, "obj_err": float(np.abs(got["pred_scores"] - ref["pred_scores"]).max())}
    assert fig["obj_err"] <= OBJ_TOL, fig
    if n == 0:
        fig.update(prob_err=0.0, triple_err=0.0, moved=0, moved_gap=0.0, bit_ties=0)
        return fig
    ref_pos = np.empty(int(src_r.max()) + 1, dtype=np.int64)
    ref_pos[src_r] = np.arange(n)
    r = ref_pos[src_g]                                   # oracle position of every device row
    fig["prob_err"] = float(np.abs(got["pred_rel_scores"] - ref["pred_rel_scores"][r]).max())
    fig["triple_err"] = float(np.abs(got["triple_scores"] - ref["triple_scores"][r]).max())
    assert fig["prob_err"] <= SCORE_TOL and fig["triple_err"] <= SCORE_TOL, fig
    assert np.array_equal(got["pred_rel_labels"], ref["pred_rel_labels"][r])
    # order: non-increasing; bit-equal neighbours in source order
    ts = got["triple_scores"]
    assert (np.diff(ts) <= 0).all(), "scores are not non-increasing"
    tie = ts[1:] == ts[:-1]
    fig["bit_ties"] = int(tie.sum())
    assert (src_g[1:][tie] > src_g[:-1][tie]).all(), "bit-equal neighbours are not in source order"
    # every pair (i < k) that the oracle has the other way round: its oracle scores lie within SCORE_TOL.  The oracle's scores
    # do not increase along its order, so for row i the worst partner is the later row that the oracle puts first of all.
    fig["moved"] = int((r != np.arange(n)).sum())
    first_later = np.minimum.accumulate(np.concatenate([r[1:], [n]])[::-1])[::-1]
    inv = first_later < r
    rs = ref["triple_scores"].astype(np.float64)
    fig["moved_gap"] = float((rs[first_later[inv]] - rs[r[inv]]).max()) if inv.any() else 0.0
    assert fig["moved_gap"] <= SCORE_TOL, fig
    if exact_order:
        assert fig["moved"] == 0, "the order differs from the oracle's where only the tie-break decides"
    return fig


# ---- evaluator inputs -----------------------------------------------------------------------------------------------------
def truncated(image, P):
    """The image with the first P rows of its prediction list."""
    out = dict(image)
    assert len(image["pred_rel_inds"]) >= P
    out["pred_rel_inds"], out["rel_scores"] = image["pred_rel_inds"][:P], image["rel_scores"][:P]
    return out


EVAL_NUM_OBJS = [2, 3, 11, 36, 5]
HALF_CELLS = (2048, 2049)    # kBig of sgg_eval.hip and one more


@functools.lru_cache(maxsize=None)
def eval_case(name):
    """(images, zeroshot, mode, C).  Names: c101_<mode>, small_c<C>, rows_c<C>, half_<N>."""
    kind, arg = name.split("_", 1)
    if kind == "c101":
        mode = arg
        if mode == "sgdet":
            images, zs = synth.synthetic_eval_images_sgdet(SEED_EVAL, EVAL_NUM_OBJS, num_rel_cls=101)
        else:
            images, zs = synth.synthetic_eval_images(SEED_EVAL, EVAL_NUM_OBJS, mode, num_rel_cls=101)
        return images, zs, mode, 101
    if kind == "small":     # M = P * (C - 1) <= 100 and just above: P = 1, 2 (M = 100), 3 at 51 classes, P = 1 (M = 100), 2 at 101
        C = int(arg[1:])
        Ps = [1, 2, 3] if C == 51 else [1, 2]
        images, zs = synth.synthetic_eval_images(SEED_EVAL + 1, [5, 6, 4][:len(Ps)], "sgcls", num_rel_cls=C)
        return [truncated(im, P) for im, P in zip(images, Ps)], zs, "sgcls", C
    if kind == "rows":      # the switch P >= 100 between the general select and the pruned path
        C = int(arg[1:])
        images, zs = synth.synthetic_eval_images(SEED_EVAL + 2, [11], "sgcls", num_rel_cls=C)
        return [truncated(images[0], P) for P in (99, 100, 101)], zs, "sgcls", C
    if kind == "half":      # the switch n_big <= 2048 inside the pruned path
        N, C, P = int(arg), 51, 120
        images, zs = synth.synthetic_eval_images(SEED_EVAL + 3, [12], "predcls", num_rel_cls=C)
        im = truncated(images[0], P)
        order = np.argsort(synth.uniform01(SEED_EVAL + 3, "half.low", P * C), kind="stable")
        low = np.empty(P * C, dtype=np.float64)
        low[order] = 0.01 + 0.38 * np.arange(P * C) / float(P * C)        # distinct values in [0.01, 0.39)
        scores = low.astype(np.float32).reshape(P, C)
        # N cells of the foreground columns at 0.5: row p takes N // P of them (+ 1 in the first N % P rows), at seeded columns
        for p in range(P):
            cols = 1 + np.argsort(synth.uniform01(SEED_EVAL + 3, "half.cols.%d" % p, C - 1), kind="stable")
            scores[p, cols[:N // P + (p < N % P)]] = 0.5
        im["rel_scores"] = scores
        return [im], zs, "predcls", C
    raise KeyError(name)


EVAL_CASES = ["c101_predcls", "c101_sgcls", "c101_sgdet", "small_c51", "small_c101", "rows_c51", "rows_c101",
              "half_%d" % HALF_CELLS[0], "half_%d" % HALF_CELLS[1]]


@functools.lru_cache(maxsize=None)
def eval_reference(name):
    images, zs, mode, C = eval_case(name)
    return so.evaluate(images, mode, zs, C)
