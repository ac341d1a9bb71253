"""The HIP post-processor (vanilla, MEET merge, expert voting) and the HIP evaluators against their oracles at production
sizes, at the 16 384-row limit, on inputs whose order the tie-break alone decides, and on both sides of every size at which
sgg_eval.hip changes its code path.  Post-processor rows are compared per source row (tests/post_eval_cases.py): no row is
left out.  The premises of the inputs are asserted on the CPU in tests/test_post_eval_scale_host.py; the figures each test
prints are kept in profiles/post_eval_scale_parity.txt."""
import ctypes

import numpy as np
import pytest
import torch

import post_eval_cases as pc
from oracle import sgg_eval_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 0x5A


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _boxes(n):
    from veto_amd.structures import BoxList
    return BoxList(torch.zeros(n, 4), (800, 600)).to(DEV)


def _fields(res, triple):
    out = {k: res.get_field(k).cpu().numpy() for k in ("rel_pair_idxs", "pred_rel_scores", "pred_rel_labels", "pred_labels", "pred_scores")}
    out["triple_scores"] = triple.cpu().numpy()
    return out


def _report(label, fig):
    print("post_eval_scale: %-28s rows %5d  max err: probabilities %.2e  triple %.2e  object score %.2e | bit-equal neighbours %5d, "
          "rows not at the oracle's position %4d (their oracle scores within %.2e)"
          % (label, fig["rows"], fig["prob_err"], fig["triple_err"], fig["obj_err"], fig["bit_ties"], fig["moved"], fig["moved_gap"]))


def _post(voting=None):
    from veto_amd import testing
    from veto_amd.postprocess import PostProcessor
    cfg = None
    if voting:
        cfg = testing.make_config(1, 8, meet=True, dataset="VG")
        cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = True
        cfg.ENSEMBLE_LEARNING.VOTING = voting
    return PostProcessor(False, use_gt_box=True, cfg=cfg)


def _run_grouped(case):
    """MEET merge or expert voting of one image through PostProcessor.forward."""
    post = _post(case.get("voting"))
    res = post(({k: _to(v) for k, v in case["rel"].items()}, [_to(case["obj"])]), [_to(case["pairs"])], [_boxes(case["n"])],
               incre_idx_list=case["incre"], ensemble=True)[0]
    torch.cuda.synchronize()
    assert res.get_field("rel_pair_idxs").dtype == torch.float32
    return _fields(res, post.last_triple_scores[0])


def _run_vanilla(case, images=None):
    """The vanilla branch on the images `images` of the batch (all of them by default); one field dict per image."""
    idx = list(range(len(case["pairs"]))) if images is None else images
    o0 = np.concatenate([[0], np.cumsum(case["num_objs"])])
    p0 = np.concatenate([[0], np.cumsum([len(p) for p in case["pairs"]])])
    rel = [_to(case["rel"][p0[i]:p0[i + 1]]) for i in idx]
    obj = [_to(case["obj"][o0[i]:o0[i + 1]]) for i in idx]
    post = _post()
    res = post((rel, obj), [_to(case["pairs"][i]) for i in idx], [_boxes(case["num_objs"][i]) for i in idx])
    torch.cuda.synchronize()
    return [_fields(r, t) for r, t in zip(res, post.last_triple_scores)]


# ---- A. post-processor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,exact", [("vg36", 6300, False), ("gqa_limit", 16384, False), ("capped_ties", 10240, True)])
def test_meet_merge_every_row_against_the_oracle(name, rows, exact):
    """36 objects x 5 VG groups (n2 = 8192); 4 096 pairs x 4 GQA groups = the 16 384-row limit with a width-67 head; the capped
    image (2 048 pairs x 5 groups) with one-hot objects and 64 distinct relation rows per group, where 320 scores are shared
    by 32 rows each and the device order must be the oracle's, row for row."""
    case = pc.meet_case(name)
    fig = pc.compare_rows(_run_grouped(case), pc.meet_reference(name), case["pairs"], case["incre"], expect_all=rows, exact_order=exact)
    _report("MEET " + name, fig)
    if exact:
        assert fig["bit_ties"] == rows - 320


@pytest.mark.parametrize("name,exact", [("vg36_C", False), ("vg36_U", False), ("capped_ties_C", True)])
def test_expert_voting_every_kept_row_against_the_oracle(name, exact):
    """The kept set equals the oracle's exactly (no expert's top-two gap is below 1e-5, asserted on the CPU), and every kept
    row is compared; on the capped tie case the order is the oracle's, row for row."""
    case = pc.vote_case(name)
    fig = pc.compare_rows(_run_grouped(case), pc.vote_reference(name), case["pairs"], case["incre"], exact_order=exact)
    _report("vote " + name, fig)
    assert 0 < fig["rows"] < 5 * len(case["pairs"])


def test_expert_voting_keeps_nothing_and_everything():
    case = pc.vote_case("none_U")               # the three experts' arg-maxes differ by construction
    got = _run_grouped(case)
    assert got["rel_pair_idxs"].shape == (0, 2) and got["pred_rel_scores"].shape == (0, 51) and got["pred_rel_labels"].shape == (0,)
    assert got["triple_scores"].shape == (0,)
    fig = pc.compare_rows(got, pc.vote_reference("none_U"), case["pairs"], case["incre"])
    assert fig["rows"] == 0
    case = pc.vote_case("all_U")                # three identical experts
    fig = pc.compare_rows(_run_grouped(case), pc.vote_reference("all_U"), case["pairs"], case["incre"], expect_all=6300)
    _report("vote all_U", fig)


def _filled(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(tensors):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in tensors)


def test_meet_merge_refuses_one_pair_more_than_the_limit():
    """4 097 pairs x 4 groups = 16 388 rows: veto_postprocess_meet refuses, launches nothing and leaves every output (and the
    workspace) as it was."""
    from veto_amd import native
    case = pc.meet_case("gqa_over")
    with pytest.raises(native.VetoError, match="exceeds 16384"):
        _run_grouped(case)
    lib = native.load_library()
    groups = [_to(case["rel"]["group_%d" % k]) for k in range(4)]
    obj, pairs = _to(case["obj"]), _to(case["pairs"])
    K, P, n_rel = 4, len(case["pairs"]), len(case["incre"])
    total = K * P
    outs = {"obj_scores": _filled(case["n"], torch.float32), "obj_pred": _filled(case["n"], torch.int64),
            "prob": _filled((total, n_rel), torch.float32), "pairs": _filled((total, 2), torch.int64),
            "labels": _filled(total, torch.int64), "triple": _filled(total, torch.float32),
            "workspace": _filled(lib.veto_postprocess_workspace_bytes(total, n_rel), torch.uint8)}
    ptrs = (ctypes.c_void_p * K)(*[g.data_ptr() for g in groups])
    widths = (ctypes.c_int32 * K)(*[g.shape[1] for g in groups])
    incre = (ctypes.c_int32 * n_rel)(*case["incre"])
    a = native.VetoPostMeetArgs()
    a.struct_size = ctypes.sizeof(native.VetoPostMeetArgs)
    a.n_obj, a.n_pair, a.n_groups, a.n_rel_cls, a.n_obj_cls = case["n"], P, K, n_rel, obj.shape[1]
    a.group_logits, a.group_widths = ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(widths, ctypes.c_void_p)
    a.incre_idx_list = ctypes.cast(incre, ctypes.c_void_p)
    a.obj_logits, a.rel_pairs = obj.data_ptr(), pairs.data_ptr()
    a.obj_scores, a.obj_pred = outs["obj_scores"].data_ptr(), outs["obj_pred"].data_ptr()
    a.rel_prob_sorted, a.rel_pairs_sorted = outs["prob"].data_ptr(), outs["pairs"].data_ptr()
    a.rel_labels_sorted, a.triple_sorted = outs["labels"].data_ptr(), outs["triple"].data_ptr()
    stream = torch.cuda.current_stream(DEV)
    call = lambda: lib.veto_postprocess_meet(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a),
                                             ctypes.c_void_p(outs["workspace"].data_ptr()), outs["workspace"].numel())
    assert call() < 0 and b"exceeds 16384" in lib.veto_last_error()
    assert _untouched(outs.values())
    a.n_pair = P - 1                    # the same buffers at the limit: accepted, and the outputs are written
    assert call() == 0
    assert not _untouched([outs["triple"][:total - K]]) and _untouched([outs["triple"][total - K:]])


@pytest.mark.parametrize("name", ["random", "ties"])
def test_vanilla_batch_with_empty_single_and_limit_sized_images(name):
    """Pair counts [0, 1, 1260, 0, 2, 16384, 90] in one batch: every row of every image against the oracle, and the batch
    equal, bit for bit, to each image run alone (an image without pairs cannot run alone: the ABI takes no empty batch).
    'ties': one-hot objects and 64 distinct relation rows per image, so the order is the tie-break's and must be the oracle's."""
    case, ref = pc.vanilla_case(name), pc.vanilla_reference(name)
    got = _run_vanilla(case)
    for i, (g, r) in enumerate(zip(got, ref)):
        cnt = pc.VANILLA_PAIR_COUNTS[i]
        assert g["rel_pair_idxs"].shape == (cnt, 2) and g["pred_rel_scores"].shape == (cnt, 51)
        fig = pc.compare_rows(g, r, case["pairs"][i], expect_all=cnt, exact_order=(name == "ties"))
        _report("vanilla %s image %d" % (name, i), fig)
        if name == "ties" and cnt:
            assert fig["bit_ties"] == cnt - min(cnt, pc.TIE_PERIOD)
    for i, cnt in enumerate(pc.VANILLA_PAIR_COUNTS):
        if cnt == 0:
            continue
        alone = _run_vanilla(case, [i])[0]
        for key, v in alone.items():
            assert v.dtype == got[i][key].dtype and v.tobytes() == got[i][key].tobytes(), (i, key)


def test_vanilla_refuses_an_image_of_one_pair_more_than_the_limit():
    from veto_amd import native
    case = pc.vanilla_case("over")
    with pytest.raises(native.VetoError, match="max_pairs_per_image 16385 outside 1..16384"):
        _run_vanilla(case)
    lib = native.load_library()
    P, n = 16385, 129
    rel, obj, pairs = _to(case["rel"]), _to(case["obj"]), _to(case["pairs"][0])
    obj_off, pair_off = _to(np.array([0, n], dtype=np.int32)), _to(np.array([0, P], dtype=np.int32))
    outs = {"obj_scores": _filled(n, torch.float32), "obj_pred": _filled(n, torch.int64), "prob": _filled((P, 51), torch.float32),
            "pairs": _filled((P, 2), torch.int64), "labels": _filled(P, torch.int64), "triple": _filled(P, torch.float32),
            "workspace": _filled(lib.veto_postprocess_workspace_bytes(P, 51), torch.uint8)}
    a = native.VetoPostArgs()
    a.struct_size = ctypes.sizeof(native.VetoPostArgs)
    a.n_img, a.n_obj, a.n_pair, a.n_rel_cls, a.n_obj_cls, a.max_pairs_per_image = 1, n, P, 51, 151, P
    a.rel_logits, a.obj_logits, a.rel_pairs = rel.data_ptr(), obj.data_ptr(), pairs.data_ptr()
    a.img_obj_offset, a.img_pair_offset = obj_off.data_ptr(), pair_off.data_ptr()
    a.obj_scores, a.obj_pred = outs["obj_scores"].data_ptr(), outs["obj_pred"].data_ptr()
    a.rel_prob_sorted, a.rel_pairs_sorted = outs["prob"].data_ptr(), outs["pairs"].data_ptr()
    a.rel_labels_sorted, a.triple_sorted = outs["labels"].data_ptr(), outs["triple"].data_ptr()
    stream = torch.cuda.current_stream(DEV)
    rc = lib.veto_postprocess(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a), ctypes.c_void_p(outs["workspace"].data_ptr()),
                              outs["workspace"].numel())
    assert rc < 0 and b"16385 outside 1..16384" in lib.veto_last_error()
    assert _untouched(outs.values())


# ---- B. evaluators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.EVAL_CASES)
def test_evaluator_code_paths_against_the_oracle(name):
    """101 predicate classes (two trips of the 64-wide row loops) in predcls / sgcls / sgdet; the M <= 100 branch and its
    neighbours (P = 1, 2, 3 at 51 classes, P = 1, 2 at 101); P = 99 / 100 / 101 around the pruned path's row-count switch;
    2 048 / 2 049 cells above the pruned path's bound, around its fall-back to the general select.
    sgdet: the reference's pair accuracy records nothing there (sgg_eval.py:356), so the device's acc_rank is NO_MATCH and A@K
    NaN; the oracle's A@K does not apply and the other five metrics are compared."""
    from veto_amd.evaluation import SGGEvaluator
    images, zeroshot, mode, C = pc.eval_case(name)
    ref = pc.eval_reference(name)
    res = SGGEvaluator(mode, C, zeroshot, iou_thres=0.5, device=DEV).evaluate(images)
    clamp = lambda x: np.minimum(np.asarray(x, dtype=np.int64), so.NO_MATCH)
    n_match = 0
    for i, r in enumerate(ref["per_image"]):
        g = res["per_image"][i]
        if r is None:
            assert g is None
            continue
        assert np.array_equal(g["ng_rows"], r["ng_rows"]) and np.array_equal(g["ng_cols"], r["ng_cols"]), (i, "ng list")
        for key in ("gc_rank", "ng_rank", "acc_rank"):
            want = np.full_like(r[key], so.NO_MATCH) if (mode == "sgdet" and key == "acc_rank") else r[key]
            assert np.array_equal(clamp(g[key]), clamp(want)), (i, key)
        assert np.array_equal(g["zeroshot"], r["zeroshot"]), i
        n_match += int((r["gc_rank"] < so.NO_MATCH).sum() + (r["ng_rank"] < so.NO_MATCH).sum())
    assert res["images_evaluated"] == sum(r is not None for r in ref["per_image"])
    worst = 0.0
    for key in ("recall", "recall_nogc", "zeroshot_recall", "accuracy", "mean_recall", "ng_mean_recall"):
        for k in so.KS:
            if mode == "sgdet" and key == "accuracy":
                assert np.isnan(res[key][k])
                continue
            assert np.isnan(res[key][k]) == np.isnan(ref[key][k]), (key, k)
            if not np.isnan(ref[key][k]):
                worst = max(worst, abs(res[key][k] - ref[key][k]))
                assert abs(res[key][k] - ref[key][k]) < 1e-12, (key, k, res[key][k], ref[key][k])
    for key in ("mean_recall_list", "ng_mean_recall_list"):
        for k in so.KS:
            assert len(res[key][k]) == C - 1
            err = np.abs(np.asarray(res[key][k]) - np.asarray(ref[key][k])).max()
            worst = max(worst, float(err))
            assert err < 1e-12, (key, k)
    print("post_eval_scale: evaluator %-14s %d images, %d classes, lists and ranks equal (%d matches), worst metric error %.1e"
          % (name, len(images), C, n_match, worst))
