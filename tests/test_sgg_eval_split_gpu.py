"""Split-level relation evaluation on the device (MI355X): SGGEvaluator.accumulate() / finalize() / state() / load_state()
and veto_sgg_eval_fold behind them, against the oracle over a whole seeded split, against the numpy restatements of
tests/sgg_eval_split_cases.py on hand-made records placed on the fold's own boundaries, against the existing host path, and
bit for bit against itself under every partition of the same split.  The premises of the inputs: test_sgg_eval_split_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import sgg_eval_split_cases as sc
from veto_amd import native

pytestmark = pytest.mark.gpu

KS = sc.KS
DEV = torch.device("cuda:0")
LISTS = ("mean_recall_list", "ng_mean_recall_list")
IMAGE_LISTS = ("recall_list", "recall_nogc_list", "zeroshot_recall_list")


def _limits():
    c, m = ctypes.c_int32(), ctypes.c_int32()
    assert native.load_library().veto_sgg_eval_fold_limits(ctypes.byref(c), ctypes.byref(m)) == 0
    return c.value, m.value


C_IMG, MAX_CLS = _limits()
FOLD_CASES = sorted(sc.fold_cases(C_IMG, MAX_CLS))


def _evaluator(mode, num_rel, zeroshot=None, **kw):
    from veto_amd.evaluation import SGGEvaluator
    return SGGEvaluator(mode, num_rel, np.zeros((0, 3), np.int64) if zeroshot is None else zeroshot, device=DEV, **kw)


def _bits(res):
    """Every number of a finalize() result as bytes (NaN payloads included)."""
    flat = [float(res["images_evaluated"]), float(res["images_with_zeroshot"])]
    for k in KS:
        flat += [res[n][k] for n in sc.SCALARS]
        for n in LISTS + IMAGE_LISTS:
            flat += [float(len(res[n][k]))] + list(res[n][k])
    return np.asarray(flat, np.float64).tobytes()


def _close(got, ref, tol=1e-12, image_lists=True, show=None):
    """Scalars, per-class lists and per-image lists within tol (NaN where the reference has NaN); returns the largest error."""
    worst = 0.0
    for k in KS:
        pairs = [(n, got[n][k], ref[n][k]) for n in sc.SCALARS]
        for n in LISTS + (IMAGE_LISTS if image_lists else ()):
            assert len(got[n][k]) == len(ref[n][k]), (n, k, len(got[n][k]), len(ref[n][k]))
            pairs += [(n, x, y) for x, y in zip(got[n][k], ref[n][k])]
        for n, x, y in pairs:
            if np.isnan(y):
                assert np.isnan(x), (n, k)
            else:
                worst = max(worst, abs(x - y))
    if show:
        print("%s: largest error %.3e" % (show, worst))
    assert worst < tol, worst
    return worst


def _feed(ev, images, sizes):
    i = 0
    for n in sizes:
        assert ev.accumulate(images[i:i + n]) is None
        i += n
    assert i == len(images)
    return ev


def _fold(rec, num_rel, mode):
    """The fold alone: hand-made records loaded as a state, then finalize()."""
    ev = _evaluator(mode, num_rel, reserve=16)
    ev.load_state([{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rec.items()}])
    return ev.finalize()


# ---- end to end against the oracle over the whole split ----------------------------------------------------------------------
@pytest.mark.parametrize("mode,num_rel", [("sgcls", 51), ("predcls", 101), ("sgdet", 51)])
def test_split_in_batches_of_12_matches_the_oracle(mode, num_rel):
    images, zeroshot = sc.split_images(mode, num_rel)
    ref = dict(sc.split_oracle(mode, num_rel))
    n = len(images)
    ev = _evaluator(mode, num_rel, zeroshot, reserve=16)      # 16 rows: the buffers are re-allocated several times
    _feed(ev, images, [12] * (n // 12) + ([n % 12] if n % 12 else []))
    assert ev._rec.shape[1] > 16 * 8 and ev._rows == sum(len(im["gt_rels"]) for im in images)
    res = ev.finalize()
    if mode == "sgdet":      # sgg_eval.py:356: SGPairAccuracy records nothing
        ref["accuracy"] = {k: float("nan") for k in KS}
    _close(res, ref, show="split %s/%d vs oracle" % (mode, num_rel))
    assert res["images_evaluated"] == sum(r is not None for r in ref["per_image"]) == n
    assert res["images_with_zeroshot"] == sum(bool(r["zeroshot"].any()) for r in ref["per_image"]) > 0
    assert 0.1 < res["recall"][20] < res["recall"][100] < 0.95 and res["mean_recall"][100] > 0.1
    assert "R @ 20: %.4f" % res["recall"][20] in ev.generate_print_string(res)
    if mode == "sgdet":
        assert "A @ 20: nan" in ev.generate_print_string(res)


# ---- the same records, whatever produced them: the same bits -------------------------------------------------------------------
def test_partitions_of_one_split_agree_bit_for_bit():
    images, zeroshot = sc.split_images("sgcls", 51)
    images = [dict(im) for im in images[:4 * C_IMG + 2]]
    images[5]["gt_rels"] = np.zeros((0, 3), np.int64)                                                      # G == 0
    images[C_IMG]["pred_rel_inds"], images[C_IMG]["rel_scores"] = np.zeros((0, 2), np.int64), np.zeros((0, 51), np.float32)      # P == 0
    n = len(images)
    uneven = [1, 30, 2, 17, 5]
    uneven += [n - sum(uneven)]
    results = {}
    for name, sizes, reserve in (("one batch", [n], 4096), ("batches of 1", [1] * n, 16), ("batches of 12", [12] * (n // 12) + [n % 12], 16),
                                 ("uneven", uneven, 100)):
        ev = _feed(_evaluator("sgcls", 51, zeroshot, reserve=reserve), images, sizes)
        results[name] = ev.finalize()
        assert _bits(ev.finalize()) == _bits(results[name]), name                                             # finalize() keeps the records
    half = n // 2 + 3
    a = _feed(_evaluator("sgcls", 51, zeroshot, reserve=16), images[:half], [half])
    b = _feed(_evaluator("sgcls", 51, zeroshot), images[half:], [7, n - half - 7])
    merged = _evaluator("sgcls", 51, zeroshot, reserve=16)
    merged.load_state([a.state(), b.state()])
    results["two halves merged"] = merged.finalize()
    cpu_states = [{k: v.cpu() for k, v in st.items()} for st in (a.state(), b.state())]                      # as a gloo exchange hands them over
    merged.load_state(cpu_states)
    results["two halves merged from host tensors"] = merged.finalize()
    want = _bits(results["one batch"])
    for name, res in results.items():
        assert _bits(res) == want, name
    assert results["one batch"]["images_evaluated"] == n - 2
    st = merged.state()
    assert st["gt_count"].tolist() == [len(im["gt_rels"]) for im in images] and st["pair_count"][C_IMG] == 0
    assert all(st[k].dtype == torch.int32 and st[k].numel() == int(st["gt_count"].sum()) for k in sc.FIELDS)
    # ... and they are the right numbers
    ref = sc.np_fold(sc.concat_records([{k: v.cpu().numpy() for k, v in st.items()}]), 51, "sgcls")
    _close(results["one batch"], ref)


# ---- the fold alone on hand-made records -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FOLD_CASES)
def test_fold_on_hand_made_records(name):
    rec, num_rel, mode = sc.fold_cases(C_IMG, MAX_CLS)[name]
    res = _fold(rec, num_rel, mode)
    ref = sc.np_fold(rec, num_rel, mode)
    assert res["images_evaluated"] == ref["images_evaluated"] and res["images_with_zeroshot"] == ref["images_with_zeroshot"]
    _close(res, ref, show="fold %s vs restatement" % name)
    for n in IMAGE_LISTS:      # a quotient with one image behind it: exact
        for k in KS:
            assert res[n][k] == ref[n][k], (n, k)
    if ref["images_evaluated"] == 1:
        for k in KS:
            assert all(res[n][k] == ref[n][k] or (np.isnan(res[n][k]) and np.isnan(ref[n][k])) for n in sc.SCALARS[:4])
            assert res["mean_recall_list"][k] == ref["mean_recall_list"][k] and res["ng_mean_recall_list"][k] == ref["ng_mean_recall_list"][k]
    # the documented summation order: chunks of images_per_chunk in image order, the chunk sums in chunk order -- the same bits
    want = sc.np_fold_chunked(rec, num_rel, mode, C_IMG)
    for k in KS:
        for n in sc.SCALARS:
            assert np.float64(res[n][k]).tobytes() == np.float64(want[n][k]).tobytes() or (np.isnan(res[n][k]) and np.isnan(want[n][k])), (n, k)
        for n in LISTS:
            assert res[n][k] == want[n][k], (n, k)


def test_fold_cases_show_what_they_are_named_for():
    cases = sc.fold_cases(C_IMG, MAX_CLS)
    r = _fold(*cases["ranks_at_k"])      # ranks 19 / 20, 49 / 50, 99 / 100: rank < K
    assert r["recall"] == {20: 2 / 8, 50: 4 / 8, 100: 6 / 8} and r["recall_nogc"] == r["recall"] and r["accuracy"] == r["recall"]
    assert r["mean_recall_list"][100] == [1.0, 1.0, 0.5, 0.5, 0.0] and r["mean_recall"][100] == 3.0 / 5      # predicate 5: no image has it
    r = _fold(*cases["no_zeroshot"])
    assert r["images_with_zeroshot"] == 0 and all(np.isnan(r["zeroshot_recall"][k]) and r["zeroshot_recall_list"][k] == [] for k in KS)
    r = _fold(*cases["all_unevaluated"])
    assert r["images_evaluated"] == 0 and np.isnan(r["recall"][20]) and np.isnan(r["accuracy"][50]) and r["mean_recall"][100] == 0.0
    assert r["recall_list"][20] == [] and r["mean_recall_list"][20] == [0.0] * 50
    r = _fold(*cases["sgdet"])
    assert all(np.isnan(r["accuracy"][k]) for k in KS) and r["images_evaluated"] == 2 * C_IMG + 2
    rec, num_rel, mode = cases["predicate_outside"]      # they count for R, ngR, zR and A, and for no class
    inside = sc.concat_records([rec])
    keep = (inside["gt_predicate"] >= 1) & (inside["gt_predicate"] < num_rel)
    r = _fold(rec, num_rel, mode)
    assert r["recall_list"][100][0] == float((rec["gc_rank"][:40] < 100).sum()) / 40.0 and not keep[:40].all()
    only = {k: (v[keep] if k in sc.FIELDS else v.copy()) for k, v in inside.items()}
    only["gt_count"] = np.array([int(keep[:40].sum()), 6])
    assert _fold(only, num_rel, mode)["mean_recall_list"] == r["mean_recall_list"]


# ---- the existing host path ------------------------------------------------------------------------------------------------
def test_accumulate_agrees_with_update_and_the_host_fold():
    images, zeroshot = sc.split_images("predcls", 101)
    images = [dict(im) for im in images[:60]]
    images[7]["gt_rels"] = np.zeros((0, 3), np.int64)
    dev_ev, host_ev = _evaluator("predcls", 101, zeroshot, reserve=16), _evaluator("predcls", 101, zeroshot)
    for i in range(0, 60, 12):
        assert dev_ev.accumulate(images[i:i + 12]) is None
        assert host_ev.update(images[i:i + 12])["images_evaluated"] in (11, 12)
    got, ref = dev_ev.finalize(), host_ev.finalize()
    assert got["images_evaluated"] == ref["images_evaluated"] == 59 and got["images_with_zeroshot"] == ref["images_with_zeroshot"]
    _close(got, ref, show="accumulate vs update + host fold")
    assert sorted(got) == sorted(ref)      # the same keys
    assert dev_ev.generate_print_string(got).count("\n") == 6


# ---- the API -----------------------------------------------------------------------------------------------------------------
def test_api_mixing_reset_empty_and_boxlists():
    from veto_amd.structures import BoxList
    images, zeroshot = sc.split_images("sgcls", 51)
    images = images[:6]
    ev = _evaluator("sgcls", 51, zeroshot, reserve=16)
    empty = ev.finalize()      # nothing fed at all
    assert empty["images_evaluated"] == 0 and np.isnan(empty["recall"][20]) and empty["mean_recall"][100] == 0.0
    assert ev.accumulate(images[:3]) is None
    with pytest.raises(ValueError, match="reset"):
        ev.update(images[3:])
    assert ev.finalize()["images_evaluated"] == 3      # the refused call left nothing behind
    ev.reset()
    assert ev._rows == 0 and ev._rec is None and ev._img_g == []
    assert ev.finalize()["images_evaluated"] == 0
    ev.update(images[:3])
    with pytest.raises(ValueError, match="reset"):
        ev.accumulate(images[3:])
    with pytest.raises(ValueError, match="reset"):
        ev.state()
    assert ev.finalize()["images_evaluated"] == 3
    ev.reset()
    assert ev.accumulate([]) is None      # a rank without an image: fed, and empty
    r = ev.finalize()
    assert r["images_evaluated"] == 0 and np.isnan(r["recall"][50]) and np.isnan(r["zeroshot_recall"][50]) and np.isnan(r["accuracy"][50])
    assert r["mean_recall"] == {20: 0.0, 50: 0.0, 100: 0.0} and r["mean_recall_list"][20] == [0.0] * 50 and r["recall_list"][20] == []
    assert "R @ 20: nan" in ev.generate_print_string(r)
    st = ev.state()
    assert all(st[k].numel() == 0 for k in st)
    # the BoxList form takes what update_boxlists takes and gives accumulate()'s numbers
    ev.reset()
    ev.accumulate(images)
    want = _bits(ev.finalize())
    gts, preds = [], []
    for im in images:
        g = BoxList(torch.from_numpy(im["gt_boxes"]), (400, 400))
        g.add_field("relation_tuple", torch.from_numpy(im["gt_rels"]))
        g.add_field("labels", torch.from_numpy(im["gt_classes"]))
        p = BoxList(torch.from_numpy(im["pred_boxes"]), (400, 400))
        for field, key in (("rel_pair_idxs", "pred_rel_inds"), ("pred_rel_scores", "rel_scores"), ("pred_labels", "pred_classes"),
                           ("pred_scores", "obj_scores")):
            p.add_field(field, torch.from_numpy(np.ascontiguousarray(im[key])))
        gts.append(g.to(DEV))
        preds.append(p.to(DEV))
    ev.reset()
    assert ev.accumulate_boxlists(gts[:4], preds[:4]) is None and ev.accumulate_boxlists(gts[4:], preds[4:]) is None
    assert _bits(ev.finalize()) == want
