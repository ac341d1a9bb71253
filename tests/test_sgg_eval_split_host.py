"""Split-level relation evaluation, the premises on the CPU (no GPU): the numpy restatement the device is compared with
(tests/sgg_eval_split_cases.py) against the oracle and against the existing host fold, four wrong restatements that the cases
must expose, the chunk-ordered restatement, and the argument checks of veto_sgg_eval_fold."""
import ctypes
import types

import numpy as np
import pytest

import sgg_eval_split_cases as sc
from veto_amd import native

KS = sc.KS


def _same(a, b, tol):
    """Largest difference over every scalar and per-class list entry (NaN equals NaN); the counts must be equal."""
    assert a["images_evaluated"] == b["images_evaluated"] and a["images_with_zeroshot"] == b["images_with_zeroshot"]
    worst = 0.0
    for k in KS:
        pairs = [(a[n][k], b[n][k]) for n in sc.SCALARS]
        for n in ("mean_recall_list", "ng_mean_recall_list"):
            assert len(a[n][k]) == len(b[n][k])
            pairs += list(zip(a[n][k], b[n][k]))
        for x, y in pairs:
            if np.isnan(x) or np.isnan(y):
                assert np.isnan(x) and np.isnan(y)
            else:
                worst = max(worst, abs(x - y))
    assert worst <= tol, worst
    return worst


def _limits():
    lib = native.load_library()
    c, m = ctypes.c_int32(), ctypes.c_int32()
    assert lib.veto_sgg_eval_fold_limits(ctypes.byref(c), ctypes.byref(m)) == 0
    assert lib.veto_sgg_eval_fold_limits(None, None) == 0
    return c.value, m.value


@pytest.mark.parametrize("mode,num_rel", [("sgcls", 51), ("predcls", 101)])
def test_restatement_equals_the_oracle_on_the_seeded_split(mode, num_rel):
    images, _ = sc.split_images(mode, num_rel)
    ref = sc.split_oracle(mode, num_rel)
    rec = sc.records_from_oracle(images, ref["per_image"])
    assert rec["gt_count"].sum() == 7312 and rec["gt_count"].min() == 4 and rec["gt_count"].max() == 25
    got = sc.np_fold(rec, num_rel, mode)
    _same(got, ref | {"images_evaluated": 520, "images_with_zeroshot": got["images_with_zeroshot"]}, 1e-12)
    assert 516 <= got["images_with_zeroshot"] <= 518
    assert all(v > 0.0 for v in got["mean_recall_list"][100])      # every class present and hit somewhere
    for name in ("recall_list", "recall_nogc_list", "zeroshot_recall_list"):
        for k in KS:
            assert got[name][k] == ref[name][k]
    # ... and in the device's summation order the same numbers within the bound of two fixed-order sums of <= 600 terms
    c, _ = _limits()
    _same(sc.np_fold_chunked(rec, num_rel, mode, c), got, 1e-12)


def _host_fold(rec, num_rel, mode):
    """The evaluator's own host fold (SGGEvaluator.finalize) on a stand-in that holds what update() would have kept."""
    from veto_amd.evaluation import SGGEvaluator
    acc = []
    for G, P, sl in sc._images_of(rec):
        if G and P:
            acc.append((rec["gc_rank"][sl].astype(np.int64), rec["ng_rank"][sl].astype(np.int64), rec["acc_rank"][sl].astype(np.int64),
                        rec["zeroshot_flag"][sl] != 0, rec["gt_predicate"][sl].astype(np.int64)))
    return SGGEvaluator.finalize(types.SimpleNamespace(_acc=acc, num_rel=num_rel, mode=mode))


def test_restatement_equals_the_existing_host_fold():
    c, max_cls = _limits()
    n = 0
    for name, (rec, num_rel, mode) in sc.fold_cases(c, max_cls).items():
        if name == "predicate_outside":      # the host fold's np.bincount takes predicates 0..C-1 only
            continue
        _same(sc.np_fold(rec, num_rel, mode), _host_fold(rec, num_rel, mode), 0.0)
        n += 1
    assert n >= 12
    images, _ = sc.split_images("sgcls", 51)
    rec = sc.records_from_oracle(images, sc.split_oracle("sgcls", 51)["per_image"])
    _same(sc.np_fold(rec, 51, "sgcls"), _host_fold(rec, 51, "sgcls"), 0.0)


def test_chunked_restatement_equals_the_plain_one_on_every_case():
    c, max_cls = _limits()
    for name, (rec, num_rel, mode) in sc.fold_cases(c, max_cls).items():
        _same(sc.np_fold_chunked(rec, num_rel, mode, c), sc.np_fold(rec, num_rel, mode), 1e-12)


@pytest.mark.parametrize("mutation,case,key", [("acc_ratio_mean", "image_sizes", "accuracy"),
                                               ("class_all_images", "n_img_3", "mean_recall"),
                                               ("zeroshot_all_images", "zs_sparse", "zeroshot_recall"),
                                               ("le_k", "ranks_at_k", "recall")])
def test_wrong_restatements_change_a_result(mutation, case, key):
    c, max_cls = _limits()
    cases = sc.fold_cases(c, max_cls)
    cases["n_img_3"] = (sc.random_split(5, "n3", [4, 2, 6], 51), 51, "sgcls")
    cases["zs_sparse"] = (sc.random_split(5, "zs", [1, 2, 1, 9, 1], 51, zs_frac=0.2), 51, "sgcls")
    rec, num_rel, mode = cases[case]
    good, bad = sc.np_fold(rec, num_rel, mode), sc.np_fold(rec, num_rel, mode, mutation=mutation)
    assert any(abs(good[key][k] - bad[key][k]) > 1e-6 for k in KS), (good[key], bad[key])
    if mutation == "le_k":      # ranks 20 / 50 / 100 exactly: every K and every list moves
        for k in KS:
            assert good["recall"][k] != bad["recall"][k] and good["recall_nogc"][k] != bad["recall_nogc"][k]
            assert good["accuracy"][k] != bad["accuracy"][k]


def test_hand_made_cases_hold_what_they_are_named_for():
    c, max_cls = _limits()
    cases = sc.fold_cases(c, max_cls)
    assert sorted(len(cases["n_img_%d" % n][0]["gt_count"]) for n in (1, c - 1, c, c + 1, 2 * c + 1)) == [1, c - 1, c, c + 1, 2 * c + 1]
    rec = cases["unevaluated_whole_chunk"][0]
    assert all(g == 0 or p == 0 for g, p in zip(rec["gt_count"][c:2 * c], rec["pair_count"][c:2 * c]))
    rec = cases["unevaluated_first_last"][0]
    assert rec["gt_count"][0] == 0 and rec["pair_count"][1] == 0 and rec["gt_count"][1] > 0 and rec["gt_count"][-1] == 0
    assert sc.np_fold(*cases["all_unevaluated"])["images_evaluated"] == 0
    assert list(cases["image_sizes"][0]["gt_count"][:5]) == [1, 63, 64, 65, 3000]
    r = sc.np_fold(*cases["ranks_at_k"])
    assert r["recall"] == {20: 2 / 8, 50: 4 / 8, 100: 6 / 8} and r["mean_recall_list"][100][4] == 0.0
    r = sc.np_fold(*cases["no_zeroshot"])
    assert r["images_with_zeroshot"] == 0 and np.isnan(r["zeroshot_recall"][50])
    assert cases["two_classes"][1] == 2 and cases["max_classes"][1] == max_cls == 1024


def test_fold_refuses_bad_arguments_without_a_gpu():
    lib = native.load_library()
    c, max_cls = _limits()
    assert c >= 1 and max_cls == 1024
    assert ctypes.sizeof(native.VetoSggEvalFoldArgs) == 6 * 4 + 9 * 8

    def args(**kw):
        a = native.VetoSggEvalFoldArgs()
        a.struct_size = ctypes.sizeof(native.VetoSggEvalFoldArgs)
        a.n_img, a.n_rel_cls, a.mode, a.n_gt_total = 3, 51, 0, 9
        for f in ("img_gt_offset", "img_pair_count", "gt_predicate", "gc_rank", "ng_rank", "acc_rank", "zeroshot_flag", "metrics"):
            setattr(a, f, 256)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    ws, big = ctypes.c_void_p(256), 1 << 40
    need = lib.veto_sgg_eval_fold_workspace_bytes(3, 51)
    assert need >= (16 + 7 * 51) * 8 and need % 256 == 0
    assert lib.veto_sgg_eval_fold_workspace_bytes(c + 1, 51) > need      # a second chunk, a second row of partials
    for bad in ((-1, 51), (3, 1), (3, max_cls + 1)):
        assert lib.veto_sgg_eval_fold_workspace_bytes(*bad) == 0
    assert lib.veto_sgg_eval_fold(None, None, ws, big) == -1 and b"null argument" in lib.veto_last_error()
    for kw, needle in ((dict(struct_size=8), b"size mismatch"), (dict(n_rel_cls=1), b"n_rel_cls"), (dict(n_rel_cls=max_cls + 1), b"n_rel_cls"),
                       (dict(mode=2), b"mode"), (dict(n_img=-1), b"bad sizes"), (dict(n_gt_total=-1), b"bad sizes"),
                       (dict(img_gt_offset=None), b"missing pointer"), (dict(img_pair_count=None), b"missing pointer"),
                       (dict(gt_predicate=None), b"missing pointer"), (dict(gc_rank=None), b"missing pointer"),
                       (dict(ng_rank=None), b"missing pointer"), (dict(acc_rank=None), b"missing pointer"),
                       (dict(zeroshot_flag=None), b"missing pointer"), (dict(metrics=None), b"missing pointer")):
        assert lib.veto_sgg_eval_fold(None, ctypes.byref(args(**kw)), ws, big) == -1, kw
        assert needle in lib.veto_last_error(), (kw, lib.veto_last_error())
    for w, nbytes in ((ws, need - 1), (None, big), (ctypes.c_void_p(264), big)):      # short, missing, misaligned
        assert lib.veto_sgg_eval_fold(None, ctypes.byref(args()), w, nbytes) == -4
        assert b"workspace" in lib.veto_last_error()


def test_evaluator_refuses_a_cpu_device_before_anything_else():
    from veto_amd.evaluation import SGGEvaluator
    with pytest.raises(RuntimeError, match="HIP device"):
        SGGEvaluator("predcls", 51, np.zeros((0, 3), np.int64), device="cpu", reserve=16)
