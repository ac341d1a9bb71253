"""What the device comparison of tests/test_deterministic_gpu.py rests on, proved on the CPU for every input it uses
(tests/deterministic_cases.py):

(a) each float32 restatement of an ordered sum lies within the any-order bound of the existing oracles: oracle/roi_align_oracle.py's
    backward with its K and sum |term| (tests/roi_pool_cases.py::backward_bound), and gamma_K x sum |term| around a float64 sum for the
    two scatter sites;
(b) the order matters: the same restatement with the ROIs / pairs / object rows walked in DESCENDING order differs in at least one bit,
    so a bit match on the device means the stated order, and the atomic path cannot pass by luck.  Exempt, by arithmetic: the inputs
    marked exact, and those where no destination receives three terms (two terms commute);
(c) the inputs marked exact have order-free float32 answers.
Plus the plumbing that needs no device: the opts field, the size query's refusal without a handle, the Python knob."""
import ctypes

import numpy as np
import pytest

import deterministic_cases as dc
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
U = 2.0 ** -24


def _bits_differ(a, b):
    return bool((np.asarray(a, dtype=F).view(np.int32) != np.asarray(b, dtype=F).view(np.int32)).any())


# ---- ROI pooling -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def roi_results():
    return {}


def _roi(name, roi_results):
    if name not in roi_results:
        case = dc.ROI_CASES[name]()
        roi_results[name] = (case, dc.pooler_backward_ordered(case), dc.pooler_backward_ordered(case, reverse=True))
    return roi_results[name]


@pytest.mark.parametrize("name", sorted(dc.ROI_CASES))
def test_roi_restatement_is_within_the_any_order_bound_and_its_order_matters(name, roi_results):
    case, (levels, dep), (levels_rev, dep_rev) = _roi(name, roi_results)
    per_level, dep_ref = _oracle(case)
    worst, touched = 0.0, 0
    for got, (want, K, A) in zip(levels + ([dep] if dep is not None else []), per_level + ([dep_ref] if dep_ref is not None else [])):
        ratio, _ = rc.check_backward(got, want, K, A)      # (a); asserts exact zeros where nothing lands
        worst, touched = max(worst, ratio), touched + int((K > 0).sum())
        if case.exact:                                    # (c)
            assert np.array_equal(got.astype(np.float64), want)
    assert worst <= 1.0 and touched > 0, (name, worst)
    differs = any(_bits_differ(a, b) for a, b in zip(levels, levels_rev)) or (dep is not None and _bits_differ(dep, dep_rev))
    assert differs != case.exact, name                    # (b); an exact input gives the same bits in every order
    print("deterministic_host: roi %-22s error / any-order bound %.3f  pixels touched %d  descending order %s"
          % (name, worst, touched, "differs" if differs else "equal (exact input)"))


def _oracle(case):
    """oracle/roi_align_oracle.py's backward (float64 accumulation, K, sum |term|) per map: ([(grad, K, A) per level], the depth map's or None)."""
    lv = dc.pooler_levels(case.rois, case.scales)
    per_level = []
    for l, (shape, sc) in enumerate(zip(case.shapes, case.scales)):
        idx = np.nonzero(lv == l)[0]
        per_level.append(ro.roi_align_backward(case.g_rgb[idx], case.rois[idx], sc, shape, case.pooled, case.ratio, stats=True))
    dep = None
    if case.g_dep is not None:
        sc = case.scales[2] if len(case.scales) > 1 else case.scales[0]
        dep = ro.roi_align_backward(case.g_dep, case.rois, sc, case.depth_shape, case.pooled, case.ratio, stats=True)
    return per_level, dep


def test_roi_cases_cover_what_they_are_named_for():
    far = dc.ROI_CASES["far_edge"]()
    H, W = far.shapes[0][2:]
    coincide = 0
    for roi in far.rois:
        (vy, ylo, yhi, _, _), (vx, xlo, xhi, _, _) = rc.roi_tables(roi, 1.0, far.pooled, far.ratio, H, W)
        coincide += int((vy & (ylo == yhi)).sum()) + int((vx & (xlo == xhi)).sum())
    assert coincide >= 4                                   # valid samples whose low and high index are both size - 1
    b = dc.ROI_CASES["level_boundaries"]()
    assert set(dc.pooler_levels(b.rois, b.scales).tolist()) == {0, 1, 2, 3}
    lv64 = rc.map_levels_f64(b.rois[:, 1:])
    assert (lv64 != dc.pooler_levels(b.rois, b.scales)).any()      # boxes that only the float32 LevelMapper puts where the device does
    e = dc.ROI_CASES["empty_image"]()
    assert sorted(set(e.rois[:, 0].astype(int).tolist())) == [0, 2, 4] and e.shapes[0][0] == 5
    for n_levels in (4, 3):
        c = dc.ROI_CASES["levels%d_depth" % n_levels]()
        assert set(dc.pooler_levels(c.rois, c.scales).tolist()) == set(range(n_levels))
    assert [dc.ROI_CASES[k]().shapes[0][1] for k in ("channels1", "channels32", "ratio2", "channels65")] == [1, 32, 33, 65]
    assert [dc.ROI_CASES["ratio%d" % g]().ratio for g in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [dc.ROI_CASES[k]().pooled for k in ("pooled1", "pooled7", "ratio2")] == [1, 7, 8]


# ---- the two scatter sites ---------------------------------------------------------------------------------------------------------------
def _any_order_check(got, want64, abs64, count):
    """|float32 sum in some order - exact sum| <= gamma_K x sum |term| (K = the number of terms of the element), one rounding included."""
    K = np.asarray(count, dtype=np.float64)
    bound = K * U / (1.0 - K * U) * abs64 + U * np.abs(want64)
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= bound).all()
    assert not got[np.broadcast_to(K == 0, got.shape)].any()
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("name", sorted(dc.ASSEMBLE_CASES))
def test_assemble_restatement_is_within_the_any_order_bound_and_its_order_matters(name):
    c = dc.ASSEMBLE_CASES[name]()
    dpatch, dlc = dc.assemble_backward_ordered(c.dx, c.subj, c.obj, c.lc, c.n_obj)
    want_p, abs_p = np.zeros(dpatch.shape), np.zeros(dpatch.shape)
    want_l, abs_l = np.zeros(dlc.shape), np.zeros(dlc.shape)
    cnt = np.zeros((c.n_obj, 1, 2))
    dx64 = c.dx.astype(np.float64)
    for p in range(c.n_pair):
        s, o = int(c.subj[p]), int(c.obj[p])
        gate = (c.lc[s, :, :dc.DIM] + c.lc[o, :, dc.DIM:]) > 0
        for dst, half, n in ((slice(0, dc.DIM), 0, s), (slice(dc.DIM, None), 1, o)):
            want_p[n, :, dst] += dx64[p, 1:17]
            abs_p[n, :, dst] += np.abs(dx64[p, 1:17])
            want_l[n, :, dst] += np.where(gate, dx64[p, 17:19], 0.0)
            abs_l[n, :, dst] += np.where(gate, np.abs(dx64[p, 17:19]), 0.0)
            cnt[n, 0, half] += 1
    K = np.repeat(cnt, dc.DIM, axis=2)
    worst = max(_any_order_check(dpatch, want_p, abs_p, K), _any_order_check(dlc, want_l, abs_l, K))      # (a)
    assert worst <= 1.0
    rev = dc.assemble_backward_ordered(c.dx, c.subj, c.obj, c.lc, c.n_obj, reverse=True)
    differs = _bits_differ(dpatch, rev[0]) and _bits_differ(dlc, rev[1])
    assert (cnt.max() <= 2) == c.single_term
    assert differs != c.single_term, name                                                                    # (b)
    print("deterministic_host: assemble %-18s pairs %4d  most terms per destination %4d  error / any-order bound %.3f  descending order %s"
          % (name, c.n_pair, int(cnt.max()), worst, "differs" if differs else "equal (no destination has three terms)"))


def test_assemble_cases_cover_what_they_are_named_for():
    hand = dc.ASSEMBLE_CASES["hand_pairs"]()
    assert 2 not in set(hand.subj.tolist()) | set(hand.obj.tolist())                        # a gap
    assert 4 in hand.obj.tolist() and 4 not in hand.subj.tolist()                           # one-sided
    assert sum(1 for s, o in zip(hand.subj, hand.obj) if (s, o) == (0, 1)) == 2             # a repeated pair
    assert hand.pair_off.tolist() == [0, 9, 10] and hand.obj_off.tolist() == [0, 6, 9]
    assert [dc.ASSEMBLE_CASES["pairs%d" % n]().n_pair for n in (1, 15, 16, 17)] == [1, 15, 16, 17]
    one = dc.ASSEMBLE_CASES["one_subject_1024"]()
    assert one.n_pair == 1024 and set(one.subj.tolist()) == {0}
    two = dc.ASSEMBLE_CASES["two_images"]()
    assert two.obj_off[1] > 0 and two.pair_off[1] > 0 and two.subj[two.pair_off[1]:].min() >= two.obj_off[1]


@pytest.mark.parametrize("name", sorted(dc.SCATTER_CASES))
def test_scatter_restatement_is_within_the_any_order_bound_and_its_order_matters(name):
    c = dc.SCATTER_CASES[name]()
    got = dc.scatter_rows_ordered(c.demb, c.labels, c.n_table_rows)
    want, absum = np.zeros(got.shape), np.zeros(got.shape)
    np.add.at(want, c.labels, c.demb.astype(np.float64))
    np.add.at(absum, c.labels, np.abs(c.demb.astype(np.float64)))
    K = np.bincount(c.labels, minlength=c.n_table_rows)[:, None]
    worst = _any_order_check(got, want, absum, np.broadcast_to(K, got.shape))                # (a)
    assert worst <= 1.0
    differs = _bits_differ(got, dc.scatter_rows_ordered(c.demb, c.labels, c.n_table_rows, reverse=True))
    assert (K.max() <= 2) == c.single_term and differs != c.single_term, name                # (b)
    print("deterministic_host: scatter %-20s rows %d  width %d  most rows per label %d  error / any-order bound %.3f  descending order %s"
          % (name, len(c.labels), c.dim, int(K.max()), worst, "differs" if differs else "equal"))


def test_scatter_cases_cover_what_they_are_named_for():
    one = dc.SCATTER_CASES["one_label_432_rows"]()
    assert len(one.labels) == 432 and len(set(one.labels.tolist())) == 1 and one.dim == 200
    d = dc.SCATTER_CASES["all_distinct"]()
    assert len(set(d.labels.tolist())) == len(d.labels)


# ---- plumbing that needs no device ------------------------------------------------------------------------------------------------------
def test_opts_field_and_size_query_without_a_device():
    from veto_amd import native
    lib = native.load_library()
    o = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts), deterministic=1)
    assert native.VetoTrainOpts.deterministic.offset == 40 and ctypes.sizeof(native.VetoTrainOpts) == 48      # appended: the old struct was 40 bytes
    assert lib.veto_train_workspace_bytes_opts(None, 10, 90, ctypes.byref(o)) == 0                             # no handle
    assert lib.veto_debug_wgrad_ordered_workspace_bytes(1000, 64, 192, 3) == \
        lib.veto_debug_wgrad_workspace_bytes(1000, 64, 192, 3) + 3 * 64 * 192 * 4                              # the planes, nothing else
    assert lib.veto_debug_wgrad_ordered_workspace_bytes(0, 64, 192, 3) == 0


def test_python_knob_sources(monkeypatch):
    import torch
    from veto_amd import config, native
    assert config.default_config().VETO_AMD.DETERMINISTIC is False
    monkeypatch.setattr(native, "_ENV_DETERMINISTIC", False)
    assert native.ordered_mode(False) is False and native.ordered_mode(True) is True
    torch.use_deterministic_algorithms(True)
    try:
        assert native.ordered_mode(False) is True
    finally:
        torch.use_deterministic_algorithms(False)
    monkeypatch.setattr(native, "_ENV_DETERMINISTIC", None)
    monkeypatch.setenv("VETO_DETERMINISTIC", "1")
    assert native.ordered_mode(False) is True
    monkeypatch.setattr(native, "_ENV_DETERMINISTIC", None)      # (the next caller of this process reads the environment again)
