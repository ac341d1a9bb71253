"""The relation-loss cases of tests/ce_loss_cases.py on the CPU: the float64 restatement is torch's cross entropy in float64 on every
case torch accepts; every case causes the event it is named for; a float32 numpy emulation of the kernels' arithmetic stays inside
the derived bounds (they are attainable); each deliberately wrong restatement leaves a bound by at least 10x on some case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_loss_cases as cc  # noqa: E402

NAMES = cc.names()
ref_and_bounds = cc.ref_and_bounds


def test_the_case_table_is_the_one_the_suite_promises():
    assert [n for n in NAMES if n.startswith("width_")] == ["width_%d" % C for C in cc.WIDTHS]
    assert [n for n in NAMES if n.startswith("rows_") and n[5:].isdigit()] == ["rows_%d" % n for n in cc.ROW_COUNTS]
    assert [n for n in NAMES if n.startswith("offset_")] == ["offset_%g" % o for o in cc.OFFSETS]
    assert len(NAMES) == len(set(NAMES)) and all(cc.cases()[n]["event"] for n in NAMES)
    assert max(cc.selected(c).size for c in cc.cases().values()) == cc.FOLD_ROWS * 51        # the largest input


@pytest.mark.parametrize("name", NAMES)
def test_the_fp64_restatement_is_torch_cross_entropy(name):
    """Loss and gradient against torch.nn.functional.cross_entropy in float64 (every negative label handed to torch as -100), NaN and
    inf in the same places.  torch raises on a label >= C: those two cases are decided by the restatement alone, and are held to what
    the header promises (NaN loss, NaN row, every other row as if the bad row were ignored)."""
    c, r, _ = ref_and_bounds(name)
    y = np.where(c["labels"] < 0, -100, c["labels"])
    if r["bad"].any():
        assert np.isnan(r["loss"]) and np.isnan(r["grad"][r["bad"]]).all()
        y = np.where(r["bad"], -100, y)
    z = torch.from_numpy(cc.selected(c).astype(np.float64)).requires_grad_()
    w = None if c["weight"] is None else torch.from_numpy(c["weight"].astype(np.float64))
    loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(y), weight=w, ignore_index=-100)
    loss.backward()
    g = z.grad.numpy()
    keep = ~r["bad"]
    assert np.array_equal(np.isnan(g[keep]), np.isnan(r["grad"][keep])) and not np.isinf(g).any() and not np.isinf(r["grad"]).any()
    fin = np.isfinite(r["grad"]) & keep[:, None]
    scale = max(np.abs(g[fin]).max(), 2.0 ** -126) if fin.any() else 1.0
    assert np.abs(g[fin] - r["grad"][fin]).max(initial=0.0) <= 1e-12 * scale
    assert not g[r["ignored"]].any() and not r["grad"][r["ignored"]].any()
    if not r["bad"].any():
        t = float(loss.detach())
        assert (np.isnan(t) and np.isnan(r["loss"])) or t == r["loss"] or abs(t - r["loss"]) <= 1e-12 * abs(t), (t, r["loss"])


def _trip(col):
    return col // 64


@pytest.mark.parametrize("name", NAMES)
def test_every_case_causes_the_event_it_is_named_for(name):
    c, r, (lb, gb) = ref_and_bounds(name)
    z, y = cc.selected(c), c["labels"]
    n, C = z.shape
    count = None
    if name.startswith("width_"):
        want = cc.width_labels(C)
        assert list(y[:4]) == want and want[0] == 0 and want[1] == C - 1 and want[2] % 64 == 0 and _trip(want[2]) == _trip(C - 1)
        assert want[3] % 64 == 63 or C < 64
        assert np.isfinite(r["loss"])
        count = len(set(want))
    elif name.startswith("rows_") and name[5:].isdigit():
        per = -(-n // 256)
        assert per == {1: 1, 3: 1, 4: 1, 5: 1, 255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 15120: 60}[n]
        empty = 256 - -(-n // per)
        assert empty == {1: 255, 3: 253, 4: 252, 5: 251, 255: 1, 256: 0, 257: 127, 511: 0, 512: 0, 513: 85, 15120: 4}[n]
        assert (n % per != 0) == (n in (257, 511))                              # the last busy thread's range is cut short by n
        assert (n % 4 != 0) == (n in (1, 3, 5, 255, 257, 511, 513))            # the last workgroup has idle waves
        count = -(-n // 4)
    elif name == "fold_200003":
        t = r["w"] * r["nll"]
        assert n == cc.FOLD_ROWS and 0.9e4 < t[0] < 1.1e4 and 1.2e-3 < t[1:].min() and t[1:].max() < 1.5 * 2.0 ** -10
        exact = float(r["loss"])
        wide = float(cc.emulate(c, "f32_fold")[0])
        split = float(cc.emulate(c, "f32_fold_split")[0])
        fixed = float(cc.emulate(c, "fixed")[0])
        print("fold_200003: loss64 %.9g bound %.3g; double fold off by %.3g, float fold by %.3g (%.1f bounds), two-level float fold by %.3g (%.2f bounds)"
              % (exact, lb, abs(fixed - exact), abs(wide - exact), abs(wide - exact) / lb, abs(split - exact), abs(split - exact) / lb))
        assert abs(wide - fixed) > 10 * lb and abs(split - exact) > lb and abs(fixed - exact) <= lb
        count = n - 1
    elif name.startswith("offset_"):
        off = c["offset"]
        base = cc.offset_base()[0]
        grid = slice(0, cc.OFFSET_GRID_ROWS)
        assert np.array_equal(z[grid].astype(np.float64), base[grid].astype(np.float64) + off)        # exact in float32
        assert off == 0 or not np.array_equal(z[16:].astype(np.float64), base[16:].astype(np.float64) + off)
        count = int(np.abs(z).min() >= abs(off) - 10) * n
    elif name == "flat":
        assert (z == z[:, :1]).all() and np.allclose(r["p"], 1 / 51.0, rtol=1e-15)
        count = n
    elif name in ("gap_30", "gap_200", "subnormal_p"):
        p32 = r["p"].astype(np.float32)
        off_dom = np.delete(p32, 5, axis=1)
        on, off = y == 5, y != 5
        assert on.any() and off.any()
        if name == "gap_30":
            assert (np.float32(r["logS"]) < 2.0 ** -24).all() and (r["logS"] > 0).all() and (off_dom > 0).all()
        elif name == "gap_200":
            assert not off_dom.any() and (p32[:, 5] == 1).all() and (np.delete(r["p"], 5, axis=1) > 0).all()
        else:
            assert (off_dom > 0).all() and (off_dom < 2.0 ** -126).all()
        count = int(off.sum())
    elif name == "neginf_label":
        k = c["special_row"]
        assert np.isposinf(r["loss"]) and np.isfinite(r["grad"]).all() and r["grad"][k, y[k]] == -r["w"][k] / r["W"]
        count = int(np.isneginf(z).sum())
    elif name == "neginf_other":
        k = c["special_row"]
        col = int(np.nonzero(np.isneginf(z[k]))[0][0])
        assert np.isfinite(r["loss"]) and col != y[k] and r["grad"][k, col] == 0
        count = 1
    elif name in ("all_neginf_row", "posinf_logit"):
        k = c["special_row"]
        others = np.arange(n) != k
        assert np.isnan(r["loss"]) and np.isnan(r["grad"][k]).all() and np.isfinite(r["grad"][others]).all() and r["grad"][others].any()
        count = int(np.isinf(z[k]).sum())
    elif name == "ignored_labels":
        assert set(y[y < 0]) == {-1, -100, -2 ** 40} and np.isfinite(r["loss"])
        count = int(r["ignored"].sum())
    elif name in ("bad_label_C", "bad_label_2p40"):
        assert set(y[y >= C]) == ({C} if name == "bad_label_C" else {2 ** 40})
        assert np.isfinite(r["grad"][~r["bad"]]).all() and r["grad"][r["valid"]].any()
        count = int(r["bad"].sum())
    elif name == "all_ignored":
        assert r["ignored"].all() and np.isnan(r["loss"]) and not r["grad"].any() and set(y) == {-1, -100, -2 ** 40}
        count = n
    elif name == "zero_weight_valid":
        assert r["W"] == 0 and r["valid"].any() and r["ignored"].any() and np.isnan(r["grad"][r["valid"]]).all() and np.isnan(r["loss"])
        count = int(r["valid"].sum())
    elif name == "tiny_weight_row":
        k = int(np.nonzero(r["w"])[0][0])
        assert (r["w"] > 0).sum() == 1 and r["w"][k] == np.float32(1e-30) and r["loss"] == r["nll"][k] * r["w"][k] / r["w"][k]
        assert not r["grad"][np.arange(n) != k].any() and abs(r["grad"][k, y[k]]) > 0.1
        count = n - 1
    elif name.startswith("weight_"):
        w = c["weight"]
        if name == "weight_beta":
            assert abs(float(w.sum()) - 51) < 1e-3 and w.max() / w.min() > 100
        if name == "weight_span":
            assert w.min() == np.float32(1e-6) and w.max() == np.float32(1e3) and {0, 50} <= set(y)
        count = n
    elif name.startswith("rows_"):
        rows, m = c["rows"], c["logits"].shape[0]
        buf = cc.logits_buffer(c)
        unused = np.setdiff1d(np.arange(m), rows)
        assert c["ld"] == {"rows_perm_ld_plus3": C + 3, "rows_repeats_ld_4c": 4 * C, "rows_one_row_n_times": C + 3, "rows_len1": 4 * C}[name]
        assert np.isnan(buf[:, C:]).all() and np.isnan(buf[unused]).all() and not np.isnan(buf[np.unique(rows), :C]).any()
        if name == "rows_perm_ld_plus3":
            assert sorted(rows) == list(range(m)) and not np.array_equal(rows, np.arange(m))
            count = m
        elif name == "rows_repeats_ld_4c":
            count = len(rows) - len(np.unique(rows))
            assert len(unused) > 0
        elif name == "rows_one_row_n_times":
            assert len(set(rows)) == 1 and len(rows) == 9 and len(set(y)) > 1
            count = len(rows)
        else:
            assert len(rows) == 1
            count = 1
    assert count is not None and count > 0, name


@pytest.mark.parametrize("name", NAMES)
def test_the_float32_emulation_of_the_kernels_stays_inside_the_bounds(name):
    c, r, b = ref_and_bounds(name)
    loss, grad = cc.emulate(c, "fixed")
    lr, gr = cc.measure(c, loss, grad, r, b)
    print("EMULATED %-22s loss err / bound %.3g  gradient err / bound %.3g" % (name, lr, gr))
    assert lr <= 1 and gr <= 1


def test_offsets_change_neither_the_bounds_nor_the_bits_of_exactly_shifted_rows():
    grid = slice(0, cc.OFFSET_GRID_ROWS)
    ref_c, _, (_, gb0) = ref_and_bounds("offset_0")
    g0 = cc.emulate(ref_c, "fixed")[1]
    old0 = cc.emulate(ref_c, "single_lse")[1]
    differs = 0
    for off in cc.OFFSETS[1:]:
        c, _, (_, gb) = ref_and_bounds("offset_%g" % off)
        assert np.array_equal(gb[grid], gb0[grid])
        assert gb.max() <= 1.01 * gb0.max()                                    # (the other rows' shifted logits were rounded: not the same rows)
        assert cc.emulate(c, "fixed")[1][grid].tobytes() == g0[grid].tobytes()
        differs += cc.emulate(c, "single_lse")[1][grid].tobytes() != old0[grid].tobytes()
    assert differs >= 3                                                         # the single-float form is not shift invariant


@pytest.mark.parametrize("form", cc.WRONG)
def test_each_wrong_restatement_leaves_a_bound_by_10x(form):
    worst, where = 0.0, None
    for name in NAMES:
        if name == "fold_200003" and form != "f32_fold":                       # (the one case that takes a second per form)
            continue
        c, r, b = ref_and_bounds(name)
        ratio = max(cc.measure(c, *cc.emulate(c, form), ref=r, bnd=b))
        if ratio > worst:
            worst, where = ratio, name
    print("MUTATION %-16s leaves a bound by %.3g x on %s" % (form, worst, where))
    assert worst >= 10, (form, worst, where)
