"""No GPU: the constructions of tests/attention_cases.py hold what tests/test_attention_forward_gpu.py relies on.

- the float64 references agree with independent float64 evaluations (torch, and plain loops for the table contract);
- the bounds are not slack: deliberately wrong references exceed them on a named case;
- the bounds can be met: the float32 torch evaluation and a numpy model of the MFMA operand format stay inside;
- the input families have the properties their names promise;
- the instance table names every kernel instance, and the device test is parametrised with exactly that table."""
import numpy as np
import pytest
import torch

import attention_cases as ac
import operand_cases as oc

T, D = ac.TOKENS, ac.DIM


def _inst(i):
    return ac.BY_ID[i]


# ---- references -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,cls_only", [(8, 0), (6, 1), (4, 0), (9, 1), (144, 0)])
def test_dense_reference_matches_torch_float64(heads, cls_only):
    qkv = ac.dense_case("plain", 3, heads).astype(np.float64)
    t = torch.from_numpy(qkv)
    dh = D // heads
    q, k, v = (t[:, i * D:(i + 1) * D].reshape(3, T, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
    out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(3, T, D)
    want = (out[:, 0] if cls_only else out.reshape(3 * T, D)).numpy()
    assert np.abs(ac.dense_ref(qkv, heads, cls_only) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("family", ["plain", "routing", "overflow"])
def test_table_matrix_matches_the_contract_row_by_row(family):
    P = 5
    t = ac.table_case(family, P, 8)
    x = ac.table_matrix(t).reshape(P, T, ac.N3)
    sw, ow, vec, qkv, stats = (np.asarray(t[k], dtype=np.float64) for k in ("sw", "ow", "vec", "qkv", "stats"))
    for p in range(P):
        for tok in range(T):
            if tok == 0:
                want = vec[2 * ac.N3:3 * ac.N3]
            elif tok <= 16:
                want = stats[p * T + tok, 1] * (sw[t["subj"][p] * 16 + tok - 1] + ow[t["obj"][p] * 16 + tok - 1]) + vec[0:ac.N3]
            else:
                want = qkv[p * T + tok]
            assert np.array_equal(x[p, tok], want), (p, tok)
    assert np.array_equal(ac.combine_rows(ac.table_matrix(t)), x[:, :17])


@pytest.mark.parametrize("heads", [8, 6, 4, 9])
def test_folded_reference_matches_the_dense_formula_on_materialised_q_k_v(heads):
    """k = a Wk, v = a Wv, u = q0 Wk^T from random weights: the folded form's abar_h Wv_h is the dense form's CLS row of head h"""
    rng = np.random.default_rng(heads)
    P, dh = 3, D // heads
    c = ac.fold_case("plain", P, heads)
    a = torch.nn.functional.layer_norm(torch.from_numpy(c["x"].astype(np.float64)), (D,), torch.from_numpy(c["ln_w"].astype(np.float64)),
                                       torch.from_numpy(c["ln_b"].astype(np.float64)), 1e-5).numpy().reshape(P, T, D)
    assert np.abs(a - ac.layernorm64(c["x"], c["ln_w"], c["ln_b"]).reshape(P, T, D)).max() <= 1e-12
    wk, wv = rng.standard_normal((heads, D, dh)) * 0.05, rng.standard_normal((heads, D, dh)) * 0.05
    q0 = rng.standard_normal((P, heads, dh))
    u = np.einsum("phd,hcd->phc", q0, wk)
    qkv = np.zeros((P, T, 3, heads, dh))
    qkv[:, 0, 0] = q0
    qkv[:, :, 1] = np.einsum("ptc,hcd->pthd", a, wk)
    qkv[:, :, 2] = np.einsum("ptc,hcd->pthd", a, wv)
    dense = ac.dense_ref(qkv.reshape(P * T, ac.N3), heads, cls_only=1).reshape(P, heads, dh)
    abar = ac.fold_ref(c["x"], c["ln_w"], c["ln_b"], u.reshape(P, heads * D), heads).reshape(P, heads, D)
    folded = np.einsum("phc,hcd->phd", abar, wv)
    assert np.abs(folded - dense).max() <= 1e-11 * np.abs(dense).max()


# ---- the bounds are not slack ---------------------------------------------------------------------------------------------------------------
def _single_fp16(qkv):
    out = np.array(qkv, dtype=np.float64)
    out[:, :2 * D] = oc.fp16_sat(qkv[:, :2 * D]).astype(np.float64)
    return out


def _wrong_references():
    """name -> (case it must show on, the wrong float64 reference of that case, the right one, the bound)"""
    out = {}
    e = ac.expectation(_inst("dense-h8"), "sharp", 3)
    out["q and k as a single fp16 (no lo plane)"] = ("dense-h8 sharp P=3", ac.dense_ref(_single_fp16(e["seen"]), 8), e)
    e = ac.expectation(_inst("dense-h8"), "plain", 3)
    out["dh^-0.5 of the other head width"] = ("dense-h8 plain P=3", ac.dense_ref(e["seen"], 8, dh_scale=96), e)
    e = ac.expectation(_inst("dense-h6"), "plain", 3)
    out["dh^-0.5 of the other head width (6 heads)"] = ("dense-h6 plain P=3", ac.dense_ref(e["seen"], 6, dh_scale=72), e)
    e = ac.expectation(_inst("dense-h8-cls"), "plain", 3)
    out["the cls_only row taken from token 1"] = ("dense-h8-cls plain P=3", ac.dense_ref(e["seen"], 8, 1, cls_row=1), e)
    e = ac.expectation(_inst("generic-h4-cls"), "plain", 3)
    out["the cls_only row taken from token 1 (generic)"] = ("generic-h4-cls plain P=3", ac.dense_ref(e["seen"], 4, 1, cls_row=1), e)
    e = ac.expectation(_inst("table-h8"), "plain", 3)
    for name, w in (("tokens 17 and 18 swapped", "tokens_17_18_swapped"), ("subj and obj swapped", "subj_obj_swapped"),
                    ("rstd of the neighbouring token", "rstd_of_neighbour"), ("c2 left out for token 1", "no_c2_token_1")):
        out[name] = ("table-h8 plain P=3", ac.dense_ref(ac.table_matrix(e["t"], wrong=(w,)), 8), e)
    e = ac.expectation(_inst("combine-h0"), "plain", 3)
    for name, w in (("combine: subj and obj swapped", "subj_obj_swapped"), ("combine: rstd of the neighbouring token", "rstd_of_neighbour"),
                    ("combine: c2 left out for token 1", "no_c2_token_1")):
        out[name] = ("combine-h0 plain P=3", ac.combine_rows(ac.table_matrix(e["t"], wrong=(w,))), e)
    for i in ("fold-h8", "fold_valu-h4"):
        e = ac.expectation(_inst(i), "plain", 3)
        c = e["c"]
        out["one head's abar taken from the next head (%s)" % i] = (i + " plain P=3", ac.fold_ref(c["x"], c["ln_w"], c["ln_b"], e["u"], _inst(i).heads, head_shift=1), e)
        out["dh^-0.5 of another head width (%s)" % i] = (i + " plain P=3", ac.fold_ref(c["x"], c["ln_w"], c["ln_b"], e["u"], _inst(i).heads, dh_scale=96 if _inst(i).heads == 8 else 72), e)
    return out


def test_wrong_references_exceed_the_bounds(capsys):
    wrong = _wrong_references()
    for needed in ("q and k as a single fp16 (no lo plane)", "dh^-0.5 of the other head width", "tokens 17 and 18 swapped", "subj and obj swapped",
                   "rstd of the neighbouring token", "c2 left out for token 1", "the cls_only row taken from token 1",
                   "one head's abar taken from the next head (fold-h8)"):
        assert needed in wrong
    for name, (case, ref_wrong, e) in wrong.items():
        ratio = ac.worst_ratio(ref_wrong, e["ref"], e["bound"])
        with capsys.disabled():
            print("attention bounds: %-62s exceeds the bound %.3g x on %s" % (name, ratio, case))
        assert ratio > 1.0, "%s: stays inside the bound on %s (%.3g)" % (name, case, ratio)


# ---- the bounds can be met --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst_id", [i.id for i in ac.INSTANCES])
def test_float32_evaluation_and_format_model_stay_inside_the_bounds(inst_id):
    inst = _inst(inst_id)
    for family in inst.families:
        for P in (1, 3):
            e = ac.expectation(inst, family, P)
            assert np.isfinite(e["bound"]).all() and np.isfinite(e["ref"]).all(), (family, P)
            assert (e["bound"] > 0).all() or inst.form == "combine", (family, P)      # (the copied CLS row and exact sums: bound 0 = equal)
            if inst.form in ("dense", "generic"):
                f32 = ac.dense_f32(e["seen"], inst.heads, inst.cls_only)
            elif inst.form == "table":
                f32 = ac.dense_f32(ac.table_matrix(e["t"], dtype=np.float32), inst.heads)
            elif inst.form == "combine":
                f32 = e["yard"]
            else:
                f32 = ac.fold_f32(e["c"]["x"], e["c"]["ln_w"], e["c"]["ln_b"], e["u"], inst.heads)
            if not (family == "overflow" and inst.form in ("dense", "table")):      # (beyond the planes' range float32 is another function)
                assert ac.worst_ratio(f32, e["ref"], e["bound"]) <= 1.0, (family, P, "float32")
            if inst.form in ("dense", "table"):
                seen = e["seen"] if inst.form == "dense" else ac.table_matrix(e["t"], dtype=np.float32)
                assert ac.worst_ratio(ac.dense_model16(seen, inst.heads, inst.cls_only), e["ref"], e["bound"]) <= 1.0, (family, P, "fp16 hi + lo model")
            if e["yard"] is not None:      # the float32 evaluation rounded into the kernel's output rows meets its own yardstick
                rows = e["yard"] if inst.form == "combine" else ac.decode_split_rows(oc.split_rows(e["yard"]), e["yard"].shape[-1])
                assert ac.worst_ratio(rows, e["ref"], ac.yardstick_allowed(e["yard"], e["ref"], split_rows=inst.form != "combine")) <= 1.0


def test_operand_planes_hold_twice_65504():
    """What clamp_planes states, on the numpy model of att_split2's two saturating conversions"""
    x = oc.f32([7.0e4, -1.0e6, 65520.0, 131008.0, 131072.0, -65504.0, 6.0e4, 100000.0])
    hi = oc.fp16_sat(x)
    lo = oc.fp16_sat(oc.f32(x - hi))
    held = hi.astype(np.float64) + lo.astype(np.float64)
    want = ac.clamp_planes(x)
    rep, _ = ac.planes16(np.abs(want))
    assert (np.abs(held - want) <= rep).all(), (held, want)
    assert held[0] == 7.0e4 and held[1] == -ac.PLANES_MAX and (np.abs(held - ac.clamp16(x))[:2] > 4000).all()


# ---- the families are what they say -----------------------------------------------------------------------------------------------------------
def _scores(qkv, heads):
    q, k, _ = ac.qkv_views(np.asarray(qkv, dtype=np.float64), heads)
    return (q @ k.transpose(0, 1, 3, 2)) * (D // heads) ** -0.5


@pytest.mark.parametrize("heads", ac.MFMA_HEADS + ac.GENERIC_HEADS)
def test_dense_families(heads):
    P = 3
    s = _scores(ac.dense_case("sharp", P, heads), heads)
    assert s.max() > 25 and s.min() < -25
    for family, gap in (("onehot", 80.0), ("routing", 60.0)):
        s = np.sort(_scores(ac.dense_case(family, P, heads), heads), -1)
        assert (s[..., -1] - s[..., -2]).min() >= gap, family
        best = _scores(ac.dense_case(family, P, heads), heads).argmax(-1)
        for h in range(heads):
            assert np.array_equal(best[:, h], np.broadcast_to(ac.route(h), (P, T))) and (ac.route(h) != np.arange(T)).any()
    p = ac.softmax64(_scores(ac.dense_case("flat", P, heads), heads))
    assert np.abs(p - 1.0 / T).max() <= 1e-15
    q, k, v = ac.qkv_views(ac.dense_case("flat", P, heads), heads)
    assert not q[:, 1::2].any() and np.array_equal(k[:, 0::2], np.broadcast_to(k[:, 0::2, :1], k[:, 0::2].shape))
    v = ac.qkv_views(ac.dense_case("routing", P, heads), heads)[2]
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 2047 and np.array_equal(v, v.astype(np.float16).astype(np.float32))
    rows = v.transpose(0, 2, 1, 3).reshape(P * T * heads, -1)
    assert len({r.tobytes() for r in rows}) == len(rows)              # every (pair, token, head) has its own row of values
    r = np.abs(ac.dense_case("range", P, heads))
    assert r.max() == 6.0e4 and np.abs(_scores(ac.dense_case("range", P, heads), heads)).max() < 40
    assert np.abs(ac.dense_case("overflow", P, heads)).max() == 1.0e6


@pytest.mark.parametrize("P", ac.SIZES + (ac.BIG,))
def test_pair_lists(P):
    subj, obj, n_obj = ac.pair_list(P)
    assert len(subj) == len(obj) == P and len({(s, o) for s, o in zip(subj, obj)}) == P
    assert subj.max() < n_obj and obj.max() < n_obj and n_obj <= 32 and 2 not in subj and 2 not in obj          # object 2 is in no pair
    if P >= 3:
        assert (subj == obj).any() and (np.diff(subj) < 0).any()
        assert 0 in subj and 0 in obj and n_obj - 1 in subj and n_obj - 1 in obj


@pytest.mark.parametrize("heads", ac.MFMA_HEADS)
def test_table_families(heads):
    P = 5
    for family, gap in (("onehot", 80.0), ("routing", 60.0)):
        t = ac.table_case(family, P, heads)
        x = ac.table_matrix(t)
        s = np.sort(_scores(x, heads), -1)
        assert (s[..., -1] - s[..., -2]).min() >= gap, family
        # rstd 1, c2 0, halves that add exactly: the float32 formation of the rows is exact
        cols = slice(0, ac.N3 if family == "routing" else 2 * D)      # (the one-hot family's values are random)
        assert np.array_equal(ac.table_matrix(t, dtype=np.float32).astype(np.float64)[:, cols], x[:, cols])
    v = ac.qkv_views(x, heads)[2]
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 2047
    # a patch token's value row names subject row + 32 x object row
    assert np.array_equal(v[:, 0, 1:17, 0], np.broadcast_to((t["subj"] + 32.0 * t["obj"])[:, None], (P, 16)))
    p = ac.softmax64(_scores(ac.table_matrix(ac.table_case("flat", P, heads)), heads))
    assert np.abs(p - 1.0 / T).max() <= 1e-15
    assert np.abs(ac.table_matrix(ac.table_case("range", P, heads))).max() == 6.0e4
    over = np.abs(ac.table_matrix(ac.table_case("overflow", P, heads)))
    assert over.max() > ac.PLANES_MAX and ((over > ac.FP16_MAX) & (over < ac.PLANES_MAX)).any()      # beyond both limits of the planes


@pytest.mark.parametrize("heads", ac.FOLD_HEADS)
def test_folded_families(heads):
    P = 3

    def scores(family):
        c = ac.fold_case(family, P, heads)
        a = ac.layernorm64(c["x"], c["ln_w"], c["ln_b"]).reshape(P, T, D)
        return (c["u"].astype(np.float64).reshape(P, heads, D) @ a.transpose(0, 2, 1)) * (D // heads) ** -0.5

    s = scores("sharp")
    assert np.abs(np.abs(s).max(-1).max(-1) - 30).max() < 1e-3 and s.max() > 15 and s.min() < -15      # every pair reaches 30 in magnitude
    for family, gap in (("onehot", 80.0), ("routing", 60.0)):
        s = scores(family)
        srt = np.sort(s, -1)
        assert (srt[..., -1] - srt[..., -2]).min() >= gap, family
        assert np.array_equal(s.argmax(-1), np.broadcast_to([ac.fold_route(h) for h in range(heads)], (P, heads)))
    assert np.abs(ac.softmax64(scores("flat")) - 1.0 / T).max() <= 1e-12
    c = ac.fold_case("ln_edges", P, heads)
    x = c["x"].reshape(P, T, D)
    assert (x[:, 3] == 2.5).all() and (x[:, 7] == np.float32(0.1)).all() and abs(np.delete(x, [3, 7], axis=1).mean() - 15) < 5
    assert np.abs(ac.fold_case("range", P, heads)["x"]).max() == 6.0e4 and np.abs(ac.fold_case("overflow", P, heads)["x"]).max() == 1.0e6


def test_sizes_reach_the_launch_edges():
    for heads in ac.GENERIC_HEADS:      # attention_kernel: 4 waves per workgroup, one per (pair, head)
        if heads % 4:
            assert any((P * heads) % 4 for P in ac.SIZES), heads      # a partly idle last workgroup
    assert [h for h in ac.GENERIC_HEADS if h % 4] == [9, 18]           # every other accepted head count is a multiple of 4: no such case exists
    assert {8, 6, 4} <= set(ac.MFMA_HEADS + ac.GENERIC_HEADS) and {8, 6, 4} <= set(ac.FOLD_HEADS)
    rows = [17 * P for P in ac.SIZES + (ac.BIG,)]                       # qkv0_combine: 4 rows per workgroup, rows dealt in eighths
    assert any(r < 8 * 4 for r in rows) and any(r % 8 for r in rows) and any(r > 4096 for r in rows)
    assert ac.BIG * min(ac.MFMA_HEADS) // 2 >= 2000                       # the MFMA forms: two items per workgroup


# ---- the instance table -----------------------------------------------------------------------------------------------------------------------
def test_instance_table_names_every_kernel_instance():
    rows = {(i.kernel, i.cls_only, i.o_fmt) for i in ac.INSTANCES}
    want = set()
    for dh in (72, 96):
        for f24 in ("false", "true"):
            want |= {("attention_mfma_kernel<%d, false, %s>" % (dh, f24), c, o) for c, o in ((0, ac.SPLIT), (0, ac.MIXED), (1, ac.SPLIT))}     # 12
        want |= {("attention_mfma_kernel<%d, true>" % dh, 0, o) for o in (ac.SPLIT, ac.MIXED)}                                                # 16
    want |= {("attention_kernel", 0, ac.SPLIT), ("attention_kernel", 1, ac.SPLIT)}
    want |= {(k, 0, ac.SPLIT) for k in ("cls_fold_attention_kernel", "cls_fold_attention_mfma_kernel<false>", "cls_fold_attention_mfma_kernel<true>",
                                        "qkv0_combine_kernel")}
    assert rows == want
    assert len(ac.KERNELS) == 6 + 1 + 3 + 1
    assert sorted({i.heads for i in ac.INSTANCES if i.kernel == "attention_kernel"}) == ac.GENERIC_HEADS == [4, 9, 12, 16, 18, 24, 36, 48, 72, 144]
    assert ac.LDS_REFUSED_HEADS == [1, 2, 3] and sorted(ac.MFMA_HEADS) == [6, 8]
    for k in ("cls_fold_attention_kernel", "cls_fold_attention_mfma_kernel<false>", "cls_fold_attention_mfma_kernel<true>"):
        assert {8, 6, 4} <= {i.heads for i in ac.INSTANCES if i.kernel == k}
    assert len({i.id for i in ac.INSTANCES}) == len(ac.INSTANCES)


def test_device_test_is_parametrised_with_the_table():
    import test_attention_forward_gpu as g

    def params(fn):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "inst_id,family"
        return list(marks[0].args[1])

    in_process = params(g.test_attention_instance) + params(g.test_folded_attention)
    assert in_process == g.LAUNCH_CASES + g.FOLD_CASES and g.test_folded_vector_alu_kernel_in_a_child_process
    everything = in_process + g.CHILD_FOLD_CASES
    assert len(everything) == len(set(everything))
    assert set(everything) == {(i.id, f) for i in ac.INSTANCES for f in i.families}
    assert all(ac.BY_ID[i].form == "fold_valu" for i, _ in g.CHILD_FOLD_CASES)
    for i in ac.INSTANCES:
        for f in i.families:
            assert set(ac.SIZES) <= set(i.sizes(f))
        assert ac.BIG in i.sizes("plain") or i.form == "generic"
