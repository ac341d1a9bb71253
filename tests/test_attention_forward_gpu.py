"""Every forward attention kernel instance of veto_amd/csrc/attention.hip, and qkv0_combine_kernel, alone on the device against its own
contract in float64 (tests/attention_cases.py: inputs, references, derived per-element bounds, the instance table).

For every (instance, family, size) of the table: the output rows start as a sentinel NaN with guard cells behind them, every element the
contract names must be overwritten and the guards must survive; the call is made twice and must repeat bit for bit; the decoded rows lie
inside the derived bound on every element (and, for the fp32-chain kernels, inside 4 x the float32 yardstick + 4 ulp); in the routing
family the decoded integers name the expected (pair, head, token, column).  Instances that share a contract are compared with each other
on the same inputs.  The vector-ALU folded kernel is selected by VETO_CLS_MFMA=0, read once per process: its cases run in a fresh child
pytest process (as test_step_gradients_behind_the_knobs does), which leaves its decoded rows behind for the comparison with the MFMA form.

One line per case starts with PARITY; profiles/attention_forward_parity.txt is those lines of one complete run."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import attention_cases as ac
import operand_cases as oc
from test_prelude_gpu import GUARD, SENT32, Guarded

pytestmark = pytest.mark.gpu

HERE = os.path.abspath(__file__)
PROFILE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "attention_forward_parity.txt")
VALU_PROCESS = os.environ.get("VETO_CLS_MFMA") == "0"          # this process launches the vector-ALU folded kernel
DUMP_DIR = os.environ.get("VETO_ATTENTION_FOLD_DUMP")           # where the child leaves its decoded rows
INVALID = -1

# what each test function below is parametrised with; tests/test_attention_forward_host.py holds the union to the instance table
LAUNCH_CASES = [(i.id, f) for i in ac.INSTANCES if i.form in ("dense", "generic", "table", "combine") for f in i.families]
FOLD_CASES = [(i.id, f) for i in ac.INSTANCES if i.form == "fold" for f in i.families]
CHILD_FOLD_CASES = [(i.id, f) for i in ac.INSTANCES if i.form == "fold_valu" for f in i.families]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _up(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _lib():
    from veto_amd import native
    return native, native.load_library()


_LINES = []


def _report(line):
    _LINES.append(line)
    print("PARITY " + line, flush=True)


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    """profiles/attention_forward_parity.txt = the PARITY lines of a run that covered the whole table (a partial run leaves it alone)"""
    yield
    have = {tuple(l.split()[1:3]) for l in _LINES if l.startswith("case ")}
    want = {(i, f) for i, f in LAUNCH_CASES + FOLD_CASES + CHILD_FOLD_CASES}
    if VALU_PROCESS or not want <= have:
        return
    with open(PROFILE, "w") as f:
        f.write("Forward attention kernels against float64 (tests/test_attention_forward_gpu.py): per case the worst |error|, the derived bound at that\n"
                "element and the worst error / bound over all elements (<= 1 is the assertion); yard = the same against 4 x the float32 evaluation's\n"
                "worst error + 4 ulp (fp32-chain kernels).  instance = form-heads[-cls][-mixed][-f24] of attention_cases.instance_table().\n")
        f.write("\n".join(sorted(_LINES)) + "\n")


# ---- one launch, twice, behind sentinels ------------------------------------------------------------------------------------------------
def _twice(what, numel, call, partial=None):
    """call(ptr) on a fresh sentinel buffer, twice; returns the int32 words of the first run after holding the second to the same bits.
    partial(words) -> bool mask of the words that must STILL be the sentinel (default: none may be)."""
    runs = []
    for _ in range(2):
        g = Guarded(numel, torch.int32, _dev())
        call(g.ptr)
        torch.cuda.synchronize()
        if partial is None:
            runs.append(g.bits(what).copy())
            continue
        raw = g.raw.cpu().numpy()
        assert (raw[numel:] == SENT32).all(), "%s: guard cells behind the buffer were written" % what
        words = raw[:numel].copy()
        keep = partial(words)
        assert (words[keep] == SENT32).all(), "%s: words outside the contract were written" % what
        assert not (words[~keep] == SENT32).any(), "%s: words of the contract were never written" % what
        runs.append(words)
    assert np.array_equal(runs[0], runs[1]), "%s: the second call differs from the first" % what
    return runs[0]


def _decode(words, rows, o_fmt, K=ac.DIM):
    if o_fmt == ac.MIXED:
        return ac.decode_mixed_rows(words.view(np.uint8).reshape(rows, 4 * K), K)
    return ac.decode_split_rows(words.view(np.uint16).reshape(rows, 2 * K), K)


def launch_attention(what, qkv, P, heads, cls_only=0, o_fmt=ac.SPLIT, f24=0, t=None, held=None):
    """veto_debug_attention on fp32 rows `qkv` (f24: rounded and packed here) -> decoded float64 rows"""
    native, lib = _lib()
    src = _up(oc.f24_rows(qkv)) if f24 else _up(oc.f32(qkv))
    tabs = [_up(t[k]) for k in ("sw", "ow", "stats", "vec", "subj", "obj")] if t is not None else []
    ptrs = [x.data_ptr() for x in tabs] if tabs else [None] * 6
    rows = P if cls_only else P * ac.TOKENS
    words = _twice(what, rows * ac.DIM, lambda o: native.check(lib.veto_debug_attention(None, src.data_ptr(), o, P, heads, cls_only, o_fmt, f24, *ptrs)))
    if held is not None:
        held.append(words)
    return _decode(words, rows, o_fmt)


def launch_combine(what, t, P):
    """veto_debug_qkv0_combine into a sentinel qkv buffer -> float32 [P, 19, 1728] whose rows 17 / 18 are still the sentinel"""
    native, lib = _lib()
    tabs = [_up(t[k]) for k in ("sw", "ow", "stats", "vec", "subj", "obj")]
    untouched = np.zeros((P, ac.TOKENS, ac.N3), dtype=bool)
    untouched[:, 17:] = True
    words = _twice(what, P * ac.TOKENS * ac.N3, lambda q: native.check(lib.veto_debug_qkv0_combine(None, *[x.data_ptr() for x in tabs], q, P)),
                   partial=lambda w: untouched.reshape(-1))
    return words.view(np.float32).reshape(P, ac.TOKENS, ac.N3)


def launch_fold(what, c, u, P, heads, u24):
    native, lib = _lib()
    x, w, b = _up(c["x"]), _up(c["ln_w"]), _up(c["ln_b"])
    ud = _up(oc.f24_rows(u)) if u24 else _up(oc.f32(u))
    words = _twice(what, P * heads * ac.DIM, lambda o: native.check(lib.veto_debug_cls_fold_attention(None, x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                                                                      ud.data_ptr(), o, P, heads, u24)))
    return _decode(words, P, ac.SPLIT, heads * ac.DIM)


def _judge(inst, family, P, got, e, extra=""):
    """the error bound (and the yardstick) of one case; prints its PARITY line and returns the ratio"""
    ref, bound = e["ref"], e["bound"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s %s P=%d: non-finite output" % (inst.id, family, P)
    err = np.abs(got - ref)
    at = np.unravel_index(np.argmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0)), err.shape)
    ratio = ac.worst_ratio(got, ref, bound)
    line = "case %s %s P=%d  max err %.3e  err / bound at the worst element %.3e / %.3e  ratio %.3g" % (inst.id, family, P, err.max(), err[at], bound[at], ratio)
    tight = None
    if e["yard"] is not None:
        tight = ac.worst_ratio(got, ref, ac.yardstick_allowed(e["yard"], ref, split_rows=inst.form != "combine"))
        line += "  yard %.3g (float32 evaluation's worst error %.2e)" % (tight, np.abs(e["yard"].astype(np.float64) - ref).max())
    _report(line + extra)
    assert ratio <= 1.0, "%s %s P=%d: %.3g x the derived bound" % (inst.id, family, P, ratio)
    if tight is not None:
        assert tight <= 1.0, "%s %s P=%d: %.3g x (4 x the float32 yardstick + 4 ulp)" % (inst.id, family, P, tight)
    return ratio


def _routed_values(v_eff, heads, cls_only):
    """[P 19, 576] value columns of the effective matrix -> what every output row must hold when query i of head h selects key route(h)[i]"""
    v = ac.heads_view(np.ascontiguousarray(v_eff), heads)
    out = np.stack([v[:, h, ac.route(h)] for h in range(heads)], axis=1)
    return ac.merge_heads(out[:, :, :1] if cls_only else out)


def _check_routing(inst, P, got, v_eff):
    want = _routed_values(v_eff, inst.heads, inst.cls_only)
    assert np.array_equal(want, np.rint(want)) and np.abs(want).max() <= 2047
    assert np.array_equal(np.rint(got), want), "%s routing P=%d: %d output elements name another (pair, head, token, column)" % (
        inst.id, P, int((np.rint(got) != want).sum()))
    assert np.abs(got - want).max() <= 2.0 ** -10


@pytest.mark.parametrize("inst_id,family", LAUNCH_CASES)
def test_attention_instance(inst_id, family):
    inst = ac.BY_ID[inst_id]
    for P in inst.sizes(family):
        e = ac.expectation(inst, family, P)
        what = "%s %s P=%d" % (inst.id, family, P)
        extra = ""
        if inst.form == "combine":
            t = e["t"]
            rows = launch_combine(what, t, P)
            got = rows[:, :17].astype(np.float64)
        elif inst.form == "table":
            t = e["t"]
            got = launch_attention(what, t["qkv"], P, inst.heads, 0, inst.o_fmt, 0, t)
            # the same contract in two launches: qkv0_combine into the rows 0..16, then the plain form on the materialised matrix
            q = launch_combine(what + " (combine)", t, P)
            q[:, 17:] = t["qkv"].reshape(P, ac.TOKENS, ac.N3)[:, 17:]
            q = q.reshape(P * ac.TOKENS, ac.N3)
            two = launch_attention(what + " (combine + plain)", q, P, inst.heads, 0, inst.o_fmt)
            eff = ac.clamp_planes(q) if family == "overflow" else q.astype(np.float64)
            b2 = ac.dense_bound(eff, inst.heads, "mfma", 0, inst.o_fmt)
            assert ac.worst_ratio(two, e["ref"], e["bound"]) <= 1.0, what
            between = ac.worst_ratio(got, two, e["bound"] + b2)
            extra = "  | against combine + plain form: %.3g of the two bounds, %s" % (between, "bit-equal" if np.array_equal(got, two) else "not bit-equal")
            assert between <= 1.0, what
        else:
            held = []
            got = launch_attention(what, e["qkv"], P, inst.heads, inst.cls_only, inst.o_fmt, inst.f24, held=held)
            if inst.f24:      # the plain form on the rounded input: the same values, and hi + lo of a 16-bit significand is exact
                plain = launch_attention(what + " (plain form, rounded input)", e["seen"], P, inst.heads, inst.cls_only, inst.o_fmt)
                b2 = ac.dense_bound(ac.clamp_planes(e["seen"]) if family == "overflow" else e["seen"], inst.heads, "mfma", inst.cls_only, inst.o_fmt)
                between = ac.worst_ratio(got, plain, e["bound"] + b2)
                extra = "  | against the plain form on the rounded input: %.3g of the two bounds, %s" % (between, "bit-equal" if np.array_equal(got, plain) else "not bit-equal")
                assert between <= 1.0, what
        if family == "overflow" and inst.form in ("dense", "table"):
            # (reported beside the assertion: against q / k / v clamped to +-65504 the planes' kept excess shows; attention_cases.clamp_planes)
            lit = ac.dense_ref(ac.clamp16(e["x"] if inst.form == "table" else e["seen"]), inst.heads, inst.cls_only)
            extra += "  | against the reference clamped to +-65504: max err %.3e, %.3g x the bound" % (np.abs(got - lit).max(), ac.worst_ratio(got, lit, e["bound"]))
        _judge(inst, family, P, got, e, extra)
        if family == "routing" and inst.form != "combine":
            _check_routing(inst, P, got, (ac.table_matrix(e["t"]) if inst.form == "table" else e["seen"].astype(np.float64))[:, 2 * ac.DIM:])
        if inst.o_fmt == ac.MIXED:      # the same fp32 results as split rows: the two decodings differ by at most the two output-format terms
            s = launch_attention(what + " (split rows)", t["qkv"] if inst.form == "table" else e["qkv"], P, inst.heads, 0, ac.SPLIT, inst.f24,
                                 t if inst.form == "table" else None)
            mag = np.maximum(np.abs(s), np.abs(got))
            assert ac.worst_ratio(got, s, ac.out_format_term(mag, ac.SPLIT) + ac.out_format_term(mag, ac.MIXED)) <= 1.0, what + ": split against mixed rows"


def _fold_rows(inst, family, P):
    e = ac.expectation(inst, family, P)
    got = launch_fold("%s %s P=%d" % (inst.id, family, P), e["c"], e["u"], P, inst.heads, inst.f24)
    return e, got


def _check_fold_routing(inst, P, got, e):
    """one-hot probabilities: abar_h is the LayerNorm'ed row of token fold_route(h) of ITS pair, nearer to it than to any other row of the case"""
    a = ac.layernorm64(e["c"]["x"], e["c"]["ln_w"], e["c"]["ln_b"])
    g = got.reshape(P, inst.heads, ac.DIM)
    for h in range(inst.heads):
        d = ((g[:, h, None, :] - a[None]) ** 2).sum(-1)
        assert np.array_equal(d.argmin(-1), np.arange(P) * ac.TOKENS + ac.fold_route(h)), "%s routing P=%d head %d" % (inst.id, P, h)


def _fold_case(inst_id, family):
    inst = ac.BY_ID[inst_id]
    for P in inst.sizes(family):
        e, got = _fold_rows(inst, family, P)
        _judge(inst, family, P, got, e)
        if family == "routing":
            _check_fold_routing(inst, P, got, e)
        if DUMP_DIR:
            np.save(os.path.join(DUMP_DIR, "%s.%s.%d.npy" % (inst.id, family, P)), got)


if VALU_PROCESS:
    @pytest.mark.parametrize("inst_id,family", CHILD_FOLD_CASES)
    def test_folded_attention(inst_id, family):
        _fold_case(inst_id, family)
else:
    @pytest.mark.parametrize("inst_id,family", FOLD_CASES)
    def test_folded_attention(inst_id, family):
        _fold_case(inst_id, family)

    def test_folded_vector_alu_kernel_in_a_child_process():
        """cls_fold_attention_kernel (VETO_CLS_MFMA=0, read once per process) at every head count and family, and against the MFMA form on
        the same inputs: both lie within their bounds of one reference, so they differ by at most the sum of the two."""
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([sys.executable, "-m", "pytest", HERE, "-q", "-x", "-s", "-m", "gpu", "-k", "test_folded_attention or test_refusals", "-p", "no:cacheprovider"],
                               env=dict(os.environ, VETO_CLS_MFMA="0", VETO_ATTENTION_FOLD_DUMP=tmp), timeout=900, cwd=os.path.dirname(os.path.dirname(HERE)),
                               capture_output=True, text=True)
            for line in p.stdout.splitlines():
                if line.startswith("PARITY "):
                    _report(line[7:])
            assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
            assert "%d passed" % (len(CHILD_FOLD_CASES) + 1) in p.stdout, p.stdout[-2000:]
            for inst_id, family in CHILD_FOLD_CASES:
                valu = ac.BY_ID[inst_id]
                mfma = ac.BY_ID["fold-h%d" % valu.heads]
                for P in valu.sizes(family):
                    v = np.load(os.path.join(tmp, "%s.%s.%d.npy" % (inst_id, family, P)))
                    e, m = _fold_rows(mfma, family, P)
                    bv = ac.expectation(valu, family, P)["bound"]
                    between = ac.worst_ratio(m, v, e["bound"] + bv)
                    _report("between %s and %s %s P=%d: %.3g of the two bounds" % (mfma.id, inst_id, family, P, between))
                    assert between <= 1.0, (inst_id, family, P, between)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Everything launch_attention / launch_cls_fold_attention reject comes back as VETO_ERR_INVALID with a reason, before any launch: the
    sentinel buffers are untouched."""
    native, lib = _lib()
    P = 2
    qkv = _up(ac.dense_case("plain", P, 8))
    t = ac.table_case("plain", P, 8)
    held = [_up(t[k]) for k in ("sw", "ow", "stats", "vec", "subj", "obj")]
    tabs = [x.data_ptr() for x in held]
    none6 = [None] * 6
    out = Guarded(P * ac.TOKENS * ac.N3, torch.int32, _dev())      # large enough for every call below, qkv0_combine included

    def refused(rc, why):
        torch.cuda.synchronize()
        assert rc == INVALID, (why, rc)
        assert lib.veto_last_error(), why
        raw = out.raw.cpu().numpy()
        assert (raw == SENT32).all() and raw.size == out.numel + GUARD, why + ": the output buffer was written"

    att = lambda *a: lib.veto_debug_attention(None, *a)      # noqa: E731
    q, o = qkv.data_ptr(), out.ptr
    refused(att(q, o, P, 8, 1, 0, 0, *tabs), "tables with cls_only")
    refused(att(q, o, P, 8, 0, 0, 1, *tabs), "tables with 3-byte rows")
    refused(att(q, o, P, 4, 0, 0, 0, *tabs), "tables at head width 144")
    refused(att(q, o, P, 4, 0, 0, 1, *none6), "3-byte rows at head width 144")
    refused(att(q, o, P, 9, 0, 0, 1, *none6), "3-byte rows at head width 64")
    refused(att(q, o, P, 4, 0, 1, 0, *none6), "mixed rows from the generic kernel")
    for heads in (0, -8, 5, 7, 10, 1000):
        refused(att(q, o, P, heads, 0, 0, 0, *none6), "heads %d does not divide 576" % heads)
    for heads in ac.LDS_REFUSED_HEADS:
        refused(att(q, o, P, heads, 0, 0, 0, *none6), "generic head width %d: LDS beyond 160 KB" % (ac.DIM // heads))
    for k in range(6):
        refused(att(q, o, P, 8, 0, 0, 0, *[None if i == k else p for i, p in enumerate(tabs)]), "table operand %d missing" % k)
        refused(att(q, o, P, 8, 0, 0, 0, *[p if i == k else None for i, p in enumerate(tabs)]), "table operand %d alone" % k)
    refused(att(None, o, P, 8, 0, 0, 0, *none6), "null qkv")
    refused(att(q, None, P, 8, 0, 0, 0, *none6), "null o")
    for n in (0, -1):
        refused(att(q, o, n, 8, 0, 0, 0, *none6), "n_pair %d" % n)
        refused(att(q, o, n, 4, 1, 0, 0, *none6), "n_pair %d, generic" % n)
    refused(att(q, o, P, 8, 2, 0, 0, *none6), "cls_only 2")
    refused(att(q, o, P, 8, 0, 2, 0, *none6), "o_fmt 2")
    refused(att(q, o, P, 8, 0, 0, 2, *none6), "qkv_f24 2")

    c = ac.fold_case("plain", P, 8)
    x, w, b, u = (_up(c[k]) for k in ("x", "ln_w", "ln_b", "u"))
    fold = lambda *a: lib.veto_debug_cls_fold_attention(None, *a)      # noqa: E731
    good = [x.data_ptr(), w.data_ptr(), b.data_ptr(), u.data_ptr(), o]
    for k in range(5):
        refused(fold(*[None if i == k else p for i, p in enumerate(good)], P, 8, 0), "folded: null argument %d" % k)
    for n in (0, -3):
        refused(fold(*good, n, 8, 0), "folded: n_pair %d" % n)
    for heads in (0, -1, 5, 7, 16, 24, 576):
        refused(fold(*good, P, heads, 0), "folded: heads %d" % heads)
    refused(fold(*good, P, 8, 2), "folded: u_f24 2")
    if VALU_PROCESS:
        refused(fold(*good, P, 8, 1), "folded: 3-byte u with the vector-ALU form")

    comb = lambda *a: lib.veto_debug_qkv0_combine(None, *a)      # noqa: E731
    for k in range(7):
        refused(comb(*[None if i == k else p for i, p in enumerate(tabs + [o])], P), "combine: null argument %d" % k)
    for n in (0, -1):
        refused(comb(*tabs, o, n), "combine: n_pair %d" % n)
