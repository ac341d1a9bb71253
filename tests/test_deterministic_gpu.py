"""The ordered mode (include/veto_amd.h: veto_train_opts_t.deterministic, veto_roi_pool_backward_ordered) on the device.

Every call runs twice into NaN-filled outputs and the two results must be bit-equal.  The three sites whose order the header states as a
float32 sequential sum (ROI pooling backward, token-assembly backward, embedding scatter) are compared BIT FOR BIT with the numpy
restatements of tests/deterministic_cases.py; tests/test_deterministic_host.py proves that on these inputs any other walk order gives
other bits.  The weight gradient and the LayerNorm backward are exact where the input makes every order exact, repeatable, and inside
the bounds of the existing tests.  Then the whole training step through VETORelationHead.forward, three times from one state.
Each test prints lines starting with "deterministic_gpu:" (pytest -s)."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import deterministic_cases as dc
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
F = np.float32
DIM, TOK = dc.DIM, dc.TOK
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _lib():
    from veto_amd import native
    return native, native.load_library()


def _t(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), **kw)


def _say(line):
    print("deterministic_gpu: " + line, flush=True)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32) if t.dtype == torch.float32 else t.detach().cpu().contiguous().view(torch.int16).numpy()


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = np.asarray(want, dtype=F)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    bad = int((got.view(np.int32) != want.view(np.int32)).sum())
    assert bad == 0, "%s: %d of %d elements differ in a bit, largest difference %g" % (what, bad, want.size, np.nanmax(np.abs(got - want)))


def _twice(run, what):
    """run() -> tuple of device tensors, freshly NaN-filled inside; the two calls must agree bit for bit.  Returns the first."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(x), _bits(y)), "%s: output %d differs between two calls" % (what, i)
    return a


# ---- site 5: ROI pooling backward, ordered entry ---------------------------------------------------------------------------------
def _roi_ordered(case, entry="veto_roi_pool_backward_ordered", zeroed=False):
    from veto_amd import native, poolers
    dev = _dev()
    call = native.Launch(dev, "test")
    rois, g_rgb = _t(case.rois), _t(case.g_rgb)
    g_dep = _t(case.g_dep) if case.g_dep is not None else None
    a = poolers._pool_args(call, case.shapes, case.scales, rois, case.shapes[0][0], case.pooled, case.ratio, case.depth_shape)
    fill = 0.0 if zeroed else NAN
    levels = [torch.full(s, fill, device=dev) for s in case.shapes]
    depth = torch.full(case.depth_shape, fill, device=dev) if g_dep is not None else None
    ptrs = (ctypes.c_void_p * 4)(*[g.data_ptr() for g in levels])
    call.run(entry, ctypes.byref(a), call.ptr(g_rgb), call.ptr(g_dep), ptrs, call.ptr(depth))
    return tuple(levels) + ((depth,) if depth is not None else ())


@pytest.mark.parametrize("name", sorted(dc.ROI_CASES))
def test_roi_pool_backward_ordered_equals_the_stated_order(name):
    """Bit-equal to the restatement, NaN-filled maps (the call writes every element; untouched pixels are exactly 0)."""
    case = dc.ROI_CASES[name]()
    got = _twice(lambda: _roi_ordered(case), name)
    levels, dep = dc.pooler_backward_ordered(case)
    want = levels + ([dep] if dep is not None else [])
    for l, (g, w) in enumerate(zip(got, want)):
        _same_bits(g, w, "%s map %d" % (name, l))
    _say("roi %-22s %d maps, %d elements bit-equal to the stated order, %d of them nonzero"
         % (name, len(want), sum(w.size for w in want), sum(int((w != 0).sum()) for w in want)))


def test_roi_pool_backward_default_entry_keeps_its_answer_on_the_exact_case():
    """Knob off: the atomic entry on the order-free input gives the one possible answer, as before."""
    case = dc.ROI_CASES["exact_contention"]()
    got = _roi_ordered(case, entry="veto_roi_pool_backward", zeroed=True)
    torch.cuda.synchronize()
    _same_bits(got[0], dc.pooler_backward_ordered(case)[0][0], "default entry, exact contention")


# ---- site 1: token-assembly backward hook -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.ASSEMBLE_CASES))
def test_assemble_backward_ordered_equals_the_stated_order(name):
    native, lib = _lib()
    dev = _dev()
    c = dc.ASSEMBLE_CASES[name]()
    dx, lc, subj, obj = _t(c.dx), _t(c.lc), _t(c.subj), _t(c.obj)
    obj_off, pair_off = _t(c.obj_off), _t(c.pair_off)

    def run():
        dpatch = torch.full((c.n_obj, 16, 2 * DIM), NAN, device=dev)
        dlc = torch.full((c.n_obj, 2, 2 * DIM), NAN, device=dev)
        native.check(lib.veto_debug_assemble_backward_ordered(None, dx.data_ptr(), subj.data_ptr(), obj.data_ptr(), lc.data_ptr(), obj_off.data_ptr(),
                                                              pair_off.data_ptr(), len(c.num_objs), c.n_obj, dpatch.data_ptr(), dlc.data_ptr()))
        return dpatch, dlc
    dpatch, dlc = _twice(run, name)
    want_p, want_l = dc.assemble_backward_ordered(c.dx, c.subj, c.obj, c.lc, c.n_obj)
    _same_bits(dpatch, want_p, name + " dpatch")
    _same_bits(dlc, want_l, name + " dlc")
    unused = sorted(set(range(c.n_obj)) - set(c.subj.tolist()) - set(c.obj.tolist()))
    assert all(not want_p[n].any() for n in unused)
    _say("assemble %-18s %4d pairs, %d objects (%d in no pair: exact zeros): dpatch and dlc bit-equal to the stated order" % (name, c.n_pair, c.n_obj, len(unused)))


# ---- site 2: embedding scatter hook -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.SCATTER_CASES))
def test_scatter_rows_ordered_equals_the_stated_order(name):
    native, lib = _lib()
    dev = _dev()
    c = dc.SCATTER_CASES[name]()
    demb, labels = _t(c.demb), _t(c.labels)

    def run():
        out = torch.full((c.n_table_rows, c.dim), NAN, device=dev)
        native.check(lib.veto_debug_scatter_rows_ordered(None, demb.data_ptr(), labels.data_ptr(), len(c.labels), c.dim, c.n_table_rows, out.data_ptr()))
        return (out,)
    (out,) = _twice(run, name)
    _same_bits(out, dc.scatter_rows_ordered(c.demb, c.labels, c.n_table_rows), name)
    _say("scatter %-20s %d rows of width %d into %d table rows: bit-equal to the stated order" % (name, len(c.labels), c.dim, c.n_table_rows))


# ---- site 4: weight gradient, ordered ------------------------------------------------------------------------------------------------------
def _wgrad_ordered(dy, x, ks):
    native, lib = _lib()
    m, n = dy.shape
    k = x.shape[1]
    need = lib.veto_debug_wgrad_ordered_workspace_bytes(m, n, k, ks)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=_dev())      # the partial planes (and everything else) start as NaN
    dw = torch.full((n, k), NAN, device=_dev())
    native.check(lib.veto_debug_wgrad_ordered(None, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), m, n, k, ks, ws.data_ptr(), ws.numel()))
    return (dw,)


# m on both sides of 32 * k_splits * j (the padded reduction length), j = 1 and 2; auto (0): one and two splits (2048 rows per split)
WGRAD_EXACT = [(ks, m, 64) for ks in (1, 2, 3) for j in (1, 2) for m in (32 * ks * j - 1, 32 * ks * j, 32 * ks * j + 1)] + \
              [(64, m, 64) for m in (2047, 2048, 2049)] + [(0, m, 64) for m in (2048, 2049)] + [(3, 97, 51)]      # (n = 51: the form with transposed copies)


@pytest.mark.parametrize("ks,m,n", WGRAD_EXACT)
def test_wgrad_ordered_is_exact_on_order_free_inputs(ks, m, n):
    """Small-integer operands (every product and partial sum an integer below 2^24) and a single-entry dy (dw = one row of x): exact
    whatever the split count, with every partial plane poisoned before the call."""
    k = 192
    g = torch.Generator().manual_seed(ks * 100000 + m * 64 + n)
    x = torch.randint(-3, 4, (m, k), generator=g).float()
    dy = torch.randint(-3, 4, (m, n), generator=g).float()
    (dw,) = _twice(lambda: _wgrad_ordered(dy.to(_dev()), x.to(_dev()), ks), "wgrad ints")
    assert torch.equal(dw.cpu().double(), dy.double().t() @ x.double())
    one = torch.zeros(m, n)
    one[m - 1, n - 1] = 1.0
    (dw,) = _twice(lambda: _wgrad_ordered(one.to(_dev()), x.to(_dev()), ks), "wgrad single entry")
    want = torch.zeros(n, k)
    want[n - 1] = x[m - 1]
    assert torch.equal(dw.cpu(), want)
    _say("wgrad ordered k_splits %2d m %4d n %2d: integers and the single-entry dy exact, planes poisoned" % (ks, m, n))


@pytest.mark.parametrize("ks,m,n,k", [(0, 4492, 576, 576), (7, 1000, 1728, 576), (64, 4099, 64, 192), (3, 513, 51, 192)])
def test_wgrad_ordered_random_operands_repeat_and_stay_within_the_bound(ks, m, n, k):
    """Bit-equal across calls; error relative to |dy|^T |x| below the 2e-5 of test_wgrad_matches_fp64."""
    g = torch.Generator().manual_seed(m + n + k)
    dy, x = torch.randn(m, n, generator=g).to(_dev()), torch.randn(m, k, generator=g).to(_dev())
    (dw,) = _twice(lambda: _wgrad_ordered(dy, x, ks), "wgrad random")
    ref = dy.double().t() @ x.double()
    scale = (dy.abs().double().t() @ x.abs().double()).clamp_min(1e-6)
    rel = ((dw.double() - ref).abs() / scale).max().item()
    _say("wgrad ordered k_splits %2d m %4d n %4d k %3d: repeatable, error / |dy|^T|x| %.2e" % (ks, m, n, k, rel))
    assert rel < 2e-5


# ---- site 3: LayerNorm backward, ordered ---------------------------------------------------------------------------------------------------
def _ln_ordered(x, dy, gamma, dres, rows, split):
    native, lib = _lib()
    dev = _dev()
    ws = torch.full((lib.veto_debug_layernorm_backward_workspace_bytes(rows),), 0xFF, dtype=torch.uint8, device=dev)
    n_part = lib.veto_debug_layernorm_backward_col_partial_rows(rows)
    dx = torch.full((rows, DIM), NAN, device=dev)
    dgb = torch.full((2, DIM), NAN, device=dev)
    srows = torch.full((rows, 2 * DIM), NAN, dtype=torch.bfloat16, device=dev) if split else None
    colp = torch.full((n_part, DIM), NAN, device=dev) if split else None
    native.check(lib.veto_debug_layernorm_backward_ordered(None, x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), dres.data_ptr() if dres is not None else None,
                                                           dx.data_ptr(), dgb.data_ptr(), srows.data_ptr() if split else None,
                                                           colp.data_ptr() if split else None, rows, 0, 0, 1.0, ws.data_ptr(), ws.numel()))
    return (dx, dgb) + ((srows, colp) if split else ())


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 513])
def test_layernorm_backward_ordered(rows, split):
    """Both forms: bit-equal across calls, inside _ln_bounds of tests/test_train_scale_gpu.py; dbeta of a small-integer dy is exact."""
    import test_train_scale_gpu as ts
    dev = _dev()
    x, dy, gamma, dres = ts._ln_inputs(rows, True, "plain")
    ref_dx, ref_dg, ref_db = ts._ln_reference(x, dy, gamma, dres)
    tol_dx, tol_dg, tol_db = ts._ln_bounds("plain", ref_dx, ref_dg, ref_db)
    out = _twice(lambda: _ln_ordered(x.to(dev), dy.to(dev), gamma.to(dev), dres.to(dev), rows, split), "layernorm rows %d" % rows)
    dx, dgb = out[0], out[1]
    e_dx = float((dx.cpu().double() - ref_dx).abs().max())
    e_dg = float((dgb[0].cpu().double() - ref_dg).abs().max())
    e_db = float((dgb[1].cpu().double() - ref_db).abs().max())
    assert e_dx < tol_dx and e_dg < tol_dg and e_db < tol_db, (e_dx, tol_dx, e_dg, tol_dg, e_db, tol_db)
    if split:
        ts._check_split_outputs(out[2], out[3], rows, ref_dx, tol_dx)
    ints = torch.randint(-8, 9, (rows, DIM), generator=torch.Generator().manual_seed(rows)).float()
    out_i = _twice(lambda: _ln_ordered(x.to(dev), ints.to(dev), gamma.to(dev), None, rows, split), "layernorm ints rows %d" % rows)
    assert torch.equal(out_i[1][1].cpu().double(), ints.double().sum(0))
    _say("layernorm ordered rows %3d %s: repeatable, error / bound dx %.1e dgamma %.1e dbeta %.1e, integer dbeta exact"
         % (rows, "split" if split else "plain", e_dx / tol_dx, e_dg / tol_dg, e_db / tol_db))


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_workspace_sizes_and_the_opts_field():
    """The default size query returns what the layout without planes needs, whatever the opts say with the knob off or in the struct's
    earlier size; the ordered mode asks for more, and the calls refuse a workspace sized for the default path."""
    from veto_amd import native, synth, testing
    native_, lib = _lib()
    dev = _dev()
    cfg = testing.make_config(2, 8, precision="precise")
    model = testing.make_predictor(cfg, synth.predictor_state_dict(2, layers=2), dev)
    eng = model._ensure_engine(dev)
    n_obj, n_pair = 36, 1260
    base = lib.veto_train_workspace_bytes(eng.handle, n_obj, n_pair)
    off = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts))
    on = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts), deterministic=1)
    old = native.VetoTrainOpts(struct_size=native.VetoTrainOpts.deterministic.offset, deterministic=1)      # a caller built before the field: not read
    sizes = [lib.veto_train_workspace_bytes_opts(eng.handle, n_obj, n_pair, ctypes.byref(o) if o is not None else None) for o in (None, off, old, on)]
    assert sizes[0] == sizes[1] == sizes[2] == base > 0 and sizes[3] > base
    bad = native.VetoTrainOpts(struct_size=44)
    assert lib.veto_train_workspace_bytes_opts(eng.handle, n_obj, n_pair, ctypes.byref(bad)) == 0
    _say("workspace bytes at %d objects / %d pairs (L2, precise): default %d, ordered %d (+%d for the split-K planes)" % (n_obj, n_pair, base, sizes[3], sizes[3] - base))


# ---- the whole step ------------------------------------------------------------------------------------------------------------------------
STEP_OBJS = (3, 5, 36)


def _step_inputs(dev):
    from veto_amd import synth
    from veto_amd.structures import BoxList
    rng = np.random.RandomState(21)
    W, H = 512, 384
    feats = [torch.from_numpy((0.5 * rng.randn(len(STEP_OBJS), 256, H >> (2 + l), W >> (2 + l))).astype(F)).to(dev).requires_grad_(True) for l in range(4)]
    depth = torch.from_numpy((0.5 * rng.randn(len(STEP_OBJS), 256, H >> 4, W >> 4)).astype(F)).to(dev).requires_grad_(True)
    props, targets = [], []
    for i, (boxes, rel) in enumerate(synth.synthetic_relation_targets(num_objs=STEP_OBJS)):
        b = torch.from_numpy(boxes)
        b[:, 2:] = b[:, :2] + b[:, 2:].abs() * 0.5 + 8
        labels = torch.from_numpy(synth.integers(3, "head.labels.%d" % i, (len(boxes),), 1, 151))
        p = BoxList(b, (W, H)).to(dev)
        p.add_field("labels", labels.to(dev))
        t = BoxList(b.clone(), (W, H)).to(dev)
        t.add_field("relation", torch.from_numpy(rel).to(dev))
        t.add_field("labels", labels.to(dev))
        props.append(p)
        targets.append(t)
    return feats, depth, props, targets


def _step_head(loss, knob, dev):
    from relation_sampling import make_roi_relation_samp_processor    # tests/: a stand-in for the host code base's sampler
    from veto_amd import synth, testing
    from veto_amd.relation_head import VETORelationHead
    meet = loss == "meet"
    cfg = testing.make_config(2, 8, meet=meet)
    cfg.VETO_AMD.DETERMINISTIC = knob
    if loss == "weighted_ce":
        cfg.GLOBAL_SETTING.BETA_LOSS = True
        cfg.GLOBAL_SETTING.REL_COUNTS = np.loadtxt(os.path.join(GOLDEN_DIR, "pred_counts.txt")).tolist()
    head = VETORelationHead(cfg, samp_processor=make_roi_relation_samp_processor(cfg))
    sd = synth.meet_state_dict(0, head.predictor.max_group_element_number_list, layers=2) if meet else synth.predictor_state_dict(3, layers=2)
    if loss == "weighted_ce":
        sd.pop("criterion_loss_rel.weight", None)
    head.predictor = testing.make_predictor(cfg, sd, dev)
    head.train()
    return cfg, head, {k: v.detach().clone() for k, v in head.predictor.state_dict().items()}


def _clone_boxes(p):
    from veto_amd.structures import BoxList
    q = BoxList(p.bbox, p.size, p.mode)
    q.extra_fields = dict(p.extra_fields)
    return q


def _one_step(cfg, head, state, inputs):
    """From `state`: forward through the head (sampler, ROI pooling, predictor with dropout at the reference's rates), backward to the
    parameters and the maps, clip_and_step.  Returns {name: bytes} of everything the step produced."""
    import optim_cases as oc
    from veto_amd import solver
    feats, depth, props, targets = inputs
    head.predictor.load_state_dict(state)
    head.train()
    for p in head.predictor.parameters():
        p.grad = None
    for m in feats + [depth]:
        m.grad = None
    opt = solver.make_optimizer(cfg, head.predictor, oc.Log())
    torch.manual_seed(5)
    random.seed(5)      # the MEET expert sampling draws from Python's random, as the reference's does
    _, _, losses = head(feats, [_clone_boxes(p) for p in props], targets=targets, depth_features=depth, logger=None, x=None)
    sum(v for v in losses.values() if v.requires_grad).backward()
    out = {"loss." + k: v.detach() for k, v in losses.items()}
    for l, m in enumerate(feats + [depth]):
        assert m.grad is not None
        out["map.%d" % l] = m.grad
    named = dict(head.predictor.named_parameters())
    out.update({"grad." + n: p.grad for n, p in named.items() if p.grad is not None})
    out = {k: v.cpu().numpy().tobytes() for k, v in out.items()}      # (before the step: the optimizer may touch the gradients)
    opt.clip_and_step(5.0)
    torch.cuda.synchronize()
    for n, p in named.items():
        out["param." + n] = p.detach().cpu().numpy().tobytes()
        st = opt.state.get(p, {})
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                out[key + "." + n] = st[key].cpu().numpy().tobytes()
    return out


@pytest.mark.parametrize("loss", ["ce", "weighted_ce", "meet"])
def test_whole_step_is_a_pure_function_of_its_inputs(loss):
    """L2 / H8, images of 3, 5 and 36 objects with sampled pairs, dropout at the reference's rates under one torch.manual_seed, FPN and
    depth maps requiring grad: three runs from one state dict with the config knob on, then one under
    torch.use_deterministic_algorithms(True) without the knob.  Every loss, parameter gradient, map gradient, parameter and Adam
    moment after clip_and_step must be the same bytes."""
    dev = _dev()
    inputs = _step_inputs(dev)
    cfg, head, state = _step_head(loss, True, dev)
    rates = [float(m.p) for m in head.predictor.modules() if isinstance(m, torch.nn.Dropout) and m.p > 0]
    assert 0.1 in rates and 0.35 in rates
    runs = [_one_step(cfg, head, state, inputs) for _ in range(3)]
    assert len(runs[0]) > 100 and any(k.startswith("exp_avg_sq.") for k in runs[0])
    for i in (1, 2):
        assert runs[i].keys() == runs[0].keys()
        diff = sorted(k for k in runs[0] if runs[i][k] != runs[0][k])
        assert not diff, "run %d differs from run 0 in %d of %d tensors: %s" % (i, len(diff), len(runs[0]), diff[:8])
    del head
    cfg2, head2, state2 = _step_head(loss, False, dev)
    torch.use_deterministic_algorithms(True)
    try:
        other = _one_step(cfg2, head2, state2, inputs)
    finally:
        torch.use_deterministic_algorithms(False)
    diff = sorted(k for k in runs[0] if other.get(k) != runs[0][k])
    assert not diff, "the step under torch.use_deterministic_algorithms(True) differs in %d tensors: %s" % (len(diff), diff[:8])
    _say("whole step %-11s: %d tensors (losses, gradients, map gradients, parameters, Adam moments) bit-equal over 3 runs and under "
         "torch.use_deterministic_algorithms(True)" % (loss, len(runs[0])))


# ---- parity is not lost --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module,select", [("test_train_scale_gpu.py", "one_image_all_pairs and mixed"), ("test_train_dropout_gpu.py", "test_dropout_step_gradients and n36-l2h8-mixed")],
                         ids=["scale-one-image-all-pairs", "dropout-on"])
def test_gradient_parity_with_the_knob_on(module, select):
    """The float64-oracle step tests in a fresh child pytest with VETO_DETERMINISTIC=1 (read once per process): GRAD_TOL unchanged."""
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, module), "-q", "-x", "-s", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       env=dict(os.environ, VETO_DETERMINISTIC="1"), timeout=900, cwd=os.path.dirname(here), capture_output=True, text=True)
    for line in p.stdout.splitlines():
        if line.startswith("PARITY "):
            _say("VETO_DETERMINISTIC=1 | " + line[7:])
    assert p.returncode == 0 and " passed" in p.stdout and "no tests ran" not in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
