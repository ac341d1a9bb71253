"""The device optimizer on the MI355X: veto_optim_step (veto_amd.solver) against the float64 restatement of tests/optim_cases.py.

The oracle is always given the device's own pre-step fp32 p, m, v and g, so every comparison is of ONE step.  The bounds come from
operation counts, not from measurement, with u = 2^-24 (optim_cases.adam_fp64 returns them per element):
  norms, total     relative error <= 2u of the float64 value (the sum is in double: only the final roundings count)
  coefficient      relative error <= 4u
  m                |m - m_ref| <= 8u M_abs,  M_abs = beta1 |m| + (1 - beta1) G_abs,  G_abs = |coef g| + wd |p|
  v                |v - v_ref| <= 8u (beta2 v + (1 - beta2) G_abs^2)
  p                |p - p_ref| <= u |p_ref| + 32u (lr / bc1) M_abs / denom,  denom = sqrt(v_new) / sqrt(bc2) + eps
Measured on an MI355X as fractions of these bounds (profiles/optim_parity.txt, the largest line): norms 0.464, coefficient 0.244,
m 0.211, v 0.347, p 0.990.  p: the bound is u |p_ref| plus the update's term, and a correctly rounded p alone reaches u |p| just
above a power of two.
Every launch is made twice on identically placed copies of the same inputs and must give the same bits.  Every measured figure is
printed before it is asserted (pytest -s); the parity figures also go to profiles/optim_parity.txt."""
import copy
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402

from veto_amd import solver  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_parity.txt")
U = oc.U
C = solver.CHUNK
MODES = {"norms": solver.NORMS, "clip": solver.CLIP, "step": solver.STEP, "clip_step": solver.CLIP_STEP}
PARITY_KEYS = tuple("sizes/" + m for m in MODES) + ("hyper", "clip/above", "clip/below", "clip/equal", "predictor")


@pytest.fixture(scope="module")
def parity_report():
    """Collects one line per case; profiles/optim_parity.txt is written once, after the last case, and only by a run that covered
    every case (a run of some cases leaves the committed record alone)."""
    lines = {}
    yield lines
    if set(lines) != set(PARITY_KEYS):
        return
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    ref = {k: max(float(oc.load_case(n)[k]) for n in oc.ALL) for k in ("ref_fp32_err_norm", "ref_fp32_err_m", "ref_fp32_err_v", "ref_fp32_err_p")}
    with open(PARITY, "w") as f:
        f.write("Device optimizer against the float64 restatement on the device's own pre-step fp32 state; every figure is the worst element "
                "as a FRACTION OF ITS BOUND (norms, total 2u; coef 4u; m 8u M_abs; v 8u (beta2 v + (1 - beta2) G_abs^2); p u |p| + 32u (lr / bc1) "
                "M_abs / denom; u = 2^-24).  The reference's own fp32 run (torch.optim.Adam and clip_grad_norm on the CPU) against its float64 "
                "run, worst fixture, same metric: norm %.3g  m %.3g  v %.3g  p %.3g\n"
                % (ref["ref_fp32_err_norm"], ref["ref_fp32_err_m"], ref["ref_fp32_err_v"], ref["ref_fp32_err_p"]))
        for k in PARITY_KEYS:
            f.write(lines[k] + "\n")


# ---- a table of tensors, placed element by element ---------------------------------------------------------------------------------

def spec(n, off=0, goff=None, grad=True, step=1, lr=1e-3, wd=5e-4, betas=(0.9, 0.999), eps=1e-8, gscale=1.0, fresh=False):
    """One tensor: n elements; p, m, v start `off` elements (0..3) past a 16-byte boundary and g `goff` (default: off); grad False:
    its gradient is None; fresh: exp_avg and exp_avg_sq start at zero."""
    return dict(n=n, off=off, goff=off if goff is None else goff, grad=grad, step=step, lr=lr, wd=wd, betas=betas, eps=eps, gscale=gscale, fresh=fresh)


def host_arrays(specs, seed):
    rng = np.random.RandomState(seed)
    out = []
    for s in specs:
        n = s["n"]
        m = np.zeros(n, np.float32) if s["fresh"] else (rng.standard_normal(n) * 0.01).astype(np.float32)
        v = np.zeros(n, np.float32) if s["fresh"] else ((rng.standard_normal(n) * 0.01) ** 2).astype(np.float32)
        out.append(dict(p=(rng.standard_normal(n) * 0.05).astype(np.float32), g=oc.seeded_grad(rng, (n,), s["gscale"]), m=m, v=v))
    return out


def _starts(specs, kind):
    starts, cursor = [], 0
    for s in specs:
        start = (cursor + 3) // 4 * 4 + (s["goff"] if kind == "g" else s["off"])
        starts.append(start)
        cursor = start + s["n"]
    return starts, cursor + 4


def launch(specs, arrs, mode, max_norm=0.0):
    """One optim_call on fresh device copies: each kind (p, g, m, v) is one flat buffer, every tensor a contiguous slice of it at
    its wanted alignment.  Returns numpy copies of everything afterwards."""
    flats, views = {}, {}
    for kind in "pgmv":
        starts, total = _starts(specs, kind)
        host = np.full(total, 777.0, np.float32)                              # (the gaps: a write outside a tensor shows)
        for s, a, st in zip(specs, arrs, starts):
            host[st:st + s["n"]] = a[kind]
        flats[kind] = torch.from_numpy(host).to(DEV)
        assert flats[kind].data_ptr() % 16 == 0
        views[kind] = [flats[kind][st:st + s["n"]] for s, st in zip(specs, starts)]
        for s, t in zip(specs, views[kind]):
            assert t.numel() == 0 or t.data_ptr() % 16 == 4 * (s["goff"] if kind == "g" else s["off"])
    rows = [(views["p"][i], views["g"][i] if s["grad"] else None, views["m"][i], views["v"][i], s["step"], s["lr"], s["wd"], s["betas"][0],
             s["betas"][1], s["eps"]) for i, s in enumerate(specs)]
    out = solver.optim_call(rows, mode, max_norm)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for kind in "pgmv":
        host = flats[kind].cpu().numpy()
        starts, _ = _starts(specs, kind)
        got[kind] = [host[st:st + s["n"]].copy() for s, st in zip(specs, starts)]
        mask = np.ones(host.size, bool)
        for s, st in zip(specs, starts):
            mask[st:st + s["n"]] = False
        assert (host[mask] == 777.0).all(), "a write outside the tensors of " + kind
    return got


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert x.tobytes() == y.tobytes(), (k, i)


def _frac(dev, ref, bound, what):
    """The worst |dev - ref| / bound; NaN exactly where the oracle has NaN."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), what + ": NaN elsewhere than the oracle"
    return oc.worst(np.abs(dev - ref)[~nan], np.asarray(bound, np.float64)[~nan])


def verify(specs, arrs, got, mode, max_norm, what, variant=None):
    """Everything a call leaves, against the oracle.  Returns the worst fractions of the bounds {norm, coef, m, v, p}; asserts
    what must hold exactly.  variant: measure against a wrong restatement instead (nothing is asserted exactly then)."""
    grads = [a["g"] if s["grad"] and s["n"] else None for s, a in zip(specs, arrs)]
    frac = dict(norm=0.0, coef=0.0, m=0.0, v=0.0, p=0.0)
    applied = 1.0
    if mode != solver.STEP:
        clip = oc.clip_fp64(grads, max_norm if max_norm > 0 else 1.0)
        if max_norm > 0:
            applied = clip["applied"]
        for i, n in enumerate(clip["norms"]):
            if n is None:
                assert got["norms"][i] == 0.0, (what, i)
            elif np.isnan(n) or np.isinf(n):
                assert np.isnan(got["norms"][i]) if np.isnan(n) else np.isinf(got["norms"][i])
            else:
                frac["norm"] = max(frac["norm"], abs(float(got["norms"][i]) - n) / (2 * U * n) if n else float(got["norms"][i] != 0))
        if np.isnan(clip["total"]):
            assert np.isnan(got["total_norm"])
        elif np.isinf(clip["total"]):
            assert np.isinf(got["total_norm"])
        else:
            frac["norm"] = max(frac["norm"], abs(float(got["total_norm"]) - clip["total"]) / (2 * U * clip["total"]) if clip["total"] else 0.0)
        if max_norm > 0:
            assert got["coef"].dtype == np.float32 and float(got["coef"]) <= 1.0
            frac["coef"] = abs(float(got["coef"]) - applied) / (4 * U * applied) if applied else float(got["coef"] != 0)
    for i, (s, a) in enumerate(zip(specs, arrs)):
        updated = mode in (solver.STEP, solver.CLIP_STEP) and grads[i] is not None
        if mode == solver.CLIP and grads[i] is not None and variant is None:
            want = a["g"] * got["coef"] if float(got["coef"]) != 1.0 else a["g"]          # one fp32 multiply by the device's own coefficient
            assert np.array_equal(got["g"][i], want, equal_nan=True), (what, i, "scaled gradient")
        elif variant is None:
            assert got["g"][i].tobytes() == a["g"].tobytes(), (what, i, "the gradient must be left as it is")
        if not updated:
            if variant is None:
                for k in "pmv":
                    assert got[k][i].tobytes() == a[k].tobytes(), (what, i, k, "must be untouched")
            continue
        o = oc.adam_fp64(a["p"], a["g"], a["m"], a["v"], s["step"], s["lr"], s["wd"], s["betas"], s["eps"], coef=applied if mode == solver.CLIP_STEP else 1.0,
                         variant=variant)
        right = o if variant is None else oc.adam_fp64(a["p"], a["g"], a["m"], a["v"], s["step"], s["lr"], s["wd"], s["betas"], s["eps"],
                                                        coef=applied if mode == solver.CLIP_STEP else 1.0)
        for k in "pmv":
            if variant is None:
                frac[k] = max(frac[k], _frac(got[k][i], o[k], right["bound_" + k], "%s tensor %d %s" % (what, i, k)))
            else:
                with np.errstate(all="ignore"):
                    frac[k] = max(frac[k], oc.worst(np.abs(got[k][i].astype(np.float64) - o[k]), right["bound_" + k]))
    return frac


def check(specs, seed, mode, max_norm, what, report=None, key=None, arrs=None):
    arrs = host_arrays(specs, seed) if arrs is None else arrs
    got, again = launch(specs, arrs, mode, max_norm), launch(specs, arrs, mode, max_norm)
    frac = verify(specs, arrs, got, mode, max_norm, what)
    line = ("%-16s %4d tensors %8d elements  total norm %-12.7g coef %-11.8g  fraction of the bound: norm %.3f  coef %.3f  m %.3f  v %.3f  p %.3f"
            % (what, len(specs), sum(s["n"] for s in specs), float(got.get("total_norm", np.nan)), float(got.get("coef", np.nan)),
               frac["norm"], frac["coef"], frac["m"], frac["v"], frac["p"]))
    print("PARITY " + line)
    if report is not None:
        report[key or what] = line
    same_bits(got, again)                                                     # two calls give the same bits
    assert max(frac.values()) <= 1.0, (what, frac)
    return arrs, got, frac


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------

def sizes_specs():
    """0, 1, 3, 4, 5, 63..65, 255..257, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 3 and 16 CHUNK + 5 elements; 300 tensors of one element
    scattered among them; slices 4, 8 and 12 bytes past a 16-byte boundary (and one whose gradient alone is); a tensor without a
    gradient first, in the middle and last."""
    main = [spec(n) for n in (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 16 * C + 5)]
    main += [spec(C + 7, off=1), spec(2 * C + 2, off=2), spec(301, off=3), spec(C + 9, off=0, goff=2), spec(70, off=2, goff=0)]
    main += [spec(1000, wd=0.0, lr=3e-3, step=7), spec(129, betas=(0.5, 0.9), eps=1e-3, step=2)]
    out = [spec(37, grad=False)]
    ones = 0
    for i, s in enumerate(main):
        out.append(s)
        for _ in range(13):
            out.append(spec(1, step=1 + ones % 3, wd=(0.0, 5e-4)[ones % 2]))
            ones += 1
        if i == len(main) // 2:
            out.append(spec(C + 1, grad=False))
    while ones < 300:
        out.append(spec(1))
        ones += 1
    out.append(spec(5, grad=False))
    assert ones == 300 and not out[0]["grad"] and not out[-1]["grad"]
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_sizes_case_in_every_mode(mode, parity_report):
    specs = sizes_specs()
    _, got, _ = check(specs, 9000, MODES[mode], 0.0 if mode == "step" else 5.0, "sizes/" + mode, parity_report)
    if mode != "step":
        assert float(got["coef"]) < 0.1                                       # total norm ~ 400: clipped


# ---- hyper-parameters ----------------------------------------------------------------------------------------------------------------

def hyper_specs():
    out = []
    for lr in (0.0, 1e-4, 3e-2):
        for wd in (0.0, 5e-4):
            for betas in ((0.9, 0.999), (0.5, 0.9)):
                for eps in (1e-8, 1e-3):
                    out.append(spec(97 + len(out), lr=lr, wd=wd, betas=betas, eps=eps, step=(1, 2, 1000)[len(out) % 3], gscale=0.1))
    return out


def test_hyper_parameters_per_tensor_and_sensitivity(parity_report):
    """lr (0 included), weight_decay, betas, eps and step (1, 2, 1000) differ from tensor to tensor in one call.  The same device
    result misses the AdamW-style and the no-bc2 restatements by more than 10 bounds: the bounds can tell the variants apart."""
    specs = hyper_specs()
    arrs, got, _ = check(specs, 9001, solver.CLIP_STEP, 5.0, "hyper", parity_report)
    for i, s in enumerate(specs):
        if s["lr"] == 0.0:
            assert got["p"][i].tobytes() == arrs[i]["p"].tobytes()
    for variant in ("adamw", "no_bc2", "eps_in_sqrt"):
        miss = verify(specs, arrs, got, solver.CLIP_STEP, 5.0, "hyper/" + variant, variant=variant)
        print("hyper against the %s restatement: p misses by %.3g bounds" % (variant, miss["p"]))
        assert miss["p"] > 10
    check(specs, 9001, solver.STEP, 0.0, "hyper/step")


# ---- clipping ------------------------------------------------------------------------------------------------------------------------

def _clip_specs():
    return [spec(C + 5, fresh=True), spec(300, wd=0.0, fresh=True), spec(64, fresh=True), spec(7, grad=False)]


def test_clip_above_below_and_at_max_norm(parity_report):
    specs = _clip_specs()
    arrs = host_arrays(specs, 9002)
    total = oc.clip_fp64([a["g"] if s["grad"] else None for s, a in zip(specs, arrs)], 1.0)["total"]
    for name, max_norm in (("above", total / 1000.0), ("below", total * 1000.0), ("equal", total + 1e-6)):
        for mode in (solver.CLIP_STEP, solver.CLIP):
            _, got, _ = check(specs, 9002, mode, max_norm, "clip/" + name, parity_report if mode == solver.CLIP_STEP else None, arrs=arrs)
            if name == "below":
                assert float(got["coef"]) == 1.0
            if name == "above":
                assert abs(float(got["coef"]) - 1e-3) < 1e-8


def test_one_nan_gradient():
    """The coefficient NaN is not < 1: the applied coefficient is exactly 1, and the NaN reaches exactly that element's p, m, v."""
    specs = _clip_specs()
    arrs = host_arrays(specs, 9003)
    arrs[0]["g"][C + 1] = np.nan
    for mode in (solver.CLIP_STEP, solver.CLIP, solver.NORMS):
        got, again = launch(specs, arrs, mode, 5.0), launch(specs, arrs, mode, 5.0)
        same_bits(got, again)
        assert float(got["coef"]) == 1.0 and np.isnan(got["total_norm"]) and np.isnan(got["norms"][0]) and np.isfinite(got["norms"][1:]).all()
        frac = verify(specs, arrs, got, mode, 5.0, "nan")
        print("one NaN gradient, mode %d: fractions %s" % (mode, frac))
        assert max(frac.values()) <= 1.0
        if mode == solver.CLIP_STEP:
            for k in "pmv":
                hit = [np.flatnonzero(np.isnan(x)).tolist() for x in got[k]]
                assert hit == [[C + 1], [], [], []], (k, hit)


def test_one_inf_gradient():
    """The total is Inf, the coefficient 0: that element's g' is Inf * 0 = NaN; every other element sees g' = weight_decay * p exactly."""
    specs = _clip_specs()
    arrs = host_arrays(specs, 9004)
    arrs[1]["g"][17] = np.inf
    got, again = launch(specs, arrs, solver.CLIP_STEP, 5.0), launch(specs, arrs, solver.CLIP_STEP, 5.0)
    same_bits(got, again)
    assert float(got["coef"]) == 0.0 and np.isinf(got["total_norm"]) and np.isinf(got["norms"][1]) and np.isfinite(got["norms"][0])
    for k in "pmv":
        assert [np.flatnonzero(np.isnan(x)).tolist() for x in got[k]] == [[], [17], [], []], k
    f32 = np.float32
    for i, s in enumerate(specs[:3]):
        keep = np.ones(s["n"], bool)
        if i == 1:
            keep[17] = False
        f64 = np.float64
        gp = f64(f32(s["wd"])) * arrs[i]["p"].astype(f64)                     # g' = +-0 + wd p, exact in double
        m = (f64(f32(1.0 - s["betas"][0])) * gp).astype(f32)                  # state starts at zero: (1 - beta1) g', rounded to fp32 once
        v = ((f64(f32(1.0 - s["betas"][1])) * gp) * gp).astype(f32)
        assert np.array_equal(got["m"][i][keep], m[keep]) and np.array_equal(got["v"][i][keep], v[keep]), i
        if s["wd"] == 0.0:
            assert not got["m"][i][keep].any() and got["p"][i][keep].tobytes() == arrs[i]["p"][keep].tobytes()
    frac = verify(specs, arrs, got, solver.CLIP_STEP, 5.0, "inf")
    assert max(frac.values()) <= 1.0, frac
    # in place: the Inf gradient becomes NaN in memory, the others 0
    got = launch(specs, arrs, solver.CLIP, 5.0)
    assert np.isnan(got["g"][1][17]) and not got["g"][0].any() and not np.delete(got["g"][1], 17).any()


def test_zero_gradient_without_decay_leaves_p_and_lets_the_state_decay():
    specs = [spec(C + 3, wd=0.0, fresh=True), spec(500, wd=0.0), spec(200)]
    arrs = host_arrays(specs, 9005)
    arrs[0]["g"][:] = 0.0
    arrs[1]["g"][:] = 0.0
    for mode in (solver.STEP, solver.CLIP_STEP):
        got, again = launch(specs, arrs, mode, 5.0), launch(specs, arrs, mode, 5.0)
        same_bits(got, again)
        assert got["p"][0].tobytes() == arrs[0]["p"].tobytes() and not got["m"][0].any() and not got["v"][0].any()     # nothing contributes
        assert np.array_equal(got["m"][1], (np.float32(0.9) * arrs[1]["m"]).astype(np.float32))                        # m, v decay
        assert np.array_equal(got["v"][1], (np.float32(0.999) * arrs[1]["v"]).astype(np.float32))
        assert max(verify(specs, arrs, got, mode, 5.0, "zero").values()) <= 1.0


# ---- the Python layer: Adam, clip_grad_norm --------------------------------------------------------------------------------------------

def _params(seed, shapes=((33, 7), (C + 11,), (5,), (2, 3, 4), (1,))):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((0.05 * torch.randn(s, generator=gen)).to(DEV)) for s in shapes]


def _set_grads(params, seed, scale=1.0, absent=()):
    rng = np.random.RandomState(seed)
    for i, p in enumerate(params):
        g = oc.seeded_grad(rng, tuple(p.shape), scale)
        p.grad = None if i in absent else torch.from_numpy(g).to(DEV)


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append(dict(p=p.detach().cpu().numpy().copy(), g=None if p.grad is None else p.grad.cpu().numpy().copy(),
                        m=st["exp_avg"].cpu().numpy().copy() if st else np.zeros(tuple(p.shape), np.float32),
                        v=st["exp_avg_sq"].cpu().numpy().copy() if st else np.zeros(tuple(p.shape), np.float32),
                        step=int(st["step"]) if st else 0))
    return out


def _group_of(opt, p):
    return next(g for g in opt.param_groups if any(q is p for q in g["params"]))


def _oracle_step(opt, params, before, max_norm=None, lr_of=None):
    """adam_fp64 of every parameter that had a gradient, from the snapshot taken before the step."""
    applied = 1.0 if max_norm is None else oc.clip_fp64([b["g"] for b in before], max_norm)["applied"]
    out = []
    for p, b in zip(params, before):
        if b["g"] is None:
            out.append(None)
            continue
        g = _group_of(opt, p)
        out.append(oc.adam_fp64(b["p"], b["g"], b["m"], b["v"], b["step"] + 1, g["lr"] if lr_of is None else lr_of(g), g["weight_decay"], g["betas"], g["eps"], coef=applied))
    return out


def _worst_against(opt, params, oracle, before):
    after = _snapshot(opt, params)
    worst, each = 0.0, dict(p=0.0, m=0.0, v=0.0)
    for o, a, b in zip(oracle, after, before):
        if o is None:
            assert a["p"].tobytes() == b["p"].tobytes() and a["m"].tobytes() == b["m"].tobytes() and a["step"] == b["step"]
            continue
        assert a["step"] == b["step"] + 1
        for k in "pmv":
            each[k] = max(each[k], _frac(a[k], o[k], o["bound_" + k], k))
    print("  fraction of the bound: m %.3f  v %.3f  p %.3f" % (each["m"], each["v"], each["p"]))
    _worst_against.each = each
    return max(each.values())


# The interchange test holds the step here AND torch's own step to the issue's bounds (1 x) against the float64 step both restate, and
# the two fp32 results to the same bounds against each other for exp_avg and exp_avg_sq (measured 0.25).  For p the two fp32 results are
# held to twice the bound, which is what two values each within the bound of the float64 one can be apart, and no less can be asked of
# two fp32 numbers: p's bound is u |p| plus a term for the update (a few per cent of it at these learning rates), two DIFFERENT fp32
# numbers are at least one ulp apart, and one ulp is between u |p| and 2u |p|.  So against another fp32 result the gap is either 0 or
# above the 1 x bound in the lower part of every binade, however either side rounds.  Measured on an MI355X: 1.31 x (torch's state
# stepped here) and 1.29 x (this state stepped by torch), one ulp each; exp_avg 0.25 and exp_avg_sq 0.26 of their bounds.
P_GAP_FP32 = 2.0


def _gap_to_torch(ours, ours_p, theirs, torch_p, oracle):
    """The step here against torch.optim.Adam's own step from the same state, in fp32 both: |here - torch| as a fraction of the
    issue's bounds (1 x), p, exp_avg and exp_avg_sq, worst element of each."""
    gap = dict(p=0.0, m=0.0, v=0.0)
    for a, b, o in zip(ours_p, torch_p, oracle):
        if o is None:
            continue
        pairs = dict(p=(a.detach(), b.detach()), m=(ours.state[a]["exp_avg"], theirs.state[b]["exp_avg"]),
                     v=(ours.state[a]["exp_avg_sq"], theirs.state[b]["exp_avg_sq"]))
        for k, (x, y) in pairs.items():
            gap[k] = max(gap[k], oc.worst(np.abs(x.cpu().numpy().astype(np.float64) - y.cpu().numpy()), o["bound_" + k]))
    return gap


def _per_param_groups(params):
    return [dict(params=[p], lr=(1e-3, 2e-3, 5e-4)[i % 3], weight_decay=(5e-4, 0.0)[i % 2]) for i, p in enumerate(params)]


def test_a_step_that_lags_uses_its_own_count():
    """Parameter 3 has no gradient at iterations 1 and 2: at the third its step is 1 and the others' 3 (bias corrections of its own
    count); every iteration is held to the one-step bounds."""
    params = _params(9100)
    opt = solver.Adam(_per_param_groups(params))
    for it in range(3):
        _set_grads(params, 9110 + it, absent=(3,) if it < 2 else ())
        before = _snapshot(opt, params)
        total = opt.clip_and_step(5.0) if it % 2 == 0 else opt.step()          # (step() returns None)
        worst = _worst_against(opt, params, _oracle_step(opt, params, before, 5.0 if it % 2 == 0 else None), before)
        print("iteration %d: worst fraction of the bounds %.3f" % (it + 1, worst))
        assert worst <= 1.0
        if total is not None:
            ref = oc.clip_fp64([b["g"] for b in before], 5.0)["total"]
            assert total.shape == () and total.is_cuda and abs(float(total) - ref) <= 2 * U * ref
    assert [int(opt.state[p]["step"]) for p in params] == [3, 3, 3, 1, 3]
    assert all(opt.state[p]["step"].device.type == "cpu" for p in params)
    # the wrong count would show: the oracle on the global count misses by more than 10 bounds
    group = _group_of(opt, params[3])
    wrong = oc.adam_fp64(before[3]["p"], before[3]["g"], before[3]["m"], before[3]["v"], 3, group["lr"], group["weight_decay"], group["betas"],
                         group["eps"], coef=oc.clip_fp64([b["g"] for b in before], 5.0)["applied"])
    right = _oracle_step(opt, params, before, 5.0)[3]
    assert oc.worst(np.abs(params[3].detach().cpu().numpy().astype(np.float64) - wrong["p"]), right["bound_p"]) > 10


def _copies(events):
    """(memcpy calls of the runtime, device activities named as device->host copies), as tests/test_boxloss_gpu.py counts them."""
    runtime = sum(1 for e in events if e.name.startswith(("hipMemcpy", "cudaMemcpy")))
    named = sum(1 for e in events if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    return runtime, named


def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    print("  memcpy events: %s" % sorted({e.name for e in ev if "emcpy" in e.name}))
    # (the runtime's own copy kernels, by which it may carry out a memcpy call, are that call's and not a launch of ours)
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name
               and "__amd_rocclr_" not in e.name and not e.name.startswith("Optimizer.step#")]      # (torch's own range around step(), no kernel)
    print("  kernels: %s" % [k[:60] for k in kernels])
    return (len(kernels), sum(1 for k in kernels if "optim_" in k)) + _copies(ev)


def test_launches_and_copies_gradients_kept_or_scaled():
    """step(): 1 launch; clip_and_step(): 2; clip_grad_norm: 1 without clip, 2 with; each with the one host-to-device upload of
    the tables and no device->host copy, whatever the number of tensors.  verbose=True: one copy, and the reference's lines.
    clip_and_step leaves the gradients as they are, clip_grad_norm(clip=True) scales them, and a second call sees the reduced norm."""
    x = torch.zeros(1000, device=DEV)
    control = _profile(lambda: x.sum().item())                               # the positive control: a read-back is a memcpy call of the runtime
    print("a read-back: (kernels, optim kernels, memcpy calls, copies named device->host) %s" % (control,))
    assert control[2] >= 1 and control[1] == 0
    for n_extra in (0, 60):
        params = _params(9200, ((33, 7), (C + 11,), (5,)) + ((3,),) * n_extra)
        named = [("p%d" % i, p) for i, p in enumerate(params)]
        opt = solver.Adam(_per_param_groups(params))
        log = oc.Log()
        _set_grads(params, 9201)
        opt.clip_and_step(5.0), opt.step(), solver.clip_grad_norm(named, 1e9, log)         # warm-up: code objects, workspace, staging
        g0 = [p.grad.clone() for p in params]
        got = {"step": _profile(opt.step), "clip_and_step": _profile(lambda: opt.clip_and_step(5.0)),
               "norm": _profile(lambda: solver.clip_grad_norm(named, 5.0, log)),
               "clip": _profile(lambda: solver.clip_grad_norm(named, 5.0, log, clip=True))}
        print("%d tensors: (kernels, optim kernels, memcpy calls, device->host copies) %s" % (len(params), got))
        assert got == {"step": (1, 1, 1, 0), "clip_and_step": (2, 2, 1, 0), "norm": (1, 1, 1, 0), "clip": (2, 2, 1, 0)}
        assert not log.lines
    # the gradients: untouched by the three calls before the last, scaled by the last
    total = oc.clip_fp64([g.cpu().numpy() for g in g0], 5.0)
    for g, p in zip(g0, params):
        assert not torch.equal(g, p.grad)
    scaled = [p.grad.cpu().numpy() for p in params]
    for g, s in zip(g0, scaled):
        assert np.abs(s.astype(np.float64) - total["applied"] * g.cpu().numpy()).max() <= 4 * U * np.abs(s).max()
    params2 = _params(9200, ((33, 7), (C + 11,), (5,)) + ((3,),) * 60)
    _set_grads(params2, 9201)
    opt2 = solver.Adam(_per_param_groups(params2))
    keep = [p.grad.clone() for p in params2]
    opt2.clip_and_step(5.0)
    assert all(torch.equal(a, p.grad) for a, p in zip(keep, params2))
    # a second clip_grad_norm sees the reduced norm; verbose reads back once and logs the reference's lines
    ran = _profile(lambda: log.lines.append(solver.clip_grad_norm(named, 5.0, log, clip=True, verbose=True)))
    second = log.lines.pop()
    ref = float(np.sqrt(sum(np.sum(s.astype(np.float64) ** 2) for s in scaled)))
    print("second norm %.9g, float64 of the scaled gradients %.9g, first %.9g" % (float(second), ref, total["total"]))
    assert abs(float(second) - ref) <= 2 * U * ref and float(second) < 5.0 * (1 + 1e-6) < total["total"]
    assert ran[3] >= 1 or ran[2] >= 2
    assert len(log.lines) == len(params) + 2 and log.lines[0].startswith("---Total norm %.5f clip coef " % float(second))
    name, rest = log.lines[1].split(": ")
    assert name == "{:<50s}".format("p0") and rest.endswith(", ({})".format(params[0].size()))
    assert abs(float(rest.split(",")[0]) - float(np.sqrt(np.sum(scaled[0].astype(np.float64) ** 2)))) <= 1e-5
    assert log.lines[-1] == "-------------------------------"


def test_state_dict_interchange_with_torch_adam_both_ways_and_lr_changes():
    def pair():
        a, b = _params(9300), _params(9300)
        return a, b, solver.Adam(_per_param_groups(a)), torch.optim.Adam(_per_param_groups(b), foreach=False)      # torch's single-tensor form

    # torch for two steps, then one step here from its state_dict
    ours_p, torch_p, ours, theirs = pair()
    for it in range(2):
        _set_grads(torch_p, 9310 + it, absent=(2,) if it == 0 else ())
        theirs.step()
    with torch.no_grad():
        for a, b in zip(ours_p, torch_p):
            a.copy_(b)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))       # (torch hands the `step` tensors over as they are: a copy keeps the two apart)
    _set_grads(torch_p, 9312)
    _set_grads(ours_p, 9312)
    before = _snapshot(ours, ours_p)
    assert [b["step"] for b in before] == [2, 2, 1, 2, 2]
    ours.step()
    theirs.step()
    oracle = _oracle_step(ours, ours_p, before)
    worst = _worst_against(ours, ours_p, oracle, before)
    torch_worst = _worst_against(theirs, torch_p, oracle, before)
    gap = _gap_to_torch(ours, ours_p, theirs, torch_p, oracle)
    print("torch -> here: fraction of the bounds against the float64 step: here %.3f, torch %.3f; here against torch's own third step, fp32 both: p %.3f  m %.3f  v %.3f"
          % (worst, torch_worst, gap["p"], gap["m"], gap["v"]))
    assert worst <= 1.0 and torch_worst <= 1.0
    assert gap["m"] <= 1.0 and gap["v"] <= 1.0 and gap["p"] <= P_GAP_FP32, gap
    # here for two steps, then torch's third step from this state_dict
    ours_p, torch_p, ours, theirs = pair()
    for it in range(2):
        _set_grads(ours_p, 9320 + it, absent=(4,) if it == 1 else ())
        ours.step()
    with torch.no_grad():
        for a, b in zip(ours_p, torch_p):
            b.copy_(a)
    theirs.load_state_dict(copy.deepcopy(ours.state_dict()))
    assert [float(theirs.state[p]["step"]) for p in torch_p] == [2, 2, 2, 2, 1]
    _set_grads(torch_p, 9322)
    _set_grads(ours_p, 9322)
    before = _snapshot(ours, ours_p)
    ours.step()
    theirs.step()
    oracle = _oracle_step(ours, ours_p, before)
    worst = _worst_against(ours, ours_p, oracle, before)
    torch_worst = _worst_against(theirs, torch_p, oracle, before)
    gap = _gap_to_torch(ours, ours_p, theirs, torch_p, oracle)
    print("here -> torch: fraction of the bounds against the float64 step: here %.3f, torch %.3f; here against torch's third step, fp32 both: p %.3f  m %.3f  v %.3f"
          % (worst, torch_worst, gap["p"], gap["m"], gap["v"]))
    assert worst <= 1.0 and torch_worst <= 1.0
    assert gap["m"] <= 1.0 and gap["v"] <= 1.0 and gap["p"] <= P_GAP_FP32, gap
    # a MultiStepLR-style change of group["lr"] between steps takes effect (a torch scheduler drives it)
    sched = torch.optim.lr_scheduler.MultiStepLR(ours, milestones=[1], gamma=0.1)
    old = [g["lr"] for g in ours.param_groups]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (torch warns when a scheduler steps before its optimizer has)
        sched.step()
    assert [g["lr"] for g in ours.param_groups] == pytest.approx([0.1 * lr for lr in old])
    _set_grads(ours_p, 9323)
    before = _snapshot(ours, ours_p)
    ours.clip_and_step(5.0)
    assert _worst_against(ours, ours_p, _oracle_step(ours, ours_p, before, 5.0), before) <= 1.0
    stale = _oracle_step(ours, ours_p, before, 5.0, lr_of=lambda g: g["lr"] * 10.0)
    right = _oracle_step(ours, ours_p, before, 5.0)
    assert min(oc.worst(np.abs(p.detach().cpu().numpy().astype(np.float64) - s["p"]), r["bound_p"]) for p, s, r in zip(ours_p, stale, right)) > 10


# ---- the predictor ---------------------------------------------------------------------------------------------------------------------

def test_predictor_trains_with_clip_and_step_and_eval_sees_the_new_weights(parity_report, monkeypatch):
    """A small VETOPredictor (L4/H8, 1 image x 4 objects, dropout off): three iterations of backward + clip_and_step(5.0), every
    parameter against the oracle fed the device's pre-step state and gradients.  Then in eval mode, without refresh_weights(),
    the logits equal bit for bit those of a fresh predictor loaded from the stepped state_dict: the step bumped the parameters'
    version counters.  A step whose bump is suppressed leaves the engine on the old weights."""
    from veto_amd import synth, testing
    from veto_amd.pairs import prepare_test_pairs
    dev = torch.device("cuda:0")
    cfg = testing.make_config(4, 8)
    model = testing.make_predictor(cfg, synth.predictor_state_dict(0, layers=4), dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    batch = synth.synthetic_batch(7, 1, [4])
    props = testing.make_proposals(batch, "predcls", dev)
    pairs = prepare_test_pairs(dev, props)
    n = sum(int(p.shape[0]) for p in pairs)
    labels = torch.from_numpy(synth.integers(5, "optim.labels", (n,), 0, 51)).to(dev)
    rel_labels = list(labels.split([int(p.shape[0]) for p in pairs]))
    kw = dict(roi_features=torch.from_numpy(batch["roi_features"]).to(dev), roi_depth_features=torch.from_numpy(batch["roi_depth_features"]).to(dev))
    log = oc.Log()
    opt = solver.make_optimizer(cfg, model, log)
    params = [p for g in opt.param_groups for p in g["params"]]
    assert type(opt) is solver.Adam and len(params) == len(opt.param_groups) == sum(1 for p in model.parameters() if p.requires_grad)
    worst_all, totals = dict(m=0.0, v=0.0, p=0.0), []
    for it in range(3):
        opt.zero_grad(set_to_none=True)
        model(props, pairs, rel_labels, None, **kw)[2]["rel_loss"].backward()
        before = _snapshot(opt, params)
        versions = [p._version for p in params]
        total = opt.clip_and_step(5.0)
        oracle = _oracle_step(opt, params, before, 5.0)
        worst = _worst_against(opt, params, oracle, before)
        ref = oc.clip_fp64([b["g"] for b in before], 5.0)
        totals.append(float(total))
        print("iteration %d: %d of %d tensors have a gradient, total norm %.7g (float64 %.7g), worst fraction of the bounds %.3f"
              % (it + 1, sum(o is not None for o in oracle), len(params), float(total), ref["total"], worst))
        assert abs(float(total) - ref["total"]) <= 2 * U * ref["total"] and worst <= 1.0
        assert all((p._version > v) == (o is not None) for p, v, o in zip(params, versions, oracle))
        worst_all = {k: max(worst_all[k], _worst_against.each[k]) for k in worst_all}
    parity_report["predictor"] = ("%-16s %4d tensors %8d elements  total norms %s  fraction of the bound, worst of 3 iterations: m %.3f  v %.3f  p %.3f"
                                  % ("predictor", len(params), sum(p.numel() for p in params), " ".join("%.7g" % t for t in totals),
                                     worst_all["m"], worst_all["v"], worst_all["p"]))

    def logits():
        with torch.no_grad():
            out = model(props, pairs, None, None, **kw)[1][0]
        torch.cuda.synchronize()
        return out.cpu().numpy()

    model.eval()
    a = logits()                                                              # the engine now holds the stepped weights, stamped
    with monkeypatch.context() as mp:
        mp.setattr(torch.autograd.graph, "increment_version", lambda tensors: None)
        opt.clip_and_step(5.0)                                                # the gradients of the third iteration are still there
    stale = logits()
    assert stale.tobytes() == a.tobytes()                                     # without the bump the write through raw pointers goes unseen
    opt.clip_and_step(5.0)
    b = logits()
    assert b.tobytes() != a.tobytes()
    fresh = testing.make_predictor(cfg, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, dev)
    with torch.no_grad():
        c = fresh(props, pairs, None, None, **kw)[1][0].cpu().numpy()
    assert b.tobytes() == c.tobytes()
