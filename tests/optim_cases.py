"""What the optimizer tests and tests/golden/make_golden_optim.py share: the toy module whose parameter names trigger every rule
of make_optimizer, the seeded cases, the fixture loader, the float64 numpy restatement of the reference's clip and of torch's Adam
step, and the bounds the device is held to.  No test lives here.

A case is the reference's iteration after backward(), three times over: clip_grad_norm(named, max_norm, logger, clip=True)
(pysgg/utils/checkpoint.py:180-219), then optimizer.step() of the torch.optim.Adam that make_optimizer builds
(pysgg/solver/build.py:7-34), with fresh seeded gradients at every step."""
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim")
U = 2.0 ** -24          # the unit roundoff of fp32
G_MIN, G_MAX = 1e-6, 1e2   # seeded gradients stay inside in magnitude: no g^2 leaves the fp32 normal range
N_STEPS = 3
VARIANTS = ("adamw", "eps_in_sqrt", "no_bc2", "global_step", "always_clip", "no_1e6", "none_counted")

# the toy module: (parameter name, shape).  "bias" in the name: BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS.  EXCEPT_WD and SLOW_HEADS
# are substring rules; "head.slow_embed.weight" matches both rules, two items of EXCEPT_WD (both are logged: that loop has no
# break) and two items of SLOW_HEADS (lr is divided ONCE: that loop breaks).
TOY = (("backbone.conv.weight", (8, 5)), ("backbone.conv.bias", (8,)), ("head.embed.weight", (6, 7)), ("head.slow_fc.weight", (5, 5)),
       ("head.slow_fc.bias", (5,)), ("head.slow_embed.weight", (9, 3)), ("head.out.weight", (4, 11)), ("head.frozen.weight", (3, 3)))
FROZEN = ("head.frozen.weight",)      # requires_grad False: no group
EXCEPT_WD = ("embed", "slow_embed")
SLOW_HEADS = ("slow", "slow_embed", "slow_fc")
SLOW_RATIO, RL_FACTOR = 5.0, 3.0
SOLVER = dict(BASE_LR=0.01, BIAS_LR_FACTOR=2.0, WEIGHT_DECAY=0.0005, WEIGHT_DECAY_BIAS=0.0)
TRAINABLE = tuple(n for n, _ in TOY if n not in FROZEN)

# seeded cases.  gscale: the gradients are N(0, gscale^2).  absent: {parameter name: the steps (1-based) at which its gradient is
# None}.  groups: {parameter name: keys set on its param group after make_optimizer returned}.
CASES = {
    "clip": dict(seed=8100, gscale=1.0, max_norm=5.0),                    # total norm ~ 15: clipped
    "below": dict(seed=8101, gscale=1e-3, max_norm=5.0),                  # total norm ~ 0.015: not clipped
    "tiny": dict(seed=8102, gscale=1e-3, max_norm=1e-3),                  # clipped at a total where the + 1e-6 shows
    "skips": dict(seed=8103, gscale=1.0, max_norm=5.0,
                  absent={"head.out.weight": (1, 2), "backbone.conv.bias": (2,), "head.embed.weight": (1, 2, 3)}),
    "hyper": dict(seed=8104, gscale=0.1, max_norm=5.0, absent={"head.slow_fc.bias": (1, 3)},
                  groups={"backbone.conv.weight": dict(betas=(0.5, 0.9), eps=1e-3), "backbone.conv.bias": dict(lr=0.0),
                          "head.out.weight": dict(eps=1e-3, weight_decay=0.0), "head.slow_fc.weight": dict(betas=(0.5, 0.9))}),
}
ALL = tuple(CASES)


def solver_cfg():
    return types.SimpleNamespace(SOLVER=types.SimpleNamespace(**SOLVER))


class Log(object):
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def toy_module(params, dtype):
    """A torch module whose named_parameters() are TOY, in that order, holding `params` ({name: array})."""
    import torch
    root = torch.nn.Module()
    for name, _ in TOY:
        *path, leaf = name.split(".")
        mod = root
        for part in path:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(leaf, torch.nn.Parameter(torch.tensor(params[name], dtype=dtype), requires_grad=name not in FROZEN))
    assert [n for n, _ in root.named_parameters()] == [n for n, _ in TOY]
    return root


def seeded_grad(rng, shape, gscale):
    g = rng.standard_normal(shape) * gscale
    return (np.where(g < 0, -1.0, 1.0) * np.clip(np.abs(g), G_MIN, G_MAX)).astype(np.float32)


def case_inputs(name):
    """dict(params {name: fp32 array}, grads [step][name] -> fp32 array or None, max_norm, groups)."""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    params = {n: (rng.standard_normal(s) * 0.05).astype(np.float32) for n, s in TOY}
    grads = []
    for step in range(1, N_STEPS + 1):
        g = {n: seeded_grad(rng, s, c["gscale"]) for n, s in TOY if n not in FROZEN}
        full = dict(g)
        for n, steps in c.get("absent", {}).items():
            if step in steps:
                g[n] = None
        grads.append(dict(present=g, full=full))
    return dict(params=params, grads=grads, max_norm=c["max_norm"], groups=c.get("groups", {}))


def reference_groups():
    """The group table solver/build.py:8-30 makes of TOY, restated: {name: (lr, weight_decay)}."""
    out = {}
    for n in TRAINABLE:
        lr, wd = SOLVER["BASE_LR"], SOLVER["WEIGHT_DECAY"]
        if "bias" in n:
            lr, wd = SOLVER["BASE_LR"] * SOLVER["BIAS_LR_FACTOR"], SOLVER["WEIGHT_DECAY_BIAS"]
        if any(item in n for item in EXCEPT_WD):
            wd = 0.0
        if any(item in n for item in SLOW_HEADS):
            lr = lr / SLOW_RATIO
        out[n] = (lr * RL_FACTOR, wd)
    return out


def case_hyper(name):
    """{parameter name: dict(lr, weight_decay, betas, eps)} of a case: the reference's groups with the case's edits."""
    out = {}
    for n, (lr, wd) in reference_groups().items():
        h = dict(lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
        h.update(CASES[name].get("groups", {}).get(n, {}))
        out[n] = h
    return out


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------

def clip_fp64(grads, max_norm, variant=None, stale=None):
    """checkpoint.py:194-211 in float64.  grads: a list of arrays or None (checkpoint.py:200: a None gradient is skipped).
    Returns dict(norms: a list with None where the gradient is None, total, coef: max_norm / (total + 1e-6), applied: coef where
    coef < 1 else 1.0 -- NaN < 1 is false).  variant: one of the wrong restatements ('always_clip', 'no_1e6', 'none_counted'
    with `stale`, the arrays counted in place of the None gradients)."""
    if variant == "none_counted":
        grads = [s if g is None else g for g, s in zip(grads, stale)]
    norms = [None if g is None else float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2))) for g in grads]
    total = 0.0
    for n in norms:                      # checkpoint.py:202: total_norm += param_norm ** 2
        if n is not None:
            total += n ** 2
    total = total ** 0.5
    with np.errstate(all="ignore"):
        coef = float(np.float64(max_norm) / (np.float64(total) + (0.0 if variant == "no_1e6" else 1e-6)))
    applied = coef if (coef < 1 or variant == "always_clip") else 1.0
    return dict(norms=norms, total=total, coef=coef, applied=applied)


def adam_fp64(p, g, m, v, step, lr, weight_decay, betas, eps, coef=1.0, variant=None):
    """One step of torch.optim.adam._single_tensor_adam (amsgrad, maximize, capturable, differentiable off) in float64 on the
    gradient coef * g, `step` counting this update:
      grad = grad.add(param, alpha=weight_decay); exp_avg.lerp_(grad, 1 - beta1);
      exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2); step_size = lr / (1 - beta1 ** step);
      denom = (exp_avg_sq.sqrt() / (1 - beta2 ** step) ** 0.5).add_(eps); param.addcdiv_(exp_avg, denom, value=-step_size)
    Returns the new p, m, v and what the bounds are made of: G_abs = |coef g| + wd |p|, M_abs = beta1 |m| + (1 - beta1) G_abs,
    denom, and the bounds themselves (bound_m, bound_v, bound_p: see the module text of tests/test_optim_gpu.py).
    variant: 'adamw' (decoupled decay), 'eps_in_sqrt', 'no_bc2'."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    with np.errstate(all="ignore"):
        gs = coef * g
        G_abs = np.abs(gs) + weight_decay * np.abs(p)
        if variant == "adamw":
            p = p * (1.0 - lr * weight_decay)
            gp = gs
        else:
            gp = gs + weight_decay * p if weight_decay != 0 else gs
        m_new = b1 * m + (1.0 - b1) * gp
        v_new = b2 * v + (1.0 - b2) * gp * gp
        bc1 = 1.0 - b1 ** step
        bc2 = 1.0 if variant == "no_bc2" else 1.0 - b2 ** step
        denom = np.sqrt(v_new / bc2 + eps) if variant == "eps_in_sqrt" else np.sqrt(v_new) / bc2 ** 0.5 + eps
        p_new = p - (lr / bc1) * (m_new / denom)
        M_abs = b1 * np.abs(m) + (1.0 - b1) * G_abs
        return dict(p=p_new, m=m_new, v=v_new, G_abs=G_abs, M_abs=M_abs, denom=denom,
                    bound_m=8 * U * M_abs, bound_v=8 * U * (b2 * v + (1.0 - b2) * G_abs ** 2),
                    bound_p=U * np.abs(p_new) + 32 * U * (lr / bc1) * M_abs / denom)


def run_fp64(name, n_steps, variant=None):
    """The case's first n_steps iterations in float64 from its fp32 inputs.  Returns dict(p, m, v, steps: {name: ...}, and of the
    LAST iteration: clip (clip_fp64's dict) and last ({name: adam_fp64's dict} of the parameters it updated))."""
    d = case_inputs(name)
    hyper = case_hyper(name)
    p = {n: d["params"][n].astype(np.float64) for n in TRAINABLE}
    m = {n: np.zeros_like(p[n]) for n in TRAINABLE}
    v = {n: np.zeros_like(p[n]) for n in TRAINABLE}
    steps = {n: 0 for n in TRAINABLE}
    clip = last = None
    for it in range(1, n_steps + 1):
        g = d["grads"][it - 1]["present"]
        clip = clip_fp64([g[n] for n in TRAINABLE], d["max_norm"], variant=variant, stale=[d["grads"][it - 1]["full"][n] for n in TRAINABLE])
        last = {}
        for n in TRAINABLE:
            if g[n] is None:
                continue
            steps[n] += 1
            h = hyper[n]
            o = adam_fp64(p[n], g[n], m[n], v[n], it if variant == "global_step" else steps[n], h["lr"], h["weight_decay"], h["betas"],
                          h["eps"], coef=clip["applied"], variant=variant)
            p[n], m[n], v[n], last[n] = o["p"], o["m"], o["v"], o
    return dict(p=p, m=m, v=v, steps=steps, clip=clip, last=last)


def flat(d):
    """{name: array} -> one float64 vector in TRAINABLE order."""
    return np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in TRAINABLE])


def load_case(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def worst(err, bound):
    """The largest err / bound over the elements (0 / 0 counts as 0; a miss of a zero bound as inf)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0
