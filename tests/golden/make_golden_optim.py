"""Writes tests/golden/optim/*.npz: what the reference's own clip_grad_norm (pysgg/utils/checkpoint.py:180-219) and the
torch.optim.Adam its make_optimizer returns (pysgg/solver/build.py:7-34) compute on CPU tensors, in fp32 and in float64, after 1
and after 3 iterations of a case of tests/optim_cases.py (clip_grad_norm(clip=True), then optimizer.step()).

The inputs are regenerated from tests/optim_cases.py, so a fixture stores outputs only: per k in (1, 3) the total norm that
iteration k returned and p, exp_avg, exp_avg_sq and the step counts after it, flattened in optim_cases.TRAINABLE order, of the
float64 run; the fp32 run's p after it; the group table (lr, weight_decay per parameter) and the logger's lines; and the
reference's own fp32-against-float64 error after ONE iteration as a fraction of the bounds of optim_cases.adam_fp64
(ref_fp32_err_m, _v, _p) and of the float64 norm (ref_fp32_err_norm).  Asserted per case: the float64 restatement
optim_cases.run_fp64 reproduces the float64 run.
Usage: python tests/golden/make_golden_optim.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402
import optim_cases as oc  # noqa: E402


def run_reference(name, dtype, n_steps):
    import types
    from pysgg.solver.build import make_optimizer
    if "pysgg.utils.model_zoo" not in sys.modules:   # checkpoint.py imports its downloader, whose torch.hub names are gone; nothing here downloads
        zoo = types.ModuleType("pysgg.utils.model_zoo")
        zoo.cache_url = None
        sys.modules["pysgg.utils.model_zoo"] = zoo
    from pysgg.utils.checkpoint import clip_grad_norm
    d = oc.case_inputs(name)
    model = oc.toy_module(d["params"], dtype)
    log = oc.Log()
    opt = make_optimizer(oc.solver_cfg(), model, log, slow_heads=list(oc.SLOW_HEADS), except_weight_decay=list(oc.EXCEPT_WD),
                         slow_ratio=oc.SLOW_RATIO, rl_factor=oc.RL_FACTOR)
    assert type(opt) is torch.optim.Adam
    named = dict(model.named_parameters())
    by_param = {id(g["params"][0]): g for g in opt.param_groups}
    table = np.array([[by_param[id(named[n])]["lr"], by_param[id(named[n])]["weight_decay"]] for n in oc.TRAINABLE], np.float64)
    for n, edits in d["groups"].items():
        by_param[id(named[n])].update(edits)
    total = None
    for it in range(n_steps):
        for n in oc.TRAINABLE:
            g = d["grads"][it]["present"][n]
            named[n].grad = None if g is None else torch.tensor(g, dtype=dtype)
        total = clip_grad_norm([(n, named[n]) for n in oc.TRAINABLE], d["max_norm"], log, clip=True)
        opt.step()
    zeros = {n: torch.zeros_like(named[n]) for n in oc.TRAINABLE}
    state = {n: opt.state.get(named[n], {}) for n in oc.TRAINABLE}
    return dict(total=float(total), p=oc.flat({n: named[n].detach().numpy() for n in oc.TRAINABLE}),
                m=oc.flat({n: state[n].get("exp_avg", zeros[n]).numpy() for n in oc.TRAINABLE}),
                v=oc.flat({n: state[n].get("exp_avg_sq", zeros[n]).numpy() for n in oc.TRAINABLE}),
                steps=np.array([float(state[n].get("step", 0.0)) for n in oc.TRAINABLE]), table=table, log=list(log.lines))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def main():
    import_reference()
    os.makedirs(oc.GOLDEN, exist_ok=True)
    for name in oc.ALL:
        z = {}
        for k in (1, 3):
            r32, r64 = run_reference(name, torch.float32, k), run_reference(name, torch.float64, k)
            o = oc.run_fp64(name, k)
            pin = max(rel(o["clip"]["total"], r64["total"]), rel(oc.flat(o["p"]), r64["p"]), rel(oc.flat(o["m"]), r64["m"]),
                      rel(oc.flat(o["v"]), r64["v"]))
            assert pin <= (1e-13 if k == 1 else 1e-11), (name, k, pin)
            assert [o["steps"][n] for n in oc.TRAINABLE] == r64["steps"].tolist(), name
            z.update({"total_fp64_%d" % k: np.float64(r64["total"]), "p_fp64_%d" % k: r64["p"], "m_fp64_%d" % k: r64["m"],
                      "v_fp64_%d" % k: r64["v"], "steps_%d" % k: r64["steps"], "p_fp32_%d" % k: r32["p"].astype(np.float32),
                      "total_fp32_%d" % k: np.float32(r32["total"]), "pin_%d" % k: np.float64(pin)})
            if k == 1:   # one iteration from the same fp32 state: the reference's own rounding in the metrics of the bounds
                def frac(key):
                    ref = np.concatenate([o["last"][n][key].reshape(-1) if n in o["last"] else np.zeros(o["p"][n].size) for n in oc.TRAINABLE])
                    bound = np.concatenate([o["last"][n]["bound_" + key].reshape(-1) if n in o["last"] else np.ones(o["p"][n].size) for n in oc.TRAINABLE])
                    got = {"p": r32["p"], "m": r32["m"], "v": r32["v"]}[key]
                    keep = np.concatenate([np.full(o["p"][n].size, n in o["last"]) for n in oc.TRAINABLE])
                    return oc.worst(np.abs(got - ref)[keep], bound[keep])
                z.update({"ref_fp32_err_m": np.float64(frac("m")), "ref_fp32_err_v": np.float64(frac("v")),
                          "ref_fp32_err_p": np.float64(frac("p")), "ref_fp32_err_norm": np.float64(rel(r32["total"], r64["total"]) / (2 * oc.U))})
                z["group_table"] = r64["table"]
                z["log"] = np.array(r64["log"])
        path = os.path.join(oc.GOLDEN, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, "total norm %.6g / %.6g" % (z["total_fp64_1"], z["total_fp64_3"]), "pin %.3g / %.3g" % (z["pin_1"], z["pin_3"]),
              "reference fp32 error as a fraction of the bound: norm %.3g m %.3g v %.3g p %.3g"
              % (z["ref_fp32_err_norm"], z["ref_fp32_err_m"], z["ref_fp32_err_v"], z["ref_fp32_err_p"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
