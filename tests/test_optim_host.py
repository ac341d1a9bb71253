"""The device optimizer without a GPU: the fixtures of tests/golden/optim and the float64 restatement pinned to them, the group
table of veto_amd.solver.make_optimizer against the reference's, the ABI's refusals, the argument checks of the Python layer,
the state_dict interchange keys, the installer, and seven wrong restatements that the bounds tell apart."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402

from veto_amd import native, registry, solver  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "veto_amd.h")


# ---- fixtures and oracle -----------------------------------------------------------------------------------------------------------

def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


@pytest.mark.parametrize("name", oc.ALL)
def test_fixture_is_present_and_the_restatement_reproduces_the_float64_run(name):
    """After one iteration to 1e-13 relative (measured when the fixtures were made: at most 1.5e-14), after three to 1e-11 (at
    most 8e-14): total norm, p, exp_avg, exp_avg_sq, and the step counts exactly."""
    z = oc.load_case(name)
    for k, tol in ((1, 1e-13), (3, 1e-11)):
        o = oc.run_fp64(name, k)
        pin = max(_rel(o["clip"]["total"], z["total_fp64_%d" % k]), _rel(oc.flat(o["p"]), z["p_fp64_%d" % k]),
                  _rel(oc.flat(o["m"]), z["m_fp64_%d" % k]), _rel(oc.flat(o["v"]), z["v_fp64_%d" % k]))
        print("%s after %d: restatement against the float64 run %.3g (recorded %.3g)" % (name, k, pin, float(z["pin_%d" % k])))
        assert pin <= tol
        assert [float(o["steps"][n]) for n in oc.TRAINABLE] == z["steps_%d" % k].tolist()
    # the reference's own fp32 run sits inside the bounds the device is held to
    for key in ("ref_fp32_err_norm", "ref_fp32_err_m", "ref_fp32_err_v", "ref_fp32_err_p"):
        assert 0 <= float(z[key]) <= 1.0, (key, float(z[key]))


def test_cases_hold_what_they_are_named_for():
    for name in oc.ALL:
        z = oc.load_case(name)
        d = oc.case_inputs(name)
        coef = d["max_norm"] / (float(z["total_fp64_1"]) + 1e-6)
        assert (coef < 0.5) == (name in ("clip", "tiny", "skips")), (name, coef)
        if name == "below":
            assert coef > 100
        if name == "tiny":
            assert 1e-6 / float(z["total_fp64_1"]) > 10 * 4 * oc.U          # the + 1e-6 moves the coefficient by more than 10 bounds
    steps = dict(zip(oc.TRAINABLE, oc.load_case("skips")["steps_3"].tolist()))
    assert steps["head.out.weight"] == 1 and steps["backbone.conv.bias"] == 2 and steps["head.embed.weight"] == 0 and steps["head.slow_fc.weight"] == 3


def test_seeded_gradients_stay_in_the_normal_range_of_their_squares():
    """|g| in [1e-6, 1e2]: g^2 is a normal fp32 number, so the device's double sum and an fp32 sum see the same values."""
    for name in oc.ALL:
        for step in oc.case_inputs(name)["grads"]:
            for g in step["full"].values():
                assert g.dtype == np.float32 and oc.G_MIN * (1 - 1e-6) <= np.abs(g).min() and np.abs(g).max() <= oc.G_MAX
    rng = np.random.RandomState(0)
    g = oc.seeded_grad(rng, (4096,), 1e3)
    assert np.abs(g).max() == np.float32(oc.G_MAX) and np.abs(oc.seeded_grad(rng, (4096,), 1e-9)).min() == np.float32(oc.G_MIN)


def test_group_table_matches_the_reference_name_by_name():
    """veto_amd.solver.make_optimizer on the toy module: lr and weight_decay of every group and the logger's lines equal what the
    reference's make_optimizer produced (stored in the fixture), and the restated table of optim_cases equals both."""
    z = oc.load_case("clip")
    model = oc.toy_module(oc.case_inputs("clip")["params"], torch.float32)
    log = oc.Log()
    opt = solver.make_optimizer(oc.solver_cfg(), model, log, slow_heads=list(oc.SLOW_HEADS), except_weight_decay=list(oc.EXCEPT_WD),
                                slow_ratio=oc.SLOW_RATIO, rl_factor=oc.RL_FACTOR)
    assert type(opt) is solver.Adam and isinstance(opt, torch.optim.Optimizer)
    named = dict(model.named_parameters())
    assert len(opt.param_groups) == len(oc.TRAINABLE)
    restated = oc.reference_groups()
    for group, name, want in zip(opt.param_groups, oc.TRAINABLE, z["group_table"].tolist()):
        assert len(group["params"]) == 1 and group["params"][0] is named[name], name
        assert [group["lr"], group["weight_decay"]] == want == list(restated[name]), (name, group["lr"], group["weight_decay"], want)
        assert group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8
    assert log.lines == z["log"].tolist()
    # every rule is hit: the bias pair, no decay, a slow head, both at once -- with two matching items each, divided once
    table = dict(zip(oc.TRAINABLE, z["group_table"].tolist()))
    assert table["backbone.conv.weight"] == [0.01 * 3.0, 0.0005] and table["backbone.conv.bias"] == [0.01 * 2.0 * 3.0, 0.0]
    assert table["head.embed.weight"] == [0.01 * 3.0, 0.0] and table["head.slow_fc.weight"] == [0.01 / 5.0 * 3.0, 0.0005]
    assert table["head.slow_embed.weight"] == [0.01 / 5.0 * 3.0, 0.0]
    assert sum("NO WEIGHT DECAY: head.slow_embed.weight" in line for line in log.lines) == 2
    assert sum("SLOW HEADS: head.slow_embed.weight" in line for line in log.lines) == 1


# ---- seven wrong restatements ------------------------------------------------------------------------------------------------------

def _miss(name, k, variant):
    """How far the restatement (a wrong one with `variant`) is from the fixture's float64 run after k iterations, as a multiple of
    the bounds: p, m, v of the parameters the last iteration updated, and the total norm (2u relative)."""
    z = oc.load_case(name)
    good, got = oc.run_fp64(name, k), oc.run_fp64(name, k, variant)
    keep = np.concatenate([np.full(good["p"][n].size, n in good["last"]) for n in oc.TRAINABLE])
    out = abs(got["clip"]["total"] - float(z["total_fp64_%d" % k])) / (2 * oc.U * float(z["total_fp64_%d" % k]))
    for key in ("p", "m", "v"):
        bound = np.concatenate([good["last"][n]["bound_" + key].reshape(-1) if n in good["last"] else np.ones(good["p"][n].size) for n in oc.TRAINABLE])
        out = max(out, oc.worst(np.abs(oc.flat(got[key]) - z["%s_fp64_%d" % (key, k)])[keep], bound[keep]))
    return out


@pytest.mark.parametrize("variant,name,k", [("adamw", "clip", 1), ("eps_in_sqrt", "hyper", 1), ("no_bc2", "clip", 1), ("global_step", "skips", 3),
                                            ("always_clip", "below", 1), ("no_1e6", "tiny", 1), ("none_counted", "skips", 1)])
def test_a_wrong_restatement_misses_a_fixture_by_more_than_ten_bounds(variant, name, k):
    assert set(v for v in oc.VARIANTS) >= {variant}
    right, wrong = _miss(name, k, None), _miss(name, k, variant)
    print("%s on %s after %d: %.3g bounds (the right restatement: %.3g)" % (variant, name, k, wrong, right))
    assert right <= 1e-3 and wrong > 10


def test_clip_restatement_edges():
    """NaN < 1 is false: the applied coefficient is 1; an Inf norm gives 0; a None gradient is skipped."""
    g = [np.array([3.0, 4.0], np.float32), None]
    o = oc.clip_fp64(g, 1.0)
    assert o["norms"] == [5.0, None] and o["total"] == 5.0 and o["applied"] == o["coef"] == 1.0 / (5.0 + 1e-6)
    assert oc.clip_fp64(g, 50.0)["applied"] == 1.0
    nan = oc.clip_fp64([np.array([np.nan, 1.0], np.float32)], 1.0)
    assert np.isnan(nan["coef"]) and nan["applied"] == 1.0
    inf = oc.clip_fp64([np.array([np.inf, 1.0], np.float32)], 1.0)
    assert inf["coef"] == 0.0 and inf["applied"] == 0.0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

def _abi_args(edit=None, **kw):
    """Two tensors of 10 000 and 5 elements behind made-up, aligned addresses: a call the checks let through up to the workspace."""
    rows = [dict(param=1 << 20, grad=2 << 20, exp_avg=3 << 20, exp_avg_sq=4 << 20, numel=10000, step=1, lr=1e-3, weight_decay=5e-4,
                 beta1=0.9, beta2=0.999, eps=1e-8),
            dict(param=5 << 20, grad=6 << 20, exp_avg=7 << 20, exp_avg_sq=8 << 20, numel=5, step=3, lr=1e-3, weight_decay=0.0,
                 beta1=0.9, beta2=0.999, eps=1e-8)]
    for i, edits in (edit or {}).items():
        rows[i].update(edits)
    table = (native.VetoOptimTensor * len(rows))(*[native.VetoOptimTensor(**r) for r in rows])
    base = dict(struct_size=ctypes.sizeof(native.VetoOptimArgs), tensor_size=ctypes.sizeof(native.VetoOptimTensor), n_tensors=len(rows),
                mode=native.VETO_OPTIM_CLIP_STEP, max_norm=5.0, tensors=table, norms=9 << 20, total_norm=10 << 20, coef=11 << 20)
    base.update(kw)
    a = native.VetoOptimArgs(**base)
    a._keep = table
    return a


def test_optim_abi_rejects_bad_arguments_without_a_gpu():
    """Every check comes before the launch (and before the staging buffer is touched)."""
    lib = native.load_library()
    nan = float("nan")
    norms_only, step_only = dict(mode=native.VETO_OPTIM_NORMS), dict(mode=native.VETO_OPTIM_STEP)
    for kw, needle in ((dict(struct_size=8), b"veto_optim_args_t size mismatch"),
                       (dict(tensor_size=80), b"veto_optim_tensor_t size mismatch"),
                       (dict(n_tensors=0), b"n_tensors 0 outside 1..4096"),
                       (dict(n_tensors=4097), b"n_tensors 4097 outside 1..4096"),
                       (dict(mode=4), b"unknown mode 4"),
                       (dict(mode=-1), b"unknown mode -1"),
                       (dict(tensors=None), b"missing pointer: tensors"),
                       (dict(edit={0: dict(numel=-1)}), b"tensor 0: numel -1 outside 0..2^31 - 1"),
                       (dict(edit={1: dict(numel=1 << 31)}), b"tensor 1: numel 2147483648 outside"),
                       (dict(edit={1: dict(step=0)}), b"tensor 1: step 0 must be >= 1"),
                       (dict(edit={0: dict(step=-2)}, **step_only), b"tensor 0: step -2 must be >= 1"),
                       (dict(max_norm=0.0), b"max_norm 0 must be > 0 in a mode that clips"),
                       (dict(max_norm=-1.0, mode=native.VETO_OPTIM_CLIP), b"max_norm -1 must be > 0"),
                       (dict(max_norm=nan), b"must be > 0 in a mode that clips"),
                       (dict(norms=None), b"missing pointer: norms, total_norm and coef"),
                       (dict(coef=None, **norms_only), b"missing pointer: norms, total_norm and coef"),
                       (dict(total_norm=(10 << 20) + 2), b"misaligned norms, total_norm or coef"),
                       (dict(edit={0: dict(grad=(2 << 20) + 1)}), b"tensor 0: misaligned grad"),
                       (dict(edit={0: dict(param=None)}), b"tensor 0: missing pointer: param, exp_avg and exp_avg_sq"),
                       (dict(edit={1: dict(exp_avg_sq=None)}, **step_only), b"tensor 1: missing pointer"),
                       (dict(edit={1: dict(exp_avg=(7 << 20) + 2)}), b"tensor 1: misaligned param, exp_avg or exp_avg_sq"),
                       (dict(edit={0: dict(lr=-1e-3)}), b"tensor 0: lr -0.001 must be >= 0"),
                       (dict(edit={0: dict(lr=nan)}), b"tensor 0: lr nan must be >= 0"),
                       (dict(edit={0: dict(eps=-1.0)}), b"tensor 0: eps -1 must be >= 0"),
                       (dict(edit={0: dict(weight_decay=-1.0)}), b"tensor 0: weight_decay -1 must be >= 0"),
                       (dict(edit={0: dict(beta1=1.0)}), b"tensor 0: beta1 1 outside [0, 1)"),
                       (dict(edit={0: dict(beta2=-0.1)}), b"tensor 0: beta2 -0.1 outside [0, 1)")):
        a = _abi_args(**kw)
        assert lib.veto_optim_step(None, ctypes.byref(a), None, 0) == -1, kw           # VETO_ERR_INVALID
        assert needle in lib.veto_last_error(), (kw, lib.veto_last_error())
    assert lib.veto_optim_step(None, None, None, 0) == -1
    # too many chunks: 4096 tensors of 2^31 - 1 elements
    big = (native.VetoOptimTensor * 4096)(*[native.VetoOptimTensor(grad=4096, numel=(1 << 31) - 1) for _ in range(4096)])
    a = _abi_args(n_tensors=4096, tensors=big, **norms_only)
    assert lib.veto_optim_step(None, ctypes.byref(a), None, 0) == -1 and b"chunks of 8192 elements, the limit is 1048576" in lib.veto_last_error()
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(a)) == 0
    # what the modes do not read is not checked: a tensor without a gradient may hold anything; the norm modes ignore step and state
    for kw in (dict(edit={0: dict(grad=None, step=0, param=None, lr=nan)}), dict(edit={0: dict(step=0, param=None, beta1=7.0)}, **norms_only),
               dict(max_norm=-1.0, **norms_only), dict(max_norm=nan, norms=None, total_norm=None, coef=None, **step_only), dict(edit={1: dict(numel=0, step=0)})):
        a = _abi_args(**kw)
        assert lib.veto_optim_step(None, ctypes.byref(a), None, 0) == -4 and b"workspace too small" in lib.veto_last_error(), (kw, lib.veto_last_error())
    a = _abi_args()
    assert lib.veto_optim_step(None, ctypes.byref(a), ctypes.c_void_p(4100), 1 << 20) == -4 and b"256-byte aligned" in lib.veto_last_error()
    # the workspace: counter | 2 table rows | 3 chunk rows || 3 partials | 2 tensor sums, each part rounded up to 256 bytes
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(a)) == 5 * 256
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(_abi_args(edit={0: dict(numel=64 * solver.CHUNK + 1)}))) == 256 + 256 + 768 + 768 + 256
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(_abi_args(edit={0: dict(grad=None)}))) == 5 * 256
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(_abi_args(n_tensors=0))) == 0
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(_abi_args(struct_size=8))) == 0
    assert lib.veto_optim_step_workspace_bytes(ctypes.byref(_abi_args(edit={0: dict(numel=-1)}))) == 0
    assert lib.veto_optim_step_workspace_bytes(None) == 0


def test_structs_and_chunk_are_the_header_s():
    """The two mirrors are in native.STRUCTS, so test_abi_symbols checks their layout against the header as the C compiler lays it
    out; the chunk size and the modes the binding repeats are the header's."""
    assert native.STRUCTS["veto_optim_tensor_t"] is native.VetoOptimTensor and native.STRUCTS["veto_optim_args_t"] is native.VetoOptimArgs
    assert "veto_optim_step" in native.EXPORTS and "veto_optim_step_workspace_bytes" in native.EXPORTS
    text = open(HEADER).read()
    defines = {k: int(v) for k, v in re.findall(r"#define (VETO_OPTIM_\w+) (\d+)", text)}
    assert defines == {"VETO_OPTIM_CHUNK": solver.CHUNK, "VETO_OPTIM_NORMS": solver.NORMS, "VETO_OPTIM_CLIP": solver.CLIP,
                       "VETO_OPTIM_STEP": solver.STEP, "VETO_OPTIM_CLIP_STEP": solver.CLIP_STEP}
    assert solver.CHUNK % 4 == 0 and ctypes.sizeof(native.VetoOptimTensor) == 88 and ctypes.sizeof(native.VetoOptimArgs) == 56


# ---- the Python layer --------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "load_library", refuse)


def _param(*shape, dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))
    if grad:
        p.grad = torch.ones_like(p)
    return p


def test_adam_checks_its_arguments_before_touching_the_library(no_library):
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(decoupled_weight_decay=True),
               dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            solver.Adam([_param(3)], **kw)
    with pytest.raises(ValueError, match="float32"):
        solver.Adam([_param(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="contiguous"):
        solver.Adam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    opt = solver.Adam([_param(3)])
    with pytest.raises(ValueError, match="float32"):
        opt.add_param_group(dict(params=[_param(2, dtype=torch.float16)]))
    opt = solver.Adam([_param(3)])
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    for call in (opt.step, lambda: opt.clip_and_step(5.0)):
        with pytest.raises(ValueError, match="HIP device"):               # CPU parameters
            call()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            opt.clip_and_step(bad)
    assert not opt.state                                                  # a refused call counts no step and makes no state
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    # gradients
    p = _param(4)
    p.grad_dtype = None            # (torch otherwise refuses the assignment itself)
    p.grad = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        solver.Adam([p]).step()
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(ValueError, match="sparse"):
        solver.Adam([p]).step()


def test_clip_grad_norm_checks_its_arguments_before_touching_the_library(no_library):
    log = oc.Log()
    with pytest.raises(ValueError, match="HIP device"):
        solver.clip_grad_norm([("w", _param(3))], 5.0, log, clip=True)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            solver.clip_grad_norm([("w", _param(3))], bad, log, clip=True)
    p = _param(4)
    p.grad_dtype = None
    p.grad = torch.ones(4, dtype=torch.float16)
    with pytest.raises(ValueError, match="the gradient of w is torch.float16"):
        solver.clip_grad_norm([("w", p)], 5.0, log)
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(ValueError, match="sparse"):
        solver.clip_grad_norm([("w", p)], 5.0, log)
    # no gradient anywhere: the reference returns the number 0.0; a generator is accepted as the reference's loop accepts it
    total = solver.clip_grad_norm(((n, q) for n, q in [("w", _param(3, grad=False))]), 5.0, log, clip=True)
    assert total.shape == () and float(total) == 0.0 and not log.lines
    with pytest.raises(ValueError, match="1..4096"):
        solver.optim_call([], solver.NORMS)
    with pytest.raises(ValueError, match="unknown mode"):
        solver.optim_call([(None, torch.ones(3), None, None, 1, 0, 0, 0, 0, 0)], 7)


def test_a_failed_call_counts_no_step_and_optim_call_checks_its_rows(monkeypatch):
    """The steps are counted only once the library has accepted the call; optim_call, the public entry, refuses a row whose
    tensors are not dense contiguous float32 of one size before the library sees a pointer."""
    monkeypatch.setattr(solver, "_hip_device", lambda device: device)        # (CPU tensors get as far as the call)
    ps = [_param(3), _param(5)]
    opt = solver.Adam(ps)
    opt._state_of(ps[0])["step"].fill_(4.0)

    def refuse(rows, mode, max_norm=0.0, table=None, checked=False):
        assert [r[4] for r in rows] == [5, 1] and checked                     # the rows carry the count including this update
        raise native.VetoError("refused")
    monkeypatch.setattr(solver, "optim_call", refuse)
    for call in (opt.step, lambda: opt.clip_and_step(5.0)):
        with pytest.raises(native.VetoError):
            call()
        assert [float(opt.state[p]["step"]) for p in ps] == [4.0, 0.0] and [p._version for p in ps] == [0, 0]
    monkeypatch.setattr(solver, "optim_call", lambda rows, mode, max_norm=0.0, table=None, checked=False: {})
    opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [5.0, 1.0] and [p._version for p in ps] == [1, 1]
    monkeypatch.undo()
    monkeypatch.setattr(solver, "_hip_device", lambda device: device)

    def refuse_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "load_library", refuse_library)
    ok = torch.zeros(4)
    for bad, needle in ((dict(p=torch.zeros(4, dtype=torch.float64)), "row 0: param is torch.float64"), (dict(m=torch.zeros(8)[::2]), "row 0: exp_avg is not contiguous"),
                        (dict(v=torch.zeros(5)), "row 0: exp_avg_sq has 5 elements"), (dict(m=None), "row 0: exp_avg is missing"),
                        (dict(g=torch.zeros(4, dtype=torch.float16)), "row 0: grad is torch.float16")):
        t = dict(p=ok, g=ok, m=ok, v=ok)
        t.update(bad)
        with pytest.raises(ValueError, match=needle):
            solver.optim_call([(t["p"], t["g"], t["m"], t["v"], 1, 1e-3, 0.0, 0.9, 0.999, 1e-8)], solver.STEP)
    with pytest.raises(ValueError, match="row 1: grad is not contiguous"):
        solver.optim_call([(None, ok, None, None, 1, 0, 0, 0, 0, 0), (None, torch.zeros(8)[::2], None, None, 1, 0, 0, 0, 0, 0)], solver.NORMS)


def test_state_dict_keys_are_torch_adams():
    """Param-group keys, defaults and per-parameter state: what torch.optim.Adam has, so either loads the other's state_dict."""
    def make(cls):
        torch.manual_seed(0)
        ps = [_param(3, 2), _param(5)]
        return cls([dict(params=[ps[0]], lr=0.01, weight_decay=5e-4), dict(params=[ps[1]], lr=0.02, weight_decay=0.0)], lr=0.01), ps
    ours, ps = make(solver.Adam)
    theirs, pt = make(torch.optim.Adam)
    theirs.step()
    for p in ps:
        ours._state_of(p)
    a, b = ours.state_dict(), theirs.state_dict()
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert set(ours.defaults) == set(theirs.defaults)
    assert sorted(a["state"]) == sorted(b["state"]) == [0, 1]
    for i in (0, 1):
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for key in a["state"][i]:
            x, y = a["state"][i][key], b["state"][i][key]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (i, key)
    # both directions load
    ours.load_state_dict(b)
    assert float(ours.state[ps[0]]["step"]) == 1.0 and torch.equal(ours.state[ps[0]]["exp_avg"], theirs.state[pt[0]]["exp_avg"])
    assert ours.param_groups[1]["lr"] == 0.02
    theirs.load_state_dict(ours.state_dict())
    theirs.step()
    assert float(theirs.state[pt[0]]["step"]) == 2.0
    # a state_dict from before torch had the newer keys still loads, and a numeric step becomes torch's host tensor
    old = ours.state_dict()
    for g in old["param_groups"]:
        for key in ("foreach", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            del g[key]
    old["state"][0]["step"] = 4
    ours.load_state_dict(old)
    assert ours.param_groups[0]["maximize"] is False and ours.param_groups[0]["fused"] is None
    st = ours._state_of(ps[0])["step"]
    assert torch.is_tensor(st) and st.dtype == torch.float32 and st.device.type == "cpu" and float(st) == 4.0


def test_installer_swaps_the_three_names_and_restores_them(monkeypatch):
    names = ["pysgg", "pysgg.solver", "pysgg.solver.build", "pysgg.utils", "pysgg.utils.checkpoint", "tools_relation_train_net", "pysgg.engine_other"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
    build, pkg, ckpt, tool, other = (mods[n] for n in ("pysgg.solver.build", "pysgg.solver", "pysgg.utils.checkpoint", "tools_relation_train_net", "pysgg.engine_other"))
    build.make_optimizer = pkg.make_optimizer = tool.make_optimizer = make = object()
    ckpt.clip_grad_norm = tool.clip_grad_norm = clip = object()
    build.make_lr_scheduler = pkg.make_lr_scheduler = sched = object()
    other.make_optimizer = other.clip_grad_norm = mine = object()           # a different object under the same name stays
    patched = registry.install_solver_ops()
    assert patched == [("pysgg.solver.build", "make_optimizer"), ("pysgg.solver", "make_optimizer"), ("tools_relation_train_net", "make_optimizer"),
                       ("pysgg.utils.checkpoint", "clip_grad_norm"), ("tools_relation_train_net", "clip_grad_norm")]
    assert build.make_optimizer is pkg.make_optimizer is tool.make_optimizer is solver.make_optimizer
    assert ckpt.clip_grad_norm is tool.clip_grad_norm is solver.clip_grad_norm
    assert build.make_lr_scheduler is pkg.make_lr_scheduler is sched and other.make_optimizer is other.clip_grad_norm is mine
    assert registry.install_solver_ops() == []                              # already installed
    assert registry.uninstall_solver_ops() == 5
    assert build.make_optimizer is pkg.make_optimizer is tool.make_optimizer is make and ckpt.clip_grad_norm is tool.clip_grad_norm is clip
    assert registry.uninstall_solver_ops() == 0
