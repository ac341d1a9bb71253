"""CPU side of the partial training step (include/veto_amd.h, veto_train_plan_t): the ABI additions as the binding sees them, and the
premises of tests/partial_train_cases.py that tests/test_partial_train_gpu.py relies on."""
import ctypes

import pytest
import torch

import partial_train_cases as pc
from veto_amd import native


def test_plan_struct_and_entry_points_are_bound_and_the_opts_keep_their_size():
    assert ctypes.sizeof(native.VetoTrainOpts) == 48      # (tests/test_deterministic_host.py pins it; the plan rides beside it)
    assert native.STRUCTS["veto_train_plan_t"] is native.VetoTrainPlan and ctypes.sizeof(native.VetoTrainPlan) == 32
    for name in ("veto_train_workspace_bytes_plan", "veto_forward_train_plan", "veto_backward_plan"):
        assert name in native.EXPORTS


def test_plan_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = native.load_library()
    plan = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan))
    assert lib.veto_train_workspace_bytes_plan(None, 5, 20, None, ctypes.byref(plan)) == 0
    assert lib.veto_train_workspace_bytes_plan(None, 5, 20, None, None) == 0
    inp = native.VetoInputs(struct_size=ctypes.sizeof(native.VetoInputs))
    for entry, tail in (("veto_forward_train_plan", (None,)), ("veto_backward_plan", (None, None))):
        assert getattr(lib, entry)(None, None, ctypes.byref(inp), None, ctypes.byref(plan), None, 0, *tail) < 0
        assert b"null argument" in lib.veto_last_error()
        assert getattr(lib, entry)(None, None, ctypes.byref(inp), None, None, None, 0, *tail) < 0      # plan == NULL: the entry point without one
        assert b"null argument" in lib.veto_last_error()


def test_shapes_are_what_the_gpu_tests_say_they_are():
    rows = {}
    for tag, shape in pc.SHAPES.items():
        pairs, labels = pc.shape_pairs_labels(shape)
        assert 1 <= len(shape.num_objs) <= 3 and all(2 <= n <= 7 for n in shape.num_objs)
        assert [len(p) for p in pairs] == [len(l) for l in labels]
        for p, n in zip(pairs, shape.num_objs):
            assert p.min() >= 0 and p.max() < n and (p[:, 0] != p[:, 1]).all()
        rows[tag] = 19 * sum(len(p) for p in pairs)
    assert rows == {"l2h8-3img": 931, "l3h6-2img": 798, "l3h6-1img": 380, "l6h6-1img": 380}
    assert rows["l2h8-3img"] % 64 and rows["l2h8-3img"] % 256 and rows["l2h8-3img"] > 3 * 256      # ragged against both tiles, four row tiles
    assert len(pc.shape_pairs_labels(pc.SHAPES["l2h8-3img"])[0][-1]) == 1                           # the single-pair image
    assert {(s.layers, s.heads) for s in pc.SHAPES.values()} == {(2, 8), (3, 6), (6, 6)}


@pytest.mark.parametrize("layers", [2, 3, 6])
def test_plans_name_real_tensors_and_the_stated_launch_counts(layers):
    from veto_amd import testing
    model = testing.make_predictor(testing.make_config(layers, 6), pc.state_dict(layers), "cpu")
    names = {name for _, name, _, _ in model._train_param_spec()}
    assert names == set(pc.weight_names(layers)) and not names & set(pc.BUFFERS)
    plans = pc.plans(layers)
    for tag, plan in plans.items():
        assert plan.trainable <= names, tag
    assert plans["heads"].trainable == set(pc.HEADS) and (plans["heads"].wgrad, plans["heads"].dgrad) == (0, 0)
    assert (plans["last_heads"].wgrad, plans["last_heads"].dgrad) == (4, 3)
    assert (plans["full"].wgrad, plans["full"].dgrad) == (4 * layers, 4 * layers) and plans["full"].trainable == names
    assert not plans["maps_only"].trainable and plans["maps_only"].maps
    assert plans["no_heads"].trainable == names - set(pc.HEADS)
    # LayerNorm1 of the last layer is the one tensor of that layer "last_heads" leaves out: it sits behind the QKV projection
    assert plans["last_all_heads"].trainable - plans["last_heads"].trainable == pc.layer(layers - 1, pc.NORMS[:2])
    assert all(k.endswith("norm.weight") for k in plans["ln_gains"].trainable) and len(plans["ln_gains"].trainable) == 2 * layers
    sizes = [len(pc.frozen_prefix(layers, k)) for k in range(layers + 1)]
    assert sizes == sorted(sizes, reverse=True) and pc.frozen_prefix(layers, layers) == set(pc.HEADS)


@pytest.mark.parametrize("tag", sorted(pc.EVAL_CASES))
def test_eval_mode_references_are_well_conditioned_and_tell_the_settings_apart(tag):
    """(1) No ReLU of the case is decided by rounding: the same reference evaluated in float32 stays within a quarter of the bound.
    (2) For the dropout cases the reference that leaves the eval-mode module's mask ON is another function: at least 20 x the bound
    away, so the device, held to the bound against the right one, must miss the wrong one by 10 x."""
    from test_train_scale_gpu import GRAD_TOL, _errors
    case = pc.EVAL_CASES[tag]
    shape = pc.SHAPES[case.shape]
    p_pos, p_emb, p_attn = pc.eval_case_rates(case)
    right = pc.oracle_step(shape, pc.STEP_SEED, p_pos, p_emb, p_attn, bn_eval=case.bn_eval)
    f32 = pc.oracle_step(shape, pc.STEP_SEED, p_pos, p_emb, p_attn, bn_eval=case.bn_eval, dtype=torch.float32)
    worst = max(max(_errors(f32["grads"][k], v)) for k, v in right["grads"].items())
    assert worst < GRAD_TOL / 4, worst
    if case.bn_eval:
        other = pc.oracle_step(shape, pc.STEP_SEED, p_pos, p_emb, p_attn, bn_eval=False)      # batch statistics instead
    else:
        other = pc.oracle_step(shape, pc.STEP_SEED, *pc.eval_case_rates(case, honour_eval=False))
    apart = max(_errors(other["grads"][k], v)[0] for k, v in right["grads"].items())
    assert apart >= 20 * GRAD_TOL, apart
