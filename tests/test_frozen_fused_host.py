"""CPU side of the frozen-fused training step (include/veto_amd.h, veto_train_plan_t.frozen_fused): the
eligibility decision as a function of module state, the layer k it finds for the plans of tests/partial_train_cases.py, and the flag's
place in the plan struct as the binding and the header see it."""
import ctypes
import os
import re

import pytest

import partial_train_cases as pc
from veto_amd import native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "veto_amd.h")


def _model(layers=3, heads=6, knob=True, precision="mixed", meet=False):
    from veto_amd import testing
    cfg = testing.make_config(layers, heads, meet=meet, precision=precision)
    cfg.VETO_AMD.FROZEN_FUSED = knob
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
    return testing.make_predictor(cfg, pc.state_dict(layers, meet), "cpu").train()


def _trunk(model):
    return model._trunk


def freeze(model, trainable):
    """The reference's fix_eval_modules over everything under the lowest trainable layer: requires_grad_(False) on every parameter that
    is not in `trainable` (engine names), eval() on pos_embed, pos_drop and the frozen layers."""
    k = model._layers
    model.train()
    for prm, name, _, _ in model._train_param_spec():
        prm.requires_grad_(name in trainable)
        m = re.match(re.escape(pc.T) + r"layers\.(\d+)\.", name)
        if m and name in trainable:
            k = min(k, int(m.group(1)))
    tr = _trunk(model).fusion_transformer.transformer
    for m in [_trunk(model).pos_embed, tr.pos_drop] + [tr.layers[l] for l in range(k)]:
        m.eval()
    return k


def test_the_flag_takes_reserved0s_place_in_the_plan_struct():
    fields = [f for f, _ in native.VetoTrainPlan._fields_]
    assert fields == ["struct_size", "bn_eval", "trainable", "p_attn_layer", "d_roi", "frozen_fused"]
    assert ctypes.sizeof(native.VetoTrainPlan) == 32 and native.VetoTrainPlan.frozen_fused.offset == 28 and native.VetoTrainPlan.frozen_fused.size == 4
    assert "veto_debug_last_finalize" in native.EXPORTS and len(native.BUILD_KINDS) == 8
    # the header's struct, read the way tests/test_abi_symbols.py reads it: comments stripped, the field list of the typedef
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct veto_train_plan \{(.*?)\}\s*veto_train_plan_t\s*;", text, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert [re.split(r"[\s*]+", d)[-1] for d in decls] == fields
    assert decls[-1] == "int32_t frozen_fused" and "reserved0" not in body
    kinds = re.search(r"enum veto_build_kind \{(.*?)\}", text, flags=re.S).group(1)
    assert [k.split("=")[0].strip().lower().replace("veto_build_", "") for k in kinds.split(",")][:-1] == list(native.BUILD_KINDS)


def test_the_entry_points_refuse_a_flagged_plan_without_a_handle():
    lib = native.load_library()
    plan = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan), frozen_fused=1, bn_eval=1)
    assert lib.veto_train_workspace_bytes_plan(None, 5, 20, None, ctypes.byref(plan)) == 0
    inp = native.VetoInputs(struct_size=ctypes.sizeof(native.VetoInputs))
    assert lib.veto_forward_train_plan(None, None, ctypes.byref(inp), None, ctypes.byref(plan), None, 0, None) < 0
    counts = (ctypes.c_int32 * 8)()
    assert lib.veto_debug_last_finalize(None, counts, 8) < 0 and b"null argument" in lib.veto_last_error()


@pytest.mark.parametrize("layers", [2, 3, 6])
def test_k_of_every_plan_and_frozen_prefix(layers):
    """k is the lowest layer with a trainable parameter; a plan with a trainable tensor under layer 0 or in layer 0 is ineligible."""
    model = _model(layers)
    prelude = set(pc.weight_names(layers)) - set(pc.HEADS) - set().union(*[pc.layer(l) for l in range(layers)])
    for tag, plan in pc.plans(layers).items():
        freeze(model, plan.trainable)
        ok, reason, k = model.frozen_fused_eligibility(plan.maps)
        in_layers = [int(n[len(pc.T) + 7:].split(".")[0]) for n in plan.trainable if n.startswith(pc.T + "layers.")]
        if plan.maps:
            assert not ok and "ROI map" in reason, (tag, reason)
        elif plan.trainable & prelude:
            assert not ok and "prelude parameter" in reason and any(n in reason for n in plan.trainable & prelude), (tag, reason)
        elif in_layers and min(in_layers) == 0:
            assert not ok and k == 0 and "k = 0" in reason, (tag, reason)
        else:
            assert ok and k == (min(in_layers) if in_layers else layers), (tag, reason, k)
    for k in range(layers + 1):
        assert freeze(model, pc.frozen_prefix(layers, k)) == k
        ok, reason, got = model.frozen_fused_eligibility(False)
        assert got == k and ok == (k >= 1), (k, reason)
    assert model.last_frozen_fused == (False, "no training step has run")      # (the query decides nothing by itself)


def test_eligibility_over_the_module_states():
    """Every state the issue lists, on CPU-constructed modules; the decision is a function of the module's state alone."""
    L = 3
    heads, last = set(pc.HEADS), pc.frozen_prefix(L, L - 1)
    model = _model(L)
    assert freeze(model, heads) == L and model.frozen_fused_eligibility() == (True, "frozen region: the prelude and layers 0..2", 3)
    assert freeze(model, last) == 2 and model.frozen_fused_eligibility() == (True, "frozen region: the prelude and layers 0..1", 2)
    tr = model.fusion_transformer.transformer
    # the last layer's own dropout stays in training mode: it is not in the frozen region
    assert tr.layers[2][0].fn.to_out[1].training and model._attn_rates()[2] > 0
    # a Dropout of the frozen region left in training mode with p > 0
    for what, drop in (("pos_embed[3]", model.pos_embed[3]), ("pos_drop", tr.pos_drop), ("frozen layer 1", tr.layers[1][0].fn.to_out[1])):
        drop.train()
        ok, reason, _ = model.frozen_fused_eligibility()
        assert not ok and what in reason and "p = " in reason, reason
        p, drop.p = drop.p, 0.0      # ... at rate 0 it is the identity: eligible
        assert model.frozen_fused_eligibility()[0]
        drop.p = p
        drop.eval()
    assert model.frozen_fused_eligibility()[0]
    model.pos_embed[0].train()
    ok, reason, _ = model.frozen_fused_eligibility()
    assert not ok and "pos_embed[0]" in reason
    model.pos_embed[0].eval()
    ok, reason, _ = model.frozen_fused_eligibility(want_maps=True)
    assert not ok and "ROI map" in reason
    model.obj_embed.weight.requires_grad_(True)
    ok, reason, _ = model.frozen_fused_eligibility()
    assert not ok and "obj_embed.weight" in reason
    model.obj_embed.weight.requires_grad_(False)
    assert model.frozen_fused_eligibility()[0]
    # the knob and the precision
    off = _model(L, knob=False)
    freeze(off, heads)
    assert off.frozen_fused_eligibility() == (False, "VETO_AMD.FROZEN_FUSED is off", L)
    fast = _model(L, precision="fast")
    freeze(fast, heads)
    ok, reason, _ = fast.frozen_fused_eligibility()
    assert not ok and "fast" in reason
    from veto_amd.config import default_config
    assert default_config().VETO_AMD.FROZEN_FUSED is False


def test_the_3_byte_residual_knob_makes_a_step_ineligible(monkeypatch):
    """The library refuses the flag under VETO_X_F24=1 (the hand-off takes fp32 rows), so the module does not ask for it."""
    model = _model(2, 8)
    freeze(model, set(pc.HEADS))
    assert model.frozen_fused_eligibility()[0]
    monkeypatch.setenv("VETO_X_F24", "1")
    ok, reason, _ = model.frozen_fused_eligibility()
    assert not ok and "VETO_X_F24" in reason


def test_a_meet_head_list_with_one_head_frozen_is_heads_only():
    model = _model(2, 8, meet=True)
    freeze(model, set(pc.HEADS))
    for p in model.model.rel_out[1].parameters():
        p.requires_grad_(False)
    assert model.frozen_fused_eligibility() == (True, "frozen region: the prelude and layers 0..1", 2)


def test_refresh_weights_takes_names():
    model = _model(2, 8)
    model._tensor_versions = {"x": 1}
    model._uploaded = "stamp"
    model.refresh_weights(["rel_out.bias"])
    assert model._uploaded is None and model._forced == {"rel_out.bias"} and model._tensor_versions == {"x": 1}
    model.refresh_weights()
    assert model._tensor_versions == {}
    assert set(model._module_tensors()) == set(pc.weight_names(2)) | set(pc.BUFFERS)
