"""The partial training step (include/veto_amd.h, veto_train_plan_t) on the device: a step that computes only the gradients somebody
reads and honours eval-mode sub-modules.  Cases and reference: tests/partial_train_cases.py (premises: tests/test_partial_train_host.py).

At the C ABI, in the ordered mode, every plan against the step without a plan on the same inputs and seed: the logits, every trainable
tensor's gradient and the map gradients bit for bit; frozen regions of a sentinel-filled gradient buffer and the guard behind the
(smaller) workspace untouched; the weight- and input-gradient GEMM launch counts through the profiling hooks; the workspace sizes.
Through the modules: eval-mode Dropout / BatchNorm against the float64 reference under the bound of tests/test_train_scale_gpu.py,
requires_grad, the optimizer step on what is left, freezing and unfreezing between steps, a MEET head list with one head frozen.
Each test prints lines starting with "partial_train:" (pytest -s)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import partial_train_cases as pc
from test_train_scale_gpu import GRAD_TOL, _errors

pytestmark = pytest.mark.gpu
SENTINEL = -7.7e7
GUARD = 4096
_STEPS, _FULL = {}, {}


def _dev():
    return torch.device("cuda:0")


def _say(line):
    print("partial_train: " + line, flush=True)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


class Step:
    """One shape's inputs on the device behind a predictor's engine, for calls at the C ABI."""

    def __init__(self, shape, bn_eval=False):
        from veto_amd import native, testing
        dev = _dev()
        self.shape, self.native, self.lib = shape, native, native.load_library()
        cfg = testing.make_config(shape.layers, shape.heads)
        self.model = testing.make_predictor(cfg, pc.state_dict(shape.layers), dev).train()
        batch = pc.shape_batch(shape)
        pairs, _ = pc.shape_pairs_labels(shape)
        props = testing.make_proposals(batch, "predcls", dev)
        rgb, dep = [torch.from_numpy(batch[k]).to(dev) for k in ("roi_features", "roi_depth_features")]
        labels = torch.cat([p.get_field("labels") for p in props]).long()
        self.stats = torch.full((12,), float("nan"), device=dev)
        self.call, self.inp, _, _, self.eng = self.model._prepare_inputs(props, [torch.from_numpy(p).to(dev) for p in pairs], rgb, dep, labels, None,
                                                                         None if bn_eval else self.stats)
        self.names = [n for n, _ in self.eng.weight_specs()]
        self.offsets = self.eng.weight_offsets()
        self.n_obj, self.n_pair, self.n_out = self.inp.n_obj, self.inp.n_pair, self.model._num_out
        g = torch.Generator().manual_seed(3)
        self.dlogits = (torch.randn(self.n_pair, self.n_out, generator=g) / self.n_pair).to(dev)
        self.grad_floats = self.lib.veto_grad_floats(self.eng.handle)

    def opts(self, rates=pc.RATES):
        o = self.native.VetoTrainOpts(struct_size=ctypes.sizeof(self.native.VetoTrainOpts), deterministic=1, seed=pc.STEP_SEED)
        o.p_pos, o.p_emb, o.p_attn = rates
        return o

    def plan(self, trainable, maps, bn_eval=False, p_layer=None):
        flags = (ctypes.c_uint8 * len(self.names))(*[1 if n in trainable else 0 for n in self.names])
        assert sum(flags) == len(trainable)
        rates = (ctypes.c_float * self.shape.layers)(*p_layer) if p_layer is not None else None
        plan = self.native.VetoTrainPlan(struct_size=ctypes.sizeof(self.native.VetoTrainPlan), bn_eval=int(bn_eval), d_roi=int(maps),
                                         trainable=ctypes.cast(flags, ctypes.c_void_p), p_attn_layer=ctypes.cast(rates, ctypes.c_void_p) if rates else None)
        plan._keep = (flags, rates)
        return plan

    def workspace_bytes(self, opts, plan):
        return self.lib.veto_train_workspace_bytes_plan(self.eng.handle, self.n_obj, self.n_pair, ctypes.byref(opts), ctypes.byref(plan) if plan else None)

    def forward(self, opts, plan, ws, need, logits):
        stream, h = ctypes.c_void_p(self.call.stream.cuda_stream), self.eng.handle
        if plan is None:
            return self.lib.veto_forward_train(h, stream, ctypes.byref(self.inp), ctypes.byref(opts), ws.data_ptr(), need, logits.data_ptr())
        return self.lib.veto_forward_train_plan(h, stream, ctypes.byref(self.inp), ctypes.byref(opts), ctypes.byref(plan), ws.data_ptr(), need, logits.data_ptr())

    def backward(self, opts, plan, ws, need, grads):
        stream, h = ctypes.c_void_p(self.call.stream.cuda_stream), self.eng.handle
        if plan is None:
            return self.lib.veto_backward(h, stream, ctypes.byref(self.inp), ctypes.byref(opts), ws.data_ptr(), need, self.dlogits.data_ptr(), grads.data_ptr())
        return self.lib.veto_backward_plan(h, stream, ctypes.byref(self.inp), ctypes.byref(opts), ctypes.byref(plan), ws.data_ptr(), need,
                                           self.dlogits.data_ptr(), grads.data_ptr())

    def run(self, plan=None, maps=True, profile=False, rates=pc.RATES):
        """Forward and backward into poisoned buffers.  Returns a dict: logits, grads (flat), d_rgb, d_dep, need, guard_ok, wgrad, dgrad."""
        dev, check = _dev(), self.native.check
        opts = self.opts(rates)
        need = self.workspace_bytes(opts, plan)
        assert need > 0, self.lib.veto_last_error()
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        logits = torch.full((self.n_pair, self.n_out), float("nan"), device=dev)
        grads = torch.full((self.grad_floats,), SENTINEL, device=dev)
        d_rgb = torch.full((self.n_obj, 256, 8, 8), float("nan"), device=dev) if maps else None
        d_dep = torch.full((self.n_obj, 256, 8, 8), float("nan"), device=dev) if maps else None
        if profile:
            self.eng.profile_enable(True)
            self.eng.profile_reset()
        try:
            check(self.forward(opts, plan, ws, need, logits))
            if maps:
                opts.d_roi_rgb, opts.d_roi_depth = d_rgb.data_ptr(), d_dep.data_ptr()
            check(self.backward(opts, plan, ws, need, grads))
            torch.cuda.synchronize()
            prof = self.eng.profile() if profile else {}
        finally:
            if profile:
                self.eng.profile_enable(False)
        return dict(logits=logits, grads=grads, d_rgb=d_rgb, d_dep=d_dep, need=need, guard_ok=bool((ws[need:] == 0xA5).all()),
                    wgrad=prof.get("bwd_wgrad", {}).get("launches", 0), dgrad=prof.get("bwd_dgrad", {}).get("launches", 0))

    def region(self, flat, name):
        off, numel = self.offsets[name]
        return flat[off:off + numel]


def _step(tag):
    if tag not in _STEPS:
        _STEPS[tag] = Step(pc.SHAPES[tag])
    return _STEPS[tag]


def _full(tag):
    """The step without a plan, ordered mode: computed once per shape and left unchanged."""
    if tag not in _FULL:
        _FULL[tag] = _step(tag).run(None, maps=True, profile=True)
    return _FULL[tag]


PLAN_TAGS = ["heads", "last_heads", "last_all_heads", "fc2_mid", "qkv_mid", "ln_gains", "obj_embed", "no_heads", "maps_only", "full"]


@pytest.mark.parametrize("plan_tag", PLAN_TAGS)
@pytest.mark.parametrize("shape_tag", ["l2h8-3img", "l3h6-2img"])
def test_planned_step_keeps_the_bits_and_touches_nothing_else(shape_tag, plan_tag):
    """Bits, untouched regions, guard cells and launch counts of one plan."""
    st, full = _step(shape_tag), _full(shape_tag)
    case = pc.plans(st.shape.layers)[plan_tag]
    got = st.run(st.plan(case.trainable, case.maps), maps=case.maps, profile=True)
    assert np.array_equal(_bits(got["logits"]), _bits(full["logits"])), "logits"
    assert torch.isfinite(full["logits"]).all()
    for name in st.names:
        mine, ref = st.region(got["grads"], name), st.region(full["grads"], name)
        if name in case.trainable:
            assert np.array_equal(_bits(mine), _bits(ref)), "gradient of %s differs from the step without a plan" % name
            assert torch.isfinite(mine).all() and (name.endswith("to_qkv.weight") or float(mine.abs().max()) > 0), name
        else:
            assert bool((mine == SENTINEL).all()), "frozen %s was written" % name
    if case.maps:
        for k in ("d_rgb", "d_dep"):
            assert np.array_equal(_bits(got[k]), _bits(full[k])), k
            assert float(full[k].abs().max()) > 0
    assert got["guard_ok"] and got["need"] <= full["need"]
    L = st.shape.layers
    assert (full["wgrad"], full["dgrad"]) == (4 * L, 4 * L)
    assert (got["wgrad"], got["dgrad"]) == (case.wgrad, case.dgrad), (got["wgrad"], got["dgrad"], case.wgrad, case.dgrad)
    _say("%s %-14s: %2d trainable tensors bit-equal, %2d frozen regions untouched, bwd_wgrad %d bwd_dgrad %d, workspace %d of %d bytes"
         % (shape_tag, plan_tag, len(case.trainable), len(st.names) - len(case.trainable), got["wgrad"], got["dgrad"], got["need"], full["need"]))


def test_single_image_shape_heads_and_last_layer():
    """The one-image shape (380 token rows: two row tiles, the second partial) under the two plans of the fine-tuning workflows."""
    st = _step("l3h6-1img")
    full = st.run(None, maps=False)
    for tag in ("heads", "last_heads"):
        case = pc.plans(3)[tag]
        got = st.run(st.plan(case.trainable, False), maps=False, profile=True)
        for name in st.names:
            mine = st.region(got["grads"], name)
            if name in case.trainable:
                assert np.array_equal(_bits(mine), _bits(st.region(full["grads"], name))), name
            else:
                assert bool((mine == SENTINEL).all()), name
        assert (got["wgrad"], got["dgrad"]) == (case.wgrad, case.dgrad) and got["guard_ok"]


@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_frozen_prefix_at_six_layers_runs_in_the_smaller_workspace(k):
    """L6: the k frozen layers under the lowest consumer (the last layer keeps its own buffers) alternate between two sets of buffers in
    the forward.  Logits and every trainable gradient keep the bits of the step without a plan, in a workspace strictly smaller, with
    the guard behind it untouched."""
    st = _step("l6h6-1img")
    full = _full("l6h6-1img")
    on = pc.frozen_prefix(6, k)
    got = st.run(st.plan(on, False), maps=False, profile=True)
    assert np.array_equal(_bits(got["logits"]), _bits(full["logits"]))
    for name in st.names:
        mine = st.region(got["grads"], name)
        if name in on:
            assert np.array_equal(_bits(mine), _bits(st.region(full["grads"], name))), name
        else:
            assert bool((mine == SENTINEL).all()), name
    assert got["guard_ok"] and got["need"] < full["need"]
    assert (got["wgrad"], got["dgrad"]) == (4 * (6 - k), 4 * (6 - k))      # (layer k's LayerNorm1 is trainable: its QKV input gradient runs)
    _say("l6h6-1img frozen prefix %d: %d trainable tensors bit-equal in %d of %d workspace bytes" % (k, len(on), got["need"], full["need"]))


def test_workspace_shrinks_with_the_frozen_prefix():
    """Non-increasing in the frozen prefix, strictly below the full size from a prefix of 3 layers at L6; plan == NULL: the _opts size."""
    from veto_amd import native, testing
    dev = _dev()
    lib = native.load_library()
    for layers, heads in ((6, 6), (2, 8), (3, 6)):
        model = testing.make_predictor(testing.make_config(layers, heads), pc.state_dict(layers), dev).train()
        eng = model._ensure_engine(dev)
        names = [n for n, _ in eng.weight_specs()]
        for det in (0, 1):
            opts = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts), deterministic=det)
            base = lib.veto_train_workspace_bytes_opts(eng.handle, 36, 1260, ctypes.byref(opts))
            assert lib.veto_train_workspace_bytes_plan(eng.handle, 36, 1260, ctypes.byref(opts), None) == base > 0
            sizes = []
            for k in range(layers + 1):
                on = pc.frozen_prefix(layers, k)
                flags = (ctypes.c_uint8 * len(names))(*[1 if n in on else 0 for n in names])
                plan = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan), trainable=ctypes.cast(flags, ctypes.c_void_p))
                sizes.append(lib.veto_train_workspace_bytes_plan(eng.handle, 36, 1260, ctypes.byref(opts), ctypes.byref(plan)))
            assert sizes[0] == base and all(a >= b > 0 for a, b in zip(sizes, sizes[1:])), sizes
            if layers == 6:
                assert all(s < base for s in sizes[3:]), sizes
            _say("workspace L%d ordered %d at 36 objects / 1260 pairs, frozen prefix 0..%d: %s" % (layers, det, layers, " ".join(str(s) for s in sizes)))
        bad = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan) - 8, trainable=ctypes.cast(flags, ctypes.c_void_p))
        assert lib.veto_train_workspace_bytes_plan(eng.handle, 36, 1260, None, ctypes.byref(bad)) == 0 and b"size mismatch" in lib.veto_last_error()


def test_a_backward_under_another_plan_is_refused_before_any_launch():
    st = _step("l2h8-3img")
    plans = pc.plans(2)
    heads, last = st.plan(plans["heads"].trainable, False), st.plan(plans["last_heads"].trainable, False)
    opts = st.opts()
    need = st.workspace_bytes(opts, None)      # (the largest: every call below fits)
    ws = torch.zeros(need, dtype=torch.uint8, device=_dev())
    logits = torch.empty((st.n_pair, st.n_out), device=_dev())
    grads = torch.full((st.grad_floats,), SENTINEL, device=_dev())
    st.eng.profile_enable(True)
    try:
        st.native.check(st.forward(opts, heads, ws, need, logits))
        st.eng.profile_reset()
        for other in (last, None):
            assert st.backward(opts, other, ws, need, grads) < 0 and b"another plan" in st.lib.veto_last_error()
        maps = st.opts()
        maps.d_roi_rgb = grads.data_ptr()
        assert st.backward(maps, heads, ws, need, grads) < 0 and b"d_roi == 0" in st.lib.veto_last_error()
        torch.cuda.synchronize()
        assert not st.eng.profile() and bool((grads == SENTINEL).all())
        st.native.check(st.backward(opts, heads, ws, need, grads))      # the forward's own plan still runs
        st.native.check(st.forward(opts, None, ws, need, logits))
        assert st.backward(opts, heads, ws, need, grads) < 0 and b"another plan" in st.lib.veto_last_error()
        st.native.check(st.backward(opts, None, ws, need, grads))
        torch.cuda.synchronize()
    finally:
        st.eng.profile_enable(False)
    # bn_eval with a trainable BatchNorm gain: refused by the size query and by the forward
    bad = st.plan({"pos_embed.0.weight"} | set(pc.HEADS), False, bn_eval=True)
    assert st.workspace_bytes(opts, bad) == 0 and b"bn_eval" in st.lib.veto_last_error()
    assert st.forward(opts, bad, ws, need, logits) < 0 and b"bn_eval" in st.lib.veto_last_error()


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
def _module_step(shape, meet=False, ordered=True, prepare=None, model=None, maps=True):
    """One step through VETOPredictor.forward with the step seed pinned to pc.STEP_SEED.  prepare(model): freezes / eval()s.
    Returns (model, {name: grad or None}, {roi name: grad}, losses)."""
    from veto_amd import testing
    dev = _dev()
    if model is None:
        cfg = testing.make_config(shape.layers, shape.heads, meet=meet)
        cfg.VETO_AMD.DETERMINISTIC = ordered
        cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
        model = testing.make_predictor(cfg, pc.state_dict(shape.layers, meet), dev)
        model.cfg_used = cfg
    model.train()
    if prepare is not None:
        prepare(model)
    for p in model.parameters():
        p.grad = None
    inner = type(model)._train_opts.__get__(model)

    def pinned():
        o = inner()
        o.seed = pc.STEP_SEED
        return o
    model._train_opts = pinned
    batch = pc.shape_batch(shape)
    pairs, labels = pc.shape_pairs_labels(shape)
    props = testing.make_proposals(batch, "predcls", dev)
    roi = {k: torch.from_numpy(batch[k]).to(dev).requires_grad_(maps) for k in ("roi_features", "roi_depth_features")}
    random.seed(1)
    try:
        out = model(props, [torch.from_numpy(p).to(dev) for p in pairs], [torch.from_numpy(l).to(dev) for l in labels], None, **roi)
        losses = {k: v for k, v in out[2].items() if v.requires_grad}
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        del model._train_opts
    grads = {n: p.grad for n, p in model.named_parameters(remove_duplicate=False)}
    return model, grads, {k: v.grad for k, v in roi.items()}, {k: float(v.detach()) for k, v in losses.items()}


def _eval_modules(model, case):
    tr = model.fusion_transformer.transformer
    for l in case.attn_eval:
        tr.layers[l][0].fn.to_out[1].eval()
    if case.pos_drop_eval:
        tr.pos_drop.eval()
    if case.bn_eval:      # the reference's fix_eval_modules: eval() and requires_grad = False on the module's own parameters
        model.pos_embed[0].eval()
        for p in model.pos_embed[0].parameters():
            p.requires_grad_(False)


def _against_oracle(grads, roi, ref, skip=()):
    res = {}
    for name, want in ref["grads"].items():
        if name in skip:
            continue
        assert grads[name] is not None, name
        res[name] = _errors(grads[name].detach().cpu(), want)
    for k in roi:
        res["d_" + k] = _errors(roi[k].detach().cpu(), ref["d_" + k])
    return res


@pytest.mark.parametrize("tag", sorted(pc.EVAL_CASES))
def test_eval_mode_modules_against_the_float64_reference(tag):
    """A Dropout / BatchNorm in eval() inside a training step: every gradient within GRAD_TOL of the float64 reference that runs the
    site at rate 0 (running statistics), and the running statistics untouched under bn_eval."""
    case = pc.EVAL_CASES[tag]
    shape = pc.SHAPES[case.shape]
    before = {}

    def prepare(model):
        _eval_modules(model, case)
        bn = model.pos_embed[0]
        before.update(mean=bn.running_mean.clone(), var=bn.running_var.clone(), n=int(bn.num_batches_tracked))
    model, grads, roi, losses = _module_step(shape, ordered=False, prepare=prepare)
    p_pos, p_emb, p_attn = pc.eval_case_rates(case)
    ref = pc.oracle_step(shape, pc.STEP_SEED, p_pos, p_emb, p_attn, bn_eval=case.bn_eval)
    frozen = ("pos_embed.0.weight", "pos_embed.0.bias") if case.bn_eval else ()
    res = _against_oracle(grads, roi, ref, skip=frozen)
    worst = max(res.items(), key=lambda kv: max(kv[1]))
    _say("eval-mode %-13s: loss %.6f (reference %.6f), worst element %.2e norm %.2e at %s" % (tag, losses["rel_loss"], ref["loss"], worst[1][0], worst[1][1], worst[0]))
    assert abs(losses["rel_loss"] - ref["loss"]) < 2e-4 * max(1.0, abs(ref["loss"]))
    for name, (e, ne) in res.items():
        assert e < GRAD_TOL and ne < GRAD_TOL, (name, e, ne)
    bn = model.pos_embed[0]
    if case.bn_eval:
        assert all(grads[n] is None for n in frozen) and grads["pos_embed.1.weight"] is not None
        assert torch.equal(bn.running_mean, before["mean"]) and torch.equal(bn.running_var, before["var"]) and int(bn.num_batches_tracked) == before["n"]
    else:
        assert int(bn.num_batches_tracked) == before["n"] + 1 and not torch.equal(bn.running_mean, before["mean"])
        # the comparison notices a mask left on: the reference that ignores eval() misses by at least 10 x the bound
        wrong = pc.oracle_step(shape, pc.STEP_SEED, *pc.eval_case_rates(case, honour_eval=False))
        miss = max(v[0] for v in _against_oracle(grads, roi, wrong).values())
        _say("eval-mode %-13s: against the reference that keeps the frozen site's mask on, worst element %.2e (%.0f x GRAD_TOL)" % (tag, miss, miss / GRAD_TOL))
        assert miss >= 10 * GRAD_TOL


def _freeze_all_but_heads(model):
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("rel_out."))


def _same(a, b, what):
    assert a is not None and b is not None, what
    assert np.array_equal(_bits(a), _bits(b)), what


def test_requires_grad_freezing_unfreezing_and_the_optimizer_step():
    """Frozen parameters keep .grad None; unfreezing gives the full step's bits again (ordered mode); Adam's clip_and_step runs on
    what is left and leaves the frozen parameters alone."""
    import optim_cases as oc
    from veto_amd import solver
    shape = pc.SHAPES["l2h8-3img"]
    _, full, full_roi, _ = _module_step(shape)
    model, g1, roi1, _ = _module_step(shape, prepare=_freeze_all_but_heads, maps=False)
    assert sorted(n for n, g in g1.items() if g is not None) == ["rel_out.bias", "rel_out.weight"]
    for n in ("rel_out.weight", "rel_out.bias"):
        _same(g1[n], full[n], n)
    assert all(v is None for v in roi1.values())
    state = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = solver.make_optimizer(model.cfg_used, model, oc.Log())
    opt.clip_and_step(5.0)
    torch.cuda.synchronize()
    moved = sorted(n for n, p in model.named_parameters() if not torch.equal(p.detach(), state[n]))
    assert moved == ["rel_out.bias", "rel_out.weight"], moved
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(state[n])

    def unfreeze(m):
        for p in m.parameters():
            p.requires_grad_(True)
    _, g2, roi2, _ = _module_step(shape, prepare=unfreeze, model=model)
    used = [n for n, g in full.items() if g is not None]
    assert sorted(used) == sorted(pc.weight_names(shape.layers))
    for n in used:
        _same(g2[n], full[n], n)
    for k in full_roi:
        _same(roi2[k], full_roi[k], k)

    def last_layer(m):
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith("rel_out.") or ".layers.1." in n)
    _, g3, _, _ = _module_step(shape, prepare=last_layer, model=model, maps=False)
    for n in used:
        if n.startswith("rel_out.") or ".layers.1." in n:
            _same(g3[n], full[n], n)
        else:
            assert g3[n] is None, n
    _say("module level: heads-only, unfrozen and last-layer steps on one module: every computed gradient bit-equal to the full step's")


def test_meet_head_list_with_one_group_frozen():
    """The heads are rows of one rel_out: a frozen head of the list gets None, the others and the trunk the full step's bits."""
    shape = pc.SHAPES["l2h8-3img"]
    _, full, _, _ = _module_step(shape, meet=True)

    def freeze_group_1(model):
        for p in model.model.rel_out[1].parameters():
            p.requires_grad_(False)
    _, got, _, _ = _module_step(shape, meet=True, prepare=freeze_group_1)
    frozen = [n for n in full if ".rel_out.1." in n]
    assert len(frozen) == 2
    for n, g in full.items():
        if n in frozen:
            assert got[n] is None, n
        elif g is not None:
            _same(got[n], g, n)
    assert sum(g is not None for g in got.values()) == sum(g is not None for g in full.values()) - 2
