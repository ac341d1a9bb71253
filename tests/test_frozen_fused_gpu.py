"""The frozen-fused training step (include/veto_amd.h, veto_train_plan_t.frozen_fused) on the device: the frozen
region of a partial training step -- the prelude and the layers under the lowest one with a trainable tensor -- runs through the fused
inference launches, the rest on the training path.

At the C ABI: a heads-only step (k = L) has veto_forward's logits bit for bit and the head's gradients within the float32 summation bound
of the float64 product of the device's own CLS rows; a frozen prefix (k < L) is held to the float64 reference of
tests/partial_train_cases.py under the project's bounds, with the same plan without the flag printed beside it; chunked handles; the
workspace sizes; every refusal by its message, before any launch.  Through VETOPredictor / VETOPredictor_MEET: the eligibility decision,
the per-tensor upload across optimizer steps and load_state_dict, and that nothing the step leaves behind changes a later full step or eval
forward.  Every C-ABI call goes into sentinel-filled buffers with guard cells and runs twice.  Lines start with "frozen_fused:" (pytest -s).

Measured on one MI355X (profiles/frozen_fused.txt has the table): a frozen prefix, with the flag, is within 4.5e-5 of the reference's
logits (bound 1e-3), 4.5e-6 of its loss (2e-4) and 8.7e-6 on the gradient measure (2e-3); the same plan without the flag 2.3e-5 /
1.7e-6 / 7.3e-6.  The head's gradients use 0.02-0.08 of their summation bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

import partial_train_cases as pc
from test_frozen_fused_host import freeze
from test_partial_train_gpu import GUARD, SENTINEL, Step, _bits, _module_step
from test_train_scale_gpu import GRAD_TOL, _errors

pytestmark = pytest.mark.gpu
U = 2.0 ** -24      # unit roundoff of float32
_STEPS, _ORACLE = {}, {}
TRAIN_ONLY = {"gemm_qkv", "gemm_kv_last", "gemm_out", "gemm_fc1", "gemm_fc2"}      # launch names a mixed handle's inference forward never records


def _dev():
    return torch.device("cuda:0")


def _say(line):
    print("frozen_fused: " + line, flush=True)


class FStep(Step):
    """Step on a handle of a given precision and chunk size, pos_embed.0 on its running statistics (no bn_batch_stats)."""

    def __init__(self, shape, precision="mixed", chunk=0):
        from veto_amd import native, testing
        dev = _dev()
        self.shape, self.native, self.lib = shape, native, native.load_library()
        cfg = testing.make_config(shape.layers, shape.heads, precision=precision, max_chunk_pairs=chunk)
        self.model = testing.make_predictor(cfg, pc.state_dict(shape.layers), dev).train()
        batch = pc.shape_batch(shape)
        pairs, labels = pc.shape_pairs_labels(shape)
        props = testing.make_proposals(batch, "predcls", dev)
        rgb, dep = [torch.from_numpy(batch[k]).to(dev) for k in ("roi_features", "roi_depth_features")]
        obj_labels = torch.cat([p.get_field("labels") for p in props]).long()
        self.call, self.inp, _, _, self.eng = self.model._prepare_inputs(props, [torch.from_numpy(p).to(dev) for p in pairs], rgb, dep, obj_labels, None, None)
        self.names = [n for n, _ in self.eng.weight_specs()]
        self.offsets = self.eng.weight_offsets()
        self.n_obj, self.n_pair, self.n_out = self.inp.n_obj, self.inp.n_pair, self.model._num_out
        g = torch.Generator().manual_seed(3)
        self.dlogits = (torch.randn(self.n_pair, self.n_out, generator=g) / self.n_pair).to(dev)
        self.grad_floats = self.lib.veto_grad_floats(self.eng.handle)
        self.rel_labels = torch.from_numpy(np.concatenate(labels)).long().to(dev)

    def fplan(self, trainable, fused=True, p_layer=None, maps=False, bn_eval=True):
        plan = self.plan(trainable, maps, bn_eval=bn_eval, p_layer=p_layer)
        plan.frozen_fused = int(fused)
        return plan

    def infer(self):
        """veto_forward on the same handle and inputs, twice: (logits, CLS rows, profile)."""
        res = []
        need = self.eng.workspace_bytes(self.n_obj, self.n_pair)
        for _ in range(2):
            ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
            out = torch.full((self.n_pair, self.n_out), float("nan"), device=_dev())
            cls = torch.full((self.n_pair, 576), float("nan"), device=_dev())
            dbg = self.native.VetoDebugOutputs(struct_size=ctypes.sizeof(self.native.VetoDebugOutputs), cls=cls.data_ptr())
            self.eng.profile_enable(True)
            self.eng.profile_reset()
            try:
                self.eng.forward(self.call.stream.cuda_stream, self.inp, ws.data_ptr(), need, out.data_ptr(), dbg)
                torch.cuda.synchronize()
                prof = self.eng.profile()
            finally:
                self.eng.profile_enable(False)
            assert bool((ws[need:] == 0xA5).all())
            res.append((out, cls, prof))
        assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
        return res[0]

    def step(self, plan, rates=(0.0, 0.0, 0.0), ce=False):
        """Forward and backward under `plan` into poisoned buffers, twice (ordered mode: the two runs must agree bit for bit).  ce: the
        backward's dlogits are the cross entropy's over the shape's labels, from the device's own logits (and "loss" is returned)."""
        runs = []
        for _ in range(2):
            opts = self.opts(rates)
            need = self.workspace_bytes(opts, plan)
            assert need > 0, self.lib.veto_last_error()
            ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
            logits = torch.full((self.n_pair, self.n_out), float("nan"), device=_dev())
            grads = torch.full((self.grad_floats,), SENTINEL, device=_dev())
            self.eng.profile_enable(True)
            self.eng.profile_reset()
            try:
                self.native.check(self.forward(opts, plan, ws, need, logits))
                torch.cuda.synchronize()
                fwd = self.eng.profile()
                self.eng.profile_reset()
                loss, keep = None, self.dlogits
                if ce:
                    z = logits.detach().clone().requires_grad_(True)
                    loss = torch.nn.functional.cross_entropy(z, self.rel_labels)
                    loss.backward()
                    self.dlogits = z.grad.contiguous()
                try:
                    self.native.check(self.backward(opts, plan, ws, need, grads))
                finally:
                    self.dlogits = keep
                torch.cuda.synchronize()
                bwd = self.eng.profile()
            finally:
                self.eng.profile_enable(False)
            assert bool((ws[need:] == 0xA5).all()), "the guard behind the workspace was written"
            runs.append(dict(logits=logits, grads=grads, need=need, fwd=fwd, bwd=bwd, loss=None if loss is None else float(loss)))
        assert np.array_equal(_bits(runs[0]["logits"]), _bits(runs[1]["logits"])) and np.array_equal(_bits(runs[0]["grads"]), _bits(runs[1]["grads"])), \
            "two ordered-mode runs differ"
        return runs[0]

    def frozen_untouched(self, grads, trainable):
        for name in self.names:
            if name not in trainable:
                assert bool((self.region(grads, name) == SENTINEL).all()), "frozen %s was written" % name


def _fstep(tag, precision="mixed", chunk=0):
    key = (tag, precision, chunk)
    if key not in _STEPS:
        _STEPS[key] = FStep(pc.SHAPES[tag], precision, chunk)
    return _STEPS[key]


def _launches(prof):
    return {k: v["launches"] for k, v in prof.items()}


def _check_head_gradients(st, got, cls, tag):
    """rel_out.weight / rel_out.bias against the float64 product of the device's own CLS rows and the dlogits given, under the any-order
    float32 summation bound P u / (1 - P u) * sum |term| per element (P pair rows: one product rounding and P - 1 additions)."""
    P = st.n_pair
    gamma = P * U / (1 - P * U)
    d, c = st.dlogits.double().cpu(), cls.double().cpu()
    want_w, bound_w = d.t() @ c, gamma * (d.abs().t() @ c.abs())
    want_b, bound_b = d.sum(0), gamma * d.abs().sum(0)
    gw = st.region(got["grads"], "rel_out.weight").double().cpu().reshape(st.n_out, 576)
    gb = st.region(got["grads"], "rel_out.bias").double().cpu()
    rw, rb = float(((gw - want_w).abs() / bound_w).max()), float(((gb - want_b).abs() / bound_b).max())
    _say("%s heads-only: rel_out.weight error %.3f of its bound, rel_out.bias %.3f of its bound (P = %d)" % (tag, rw, rb, P))
    assert bool(((gw - want_w).abs() <= bound_w).all()), "rel_out.weight: %.3f x the summation bound" % rw
    assert bool(((gb - want_b).abs() <= bound_b).all()), "rel_out.bias: %.3f x the summation bound" % rb
    assert float(gw.abs().max()) > 0 and float(gb.abs().max()) > 0


# ---- heads-only at the C ABI (k = L) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["mixed", "precise"])
@pytest.mark.parametrize("shape_tag", ["l2h8-3img", "l3h6-2img"])
def test_heads_only_step_is_the_inference_forward(shape_tag, precision):
    st = _fstep(shape_tag, precision)
    logits, cls, prof = st.infer()
    got = st.step(st.fplan(set(pc.HEADS)))
    assert np.array_equal(_bits(got["logits"]), _bits(logits)), "the flagged step's logits are not veto_forward's"
    _check_head_gradients(st, got, cls, "%s %s" % (shape_tag, precision))
    st.frozen_untouched(got["grads"], set(pc.HEADS))
    assert "bwd_wgrad" not in got["bwd"] and "bwd_dgrad" not in got["bwd"], got["bwd"].keys()
    # the forward is veto_forward's launches: the same names as often
    assert _launches(got["fwd"]) == _launches(prof), (sorted(got["fwd"]), sorted(prof))
    assert "gemm_qkv0_tab" in got["fwd"] and "gemm_kv_last" not in got["fwd"]
    if precision == "mixed":
        assert "layer_tail_fused" in got["fwd"] and not TRAIN_ONLY & set(got["fwd"]), sorted(got["fwd"])
    # ... against the same plan without the flag: other launches, a larger workspace
    plain = st.step(st.fplan(set(pc.HEADS), fused=False))
    assert "gemm_qkv0_tab" not in plain["fwd"] and "gemm_kv_last" in plain["fwd"] and got["need"] < plain["need"]
    _say("%s %s heads-only: logits bit-equal to veto_forward's (max |flagged - unflagged| %.2e), forward launches %s, workspace %d of %d bytes"
         % (shape_tag, precision, float((got["logits"] - plain["logits"]).abs().max()), sorted(got["fwd"]), got["need"], plain["need"]))


# ---- a frozen prefix at the C ABI (k < L) -------------------------------------------------------------------------------------------------
def _oracle(shape_tag, k):
    """The float64 reference of the step with the layers under k at rate 0 and pos_embed.0 on its running statistics: computed once."""
    key = (shape_tag, k)
    if key not in _ORACLE:
        shape = pc.SHAPES[shape_tag]
        _ORACLE[key] = pc.oracle_step(shape, pc.STEP_SEED, 0.0, 0.0, _rates(shape.layers, k), bn_eval=True)
    return _ORACLE[key]


def _rates(layers, k):
    return [0.0 if l < k else pc.RATES[2] for l in range(layers)]


def _against_oracle(st, run, ref, trainable):
    """{name: (element error, norm error)} on the scaled measure of tests/test_train_scale_gpu.py, the loss and the logit error."""
    res = {name: _errors(st.region(run["grads"], name).cpu(), ref["grads"][name]) for name in sorted(trainable)}
    return res, abs(run["loss"] - ref["loss"]), float((run["logits"].double().cpu() - ref["logits"]).abs().max())


def _check_prefix(st, shape_tag, k, label):
    L = st.shape.layers
    on = pc.frozen_prefix(L, k)
    ref = _oracle(shape_tag, k)
    rates = (0.0, 0.0, pc.RATES[2])
    runs = {}
    for fused in (True, False):
        runs[fused] = st.step(st.fplan(on, fused=fused, p_layer=_rates(L, k)), rates=rates, ce=True)
    (res, dloss, dlogit), (res0, dloss0, dlogit0) = _against_oracle(st, runs[True], ref, on), _against_oracle(st, runs[False], ref, on)
    worst, worst0 = max(res.items(), key=lambda kv: max(kv[1])), max(res0.items(), key=lambda kv: max(kv[1]))
    _say("%s k=%d: flagged   loss error %.2e logit error %.2e worst gradient element %.2e norm %.2e at %s" % (label, k, dloss, dlogit, worst[1][0], worst[1][1], worst[0]))
    _say("%s k=%d: unflagged loss error %.2e logit error %.2e worst gradient element %.2e norm %.2e at %s" % (label, k, dloss0, dlogit0, worst0[1][0], worst0[1][1], worst0[0]))
    got = runs[True]
    st.frozen_untouched(got["grads"], on)
    assert got["need"] < runs[False]["need"]
    assert "gemm_qkv0_tab" in got["fwd"] and "gemm_kv_last" in got["fwd"], sorted(got["fwd"])      # the fused prefix, then the training path's last layer
    if st.model._precision == st.native.VETO_MIXED:      # (a precise handle's frozen middle layers record gemm_qkv as well)
        assert got["fwd"].get("gemm_qkv", {}).get("launches", 0) == L - 1 - k and "layer_tail_fused" in got["fwd"]
    assert _launches(got["bwd"]) == _launches(runs[False]["bwd"])      # the backward is the planned step's
    assert dlogit < 1e-3, dlogit
    assert dloss < 2e-4 * max(1.0, abs(ref["loss"])), (dloss, ref["loss"])
    for name, (e, ne) in res.items():
        assert e < GRAD_TOL and ne < GRAD_TOL, (name, e, ne, "without the flag: %s" % (res0[name],))


@pytest.mark.parametrize("precision", ["mixed", "precise"])
@pytest.mark.parametrize("shape_tag,k", [("l2h8-3img", 1), ("l3h6-2img", 1), ("l3h6-2img", 2)])
def test_frozen_prefix_against_the_float64_reference(shape_tag, k, precision):
    _check_prefix(_fstep(shape_tag, precision), shape_tag, k, "%s %s" % (shape_tag, precision))


# ---- chunks ------------------------------------------------------------------------------------------------------------------------------
def test_chunked_handle_with_a_partial_last_chunk():
    """max_chunk_pairs = 7 on the 20-pair shape: chunks of 7, 7 and 6 pairs."""
    st = _fstep("l3h6-1img", "mixed", 7)
    assert st.n_pair == 20
    logits, cls, _ = st.infer()
    got = st.step(st.fplan(set(pc.HEADS)))
    assert np.array_equal(_bits(got["logits"]), _bits(logits))
    _check_head_gradients(st, got, cls, "l3h6-1img chunk 7")
    st.frozen_untouched(got["grads"], set(pc.HEADS))
    assert got["fwd"]["assemble_tokens"]["launches"] == 3
    _check_prefix(st, "l3h6-1img", 1, "l3h6-1img chunk 7")
    _check_prefix(st, "l3h6-1img", 2, "l3h6-1img chunk 7")


# ---- workspace ---------------------------------------------------------------------------------------------------------------------------
def test_workspace_sizes():
    """With the flag strictly below the same plan without it, non-increasing in k; plan == NULL and flag 0: the sizes recorded before this
    flag existed (profiles/partial_train.txt: L4 / H8, 432 objects, 15 120 pairs, default path)."""
    for tag, precision, chunk in (("l2h8-3img", "mixed", 0), ("l3h6-2img", "mixed", 0), ("l3h6-2img", "precise", 0), ("l3h6-1img", "mixed", 7)):
        st = _fstep(tag, precision, chunk)
        L = st.shape.layers
        for n_obj, n_pair in ((st.n_obj, st.n_pair), (36, 1260)):
            for det in (0, 1):
                opts = st.native.VetoTrainOpts(struct_size=ctypes.sizeof(st.native.VetoTrainOpts), deterministic=det)
                sizes = []
                for k in range(1, L + 1):
                    pair = []
                    for fused in (True, False):
                        plan = st.fplan(pc.frozen_prefix(L, k), fused=fused)
                        pair.append(st.lib.veto_train_workspace_bytes_plan(st.eng.handle, n_obj, n_pair, ctypes.byref(opts), ctypes.byref(plan)))
                    assert 0 < pair[0] < pair[1], (tag, precision, chunk, n_obj, n_pair, det, k, pair)
                    sizes.append(pair[0])
                assert all(a >= b for a, b in zip(sizes, sizes[1:])), sizes
                _say("workspace %s %s chunk %d, %d objects / %d pairs, ordered %d, k = 1..%d: %s" % (tag, precision, chunk, n_obj, n_pair, det, L, " ".join(map(str, sizes))))
    from veto_amd import testing
    model = testing.make_predictor(testing.make_config(4, 8), pc.state_dict(4), _dev()).train()
    eng, lib, native = model._ensure_engine(_dev()), st.lib, st.native
    names = [n for n, _ in eng.weight_specs()]
    flags = (ctypes.c_uint8 * len(names))(*[1 if n in pc.HEADS else 0 for n in names])
    heads = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan), trainable=ctypes.cast(flags, ctypes.c_void_p))
    assert lib.veto_train_workspace_bytes_plan(eng.handle, 432, 15120, None, None) == lib.veto_train_workspace_bytes(eng.handle, 432, 15120) == 29735209472
    assert lib.veto_train_workspace_bytes_plan(eng.handle, 432, 15120, None, ctypes.byref(heads)) == 22283520512
    heads.frozen_fused, heads.bn_eval = 1, 1
    fused = lib.veto_train_workspace_bytes_plan(eng.handle, 432, 15120, None, ctypes.byref(heads))
    assert 0 < fused < 22283520512
    _say("workspace L4 / H8, 432 objects / 15 120 pairs, heads-only: %d bytes with the flag, 22283520512 without" % fused)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _refused(st, plan, message, rates=(0.0, 0.0, 0.0)):
    """The size query returns 0, the forward and the backward refuse, each with `message`, before any launch."""
    opts = st.opts(rates)
    assert st.workspace_bytes(opts, plan) == 0 and message in st.lib.veto_last_error(), (message, st.lib.veto_last_error())
    need = st.workspace_bytes(st.opts(), None)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=_dev())
    logits = torch.full((st.n_pair, st.n_out), SENTINEL, device=_dev())
    grads = torch.full((st.grad_floats,), SENTINEL, device=_dev())
    st.eng.profile_enable(True)
    st.eng.profile_reset()
    try:
        for _ in range(2):
            assert st.forward(opts, plan, ws, need, logits) < 0 and message in st.lib.veto_last_error(), (message, st.lib.veto_last_error())
            assert st.backward(opts, plan, ws, need, grads) < 0 and message in st.lib.veto_last_error(), (message, st.lib.veto_last_error())
        torch.cuda.synchronize()
        assert not st.eng.profile(), "a refused call launched something"
    finally:
        st.eng.profile_enable(False)
    assert bool((logits == SENTINEL).all()) and bool((grads == SENTINEL).all()) and bool((ws == 0xA5).all())


def test_every_refusal_names_its_cause_before_any_launch():
    st = _fstep("l3h6-2img")
    L, heads = 3, set(pc.HEADS)
    _refused(st, st.fplan(heads | {"obj_embed.weight"}), b"'obj_embed.weight' is trainable inside the frozen prelude")
    _refused(st, st.fplan(heads | {pc.T + "cls_token"}), b"cls_token' is trainable inside the frozen prelude")
    _refused(st, st.fplan(pc.frozen_prefix(L, 0)), b"k = 0")
    _refused(st, st.fplan(heads, bn_eval=False), b"bn_eval == 0")
    _refused(st, st.fplan(heads, maps=True), b"d_roi != 0")
    _refused(st, st.fplan(heads), b"p_pos = 0.1", rates=(0.1, 0.0, 0.0))
    _refused(st, st.fplan(heads), b"p_emb = 0.35", rates=(0.0, 0.35, 0.0))
    _refused(st, st.fplan(heads), b"frozen layer 0", rates=(0.0, 0.0, 0.35))      # (no p_attn_layer: opts->p_attn holds for every layer)
    _refused(st, st.fplan(pc.frozen_prefix(L, 2), p_layer=[0.0, 0.35, 0.35]), b"frozen layer 1")
    _refused(_fstep("l3h6-2img", "fast"), _fstep("l3h6-2img", "fast").fplan(heads), b"VETO_FAST")
    os.environ["VETO_X_F24"] = "1"
    try:
        _refused(st, st.fplan(heads), b"VETO_X_F24=1")
    finally:
        del os.environ["VETO_X_F24"]
    # the same plans without the flag are not refused for any of these reasons
    assert st.workspace_bytes(st.opts(), st.fplan(heads | {"obj_embed.weight"}, fused=False)) > 0
    assert st.workspace_bytes(st.opts((0.1, 0.35, 0.35)), st.fplan(heads, fused=False)) > 0


def test_a_backward_under_a_plan_that_differs_only_in_the_flag_is_refused():
    st = _fstep("l2h8-3img")
    on = pc.frozen_prefix(2, 1)
    fused, plain = st.fplan(on, fused=True), st.fplan(on, fused=False)
    opts = st.opts((0.0, 0.0, 0.0))
    need = st.workspace_bytes(opts, plain)
    assert need > st.workspace_bytes(opts, fused) > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=_dev())
    logits = torch.empty((st.n_pair, st.n_out), device=_dev())
    grads = torch.full((st.grad_floats,), SENTINEL, device=_dev())
    for first, other in ((fused, plain), (plain, fused)):
        st.native.check(st.forward(opts, first, ws, need, logits))
        st.eng.profile_enable(True)
        st.eng.profile_reset()
        try:
            assert st.backward(opts, other, ws, need, grads) < 0 and b"another plan" in st.lib.veto_last_error()
            torch.cuda.synchronize()
            assert not st.eng.profile() and bool((grads == SENTINEL).all())
        finally:
            st.eng.profile_enable(False)
        st.native.check(st.backward(opts, first, ws, need, grads))      # the forward's own plan still runs
        torch.cuda.synchronize()
        grads.fill_(SENTINEL)


# ---- through the modules -----------------------------------------------------------------------------------------------------------------
def _model(shape, knob=True, meet=False, precision="mixed", state=None, drop_knob=False):
    from veto_amd import testing
    cfg = testing.make_config(shape.layers, shape.heads, meet=meet, precision=precision)
    cfg.VETO_AMD.DETERMINISTIC = True
    cfg.VETO_AMD.FROZEN_FUSED = knob
    if drop_knob:      # a configuration written before the knob existed
        del cfg.VETO_AMD["FROZEN_FUSED"]
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
    sd = pc.state_dict(shape.layers, meet) if state is None else {k: v.detach().cpu().numpy() for k, v in state.items()}
    model = testing.make_predictor(cfg, sd, _dev())
    model.cfg_used = cfg
    inner = model._run_native_train_grad

    def capture(*a, **kw):      # the training logits of the last step
        out = inner(*a, **kw)
        model.__dict__["last_logits"] = out.detach().clone()
        return out
    model._run_native_train_grad = capture
    return model


def _profiled_step(shape, model, prepare, meet=False):
    """_module_step with the engine's profile on: (grads, profile of the step)."""
    eng = model._ensure_engine(_dev())
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        _, grads, _, losses = _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
        prof = eng.profile()
    finally:
        eng.profile_enable(False)
    return grads, prof, losses


def _eval_logits(shape, model):
    from veto_amd import testing
    batch = pc.shape_batch(shape)
    pairs, _ = pc.shape_pairs_labels(shape)
    props = testing.make_proposals(batch, "predcls", _dev())
    roi = {k: torch.from_numpy(batch[k]).to(_dev()) for k in ("roi_features", "roi_depth_features")}
    model.eval()
    with torch.no_grad():
        out = model(props, [torch.from_numpy(p).to(_dev()) for p in pairs], None, None, **roi)[1]
    torch.cuda.synchronize()
    return torch.cat(list(out.values()) if isinstance(out, dict) else list(out), 0 if not isinstance(out, dict) else 1)


def _heads_only(model):
    freeze(model, set(pc.HEADS))


def _last_and_heads(model):
    freeze(model, pc.frozen_prefix(model._layers, model._layers - 1))


def test_module_decision_and_the_ineligible_states():
    """last_frozen_fused for the two fine-tuning steps, and for each ineligible state, whose step then runs the launches it always ran."""
    shape = pc.SHAPES["l3h6-2img"]
    model = _model(shape)
    _, prof, _ = _profiled_step(shape, model, _heads_only)
    assert model.last_frozen_fused == (True, "frozen region: the prelude and layers 0..2") and "gemm_qkv0_tab" in prof and not TRAIN_ONLY & set(prof), sorted(prof)
    grads, prof, _ = _profiled_step(shape, model, _last_and_heads)
    assert model.last_frozen_fused == (True, "frozen region: the prelude and layers 0..1") and "gemm_qkv0_tab" in prof and "gemm_kv_last" in prof
    assert prof["bwd_wgrad"]["launches"] == 4 and all((g is not None) == (n.startswith("rel_out.") or ".layers.2." in n) for n, g in grads.items() if "obj_embed2" not in n)
    tr = model.fusion_transformer.transformer

    def state(change, word, roi=False):      # (every step starts from model.train() and the heads-only freeze again)
        def prepare(m):
            _heads_only(m)
            change(m)
        eng = model._ensure_engine(_dev())
        eng.profile_enable(True)
        eng.profile_reset()
        try:
            _, grads, _, _ = _module_step(shape, model=model, prepare=prepare, maps=roi)
            prof = eng.profile()
        finally:
            eng.profile_enable(False)
        ok, reason = model.last_frozen_fused
        assert not ok and word in reason, (word, reason)
        assert "gemm_qkv0_tab" not in prof and "gemm_kv_last" in prof and prof["gemm_qkv"]["launches"] == 2, sorted(prof)
        assert grads["rel_out.weight"] is not None and (grads["obj_embed.weight"] is not None) == (word == "obj_embed.weight")
        _say("ineligible (%s): the step ran the training path's launches" % reason)

    state(lambda m: tr.layers[1][0].fn.to_out[1].train(), "frozen layer 1")
    state(lambda m: m.pos_embed[0].train(), "pos_embed[0]")
    state(lambda m: None, "ROI map", roi=True)
    state(lambda m: m.obj_embed.weight.requires_grad_(True), "obj_embed.weight")
    fast = _model(shape, precision="fast")
    # (a fast handle has no training path at all: the decision is made, and the step is refused as it always was)
    with pytest.raises(Exception, match="precise / mixed"):
        _module_step(shape, model=fast, prepare=_heads_only, maps=False)
    assert fast.last_frozen_fused[0] is False and "fast" in fast.last_frozen_fused[1]


@pytest.mark.parametrize("meet", [False, True])
def test_two_steps_with_adam_between_then_everything_else_still_works(meet):
    """Heads-only: the second step's logits are a fresh eval-mode module's on the updated state, bit for bit; the running statistics
    stay; frozen parameters keep .grad None (MEET: one head of the list frozen as well).  Then: load_state_dict of changed frozen
    weights is picked up; an eval forward equals a fresh module's; after unfreezing, an ordered-mode full step equals a fresh module's."""
    import optim_cases as oc
    from veto_amd import solver
    shape = pc.SHAPES["l2h8-3img"]
    model = _model(shape, meet=meet)
    trunk = model._trunk

    def prepare(m):
        _heads_only(m)
        if meet:
            for p in m.model.rel_out[1].parameters():
                p.requires_grad_(False)
    bn = trunk.pos_embed[0]
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    _, g1, _, _ = _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
    assert model.last_frozen_fused[0], model.last_frozen_fused
    first = model.last_logits
    opt = solver.make_optimizer(model.cfg_used, model, oc.Log())
    opt.clip_and_step(5.0)
    torch.cuda.synchronize()
    _, g2, _, _ = _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
    assert model.last_frozen_fused[0]
    second = model.last_logits
    built = model._engine.last_finalize()      # (the second step uploaded the heads alone)
    assert built == dict(dict.fromkeys(built, 0), head_t=1), built
    fresh = _model(shape, meet=meet, state=model.state_dict())
    assert np.array_equal(_bits(second), _bits(_eval_logits(shape, fresh))), "the second step's logits are not a fresh eval-mode module's"
    assert not np.array_equal(_bits(first), _bits(second))
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == before[2]
    for n, g in g2.items():
        trainable = ".rel_out." in "." + n and not (meet and ".rel_out.1." in n)
        assert (g is not None) == trainable, n
    # load_state_dict of changed frozen weights between two steps
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    key = [k for k in sd if k.endswith("layers.0.1.fn.net.0.weight")][0]
    sd[key] = sd[key] * 1.125
    model.load_state_dict(sd)
    _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
    third = model.last_logits
    fresh.load_state_dict(sd)
    want = _eval_logits(shape, fresh)
    assert np.array_equal(_bits(third), _bits(want)) and not np.array_equal(_bits(third), _bits(second))
    # a write through .data is not seen (the documented caveat) until refresh_weights names the tensor
    with torch.no_grad():
        prm = dict(model.named_parameters())[key]
        prm.data.mul_(0.5)
    _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
    assert np.array_equal(_bits(model.last_logits), _bits(third))
    model.refresh_weights([key[len("model."):] if meet else key])
    _module_step(shape, meet=meet, model=model, prepare=prepare, maps=False)
    fresh.load_state_dict(model.state_dict())
    assert np.array_equal(_bits(model.last_logits), _bits(_eval_logits(shape, fresh))) and not np.array_equal(_bits(model.last_logits), _bits(third))
    # an eval forward after the frozen-fused steps
    assert np.array_equal(_bits(_eval_logits(shape, model)), _bits(_eval_logits(shape, fresh)))

    # unfreeze everything, every module back in training mode: an ordered-mode full step equals a fresh module's
    def unfreeze(m):
        for p in m.parameters():
            p.requires_grad_(True)
    other = _model(shape, meet=meet, state=model.state_dict())
    _, ga, ra, la = _module_step(shape, meet=meet, model=model, prepare=unfreeze)
    assert model.last_frozen_fused[0] is False
    _, gb, rb, lb = _module_step(shape, meet=meet, model=other, prepare=unfreeze)
    assert la == lb and np.array_equal(_bits(model.last_logits), _bits(other.last_logits))
    used = 0
    for n, g in gb.items():
        if g is not None:
            assert ga[n] is not None and np.array_equal(_bits(ga[n]), _bits(g)), n
            used += 1
    for k in rb:
        assert np.array_equal(_bits(ra[k]), _bits(rb[k])), k
    _say("%s: two heads-only steps with Adam between, load_state_dict, refresh_weights(names), eval forward, then a full step: %d gradients bit-equal to a fresh module's"
         % ("VETOPredictor_MEET" if meet else "VETOPredictor", used))
    del g1


def test_knob_off_is_the_step_as_it_was():
    """VETO_AMD.FROZEN_FUSED False, and a configuration without the key: the same launch names, logits and gradients, bit for bit."""
    shape = pc.SHAPES["l3h6-2img"]
    res = []
    for drop in (False, True):
        model = _model(shape, knob=False, drop_knob=drop)
        grads, prof, losses = _profiled_step(shape, model, _last_and_heads)
        assert model.last_frozen_fused == (False, "VETO_AMD.FROZEN_FUSED is off")
        assert "gemm_qkv0_tab" not in prof and prof["gemm_qkv"]["launches"] == 2 and prof["bwd_wgrad"]["launches"] == 4, sorted(prof)
        res.append((model.last_logits, grads, _launches(prof), losses))
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3] and np.array_equal(_bits(res[0][0]), _bits(res[1][0]))
    for n, g in res[0][1].items():
        assert (g is None) == (res[1][1][n] is None) and (g is None or np.array_equal(_bits(g), _bits(res[1][1][n]))), n
