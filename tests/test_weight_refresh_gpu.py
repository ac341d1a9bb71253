"""The per-tensor weight refresh of the handle (include/veto_amd.h, veto_load_weights): after one tensor is
uploaded again, a forward rebuilds the derived operands that read it and no others, and every operand has the bytes a rebuild of
everything gives it -- so the logits, and an ordered-mode training step's logits and gradients, are those of a fresh handle loaded
with the same final weights, bit for bit.  One tensor of every class of the dependency table, and three that are read in place, on
mixed and precise handles; the rebuild counts through veto_debug_last_finalize.
Every call goes into sentinel-filled buffers with guard cells and runs twice.  Lines start with "weight_refresh:" (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import partial_train_cases as pc
from test_partial_train_gpu import GUARD, SENTINEL, Step, _bits

pytestmark = pytest.mark.gpu
SHAPE = "l3h6-2img"      # three layers: a middle layer that is neither layer 0 (the table form) nor the last (the fold)
T = pc.T
TENSORS = {      # case -> state-dict name, by class of the dependency table
    "mid-linear": T + "layers.1.1.fn.net.0.weight",
    "l0-ln1-gain": T + "layers.0.0.norm.weight",
    "l0-qkv": T + "layers.0.0.fn.to_qkv.weight",
    "pos-embedding": T + "pos_embedding",
    "cls-token": T + "cls_token",
    "last-qkv": T + "layers.2.0.fn.to_qkv.weight",
    "last-out": T + "layers.2.0.fn.to_out.0.weight",
    "patch-proj-d": T + "patch_embed.proj_d.weight",
    "loc-proj": "location_projection.0.weight",
    "cls-proj": "class_projection.0.weight",
    "head": "rel_out.weight",
    # read in place: no derived operand
    "head-bias": "rel_out.bias",
    "ln2-gain": T + "layers.1.1.norm.weight",
    "obj-embed": "obj_embed.weight",
}
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _say(line):
    print("weight_refresh: " + line, flush=True)


def _step():
    """The shape's inputs (a veto_inputs_t on the device); its own engine is not used here."""
    if "step" not in _CACHE:
        _CACHE["step"] = Step(pc.SHAPES[SHAPE])
    return _CACHE["step"]


def _weights():
    if "weights" not in _CACHE:
        st = _step()
        sd = pc.state_dict(st.shape.layers)
        _CACHE["weights"] = {n: torch.from_numpy(np.asarray(sd[n], dtype=np.float32)).to(_dev()).contiguous() for n in st.names}
    return _CACHE["weights"]


def _changed(name):
    """Another tensor of the same size and scale, a function of the name alone."""
    w = _weights()[name]
    g = torch.Generator().manual_seed(sum(name.encode()))
    return (w * 1.0625 + 0.03 * float(w.abs().mean() + 1e-3) * torch.randn(w.shape, generator=g).to(w.device)).contiguous()


def _load(eng, name, tensor):
    eng.load_weight(name, tensor.data_ptr(), tensor.numel(), torch.cuda.current_stream().cuda_stream)


def _engine(precision, weights):
    from veto_amd import native
    shape = pc.SHAPES[SHAPE]
    eng = native.Engine(shape.layers, shape.heads, 151, 51, precision={"mixed": native.VETO_MIXED, "precise": native.VETO_PRECISE}[precision], device=0)
    for name, _ in eng.weight_specs():
        _load(eng, name, weights[name])
    return eng


def _forward(eng):
    """veto_forward twice into poisoned buffers: the logits (equal both times), the guard behind the workspace intact."""
    st, outs = _step(), []
    need = eng.workspace_bytes(st.n_obj, st.n_pair)
    for _ in range(2):
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
        out = torch.full((st.n_pair, st.n_out), float("nan"), device=_dev())
        eng.forward(torch.cuda.current_stream().cuda_stream, st.inp, ws.data_ptr(), need, out.data_ptr())
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()) and bool(torch.isfinite(out).all())
        outs.append(out)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    return outs[0]


def _train_step(eng):
    """An unplanned ordered-mode step (veto_forward_train + veto_backward), twice: (logits, flat gradients)."""
    st, lib, res = _step(), _step().lib, []
    opts = st.opts()
    need = lib.veto_train_workspace_bytes_opts(eng.handle, st.n_obj, st.n_pair, ctypes.byref(opts))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
        out = torch.full((st.n_pair, st.n_out), float("nan"), device=_dev())
        grads = torch.full((st.grad_floats,), SENTINEL, device=_dev())
        st.native.check(lib.veto_forward_train(eng.handle, stream, ctypes.byref(st.inp), ctypes.byref(opts), ws.data_ptr(), need, out.data_ptr()))
        st.native.check(lib.veto_backward(eng.handle, stream, ctypes.byref(st.inp), ctypes.byref(opts), ws.data_ptr(), need, st.dlogits.data_ptr(),
                                          grads.data_ptr()))
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all())
        res.append((out, grads))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
    return res[0]


def _warm(precision):
    """One long-lived handle per precision that has run a forward on the original weights: every operand is built."""
    key = ("warm", precision)
    if key not in _CACHE:
        _CACHE[key] = _engine(precision, _weights())
        _CACHE[key, "logits"] = _forward(_CACHE[key])
    return _CACHE[key]


@pytest.mark.parametrize("case", sorted(TENSORS))
@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_single_tensor_reload_gives_the_logits_of_a_fresh_handle(precision, case):
    name = TENSORS[case]
    eng, new = _warm(precision), _changed(name)
    _load(eng, name, new)
    try:
        got = _forward(eng)
        fresh =_engine(precision, dict(_weights(), **{name: new}))
        want = _forward(fresh)
        fresh.close()
        assert np.array_equal(_bits(got), _bits(want)), "logits after reloading %s differ from a fresh handle's" % name
        assert not np.array_equal(_bits(got), _bits(_CACHE[("warm", precision), "logits"])), "%s did not reach the logits" % name
        _say("%-8s %-13s: logits bit-equal to a fresh handle's, max |change| %.3e" % (precision, case, float((got - _CACHE[("warm", precision), "logits"]).abs().max())))
    finally:
        _load(eng, name, _weights()[name])
    assert np.array_equal(_bits(_forward(eng)), _bits(_CACHE[("warm", precision), "logits"])), "restoring %s" % name


@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_rebuild_counts(precision):
    """A head weight rebuilds the head transpose and nothing else, a bias nothing, a first upload everything."""
    from veto_amd import native
    L = pc.SHAPES[SHAPE].layers
    mixed = precision == "mixed"
    none = dict.fromkeys(native.BUILD_KINDS, 0)
    fresh = _engine(precision, _weights())
    _forward(fresh)
    # (_forward runs twice; the second forward found nothing to do and did not touch the counts)
    everything = dict(none, split_rows=4 * L, mixed_rows=4 * L if mixed else 0, patch=1, loc_t=1, cls_t=1, head_t=1, qkv0=1, fold=1)
    assert fresh.last_finalize() == everything, fresh.last_finalize()
    cases = {"rel_out.weight": dict(none, head_t=1), "rel_out.bias": none, T + "layers.1.1.norm.weight": none, "obj_embed.weight": none,
             T + "layers.1.1.fn.net.0.weight": dict(none, split_rows=1, mixed_rows=int(mixed)),
             T + "layers.0.0.norm.weight": dict(none, qkv0=1), T + "cls_token": dict(none, qkv0=1),
             T + "layers.0.0.fn.to_qkv.weight": dict(none, split_rows=1, mixed_rows=int(mixed), qkv0=1),
             T + "layers.2.0.fn.to_out.0.weight": dict(none, split_rows=1, mixed_rows=int(mixed), fold=1),
             T + "patch_embed.proj_v.bias": dict(none, patch=1), "location_projection.0.weight": dict(none, loc_t=1),
             "class_projection.0.weight": dict(none, cls_t=1)}
    for name, want in cases.items():
        _load(fresh, name, _changed(name))
        _forward(fresh)
        assert fresh.last_finalize() == want, (name, fresh.last_finalize())
    # a training forward builds the training side only; the inference forward behind it completes the rest
    st, lib = _step(), _step().lib
    name = T + "layers.1.0.fn.to_qkv.weight"
    _load(fresh, name, _changed(name))
    _train_step(fresh)
    assert fresh.last_finalize() == dict(none, split_rows=1), fresh.last_finalize()
    _forward(fresh)      # (a precise handle has no mixed rows: nothing is missing, the counts stay the training forward's)
    assert fresh.last_finalize() == (dict(none, mixed_rows=1) if mixed else dict(none, split_rows=1)), fresh.last_finalize()
    counts = (ctypes.c_int32 * 4)()
    assert lib.veto_debug_last_finalize(fresh.handle, counts, 4) < 0 and b"VETO_BUILD_KINDS" in lib.veto_last_error()
    fresh.close()
    _say("%s: first upload rebuilds %s; %d single-tensor cases rebuild exactly their operands" % (precision, everything, len(cases)))
    del st


@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_training_side_operands_after_a_reload(precision):
    """An unplanned ordered-mode step after a single-tensor change gives a fresh handle's logits and gradients bit for bit; and changing
    A, running a forward, changing B and running a forward equals changing both at once."""
    a, b = T + "layers.1.0.fn.to_out.0.weight", T + "patch_embed.proj_d.weight"
    eng = _engine(precision, _weights())
    _train_step(eng)
    _load(eng, a, _changed(a))
    got = _train_step(eng)
    fresh = _engine(precision, dict(_weights(), **{a: _changed(a)}))
    want = _train_step(fresh)
    fresh.close()
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "training logits"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "gradients"
    assert bool((got[1] != SENTINEL).any()) and bool(torch.isfinite(got[1][got[1] != SENTINEL]).all())
    # A, forward, B, forward == both at once (inference and training side)
    infer_a = _forward(eng)
    _load(eng, b, _changed(b))
    infer_ab, train_ab = _forward(eng), _train_step(eng)
    both = _engine(precision, dict(_weights(), **{a: _changed(a), b: _changed(b)}))
    want_infer, want_train = _forward(both), _train_step(both)
    both.close()
    eng.close()
    assert np.array_equal(_bits(infer_ab), _bits(want_infer)) and not np.array_equal(_bits(infer_ab), _bits(infer_a))
    assert np.array_equal(_bits(train_ab[0]), _bits(want_train[0])) and np.array_equal(_bits(train_ab[1]), _bits(want_train[1]))
    _say("%s: ordered-mode step after reloading %s bit-equal to a fresh handle's; A then B equals both at once" % (precision, a.split("layers.")[-1]))
