"""veto_meet_sample_parallel (all three GCL_SETTING.ZERO_LABEL_PADDING_MODEs) on the device, bit for bit against the restatements of
tests/meet_sample_cases.py and, in rand_insert, against the serial veto_meet_sample; then MeetTrainingSampler, the predictor's
fifth return value and one training step per new mode against oracle/train_oracle.py.  Every ABI call is made twice."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import meet_sample_cases as mc
from conftest import GOLDEN_DIR
from veto_amd import native

pytestmark = pytest.mark.gpu

SENT, GUARD = -7, 256
CASES = {c["name"]: c for c in mc.crafted_cases()}
_EXPECTED = {}


def _expected(case):
    """(chosen lists, words_used) of the word restatement, once per case."""
    if case["name"] not in _EXPECTED:
        chosen, used, _ = mc.sample_words(case["labels"], case["incre"], case["rates"], case["G"], case["mode"], case["words"])
        _EXPECTED[case["name"]] = ([np.array(c, dtype=np.int64) for c in chosen], used)
    return _EXPECTED[case["name"]]


def _device_inputs(case, n_words):
    dev = torch.device("cuda:0")
    pos, size = mc.tables_of(case["incre"])
    i32 = dict(dtype=torch.int32, device=dev)
    return dict(labels=torch.from_numpy(case["labels"]).to(dev), words=torch.from_numpy(case["words"][:n_words].view(np.int32).copy()).to(dev),
                incre=torch.tensor(case["incre"], **i32), pos=torch.tensor(pos, **i32), size=torch.tensor(size, **i32),
                rates=torch.from_numpy(case["rates"]).to(dev))


def _outputs(G, n):
    dev = torch.device("cuda:0")
    return (torch.full((G, n), SENT, dtype=torch.int64, device=dev), torch.full((G, n), SENT, dtype=torch.int64, device=dev),
            torch.full((G + 1,), SENT, dtype=torch.int32, device=dev))


def run_parallel(case, n_words=None, mode=None):
    """One call of the new entry: (chosen, group_labels, counts + words_used) as numpy, sentinel-filled before the call; the bytes
    behind the workspace's stated size are checked."""
    n, G = len(case["labels"]), case["G"]
    n_words = len(case["words"]) if n_words is None else n_words
    t = _device_inputs(case, n_words)
    chosen, glabels, meta = _outputs(G, n)
    call = native.Launch(chosen.device, "test")
    need = call.lib.veto_meet_sample_parallel_workspace_bytes(n, n_words)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=chosen.device)
    a = call.args(native.VetoMeetSampleArgs, mode=native.MEET_PAD_MODES[mode or case["mode"]], n=n, n_words=n_words, n_groups=G,
                  n_cls=case["n_cls"], labels=t["labels"], words=t["words"], incre_idx_list=t["incre"], pos_in_group=t["pos"],
                  group_size=t["size"], sample_rates=t["rates"], chosen=chosen, group_labels=glabels, counts=meta, words_used=meta[G:])
    call.run("veto_meet_sample_parallel", ctypes.byref(a), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    return chosen.cpu().numpy(), glabels.cpu().numpy(), meta.cpu().numpy()


def run_serial(case, n_words=None):
    n, G = len(case["labels"]), case["G"]
    n_words = len(case["words"]) if n_words is None else n_words
    t = _device_inputs(case, n_words)
    chosen, glabels, meta = _outputs(G, n)
    call = native.Launch(chosen.device, "test")
    call.run("veto_meet_sample", call.ptr(t["labels"]), n, call.ptr(t["words"]), n_words, t["incre"].data_ptr(), t["pos"].data_ptr(),
             t["size"].data_ptr(), t["rates"].data_ptr(), G, case["n_cls"], chosen.data_ptr(), glabels.data_ptr(), meta.data_ptr(),
             meta[G:].data_ptr())
    torch.cuda.synchronize()
    return chosen.cpu().numpy(), glabels.cpu().numpy(), meta.cpu().numpy()


def check_against_restatement(case, got):
    chosen, glabels, meta = got
    want, used = _expected(case)
    G = case["G"]
    assert int(meta[G]) == used == len(case["words"]), (int(meta[G]), used)
    assert meta[:G].tolist() == [len(w) for w in want]
    for k in range(G):
        c = len(want[k])
        assert np.array_equal(chosen[k, :c], want[k]), k
        assert np.array_equal(glabels[k, :c], mc.group_labels(case["labels"], want[k], case["incre"], k)), k
        assert bool((chosen[k, c:] == SENT).all()) and bool((glabels[k, c:] == SENT).all()), k      # nothing behind counts[k]


def test_library_sizes_are_the_ones_the_cases_are_built_for():
    v = [ctypes.c_int32() for _ in range(3)]
    lib = native.load_library()
    assert lib.veto_meet_sample_parallel_limits(*[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == mc.LIMITS
    assert lib.veto_meet_sample_parallel_limits(None, None, None) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_parallel_sampler_matches_the_restatement_bit_for_bit(name):
    case = CASES[name]
    first, again = run_parallel(case), run_parallel(case)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    check_against_restatement(case, first)
    if case["mode"] == "rand_insert":           # the serial entry is the on-device control
        for a, b in zip(first, run_serial(case)):
            assert np.array_equal(a, b)
    # one word short: -1 (rand_insert: for a case that ends with a background relation, inside its run of attempts)
    exact = len(case["words"])
    if exact > 0:
        for _ in range(2):
            assert int(run_parallel(case, exact - 1)[2][case["G"]]) == -1
        if case["mode"] == "rand_insert" and exact > 1:
            assert int(run_serial(case, exact - 1)[2][case["G"]]) == -1
    # a longer block changes nothing but n_words
    longer = dict(case, words=np.concatenate([case["words"], np.full(3, mc.ALL_ONES, dtype=np.uint32)]))
    got = run_parallel(longer)
    assert int(got[2][case["G"]]) == exact
    for a, b in zip(first[:2], got[:2]):
        assert np.array_equal(a, b)


def test_refusals_launch_nothing():
    lib = native.load_library()
    case = CASES["foreground_edges_rand_choose"]
    n, G = len(case["labels"]), case["G"]
    t = _device_inputs(case, len(case["words"]))
    chosen, glabels, meta = _outputs(G, n)
    need = lib.veto_meet_sample_parallel_workspace_bytes(n, len(case["words"]))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=chosen.device)

    def rc(ws_ptr=None, ws_bytes=None, **kw):
        f = dict(struct_size=ctypes.sizeof(native.VetoMeetSampleArgs), mode=1, n=n, n_words=len(case["words"]), n_groups=G, n_cls=case["n_cls"],
                 labels=t["labels"].data_ptr(), words=t["words"].data_ptr(), incre_idx_list=t["incre"].data_ptr(),
                 pos_in_group=t["pos"].data_ptr(), group_size=t["size"].data_ptr(), sample_rates=t["rates"].data_ptr(),
                 chosen=chosen.data_ptr(), group_labels=glabels.data_ptr(), counts=meta.data_ptr(), words_used=meta[G:].data_ptr())
        f.update(kw)
        a = native.VetoMeetSampleArgs(**f)
        return lib.veto_meet_sample_parallel(None, ctypes.byref(a), ws.data_ptr() if ws_ptr is None else ws_ptr, need if ws_bytes is None else ws_bytes)

    for kw, needle in ((dict(struct_size=8), b"size mismatch"), (dict(mode=3), b"mode"), (dict(n=0), b"bad sizes"), (dict(n_groups=65), b"bad sizes"),
                       (dict(n_words=-1), b"bad sizes"), (dict(words=None), b"missing pointer"), (dict(counts=None), b"missing pointer")):
        assert rc(**kw) < 0, kw
        assert needle in lib.veto_last_error(), (kw, lib.veto_last_error())
    assert rc(ws_bytes=need - 1) < 0 and b"workspace too small" in lib.veto_last_error()
    assert rc(ws_ptr=ws.data_ptr() + 8) < 0 and b"aligned" in lib.veto_last_error()
    assert lib.veto_meet_sample_parallel_workspace_bytes(0, 4) == 0 and lib.veto_meet_sample_parallel_workspace_bytes(4, -1) == 0
    torch.cuda.synchronize()
    assert bool((chosen == SENT).all()) and bool((meta == SENT).all())


# ---- MeetTrainingSampler and the predictor ---------------------------------------------------------------------------
def _golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


@pytest.mark.parametrize("seed", [1, 2, 12345])
@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("dataset", ["VG", "GQA"])
def test_sampler_stays_in_lock_step_with_pythons_generator(dataset, mode, seed):
    from veto_amd import meet_tables
    from veto_amd.losses import MeetTrainingSampler
    dev = torch.device("cuda:0")
    incre, rates = mc.dataset_tables(dataset)
    sizes = mc.tables_of(incre)[1]
    rng = np.random.RandomState(seed)
    labels = np.where(rng.random_sample(1500) < 0.25, rng.randint(1, len(incre), size=1500), 0)
    random.seed(seed)
    want = mc.sample_stdlib(labels, incre, meet_tables.sample_rate_matrix(dataset, sizes), len(sizes), mode)
    after = random.random()
    sampler = MeetTrainingSampler(dataset, sizes, device=dev, zero_label_padding_mode=mode)
    random.seed(seed)
    chosen, glabels = sampler.sample(torch.from_numpy(labels).to(dev))
    assert random.random() == after
    for k in range(len(sizes)):
        assert np.array_equal(chosen[k].cpu().numpy(), np.array(want[k], dtype=np.int64)), k
        assert np.array_equal(glabels[k].cpu().numpy(), mc.group_labels(labels, want[k], incre, k)), k


def test_sampler_refuses_an_unknown_mode():
    from veto_amd.losses import MeetTrainingSampler
    with pytest.raises(NotImplementedError):
        MeetTrainingSampler("VG", [4, 6, 9, 19, 12], device="cuda:0", zero_label_padding_mode="rand_drop")


GRAD_TOL = 2e-3      # tests/test_train_scale_gpu.py: the bound of the same step, per element and on the norm


def _errors(got, ref):      # tests/test_train_scale_gpu.py::_errors
    got, ref = got.reshape(-1).double(), ref.reshape(-1).double()
    norm = float(ref.norm())
    scale = max(float(ref.abs().max()), norm / ref.numel() ** 0.5, 1e-12)
    return float((got - ref).abs().max()) / scale, abs(float(got.norm()) - norm) / max(norm, 1e-12)


def _meet_predictor(name, mode, forward_only):
    """The predictor of a MEET training golden's shapes (2 layers / 8 heads, 7 + 5 + 9 objects) in .train(), dropout off, under `mode`."""
    from veto_amd import meet_tables, synth, testing
    from veto_amd.pairs import prepare_test_pairs
    dev = torch.device("cuda:0")
    g = _golden(name)
    dataset = str(g["dataset"])
    n_obj_cls = 151 if dataset == "VG" else 201
    num_objs, sizes = [int(x) for x in g["num_objs"]], [int(x) for x in g["group_sizes"]]
    layers, heads = int(g.get("layers", 2)), int(g.get("heads", 8))
    assert (layers, heads, num_objs) == (2, 8, [7, 5, 9])
    cfg = testing.make_config(layers, heads, str(g["mode"]), True, dataset)
    cfg.GCL_SETTING.ZERO_LABEL_PADDING_MODE = mode
    cfg.VETO_AMD.TRAIN_FORWARD_ONLY = forward_only
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
    sd = synth.meet_state_dict(0, sizes, layers=layers, num_obj_cls=n_obj_cls)
    model = testing.make_predictor(cfg, sd, dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    batch = synth.synthetic_batch(7, len(num_objs), num_objs, num_obj_cls=n_obj_cls)
    props = testing.make_proposals(batch, str(g["mode"]), dev)
    pairs = prepare_test_pairs(dev, props)
    labels = g["labels"]
    assert int((labels == 0).sum()) > 0 and int((labels != 0).sum()) > 0
    rel_labels = list(torch.from_numpy(labels).to(dev).split([int(p.shape[0]) for p in pairs]))
    incre = meet_tables.incre_idx_list(sizes)
    rates = meet_tables.sample_rate_matrix(dataset, sizes)

    def run():
        return model(props, pairs, rel_labels, None, roi_features=torch.from_numpy(batch["roi_features"]).to(dev),
                     roi_depth_features=torch.from_numpy(batch["roi_depth_features"]).to(dev))
    return dict(g=g, model=model, run=run, sd=sd, batch=batch, pairs=pairs, labels=labels, sizes=sizes, incre=incre, rates=rates,
                layers=layers, heads=heads)


@pytest.mark.parametrize("mode", mc.MODES)
def test_predictor_returns_the_restatements_lists(mode):
    """The fifth return value of VETOPredictor_MEET in training mode, for several seeds of Python's generator on one model."""
    c = _meet_predictor("train_meet_vg", mode, forward_only=True)
    for seed in (1, 5, 99):
        random.seed(seed)
        want = mc.sample_stdlib(c["labels"], c["incre"], c["rates"], len(c["sizes"]), mode)
        after = random.random()
        random.seed(seed)
        out = c["run"]()
        assert random.random() == after
        for k in range(len(c["sizes"])):
            assert np.array_equal(out[4][0][k].cpu().numpy(), np.array(want[k], dtype=np.int64)), (seed, k)
        assert all(bool(torch.isfinite(v)) for v in out[2].values())


@pytest.mark.parametrize("mode", ["rand_choose", "all_include"])
@pytest.mark.parametrize("name", ["train_meet_vg", "train_meet_gqa"])
def test_training_step_in_the_new_modes(name, mode):
    """One step at the smallest golden shapes (2 layers / 8 heads, 7 + 5 + 9 objects, dropout off): the predictor's lists equal the
    stdlib restatement and leave Python's generator where it would; losses and EVERY element of every parameter gradient against
    oracle.train_oracle.train_step on the device's own lists."""
    from oracle import train_oracle as to
    from oracle import veto_oracle as vo
    c = _meet_predictor(name, mode, forward_only=False)
    g, model, sd, batch, pairs, labels, sizes, incre = (c[k] for k in ("g", "model", "sd", "batch", "pairs", "labels", "sizes", "incre"))
    layers, heads = c["layers"], c["heads"]
    random.seed(3)
    want = mc.sample_stdlib(labels, incre, c["rates"], len(sizes), mode)
    after = random.random()
    random.seed(3)
    out = c["run"]()
    assert random.random() == after
    lists = [c.cpu().numpy() for c in out[4][0]]
    for k in range(len(sizes)):
        assert np.array_equal(lists[k], np.array(want[k], dtype=np.int64)), k
    sum(out[2].values()).backward()
    torch.cuda.synchronize()
    ocfg = vo.OracleConfig(layers, heads, mode=str(g["mode"]), meet_groups=sizes, prefix="model.")
    ref = to.train_step(sd, ocfg, batch, [p.cpu().numpy() for p in pairs], labels, {"chosen": lists, "incre_idx_list": incre})
    assert set(out[2]) == set(ref["losses"])
    for k, v in out[2].items():
        assert abs(float(v.detach()) - ref["losses"][k]) < 2e-4 * max(1.0, abs(ref["losses"][k])), (k, float(v.detach()), ref["losses"][k])
    params = dict(model.named_parameters(remove_duplicate=False))
    worst = 0.0
    for pname, wanted in ref["grads"].items():
        assert params[pname].grad is not None, pname
        e, ne = _errors(params[pname].grad.detach().cpu(), wanted)
        worst = max(worst, e, ne)
        assert e < GRAD_TOL and ne < GRAD_TOL, (pname, e, ne)
    print("PARITY step %s %s: worst element / norm error %.2e over %d parameters" % (name, mode, worst, len(ref["grads"])))
