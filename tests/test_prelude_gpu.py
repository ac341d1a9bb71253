"""The eval forward outside the two fused kernels, stage by stage against float64, at the edges (tests/prelude_cases.py):
pair_indices_kernel, bn_batch_stats_kernel, obj_prep_kernel, patchify_kernel + gemm_patch, both instantiations of
assemble_kernel (L = 1: the LayerNorm-storing one, L >= 2: STATS_ONLY; VETO_X_F24=1: the 3-byte store path) and head_kernel.

Every call goes through veto_forward with a hand-filled veto_inputs_t (zero-pair images, xywh boxes and batch statistics in an eval
call cannot be expressed through the predictor).  Every output buffer starts as a sentinel with guard cells behind it: each element
must be overwritten, the guards must survive, and every call is made twice and must repeat bit for bit.

Precision modes: the prelude does not differ between VETO_PRECISE and VETO_MIXED in anything these tests read.  gemm_patch takes
split-bf16 operands in both (abi_forward.hip, object_side: run_gemm on ws.pa / h->patch_w without a mixed exponent), obj_prep and
assemble compute in float32, and assemble_args' a_fmt only selects the format of the LayerNorm'ed rows of tokens 17 / 18, which go
to layer 0's QKV GEMM, not into the token rows.  So the cases run on the default (mixed) handle and
test_token_rows_do_not_depend_on_the_precision_mode holds a precise handle to the same bits.  The only prelude store path a mode
owns is the 3-byte one (mixed, L >= 3, VETO_X_F24=1): test_three_byte_token_rows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prelude_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 64
SENT32 = 0x7fc5a5a5                       # a NaN no kernel produces
SENT64 = 0x5a5a5a5a5a5a5a5a               # no index


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Guarded:
    """numel elements of sentinel, GUARD more behind them"""

    def __init__(self, numel, dtype, dev):
        self.numel, self.wide = numel, dtype == torch.int64
        self.raw = torch.full((numel + GUARD,), SENT64 if self.wide else SENT32, dtype=torch.int64 if self.wide else torch.int32, device=dev)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def bits(self, what):
        raw = self.raw.cpu().numpy()
        sent = SENT64 if self.wide else SENT32
        assert (raw[self.numel:] == sent).all(), "%s: guard cells behind the buffer were written" % what
        left = int((raw[:self.numel] == sent).sum())
        assert left == 0, "%s: %d of %d elements were never written" % (what, left, self.numel)
        return raw[:self.numel]


_ENGINES = {}


def engine(layers, num_obj_cls=151, num_out=51, precision="mixed", chunk=0, var0=False, heads=8, keep=True):
    """(native.Engine with the synthetic weights loaded, its state dict)"""
    from veto_amd import native
    key = (layers, num_obj_cls, num_out, precision, chunk, var0, heads)
    if key in _ENGINES:
        return _ENGINES[key]
    dev = _dev()
    sd = pc.state_dict(layers, num_obj_cls, num_out, var0)
    eng = native.Engine(layers, heads, num_obj_cls, num_out, precision={"mixed": native.VETO_MIXED, "precise": native.VETO_PRECISE}[precision],
                        device=0, max_chunk_pairs=chunk)
    stream = torch.cuda.current_stream(dev).cuda_stream
    held = []
    for name, numel in eng.weight_specs():
        t = torch.from_numpy(np.ascontiguousarray(sd[name], dtype=np.float32)).to(dev).reshape(-1)
        assert t.numel() == numel, (name, t.numel(), numel)
        held.append(t)
        eng.load_weight(name, t.data_ptr(), numel, stream)
    torch.cuda.synchronize()
    if keep:
        _ENGINES[key] = (eng, sd)
    return eng, sd


def run(eng, case, num_out=51):
    """veto_forward on the case, twice; returns dict(logits [P, n_out], subj, obj int64 [P], tokens [P, 19, 576], cls [P, 576]
    float32, stats [12] or None) of the first call after holding the second to the same bits."""
    from veto_amd import native
    dev = _dev()
    P, N = pc.n_pair(case), len(case["boxes"])

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    rgb, dep, boxes = up(case["rgb"]), up(case["dep"]), up(case["boxes"])
    pairs = up(np.concatenate(case["pairs"]).astype(np.int64))
    ooff = up(np.concatenate([[0], np.cumsum(case["num_objs"])]).astype(np.int32))
    poff = up(np.concatenate([[0], np.cumsum([len(p) for p in case["pairs"]])]).astype(np.int32))
    lab = up(case["labels"]) if case["labels"] is not None else None
    lg = up(case["logits"]) if case["logits"] is not None else None
    ws = torch.empty(eng.workspace_bytes(N, P), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = []
    for _ in range(2):
        f32, i64 = torch.float32, torch.int64
        bufs = {"logits": Guarded(P * num_out, f32, dev), "subj": Guarded(P, i64, dev), "obj": Guarded(P, i64, dev),
                "tokens": Guarded(P * pc.TOKENS * pc.DIM, f32, dev), "cls": Guarded(P * pc.DIM, f32, dev)}
        if case["bn_batch"]:
            bufs["stats"] = Guarded(12, f32, dev)
        inp = native.VetoInputs(struct_size=ctypes.sizeof(native.VetoInputs), n_obj=N, n_pair=P, n_img=len(case["num_objs"]),
                                roi_rgb=rgb.data_ptr(), roi_depth=dep.data_ptr(), boxes=boxes.data_ptr(), box_mode=case["box_mode"],
                                obj_labels=lab.data_ptr() if lab is not None else None, obj_logits=lg.data_ptr() if lg is not None else None,
                                rel_pairs=pairs.data_ptr(), img_obj_offset=ooff.data_ptr(), img_pair_offset=poff.data_ptr(),
                                bn_batch_stats=bufs["stats"].ptr if case["bn_batch"] else None)
        # dbg.tokens and dbg.cls are copies of workspace rows: a row the kernels never wrote would otherwise show whatever an earlier
        # call left there -- possibly the right values.  (The workspace holds no index that is read before it is written.)
        ws.fill_(0x5a)
        dbg = native.VetoDebugOutputs(struct_size=ctypes.sizeof(native.VetoDebugOutputs), subj_inds=bufs["subj"].ptr,
                                      obj_inds=bufs["obj"].ptr, tokens=bufs["tokens"].ptr, cls=bufs["cls"].ptr)
        eng.forward(stream, inp, ws.data_ptr(), ws.numel(), bufs["logits"].ptr, dbg)
        torch.cuda.synchronize()
        reps.append({k: b.bits("%s / %s" % (case["name"], k)) for k, b in bufs.items()})
    for k in reps[0]:
        assert np.array_equal(reps[0][k], reps[1][k]), "%s / %s: the second call differs from the first" % (case["name"], k)
    r = reps[0]
    out = {"logits": r["logits"].view(np.float32).reshape(P, num_out), "subj": r["subj"], "obj": r["obj"],
           "tokens": r["tokens"].view(np.float32).reshape(P, pc.TOKENS, pc.DIM), "cls": r["cls"].view(np.float32).reshape(P, pc.DIM),
           "stats": r["stats"].view(np.float32) if "stats" in r else None}
    return out


KINDS = (("patch", slice(1, 17)), ("location", slice(17, 18)), ("class", slice(18, 19)))


def check_tokens(tag, sd, case, got, stats=None, patch=True):
    """The device's token rows against the float64 oracle, per element inside the derived bound of prelude_cases.restate; the
    float32 oracle's error on the same bound is printed beside it (the yardstick: what plain float32 costs on this case)."""
    ref, subj, obj = pc.oracle_tokens(sd, case, stats=stats, patch=patch)
    f32, _, _ = pc.oracle_tokens(sd, case, dtype=torch.float32, stats=stats, patch=patch)
    _, bound, _, _ = pc.restate(sd, case, stats=stats, patch=patch)
    assert np.array_equal(got["subj"], subj) and np.array_equal(got["obj"], obj), tag
    assert np.array_equal(got["tokens"][:, 0].view(np.uint32), np.broadcast_to(pc.cls_row(sd), (len(subj), pc.DIM)).view(np.uint32)), \
        "%s: the CLS row is not the float32 sum of cls_token and pos_embedding" % tag
    line, worst = [], {}
    for kind, sl in KINDS:
        if not patch and kind == "patch":
            continue
        worst[kind] = pc.worst_ratio(got["tokens"][:, sl], ref[:, sl], bound[:, sl])
        line.append("%s err %.2e of bound %.3f (float32 oracle %.3f)" % (
            kind, np.abs(got["tokens"][:, sl].astype(np.float64) - ref[:, sl]).max(), worst[kind], pc.worst_ratio(f32[:, sl], ref[:, sl], bound[:, sl])))
        if kind != "patch":
            # The derived bound is a worst case (every rounding in the same direction).  The location / class rows are plain float32
            # chains, so they are also held to the yardstick convention of test_train_scale_gpu.py: 4 x the error of the float32
            # oracle against the float64 one on this case, plus a floor of 4 float32 ulps of the element.  (Not the patch rows: their
            # operands are split bf16, a 2^-16-class format the float32 oracle says nothing about.)
            yard = np.abs(f32[:, sl].astype(np.float64) - ref[:, sl]).max()
            allowed = 4 * yard + 4 * pc.ulp32(ref[:, sl])
            tight = pc.worst_ratio(got["tokens"][:, sl], ref[:, sl], allowed)
            line[-1] += ", %.3f of 4 x yardstick %.2e + 4 ulp" % (tight, yard)
            worst[kind + " (yardstick)"] = tight
    print("PRELUDE %s: %s" % (tag, "; ".join(line)))
    for kind, w in worst.items():
        assert w <= 1.0, "%s: %s tokens at %.3g x their bound" % (tag, kind, w)
    return ref, bound


# ---- pair indices -------------------------------------------------------------------------------------------------------------------
PAIR_INDEX_CASES = pc.pair_index_cases()


@pytest.mark.parametrize("name", sorted(PAIR_INDEX_CASES))
def test_pair_indices_bit_exact(name):
    """pair_indices_kernel against the loop of roi_relation_predictors.py:4106-4115: 1 to 257 images, one-object images with their
    (0, 0) placeholder, images without pairs at the front, in the middle, twice in a row and at the end, sampled lists with
    repeats and self-pairs.  The int64 outputs bit for bit; the int32 ones are what assemble_kernel gathers with, so the location /
    class rows of every pair must be those of the oracle's pair."""
    case = PAIR_INDEX_CASES[name]
    eng, sd = engine(1)
    got = run(eng, case)
    subj, obj = pc.reference_indices(case)
    assert np.array_equal(got["subj"], subj) and np.array_equal(got["obj"], obj)
    check_tokens(name, sd, case, got, patch=False)


# ---- token rows ---------------------------------------------------------------------------------------------------------------------
TOKEN_CASES = pc.token_cases()
TOKEN_RUNS = [(n, layers, 0) for n in sorted(TOKEN_CASES) for layers in (1, 2)] + \
             [("pairs_%d" % c, layers, chunk) for c in (6, 27, 28, 36) for layers in (1, 2) for chunk in (5, 7)]


@pytest.mark.parametrize("name,layers,chunk", TOKEN_RUNS)
def test_token_rows_against_fp64(name, layers, chunk):
    """All 19 token kinds per element: the CLS row bit for bit, the patch tokens inside the split-bf16 bound of gemm_patch, the
    location / class rows inside the float32 chain's bound.  L = 1 runs assemble_kernel<false>, L = 2 assemble_kernel<true>; the
    pair counts put 19 n_pair rows on either side of the grid's roundings to 8 workgroups; chunks of 5 and 7 split images and end
    on one pair (6 = 5 + 1, 36 = 7 x 5 + 1 = 5 x 7 + 1) and must give the unchunked rows bit for bit."""
    case = TOKEN_CASES[name]
    eng, sd = engine(layers, case["num_obj_cls"], chunk=chunk, var0=case["var0"])
    got = run(eng, case)
    check_tokens("%s L%d chunk %d" % (name, layers, chunk), sd, case, got)
    if chunk:
        whole = run(engine(layers, case["num_obj_cls"], var0=case["var0"])[0], case)
        assert np.array_equal(got["tokens"].view(np.uint32), whole["tokens"].view(np.uint32))


@pytest.mark.parametrize("maps", ["outliers", "var0"])
@pytest.mark.parametrize("layers", [1, 2])
def test_xyxy_and_xywh_boxes_give_the_same_rows(maps, layers):
    """The xyxy and the xywh form of the same boxes.  The boxes lie on a grid of quarters, so fl(x2 - x1) + 1 is exact and the
    rounding in which the two modes could differ does not happen: the token rows must be equal bit for bit."""
    a, b = TOKEN_CASES["hard_boxes_xyxy_" + maps], TOKEN_CASES["hard_boxes_xywh_" + maps]
    eng, _ = engine(layers, var0=a["var0"])
    ta, tb = run(eng, a)["tokens"], run(eng, b)["tokens"]
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))


def test_token_rows_do_not_depend_on_the_precision_mode():
    case = TOKEN_CASES["pairs_28"]
    for layers in (1, 2):
        mixed = run(engine(layers)[0], case)["tokens"]
        precise = run(engine(layers, precision="precise")[0], case)["tokens"]
        assert np.array_equal(mixed.view(np.uint32), precise.view(np.uint32)), layers


def f24_child(path):
    """(child process, VETO_X_F24=1) the token rows of an L = 3 mixed handle"""
    case = pc.token_cases()["pairs_36"]
    eng, _ = engine(3)
    np.save(path, run(eng, case)["tokens"])


def test_three_byte_token_rows(tmp_path):
    """VETO_X_F24=1 (read once per process, hence a child): assemble_kernel<true> writes the token rows as 3-byte floats.  Every
    value must lie on that grid (otherwise the knob was not on and the test checked nothing), the CLS row is the 3-byte rounding
    of its float32 sum, and every other element is within its float32 bound plus one step of the 3-byte format of the oracle."""
    import operand_cases as oc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_prelude_gpu as t\nt.f24_child(sys.argv[1])\n" % (root, os.path.join(root, "tests")))
    path = str(tmp_path / "tokens.npy")
    subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, VETO_X_F24="1"), timeout=300)
    tok = np.load(path)
    assert (tok.view(np.uint32) & 0xff == 0).all(), "the token rows are not 3-byte floats: VETO_X_F24 was not in force"
    case = TOKEN_CASES["pairs_36"]
    sd = pc.state_dict(3)
    assert np.array_equal(tok[:, 0].view(np.uint32), np.broadcast_to(oc.f24(pc.cls_row(sd)), tok[:, 0].shape).view(np.uint32))
    ref, _, _ = pc.oracle_tokens(sd, case)
    _, bound, _, _ = pc.restate(sd, case)
    wide = bound + pc.f24_step(np.abs(ref) + bound)
    w = pc.worst_ratio(tok[:, 1:], ref[:, 1:], wide[:, 1:])
    print("PRELUDE f24 pairs_36 L3: err %.2e, %.3f of (float32 bound + one 3-byte step)" % (np.abs(tok[:, 1:] - ref[:, 1:]).max(), w))
    assert w <= 1.0, w


# ---- training-mode BatchNorm inside the eval forward --------------------------------------------------------------------------------
BN_CASES = pc.bn_cases()


@pytest.mark.parametrize("name", sorted(BN_CASES))
def test_batch_statistics_in_the_eval_forward(name):
    """veto_inputs_t.bn_batch_stats in a veto_forward call: the twelve statistics of bn_batch_stats_kernel (a double two-pass with
    one float32 rounding at the store) against float64 at 2, 255, 256, 257 and 513 objects, in both box modes, and the location rows
    against the oracle normalising with the device's statistics.  Identical boxes: both variances exactly 0, the mean exactly the
    feature."""
    case = BN_CASES[name]
    eng, sd = engine(1)
    got = run(eng, case)
    ref, bound = pc.batch_statistics(case)
    st = got["stats"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(st == ref, 0.0, np.abs(st - ref) / bound)
    print("PRELUDE %s: statistics at most %.3f of their bound (mean %.2e, var %.2e relative)" % (
        name, ratio.max(), (np.abs(st - ref)[:4] / np.abs(ref[:4])).max(), (np.abs(st - ref)[4:] / np.maximum(ref[4:], 1e-300)).max()))
    assert ratio.max() <= 1.0, (name, ratio)
    if "identical" in name:
        v, _ = pc.box_features(case)
        assert np.array_equal(got["stats"][:4], v[0].astype(np.float32)) and (got["stats"][4:] == 0).all()
    check_tokens(name, sd, case, got, stats=got["stats"], patch=False)
    if name.endswith("xywh"):      # the same boxes in xyxy mode (features exact in both): the same twelve numbers
        twin = run(eng, BN_CASES[name.replace("xywh", "xyxy")])
        assert np.array_equal(twin["stats"].view(np.uint32), got["stats"].view(np.uint32))


def test_batch_statistics_of_one_object():
    """n_obj = 1: the reference's nn.BatchNorm1d raises ('Expected more than 1 value per channel when training').  The library
    does not: it returns mean = the feature, biased variance 0 and, where n - 1 would divide, the plain sum of squares, 0, and
    normalises with (v - v) / sqrt(eps) = 0, so the box enters as the BatchNorm bias alone.  Pinned here, not changed."""
    case = pc.make_case("bn_one_object", [1], [np.zeros((1, 2), dtype=np.int64)], maps="zeros", bn_batch=True)
    eng, sd = engine(1)
    got = run(eng, case)
    v, _ = pc.box_features(case)
    assert np.array_equal(got["stats"][:4], v[0].astype(np.float32)) and (got["stats"][4:] == 0).all()
    check_tokens("bn_one_object", sd, case, got, stats=got["stats"], patch=False)


# ---- classifier head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", pc.HEAD_CHUNKS)
@pytest.mark.parametrize("width", pc.HEAD_WIDTHS)
def test_head_against_its_own_input(width, chunk):
    """head_kernel isolated from the transformer: out_logits against cls_dev @ W^T + b in float64 with the device's own dbg.cls,
    per element inside gamma(577) (sum |w||cls| + |b|).  Widths 51 / 101 / 60 / 108 are the shipped ones; 128, 129 and 257 (which
    veto_create accepts: num_out up to 4096) end the class loop's first trip exactly, start its second and reach its third.  Pair
    counts 1..5 with chunks of 1, 3 and 5 give workgroups of 1, 2, 3 and 4 live pairs at chunk offsets 0..4."""
    eng, sd = engine(1, num_out=width, chunk=chunk, keep=False)
    worst = 0.0
    for count in pc.HEAD_PAIR_COUNTS:
        num_objs, pairs = ([1], [np.zeros((1, 2), dtype=np.int64)]) if count == 1 else ([3], [pc.vo.enumerate_test_pairs(3)[:count]])
        case = pc.make_case("head_%d" % count, num_objs, pairs, maps="gauss")
        got = run(eng, case, num_out=width)
        ref, bound = pc.head_reference(sd, got["cls"])
        assert np.isfinite(got["logits"]).all()
        worst = max(worst, float((np.abs(got["logits"] - ref) / bound).max()))
    eng.close()
    print("PRELUDE head width %d chunk %d: at most %.3f of gamma_577 (sum |w||cls| + |b|)" % (width, chunk, worst))
    assert worst <= 1.0, worst
