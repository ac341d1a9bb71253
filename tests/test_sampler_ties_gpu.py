"""Hash ties at the quota cut on the MI355X: box_subsample_kernel, rpn_sample_kernel (both paths) and gtbox_relsample_kernel on the
constructions of tests/sampler_tie_cases.py, where two members of a draw share a 32-bit hash and the cut falls before, inside or
behind that pair.  Every output buffer is pre-filled with a sentinel; indices, pairs, labels and counts are compared bit for bit
with the numpy restatements, the rows behind the counts must still hold the sentinel, and independently of the restatements there
are exactly K rows, none twice, all members, in the documented order, with the lower index of a split pair kept.  Every call runs
twice.  Nothing here has a tolerance."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_tie_cases as tc  # noqa: E402
from sampler_tie_cases import PICK_BG, PICK_FG, np_hash32  # noqa: E402
from test_rpnloss_gpu import _call, _inputs_for_labels  # noqa: E402

from veto_amd import boxsampling as bs  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777


@contextlib.contextmanager
def sentinel_outputs():
    """The wrappers allocate their outputs with torch.empty: inside this block every such tensor starts as the sentinel."""
    real = torch.empty

    def filled(*args, **kw):
        t = real(*args, **kw)
        if t.numel():
            t.fill_(0xA5 if t.dtype == torch.uint8 else SENTINEL)
        return t
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _twice(fn):
    """fn() under the sentinel, twice: the second result, after asserting both are the same bytes."""
    with sentinel_outputs():
        first, second = fn(), fn()
    torch.cuda.synchronize()
    first, second = [x.cpu().numpy() for x in first], [x.cpu().numpy() for x in second]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two calls of the same inputs differ"
    return second


def _assert_tie_rows(im, rows):
    """What the placement says about the tied pair, whatever the restatement: the lower index wins a split."""
    rows = set(np.asarray(rows).tolist())
    for t in im["ties"]:
        want = {"split": (True, False), "both": (True, True), "neither": (False, False)}[t["placement"]]
        assert (t["e_lo"] in rows, t["e_hi"] in rows) == want, (im["name"], t)


def _assert_label_rows(im, buffer, counts):
    """One image of a label kernel: buffer [batch] int64 with the sentinel behind the rows, counts = its number of rows or
    (positives, negatives)."""
    pos, neg, num_pos, num_neg = tc.np_quota(im["labels"], im["batch"], im["fraction"])
    total = int(np.sum(counts))
    if np.ndim(counts):
        assert list(counts) == [num_pos, num_neg], im["name"]
    assert total == num_pos + num_neg, (im["name"], total, num_pos, num_neg)            # exactly K rows per class
    rows = buffer[:total]
    assert (buffer[total:] == SENTINEL).all(), "%s: a row was written behind the count" % im["name"]
    assert (np.diff(rows) > 0).all(), "%s: not ascending, or a row twice" % im["name"]
    assert int(np.isin(rows, pos).sum()) == num_pos and int(np.isin(rows, neg).sum()) == num_neg, im["name"]   # every row a member
    _assert_tie_rows(im, rows)
    np.testing.assert_array_equal(rows, tc.label_expected(im), err_msg=im["name"])


# ---- box_subsample_kernel ---------------------------------------------------------------------------------------------------

FILLER = np.array([1, 0, 0, -1, 0] * 10, np.int64)      # the images in front of a case whose image index is above 0


def _box_run(label_lists, batch, fraction, seed):
    labels = torch.from_numpy(np.concatenate(label_lists)).to(DEV)
    return _twice(lambda: bs.box_subsample(labels, [len(x) for x in label_lists], batch, fraction, seed=seed))


@pytest.mark.parametrize("case", [c[0] for c in tc.BOX_CASES])
def test_box_subsample_with_a_hash_tie_at_the_cut(case):
    im = tc.box_images()[[c[0] for c in tc.BOX_CASES].index(case)]
    sampled, counts = _box_run([FILLER] * im["img"] + [im["labels"]], im["batch"], im["fraction"], im["seed"])
    assert sampled.shape == (im["img"] + 1, im["batch"]) and sampled.dtype == np.int64 and counts.dtype == np.int32
    _assert_label_rows(im, sampled[im["img"]], counts[im["img"]])


def test_box_subsample_batch_of_four_with_a_tie_in_image_2_only():
    """Images 0, 1 and 3 give the rows they give beside an image 2 without a tie; image 2 its own."""
    tied, lists, plain = tc.box_batch_of_four()
    sampled, counts = _box_run(lists, tied["batch"], tied["fraction"], tied["seed"])
    other, other_counts = _box_run(plain, tied["batch"], tied["fraction"], tied["seed"])
    _assert_label_rows(tied, sampled[2], counts[2])
    for i in (0, 1, 3):
        im = dict(tied, name="image %d" % i, img=i, labels=lists[i], ties=[])
        _assert_label_rows(im, sampled[i], counts[i])
        assert sampled[i].tobytes() == other[i].tobytes() and counts[i] == other_counts[i]


def test_box_subsample_at_the_first_digits_bin_boundaries():
    images = tc.box_boundary_images()
    sampled, counts = _box_run([im["labels"] for im in images], images[0]["batch"], images[0]["fraction"], images[0]["seed"])
    for im in images:
        _assert_label_rows(im, sampled[im["img"]], counts[im["img"]])


# ---- rpn_sample_kernel ------------------------------------------------------------------------------------------------------

def _rpn_run(images, levels):
    d = tc.rpn_inputs(images, levels, _inputs_for_labels)
    c = dict(high=0.7, low=0.3, lowq=False, straddle=-1, batch=images[0]["batch"], fraction=images[0]["fraction"])
    assert all((im["batch"], im["fraction"], im["seed"], im["img"]) == (c["batch"], c["fraction"], images[0]["seed"], i) for i, im in enumerate(images))
    outs = []
    with sentinel_outputs():
        for _ in range(2):
            outs.append(_call(c, d, ("labels", "sampled_inds", "counts"), seed=images[0]["seed"], head=False))
    for key in ("labels", "sampled_inds", "counts"):
        assert outs[0][key].tobytes() == outs[1][key].tobytes(), key
    out = outs[1]
    assert out["sampled_inds"].shape == (len(images), c["batch"]) and out["sampled_inds"].dtype == np.int64 and out["counts"].dtype == np.int32
    for im in images:
        np.testing.assert_array_equal(out["labels"][im["img"]], im["labels"].astype(np.float32), err_msg="the labels the inputs were built for")
        _assert_label_rows(im, out["sampled_inds"][im["img"]], out["counts"][im["img"]])
    return out


@pytest.mark.parametrize("call", ["neg", "pos"])
def test_rpn_sampler_lds_path_with_a_hash_tie_in_the_cut_bin(call):
    _rpn_run(tc.rpn_lds_calls()[call], tc.RPN_LDS_LEVELS)


@pytest.fixture(scope="module")
def stream_rows():
    return {}


@pytest.mark.parametrize("call", ["a", "b"])
def test_rpn_sampler_streaming_path_with_a_hash_tie_at_the_cut(call, stream_rows):
    """Four images per call, each its own construction; image 0 of "a" has 2 049 members in the negatives' cut bin (streaming),
    image 0 of "b" is the same image with one of them ignored (2 048: the LDS path), and both give the same rows."""
    out = _rpn_run(tc.rpn_stream_calls()[call], tc.RPN_STREAM_LEVELS)
    stream_rows[call] = out["sampled_inds"][0].copy()
    if len(stream_rows) == 2:
        assert stream_rows["a"].tobytes() == stream_rows["b"].tobytes()


def test_rpn_sampler_streaming_path_at_the_first_digits_bin_boundaries():
    _rpn_run(tc.rpn_boundary_images(), tc.RPN_STREAM_LEVELS)


# ---- gtbox_relsample_kernel -------------------------------------------------------------------------------------------------

def _gtbox_run(rels, batch, fraction, seed):
    from veto_amd.sampling import GTBoxRelationSampler

    def run():
        props, targets = [], []
        for rel in rels:
            boxes = torch.zeros((len(rel), 4), device=DEV)
            props.append(BoxList(boxes, (800, 600), "xyxy"))
            t = BoxList(boxes.clone(), (800, 600), "xyxy")
            t.add_field("relation", torch.from_numpy(np.ascontiguousarray(rel)).to(DEV))
            targets.append(t)
        _, labels, pairs, binary = GTBoxRelationSampler(batch, fraction).gtbox_relsample(props, targets, seed=seed)
        assert pairs[-1]._base is not None and labels[-1]._base is not None       # views of the whole [n_img * batch] buffers
        return [pairs[-1], labels[-1], binary[-1], pairs[-1]._base, labels[-1]._base]
    return _twice(run)


@pytest.mark.parametrize("case", [c[0] for c in tc.GTBOX_CASES])
def test_gtbox_relsample_with_a_hash_tie_at_the_cut(case):
    im = tc.gtbox_images()[[c[0] for c in tc.GTBOX_CASES].index(case)]
    n, B, img = im["n"], im["batch"], im["img"]
    rels = [np.zeros((1, 1), np.int64)] * img + [im["rel"]]          # (one object: no candidate, no row)
    pairs, labels, binary, all_pairs, all_labels = _gtbox_run(rels, B, im["num_pos"] / B, im["seed"])
    want_pairs, want_labels, want_binary, n_fg, n_bg = tc.gtbox_expected(im)
    cls = tc.gtbox_classes(im)
    # independently of the restatement: the counts, the members, no row twice, (hash, index) ascending per part
    assert (n_fg, n_bg) == (im["num_pos"], B - im["num_pos"]) and len(pairs) == len(labels) == B
    cells = pairs[:, 0] * n + pairs[:, 1]
    assert len(set(cells.tolist())) == len(cells)
    for purpose, part in ((PICK_FG, cells[:n_fg]), (PICK_BG, cells[n_fg:])):
        assert np.isin(part, cls[purpose][0]).all(), case
        key = (np_hash32(im["seed"], img, purpose, part).astype(np.uint64) << np.uint64(32)) | part.astype(np.uint64)
        assert (key[1:] > key[:-1]).all(), "%s: not in (hash, index) order" % case
    (t,) = im["ties"]
    part = (cells[:n_fg] if t["purpose"] == PICK_FG else cells[n_fg:]).tolist()
    _assert_tie_rows(im, part)
    if t["placement"] == "both":               # adjacent, the lower cell first: the order, not only the set
        assert part.index(t["e_hi"]) == part.index(t["e_lo"]) + 1 == len(part) - 1, case
    if t["placement"] == "split":
        assert part[-1] == t["e_lo"], case
    assert (labels[:n_fg] == im["rel"].reshape(-1)[cells[:n_fg]]).all() and (labels[n_fg:] == 0).all()
    # bit for bit against the restatement, and the sentinel everywhere behind the rows (the images in front have none)
    np.testing.assert_array_equal(pairs, want_pairs)
    np.testing.assert_array_equal(labels, want_labels)
    np.testing.assert_array_equal(binary, want_binary)
    assert all_pairs.shape == ((img + 1) * B, 2) and all_labels.shape == ((img + 1) * B,)
    assert (all_pairs[:img * B] == SENTINEL).all() and (all_labels[:img * B] == SENTINEL).all()


# ---- detect_relsample_kernel ------------------------------------------------------------------------------------------------

def _detect_lists(d):
    p = BoxList(torch.from_numpy(d["prp_boxes"]).to(DEV), (800, 600), "xyxy")
    p.add_field("labels", torch.from_numpy(d["prp_labels"]).to(DEV))
    p.add_field("pred_scores", torch.from_numpy(d["pred_scores"]).to(DEV))
    t = BoxList(torch.from_numpy(d["tgt_boxes"]).to(DEV), (800, 600), "xyxy")
    t.add_field("labels", torch.from_numpy(d["tgt_labels"]).to(DEV))
    t.add_field("relation", torch.from_numpy(d["relation"]).to(DEV))
    return p, t


# the image in front of a case whose image index is 1: one proposal, no candidate, so the two (0, 0, 0) placeholder rows
DETECT_FRONT = dict(prp_boxes=np.array([[0, 0, 9, 9]], np.float32), prp_labels=np.array([1], np.int64), pred_scores=np.array([0.5], np.float32),
                    tgt_boxes=np.array([[700, 500, 720, 520]], np.float32), tgt_labels=np.array([1], np.int64), relation=np.zeros((1, 1), np.int64))


@pytest.mark.parametrize("case", [c[0] for c in tc.DETECT_CASES])
def test_detect_relsample_with_a_hash_tie_at_the_cut(case):
    """The background pick over a whole window (purpose 2) and the foreground cap (purpose 1)."""
    from veto_amd.sampling import DetectRelationSampler
    im = tc.detect_images()[[c[0] for c in tc.DETECT_CASES].index(case)]
    img, cfg = im["img"], im["cfg"]

    def run():
        lists = [_detect_lists(DETECT_FRONT)] * img + [_detect_lists(im["d"])]
        _, labels, _, pairs, _ = DetectRelationSampler(*cfg).detect_relsample([p for p, _ in lists], [t for _, t in lists], seed=im["seed"])
        return [pairs[-1], labels[-1], pairs[-1]._base, labels[-1]._base]
    pairs, labels, all_pairs, all_labels = _twice(run)
    want = tc.detect_expected(im)
    s, cls = tc.detect_parts(im)
    (t,) = im["ties"]
    n_fg, num_neg, P = s["n_fg"], s["num_neg"], len(im["d"]["prp_boxes"])
    # independently of the restatement: exactly K rows of the tied draw, none twice, all members, (hash, element) ascending
    assert len(pairs) == len(labels) == n_fg + num_neg and (labels[:n_fg] > 0).all() and (labels[n_fg:] == 0).all()
    assert (n_fg if t["purpose"] == tc.DETECT_CAP_FG else num_neg) == t["K"]
    triplets = {(r["cand"][0][0], r["cand"][0][1]): k for k, r in enumerate(s["rels"])}          # one candidate per relation
    fg_pos = np.array([triplets[tuple(x)] for x in pairs[:n_fg].tolist()], np.int64)
    bg_flat = pairs[n_fg:, 0] * P + pairs[n_fg:, 1]
    for purpose, part in ((tc.DETECT_CAP_FG, fg_pos), (tc.DETECT_PICK_BG, bg_flat)):
        members, K = cls[purpose]
        assert len(set(part.tolist())) == len(part) and np.isin(part, members).all(), case
        if K is not None:
            key = (np_hash32(im["seed"], img, purpose, part).astype(np.uint64) << np.uint64(32)) | part.astype(np.uint64)
            assert (key[1:] > key[:-1]).all(), "%s: not in (hash, element) order" % case
    part = (fg_pos if t["purpose"] == tc.DETECT_CAP_FG else bg_flat).tolist()
    _assert_tie_rows(im, part)
    if t["placement"] == "both":
        assert part.index(t["e_hi"]) == part.index(t["e_lo"]) + 1 == len(part) - 1, case
    if t["placement"] == "split":
        assert part[-1] == t["e_lo"], case
    # bit for bit against the restatement, and the sentinel behind the rows of every image
    np.testing.assert_array_equal(pairs, want[:, :2])
    np.testing.assert_array_equal(labels, want[:, 2])
    rows = max(cfg[3], 2)
    assert all_pairs.shape == ((img + 1) * rows, 2) and all_labels.shape == ((img + 1) * rows,)
    for i, used in [(k, 2) for k in range(img)] + [(img, len(pairs))]:
        assert (all_pairs[i * rows + used:(i + 1) * rows] == SENTINEL).all() and (all_labels[i * rows + used:(i + 1) * rows] == SENTINEL).all(), case
