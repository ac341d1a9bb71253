"""sgdet decode and test pairs on the MI355X, on every branch, limit and tie: the cases of tests/sgdet_cases.py (their premises
are asserted on the CPU by tests/test_sgdet_cases_host.py) through veto_amd.sgdet.decode_objects, veto_amd.pairs.prepare_test_pairs
and the raw C ABI with guard cells behind every output and behind the workspace's stated size.

Decode: labels bit-equal to the numpy restatement on every row (re-picked and never-picked rows included), boxes bit-equal to
boxes_per_cls[i, label_i], scores within rtol 1e-6.  Pairs: rows, order and counts bit-equal to np_pairs.  mixed_homes and
word_edges: every image also bit-equal to the same image run alone."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgdet_cases as sc  # noqa: E402
from test_sgdet_host import load_golden, np_decode_scores, np_pairs, pair_qualities  # noqa: E402

from veto_amd import native  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                      # cells behind every output
SENTINEL = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, tail=()):
    return torch.full((n + GUARD,) + tuple(tail), SENTINEL, dtype=dtype, device=DEV)


def _intact(t, n, what):
    assert bool((t[n:] == SENTINEL).all()), "guard cells behind %s were written" % what
    return t[:n].cpu().numpy()


def _wrapper_decode(imgs, thr, mode):
    from veto_amd.sgdet import decode_objects
    n_objs = [len(d["predict_logits"]) for d in imgs]
    bpc = _dev(np.concatenate([d["boxes_per_cls"] for d in imgs]))
    if mode == "post":
        lab, s, b = decode_objects(_dev(np.concatenate([d["predict_logits"] for d in imgs])), bpc, n_objs, thr, mode="post")
        return lab.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy()
    lab, _, b = decode_objects(_dev(np.concatenate([d["pred_labels"] for d in imgs])), bpc, n_objs, thr, mode="meet", want_scores=False)
    return lab.cpu().numpy(), None, b.cpu().numpy()


WS_FILL = 0x5A


def _raw_decode(imgs, thr, mode, want_scores=True, want_boxes=True, ws_out=None):
    """veto_obj_decode through the raw ABI: guard cells behind obj_pred, obj_scores, boxes and the workspace's stated size.
    In "meet" mode with want_scores the logits are passed too (the ABI allows scores there).  ws_out: a list that receives
    the workspace's first n_obj * C floats as the launch left them (every byte was WS_FILL before)."""
    n_objs = [len(d["predict_logits"]) for d in imgs]
    n_obj, C = sum(n_objs), imgs[0]["predict_logits"].shape[1]
    call = native.Launch(DEV, "needs a HIP device")
    logits = _dev(np.concatenate([d["predict_logits"] for d in imgs])) if mode == "post" or want_scores else None
    labels = _dev(np.concatenate([d["pred_labels"] for d in imgs])) if mode == "meet" else None
    bpc = _dev(np.concatenate([d["boxes_per_cls"] for d in imgs]))
    pred = _guarded(n_obj, torch.int64)
    scores = _guarded(n_obj, torch.float32) if want_scores else None
    boxes = _guarded(n_obj, torch.float32, (4,)) if want_boxes else None
    need = call.lib.veto_obj_decode_workspace_bytes(n_obj, C)
    assert need >= n_obj * C * 4
    ws = torch.full((need + 4 * GUARD,), WS_FILL, dtype=torch.uint8, device=DEV)
    a = call.args(native.VetoObjDecodeArgs, n_img=len(n_objs), n_obj=n_obj, n_cls=C, max_obj_per_image=max(n_objs),
                  mode={"post": 0, "meet": 1}[mode], nms_thres=float(thr), logits=logits, labels=labels, boxes_per_cls=bpc,
                  img_obj_offset=native.device_offsets(n_objs, device=torch.device(DEV))[0], obj_pred=pred, obj_scores=scores, boxes=boxes)
    call.run("veto_obj_decode", ctypes.byref(a), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert bool((ws[need:] == WS_FILL).all()), "the workspace was written past its stated size"
    if ws_out is not None:
        ws_out.append(ws[:n_obj * C * 4].cpu().numpy().view(np.float32).reshape(n_obj, C))
    return (_intact(pred, n_obj, "obj_pred"), _intact(scores, n_obj, "obj_scores") if want_scores else None,
            _intact(boxes, n_obj, "boxes") if want_boxes else None)


def _check_decode(imgs, thr, mode, got, what):
    lab, scores, boxes = got
    want = np.concatenate([sc.expected_decode(d, thr, mode) for d in imgs])
    np.testing.assert_array_equal(lab, want, err_msg=what)                       # every row: no row is excluded
    bpc = np.concatenate([d["boxes_per_cls"] for d in imgs])
    if boxes is not None:
        np.testing.assert_array_equal(boxes, bpc[np.arange(len(lab)), lab], err_msg=what)
    if scores is not None:
        ref = np_decode_scores(np.concatenate([d["predict_logits"] for d in imgs]), lab)
        np.testing.assert_allclose(scores, ref, rtol=1e-6, atol=0, err_msg=what)
        np.testing.assert_array_equal(scores == 0, lab == 0)                     # background rows: exactly 0


@pytest.mark.parametrize("name", sc.DECODE_CASE_NAMES)
def test_decode_matches_the_restatement(name):
    for li, (imgs, thr) in enumerate(sc.decode_case(name)):
        for mode in sc.MODES:                    # both modes on every case, whichever it is named for
            what = "%s launch %d %s" % (name, li, mode)
            _check_decode(imgs, thr, mode, _wrapper_decode(imgs, thr, mode), what + " (wrapper)")
            _check_decode(imgs, thr, mode, _raw_decode(imgs, thr, mode), what + " (raw ABI)")


@pytest.mark.parametrize("name", sc.GOLDEN_DECODE)
def test_decode_matches_the_reference_on_the_cases(name):
    g = load_golden("decode_cases")
    mode, = sc.decode_modes(name)
    labs, scores = [], []
    for imgs, thr in sc.decode_case(name):
        lab, s, _ = _raw_decode(imgs, thr, mode, want_scores=mode == "post")
        labs.append(lab)
        scores.append(s)
    np.testing.assert_array_equal(np.concatenate(labs), g[name + "__labels"])
    if mode == "post":
        np.testing.assert_allclose(np.concatenate(scores), g[name + "__scores"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", ["post", "meet"])
def test_mixed_homes_images_equal_themselves_alone_and_outputs_are_independent(mode):
    imgs, thr = sc.mixed_homes()[0]
    full = _raw_decode(imgs, thr, mode)
    _check_decode(imgs, thr, mode, full, "mixed_homes " + mode)
    off = np.cumsum([0] + [len(d["predict_logits"]) for d in imgs])
    assert off[4] > 0 and off[1] > 0                                    # the second workspace image sits at a non-zero offset
    for i, d in enumerate(imgs):
        if not len(d["predict_logits"]):
            continue
        alone = _raw_decode([d], thr, mode)
        for f, a in zip(full, alone):
            np.testing.assert_array_equal(f[off[i]:off[i + 1]], a, err_msg="image %d alone" % i)     # bit-equal, scores included
    # obj_scores null, boxes null, both null: what remains is unchanged
    for want_scores, want_boxes in ((False, True), (True, False), (False, False)):
        part = _raw_decode(imgs, thr, mode, want_scores=want_scores, want_boxes=want_boxes)
        for f, p in zip(full, part):
            if p is not None:
                np.testing.assert_array_equal(f, p, err_msg="scores %s boxes %s" % (want_scores, want_boxes))


@pytest.mark.parametrize("mode", ["post", "meet"])
def test_workspace_images_use_their_own_rows_of_the_workspace(mode):
    """The matrix of an image that does not fit in LDS lives at prob_ws + offset * C (sgdet.hip's header): after a launch those
    rows hold the decode's last state (0, -1 or a probability) and the rows of LDS and empty images still hold the fill.
    An image handed another image's rows computes the right answer whenever the two workgroups do not see each other's
    stores, so the labels alone cannot show it."""
    fill = np.frombuffer(bytes([WS_FILL] * 4), np.float32)[0]
    for imgs, thr in sc.mixed_homes():
        ws = []
        _check_decode(imgs, thr, mode, _raw_decode(imgs, thr, mode, ws_out=ws), "mixed_homes " + mode)
        off = np.cumsum([0] + [len(d["predict_logits"]) for d in imgs])
        seen = 0
        for i, d in enumerate(imgs):
            rows = ws[0][off[i]:off[i + 1]]
            if d["predict_logits"].size > sc.LDS_CELLS:
                assert not (rows == fill).any(), "image %d: workspace rows %d..%d were not all written" % (i, off[i], off[i + 1])
                assert ((rows >= -1) & (rows <= 1)).all()
                seen += off[i] > 0
            else:
                assert (rows == fill).all(), "image %d lives in LDS, yet its workspace rows were written" % i
        assert seen >= 1


# ---- test pairs ---------------------------------------------------------------------------------------------------------------

def _props(imgs):
    props = []
    for d in imgs:
        b = BoxList(_dev(d["boxes"]).reshape(-1, 4), d["image_size"], "xyxy")
        b.add_field("pred_scores", _dev(d["pred_scores"]))
        props.append(b)
    return props


def _wrapper_pairs(imgs, cap, overlap):
    from veto_amd.pairs import prepare_test_pairs
    return [p.cpu().numpy() for p in prepare_test_pairs(DEV, _props(imgs), cap, require_overlap=overlap, use_gt_box=False)]


def _raw_pairs(imgs, cap, overlap):
    """veto_prepare_test_pairs through the raw ABI: guard cells behind pairs and counts, and every image's rows past its count
    (up to the rows reserved for it) untouched.  Returns ([pairs of image i], counts)."""
    from veto_amd.pairs import pair_capacity
    n_objs = [len(d["boxes"]) for d in imgs]
    room = [pair_capacity(n, cap) for n in n_objs]
    call = native.Launch(DEV, "needs a HIP device")
    off = native.device_offsets(n_objs, room, device=torch.device(DEV))
    pairs = _guarded(sum(room), torch.int64, (2,))
    counts = _guarded(len(imgs), torch.int32)
    a = call.args(native.VetoPairArgs, n_img=len(imgs), n_obj=sum(n_objs), max_obj_per_image=max(n_objs), max_pairs=cap,
                  require_overlap=int(overlap), boxes=_dev(np.concatenate([d["boxes"] for d in imgs])),
                  scores=_dev(np.concatenate([d["pred_scores"] for d in imgs])), img_obj_offset=off[0], img_out_offset=off[1],
                  pairs=pairs, counts=counts)
    call.run("veto_prepare_test_pairs", ctypes.byref(a))
    torch.cuda.synchronize()
    rows = _intact(pairs, sum(room), "pairs")
    cnt = _intact(counts, len(imgs), "counts")
    out, start = [], 0
    for r, k in zip(room, cnt):
        assert 1 <= k <= r
        assert (rows[start + k:start + r] == SENTINEL).all(), "rows past an image's count were written"
        out.append(rows[start:start + k])
        start += r
    return out, cnt


def _check_pairs(imgs, cap, overlap, what):
    want = [np_pairs(d["boxes"], d["pred_scores"], cap, overlap) for d in imgs]
    raw, cnt = _raw_pairs(imgs, cap, overlap)
    np.testing.assert_array_equal(cnt, [len(w) for w in want], err_msg=what)
    for i, (w, r, p) in enumerate(zip(want, raw, _wrapper_pairs(imgs, cap, overlap))):
        np.testing.assert_array_equal(r, w, err_msg="%s image %d (raw ABI)" % (what, i))     # rows and order
        np.testing.assert_array_equal(p, w, err_msg="%s image %d (wrapper)" % (what, i))
    return raw


@pytest.mark.parametrize("name", sc.PAIR_CASE_NAMES)
def test_pairs_match_the_restatement(name):
    for k, (imgs, cap, overlap) in enumerate(sc.pair_case(name)):
        _check_pairs(imgs, cap, overlap, "%s instance %d cap %d filter %d" % (name, k, cap, overlap))


def test_word_edge_images_equal_themselves_alone():
    for imgs, cap, overlap in sc.word_edges():
        batch, cnt = _raw_pairs(imgs, cap, overlap)
        for i, d in enumerate(imgs):
            alone, c1 = _raw_pairs([d], cap, overlap)
            np.testing.assert_array_equal(alone[0], batch[i], err_msg="image %d filter %d" % (i, overlap))
            assert c1[0] == cnt[i]


@pytest.mark.parametrize("name", sc.GOLDEN_PAIRS)
def test_pairs_match_the_reference_on_the_cases(name):
    g = load_golden("pairs_cases")
    case = sc.pair_case(name)
    for k in sc.golden_pair_instances(name):
        imgs, cap, overlap = case[k]
        counts = g["%s__%d__counts" % (name, k)]
        ref = np.split(g["%s__%d__pairs" % (name, k)].astype(np.int64), np.cumsum(counts)[:-1])
        got, cnt = _raw_pairs(imgs, cap, overlap)
        np.testing.assert_array_equal(cnt, counts)
        for d, r, p in zip(imgs, ref, got):
            if not sc.pairs_trace(d["boxes"], d["pred_scores"], cap, overlap)["capped"]:
                np.testing.assert_array_equal(p, r)
            else:                                                         # the reference's sort is unstable
                q_ref, q = pair_qualities(r, d["pred_scores"]), pair_qualities(p, d["pred_scores"])
                np.testing.assert_array_equal(q, q_ref)
                t = q_ref[-1]
                assert set(map(tuple, r[q_ref > t])) == set(map(tuple, p[q > t]))
