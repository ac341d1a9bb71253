"""Premises of tests/test_post_batch_gpu.py, asserted on the CPU: the batches of tests/post_batch_cases.py have the stated row and
kept counts, the vote images' arg-maxes do not hang on rounding, the tie images are decided by the tie-break alone, and the row
layout that include/veto_amd.h states for veto_postprocess_groups_batch -- restated on the oracle's rows -- gives the oracle's
one-image result for every image, while wrong restatements of it change an expected row."""
import numpy as np
import pytest

import post_batch_cases as bc
import post_eval_cases as pc


def test_batches_have_the_stated_row_counts():
    rows = lambda b: [bc.n_groups(b) * p for p in bc.inputs(b)["n_pairs"]]
    assert rows("meet_vg") == [6300, 10240, 5, 10, 450] and bc.inputs("meet_vg")["n_objs"] == [36, 64, 1, 2, 10]
    assert rows("meet_vg_reversed") == rows("meet_vg")[::-1]
    assert np.array_equal(bc.inputs("meet_vg")["pairs"][2], [[0, 0]])               # the placeholder of an image without a pair
    assert rows("meet_gqa_limit") == [pc.MAX_ROWS, 24] and bc.inputs("meet_gqa_limit")["n_objs"] == [65, 3]
    assert rows("meet_gqa_pow2") == [8192, 8196]                                    # n2 = 8192 and 16384
    assert rows("meet_gqa_over") == [pc.MAX_ROWS + 4] and bc.inputs("meet_gqa_over")["n_pairs"] == [4097]
    assert rows("vote_C") == [6300, 10240, 10] and rows("vote_U") == [6300, 6300, 6300, 5]
    for b in bc.BATCH_NAMES:
        x = bc.inputs(b)
        assert all(p.max() < n for p, n in zip(x["pairs"], x["n_objs"]))
        assert all(v.shape[0] == sum(x["n_pairs"]) and v.dtype == np.float32 for v in x["rel"].values())
        assert max(rows(b)) <= pc.MAX_ROWS and len(x["incre"]) <= 256
        # the group widths are what the kernels hold, and the head of group k is its class count + 2 wide
        K = bc.n_groups(b)
        key = (lambda k: "group_%d1" % k) if bc.voting(b) else (lambda k: "group_%d" % k)
        assert all(x["rel"][key(k)].shape[1] == x["incre"].count(k + 1) + 2 <= 105 for k in range(K))


@pytest.mark.parametrize("batch", bc.BATCH_NAMES)
def test_at_least_two_images_of_every_batch_have_object_scores_that_differ(batch):
    """... so that reading the object scores without the image's offset changes a triple score."""
    scores = [r["pred_scores"] for r in bc.expected(batch)]
    soft = [i for i, s in enumerate(scores) if not (s == 1.0).all()]
    assert len(soft) >= 2
    assert any(len(scores[i]) != len(scores[j]) or not np.array_equal(scores[i], scores[j]) for i in soft for j in soft if i < j)


def test_vote_batches_keep_nothing_everything_and_in_between_with_clear_arg_maxes():
    for batch in ("vote_C", "vote_U"):
        for im in bc.images(batch):
            assert pc.expert_top_two_gaps(im).min() >= pc.ARGMAX_GAP
    kept = [len(r["triple_scores"]) for r in bc.expected("vote_U")]
    assert 0 < kept[0] < 6300 and kept[1] == 0 and kept[2] == 6300 and 0 <= kept[3] <= 5, kept
    kept = [len(r["triple_scores"]) for r in bc.expected("vote_C")]
    assert 0 < kept[0] < 6300 and 0 < kept[1] < 10240 and 0 < kept[2] <= 10, kept


def test_tie_images_are_decided_by_the_tie_break_alone():
    for batch in bc.BATCH_NAMES:
        for (name, exact), ref in zip(bc.BATCHES[batch], bc.expected(batch)):
            if exact:
                n, gap = pc.distinct_score_gaps(ref["triple_scores"])
                assert len(ref["triple_scores"]) == 32 * n and gap >= pc.TIE_GAP, (name, n, gap)
    assert sum(bc.exact("meet_vg")) == 1 and sum(bc.exact("vote_C")) == 1


@pytest.mark.parametrize("batch", bc.BATCH_NAMES)
def test_the_stated_row_layout_gives_the_oracles_one_image_result(batch):
    for i, ref in enumerate(bc.expected(batch)):
        pairs, triple, _ = bc.sorted_rows(batch, i)
        assert pairs.tobytes() == ref["rel_pair_idxs"].tobytes() and triple.tobytes() == ref["triple_scores"].tobytes(), (batch, i)


def _changed(batch, wrong):
    """Images of the batch of which the wrong restatement changes an expected row (pair or score at some position)."""
    out = []
    for i in range(len(bc.BATCHES[batch])):
        good, bad = bc.sorted_rows(batch, i), bc.sorted_rows(batch, i, wrong)
        if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
            out.append(i)
    return out


def test_reading_object_scores_without_the_image_offset_changes_rows():
    for batch in bc.BATCH_NAMES:
        changed = _changed(batch, "obj_offset_0")
        assert 0 not in changed and changed, batch                      # image 0 sits at offset 0; every batch has an image that moves


def test_pair_major_order_before_the_sort_changes_rows():
    """Row p * K + k instead of k * P_i + p, the gather still taking row % P_i: every image with more than one pair and a kept
    row gets wrong pairs.  (The tie images' ties lie inside one group -- row i of a head is rows[i % 64] --, where both orders
    agree, so it is the pair look-up that shows this error, not the order.)"""
    for batch in bc.BATCH_NAMES:
        x = bc.inputs(batch)
        rows = [len(r["triple_scores"]) for r in bc.expected(batch)]
        assert _changed(batch, "pair_major") == [i for i, P in enumerate(x["n_pairs"]) if P > 1 and rows[i]], batch
        assert _changed(batch, "pair_major"), batch


def test_gathering_with_the_first_images_pair_count_changes_rows():
    """row % P_0 for every image: every image behind the first with another pair count and a kept row gets wrong pairs.  In
    vote_U the three large images have 1 260 pairs each and the placeholder image keeps nothing: that batch cannot show it."""
    shown = []
    for batch in bc.BATCH_NAMES:
        x = bc.inputs(batch)
        rows = [len(r["triple_scores"]) for r in bc.expected(batch)]
        changed = _changed(batch, "gather_mod_p0")
        assert changed == [i for i, P in enumerate(x["n_pairs"]) if P != x["n_pairs"][0] and rows[i]], batch
        shown += [batch] * bool(changed)
    assert shown == [b for b in bc.BATCH_NAMES if b != "vote_U"]


def test_a_batch_wide_merged_index_is_the_same_tie_break():
    """The fourth restatement, the batch-wide merged index k * n_pair + img_pair_offset[i] + p in place of the image-local
    k * P_i + p, cannot change a row: inside one image both indices order the rows by (group, pair), and the sort is per image.
    Asserted as what it is -- an equivalent statement, here on every image of every batch, the 32-fold ties included --: no
    input can tell the two apart, so no batch is asked to."""
    for batch in bc.BATCH_NAMES:
        assert _changed(batch, "batch_index") == [], batch


def test_the_abi_refuses_before_it_touches_a_device():
    """The argument checks of veto_postprocess_groups_batch need no GPU: struct size, voting, and the image beyond the sort limit,
    named by its index, from host arrays alone."""
    import ctypes
    from veto_amd import native
    lib = native.load_library()
    a = native.VetoPostGroupsBatchArgs()
    call = lambda: lib.veto_postprocess_groups_batch(None, ctypes.byref(a), ctypes.c_void_p(256), 0)
    assert call() == -1 and b"size mismatch" in lib.veto_last_error()
    a.struct_size = ctypes.sizeof(native.VetoPostGroupsBatchArgs)
    x = bc.inputs("meet_gqa_over")
    counts = [6, 4097, 2]
    a.n_img, a.n_obj, a.n_pair, a.n_groups, a.experts_per_group = 3, 70, sum(counts), 4, 3
    a.n_rel_cls, a.n_obj_cls, a.voting, a.max_pairs_per_image = len(x["incre"]), 201, 2, max(counts)
    assert call() == -1 and b"voting" in lib.veto_last_error()
    a.experts_per_group, a.voting = 1, 0
    host = ((ctypes.c_void_p * 4)(8, 8, 8, 8), (ctypes.c_int32 * 4)(*[g + 2 for g in bc.GQA_MEET_GROUPS]),
            (ctypes.c_int32 * len(x["incre"]))(*x["incre"]), (ctypes.c_int32 * 3)(*counts))
    a.head_logits, a.group_widths, a.incre_idx_list, a.pairs_per_image = [ctypes.cast(h, ctypes.c_void_p) for h in host]
    for f in ("rel_pairs", "img_obj_offset", "img_pair_offset", "obj_scores", "obj_pred", "rel_prob_sorted", "rel_pairs_sorted",
              "rel_labels_sorted"):
        setattr(a, f, 8)                    # never dereferenced: the call is refused first
    assert call() == -1 and b"image 1: n_groups * pairs = 16388 exceeds 16384" in lib.veto_last_error(), lib.veto_last_error()
    counts[1] = 4096                        # at the limit the sizes pass, and the empty workspace is what is refused
    host[3][1], a.n_pair, a.max_pairs_per_image = 4096, sum(counts), 4096
    assert call() == -4 and b"workspace too small" in lib.veto_last_error()


@pytest.mark.parametrize("vote", [False, True])
def test_the_one_image_entry_points_refuse_before_they_touch_a_device(vote):
    """veto_postprocess_meet / veto_postprocess_vote are the batch call with n_img = 1 and share its checks: a wrong struct size,
    voting = 2, a null head, a group width that is not its class count + 2, n_groups * n_pair = 16 388 and n_rel_cls = 257 each
    return -1 with their message, from host arrays alone (4 GQA groups, 101 classes; device pointers that are never read)."""
    import ctypes
    from veto_amd import native
    lib = native.load_library()
    incre, K, per = bc.inputs("meet_gqa_over")["incre"], len(bc.GQA_MEET_GROUPS), 3 if vote else 1
    struct = native.VetoPostVoteArgs if vote else native.VetoPostMeetArgs
    entry = lib.veto_postprocess_vote if vote else lib.veto_postprocess_meet

    def call(heads=None, widths=None, workspace=True, **fields):
        heads = [8] * (per * K) if heads is None else heads
        host = ((ctypes.c_void_p * len(heads))(*heads), (ctypes.c_int32 * K)(*(widths or [g + 2 for g in bc.GQA_MEET_GROUPS])),
                (ctypes.c_int32 * len(incre))(*incre))
        a = struct()
        a.struct_size = ctypes.sizeof(struct)
        a.n_obj, a.n_pair, a.n_groups, a.n_rel_cls, a.n_obj_cls = 3, 6, K, len(incre), 201
        setattr(a, "expert_logits" if vote else "group_logits", ctypes.cast(host[0], ctypes.c_void_p))
        a.group_widths, a.incre_idx_list = ctypes.cast(host[1], ctypes.c_void_p), ctypes.cast(host[2], ctypes.c_void_p)
        for f in ("rel_pairs", "obj_scores", "obj_pred", "rel_prob_sorted", "rel_pairs_sorted", "rel_labels_sorted") + ("kept_count",) * vote:
            setattr(a, f, 8)                    # never dereferenced: the call is refused first
        for f, v in fields.items():
            setattr(a, f, v)
        ws = lib.veto_postprocess_workspace_bytes(K * a.n_pair, min(a.n_rel_cls, 256))
        return entry(None, ctypes.byref(a), ctypes.c_void_p(256), ws if workspace else 0), lib.veto_last_error()

    cases = [(dict(struct_size=ctypes.sizeof(struct) - 8), b"size mismatch"),
             (dict(heads=[8, None] + [8] * (per * K - 2)), b"group %d head %d: null logits" % ((0, 2) if vote else (1, 1))),
             (dict(widths=[7, 12, 23, 67]), b"group 2: 20 classes but head width 23"),
             (dict(n_pair=4097), b"n_groups * n_pair = 16388 exceeds 16384"),
             (dict(n_rel_cls=257), b"n_rel_cls 2..256")]
    if vote:
        cases.append((dict(voting=2), b"voting must be 0 ('C') or 1 ('U')"))
    for change, needle in cases:
        rc, msg = call(**change)
        assert rc == -1 and needle in msg, (change, rc, msg)
    rc, msg = call(n_pair=4096, workspace=False)      # at the limit the sizes pass, and the empty workspace is what is refused
    assert rc == -4 and b"workspace too small" in msg, msg
