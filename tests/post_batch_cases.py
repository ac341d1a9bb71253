"""TEST INFRASTRUCTURE: batches of images for the MEET merge and the expert vote of a whole batch
(veto_postprocess_groups_batch), shared by tests/test_post_batch_host.py (premises, CPU) and tests/test_post_batch_gpu.py.

A batch is a list of single-image cases in the form of post_eval_cases.meet_case / vote_case ({'rel', 'obj', 'pairs', 'incre',
'n'[, 'voting']}), composed from those cases plus small images made here.  `inputs(batch)` gives what one PostProcessor call takes:
the batch-wide head logits (row p of every head = pair p of the concatenated pair list), the per-image refine logits and pair lists.
The expectation of image i is the oracle's one-image result on image i (oracle/veto_oracle.py); `sorted_rows` restates the row
layout of include/veto_amd.h on top of it, with one knob per wrong restatement that tests/test_post_batch_host.py tries."""
import functools

import numpy as np

import post_eval_cases as pc
from conftest import GQA_MEET_GROUPS, VG_MEET_GROUPS
from oracle import veto_oracle as vo
from veto_amd import synth

# seeds of the small images, chosen on the CPU so that the premises test_post_batch_host.py asserts hold
SEED_SMALL = 510


def small_meet(seed, n, groups, n_objc, P=None):
    """An image of n objects with random (not one-hot) refine logits and its first P pairs (all of them by default)."""
    pairs = vo.enumerate_test_pairs(n)
    P = len(pairs) if P is None else P
    assert P <= len(pairs)
    rel = {"group_%d" % k: synth.normal(seed, "batch.group_%d" % k, (P, g + 2), 0.0, 2.0) for k, g in enumerate(groups)}
    return {"rel": rel, "obj": synth.normal(seed, "batch.obj_logits", (n, n_objc), 0.0, 3.0), "pairs": pairs[:P],
            "incre": vo.meet_incre_idx_list(groups), "n": n}


def small_vote(seed, n, voting, groups=VG_MEET_GROUPS, n_objc=151):
    """As post_eval_cases.vote_case's random images: three experts that share a part, so that they often agree."""
    pairs = vo.enumerate_test_pairs(n)
    P = len(pairs)
    rel = {}
    for k, g in enumerate(groups):
        base = synth.normal(seed, "batch.vote.base_%d" % k, (P, g + 2), 0.0, 1.5)
        for e in range(3):
            own = synth.normal(seed, "batch.vote.group_%d%d" % (k, e + 1), (P, g + 2), 0.0, 1.0)
            rel["group_%d%d" % (k, e + 1)] = (base + own).astype(np.float32)
    return {"rel": rel, "obj": synth.normal(seed, "batch.vote.obj_logits", (n, n_objc), 0.0, 3.0), "pairs": pairs,
            "incre": vo.meet_incre_idx_list(groups), "n": n, "voting": voting}


# name -> [(image name, exact order expected)]; the image names are resolved by image()
BATCHES = {
    # 6 300 + 10 240 (320 scores shared by 32 rows each) + 5 (the [[0, 0]] placeholder) + 10 + 450 rows, K = 5
    "meet_vg": [("meet:vg36", False), ("meet:capped_ties", True), ("small_vg:1", False), ("small_vg:2", False), ("small_vg:10", False)],
    # 4 096 pairs x 4 groups = the 16 384-row limit of one image, beside a 3-object image
    "meet_gqa_limit": [("meet:gqa_limit", False), ("small_gqa:3", False)],
    # 8 192 and 8 196 rows: both sides of the sort's power-of-two padding
    "meet_gqa_pow2": [("sized_gqa:2048", False), ("sized_gqa:2049", False)],
    "vote_C": [("vote:vg36_C", False), ("vote:capped_ties_C", True), ("small_vote_C:2", False)],
    # kept counts: in between, 0, all, and the placeholder image.  The three 36-object cases share their refine logits, so all_U
    # gets refine logits of its own here (its three identical experts keep every row whatever the object scores)
    "vote_U": [("vote:vg36_U", False), ("vote:none_U", False), ("vote_own_obj:all_U", False), ("small_vote_U:1", False)],
}
BATCHES["meet_vg_reversed"] = BATCHES["meet_vg"][::-1]
REVERSED = {"meet_vg_reversed": "meet_vg"}
REFUSED = {"meet_gqa_over": [("meet:gqa_over", False)]}       # one image of 4 097 pairs: 16 388 rows
BATCH_NAMES = sorted(BATCHES)


@functools.lru_cache(maxsize=None)
def image(name):
    kind, arg = name.split(":")
    if kind == "meet":
        return pc.meet_case(arg)
    if kind == "vote":
        return pc.vote_case(arg)
    if kind == "vote_own_obj":
        c = pc.vote_case(arg)
        return dict(c, obj=synth.normal(SEED_SMALL + 70, "batch.vote.own_obj_logits", c["obj"].shape, 0.0, 3.0))
    if kind == "small_vg":
        return small_meet(SEED_SMALL + int(arg), int(arg), VG_MEET_GROUPS, 151)
    if kind == "small_gqa":
        return small_meet(SEED_SMALL + int(arg), int(arg), GQA_MEET_GROUPS, 201)
    if kind == "sized_gqa":      # 65 objects (4 160 candidate pairs), the first `arg` pairs
        return small_meet(SEED_SMALL + int(arg), 65, GQA_MEET_GROUPS, 201, P=int(arg))
    if kind in ("small_vote_C", "small_vote_U"):
        return small_vote(SEED_SMALL + 50 + int(arg), int(arg), kind[-1])
    raise KeyError(name)


def images(batch):
    return [image(n) for n, _ in {**BATCHES, **REFUSED}[batch]]


def exact(batch):
    return [e for _, e in BATCHES[batch]]


def voting(batch):
    return images(batch)[0].get("voting")


@functools.lru_cache(maxsize=None)
def inputs(batch):
    """{'rel': {key: [sum P, g + 2]}, 'obj': [per-image arrays], 'pairs': [per-image arrays], 'incre', 'n_objs', 'n_pairs'}"""
    ims = images(batch)
    assert all(im["incre"] == ims[0]["incre"] and im.get("voting") == ims[0].get("voting") for im in ims)
    return {"rel": {k: np.concatenate([im["rel"][k] for im in ims]) for k in ims[0]["rel"]},
            "obj": [im["obj"] for im in ims], "pairs": [im["pairs"] for im in ims], "incre": ims[0]["incre"],
            "n_objs": [im["n"] for im in ims], "n_pairs": [len(im["pairs"]) for im in ims]}


def image_slices(batch, i):
    """Image i of the batch cut out of the batch's inputs: what the one-image call is given."""
    x = inputs(batch)
    p0 = int(sum(x["n_pairs"][:i]))
    return {"rel": {k: v[p0:p0 + x["n_pairs"][i]] for k, v in x["rel"].items()}, "obj": x["obj"][i], "pairs": x["pairs"][i]}


def n_groups(batch):
    ims = images(batch)
    return len(ims[0]["rel"]) // (3 if "voting" in ims[0] else 1)


def _oracle(im, obj=None):
    obj = im["obj"] if obj is None else obj
    if "voting" in im:
        out = vo.postprocess_vote(im["rel"], obj, im["pairs"], im["incre"], len(im["incre"]), voting=im["voting"])
    else:
        out = vo.postprocess_meet(im["rel"], obj, im["pairs"], im["incre"], len(im["incre"]))
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's one-image result of image `name` (the references of post_eval_cases for its cases: one computation)."""
    kind, arg = name.split(":")
    if kind == "meet":
        return pc.meet_reference(arg)
    if kind == "vote":
        return pc.vote_reference(arg)
    return _oracle(image(name))


def expected(batch):
    return [reference(n) for n, _ in BATCHES[batch]]


# ---- the row layout of include/veto_amd.h, restated on the oracle's rows -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def sorted_rows(batch, i, wrong=None):
    """(rel_pair_idxs, triple_scores, source rows) of image i of the batch under the header's layout: the image's (kept) rows with
    their oracle scores, sorted by (score descending, image-local merged index k * P_i + p ascending), each row's pair looked up as
    pairs[img_pair_offset[i] + source % P_i] of the concatenated pair list, the object scores read at img_obj_offset[i] + index.
    wrong: None, or one of the four wrong restatements
      'obj_offset_0'   the object scores are read at index alone, in the batch-wide score list
      'batch_index'    the tie-break is the batch-wide merged index k * n_pair + img_pair_offset[i] + p
      'pair_major'     the order before the sort is (pair, group): row p * K + k, which is the tie-break and what the gather
                       (row % P_i, as stated) takes the pair from
      'gather_mod_p0'  the gather takes source % P_0 for every image"""
    x, ims = inputs(batch), images(batch)
    im, K = ims[i], n_groups(batch)
    P, P0, off = x["n_pairs"][i], x["n_pairs"][0], int(sum(x["n_pairs"][:i]))
    n_pair = int(sum(x["n_pairs"]))
    if wrong == "obj_offset_0":
        ref = _oracle(im, obj=np.concatenate(x["obj"]))   # index j of image i reads entry j of the batch-wide score list
    else:
        ref = reference(BATCHES[batch][i][0])
    src = pc.source_rows(ref["rel_pair_idxs"], ref["pred_rel_scores"], im["pairs"], im["incre"])
    k, p = src // P, src % P
    row = p * K + k if wrong == "pair_major" else src          # the row's place in the image's block before the sort
    tie = k * n_pair + off + p if wrong == "batch_index" else row
    order = np.lexsort((tie, -ref["triple_scores"].astype(np.float64)))
    src, row = src[order], row[order]
    all_pairs = np.concatenate(x["pairs"])
    pair_row = off + row % (P0 if wrong == "gather_mod_p0" else P)
    return all_pairs[pair_row % n_pair].astype(np.float32), ref["triple_scores"][order], src


# ---- sgdet: detected boxes, both branches ----------------------------------------------------------------------------------------
SGDET_N = (1, 5, 20)
SGDET_THR = 0.5


@functools.lru_cache(maxsize=None)
def sgdet_batch(expert):
    """Three images of 1, 5 and 20 detections (veto_amd.synth.synthetic_detections, with boxes_per_cls) and MEET VG heads over
    their GT-style pair lists: {'dets': [...], 'rel': {key: [sum P, g + 2]}, 'pairs': [...], 'incre', 'n_pairs'}"""
    dets = [synth.synthetic_detections(SEED_SMALL + 80 + n, n, 151) for n in SGDET_N]
    pairs = [vo.enumerate_test_pairs(n) for n in SGDET_N]
    total = sum(len(p) for p in pairs)
    rel = {}
    for k, g in enumerate(VG_MEET_GROUPS):
        for e in range(3 if expert else 1):
            key = "group_%d%d" % (k, e + 1) if expert else "group_%d" % k
            base = synth.normal(SEED_SMALL + 90, "batch.sgdet.base_%d" % k, (total, g + 2), 0.0, 1.5)
            rel[key] = (base + synth.normal(SEED_SMALL + 90, "batch.sgdet." + key, (total, g + 2), 0.0, 1.0)).astype(np.float32)
    return {"dets": dets, "rel": rel, "pairs": pairs, "incre": vo.meet_incre_idx_list(VG_MEET_GROUPS),
            "n_pairs": [len(p) for p in pairs]}
