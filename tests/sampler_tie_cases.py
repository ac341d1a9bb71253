"""Hash ties at the quota cut of the four device samplers (box_subsample_kernel, rpn_sample_kernel, gtbox_relsample_kernel,
detect_relsample_kernel): the constructions.  No test lives here.

Every sampler keeps the K members of a class with the smallest (hash, element index), hash = the upper 32 bits of
rng64(seed, image, purpose, element).  The hash never depends on the labels, so a seed whose stream holds two elements with one
hash can be searched for on the CPU (find_collisions), and the population (which elements belong to the class) can then be
chosen so that the cut falls before, inside or behind that pair (population_for).  The seeds the cases use are constants of this
module; the function that found them stays, so that tests/test_sampler_ties_host.py can re-derive some of them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_boxsample_host import PICK_NEG, PICK_POS, np_box_subsample, np_quota  # noqa: E402,F401
from test_relsample_gtbox_host import PICK_BG, PICK_FG, np_gtbox_relsample, np_hash32, np_pick  # noqa: E402,F401

PLACEMENTS = ("split", "both", "neither")
CAND_CAP = 2048           # rpn_sample_kernel: a cut bin of at most this many members is sorted in LDS
DETECT_PICK_BG = 2        # detect_relsample_kernel's purpose of the background pick (kCapFg = 1 is its foreground cap)


# ---- the search and the construction ---------------------------------------------------------------------------------------

def find_collisions(purpose, n_elems, img, first_seed, max_seeds):
    """[(seed, e_lo, e_hi)] for the streams (seed, img, purpose), seed ascending from first_seed, in which two elements of
    [0, n_elems) share a hash (e_lo < e_hi; a stream with several pairs gives one entry per pair, in hash order)."""
    elems = np.arange(n_elems)
    found = []
    for seed in range(first_seed, first_seed + max_seeds):
        h = np_hash32(seed, img, purpose, elems)
        hs = np.sort(h)
        if not (hs[1:] == hs[:-1]).any():
            continue
        order = np.argsort(h, kind="stable")
        for at in np.nonzero(h[order][1:] == h[order][:-1])[0]:
            found.append((seed, int(order[at]), int(order[at + 1])))
    return found


def population_for(seed, img, purpose, n_elems, e_lo, e_hi, K, placement, min_members=0, cut_bin_members=None, bin_below=None,
                   allowed=None):
    """A boolean membership mask over [0, n_elems) that holds both tied elements and no third element of their hash, and
    exactly K - 1 ("split"), K - 2 ("both") or K ("neither") members with a smaller hash, so that with a quota of K the cut
    takes one of the pair, both, or neither.  min_members members in all where the elements with a larger hash allow as many.
    cut_bin_members fixes how many members share the tied key's top 8 bits (the first radix digit: the cut bin of
    rpn_sample_kernel), bin_below how many of those have a smaller hash than the pair; allowed restricts the members to a mask
    (a second class of the same image).  Which other elements are members is drawn from a generator seeded by the arguments:
    the same call gives the same mask."""
    elems = np.arange(n_elems)
    h = np_hash32(seed, img, purpose, elems)
    H = int(h[e_lo])
    assert e_lo < e_hi and int(h[e_hi]) == H, "the two elements do not share a hash"
    ok = np.ones(n_elems, bool) if allowed is None else np.asarray(allowed, bool).copy()
    assert ok[e_lo] and ok[e_hi]
    ok &= h != H                                   # neither the pair nor a third element of its hash is drawn below
    smaller = {"split": K - 1, "both": K - 2, "neither": K}[placement]
    assert smaller >= 0, "K too small for the placement"
    rng = np.random.RandomState((seed * 1000003 + img * 101 + purpose * 7 + K) % 2 ** 32)
    in_bin = (h >> 24) == (H >> 24)
    below_in, below_out = elems[ok & (h < H) & in_bin], elems[ok & (h < H) & ~in_bin]
    above_in, above_out = elems[ok & (h > H) & in_bin], elems[ok & (h > H) & ~in_bin]

    def draw(pool, k, what):
        assert 0 <= k <= len(pool), "%s: %d wanted, %d there" % (what, k, len(pool))
        return rng.choice(pool, k, replace=False) if k else pool[:0]

    if cut_bin_members is None:
        below = draw(np.concatenate([below_in, below_out]), smaller, "members with a smaller hash")
        pool = np.concatenate([above_in, above_out])
        above = draw(pool, min(max(min_members - smaller - 2, 8), len(pool)), "members with a larger hash")
    else:
        b = bin_below
        if b is None:                              # what the bin allows, half of it where it can be: "neither" then cuts inside the tied key's bin
            lo = max(0, cut_bin_members - 2 - len(above_in), smaller - len(below_out))
            hi = min(smaller, len(below_in), cut_bin_members - 2)
            assert lo <= hi, "no %d members fit the tied key's bin (%d below, %d above the pair)" % (cut_bin_members, len(below_in), len(above_in))
            b = max(lo, min(hi, (cut_bin_members - 2) // 2))
        a = cut_bin_members - 2 - b
        below = np.concatenate([draw(below_in, b, "smaller hashes in the bin"), draw(below_out, smaller - b, "smaller hashes in other bins")])
        above = np.concatenate([draw(above_in, a, "larger hashes in the bin"),
                                draw(above_out, min(max(min_members - smaller - 2 - a, 1), len(above_out)), "larger hashes in other bins")])
    mask = np.zeros(n_elems, bool)
    mask[below] = mask[above] = True
    mask[[e_lo, e_hi]] = True
    assert int(mask.sum()) > K and int((mask & (h < H)).sum()) == smaller and int((mask & (h == H)).sum()) == 2
    return mask


def cut_of(seed, img, purpose, members, K):
    """The sorted (hash, index) list of the members around the cut: (K-th entry, (K+1)-th entry), each (hash, element)."""
    h = np_hash32(seed, img, purpose, members)
    order = np.lexsort((members, h))
    return (int(h[order[K - 1]]), int(members[order[K - 1]])), (int(h[order[K]]), int(members[order[K]]))


def bin_count(seed, img, purpose, members, e):
    """How many members share the top 8 bits of element e's hash (the first digit of the radix select)."""
    h = np_hash32(seed, img, purpose, members)
    return int(((h >> 24) == (int(np_hash32(seed, img, purpose, [e])[0]) >> 24)).sum())


def labels_of(n, pos=None, neg=None, pos_label=1):
    """Labels over {pos_label, 0, -1} from the two classes' membership masks (anything in neither is ignored)."""
    labels = np.full(n, -1, np.int64)
    if neg is not None:
        labels[neg] = 0
    if pos is not None:
        assert neg is None or not (pos & neg).any()
        labels[pos] = pos_label
    return labels


# ---- the committed collisions ----------------------------------------------------------------------------------------------
# name -> (a first_seed from which the search reaches it, seed, image, purpose, e_lo, e_hi): find_collisions(purpose, n,
# image, first_seed, seed - first_seed + 1) ends with the entry's stream.  The searches themselves began at seed 1.  Layout
# names: "waves" = the two elements' owning threads lie in different waves, "wave" = in one wave but different threads,
# "thread" = both in one thread's consecutive range.

BOX_N = 6144                       # box_subsample_kernel's limit: 24 consecutive proposals per thread
BOX_PAIRS = {
    "pos_waves": (1, 400, 0, PICK_POS, 3892, 4876),
    "pos_wave": (1, 313, 0, PICK_POS, 4192, 4447),
    "pos_thread": (39900, 39991, 0, PICK_POS, 3931, 3932),        # the first of 80 000 streams (image 0, either class)
    "pos_img1": (1, 965, 1, PICK_POS, 3181, 3212),
    "neg_waves": (1, 97, 0, PICK_NEG, 4205, 4608),
    "neg_wave": (1, 616, 0, PICK_NEG, 5453, 5774),
    "neg_thread": (33800, 33843, 0, PICK_NEG, 1685, 1694),
    "neg_img2": (1, 1162, 2, PICK_NEG, 5788, 5909),
    "neg_img2_batch": (1, 1819, 2, PICK_NEG, 25, 481),
    "both_pos": (48400, 48469, 1, PICK_POS, 334, 3329),           # one stream pair (seed, image 1) with a tie in either class
    "both_neg": (48400, 48469, 1, PICK_NEG, 471, 3823),
}
BOX_LAYOUT = {"pos_waves": "waves", "pos_wave": "wave", "pos_thread": "thread", "pos_img1": "wave", "neg_waves": "waves",
              "neg_wave": "wave", "neg_thread": "thread", "neg_img2": "wave", "neg_img2_batch": "wave", "both_pos": "waves",
              "both_neg": "waves"}
# (case, pairs, placements): every pair of a case in the same image
BOX_CASES = [("%s_%s" % (p, w), (p,), (w,)) for p in ("pos_waves", "neg_waves", "pos_wave", "neg_wave", "pos_thread", "neg_thread",
                                                      "pos_img1", "neg_img2") for w in PLACEMENTS] + \
            [("both_%s_%s" % (a, b), ("both_pos", "both_neg"), (a, b)) for a, b in (("split", "split"), ("both", "neither"), ("neither", "both"))]
BOX_BATCH, BOX_FRACTION = 64, 0.25

GTBOX_PAIRS = {   # elements are cells of the row-major relation matrix; none on the diagonal
    "fg256_waves": (1, 2, 0, PICK_FG, 21434, 56976),
    "fg256_wave": (1, 11, 1, PICK_FG, 18528, 21645),
    "fg256_thread": (1, 119, 1, PICK_FG, 21855, 21897),
    "bg256_waves": (1, 5, 0, PICK_BG, 3464, 45640),
    "bg256_wave": (1, 7, 1, PICK_BG, 47022, 49013),
    "bg256_thread": (1, 59, 0, PICK_BG, 51599, 51689),
    "fg100_waves": (600, 641, 0, PICK_FG, 1279, 6814),
    "fg100_wave": (200, 249, 1, PICK_FG, 3973, 5046),
    "bg100_waves": (150, 196, 0, PICK_BG, 2360, 9065),
    "bg100_wave": (250, 283, 1, PICK_BG, 6467, 6677),
}
GTBOX_CASES = [("%s_%s" % (p, w), p, w) for p in GTBOX_PAIRS for w in PLACEMENTS]
GTBOX_BATCH, GTBOX_NUM_POS = 64, 16

RPN_BATCH, RPN_FRACTION = 256, 0.5
RPN_LDS_N, RPN_LDS_LEVELS, RPN_LDS_SEED = 100003, (75000, 18750, 4700, 1200, 353), 22
RPN_LDS_PAIRS = {   # (image, purpose) -> (e_lo, e_hi): seed 22 is the first whose eight streams all hold a pair
    (0, PICK_POS): (14053, 60905), (0, PICK_NEG): (66103, 92747), (1, PICK_POS): (32536, 63948), (1, PICK_NEG): (80239, 91541),
    (2, PICK_POS): (15045, 71576), (2, PICK_NEG): (1752, 81015), (3, PICK_POS): (24658, 49051), (3, PICK_NEG): (5113, 22942),
}
# (call, image, class, placement, cut_bin_members, bin_below): bin_need = the members of the cut bin that are taken
RPN_LDS_CASES = [
    ("neg", 0, PICK_NEG, "split", 20, 0),       # bin_need 1: the lower of the pair is the bin's best and its only one taken
    ("neg", 1, PICK_NEG, "both", 300, 0),       # bin_need 2: exactly the pair
    ("neg", 2, PICK_NEG, "neither", 300, 5),    # bin_need 5: the cut falls on the key just before the pair
    ("neg", 3, PICK_NEG, "both", 12, 10),       # bin_need 12 of 12: the pair closes a bin that is taken whole
    ("pos", 0, PICK_POS, "split", 40, 1),       # bin_need 2: one member, then the lower of the pair
    ("pos", 1, PICK_POS, "both", 30, 0),
    ("pos", 2, PICK_POS, "neither", 40, 3),
    ("pos", 3, PICK_POS, "split", 40, 0),
]
RPN_STREAM_N, RPN_STREAM_LEVELS, RPN_STREAM_SEED = 600037, (450000, 112500, 28000, 7000, 2537), 139
RPN_STREAM_BATCH = 2048            # a quota of about 2 040 negatives: only then can 2 049 members of one bin lie around the cut
RPN_STREAM_PAIRS = {   # seed 139: the first with a pair inside one 256-anchor tile in one image (3) and inside one 4-tile load group in another (1)
    (0, PICK_NEG): (412754, 581693), (1, PICK_NEG): (300735, 300817), (2, PICK_NEG): (224140, 324760), (3, PICK_NEG): (221224, 221438),
    (1, PICK_POS): (126315, 584250),
}
RPN_STREAM_LAYOUT = {0: "groups", 1: "group", 2: "groups", 3: "tile"}
# (call, image, [(class, placement, cut_bin_members, bin_below)], path)
RPN_STREAM_CASES = [
    ("a", 0, [(PICK_NEG, "split", CAND_CAP + 1, None)], "stream"),      # the path switch, streaming side: 2049 members in the cut bin
    ("a", 1, [(PICK_NEG, "both", 2200, None)], "stream"),
    ("a", 2, [(PICK_NEG, "neither", 2200, None)], "stream"),
    ("a", 3, [(PICK_NEG, "split", 2200, None)], "stream"),
    ("b", 0, [(PICK_NEG, "split", CAND_CAP + 1, None)], "lds"),         # the same image with one member of the cut bin ignored: 2048
    ("b", 1, [(PICK_POS, "split", None, None), (PICK_NEG, "split", 2200, None)], "stream"),   # both packed fields in one scan
    ("b", 2, [(PICK_NEG, "split", 2200, None)], "stream"),
    ("b", 3, [(PICK_NEG, "neither", 2200, None)], "stream"),
]


# ---- the images --------------------------------------------------------------------------------------------------------------
# An image of a label kernel (box_subsample_kernel, rpn_sample_kernel) is a dict: name, seed, img (its index in the batch), n,
# batch, fraction, labels, ties = [dict(purpose, e_lo, e_hi, placement, layout, ...)].  An image of gtbox_relsample_kernel has
# rel [n, n] and num_pos instead of labels and fraction.

def layout_of(chunk, e_lo, e_hi):
    """Where the owners of two elements lie when thread t owns the elements [t * chunk, (t + 1) * chunk)."""
    a, b = e_lo // chunk, e_hi // chunk
    return "thread" if a == b else ("wave" if a // 64 == b // 64 else "waves")


def stream_layout_of(e_lo, e_hi):
    """rpn_sample_kernel's streaming path: one scan per 256 consecutive anchors, four tiles loaded ahead of their scans."""
    return "tile" if e_lo // 256 == e_hi // 256 else ("group" if e_lo // 1024 == e_hi // 1024 else "groups")


def _few(n, count, avoid, stride=997):
    """`count` elements of [0, n) off `avoid` (a mask), spread by a stride: a class that stays under its quota."""
    out, e = [], 3
    while len(out) < count:
        if not avoid[e]:
            out.append(e)
        e = (e + stride) % n
    mask = np.zeros(n, bool)
    mask[out] = True
    return mask


def label_image(name, seed, img, n, batch, fraction, ties, min_members, neg_fill=20, pos_fill=5):
    """One image of a label kernel with a tie in one class or in both.  ties: [dict(purpose, e_lo, e_hi, placement,
    cut_bin_members, bin_below)].  A tied positive class has int(batch * fraction) as its quota; a tied negative class what the
    positives leave; a class without a tie stays under its quota (pos_fill / neg_fill members, all taken)."""
    by = {t["purpose"]: t for t in ties}
    num_pos = int(batch * fraction)
    taken = np.zeros(n, bool)
    for t in ties:
        taken[[t["e_lo"], t["e_hi"]]] = True
    if PICK_POS in by:
        t = by[PICK_POS]
        pos = population_for(seed, img, PICK_POS, n, t["e_lo"], t["e_hi"], num_pos, t["placement"], min_members[PICK_POS],
                             t.get("cut_bin_members"), t.get("bin_below"), allowed=~taken | _pair_mask(n, t))
        t["K"] = num_pos
    else:
        pos = _few(n, pos_fill, taken)
    if PICK_NEG in by:
        t = by[PICK_NEG]
        t["K"] = batch - min(int(pos.sum()), num_pos)
        neg = population_for(seed, img, PICK_NEG, n, t["e_lo"], t["e_hi"], t["K"], t["placement"], min_members[PICK_NEG],
                             t.get("cut_bin_members"), t.get("bin_below"), allowed=~pos)
    else:
        neg = _few(n, neg_fill, pos | taken, stride=1009)
    for t in ties:
        t["M"] = int((pos if t["purpose"] == PICK_POS else neg).sum())
    return dict(name=name, seed=seed, img=img, n=n, batch=batch, fraction=fraction, labels=labels_of(n, pos, neg), ties=ties)


def _pair_mask(n, t):
    m = np.zeros(n, bool)
    m[[t["e_lo"], t["e_hi"]]] = True
    return m


def label_classes(im):
    """{purpose: (members, K)} of a label image: K is None where the class does not draw (none or all of it are taken)."""
    pos, neg, num_pos, num_neg = np_quota(im["labels"], im["batch"], im["fraction"])
    return {PICK_POS: (pos, num_pos if 0 < num_pos < len(pos) else None), PICK_NEG: (neg, num_neg if 0 < num_neg < len(neg) else None)}


def label_expected(im):
    return np_box_subsample(im["labels"], im["img"], im["seed"], im["batch"], im["fraction"])


def rpn_cut_bins(im):
    """{purpose: (members of the cut bin, bin_need)} for the classes of an rpn_sample_kernel image that draw: the cut bin is
    the top-8-bit bin of the K-th smallest hash, bin_need how many of that bin the quota still takes."""
    out = {}
    for purpose, (members, K) in label_classes(im).items():
        if K is not None:
            top = np.sort(np_hash32(im["seed"], im["img"], purpose, members)) >> 24
            out[purpose] = (int((top == top[K - 1]).sum()), int(K - (top < top[K - 1]).sum()))
    return out


def rpn_path(im):
    """"lds" when every drawing class's cut bin fits the candidate sort (<= 2048 members), else "stream"."""
    return "lds" if all(count <= CAND_CAP for count, _ in rpn_cut_bins(im).values()) else "stream"


def rpn_inputs(images, levels, inputs_for_labels):
    """The arguments of one veto_rpn_loss call whose labels are the images': the anchors split into `levels`."""
    anchors, tgt = inputs_for_labels([im["labels"] for im in images])
    assert sum(levels) == len(anchors)
    return dict(anchors=np.split(anchors, np.cumsum(levels)[:-1]), tgt_boxes=tgt, image_sizes=[(64, 64)] * len(tgt),
                level_shapes=[(1, 1, k) for k in levels])


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def box_images():
    """One image per entry of BOX_CASES, in its order."""
    def make():
        out = []
        for name, pairs, placements in BOX_CASES:
            ties = []
            for p, w in zip(pairs, placements):
                _, seed, img, purpose, e_lo, e_hi = BOX_PAIRS[p]
                ties.append(dict(pair=p, purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement=w, layout=BOX_LAYOUT[p]))
            out.append(label_image(name, seed, img, BOX_N, BOX_BATCH, BOX_FRACTION, ties, {PICK_POS: 700, PICK_NEG: 3000}))
        return out
    return _cached("box", make)


def box_batch_of_four():
    """(seed, four label vectors, the same four with image 2 replaced by an image without a tie): only image 2 has a tie, and
    the rows of the other three must not depend on it."""
    _, seed, img, purpose, e_lo, e_hi = BOX_PAIRS["neg_img2_batch"]
    tied = label_image("batch_of_four", seed, img, BOX_N, BOX_BATCH, BOX_FRACTION,
                       [dict(pair="neg_img2_batch", purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement="split", layout="wave")],
                       {PICK_NEG: 3000})
    rng = np.random.RandomState(4)
    others = [rng.choice([1, 0, 0, 0, -1], size=n).astype(np.int64) for n in (1000, 6144, 333)]
    return tied, [others[0], others[1], tied["labels"], others[2]], [others[0], others[1], others[0], others[2]]


def gtbox_images():
    """One image per entry of GTBOX_CASES.  A foreground tie: the members are the foreground cells, above num_pos, and every
    other off-diagonal cell is background.  A background tie: the members are the background cells, so every off-diagonal
    cell outside them is foreground (far above num_pos: the cap draws too, and the background quota is batch - num_pos)."""
    def make():
        out = []
        for name, p, w in GTBOX_CASES:
            _, seed, img, purpose, e_lo, e_hi = GTBOX_PAIRS[p]
            n = 256 if "256" in p else 100
            cells = np.arange(n * n)
            off = cells // n != cells % n
            K = GTBOX_NUM_POS if purpose == PICK_FG else GTBOX_BATCH - GTBOX_NUM_POS
            members = population_for(seed, img, purpose, n * n, e_lo, e_hi, K, w, 500 if purpose == PICK_FG else 2000, allowed=off)
            fg = members if purpose == PICK_FG else off & ~members
            rel = np.where(fg, 1 + cells % 50, 0).astype(np.int64).reshape(n, n)
            chunk = -(-n * n // 256)
            tie = dict(pair=p, purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement=w, layout=layout_of(chunk, e_lo, e_hi), K=K,
                       M=int(members.sum()))
            out.append(dict(name=name, seed=seed, img=img, n=n, batch=GTBOX_BATCH, num_pos=GTBOX_NUM_POS, rel=rel, ties=[tie]))
        return out
    return _cached("gtbox", make)


def gtbox_classes(im):
    n = im["n"]
    flat, cells = im["rel"].reshape(-1), np.arange(n * n)
    fg, bg = cells[flat > 0], cells[(flat <= 0) & (cells // n != cells % n)]
    n_fg = min(len(fg), im["num_pos"])
    n_bg = min(len(bg), im["batch"] - n_fg)
    return {PICK_FG: (fg, n_fg if 0 < n_fg < len(fg) else None), PICK_BG: (bg, n_bg if 0 < n_bg < len(bg) else None)}


def gtbox_expected(im):
    """(pairs, labels, binary, n_fg, n_bg) of np_gtbox_relsample."""
    return np_gtbox_relsample(im["rel"], im["img"], im["seed"], im["batch"], im["num_pos"])


def rpn_lds_calls():
    """{call: four images} of RPN_LDS_CASES: about 100 000 anchors over five levels, every cut bin far below 2 048 members."""
    def make():
        calls = {}
        for call, img, purpose, w, members, below in RPN_LDS_CASES:
            e_lo, e_hi = RPN_LDS_PAIRS[(img, purpose)]
            tie = dict(purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement=w, cut_bin_members=members, bin_below=below, path="lds",
                       layout="lanes" if e_lo % 256 != e_hi % 256 else "lane")
            im = label_image("lds_%s_%d_%s" % (call, img, w), RPN_LDS_SEED, img, RPN_LDS_N, RPN_BATCH, RPN_FRACTION, [tie],
                             {PICK_POS: 3000, PICK_NEG: 60000}, neg_fill=50000, pos_fill=7)
            im["path"] = "lds"
            calls.setdefault(call, []).append(im)
        return calls
    return _cached("rpn_lds", make)


def rpn_stream_calls():
    """{call: four images} of RPN_STREAM_CASES: about 600 000 anchors, where one bin of the top 8 bits can hold more than 2 048
    members.  Image 0 of call "b" is image 0 of call "a" with one member of the cut bin (the one with the largest hash, far
    behind the cut) set to ignored: 2 048 members, the LDS path, and the same rows."""
    def make():
        calls = {}
        for call, img, tie_list, path in RPN_STREAM_CASES:
            ties = []
            for purpose, w, members, below in tie_list:
                e_lo, e_hi = RPN_STREAM_PAIRS[(img, purpose)]
                ties.append(dict(purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement=w, cut_bin_members=members, bin_below=below,
                                 layout=stream_layout_of(e_lo, e_hi)))
            im = label_image("stream_%s_%d_%s" % (call, img, "_".join(t["placement"] for t in ties)), RPN_STREAM_SEED, img,
                             RPN_STREAM_N, RPN_STREAM_BATCH, RPN_FRACTION, ties, {PICK_POS: 3000, PICK_NEG: 400000}, pos_fill=7)
            if path == "lds":
                t = ties[0]
                neg = np.nonzero(im["labels"] == 0)[0]
                h = np_hash32(im["seed"], img, PICK_NEG, neg)
                in_bin = neg[(h >> 24) == (int(np_hash32(im["seed"], img, PICK_NEG, [t["e_lo"]])[0]) >> 24)]
                flipped = in_bin[np.argmax(np_hash32(im["seed"], img, PICK_NEG, in_bin))]
                im["labels"][flipped] = -1
                im["flipped"] = int(flipped)
                t["cut_bin_members"] -= 1
                t["M"] -= 1
            im["path"] = path
            calls.setdefault(call, []).append(im)
        return calls
    return _cached("rpn_stream", make)


# ---- detect_relsample_kernel ---------------------------------------------------------------------------------------------------
# Background pick (purpose 2, element = i * P + j): with no foreground and n_bg <= 2 * batch the window is whole, so the
# population is every cell off the diagonal between proposals labelled above 0, whatever the scores.  It is shaped only by
# which proposals are labelled 0, so the rank of the tied pair cannot be constructed: the seeds below are those of 20 000
# streams per image index (64 proposals) for which zero-labelling the first z proposals outside the pair's rows and columns
# leaves the pair at a rank s with n_bg / 2 <= s and s + 2 <= min(2048, n_bg - 1); batch_size_per_image = s + 1, s + 2, s then
# gives the three placements.  With 64 proposals every row's thread is in wave 0; two of the 74 pairs found lie in one row.
# Foreground cap (purpose 1, element = the triplet's position in [0, F)): 50 GT boxes, each matched by exactly one proposal, and
# F = 2000 relations, so every relation yields one triplet and its position is its rank in nonzero(relation) order; the quota
# int(batch * fraction) is set to s + 1, s + 2, s.
DETECT_CAP_FG = 1
DETECT_P, DETECT_T, DETECT_F = 64, 50, 2000
DETECT_BG_PAIRS = {   # name -> (first_seed, seed, image, e_lo, e_hi, proposals labelled 0)
    "bg_img0": (200, 225, 0, 1119, 2479, 4),
    "bg_img1": (50, 100, 1, 1195, 1618, 17),
    "bg_img0_thread": (6300, 6345, 0, 3462, 3487, 20),       # both cells in candidate row 54: one thread
}
DETECT_CAP_PAIRS = {  # name -> (first_seed, seed, image, e_lo, e_hi)
    "cap_img0_waves": (11500, 11584, 0, 1257, 1692),
    "cap_img1_wave": (13300, 13341, 1, 1485, 1523),
}
DETECT_CASES = [(p + "_" + w, p, w) for p in list(DETECT_BG_PAIRS) + list(DETECT_CAP_PAIRS) for w in PLACEMENTS]


def _detect_bg_inputs(e_lo, e_hi, zeroed):
    P = DETECT_P
    used = {e_lo // P, e_lo % P, e_hi // P, e_hi % P}
    labels = 1 + np.arange(P, dtype=np.int64) % 5
    labels[[p for p in range(P) if p not in used][:zeroed]] = 0
    x0 = 12.0 * np.arange(P, dtype=np.float32)
    boxes = np.stack([x0, np.zeros_like(x0), x0 + 9, np.full_like(x0, 9)], 1)
    scores = (0.3 + 0.01 * np.arange(P)).astype(np.float32)
    return dict(prp_boxes=boxes, prp_labels=labels, pred_scores=scores, tgt_boxes=np.array([[700, 500, 720, 520]], np.float32),
                tgt_labels=np.array([1], np.int64), relation=np.zeros((1, 1), np.int64))


def _detect_cap_inputs():
    T = DETECT_T
    i = np.arange(T, dtype=np.float32)
    boxes = np.stack([15 * (i % 10), 15 * (i // 10), 15 * (i % 10) + 9, 15 * (i // 10) + 9], 1).astype(np.float32)
    labels = 1 + np.arange(T, dtype=np.int64) % 7
    cells = np.arange(T * T)
    off = cells[cells // T != cells % T][:DETECT_F]
    rel = np.zeros(T * T, np.int64)
    rel[off] = 1 + off % 50
    return dict(prp_boxes=boxes, prp_labels=labels, pred_scores=(0.3 + 0.01 * i).astype(np.float32), tgt_boxes=boxes.copy(),
                tgt_labels=labels.copy(), relation=rel.reshape(T, T))


def detect_parts(im):
    """np_relsample_parts of the image, and the members and quota of its two hash draws: {purpose: (members, K or None)}."""
    from test_relsample_host import np_relsample_parts
    s = np_relsample_parts(im["d"], *im["cfg"])
    assert all(len(r["cand"]) <= im["cfg"][2] for r in s["rels"])          # no weighted per-relation draw in these cases
    P = len(im["d"]["prp_boxes"])
    win = s["bg_sorted"][:s["window"]]
    flat = np.sort(win[:, 0] * P + win[:, 1]).astype(np.int64)
    fg = np.arange(s["n_pre"])
    return s, {DETECT_CAP_FG: (fg, s["n_fg"] if 0 < s["n_fg"] < len(fg) else None),
               DETECT_PICK_BG: (flat, s["num_neg"] if 0 < s["num_neg"] < len(flat) else None)}


def detect_classes(im):
    return detect_parts(im)[1]


def detect_expected(im):
    """Rows [n, 3] (subject, object, label) of detect_relsample_kernel: the capped foreground in (hash, position) order, then the
    background in (hash, cell) order."""
    s, cls = detect_parts(im)
    P = len(im["d"]["prp_boxes"])
    trip = np.array([(a, b, r["label"]) for r in s["rels"] for a, b in r["cand"]], np.int64).reshape(-1, 3)
    fg, K = cls[DETECT_CAP_FG]
    if K is not None:
        trip = trip[np_pick(im["seed"], im["img"], DETECT_CAP_FG, fg, K)]
    flat, _ = cls[DETECT_PICK_BG]
    bg = np_pick(im["seed"], im["img"], DETECT_PICK_BG, flat, s["num_neg"])
    rows = np.concatenate([trip, np.stack([bg // P, bg % P, np.zeros_like(bg)], 1)], 0)
    return rows if len(rows) else np.zeros((2, 3), np.int64)


def detect_images():
    """One image per entry of DETECT_CASES: d (the inputs), cfg (fg_thres, require_overlap, per_rel, batch, fraction)."""
    def make():
        out = []
        for name, p, w in DETECT_CASES:
            if p in DETECT_BG_PAIRS:
                _, seed, img, e_lo, e_hi, zeroed = DETECT_BG_PAIRS[p]
                purpose, d = DETECT_PICK_BG, _detect_bg_inputs(e_lo, e_hi, zeroed)
                labelled = d["prp_labels"] > 0
                cells = np.arange(DETECT_P ** 2)
                members = cells[labelled[cells // DETECT_P] & labelled[cells % DETECT_P] & (cells // DETECT_P != cells % DETECT_P)]
                layout = layout_of(DETECT_P, e_lo, e_hi)                       # thread i owns candidate row i
            else:
                _, seed, img, e_lo, e_hi = DETECT_CAP_PAIRS[p]
                purpose, d, members = DETECT_CAP_FG, _detect_cap_inputs(), np.arange(DETECT_F)
                layout = layout_of(-(-DETECT_F // 256), e_lo, e_hi)
            h = np_hash32(seed, img, purpose, members)
            smaller = int((h < int(np_hash32(seed, img, purpose, [e_lo])[0])).sum())
            K = smaller + {"split": 1, "both": 2, "neither": 0}[w]
            cfg = (0.5, False, 4, K, 0.25) if purpose == DETECT_PICK_BG else (0.5, False, 4, 2048, (K + 0.5) / 2048)
            tie = dict(pair=p, purpose=purpose, e_lo=e_lo, e_hi=e_hi, placement=w, layout=layout, K=K, M=len(members))
            out.append(dict(name=name, seed=seed, img=img, n=len(d["prp_boxes"]), d=d, cfg=cfg, ties=[tie]))
        return out
    return _cached("detect", make)


# ---- radix_select's bin boundaries at the first pass (no tie: the population alone places the cut) ------------------------------
# The kernels select on ~hash, so their digit 255 is the hashes' top byte 0 and their digit 0 the top byte 255.

BOUNDARY_KINDS = ("last_of_bin", "first_of_bin", "digit_255", "digit_0")
BOUNDARY_BATCH, BOUNDARY_FRACTION = 2048, 2040.5 / 2048     # a positive quota of 2040: with p <= 2040 positives the negatives' is 2048 - p


def boundary_members(seed, img, n, kind, low, count, bin_index, allowed=None, whole_next_bin=False):
    """(negative members, K) with the cut (the K-th smallest hash) at a boundary of the first radix digit: `low` members in the
    top-byte bins <= bin_index and count - low in the bins above.
    last_of_bin: K = low, the cut is the last member of bin bin_index or below (need == that bin's count);
    first_of_bin: K = low + 1, the first member of the next bin (need == 1; whole_next_bin puts every allowed element of that bin in);
    digit_255: K = low, far below count / 256, the cut inside the hashes' lowest bin (bin_index 0, low below that bin's count);
    digit_0: K = count - 1 with the last two members in the hashes' highest bin (bin_index 254), or all of them (bin_index -1)."""
    elems = np.arange(n)
    ok = np.ones(n, bool) if allowed is None else allowed
    top = np_hash32(seed, img, PICK_NEG, elems) >> 24
    rng = np.random.RandomState(seed + 17 * img)
    lower, upper = elems[ok & (top <= bin_index)], elems[ok & (top > bin_index)]
    if kind == "digit_0":
        upper = elems[ok & (top == 255)]
    if kind == "digit_255":
        lower, upper = elems[ok], elems[:0]
        low = count
    assert low <= len(lower) and count - low <= len(upper), (kind, low, len(lower), count - low, len(upper))
    members = np.concatenate([rng.choice(lower, low, replace=False), rng.choice(upper, count - low, replace=False)])
    if whole_next_bin:
        members = np.union1d(members, elems[ok & (top == bin_index + 1)])
    members = np.sort(members)
    K = {"last_of_bin": low, "first_of_bin": low + 1, "digit_255": 8, "digit_0": len(members) - 1}[kind]
    return members, K


def _boundary_image(prefix, seed, img, n, kind, members, K, pos=None):
    neg = np.zeros(n, bool)
    neg[members] = True
    if pos is None:                       # under their quota: all taken, and the negatives' quota is what they leave
        pos = np.zeros(n, bool)
        pos[np.nonzero(~neg)[0][:BOUNDARY_BATCH - K]] = True
        assert int(pos.sum()) == BOUNDARY_BATCH - K <= int(BOUNDARY_BATCH * BOUNDARY_FRACTION)
    return dict(name=prefix + kind, kind=kind, seed=seed, img=img, n=n, batch=BOUNDARY_BATCH, fraction=BOUNDARY_FRACTION,
                labels=labels_of(n, pos, neg), ties=[], K=K)


def box_boundary_images(seed=7):
    """One batch of four images of box_subsample_kernel at 6 144 proposals.  Random populations have about 16 members per bin
    here, so `need == 1` meets a bin of tens, not of hundreds."""
    def make():
        spec = {"last_of_bin": (45, 4000, 2), "first_of_bin": (45, 4000, 2), "digit_255": (0, 4000, 0), "digit_0": (499, 501, 254)}
        out = []
        for img, kind in enumerate(BOUNDARY_KINDS):
            members, K = boundary_members(seed, img, BOX_N, kind, *spec[kind])
            out.append(_boundary_image("box_", seed, img, BOX_N, kind, members, K))
        return out
    return _cached("box_boundary", make)


def rpn_boundary_images(seed=RPN_STREAM_SEED):
    """The same four boundaries in one call of rpn_sample_kernel on the streaming path.  A class whose own cut bin exceeds 2 048
    members cannot have need == the bin's count (K <= 2 048), so for last_of_bin the positives force the path: 2 200 positives,
    all in the lowest bin of their own stream, against their quota of 2 040.  The others reach it by themselves: first_of_bin
    with the whole next bin (about 2 300) as members, digit_255 with 590 000 negatives, digit_0 with 2 049 negatives that all
    lie in the hashes' highest bin (K = 2 048)."""
    def make():
        n, out = RPN_STREAM_N, []
        elems = np.arange(n)
        for img, kind in enumerate(BOUNDARY_KINDS):
            pos = None
            if kind == "last_of_bin":
                pos = np.zeros(n, bool)
                pos[elems[(np_hash32(seed, img, PICK_POS, elems) >> 24) == 0][:2200]] = True
                members, K = boundary_members(seed, img, n, kind, BOUNDARY_BATCH - 2040, 100000, 0, allowed=~pos)
            elif kind == "first_of_bin":
                members, K = boundary_members(seed, img, n, kind, 1500, 100000, 0, whole_next_bin=True)
            elif kind == "digit_255":
                members, K = boundary_members(seed, img, n, kind, 0, 590000, 0)
            else:
                members, K = boundary_members(seed, img, n, kind, 0, 2049, -1)
            im = _boundary_image("rpn_", seed, img, n, kind, members, K, pos)
            im["path"] = "stream"
            out.append(im)
        return out
    return _cached("rpn_boundary", make)


# ---- wrong restatements ------------------------------------------------------------------------------------------------------

WRONG = ("higher_index", "all_tied", "no_tied", "need_per_thread", "room_not_reduced")


def wrong_pick(variant, owner):
    """np_pick with one of the tie mistakes the kernels could make.  owner(e) is the thread that owns element e
    (need_per_thread: every thread takes the first `need` of its own tied elements) or the 256-anchor scan tile of the streaming
    path (room_not_reduced: every tile does)."""
    def pick(seed, img, purpose, cells, k):
        h = np_hash32(seed, img, purpose, cells)
        order = np.lexsort((cells, h))
        if k <= 0 or k >= len(cells):
            return cells[order[:k]]
        T = h[order[k - 1]]
        sure = cells[order][h[order] < T]
        tied = np.sort(cells[h == T])
        need = k - len(sure)
        if variant == "higher_index":
            tied = tied[::-1][:need][::-1]
        elif variant == "no_tied":
            tied = tied[:0] if need < len(tied) else tied
        elif variant in ("need_per_thread", "room_not_reduced"):
            seen, keep = {}, []
            for e in tied:
                seen[owner(int(e))] = seen.get(owner(int(e)), 0) + 1
                if seen[owner(int(e))] <= need:
                    keep.append(e)
            tied = np.array(keep, cells.dtype)
        elif variant != "all_tied":
            raise ValueError(variant)
        return np.concatenate([sure, tied])
    return pick
