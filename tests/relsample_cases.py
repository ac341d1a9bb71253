"""What the detected-box relation sampler's host and device tests and tests/golden/make_golden_relsample_sgdet.py share at real
and limit sizes: the case table of tests/golden/sgdet/relsample_large.npz with its input builder, the front padding that moves a
small image into the last mask words and relation cells of a 256 x 256 one, the quantised scores of the tie case, the edge sweep,
and the facts about a case that the coverage test and the parity record state (loop steps, mask words in use).  No test lives
here."""
import os

import numpy as np

from veto_amd import synth

GOLDEN_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgdet", "relsample_large.npz")
MAX_OBJ = 256      # proposals and GT boxes per image: eight 32-bit mask words per row
STEP = 256         # relation matrix cells per step of the kernel's relation loop
SORT_BUFFER = 2048

# name: (image seed, n_gt, n_det, n_rel, synth options, (fg_thres, overlap, per_rel, batch, fraction), non_masked, transform)
# transform: None | ("pad", P, T): pad_front to P proposals and T GT boxes | ("quantise", levels): pred_scores on `levels` values
LARGE_CASES = {
    "real": (21, 17, 80, 30, dict(), (0.5, False, 4, 1024, 0.25), True, None),
    "word_edge": (22, 33, 65, 40, dict(), (0.5, False, 4, 64, 0.25), True, None),
    "limit": (23, 60, 256, 150, dict(), (0.5, False, 4, 1024, 0.25), True, None),
    "limit_overlap": (24, 256, 256, 600, dict(), (0.5, True, 16, 2048, 0.25), True, None),
    "over_sort_buffer": (25, 40, 256, 600, dict(max_copies=12), (0.5, False, 16, 2048, 0.25), True, None),
    "padded_deterministic": (26, 20, 40, 30, dict(max_copies=2), (0.5, False, 4, 2048, 0.25), True, ("pad", 256, 256)),
    "ties": (27, 17, 80, 30, dict(), (0.5, False, 4, 512, 0.25), True, ("quantise", 4)),
}


def pad_front(d, P, T):
    """The image `d` with label-0 proposals in front of its proposals (up to P) and unrelated GT boxes in front of its GT boxes
    (up to T): the relation matrices sit in the bottom-right corner of the [T, T] ones, every old proposal index moves up by
    P - n_det and every old GT index by T - n_gt.  The padding proposals are 3 x 3 boxes in the top-left corner and the padding GT
    boxes 3 x 3 boxes in the bottom-right one, so they overlap neither each other nor (above IoU 0.5) anything of the image; a
    label-0 proposal matches no GT box and is no candidate, so the padding changes no match, candidate or relation."""
    n_det, n_gt = len(d["prp_boxes"]), len(d["tgt_boxes"])
    kp, kt = P - n_det, T - n_gt
    assert kp >= 0 and kt >= 0, (P, T, n_det, n_gt)
    W, H = d.get("image_size", (800, 600))
    i = np.arange(kp)
    pp = np.stack([4.0 * (i % 64), 4.0 * (i // 64), 4.0 * (i % 64) + 2, 4.0 * (i // 64) + 2], 1).astype(np.float32).reshape(kp, 4)
    j = np.arange(kt)
    x1, y1 = W - 4.0 - 4.0 * (j % 64), H - 4.0 - 4.0 * (j // 64)
    pt = np.stack([x1, y1, x1 + 2, y1 + 2], 1).astype(np.float32).reshape(kt, 4)
    out = dict(d)
    out["prp_boxes"] = np.concatenate([pp, d["prp_boxes"].astype(np.float32)], 0)
    out["prp_labels"] = np.concatenate([np.zeros(kp, np.int64), d["prp_labels"].astype(np.int64)])
    out["pred_scores"] = np.concatenate([np.full(kp, 0.5, np.float32), d["pred_scores"].astype(np.float32)])
    out["tgt_boxes"] = np.concatenate([pt, d["tgt_boxes"].astype(np.float32)], 0)
    out["tgt_labels"] = np.concatenate([1 + j % 150, d["tgt_labels"]]).astype(np.int64)
    for k in ("relation", "relation_non_masked"):
        if k in d:
            m = np.zeros((T, T), np.int64)
            m[kt:, kt:] = d[k]
            out[k] = m
    return out


def quantise_scores(d, levels):
    """pred_scores rounded onto `levels` values, so that whole runs of pair qualities (score products) are equal."""
    out = dict(d)
    grid = np.linspace(0.2, 0.95, levels).astype(np.float32)
    q = d["pred_scores"].astype(np.float32)
    out["pred_scores"] = grid[np.abs(q[:, None] - grid[None, :]).argmin(1)]
    return out


def seeded_image(seed, n_gt, n_det, n_rel, opts=None, transform=None):
    d = synth.synthetic_relsample_image(seed, n_gt, n_det, n_rel, **(opts or {}))
    if transform is None:
        return d
    if transform[0] == "pad":
        return pad_front(d, transform[1], transform[2])
    if transform[0] == "quantise":
        return quantise_scores(d, transform[1])
    raise ValueError(transform)


def large_case_inputs(name):
    """(image dict, config, non_masked) of a LARGE_CASES entry."""
    seed, n_gt, n_det, n_rel, opts, cfg, non_masked, transform = LARGE_CASES[name]
    return seeded_image(seed, n_gt, n_det, n_rel, opts, transform), cfg, non_masked


# ---- the edge sweep: one launch per config, (P, T, n_rel) per image; a generated size below (P, T) is padded in front ------------
# every P of {31, 32, 33, 63, 64, 65, 255, 256}, every T of {15, 16, 17, 32, 33, 256}, every per_rel of {1, 4, 16} and every batch
# of {2, 64, 2048} appears, both require_overlap settings, and every P at the 64/65 and 255/256 edges meets a T above 16
SWEEPS = {
    "capped": ((0.5, False, 4, 64, 0.25), [
        dict(P=31, T=15, n_rel=30), dict(P=32, T=16, n_rel=30), dict(P=33, T=17, n_rel=40), dict(P=63, T=32, n_rel=60),
        dict(P=64, T=33, n_rel=60), dict(P=65, T=17, n_rel=40), dict(P=255, T=33, n_rel=90), dict(P=256, T=32, n_rel=90),
        dict(P=256, T=256, n_rel=30, gen=(40, 17)),
    ]),
    "overlap_wide": ((0.5, True, 16, 2048, 0.25), [
        dict(P=63, T=16, n_rel=40), dict(P=64, T=17, n_rel=40, opts=dict(max_copies=8)), dict(P=65, T=33, n_rel=80),
        dict(P=255, T=17, n_rel=60, opts=dict(max_copies=12)), dict(P=256, T=256, n_rel=600),
        dict(P=33, T=256, n_rel=30, gen=(33, 15)), dict(P=255, T=256, n_rel=60, gen=(80, 33), opts=dict(max_copies=8)),
    ]),
    "tiny_batch": ((0.5, False, 1, 2, 0.25), [
        dict(P=31, T=17, n_rel=40), dict(P=32, T=33, n_rel=60), dict(P=33, T=15, n_rel=30), dict(P=64, T=32, n_rel=60),
        dict(P=65, T=256, n_rel=40, gen=(65, 17)), dict(P=255, T=32, n_rel=90), dict(P=256, T=17, n_rel=40),
    ]),
}


def sweep_images(name):
    """(config, [image dict, ...]) of a sweep; every image has relation_non_masked."""
    cfg, items = SWEEPS[name]
    images = []
    for k, it in enumerate(items):
        n_det, n_gt = it.get("gen", (it["P"], it["T"]))
        seed = 7000 + 100 * sorted(SWEEPS).index(name) + k
        d = synth.synthetic_relsample_image(seed, n_gt, n_det, it["n_rel"], **it.get("opts", {}))
        if (n_det, n_gt) != (it["P"], it["T"]):
            d = pad_front(d, it["P"], it["T"])
        assert len(d["prp_boxes"]) == it["P"] and len(d["tgt_boxes"]) == it["T"]
        images.append(d)
    return cfg, images


# ---- facts about a case, from the restatement's parts (np_relsample_parts of test_relsample_host.py) ------------------------------

def relation_cells(s, T):
    """The flat cell index h * T + t of every GT relation, in the sampler's (nonzero) order."""
    return [r["h"] * T + r["t"] for r in s["rels"]]


def steps_of(T):
    """Steps of the kernel's relation loop: 256 matrix cells each."""
    return max(1, -(-(T * T) // STEP))


def match_words(s):
    """The mask words (proposal index // 32) that hold at least one match bit of a GT box that a relation uses."""
    used = sorted({r["h"] for r in s["rels"]} | {r["t"] for r in s["rels"]})
    cols = np.nonzero(s["is_match"][used].any(0))[0] if used else np.zeros(0, np.int64)
    return sorted({int(c) // 32 for c in cols})


def window_tie_run(s):
    """The background candidates whose quality equals the quality at the window's edge, as (taken, left out): both in the
    window's (quality desc, row-major asc) order.  Both empty when the window is the whole background."""
    w, q = s["window"], s["bg_quality"]
    if w == 0 or w >= len(q) or q[w] != q[w - 1]:
        return s["bg_sorted"][:0], s["bg_sorted"][:0]
    run = np.nonzero(q == q[w - 1])[0]
    return s["bg_sorted"][run[run < w]], s["bg_sorted"][run[run >= w]]


def record_line(case, d, cfg, s, compared):
    """One line of profiles/relsample_scale_parity.txt."""
    P, T = len(d["prp_boxes"]), len(d["tgt_boxes"])
    rows = 2 if s["n_fg"] == 0 and s["num_neg"] == 0 else s["n_fg"] + s["num_neg"]
    return ("relsample_scale_parity case=%s P=%d T=%d relations=%d steps=%d match_words=%s overlap=%d per_rel=%d batch=%d F=%d "
            "n_fg=%d background=%d window=%d rows=%d deterministic_rows_compared=%s"
            % (case, P, T, len(s["rels"]), steps_of(T), ",".join(map(str, match_words(s))), int(cfg[1]), cfg[2], cfg[3],
               s["n_pre"], s["n_fg"], len(s["bg_sorted"]), s["window"], rows, "yes" if compared else "no"))
