"""Hash ties at the quota cut, host side: every construction of tests/sampler_tie_cases.py is what its name says.  The two tied
elements are members and share a hash and no third member does; the cut falls where the placement says; the owners of the tied
elements, the cut bin's count and the path it selects are as named; some committed seeds are found again by the search; and
every wrong way of breaking the tie changes the expected rows of at least one case of every kernel, so a device that made that
mistake could not pass tests/test_sampler_ties_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_tie_cases as tc  # noqa: E402
import test_boxsample_host as box_host  # noqa: E402
import test_relsample_gtbox_host as gtbox_host  # noqa: E402
from sampler_tie_cases import PICK_BG, PICK_FG, PICK_NEG, PICK_POS, np_hash32  # noqa: E402


def tie_images():
    """[(kernel, classes function, expected function, image)] of every tie case of every table."""
    out = [("box", tc.label_classes, tc.label_expected, im) for im in tc.box_images()]
    out += [("gtbox", tc.gtbox_classes, lambda im: tc.gtbox_expected(im)[0], im) for im in tc.gtbox_images()]
    out += [("rpn_lds", tc.label_classes, tc.label_expected, im) for call in ("neg", "pos") for im in tc.rpn_lds_calls()[call]]
    out += [("rpn_stream", tc.label_classes, tc.label_expected, im) for call in ("a", "b") for im in tc.rpn_stream_calls()[call]]
    out += [("detect", tc.detect_classes, tc.detect_expected, im) for im in tc.detect_images()]
    return out


def test_every_case_of_the_tables_is_built():
    """No case is skipped at run time: a table entry that cannot be constructed fails here (population_for asserts)."""
    assert [im["name"] for im in tc.box_images()] == [c[0] for c in tc.BOX_CASES] and len(tc.BOX_CASES) == 27
    assert [im["name"] for im in tc.gtbox_images()] == [c[0] for c in tc.GTBOX_CASES] and len(tc.GTBOX_CASES) == 30
    assert sum(len(v) for v in tc.rpn_lds_calls().values()) == len(tc.RPN_LDS_CASES) == 8
    assert sum(len(v) for v in tc.rpn_stream_calls().values()) == len(tc.RPN_STREAM_CASES) == 8
    assert [im["name"] for im in tc.detect_images()] == [c[0] for c in tc.DETECT_CASES] and len(tc.DETECT_CASES) == 15
    assert [im["kind"] for im in tc.box_boundary_images()] == [im["kind"] for im in tc.rpn_boundary_images()] == list(tc.BOUNDARY_KINDS)
    for kernel, _, _, im in tie_images():
        assert im["ties"] and {t["placement"] for t in im["ties"]} <= set(tc.PLACEMENTS), (kernel, im["name"])
    # what the issue asks of the tables: all three placements per kernel and class, an image index above 0 per kernel
    seen = {(k, t["purpose"], t["placement"]) for k, _, _, im in tie_images() for t in im["ties"]}
    for kernel, purposes in (("box", (PICK_POS, PICK_NEG)), ("gtbox", (PICK_FG, PICK_BG)), ("rpn_lds", (PICK_POS, PICK_NEG)), ("rpn_stream", (PICK_NEG,)),
                             ("detect", (tc.DETECT_CAP_FG, tc.DETECT_PICK_BG))):
        assert all((kernel, p, w) in seen for p in purposes for w in tc.PLACEMENTS), kernel
        assert any(im["img"] > 0 for k, _, _, im in tie_images() if k == kernel), kernel
    layouts = {(k, t["layout"]) for k, _, _, im in tie_images() for t in im["ties"]}
    assert {("box", "waves"), ("box", "wave"), ("box", "thread"), ("gtbox", "waves"), ("gtbox", "wave"), ("gtbox", "thread"),
            ("rpn_stream", "tile"), ("rpn_stream", "group"), ("rpn_stream", "groups"), ("detect", "waves"), ("detect", "wave"), ("detect", "thread")} <= layouts


def test_the_tied_pair_and_the_cut_are_where_each_case_says():
    for kernel, classes, _, im in tie_images():
        cls = classes(im)
        for t in im["ties"]:
            members, K = cls[t["purpose"]]
            what = (kernel, im["name"])
            assert K is not None and K == t["K"] and len(members) == t["M"] > K, what
            h = np_hash32(im["seed"], im["img"], t["purpose"], members)
            H = int(np_hash32(im["seed"], im["img"], t["purpose"], [t["e_lo"]])[0])
            assert t["e_lo"] < t["e_hi"] and sorted(members[h == H].tolist()) == [t["e_lo"], t["e_hi"]], what   # both, and no third
            (hk, ek), (hn, en) = tc.cut_of(im["seed"], im["img"], t["purpose"], members, K)
            if t["placement"] == "split":          # T is the tied key, need 1 of 2
                assert (hk, ek, hn, en) == (H, t["e_lo"], H, t["e_hi"]), what
            elif t["placement"] == "both":         # T is the tied key, need 2 of 2
                assert (hk, ek) == (H, t["e_hi"]) and hn > H and int((h < H).sum()) == K - 2, what
            else:                                  # T is the key just below, the pair is left out
                assert hk < H and (hn, en) == (H, t["e_lo"]), what
            # the same tie at another image index is no tie: rng64 mixes the image in
            other = np_hash32(im["seed"], im["img"] + 1, t["purpose"], [t["e_lo"], t["e_hi"]])
            assert other[0] != other[1], what


def test_the_owners_of_the_tied_elements_are_as_each_case_is_named():
    for kernel, _, _, im in tie_images():
        for t in im["ties"]:
            lo, hi = t["e_lo"], t["e_hi"]
            if kernel in ("box", "gtbox", "detect"):
                # detect: thread i owns candidate row i of the background, 8 consecutive positions of the 2 000 triplets
                cells = {"box": im["n"], "gtbox": im["n"] ** 2, "detect": 64 * 256 if t["purpose"] == tc.DETECT_PICK_BG else tc.DETECT_F}[kernel]
                chunk = -(-cells // 256)
                assert chunk == {6144: 24, 65536: 256, 10000: 40, 16384: 64, 2000: 8}[cells]
                assert tc.layout_of(chunk, lo, hi) == t["layout"], im["name"]
                same_thread, same_wave = lo // chunk == hi // chunk, lo // chunk // 64 == hi // chunk // 64
                assert {"thread": same_thread, "wave": same_wave and not same_thread, "waves": not same_wave}[t["layout"]]
                if t["layout"] == "thread" and kernel == "box":
                    assert hi - lo < 24
            elif kernel == "rpn_stream":
                assert tc.stream_layout_of(lo, hi) == t["layout"], im["name"]
                tile, group = lo // 256 == hi // 256, lo // 1024 == hi // 1024
                assert {"tile": tile, "group": group and not tile, "groups": not group}[t["layout"]]


def test_cut_bins_and_paths_of_the_rpn_cases():
    need_seen = set()
    for call in ("neg", "pos"):
        for im in tc.rpn_lds_calls()[call]:
            (t,) = im["ties"]
            count, need = tc.rpn_cut_bins(im)[t["purpose"]]
            members, K = tc.label_classes(im)[t["purpose"]]
            assert count == t["cut_bin_members"] == tc.bin_count(im["seed"], im["img"], t["purpose"], members, t["e_lo"]), im["name"]
            want = t["bin_below"] + {"split": 1, "both": 2, "neither": 0}[t["placement"]]
            assert need == want and tc.rpn_path(im) == "lds", (im["name"], need, want)
            need_seen.add("full" if need == count else need)
    assert {1, 2, "full"} <= need_seen                                    # bin_need of 1, of 2 and of the bin's full count
    for call in ("a", "b"):
        for im in tc.rpn_stream_calls()[call]:
            bins = tc.rpn_cut_bins(im)
            for t in im["ties"]:
                members, _ = tc.label_classes(im)[t["purpose"]]
                if t["cut_bin_members"] is not None:
                    assert bins[t["purpose"]][0] == t["cut_bin_members"] == tc.bin_count(im["seed"], im["img"], t["purpose"], members, t["e_lo"])
            assert tc.rpn_path(im) == im["path"], im["name"]
    # the path switch: the same image with one label flipped to ignore, 2049 members of the negatives' cut bin against 2048
    a, b = tc.rpn_stream_calls()["a"][0], tc.rpn_stream_calls()["b"][0]
    assert (a["seed"], a["img"]) == (b["seed"], b["img"]) and np.nonzero(a["labels"] != b["labels"])[0].tolist() == [b["flipped"]]
    assert (a["labels"][b["flipped"]], b["labels"][b["flipped"]]) == (0, -1)
    assert tc.rpn_cut_bins(a)[PICK_NEG][0] == tc.CAND_CAP + 1 and tc.rpn_cut_bins(b)[PICK_NEG][0] == tc.CAND_CAP
    assert (tc.rpn_path(a), tc.rpn_path(b)) == ("stream", "lds")
    np.testing.assert_array_equal(tc.label_expected(a), tc.label_expected(b))   # the ignored member lay behind the cut: the same rows
    both = tc.rpn_stream_calls()["b"][1]
    assert {t["purpose"] for t in both["ties"]} == {PICK_POS, PICK_NEG} and all(K is not None for _, K in tc.label_classes(both).values())


def test_boundary_populations_put_the_cut_where_they_say():
    for images in (tc.box_boundary_images(), tc.rpn_boundary_images()):
        assert len({(im["batch"], im["fraction"], im["seed"]) for im in images}) == 1 and [im["img"] for im in images] == [0, 1, 2, 3]
        for im in images:
            members, K = tc.label_classes(im)[PICK_NEG]
            assert K == im["K"], im["name"]
            top = np.sort(np_hash32(im["seed"], im["img"], PICK_NEG, members)) >> 24
            kth, nxt, in_bin, above = top[K - 1], top[K], int((top == top[K - 1]).sum()), int((top < top[K - 1]).sum())
            if im["kind"] == "last_of_bin":        # need == h: above + h == K
                assert nxt > kth and above + in_bin == K, im["name"]
            elif im["kind"] == "first_of_bin":     # need == 1
                assert above == K - 1 and in_bin >= (2049 if "path" in im else 8), (im["name"], in_bin)
            elif im["kind"] == "digit_255":        # the kernels' digit 255 is the hashes' top byte 0
                # K below M / 256: half of it at 6 144 proposals (4 000 members, K = 8), a 280th at 590 000 anchors
                assert kth == 0 and K * 256 * (100 if "path" in im else 1) < len(members), im["name"]
            else:                                  # their digit 0 the top byte 255
                assert kth == 255 and K == len(members) - 1, im["name"]
            if "path" in im:
                assert tc.rpn_path(im) == "stream", im["name"]


def test_committed_seeds_are_found_again_by_the_search():
    for table, n_of, names in ((tc.BOX_PAIRS, lambda k: tc.BOX_N, ("pos_waves", "neg_waves", "pos_thread", "both_neg")),
                               (tc.GTBOX_PAIRS, lambda k: (256 if "256" in k else 100) ** 2, ("fg256_waves", "bg256_wave", "bg100_waves"))):
        for name in names:
            first, seed, img, purpose, e_lo, e_hi = table[name]
            found = tc.find_collisions(purpose, n_of(name), img, first, seed - first + 1)
            assert (seed, e_lo, e_hi) in found and found[-1][0] == seed, (name, found[-3:])   # (a stream may hold a second pair)
    for n, seed, pairs in ((tc.RPN_LDS_N, tc.RPN_LDS_SEED, tc.RPN_LDS_PAIRS), (tc.RPN_STREAM_N, tc.RPN_STREAM_SEED, tc.RPN_STREAM_PAIRS)):
        (img, purpose), pair = sorted(pairs.items())[-1]
        assert (seed,) + pair in tc.find_collisions(purpose, n, img, seed, 1)


# ---- wrong restatements ----------------------------------------------------------------------------------------------------

def _owner(kernel, im, variant):
    if variant == "room_not_reduced":
        return lambda e: e // 256                          # the streaming path's scan tile
    if kernel in ("rpn_lds", "rpn_stream"):
        return lambda e: e % 256                           # both paths read the labels strided
    if kernel == "detect":
        return (lambda e: e // tc.DETECT_P) if im["ties"][0]["purpose"] == tc.DETECT_PICK_BG else (lambda e: e // -(-tc.DETECT_F // 256))
    chunk = -(-(im["n"] if kernel == "box" else im["n"] ** 2) // 256)
    return lambda e: e // chunk


@pytest.mark.parametrize("variant", tc.WRONG)
def test_a_wrong_tie_break_changes_the_expected_rows_of_every_kernel(variant, monkeypatch):
    """The restatements with the tie broken towards the higher index, with all or none of the tied members taken, with `need`
    counted per thread, and (streaming path) with `room` not reduced by earlier tiles: each differs from the right rows on at
    least one case of every kernel it applies to, and where it differs the row count is the one the mistake implies."""
    changed = {}
    for kernel, _, expected, im in tie_images():
        if variant == "room_not_reduced" and kernel != "rpn_stream":
            continue
        right = expected(im)
        with monkeypatch.context() as m:
            wrong_pick = tc.wrong_pick(variant, _owner(kernel, im, variant))
            m.setattr(box_host, "np_pick", wrong_pick)
            m.setattr(gtbox_host, "np_pick", wrong_pick)
            m.setattr(tc, "np_pick", wrong_pick)
            wrong = expected(im)
        differs = wrong.shape != right.shape or not np.array_equal(wrong, right)
        changed.setdefault(kernel, []).append(differs)
        split = [t for t in im["ties"] if t["placement"] == "split"]
        if differs:
            assert split, (im["name"], "only a cut inside the pair can tell the variants apart")
            delta = {"higher_index": 0, "all_tied": len(split), "no_tied": -len(split)}.get(variant, len(split))
            if kernel != "gtbox":                  # (its restatement fills the batch: a foreground row more is a background row less)
                assert len(wrong) - len(right) == delta, (variant, im["name"])
        elif split and variant in ("higher_index", "all_tied", "no_tied"):
            raise AssertionError("%s leaves the rows of %s unchanged" % (variant, im["name"]))
    kernels = {"rpn_stream"} if variant == "room_not_reduced" else {"box", "gtbox", "rpn_lds", "rpn_stream", "detect"}
    assert set(changed) == kernels and all(any(v) for v in changed.values()), (variant, {k: sum(v) for k, v in changed.items()})
