"""The two restatements of MEET expert sampling (tests/meet_sample_cases.py) against each other, against the reference's own
sampling in the training goldens, and against the wrong restatements the crafted cases are there to tell apart.  No GPU.

`python tests/test_meet_sample_host.py` prints the case table, the event counts and the mutation log
(profiles/meet_sample_parity.txt)."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meet_sample_cases as mc      # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES_MEET = ["train_meet_vg", "train_meet_gqa", "train_meet_sgcls", "train_meet_l3h4"]      # tests/test_train_losses.py
CASES = mc.crafted_cases()
# which wrong restatement each mode's cases must catch
WRONG_FOR = {"gt_at_0.4": ("rand_choose",), "choose_one_word": ("rand_choose",), "choose_single_group": ("rand_choose",),
             "all_include_one_word": ("all_include",), "kbits_of_g_minus_1": ("rand_insert",), "u_lt_rate": mc.MODES, "descending": mc.MODES}


def _state_words(n):
    """The next n raw words of Python's generator, without moving it."""
    st = random.getstate()
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": np.array(st[1][:624], dtype=np.uint32), "pos": int(st[1][624])}}
    return bg.random_raw(n).astype(np.uint32)


def _both(labels, incre, rates, G, mode, seed):
    """(lists, next random()) of the stdlib restatement and of the word restatement fed the same generator's words."""
    random.seed(seed)
    words = _state_words(4 * len(labels) + 4096)
    a = mc.sample_stdlib(labels, incre, rates, G, mode)
    after_a = random.random()
    b, used, _ = mc.sample_words(labels, incre, rates, G, mode, words)
    assert used >= 0
    from oracle.train_oracle import PyRandomStream
    stream = PyRandomStream(words)
    stream.pos = used
    return a, after_a, b, stream.random()


def test_the_words_of_0p4_are_the_double_0p4():
    w0, w1 = mc.POINT4_WORDS
    u = ((w0 >> 5) * 67108864.0 + (w1 >> 6)) * (1.0 / 9007199254740992.0)
    assert u == 0.4 and (w0, w1) == (53687091 << 5, 13421773 << 6)
    below = mc.words_of_mantissa(mc.POINT4_MANTISSA - 1)
    assert 0.4 - ((below[0] >> 5) * 67108864.0 + (below[1] >> 6)) * (1.0 / 9007199254740992.0) == 2.0 ** -53


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_two_restatements_agree(case):
    """On the case's labels and tables under Python's generator (the crafted WORDS cannot be put into the stdlib generator: they are
    held to the word restatement alone, by the premises below and on the device)."""
    for seed in (1, 77):
        a, after_a, b, after_b = _both(case["labels"], case["incre"], case["rates"], case["G"], case["mode"], seed)
        assert a == b and after_a == after_b


@pytest.mark.parametrize("name", CASES_MEET)
def test_both_reproduce_the_reference_sampling_of_the_goldens(name):
    from veto_amd import meet_tables
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    sizes = [int(x) for x in g["group_sizes"]]
    incre = meet_tables.incre_idx_list(sizes)
    rates = meet_tables.sample_rate_matrix(str(g["dataset"]), sizes)
    a, after_a, b, after_b = _both(g["labels"], incre, rates, len(sizes), "rand_insert", 1)
    for k in range(len(sizes)):
        assert np.array_equal(np.array(a[k], dtype=np.int64), g["chosen_%d" % k]) and a[k] == b[k], k
    assert after_a == after_b == float(g["random_after"][0])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_premise_of_a_case_holds(case):
    _, used, ev = mc.sample_words(case["labels"], case["incre"], case["rates"], case["G"], case["mode"], case["words"])
    assert used == len(case["words"])                  # the block is exactly as long as the sampling consumes
    for event in case["expect"]:
        assert ev[event] > 0, event
    if used > 0:                                        # and one word less is too short
        assert mc.sample_words(case["labels"], case["incre"], case["rates"], case["G"], case["mode"], case["words"][:-1])[1] == -1


def test_named_events_of_the_crafted_cases():
    by = {c["name"]: mc.sample_words(c["labels"], c["incre"], c["rates"], c["G"], c["mode"], c["words"])[2] for c in CASES}
    assert by["rejection_runs_1_8_200"]["longest_rejection_run"] == 200 and by["rejection_runs_1_8_200"]["rejected"] == 209
    assert by["run_of_200_crosses_mask_words"]["longest_rejection_run"] == 200
    assert by["u_exactly_0p4_kept_one_step_below_dropped"]["u_eq_0p4"] == 2 and by["u_exactly_0p4_kept_one_step_below_dropped"]["bg_dropped"] == 1
    for G in (1, 2, 4, 8):      # a power of two (and 1) rejects about half of its draws
        ev = by["g%d_rand_insert_n65" % G]
        assert 0.25 * ev["bg"] < ev["rejected"] < 2.5 * ev["bg"], (G, ev)
    assert by["foreground_joins_no_group"]["fg_nowhere"] == 2
    for mode in mc.MODES:
        ev = by["foreground_edges_" + mode]
        assert ev["u_eq_rate"] >= 2 and ev["by_group"] == 2 and ev["act1"] == 1


def mutation_log():
    """{wrong restatement: names of the cases whose lists or word count it changes}."""
    log = {}
    for wrong in mc.WRONG:
        caught = []
        for c in CASES:
            if c["mode"] not in WRONG_FOR[wrong]:
                continue
            good = mc.sample_words(c["labels"], c["incre"], c["rates"], c["G"], c["mode"], c["words"])
            try:
                bad = mc.sample_words(c["labels"], c["incre"], c["rates"], c["G"], c["mode"], c["words"], wrong=wrong)
            except ValueError:      # (kbits 0: a shift by 32 bits)
                bad = (None, None)
            if bad[0] != good[0] or bad[1] != good[1]:
                caught.append(c["name"])
        log[wrong] = caught
    return log


def test_each_wrong_restatement_changes_a_crafted_case():
    log = mutation_log()
    for wrong, caught in log.items():
        assert caught, wrong
    # the cases made for a mistake catch it, not only the large random ones
    assert "u_exactly_0p4_kept_one_step_below_dropped" in log["gt_at_0.4"]
    assert any(n.startswith("foreground_edges_") for n in log["u_lt_rate"])
    assert any(n.startswith("all_ones_rejected_g") or n.startswith("rejection_runs") for n in log["kbits_of_g_minus_1"])


if __name__ == "__main__":
    print("case | mode | G | n | words | events")
    for c in CASES:
        ev = mc.sample_words(c["labels"], c["incre"], c["rates"], c["G"], c["mode"], c["words"])[2]
        print("%s | %s | %d | %d | %d | %s" % (c["name"], c["mode"], c["G"], len(c["labels"]), len(c["words"]),
                                              " ".join("%s=%d" % kv for kv in ev.items() if kv[1])))
    print()
    print("wrong restatement | cases of its modes | cases it changes | first of them")
    for wrong, caught in mutation_log().items():
        total = sum(1 for c in CASES if c["mode"] in WRONG_FOR[wrong])
        print("%s | %d | %d | %s" % (wrong, total, len(caught), ", ".join(caught[:4])))
