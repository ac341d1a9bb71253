"""MEET expert sampling in the three GCL_SETTING.ZERO_LABEL_PADDING_MODEs: two independent restatements of the reference loop
(roi_relation_predictors.py:3940-3969) and the inputs of tests/test_meet_sample_host.py and tests/test_meet_sample_gpu.py.

  sample_stdlib   on the standard library's `random` (random.random, random.randint: the generator the reference itself calls)
  sample_words    on raw 32-bit words through oracle.train_oracle.PyRandomStream, with each mode's consumption spelled out; it
                  counts the events the crafted cases are named for, and takes `wrong=` to become one of the wrong restatements
                  (WRONG) that the host tests hold the cases against

A case is a dict: name, mode, G, n_cls, incre, rates [G, n_cls] float64, labels [n] int64, words [exact] uint32 -- the block is
EXACTLY as long as the sampling consumes -- and `expect`, names of events whose count must be non-zero (the case's premises).
"""
import random

import numpy as np

from oracle.train_oracle import PyRandomStream

MODES = ("rand_insert", "rand_choose", "all_include")
MODE_ID = {"rand_insert": 0, "rand_choose": 1, "all_include": 2}
WRONG = ("gt_at_0.4", "choose_one_word", "all_include_one_word", "choose_single_group", "kbits_of_g_minus_1", "u_lt_rate", "descending")
LIMITS = (1024, 4096, 64)      # (tile, window, chunk) of veto_meet_sample_parallel_limits: tests/test_meet_sample_gpu.py compares
ALL_ONES, POINT4_WORDS, POINT4_MANTISSA = 0xFFFFFFFF, (53687091 << 5, 13421773 << 6), 53687091 * (1 << 26) + 13421773


def sample_stdlib(labels, incre, rates, G, mode):
    """The reference loop on Python's own generator (seed it first; random.random() afterwards is the lock-step check)."""
    chosen = [[] for _ in range(G)]
    for i, lab in enumerate(labels):
        lab = int(lab)
        if lab == 0:
            if mode == "rand_insert":
                chosen[random.randint(0, G - 1)].append(i)
            else:
                keep = random.random() if mode == "rand_choose" else 1.0
                if mode not in ("rand_choose", "all_include"):
                    raise ValueError(mode)
                if keep >= 0.4:
                    for k in range(G):
                        chosen[k].append(i)
            continue
        u = random.random()
        for act in range(G, 0, -1):
            if u <= rates[act - 1][lab] or act < incre[lab]:
                for k in range(act):
                    chosen[k].append(i)
                break
    return chosen


def sample_words(labels, incre, rates, G, mode, words, wrong=None):
    """The same on raw words.  Returns (chosen, words_used, events); words_used is -1 when the block is too short (the lists are
    then those up to the relation that ran out)."""
    assert wrong is None or wrong in WRONG
    stream = PyRandomStream(words)
    chosen = [[] for _ in range(G)]
    ev = dict(bg=0, fg=0, rejected=0, longest_rejection_run=0, bg_kept=0, bg_dropped=0, u_eq_0p4=0, u_eq_rate=0, by_rate=0, by_group=0,
              act1=0, fg_nowhere=0, fg_all=0, group0_word0=0)
    kbits = (G - 1).bit_length() if wrong == "kbits_of_g_minus_1" else G.bit_length()

    def put(i, groups):
        for k in groups:
            if wrong == "descending":
                chosen[k].insert(0, i)
            else:
                chosen[k].append(i)

    try:
        for i, lab in enumerate(labels):
            lab = int(lab)
            if lab == 0:
                ev["bg"] += 1
                if mode == "rand_insert":           # one word per attempt: the top kbits bits, again while they are >= G
                    run = 0
                    while True:
                        w = stream._u32()
                        r = w >> (32 - kbits)
                        if r < G:
                            break
                        run += 1
                    ev["rejected"] += run
                    ev["longest_rejection_run"] = max(ev["longest_rejection_run"], run)
                    ev["group0_word0"] += int(w == 0)
                    put(i, [r])
                elif mode == "rand_choose":         # two words: u = random()
                    if wrong == "choose_one_word":
                        u = (stream._u32() >> 5) / float(1 << 27)
                    elif wrong == "choose_single_group":
                        put(i, [stream.randint0(G)])
                        continue
                    else:
                        u = stream.random()
                    ev["u_eq_0p4"] += int(u == 0.4)
                    keep = u > 0.4 if wrong == "gt_at_0.4" else u >= 0.4
                    ev["bg_kept" if keep else "bg_dropped"] += 1
                    if keep:
                        put(i, range(G))
                elif mode == "all_include":         # no word
                    if wrong == "all_include_one_word":
                        stream._u32()
                    ev["bg_kept"] += 1
                    put(i, range(G))
                else:
                    raise ValueError(mode)
                continue
            ev["fg"] += 1
            u = stream.random()                    # two words
            hit = 0
            for act in range(G, 0, -1):
                rate = float(rates[act - 1][lab])
                by_rate = u < rate if wrong == "u_lt_rate" else u <= rate
                ev["u_eq_rate"] += int(u == rate)
                if by_rate or act < incre[lab]:
                    ev["by_rate" if by_rate else "by_group"] += 1
                    hit = act
                    break
            ev["act1"] += int(hit == 1)
            ev["fg_nowhere"] += int(hit == 0)
            ev["fg_all"] += int(hit == G)
            put(i, range(hit))
    except IndexError:
        return chosen, -1, ev
    return chosen, stream.pos, ev


def group_labels(labels, rows, incre, k):
    """Ensemble.forward :3812-3821 for the rows of group k: own classes 1.., other foreground classes size + 1, background 0."""
    own = [c for c, g in enumerate(incre) if g == k + 1]
    return np.array([0 if labels[i] == 0 else (own.index(int(labels[i])) + 1 if incre[int(labels[i])] == k + 1 else len(own) + 1)
                     for i in rows], dtype=np.int64)


def tables_of(incre):
    """(pos_in_group, group_size) as MeetTrainingSampler builds them."""
    G = max(incre)
    pos, seen = [0] * len(incre), {}
    for c, g in enumerate(incre):
        if g:
            seen[g] = seen.get(g, 0) + 1
            pos[c] = seen[g]
    return pos, [seen.get(g + 1, 0) for g in range(G)]


# ---- word crafting -------------------------------------------------------------------------------------------------
def words_of_mantissa(m):
    """The two words random() turns into m / 2^53 (0 <= m < 2^53)."""
    return [(m >> 26) << 5, (m & ((1 << 26) - 1)) << 6]


def mantissa_of(u):
    m = int(u * (1 << 53))
    assert m / float(1 << 53) == u
    return m


def accept_word(G, group, low=0):
    k = G.bit_length()
    return (group << (32 - k)) | (low & ((1 << (32 - k)) - 1))


def synthetic_tables(G, seed):
    """Two classes per group (class 0 = background); rates: random doubles, a few exact 0.0 / 1.0."""
    rng = np.random.RandomState(seed)
    incre = [0] + [g + 1 for g in range(G) for _ in range(2)]
    rates = rng.random_sample((G, len(incre)))
    rates[rng.random_sample(rates.shape) < 0.15] = 1.0
    rates[rng.random_sample(rates.shape) < 0.10] = 0.0
    return incre, rates


def dataset_tables(dataset):
    from veto_amd import meet_tables
    sizes = {"VG": [4, 6, 9, 19, 12], "GQA": [5, 10, 20, 65]}[dataset]
    return meet_tables.incre_idx_list(sizes), np.array(meet_tables.sample_rate_matrix(dataset, sizes), dtype=np.float64)


def _finish(name, mode, incre, rates, labels, words, expect=()):
    """Cuts the word block to exactly what the sampling consumes."""
    G = max(incre)
    labels = np.asarray(labels, dtype=np.int64)
    words = np.asarray(words, dtype=np.uint64).astype(np.uint32)
    _, used, _ = sample_words(labels, incre, rates, G, mode, words)
    assert used >= 0, (name, "the crafted block is too short")
    return dict(name=name, mode=mode, G=G, n_cls=len(incre), incre=list(incre), rates=np.ascontiguousarray(rates, dtype=np.float64),
                labels=labels, words=np.ascontiguousarray(words[:used]), expect=tuple(expect))


def seeded_case(name, mode, incre, rates, n, seed, mix="random", fg_fraction=0.25, expect=()):
    rng = np.random.RandomState(seed)
    n_cls = len(incre)
    fg = rng.randint(1, n_cls, size=n)
    if mix == "random":
        labels = np.where(rng.random_sample(n) < fg_fraction, fg, 0)
    elif mix == "all_bg":
        labels = np.zeros(n, dtype=np.int64)
    elif mix == "all_fg":
        labels = fg
    elif mix == "alternating":
        labels = np.where(np.arange(n) % 2 == 0, 0, fg)
    elif mix == "one_fg":
        labels = np.zeros(n, dtype=np.int64)
        labels[(2 * n) // 3] = fg[0]
    else:
        raise ValueError(mix)
    words = rng.randint(0, 1 << 32, size=4 * n + 4096, dtype=np.uint64)
    return _finish(name, mode, incre, rates, labels, words, expect)


def crafted_cases(limits=LIMITS):
    """limits: the sizes the cases sit on both sides of."""
    tile, window, chunk = limits
    cases = []
    vg, gqa = dataset_tables("VG"), dataset_tables("GQA")
    # group counts x modes, small and odd sizes; for G in 1, 2, 4, 8 half of randint's draws are rejected
    for G in (1, 2, 3, 4, 5, 8):
        incre, rates = synthetic_tables(G, 100 + G)
        for mode in MODES:
            cases.append(seeded_case("g%d_%s_n65" % (G, mode), mode, incre, rates, 65, 7 * G + MODE_ID[mode],
                                     expect=("bg", "fg") + (("rejected",) if mode == "rand_insert" and G in (1, 2, 4, 8) else ())))
    # sizes: 1, 2, around the chunk, around the tile, around the window (in words: rand_choose consumes 2 n, so n = window / 2
    # puts the block's end on the window's; rand_insert and all_include cross it inside the larger cases), the real batch
    sizes = sorted({1, 2, chunk - 1, chunk, chunk + 1, tile - 1, tile, tile + 1, window // 2 - 1, window // 2, window // 2 + 1,
                    window - 1, window, window + 1, 2 * window + 1})
    for n in sizes:
        for mode in MODES:
            incre, rates = vg if n % 2 else gqa
            cases.append(seeded_case("n%d_%s" % (n, mode), mode, incre, rates, n, 1000 + n))
    for mode in MODES:
        cases.append(seeded_case("real_batch_12288_%s" % mode, mode, *vg, 12288, 5, expect=("bg", "fg", "by_rate")))
    # label mixes
    for mix in ("all_bg", "all_fg", "alternating", "one_fg"):
        for mode in MODES:
            cases.append(seeded_case("%s_%s" % (mix, mode), mode, *gqa, 3 * chunk + 5 if mix != "one_fg" else tile + chunk + 3, 31,
                                     mix=mix, expect=("bg",) if mix == "all_bg" else ("fg",) if mix == "all_fg" else ("bg", "fg")))
    cases += _rejection_cases(tile, window, chunk, vg)
    cases += _choose_cases(vg)
    cases += _foreground_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def _rejection_cases(tile, window, chunk, vg):
    incre, rates = vg
    G = max(incre)                       # 5: three bits, 5..7 rejected
    fg_words = words_of_mantissa(mantissa_of(0.25))
    out = []

    def bg(run, group, low=0):
        return [ALL_ONES] * run + [accept_word(G, group, low)]

    # runs of 1, 8 and 200 rejected words; 0xFFFFFFFF is rejected for every G, the word 0 is accepted as group 0
    labels, words = [], []
    for run, group in ((1, 4), (8, 0), (200, 2), (0, 0)):
        labels.append(0)
        words += bg(run, group) if (run, group) != (0, 0) else [0]
    out.append(_finish("rejection_runs_1_8_200", "rand_insert", incre, rates, labels, words, ("rejected", "group0_word0")))
    for G2 in (1, 2, 3, 4, 8):
        inc2, rates2 = synthetic_tables(G2, 200 + G2)
        out.append(_finish("all_ones_rejected_g%d" % G2, "rand_insert", inc2, rates2, [0, 0, 1, 0],
                           [ALL_ONES, ALL_ONES, 0] + [0] + fg_words + [ALL_ONES] * 3 + [accept_word(G2, G2 - 1, 12345)], ("rejected", "group0_word0")))
    # a run that crosses a mask word's end (bit 64), and runs that cross the ends of the first three windows
    for name, lead in (("run_crosses_mask_word", chunk - 3), ("run_crosses_window", window - 5), ("run_crosses_second_window", 2 * window - 5),
                       ("run_crosses_third_window", 3 * window - 5)):
        labels = [0] * lead + [0, 0]
        words = [accept_word(G, i % G, i) for i in range(lead)] + bg(10, 3) + bg(0, 1)
        out.append(_finish(name, "rand_insert", incre, rates, labels, words, ("rejected",)))
    labels = [0] * 5 + [0, 1, 0]
    out.append(_finish("run_of_200_crosses_mask_words", "rand_insert", incre, rates, labels,
                       [accept_word(G, i, 77) for i in range(5)] + bg(200, 4) + fg_words + bg(3, 1), ("rejected", "fg")))
    # a foreground draw that starts inside a run of rejectable words: its two words are 0xFFFFFFFF, taken as u, not as attempts
    m = (ALL_ONES >> 5) * (1 << 26) + (ALL_ONES >> 6)
    assert words_of_mantissa(m) == [(ALL_ONES >> 5) << 5, (ALL_ONES >> 6) << 6]
    labels = [0, 7, 0, 7, 0]
    words = bg(2, 1) + [ALL_ONES, ALL_ONES] + bg(5, 2) + [ALL_ONES, ALL_ONES] + bg(0, 3)
    out.append(_finish("foreground_inside_rejectable_words", "rand_insert", incre, rates, labels, words, ("rejected", "fg")))
    # the block ends inside a rejection run once it is one word short: the last relation is a background with a run of 8
    out.append(_finish("ends_with_rejection_run", "rand_insert", incre, rates, [3, 0, 0], fg_words + bg(0, 2) + bg(8, 4), ("rejected",)))
    # many foreground relations in front of a background: the walk's position runs ahead of its mask word by more than one word
    labels = [9] * (2 * chunk + 7) + [0, 0] + [9] * chunk + [0]
    words = fg_words * (2 * chunk + 7) + bg(3, 0) + bg(0, 1) + fg_words * chunk + bg(70, 2)
    out.append(_finish("foreground_runs_then_background", "rand_insert", incre, rates, labels, words, ("rejected", "fg")))
    return out


def _choose_cases(vg):
    incre, rates = vg
    at, below, above = POINT4_MANTISSA, POINT4_MANTISSA - 1, POINT4_MANTISSA + 1
    assert at / float(1 << 53) == 0.4 and words_of_mantissa(at) == list(POINT4_WORDS)
    labels = [0, 0, 0, 5, 0]
    words = words_of_mantissa(at) + words_of_mantissa(below) + words_of_mantissa(above) + words_of_mantissa(mantissa_of(0.5)) + words_of_mantissa(at)
    return [_finish("u_exactly_0p4_kept_one_step_below_dropped", "rand_choose", incre, rates, labels, words,
                    ("u_eq_0p4", "bg_kept", "bg_dropped", "fg"))]


def _foreground_cases():
    """Tables set through the ABI: rates equal to u, and the doubles just below and above it; act < incre deciding; act = 1 only;
    no group at all.  G = 4, one class per group plus two more in group 3."""
    incre = [0, 1, 2, 3, 4, 3, 3]
    G, n_cls = 4, len(incre)
    u = 0.3718745768070221
    m = mantissa_of(u)
    out = []
    for mode in MODES:
        rates = np.zeros((G, n_cls))
        labels, words = [], []
        # class 4 (group 4): rate of act 4 just below u -> not taken; act 3: exactly u -> taken by rate (u <= rate): groups 0..2
        rates[3][4], rates[2][4] = np.nextafter(u, 0.0), u
        # class 2 (group 2): act 4: just above u -> all four groups
        rates[3][2] = np.nextafter(u, 1.0)
        # class 3 (group 3): every rate below u; act 2 < incre 3 decides: groups 0..1
        rates[:, 3] = np.nextafter(u, 0.0)
        # class 1 (group 1): only act 1 has a rate >= u: group 0 alone
        rates[0][1] = 1.0
        # class 5 (group 3): rates 0 except nothing ... act 2 < 3 decides as well; class 6: all rates exactly u -> act 4
        rates[:, 6] = u
        for lab in (4, 2, 3, 1, 5, 6, 0, 4):
            labels.append(lab)
            if lab != 0:
                words += words_of_mantissa(m)
            elif mode == "rand_insert":
                words += [ALL_ONES, accept_word(G, 3)]
            elif mode == "rand_choose":
                words += words_of_mantissa(mantissa_of(0.75))
        out.append(_finish("foreground_edges_%s" % mode, mode, incre, rates, labels, words, ("u_eq_rate", "by_rate", "by_group", "act1", "fg_all")))
    # a foreground relation that joins no group: group 1's class with every rate below u (act < 1 never holds)
    rates = np.zeros((G, n_cls))
    rates[:, 2] = 1.0
    out.append(_finish("foreground_joins_no_group", "all_include", incre, rates, [1, 2, 0, 1], words_of_mantissa(m) * 3, ("fg_nowhere", "fg_all")))
    return out
