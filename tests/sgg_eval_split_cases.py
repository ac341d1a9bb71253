"""Inputs and yardsticks of the split-level relation evaluation (SGGEvaluator.accumulate / finalize, veto_sgg_eval_fold):
tests/test_sgg_eval_split_host.py (CPU) checks the premises, tests/test_sgg_eval_split_gpu.py (MI355X) the device.

A set of RECORDS is what the evaluator keeps on the device: per image the GT-relation count and the pair count, per GT relation
the three match ranks, the zero-shot flag and the GT predicate.  np_fold restates the reference's accumulation over them
(sgg_eval.py:133-136, :209, :331-336, :420-466: per-image lists, np.mean at the end); np_fold_chunked restates the SAME numbers
in the summation order the device documents (include/veto_amd.h), so its bits are the device's bits."""
import functools

import numpy as np

from veto_amd import synth

KS = (20, 50, 100)
NO_MATCH = 0x3fffffff
FIELDS = ("gc_rank", "ng_rank", "acc_rank", "zeroshot_flag", "gt_predicate")
SCALARS = ("recall", "recall_nogc", "zeroshot_recall", "accuracy", "mean_recall", "ng_mean_recall")
MUTATIONS = ("acc_ratio_mean", "class_all_images", "zeroshot_all_images", "le_k")

SPLIT_SEED = 91
SPLIT_NUM_OBJS = [5 + (i * 7) % 8 for i in range(520)]
SGDET_NUM_OBJS = SPLIT_NUM_OBJS[:96]


@functools.lru_cache(maxsize=None)
def split_images(mode, num_rel):
    """The seeded split: 520 images, 7 312 GT relations (sgdet: the first 96 images, predictions on the detector's own boxes)."""
    if mode == "sgdet":
        return synth.synthetic_eval_images_sgdet(SPLIT_SEED, SGDET_NUM_OBJS, num_rel_cls=num_rel)
    return synth.synthetic_eval_images(SPLIT_SEED, SPLIT_NUM_OBJS, mode, num_rel_cls=num_rel)


@functools.lru_cache(maxsize=None)
def split_oracle(mode, num_rel):
    """oracle.evaluate over the whole seeded split, computed once per process."""
    from oracle import sgg_eval_oracle as so
    images, zeroshot = split_images(mode, num_rel)
    return so.evaluate(images, mode, zeroshot, num_rel)


def make_records(gt_count, pair_count, **fields):
    rec = {"gt_count": np.asarray(gt_count, np.int64), "pair_count": np.asarray(pair_count, np.int64)}
    rows = int(rec["gt_count"].sum())
    for name in FIELDS:
        rec[name] = np.asarray(fields[name], np.int32).reshape(-1)
        assert rec[name].size == rows, name
    return rec


def records_from_oracle(images, per_image):
    """The records the device would hold for `images`, from the oracle's per-image ranks (None: the image is not evaluated)."""
    cols = {name: [] for name in FIELDS}
    g_cnt, p_cnt = [], []
    for im, r in zip(images, per_image):
        gt_rels = np.asarray(im["gt_rels"], np.int64).reshape(-1, 3)
        G = len(gt_rels)
        g_cnt.append(G)
        p_cnt.append(len(np.asarray(im["pred_rel_inds"]).reshape(-1, 2)))
        cols["gt_predicate"].append(gt_rels[:, 2])
        for name, key in (("gc_rank", "gc_rank"), ("ng_rank", "ng_rank"), ("acc_rank", "acc_rank"), ("zeroshot_flag", "zeroshot")):
            cols[name].append(np.full(G, 0 if key == "zeroshot" else NO_MATCH, np.int64) if r is None
                              else np.minimum(np.asarray(r[key]).astype(np.int64), NO_MATCH))
    return make_records(g_cnt, p_cnt, **{k: np.concatenate(v) if v else np.zeros(0) for k, v in cols.items()})


def concat_records(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in ("gt_count", "pair_count") + FIELDS}


def _images_of(rec):
    """(G, P, slice of the image's rows) per image."""
    off = np.concatenate([[0], np.cumsum(rec["gt_count"])])
    return [(int(g), int(p), slice(int(off[i]), int(off[i + 1]))) for i, (g, p) in enumerate(zip(rec["gt_count"], rec["pair_count"]))]


def np_fold(rec, num_rel, mode, mutation=None):
    """The reference's accumulation over a set of records, in its own form: lists over the evaluated images, np.mean at the end.
    mutation: one of MUTATIONS, a wrong restatement that the cases must tell from the right one."""
    C = num_rel
    hit_k = (lambda r, k: r <= k) if mutation == "le_k" else (lambda r, k: r < k)
    lists = {n: {k: [] for k in KS} for n in ("recall", "recall_nogc", "zeroshot_recall", "acc_hit", "acc_cnt", "acc_ratio")}
    coll = {n: {k: [[] for _ in range(C)] for k in KS} for n in ("mean_recall", "ng_mean_recall")}
    n_eval = n_zs = 0
    for G, P, sl in _images_of(rec):
        if G == 0 or P == 0:      # vg_eval.py:474, :548
            continue
        n_eval += 1
        gc, ng, ac = rec["gc_rank"][sl], rec["ng_rank"][sl], rec["acc_rank"][sl]
        zs, pred = rec["zeroshot_flag"][sl] != 0, rec["gt_predicate"][sl].astype(np.int64)
        n_zs += bool(zs.any())
        inside = (pred >= 1) & (pred < C)      # a predicate outside 1..C-1 counts for no class
        cnt = np.bincount(pred[inside], minlength=C)
        for k in KS:
            hit, nghit = hit_k(gc, k), hit_k(ng, k)
            lists["recall"][k].append(float(hit.sum()) / float(G))
            lists["recall_nogc"][k].append(float(nghit.sum()) / float(G))
            if zs.any():
                lists["zeroshot_recall"][k].append(float((hit & zs).sum()) / float(zs.sum()))
            elif mutation == "zeroshot_all_images":
                lists["zeroshot_recall"][k].append(0.0)
            if mode != "sgdet":
                lists["acc_hit"][k].append(float(hit_k(ac, k).sum()))
                lists["acc_cnt"][k].append(float(G))
                lists["acc_ratio"][k].append(float(hit_k(ac, k).sum()) / float(G))
            for name, h in (("mean_recall", hit), ("ng_mean_recall", nghit)):
                hc = np.bincount(pred[inside & h], minlength=C)
                for n in range(1, C):
                    if cnt[n] > 0:
                        coll[name][k][n].append(float(hc[n]) / float(cnt[n]))
                    elif mutation == "class_all_images":
                        coll[name][k][n].append(0.0)
    res = {"images_evaluated": n_eval, "images_with_zeroshot": n_zs}
    for name in ("recall", "recall_nogc", "zeroshot_recall"):
        res[name] = {k: (float(np.mean(v)) if len(v) else float("nan")) for k, v in lists[name].items()}
        res[name + "_list"] = lists[name]
    if mutation == "acc_ratio_mean":
        res["accuracy"] = {k: (float(np.mean(lists["acc_ratio"][k])) if lists["acc_ratio"][k] else float("nan")) for k in KS}
    else:
        res["accuracy"] = {k: (float(np.mean(lists["acc_hit"][k]) / np.mean(lists["acc_cnt"][k])) if lists["acc_cnt"][k] else float("nan"))
                           for k in KS}
    for name in ("mean_recall", "ng_mean_recall"):
        res[name + "_list"] = {k: [float(np.mean(coll[name][k][n])) if coll[name][k][n] else 0.0 for n in range(1, C)] for k in KS}
        res[name] = {k: sum(res[name + "_list"][k]) / float(C - 1) for k in KS}
    return res


def np_fold_chunked(rec, num_rel, mode, images_per_chunk):
    """The scalars and per-class lists of np_fold in the device's documented summation order: chunks of `images_per_chunk`
    images (unevaluated ones hold their place), each added in image order from 0.0, the chunk sums added in chunk order from
    0.0.  Plain Python floats: IEEE double add and divide, nothing fused."""
    C = num_rel
    imgs = _images_of(rec)
    n_q = 15 + 7 * C
    total = [0.0] * n_q
    for c0 in range(0, len(imgs), images_per_chunk):
        part = [0.0] * n_q
        for G, P, sl in imgs[c0:c0 + images_per_chunk]:
            if G == 0 or P == 0:
                continue
            ranks = (rec["gc_rank"][sl], rec["ng_rank"][sl], rec["acc_rank"][sl])
            zs, pred = rec["zeroshot_flag"][sl] != 0, rec["gt_predicate"][sl].astype(np.int64)
            n_zs = int(zs.sum())
            for i, k in enumerate(KS):
                part[i] += float((ranks[0] < k).sum()) / float(G)
                part[3 + i] += float((ranks[1] < k).sum()) / float(G)
                if n_zs:
                    part[6 + i] += float(((ranks[0] < k) & zs).sum()) / float(n_zs)
                part[9 + i] += float((ranks[2] < k).sum())
            part[12] += float(G)
            part[13] += 1.0
            part[14] += 1.0 if n_zs else 0.0
            inside = (pred >= 1) & (pred < C)
            cnt = np.bincount(pred[inside], minlength=C)
            for n in np.nonzero(cnt)[0]:
                for kind in range(2):
                    for i, k in enumerate(KS):
                        part[15 + (kind * 3 + i) * C + n] += float((pred[inside & (ranks[kind] < k)] == n).sum()) / float(cnt[n])
                part[15 + 6 * C + n] += 1.0
        total = [t + p for t, p in zip(total, part)]
    nan = float("nan")
    n_eval, n_zs = total[13], total[14]
    res = {"images_evaluated": int(n_eval), "images_with_zeroshot": int(n_zs)}
    for j, name in enumerate(("recall", "recall_nogc")):
        res[name] = {k: (total[3 * j + i] / n_eval if n_eval else nan) for i, k in enumerate(KS)}
    res["zeroshot_recall"] = {k: (total[6 + i] / n_zs if n_zs else nan) for i, k in enumerate(KS)}
    res["accuracy"] = {k: ((total[9 + i] / n_eval) / (total[12] / n_eval) if n_eval and mode != "sgdet" else nan) for i, k in enumerate(KS)}
    for kind, name in enumerate(("mean_recall", "ng_mean_recall")):
        res[name + "_list"] = {}
        for i, k in enumerate(KS):
            base = 15 + (kind * 3 + i) * C
            res[name + "_list"][k] = [total[base + n] / total[15 + 6 * C + n] if total[15 + 6 * C + n] else 0.0 for n in range(1, C)]
        res[name] = {k: sum(res[name + "_list"][k], 0.0) / float(C - 1) for k in KS}
    return res


# ---- hand-made records ---------------------------------------------------------------------------------------------------
def random_image(seed, tag, G, num_rel, zs_frac=0.3, pred=None):
    """One evaluated image's rows: ranks spread over 0..139 with a quarter unmatched, so every K separates something."""
    def ranks(name):
        r = synth.integers(seed, "%s.%s" % (tag, name), (G,), 0, 140).astype(np.int64)
        miss = synth.uniform01(seed, "%s.%s.miss" % (tag, name), G) < 0.25
        return np.where(miss, NO_MATCH, r)
    return {"gc_rank": ranks("gc"), "ng_rank": ranks("ng"), "acc_rank": ranks("acc"),
            "zeroshot_flag": (synth.uniform01(seed, tag + ".zs", G) < zs_frac).astype(np.int64),
            "gt_predicate": synth.integers(seed, tag + ".pred", (G,), 1, num_rel).astype(np.int64) if pred is None
            else np.full(G, pred, np.int64)}


def records_of(images):
    """images: a list of (rows dict or None, G, P); None rows of an unevaluated image are filled with what the device holds."""
    cols = {name: [] for name in FIELDS}
    for rows, G, P in images:
        for name in FIELDS:
            cols[name].append(np.asarray(rows[name], np.int64) if rows is not None
                              else np.full(G, 0 if name in ("zeroshot_flag", "gt_predicate") else NO_MATCH, np.int64))
    return make_records([g for _, g, _ in images], [p for _, _, p in images],
                        **{k: np.concatenate(v) if v else np.zeros(0) for k, v in cols.items()})


def random_split(seed, tag, sizes, num_rel, unevaluated=(), zs_frac=0.3):
    """len(sizes) images of the given GT-relation counts; unevaluated: {image: 'G0' (no GT relation) | 'P0' (GT relations, no pair)}."""
    images = []
    for i, G in enumerate(sizes):
        how = dict(unevaluated).get(i)
        if how == "G0":
            images.append((None, 0, 7))
        elif how == "P0":
            images.append((random_image(seed, "%s.%d" % (tag, i), G, num_rel, zs_frac), G, 0))      # rows the fold must not read into a result
        else:
            images.append((random_image(seed, "%s.%d" % (tag, i), G, num_rel, zs_frac), G, 11))
    return records_of(images)


def fold_cases(c, max_cls):
    """name -> (records, num_rel, mode), on the fold's own boundaries: c = images_per_chunk, max_cls = max_rel_cls."""
    cases = {}
    sizes = lambda n: [1 + (i * 5) % 9 for i in range(n)]
    for n in (1, c - 1, c, c + 1, 2 * c + 1):
        cases["n_img_%d" % n] = (random_split(5, "n%d" % n, sizes(n), 51), 51, "sgcls")
    n = 3 * c + 2
    cases["unevaluated_first_last"] = (random_split(6, "ufl", sizes(n), 51, {0: "G0", 1: "P0", n - 2: "P0", n - 1: "G0"}), 51, "predcls")
    cases["unevaluated_whole_chunk"] = (random_split(7, "uwc", sizes(n), 51, {i: ("G0" if i % 2 else "P0") for i in range(c, 2 * c)}),
                                        51, "predcls")
    cases["all_unevaluated"] = (random_split(8, "all", sizes(c + 3), 51, {i: ("G0" if i % 3 else "P0") for i in range(c + 3)}), 51, "sgcls")
    cases["image_sizes"] = (random_split(9, "sz", [1, 63, 64, 65, 3000, 2, 1025], 51), 51, "sgcls")
    cases["one_predicate"] = (records_of([(random_image(10, "op.%d" % i, G, 51, pred=p), G, 5) for i, (G, p) in
                                          enumerate([(70, 7), (1, 7), (9, 50), (12, 1)])]), 51, "predcls")
    edge = np.array([19, 20, 49, 50, 99, 100, NO_MATCH, 0], np.int64)      # exactly at every K, one below, none, first
    rows = {"gc_rank": edge, "ng_rank": edge[::-1].copy(), "acc_rank": np.roll(edge, 3), "zeroshot_flag": np.array([1, 1, 0, 1, 0, 1, 1, 0]),
            "gt_predicate": np.array([1, 1, 2, 2, 3, 3, 4, 4])}
    cases["ranks_at_k"] = (records_of([(rows, 8, 3)]), 6, "predcls")      # predicate 5: no image has it -> list entry 0.0
    cases["no_zeroshot"] = (random_split(11, "nz", sizes(c + 5), 51, zs_frac=0.0), 51, "sgcls")
    out = random_image(12, "out", 40, 11)
    out["gt_predicate"] = np.array(([0, -3, 11, 12, 2 ** 31 - 1, 5, 10, 1] * 5), np.int64)
    cases["predicate_outside"] = (records_of([(out, 40, 9), (random_image(12, "out2", 6, 11), 6, 2)]), 11, "sgcls")
    cases["two_classes"] = (random_split(13, "c2", sizes(c + 1), 2), 2, "predcls")
    cases["max_classes"] = (random_split(14, "cmax", [40, 900, 3, 2500], max_cls), max_cls, "sgcls")
    cases["sgdet"] = (random_split(15, "sgdet", sizes(2 * c + 3), 51, {4: "P0"}), 51, "sgdet")
    return cases
