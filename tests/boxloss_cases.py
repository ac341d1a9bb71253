"""What the box-loss tests and tests/golden/make_golden_boxloss.py share: the cases and their inputs (built from a seed or by
hand), the fixture loader, the float64 numpy oracle `box_loss_fp64` (FastRCNNLossComputation.__call__, loss.py:42-84: both losses
and both full gradients) and the error metrics the fixtures and the device tests are measured in.  No test lives here."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxloss")
TINY = 2.0 ** -126      # the smallest normal float: the floor of the d_class_logits metric
FULL_GRADS = 65536      # a fixture keeps every gradient row when R * 4C is at most this, else GRAD_ROWS seeded rows + the forced ones
GRAD_ROWS = 64

# seeded cases: rows per image, classes, the fraction of positive rows (None: `labels` gives them all), labels forced on the
# first rows of the first non-empty image, the logits' scale
SEEDED = {
    "vg": dict(rows=(64, 64), C=151, pos=0.25, seed=7000),
    "agnostic": dict(rows=(64, 64), C=151, pos=0.25, agnostic=True, seed=7001),
    "two_cls": dict(rows=(5,), C=2, pos=0.5, forced=(0, 1), seed=7002),
    "lanes63": dict(rows=(7,), C=63, pos=0.5, forced=(0, 62, 1), seed=7003),
    "lanes64": dict(rows=(7,), C=64, pos=0.5, forced=(0, 63, 1), seed=7004),
    "lanes65": dict(rows=(7,), C=65, pos=0.5, forced=(0, 64, 63), seed=7005),
    "wide": dict(rows=(9,), C=1024, pos=0.5, forced=(1023, 960, 0, 64), seed=7006),
    "no_pos": dict(rows=(33,), C=151, pos=0.0, seed=7007),
    "all_pos": dict(rows=(33,), C=151, pos=1.0, seed=7008),
    "ragged": dict(rows=(1, 0, 130), C=151, pos=0.25, forced=(17,), seed=7009),
    "sharp": dict(rows=(16,), C=151, pos=0.5, scale=30.0, forced=(0, 150, 3), shifted_row=2, inf_row=5, seed=7010),
}
# the residuals d = input - target of the hand-built case: both sides of |d| = beta = 1 at one ulp, the kink itself, 0, both branches
KINK_D = [0.0, 1.0, -1.0, 1.0 - 2.0 ** -23, -(1.0 - 2.0 ** -23), 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 0.5, -0.5, 3.0, -3.0]
ALL = tuple(SEEDED) + ("kink",)


def _kink():
    """R = 16 rows (a power of two: every gradient is exact in fp32), C = 2 with all-zero logits (softmax exactly 1/2), three
    positive rows carrying the eleven residuals of KINK_D and a twelfth of 0.25; targets from {0, 0.5, -1}, inputs target + d,
    each asserted exact in fp32."""
    R, C = 16, 2
    logits = np.zeros((R, C), np.float32)
    reg = np.zeros((R, 4 * C), np.float32)
    tgt = np.zeros((R, 4), np.float32)
    labels = np.zeros(R, np.int64)
    ds = KINK_D + [0.25]
    for k, d in enumerate(ds):
        r, c = (1, 6, 11)[k // 4], k % 4
        labels[r] = 1
        for t in ((0.0, 0.5, -1.0)[k % 3], 0.0, 0.5, -1.0):
            x = np.float32(t + d)
            if float(x) - t == d:
                break
        else:
            raise AssertionError("no exact target for d = %r" % d)
        tgt[r, c], reg[r, 4 + c] = t, x
    # the unused columns of class 0 carry values the loss must not read
    reg[:, :4] = 7.0
    return dict(class_logits=[logits], box_regression=[reg], labels=[labels], regression_targets=[tgt], agnostic=False, forced_rows=[1, 6, 11])


def case_inputs(name):
    """dict(class_logits, box_regression, labels, regression_targets: per-image lists of numpy arrays; agnostic; forced_rows: the
    hand-set rows inside the concatenated batch)."""
    if name == "kink":
        return _kink()
    c = SEEDED[name]
    rng = np.random.RandomState(c["seed"])
    C, agnostic = c["C"], bool(c.get("agnostic"))
    cols = 8 if agnostic else 4 * C
    out = dict(class_logits=[], box_regression=[], labels=[], regression_targets=[], agnostic=agnostic, forced_rows=[])
    forced, row0 = list(c.get("forced", ())), 0
    for n in c["rows"]:
        logits = (rng.standard_normal((n, C)) * c.get("scale", 1.0)).astype(np.float32)
        reg = (rng.standard_normal((n, cols)) * 0.7).astype(np.float32)
        tgt = (rng.standard_normal((n, 4)) * 0.7).astype(np.float32)
        labels = np.where(rng.random_sample(n) < c["pos"], rng.randint(1, C, n), 0).astype(np.int64)
        if forced and n >= len(forced):
            labels[:len(forced)] = forced
            out["forced_rows"] += list(range(row0, row0 + len(forced)))
            forced = []
        if n and "shifted_row" in c:
            logits[c["shifted_row"]] += np.float32(1e4)       # an exponential without max subtraction overflows
            r = c["inf_row"]
            logits[r, (labels[r] + 7) % C] = -np.inf           # a non-label class: finite loss, exactly 0 gradient there
            out["forced_rows"] += [row0 + c["shifted_row"], row0 + r]
        for k, v in (("class_logits", logits), ("box_regression", reg), ("labels", labels), ("regression_targets", tgt)):
            out[k].append(v)
        row0 += n
    assert not forced, name
    return out


def concatenated(d):
    """(class_logits [R, C], box_regression, labels, regression_targets) of a case, the images concatenated."""
    return tuple(np.concatenate(d[k]) for k in ("class_logits", "box_regression", "labels", "regression_targets"))


def seeded_batch(seed, R, C, pos=0.25):
    """One image of R rows for the launch-shape tests: (class_logits, box_regression [R, 4C], labels, regression_targets)."""
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((R, C)).astype(np.float32)
    reg = (rng.standard_normal((R, 4 * C)) * 0.7).astype(np.float32)
    tgt = (rng.standard_normal((R, 4)) * 0.7).astype(np.float32)
    labels = np.where(rng.random_sample(R) < pos, rng.randint(1, C, R), 0).astype(np.int64)
    return logits, reg, labels, tgt


def grad_rows(name, d):
    """The rows whose float64 gradients a fixture keeps."""
    logits = np.concatenate(d["class_logits"])
    R, C = logits.shape
    if R * 4 * C <= FULL_GRADS:
        return np.arange(R)
    picked = np.random.RandomState(SEEDED[name]["seed"] + 500).choice(R, GRAD_ROWS, replace=False)
    return np.unique(np.concatenate([picked, np.asarray(d["forced_rows"], np.int64)]))


def load_case(name):
    """(fixture, inputs): the inputs are regenerated from this module."""
    return np.load(os.path.join(GOLDEN, name + ".npz")), case_inputs(name)


# ---- the float64 oracle -------------------------------------------------------------------------------------------------------

def box_loss_fp64(class_logits, box_regression, labels, regression_targets, agnostic=False, beta=1.0, box_norm="rows", ce_over="rows"):
    """loss.py:42-84 in numpy float64 on the given (fp32) inputs: dict(losses [2], d_class_logits [R, C], d_box_regression, p
    (the softmax), onehot).  beta, box_norm ('rows' | 'positives') and ce_over ('rows' | 'positives') exist so that the host test
    can show that a wrong restatement changes the result; the defaults are the reference."""
    z = np.asarray(class_logits, np.float64)
    x = np.asarray(box_regression, np.float64)
    y = np.asarray(labels, np.int64)
    t = np.asarray(regression_targets, np.float64)
    R, C = z.shape
    rows = np.arange(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        if R:
            m = z.max(1, keepdims=True)
            e = np.exp(z - m)
            s = e.sum(1, keepdims=True)
            p = e / s
            ce = (m[:, 0] + np.log(s[:, 0])) - z[rows, y]
        else:
            p, ce = np.zeros((0, C)), np.zeros(0)
        onehot = np.zeros((R, C))
        onehot[rows, y] = 1.0
        pos = y > 0
        n_ce = R if ce_over == "rows" else int(pos.sum())
        w = np.ones(R) if ce_over == "rows" else pos.astype(np.float64)
        cls_loss = (ce * w).sum() / n_ce if n_ce else np.nan
        d_logits = (p - onehot) * w[:, None] / n_ce if n_ce else np.zeros((R, C))
        cols = (np.full(R, 4) if agnostic else 4 * y)[:, None] + np.arange(4)[None, :]
        d = np.zeros((R, 4))
        d[pos] = x[rows[pos, None], cols[pos]] - t[pos]
        n = np.abs(d)
        terms = np.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta) * pos[:, None]
        n_box = R if box_norm == "rows" else int(pos.sum())
        box_loss = terms.sum() / n_box if n_box else np.nan
        g = np.where(n < beta, d / beta, np.sign(d)) * pos[:, None] / max(n_box, 1)
        d_reg = np.zeros(x.shape)
        d_reg[rows[pos, None], cols[pos]] = g[pos]
    return dict(losses=np.array([cls_loss, box_loss]), d_class_logits=d_logits, d_box_regression=d_reg, p=p, onehot=onehot)


# ---- the metrics ----------------------------------------------------------------------------------------------------------------

def loss_err(got, want):
    """Largest relative error of the two losses; a loss the oracle has as exactly 0 must be exactly 0."""
    err = 0.0
    for g, w in zip(np.asarray(got, np.float64), np.asarray(want, np.float64)):
        if w == 0:
            assert g == 0, "a loss of exactly 0 came out as %r" % g
        else:
            err = max(err, abs(g - w) / abs(w))
    return err


def dbox_err(got, want):
    """d_box_regression: the largest relative error at the elements the oracle's gradient touches; exactly 0 everywhere else and
    non-zero where the oracle's is (asserted)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    hit = want != 0
    assert not got[~hit].any(), "a gradient outside the oracle's elements"
    assert got[hit].all(), "a zero where the oracle's gradient is not"
    return float((np.abs(got[hit] - want[hit]) / np.abs(want[hit])).max()) if hit.any() else 0.0


def dlogits_err(got, want, p, onehot, R=None):
    """d_class_logits in units of the terms' magnitude before their cancellation: the largest of
    (|g - g64| - 2^-126) / ((p + onehot) / R), so that `err <= b` reads |g - g64| <= b (p + onehot) / R + 2^-126 element by element.
    Where p + onehot is 0 (a -inf logit) the difference must be within the floor (asserted)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    R = max(p.shape[0] if R is None else R, 1)   # (R: the batch, when only some of its rows are given)
    mag = (p + onehot) / R
    over = np.maximum(np.abs(got - want) - TINY, 0.0)
    assert not over[mag == 0].any(), "a gradient where the probability is exactly 0"
    live = mag > 0
    return float((over[live] / mag[live]).max()) if live.any() else 0.0
