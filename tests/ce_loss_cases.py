"""Cases, the float64 restatement and the per-element error bounds of the relation loss veto_ce_loss (veto_amd/csrc/losses.hip:
ce_rows_kernel, ce_reduce_kernel, ce_grad_kernel).  CPU only, no test lives here: tests/test_ce_loss_host.py checks the premises of
every case, pins the restatement to torch and shows that wrong restatements leave the bounds; tests/test_ce_loss_gpu.py runs the
cases through the C ABI and through veto_amd.losses.

The reference.  ce_fp64 is nn.CrossEntropyLoss(weight)(logits[rows], labels), mean reduction, in float64 numpy, written as torch
computes it: logp = (z - max z) - log sum exp(z - max z), loss = sum_i w[y_i] (-logp_i[y_i]) / sum_i w[y_i] over the valid rows,
d loss / d z_i = w[y_i] / W (exp(logp_i) - e_{y_i}).  A negative label is an ignored row (weight 0, gradient exactly 0); a label
>= C (torch raises) makes the loss NaN and its gradient row NaN and otherwise counts as weight 0.  The non-finite answers are
torch's: no valid row or a weight sum of 0 gives a NaN loss (and NaN gradient rows for the valid rows, 0 for ignored ones); a -inf
label logit gives loss +inf and a finite gradient with -w/W at the label; an all -inf row or a +inf logit gives a NaN loss and a
NaN gradient row.

Error model.  u = 2^-24 is the unit roundoff of float32, gamma(k) = k u / (1 - k u).  Per row, with x_c = z_c - mx (exact in
float64 from the float32 inputs), e_c = exp(x_c), S = sum e_c, p_c = e_c / S, nll = log S - x_y, T = ceil(C / 64), s = w / W:
  d_c   = fl(z_c - mx)                 one rounding: |d_c - x_c| <= u |x_c| (mx itself is exact: a maximum of inputs)
  expf(d_c)                            ULP relative: 2 ULP u_f = 2 * 2^-23 = 4 u, plus 2 * 2^-149 absolute where the result is subnormal
  sum                                  T lane-serial adds (the first onto 0 is exact) and the 6 steps of the wave sum, all terms
                                       positive: relative gamma(T + 5)
    => rel_S = sum_c e_c (u |x_c| + 4 u + gamma(T + 5)) / S + C 2^-148 / S
  logf(sum)                            2 ULP = 4 u relative:  dL = 4 u |log S| + rel_S
  nll   = fl(log_sum - d_y)            u |x_y| inherited from d_y, one rounding u nll
  nll_w = fl(w nll)                    one rounding u w nll
    => row bound  B = K w (dL + u |x_y| + 2 u nll) + 2^-149
  loss  = float(num / den)             the fold is in double (n 2^-53 relative, counted), one float32 rounding of the quotient:
    => |loss - loss64| <= sum_i B_i / W + n 2^-53 sum_i |w_i nll_i| / W + u |loss64|
  scale = fl(w_row fl(1 / W))          2 u relative
  a_c   = fl(d_c - log_sum)            u |x_c| + dL inherited, one rounding u |x_c - log S|
  p_c   = expf(a_c)                    4 u relative (+ 2 * 2^-149 absolute where subnormal)
    => E_c = u |x_c| + dL + u |x_c - log S| + 4 u  relative on p_c
  g_c   = fl(fl(p_c - 1[c = y]) scale) the subtraction rounds only at c = y (u |p_y - 1|); the product u; the scale 2 u
    => |g_c - g64_c| <= K s (p_c E_c + 1[c = y] u |p_c - 1| + 3 u |p_c - 1[c = y]|) + s 2^-148 + 2^-149
K = 1 + 2^-10 covers the second-order terms.  Nothing in these bounds depends on the offset of a row's logits: only x = z - mx enters.
The ULP figures of expf and logf: the device math library's accuracy table is not among the documents installed with the toolchain, so
both are taken at 2 ULP (the HIP math API documents 1 ULP for each; profiles/ce_loss_parity.txt records what was measured)."""
import os

import numpy as np

U = 2.0 ** -24
K2 = 1.0 + 2.0 ** -10
SUB = 2.0 ** -149
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFFSETS = (0.0, 16.0, 100.0, 1e3, 1e4, -1e4)
WIDTHS = (2, 6, 21, 51, 63, 64, 65, 101, 128, 129, 151, 201, 1024)
ROW_COUNTS = (1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 15120)
FOLD_ROWS = 200003


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def _case(name, event, logits, labels, weight=None, rows=None, ld=None, **extra):
    logits = np.ascontiguousarray(logits, np.float32)
    c = dict(name=name, event=event, logits=logits, labels=np.asarray(labels, np.int64), ld=int(ld or logits.shape[1]),
             weight=None if weight is None else np.asarray(weight, np.float32), rows=None if rows is None else np.asarray(rows, np.int64))
    c.update(extra)
    return c


def beta_weights():
    """The BETA_LOSS class weights (roi_relation_predictors.py:4058-4066) of the 51 predicate counts of tests/golden/pred_counts.txt."""
    from veto_amd import predictor
    return predictor.class_balanced_weights(np.loadtxt(os.path.join(GOLDEN, "pred_counts.txt")), 51).numpy()


def span_weights(C, seed):
    """Class weights spanning 1e-6 .. 1e3, both ends present."""
    w = 10.0 ** np.random.RandomState(seed).uniform(-6, 3, C)
    w[0], w[C - 1] = 1e-6, 1e3
    return w.astype(np.float32)


def width_labels(C):
    """The forced labels of a class-width case: first and last column, lane 0 of the last trip, lane 63 of the last trip that has one."""
    last = 64 * ((C - 1) // 64)
    lane63 = last + 63 if last + 63 < C else max(last - 1, 0)
    return [0, C - 1, last, lane63]


def _width(C):
    rng = np.random.RandomState(9000 + C)
    n = 9
    labels = rng.randint(0, C, n)
    labels[:4] = width_labels(C)
    return _case("width_%d" % C, "C = %d: %d trip(s) of the lane loop, the last with %d lanes" % (C, -(-C // 64), (C - 1) % 64 + 1),
                 rng.standard_normal((n, C)) * 2.0, labels, weight=span_weights(C, C) if C % 2 else None)


def _rows_n(n):
    rng = np.random.RandomState(9100 + n % 9973)
    per = -(-n // 256)
    labels = rng.randint(0, 51, n)
    if n >= 255:
        labels[rng.choice(n, n // 16, replace=False)] = -100
    return _case("rows_%d" % n, "n = %d: %d workgroup(s), per = %d, %d empty reduce threads" % (n, -(-n // 4), per, 256 - -(-n // per)),
                 rng.standard_normal((n, 51)) * 2.0, labels, weight=beta_weights() if n == 15120 else None)


def _fold():
    """Row 0: class 0 of weight 1000 with its label logit 10 below the maximum (weighted term near 1e4).  Every other row: weight 1,
    label logit 10.5 above 50 logits near 0 (term near 1.4e-3, under 1.5 ulp of 1e4: a float32 accumulator that holds row 0 takes
    each as ONE ulp, 9.77e-4)."""
    rng = np.random.RandomState(9200)
    n, C = FOLD_ROWS, 51
    z = (rng.standard_normal((n, C)) * 0.01).astype(np.float32)
    labels = rng.randint(1, C, n)
    z[np.arange(n), labels] = 10.5
    labels[0] = 0
    z[0] = 0.0
    z[0, 0], z[0, 7] = -2.0, 8.0
    w = np.ones(C, np.float32)
    w[0] = 1000.0
    return _case("fold_200003", "one weighted term near 1e4 in front of 200002 near 1.4e-3", z, labels, weight=w)


def offset_base():
    """64 x 51 logits: rows 0..15 on the grid of eighths in [-8, 8] (every shifted value is exact in float32 up to |offset| = 1e4),
    rows 16..63 drawn from N(0, 2^2)."""
    rng = np.random.RandomState(9300)
    z = (rng.standard_normal((64, 51)) * 2.0).astype(np.float32)
    z[:16] = np.round(np.clip(z[:16], -8, 8) * 8) / 8
    labels = rng.randint(0, 51, 64)
    return z, labels, span_weights(51, 9301)


OFFSET_GRID_ROWS = 16


def _offset(off):
    z, labels, w = offset_base()
    return _case("offset_%g" % off, "every logit shifted by %g" % off, z + np.float32(off), labels, weight=w, offset=off)


def _sharp(name, gap, event):
    """C = 51, 8 rows: column 5 is `gap` above the other logits (small values on the grid of eighths); the label is on the dominant
    column in even rows and off it in odd rows."""
    rng = np.random.RandomState(9400)
    z = np.round(rng.uniform(-1, 1, (8, 51)) * 8) / 8
    z[:, 5] = gap
    labels = np.where(np.arange(8) % 2 == 0, 5, rng.randint(6, 51, 8))
    return _case(name, event, z, labels, gap=gap)


def _nonfinite(name, event, kind):
    rng = np.random.RandomState(9500)
    z = (rng.standard_normal((12, 51)) * 2.0).astype(np.float32)
    labels = rng.randint(0, 51, 12)
    if kind == "neginf_label":
        z[5, labels[5]] = -np.inf
    elif kind == "all_neginf":
        z[5] = -np.inf
    elif kind == "posinf":
        z[5, (labels[5] + 3) % 51] = np.inf
    elif kind == "neginf_other":
        z[5, (labels[5] + 3) % 51] = -np.inf
    return _case(name, event, z, labels, weight=span_weights(51, 9501), special_row=5)


def _labels(name, event, kind):
    rng = np.random.RandomState(9600)
    C, n = 21, 13
    z = (rng.standard_normal((n, C)) * 2.0).astype(np.float32)
    labels = rng.randint(0, C, n)
    w = (rng.uniform(0.1, 2.0, C)).astype(np.float32)
    if kind == "ignored":
        labels[[2, 6, 11]] = (-1, -100, -2 ** 40)
    elif kind == "bad_C":
        labels[4], labels[9] = C, -100
    elif kind == "bad_2p40":
        labels[4] = 2 ** 40
    elif kind == "all_ignored":
        labels[:] = -100
        labels[3], labels[8] = -1, -2 ** 40
    elif kind == "zero_weight":
        w[:5] = 0.0
        labels = rng.randint(0, 5, n)
        labels[[1, 7]] = -100
    elif kind == "tiny_weight":
        w[:5] = 0.0
        w[5] = 1e-30
        labels = rng.randint(0, 5, n)
        labels[6] = 5
    return _case(name, event, z, labels, weight=w)


def _weights(kind):
    rng = np.random.RandomState(9700)
    z = (rng.standard_normal((130, 51)) * 2.0).astype(np.float32)
    labels = rng.randint(0, 51, 130)
    labels[:2] = (0, 50)
    w = {"none": None, "beta": beta_weights(), "span": span_weights(51, 9701)}[kind]
    return _case("weight_" + kind, "class weights: " + kind, z, labels, weight=w)


def _indirect(name, event, C, m, ld, rows):
    rng = np.random.RandomState(9800 + len(name))
    rows = np.asarray(rows, np.int64)
    labels = rng.randint(0, C, len(rows))
    return _case(name, event, rng.standard_normal((m, C)) * 2.0, labels, rows=rows, ld=ld, weight=span_weights(C, 9801) if C == 151 else None)


def _build():
    rng = np.random.RandomState(9900)
    cases = [_width(C) for C in WIDTHS] + [_rows_n(n) for n in ROW_COUNTS] + [_fold()] + [_offset(o) for o in OFFSETS]
    cases += [
        _case("flat", "all logits of a row equal", np.repeat(np.array([[3.25], [-7.5], [0.0], [1e4]], np.float32), 51, 1), [0, 50, 17, 33]),
        _sharp("gap_30", 30.0, "one dominant logit, gap 30: log sum rounds to 0 in float32"),
        _sharp("gap_200", 200.0, "gap 200: the float32 softmax is exactly one-hot"),
        _sharp("subnormal_p", 95.0, "gap 95: the other probabilities are float32 subnormals"),
        _nonfinite("neginf_label", "a -inf label logit: loss +inf, finite gradient with -w/W at the label", "neginf_label"),
        _nonfinite("neginf_other", "a -inf logit off the label: finite loss, exactly 0 gradient there", "neginf_other"),
        _nonfinite("all_neginf_row", "a row of -inf: NaN loss, NaN gradient row", "all_neginf"),
        _nonfinite("posinf_logit", "a +inf logit: NaN loss, NaN gradient row", "posinf"),
        _labels("ignored_labels", "labels -1, -100 and -2^40 are ignored", "ignored"),
        _labels("bad_label_C", "label == C: NaN loss, NaN gradient row", "bad_C"),
        _labels("bad_label_2p40", "label 2^40: NaN loss, NaN gradient row", "bad_2p40"),
        _labels("all_ignored", "every label negative: NaN loss, gradient exactly 0", "all_ignored"),
        _labels("zero_weight_valid", "every valid row on a zero-weight class: NaN like torch", "zero_weight"),
        _labels("tiny_weight_row", "one row of weight 1e-30 among zero-weight rows", "tiny_weight"),
        _weights("none"), _weights("beta"), _weights("span"),
        _indirect("rows_perm_ld_plus3", "rows a permutation, ld = C + 3", 21, 37, 24, rng.permutation(37)),
        _indirect("rows_repeats_ld_4c", "rows with repeats out of a larger table, ld = 4 C", 151, 40, 604, rng.randint(0, 40, 23)),
        _indirect("rows_one_row_n_times", "rows picks logit row 7 n = 9 times", 21, 12, 24, np.full(9, 7)),
        _indirect("rows_len1", "rows of length 1", 151, 6, 604, [4]),
    ]
    return {c["name"]: c for c in cases}


_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(_build())
    return _CASES


def names():
    return list(cases())


make_case = _case
_REF = {}


def ref_and_bounds(name):
    """(case, ce_fp64(case), bounds(case)), computed once and shared by every test that needs them."""
    if name not in _REF:
        c = cases()[name]
        r = ce_fp64(c)
        _REF[name] = (c, r, bounds(c, r))
    return _REF[name]


def selected(c):
    """The [n, C] logits the labels are aligned with."""
    return c["logits"] if c["rows"] is None else c["logits"][c["rows"]]


NAN_PATTERN = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]


def logits_buffer(c):
    """The [m, ld] buffer handed to the C ABI: the NaN pattern in the padding columns and in every row `rows` does not select."""
    m, C = c["logits"].shape
    buf = np.full((m, c["ld"]), NAN_PATTERN, np.float32)
    used = np.arange(m) if c["rows"] is None else np.unique(c["rows"])
    buf[used, :C] = c["logits"][used]
    return buf


# ---- the float64 restatement and its intermediate quantities ----------------------------------------------------------------------

def ce_fp64(c):
    """dict(loss, grad [n, C] float64, valid, ignored, bad [n] bool, and the per-row quantities the bounds are made of)."""
    z = selected(c).astype(np.float64)
    y = c["labels"]
    n, C = z.shape
    ignored, bad = y < 0, y >= C
    valid = ~ignored & ~bad
    yy = np.where(valid, y, 0)
    w = np.where(valid, (np.ones(C) if c["weight"] is None else c["weight"].astype(np.float64))[yy], 0.0)
    with np.errstate(all="ignore"):
        mx = z.max(1, keepdims=True)
        x = z - mx
        e = np.exp(x)
        S = e.sum(1)
        logS = np.log(S)
        logp = x - logS[:, None]
        nll = -logp[np.arange(n), yy]
        W = w.sum()
        terms = np.where(valid, w * nll, 0.0)
        terms[bad] = np.nan
        loss = terms.sum() / W
        onehot = np.zeros((n, C))
        onehot[np.arange(n)[valid], y[valid]] = 1.0
        p = np.exp(logp)
        grad = (w / W)[:, None] * (p - onehot)
        grad[ignored] = 0.0
        grad[bad] = np.nan
    return dict(loss=float(loss), grad=grad, valid=valid, ignored=ignored, bad=bad, w=w, W=W, x=x, e=e, S=S, logS=logS, p=p, nll=nll,
                onehot=onehot, yy=yy)


def bounds(c, ref=None):
    """(loss bound, gradient bound [n, C]) from the docstring's formulas; entries of rows whose reference is not finite mean nothing."""
    r = ref or ce_fp64(c)
    n, C = r["x"].shape
    T = -(-C // 64)
    with np.errstate(all="ignore"):
        ax = np.where(r["e"] > 0, np.abs(r["x"]), 0.0)
        rel_S = (r["e"] * (U * ax + 4 * U + gamma(T + 5))).sum(1) / r["S"] + C * 2 * SUB / r["S"]
        dL = 4 * U * np.abs(r["logS"]) + rel_S
        xy = np.abs(r["x"][np.arange(n), r["yy"]])
        B = K2 * r["w"] * (dL + U * xy + 2 * U * r["nll"]) + SUB
        B = np.where(r["valid"], B, 0.0)
        absterms = np.where(r["valid"], np.abs(r["w"] * r["nll"]), 0.0)
        loss_bound = B.sum() / r["W"] + n * 2.0 ** -53 * absterms.sum() / r["W"] + U * abs(r["loss"])
        s = (r["w"] / r["W"])[:, None]
        E = U * ax + dL[:, None] + U * np.where(r["p"] > 0, np.abs(r["x"] - r["logS"][:, None]), 0.0) + 4 * U
        pm = np.abs(r["p"] - r["onehot"])
        gb = K2 * s * (np.where(r["p"] > 0, r["p"] * E, 0.0) + r["onehot"] * U * pm + 3 * U * pm) + s * 2 * SUB + SUB
        gb[r["ignored"]] = 0.0
    return float(loss_bound), gb


def measure(c, loss, grad, ref=None, bnd=None):
    """(loss error / bound, worst gradient error / bound) of a float32 result.  A NaN or inf where the reference has none (or the
    reverse), or an ignored row that is not all +0, is an infinite ratio."""
    r = ref or ce_fp64(c)
    lb, gb = bnd or bounds(c, r)
    loss, grad = float(np.asarray(loss).reshape(-1)[0]), np.asarray(grad)
    if np.isnan(r["loss"]) or np.isinf(r["loss"]):
        lr = 0.0 if (np.isnan(loss) if np.isnan(r["loss"]) else loss == r["loss"]) else np.inf
    else:
        lr = abs(loss - r["loss"]) / lb if np.isfinite(loss) else np.inf
    gr = 0.0
    if grad is not None:
        assert grad.dtype == np.float32 and grad.shape == r["grad"].shape
        if r["ignored"].any() and grad[r["ignored"]].view(np.uint32).any():
            gr = np.inf
        fin = np.isfinite(r["grad"])
        if not np.array_equal(np.isnan(grad), np.isnan(r["grad"])) or np.isinf(grad).any():
            gr = np.inf
        live = fin & ~r["ignored"][:, None]
        if live.any() and np.isfinite(gr):
            with np.errstate(all="ignore"):
                gr = max(gr, float((np.abs(grad.astype(np.float64)[live] - r["grad"][live]) / gb[live]).max()))
    return lr, gr


# ---- the kernel's arithmetic in numpy float32, and its wrong variants -----------------------------------------------------------------

# f32_fold: ONE float32 accumulator over the rows in index order (the plain float fold).  f32_fold_split: ce_reduce_kernel's own
# two-level shape with float accumulators -- only the 782 rows of the thread that holds the large term lose their small terms, so it
# leaves the bound of the fold case by less (the host test asserts that it does leave it).
FORMS = ("fixed", "single_lse", "no_max", "mean_n", "ignored_in_den", "unweighted_grad", "gt_label", "f32_fold", "label_plus_64",
         "ignored_scaled", "f32_fold_split")
WRONG = FORMS[1:-1]


def _reduce(v, acc_type):
    """ce_reduce_kernel: thread t folds rows t per .. (t + 1) per - 1 in order, thread 0 the 256 partial sums in order."""
    n = len(v)
    per = -(-n // 256)
    a = np.zeros(256 * per, acc_type)
    a[:n] = v
    a = a.reshape(256, per)
    part = np.zeros(256, acc_type)
    for k in range(per):
        part = (part + a[:, k]).astype(acc_type)
    tot = acc_type(0)
    for t in range(256):
        tot = acc_type(tot + part[t])
    return tot


def emulate(c, form="fixed"):
    """(loss float32, grad [n, C] float32) as the kernels compute them: float32 throughout, the lane-serial sum and the wave butterfly
    in their order, the fold in double.  `form` picks the kernel as it stands ('fixed') or one deliberately wrong restatement."""
    assert form in FORMS
    f32 = np.float32
    buf = np.concatenate([logits_buffer(c).ravel(), [NAN_PATTERN]]).astype(f32)
    z = selected(c)
    y = c["labels"]
    n, C = z.shape
    rows = np.arange(n) if c["rows"] is None else c["rows"]
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(z, axis=1)
        d = z if form == "no_max" else (z - mx[:, None]).astype(f32)
        e = np.exp(d).astype(f32)
        T = -(-C // 64)
        ep = np.zeros((n, T * 64), f32)
        ep[:, :C] = e
        acc = np.zeros((n, 64), f32)
        for t in range(T):
            acc = acc + ep[:, 64 * t:64 * t + 64]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ o]
        log_sum = np.log(acc[:, 0]).astype(f32)
        top = C + 1 if form == "gt_label" else C
        ignored, bad = y < 0, y >= top
        valid = ~ignored & ~bad
        yy = np.where(valid, y, 0)
        ycol = np.where(yy + 64 < C, yy + 64, yy) if form == "label_plus_64" else yy
        zy = buf[rows * c["ld"] + ycol]                      # (the kernel's own address: a label == C reads past the row)
        wcls = np.ones(C + 1, f32) if c["weight"] is None else np.concatenate([c["weight"], [f32(1)]])
        w = np.where(valid, wcls[yy], f32(0)).astype(f32)
        if form == "single_lse":
            lse = (mx + log_sum).astype(f32)
            nll = (lse - zy).astype(f32)
            p = np.exp((z - lse[:, None]).astype(f32)).astype(f32)
        else:
            dy = zy if form == "no_max" else (zy - mx).astype(f32)
            nll = (log_sum - dy).astype(f32)
            p = np.exp((d - log_sum[:, None]).astype(f32)).astype(f32)
        nll_w = np.where(valid, (w * nll).astype(f32), f32(0)).astype(f32)
        nll_w[bad] = np.nan
        acc_type = np.float32 if form in ("f32_fold", "f32_fold_split") else np.float64
        if form == "f32_fold":
            num, den = np.add.accumulate(nll_w, dtype=f32)[-1], np.add.accumulate(w, dtype=f32)[-1]
        else:
            num, den = _reduce(nll_w, acc_type), _reduce(w, acc_type)
        if form == "mean_n":
            den = acc_type(n)
        elif form == "ignored_in_den":
            den = acc_type(den + acc_type(wcls[0]) * ignored.sum())
        loss = f32(np.float64(num) / np.float64(den))
        inv = f32(1.0 / np.float64(den))
        scale = (w * inv).astype(f32)
        if form == "unweighted_grad":
            scale = np.where(valid, inv, f32(0)).astype(f32)
        scale[bad] = np.nan
        onehot = np.zeros((n, C), f32)
        hit = valid & (ycol < C)
        onehot[np.arange(n)[hit], ycol[hit]] = 1
        grad = ((p - onehot).astype(f32) * scale[:, None]).astype(f32)
        if form != "ignored_scaled":
            grad[ignored] = 0
    return loss, grad
