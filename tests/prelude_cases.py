"""Cases and float64 restatements for the part of the eval forward outside the fused kernels: pair indices, the per-object side
(BatchNorm on running or batch statistics, box / class embeddings, patchify + the patch GEMM), token assembly and the classifier
head.  CPU only: tests/test_prelude_host.py checks the premises of every case and that deliberately wrong restatements leave the
bounds; tests/test_prelude_gpu.py runs the cases through the C ABI.

The token VALUES the device is held to come from oracle/veto_oracle.py in float64 (oracle_tokens).  restate() computes the same
rows a second time in the per-object form the kernels use (veto_amd/csrc/rowops.hip), because the error BOUNDS follow that
arithmetic, and because the wrong variants of the host test are variants of it; the host test holds the two to each other.

Reference lines restated here (relative to pysgg/modeling/roi_heads/relation_head/):
  roi_relation_predictors.py:4086-4095  object embedding (label lookup / softmax(logits) @ embedding)
  roi_relation_predictors.py:4097-4102  box features: xyxy -> xywh with the +1 convention, xywh taken as it is; BatchNorm1d(4)
  roi_relation_predictors.py:4104-4115  pair indices
  roi_relation_predictors.py:4118-4126  pair gathers, location / class projection, classifier
  model_veto.py:52-64                   patch embedding, token rows, positional embedding

Error model.  u = 2^-24 is the unit roundoff of float32, gamma(n) = n u / (1 - n u) bounds a float32 sum of n terms in any order
(fused multiply-adds only remove roundings).  Every bound below is a sum of such terms over the kernel's own chain of operations,
propagated with the absolute values of the weights; the float32 division and square root of the BatchNorm are correctly rounded
(the compiler's default for HIP), expf is taken at 2 ulp (its documented accuracy is 1)."""
import zlib

import numpy as np
import torch

import operand_cases as oc
from oracle import veto_oracle as vo
from veto_amd import synth

U = 2.0 ** -24
TOKENS, DIM, POS_DIM, EMBED_DIM = 19, 576, 128, 200
T = "fusion_transformer.transformer."
SD_SEED = 3


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- weights ------------------------------------------------------------------------------------------------------------------------
_SD = {}


def state_dict(layers, num_obj_cls=151, num_out=51, var0=False):
    """Synthetic predictor weights (numpy float32).  var0: the running variance of pos_embed's BatchNorm is exactly 0 (eps only)."""
    key = (layers, num_obj_cls, num_out, var0)
    if key not in _SD:
        sd = synth.predictor_state_dict(SD_SEED, layers=layers, num_obj_cls=num_obj_cls, num_rel_cls=num_out)
        if var0:
            sd["pos_embed.0.running_var"] = np.zeros(4, dtype=np.float32)
        _SD[key] = sd
    return _SD[key]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _rng(name, seed=0):
    return np.random.default_rng([seed, zlib.crc32(name.encode())])


def plain_boxes(n, rng):
    """xyxy boxes on a grid of quarters (so that the xywh form of the same boxes is exact in float32)"""
    xy = np.round(rng.uniform(0.0, 400.0, (n, 2)) * 4) / 4
    wh = np.round(rng.uniform(10.0, 210.0, (n, 2)) * 4) / 4
    return np.concatenate([xy, xy + wh], axis=1).astype(np.float32)


HARD_BOXES = np.array([   # xyxy, all on the grid of quarters
    [10.0, 20.0, 10.0, 50.0],            # x2 == x1: width 1 under the +1 convention
    [33.25, 40.0, 90.5, 40.0],           # y2 == y1
    [7.0, 7.0, 7.0, 7.0],                # a point
    [-120.5, -80.0, -20.25, -10.0],      # negative coordinates
    [-50.0, -60.0, 70.0, 30.0],          # straddling the origin
    [-300.0, 12.0, -299.75, 400.0],
    [3000.0, 4100.25, 3500.5, 5900.0],   # coordinates in the thousands
    [5000.0, 2000.0, 8191.75, 6000.0],
    [4095.75, 4096.0, 4096.25, 4097.0],
    [0.0, 0.0, 799.0, 599.0],            # the whole image
    [120.0, 80.0, 260.5, 210.25],
    [0.25, 0.5, 0.75, 1.0],
], dtype=np.float32)


def to_xywh(xyxy):
    """The xywh BoxList of the same boxes (structures/bounding_box.py:60-78); exact for boxes on the grid of quarters."""
    b = xyxy.astype(np.float64)
    out = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1], axis=1)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def roi_maps(n, kind, rng):
    """[n, 256, 8, 8] float32.  gauss: N(0, 1); outliers: one value in 500 multiplied by 300; offset: N(15, 40), row means far
    from zero; zeros: for the cases that do not look at the patch tokens."""
    if kind == "zeros":
        return np.zeros((n, 256, 8, 8), dtype=np.float32)
    x = rng.standard_normal((n, 256, 8, 8), dtype=np.float32)
    if kind == "outliers":
        x = np.where(rng.random(x.shape) < 0.002, x * np.float32(300.0), x).astype(np.float32)
    elif kind == "offset":
        x = (x * np.float32(40.0) + np.float32(15.0)).astype(np.float32)
    else:
        assert kind == "gauss", kind
    return x


NO_PAIRS = np.zeros((0, 2), dtype=np.int64)


def sampled_pairs(n, count, rng):
    """A sampled pair list of an n-object image: repeats and self-pairs included (rows 1 and 2 make sure of both)"""
    p = rng.integers(0, n, (count, 2)).astype(np.int64)
    if count >= 3:
        p[1] = p[0]
        p[2] = (p[2, 0], p[2, 0])
    return p


def make_case(name, num_objs, pairs, boxes=None, box_mode=0, labels=None, logits=None, num_obj_cls=151, maps="gauss",
              bn_batch=False, var0=False, like=None):
    """A batch for veto_forward: per-image object counts and image-local pair lists, boxes in `box_mode`'s convention (0 xyxy,
    1 xywh), predcls labels or sgcls logits.  like: the name of the case whose random draws (labels, ROI maps) this one repeats."""
    rng = _rng(like or name)
    n = int(sum(num_objs))
    assert len(pairs) == len(num_objs)
    if boxes is None:
        boxes = plain_boxes(n, rng)
    if labels is None and logits is None:
        labels = rng.integers(0, num_obj_cls, n).astype(np.int64)
        labels[0], labels[-1] = 0, num_obj_cls - 1         # both ends of the embedding table
    assert boxes.shape == (n, 4)
    return dict(name=name, num_objs=[int(x) for x in num_objs], pairs=[np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs],
                boxes=np.ascontiguousarray(boxes, dtype=np.float32), box_mode=box_mode, labels=labels, logits=logits,
                num_obj_cls=num_obj_cls, rgb=roi_maps(n, maps, rng), dep=roi_maps(n, maps, rng), bn_batch=bn_batch, var0=var0)


def n_pair(case):
    return int(sum(len(p) for p in case["pairs"]))


# ---- pair-index cases -----------------------------------------------------------------------------------------------------------------
def _image_mix(n_img, rng, zero_at=()):
    """n_img images of 1..3 objects: all pairs, the (0, 0) placeholder for one-object images, a sampled list for every third
    image, and NO pairs for the images listed in zero_at."""
    num_objs = [int(x) for x in rng.integers(1, 4, n_img)]
    num_objs[0] = 1 if n_img > 1 else 3                    # a one-object image with its placeholder in every multi-image case
    pairs = []
    for i, n in enumerate(num_objs):
        if i in zero_at:
            pairs.append(NO_PAIRS)
        elif i % 3 == 2:
            pairs.append(sampled_pairs(n, int(rng.integers(1, 9)), rng))
        else:
            pairs.append(vo.enumerate_test_pairs(n))
    return num_objs, pairs


def pair_index_cases():
    out = {}
    for n_img in (1, 2, 3, 64, 65, 257):
        name = "images_%d" % n_img
        out[name] = make_case(name, *_image_mix(n_img, _rng(name, 1)), maps="zeros")
    for tag, n_img, zero_at in (("front", 5, (0,)), ("middle", 6, (3,)), ("twice", 7, (2, 3)), ("end", 5, (4,)),
                                ("front_twice_end", 66, (0, 1, 30, 31, 32, 65))):
        name = "zero_pairs_" + tag
        out[name] = make_case(name, *_image_mix(n_img, _rng(name, 1), zero_at), maps="zeros")
    return out


# ---- token cases ----------------------------------------------------------------------------------------------------------------------
GRID_PAIR_COUNTS = (1, 6, 7, 27, 28)      # 19 n_pair rows in workgroups of 16: 2, 8, 9, 33, 34 workgroups (grid: 8, 8, 16, 40, 40)


def _pairs_for_count(count, rng):
    """(num_objs, pairs) with exactly `count` pairs"""
    if count == 1:
        return [1], [vo.enumerate_test_pairs(1)]
    if count == 6:
        return [3], [vo.enumerate_test_pairs(3)]
    if count == 7:
        return [3, 1], [vo.enumerate_test_pairs(3), vo.enumerate_test_pairs(1)]
    if count == 36:      # 5 x 7 + 1 = 7 x 5 + 1: chunks of 5 and of 7 both split the images and end on one pair
        return [4, 6], [vo.enumerate_test_pairs(4), sampled_pairs(6, 24, rng)]
    return [6], [vo.enumerate_test_pairs(6)[:count]]


def softmax_logit_rows(num_obj_cls, rng):
    """One row of every kind obj_prep_kernel's softmax has to survive, as (names, [rows, num_obj_cls] float32)"""
    C = num_obj_cls
    rows, names = [], []

    def add(name, r):
        names.append(name)
        rows.append(np.asarray(r, dtype=np.float32))

    add("randn", rng.standard_normal(C))
    add("equal", np.full(C, 2.5))
    add("equal_zero", np.zeros(C))
    r = rng.standard_normal(C); r[C - 1] = 60.0
    add("dominant_last", r)
    r = rng.standard_normal(C); r[0] = 45.0
    add("dominant_first", r)
    r = rng.standard_normal(C); r[::3] = -np.inf
    add("minus_inf_entries", r)
    r = np.full(C, -np.inf); r[C // 2] = 0.5
    add("minus_inf_all_but_one", r)
    add("magnitude_1e4", rng.standard_normal(C) * 1.0e4)
    r = rng.standard_normal(C) - 1.0e4
    add("offset_minus_1e4", r)
    r = rng.standard_normal(C) * 3.0 + 1.0e4
    add("offset_plus_1e4", r)
    return names, np.stack(rows)


def token_cases():
    """name -> case; every case is small enough for the float64 patch bound (a handful of objects)"""
    out = {}

    def add(case):
        out[case["name"]] = case

    for count in GRID_PAIR_COUNTS + (36,):
        name = "pairs_%d" % count
        add(make_case(name, *_pairs_for_count(count, _rng(name, 2)), maps="gauss"))
    hard_pairs = [vo.enumerate_test_pairs(5), sampled_pairs(7, 20, _rng("hard", 2))]
    for maps in ("outliers", "offset"):
        add(make_case("hard_boxes_xyxy_" + maps, [5, 7], hard_pairs, boxes=HARD_BOXES, maps=maps))
    add(make_case("hard_boxes_xywh_outliers", [5, 7], hard_pairs, boxes=to_xywh(HARD_BOXES), box_mode=1, maps="outliers",
                  like="hard_boxes_xyxy_outliers"))
    add(make_case("hard_boxes_xyxy_var0", [5, 7], hard_pairs, boxes=HARD_BOXES, maps="gauss", var0=True))
    add(make_case("hard_boxes_xywh_var0", [5, 7], hard_pairs, boxes=to_xywh(HARD_BOXES), box_mode=1, maps="gauss", var0=True,
                  like="hard_boxes_xyxy_var0"))
    for C in (151, 201):
        names, logits = softmax_logit_rows(C, _rng("softmax_%d" % C, 2))
        k = len(names)
        add(make_case("sgcls_%d" % C, [k], [sampled_pairs(k, 3 * k, _rng("sgp_%d" % C, 2))], logits=logits, num_obj_cls=C, maps="gauss"))
    return out


# ---- batch-statistics cases -------------------------------------------------------------------------------------------------------------
BN_COUNTS = (2, 255, 256, 257, 513)


def bn_boxes(kind, n, rng):
    if kind == "identical":
        return np.tile(np.array([[123.25, 45.5, 310.75, 200.0]], dtype=np.float32), (n, 1))
    if kind == "offset_1e4":      # spread 1 at offset 1e4, on a grid of 1/8 (exact in float32: the spacing there is 2^-10)
        xy = 1.0e4 + np.round(rng.uniform(0.0, 1.0, (n, 2)) * 8) / 8
        wh = 20.0 + np.round(rng.uniform(0.0, 1.0, (n, 2)) * 8) / 8
        return np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    assert kind == "plain"
    return plain_boxes(n, rng)


def bn_cases():
    out = {}
    for n in BN_COUNTS:
        for kind in ("identical", "offset_1e4", "plain"):
            for mode in (0, 1):
                name = "bn_%s_%d_%s" % (kind, n, "xywh" if mode else "xyxy")
                rng = _rng("bn_%s_%d" % (kind, n), 3)      # the two modes hold the same boxes, pairs and labels
                xyxy = bn_boxes(kind, n, rng)
                pairs = sampled_pairs(n, 24, rng)
                pairs[3] = (n - 1, 0)       # the last object as a subject, the first as an object
                out[name] = make_case(name, [n], [pairs], boxes=to_xywh(xyxy) if mode else xyxy, box_mode=mode, maps="zeros",
                                      bn_batch=True, like="bn_%s_%d" % (kind, n))
    return out


# ---- float64 restatement in the kernels' per-object form, with bounds -------------------------------------------------------------------
def reference_indices(case, wrong=()):
    """The loop of roi_relation_predictors.py:4106-4115."""
    total = n_pair(case) if "placeholder_dropped" not in wrong else \
        sum(len(p) for p, n in zip(case["pairs"], case["num_objs"]) if not (n == 1 and len(p) == 1))
    subj, obj = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
    start = cumulative = 0
    for pairs, n in zip(case["pairs"], case["num_objs"]):
        if "next_image_offset" in wrong:
            cumulative += n
        if not ("placeholder_dropped" in wrong and n == 1 and len(pairs) == 1):
            end = start + len(pairs)
            subj[start:end] = pairs[:, 0] + cumulative
            obj[start:end] = pairs[:, 1] + cumulative
            start = end
        if "next_image_offset" not in wrong:
            cumulative += n
    return subj, obj


def box_features(case, wrong=()):
    """(v [N, 4] float64: centre x, centre y, w, h; dv: the float32 rounding in the device's v).  The kernels form
    w = fl(fl(x2 - x1) + 1) (xyxy) or take it as it is (xywh) and c = fl(x1 + 0.5 w), which the compiler may contract into one fused
    multiply-add: float32 operations are deterministic, so dv is not a bound but the error itself, the larger of the two forms
    (0 for boxes whose features float32 holds exactly)."""
    b32 = case["boxes"]
    b = b32.astype(np.float64)
    if case["box_mode"] == 0:
        wh = b[:, 2:] - b[:, :2] + 1.0
        wh32 = (b32[:, 2:] - b32[:, :2]) + np.float32(1.0)
    else:
        wh, wh32 = b[:, 2:], b32[:, 2:]
    c = b[:, :2] + 0.5 * wh
    c_two = (b32[:, :2] + np.float32(0.5) * wh32).astype(np.float64)                  # two roundings (0.5 w is exact)
    c_fma = (b[:, :2] + 0.5 * wh32.astype(np.float64)).astype(np.float32).astype(np.float64)
    dv = np.concatenate([np.maximum(np.abs(c_two - c), np.abs(c_fma - c)), np.abs(wh32.astype(np.float64) - wh)], axis=1)
    if "xywh_plus_one" in wrong and case["box_mode"] == 1:
        wh = wh + 1.0
        c = b[:, :2] + 0.5 * wh
    return np.concatenate([c, wh], axis=1), dv


def batch_statistics(case, wrong=()):
    """(the twelve values bn_batch_stats_kernel writes: mean, biased variance, unbiased variance -- float64 --, their bounds).
    The kernel forms the features in float32 (dv each), sums them in double (two passes) and rounds once at the store:
    |mean' - mean| <= mean(dv) + u |mean|; var(v + e) - var(v) = 2 cov(v, e) + var(e), so
    |var' - var| <= 2 sqrt(var) max|e| + max|e|^2 + u var'; the double sums themselves add 2^-50 relative."""
    v, dv = box_features(case, wrong)
    n = v.shape[0]
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    unb = var * n / (n - 1) if n > 1 else ((v - mean) ** 2).sum(0)
    e = dv.max(0)
    dmean = dv.mean(0) + U * np.abs(mean) + 2.0 ** -50 * np.abs(v).mean(0)
    dvar = 2 * np.sqrt(var) * e + e * e
    dvar = dvar + U * (var + dvar) + 2.0 ** -48 * var
    return np.concatenate([mean, var, unb]), np.concatenate([dmean, dvar, dvar * (n / (n - 1) if n > 1 else n)])


def _f64(sd, key):
    return np.asarray(sd[key], dtype=np.float64)


def object_tables(sd, case, stats=None, wrong=()):
    """Per-object rows of the location / class projections in the kernel's form (obj_prep_kernel): the subject half carries the
    bias.  Returns dict(LS, LO, CS, CO [N, 576] float64 and dLS, dLO, dCS, dCO, their bounds).  `stats`: the twelve batch
    statistics to normalise with (a bn_batch case; None: computed here), else the running statistics."""
    v, dv = box_features(case, wrong)
    if case["bn_batch"]:
        st = batch_statistics(case, wrong)[0] if stats is None else np.asarray(stats, dtype=np.float64)
        mean, var = st[0:4], (st[8:12] if "unbiased_variance" in wrong else st[4:8])
    else:
        mean, var = _f64(sd, "pos_embed.0.running_mean"), _f64(sd, "pos_embed.0.running_var")
    bw, bb = _f64(sd, "pos_embed.0.weight"), _f64(sd, "pos_embed.0.bias")
    std = np.sqrt(var + 1e-5)
    t3 = (v - mean) / std * bw
    box = t3 + bb
    # t1 = fl(v' - mean): dv + u |t1|; s = sqrtf(fl(var + eps)): 2 u relative, and eps itself is 1e-5f (0.2 u in s when var = 0);
    # fl(t1 / s), fl(. * w): u each; fl(. + b): u |box|
    dbox = np.abs(bw) / std * (dv + U * np.abs(v - mean)) + 6 * U * np.abs(t3) + U * np.abs(box)
    pw, pb = _f64(sd, "pos_embed.1.weight"), _f64(sd, "pos_embed.1.bias")
    pos_pre = box @ pw.T + pb
    dpos = dbox @ np.abs(pw).T + gamma(5) * (np.abs(box) @ np.abs(pw).T + np.abs(pb))
    pos = np.maximum(pos_pre, 0.0)                                    # ReLU is 1-Lipschitz: dpos carries over

    E = _f64(sd, "obj_embed.weight")
    C = E.shape[0]
    if case["logits"] is None:
        emb, demb = E[case["labels"]], np.zeros((len(case["labels"]), E.shape[1]))
    else:
        lg = case["logits"].astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            d = lg - (0.0 if "softmax_no_max" in wrong else lg.max(1, keepdims=True))
            e = np.exp(d)
            p = e / e.sum(1, keepdims=True)
        live = d > -104.0                                             # below: expf gives 0 (2^-149 = e^-103.3)
        D = np.where(live, np.abs(d), 0.0).max(1, keepdims=True)
        # e_c = expf(fl(s_c - mx)): u |d_c| from the argument, 4 u from expf (2 ulp); the sum: the worst e_c plus gamma(C);
        # 1 / sum and e_c * inv: u each; results in float32's subnormal range may be flushed (2^-126 absolute)
        rel = U * (np.abs(np.where(live, d, 0.0)) + 4) + U * (D + 4) + gamma(C) + 2 * U
        dp = np.where(np.isfinite(p), rel * p, np.inf) + 2.0 ** -126
        emb = p @ E
        demb = dp @ np.abs(E) + gamma(C) * (p @ np.abs(E))

    out = {"pos": pos, "emb": emb}
    for tag, x, dx, wkey, kin in (("L", pos, dpos, "location_projection.0.", POS_DIM), ("C", emb, demb, "class_projection.0.", EMBED_DIM)):
        W, b = _f64(sd, wkey + "weight"), _f64(sd, wkey + "bias")
        Ws, Wo = W[:, :kin], W[:, kin:]
        out[tag + "S"] = x @ Ws.T + b
        out[tag + "O"] = x @ Wo.T
        out["d" + tag + "S"] = dx @ np.abs(Ws).T + gamma(kin + 1) * (np.abs(x) @ np.abs(Ws).T + np.abs(b))
        out["d" + tag + "O"] = dx @ np.abs(Wo).T + gamma(kin) * (np.abs(x) @ np.abs(Wo).T)
    return out


def _hu(v):
    """half a bf16 step at |v| (tests/operand_cases.py), 0 at 0"""
    return np.where(v == 0, 0.0, oc._half_ulp(v, 7, -126))


def split_gemm_bound(A, W):
    """Bound of |gemm_patch(A, W) - A W^T| for fp32 A [M, K], W [N, K] on split-bf16 operands (the format gemm_patch runs on in
    VETO_PRECISE and VETO_MIXED alike: run_gemm is handed the split rows of patchify_kernel and build_patch_weight_kernel).
    Per product the bound of tests/operand_cases.product_bound, mode PRECISE: a = ah + al + ra with |al| <= hu(a), |ra| <= hu(al),
    the same for w, the kept terms are ah wh + al wh + ah wl: |ra||w| + |a||rw| + |ra||rw| + |al||wl|; summed over k as four
    matrix products.  Plus the float32 accumulation of the 3 K' kept products, gamma(3 K') sum |a||w|, K' = the number of
    k's with a non-zero weight (adding an exact zero rounds nothing)."""
    aa, aw = np.abs(A), np.abs(W)
    al, wl = _hu(aa), _hu(aw)
    ra, rw = _hu(al), _hu(wl)
    fmt = np.concatenate([ra, aa, ra, al], axis=1) @ np.concatenate([aw, rw, rw, wl], axis=1).T
    k_live = int((aw != 0).sum(1).max())
    return fmt + gamma(3 * k_live) * (aa @ aw.T + fmt)


def patch_tables(sd, case):
    """Per-object patch rows in the kernel's form (build_patch_weight_kernel): TS [N, 16, 576] = subject half with the bias,
    TO = object half; columns [depth -> proj_d 512 | rgb -> proj_v 64].  Returns (TS, TO, dTS, dTO)."""
    dep = vo.patchify(torch.from_numpy(case["dep"]).double(), 2).numpy()     # [N, 16, (p1 p2 c)]: 4 x 256 features
    rgb = vo.patchify(torch.from_numpy(case["rgb"]).double(), 2).numpy()
    N = dep.shape[0]
    dep, rgb = dep.reshape(N * 16, 1024), rgb.reshape(N * 16, 1024)
    wd = _f64(sd, T + "patch_embed.proj_d.weight").reshape(512, 4, 2, 256)  # [out, (p1 p2), subject | object, c]
    wv = _f64(sd, T + "patch_embed.proj_v.weight").reshape(64, 4, 2, 256)
    bias = np.concatenate([_f64(sd, T + "patch_embed.proj_d.bias"), _f64(sd, T + "patch_embed.proj_v.bias")])
    tabs, bounds = [], []
    for half in (0, 1):
        Wd, Wv = wd[:, :, half, :].reshape(512, 1024), wv[:, :, half, :].reshape(64, 1024)
        t = np.concatenate([dep @ Wd.T, rgb @ Wv.T], axis=1)
        d = np.concatenate([split_gemm_bound(dep, Wd), split_gemm_bound(rgb, Wv)], axis=1)
        if half == 0:
            t = t + bias
            d = d + U * np.abs(t)                                     # the bias add of the GEMM epilogue
        tabs.append(t.reshape(N, 16, DIM))
        bounds.append(d.reshape(N, 16, DIM))
    return tabs[0], tabs[1], bounds[0], bounds[1]


def cls_row(sd):
    """Token 0: ONE float32 add of two parameters (assemble_kernel), bit for bit"""
    return (np.asarray(sd[T + "cls_token"], dtype=np.float32) + np.asarray(sd[T + "pos_embedding"], dtype=np.float32)).reshape(DIM)


def restate(sd, case, stats=None, wrong=(), patch=True):
    """(tokens [P, 19, 576] float64, bound [P, 19, 576], subj, obj) in the kernels' per-object form.  patch=False leaves the rows
    of the patch tokens NaN (cases that only look at tokens 0, 17, 18).  `wrong`: names of deliberate mistakes (host test)."""
    subj, obj = reference_indices(case, wrong)
    s, o = (obj, subj) if "halves_swapped" in wrong else (subj, obj)
    P = len(subj)
    pe = _f64(sd, T + "pos_embedding").reshape(DIM)
    tok = np.full((P, TOKENS, DIM), np.nan)
    bound = np.full((P, TOKENS, DIM), np.nan)
    tok[:, 0], bound[:, 0] = cls_row(sd).astype(np.float64), 0.0
    ot = object_tables(sd, case, stats, wrong)
    for t, tag in ((17, "L"), (18, "C")):
        S, O = ot[tag + "S"][s], ot[tag + "O"][o]
        pre = S + O
        dpre = ot["d" + tag + "S"][s] + ot["d" + tag + "O"][o]
        dpre = dpre + U * (np.abs(pre) + dpre)                        # fl(S + O)
        if "relu_per_half" in wrong:
            row = np.maximum(S, 0.0) + np.maximum(O, 0.0) + pe
        elif "pos_before_relu" in wrong:
            row = np.maximum(pre + pe, 0.0)
        else:
            row = np.maximum(pre, 0.0) + pe
        tok[:, t] = row
        bound[:, t] = dpre + U * (np.abs(row) + dpre)                 # fl(relu(.) + pos)
    if patch:
        TS, TO, dTS, dTO = patch_tables(sd, case)
        pre = TS[s] + TO[o]
        dpre = dTS[s] + dTO[o]
        dpre = dpre + U * (np.abs(pre) + dpre)
        tok[:, 1:17] = pre + pe
        bound[:, 1:17] = dpre + U * (np.abs(pre + pe) + dpre)
    return tok, bound, subj, obj


# ---- the oracle's own tokens ------------------------------------------------------------------------------------------------------------
def oracle_sd(sd, case, stats=None):
    """The state dict oracle/veto_oracle.py normalises with: for a bn_batch case given the device's statistics, those in the place
    of the running ones (BatchNorm on batch statistics is the same formula on other numbers)."""
    if not case["bn_batch"] or stats is None:
        return sd
    sd = dict(sd)
    sd["pos_embed.0.running_mean"] = np.asarray(stats[0:4], dtype=np.float32)
    sd["pos_embed.0.running_var"] = np.asarray(stats[4:8], dtype=np.float32)
    return sd


def oracle_tokens(sd, case, dtype=torch.float64, stats=None, patch=True):
    """oracle/veto_oracle.py on the case: ([P, 19, 576] tokens (patch=False: rows 1..16 NaN), subj, obj)"""
    cfg = vo.OracleConfig(layers=1, heads=8, mode="predcls" if case["logits"] is None else "sgcls")
    subj, obj = vo.build_pair_indices(case["pairs"], case["num_objs"])
    s, o = torch.from_numpy(subj), torch.from_numpy(obj)
    emb, _ = vo.object_embeddings(sd, cfg, case["labels"], case["logits"], np.zeros(len(case["boxes"]), dtype=np.int64), dtype)
    pos = vo.position_embedding(oracle_sd(sd, case, stats), cfg, case["boxes"], dtype,
                                batch_stats=case["bn_batch"] and stats is None, xywh=case["box_mode"] == 1)
    if patch:
        x = vo.pair_tokens(sd, cfg, emb, pos, torch.from_numpy(case["rgb"]).to(dtype), torch.from_numpy(case["dep"]).to(dtype), s, o, dtype)
        return x.numpy(), subj, obj
    _, (loc, cls) = vo.pair_location_class(sd, cfg, emb, pos, s, o, dtype)
    pe = vo._t(sd[T + "pos_embedding"], dtype).reshape(DIM)
    x = torch.full((len(subj), TOKENS, DIM), float("nan"), dtype=dtype)
    x[:, 0] = (vo._t(sd[T + "cls_token"], dtype).reshape(DIM) + pe)
    x[:, 17], x[:, 18] = loc + pe, cls + pe
    return x.numpy(), subj, obj


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the rows both have (NaN rows of `ref` are skipped); a non-finite `got` counts as infinite,
    an element with bound 0 must be equal"""
    have = ~np.isnan(ref)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(np.asarray(got, dtype=np.float64)) | ~have, r, np.inf)
    return float(r[have].max()) if have.any() else 0.0


# ---- classifier head ------------------------------------------------------------------------------------------------------------------
HEAD_WIDTHS = (51, 101, 60, 108, 128, 129, 257)      # the shipped widths, then the ones that take the class loop's second / third trip
HEAD_PAIR_COUNTS = (1, 2, 3, 4, 5)
HEAD_CHUNKS = (1, 3, 5)


def head_reference(sd, cls_dev):
    """(cls_dev @ W^T + b in float64, gamma(577) (sum |w||cls| + |b|)): head_kernel adds 576 products and the bias in float32"""
    W, b = _f64(sd, "rel_out.weight"), _f64(sd, "rel_out.bias")
    c = np.asarray(cls_dev, dtype=np.float64)
    return c @ W.T + b, gamma(577) * (np.abs(c) @ np.abs(W).T + np.abs(b))


def f24_step(v):
    """the spacing of the 3-byte float's grid (15 stored mantissa bits) at |v|"""
    return 2 * oc._half_ulp(v, 15, -126)


def ulp32(v):
    """the spacing of float32 at |v|"""
    return 2 * oc._half_ulp(v, 23, -126)
