"""The forward attention kernels of veto_amd/csrc/attention.hip and qkv0_combine_kernel (rowops.hip), each against ITS OWN stated
contract: the inputs, the float64 references, the per-element bounds and the instance table (no test lives here;
tests/test_attention_forward_host.py proves the constructions, tests/test_attention_forward_gpu.py runs them on the device).

The contracts are the comments on AttnArgs in kernels.h and the header comment of the folded kernel in attention.hip:
  dense    per pair and head over the 19 tokens: softmax(q k^T dh^-0.5) v, heads merged (model_veto.py:85-96); cls_only = row 0
  table    the row of token t = 1..16 of pair p is rstd[p, t] (sw[subj[p] 16 + t - 1] + ow[obj[p] 16 + t - 1]) + c2, token 0 is the
           third row of vec = [c2 | b0 | qkv_cls], tokens 17 / 18 come from qkv; then the dense form (qkv0_combine writes rows 0..16)
  folded   a_j = LayerNorm(x_j) (eps 1e-5), score[h][j] = dh^-0.5 u_h . a_j, p = softmax over j, abar_h = sum_j p[h][j] a_j
The tests hand the kernels tables, statistics and u rows they make themselves; no layer algebra is restated.

The bounds are worst-case sums in the style of prelude_cases.restate (every rounding in the same direction), from what the kernels'
comments state about their formats (U = 2^-24, gamma(n) = n U / (1 - n U), hu16 / hu8 = half a grid step of fp16 / bf16):
  operand planes   MFMA forms: x ~ hi + lo, hi = fp16(x), lo = fp16(x - hi): |x - hi - lo| <= hu16(hu16 x), never below 2^-25 (a lo
                   part under fp16's last subnormal step is lost: the absolute term); of the four products hi hi + hi lo + lo hi are
                   kept, lo lo <= hu16(x) hu16(y) is dropped.  3-byte inputs carry 16 significant bits: hi + lo is exact unless the
                   value's own grid is finer than 2^-24.  The folded MFMA kernel splits into bf16 hi + bf16 lo (hu8(hu8 x), fp32's
                   range: nothing saturates).  The vector-ALU kernels read fp32 as it is.
  accumulation     every product enters an fp32 sum once: gamma(3 x 16 x k-steps) of sum |x||y| for a matrix-core product,
                   gamma(dh) / gamma(19) for the vector-ALU chains, plus the roundings of dh^-0.5 and of the scaling
  softmax          a score error e_j changes exp(s_j - max) by the factor exp(e_j); with A_j = expm1(e_j + U |s_j - max| + 4 U) (the
                   subtraction's rounding and expf's 2 ulp) p_j moves by at most p_j ((1 + A_j)(1 + gamma(22)) / (1 - max A) - 1)
  output format    split rows: hu8(hu8 o); mixed rows decoded as h + X 2^-11: the e4m3 step of the residual 2^11 (o - h), or its
                   distance to 448 where it saturates
The vector-ALU kernels and qkv0_combine are plain fp32 chains and are ALSO held to the yardstick of test_train_scale_gpu.py /
test_prelude_gpu.py: 4 x the worst error of the float32 torch evaluation against float64 on the case + 4 fp32 ulps of the element."""
import functools

import numpy as np
import torch

import operand_cases as oc
from prelude_cases import U, gamma, ulp32, worst_ratio      # noqa: F401  (re-exported for the two test modules)

TOKENS, DIM, PATCH = 19, 576, 16
N3 = 3 * DIM
SPLIT, MIXED = 0, 1
FP16_MAX = oc.FP16_MAX
PLANES_MAX = 2 * FP16_MAX          # what fp16 hi + fp16 lo can hold once both conversions saturate
LDS_LIMIT = 160 * 1024

# ---- head counts ------------------------------------------------------------------------------------------------------------------
CREATE_HEADS = [h for h in range(1, DIM + 1) if DIM % h == 0 and (DIM // h) % 4 == 0]      # what veto_create accepts
MFMA_HEADS = [h for h in CREATE_HEADS if DIM // h in (72, 96)]                              # 8, 6


def generic_lds_bytes(dh):
    """dynamic LDS of attention_kernel: 4 waves x (q, k, v [19][dh + 4] + probabilities [19][20]) floats"""
    return 4 * (3 * TOKENS * (dh + 4) + TOKENS * 20) * 4


GENERIC_HEADS = [h for h in CREATE_HEADS if h not in MFMA_HEADS and generic_lds_bytes(DIM // h) <= LDS_LIMIT]     # 4, 9, 12, ... 144
LDS_REFUSED_HEADS = [h for h in CREATE_HEADS if h not in MFMA_HEADS and h not in GENERIC_HEADS]                  # 1, 2, 3
FOLD_HEADS = [8, 6, 4, 12, 9, 1]                 # the folded kernels take up to 12 heads; 9: an odd count, 1: a wave without a partner head
SIZES = (1, 3, 37)
BIG = 700                                         # "plain" only: the MFMA forms launch 2 800 (8 heads) workgroups

FAMILIES = ("plain", "sharp", "onehot", "flat", "routing", "range", "overflow")
FOLD_FAMILIES = FAMILIES + ("ln_edges",)


# ---- the instance table -------------------------------------------------------------------------------------------------------------
class Instance:
    def __init__(self, kernel, form, heads, cls_only=0, o_fmt=SPLIT, f24=0):
        self.kernel, self.form, self.heads, self.cls_only, self.o_fmt, self.f24 = kernel, form, heads, cls_only, o_fmt, f24
        self.id = "%s-h%d%s%s%s" % (form, heads, "-cls" if cls_only else "", "-mixed" if o_fmt == MIXED else "", "-f24" if f24 else "")

    @property
    def families(self):
        return FOLD_FAMILIES if self.form.startswith("fold") else FAMILIES

    def sizes(self, family):
        return SIZES + ((BIG,) if family == "plain" and self.form != "generic" else ())


def instance_table():
    t = []
    for h in MFMA_HEADS:
        dh = DIM // h
        for f24 in (0, 1):
            for cls_only, o_fmt in ((0, SPLIT), (0, MIXED), (1, SPLIT)):
                t.append(Instance("attention_mfma_kernel<%d, false, %s>" % (dh, "true" if f24 else "false"), "dense", h, cls_only, o_fmt, f24))
        for o_fmt in (SPLIT, MIXED):
            t.append(Instance("attention_mfma_kernel<%d, true>" % dh, "table", h, 0, o_fmt))
    for h in GENERIC_HEADS:
        for cls_only in (0, 1):
            t.append(Instance("attention_kernel", "generic", h, cls_only))
    for h in FOLD_HEADS:
        t.append(Instance("cls_fold_attention_mfma_kernel<false>", "fold", h))
        t.append(Instance("cls_fold_attention_mfma_kernel<true>", "fold", h, f24=1))
        t.append(Instance("cls_fold_attention_kernel", "fold_valu", h))
    t.append(Instance("qkv0_combine_kernel", "combine", 0))
    return t


INSTANCES = instance_table()
BY_ID = {i.id: i for i in INSTANCES}
KERNELS = sorted({i.kernel for i in INSTANCES})      # the sixteen attention instances + qkv0_combine_kernel


# ---- half grid steps ------------------------------------------------------------------------------------------------------------------
def _hu(v, mant_bits, emin):
    """half the spacing of a binary format's grid at |v| (float64); at 0 the subnormal step"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, ex = np.frexp(v)
    ex = np.where(v == 0, -10 ** 6, ex)
    return np.ldexp(0.5, np.maximum(ex - 1, emin) - mant_bits)


def hu16(v):
    return _hu(v, 10, -14)


def hu8(v):
    return _hu(v, 7, -126)


def planes16(x, dx=0.0):
    """(|x - hi - lo| bound, |lo| bound) of the fp16 hi / lo planes of a value within dx of x.
    Beyond 65504 hi stays at 65504 and lo = fp16(x - hi) carries the excess with lo's own 11 bits (PLANES_MAX: both saturated)."""
    a = np.abs(x) + dx
    lo = np.where(a > FP16_MAX, np.minimum(a - FP16_MAX, FP16_MAX), hu16(np.minimum(a, FP16_MAX)))
    return dx + hu16(lo), lo


def planes16_f24(x):
    """the same for a 3-byte float: 16 significant bits, so hi + lo is exact unless the value's grid is finer than fp16's last step
    (or the value lies beyond 65504, where lo alone carries the excess)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    step = 2 * _hu(x, 15, -126)
    rep, lo = planes16(x)
    return np.where(x > FP16_MAX, rep, np.where((x != 0) & (step < 2.0 ** -24), 2.0 ** -25, 0.0)), lo


def planes8(x, dx=0.0, exact16=False):
    """bf16 hi + bf16 lo (the folded MFMA kernel): a 16-bit value splits exactly"""
    a = np.abs(x) + dx
    lo = hu8(a)
    return np.zeros_like(a) + dx + (0.0 if exact16 else hu8(lo)), lo


def out_format_term(o_abs, o_fmt):
    """rounding of a value of magnitude <= o_abs into the output rows, as the tests decode them"""
    if o_fmt == SPLIT:
        return hu8(hu8(o_abs))
    l = np.where(o_abs > FP16_MAX, o_abs - FP16_MAX, hu16(np.minimum(o_abs, FP16_MAX)))      # |o - h|, h = fp16 saturating
    s = 2.0 ** oc.ACT_RES_EXP
    return oc._e4m3_err(l * s) / s


# ---- views ----------------------------------------------------------------------------------------------------------------------------
def heads_view(m, heads):
    """[P 19, 576] -> [P, H, 19, dh]"""
    P = m.shape[0] // TOKENS
    return m.reshape(P, TOKENS, heads, DIM // heads).transpose(0, 2, 1, 3)


def merge_heads(o):
    """[P, H, n, dh] -> [P n, 576]"""
    P, H, n, dh = o.shape
    return o.transpose(0, 2, 1, 3).reshape(P * n, H * dh)


def qkv_views(qkv, heads):
    return tuple(heads_view(np.ascontiguousarray(qkv[:, i * DIM:(i + 1) * DIM]), heads) for i in range(3))


def softmax64(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ---- float64 references -----------------------------------------------------------------------------------------------------------------
def dense_ref(qkv, heads, cls_only=0, dh_scale=None, cls_row=0):
    """model_veto.py:85-96 on [P 19, 1728] float64 -> [P 19, 576] (cls_only: [P, 576], the row of token 0).  dh_scale / cls_row: the
    deliberate mistakes of the host test."""
    q, k, v = qkv_views(np.asarray(qkv, dtype=np.float64), heads)
    if cls_only:
        q = q[:, :, cls_row:cls_row + 1]
    s = (q @ k.transpose(0, 1, 3, 2)) * float(dh_scale or DIM // heads) ** -0.5
    return merge_heads(softmax64(s) @ v)


def table_matrix(t, wrong=(), dtype=np.float64):
    """The effective q / k / v matrix [P 19, 1728] of the table contract (rows 17 / 18 from t['qkv']).  `wrong`: host-test mistakes."""
    sw, ow, vec, qkv = (np.asarray(t[k], dtype=dtype) for k in ("sw", "ow", "vec", "qkv"))
    rstd = np.asarray(t["stats"], dtype=dtype).reshape(-1, TOKENS, 2)[:, :, 1]
    subj, obj = (t["obj"], t["subj"]) if "subj_obj_swapped" in wrong else (t["subj"], t["obj"])
    P = len(subj)
    x = qkv.reshape(P, TOKENS, N3).copy()
    if "tokens_17_18_swapped" in wrong:
        x[:, [17, 18]] = x[:, [18, 17]]
    tt = np.arange(PATCH)
    r = np.roll(rstd, -1, axis=1) if "rstd_of_neighbour" in wrong else rstd
    pre = sw[subj[:, None] * PATCH + tt] + ow[obj[:, None] * PATCH + tt]
    c2 = np.broadcast_to(vec[0:N3], (P, PATCH, N3)).copy()
    if "no_c2_token_1" in wrong:
        c2[:, 0] = 0
    x[:, 1:17] = (r[:, 1:17, None] * pre).astype(dtype) + c2
    x[:, 0] = vec[2 * N3:3 * N3]
    return x.reshape(P * TOKENS, N3)


def table_dx(t):
    """fp32 formation of the table rows: fl(s + o), fl(rstd .), fl(. + c2) -- U (2 |rstd (s + o)| + |x|) and second order; 0 elsewhere"""
    sw, ow, vec = (np.asarray(t[k], dtype=np.float64) for k in ("sw", "ow", "vec"))
    rstd = np.asarray(t["stats"], dtype=np.float64).reshape(-1, TOKENS, 2)[:, :, 1]
    P = len(t["subj"])
    tt = np.arange(PATCH)
    pre = np.abs(rstd[:, 1:17, None]) * (np.abs(sw[t["subj"][:, None] * PATCH + tt]) + np.abs(ow[t["obj"][:, None] * PATCH + tt]))
    dx = np.zeros((P, TOKENS, N3))
    dx[:, 1:17] = (U * (2 * pre + pre + np.abs(vec[0:N3]))) * (1 + 4 * U)
    return dx.reshape(P * TOKENS, N3)


def combine_rows(m):
    """rows 0..16 of every pair of a [P 19, N] matrix (what qkv0_combine writes)"""
    return m.reshape(-1, TOKENS, m.shape[-1])[:, :PATCH + 1]


def layernorm64(x, w, b):
    x = np.asarray(x, dtype=np.float64)
    d = x - x.mean(-1, keepdims=True)
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * np.asarray(w, dtype=np.float64) + np.asarray(b, dtype=np.float64)


def fold_ref(x, ln_w, ln_b, u, heads, dh_scale=None, head_shift=0):
    """[P 19, 576], [P, H 576] -> abar [P, H 576] float64.  head_shift: head h's abar taken from head h + shift (host test)."""
    a = layernorm64(x, ln_w, ln_b).reshape(-1, TOKENS, DIM)
    P = a.shape[0]
    uu = np.asarray(u, dtype=np.float64).reshape(P, heads, DIM)
    p = softmax64((uu @ a.transpose(0, 2, 1)) * float(dh_scale or DIM // heads) ** -0.5)
    return np.roll(p @ a, -head_shift, axis=1).reshape(P, heads * DIM)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    return a @ np.swapaxes(b, -1, -2)


def _softmax_bound(s, es):
    """|p^ - p| for scores s [.., nq, 19] known to within es (after scaling)"""
    p = softmax64(s)
    dist = np.minimum(s.max(-1, keepdims=True) - s, 110.0)
    with np.errstate(over="ignore", invalid="ignore"):
        A = np.expm1(es + U * (dist + 2 * es.max(-1, keepdims=True)) + 4 * U)
        Amax = A.max(-1, keepdims=True)
        dp = np.where(Amax < 1, p * ((1 + A) * (1 + gamma(22)) / np.where(Amax < 1, 1 - Amax, 1.0) - 1), np.inf)
    return p, dp + 2.0 ** -120


def dense_bound(qkv, heads, kind, cls_only=0, o_fmt=SPLIT, f24=0, dx=None):
    """Per-element bound of the dense form on the effective matrix qkv (float64 [P 19, 1728]; dx = how far the kernel's own fp32
    rows may lie from it: the table form).  kind "mfma" / "valu".  Returns [rows, 576]."""
    dh = DIM // heads
    q, k, v = (np.abs(m) for m in qkv_views(np.asarray(qkv, dtype=np.float64), heads))
    sq, sk, _ = qkv_views(np.asarray(qkv, dtype=np.float64), heads)
    dq, dk, dv = qkv_views(dx, heads) if dx is not None else (0.0, 0.0, 0.0)
    nq = 1 if cls_only else TOKENS
    q, sq = q[:, :, :nq], sq[:, :, :nq]
    dq = dq[:, :, :nq] if dx is not None else 0.0
    if kind == "mfma":
        pl = planes16_f24 if f24 else planes16
        (rq, hq), (rk, hk), (rv, hv) = (pl(q) if f24 else pl(q, dq)), (pl(k) if f24 else pl(k, dk)), (pl(v) if f24 else pl(v, dv))
        ks = (dh + 15) // 16
        es = _mm(rq, k) + _mm(q, rk) + _mm(rq, rk) + _mm(hq, hk) + gamma(3 * 16 * ks + 2) * _mm(q + 2 * hq, k + 2 * hk)
    else:
        es = gamma(dh + 2) * _mm(q, k)
    scale = float(dh) ** -0.5
    s = _mm(sq, sk) * scale
    es = scale * es * (1 + 3 * U) + 3 * U * np.abs(s)
    p, dp = _softmax_bound(s, es)
    if kind == "mfma":
        rp, hp = planes16(p, dp)
        eo = rp @ v + p @ rv + rp @ rv + hp @ hv + gamma(3 * 32 + 2) * ((p + dp + 2 * hp) @ (v + 2 * hv))
    else:
        eo = dp @ v + gamma(TOKENS + 2) * ((p + dp) @ v)
    o = np.abs(p @ qkv_views(np.asarray(qkv, dtype=np.float64), heads)[2])
    with np.errstate(invalid="ignore"):
        total = eo + out_format_term(np.where(np.isfinite(eo), o + eo, o), o_fmt) + 2.0 ** -126
    return merge_heads(total)


def combine_bound(t):
    return combine_rows(table_dx(t))


def layernorm_bound(x, w, b):
    """|fl32 LayerNorm - LayerNorm| per element for the kernels' two-pass form: the mean over 36 + 4 (a quarter wave per row) or 9 + 6
    (a wave per row) partial sums, the variance likewise on d = x - mean, rstd = 1 / sqrtf(var + eps), (d rstd) g + b."""
    x = np.asarray(x, dtype=np.float64)
    w, b = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    g = gamma(50)
    dm = g * np.abs(x).mean(-1, keepdims=True)
    d = np.abs(x - x.mean(-1, keepdims=True))
    dd = dm + U * (d + dm)
    var = (d * d).mean(-1, keepdims=True) + 1e-5
    dvar = (2 * d * dd + dd * dd).mean(-1, keepdims=True) + g * var + 2 * U * var
    rstd = 1 / np.sqrt(var)
    drstd = rstd * (0.5 * dvar / np.maximum(var - dvar, 1e-5 * (1 - 8 * U)) + 4 * U)
    core = (d * rstd) * w
    return w * (dd * rstd + d * drstd + dd * drstd) + 3 * U * (core + core + b) + 2.0 ** -126


def fold_bound(x, ln_w, ln_b, u, heads, kind, u24=0):
    """Per-element bound of abar [P, H 576].  kind "mfma": bf16 hi / lo planes of a, u and p, 18 k-steps of 32 dealt over four waves
    (5 each at most, then three adds of the partial tiles), one k-step of 32 token slots for abar; "valu": fp32 chains of 9 + 4 + 3."""
    a = layernorm64(x, ln_w, ln_b).reshape(-1, TOKENS, DIM)
    da = layernorm_bound(x, ln_w, ln_b).reshape(-1, TOKENS, DIM)
    P = a.shape[0]
    uu = np.asarray(u, dtype=np.float64).reshape(P, heads, DIM)
    au, aa = np.abs(uu), np.abs(a)
    if kind == "mfma":
        (ra, ha), (ru, hu) = planes8(aa, da), planes8(au, exact16=bool(u24))
        es = _mm(ru, aa) + _mm(au, ra) + _mm(ru, ra) + _mm(hu, ha) + gamma(3 * 32 * 5 + 5) * _mm(au + 2 * hu, aa + da + 2 * ha)
    else:
        ra, ha = da, 0.0
        es = _mm(au, da) + gamma(9 + 4 + 3 + 2) * _mm(au, aa + da)
    scale = float(DIM // heads) ** -0.5
    s = _mm(uu, a) * scale
    es = scale * es * (1 + 3 * U) + 3 * U * np.abs(s)
    p, dp = _softmax_bound(s, es)
    if kind == "mfma":
        rp, hp = planes8(p, dp)
        eo = rp @ aa + p @ ra + rp @ ra + hp @ ha + gamma(3 * 32 + 2) * ((p + dp + 2 * hp) @ (aa + da + 2 * ha))
    else:
        eo = dp @ aa + (p + dp) @ da + gamma(TOKENS + 2) * ((p + dp) @ (aa + da))
    o = np.abs(p @ a)
    with np.errstate(invalid="ignore"):
        total = eo + out_format_term(np.where(np.isfinite(eo), o + eo, o), SPLIT) + 2.0 ** -126
    return total.reshape(P, heads * DIM)


# ---- float32 evaluations (the yardstick) and the numpy model of the MFMA operand format ----------------------------------------------------
def dense_f32(qkv, heads, cls_only=0):
    t = torch.from_numpy(np.array(qkv, dtype=np.float32))
    P, dh = t.shape[0] // TOKENS, DIM // heads
    q, k, v = (t[:, i * DIM:(i + 1) * DIM].reshape(P, TOKENS, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    if cls_only:
        q = q[:, :, :1]
    p = torch.softmax((q @ k.transpose(-1, -2)) * torch.tensor(float(dh) ** -0.5, dtype=torch.float32), -1)
    o = (p @ v).permute(0, 2, 1, 3)
    return o.reshape(-1, DIM).numpy()


def fold_f32(x, ln_w, ln_b, u, heads):
    f = lambda z: torch.from_numpy(np.array(z, dtype=np.float32))      # noqa: E731
    a = torch.nn.functional.layer_norm(f(x), (DIM,), f(ln_w), f(ln_b), 1e-5).reshape(-1, TOKENS, DIM)
    uu = f(u).reshape(a.shape[0], heads, DIM)
    p = torch.softmax((uu @ a.transpose(-1, -2)) * torch.tensor(float(DIM // heads) ** -0.5, dtype=torch.float32), -1)
    return (p @ a).reshape(a.shape[0], heads * DIM).numpy()


def _hi_lo16(x):
    x = oc.f32(x)
    hi = oc.fp16_sat(x)
    with np.errstate(invalid="ignore"):
        lo = oc.fp16_sat(oc.f32(x - hi))
    return hi.astype(np.float64), lo.astype(np.float64)


def dense_model16(qkv, heads, cls_only=0):
    """numpy model of the MFMA forms' operand format: q / k / v / P as fp16 hi + lo, three terms per product, fp32 results, an fp32
    softmax.  (A model of the FORMAT, not of the kernel: it shows that the bound can be met.)"""
    (qh, ql), (kh, kl), (vh, vl) = (tuple(heads_view(np.ascontiguousarray(p), heads) for p in _hi_lo16(qkv[:, i * DIM:(i + 1) * DIM])) for i in range(3))
    if cls_only:
        qh, ql = qh[:, :, :1], ql[:, :, :1]
    s = oc.f32(_mm(qh, kh) + _mm(qh, kl) + _mm(ql, kh)) * np.float32(float(DIM // heads) ** -0.5)
    e = np.exp(s - s.max(-1, keepdims=True), dtype=np.float32)
    p = e / e.sum(-1, keepdims=True, dtype=np.float32)
    ph, pl = _hi_lo16(p)
    return merge_heads(oc.f32(ph @ vh + ph @ vl + pl @ vh).astype(np.float64))


# ---- decoding the device's rows -----------------------------------------------------------------------------------------------------------
def decode_split_rows(raw, K):
    """[R, 2K] uint16 split rows -> float64 [R, K] = hi + lo"""
    raw = np.asarray(raw, dtype=np.uint16).reshape(-1, 2 * K)
    idx = oc.split_index(np.arange(K))
    hi = oc.from_bits(raw[:, idx].astype(np.uint32) << 16).astype(np.float64)
    lo = oc.from_bits(raw[:, idx + 32].astype(np.uint32) << 16).astype(np.float64)
    return hi + lo


def decode_mixed_rows(raw, K):
    """[R, 4K] bytes of mixed activation rows -> float64 [R, K] = h + X 2^-11 (the value the GEMM behind multiplies with its fp16 weight plane)"""
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1, 4 * K)
    k = np.arange(K)
    hb = raw[:, oc.mixed_h_offset(k)].astype(np.uint16) | (raw[:, oc.mixed_h_offset(k) + 1].astype(np.uint16) << 8)
    h = hb.view(np.float16).astype(np.float64)
    return h + oc.E4M3_VALUE[raw[:, oc.mixed_x_offset(k)]] * 2.0 ** -oc.ACT_RES_EXP


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _seed(family, P, heads, salt):
    return np.random.default_rng([FOLD_FAMILIES.index(family), P, heads, salt])


def route(h):
    """the key that query i of head h selects: a fixed permutation without the identity's fixed points at i = 0"""
    i = np.arange(TOKENS)
    return (7 * i + 3 + h) % TOKENS


def _circle(heads, gap=60.0):
    """q / k directions on a circle in two columns of every head: score(i, j) = R cos(angle_j - angle_route(i)), whose best key leads by
    R (1 - cos(2 pi / 19)) >= gap.  Returns q, k [H, 19, dh]."""
    dh = DIM // heads
    amp = np.sqrt(gap * 1.05 * np.sqrt(dh) / (1 - np.cos(2 * np.pi / TOKENS)))
    ang = 2 * np.pi * np.arange(TOKENS) / TOKENS
    q, k = np.zeros((heads, TOKENS, dh)), np.zeros((heads, TOKENS, dh))
    for h in range(heads):
        c0 = (3 * h) % dh
        c1 = (c0 + dh // 2) % dh
        k[h, :, c0], k[h, :, c1] = amp * np.cos(ang), amp * np.sin(ang)
        q[h, :, c0], q[h, :, c1] = amp * np.cos(ang[route(h)]), amp * np.sin(ang[route(h)])
    return q, k


def _to_rows(x):
    """[P, H, 19, dh] -> [P 19, 576]"""
    return merge_heads(np.asarray(x))


def _value_codes(P, heads, field0):
    """v [P, H, 19, dh] of small integers (|.| <= 2047, exact in fp16): column d carries field d % 4 of (field0, token, head, d // 4)"""
    dh = DIM // heads
    v = np.zeros((P, heads, TOKENS, dh))
    d = np.arange(dh)
    v[..., d % 4 == 0] = np.asarray(field0, dtype=np.float64).reshape(P, 1, TOKENS, 1)
    v[..., d % 4 == 1] = np.arange(TOKENS).reshape(1, 1, TOKENS, 1) + 100.0
    v[..., d % 4 == 2] = -(np.arange(heads).reshape(1, heads, 1, 1) + 200.0)
    v[..., d % 4 == 3] = (d[d % 4 == 3] // 4) + 300.0
    return v


@functools.lru_cache(maxsize=8)
def dense_case(family, P, heads):
    """qkv float32 [P 19, 1728] of a family; plus 'clamped' for the family whose reference is evaluated on the clamped matrix"""
    rng = _seed(family, P, heads, 1)
    dh = DIM // heads
    shape = (P, heads, TOKENS, dh)
    q, k, v = (rng.standard_normal(shape) for _ in range(3))
    if family == "plain":
        q, k, v = (m * (1 + 4 * rng.random((P, 1, TOKENS, 1))) for m in (q, k, v))
    elif family == "sharp":              # scores of standard deviation 10: they reach +-30
        q, k = q * 10 ** 0.5, k * 10 ** 0.5
    elif family == "onehot":             # every query's best key leads by more than 80: the other exponentials underflow
        cq, ck = _circle(heads, gap=85.0)
        q, k = np.broadcast_to(cq, shape).copy(), np.broadcast_to(ck, shape).copy()
    elif family == "flat":               # even heads: all keys of a pair identical; odd heads: an all-zero query
        k[:, 0::2] = k[:, 0::2, :1]
        q[:, 1::2] = 0.0
    elif family == "routing":
        cq, ck = _circle(heads)
        q, k = np.broadcast_to(cq, shape).copy(), np.broadcast_to(ck, shape).copy()
        v = _value_codes(P, heads, np.broadcast_to((np.arange(P) % 2000)[:, None], (P, TOKENS)))
    elif family in ("range", "overflow"):      # |q|, |v| up to 6e4 (k small: the scores stay O(1), and its lo parts fall below 2^-24)
        q = (rng.random(shape) * 2 - 1) * 6.0e4
        k = k * 3.0e-5 / np.sqrt(dh / 72.0)
        v = (rng.random(shape) * 2 - 1) * 6.0e4
        v[..., 0, 0], v[..., 1, 1] = 6.0e4, -6.0e4
        if family == "overflow":         # beyond 65504 in q and in v
            q[..., 2, 0], q[..., 3, 1] = 7.0e4, -1.0e6
            v[..., 0, 2], v[..., 1, 3], v[..., 2, 0], v[..., 18, dh - 1] = 7.0e4, -1.0e6, 65520.0, -7.0e4
    qkv = oc.f32(np.concatenate([_to_rows(q), _to_rows(k), _to_rows(v)], axis=1))
    qkv.setflags(write=False)
    return qkv


def pair_list(P):
    """(subj, obj int32 [P], n_obj): object rows of the per-object tables.  From 3 pairs on: the last object as a subject first (the list
    is not sorted by subject), a pair whose subject row equals its object row, the first and the last object; object 2 is in no pair."""
    n_obj = max(4, int(np.ceil(np.sqrt(P))) + 3)
    last = n_obj - 1
    head = [(last, 0), (1, 1), (0, last)]
    rest = [(s, o) for s in range(n_obj) for o in range(n_obj) if s != 2 and o != 2 and (s, o) not in head]
    order = np.random.default_rng(P).permutation(len(rest))
    pairs = (head + [rest[i] for i in order])[:P]
    return np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32), n_obj


@functools.lru_cache(maxsize=8)
def table_case(family, P, heads):
    """dict(sw, ow [n_obj 16, 1728], stats [P 19, 2], vec [3 1728], subj, obj, qkv [P 19, 1728] (rows 17 / 18 count), n_obj), float32"""
    rng = _seed(family, P, heads, 2)
    dh = DIM // heads
    subj, obj, n_obj = pair_list(P)
    R = n_obj * PATCH

    def cols(part, x):      # [rows, H, dh] -> the q / k / v third of [rows, 1728]
        out = np.zeros((x.shape[0], N3))
        out[:, part * DIM:(part + 1) * DIM] = x.reshape(x.shape[0], DIM)
        return out

    def three(qf, kf, vf, rows):
        return cols(0, qf(rows)) + cols(1, kf(rows)) + cols(2, vf(rows))

    rn = lambda s=1.0: (lambda rows: rng.standard_normal((rows, heads, dh)) * s)      # noqa: E731
    rstd = 0.3 + 2.7 * rng.random((P, TOKENS))
    mean = rng.standard_normal((P, TOKENS))
    if family in ("plain", "sharp"):
        s = 10 ** 0.5 / 2 if family == "sharp" else 1.5
        sw, ow = three(rn(s), rn(s), rn(1.5), R), three(rn(s), rn(s), rn(1.5), R)
        vec = three(rn(s), rn(s), rn(), 3)
        qkv = three(rn(2 * s), rn(2 * s), rn(3.0), P * TOKENS)
    elif family == "flat":               # even heads: every key row of a pair the same; odd heads: zero queries
        rstd[:] = 1.0
        kk = rng.standard_normal((1, heads, dh))
        even = (np.arange(heads) % 2 == 0).reshape(1, heads, 1)
        qf = lambda rows: rng.standard_normal((rows, heads, dh)) * even      # noqa: E731
        kh = lambda w: (lambda rows: np.where(even, w * kk, rng.standard_normal((rows, heads, dh))))      # noqa: E731
        sw, ow = three(qf, kh(1.0), rn(), R), three(qf, kh(0.0), rn(), R)
        vec = three(lambda r: np.zeros((r, heads, dh)), kh(0.0), lambda r: np.zeros((r, heads, dh)), 3)
        vec[2] = three(qf, kh(1.0), rn(), 1)[0]
        qkv = three(qf, kh(1.0), rn(), P * TOKENS)
    elif family in ("onehot", "routing"):      # rstd 1, c2 0, each table half of the circle: the sums are exact
        rstd[:] = 1.0
        cq, ck = _circle(heads, gap=85.0 if family == "onehot" else 60.0)
        tok = lambda m, t: m[:, t].transpose(1, 0, 2)      # noqa: E731  [H, 19, dh] -> the rows of tokens t, [len(t), H, dh]
        patch_t = np.tile(np.arange(1, 17), n_obj)
        half = lambda m: (lambda rows: 0.5 * tok(m, patch_t))      # noqa: E731
        obj_id = np.repeat(np.arange(n_obj), PATCH)
        if family == "routing":          # v names (subject row + 32 x object row | token | head | column): sw and ow each carry their part
            vs = _value_codes(R, heads, np.zeros((R, TOKENS)))[:, :, 0]
            vo = np.zeros_like(vs)
            d = np.arange(dh)
            vs[..., d % 4 == 0] = obj_id.reshape(R, 1, 1)
            vo[..., d % 4 == 0] = 32.0 * obj_id.reshape(R, 1, 1)
            vs[..., d % 4 == 1] = patch_t.reshape(R, 1, 1) + 100.0
            vsf, vof = (lambda rows: vs), (lambda rows: vo)
        else:
            vsf = vof = rn()
        sw, ow = three(half(cq), half(ck), vsf, R), three(half(cq), half(ck), vof, R)
        vec = np.zeros((3, N3))
        every = np.tile(np.arange(TOKENS), P)
        vfull = _value_codes(P, heads, 1500.0 + np.broadcast_to((np.arange(P) % 500)[:, None], (P, TOKENS))) if family == "routing" else None
        vall = (lambda rows: vfull.transpose(0, 2, 1, 3).reshape(P * TOKENS, heads, dh)) if family == "routing" else rn()
        qkv = three(lambda rows: tok(cq, every), lambda rows: tok(ck, every), vall, P * TOKENS)
        vec[2] = qkv[0]
        if family == "routing":
            vec[2, 2 * DIM:] = _value_codes(1, heads, np.full((1, TOKENS), 2040.0))[0, :, 0].reshape(DIM)
    else:                                # range / overflow: |q| and |v| up to 6e4 through both tables, k small
        rstd[:] = 1.0
        big = lambda rows: (rng.random((rows, heads, dh)) * 2 - 1) * 2.9e4      # noqa: E731
        small = rn(1.5e-5 / np.sqrt(dh / 72.0))
        sw, ow = three(big, small, big, R), three(big, small, big, R)
        vec = three(rn(100.0), rn(1e-6), rn(100.0), 3)
        qkv = three(lambda r: 2 * big(r), lambda r: 2 * small(r), lambda r: 2 * big(r), P * TOKENS)
        sw[:, 2 * DIM + 1], ow[:, 2 * DIM + 1], vec[0, 2 * DIM + 1] = 3.0e4, 3.0e4, 0.0      # v column 1 of head 0: 6e4 exactly
        if family == "overflow":
            sw[:, 2 * DIM + 2], ow[:, 2 * DIM + 2] = 3.6e4, 3.4e4               # v column 2 of head 0: 7e4 for every patch token
            sw[:, 5], ow[:, 5] = -5.0e5, -5.0e5                                  # q column 5: -1e6
            qkv[:, 2 * DIM + 7] = -7.0e4
    stats = np.stack([mean, rstd], axis=-1).reshape(P * TOKENS, 2)
    qkv = qkv.reshape(P, TOKENS, N3).copy()
    qkv[:, :17] = 12345.0      # rows 0..16 of qkv are never read by the table form
    t = dict(sw=oc.f32(sw), ow=oc.f32(ow), stats=oc.f32(stats), vec=oc.f32(vec.reshape(3 * N3)), subj=subj, obj=obj,
             qkv=oc.f32(qkv.reshape(P * TOKENS, N3)), n_obj=n_obj)
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def fold_route(h):
    return (5 * h + 2) % TOKENS


@functools.lru_cache(maxsize=8)
def fold_case(family, P, heads):
    """dict(x [P 19, 576], ln_w, ln_b [576], u [P, H 576]) float32"""
    rng = _seed(family, P, heads, 3)
    dh = DIM // heads
    x = rng.standard_normal((P, TOKENS, DIM)) * (1 + 2 * rng.random((P, TOKENS, 1))) + 0.3 * rng.standard_normal((P, TOKENS, 1))
    ln_w, ln_b = 1 + 0.3 * rng.standard_normal(DIM), 0.2 * rng.standard_normal(DIM)
    u = rng.standard_normal((P, heads, DIM)) * 0.5
    if family == "flat":               # even pairs: 19 identical token rows; odd pairs: u = 0
        x[0::2] = x[0::2, :1]
        u[1::2] = 0.0
    elif family == "range":
        x = np.clip(x * 2.0e4, -6.0e4, 6.0e4)
    elif family == "overflow":           # the folded kernels split into bf16 planes (fp32's range): nothing clamps, the plain reference holds
        x = x * 2.0e4
        x[:, :, 0], x[:, :, 5] = 1.0e6, -7.0e4
    elif family == "ln_edges":           # a row mean far from zero; token 3 a constant row (exact in fp32 sums), token 7 one that is not
        x = x * 40 + 15
        x[:, 3], x[:, 7] = 2.5, 0.1
    x, ln_w, ln_b = oc.f32(x.reshape(P * TOKENS, DIM)), oc.f32(ln_w), oc.f32(ln_b)
    if family == "sharp":                # every pair's scores reach 30 in magnitude
        a = layernorm64(x, ln_w, ln_b).reshape(P, TOKENS, DIM)
        s = (u @ a.transpose(0, 2, 1)) * float(dh) ** -0.5
        u = u * (30.0 / np.abs(s).max(-1).max(-1))[:, None, None]
    if family in ("onehot", "routing"):  # u_h along a_t, t = fold_route(h): that token leads by more than the gap
        a = layernorm64(x, ln_w, ln_b).reshape(P, TOKENS, DIM)
        gap = 85.0 if family == "onehot" else 60.0
        for h in range(heads):
            t = fold_route(h)
            others = np.delete(np.arange(TOKENS), t)
            lead = (a[:, t] * a[:, t]).sum(-1) - (a[:, t, None] * a[:, others]).sum(-1).max(-1)
            u[:, h] = a[:, t] * (1.1 * gap * np.sqrt(dh) / lead)[:, None]
    c = dict(x=x, ln_w=ln_w, ln_b=ln_b, u=oc.f32(u.reshape(P, heads * DIM)))
    for a in c.values():
        a.setflags(write=False)
    return c


def clamp16(m):
    """q / k / v clamped to +-65504: what a reading of "the conversions saturate" as a clamp of the OPERAND would give.  Reported, not held:
    see clamp_planes."""
    return np.clip(np.asarray(m, dtype=np.float64), -FP16_MAX, FP16_MAX)


def clamp_planes(m):
    """What the MFMA forms' operand planes hold of a value beyond the fp16 range.  att_split2 (attention.hip) converts x to hi = fp16(x),
    forms l = x - hi in fp32 and converts l to lo, both conversions saturating: for 65504 < |x| <= 2 x 65504 that is hi = 65504 and
    lo = fp16(|x| - 65504), i.e. the operand is still x (to lo's 11 bits: planes16), and only beyond PLANES_MAX = 131008 does it clamp.
    The statement "the conversions saturate" is true of each conversion and does NOT make the operand clamp at 65504; the over-range
    case is therefore held to the reference on the matrix clamped to +-PLANES_MAX.  (Measured against the reference clamped to +-65504
    the MFMA forms are off by the kept excess, e.g. 7e4 - 65504 = 4496 times a probability: test_attention_forward_gpu.py prints that
    figure on its PARITY lines.)"""
    return np.clip(np.asarray(m, dtype=np.float64), -PLANES_MAX, PLANES_MAX)


# ---- what a case is held to ---------------------------------------------------------------------------------------------------------------
def expectation(inst, family, P):
    """dict(ref, bound [rows, cols] float64, yard = the float32 evaluation for the fp32-chain kernels or None, inputs) of one case"""
    return _expectation(inst.id, family, P)


@functools.lru_cache(maxsize=4)
def _expectation(inst_id, family, P):
    inst = BY_ID[inst_id]
    if inst.form in ("dense", "generic"):
        qkv = dense_case(family, P, inst.heads)
        seen = oc.f24(qkv) if inst.f24 else qkv                         # the 3-byte form is held to the reference on the ROUNDED input
        kind = "mfma" if inst.form == "dense" else "valu"
        eff = clamp_planes(seen) if (family == "overflow" and kind == "mfma") else seen.astype(np.float64)      # "the conversions saturate"
        return dict(ref=dense_ref(eff, inst.heads, inst.cls_only), bound=dense_bound(eff, inst.heads, kind, inst.cls_only, inst.o_fmt, inst.f24),
                    yard=dense_f32(seen, inst.heads, inst.cls_only) if kind == "valu" else None, qkv=qkv, seen=seen)
    if inst.form == "table":
        t = table_case(family, P, inst.heads)
        x = table_matrix(t)
        eff = clamp_planes(x) if family == "overflow" else x
        return dict(ref=dense_ref(eff, inst.heads), bound=dense_bound(eff, inst.heads, "mfma", 0, inst.o_fmt, dx=table_dx(t)), yard=None, t=t, x=x)
    if inst.form == "combine":
        t = table_case(family, P, 8)
        return dict(ref=combine_rows(table_matrix(t)), bound=combine_bound(t), yard=combine_rows(table_matrix(t, dtype=np.float32)), t=t)
    c = fold_case(family, P, inst.heads)
    u = oc.f24(c["u"]) if inst.f24 else c["u"]
    kind = "mfma" if inst.form == "fold" else "valu"
    return dict(ref=fold_ref(c["x"], c["ln_w"], c["ln_b"], u, inst.heads), bound=fold_bound(c["x"], c["ln_w"], c["ln_b"], u, inst.heads, kind, inst.f24),
                yard=fold_f32(c["x"], c["ln_w"], c["ln_b"], u, inst.heads) if kind == "valu" else None, c=c, u=u)


def yardstick_allowed(yard, ref, split_rows=True):
    """4 x the worst error of the float32 evaluation on the case + 4 fp32 ulps of the element: what the fp32 CHAIN is held to.  The
    attention kernels then round that result into split rows (16 significant bits, 2^-17 of the element: 64 fp32 ulps), which the
    float32 evaluation does not do, so the rows' own term is added for them; qkv0_combine writes fp32 (split_rows=False)."""
    chain = 4 * np.abs(yard.astype(np.float64) - ref).max() + 4 * ulp32(ref)
    return chain + (out_format_term(np.abs(ref) + chain, SPLIT) if split_rows else 0.0)
