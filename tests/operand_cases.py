"""The GEMM operand formats of veto_amd/csrc/common.h restated in numpy, and the probe inputs built with them (no test lives here;
tests/test_operand_formats_host.py proves the constructions, tests/test_operand_probes_gpu.py runs them on the device).

Written from the comments of common.h, not from the kernels:
  split rows   x ~= hi + lo, hi = bf16(x), lo = bf16(x - hi); per 32 k's 32 hi then 32 lo
  mixed rows   per 64 k's: 64 fp16 h (128 B), then 16 groups of 8 B = { X(4j .. 4j+3), Y(4j .. 4j+3) } of e4m3
               activation rows  X = e4m3(2^11 (a - h)),  Y = e4m3(a)
               weight rows      X = e4m3(2^e h),         Y = e4m3(2^(e+11) (w - h)),  e = weight_exp(max |w|) per tensor
               fp16 saturates at +-65504 and e4m3 at +-448 (the producers switch saturating conversions on); a NaN stays a NaN
  f24          the top three bytes of the fp32 rounded to nearest even at bit 8; NaN keeps sign and exponent, quiet bit set
A selector (one-hot) weight row makes an output element ONE product, whose value then follows from the formats alone: product().

Every rounding takes a `W` (a Wrong instance) so that tests can restate the formats wrongly on purpose (the mutation check)."""
import numpy as np

PRECISE, FAST, MIXED = 0, 1, 2
MODE_NAMES = {PRECISE: "precise", FAST: "fast", MIXED: "mixed"}
ACT_RES_EXP = 11           # activation residual scale 2^11 = the weight residual scale relative to the weight value scale
E4M3_MAX, FP16_MAX = 448.0, 65504.0


class Wrong:
    """Switches of the wrong restatements (all off = the formats as documented)."""
    def __init__(self, **kw):
        self.trunc_fp16 = self.trunc_bf16 = self.trunc_e4m3 = self.trunc_f24 = False
        self.swap_xy_act = self.no_correction = self.exp_plus_one = self.no_saturation = self.lo_from_x = False
        self.reverse_groups = False
        self.res_exp = ACT_RES_EXP
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


RIGHT = Wrong()
MUTATIONS = {
    "fp16 truncates": dict(trunc_fp16=True), "bf16 truncates": dict(trunc_bf16=True), "e4m3 truncates": dict(trunc_e4m3=True),
    "f24 truncates": dict(trunc_f24=True), "X and Y exchanged in activation rows": dict(swap_xy_act=True),
    "no correction term": dict(no_correction=True), "residual scale 2^10": dict(res_exp=10),
    "weight exponent one too high": dict(exp_plus_one=True), "no saturation": dict(no_saturation=True),
    "lo taken from x": dict(lo_from_x=True), "mixed_x_offset with the groups reversed": dict(reverse_groups=True),
}


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def bits(x):
    return f32(x).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint32)).view(np.float32)


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x, W=RIGHT):
    """bf16(x) as a float32 (low 16 bits zero)."""
    b = bits(x).astype(np.uint64)
    r = b if W.trunc_bf16 else b + 0x7fff + ((b >> 16) & 1)
    r = np.where(np.isnan(f32(x)), b | 0x00400000, r) & 0xffff0000
    return from_bits(r.astype(np.uint32))


def split(x, W=RIGHT):
    x = f32(x)
    hi = bf16_rne(x, W)
    with np.errstate(invalid="ignore"):
        lo = bf16_rne(x if W.lo_from_x else x - hi, W)        # x - hi is exact in fp32
    return hi, lo


# ---- fp16 -------------------------------------------------------------------------------------------------------------------------
def _grid_round(v, mant_bits, emin, trunc):
    """float64 v rounded to the grid of a binary format with `mant_bits` stored mantissa bits and smallest normal 2^emin (gradual
    underflow below it); no upper limit.  Exact: v / quantum is a float64 without rounding for float32 inputs."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, ex = np.frexp(v)                                    # |v| in [2^(ex-1), 2^ex)
        q = np.ldexp(1.0, np.maximum(ex - 1, emin) - mant_bits)
        r = (np.trunc(v / q) if trunc else np.rint(v / q)) * q    # np.rint rounds halves to even
    return np.where(np.isfinite(v), r, v)


def fp16_sat(x, W=RIGHT):
    """fp16(x) as a float32: nearest even, every finite value saturating at +-65504; a NaN stays a NaN and a true infinity stays
    an infinity (the saturating mode clamps overflowed results, not infinite inputs)."""
    x = f32(x)
    r = _grid_round(x.astype(np.float64), 10, -14, W.trunc_fp16)
    if W.no_saturation:
        r = np.where(np.abs(r) > FP16_MAX, np.copysign(np.inf, r), r)
    else:
        r = np.where(np.isinf(x), x, np.clip(r, -FP16_MAX, FP16_MAX))                    # (np.clip keeps a NaN)
    return f32(r)


def fp16_bits(h):
    """the 16 bits of an fp16-representable float32"""
    return f32(h).astype(np.float16).view(np.uint16)


# ---- e4m3 (e4m3fn: bias 7, no infinities, 0x7f / 0xff = NaN, largest 448 = 0x7e, smallest subnormal 2^-9) ---------------------------
def _e4m3_table():
    t = np.zeros(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = np.nan if (c & 0x7f) == 0x7f else (m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10))
        t[c] = -v if c & 0x80 else v
    return t


E4M3_VALUE = _e4m3_table()


def e4m3_sat_bits(x, W=RIGHT):
    """x -> e4m3 code (uint8), by hand on the float32 bits: nearest even, gradual underflow, saturating at +-448, NaN -> 0x7f | sign."""
    b = bits(x).astype(np.int64)
    sign = (b >> 31) << 7
    a = b & 0x7fffffff
    E = (a >> 23) - 127
    M = np.where((a >> 23) == 0, 0, (a & 0x7fffff) | 0x800000)          # fp32 subnormals are far below 2^-10: zero
    normal = E >= -6
    shift = np.minimum(np.where(normal, 20, 20 + (-6 - E)), 40)
    q = M >> shift
    rem = M & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    if not W.trunc_e4m3:
        q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    carry = normal & (q == 16)
    En = np.where(carry, E + 1, E)
    qn = np.where(carry, 8, q)
    code = np.where(normal, ((En + 7) << 3) | (qn - 8), q)               # a subnormal that rounds up to 8 is code 8 = 2^-6
    over = normal & ((En > 8) | (code >= 0x7f))
    code = np.where(over, 0x7f if W.no_saturation else 0x7e, code)       # unsaturated: above the 448 / 480 tie the result is NaN
    code = np.where(a > 0x7f800000, 0x7f, code)
    return (code | sign).astype(np.uint8)


def e4m3_sat_bits_torch(x):
    """The same through torch's CPU conversion (nearest even, subnormals kept, NaN above the 448 / 480 tie: hence the clamp first)."""
    import torch
    t = torch.from_numpy(f32(x).copy()).clamp(-E4M3_MAX, E4M3_MAX)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_sat(x, W=RIGHT):
    """e4m3(x) as a float64 value"""
    return E4M3_VALUE[e4m3_sat_bits(x, W)]


# ---- mixed planes -------------------------------------------------------------------------------------------------------------------
def weight_exp(max_abs, W=RIGHT):
    """the largest e in [0, 24] with 2^e max|w| <= 448; an all-zero tensor gets 24"""
    mx = float(np.float32(max_abs))
    e = 24
    while e > 0 and not (mx * 2.0 ** e <= E4M3_MAX):
        e -= 1
    return min(e + 1, 31) if W.exp_plus_one else e


def _scaled(x, e):
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(x) * np.float32(2.0 ** e))                          # a power of two: exact (or an overflow to Inf)


def mixed_act_planes(a, W=RIGHT):
    """(h as float32, X code, Y code) of activation values"""
    a = f32(a)
    h = fp16_sat(a, W)
    with np.errstate(invalid="ignore"):
        x, y = e4m3_sat_bits(_scaled(a - h, W.res_exp), W), e4m3_sat_bits(a, W)
    return (h, y, x) if W.swap_xy_act else (h, x, y)


def mixed_weight_planes(w, e, W=RIGHT):
    """(h as float32, X code, Y code) of weight values of a tensor with exponent e"""
    w = f32(w)
    h = fp16_sat(w, W)
    with np.errstate(invalid="ignore"):
        return h, e4m3_sat_bits(_scaled(h, e), W), e4m3_sat_bits(_scaled(w - h, e + W.res_exp), W)


# ---- f24 ----------------------------------------------------------------------------------------------------------------------------
def f24(x, W=RIGHT):
    """the 3-byte float as a float32 with a zero low byte"""
    b = bits(x).astype(np.uint64)
    r = b if W.trunc_f24 else b + 0x7f + ((b >> 8) & 1)
    r = np.where(np.isnan(f32(x)), b | 0x00400000, r) & 0xffffff00
    return from_bits(r.astype(np.uint32))


# ---- byte layouts -------------------------------------------------------------------------------------------------------------------
def split_index(k):
    """bf16 index of column k's hi inside a split row; its lo is 32 further"""
    k = np.asarray(k)
    return ((k >> 5) << 6) + (k & 31)


def mixed_h_offset(k):
    k = np.asarray(k)
    return ((k >> 6) << 8) + ((k & 63) << 1)


def mixed_x_offset(k, W=RIGHT):
    """byte offset of column k's X inside a mixed row; its Y is 4 further"""
    k = np.asarray(k)
    g = (k & 63) >> 2
    if W.reverse_groups:
        g = 15 - g
    return ((k >> 6) << 8) + 128 + (g << 3) + (k & 3)


def split_rows(x, W=RIGHT):
    """[R, K] fp32 -> [R, 2K] uint16 split rows"""
    x = f32(x)
    R, K = x.shape
    hi, lo = split(x, W)
    out = np.zeros((R, 2 * K), dtype=np.uint16)
    idx = split_index(np.arange(K))
    out[:, idx] = (bits(hi) >> 16).astype(np.uint16)
    out[:, idx + 32] = (bits(lo) >> 16).astype(np.uint16)
    return out


def _mixed_rows(h, x, y, W):
    R, K = h.shape
    out = np.zeros((R, 4 * K), dtype=np.uint8)
    k = np.arange(K)
    hb = fp16_bits(h)
    out[:, mixed_h_offset(k)] = (hb & 0xff).astype(np.uint8)
    out[:, mixed_h_offset(k) + 1] = (hb >> 8).astype(np.uint8)
    out[:, mixed_x_offset(k, W)] = x
    out[:, mixed_x_offset(k, W) + 4] = y
    return out


def mixed_act_rows(a, W=RIGHT):
    """[R, K] fp32 (K % 64 == 0) -> [R, 4K] bytes"""
    return _mixed_rows(*mixed_act_planes(a, W), W)


def mixed_weight_rows(w, W=RIGHT):
    """[R, K] fp32 -> ([R, 4K] bytes, e)"""
    e = weight_exp(np.abs(f32(w)).max(), W)
    return _mixed_rows(*mixed_weight_planes(w, e, W), W), e


def f24_rows(c, W=RIGHT):
    """[R, N] fp32 -> [R, 3N] bytes, low address first: bits 8..15, 16..23, 24..31"""
    b = bits(f24(c, W))
    return np.stack([(b >> 8) & 0xff, (b >> 16) & 0xff, b >> 24], axis=-1).astype(np.uint8).reshape(b.shape[0], -1)


def decode_f24_rows(rows):
    b = rows.reshape(rows.shape[0], -1, 3).astype(np.uint32)
    return from_bits((b[:, :, 0] << 8) | (b[:, :, 1] << 16) | (b[:, :, 2] << 24))


# ---- one product ----------------------------------------------------------------------------------------------------------------------
def product_terms(a, w, mode, e=None, W=RIGHT):
    """The exact terms (float64) whose fp32 sum a single-term GEMM output is."""
    a, w = np.broadcast_arrays(f32(a), f32(w))
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == MIXED:
            ah, xa, ya = mixed_act_planes(a, W)
            wh, xw, yw = mixed_weight_planes(w, e, W)
            main = ah.astype(np.float64) * wh.astype(np.float64)                    # 22 significant bits
            corr = (E4M3_VALUE[xa] * E4M3_VALUE[xw] + E4M3_VALUE[ya] * E4M3_VALUE[yw]) * 2.0 ** -(W.res_exp + e)
            return [main] if W.no_correction else [main, corr]
        (ah, al), (wh, wl) = split(a, W), split(w, W)
        ah, al, wh, wl = (t.astype(np.float64) for t in (ah, al, wh, wl))
        if mode == FAST or W.no_correction:
            return [ah * wh]
        return [ah * wh, al * wh, ah * wl]


def product(a, w, mode, e=None, W=RIGHT):
    """fl32 of the exact sum of the terms: each term is exact in float64 and so is their sum (the terms of one product span fewer
    than 53 bits unless one of them is in fp32's subnormal range, a class the probes exclude), so the cast is the only rounding."""
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(sum(product_terms(a, w, mode, e, W)))


def ulp_key(x):
    """float32 -> int64, monotone in the value: the difference of two keys is their distance in ulps (-0 and +0 coincide)"""
    i = bits(x).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


# ---- derived per-product error bounds -------------------------------------------------------------------------------------------------
def _half_ulp(v, mant_bits, emin):
    """half the spacing of the format's grid at |v| (float64)"""
    _, ex = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.ldexp(0.5, np.maximum(ex - 1, emin) - mant_bits)


def _e4m3_err(v):
    """bound of |e4m3_sat(v) - v| for a float64 v: half a grid step, or the distance to 448 beyond it"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.where(v > E4M3_MAX, v - E4M3_MAX, _half_ulp(np.minimum(v, E4M3_MAX), 3, -6))


def product_bound(a, w, mode, e=None):
    """Bound of |product(a, w, mode) - a w| against float64, from the formats alone (finite a, w):
    precise  a = ah + al + ra, |al| <= hu8(a), |ra| <= hu8(al) (hu8 = half a bf16 step), the same for w; the three kept terms are
             (a - ra)(w - rw) - al wl, so the error is at most |ra||w| + |a||rw| + |ra||rw| + |al||wl| (the dropped second-order term)
    fast     ah wh = (a - al')(w - wl') with |al'| <= hu8(a): |al'||w| + |a||wl'| + |al'||wl'|
    mixed    a = h + l exactly, and h wh + (l + dXa)(wh + dXw) + (a + dYa)(wl + dYw) - a w has NO dropped term (a wl = h wl + l wl):
             |l| dXw + dXa |wh| + dXa dXw + |a| dYw + dYa |wl| + dYa dYw, each d = half an e4m3 step of the plane's scaled value over
             its scale, or its distance to 448 where it saturates (fp16's own saturation is inside l)
    plus 2^-23 of the result for the one fp32 rounding of the sum (either direction) and one step of fp32's subnormal grid."""
    a, w = np.broadcast_arrays(f32(a).astype(np.float64), f32(w).astype(np.float64))
    aa, aw = np.abs(a), np.abs(w)
    if mode == MIXED:
        ha, hw = fp16_sat(a).astype(np.float64), fp16_sat(w).astype(np.float64)
        la, lw = np.abs(a - ha), np.abs(w - hw)
        s = 2.0 ** ACT_RES_EXP
        dXa, dYa = _e4m3_err(la * s) / s, _e4m3_err(aa)
        dXw, dYw = _e4m3_err(np.abs(hw) * 2.0 ** e) / 2.0 ** e, _e4m3_err(lw * s * 2.0 ** e) / (s * 2.0 ** e)
        err = la * dXw + dXa * np.abs(hw) + dXa * dXw + aa * dYw + dYa * lw + dYa * dYw
    else:
        hu = lambda v: _half_ulp(v, 7, -126)      # noqa: E731
        al, wl = hu(aa), hu(aw)
        if mode == FAST:
            err = al * aw + aa * wl + al * wl
        else:
            ra, rw = hu(al), hu(wl)
            err = ra * aw + aa * rw + ra * rw + al * wl
    return err + 2.0 ** -23 * (aa * aw + err) + 2.0 ** -149


# ---- probe values ---------------------------------------------------------------------------------------------------------------------
def _pm(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, -v])


def _next_up(x, n=1):
    """the float32 n steps above a positive scalar x, as a Python float"""
    return float(from_bits(bits(x).ravel()[:1] + np.uint32(n))[0])


def activation_classes():
    """name -> float32 values; every class is a value CLASS of the layout (one residue of class_of)."""
    rng = np.random.default_rng(20240607)
    c = {}
    E = np.array([-6, -3, 0, 1, 5, 8])                                     # binades inside e4m3's normal range and |a| <= 448
    m_even, m_odd = np.array([0, 2, 512, 1022]), np.array([1, 3, 511, 1023])
    tie16 = lambda m: ((1024 + m[None, :] + 0.5) * 2.0 ** (E[:, None] - 10)).ravel()      # noqa: E731  halfway between two fp16
    c["fp16_tie_down"] = _pm(tie16(m_even))                               # RNE keeps the even lower neighbour
    c["fp16_tie_up"] = _pm(tie16(m_odd))
    m8e, m8o = np.array([0, 2, 64, 126]), np.array([1, 3, 65, 127])
    tie8 = lambda m: ((128 + m[None, :] + 0.5) * 2.0 ** (E[:, None] - 7)).ravel()         # noqa: E731  halfway between two bf16
    c["bf16_hi_tie_down"] = _pm(tie8(m8e))
    c["bf16_hi_tie_up"] = _pm(tie8(m8o))
    # x = hi + (a 9-bit residual that is a bf16 tie), 10 binades below hi: the rounding of lo itself ties, both directions; and the
    # values whose 16-bit form ties again in the f24 epilogue (1 + 2^-16: low byte 0x80, even; 1 + 2^-15 + 2^-16: odd)
    lo_tie = (128 + np.concatenate([m8e, m8o]) + 0.5) * 2.0 ** (-10 - 7)
    c["bf16_lo_tie"] = _pm(np.concatenate([1.5 + lo_tie, 6.0 + 4 * lo_tie, [1 + 2.0 ** -16, 1 + 2.0 ** -15 + 2.0 ** -16,
                                                                                   1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]]))
    c["zero_residual"] = _pm([1.0, 1.5, 0.375, 3.0, 96.0, 2.0 ** -6, 0.4375, 224.0, 7.0, 2.0 ** -10, 0.0078125 * 5])
    # one float below a tie: the largest fp16 residual, with low bits that the e4m3 rounding of 2^11 l must carry upwards
    c["max_residual"] = f32(np.concatenate([from_bits(bits(f32(tie16(m_even))) - np.uint32(1)),
                                            -from_bits(bits(f32(tie16(m_odd))) - np.uint32(1))]))
    # e4m3 ties: X = 2^11 l halfway between two e4m3 values, one and two binades below h's; Y = a halfway (then l = 0)
    j_even, j_odd = np.array([0, 2, 6]), np.array([1, 3, 7])
    xt = []
    for Eh in (0, 4, 8):
        for F in (Eh - 1, Eh - 2):
            for j in np.concatenate([j_even, j_odd]):
                xt.append(1.25 * 2.0 ** Eh + (8 + j + 0.5) * 2.0 ** (F - 3 - ACT_RES_EXP))
    yt = [(8 + j + 0.5) * 2.0 ** (F - 3) for F in (-6, 0, 8) for j in np.concatenate([j_even, j_odd])]
    c["e4m3_tie"] = _pm(np.concatenate([xt, yt]))
    c["clamp_448"] = _pm(np.concatenate([[448.0, float(_next_up(448.0)), 464.0, float(_next_up(464.0)), 480.0, 1000.0, 447.9, 500.123,
                                          1000.3, 3000.7]]))
    c["clamp_65504"] = _pm([65504.0, _next_up(65520.0, 0xffffffff), 65520.0, 7.0e4, 65503.0, 60000.5, 65536.0, 1.0e6])
    c["fp16_subnormal"] = _pm([2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -15 + 2.0 ** -26,
                               1.1e-5, 2.0 ** -14 + 2.0 ** -25])
    # 2^11 l inside e4m3's subnormal range [2^-9, 2^-6): exact, ties to even in both directions, and inexact
    c["e4m3_subnormal_residual"] = _pm([1 + 3 * 2.0 ** -20, 1 + 2.5 * 2.0 ** -20, 1 + 1.5 * 2.0 ** -20, 1 + 2.0 ** -20, 1 + 7 * 2.0 ** -20,
                                        1 + 6.3 * 2.0 ** -20, 0.03125 + 5 * 2.0 ** -20, 2.0 ** -8, 3 * 2.0 ** -9, 2.5 * 2.0 ** -9])
    # 2^11 l at or below half the smallest subnormal (2^-10): the tie goes to zero; Y below it as well
    c["e4m3_below_subnormal"] = _pm([1 + 2.0 ** -21, 1 + 2.0 ** -22, 1 + 2.0 ** -23, 0.5 + 2.0 ** -22, 1 + 2.0 ** -21 + 2.0 ** -23, 2.0 ** -10,
                                     2.0 ** -11, 2.0 ** -10 + 2.0 ** -20])
    c["zero_and_fp32_subnormal"] = f32([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -130, 2.0 ** -126, -2.0 ** -126,
                                        3 * 2.0 ** -128, 0.0])
    c["normal"] = f32(rng.standard_normal(256))
    c["outlier"] = f32(rng.standard_normal(256) * 30.0)
    assert len(c) == N_CLASSES
    return {k: f32(v) for k, v in c.items()}


N_CLASSES = 16
NONFINITE = from_bits(np.uint32([0x7f800000, 0xff800000, 0x7fc00000, 0xffffffff, 0x7f800001]))     # +-Inf, three NaNs


def class_of(m, k):
    """Value class of element (m, k): for a fixed k slot of a 64-block and a fixed swizzle class (m >> 1) & 7 the class walks
    through all 16 with m >> 4 (16 consecutive 16-row groups), and the 64-blocks of a row start one class apart."""
    return ((k & 63) + (k >> 6) + (m >> 4) + 3 * ((m >> 1) & 7)) % N_CLASSES


def activation_matrix(M, K, classes=None):
    """A [M, K] of probe values, and the class index of every element"""
    classes = classes or activation_classes()
    names = list(classes)
    m, k = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
    cls = class_of(m, k)
    a = np.zeros((M, K), dtype=np.float32)
    for ci, name in enumerate(names):
        v = classes[name]
        sel = cls == ci
        a[sel] = v[(m[sel] * 131 + k[sel] * 31 + (k[sel] >> 6) * 7) % len(v)]
    return a, cls


def weight_sets():
    """name -> (values that the selector rows carry, cyclically; the tensor's exponent follows from their maximum)"""
    rng = np.random.default_rng(99)
    common = np.array([1.0, -0.75, 0.3, -0.123456, 0.04, (1024 + 5 + 0.5) * 2.0 ** -17, -(1024 + 6 + 0.5) * 2.0 ** -15,   # fp16 ties
                       (128 + 3 + 0.5) * 2.0 ** -9, 0.011, -(1 + 2.0 ** -16) / 8, 0.2 + 2.0 ** -20])
    s = {}
    s["zeros"] = np.zeros(4)
    s["tiny"] = np.array([448 * 2.0 ** -24 * 0.99, -1.3e-5, 2.0 ** -17, 7.77e-6, -2.0 ** -24, 1.9e-5])           # e = 24
    s["boundary_e10"] = np.concatenate([[448 * 2.0 ** -10], common[2:]])                                     # exactly 448 * 2^-10
    s["boundary_e9"] = np.concatenate([[float(_next_up(448 * 2.0 ** -10))], common[2:]])                     # one float above it
    s["max_448"] = np.concatenate([[448.0, -100.5, 17.03125], common])                                             # e = 0
    s["above_448"] = np.concatenate([[1000.0, -448.0, 480.0, 464.0, 600.7], common])                               # e = 0, X saturates
    s["ordinary"] = np.concatenate([rng.standard_normal(64) * 0.04, common[3:] * 0.125])
    return {k: f32(v) for k, v in s.items()}


def sigma(name, N, K, seed=0):
    """the k of selector row n"""
    n = np.arange(N)
    if name == "identity":
        return n % K
    if name == "reversal":
        return (K - 1 - n) % K
    perm = np.random.default_rng(1000 + seed + K).permutation(K)
    return perm[(n * 7 + n // K) % K]


def selector_weight(N, K, values, sig, outside=0.0):
    """W [N, K]: row n holds values[n % len] at k = sig[n] and `outside` elsewhere; also the per-row value"""
    wv = f32(values)[np.arange(N) % len(values)]
    w = np.full((N, K), outside, dtype=np.float32)
    w[np.arange(N), sig] = wv
    return w, wv


def excluded(a, w, mode, e=None):
    """Elements left out of the bit-exact claim, by value range alone: a bf16 plane, a term or the result in fp32's subnormal range,
    0 < |.| < 2^-126 (the matrix pipe may flush it).  fp16 and e4m3 subnormals are NOT excluded."""
    a, w = np.broadcast_arrays(f32(a), f32(w))
    tiny32 = lambda v: (np.abs(v) < 2.0 ** -126) & (v != 0)              # noqa: E731
    terms = product_terms(a, w, mode, e)
    ex = tiny32(sum(terms))
    for t in terms:
        ex |= tiny32(t)
    if mode != MIXED:
        for p in split(a) + split(w):
            ex |= tiny32(p)
    return ex


def excluded_bound(a, w, mode, e=None):
    """What an excluded element is held to instead: the derived bound plus every term that could be flushed (a flushed operand or
    term removes at most that term; a flushed result at most 2^-126)."""
    terms = product_terms(a, w, mode, e)
    return product_bound(a, w, mode, e) + _flush_allowance(a, w, mode, e, terms)


def _flush_allowance(a, w, mode, e, terms):
    a, w = np.broadcast_arrays(f32(a), f32(w))
    tiny32 = lambda v: (np.abs(v) < 2.0 ** -126) & (v != 0)              # noqa: E731
    allow = np.full(a.shape, 2.0 ** -126)
    if mode != MIXED:
        (ah, al), (wh, wl) = split(a), split(w)
        allow = allow + np.where(tiny32(ah) | tiny32(wh), sum(np.abs(t) for t in terms), 0.0)
        if len(terms) == 3:
            allow = allow + np.where(tiny32(al), np.abs(terms[1]), 0.0) + np.where(tiny32(wl), np.abs(terms[2]), 0.0)
    for t in terms:
        allow = allow + np.where(tiny32(t), np.abs(t), 0.0)
    return allow


# ---- the selector cases of the device test ----------------------------------------------------------------------------------------------
SELECTOR_SHAPES = [   # (M, N, K, precisions)
    (513, 576, 576, (PRECISE, FAST, MIXED)),
    (1, 192, 64, (PRECISE, FAST, MIXED)), (255, 192, 64, (PRECISE, FAST, MIXED)),
    (1, 192, 32, (PRECISE, FAST)), (255, 192, 32, (PRECISE, FAST)),
    (257, 1152, 1152, (PRECISE, FAST, MIXED)),
]
SIGMAS = ("identity", "reversal", "permutation")
TILE_WALK = dict(M=14592, N=1728, period=509)      # 57 x 9 = 513 tiles of 256 x 192; rows repeat with a prime period


def wgrad_rows(m, ks):
    """the rows of dy that carry an entry: first and last, both sides of the multiples of 32 and 256 next to the ends, and of every
    split-K boundary (the reduction rows are padded to a multiple of 32 ks and cut into ks equal ranges)"""
    mp = (m + 32 * ks - 1) // (32 * ks) * (32 * ks)
    rows = {0, m - 1}
    for step in (32, 256):
        last = (m - 1) // step * step
        for b in (step, 2 * step, last - step, last):
            rows |= {b - 1, b}
    for i in range(1, ks):
        rows |= {i * (mp // ks) - 1, i * (mp // ks)}
    return sorted(r for r in rows if 0 <= r < m)
