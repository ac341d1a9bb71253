"""Bit-level probes of the GEMM operand formats on the MI355X (tests/operand_cases.py builds the inputs and restates the formats;
tests/test_operand_formats_host.py proves both on the CPU).  With a one-hot ("selector") weight row every output element of
gemm_split_ps_kernel is ONE product of a probe value and a weight value, whose bits follow from the format definitions: it is
compared with product() to bit equality or one fp32 ulp (the one accumulation in the matrix pipe, whose rounding nobody has written
down), and the operand rows that split_rows_kernel, mixed_act_rows_kernel, absmax_bits_kernel + mixed_weight_rows_kernel leave in
the hook's workspace are compared byte for byte.  Every output goes into a sentinel-filled buffer with spare rows behind it, every
call runs twice and must repeat itself.

Left out of the bit-exact claim, by value range defined on the CPU before the run (operand_cases.excluded): elements with a bf16
plane, a term or the result in fp32's subnormal range (the matrix pipe may flush them) -- held to the derived value bound plus what
a flush can remove -- and non-finite inputs, which have cases of their own.  fp16 and e4m3 subnormals are inside the claim.  Nothing
else has a tolerance.

What the device does, as measured (profiles/operand_probes_parity.txt has the figures that every test prints): the fast mode is
bit-equal everywhere; the precise mode is bit-equal on about 98 % of the elements and one ulp off on the rest (three MFMAs, each
rounding its partial sum), the mixed mode bit-equal but for about 0.1 % one ulp off; operand rows, split-row and f24 bytes equal
the restatement's without exception, subnormals included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operand_cases as oc  # noqa: E402
from operand_cases import FAST, MIXED, PRECISE  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fa5a5a5           # a NaN pattern no kernel here produces
SPARE = 3                       # rows behind every output
BM = 256                        # activation rows of the hook's workspace are padded to whole GEMM tiles


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from veto_amd import native
    return native, native.load_library()


def _sentinel(rows, cols, dtype=torch.float32):
    t = torch.empty((rows + SPARE, cols), dtype=dtype, device=_dev())
    if dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL)
    else:
        t.view(torch.uint8).fill_(0xA5)
    return t


def _twice(call, rows, cols, dtype=torch.float32):
    """call(out) into a fresh sentinel-filled buffer, twice: the valid rows of the second run, after asserting that both runs left the
    same bytes and that the spare rows still hold the sentinel"""
    outs = []
    for _ in range(2):
        out = _sentinel(rows, cols, dtype)
        call(out)
        torch.cuda.synchronize()
        outs.append(out)
    a, b = (o.view(torch.uint8) for o in outs)
    assert torch.equal(a, b), "two calls of the same inputs differ"
    assert torch.equal(b[rows:], _sentinel(0, cols, dtype).view(torch.uint8)), "the rows behind the output were written"
    return outs[1][:rows]


def _gemm(a, w, bias, mode):
    """C [m, n] of veto_debug_gemm (twice), and the workspace it left"""
    native, lib = _lib()
    (m, k), n = a.shape, w.shape[0]
    ws = torch.full((lib.veto_debug_gemm_workspace_bytes(m, n, k),), 0xA5, dtype=torch.uint8, device=_dev())

    def call(c):
        native.check(lib.veto_debug_gemm(None, a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, c.data_ptr(),
                                         m, n, k, mode, ws.data_ptr(), ws.numel()))
    return _twice(call, m, n), ws


def _forms(a, w, form, kb_tiles, kb_steps):
    native, lib = _lib()
    (m, k), n = a.shape, w.shape[0]
    ws = torch.full((lib.veto_debug_gemm_workspace_bytes(m, n, k),), 0xA5, dtype=torch.uint8, device=_dev())
    cols, dtype = {0: (n, torch.float32), 1: (2 * n, torch.bfloat16), 2: (3 * n, torch.uint8)}[form]

    def call(c):
        native.check(lib.veto_debug_gemm_forms(None, a.data_ptr(), w.data_ptr(), c.data_ptr(), m, n, k, kb_tiles, kb_steps, form,
                                               ws.data_ptr(), ws.numel()))
    return _twice(call, m, cols, dtype)


def _key(t):
    """float32 tensor -> int64, monotone in the value (operand_cases.ulp_key on the device)"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7fffffff), i)


class Table:
    """Expected values of every (distinct probe value, weight value) pair of a case, computed once on the CPU and gathered per element:
    a probe matrix holds some 700 distinct values and a weight set at most 80."""

    def __init__(self, a, wvals, mode):
        self.ua, inv = np.unique(oc.bits(a), return_inverse=True)
        self.inv = inv.reshape(a.shape)
        ua, wv = oc.from_bits(self.ua)[:, None], oc.f32(wvals)[None, :]
        self.e = oc.weight_exp(np.abs(wvals).max())
        self.product = oc.product(ua, wv, mode, self.e)
        self.exact = ua.astype(np.float64) * wv.astype(np.float64)
        self.excluded = oc.excluded(ua, wv, mode, self.e)
        self.bound = np.where(self.excluded, oc.excluded_bound(ua, wv, mode, self.e), oc.product_bound(ua, wv, mode, self.e))

    def gather(self, field, sig, n_vals):
        """[M, N] of a field for selector rows n -> (k = sig[n], value index n % n_vals)"""
        return getattr(self, field)[self.inv[:, sig], (np.arange(len(sig)) % n_vals)[None, :]]


def _expected(tab, sig, n_vals, dev, bias=None):
    """The table gathered for selector rows n -> (k = sig[n], value n % n_vals), on the device.  With a bias the device computes
    fl32(p + bias) from its own p, which may be the neighbour of the restatement's: there are three candidates."""
    p = tab.gather("product", sig, n_vals)
    exact, bound = tab.gather("exact", sig, n_vals), tab.gather("bound", sig, n_vals)
    cands = [p]
    if bias is not None:
        b64 = bias.astype(np.float64)[None, :]
        cands = [oc.f32(oc.from_bits((oc.bits(p).astype(np.int64) + s).astype(np.uint32)).astype(np.float64) + b64) for s in (0, 1, -1)]
        exact, bound = exact + b64, bound + np.abs(b64) * 2.0 ** -23
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    return {"cands": cands, "keys": [_key(up(x)) for x in cands], "excluded": up(tab.gather("excluded", sig, n_vals)), "exact": up(exact),
            "bound": up(bound)}


def _check_products(c, exp, what="", rows=None):
    """c [M, N] against _expected (its first `rows` rows): bit equality or one ulp on every element outside the excluded classes, the
    value bound on all.  Returns (elements, bit-equal, one ulp off / a neighbour's sum, excluded, bit-equal among the excluded, worst
    fraction of the bound)."""
    r = slice(0, c.shape[0] if rows is None else rows)
    excl, kc = exp["excluded"][r], _key(c)
    ds = torch.stack([(kc - k[r]).abs() for k in exp["keys"]])
    d = ds[0] if len(exp["keys"]) == 1 else torch.where(ds.min(dim=0).values == 0, ds[0].clamp_max(1), ds[0].clamp_min(2))
    finite = torch.isfinite(c)
    assert finite.all(), "%s: %d non-finite outputs" % (what, int((~finite).sum()))
    bad = (d > 1) & ~excl
    if bad.any():
        i = torch.nonzero(bad)[:8].cpu().numpy()
        p = exp["cands"][0]
        txt = ["(m %d, n %d): got %s want %s" % (a, q, hex(int(c[a, q].view(torch.int32)) & 0xffffffff), hex(int(oc.bits(p[a, q])[0]))) for a, q in i]
        raise AssertionError("%s: %d of %d elements differ by more than one ulp: %s" % (what, int(bad.sum()), c.numel(), "; ".join(txt)))
    frac = (c.double() - exp["exact"][r]).abs() / exp["bound"][r]
    assert frac.max().item() <= 1.0, "%s: %.3f of the value bound" % (what, frac.max().item())
    ok = ~excl
    return c.numel(), int(((d == 0) & ok).sum()), int(((d == 1) & ok).sum()), int(excl.sum()), int(((d == 0) & excl).sum()), frac.max().item()


def _planes_of_mixed_rows(rows, k):
    """[R, 4K] bytes -> (h bits uint16, X, Y) per column, through the restated offsets"""
    kk = np.arange(k)
    h = rows[:, oc.mixed_h_offset(kk)].astype(np.uint16) | (rows[:, oc.mixed_h_offset(kk) + 1].astype(np.uint16) << 8)
    return h, rows[:, oc.mixed_x_offset(kk)], rows[:, oc.mixed_x_offset(kk) + 4]


def _check_workspace_rows(ws, a, w, mode):
    """The operand rows behind a veto_debug_gemm call (activation rows padded to whole tiles, then the weight rows, then the mixed
    weights' exponent) equal the restatement's bytes; returns the number of bytes compared."""
    (m, k), n = a.shape, w.shape[0]
    mp = (m + BM - 1) // BM * BM
    raw = ws.cpu().numpy()
    a_rows, w_rows = raw[:m * 4 * k].reshape(m, 4 * k), raw[mp * 4 * k:mp * 4 * k + n * 4 * k].reshape(n, 4 * k)
    assert not raw[m * 4 * k:mp * 4 * k].any(), "the padding rows of the activation operand are not zero"
    if mode == MIXED:
        want_a, (want_w, e) = oc.mixed_act_rows(a), oc.mixed_weight_rows(w)
        assert int(raw[(mp + n) * 4 * k:(mp + n) * 4 * k + 4].view(np.int32)[0]) == e, "weight exponent"
        for got, want, x in ((a_rows, want_a, a), (w_rows, want_w, w)):       # (fp16 and e4m3 subnormals included: nothing is left out)
            for name, g, q in zip("hXY", _planes_of_mixed_rows(got, k), _planes_of_mixed_rows(want, k)):
                diff = g != q
                assert not diff.any(), "mixed rows, plane %s: %d bytes differ, first at %s: got %s want %s (value %r)" % (
                    name, diff.sum(), np.argwhere(diff)[0], hex(g[diff][0]), hex(q[diff][0]), x[diff][0])
            assert np.array_equal(got, want)
    else:
        for got, want, x in ((a_rows, oc.split_rows(a), a), (w_rows, oc.split_rows(w), w)):
            got = got.view(np.uint16)
            kk = np.arange(k)
            tiny = (np.abs(x) < 2.0 ** -100) & (x != 0)       # a part in fp32's subnormal range: excluded
            for off, name in ((0, "hi"), (32, "lo")):
                g, q = got[:, oc.split_index(kk) + off], want[:, oc.split_index(kk) + off]
                diff = (g != q) & ~tiny
                assert not diff.any(), "split rows, plane %s: %d values differ, first at %s: got %s want %s (value %r)" % (
                    name, diff.sum(), np.argwhere(diff)[0], hex(g[diff][0]), hex(q[diff][0]), x[diff][0])
    return a_rows.size + w_rows.size


@pytest.fixture(scope="module")
def probes():
    classes = oc.activation_classes()
    return {"classes": classes, "weights": oc.weight_sets(), "log": []}


@pytest.mark.parametrize("sig_name", oc.SIGMAS)
@pytest.mark.parametrize("m,n,k,modes", oc.SELECTOR_SHAPES, ids=["%dx%dx%d" % s[:3] for s in oc.SELECTOR_SHAPES])
def test_selector_products(m, n, k, modes, sig_name, probes, capsys):
    """Every probe value class in every k slot and swizzle class, times every weight set, in every precision: one product per element."""
    dev = _dev()
    a, _ = oc.activation_matrix(m, k, probes["classes"])
    a_t = torch.from_numpy(a).to(dev)
    sig = oc.sigma(sig_name, n, k)
    lines = []
    for wname, vals in probes["weights"].items():
        w, _ = oc.selector_weight(n, k, vals, sig)
        w_t = torch.from_numpy(w).to(dev)
        for mode in modes:
            c, ws = _gemm(a_t, w_t, None, mode)
            tab = Table(a, vals, mode)
            total, same, one, excl, excl_same, frac = _check_products(c, _expected(tab, sig, len(vals), dev), "%s %s %s" % (wname, oc.MODE_NAMES[mode], sig_name))
            if mode != FAST and sig_name == "permutation" and k <= 576:
                _check_workspace_rows(ws, a, w, mode)
            lines.append("%-13s %-8s e %2d: %7d elements, %7d bit-equal, %5d one ulp off, %6d excluded (%6d of them bit-equal), worst %.3f of the bound"
                         % (wname, oc.MODE_NAMES[mode], tab.e, total, same, one, excl, excl_same, frac))
    with capsys.disabled():
        print("\n[operand probes] selector M %d N %d K %d sigma %s\n  %s" % (m, n, k, sig_name, "\n  ".join(lines)))


@pytest.mark.parametrize("k,mode", [(64, PRECISE), (64, FAST), (64, MIXED), (32, PRECISE)])
def test_more_tiles_than_workgroups(k, mode, probes, capsys):
    """513 tiles (57 x 9) on at most 256 persistent workgroups, with a bias: the tile walk, the loaders running into the next tile (a
    tile is one or two k-steps here) and the three bias slices.  Rows repeat with the prime period 509, so no two row tiles of the
    walk hold the same data; expected = fl32(product + bias) everywhere."""
    dev = _dev()
    M, N, P = oc.TILE_WALK["M"], oc.TILE_WALK["N"], oc.TILE_WALK["period"]
    base, _ = oc.activation_matrix(P, k, probes["classes"])
    vals = probes["weights"]["ordinary"]
    sig = oc.sigma("permutation", N, k)
    w, _ = oc.selector_weight(N, k, vals, sig)
    bias = oc.f32(((np.arange(N) * 37) % 513 - 256) / 64.0)              # multiples of 2^-6 in [-4, 4], a different one per column of a tile
    rows = torch.arange(M, device=dev) % P
    a_t = torch.from_numpy(base).to(dev)[rows].contiguous()
    c, _ = _gemm(a_t, torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev), mode)
    tab = Table(base, vals, mode)
    # compare the 509 distinct rows' expectation with every row of C that holds them
    exp = _expected(tab, sig, len(vals), dev, bias=bias)
    tot = [0, 0, 0, 0, 0, 0.0]
    for r0 in range(0, M, P):
        r1 = min(r0 + P, M)
        res = _check_products(c[r0:r1], exp, "rows %d..%d" % (r0, r1), rows=r1 - r0)
        tot = [x + y for x, y in zip(tot[:5], res[:5])] + [max(tot[5], res[5])]
    with capsys.disabled():
        print("\n[operand probes] tile walk K %d %s: %d elements, %d equal to fl32(p + bias), %d to a neighbour's, %d excluded (%d of them equal), worst "
              "%.3f of the bound" % (k, oc.MODE_NAMES[mode], *tot))


@pytest.mark.parametrize("kb_tiles,kb_steps", [(0, 0), (1, 6), (3, 18)])
def test_output_forms(kb_tiles, kb_steps, probes, capsys):
    """The split-row and 3-byte epilogues on selector products (M 513, N = K = 576), dense and block-diagonal (selectors inside their
    blocks, NaN outside): the fp32 form within one ulp of the restatement, and the other two forms equal to the restatement's bytes
    of that fp32 result -- layout, rounding at ties, zero low byte."""
    dev = _dev()
    m, n, k = 513, 576, 576
    a, _ = oc.activation_matrix(m, k, probes["classes"])
    vals = probes["weights"]["max_448"]              # holds 1.0: the 16-bit form of a probe value reaches the epilogue unchanged
    if kb_tiles:
        blk = kb_steps * 32
        first = (np.arange(n) // 192 // kb_tiles) * blk
        sig = first + oc.sigma("permutation", n, blk)
        w, _ = oc.selector_weight(n, k, vals, sig, outside=np.nan)
        for j in range(n):
            w[j, first[j]:first[j] + blk] = np.where(np.isnan(w[j, first[j]:first[j] + blk]), 0.0, w[j, first[j]:first[j] + blk])
        assert np.isnan(w).sum() == n * (k - blk)
    else:
        sig = oc.sigma("permutation", n, k)
        w, _ = oc.selector_weight(n, k, vals, sig)
    a_t, w_t = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    c = _forms(a_t, w_t, 0, kb_tiles, kb_steps)
    tab = Table(a, vals, PRECISE)
    res = _check_products(c, _expected(tab, sig, len(vals), dev), "form 0 kb (%d, %d)" % (kb_tiles, kb_steps))
    c_np = c.cpu().numpy()
    ties24, ties16 = int(((oc.bits(c_np) & 0xff) == 0x80).sum()), int(((oc.bits(c_np) & 0xffff) == 0x8000).sum())
    assert ties24 > 100 and ties16 > 100, (ties24, ties16)               # the epilogues' own roundings meet ties
    sp = _forms(a_t, w_t, 1, kb_tiles, kb_steps).view(torch.int16).cpu().numpy().view(np.uint16)
    tiny = (np.abs(c_np) < 2.0 ** -100) & (c_np != 0)                      # (a part in fp32's subnormal range: excluded)
    want = oc.split_rows(c_np)
    nn = np.arange(n)
    for off in (0, 32):
        g, q = sp[:, oc.split_index(nn) + off], want[:, oc.split_index(nn) + off]
        assert not ((g != q) & ~tiny).any(), "split-row epilogue, %s plane: %d differ" % ("lo" if off else "hi", ((g != q) & ~tiny).sum())
    f24 = _forms(a_t, w_t, 2, kb_tiles, kb_steps).cpu().numpy()
    assert np.array_equal(f24, oc.f24_rows(c_np)), "f24 epilogue: %d bytes differ" % (f24 != oc.f24_rows(c_np)).sum()
    with capsys.disabled():
        print("\n[operand probes] forms kb (%d, %d): fp32 %d elements, %d bit-equal, %d one ulp off, %d excluded (%d of them bit-equal); f24 ties "
              "%d, bf16 ties %d; split rows and f24 bytes equal the restatement's" % (kb_tiles, kb_steps, *res[:5], ties24, ties16))


def test_output_forms_keep_non_finite_values(probes, capsys):
    """A NaN stays a NaN and an infinity never becomes finite, in all three forms: rows holding one Inf / -Inf / NaN (NaN in every
    column, the lo plane of an Inf being Inf - Inf), and a row whose products overflow fp32 (a true Inf in the accumulator)."""
    dev = _dev()
    m, n, k = 513, 576, 576
    a, _ = oc.activation_matrix(m, k, probes["classes"])
    for r, v in enumerate(oc.NONFINITE):
        a[r, 7 + 64 * r] = v
    a[5, :] = 3.0e38
    a[300, :] = -3.0e38
    vals = probes["weights"]["max_448"]
    sig = oc.sigma("permutation", n, k)
    w, wv = oc.selector_weight(n, k, vals, sig)
    a_t, w_t = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    c = _forms(a_t, w_t, 0, 0, 0).cpu().numpy()
    sp = _forms(a_t, w_t, 1, 0, 0).view(torch.int16).cpu().numpy().view(np.uint16)
    f24 = oc.decode_f24_rows(_forms(a_t, w_t, 2, 0, 0).cpu().numpy())
    hi = oc.from_bits(sp[:, oc.split_index(np.arange(n))].astype(np.uint32) << 16)
    nan_rows, inf_rows = [2, 3, 4], [0, 1]
    for name, x in (("fp32", c), ("f24", f24), ("split hi", hi)):
        assert np.isnan(x[nan_rows]).all(), name
        assert (~np.isfinite(x[inf_rows])).all(), name
        assert np.isfinite(x[6:300]).all() and np.isfinite(x[301:]).all(), name
    want = oc.product(a[5][sig][None, :], wv[None, :], PRECISE)[0]
    over = np.isinf(want)
    assert over.sum() > 100 and (~over).sum() > 100
    for name, x in (("fp32", c), ("f24", f24), ("split hi", hi)):
        assert np.array_equal(x[5][over], want[over]) and np.array_equal(x[300][over], -want[over]), name     # +-Inf of the product's sign
        assert np.isfinite(x[5][~over]).all(), name
    fin = np.isfinite(c)
    assert np.array_equal(oc.bits(f24)[fin], oc.bits(oc.f24(c))[fin]) and ((oc.bits(f24) & 0xff) == 0).all()
    assert np.array_equal(oc.bits(f24)[np.isnan(c)] & 0x7fc00000, np.full(np.isnan(c).sum(), 0x7fc00000, dtype=np.uint32))
    with capsys.disabled():
        print("\n[operand probes] non-finite, forms: NaN rows NaN in fp32 / f24 / split rows; Inf rows: %d NaN, %d Inf of %d; overflowing "
              "products: %d +-Inf" % (np.isnan(c[inf_rows]).sum(), np.isinf(c[inf_rows]).sum(), c[inf_rows].size, 2 * over.sum()))


@pytest.mark.parametrize("mode", [PRECISE, FAST, MIXED])
def test_gemm_keeps_non_finite_values(mode, probes, capsys):
    """NaN in, NaN out, in every precision: rows holding one Inf / -Inf / NaN and a weight row holding a NaN.  The mixed mode lost them
    before this test existed: with the saturating-conversion mode bit set the matrix pipe returns +0 for a dot product that holds a
    NaN, and gemm_split_ps_kernel set the bit in every mixed instantiation (now only where it writes mixed rows).  The mixed producers'
    planes of the non-finite values are pinned too: NaN -> NaN in h, X and Y; +-Inf -> +-Inf in h, +-448 in Y, NaN in X (Inf - Inf);
    +-3e38 -> +-65504 and +-448 twice, a finite result."""
    dev = _dev()
    m, n, k = 513, 576, 576
    a, _ = oc.activation_matrix(m, k, probes["classes"])
    at = [(r, 7 + 64 * r) for r in range(len(oc.NONFINITE))]
    for (r, kk), v in zip(at, oc.NONFINITE):
        a[r, kk] = v
    a[5, :], a[300, :] = 3.0e38, -3.0e38
    vals = probes["weights"]["max_448"]
    sig = oc.sigma("permutation", n, k)
    w, wv = oc.selector_weight(n, k, vals, sig)
    w[100, sig[100]] = np.nan
    c, ws = _gemm(torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev), None, mode)
    c = c.cpu().numpy()
    assert np.isnan(c[[2, 3, 4]]).all() and np.isnan(c[:, 100]).all()
    assert (~np.isfinite(c[[0, 1]])).all()
    rest = np.ones(c.shape, dtype=bool)
    rest[:5], rest[:, 100] = False, False
    if mode != MIXED:
        rest[[5, 300]] = False                       # (products of +-3e38 overflow fp32 in the split modes; fp16 saturates)
    assert np.isfinite(c[rest]).all()
    if mode == MIXED:
        e = oc.weight_exp(np.abs(vals).max())
        big = oc.product(a[[5, 300]][:, sig], wv[None, :], MIXED, e)
        cols = np.arange(n) != 100
        assert (np.abs(oc.ulp_key(c[[5, 300]]) - oc.ulp_key(big))[:, cols] <= 1).all() and (np.abs(big) <= 65504.0 * 448 * 1.01).all()
        rows = ws.cpu().numpy()[:m * 4 * k].reshape(m, 4 * k)
        h, x, y = _planes_of_mixed_rows(rows, k)
        got = [(int(h[r, kk]), int(x[r, kk]), int(y[r, kk])) for r, kk in at] + [(int(h[5, 0]), int(x[5, 0]), int(y[5, 0]))]
        assert got[0] == (0x7c00, got[0][1], 0x7e) and got[1] == (0xfc00, got[1][1], 0xfe) and got[5] == (0x7bff, 0x7e, 0x7e), got
        assert all((g[1] & 0x7f) == 0x7f for g in got[:5]) and all((g[0] & 0x7c00) == 0x7c00 and g[0] & 0x3ff and (g[2] & 0x7f) == 0x7f for g in got[2:5]), got
        want_h, want_x, want_y = oc.mixed_act_planes(a[[r for r, _ in at], [kk for _, kk in at]])     # the restatement says the same
        assert [int(v) for v in oc.fp16_bits(want_h)[:2]] == [0x7c00, 0xfc00] and np.isnan(want_h[2:]).all()
        assert ((want_x & 0x7f) == 0x7f).all() and want_y[:2].tolist() == [0x7e, 0xfe] and ((want_y[2:] & 0x7f) == 0x7f).all()
    with capsys.disabled():
        print("\n[operand probes] non-finite, %s GEMM: NaN rows and the NaN weight's column NaN; Inf rows: %d NaN, %d Inf of %d; rows of "
              "+-3e38: %d of %d finite" % (oc.MODE_NAMES[mode], np.isnan(c[[0, 1]]).sum(), np.isinf(c[[0, 1]]).sum(), c[[0, 1]].size,
                                           np.isfinite(c[[5, 300]]).sum(), c[[5, 300]].size))


@pytest.mark.parametrize("m,n,k,ks", [(1000, 100, 192, 1), (9999, 1152, 384, 7)])
def test_wgrad_selectors(m, n, k, ks, probes, capsys):
    """dw = dy^T x with dy zero except for one 2^-j per chosen row (first, last, both sides of the multiples of 32 and 256 next to the
    ends and of every split-K boundary), each in a column of its own: dw[n, :] is the 16-bit form of that x row times 2^-j, exactly,
    and exactly zero elsewhere -- transpose_split_kernel's M and N tails (n = 100), the Mp padding and k_valid (n % 32 == 0)."""
    native, lib = _lib()
    dev = _dev()
    rows = oc.wgrad_rows(m, ks)
    assert len(rows) <= n
    rng = np.random.default_rng(m + n)
    x = oc.f32(rng.standard_normal((m, k)))
    fin = np.concatenate([probes["classes"][c] for c in ("bf16_hi_tie_down", "bf16_hi_tie_up", "bf16_lo_tie", "max_residual", "outlier")])
    for i, r in enumerate(rows):                    # the chosen rows carry the split planes' tie probes
        x[r, :] = fin[(np.arange(k) * 7 + i * 13) % len(fin)]
    cols = [0, n - 1, 63, 64, n // 2] + [c for c in ((np.arange(n) * 29 + 5) % n).tolist()]
    cols = list(dict.fromkeys(c for c in cols if 0 <= c < n))[:len(rows)]
    dy = np.zeros((m, n), dtype=np.float32)
    want = np.zeros((n, k), dtype=np.float32)
    for i, (r, cn) in enumerate(zip(rows, cols)):
        s = np.float32(2.0 ** -(i % 9)) * (-1 if i % 2 else 1)
        dy[r, cn] = s
        hi, lo = oc.split(x[r])
        want[cn] = (hi + lo) * s                     # exact: hi + lo lies inside x's 24 bits, the scale is a power of two
    assert (np.abs(want[want != 0]) > 2.0 ** -100).all()
    dy_t, x_t = torch.from_numpy(dy).to(dev), torch.from_numpy(x).to(dev)
    ws = torch.full((lib.veto_debug_wgrad_workspace_bytes(m, n, k, ks),), 0xA5, dtype=torch.uint8, device=dev)

    def call(dw):
        native.check(lib.veto_debug_wgrad(None, dy_t.data_ptr(), x_t.data_ptr(), dw.data_ptr(), m, n, k, ks, ws.data_ptr(), ws.numel()))
    dw = _twice(call, n, k).cpu().numpy()
    chosen = np.zeros(n, dtype=bool)
    chosen[cols] = True
    assert (dw[~chosen] == 0).all(), "%d non-zero values in rows without an entry" % (dw[~chosen] != 0).sum()
    nz = want != 0
    diff = (oc.bits(dw) != oc.bits(want)) & nz
    assert not diff.any(), "%d values differ, first at %s" % (diff.sum(), np.argwhere(diff)[0])
    assert (dw[~nz] == 0).all()
    with capsys.disabled():
        print("\n[operand probes] wgrad m %d n %d k %d ks %d: %d chosen rows (%s ...), %d values bit-equal, %d exact zeros" %
              (m, n, k, ks, len(rows), rows[:8], nz.sum(), (~nz).sum()))


@pytest.mark.parametrize("mode", [PRECISE, FAST, MIXED])
def test_element_level_precision(mode, probes, capsys):
    """The "2^-16 class" where no sum hides it: on the N(0, 1) block and the x 30 outlier block, per element, |C - a w| against
    float64 stays inside the per-product bound derived in operand_cases.product_bound (never taken from a device run)."""
    dev = _dev()
    m, n, k = 513, 576, 576
    a = np.where(np.arange(m)[:, None] % 2 == 0, probes["classes"]["normal"][(np.arange(m)[:, None] * 7 + np.arange(k)[None, :]) % 256],
                 probes["classes"]["outlier"][(np.arange(m)[:, None] * 5 + np.arange(k)[None, :] * 3) % 256]).astype(np.float32)
    vals = probes["weights"]["ordinary"]
    sig = oc.sigma("permutation", n, k)
    w, wv = oc.selector_weight(n, k, vals, sig)
    c, _ = _gemm(torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev), None, mode)
    c = c.cpu().numpy().astype(np.float64)
    e = oc.weight_exp(np.abs(vals).max())
    ref = a[:, sig].astype(np.float64) * wv[None, :].astype(np.float64)
    bound = oc.product_bound(a[:, sig], wv[None, :], mode, e)
    frac = np.abs(c - ref) / bound
    assert frac.max() <= 1.0, frac.max()
    rel = np.abs(c - ref)[np.abs(ref) > 1e-3] / np.abs(ref)[np.abs(ref) > 1e-3]
    with capsys.disabled():
        print("\n[operand probes] element precision %s: worst %.3f of the derived bound; relative error max %.3g (2^%.1f), mean %.3g"
              % (oc.MODE_NAMES[mode], frac.max(), rel.max(), np.log2(rel.max()), rel.mean()))
