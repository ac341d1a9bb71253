"""The training path at the sizes and in the forms a training step runs it (tests/test_backward_blocks.py and the train_*.npz goldens
stop at 134 pairs): the backward blocks against float64 autograd through the debug entry points that select the shipped forms, and the
gradient of the whole step, EVERY element of every parameter and of both ROI inputs, against oracle/train_oracle.py::train_step
(float64 autograd over the restated forward, itself pinned to the goldens by tests/test_train_oracle.py).

Every test prints its worst figures on lines starting with PARITY; profiles/train_scale_parity.txt is those lines of one run."""
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, VG_MEET_GROUPS
from oracle.dropout import keep_mask      # the one host restatement of the device's masks

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-3      # the project's own bound: test_training_backward_matches_reference_gradients
DIM, TOK = 576, 19
F_CLS, F_F24, F_SPLIT = 1, 2, 4


def _lib():
    from veto_amd import native
    return native, native.load_library()


def _report(line):
    print("PARITY " + line, flush=True)


# ---- the two storage formats a test has to speak ------------------------------------------------------------------------
def _f24_round(x):
    """uint32 bit patterns of x rounded to nearest even at bit 8 (numpy, wrapping)."""
    b = x.contiguous().numpy().view(np.uint32)
    return b + np.uint32(0x7F) + ((b >> np.uint32(8)) & np.uint32(1))


def pack_f24(x):
    """fp32 -> 3-byte floats (include/veto_amd.h): the top three bytes of the value rounded to nearest even, low address first."""
    r = _f24_round(x)
    return torch.from_numpy(np.ascontiguousarray(r.view(np.uint8).reshape(-1, 4)[:, 1:4]).reshape(x.shape[0], -1))


def unsplit(buf, rows, n):
    """Split rows [rows, 2n] bf16, blocks of 32 columns [hi | lo] -> hi + lo in float64."""
    t = buf.view(torch.bfloat16).reshape(rows, n // 32, 2, 32).cpu()
    return (t[:, :, 0].double() + t[:, :, 1].double()).reshape(rows, n)


# ---- attention backward -----------------------------------------------------------------------------------------------
def _attention_reference(qkv, dout, n_pair, heads, cls_only, chunk=1024):
    """d qkv of sum(out * dout) through softmax attention (model_veto.py:85-96) in float64 autograd, pairs in chunks.  cls_only: only
    the CLS query's output row has a gradient (dout is [n_pair, 576])."""
    dh = DIM // heads
    out = torch.empty(n_pair * TOK, 3 * DIM, dtype=torch.float64)
    for a in range(0, n_pair, chunk):
        b = min(n_pair, a + chunk)
        x = qkv[a * TOK:b * TOK].double().requires_grad_(True)
        q, k, v = [t.reshape(b - a, TOK, heads, dh).transpose(1, 2) for t in x.split(DIM, dim=1)]
        attn = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
        o = (attn @ v).transpose(1, 2)                       # [b, 19, H, dh]
        if cls_only:
            loss = (o[:, 0].reshape(b - a, DIM) * dout[a:b].double()).sum()
        else:
            loss = (o.reshape((b - a) * TOK, DIM) * dout[a * TOK:b * TOK].double()).sum()
        loss.backward()
        out[a * TOK:b * TOK] = x.grad
    return out


SMALL, LARGE = [1, 2, 37, 1260], [4099, 15120]
ATTN_CASES = [(h, n, c, f, 1.0, 1.0) for h in (8, 6, 4) for n in SMALL for c in (0, 1) for f in ((0, 1) if h != 4 else (0,))]
# the two largest sizes: the shipped form (3-byte q / k / v where the head width has it; both outputs are checked in every case) and the
# plain one, the last layer's CLS-only form and a middle layer's
ATTN_CASES += [(h, n, c, (1 if h != 4 else 0), 1.0, 1.0) for h in (8, 6, 4) for n in LARGE for c in (0, 1)]
ATTN_CASES += [(8, n, 0, 0, 1.0, 1.0) for n in LARGE]
# near-one-hot softmax (q and k scaled so that the logits are 3 x as large) and output gradients of magnitude 1e3
ATTN_CASES += [(8, 1260, 0, 1, 3.0, 1.0), (4, 1260, 1, 0, 3.0, 1.0), (6, 1260, 1, 1, 1.0, 1e3), (4, 4099, 0, 0, 1.0, 1e3)]


@pytest.mark.parametrize("heads,n_pair,cls_only,f24,sharp,dscale", ATTN_CASES)
def test_attention_backward_shipped_forms(heads, n_pair, cls_only, f24, sharp, dscale):
    """fp32 and split-bf16 output of the same launch form against float64 autograd.  Bound: the 2e-5 x max(1, max |ref|) of
    test_attention_backward_against_autograd; the split output adds its format's rounding, hi + lo keeps 16 significand bits:
    2^-16 |value|.  3-byte inputs: the reference starts from the values the kernel sees (the entry point unpacks them with the
    device's own unpack, compared bit for bit with the host packing's rounding)."""
    native, lib = _lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(heads * 100000 + n_pair * 4 + cls_only * 2 + f24)
    rows = n_pair * TOK
    qkv = torch.randn(rows, 3 * DIM, generator=g)
    qkv[:, :2 * DIM] *= sharp ** 0.5
    dout = torch.randn(n_pair if cls_only else rows, DIM, generator=g) * dscale
    dout_d = dout.to(dev)
    flags = (F_CLS if cls_only else 0) | (F_F24 if f24 else 0)
    if f24:
        packed = pack_f24(qkv)
        pad = torch.zeros(rows * 3 * DIM * 3 + 256, dtype=torch.uint8, device=dev)
        pad[:packed.numel()] = packed.reshape(-1).to(dev)
        seen = torch.full((rows, 3 * DIM), float("nan"), device=dev)
        qkv_in, seen_ptr = pad, seen.data_ptr()
    else:
        qkv_in, seen_ptr = qkv.to(dev), None
    got = {}
    for split in (0, 1):
        out = torch.full((rows, 2 * 3 * DIM), float("nan"), dtype=torch.bfloat16, device=dev) if split else \
            torch.full((rows, 3 * DIM), float("nan"), device=dev)
        native.check(lib.veto_debug_attention_backward_forms(None, qkv_in.data_ptr(), dout_d.data_ptr(), out.data_ptr(), seen_ptr, n_pair, heads,
                                                             flags | (F_SPLIT if split else 0)))
        torch.cuda.synchronize()
        got[split] = unsplit(out, rows, 3 * DIM) if split else out.cpu().double()
        del out
    if f24:
        qkv_seen = seen.cpu()
        # round to nearest even at bit 8: the device's unpack of the host's bytes IS the host's rounding with the low byte cleared
        assert np.array_equal(qkv_seen.numpy().view(np.uint32), _f24_round(qkv) & np.uint32(0xFFFFFF00))
        assert float((qkv_seen - qkv).abs().max()) <= 2.0 ** -16 * float(qkv.abs().max())
        qkv = qkv_seen
    ref = _attention_reference(qkv, dout, n_pair, heads, cls_only)
    scale = max(1.0, float(ref.abs().max()))
    errs = {}
    for split in (0, 1):
        assert torch.isfinite(got[split]).all()
        errs[split] = float((got[split] - ref).abs().max()) / scale
        if cls_only:      # d q of the query rows that have no output gradient: written, and exactly zero
            dq = got[split].reshape(n_pair, TOK, 3 * DIM)[:, 1:, :DIM]
            assert float(dq.abs().max()) == 0.0 if n_pair * (TOK - 1) else True
            assert float(ref.reshape(n_pair, TOK, 3 * DIM)[:, 1:, :DIM].abs().max()) == 0.0
    _report("attention_backward heads %d n_pair %d cls_only %d f24_in %d sharp %g dout %g: max err / max(1, max|ref|) fp32 out %.2e split out %.2e"
            % (heads, n_pair, cls_only, f24, sharp, dscale, errs[0], errs[1]))
    assert errs[0] < 2e-5, errs
    assert errs[1] < 2e-5 + 2.0 ** -16, errs


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------
LN_ROWS = [1, 63, 64, 65, 1000, 40000, 287280]
LN_CASES = [(r, w, "plain") for r in LN_ROWS for w in (False, True)] + [(1000, True, "constant"), (1000, False, "offset"), (40000, True, "offset")]


def _ln_inputs(rows, with_res, kind):
    g = torch.Generator().manual_seed(rows * 7 + with_res + len(kind))
    x = torch.randn(rows, DIM, generator=g) * 2 + 0.3
    if kind == "constant":      # variance 0: the eps path (every other row, so that plain rows share the block).  Multiples of 1/4: every
        x[::2] = torch.round(torch.randn(rows, 1, generator=g)[::2] * 12) / 4      # fp32 partial sum of the row is exact, the row mean too
    if kind == "offset":
        x = x + 1e3
    dy = torch.randn(rows, DIM, generator=g)
    gamma = torch.randn(DIM, generator=g)
    dres = torch.randn(rows, DIM, generator=g) if with_res else None
    return x, dy, gamma, dres


def _ln_reference(x, dy, gamma, dres):
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = torch.zeros(DIM, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.layer_norm(xd, (DIM,), gd, bd, 1e-5) * dy.double()).sum().backward()
    return xd.grad + (dres.double() if dres is not None else 0), gd.grad, bd.grad


def _ln_bounds(kind, ref_dx, ref_dg, ref_db):
    """The bounds of test_layernorm_backward_against_autograd (2e-5 on dx, 1e-4 x max(1, max |ref|) on dgamma / dbeta), dx relative to
    max(1, max |ref dx|) because constant rows have rstd = 316.  Rows offset by A = 1e3 are ill-conditioned for ANY fp32 evaluation: the
    row mean of 576 values of magnitude A carries up to ~8 ulp(A) = 8 x 2^-24 A of rounding (a depth-10 summation tree), which moves
    xhat by that over the row's sigma (2), and dx and the dgamma terms with it: 8 x 2^-24 x 1e3 / 2 = 2.4e-4 is added there."""
    extra = 8 * 2.0 ** -24 * 1e3 / 2 if kind == "offset" else 0.0
    sdx = max(1.0, float(ref_dx.abs().max()))
    return (2e-5 + extra) * sdx, (1e-4 + extra) * max(1.0, float(ref_dg.abs().max())), 1e-4 * max(1.0, float(ref_db.abs().max()))


@pytest.mark.parametrize("rows,with_res,kind", LN_CASES)
def test_layernorm_backward_both_forms(rows, with_res, kind):
    """The plain form and the SPLIT form (split rows of dx, per-32-row column partials; dropout threshold 0 here) on the same inputs."""
    native, lib = _lib()
    dev = torch.device("cuda:0")
    x, dy, gamma, dres = _ln_inputs(rows, with_res, kind)
    ref_dx, ref_dg, ref_db = _ln_reference(x, dy, gamma, dres)
    tol_dx, tol_dg, tol_db = _ln_bounds(kind, ref_dx, ref_dg, ref_db)
    x_d, dy_d, gamma_d = x.to(dev), dy.to(dev), gamma.to(dev)
    dres_d = dres.to(dev) if with_res else None
    ws = torch.empty(lib.veto_debug_layernorm_backward_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    n_part = lib.veto_debug_layernorm_backward_col_partial_rows(rows)
    assert n_part == (rows + 63) // 64 * 2
    worst = {}
    for form in ("plain", "split"):
        dx = torch.full((rows, DIM), float("nan"), device=dev)
        dgb = torch.full((2, DIM), float("nan"), device=dev)
        if form == "plain":
            native.check(lib.veto_debug_layernorm_backward(None, x_d.data_ptr(), dy_d.data_ptr(), gamma_d.data_ptr(), dres_d.data_ptr() if with_res else None,
                                                           dx.data_ptr(), dgb.data_ptr(), rows, ws.data_ptr(), ws.numel()))
        else:
            srows = torch.full((rows, 2 * DIM), float("nan"), dtype=torch.bfloat16, device=dev)
            colp = torch.full((n_part, DIM), float("nan"), device=dev)
            native.check(lib.veto_debug_layernorm_backward_split(None, x_d.data_ptr(), dy_d.data_ptr(), gamma_d.data_ptr(), dres_d.data_ptr() if with_res else None,
                                                                 dx.data_ptr(), dgb.data_ptr(), srows.data_ptr(), colp.data_ptr(), rows, 0, 0, 1.0,
                                                                 ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        e_dx = float((dx.cpu().double() - ref_dx).abs().max())
        e_dg = float((dgb[0].cpu().double() - ref_dg).abs().max())
        e_db = float((dgb[1].cpu().double() - ref_db).abs().max())
        worst[form] = (e_dx / tol_dx, e_dg / tol_dg, e_db / tol_db)
        assert e_dx < tol_dx and e_dg < tol_dg and e_db < tol_db, (form, e_dx, tol_dx, e_dg, tol_dg, e_db, tol_db)
        if form == "split":
            _check_split_outputs(srows, colp, rows, ref_dx, tol_dx)
    _report("layernorm_backward rows %d dres %d %s: error / bound (dx, dgamma, dbeta) plain %s split %s"
            % (rows, with_res, kind, " ".join("%.1e" % v for v in worst["plain"]), " ".join("%.1e" % v for v in worst["split"])))


def _check_split_outputs(srows, colp, rows, ref_masked, tol_dx):
    """Split rows = ref (+ 2^-16 |value| of the format); column partials = sums over each 32 rows (at most 32 x the per-element bound,
    + 2^-24 rounding of an fp32 sum of 32 terms of the column's magnitude)."""
    got = unsplit(srows, rows, DIM)
    assert torch.isfinite(got).all()
    assert bool(((got - ref_masked).abs() <= tol_dx + 2.0 ** -16 * ref_masked.abs()).all())
    n_part = colp.shape[0]
    padded = torch.zeros(n_part * 32, DIM, dtype=torch.float64)
    padded[:rows] = ref_masked
    absum = padded.abs().reshape(n_part, 32, DIM).sum(1)
    want = padded.reshape(n_part, 32, DIM).sum(1)
    cp = colp.cpu().double()
    assert torch.isfinite(cp).all()
    assert bool(((cp - want).abs() <= 32 * tol_dx + 32 * 2.0 ** -24 * absum).all())


@pytest.mark.parametrize("rows,p", [(65, 0.1), (40000, 0.35)])
def test_layernorm_backward_split_form_applies_the_dropout_mask(rows, p):
    """SPLIT form with a dropout site: dx itself stays unmasked, the split rows and the column partials carry the mask of
    (seed, threshold) scaled by 1 / (1 - p) -- the same mask regenerated on the host."""
    native, lib = _lib()
    dev = torch.device("cuda:0")
    x, dy, gamma, dres = _ln_inputs(rows, True, "plain")
    ref_dx, ref_dg, ref_db = _ln_reference(x, dy, gamma, dres)
    tol_dx, tol_dg, tol_db = _ln_bounds("plain", ref_dx, ref_dg, ref_db)
    seed, thresh, scale = 0x1234567890ABCDEF, int(p * 2 ** 24), float(np.float32(1.0 / (1.0 - p)))
    keep = keep_mask(seed, rows, DIM, thresh)
    assert abs(float(keep.double().mean()) - (1 - p)) < 4 * (p * (1 - p) / keep.numel()) ** 0.5 + 2.0 ** -24
    x_d, dy_d, gamma_d, dres_d = x.to(dev), dy.to(dev), gamma.to(dev), dres.to(dev)
    ws = torch.empty(lib.veto_debug_layernorm_backward_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    n_part = lib.veto_debug_layernorm_backward_col_partial_rows(rows)
    dx = torch.full((rows, DIM), float("nan"), device=dev)
    dgb = torch.full((2, DIM), float("nan"), device=dev)
    srows = torch.full((rows, 2 * DIM), float("nan"), dtype=torch.bfloat16, device=dev)
    colp = torch.full((n_part, DIM), float("nan"), device=dev)
    native.check(lib.veto_debug_layernorm_backward_split(None, x_d.data_ptr(), dy_d.data_ptr(), gamma_d.data_ptr(), dres_d.data_ptr(), dx.data_ptr(),
                                                         dgb.data_ptr(), srows.data_ptr(), colp.data_ptr(), rows, seed, thresh, scale, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    assert float((dx.cpu().double() - ref_dx).abs().max()) < tol_dx
    got = unsplit(srows, rows, DIM)
    assert bool((got[~keep] == 0).all()) and float((got != 0).double().mean()) > 0.5      # dropped elements are exact zeros, at the host's positions
    _check_split_outputs(srows, colp, rows, ref_dx * keep.double() * scale, tol_dx * scale)
    _report("layernorm_backward split form with dropout rows %d p %.2f: mask identical to the host's, kept fraction %.4f" % (rows, p, float(keep.double().mean())))


# ---- column sums, gelu' ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4492, 287280])
def test_column_sums_sizes(rows):
    """ld > n_cols, n_cols not a multiple of 256.  (1) Small integers: every fp32 partial sum is exact, so the result must be EXACT -- a
    row dropped or taken twice at a chunk border cannot hide.  (2) Gaussian entries against float64 with the rigorous bound of the
    kernel's own scheme (fp32 in-order sums of ceil(rows / 256) rows, folded in double): (chunk + 1) x 2^-24 x sum |x| per column."""
    native, lib = _lib()
    dev = torch.device("cuda:0")
    n_cols, ld = 600, 640
    g = torch.Generator().manual_seed(rows)
    ws = torch.empty(256 * n_cols * 4, dtype=torch.uint8, device=dev)
    ints = torch.randint(-8, 9, (rows, ld), generator=g).float()
    gauss = torch.randn(rows, ld, generator=g)
    chunk = (rows + 255) // 256
    worst = 0.0
    for name, m in (("ints", ints), ("gauss", gauss)):
        m_d = m.to(dev)
        out = torch.full((n_cols + 8,), float("nan"), device=dev)
        native.check(lib.veto_debug_column_sums(None, m_d.data_ptr(), ld, rows, n_cols, out.data_ptr(), ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[n_cols:]).all())            # nothing written past the n_cols columns
        got, ref = out[:n_cols].cpu().double(), m[:, :n_cols].double().sum(0)
        if name == "ints":
            assert torch.equal(got, ref)
        else:
            bound = (chunk + 1) * 2.0 ** -24 * m[:, :n_cols].double().abs().sum(0)
            worst = float(((got - ref).abs() / bound).max())
            assert worst < 1.0
    _report("column_sums rows %d n_cols %d ld %d: integers exact, gaussian error / bound %.3f" % (rows, n_cols, ld, worst))


@pytest.mark.parametrize("n", [4, 1152 * 513, 1152 * 40000])
def test_gelu_backward_sizes_and_tails(n):
    """pre spread over [-40, 40] (both tails, where gelu' is 0 and 1, and a dense cluster around 0).  Bound: the 2e-6 of
    test_gelu_backward_and_column_sums_against_autograd per unit of |dh| (fp32 erff / expf, relative 1e-7-class errors on a factor <= 1.13)."""
    native, lib = _lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n % 9973)
    pre = (torch.rand(n, generator=g) * 80 - 40)
    pre[::3] = torch.randn((n + 2) // 3, generator=g) * 2
    if n == 4:
        pre = torch.tensor([-40.0, -0.3, 0.0, 40.0])
    dh = torch.randn(n, generator=g)
    pd = pre.double().requires_grad_(True)
    (torch.nn.functional.gelu(pd) * dh.double()).sum().backward()
    pre_d, dh_d = pre.to(dev), dh.to(dev)
    dpre = torch.full((n,), float("nan"), device=dev)
    native.check(lib.veto_debug_gelu_backward(None, pre_d.data_ptr(), dh_d.data_ptr(), dpre.data_ptr(), n))
    torch.cuda.synchronize()
    got = dpre.cpu().double()
    err = float((got - pd.grad).abs().max())
    tol = 2e-6 * max(1.0, float(dh.abs().max()))
    _report("gelu_backward n %d: max abs err %.2e (bound %.2e)" % (n, err, tol))
    assert err < tol
    assert bool((got[pre < -39] == 0).all()) and bool((got[pre > 39] == dh.double()[pre > 39]).all())


# ---- whole-step gradients against the float64 oracle -----------------------------------------------------------------------
BIG_REDUCTIONS = ("pos_embedding", "cls_token", ".bias", "norm.weight")     # sums over every token row / every pair


def _errors(got, ref):
    got, ref = got.reshape(-1).double(), ref.reshape(-1).double()
    norm = float(ref.norm())
    scale = max(float(ref.abs().max()), norm / ref.numel() ** 0.5, 1e-12)
    return float((got - ref).abs().max()) / scale, abs(float(got.norm()) - norm) / max(norm, 1e-12)


def _group(name):
    for key, grp in (("to_qkv", "qkv"), ("to_out", "attn_out"), ("fn.net", "ffn"), ("norm.", "layernorm"), ("patch_embed", "patch_embed"),
                     ("rel_out", "heads"), ("pos_embedding", "pos_embedding"), ("cls_token", "cls_token")):
        if key in name:
            return grp
    return "prelude"


def sampled_pairs(num_objs, seed=0):
    """Pair lists and labels from the stand-in relation sampler (tests/relation_sampling.py) at the reference's budget: at most 1024
    per image, at most a quarter of them foreground (a random subset when there are more), the rest a random draw of the other pairs."""
    from relation_sampling import RelationSampling
    from veto_amd import synth
    from veto_amd.structures import BoxList
    samp = RelationSampling(0.5, False, 4, 1024, 0.25, 2048, True, False)
    props, targets = [], []
    for boxes, rel in synth.synthetic_relation_targets(seed=43 + seed, num_objs=tuple(num_objs)):
        b = torch.from_numpy(boxes)
        t = BoxList(b.clone(), (800, 600), mode="xyxy")
        t.add_field("relation", torch.from_numpy(rel))
        props.append(BoxList(b, (800, 600), mode="xyxy"))
        targets.append(t)
    torch.manual_seed(seed)
    _, labels, pairs, _ = samp.gtbox_relsample(props, targets)
    return [p.numpy() for p in pairs], [l.numpy() for l in labels]


REFERENCE_RATES = (0.1, 0.35, 0.35)      # pos_embed's Dropout, pos_drop, the attention out projections: the reference's, the modules' defaults


def _dropout_modules(model):
    tr = model._trunk.fusion_transformer.transformer
    return [model._trunk.pos_embed[3]], [tr.pos_drop], [layer[0].fn.to_out[1] for layer in tr.layers]


def run_step_case(tag, layers, heads, num_objs, pairs, labels, mode="predcls", meet=False, weighted=False, precision="mixed",
                  oracle_dtype=torch.float64, yardstick=None, perturb=None, dropout=False, torch_seed=0, rates=None, batch_seed=13,
                  wrong_masks=None, collect=None):
    """One training step on the device and in the oracle; returns {name: (element error, norm error)} after asserting GRAD_TOL on all.
    yardstick {name: float32-oracle error}: parameters in BIG_REDUCTIONS may use 4 x that where it exceeds GRAD_TOL.
    perturb(oracle result): the deliberately wrong reference of the self-check (see the pull request).
    dropout: False sets every nn.Dropout to p = 0.  True leaves the modules as configured (asserted to be REFERENCE_RATES; `rates`, if
    given, then overrides the three sites on the modules), runs the step under torch.manual_seed(torch_seed), records the seed and the
    rates the step REALLY handed to the library (VETOPredictor._train_opts, wrapped for the call) and gives exactly those to the oracle,
    which applies the library's counter-based masks (oracle/dropout.py).  wrong_masks(Dropout): the self-check's wrong reference.
    collect: a dict that receives "res" (every error) and "seed" before anything is asserted."""
    from oracle import dropout as od
    from oracle import train_oracle as to
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    dev = torch.device("cuda:0")
    cfg = testing.make_config(layers, heads, mode, meet, "VG", precision=precision)
    if weighted:
        cfg.GLOBAL_SETTING.BETA_LOSS = True
        cfg.GLOBAL_SETTING.REL_COUNTS = np.loadtxt(os.path.join(GOLDEN_DIR, "pred_counts.txt")).tolist()
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = False
    sd = synth.meet_state_dict(2, VG_MEET_GROUPS, layers=layers) if meet else synth.predictor_state_dict(2, layers=layers)
    if weighted:
        sd.pop("criterion_loss_rel.weight")
    model = testing.make_predictor(cfg, sd, dev).train()
    used_opts = []
    if dropout:
        sites = _dropout_modules(model)
        assert tuple(float(m.p) for mods in sites for m in mods) == (REFERENCE_RATES[0], REFERENCE_RATES[1]) + (REFERENCE_RATES[2],) * layers
        for mods, p in zip(sites, rates if rates is not None else REFERENCE_RATES):
            for m in mods:
                m.p = p
        inner_opts = model._train_opts

        def recording_opts():
            used_opts.append(inner_opts())
            return used_opts[-1]
        model._train_opts = recording_opts
    else:
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    batch = synth.synthetic_batch(batch_seed, len(num_objs), list(num_objs))
    props = testing.make_proposals(batch, mode, dev)
    roi = {k: torch.from_numpy(batch[k]).to(dev).requires_grad_(True) for k in ("roi_features", "roi_depth_features")}
    random.seed(1)
    pairs_d, labels_d = [torch.from_numpy(p).to(dev) for p in pairs], [torch.from_numpy(l).to(dev) for l in labels]
    if dropout:
        torch.manual_seed(torch_seed)
    out = model(props, pairs_d, labels_d, None, **roi)
    trainable = {k: v for k, v in out[2].items() if v.requires_grad}
    sum(trainable.values()).backward()
    torch.cuda.synchronize()
    drop = None
    if dropout:
        del model._train_opts      # (the instance attribute: the class's method is back)
        assert len(used_opts) == 1, "one step, one draw of the dropout seed"
        o = used_opts[0]
        drop = od.Dropout(o.p_pos, o.p_emb, o.p_attn, seed=o.seed)
        if wrong_masks is not None:
            drop = wrong_masks(drop)
    ocfg = vo.OracleConfig(layers, heads, mode=mode, meet_groups=VG_MEET_GROUPS if meet else None, prefix="model." if meet else "")
    if meet:
        loss = {"chosen": [c.cpu().numpy() for c in out[4][0]], "incre_idx_list": model.incre_idx_list}
    else:
        loss = {"weight": model.criterion_loss_rel.weight.detach().cpu().numpy()} if weighted else None
    t0 = time.time()
    ref = to.train_step(sd, ocfg, batch, pairs, np.concatenate(labels), loss, dtype=oracle_dtype, dropout=drop)
    wall = time.time() - t0
    if perturb is not None:
        perturb(ref)
    params = dict(model.named_parameters(remove_duplicate=False))
    res = {}
    for name, want in ref["grads"].items():
        assert params[name].grad is not None, name
        res[name] = _errors(params[name].grad.detach().cpu(), want)
    for k in roi:
        res["d_" + k] = _errors(roi[k].grad.detach().cpu(), ref["d_" + k])
    if collect is not None:
        collect.update(res=res, seed=used_opts[0].seed if dropout else None)
    for k, v in trainable.items():
        assert abs(float(v.detach()) - ref["losses"][k]) < 2e-4 * max(1.0, abs(ref["losses"][k])), (k, float(v.detach()), ref["losses"][k])
    used = {id(params[n]) for n in ref["grads"]}
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in params.values() if id(p) not in used)
    groups = {}
    for name, (e, ne) in res.items():
        grp = _group(name)
        groups[grp] = (max(groups.get(grp, (0, 0))[0], e), max(groups.get(grp, (0, 0))[1], ne))
    n_pair = sum(len(p) for p in pairs)
    worst = max(res.items(), key=lambda kv: max(kv[1]))
    how = "" if not dropout else " dropout %g/%g/%g" % (drop.p_pos, drop.p_emb, drop.p_attn)
    _report("step %s L%d H%d %s %s %s%s %d pairs (oracle %s, %.1f s): worst element %.2e norm %.2e at %s | per group (element, norm): %s"
            % (tag, layers, heads, mode, "meet" if meet else ("weighted-ce" if weighted else "ce"), precision, how, n_pair,
               str(oracle_dtype).replace("torch.", ""), wall, worst[1][0], worst[1][1], worst[0],
               "  ".join("%s %.1e %.1e" % (k, v[0], v[1]) for k, v in sorted(groups.items()))))
    for name, (e, ne) in res.items():
        tol = GRAD_TOL
        if yardstick is not None and any(k in name for k in BIG_REDUCTIONS):
            tol = max(GRAD_TOL, 4 * yardstick.get(name, 0.0))
        assert e < tol and ne < tol, (name, e, ne, tol)
    return res, ref, (model, roi, batch)


def all_pairs(num_objs):
    from oracle import veto_oracle as vo
    return [vo.enumerate_test_pairs(n) for n in num_objs]


def uniform_labels(pairs, seed=5):
    from veto_amd import synth
    n = sum(len(p) for p in pairs)
    lab = synth.integers(seed, "scale.labels", (n,), 0, 51)
    return list(np.split(lab, np.cumsum([len(p) for p in pairs])[:-1]))


@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_step_gradients_one_image_all_pairs(precision):
    pairs = all_pairs([36])
    run_step_case("n36-all-pairs", 2, 8, [36], pairs, uniform_labels(pairs), precision=precision)


RAGGED = [3, 5, 8, 12, 36, 36, 20, 17, 9, 30, 25, 14]


@pytest.mark.parametrize("layers,heads,mode,meet", [(1, 6, "predcls", False), (2, 8, "sgcls", False), (3, 4, "predcls", True), (2, 8, "sgcls", True)],
                         ids=["l1h6-predcls-weighted-ce", "l2h8-sgcls-weighted-ce", "l3h4-predcls-meet", "l2h8-sgcls-meet"])
def test_step_gradients_ragged_batch_sampled_pairs(layers, heads, mode, meet):
    """12 images of 3 to 36 objects, pair lists from the sampler (1024 / 0.25): images whose foreground was cut to the 256 budget and
    whose background is a random draw, images that keep every candidate pair, foreground first.

    Measured: every group 1e-5 or below except ONE row of class_projection.0.weight in every predcls case of this batch (row 324:
    1.5e-3 to 2.0e-3 with L1 / H6, L1 / H8, L2 / H6, weighted or not; its bias and obj_embed 2e-4 to 4e-4).  Cause: pair 534 has the
    pre-activation of unit 324 of class_projection at -2.4e-8 in float64 (-4.1e-8 in float32 torch; typical |value| 0.23), below the
    float32 rounding of the 400-term dot product, so the ReLU derivative of that one (pair, unit) is decided by rounding and the
    device's per-object formulation lands on the other side.  A property of the input at the kink, not of a kernel: nothing else moves."""
    pairs, labels = sampled_pairs(RAGGED)
    assert max(int((l > 0).sum()) for l in labels) == 256 and min(len(p) for p in pairs) == 6 and sum(len(p) for p in pairs) > 4000
    run_step_case("ragged-sampled", layers, heads, RAGGED, pairs, labels, mode=mode, meet=meet, weighted=not meet)


def test_step_gradients_hand_made_pair_list():
    """Object 2 of the first image is in no pair, object 4 only ever on the object side, the ordered pair (0, 1) is listed twice, the
    second image has one pair: the scatter into the per-object gradient rows sees gaps, one-sided objects and repeats."""
    from train_dropout_cases import HAND_LABELS as labels, HAND_OBJS as num_objs, HAND_PAIRS as pairs      # (shared with the dropout-on step)
    res, ref, (model, roi, batch) = run_step_case("hand-made", 2, 8, num_objs, pairs, labels)
    for k in roi:
        assert float(roi[k].grad[2].abs().max()) == 0.0 and float(ref["d_" + k][2].abs().max()) == 0.0      # the unused object
        assert float(roi[k].grad[6 + 1].abs().max()) == 0.0                                                 # second image: object 1 unused
        assert float(roi[k].grad[4].abs().max()) > 0


def test_step_gradients_full_size_step():
    """The step the benchmark's training line times: 12 x 36 objects, 15 120 pairs, 287 280 token rows, L2 / H8, plain CE.  The
    oracle runs once in float64, chunked, and once in float32 for the yardstick: what plain float32 accumulation over this many rows
    costs in the big reductions, no kernel involved."""
    from oracle import train_oracle as to
    from oracle import veto_oracle as vo
    from veto_amd import synth
    num_objs = [36] * 12
    pairs = all_pairs(num_objs)
    labels = uniform_labels(pairs)
    res, ref, (model, roi, batch) = run_step_case("full-size", 2, 8, num_objs, pairs, labels)
    del model
    torch.cuda.empty_cache()
    t0 = time.time()
    sd = synth.predictor_state_dict(2, layers=2)
    f32 = to.train_step(sd, vo.OracleConfig(2, 8), batch, pairs, np.concatenate(labels), None, dtype=torch.float32)
    yard = {k: _errors(f32["grads"][k], v) for k, v in ref["grads"].items()}
    top = sorted(yard.items(), key=lambda kv: -max(kv[1]))[:6]
    _report("yardstick float32 oracle against float64 oracle, full size (%.1f s): %s" % (time.time() - t0, "  ".join("%s %.1e %.1e" % (k, v[0], v[1]) for k, v in top)))
    _report("full-size HIP error on the same parameters: %s" % "  ".join("%s %.1e %.1e" % (k, res[k][0], res[k][1]) for k, _ in top))


@pytest.mark.parametrize("env", [{"VETO_TRAIN_LN_SPLIT": "1"}, {"VETO_TRAIN_GELU_EPI": "0", "VETO_TRAIN_QKV_F24": "0"}, {"VETO_TRAIN_RECOMPUTE": "1"}],
                         ids=["ln-backward-emits-split-rows", "round5-forms", "recompute-instead-of-keeping"])
def test_step_gradients_behind_the_knobs(env):
    """The 1260-pair case in the forms a knob selects (read once per process: a fresh child pytest process per environment, as
    test_training_variants_behind_the_knobs_match_reference_gradients does)."""
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "one_image_all_pairs and mixed",
                        "-p", "no:cacheprovider"], env=dict(os.environ, **env), timeout=900, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       capture_output=True, text=True)
    for line in p.stdout.splitlines():
        if line.startswith("PARITY "):
            _report("knobs %s | %s" % (" ".join("%s=%s" % kv for kv in env.items()), line[7:]))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
