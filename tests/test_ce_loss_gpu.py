"""The relation loss on the MI355X: veto_ce_loss through the C ABI on every case of tests/ce_loss_cases.py, held element by element to
the bounds derived there from the kernels' own arithmetic (no bare tolerance), with sentinel-filled outputs and guard cells; its
refusals; and veto_amd.losses against torch float64 autograd on the CPU of the same expression.  Every measured figure is printed as
measured / bound before it is asserted (pytest -s); profiles/ce_loss_parity.txt keeps a run."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_loss_cases as cc  # noqa: E402

from veto_amd import native  # noqa: E402
from veto_amd.losses import ce_loss, relation_ce_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # cells behind every stated size
SENTINEL = -(2.0 ** 62)          # a finite float32 no case produces
WS_FILL = 0xA5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(numel):
    return torch.full((numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class AbiCall:
    """One veto_ce_loss call on a case: the [m, ld] logits buffer with the NaN pattern wherever the call must not read, sentinel-filled
    loss, gradient and workspace, each with GUARD cells behind its stated size."""

    def __init__(self, c, want_grad=True, ws_offset=0):
        self.c = c
        self.n, self.C = len(c["labels"]), c["logits"].shape[1]
        self.lib = native.load_library()
        self.logits = _dev(cc.logits_buffer(c))
        self.labels, self.weight, self.rows = _dev(c["labels"]), _dev(c["weight"]), _dev(c["rows"])
        self.before = [t.clone() for t in (self.logits, self.labels, self.weight, self.rows) if t is not None]
        self.loss = _guarded(1)
        self.grad = _guarded(self.n * self.C) if want_grad else None
        self.need = self.lib.veto_ce_loss_workspace_bytes(self.n)
        self.ws_offset = ws_offset
        self.ws = torch.full((ws_offset + self.need + 4 * GUARD,), WS_FILL, dtype=torch.uint8, device=DEV)

    def run(self, **over):
        kw = dict(logits=_ptr(self.logits), ld=self.c["ld"], labels=_ptr(self.labels), weight=_ptr(self.weight), rows=_ptr(self.rows),
                  n=self.n, n_cls=self.C, loss=_ptr(self.loss), grad=_ptr(self.grad),
                  workspace=ctypes.c_void_p(self.ws.data_ptr() + self.ws_offset), workspace_bytes=self.need)
        kw.update(over)
        rc = self.lib.veto_ce_loss(None, kw["logits"], kw["ld"], kw["labels"], kw["weight"], kw["rows"], kw["n"], kw["n_cls"], kw["loss"],
                                   kw["grad"], kw["workspace"], kw["workspace_bytes"])
        torch.cuda.synchronize()
        return rc, self.lib.veto_last_error()

    def outputs(self):
        """(loss [1], grad [n, C] or None) as numpy, after the guards and everything the call may only read were found untouched."""
        for now, was in zip([t for t in (self.logits, self.labels, self.weight, self.rows) if t is not None], self.before):
            assert now.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()
        assert (self.loss[1:] == SENTINEL).all()
        assert (self.ws[:self.ws_offset] == WS_FILL).all() and (self.ws[self.ws_offset + self.need:] == WS_FILL).all()
        if self.grad is None:
            return self.loss[:1].cpu().numpy(), None
        assert (self.grad[self.n * self.C:] == SENTINEL).all()
        g = self.grad[:self.n * self.C].cpu().numpy().reshape(self.n, self.C)
        assert not (g == np.float32(SENTINEL)).any()                              # every element was written
        return self.loss[:1].cpu().numpy(), g

    def untouched(self):
        return bool((self.loss == SENTINEL).all() and (self.grad is None or (self.grad == SENTINEL).all()) and (self.ws == WS_FILL).all())


# ---- every case through the C ABI ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.names())
def test_loss_and_gradient_stay_inside_the_derived_bounds(name):
    c, r, b = cc.ref_and_bounds(name)
    first, second = AbiCall(c), AbiCall(c)
    for call in (first, second):
        rc, msg = call.run()
        assert rc == 0, msg
    loss, grad = first.outputs()
    loss2, grad2 = second.outputs()
    lr, gr = cc.measure(c, loss, grad, r, b)
    print("PARITY %-22s n %6d C %4d ld %4d  loss %-13.9g err / bound %-9.3g gradient err / bound %-9.3g %s"
          % (name, first.n, first.C, c["ld"], loss[0], lr, gr, c["event"]))
    assert loss.tobytes() == loss2.tobytes() and grad.tobytes() == grad2.tobytes()       # two calls, the same bits
    assert lr <= 1 and gr <= 1, (name, lr, gr)
    # exact zeros on ignored rows, NaN and inf where torch has them (measure() reports either as an infinite ratio; spelled out once more)
    assert not grad[r["ignored"]].view(np.uint32).any()
    assert np.array_equal(np.isnan(grad), np.isnan(r["grad"])) and not np.isinf(grad).any()
    assert (math.isnan(loss[0]) == math.isnan(r["loss"])) and (math.isinf(loss[0]) == math.isinf(r["loss"]))
    # grad == NULL: the same loss bits, nothing else written
    only = AbiCall(c, want_grad=False)
    rc, msg = only.run()
    assert rc == 0, msg
    assert only.outputs()[0].tobytes() == loss.tobytes()


def test_exactly_shifted_rows_give_the_same_gradient_bits_at_every_offset():
    """Rows 0..15 of the offset cases hold the same logits shifted exactly (every value representable): z - mx is the same float in
    each, so the gradient rows are the same bits.  The remaining rows were rounded by the shift and are held to their bounds above."""
    got = {}
    for off in cc.OFFSETS:
        call = AbiCall(cc.cases()["offset_%g" % off])
        rc, msg = call.run()
        assert rc == 0, msg
        got[off] = call.outputs()[1][:cc.OFFSET_GRID_ROWS]
    differing = [off for off in cc.OFFSETS[1:] if got[off].tobytes() != got[0.0].tobytes()]
    print("offsets whose exactly shifted rows differ from offset 0 in some bit: %s" % (differing or "none"))
    assert not differing


def test_a_workspace_at_an_odd_float_offset_gives_the_same_bits():
    """check_workspace does not ask veto_ce_loss's workspace for 256-byte alignment (it holds floats only), so nothing is refused:
    a workspace 4 bytes past an aligned address gives the bits of an aligned one."""
    c = cc.cases()["rows_257"]
    a, b = AbiCall(c), AbiCall(c, ws_offset=4)
    assert a.run()[0] == 0 and b.run()[0] == 0
    (la, ga), (lb, gb) = a.outputs(), b.outputs()
    assert la.tobytes() == lb.tobytes() and ga.tobytes() == gb.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_name_their_reason():
    c = cc.cases()["rows_perm_ld_plus3"]
    for over, needle in ((dict(n=0), b"bad sizes (n 0,"), (dict(n=-3), b"bad sizes (n -3,"), (dict(n_cls=1), b"n_cls 1,"), (dict(n_cls=0), b"n_cls 0,"),
                         (dict(ld=20), b"ld 20)"), (dict(logits=None), b"null argument"), (dict(labels=None), b"null argument"),
                         (dict(loss=None), b"null argument"), (dict(workspace=None), b"null argument"),
                         (dict(workspace_bytes=None), b"workspace too small: need")):
        call = AbiCall(c)
        if "workspace_bytes" in over:
            over = dict(workspace_bytes=call.need - 1)                           # one byte short
        rc, msg = call.run(**over)
        assert rc < 0 and needle in msg, (over, rc, msg)
        assert call.untouched(), over
    call = AbiCall(c)                                                            # the same buffers are fine when nothing is wrong
    assert call.run()[0] == 0 and not call.untouched()


# ---- through veto_amd.losses, against torch float64 autograd on the CPU ------------------------------------------------------------------

def _f64_grad(rel, terms):
    """d (sum_k coeff_k CE(rel[:, a_k:b_k][rows_k], labels_k, weight_k)) / d rel in float64 on the CPU."""
    x = torch.from_numpy(rel.astype(np.float64)).requires_grad_()
    total = 0
    losses = []
    for t in terms:
        z = x[:, t["a"]:t["b"]]
        z = z if t.get("rows") is None else z[torch.from_numpy(t["rows"])]
        w = None if t.get("weight") is None else torch.from_numpy(t["weight"].astype(np.float64))
        l = torch.nn.functional.cross_entropy(z, torch.from_numpy(t["labels"]), weight=w)
        losses.append(float(l.detach()))
        total = total + t["coeff"] * l
    total.backward()
    return losses, x.grad.numpy()


def _allowed(rel, terms):
    """The bound of rel.grad: per term the case bound of each selected row times |coeff|, summed where rows repeat or terms overlap;
    the float32 accumulation of k contributions into one element adds gamma(k) of their absolute sum, the product with the upstream
    gradient one rounding (none for a power of two, counted all the same)."""
    allow = np.zeros(rel.shape)
    mag = np.zeros(rel.shape)
    hits = np.zeros(rel.shape[0])
    loss_bounds = []
    for t in terms:
        c = cc.make_case("py", "python path", rel[:, t["a"]:t["b"]], t["labels"], weight=t.get("weight"), rows=t.get("rows"))
        r = cc.ce_fp64(c)
        lb, gb = cc.bounds(c, r)
        loss_bounds.append(lb)
        rows = np.arange(rel.shape[0]) if t.get("rows") is None else t["rows"]
        k = abs(t["coeff"])
        np.add.at(allow[:, t["a"]:t["b"]], rows, k * (gb + cc.U * np.abs(r["grad"])))
        np.add.at(mag[:, t["a"]:t["b"]], rows, k * np.abs(r["grad"]))
        np.add.at(hits, rows, 1)
    return loss_bounds, allow + cc.gamma(hits.max() + len(terms)) * mag, mag


def _python_path(rel, terms, what):
    x = torch.from_numpy(rel).to(DEV).requires_grad_()
    total, got_losses = 0, []
    for t in terms:
        z = x[:, t["a"]:t["b"]]
        assert not z.is_contiguous()
        l = ce_loss(z, _dev(t["labels"]), weight=_dev(t.get("weight")), rows=_dev(t.get("rows")))
        assert l.dim() == 0 and l.dtype == torch.float32 and l.requires_grad
        got_losses.append(float(l.detach()))
        total = total + t["coeff"] * l
    total.backward()
    got = x.grad.cpu().numpy()
    want_losses, want = _f64_grad(rel, terms)
    loss_bounds, allow, mag = _allowed(rel, terms)
    touched = mag > 0
    ratio = float((np.abs(got - want)[touched] / allow[touched]).max())
    lratio = max(abs(g - w) / b for g, w, b in zip(got_losses, want_losses, loss_bounds))
    print("PARITY python %-34s loss err / bound %-9.3g rel.grad err / bound %-9.3g over %d elements, %d exactly 0" % (what, lratio, ratio, touched.sum(), (~touched).sum()))
    assert lratio <= 1 and ratio <= 1
    assert not got[~touched].any() and not want[~touched].any() and (~touched).any()         # zeros everywhere else
    return got


def _rel(seed, P=60, width=51):
    rng = np.random.RandomState(seed)
    return rng, (rng.standard_normal((P, width)) * 2.0).astype(np.float32)


def test_a_column_slice_with_rows_puts_its_gradient_into_the_right_rows_and_columns():
    """ce_loss(rel[:, a:b], labels, rows=rows) as VETOPredictor_MEET calls it: a MEET group's 21 columns of a [60, 51] tensor, 17 rows."""
    rng, rel = _rel(9901)
    rows = rng.permutation(60)[:17]
    _python_path(rel, [dict(a=7, b=28, rows=rows, labels=rng.randint(0, 21, 17), coeff=1.0)], "rel[:, 7:28], 17 distinct rows")


def test_repeated_rows_accumulate():
    rng, rel = _rel(9902)
    rows = np.array([3, 3, 3, 41, 8, 41, 3, 59, 0, 8])
    got = _python_path(rel, [dict(a=30, b=51, rows=rows, labels=rng.randint(0, 21, 10), coeff=1.0)], "rel[:, 30:51], rows repeat up to 4 times")
    assert sorted(np.nonzero(got.any(1))[0]) == [0, 3, 8, 41, 59]


def test_upstream_gradients_other_than_one():
    rng, rel = _rel(9903)
    rows = rng.permutation(60)[:25]
    w = cc.span_weights(30, 9904)
    _python_path(rel, [dict(a=0, b=21, rows=rows, labels=rng.randint(0, 21, 25), coeff=0.5)], "0.5 * loss")
    _python_path(rel, [dict(a=0, b=21, rows=rows, labels=rng.randint(0, 21, 25), coeff=1.0),
                       dict(a=21, b=51, rows=None, labels=rng.randint(0, 30, 60), weight=w, coeff=1.0)], "two losses on two slices")
    _python_path(rel, [dict(a=0, b=30, rows=rows, labels=rng.randint(0, 30, 25), coeff=0.5),
                       dict(a=20, b=50, rows=rows[::-1].copy(), labels=rng.randint(0, 30, 25), weight=w, coeff=3.0)], "0.5 l1 + 3 l2, overlapping")


def test_int32_and_cpu_labels_and_no_gradient():
    c, r, b = cc.ref_and_bounds("weight_beta")
    z, w = _dev(c["logits"]), _dev(c["weight"])
    loss, grad = relation_ce_loss(z, _dev(c["labels"]), weight=w, want_grad=True)
    lr, gr = cc.measure(c, loss.cpu().numpy(), grad.cpu().numpy(), r, b)
    print("PARITY python relation_ce_loss(weight_beta)         loss err / bound %-9.3g gradient err / bound %-9.3g" % (lr, gr))
    assert lr <= 1 and gr <= 1
    for labels in (_dev(c["labels"].astype(np.int32)), torch.from_numpy(c["labels"]), torch.from_numpy(c["labels"].astype(np.int32))):
        l2, g2 = relation_ce_loss(z, labels, weight=w, want_grad=True)
        assert torch.equal(l2, loss) and torch.equal(g2, grad)
    l3, g3 = relation_ce_loss(z, _dev(c["labels"]), weight=w, want_grad=False)
    assert g3 is None and torch.equal(l3, loss)
    l4, g4 = relation_ce_loss(z, _dev(c["labels"]), weight=w)
    assert g4 is None and torch.equal(l4, loss)


def test_no_rows_is_nan_with_an_empty_gradient_and_no_launch(monkeypatch):
    calls = []
    real = native.Launch.run

    def run(self, name, *tail, **kw):
        calls.append(name)
        return real(self, name, *tail, **kw)
    monkeypatch.setattr(native.Launch, "run", run)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    for logits, rows in ((torch.zeros((0, 7), device=DEV), None), (torch.randn(5, 7, device=DEV), none)):
        loss, grad = relation_ce_loss(logits, none, rows=rows, want_grad=True)
        assert loss.shape == (1,) and torch.isnan(loss).all() and grad.shape == (0, 7) and grad.dtype == torch.float32
        loss, grad = relation_ce_loss(logits, none, rows=rows)
        assert torch.isnan(loss).all() and grad is None
    assert calls == []
    x = torch.randn(5, 7, device=DEV, requires_grad=True)
    l = ce_loss(x, none, rows=none)
    assert math.isnan(float(l.detach()))
    l.backward()
    assert x.grad.shape == (5, 7) and not x.grad.any()                          # an empty selection touches no row
    with pytest.raises(ValueError, match="same length"):
        relation_ce_loss(torch.randn(5, 7, device=DEV), none, rows=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="one entry per logit row"):
        relation_ce_loss(torch.randn(5, 7, device=DEV), none)
    assert calls == []
