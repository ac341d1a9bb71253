"""The training step with dropout ON (the configuration training and tools/train_bench.py run) against the float64 oracle under the
DEVICE's masks: the masks are a counter-based hash of (seed, site, element index) (include/veto_amd.h, veto_train_opts_t), restated on
the host by oracle/dropout.py, so the oracle applies the same masks element for element and EVERY element of every parameter gradient
and of both ROI gradients is held to the bound of the dropout-off step (GRAD_TOL, the same comparison: run_step_case of
tests/test_train_scale_gpu.py with its dropout switch).  The cases and the premise about their inputs (no ReLU within float32
rounding of its kink; asserted on the CPU by tests/test_train_dropout_host.py) are in tests/train_dropout_cases.py.

Every test prints its figures on lines starting with PARITY; profiles/train_dropout_parity.txt is those lines of one run."""
import os
import subprocess
import sys

import pytest
import torch

import train_dropout_cases as tc
from test_train_scale_gpu import GRAD_TOL, REFERENCE_RATES, _report, run_step_case

pytestmark = pytest.mark.gpu


def run_case(case, **kw):
    assert REFERENCE_RATES == tc.RATES
    pairs, labels = tc.case_pairs_labels(case)
    got = {}
    try:
        return run_step_case(case.tag, case.layers, case.heads, list(case.num_objs), pairs, labels, mode=case.mode, meet=case.meet,
                             precision=case.precision, dropout=True, torch_seed=case.torch_seed, batch_seed=case.batch_seed,
                             rates=None if case.rates == tc.RATES else case.rates, collect=got, **kw)
    finally:
        # the masks the CPU premise was stated for are the masks the step used: another draw from torch's generator in front of the
        # step's would show here, not as a silent change of inputs
        if "seed" in got:
            assert got["seed"] == tc.step_seed(case.torch_seed), (got["seed"], tc.step_seed(case.torch_seed))


WHOLE = ["hand-made", "ragged-l2h8-mixed", "ragged-l2h8-precise", "ragged-l3h6-mixed", "n36-l2h8-mixed", "ragged-sgcls", "ragged-meet"]


@pytest.mark.parametrize("tag", WHOLE)
def test_dropout_step_gradients(tag):
    """All three sites at the reference's rates.  hand-made: 190 token rows (one full 128-row panel and a partial one), repeats and an
    unused object.  ragged: 214 pairs / 4 066 token rows, neither a multiple of 128 rows nor of 8 pairs (the XCD row remap of the token
    assembly and the GEMM's last panel see a ragged edge); L3 / H6 runs site 3 + l for l = 2 and the other head width.  n36: 1 260
    pairs, 23 940 rows.  sgcls / meet: the soft-label class branch and the stacked heads."""
    case = tc.CASES[tag]
    res, ref, (model, roi, batch) = run_case(case)
    if tag == "hand-made":
        for k in roi:      # the pos_embed mask row of an unused object must not leak into anything
            assert float(roi[k].grad[2].abs().max()) == 0.0 and float(ref["d_" + k][2].abs().max()) == 0.0
            assert float(roi[k].grad[6 + 1].abs().max()) == 0.0
            assert float(roi[k].grad[4].abs().max()) > 0


@pytest.mark.parametrize("tag", ["ragged-only-pos", "ragged-only-emb", "ragged-only-attn"])
def test_dropout_step_gradients_one_site_only(tag):
    """One site at its rate, the other two at p = 0 on the modules: an error at one site that another site's compensates cannot hide,
    and p == 0 must leave a site untouched (threshold 0: no mask, no scale)."""
    run_case(tc.CASES[tag])


SENSITIVITY = {
    "pos_embed mask from another seed": dict(site_seeds={1: 12345}),
    "pos_drop mask from another seed": dict(site_seeds={2: 12345}),
    "to_out masks from another seed": dict(site_seeds={3: 12345, 4: 12345}),
    "pos_drop mask displaced by one token row": dict(row_shift={2: 1}),
    # the last layer runs on compact CLS rows: numbering its site by THOSE rows (pair p -> row p, what the library did before this test
    # existed) instead of by token row 19 p is a mask in the wrong place like any other
    "last layer's to_out mask numbered by compact CLS rows": dict(row_div={4: 19}),
}


@pytest.mark.parametrize("what", list(SENSITIVITY))
def test_dropout_parity_notices_a_mask_in_the_wrong_place(what):
    """Self-check of the comparison: a reference whose masks are right in distribution and wrong in place (one site seeded differently;
    pos_drop's mask one token row further) must FAIL the same comparison, its worst element by at least 10 x GRAD_TOL."""
    from oracle.dropout import Dropout
    case = tc.CASES["ragged-l2h8-mixed"]
    wrong = SENSITIVITY[what]
    pairs, labels = tc.case_pairs_labels(case)
    got = {}
    with pytest.raises(AssertionError):
        run_step_case("wrong reference: " + what, case.layers, case.heads, list(case.num_objs), pairs, labels, precision=case.precision,
                      dropout=True, torch_seed=case.torch_seed, batch_seed=case.batch_seed, collect=got,
                      wrong_masks=lambda d: Dropout(d.p_pos, d.p_emb, d.p_attn, d.seed, **wrong))
    name, (elem, norm) = max(got["res"].items(), key=lambda kv: kv[1][0])
    _report("sensitivity %s: the comparison fails, worst element error %.2e (%.0f x GRAD_TOL) at %s" % (what, elem, elem / GRAD_TOL, name))
    assert elem >= 10 * GRAD_TOL, (what, name, elem)


@pytest.mark.parametrize("env", [{"VETO_TRAIN_LN_SPLIT": "1"}, {"VETO_TRAIN_RECOMPUTE": "1"}, {"VETO_TRAIN_GELU_EPI": "0", "VETO_TRAIN_QKV_F24": "0"}],
                         ids=["ln-backward-emits-masked-split-rows", "recompute-instead-of-keeping", "round5-forms"])
def test_dropout_step_gradients_behind_the_knobs(env):
    """The ragged mixed case in the forms a knob selects (read once per process: a fresh child pytest process per environment, as
    test_step_gradients_behind_the_knobs does): the LayerNorm backward that applies the to_out mask to its split rows and column
    partials itself, and the recompute path, which must see the forward's masks."""
    here = os.path.abspath(__file__)
    p = subprocess.run([sys.executable, "-m", "pytest", here + "::test_dropout_step_gradients[ragged-l2h8-mixed]", "-q", "-x", "-s", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=dict(os.environ, **env), timeout=900, cwd=os.path.dirname(os.path.dirname(here)),
                       capture_output=True, text=True)
    lines = [line for line in p.stdout.splitlines() if line.startswith("PARITY ")]
    for line in lines:
        _report("knobs %s | %s" % (" ".join("%s=%s" % kv for kv in env.items()), line[7:]))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert len(lines) == 1 and "1 passed" in p.stdout, p.stdout[-2000:]
