"""CPU side of the dropout-on training step parity (tests/test_train_dropout_gpu.py): the oracle with explicit masks
(oracle/train_oracle.py::train_step(dropout=...), oracle/dropout.py) is checked against itself, and the premise about the GPU cases'
inputs -- no ReLU within float32 rounding of its kink -- is asserted here, where it can be computed without a device."""
import numpy as np
import pytest
import torch

import train_dropout_cases as tc
from conftest import VG_MEET_GROUPS
from oracle import dropout as od
from oracle import train_oracle as to
from oracle import veto_oracle as vo


def _inputs(case):
    pairs, labels = tc.case_pairs_labels(case)
    cfg = vo.OracleConfig(case.layers, case.heads, mode=case.mode, meet_groups=VG_MEET_GROUPS if case.meet else None, prefix="model." if case.meet else "")
    return tc.case_state_dict(case), cfg, tc.case_batch(case), pairs, np.concatenate(labels)


def _outputs(res):
    return [res["logits"], res["d_roi_features"], res["d_roi_depth_features"]] + [res["grads"][k] for k in sorted(res["grads"])]


def test_no_dropout_and_zero_rates_are_todays_step_bit_for_bit():
    sd, cfg, batch, pairs, labels = _inputs(tc.CASES["hand-made"])
    plain = to.train_step(sd, cfg, batch, pairs, labels)
    for drop in (None, od.Dropout(0.0, 0.0, 0.0, seed=0x1234567890ABCDEF)):
        res = to.train_step(sd, cfg, batch, pairs, labels, dropout=drop)
        assert res["losses"] == plain["losses"] and sorted(res["grads"]) == sorted(plain["grads"])
        assert all(torch.equal(a, b) for a, b in zip(_outputs(res), _outputs(plain)))
    # and the masks do something: the reference's rates change the loss
    res = to.train_step(sd, cfg, batch, pairs, labels, dropout=tc.case_dropout(tc.CASES["hand-made"]))
    assert abs(res["losses"]["rel_loss"] - plain["losses"]["rel_loss"]) > 1e-3


def test_masks_are_numbered_by_the_global_pair_row_whatever_the_chunk():
    """214 pairs in chunks of 37 and of 100 (neither divides 214) and in one chunk: only the order of float64 sums changes."""
    case = tc.CASES["ragged-l2h8-mixed"]
    sd, cfg, batch, pairs, labels = _inputs(case)
    drop = tc.case_dropout(case)
    runs = [to.train_step(sd, cfg, batch, pairs, labels, dropout=drop, pair_chunk=c) for c in (37, 100, 1 << 20)]
    for other in runs[1:]:
        worst = max(float((a - b).abs().max() / b.abs().max().clamp(min=1e-300)) for a, b in zip(_outputs(runs[0]), _outputs(other)))
        assert worst < 1e-11, worst
        assert all(abs(runs[0]["losses"][k] - other["losses"][k]) < 1e-12 for k in other["losses"])
    assert od.keep_mask(5, 7, 576, 1000, row0=3).equal(od.keep_mask(5, 10, 576, 1000)[3:])
    assert od.keep_mask(5, 4, 576, 1000, row_step=19).equal(od.keep_mask(5, 58, 576, 1000)[::19])


FD_TENSORS = ["pos_embed.1.weight", "fusion_transformer.transformer.pos_embedding", "fusion_transformer.transformer.layers.0.0.fn.to_out.0.weight",
              "fusion_transformer.transformer.layers.1.0.fn.to_out.0.weight", "fusion_transformer.transformer.layers.0.0.fn.to_out.0.bias",
              "fusion_transformer.transformer.layers.1.0.fn.to_out.0.bias", "roi_features", "roi_depth_features"]
# (not location_projection.0 / class_projection.0: a step along them moves a ReLU's pre-activation directly, 1e-6 for a step of 1e-7 against
# the case's smallest 2e-6, and a difference quotient across a kink measures the kink)


@pytest.mark.parametrize("name", FD_TENSORS + ["all of them"])
def test_masked_oracle_is_its_own_gradient(name):
    """Central finite differences of the masked forward in float64 along a random direction of one tensor (and of all of them at once)
    against <gradient, direction>: 1e-6 relative.  Step 1e-7: truncation ~ 1e-14, rounding of the loss (~4, 2^-52) over the step ~ 1e-8
    absolute; it moves no pre-activation of the case across a ReLU kink (smallest 2e-6, below)."""
    case = tc.CASES["hand-made"]
    sd, cfg, batch, pairs, labels = _inputs(case)
    drop = tc.case_dropout(case)
    names = FD_TENSORS if name == "all of them" else [name]
    gen = torch.Generator().manual_seed(len(name))
    base = {n: torch.from_numpy(np.asarray(batch[n] if n.startswith("roi_") else sd[n])).double() for n in names}
    res = to.train_step(sd, cfg, batch, pairs, labels, dropout=drop)
    grads = {n: res["d_" + n] if n.startswith("roi_") else res["grads"][n] for n in names}
    # random magnitudes, every component uphill: the directional derivative is then sum |g_i| |r_i|, far above the rounding of the
    # difference quotient, where a plain random direction leaves a near-cancelling sum (2e-3 for pos_embed.1.weight: 4e-6 of rounding)
    dirs = {n: torch.randn(v.shape, generator=gen, dtype=torch.float64).abs() * torch.sign(grads[n]) for n, v in base.items()}
    analytic = sum(float((grads[n] * dirs[n]).sum()) for n in names)

    def loss_at(eps):
        sd2, batch2 = dict(sd), dict(batch)
        for n in names:
            (batch2 if n.startswith("roi_") else sd2)[n] = base[n] + eps * dirs[n]
        return sum(to.train_step(sd2, cfg, batch2, pairs, labels, dropout=drop)["losses"].values())

    eps = 1e-7
    numeric = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
    assert abs(analytic) > 1e-2 and abs(numeric - analytic) < 1e-6 * abs(analytic), (numeric, analytic)


def test_sites_keep_their_share_and_differ_from_each_other():
    drop = od.Dropout(*tc.RATES, seed=tc.step_seed(2))
    rows = 4066
    f = {site: drop.factor(site, rows, 576, torch.float64) for site in (1, 2, 3, 4)}
    f[1] = drop.factor(1, 28, 128, torch.float64)
    for site, fac in f.items():
        p = drop.rate(site)
        assert set(fac.unique().tolist()) == {0.0, od.scale(p)} and abs(od.scale(p) - 1 / (1 - p)) < 1e-6
        kept = float((fac != 0).double().mean())
        assert abs(kept - (1 - p)) < 4 * (p * (1 - p) / fac.numel()) ** 0.5 + 2.0 ** -24, (site, kept)
    # two sites are independent masks: they agree on p_a p_b + (1 - p_a)(1 - p_b) of the elements, not on all of them
    for a, b in ((2, 3), (2, 4), (3, 4)):      # (3, 4): layer 0's mask against layer 1's
        agree = float(((f[a] != 0) == (f[b] != 0)).double().mean())
        pa, pb = drop.rate(a), drop.rate(b)
        want = pa * pb + (1 - pa) * (1 - pb)
        assert abs(agree - want) < 4 * (want * (1 - want) / f[a].numel()) ** 0.5, (a, b, agree)
    head = drop.factor(2, 28, 128, torch.float64)      # site 2 on site 1's element indices (0 .. 28 * 128 - 1), at site 1's rate
    same_rate = od.keep_mask(drop.site_seed(2), 28, 128, od.threshold(0.1))
    assert float(((f[1] != 0) == same_rate).double().mean()) < 0.9 and head is not None
    assert od.threshold(0.1) == 1677721 and od.threshold(0.35) == 5872025 and od.threshold(0.0) == 0


@pytest.mark.parametrize("tag", list(tc.CASES))
def test_no_relu_of_a_gpu_case_sits_on_its_kink(tag):
    """The premise of the element-wise comparison on the device: under the masks the step will use, the smallest |pre-activation| at
    the ReLUs of pos_embed, location_projection and class_projection (float64) exceeds MARGIN x the largest float32 rounding of the dot
    product in front of it, so no ReLU derivative of the case can be decided by rounding (the docstring of
    test_step_gradients_ragged_batch_sampled_pairs documents what that looks like).  The seeds in tests/train_dropout_cases.py were
    chosen on the CPU for this to hold; a change of the synthetic inputs or of the seed draw that breaks it fails here first."""
    prem = tc.relu_premise(tc.CASES[tag])
    assert set(prem) == {"pos_embed", "location_projection", "class_projection"}
    for relu, (smallest, rounding) in prem.items():
        assert rounding < 2e-6, (relu, rounding)      # float32 on O(1) dot products of at most 400 terms
        assert smallest > tc.MARGIN * rounding, (tag, relu, smallest, rounding)
