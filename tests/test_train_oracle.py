"""oracle/train_oracle.py::train_step -- the float64 autograd restatement of the whole training step -- held to what the
reference's own autograd produced (tests/golden/train_*.npz: losses, classifier logits, per parameter and per ROI input
the gradient norm and a strided sample), and its chunked accumulation held to itself.  No GPU: the GPU tests in
tests/test_train_scale_gpu.py take this function as their reference at sizes no golden exists for."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle import train_oracle as to
from oracle import veto_oracle as vo

TRAIN_GOLDENS = ["train_vanilla", "train_vanilla_beta", "train_vanilla_sgcls", "train_vanilla_l1h6_ragged",
                 "train_meet_vg", "train_meet_gqa", "train_meet_sgcls", "train_meet_l3h4", "train_meet_experts"]

# The goldens are float32 autograd, the oracle float64: their distance is the reference's own float32 rounding.  Measured over
# the nine goldens on the CPU (scale as in test_training_backward_matches_reference_gradients), worst case and where:
#   gradient sample 1.65e-6, gradient norm 1.03e-6, ROI-input sample 8.78e-7, ROI-input norm 2.68e-7 (all train_vanilla_beta),
#   loss 9.03e-7 absolute (train_meet_experts), logits 4.48e-6 absolute (train_meet_vg, logits up to 5.8).
# The assertions are those figures times 4 (float32 reductions of the reference depend on its thread count,
# tests/cpu_probe_oracle_threads.py); the gradient ones are 300 times below the 2e-3 of the GPU gradient tests.
GRAD_SAMPLE_TOL = 4 * 1.65e-6
GRAD_NORM_TOL = 4 * 1.03e-6
INPUT_SAMPLE_TOL = 4 * 8.78e-7
INPUT_NORM_TOL = 4 * 2.68e-7
LOSS_TOL = 4 * 9.03e-7
LOGIT_TOL = 4 * 4.48e-6


def golden_case(name):
    """(fixture, state dict, OracleConfig, batch, pair lists, loss spec) of one train_*.npz, inputs regenerated."""
    from veto_amd import synth
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    dataset, meet = str(g["dataset"]), bool(int(g["meet"]))
    n_obj_cls, n_rel = (151, 51) if dataset == "VG" else (201, 101)
    layers, heads = int(g["layers"]), int(g["heads"])
    num_objs = [int(x) for x in g["num_objs"]]
    experts = 3 if int(g["experts"]) else 0
    if meet:
        groups = [int(x) for x in g["group_sizes"]]
        sd = synth.meet_state_dict(0, groups, layers=layers, num_obj_cls=n_obj_cls, experts=experts)
        cfg = vo.OracleConfig(layers, heads, mode=str(g["mode"]), meet_groups=groups, prefix="model.", experts=experts)
        loss = {"chosen": [g["chosen_%d" % k] for k in range(len(groups))], "incre_idx_list": g["incre_idx_list"]}
    else:
        sd = synth.predictor_state_dict(0, layers=layers, num_obj_cls=n_obj_cls, num_rel_cls=n_rel)
        cfg = vo.OracleConfig(layers, heads, mode=str(g["mode"]))
        loss = {"weight": g["class_weights"]} if int(g["beta_loss"]) else None
    batch = synth.synthetic_batch(7, len(num_objs), num_objs, num_obj_cls=n_obj_cls)
    pairs = [vo.enumerate_test_pairs(n) for n in num_objs]
    return g, sd, cfg, batch, pairs, loss


def _sample_errors(got, ref_norm, ref_s, step):
    got = got.reshape(-1).numpy().astype(np.float64)
    ref_s = ref_s.astype(np.float64)
    scale = max(np.abs(ref_s).max(), ref_norm / np.sqrt(got.size), 1e-12)
    return np.abs(got[::step] - ref_s).max() / scale, abs(np.linalg.norm(got) - ref_norm) / max(ref_norm, 1e-12)


@pytest.mark.parametrize("name", TRAIN_GOLDENS)
def test_train_oracle_matches_reference_losses_and_gradients(name):
    g, sd, cfg, batch, pairs, loss = golden_case(name)
    res = to.train_step(sd, cfg, batch, pairs, g["labels"], loss)
    ref_losses = {k[5:]: float(v) for k, v in g.items() if k.startswith("loss_")}
    assert set(res["losses"]) == set(ref_losses)
    worst = {"loss": 0.0, "logits": 0.0, "grad": 0.0, "gradnorm": 0.0, "input": 0.0, "inputnorm": 0.0}
    for k, ref in ref_losses.items():
        worst["loss"] = max(worst["loss"], abs(res["losses"][k] - ref))
    col = 0
    for k in range(sum(1 for x in g if x.startswith("logits_"))):
        ref = g["logits_%d" % k]
        worst["logits"] = max(worst["logits"], float(np.abs(res["logits"][:, col:col + ref.shape[1]].numpy() - ref).max()))
        col += ref.shape[1]
    assert col == res["logits"].shape[1]
    names = [k[9:] for k in g if k.startswith("gradnorm_")]
    # (EXPERT_GROUP: named_parameters() lists the last expert's heads once, as rel_out.k; the oracle gives both names)
    extra = set(res["grads"]) - set(names)
    assert set(names) <= set(res["grads"]) and all(".rel_out_group.%d." % (cfg.experts - 1) in k for k in extra), set(names) ^ set(res["grads"])
    who = None
    for pname in names:
        err, nerr = _sample_errors(res["grads"][pname], float(g["gradnorm_" + pname]), g["gradsample_" + pname], int(g["gradstep_" + pname]))
        if err > worst["grad"]:
            who = pname
        worst["grad"], worst["gradnorm"] = max(worst["grad"], err), max(worst["gradnorm"], nerr)
    for iname in ("roi_features", "roi_depth_features"):
        err, nerr = _sample_errors(res["d_" + iname], float(g["inputgradnorm_" + iname]), g["inputgradsample_" + iname],
                                   int(g["inputgradstep_" + iname]))
        worst["input"], worst["inputnorm"] = max(worst["input"], err), max(worst["inputnorm"], nerr)
    print("%s: %s (worst gradient sample at %s)" % (name, " ".join("%s %.2e" % kv for kv in worst.items()), who))
    assert worst["loss"] < LOSS_TOL and worst["logits"] < LOGIT_TOL, worst
    assert worst["grad"] < GRAD_SAMPLE_TOL and worst["gradnorm"] < GRAD_NORM_TOL, (worst, who)
    assert worst["input"] < INPUT_SAMPLE_TOL and worst["inputnorm"] < INPUT_NORM_TOL, worst


def _rel_diff(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_train_oracle_chunking_does_not_change_the_result():
    """Pairs are independent given the per-object prelude, so the chunk size only reorders float64 sums: two chunk sizes (one of
    them not dividing the pair count, the other a single chunk) agree to ~1e-12 relative on every output."""
    g, sd, cfg, batch, pairs, loss = golden_case("train_meet_sgcls")
    a = to.train_step(sd, cfg, batch, pairs, g["labels"], loss, pair_chunk=37)
    b = to.train_step(sd, cfg, batch, pairs, g["labels"], loss, pair_chunk=1 << 20)
    assert set(a["grads"]) == set(b["grads"])
    worst = max([_rel_diff(a["grads"][k], b["grads"][k]) for k in a["grads"]]
                + [_rel_diff(a["d_roi_features"], b["d_roi_features"]), _rel_diff(a["d_roi_depth_features"], b["d_roi_depth_features"]),
                   _rel_diff(a["logits"], b["logits"])]
                + [abs(a["losses"][k] - b["losses"][k]) for k in a["losses"]])
    print("chunk 37 against one chunk: worst relative difference %.2e" % worst)
    assert worst < 1e-12


def test_train_oracle_batchnorm_uses_batch_statistics():
    """pos_embed.0 in training mode: the result does not depend on the stored running statistics, and the statistics it reports
    are the ones nn.BatchNorm1d normalises with (biased) and moves its running variance by (unbiased)."""
    g, sd, cfg, batch, pairs, loss = golden_case("train_vanilla_l1h6_ragged")
    a = to.train_step(sd, cfg, batch, pairs, g["labels"], loss)
    sd2 = dict(sd)
    sd2["pos_embed.0.running_mean"] = sd["pos_embed.0.running_mean"] + 50.0
    sd2["pos_embed.0.running_var"] = sd["pos_embed.0.running_var"] * 3.0
    b = to.train_step(sd2, cfg, batch, pairs, g["labels"], loss)
    assert torch.equal(a["logits"], b["logits"])
    bn = torch.nn.BatchNorm1d(4, momentum=0.001).double().train()
    feat = vo.center_xywh_from_xyxy(torch.from_numpy(batch["boxes"]).double())
    bn(feat)
    mean, var_b, var_u = a["bn_batch_stats"]
    assert torch.allclose(bn.running_mean, 0.001 * mean, rtol=1e-12)
    assert torch.allclose(bn.running_var, 0.999 + 0.001 * var_u, rtol=1e-12)
    assert torch.allclose(var_b * len(feat) / (len(feat) - 1), var_u, rtol=1e-12)
