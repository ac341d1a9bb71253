"""Patch grids other than (8, 2) on the CPU: the oracles against the real reference's outputs at (4, 1), (12, 3) and (16, 4)
(tests/golden/patchgrid/, made by tests/golden/make_golden_patchgrid.py), the numpy patchify of tests/patchgrid_cases.py against
einops, the self-check of the restatement the GPU tests use (three wrong ones must move an expected row), and the refusals the
predictor raises before the library is touched.

oracle/veto_oracle.py and oracle/train_oracle.py turned out to assume nothing about 8 x 8 maps: both go through
veto_oracle.patchify(x, cfg.patch), so nothing had to be restated for them."""
import numpy as np
import pytest
import torch

import patchgrid_cases as pg
import test_oracle_golden as tog
import test_train_oracle as tto
from oracle import train_oracle as to
from oracle import veto_oracle as vo

EVAL_FIXTURES = [pg.golden_name(r, p, k) for r, p in pg.NEW_GRIDS for k in pg.KINDS]


@pytest.mark.parametrize("name", EVAL_FIXTURES)
def test_oracle_matches_reference_at_every_patch_grid(name):
    """veto_oracle.forward(patch=p) against the reference's logits, token sample and object decisions, within the bound of
    tests/test_oracle_golden.py; the pair enumeration (placeholder pair of the one-object image included) bit for bit."""
    g, sd, batch, cfg, pairs = pg.load(name)
    assert np.array_equal(np.concatenate([vo.enumerate_test_pairs(n) for n in batch["num_objs"]]), g["pair_idx"])
    if "sgcls" in name:
        assert 1 in batch["num_objs"] and len(pairs[batch["num_objs"].index(1)]) == 1
    want_p = 256 * 2 * cfg.patch ** 2
    assert sd[cfg.prefix + pg.T + "patch_embed.proj_d.weight"].shape == (512, want_p)
    assert batch["roi_features"].shape[1:] == (256, 4 * cfg.patch, 4 * cfg.patch)
    torch.set_num_threads(8)
    logits, _, _, inter = vo.forward(sd, cfg, batch, rel_pair_idxs=pairs, return_intermediates=True)
    assert np.array_equal(inter["obj_dists"].argmax(1).numpy(), g["obj_dists_argmax"])
    err = np.abs(logits.numpy() - pg.golden_logits(g, cfg)).max()
    print("PATCHGRID oracle %s: logits %.2e of %.0e" % (name, err, tog.TOL))
    assert err <= tog.TOL, (name, err)
    if cfg.meet_groups is None:
        step = int(g["tokens_step"])
        assert np.abs(inter["tokens"][::step, :, ::9].numpy() - g["tokens_sample"]).max() <= 1e-5
    else:
        assert vo.meet_incre_idx_list(cfg.meet_groups) == [int(x) for x in g["incre_idx_list"]]


def test_state_dict_keys_do_not_depend_on_the_patch_size():
    a = pg.load("r16p4_predcls")[0]["state_dict_keys"]
    b = np.load(pg.os.path.join(pg.os.path.dirname(pg.GOLDEN_DIR), "predcls_n10_l4h8.npz"))["state_dict_keys"]
    strip = lambda keys: sorted(k for k in keys if ".layers." not in k)      # (the fixtures differ in ENC_LAYERS only)
    assert strip(a) == strip(b)


def test_train_oracle_matches_reference_gradients_at_16_4():
    """train_oracle.train_step at (16, 4) against the reference's own autograd, under the bounds of tests/test_train_oracle.py.  The
    proj_d gradient has 4 M entries: the fixture holds its norm and a strided sample, as for every large tensor."""
    g, sd, cfg, batch, pairs = pg.train_case()
    assert int(g["gradstep_fusion_transformer.transformer.patch_embed.proj_d.weight"]) == 512 * 8192 // 512
    res = to.train_step(sd, cfg, batch, pairs, g["labels"], None)
    assert abs(res["losses"]["rel_loss"] - float(g["loss_rel_loss"])) < tto.LOSS_TOL
    assert float(np.abs(res["logits"].numpy() - g["logits_0"]).max()) < tto.LOGIT_TOL
    names = [k[9:] for k in g if k.startswith("gradnorm_")]
    assert set(names) == set(res["grads"])
    worst = [0.0, 0.0, 0.0, 0.0]
    for n in names:
        e, ne = tto._sample_errors(res["grads"][n], float(g["gradnorm_" + n]), g["gradsample_" + n], int(g["gradstep_" + n]))
        worst[0], worst[1] = max(worst[0], e), max(worst[1], ne)
    for n in ("roi_features", "roi_depth_features"):
        assert tuple(res["d_" + n].shape[1:]) == (256, 16, 16)
        e, ne = tto._sample_errors(res["d_" + n], float(g["inputgradnorm_" + n]), g["inputgradsample_" + n], int(g["inputgradstep_" + n]))
        worst[2], worst[3] = max(worst[2], e), max(worst[3], ne)
    print("PATCHGRID train oracle (16, 4): gradient sample %.2e norm %.2e, ROI input sample %.2e norm %.2e" % tuple(worst))
    assert worst[0] < tto.GRAD_SAMPLE_TOL and worst[1] < tto.GRAD_NORM_TOL, worst
    assert worst[2] < tto.INPUT_SAMPLE_TOL and worst[3] < tto.INPUT_NORM_TOL, worst


# ---- patchify ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_numpy_patchify_is_the_reference_rearrange(p):
    from einops import rearrange
    x = np.random.default_rng(p).standard_normal((3, 5, 4 * p, 4 * p))
    ref = rearrange(torch.from_numpy(x), "b c (h p1) (w p2) -> b (h w) (p1 p2 c)", p1=p, p2=p).numpy()
    assert np.array_equal(pg.patchify_np(x, p), ref)
    assert np.array_equal(vo.patchify(torch.from_numpy(x), p).numpy(), ref)
    if p > 1:
        assert not np.array_equal(pg.patchify_np(x, p, ("c_first",)), ref) and not np.array_equal(pg.patchify_np(x, p, ("p_swapped",)), ref)


def test_restatement_agrees_with_the_oracle_and_wrong_ones_do_not():
    """The per-object float64 restatement at p = 3 equals the oracle's per-pair tokens to float64 rounding, and each of three wrong
    restatements -- (c p1 p2) feature order, p1 / p2 swapped, proj_d on the RGB maps -- moves the row of the first pair's first patch
    token by far more than the bound the GPU test allows there."""
    _, sd, batch, cfg, pairs = pg.load("r12p3_predcls")
    ref = pg.oracle_patch_tokens(sd, cfg, batch, pairs)
    tok, bound = pg.patch_tokens(sd, batch, pairs, 3)
    assert np.abs(tok - ref).max() < 1e-11
    assert (bound > 0).all() and bound.max() < 0.05      # a bound that could not tell a wrong row from a right one would be no check
    for wrong in ("c_first", "p_swapped", "rgb_first"):
        bad, _ = pg.patch_tokens(sd, batch, pairs, 3, wrong=(wrong,))
        moved = np.abs(bad[0, 0] - ref[0, 0]) / bound[0, 0]
        print("PATCHGRID wrong restatement %s: row (pair 0, token 1) moves by up to %.0f bounds, median %.0f" % (wrong, moved.max(), np.median(moved)))
        assert np.median(moved) > 10, wrong


# ---- refusals in Python -----------------------------------------------------------------------------------------------------------------
def _predictor(res, patch):
    from veto_amd import synth, testing
    return testing.make_predictor(testing.make_config(2, 8, patch=patch, resolution=res), synth.predictor_state_dict(0, layers=2, patch=patch), "cpu")


@pytest.mark.parametrize("res,patch", pg.REFUSED)
def test_predictor_refuses_other_grids_by_name(res, patch, monkeypatch):
    from veto_amd import native
    monkeypatch.setattr(native, "load_library", lambda *a, **k: pytest.fail("the library was touched"))
    with pytest.raises(ValueError) as e:
        _predictor(res, patch)
    msg = str(e.value)
    assert all("(%d, %d)" % q in msg for q in pg.GRIDS) and "19 tokens" in msg and str(res) in msg


@pytest.mark.parametrize("res,patch", pg.GRIDS)
def test_predictor_builds_every_supported_grid_and_checks_the_map_shape(res, patch, monkeypatch):
    from veto_amd import native
    from veto_amd.structures import BoxList
    monkeypatch.setattr(native, "load_library", lambda *a, **k: pytest.fail("the library was touched"))
    model = _predictor(res, patch)
    assert model.fusion_transformer.transformer.patch_embed.proj_d.weight.shape == (512, 512 * patch * patch)
    props = [BoxList(torch.zeros(2, 4), (800, 600), mode="xyxy")]
    props[0].add_field("labels", torch.ones(2, dtype=torch.int64))
    wrong = res + 4 if res < 16 else 8
    maps = torch.zeros(2, 256, wrong, wrong)
    with pytest.raises(ValueError, match=r"\[N, 256, %d, %d\]" % (res, res)):
        model(props, [torch.tensor([[0, 1], [1, 0]])], None, None, roi_features=maps, roi_depth_features=maps)
