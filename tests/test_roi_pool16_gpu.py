"""ROI pooling with outputs of 9 x 9 to 16 x 16 on the device (a lane of roi_pool_kernel walks ceil(P*P / 64) bins): forward bit for
bit against oracle/roi_align_oracle.py -- which tests/test_roi_pool16_cases_host.py holds to the reference's compiled kernel -- and
against that kernel's fixture directly, every launch twice; the atomic backward per pixel inside the any-order float32 bound of
tests/test_roi_pool_gpu.py with K and the sum taken from the oracle; the ordered backward twice, bit-equal, and equal to the order
include/veto_amd.h states; P = 17 and P * G = 33 refused; one end-to-end VETORelationHead.forward at (16, 4)."""
import ctypes

import numpy as np
import pytest
import torch

import deterministic_cases as dc
import roi_pool16_cases as c16
import roi_pool_cases as rc
import test_deterministic_gpu as tdg
import test_roi_pool_gpu as trp
from oracle import roi_align_oracle as ro
from test_roi_pool16_cases_host import FIXTURE

pytestmark = pytest.mark.gpu
F = np.float32
_t, _dev = trp._t, trp._dev


@pytest.mark.parametrize("channels", c16.CHANNELS)
@pytest.mark.parametrize("pooled,ratio", c16.INSTANCES)
def test_forward_four_levels_and_depth_bit_exact(pooled, ratio, channels):
    """Pooler over 4 levels plus the depth map (with another channel count), 17 boxes: sub-pixel, hanging over the map edge,
    either side of every level boundary.  Two calls; outputs and levels bit for bit."""
    dch = c16.depth_channels_for(channels)
    feats, depth = c16.pyramid(channels, dch)
    boxes = c16.boxes()
    want_rgb, want_dep, want_lv = ro.pooler_forward(feats, boxes, depth, scales=rc.SCALES4, pooled=pooled, sampling_ratio=ratio, return_levels=True)
    p = trp._pooler(rc.SCALES4, pooled, ratio)
    maps, props, td = [_t(m) for m in feats], trp._props(boxes, (c16.W, c16.H)), _t(depth)
    rgb, dep = p(maps, props, depth_features=td)
    rgb2, dep2 = p(maps, props, depth_features=td)
    assert torch.equal(rgb.view(torch.int32), rgb2.view(torch.int32)) and torch.equal(dep.view(torch.int32), dep2.view(torch.int32))
    case = "pooler (%d, %d) C %d / depth %d" % (pooled, ratio, channels, dch)
    assert np.array_equal(p.last_levels.cpu().numpy(), want_lv), case
    trp._same_bits(rgb, want_rgb, case + " rgb")
    trp._same_bits(dep, want_dep, case + " depth")


@pytest.mark.parametrize("pooled,ratio", c16.INSTANCES)
def test_forward_equals_the_reference_kernel_fixture(pooled, ratio):
    from veto_amd import synth
    want = np.load(FIXTURE)["out_p%d_r%d" % (pooled, ratio)]
    feat, rois = synth.synthetic_roi_single(pooled, ratio, channels=want.shape[1])
    got = trp._roi_align(_t(feat), _t(rois), rc.SCALE, pooled, ratio)
    trp._same_bits(got, want, "reference kernel (%d, %d)" % (pooled, ratio))


BACKWARD = [(p, g, 33) for p, g in c16.INSTANCES] + [(16, 2, 1), (16, 2, 65)]


@pytest.mark.parametrize("pooled,ratio,channels", BACKWARD)
def test_backward_per_pixel_and_ordered_twice(pooled, ratio, channels):
    """The atomic entry through autograd against the oracle's gradients under gamma_K * A + one rounding per pixel (exact zeros where
    nothing lands); the ordered entry twice on NaN-filled maps: bit-equal to itself and to the stated order, and inside the same
    bound."""
    case = c16.roi_case(pooled, ratio, channels)
    boxes = c16.boxes()
    per_level, dep_ref = rc.pyramid_backward(case.g_rgb, case.g_dep, boxes, case.shapes, rc.SCALES4, case.depth_shape, pooled, ratio)
    feats, depth = c16.pyramid(channels, case.depth_shape[1])
    tf = [_t(f).requires_grad_(True) for f in feats]
    td = _t(depth).requires_grad_(True)
    rgb, dep = trp._pooler(rc.SCALES4, pooled, ratio)(tf, trp._props(boxes, (c16.W, c16.H)), depth_features=td)
    ((rgb * _t(case.g_rgb)).sum() + (dep * _t(case.g_dep)).sum()).backward()
    tag = "backward (%d, %d) C %d" % (pooled, ratio, channels)
    for l in range(4):
        trp._check_grad(tf[l].grad, per_level[l], "%s level %d" % (tag, l))
    trp._check_grad(td.grad, dep_ref, tag + " depth map")
    got = tdg._twice(lambda: tdg._roi_ordered(case), tag + " ordered")
    levels, dmap = dc.pooler_backward_ordered(case)
    for l, (g, w, ref) in enumerate(zip(got, levels + [dmap], per_level + [dep_ref])):
        tdg._same_bits(g, w, "%s ordered map %d" % (tag, l))
        trp._check_grad(g, ref, "%s ordered map %d" % (tag, l))


@pytest.mark.parametrize("pooled,ratio", c16.REFUSED)
def test_sizes_beyond_the_axis_tables_are_refused_and_nothing_is_written(pooled, ratio):
    from veto_amd import native, poolers
    feats, depth = c16.pyramid(1, 1)
    rois = _t(ro.to_rois(c16.boxes()))
    maps, td = [_t(m) for m in feats], _t(depth)
    out_rgb = torch.full((len(rois), 1, pooled, pooled), -7.0, device=_dev())
    out_dep = torch.full((len(rois), 1, pooled, pooled), -7.0, device=_dev())
    call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
    a = poolers._pool_args(call, maps, rc.SCALES4, rois, 2, pooled, ratio, tuple(td.shape), depth_feat=td, out_rgb=out_rgb, out_depth=out_dep)
    with pytest.raises(native.VetoError, match="pooled must be 1..16" if pooled > 16 else "at most 32"):
        call.run("veto_roi_pool", ctypes.byref(a))
    grads = [torch.full(m.shape, -7.0, device=_dev()) for m in maps]
    ptrs = (ctypes.c_void_p * 4)(*[g.data_ptr() for g in grads])
    for entry in ("veto_roi_pool_backward", "veto_roi_pool_backward_ordered"):
        with pytest.raises(native.VetoError):
            call.run(entry, ctypes.byref(a), call.ptr(out_rgb), None, ptrs, None)
    torch.cuda.synchronize()
    assert bool((out_rgb == -7).all()) and bool((out_dep == -7).all()) and all(bool((g == -7).all()) for g in grads)


def test_relation_head_from_feature_maps_at_16_4():
    """VETORelationHead.forward from tiny pyramid maps at POOLER_RESOLUTION 16 / PATCH_SIZE 4: the ROI maps it pools equal the pooler
    oracle's bit for bit, and the relation scores those of the predictor oracle on the oracle's maps, post-processed."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    from veto_amd.relation_head import VETORelationHead
    dev = _dev()
    num_objs = [3, 4]
    W, H = 128, 96
    sd = synth.predictor_state_dict(3, layers=2, patch=4)
    batch = synth.synthetic_batch(13, 2, num_objs, patch=4)
    batch["boxes"] = (batch["boxes"] * F(0.16)).astype(F)
    batch["image_size"] = (W, H)
    rng = np.random.RandomState(164)
    feats = [rng.randn(2, 256, H >> (2 + l), W >> (2 + l)).astype(F) for l in range(4)]
    depth = rng.randn(2, 256, H >> 4, W >> 4).astype(F)
    cfg = testing.make_config(2, 8, patch=4, resolution=16)
    ratio = int(cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO)
    head = VETORelationHead(cfg)
    head.predictor = testing.make_predictor(cfg, sd, dev)
    head.to(dev).eval()
    props = testing.make_proposals(batch, "predcls", dev)
    with torch.no_grad():
        roi, result, losses = head([_t(f) for f in feats], props, depth_features=_t(depth))
    torch.cuda.synchronize()
    boxes = np.split(batch["boxes"], np.cumsum(num_objs)[:-1])
    want_rgb, want_dep = ro.pooler_forward(feats, boxes, depth, scales=rc.SCALES4, pooled=16, sampling_ratio=ratio)
    trp._same_bits(roi, want_rgb, "relation head (16, 4) roi_features")
    batch["roi_features"], batch["roi_depth_features"] = want_rgb, want_dep
    logits, _, _ = vo.forward(sd, vo.OracleConfig(layers=2, heads=8, patch=4), batch)
    pairs = [vo.enumerate_test_pairs(n) for n in num_objs]
    onehot = np.full((sum(num_objs), 151), -1000.0, dtype=F)
    onehot[np.arange(sum(num_objs)), batch["labels"]] = 1000.0
    ref = vo.postprocess(logits.numpy(), onehot, pairs, num_objs)
    assert losses == {}
    for r, o in zip(result, ref):
        # row by pair, not by rank: near-ties (logit noise 3e-5) may swap neighbours in the ranking
        got = {tuple(p): (s, l) for p, s, l in zip(r.get_field("rel_pair_idxs").cpu().numpy().tolist(), r.get_field("pred_rel_scores").cpu().numpy(),
                                                  r.get_field("pred_rel_labels").cpu().numpy())}
        want = {tuple(p): (s, l) for p, s, l in zip(o["rel_pair_idxs"].numpy().tolist(), o["pred_rel_scores"].numpy(), o["pred_rel_labels"].numpy())}
        assert set(got) == set(want)
        for k in want:
            assert np.abs(got[k][0] - want[k][0]).max() < 1e-4 and got[k][1] == want[k][1], k
