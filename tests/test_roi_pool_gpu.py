"""ROI pooling on the device against oracle/roi_align_oracle.py: every kernel instance, edge, level and gradient.

Forward: bit for bit.  Backward: per pixel, |device - oracle| <= gamma_K * A + one rounding, where K (number of contributions) and
A (sum of their absolute values) come from the oracle and gamma_K = K u / (1 - K u), u = 2^-24 -- the error of a float32 accumulation
of K terms in ANY order; where K = 0 the device value must be exactly 0.  The inputs and the reasons they can tell a wrong kernel from a
right one are in tests/roi_pool_cases.py and tests/test_roi_pool_cases_host.py.  Each test prints one "roi_pool_parity:" line (pytest -s);
profiles/roi_pool_parity.txt keeps them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

pytestmark = pytest.mark.gpu
F = np.float32


def _dev():
    return torch.device("cuda:0")


def _t(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), **kw)


def _line(case, compared, mismatches, extra=""):
    print("roi_pool_parity: %-34s compared %9d  mismatches %d%s" % (case, compared, mismatches, ("  " + extra) if extra else ""))


def _same_bits(got, want, case, extra=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = int((got.view(np.int32) != np.asarray(want, dtype=F).view(np.int32)).sum()) if got.shape == want.shape else -1
    _line(case, want.size, bad, extra)
    assert got.shape == want.shape and got.dtype == np.float32, (case, got.shape, want.shape)
    assert np.array_equal(got, want), (case, bad, np.abs(got - want).max())      # (no NaN is expected on either side)
    return got


def _roi_align(feat, rois, scale, pooled, ratio):
    """Two launches of the same call: (first output, asserted bit-identical to the second)."""
    from veto_amd.poolers import ROIAlign
    m = ROIAlign((pooled, pooled), scale, ratio)
    a, b = m(feat, rois), m(feat, rois)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches of one call differ"
    return a


def _pooler(scales, pooled=8, ratio=2):
    from veto_amd.poolers import Pooler
    p = Pooler((pooled, pooled), scales, ratio)
    p.keep_levels = True
    return p


def _props(boxes, size):
    from veto_amd.structures import BoxList
    return [BoxList(torch.from_numpy(np.asarray(b, dtype=F).reshape(-1, 4)), size).to(_dev()) for b in boxes]


def _check_grad(got, ref, case, extra_tol=None):
    """got against ref = (want, K, A) of the oracle under the bound of the module docstring; prints K max and error / bound."""
    want, K, A = ref
    got = got.detach().float().cpu().numpy()
    if extra_tol is not None:                  # a gradient that was rounded once more on its way (float16 leaves)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= rc.backward_bound(want, K, A) + extra_tol(want)).all(), case
        assert not got[np.broadcast_to((K == 0)[:, None], want.shape)].any(), case
        _line(case, want.size, 0, "K max %d" % K.max())
        return
    ratio, kmax = rc.check_backward(got, want, K, A)
    _line(case, want.size, 0, "K max %d  zero pixels %d  error / bound %.3f" % (kmax, int((K == 0).sum()) * want.shape[1], ratio))
    assert ratio <= 1.0, (case, ratio)


# ---- section 1: forward, bit for bit, every instance and lane layout -----------------------------------------------------------------
@pytest.mark.parametrize("pooled,ratio", rc.FORWARD_INSTANCES)
def test_forward_every_instance_bit_exact(pooled, ratio):
    feat, rois = rc.single(pooled, ratio, 40)
    got = _roi_align(_t(feat), _t(rois), rc.SCALE, pooled, ratio)
    _same_bits(got, ro.roi_align(feat, rois, rc.SCALE, pooled, ratio), "forward (%d, %d) C 40" % (pooled, ratio))


@pytest.mark.parametrize("channels", rc.FORWARD_CHANNELS)
def test_forward_channel_tails_bit_exact(channels):
    feat, rois = rc.single(8, 2, channels)
    got = _roi_align(_t(feat), _t(rois), rc.SCALE, 8, 2)
    _same_bits(got, ro.roi_align(feat, rois, rc.SCALE, 8, 2), "forward (8, 2) C %d" % channels)


# ---- section 2: unequal channel counts and level counts through Pooler ------------------------------------------------------------
@pytest.mark.parametrize("n_levels", [4, 3, 1])
@pytest.mark.parametrize("depth_channels", [8, 72])
def test_pooler_unequal_channels_and_level_counts(depth_channels, n_levels):
    feats, depth, boxes = rc.pyramid(channels=40, depth_channels=depth_channels)
    maps, scales = rc.level_form(feats, n_levels)
    want_rgb, want_dep, want_lv = ro.pooler_forward(maps, boxes, depth, scales=scales, return_levels=True)
    if n_levels == 3:
        assert (want_lv == 2).sum() >= 6
    p = _pooler(scales)
    rgb, dep = p([_t(m) for m in maps], _props(boxes, (rc.PYR_W, rc.PYR_H)), depth_features=_t(depth))
    case = "pooler %d levels, C 40 / depth %d" % (n_levels, depth_channels)
    assert p.last_levels.dtype == torch.int32 and np.array_equal(p.last_levels.cpu().numpy(), want_lv), case
    _same_bits(rgb, want_rgb, case + " rgb")
    _same_bits(dep, want_dep, case + " depth")


def test_two_scales_with_a_depth_map_are_refused_and_nothing_is_written():
    from veto_amd import native, poolers
    feats, depth, boxes = rc.pyramid(channels=40, depth_channels=8)
    maps, scales = [_t(m) for m in feats[:2]], rc.SCALES4[:2]
    with pytest.raises(native.VetoError, match="depth pooler is level 2"):
        _pooler(scales)(maps, _props(boxes, (rc.PYR_W, rc.PYR_H)), depth_features=_t(depth))
    # the same call through the C ABI with outputs of our own: refused before any launch
    rois, td = _t(ro.to_rois(boxes)), _t(depth)
    out_rgb = torch.full((len(rois), 40, 8, 8), -7.0, device=_dev())
    out_dep = torch.full((len(rois), 8, 8, 8), -7.0, device=_dev())
    out_lv = torch.full((len(rois),), -7, dtype=torch.int32, device=_dev())
    call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
    a = poolers._pool_args(call, maps, scales, rois, 2, 8, 2, tuple(td.shape), depth_feat=td, out_rgb=out_rgb, out_depth=out_dep,
                           out_levels=out_lv)
    with pytest.raises(native.VetoError, match="depth pooler is level 2"):
        call.run("veto_roi_pool", ctypes.byref(a))
    torch.cuda.synchronize()
    assert bool((out_rgb == -7).all()) and bool((out_dep == -7).all()) and bool((out_lv == -7).all())
    _line("two scales + depth refused", out_rgb.numel() + out_dep.numel() + out_lv.numel(), 0)


# ---- section 3: level boundaries --------------------------------------------------------------------------------------------------
def test_level_boundaries_in_single_float32_steps():
    """Level l is the constant l + 1, so the pooled output names the level the kernel read: it must be the float32 LevelMapper's.
    (The four float32 weights of a sample need not sum to exactly 1, so a pooled constant may sit an ulp or two beside l + 1:
    the output is held to the oracle's pooling bit for bit, and to l + 1 within 4 ulp.)"""
    boxes = rc.boundary_boxes()
    want_lv = ro.map_levels(boxes)
    p = _pooler(rc.SCALES4)
    rgb = p([_t(m) for m in rc.boundary_maps()], _props([boxes], (464, 464)))
    got_lv = p.last_levels.cpu().numpy()
    rgb = rgb.cpu().numpy()
    wrong = np.nonzero(got_lv != want_lv)[0]
    _line("level boundaries 112 / 224 / 448", len(boxes), len(wrong), "float64 levels differ on %d" % (rc.map_levels_f64(boxes) != want_lv).sum())
    assert len(wrong) == 0, [(int(i), boxes[i].tolist(), int(got_lv[i]), int(want_lv[i])) for i in wrong[:8]]
    named = (want_lv + 1).astype(F)[:, None, None, None]
    off = np.abs(rgb - named) / np.spacing(named)
    _line("level boundaries: output names level", rgb.size, int((off > 4).sum()), "largest distance %.0f ulp" % off.max())
    assert (off <= 4).all()
    _same_bits(rgb, ro.pooler_forward(rc.boundary_maps(), [boxes])[0], "level boundaries: pooled constant")


# ---- section 4: samples exactly on the validity edge ----------------------------------------------------------------------------------
def test_exact_edge_samples():
    for name, feat, rois in (("edge 6 x 5", rc.edge_map(), rc.edge_rois()), ("hand 4 x 4", rc.hand_map(), rc.HAND_ROIS),
                             ("hand 4 x 4 + 1", rc.hand_map() + F(1), rc.HAND_ROIS)):
        got = _roi_align(_t(feat), _t(rois), 1.0, 2, 1)
        _same_bits(got, ro.roi_align(feat, rois, 1.0, 2, 1), "exact edges: " + name)
    got = _roi_align(_t(rc.edge_map()), _t(rc.edge_rois()), 1.0, 2, 1).cpu().numpy().reshape(6, 4)
    assert got[0].tolist() == [1.0, 2.0, 6.0, 7.0] and got[1].tolist() == [30.0, 0.0, 0.0, 0.0]
    assert np.array_equal(got[2], np.array([0, 1.9999998, 0, 6.9999995], dtype=F)) and not got[4:].any()


# ---- section 5: masked samples do not leak ----------------------------------------------------------------------------------------
def test_invalid_samples_do_not_leak_what_lies_at_pixel_0():
    feat, poisoned, rois = rc.leak_case()
    clean = _roi_align(_t(feat), _t(rois), rc.SCALE, 8, 2).cpu().numpy()
    got = _roi_align(_t(poisoned), _t(rois), rc.SCALE, 8, 2).cpu().numpy()
    bad = int((got.view(np.int32) != clean.view(np.int32)).sum())
    _line("poisoned map (NaN at 0, Inf untouched)", clean.size, bad, "non-finite outputs %d" % int((~np.isfinite(got)).sum()))
    assert bad == 0
    _same_bits(clean, ro.roi_align(feat, rois, rc.SCALE, 8, 2), "poisoned map: clean run")


def test_an_roi_outside_the_map_with_nan_gradients_adds_nothing():
    shape, rois, gout, k = rc.leak_backward_case()
    keep = np.arange(len(rois)) != k
    ref = ro.roi_align_backward(gout[keep], rois[keep], rc.SCALE, shape, 8, 2, stats=True)
    feat = torch.zeros(shape, device=_dev(), requires_grad=True)
    out = _roi_align(feat, _t(rois), rc.SCALE, 8, 2)
    out.backward(_t(gout))
    assert bool(torch.isfinite(feat.grad).all())
    _check_grad(feat.grad, ref, "backward, NaN cotangent of an outside ROI")


# ---- section 6: backward, per pixel, every instance ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single_backward_ref(pooled, ratio):
    feat, rois = rc.single(pooled, ratio, 33)
    gout = rc.cotangent((len(rois), 33, pooled, pooled), 100 + pooled * 10 + ratio)
    return feat, rois, gout, ro.roi_align_backward(gout, rois, rc.SCALE, feat.shape, pooled, ratio, stats=True)


@pytest.mark.parametrize("pooled,ratio", rc.BACKWARD_INSTANCES)
def test_backward_every_instance_per_pixel(pooled, ratio):
    feat, rois, gout, ref = _single_backward_ref(pooled, ratio)
    tf = _t(feat).requires_grad_(True)
    out = _roi_align(tf, _t(rois), rc.SCALE, pooled, ratio)
    out.backward(_t(gout))
    _check_grad(tf.grad, ref, "backward (%d, %d) C 33" % (pooled, ratio))
    # the adjoint identity <pool(f), g> = <f, pool_backward(g)> on the device
    lhs = float((out.detach().double() * _t(gout).double()).sum())
    rhs = float((tf.detach().double() * tf.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)


@functools.lru_cache(maxsize=None)
def _pyramid_backward_ref(depth_channels):
    feats, depth, boxes = rc.pyramid(channels=40, depth_channels=depth_channels)
    n = sum(len(b) for b in boxes)
    g_rgb, g_dep = rc.cotangent((n, 40, 8, 8), 31), rc.cotangent((n, depth_channels, 8, 8), 32)
    per_level, dep = rc.pyramid_backward(g_rgb, g_dep, boxes, [f.shape for f in feats], rc.SCALES4, depth.shape)
    return feats, depth, boxes, g_rgb, g_dep, per_level, dep


@pytest.mark.parametrize("depth_channels", [8, 72])
def test_backward_four_levels_and_depth_unequal_channels(depth_channels):
    feats, depth, boxes, g_rgb, g_dep, per_level, dep_ref = _pyramid_backward_ref(depth_channels)
    tf = [_t(f).requires_grad_(True) for f in feats]
    td = _t(depth).requires_grad_(True)
    rgb, dep = _pooler(rc.SCALES4)(tf, _props(boxes, (rc.PYR_W, rc.PYR_H)), depth_features=td)
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for l in range(4):
        _check_grad(tf[l].grad, per_level[l], "backward pyramid C 40 / depth %d, level %d" % (depth_channels, l))
    _check_grad(td.grad, dep_ref, "backward pyramid C 40 / depth %d, depth map" % depth_channels)
    lhs = float((rgb.detach().double() * _t(g_rgb).double()).sum() + (dep.detach().double() * _t(g_dep).double()).sum())
    rhs = float(sum((t.detach().double() * t.grad.double()).sum() for t in tf + [td]))
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)


def test_backward_contention_thousands_of_adds_per_pixel():
    shape, rois, gout = rc.contention_case()
    ref = ro.roi_align_backward(gout, rois, rc.SCALE, shape, 8, 2, stats=True)
    assert ref[1].max() == 16384 and (ref[1] > 0).sum() == 9
    feat = torch.zeros(shape, device=_dev(), requires_grad=True)
    _roi_align(feat, _t(rois), rc.SCALE, 8, 2).backward(_t(gout))
    _check_grad(feat.grad, ref, "backward contention, 64 x one sub-pixel ROI")


def test_backward_exact_contention_a_single_lost_update_shows():
    """64 copies of an ROI whose terms are multiples of 2^-12 with absolute sums below 2^12: the float32 accumulation is exact in any
    order (tests/test_roi_pool_cases_host.py), so the 16 384 atomic adds into each of the four pixels must give the oracle EXACTLY."""
    shape, rois, gout = rc.exact_contention_case()
    want, K, A = ro.roi_align_backward(gout, rois, rc.SCALE, shape, 8, 2, stats=True)
    assert (K > 0).sum() == 4 and K.max() == K[K > 0].min() == 16384 and A.max() < 2.0 ** 12
    feat = torch.zeros(shape, device=_dev(), requires_grad=True)
    _roi_align(feat, _t(rois), rc.SCALE, 8, 2).backward(_t(gout))
    got = feat.grad.cpu().numpy()
    bad = int((got.astype(np.float64) != want).sum())
    _line("backward exact contention, 4 pixels", want.size, bad, "K 16384 on each  largest |sum| %.0f" % np.abs(want).max())
    assert bad == 0


def test_backward_level_boundaries_in_single_float32_steps():
    """The backward kernel chooses the level with code of its own: the 579 boundary boxes through it, a gradient on each level map.
    The boxes of a sweep share their footprint, so a box routed to the neighbouring level moves about 1 / 193 of a pixel's
    gradient, hundreds of bounds, and puts gradient where the oracle's K is 0."""
    boxes = rc.boundary_boxes()
    maps = rc.boundary_maps()
    g_rgb = rc.cotangent((len(boxes), 2, 2, 2), 51)      # pooled 2: the level choice does not depend on it, the oracle's time does
    per_level, _ = rc.pyramid_backward(g_rgb, None, [boxes], [m.shape for m in maps], rc.SCALES4, None, pooled=2, ratio=2)
    tf = [_t(m).requires_grad_(True) for m in maps]
    rgb = _pooler(rc.SCALES4, pooled=2, ratio=2)(tf, _props([boxes], (464, 464)))
    (rgb * _t(g_rgb)).sum().backward()
    for l in range(4):
        _check_grad(tf[l].grad, per_level[l], "backward level boundaries, level %d" % l)


def test_gradient_routing_only_some_maps_require_grad():
    feats, depth, boxes, g_rgb, g_dep, per_level, dep_ref = _pyramid_backward_ref(8)
    props = _props(boxes, (rc.PYR_W, rc.PYR_H))
    # only the depth map
    tf, td = [_t(f) for f in feats], _t(depth).requires_grad_(True)
    rgb, dep = _pooler(rc.SCALES4)(tf, props, depth_features=td)
    (dep * _t(g_dep)).sum().backward()
    assert all(t.grad is None for t in tf)
    _check_grad(td.grad, dep_ref, "routing: only the depth map requires grad")
    # only level 1
    tf, td = [_t(f) for f in feats], _t(depth)
    tf[1].requires_grad_(True)
    rgb, dep = _pooler(rc.SCALES4)(tf, props, depth_features=td)
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    assert td.grad is None and all(tf[l].grad is None for l in (0, 2, 3))
    _check_grad(tf[1].grad, per_level[1], "routing: only level 1 requires grad")


# ---- section 7: host input forms ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forms_ref():
    feats, depth, boxes, g_rgb, g_dep, per_level, dep_ref = _pyramid_backward_ref(8)
    want_rgb, want_dep = ro.pooler_forward(feats, boxes, depth)
    return feats, depth, ro.to_rois(boxes), g_rgb, g_dep, per_level, dep_ref, want_rgb, want_dep


def _pool_direct(maps, depth, rois):
    from veto_amd.poolers import _roi_pool_autograd
    return _roi_pool_autograd(maps, rc.SCALES4, rois, 2, 8, 2, depth=depth, want_levels=True)


@pytest.mark.parametrize("form", ["channels_last", "strided_view", "float16", "rois_float64"])
def test_host_input_forms(form):
    feats, depth, rois, g_rgb, g_dep, per_level, dep_ref, want_rgb, want_dep = _forms_ref()
    trois, extra_tol = _t(rois), None
    if form == "float16":      # the maps rounded to half; the reference is the oracle on the upcast values
        feats, depth = [f.astype(np.float16) for f in feats], depth.astype(np.float16)
        boxes = [rois[rois[:, 0] == i, 1:] for i in range(2)]
        want_rgb, want_dep = ro.pooler_forward([f.astype(F) for f in feats], boxes, depth.astype(F))
        # the float32 gradient is rounded to the leaf's float16: half an ulp (2^-11 relative), half the subnormal spacing below
        extra_tol = lambda want: 2.0 ** -11 * np.abs(want) + 2.0 ** -25  # noqa: E731
    leaves = [_t(m) for m in feats + [depth]]
    if form == "channels_last":
        leaves = [m.to(memory_format=torch.channels_last) for m in leaves]
        assert not leaves[0].is_contiguous()
    if form == "strided_view":      # every second image of a batch twice as large; the images between are NaN and must not be read
        big = []
        for m in leaves:
            b = torch.full((2 * m.shape[0],) + tuple(m.shape[1:]), float("nan"), device=_dev())
            b[::2] = m
            big.append(b)
        leaves = big
    if form == "rois_float64":
        trois = trois.double()
    for m in leaves:
        m.requires_grad_(True)
    maps = [m[::2] for m in leaves] if form == "strided_view" else leaves
    rgb, dep, lv = _pool_direct(maps[:4], maps[4], trois)
    # the contiguous float32 call on the same values
    ref_rgb, ref_dep, ref_lv = _pool_direct([m.detach().float().contiguous() for m in maps[:4]], maps[4].detach().float().contiguous(),
                                            trois.float())
    assert torch.equal(rgb.view(torch.int32), ref_rgb.view(torch.int32)) and torch.equal(dep.view(torch.int32), ref_dep.view(torch.int32))
    assert torch.equal(lv, ref_lv)
    _same_bits(rgb, want_rgb, "form %s rgb" % form)
    _same_bits(dep, want_dep, "form %s depth" % form)
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for i, (m, ref) in enumerate(zip(leaves, per_level + [dep_ref])):
        assert m.grad is not None and m.grad.shape == m.shape and m.grad.dtype == m.dtype, (form, i)
        g = m.grad
        if form == "strided_view":
            assert not bool(g[1::2].any()), (form, i)
            g = g[::2]
        _check_grad(g, ref, "form %s grad %s" % (form, "depth" if i == 4 else "level %d" % i), extra_tol)


def test_batch_with_empty_images_in_the_middle():
    feats, depth, boxes = rc.empty_image_case()
    n = sum(len(b) for b in boxes)
    want_rgb, want_dep, want_lv = ro.pooler_forward(feats, [np.asarray(b).reshape(-1, 4) for b in boxes], depth, return_levels=True)
    g_rgb, g_dep = rc.cotangent((n, 40, 8, 8), 41), rc.cotangent((n, 8, 8, 8), 42)
    per_level, dep_ref = rc.pyramid_backward(g_rgb, g_dep, boxes, [f.shape for f in feats], rc.SCALES4, depth.shape)
    tf = [_t(f).requires_grad_(True) for f in feats]
    td = _t(depth).requires_grad_(True)
    p = _pooler(rc.SCALES4)
    rgb, dep = p(tf, _props(boxes, (512, 320)), depth_features=td)
    assert np.array_equal(p.last_levels.cpu().numpy(), want_lv)
    _same_bits(rgb, want_rgb, "images with (3, 0, 7, 0, 2) boxes rgb")
    _same_bits(dep, want_dep, "images with (3, 0, 7, 0, 2) boxes depth")
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for l in range(4):
        _check_grad(tf[l].grad, per_level[l], "images with (3, 0, 7, 0, 2) boxes grad level %d" % l)
    _check_grad(td.grad, dep_ref, "images with (3, 0, 7, 0, 2) boxes grad depth")
    # no ROI maps to level 3: a zero gradient of the map's shape; the images without boxes get none either
    assert (want_lv != 3).all() and tf[3].grad.shape == tf[3].shape and not bool(tf[3].grad.any())
    assert not bool(tf[0].grad[[1, 3]].any()) and not bool(td.grad[[1, 3]].any())
