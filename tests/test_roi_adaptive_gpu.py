"""ROI pooling on the adaptive grid (sampling_ratio = 0, veto_roi_pool_adaptive / veto_roi_pool_adaptive_backward) on the device.

Forward: bit for bit against the reference's compiled kernel (tests/golden/roialign_single.npz::out_p6_r0) and against
oracle/roi_align_oracle.py on the cases of tests/roi_adaptive_cases.py, whose premises tests/test_roi_adaptive_host.py asserts.
Backward: per pixel |device - float64 sum| <= K u / (1 - K u) * sum |term| with K and the sum from the tap-list restatement, exactly
0 where nothing contributes, and one contention case compared exactly.  Every launch through the C ABI runs twice, into outputs
filled with a sentinel and fenced by guard cells: the two runs agree bit for bit (forward), every element is written, no guard is."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import roi_adaptive_cases as ac
import roi_pool16_cases as c16
import roi_pool_cases as rc
import test_roi_pool_gpu as trp
from oracle import roi_align_oracle as ro

pytestmark = pytest.mark.gpu
F = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roialign_single.npz")
_dev = trp._dev


def _t(a):
    return trp._t(np.array(a))      # (a copy: the shared references are read-only)


SENTINEL = 0x7FC0DEAD      # a NaN no arithmetic produces
GUARD = 64
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


class _Fenced(object):
    """A tensor of `shape` inside a sentinel-filled buffer with GUARD cells on either side"""

    def __init__(self, shape, dtype=torch.float32, zero=False):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=_dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)
        if zero:
            self.t.zero_()

    def check(self, what, all_written=True):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), what + ": a guard cell was written"
        if all_written:
            assert bool((self.buf[GUARD:GUARD + self.n] != SENTINEL).all()), what + ": an element was not written"

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _args(call, maps, scales, rois, n_img, pooled, ratio, depth, rgb, dep, lv, **kw):
    from veto_amd import native, poolers
    codes = poolers._DTYPE_CODES
    return poolers._pool_args(call, maps, scales, rois, n_img, pooled, ratio, tuple(depth.shape) if depth is not None else None,
                              depth_feat=depth, out_rgb=rgb.t, out_depth=dep.t if dep is not None else None,
                              out_levels=lv.t if lv is not None else None, level_dtype=codes[maps[0].dtype],
                              depth_dtype=codes[depth.dtype] if depth is not None else native.VETO_ROI_F32, **kw)


def _forward(maps, scales, rois, pooled, depth=None, what="forward"):
    """veto_roi_pool_adaptive twice into fenced outputs: (rgb, depth or None, levels) of the first run as numpy"""
    from veto_amd import native
    n_img, n_roi = maps[0].shape[0], rois.shape[0]
    runs = []
    for _ in range(2):
        call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
        rgb = _Fenced((n_roi, maps[0].shape[1], pooled, pooled))
        dep = _Fenced((n_roi, depth.shape[1], pooled, pooled)) if depth is not None else None
        lv = _Fenced((n_roi,), torch.int32)
        a = _args(call, maps, scales, rois, n_img, pooled, 0, depth, rgb, dep, lv)
        call.run("veto_roi_pool_adaptive", ctypes.byref(a))
        torch.cuda.synchronize()
        for f, name in ((rgb, "rgb"), (dep, "depth"), (lv, "levels")):
            if f is not None:
                f.check("%s %s" % (what, name))
        runs.append((rgb, dep, lv))
    for x, y in zip(*runs):
        if x is not None:
            assert torch.equal(x.buf, y.buf), what + ": two launches of one call differ"
    rgb, dep, lv = runs[0]
    return rgb.t.cpu().numpy(), dep.t.cpu().numpy() if dep is not None else None, lv.t.cpu().numpy()


def _backward(shapes, scales, rois, pooled, g_rgb, depth_shape=None, g_dep=None, what="backward"):
    """veto_roi_pool_adaptive_backward twice into fenced, zeroed gradient maps: ([per level], depth) of each run as numpy"""
    from veto_amd import native, poolers
    out = []
    for _ in range(2):
        call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
        a = poolers._pool_args(call, shapes, scales, rois, shapes[0][0], pooled, 0, depth_shape)
        grads = [_Fenced(s, zero=True) for s in shapes]
        dgrad = _Fenced(depth_shape, zero=True) if depth_shape is not None else None
        ptrs = (ctypes.c_void_p * 4)(*[g.t.data_ptr() for g in grads])
        call.run("veto_roi_pool_adaptive_backward", ctypes.byref(a), call.ptr(g_rgb), call.ptr(g_dep), ptrs,
                 dgrad.t.data_ptr() if dgrad is not None else None)
        torch.cuda.synchronize()
        for g in grads + ([dgrad] if dgrad is not None else []):
            g.check(what)
        out.append(([g.t.cpu().numpy() for g in grads], dgrad.t.cpu().numpy() if dgrad is not None else None))
    return out


def _check_grad(got, ref, case):
    """per pixel: |got - want| <= K u / (1 - K u) * sum |term|; exactly 0 where K = 0"""
    want, K, A = ref
    got = np.asarray(got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), case
    zero = np.broadcast_to((K == 0)[:, None], want.shape)
    assert not got[zero].any(), case + ": a pixel nothing contributes to is not 0"
    err, bound = np.abs(got - want), ac.adaptive_bound(K, A)
    worst = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    trp._line(case, want.size, int((err > bound).sum()), "K max %d  zero pixels %d  error / bound %.3f" % (K.max(), int((K == 0).sum()) * want.shape[1], worst))
    assert (err <= bound).all(), (case, worst)


# ---- 1: the reference's compiled kernel ---------------------------------------------------------------------------------------------------
def test_forward_equals_the_reference_kernel_fixture_p6_r0():
    from veto_amd import synth
    want = np.load(FIXTURE)["out_p6_r0"]
    feat, rois = synth.synthetic_roi_single(6, 0, channels=want.shape[1])
    got, _, lv = _forward([_t(feat)], [rc.SCALE], _t(rois), 6, what="reference kernel (6, 0)")
    trp._same_bits(got, want, "reference kernel (6, 0)")
    assert not lv.any()


# ---- 2: every case against the oracle, bit for bit ------------------------------------------------------------------------------------------
SINGLE = [(p, d, 65) for d in DTYPES for p in ac.POOLED] + [(p, "float32", c) for p in (7, 16) for c in (1, 33)]


@pytest.mark.parametrize("pooled,dtype,channels", SINGLE)
def test_forward_single_map_cases_bit_exact(pooled, dtype, channels):
    feat, rois, want = ac.single_reference(pooled)
    m = _t(feat[:, :channels]).to(DTYPES[dtype])
    got, _, _ = _forward([m], [ac.SCALE], _t(rois), pooled, what="adaptive P %d %s C %d" % (pooled, dtype, channels))
    trp._same_bits(got, np.ascontiguousarray(want[:, :channels]), "adaptive P %d %s C %d" % (pooled, dtype, channels))


FORMS = [("float32", "float32"), ("float16", "float16"), ("bfloat16", "bfloat16"), ("float32", "bfloat16")]      # (levels, depth map)


@pytest.mark.parametrize("forms", FORMS, ids=["-".join(f) for f in FORMS])
@pytest.mark.parametrize("pooled", ac.POOLED)
def test_forward_four_levels_and_depth_bit_exact(pooled, forms):
    feats, depth, boxes, want_rgb, want_dep, want_lv = ac.pyramid_reference(pooled)
    maps = [_t(f).to(DTYPES[forms[0]]) for f in feats]
    case = "adaptive pyramid P %d %s / %s" % (pooled, forms[0], forms[1])
    rgb, dep, lv = _forward(maps, rc.SCALES4, _t(ro.to_rois(boxes)), pooled, depth=_t(depth).to(DTYPES[forms[1]]), what=case)
    assert np.array_equal(lv, want_lv), case
    trp._same_bits(rgb, want_rgb, case + " rgb")
    trp._same_bits(dep, want_dep, case + " depth")


def test_forward_where_float64_picks_another_grid():
    rois, g32, g64 = ac.grid_rounding_rois()
    feat = ac.feature_map(33, seed=6, shape=(1,) + ac.QUARTER_HW)
    got, _, _ = _forward([_t(feat)], [ac.QUARTER], _t(rois), 7, what="float32 grid")
    trp._same_bits(got, ro.roi_align(feat, rois, ac.QUARTER, 7, 0), "adaptive: float32 grid where float64 differs")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_forward_at_a_scale_that_is_no_power_of_two(dtype):
    """Scale 0.3: hi*scale and lo*scale round in float32, and float64 picks another grid each way on these boxes.  A kernel that
    computed (hi - lo) * scale, or contracted hi*scale - lo*scale into a fused multiply-add, differs here and nowhere else."""
    rois, g32, g64 = ac.odd_scale_rois()
    feat = ac.feature_map(33, seed=8, shape=(1,) + ac.ODD_HW)
    got, _, _ = _forward([_t(feat).to(DTYPES[dtype])], [ac.ODD_SCALE], _t(rois), 7, what="scale 0.3 " + dtype)
    trp._same_bits(got, ro.roi_align(feat, rois, ac.ODD_SCALE, 7, 0), "adaptive: scale 0.3, float64 differs each way, " + dtype)


def test_backward_at_a_scale_that_is_no_power_of_two():
    rois, _, _ = ac.odd_scale_rois()
    shape = (1, 33) + ac.ODD_HW
    gout = rc.cotangent((len(rois), 33, 7, 7), 63)
    ref = ac.taps_backward(ac.np_adaptive_taps(rois, ac.ODD_SCALE, shape, 7), gout)
    for i, (grads, _) in enumerate(_backward([shape], [ac.ODD_SCALE], _t(rois), 7, _t(gout))):
        _check_grad(grads[0], ref, "adaptive backward at scale 0.3, run %d" % i)


# ---- 3: where every grid is (g, g) the output is that of the fixed ratio g --------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_forward_equals_the_fixed_ratio_where_every_grid_is_gxg(g):
    rois = ac.square_grid_rois(g)
    t = ac.np_adaptive_taps(rois, ac.SCALE, (2, 1, ac.H, ac.W), 7)
    assert (t.grid == g).all()
    feat = _t(ac.feature_map(33))
    got, _, _ = _forward([feat], [ac.SCALE], _t(rois), 7, what="grid (%d, %d)" % (g, g))
    fixed = trp._roi_align(feat, _t(rois), ac.SCALE, 7, g)
    trp._same_bits(got, fixed.cpu().numpy(), "adaptive == veto_roi_pool at ratio %d" % g)


# ---- 4: backward --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single_backward_ref(pooled, channels=33):
    rois = ac.single_rois()
    shape = (2, channels, ac.H, ac.W)
    gout = rc.cotangent((len(rois), channels, pooled, pooled), 300 + pooled)
    return shape, rois, gout, ac.taps_backward(ac.np_adaptive_taps(rois, ac.SCALE, shape, pooled), gout)


@pytest.mark.parametrize("pooled", [1, 7, 14])
def test_backward_single_map_per_pixel(pooled):
    shape, rois, gout, ref = _single_backward_ref(pooled)
    for i, (grads, _) in enumerate(_backward([shape], [ac.SCALE], _t(rois), pooled, _t(gout))):
        _check_grad(grads[0], ref, "adaptive backward P %d C 33, run %d" % (pooled, i))


def test_backward_four_levels_and_depth_per_pixel():
    pooled, C, Cd = 7, 33, 65
    boxes = c16.boxes()
    n = sum(len(b) for b in boxes)
    shapes = [(2, C, c16.H >> (2 + l), c16.W >> (2 + l)) for l in range(4)]
    dshape = (2, Cd, c16.H >> 4, c16.W >> 4)
    g_rgb, g_dep = rc.cotangent((n, C, pooled, pooled), 61), rc.cotangent((n, Cd, pooled, pooled), 62)
    per_level, dep_ref = ac.pyramid_taps_backward(g_rgb, g_dep, boxes, shapes, dshape, pooled)
    for i, (grads, dgrad) in enumerate(_backward(shapes, rc.SCALES4, _t(ro.to_rois(boxes)), pooled, _t(g_rgb), dshape, _t(g_dep))):
        for l in range(4):
            _check_grad(grads[l], per_level[l], "adaptive backward pyramid level %d, run %d" % (l, i))
        _check_grad(dgrad, dep_ref, "adaptive backward pyramid depth map, run %d" % i)


def test_backward_exact_contention_a_single_lost_update_shows():
    """64 copies of a ROI with a (4, 2) grid whose terms are multiples of 2^-5 with absolute sums below 2^12: the float32 accumulation
    is exact in any order (tests/test_roi_adaptive_host.py), so the device must give the float64 sums EXACTLY at every pixel."""
    shape, rois, gout = ac.exact_contention_case()
    want, K, A = ac.taps_backward(ac.np_adaptive_taps(rois, ac.SCALE, shape, 8), gout)
    assert K.max() == 256 and A.max() < 2.0 ** 12
    for i, (grads, _) in enumerate(_backward([shape], [ac.SCALE], _t(rois), 8, _t(gout))):
        bad = int((grads[0].astype(np.float64) != want).sum())
        trp._line("adaptive backward exact contention, run %d" % i, want.size, bad, "K max %d" % K.max())
        assert bad == 0


# ---- 5: through torch ---------------------------------------------------------------------------------------------------------------------
def test_roi_align_module_forward_and_autograd():
    from veto_amd.poolers import ROIAlign
    feat, rois, want = ac.single_reference(7)
    shape, _, gout, ref = _single_backward_ref(7)
    tf = _t(feat[:, :33]).requires_grad_(True)
    out = ROIAlign((7, 7), ac.SCALE, 0)(tf, _t(rois))
    trp._same_bits(out, np.ascontiguousarray(want[:, :33]), "ROIAlign((7, 7), s, 0)")
    out.backward(_t(gout))
    _check_grad(tf.grad, ref, "ROIAlign((7, 7), s, 0) autograd")
    with pytest.raises(NotImplementedError, match="square"):
        ROIAlign((7, 5), ac.SCALE, 0)


def _pyramid_torch_case():
    feats, depth, boxes, want_rgb, want_dep, want_lv = ac.pyramid_reference(7)
    n = sum(len(b) for b in boxes)
    g_rgb, g_dep = rc.cotangent((n, 33, 7, 7), 61), rc.cotangent((n, 65, 7, 7), 62)
    refs = ac.pyramid_taps_backward(g_rgb, g_dep, boxes, [f.shape for f in feats], depth.shape, 7)
    return feats, depth, boxes, want_rgb, want_dep, want_lv, g_rgb, g_dep, refs


def test_pooler_and_feature_extractor_with_ratio_0():
    from veto_amd import poolers, testing
    feats, depth, boxes, want_rgb, want_dep, want_lv, g_rgb, g_dep, (per_level, dep_ref) = _pyramid_torch_case()
    props = trp._props(boxes, (c16.W, c16.H))
    tf = [_t(f).requires_grad_(True) for f in feats]
    td = _t(depth).requires_grad_(True)
    p = trp._pooler(rc.SCALES4, 7, 0)
    rgb, dep = p(tf, props, depth_features=td)
    assert np.array_equal(p.last_levels.cpu().numpy(), want_lv)
    trp._same_bits(rgb, want_rgb, "Pooler ratio 0 rgb")
    trp._same_bits(dep, want_dep, "Pooler ratio 0 depth")
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for l in range(4):
        _check_grad(tf[l].grad, per_level[l], "Pooler ratio 0 grad level %d" % l)
    _check_grad(td.grad, dep_ref, "Pooler ratio 0 grad depth")
    cfg = testing.make_config(2, 8, resolution=7)
    cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO = 0
    ext = poolers.make_roi_box_feature_extractor(cfg, 256, for_relation=True)
    assert ext.pooler.sampling_ratio == 0 and ext.pooler.output_size == (7, 7)
    x_2d, d_2d, _, _ = ext([_t(f) for f in feats], props, depth_features=_t(depth))
    trp._same_bits(x_2d, want_rgb, "feature extractor ratio 0 rgb")
    trp._same_bits(d_2d, want_dep, "feature extractor ratio 0 depth")


def test_images_with_no_roi():
    feats, depth, boxes, want_rgb, want_dep, want_lv = ac.empty_image_reference()
    p = trp._pooler(rc.SCALES4, 7, 0)
    rgb, dep = p([_t(f) for f in feats], trp._props(boxes, (c16.W, c16.H)), depth_features=_t(depth))
    assert np.array_equal(p.last_levels.cpu().numpy(), want_lv)
    trp._same_bits(rgb, want_rgb, "adaptive, images with (3, 0, 7, 0, 2) boxes rgb")
    trp._same_bits(dep, want_dep, "adaptive, images with (3, 0, 7, 0, 2) boxes depth")


def test_channels_last_bfloat16_leaf_gets_its_gradient_in_that_form():
    """channels_last maps take the float32 NCHW copy (the same bits); the gradient comes back in the leaf's dtype and memory format,
    rounded once more to bfloat16 (8 significant bits: unit roundoff 2^-8) on top of the bound."""
    feat, rois, want = ac.single_reference(7)
    shape, _, gout, (gw, K, A) = _single_backward_ref(7)
    leaf = _t(feat[:, :33]).to(torch.bfloat16).to(memory_format=torch.channels_last).requires_grad_(True)
    assert not leaf.is_contiguous()
    from veto_amd.poolers import ROIAlign
    out = ROIAlign((7, 7), ac.SCALE, 0)(leaf, _t(rois))
    trp._same_bits(out, np.ascontiguousarray(want[:, :33]), "adaptive, channels_last bfloat16 leaf")
    out.backward(_t(gout))
    g = leaf.grad
    assert g.dtype == torch.bfloat16 and g.shape == leaf.shape and g.is_contiguous(memory_format=torch.channels_last) and not g.is_contiguous()
    got = g.float().cpu().numpy().astype(np.float64)
    bound = ac.adaptive_bound(K, A)
    assert (np.abs(got - gw) <= bound + 2.0 ** -8 * (np.abs(gw) + bound)).all()
    assert not got[np.broadcast_to((K == 0)[:, None], gw.shape)].any()


def test_after_install_pooler_ops_the_reference_names_pool_with_ratio_0(monkeypatch):
    from test_roi_layouts_host import BASE, _fake_pysgg, _originals
    from veto_amd import registry
    mods = _fake_pysgg(monkeypatch, BASE)
    _originals(mods)
    registry.install_pooler_ops()
    feat, rois, want = ac.single_reference(7)
    out = mods["pysgg.layers"].ROIAlign((7, 7), ac.SCALE, 0)(_t(feat[:, :33]), _t(rois))
    trp._same_bits(out, np.ascontiguousarray(want[:, :33]), "installed ROIAlign ratio 0")
    feats, depth, boxes, want_rgb, want_dep, want_lv = ac.pyramid_reference(7)
    pooler = mods["pysgg.modeling.poolers"].Pooler((7, 7), rc.SCALES4, 0)
    rgb = pooler([_t(f) for f in feats], trp._props(boxes, (c16.W, c16.H)))
    trp._same_bits(rgb, want_rgb, "installed Pooler ratio 0 (the box head's 7 x 7)")


# ---- 6: refusals, with nothing written behind them ----------------------------------------------------------------------------------------
REFUSALS = [("ratio 2", dict(ratio=2), "sampling_ratio must be 0"), ("NHWC levels", dict(level_layout=1), "NHWC"),
            ("NHWC depth", dict(depth_layout=1), "NHWC"), ("pooled 17", dict(pooled=17), "pooled must be 1..16"),
            ("null rois", dict(null_rois=True), "rois")]


@pytest.mark.parametrize("name,how,message", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_write_nothing(name, how, message):
    from veto_amd import native
    pooled, ratio = how.get("pooled", 7), how.get("ratio", 0)
    feats, depth = c16.pyramid(1, 1)
    maps, td = [_t(m) for m in feats], _t(depth)
    rois = _t(ro.to_rois(c16.boxes()))
    n = len(rois)
    rgb, dep, lv = _Fenced((n, 1, pooled, pooled)), _Fenced((n, 1, pooled, pooled)), _Fenced((n,), torch.int32)
    call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
    layouts = {k: v for k, v in how.items() if k.endswith("_layout")}
    a = _args(call, maps, rc.SCALES4, rois, 2, pooled, ratio, td, rgb, dep, lv, **layouts)
    if how.get("null_rois"):
        a.rois = None
    with pytest.raises(native.VetoError, match=message):
        call.run("veto_roi_pool_adaptive", ctypes.byref(a))
    grads = [_Fenced(m.shape) for m in maps]
    dgrad = _Fenced(td.shape)
    ptrs = (ctypes.c_void_p * 4)(*[g.t.data_ptr() for g in grads])
    gout = torch.ones((n, 1, pooled, pooled), device=_dev())
    with pytest.raises(native.VetoError, match=message):
        call.run("veto_roi_pool_adaptive_backward", ctypes.byref(a), call.ptr(gout), call.ptr(gout), ptrs, dgrad.t.data_ptr())
    torch.cuda.synchronize()
    assert all(f.untouched() for f in [rgb, dep, lv, dgrad] + grads), name


def test_the_fixed_ratio_entry_points_keep_refusing_ratio_0():
    from veto_amd import native, poolers
    feat, rois, _ = ac.single_reference(7)
    m, r = _t(feat[:, :1]), _t(rois)
    out = _Fenced((len(rois), 1, 7, 7))
    call = native.Launch(_dev(), "ROI pooling runs only on a HIP device")
    a = poolers._pool_args(call, [m], [ac.SCALE], r, 2, 7, 0, None, out_rgb=out.t)
    grad = _Fenced(m.shape)
    ptrs = (ctypes.c_void_p * 4)(grad.t.data_ptr())
    with pytest.raises(native.VetoError, match="adaptive sampling is not built"):
        call.run("veto_roi_pool", ctypes.byref(a))
    for entry in ("veto_roi_pool_backward", "veto_roi_pool_backward_ordered"):
        with pytest.raises(native.VetoError, match="adaptive sampling is not built"):
            call.run(entry, ctypes.byref(a), call.ptr(torch.ones((len(rois), 1, 7, 7), device=_dev())), None, ptrs, None)
    torch.cuda.synchronize()
    assert out.untouched() and grad.untouched()


def test_ordered_mode_refuses_the_adaptive_backward():
    """VETO_AMD.DETERMINISTIC reaches the pooler as `deterministic`; torch.use_deterministic_algorithms(True) switches the same mode on.
    Neither falls back to atomic adds: the backward raises and no gradient is written."""
    feat, rois, _ = ac.single_reference(7)
    p = trp._pooler([ac.SCALE], 7, 0)
    p.deterministic = True
    from veto_amd.structures import BoxList
    props = [BoxList(torch.from_numpy(rois[rois[:, 0] == i, 1:].copy()), (ac.W * 16, ac.H * 16)).to(_dev()) for i in range(2)]
    tf = _t(feat[:, :3]).requires_grad_(True)
    out = p([tf], props)
    with pytest.raises(NotImplementedError, match=r"(?s)sampling_ratio = 0.*VETO_AMD.DETERMINISTIC.*1-4"):
        out.sum().backward()
    assert tf.grad is None
    from veto_amd.poolers import ROIAlign
    tf2 = _t(feat[:, :3]).requires_grad_(True)
    out = ROIAlign((7, 7), ac.SCALE, 0)(tf2, _t(rois))
    torch.use_deterministic_algorithms(True)
    try:
        with pytest.raises(NotImplementedError, match="use_deterministic_algorithms"):
            out.sum().backward()
    finally:
        torch.use_deterministic_algorithms(False)
    assert tf2.grad is None


def test_ordered_mode_from_the_environment_refuses_the_adaptive_backward(monkeypatch):
    """VETO_DETERMINISTIC=1 is read once per process: the cached answer is reset for this test and restored after it."""
    from veto_amd import native
    from veto_amd.poolers import ROIAlign
    monkeypatch.setenv("VETO_DETERMINISTIC", "1")
    monkeypatch.setattr(native, "_ENV_DETERMINISTIC", None)
    feat, rois, _ = ac.single_reference(7)
    tf = _t(feat[:, :3]).requires_grad_(True)
    out = ROIAlign((7, 7), ac.SCALE, 0)(tf, _t(rois))
    with pytest.raises(NotImplementedError, match="VETO_DETERMINISTIC=1"):
        out.sum().backward()
    assert tf.grad is None
