"""ROI pooling on maps read in place: NCHW / NHWC, float32 / float16 / bfloat16 (include/veto_amd.h, "Map forms").

Through the C ABI with pointers into buffers of the form under test (no conversion anywhere), outputs filled with a sentinel and
followed by guard cells, every launch twice; then through veto_amd.poolers on torch leaves.  Forward and ordered backward: bit for
bit against the float32 NCHW call on the same values AND against the CPU oracle.  Atomic backward: the any-order bound of
tests/roi_pool_cases.py.  The inputs and why they can tell a wrong kernel from a right one: tests/roi_layout_cases.py and
tests/test_roi_layouts_host.py.  Each test prints "roi_layouts:" lines (pytest -s); profiles/roi_layouts.txt keeps them."""
import ctypes

import numpy as np
import pytest
import torch

import deterministic_cases as dc
import roi_layout_cases as lc
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL, GUARD = -7.0, 64
TORCH_DTYPES = {lc.F32: torch.float32, lc.F16: torch.float16, lc.BF16: torch.bfloat16}


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _say(line):
    print("roi_layouts: " + line, flush=True)


class DevMap:
    """A map on the device in one form: `t` is the flat buffer the kernel reads (it may start off a 16-byte boundary)."""

    def __init__(self, values, form, off=False):
        self.shape, self.form = tuple(values.shape), form
        raw = lc.pack(values, form).reshape(-1)
        raw = raw.view(np.int16) if raw.dtype == np.uint16 else raw
        n = raw.size
        if off:
            self.owner = torch.empty(n + 17, dtype=torch.from_numpy(raw[:1]).dtype, device=_dev())
            assert self.owner.data_ptr() % 16 == 0
            self.t = self.owner[1:1 + n]
            self.t.copy_(torch.from_numpy(raw))
            assert self.t.data_ptr() % 16 == lc.ITEMSIZE[form[0]]
        else:
            self.t = torch.from_numpy(raw).to(_dev())
            assert self.t.data_ptr() % 16 == 0


def _guarded(shape, fill, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=_dev())
    return buf, buf[:n].view(shape)


def _guard_ok(buf, n, fill):
    g = buf[n:]
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _args(native, levels, scales, rois, pooled, ratio, depth=None, struct_size=None, codes=None):
    """levels / depth: DevMap (forward) or (shape, layout) (backward).  codes: (level_dtype, depth_dtype, level_layout, depth_layout)
    to override what the maps say."""
    a = native.VetoRoiPoolArgs()
    a.struct_size = ctypes.sizeof(native.VetoRoiPoolArgs) if struct_size is None else struct_size
    shape0 = levels[0].shape if isinstance(levels[0], DevMap) else levels[0][0]
    a.n_levels, a.n_img, a.n_roi, a.channels, a.pooled, a.sampling_ratio = len(levels), shape0[0], rois.shape[0], shape0[1], pooled, ratio
    a.rois = rois.data_ptr()
    for l, (m, sc) in enumerate(zip(levels, scales)):
        shape, form = (m.shape, m.form) if isinstance(m, DevMap) else (m[0], (lc.F32, m[1]))
        a.level_h[l], a.level_w[l], a.level_scale[l] = shape[2], shape[3], float(sc)
        if isinstance(m, DevMap):
            a.level_feat[l] = m.t.data_ptr()
        a.level_dtype, a.level_layout = form
    if depth is not None:
        shape, form = (depth.shape, depth.form) if isinstance(depth, DevMap) else (depth[0], (lc.F32, depth[1]))
        a.depth_channels, a.depth_h, a.depth_w = shape[1], shape[2], shape[3]
        if isinstance(depth, DevMap):
            a.depth_feat = depth.t.data_ptr()
        a.depth_dtype, a.depth_layout = form
    if codes is not None:
        a.level_dtype, a.depth_dtype, a.level_layout, a.depth_layout = codes
    return a


def _forward(levels, scales, rois, pooled, ratio, depth=None, struct_size=None, codes=None, expect_error=None):
    """veto_roi_pool twice on sentinel-filled, guarded outputs: (rgb, depth or None, levels) as numpy."""
    from veto_amd import native
    trois = _t(rois)
    runs = []
    for _ in range(2):
        call = native.Launch(_dev(), "test")
        n = len(rois)
        rgb_buf, rgb = _guarded((n, levels[0].shape[1], pooled, pooled), SENTINEL)
        dep_buf, dep = _guarded((n, depth.shape[1], pooled, pooled), SENTINEL) if depth is not None else (None, None)
        lv_buf, lv = _guarded((n,), -7, torch.int32)
        a = _args(native, levels, scales, trois, pooled, ratio, depth, struct_size, codes)
        a.out_rgb, a.out_levels = rgb.data_ptr(), lv.data_ptr()
        if dep is not None:
            a.out_depth = dep.data_ptr()
        if expect_error is not None:
            with pytest.raises(native.VetoError, match=expect_error):
                call.run("veto_roi_pool", ctypes.byref(a))
            torch.cuda.synchronize()
            assert bool((rgb_buf == SENTINEL).all()) and bool((lv_buf == -7).all()) and (dep_buf is None or bool((dep_buf == SENTINEL).all()))
            return None
        call.run("veto_roi_pool", ctypes.byref(a))
        torch.cuda.synchronize()
        assert _guard_ok(rgb_buf, rgb.numel(), SENTINEL) and bool((lv_buf[n:] == -7).all()), "a write behind the outputs"
        assert dep is None or _guard_ok(dep_buf, dep.numel(), SENTINEL), "a write behind out_depth"
        runs.append((rgb.cpu().numpy(), dep.cpu().numpy() if dep is not None else None, lv.cpu().numpy()))
    for x, y in zip(*runs):
        assert x is None or np.array_equal(x.view(np.int32), y.view(np.int32)), "two launches of one call differ"
    return runs[0]


def _same_bits(got, want, what):
    want = np.asarray(want, dtype=F)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    bad = int((got.view(np.int32) != want.view(np.int32)).sum())
    _say("%-58s compared %8d  mismatches %d" % (what, want.size, bad))
    assert bad == 0, (what, bad)


def _f32(values):
    return DevMap(values, (lc.F32, lc.NCHW))


# ---- 1. forward: every form x every kernel instance ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled,ratio", lc.FORWARD_INSTANCES)
@pytest.mark.parametrize("form", lc.FORMS, ids=lc.form_id)
def test_forward_every_form_and_instance_bit_exact(form, pooled, ratio):
    q, rois, want = lc.single_forward(pooled, ratio, 40, form[0])
    got = _forward([DevMap(q, form)], (rc.SCALE,), rois, pooled, ratio)[0]
    ref = _forward([_f32(q)], (rc.SCALE,), rois, pooled, ratio)[0]
    what = "forward %s (%d, %d) C 40" % (lc.form_id(form), pooled, ratio)
    _same_bits(got, ref, what + " vs float32 NCHW call")
    _same_bits(got, want, what + " vs oracle")


# ---- 2. channel counts and alignment ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", lc.CHANNELS)
@pytest.mark.parametrize("form", lc.FORMS, ids=lc.form_id)
def test_forward_channel_counts_depth_widths_and_off_boundary_maps(form, channels):
    q, rois, want = lc.single_forward(8, 2, channels, form[0])
    depth_channels = 8 if channels >= 32 else 70      # narrower and wider than the pyramid
    dq, dwant = lc.depth_forward(depth_channels, form[0], channels)
    for off in (False, True):
        rgb, dep, _ = _forward([DevMap(q, form, off)], (rc.SCALE,), rois, 8, 2, depth=DevMap(dq, form, off))
        what = "forward %s C %d / depth %d%s" % (lc.form_id(form), channels, depth_channels, ", off a 16-byte boundary" if off else "")
        _same_bits(rgb, want, what + " rgb")
        _same_bits(dep, dwant, what + " depth")


# ---- 3. levels and leaks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels", [4, 3, 1])
def test_level_counts_nhwc_bf16_pyramid_with_an_nchw_f16_depth_map(n_levels):
    """The pyramid and the depth map in different forms: each gets the launch of its own form."""
    maps, scales, depth, rois, want_rgb, want_dep, want_lv = lc.pyramid_forward(n_levels, lc.BF16, lc.F16)
    rgb, dep, lv = _forward([DevMap(m, (lc.BF16, lc.NHWC)) for m in maps], scales, rois, 8, 2, depth=DevMap(depth, (lc.F16, lc.NCHW)))
    ref = _forward([_f32(m) for m in maps], scales, rois, 8, 2, depth=_f32(depth))
    assert np.array_equal(lv, want_lv) and np.array_equal(lv, ref[2])
    _same_bits(rgb, ref[0], "%d levels NHWC bf16 rgb vs float32 NCHW call" % n_levels)
    _same_bits(dep, ref[1], "%d levels NCHW f16 depth vs float32 NCHW call" % n_levels)
    _same_bits(rgb, want_rgb, "%d levels NHWC bf16 rgb vs oracle" % n_levels)
    _same_bits(dep, want_dep, "%d levels NCHW f16 depth vs oracle" % n_levels)


def test_level_boundaries_nhwc_bf16():
    boxes = rc.boundary_boxes()
    rois, maps = ro.to_rois([boxes]), rc.boundary_maps()      # the constants 1..4: exact in bfloat16
    rgb, _, lv = _forward([DevMap(m, (lc.BF16, lc.NHWC)) for m in maps], rc.SCALES4, rois, 8, 2)
    ref = _forward([_f32(m) for m in maps], rc.SCALES4, rois, 8, 2)
    wrong = int((lv != ref[2]).sum())
    _say("level boundaries NHWC bf16: %d boxes, levels that differ from the NCHW call %d" % (len(boxes), wrong))
    assert wrong == 0 and np.array_equal(lv, ro.map_levels(boxes))
    _same_bits(rgb, ref[0], "level boundaries NHWC bf16 vs float32 NCHW call")


@pytest.mark.parametrize("form", [(lc.F32, lc.NHWC), (lc.BF16, lc.NHWC)], ids=lc.form_id)
def test_invalid_samples_do_not_leak_nhwc(form):
    """NaN at pixel 0 of every plane, Inf wherever nothing samples: the outputs are those of the clean map."""
    feat, poisoned, rois = rc.leak_case()
    clean_q, poisoned_q = lc.quantise(feat, form[0]), lc.quantise(poisoned, form[0])
    assert np.isnan(poisoned_q[:, :, 0, 0]).all() and np.isinf(poisoned_q).any()
    clean = _forward([DevMap(clean_q, form)], (rc.SCALE,), rois, 8, 2)[0]
    got = _forward([DevMap(poisoned_q, form)], (rc.SCALE,), rois, 8, 2)[0]
    assert np.isfinite(got).all()
    _same_bits(got, clean, "poisoned map %s vs clean" % lc.form_id(form))
    _same_bits(clean, ro.roi_align(clean_q, rois, rc.SCALE, 8, 2), "poisoned map %s: clean run vs oracle" % lc.form_id(form))


def test_batch_with_empty_images_nhwc_f16():
    feats, depth, boxes = rc.empty_image_case()
    feats, depth = [lc.quantise(f, lc.F16) for f in feats], lc.quantise(depth, lc.F16)
    want_rgb, want_dep, want_lv = ro.pooler_forward(feats, [np.asarray(b).reshape(-1, 4) for b in boxes], depth, return_levels=True)
    form = (lc.F16, lc.NHWC)
    rgb, dep, lv = _forward([DevMap(f, form) for f in feats], rc.SCALES4, rc.to_rois(boxes), 8, 2, depth=DevMap(depth, form))
    assert np.array_equal(lv, want_lv)
    _same_bits(rgb, want_rgb, "images with (3, 0, 7, 0, 2) boxes NHWC f16 rgb")
    _same_bits(dep, want_dep, "images with (3, 0, 7, 0, 2) boxes NHWC f16 depth")


# ---- 4. / 5. backward -----------------------------------------------------------------------------------------------------------------------
def _backward(entry, shapes, scales, rois, pooled, ratio, g_rgb, layout, depth_shape=None, g_dep=None, depth_layout=None, off=False):
    """One backward entry point twice on guarded float32 buffers in `layout` (NaN-filled for the ordered entry, zeroed for the atomic
    one): per map the flat buffer as numpy."""
    from veto_amd import native
    ordered = entry.endswith("ordered")
    fill = float("nan") if ordered else 0.0
    trois, tg, td = _t(rois), _t(g_rgb), (_t(g_dep) if g_dep is not None else None)
    depth_layout = layout if depth_layout is None else depth_layout
    runs = []
    for _ in range(2):
        call = native.Launch(_dev(), "test")
        all_shapes = list(shapes) + ([depth_shape] if g_dep is not None else [])
        bufs = []
        for s in all_shapes:
            n = int(np.prod(s))
            buf = torch.full((n + GUARD + 1,), fill, device=_dev())
            bufs.append((buf, buf[1:1 + n] if off else buf[:n], n))
        a = _args(native, [(s, layout) for s in shapes], scales, trois, pooled, ratio,
                  depth=(depth_shape, depth_layout) if g_dep is not None else None)
        ptrs = (ctypes.c_void_p * 4)(*[v.data_ptr() for _, v, _ in bufs[:len(shapes)]])
        call.run(entry, ctypes.byref(a), tg.data_ptr(), td.data_ptr() if td is not None else None, ptrs,
                 bufs[-1][1].data_ptr() if g_dep is not None else None)
        torch.cuda.synchronize()
        for buf, v, n in bufs:
            lo = 1 if off else 0
            assert _guard_ok(buf, lo + n, fill) and (not off or _guard_ok(buf[:1], 0, fill)), "a write outside a gradient map"
        runs.append([v.cpu().numpy() for _, v, _ in bufs])
    if ordered:
        for x, y in zip(*runs):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), "two ordered calls differ"
    return runs[0]


def _check(got, ref, what):
    want, K, A = ref
    ratio, kmax = rc.check_backward(got, want, K, A)
    _say("%-58s K max %5d  error / bound %.3f" % (what, kmax, ratio))
    assert ratio <= 1.0, (what, ratio)


def _misread_fails(flat, ref):
    """The NHWC buffer read as NCHW must NOT pass the check."""
    want, K, A = ref
    try:
        ratio, _ = rc.check_backward(lc.unpack(flat, (lc.F32, lc.NCHW), want.shape), want, K, A)
    except AssertionError:
        return True
    return ratio > 1.0


def test_atomic_backward_nhwc_single_map_per_pixel():
    shape, rois, gout, ref = lc.single_backward()
    for off in (False, True):
        (flat,) = _backward("veto_roi_pool_backward", [shape], (rc.SCALE,), rois, 8, 2, gout, lc.NHWC, off=off)
        _check(lc.unpack(flat, (lc.F32, lc.NHWC), shape), ref, "atomic backward NHWC (8, 2) C 33%s" % (", off boundary" if off else ""))
        assert _misread_fails(flat, ref)


def test_atomic_backward_nhwc_pyramid_and_depth_in_either_layout():
    feats, depth, boxes, g_rgb, g_dep, per_level, dep_ref = lc.pyramid_backward(8)
    shapes, rois = [f.shape for f in feats], ro.to_rois(boxes)
    for depth_layout in (lc.NHWC, lc.NCHW):
        flats = _backward("veto_roi_pool_backward", shapes, rc.SCALES4, rois, 8, 2, g_rgb, lc.NHWC, depth.shape, g_dep, depth_layout)
        for l in range(4):
            _check(lc.unpack(flats[l], (lc.F32, lc.NHWC), shapes[l]), per_level[l], "atomic backward NHWC pyramid level %d" % l)
        _check(lc.unpack(flats[4], (lc.F32, depth_layout), depth.shape), dep_ref, "atomic backward depth map %s" % lc.LAYOUT_NAMES[depth_layout])
    assert _misread_fails(flats[0], per_level[0])


def test_atomic_backward_nhwc_contention():
    shape, rois, gout = rc.exact_contention_case()
    want, K, A = ro.roi_align_backward(gout, rois, rc.SCALE, shape, 8, 2, stats=True)
    (flat,) = _backward("veto_roi_pool_backward", [shape], (rc.SCALE,), rois, 8, 2, gout, lc.NHWC)
    got = lc.unpack(flat, (lc.F32, lc.NHWC), shape)
    bad = int((got.astype(np.float64) != want).sum())
    _say("atomic backward NHWC exact contention: compared %d  mismatches %d  K %d" % (want.size, bad, K.max()))
    assert bad == 0 and K.max() == 16384
    shape, rois, gout = rc.contention_case()
    ref = ro.roi_align_backward(gout, rois, rc.SCALE, shape, 8, 2, stats=True)
    (flat,) = _backward("veto_roi_pool_backward", [shape], (rc.SCALE,), rois, 8, 2, gout, lc.NHWC)
    _check(lc.unpack(flat, (lc.F32, lc.NHWC), shape), ref, "atomic backward NHWC contention, 64 x one sub-pixel ROI")


@pytest.mark.parametrize("name", lc.ORDERED_CASES)
def test_ordered_backward_nhwc_is_the_nchw_result_permuted(name):
    case, want_levels, want_dep = lc.ordered_reference(name)
    entry = "veto_roi_pool_backward_ordered"
    for off in (False, True):
        nhwc = _backward(entry, case.shapes, case.scales, case.rois, case.pooled, case.ratio, case.g_rgb, lc.NHWC, case.depth_shape,
                         case.g_dep, off=off)
        nchw = _backward(entry, case.shapes, case.scales, case.rois, case.pooled, case.ratio, case.g_rgb, lc.NCHW, case.depth_shape,
                         case.g_dep, off=off)
        shapes = case.shapes + ([case.depth_shape] if case.g_dep is not None else [])
        wants = want_levels + ([want_dep] if want_dep is not None else [])
        for i, (a, b, s, w) in enumerate(zip(nhwc, nchw, shapes, wants)):
            got = lc.unpack(a, (lc.F32, lc.NHWC), s)
            what = "ordered NHWC %s map %d%s" % (name, i, ", off boundary" if off else "")
            _same_bits(got, b.reshape(s), what + " vs NCHW call")
            _same_bits(got, w, what + " vs stated order")


# ---- 6. refusals and the old struct size --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codes", [(3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2), (-1, 0, 0, 0), (0, 0, 0, -1)])
def test_codes_out_of_range_are_refused_before_any_launch(codes):
    q, rois, _ = lc.single_forward(8, 2, 40, lc.F32)
    dq, _ = lc.depth_forward(8, lc.F32, 40)
    _forward([_f32(q)], (rc.SCALE,), rois, 8, 2, depth=_f32(dq), codes=codes, expect_error="dtype|layout")


def test_the_old_struct_size_means_float32_nchw():
    from veto_amd import native
    maps, scales, depth, rois, want_rgb, want_dep, want_lv = lc.pyramid_forward(4, lc.F32, lc.F32)
    levels, d = [_f32(m) for m in maps], _f32(depth)
    new = _forward(levels, scales, rois, 8, 2, depth=d, codes=(0, 0, 0, 0))
    # garbage in the new fields: a call of the old size must not read them
    old = _forward(levels, scales, rois, 8, 2, depth=d, struct_size=native.ROI_POOL_ARGS_SIZE_V1, codes=(9, 9, 9, 9))
    assert native.ROI_POOL_ARGS_SIZE_V1 == ctypes.sizeof(native.VetoRoiPoolArgs) - 16
    _same_bits(old[0], new[0], "old struct size rgb vs new size with zero fields")
    _same_bits(old[1], new[1], "old struct size depth vs new size with zero fields")
    assert np.array_equal(old[2], new[2]) and np.array_equal(old[2], want_lv)
    _same_bits(new[0], want_rgb, "new struct size rgb vs oracle")
    _forward(levels, scales, rois, 8, 2, depth=d, struct_size=native.ROI_POOL_ARGS_SIZE_V1 + 8, expect_error="size mismatch")


# ---- 7. Pooler on leaves of every form ---------------------------------------------------------------------------------------------------
def _props(boxes, size):
    from veto_amd.structures import BoxList
    return [BoxList(torch.from_numpy(np.asarray(b, dtype=F).reshape(-1, 4)), size).to(_dev()) for b in boxes]


def _leaf(values, form):
    t = _t(values).to(TORCH_DTYPES[form[0]])
    if form[1] == lc.NHWC:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True)


def _pooler(deterministic=False):
    from veto_amd.poolers import Pooler
    p = Pooler((8, 8), rc.SCALES4, 2)
    p.deterministic = deterministic
    return p


GRAD_TOL = {lc.F32: lambda want: 0.0,
            lc.F16: lambda want: 2.0 ** -11 * np.abs(want) + 2.0 ** -25,      # half an ulp of float16, half its subnormal spacing
            lc.BF16: lambda want: 2.0 ** -8 * np.abs(want)}                   # half an ulp of an 8-bit significand


@pytest.mark.parametrize("form", lc.FORMS, ids=lc.form_id)
def test_pooler_on_leaves_of_every_form(form):
    feats, depth, boxes, g_rgb, g_dep, per_level, dep_ref = lc.pyramid_backward(8)
    props = _props(boxes, (rc.PYR_W, rc.PYR_H))
    leaves = [_leaf(m, form) for m in feats + [depth]]
    fmt = torch.channels_last if form[1] == lc.NHWC else torch.contiguous_format
    assert all(m.is_contiguous(memory_format=fmt) for m in leaves)
    rgb, dep = _pooler()(leaves[:4], props, depth_features=leaves[4])
    ref_rgb, ref_dep = _pooler()([m.detach().float().contiguous() for m in leaves[:4]], props,
                                 depth_features=leaves[4].detach().float().contiguous())
    assert rgb.dtype == torch.float32 and rgb.is_contiguous() and dep.is_contiguous()
    _same_bits(rgb.detach().cpu().numpy(), ref_rgb.cpu().numpy(), "Pooler %s rgb vs .float().contiguous() leaves" % lc.form_id(form))
    _same_bits(dep.detach().cpu().numpy(), ref_dep.cpu().numpy(), "Pooler %s depth vs .float().contiguous() leaves" % lc.form_id(form))
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for i, (m, (want, K, A)) in enumerate(zip(leaves, per_level + [dep_ref])):
        g = m.grad
        assert g is not None and g.dtype == m.dtype and g.shape == m.shape and g.is_contiguous(memory_format=fmt), (i, g.dtype, g.stride())
        got = g.detach().float().cpu().numpy().astype(np.float64)
        bound = rc.backward_bound(want, K, A) + GRAD_TOL[form[0]](want)
        err, live = np.abs(got - want), bound > 0
        worst = float((err[live] / bound[live]).max())
        _say("Pooler %s grad of map %d: largest error / bound %.3f over %d elements" % (lc.form_id(form), i, worst, int(live.sum())))
        assert worst <= 1.0 and not err[~live].any(), (i, worst)
        assert not got[np.broadcast_to((K == 0)[:, None], want.shape)].any()


@pytest.mark.parametrize("form", lc.FORMS, ids=lc.form_id)
def test_pooler_deterministic_backward_twice_bit_equal(form):
    feats, depth, boxes, g_rgb, g_dep, _, _ = lc.pyramid_backward(8)
    props = _props(boxes, (rc.PYR_W, rc.PYR_H))
    grads = []
    for _ in range(2):
        leaves = [_leaf(m, form) for m in feats + [depth]]
        rgb, dep = _pooler(deterministic=True)(leaves[:4], props, depth_features=leaves[4])
        ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
        grads.append([m.grad.float().cpu().numpy() for m in leaves])
    for x, y in zip(*grads):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # and the ordered result in this form is the ordered result of float32 NCHW leaves, cast once
    leaves = [_t(lc.quantise(m, form[0])).requires_grad_(True) for m in feats + [depth]]
    rgb, dep = _pooler(deterministic=True)(leaves[:4], props, depth_features=leaves[4])
    ((rgb * _t(g_rgb)).sum() + (dep * _t(g_dep)).sum()).backward()
    for x, m in zip(grads[0], leaves):
        want = m.grad.to(TORCH_DTYPES[form[0]]).float().cpu().numpy()
        assert np.array_equal(x.view(np.int32), want.view(np.int32))


# ---- 8. no copy -----------------------------------------------------------------------------------------------------------------------------
def test_channels_last_bf16_maps_are_pooled_without_a_copy():
    """Four channels_last bfloat16 levels of 256 channels (64 x 96 down to 8 x 12), a 256 x 16 x 24 depth map, 24 ROIs, pooled 8: the two
    outputs are 3.1 MB, a float32 copy of level 0 alone is 12.6 MB.  The forward call may raise the peak by less than 6 MB."""
    from veto_amd.poolers import _roi_pool
    g = torch.Generator(device="cpu").manual_seed(5)
    maps = [torch.randn(2, 256, 64 >> l, 96 >> l, generator=g).to(_dev(), torch.bfloat16).contiguous(memory_format=torch.channels_last)
            for l in range(4)]
    depth = torch.randn(2, 256, 16, 24, generator=g).to(_dev(), torch.bfloat16).contiguous(memory_format=torch.channels_last)
    boxes = np.random.RandomState(6).uniform(0, 1, size=(24, 4)).astype(F)
    x1, y1 = boxes[:, 0] * 300, boxes[:, 1] * 200
    rois = np.stack([np.arange(24) % 2, x1, y1, x1 + 8 + boxes[:, 2] * 75, y1 + 8 + boxes[:, 3] * 50], 1).astype(F)
    trois = _t(rois)
    _roi_pool(maps, rc.SCALES4, trois, 2, 8, 2, depth=depth)      # the library is loaded, the stream's caches are warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    rgb, dep, _ = _roi_pool(maps, rc.SCALES4, trois, 2, 8, 2, depth=depth)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    _say("no copy: outputs %.1f MB, float32 copy of level 0 %.1f MB, peak rise %.2f MB"
         % ((rgb.numel() + dep.numel()) * 4 / 1e6, maps[0].numel() * 4 / 1e6, rise / 1e6))
    assert rise < 6e6, rise
    ref = _roi_pool([m.float().contiguous() for m in maps], rc.SCALES4, trois, 2, 8, 2, depth=depth.float().contiguous())
    assert torch.equal(rgb.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(dep.view(torch.int32), ref[1].view(torch.int32))


# ---- 9. fallback ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["strided_view", "mixed_formats", "float64"])
def test_other_inputs_still_take_the_copy_path(kind):
    from veto_amd.poolers import _map_form, _roi_pool
    maps, scales, depth, rois, want_rgb, want_dep, _ = lc.pyramid_forward(4, lc.F32, lc.F32)
    tm, td, trois = [_t(m) for m in maps], _t(depth), _t(rois)
    if kind == "strided_view":
        big = [torch.full((4,) + tuple(m.shape[1:]), float("nan"), device=_dev()) for m in tm]
        for b, m in zip(big, tm):
            b[::2] = m
        tm = [b[::2] for b in big]
    elif kind == "mixed_formats":
        tm = [tm[0]] + [m.contiguous(memory_format=torch.channels_last) for m in tm[1:]]
    else:
        tm, td = [m.double() for m in tm], td.double()
    assert _map_form(tm) is None
    rgb, dep, _ = _roi_pool(tm, scales, trois, 2, 8, 2, depth=td)
    _same_bits(rgb.cpu().numpy(), want_rgb, "fallback %s rgb" % kind)
    _same_bits(dep.cpu().numpy(), want_dep, "fallback %s depth" % kind)
