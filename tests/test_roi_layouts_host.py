"""What tests/test_roi_layouts_gpu.py rests on, checked on the CPU: the buffers of every map form hold exactly the values they are
compared on, the off-boundary maps are off a boundary, the numpy bfloat16 rounding is torch's, a kernel that ignores a layout or
dtype flag would compute something else on every case, and install_pooler_ops re-points the names it promises to."""
import sys
import types

import numpy as np
import pytest

import deterministic_cases as dc
import roi_layout_cases as lc
import roi_pool_cases as rc
from oracle import roi_align_oracle as ro

F = np.float32
ALL_FORMS = [(lc.F32, lc.NCHW)] + lc.FORMS


# ---- case premises ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL_FORMS, ids=lc.form_id)
def test_every_buffer_holds_exactly_the_values_it_is_compared_on(form):
    feat, _ = rc.single(8, 2, 33)
    feat = feat.copy()
    feat[0, 0, 0, :4] = [np.nan, np.inf, -np.inf, -0.0]
    q = lc.quantise(feat, form[0])
    buf = lc.pack(q, form)
    assert buf.dtype == {lc.F32: np.float32, lc.F16: np.float16, lc.BF16: np.uint16}[form[0]]
    assert buf.shape == ((2, 50, 84, 33) if form[1] == lc.NHWC else (2, 33, 50, 84)) and buf.flags.c_contiguous
    back = lc.unpack(buf, form, feat.shape)
    assert np.array_equal(back.view(np.int32), q.view(np.int32))                       # NaN, the infinities and -0 included
    assert np.array_equal(lc.quantise(q, form[0]).view(np.int32), q.view(np.int32))   # quantising is idempotent
    if form[1] == lc.NHWC:      # one pixel's channels are adjacent
        assert np.array_equal(lc.unpack(buf, form, feat.shape)[1, :, 7, 9].view(np.int32),
                              lc.unpack(buf.reshape(-1)[((1 * 50 + 7) * 84 + 9) * 33:][:33], (form[0], lc.NCHW), (1, 33, 1, 1)).reshape(-1).view(np.int32))
    if form[0] != lc.F32:
        assert (q != feat)[np.isfinite(feat)].any()      # the rounding is not a no-op on these maps


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint16])
def test_off_boundary_maps_are_off_a_16_byte_boundary(dtype):
    flat = np.arange(100).astype(dtype)
    view, owner = lc.off_boundary(flat)
    assert view.ctypes.data % 16 == flat.dtype.itemsize and np.array_equal(view, flat)
    assert owner.ctypes.data <= view.ctypes.data and view.ctypes.data + view.nbytes <= owner.ctypes.data + owner.nbytes


# ---- bfloat16 rounding, written twice -----------------------------------------------------------------------------------------------
def test_numpy_bf16_rounding_is_torch_bfloat16():
    rng = np.random.RandomState(9)
    bits = np.concatenate([
        rng.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32),
        np.array([0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,       # ties to even, both ways
                  0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008000, 0x807F8000,                  # subnormals
                  0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,                                          # the largest finite value
                  0x7F800000, 0xFF800000, 0x00000000, 0x80000000], dtype=np.uint32)])
    x = bits.view(F)
    a, b = lc.bf16_bits(x), lc.bf16_bits_torch(x)
    nan = np.isnan(x)
    assert np.array_equal(a[~nan], b[~nan])
    assert np.isnan(lc.bf16_to_f32(a[nan])).all() and np.isnan(lc.bf16_to_f32(b[nan])).all()      # a NaN stays a NaN, never an infinity
    nans = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF80FFFF], dtype=np.uint32).view(F)
    assert np.isnan(lc.bf16_to_f32(lc.bf16_bits(nans))).all() and np.isnan(lc.bf16_to_f32(lc.bf16_bits_torch(nans))).all()
    named = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80, 0x00008000: 0x0000, 0x00018000: 0x0002}
    for src, want in named.items():
        assert int(lc.bf16_bits(np.array([src], dtype=np.uint32).view(F))[0]) == want, hex(src)


# ---- layout and dtype sensitivity ------------------------------------------------------------------------------------------------------
def _misread_layout(values):
    """What a kernel that ignores the NHWC flag sees: the NHWC buffer of `values` read as NCHW."""
    return lc.unpack(lc.pack(values, (lc.F32, lc.NHWC)), (lc.F32, lc.NCHW), values.shape)


def test_forward_cases_tell_a_misread_layout_and_a_misread_dtype():
    checked = 0
    for channels in lc.CHANNELS:
        q, rois, want = lc.single_forward(8, 2, channels, lc.BF16)
        if channels > 1:      # (C == 1: both layouts are the same buffer, and the host takes NCHW)
            assert not np.array_equal(ro.roi_align(_misread_layout(q), rois, rc.SCALE, 8, 2), want), channels
        as_f16 = lc.unpack(lc.pack(q, (lc.BF16, lc.NCHW)), (lc.F16, lc.NCHW), q.shape)
        with np.errstate(invalid="ignore"):
            assert not np.array_equal(ro.roi_align(np.nan_to_num(as_f16), rois, rc.SCALE, 8, 2), want), channels
        checked += 1
    for pooled, ratio in lc.FORWARD_INSTANCES:
        q, rois, want = lc.single_forward(pooled, ratio, 40, lc.F16)
        assert not np.array_equal(ro.roi_align(_misread_layout(q), rois, rc.SCALE, pooled, ratio), want), (pooled, ratio)
        checked += 1
    assert checked == len(lc.CHANNELS) + len(lc.FORWARD_INSTANCES)


def test_pyramid_and_boundary_cases_tell_a_misread_layout():
    maps, scales, depth, rois, want_rgb, want_dep, _ = lc.pyramid_forward(4, lc.BF16, lc.F16)
    boxes = [rois[rois[:, 0] == i, 1:] for i in range(2)]
    rgb, dep = ro.pooler_forward([_misread_layout(m) for m in maps], boxes, _misread_layout(depth), scales=scales)
    assert not np.array_equal(rgb, want_rgb) and not np.array_equal(dep, want_dep)
    # the boundary maps are constants: their NHWC and NCHW buffers are the same bytes, so that case tests the level choice alone
    for m in rc.boundary_maps():
        assert np.array_equal(_misread_layout(m), m)


def test_backward_cases_tell_a_misread_layout():
    """The expected gradient, packed NHWC and read as NCHW, is another gradient: at the atomic cases it misses the bound, at every
    ordered case it differs in a bit."""
    shape, rois, gout, (want, K, A) = lc.single_backward()
    wrong = _misread_layout(want.astype(F))
    with pytest.raises(AssertionError):
        ratio, _ = rc.check_backward(wrong, want, K, A)
        assert ratio <= 1.0
    for name in lc.ORDERED_CASES:
        case, levels, dep = lc.ordered_reference(name)
        differs = [not np.array_equal(_misread_layout(g), g) for g in levels + ([dep] if dep is not None else []) if g.shape[1] > 1]
        assert differs and all(differs), name
    assert set(lc.ORDERED_CASES) <= set(dc.ROI_CASES)


def test_ordered_cases_cover_the_vector_and_the_scalar_store():
    """The NHWC ordered kernel stores four floats at once where C is a multiple of 4 and the map is 16-byte aligned: the cases hold
    both kinds of C, and the device test runs each aligned and 4 bytes off."""
    cs = {dc.ROI_CASES[n]().shapes[0][1] for n in lc.ORDERED_CASES}
    assert any(c % 4 == 0 for c in cs) and any(c % 4 for c in cs) and any(c > 32 for c in cs)


# ---- install_pooler_ops ------------------------------------------------------------------------------------------------------------------
def _fake_pysgg(monkeypatch, names):
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
        monkeypatch.setitem(sys.modules, n, m)
        if "." in n:
            setattr(mods[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], m)
    return mods


BASE = ["pysgg", "pysgg.layers", "pysgg.layers.roi_align", "pysgg.modeling", "pysgg.modeling.poolers"]
EXTRACTORS = "pysgg.modeling.roi_heads.box_head.roi_box_feature_extractors"


def _originals(mods):
    align, pooler = type("ROIAlign", (), {}), type("Pooler", (), {})
    mods["pysgg.layers.roi_align"].ROIAlign = align
    mods["pysgg.layers"].ROIAlign = align
    mods["pysgg.modeling.poolers"].ROIAlign = align      # poolers.py binds it by name and builds its ROIAlign modules through it
    mods["pysgg.modeling.poolers"].Pooler = pooler
    return align, pooler


def test_install_pooler_ops_repoints_the_classes_and_their_bound_names(monkeypatch):
    from veto_amd import poolers, registry
    mods = _fake_pysgg(monkeypatch, BASE + ["pysgg.modeling.roi_heads", "pysgg.modeling.roi_heads.box_head", EXTRACTORS])
    align, pooler = _originals(mods)
    mods[EXTRACTORS].Pooler = pooler
    sentinel = object()
    mods["pysgg.layers"].nms = sentinel
    patched = registry.install_pooler_ops()
    assert mods["pysgg.layers"].ROIAlign is poolers.ROIAlign and mods["pysgg.layers.roi_align"].ROIAlign is poolers.ROIAlign
    assert mods["pysgg.modeling.poolers"].ROIAlign is poolers.ROIAlign and mods["pysgg.modeling.poolers"].Pooler is poolers.Pooler
    assert mods[EXTRACTORS].Pooler is poolers.Pooler
    assert mods["pysgg.layers"].nms is sentinel      # nothing else is touched
    assert patched == [("pysgg.layers", "ROIAlign"), ("pysgg.layers.roi_align", "ROIAlign"), ("pysgg.modeling.poolers", "ROIAlign"),
                       ("pysgg.modeling.poolers", "Pooler"), (EXTRACTORS, "Pooler")]
    assert registry.install_pooler_ops() == []      # a second call finds nothing left to patch


def test_install_pooler_ops_without_the_extractor_module_loaded(monkeypatch):
    from veto_amd import poolers, registry
    mods = _fake_pysgg(monkeypatch, BASE)
    _originals(mods)
    monkeypatch.delitem(sys.modules, EXTRACTORS, raising=False)
    patched = registry.install_pooler_ops()
    assert ("pysgg.modeling.poolers", "Pooler") in patched and all(m != EXTRACTORS for m, _ in patched)
    assert mods["pysgg.modeling.poolers"].Pooler is poolers.Pooler


def test_the_installed_pooler_keeps_refusing_what_it_does_not_build():
    from veto_amd import poolers
    with pytest.raises(NotImplementedError, match="cat_all_levels"):
        poolers.Pooler((7, 7), (0.25, 0.125), 2, cat_all_levels=True)
    p = poolers.Pooler((7, 7), (0.25, 0.125, 0.0625, 0.03125), 2)      # the box head's pooler builds
    assert p.output_size == (7, 7)
    with pytest.raises(NotImplementedError, match="union"):
        p([], [], union=True)


# ---- the host's choice of form ---------------------------------------------------------------------------------------------------------------
def test_map_form_of_the_host():
    import torch
    from veto_amd import native
    from veto_amd.poolers import _map_form
    m = torch.zeros(4, 6, 5, 7)
    cl =m.contiguous(memory_format=torch.channels_last)
    assert _map_form([m, m]) == (native.VETO_ROI_F32, native.VETO_ROI_NCHW)
    assert _map_form([cl.half(), cl.half()]) == (native.VETO_ROI_F16, native.VETO_ROI_NHWC)
    assert _map_form([cl.bfloat16()]) == (native.VETO_ROI_BF16, native.VETO_ROI_NHWC)
    assert _map_form([m, cl]) is None and _map_form([m.double()]) is None and _map_form([m[::2]]) is None and _map_form([m, m.half()]) is None
    one = torch.zeros(2, 1, 5, 7).contiguous(memory_format=torch.channels_last)      # both formats hold: NCHW
    assert _map_form([one]) == (native.VETO_ROI_F32, native.VETO_ROI_NCHW)
    assert _map_form([torch.zeros(2, 6, 1, 1)]) == (native.VETO_ROI_F32, native.VETO_ROI_NCHW)
    assert native.ROI_POOL_ARGS_SIZE_V1 == native.VetoRoiPoolArgs.level_dtype.offset
