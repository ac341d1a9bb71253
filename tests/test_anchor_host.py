"""The anchor generator without a GPU: the cell anchors against the reference's fixtures (tests/golden/anchors/), the module's
interface and state dict, the factories, the installer, the refusals of veto_anchor_grid, and the mutation check of the numpy
restatements the GPU tests compare against."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_cases as ac  # noqa: E402

from veto_amd import native  # noqa: E402
from veto_amd.config import CfgNode, default_config  # noqa: E402


def _generator(c, t=0):
    from veto_amd.rpn import AnchorGenerator
    return AnchorGenerator(*ac.generator_args(c), t)


# ---- fixtures and yardsticks ---------------------------------------------------------------------------------------------------

def test_fixtures_are_present_and_small():
    total = 0
    for name, c in ac.CASES.items():
        path = os.path.join(ac.GOLDEN, name + ".npz")
        assert os.path.getsize(path) < 16 * 1024, name
        z = ac.load(name)
        total += sum(len(z[k]) for k in z.files if k.startswith("anchors_"))
        assert ("anchors_0" in z.files) == (not c.get("big"))
    assert total < 4000      # a few thousand anchor rows in all


@pytest.mark.parametrize("name", ["classic", "veto4", "retina"])
def test_cell_anchors_equal_the_reference(name):
    c, z = ac.CASES[name], ac.load(name)
    gen = _generator(c)
    assert len(gen.cell_anchors) == len(c["grids"])
    for l, cell in enumerate(gen.cell_anchors):
        assert cell.dtype == torch.float32
        np.testing.assert_array_equal(cell.numpy(), z["cell_%d" % l])
    if name == "classic":
        # the table of anchor_generator.py:197-217, (-83, -39, 100, 56) ... (-167, -343, 184, 360), is the matlab original's: 1-based
        # pixel coordinates.  The reference's own code, the fixture above, gives the 0-based form: every coordinate one less.
        matlab = [[-83, -39, 100, 56], [-175, -87, 192, 104], [-359, -183, 376, 200], [-55, -55, 72, 72], [-119, -119, 136, 136],
                  [-247, -247, 264, 264], [-35, -79, 52, 96], [-79, -167, 96, 184], [-167, -343, 184, 360]]
        np.testing.assert_array_equal(list(gen.cell_anchors)[0].numpy() + 1, np.asarray(matlab, np.float32))
        assert gen.num_anchors_per_location() == [9]
    if name == "veto4":
        assert gen.num_anchors_per_location() == [4] * 5
    if name == "retina":       # octave sizes: cell anchors that are no integers
        assert gen.num_anchors_per_location() == [9] * 5
        assert np.any(z["cell_0"] != np.round(z["cell_0"]))


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_numpy_restatements_reproduce_every_fixture(name):
    c, z = ac.CASES[name], ac.load(name)
    anchors = ac.np_anchors(c)
    assert ac.sha256(anchors) == str(z["anchor_sha256"])
    if not c.get("big"):
        for a, want in zip(anchors, ac.fixture_anchors(z, c)):
            np.testing.assert_array_equal(a, want)
    for t in c["thresholds"]:
        plane = ac.np_visibility_plane(anchors, c["images"], t)
        assert ac.sha256([plane]) == str(z["visibility_sha256_t%d" % t]), (name, t)
        assert str(z["visibility_dtype_t%d" % t]) == ("torch.bool" if t >= 0 else "torch.uint8")
        if not c.get("big"):
            np.testing.assert_array_equal(plane, z["visibility_t%d" % t])
        if t < 0:
            assert plane.all()


def test_edge_fixture_holds_the_equalities():
    c, z = ac.CASES["edges"], ac.load("edges")
    a = z["anchors_0"]
    assert a[ac._R].tolist() == [8, 8, 39, 39] and a[1].tolist() == [-16, -16, 31, 31]
    for (t, img, row), want in ac.EDGE_EXPECT.items():
        assert z["visibility_t%d" % t][img, row] == want, (t, img, row)
    assert not z["visibility_t0"][8].any() and not z["visibility_t16"][8].any()      # the 1 x 1 image sees no anchor
    z5 = ac.load("offsets5")                                                            # (20, 20): nothing of the coarsest level
    assert not z5["visibility_t0"][4, -3:].any() and z5["visibility_t0"][11].any()


MUTATIONS = {
    "h / w swapped in the row order": lambda c, t: (ac.np_anchors(c, order="wha"), None),
    "a as the slowest index": lambda c, t: (ac.np_anchors(c, order="ahw"), None),
    "<= at the far edge": lambda c, t: (None, dict(far="<=")),
    "image (height, width) swapped": lambda c, t: (None, dict(swap_size=True)),
    "the neighbouring level's stride": lambda c, t: (ac.np_anchors(c, stride_shift=1), None),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_wrong_restatement_changes_an_expected_array(mutation):
    """Each wrong restatement must disagree with the reference's stored arrays in at least one small case: the fixtures can tell
    the right order, comparison and stride from the wrong ones."""
    changed = []
    for name in ac.SMALL:
        c, z = ac.CASES[name], ac.load(name)
        for t in c["thresholds"]:
            anchors, kw = MUTATIONS[mutation](c, t)
            if anchors is not None:
                same = all(np.array_equal(a, w) for a, w in zip(anchors, ac.fixture_anchors(z, c)))
            else:
                same = np.array_equal(ac.np_visibility_plane(ac.fixture_anchors(z, c), c["images"], t, **kw), z["visibility_t%d" % t])
            if not same:
                changed.append((name, t))
    print(mutation, "changes", changed)
    assert changed


# ---- interface -------------------------------------------------------------------------------------------------------------------

def test_signatures_follow_the_reference():
    from veto_amd import rpn
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    sig = inspect.signature(rpn.AnchorGenerator.__init__)
    assert names(rpn.AnchorGenerator.__init__) == ["self", "sizes", "aspect_ratios", "anchor_strides", "straddle_thresh"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [(128, 256, 512), (0.5, 1.0, 2.0), (8, 16, 32), 0]
    assert names(rpn.AnchorGenerator.num_anchors_per_location) == ["self"]
    assert names(rpn.AnchorGenerator.grid_anchors) == ["self", "grid_sizes"]
    assert names(rpn.AnchorGenerator.add_visibility_to) == ["self", "boxlist"]
    assert names(rpn.AnchorGenerator.forward) == ["self", "image_list", "feature_maps"]
    assert names(rpn.make_anchor_generator) == ["config"] and names(rpn.make_anchor_generator_retinanet) == ["config"]
    gen = rpn.AnchorGenerator()
    assert gen.strides == (8, 16, 32) and gen.straddle_thresh == 0 and gen.num_anchors_per_location() == [3, 3, 3]
    one = rpn.AnchorGenerator(anchor_strides=(16,))      # the single-stride form: every size on the one level
    assert one.num_anchors_per_location() == [9]
    with pytest.raises(RuntimeError, match="FPN should have #anchor_strides == #sizes"):
        rpn.AnchorGenerator(sizes=(32, 64), anchor_strides=(4, 8, 16))
    assert rpn.ANCHOR_CACHE_SIZE == 4 and "ANCHOR_CACHE_SIZE" in rpn.AnchorGenerator.__doc__ and "in place" in rpn.AnchorGenerator.__doc__


class _RefBufferList(torch.nn.Module):      # the reference's module tree, for the state dict: a module holding buffers "0", "1", ...
    def __init__(self, buffers):
        super().__init__()
        for i, b in enumerate(buffers):
            self.register_buffer(str(i), b)


class _RefGenerator(torch.nn.Module):
    def __init__(self, cells):
        super().__init__()
        self.cell_anchors = _RefBufferList(cells)


def test_state_dict_keys_and_strict_loading_both_ways():
    c = ac.CASES["veto4"]
    gen = _generator(c)
    keys = ["cell_anchors.%d" % l for l in range(5)]
    assert list(gen.state_dict()) == keys
    ref = _RefGenerator([torch.from_numpy(ac.load("veto4")["cell_%d" % l]) + 1 for l in range(5)])
    assert list(ref.state_dict()) == keys
    gen.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(list(gen.cell_anchors)[2], list(ref.cell_anchors._buffers.values())[2])
    back = _RefGenerator([torch.zeros(4, 4) for _ in range(5)])
    back.load_state_dict(_generator(c).state_dict(), strict=True)
    np.testing.assert_array_equal(back.cell_anchors._buffers["4"].numpy(), ac.load("veto4")["cell_4"])
    whole = torch.nn.Sequential(torch.nn.Linear(2, 2), _generator(c))      # inside a larger module the keys keep their prefix
    assert [k for k in whole.state_dict() if "cell" in k] == ["1." + k for k in keys]


def test_factories_read_the_reference_keys():
    from veto_amd import rpn
    cfg = default_config()
    gen = rpn.make_anchor_generator(cfg)      # the VETO configuration: five levels, FOUR aspect ratios
    assert gen.num_anchors_per_location() == [4] * 5 and gen.strides == (4, 8, 16, 32, 64) and gen.straddle_thresh == 0
    for l, cell in enumerate(gen.cell_anchors):
        np.testing.assert_array_equal(cell.numpy(), ac.load("veto4")["cell_%d" % l])
    cfg.MODEL.RPN.ANCHOR_STRIDE = (4, 8)
    with pytest.raises(AssertionError, match="FPN should have"):
        rpn.make_anchor_generator(cfg)
    cfg.MODEL.RPN.USE_FPN = False
    with pytest.raises(AssertionError, match="single ANCHOR_STRIDE"):
        rpn.make_anchor_generator(cfg)
    cfg.MODEL.RPN.ANCHOR_STRIDE, cfg.MODEL.RPN.STRADDLE_THRESH = (16,), -1
    gen = rpn.make_anchor_generator(cfg)
    assert gen.num_anchors_per_location() == [20] and gen.straddle_thresh == -1
    r = cfg.MODEL.RETINANET = CfgNode()
    r.ANCHOR_SIZES, r.ASPECT_RATIOS, r.ANCHOR_STRIDES = ac.FPN_SIZES, ac.CLASSIC, ac.RETINA_STRIDES
    r.STRADDLE_THRESH, r.OCTAVE, r.SCALES_PER_OCTAVE = 0, 2.0, 3
    gen = rpn.make_anchor_generator_retinanet(cfg)
    assert gen.num_anchors_per_location() == [9] * 5
    for l, cell in enumerate(gen.cell_anchors):
        np.testing.assert_array_equal(cell.numpy(), ac.load("retina")["cell_%d" % l])
    r.ANCHOR_STRIDES = (8, 16)
    with pytest.raises(AssertionError, match="Only support FPN now"):
        rpn.make_anchor_generator_retinanet(cfg)


def test_cpu_feature_maps_are_refused():
    gen = _generator(ac.CASES["classic"])
    images = types.SimpleNamespace(image_sizes=[(48, 80)])
    with pytest.raises(RuntimeError, match="runs on a HIP device only"):
        gen(images, [torch.zeros(1, 1, 3, 5)])
    with pytest.raises(RuntimeError, match="runs on a HIP device only"):
        gen.grid_anchors([(3, 5)])


# ---- the installer ---------------------------------------------------------------------------------------------------------------

def test_install_anchor_ops_repoints_and_restores(monkeypatch):
    from test_roi_layouts_host import _fake_pysgg
    from veto_amd import registry, rpn
    GEN, RPN, RETINA = "pysgg.modeling.rpn.anchor_generator", "pysgg.modeling.rpn.rpn", "pysgg.modeling.rpn.retinanet.retinanet"
    mods = _fake_pysgg(monkeypatch, ["pysgg", "pysgg.modeling", "pysgg.modeling.rpn", GEN, RPN, "pysgg.modeling.rpn.retinanet", RETINA,
                                     "pysgg.modeling.rpn.inference"])
    make, make_retina, cls = (lambda config: "rpn"), (lambda config: "retina"), type("AnchorGenerator", (), {})
    mods[GEN].make_anchor_generator, mods[GEN].make_anchor_generator_retinanet, mods[GEN].AnchorGenerator = make, make_retina, cls
    mods[RPN].make_anchor_generator = make                       # rpn/rpn.py:9
    mods[RETINA].make_anchor_generator_retinanet = make_retina   # rpn/retinanet/retinanet.py:8
    sentinel = object()
    mods["pysgg.modeling.rpn.inference"].make_rpn_postprocessor = mods[RPN].make_rpn_postprocessor = sentinel
    mods[RPN].make_rpn_loss_evaluator = sentinel
    patched = registry.install_anchor_ops()
    assert mods[GEN].make_anchor_generator is rpn.make_anchor_generator and mods[RPN].make_anchor_generator is rpn.make_anchor_generator
    assert mods[GEN].make_anchor_generator_retinanet is rpn.make_anchor_generator_retinanet
    assert mods[RETINA].make_anchor_generator_retinanet is rpn.make_anchor_generator_retinanet
    assert mods[GEN].AnchorGenerator is rpn.AnchorGenerator
    assert patched == [(GEN, "make_anchor_generator"), (RPN, "make_anchor_generator"), (GEN, "make_anchor_generator_retinanet"),
                       (RETINA, "make_anchor_generator_retinanet"), (GEN, "AnchorGenerator")]
    assert mods[RPN].make_rpn_postprocessor is sentinel and mods[RPN].make_rpn_loss_evaluator is sentinel      # independent of the others
    assert registry.install_anchor_ops() == []      # a second call finds nothing left to patch
    assert registry.uninstall_anchor_ops() == 5
    assert mods[GEN].make_anchor_generator is make and mods[RPN].make_anchor_generator is make
    assert mods[GEN].make_anchor_generator_retinanet is make_retina and mods[RETINA].make_anchor_generator_retinanet is make_retina
    assert mods[GEN].AnchorGenerator is cls
    assert registry.uninstall_anchor_ops() == 0


def test_install_anchor_ops_without_the_rpn_modules_loaded(monkeypatch):
    from test_roi_layouts_host import _fake_pysgg
    from veto_amd import registry, rpn
    GEN = "pysgg.modeling.rpn.anchor_generator"
    mods = _fake_pysgg(monkeypatch, ["pysgg", "pysgg.modeling", "pysgg.modeling.rpn", GEN])
    monkeypatch.delitem(sys.modules, "pysgg.modeling.rpn.rpn", raising=False)
    mods[GEN].make_anchor_generator, mods[GEN].make_anchor_generator_retinanet = (lambda config: 0), (lambda config: 1)
    mods[GEN].AnchorGenerator = type("AnchorGenerator", (), {})
    patched = registry.install_anchor_ops()
    assert [m for m, _ in patched] == [GEN] * 3 and mods[GEN].AnchorGenerator is rpn.AnchorGenerator
    assert registry.uninstall_anchor_ops() == 3


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------------

def _args(**kw):
    a = native.VetoAnchorArgs(struct_size=ctypes.sizeof(native.VetoAnchorArgs), n_img=2, n_lvl=2, straddle_thresh=0.0)
    for l, (A, H, W, s) in enumerate(((3, 4, 6, 8), (3, 2, 3, 16))):
        a.level_a[l], a.level_h[l], a.level_w[l], a.level_stride[l] = A, H, W, s
        a.cell_anchors[l] = 256
    a.image_sizes, a.anchors, a.anchors_in, a.visibility = 256, 512, None, 1024      # (never dereferenced: every call is refused)
    for k, v in kw.items():
        if isinstance(v, dict):
            for l, x in v.items():
                getattr(a, k)[l] = x
        else:
            setattr(a, k, v)
    return a


REFUSALS = [
    (dict(struct_size=8), "veto_anchor_args_t size mismatch"),
    (dict(n_lvl=0), "n_lvl 0 outside 1..8"),
    (dict(n_lvl=9), "n_lvl 9 outside 1..8"),
    (dict(level_a={1: 0}), "level 1: bad shape (A 0, H 2, W 3)"),
    (dict(level_h={0: 0}), "level 0: bad shape (A 3, H 0, W 6)"),
    (dict(level_w={0: -1}), "level 0: bad shape (A 3, H 4, W -1)"),
    (dict(level_stride={1: 0}), "level 1: stride 0 must be >= 1"),
    (dict(level_a={0: 1}, level_h={0: 1}, level_w={0: 2}, level_stride={0: 1 << 24}), "must stay below 2^24"),
    (dict(level_a={0: 1}, level_h={0: 1025}, level_w={0: 1}, level_stride={0: 1 << 14}), "must stay below 2^24"),
    (dict(level_a={0: 4}, level_h={0: 512}, level_w={0: 512}), "an image holds 1048594 anchors, the limit is 1048576"),
    (dict(anchors=None, visibility=None), "anchors and visibility are both NULL"),
    (dict(anchors=None), "missing pointer: anchors_in"),
    (dict(anchors=520), "16-byte aligned"),
    (dict(cell_anchors={1: None}), "missing pointer: cell_anchors[1]"),
    (dict(cell_anchors={0: 260}), "cell_anchors[0] must be 16-byte aligned"),
    (dict(n_img=0), "n_img 0 outside 1..65535 (visibility is asked for)"),
    (dict(image_sizes=None), "missing pointer: image_sizes"),
]


@pytest.mark.parametrize("change, needle", REFUSALS, ids=[n for _, n in REFUSALS])
def test_anchor_grid_names_the_cause_of_every_refusal(change, needle):
    lib = native.load_library()
    assert lib.veto_anchor_grid(None, ctypes.byref(_args(**change))) == -1
    assert needle in lib.veto_last_error().decode(), lib.veto_last_error()


def test_anchor_grid_null_argument_and_export():
    lib = native.load_library()
    assert lib.veto_anchor_grid(None, None) == -1 and b"null argument" in lib.veto_last_error()
    assert "veto_anchor_grid" in native.EXPORTS and native.STRUCTS["veto_anchor_args_t"] is native.VetoAnchorArgs
