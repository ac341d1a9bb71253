"""The anchor generator on the MI355X: veto_anchor_grid against the reference's fixtures (tests/golden/anchors/) and synth.anchor_grid,
bit for bit -- anchors as uint32 words, visibility as bytes --, every C-ABI call made twice into sentinel-filled outputs with guard
cells behind them; then the module (structure, sharing, cache), its two consumers and the launches of a forward."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_cases as ac  # noqa: E402

from veto_amd import native, synth  # noqa: E402
from veto_amd.structures import BoxList  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
F_SENTINEL, B_SENTINEL = -7777.25, 0xAB
_CELLS = {}


def _levels(c):
    """((A, H, W, stride) per level, the fixture's cell anchors on the device), made once per case."""
    key = id(c)
    if key not in _CELLS:
        name = next(n for n, v in ac.CASES.items() if v is c)
        z = ac.load(name)
        cells = [torch.from_numpy(z["cell_%d" % l]).to(DEV) for l in range(len(c["grids"]))]
        strides = c["strides"]
        _CELLS[key] = (tuple((len(cell), h, w, strides[l]) for l, (cell, (h, w)) in enumerate(zip(cells, c["grids"]))), cells)
    return _CELLS[key]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _abi(c, t=0, images=None, generate=True, anchors_in=None, want_visibility=True):
    """veto_anchor_grid twice, each time into fresh sentinel-filled outputs with GUARD untouched cells behind them; the two results
    must agree bit for bit.  Returns (anchors [total, 4] float32 numpy or None, visibility [n_img, total] uint8 numpy or None)."""
    from veto_amd.rpn import _anchor_call
    levels, cells = _levels(c)
    total = sum(A * H * W for A, H, W, _ in levels)
    images = list(c["images"] if images is None else images)
    results = []
    for _ in range(2):
        out = torch.full((total + GUARD, 4), F_SENTINEL, dtype=torch.float32, device=DEV) if generate else None
        vis = torch.full((len(images) * total + GUARD,), B_SENTINEL, dtype=torch.uint8, device=DEV) if want_visibility else None
        _anchor_call(DEV, levels, cells, anchors=out[:total] if generate else None, anchors_in=anchors_in, image_sizes=images,
                     straddle_thresh=t, visibility=vis[:len(images) * total] if want_visibility else None)
        a = v = None
        if generate:
            host = out.cpu().numpy()
            assert (host[total:] == np.float32(F_SENTINEL)).all(), "anchors: a guard cell was written"
            a = host[:total]
            assert not (a == np.float32(F_SENTINEL)).any(), "anchors: a row was left unwritten"
        if want_visibility:
            host = vis.cpu().numpy()
            assert (host[len(images) * total:] == B_SENTINEL).all(), "visibility: a guard cell was written"
            v = host[:len(images) * total].reshape(len(images), total)
            assert np.isin(v, (0, 1)).all(), "visibility: a byte is neither 0 nor 1"
        results.append((a, v))
    (a0, v0), (a1, v1) = results
    if generate:
        assert np.array_equal(_bits(a0), _bits(a1))
    if want_visibility:
        assert np.array_equal(v0, v1)
    return a0, v0


def _check_small(name, thresholds=None, images=None):
    c, z = ac.CASES[name], ac.load(name)
    want = np.concatenate(ac.fixture_anchors(z, c))
    second = np.concatenate(ac.np_anchors(c))
    idx = list(range(len(c["images"]))) if images is None else list(images)
    for t in (c["thresholds"] if thresholds is None else thresholds):
        a, v = _abi(c, t, [c["images"][i] for i in idx])
        assert np.array_equal(_bits(a), _bits(want)), (name, "anchors differ from the reference's")
        assert np.array_equal(_bits(a), _bits(second)), (name, "anchors differ from synth.anchor_grid")
        assert np.array_equal(v, z["visibility_t%d" % t][idx]), (name, t, "visibility differs from the reference's")
        # the cache-hit call: anchors NULL, the plane computed from an existing buffer
        _, v2 = _abi(c, t, [c["images"][i] for i in idx], generate=False, anchors_in=torch.from_numpy(want).to(DEV))
        assert np.array_equal(v2, v)
        if t < 0:
            assert v.all()


@pytest.mark.parametrize("name", [n for n in ac.SMALL if n.startswith("flat_")])
def test_flat_index_boundaries(name):
    _check_small(name)


@pytest.mark.parametrize("name", ["classic", "veto4", "retina", "offsets5", "levels8", "edges"])
def test_small_cases_equal_the_reference_bit_for_bit(name):
    _check_small(name)


@pytest.mark.parametrize("n_img", [1, 2, 12, 13])
def test_visibility_for_batches_of_different_images(n_img):
    """1, 2, 12 and 13 images whose sizes all differ (13: more than a multiple of anything), t = 0, 16 and -1; image 4 is smaller than
    every anchor of the coarsest level, image 5 than every anchor."""
    assert len(set(ac.THIRTEEN)) == 13
    _check_small("offsets5", images=range(13 - n_img, 13) if n_img < 13 else None)
    _check_small("offsets5", thresholds=(0,), images=range(n_img))


def test_edge_equalities_on_the_device():
    c = ac.CASES["edges"]
    for t in c["thresholds"]:
        _, v = _abi(c, t, generate=True)
        for (tt, img, row), want in ac.EDGE_EXPECT.items():
            if tt == t:
                assert v[img, row] == want, (t, img, row)
        assert not v[8].any()      # the 1 x 1 image: all zero
    _, v = _abi(c, -1)
    assert v.all()


def test_anchors_without_visibility_and_nine_levels():
    c = ac.CASES["levels8"]
    a, v = _abi(c, want_visibility=False)
    assert v is None and np.array_equal(_bits(a), _bits(np.concatenate(ac.np_anchors(c))))
    from veto_amd.rpn import _anchor_call
    levels, cells = _levels(c)
    out = torch.empty((8, 4), dtype=torch.float32, device=DEV)
    with pytest.raises(native.VetoError, match="n_lvl 9 outside 1..8"):
        _anchor_call(DEV, levels + (levels[0],), cells + [cells[0]], anchors=out)


@pytest.mark.parametrize("name", ["wide15", "retina9", "veto_big"])
def test_big_cases_against_the_yardstick_and_the_checksums(name):
    """wide15: A = 15 on a 38 x 50 grid; retina9: A = 9 with non-integer cell anchors; veto_big: the 200 x 336 level with A = 4
    (268 800 rows) and the four levels behind it, 12 images."""
    c, z = ac.CASES[name], ac.load(name)
    a, v = _abi(c, 0)
    want = ac.np_anchors(c)
    assert np.array_equal(_bits(a), _bits(np.concatenate(want)))
    rows = np.cumsum([0] + [len(w) for w in want])
    assert ac.sha256([a[rows[l]:rows[l + 1]] for l in range(len(want))]) == str(z["anchor_sha256"])
    assert np.array_equal(v, ac.np_visibility_plane(want, c["images"], 0))
    assert ac.sha256([v]) == str(z["visibility_sha256_t0"])


# ---- the module ------------------------------------------------------------------------------------------------------------------

def _module(c, t=0):
    from veto_amd.rpn import AnchorGenerator
    return AnchorGenerator(*ac.generator_args(c), t).to(DEV)


def _inputs(c, grids=None, images=None):
    images = c["images"] if images is None else images
    maps = [torch.empty((len(images), 1, h, w), device=DEV) for h, w in (c["grids"] if grids is None else grids)]
    return types.SimpleNamespace(image_sizes=[(h, w) for w, h in images]), maps


def _ptrs(out):
    return [lvl.bbox.data_ptr() for lvl in out[0]]


@pytest.mark.parametrize("t", [0, 16, -1])
def test_forward_structure_sharing_and_values(t):
    c, z = ac.CASES["offsets5"], ac.load("offsets5")
    gen = _module(c, t)
    out = gen(*_inputs(c))
    assert len(out) == 13 and all(len(per_img) == 5 for per_img in out)
    want = ac.fixture_anchors(z, c)
    plane = z["visibility_t%d" % t]
    rows = np.cumsum([0] + [len(w) for w in want])
    for i, (per_img, size) in enumerate(zip(out, c["images"])):
        for l, lvl in enumerate(per_img):
            assert type(lvl) is BoxList and lvl.mode == "xyxy" and tuple(lvl.size) == tuple(size)
            assert lvl.bbox.dtype == torch.float32 and lvl.bbox.device.type == "cuda" and lvl.bbox.shape == (len(want[l]), 4)
            assert lvl.bbox.data_ptr() == out[0][l].bbox.data_ptr()      # one tensor per level across the images
            vis = lvl.get_field("visibility")
            assert vis.dtype == (torch.bool if t >= 0 else torch.uint8) and vis.shape == (len(want[l]),)
            assert np.array_equal(vis.cpu().numpy().astype(np.uint8), plane[i, rows[l]:rows[l + 1]]), (t, i, l)
            if i == 0:
                assert np.array_equal(_bits(lvl.bbox.cpu().numpy()), _bits(want[l]))
    assert len({p for p in _ptrs(out)}) == 5
    # grid_anchors and add_visibility_to, the reference's other two entry points
    for g, w in zip(gen.grid_anchors(c["grids"]), want):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w))
    assert [g.data_ptr() for g in gen.grid_anchors(c["grids"])] == _ptrs(out)
    one = BoxList(torch.from_numpy(want[0]).to(DEV), c["images"][3], "xyxy")
    gen.add_visibility_to(one)
    assert one.get_field("visibility").dtype == (torch.bool if t >= 0 else torch.uint8)
    assert np.array_equal(one.get_field("visibility").cpu().numpy().astype(np.uint8), plane[3, :rows[1]])


def test_cache_hits_misses_eviction_and_invalidation():
    from veto_amd.rpn import ANCHOR_CACHE_SIZE
    c, z = ac.CASES["offsets5"], ac.load("offsets5")
    gen = _module(c)
    grids = [tuple((h + k, w) for h, w in c["grids"]) for k in range(ANCHOR_CACHE_SIZE + 1)]
    first = gen(*_inputs(c, grids[0]))
    p0 = _ptrs(first)
    assert _ptrs(gen(*_inputs(c, grids[0], images=c["images"][:2]))) == p0      # same grids, other images: a hit
    other = gen(*_inputs(c, grids[1]))
    assert not set(_ptrs(other)) & set(p0)                                        # other grids: another buffer
    assert _ptrs(gen(*_inputs(c, grids[0]))) == p0                                # back to the first grids: a hit again
    assert np.array_equal(_bits(first[0][0].bbox.cpu().numpy()), _bits(z["anchors_0"]))      # and the first buffer kept its values
    assert np.array_equal(_bits(other[0][0].bbox.cpu().numpy()),
                          _bits(synth.anchor_grid(ac.level_sizes(c), c["strides"], c["ratios"], grids[1])[0]))
    # LRU at the bound: grids[0] was used last, so filling the cache with grids[2..] evicts grids[1] first and grids[0] last
    for g in grids[2:]:
        gen(*_inputs(c, g))
    assert len(gen._cache) == ANCHOR_CACHE_SIZE
    assert _ptrs(gen(*_inputs(c, grids[0]))) == p0                                # still cached (4 shapes: 0, 2, 3, 4)
    gen(*_inputs(c, grids[1]))                                                    # a miss: evicts the least recently used, grids[2]
    keys = [k[1] for k in gen._cache]
    assert grids[2] not in keys and grids[0] in keys and grids[1] in keys and len(keys) == ANCHOR_CACHE_SIZE
    held = first[0][0].bbox                                                       # (keeps the old buffer alive: its address is not reused)
    # .to() empties the cache; a changed cell_anchors buffer does too, and the new anchors follow the new cell anchors
    gen.to(DEV)
    assert len(gen._cache) == 0
    again = gen(*_inputs(c, grids[0]))
    assert _ptrs(again) != p0 and np.array_equal(_bits(again[0][0].bbox.cpu().numpy()), _bits(z["anchors_0"]))
    sd = {k: v + 1 for k, v in gen.state_dict().items()}
    gen.load_state_dict(sd, strict=True)
    moved = gen(*_inputs(c, grids[0]))
    assert np.array_equal(_bits(moved[0][0].bbox.cpu().numpy()), _bits(z["anchors_0"] + 1))
    assert np.array_equal(_bits(held.cpu().numpy()), _bits(z["anchors_0"]))


def test_a_forward_on_another_stream_takes_its_own_buffer():
    """The buffer is written on the stream of its miss: a forward on another stream must not read it unordered, so it is a miss."""
    c, z = ac.CASES["offsets5"], ac.load("offsets5")
    gen = _module(c)
    p0 = _ptrs(gen(*_inputs(c)))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = gen(*_inputs(c))
        assert not set(_ptrs(out)) & set(p0)
        assert _ptrs(gen(*_inputs(c))) == _ptrs(out)      # and a hit on that stream
    side.synchronize()
    assert np.array_equal(_bits(out[0][0].bbox.cpu().numpy()), _bits(z["anchors_0"]))
    assert _ptrs(gen(*_inputs(c))) == p0


# ---- the consumers ---------------------------------------------------------------------------------------------------------------

def _generated_and_plain(sizes, strides, ratios, grids, images):
    """(the generator's output, BoxLists built from synth.anchor_grid) for one geometry."""
    from veto_amd.rpn import AnchorGenerator
    gen = AnchorGenerator(tuple(sizes), tuple(ratios), tuple(strides), 0).to(DEV)
    maps = [torch.empty((len(images), 1, h, w), device=DEV) for h, w in grids]
    made = gen(types.SimpleNamespace(image_sizes=[(h, w) for w, h in images]), maps)
    level_sizes = [s if isinstance(s, tuple) else (s,) for s in sizes] if len(strides) > 1 else [tuple(sizes)]
    plain_t = [torch.from_numpy(a).to(DEV) for a in synth.anchor_grid(level_sizes, strides, ratios, grids)]
    plain = [[BoxList(a, size, "xyxy") for a in plain_t] for size in images]
    return made, plain


def test_rpn_post_processor_returns_the_same_bits():
    from test_rpn_host import CASES, RATIOS, case_inputs
    from veto_amd.rpn import RPNPostProcessor
    c = CASES["small5"]
    z = np.load(os.path.join(os.path.dirname(ac.GOLDEN), "rpn", "small5.npz"))
    d = case_inputs("small5", int(z["seed"]))
    made, plain = _generated_and_plain(c["sizes"], c["strides"], RATIOS, c["grids"], c["images"])
    obj, reg = [torch.from_numpy(x).to(DEV) for x in d["objectness"]], [torch.from_numpy(x).to(DEV) for x in d["box_regression"]]
    post = RPNPostProcessor(c["pre"], c["post"], c["thr"], c["min_size"], None, c["fpn"]).eval()
    got, want = post(made, obj, reg), post(plain, obj, reg)
    assert len(got) == len(want) == 3 and sum(len(g) for g in got) > 0
    for g, w in zip(got, want):
        assert g.size == w.size and torch.equal(g.bbox, w.bbox) and torch.equal(g.get_field("objectness"), w.get_field("objectness"))


def test_rpn_loss_returns_the_same_bits():
    from rpnloss_cases import RATIOS, SEEDED, load_case
    from veto_amd.rpnloss import make_rpn_loss_evaluator
    from veto_amd.boxhead import BoxCoder
    from veto_amd.config import CfgNode
    z, c, d = load_case("fpn5")
    made, plain = _generated_and_plain(SEEDED["fpn5"]["sizes"], c["strides"], RATIOS, c["grids"], c["images"])
    cfg = CfgNode(MODEL=CfgNode(RPN=CfgNode(FG_IOU_THRESHOLD=c["high"], BG_IOU_THRESHOLD=c["low"], BATCH_SIZE_PER_IMAGE=c["batch"],
                                            POSITIVE_FRACTION=c["fraction"], STRADDLE_THRESH=c["straddle"])))
    loss = make_rpn_loss_evaluator(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)))
    targets = [BoxList(torch.from_numpy(np.asarray(t, np.float32)).to(DEV), size, "xyxy") for t, size in zip(d["tgt_boxes"], c["images"])]
    obj, reg = [torch.from_numpy(x).to(DEV) for x in d["objectness"]], [torch.from_numpy(x).to(DEV) for x in d["box_regression"]]
    got, want = loss(made, obj, reg, targets, seed=11), loss(plain, obj, reg, targets, seed=11)
    assert torch.equal(torch.stack(got), torch.stack(want)) and float(want[0]) > 0 and float(want[1]) > 0
    for g, w in zip(loss.prepare_targets(made, targets), loss.prepare_targets(plain, targets)):
        assert all(torch.equal(x, y) for x, y in zip(g, w))
    # the labels' -1 for anchors outside the image is the visibility the generator hands out
    labels = loss.prepare_targets(made, targets)[0]
    for i, per_img in enumerate(made):
        visible = torch.cat([lvl.get_field("visibility") for lvl in per_img])
        assert (labels[i][~visible] == -1).all() and (~visible).any() and visible.any()


# ---- launches and copies of a forward ---------------------------------------------------------------------------------------------

def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    device = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA]
    copy_like = lambda n: any(s in n for s in ("Memcpy", "memcpy", "Memset", "memset", "Copy"))      # noqa: E731
    ours = [n for n in device if "anchor_grid_kernel" in n]
    other = [n for n in device if "anchor_grid_kernel" not in n and not copy_like(n)]
    memcpy = sum(1 for e in ev if e.name.startswith(("hipMemcpy", "cudaMemcpy")))
    d2h = sum(1 for e in ev if "DtoH" in e.name or "Device -> Host" in e.name or "DeviceToHost" in e.name)
    print("device activities:", device, "| runtime memcpy calls:", memcpy, "| named device->host:", d2h)
    return len(ours), other, memcpy, d2h


def test_launches_and_copies_of_a_forward():
    """Miss: at most 2 kernels; hit: at most 1; no ATen kernel, no device->host copy, at most one copy in all (the image sizes, host->device,
    when they are new)."""
    c = ac.CASES["veto4"]
    gen = _module(c)
    images, maps = _inputs(c)
    gen(*_inputs(c, grids=tuple((h + 1, w) for h, w in c["grids"])))      # warm-up: the code object, the image sizes' table
    ours, other, memcpy, d2h = _profile(lambda: gen(images, maps))                 # a miss with known image sizes
    assert 1 <= ours <= 2 and other == [] and memcpy == 0 and d2h == 0, (ours, other, memcpy, d2h)
    ours, other, memcpy, d2h = _profile(lambda: gen(images, maps))                 # a hit
    assert ours == 1 and other == [] and memcpy == 0 and d2h == 0, (ours, other, memcpy, d2h)
    fresh, _ = _inputs(c, images=((171, 99), (163, 97)))                            # a hit with image sizes never seen: one upload
    ours, other, memcpy, d2h = _profile(lambda: gen(fresh, maps))
    assert ours == 1 and other == [] and memcpy <= 1 and d2h == 0, (ours, other, memcpy, d2h)
    t_neg = _module(c, -1)
    ours, other, memcpy, d2h = _profile(lambda: t_neg(images, maps))               # straddle_thresh < 0: ones, still no ATen kernel
    assert 1 <= ours <= 2 and other == [] and memcpy == 0 and d2h == 0, (ours, other, memcpy, d2h)
