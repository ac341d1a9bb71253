"""Writes tests/golden/anchors/*.npz: what the reference's AnchorGenerator (pysgg/modeling/rpn/anchor_generator.py:34-125) returns.

Runs the reference's own AnchorGenerator.forward on the CPU (pysgg, imported with make_golden's stubs) for every case of
tests/anchor_cases.py and stores per case: the cell anchors of every level (`cell_<l>`), the SHA-256 of the anchors of all levels
(`anchor_sha256`) and, per straddle threshold t of the case, the SHA-256 and the dtype of the visibility of all images
(`visibility_sha256_t<t>`, `visibility_dtype_t<t>`).  Small cases also store the arrays themselves (`anchors_<l>` float32
[A H W, 4]; `visibility_t<t>` uint8 [n_img, total], levels concatenated).  It asserts on the way what the device module relies on:
every image's BoxList of a level holds the same tensor object, the fields are bool for t >= 0 and uint8 ones below, and
synth.anchor_grid equals the reference bit for bit.
Usage: python tests/golden/make_golden_anchors.py [case ...]   (no case: all of them)"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference  # noqa: E402
from anchor_cases import CASES, generator_args, np_anchors, sha256  # noqa: E402

OUT = os.path.join(HERE, "anchors")


def run_case(c):
    from pysgg.modeling.rpn.anchor_generator import AnchorGenerator
    z = {}
    sizes, ratios, strides = generator_args(c)
    maps = [torch.zeros(1, 1, h, w) for h, w in c["grids"]]
    images = types.SimpleNamespace(image_sizes=[(h, w) for w, h in c["images"]])
    for t in c["thresholds"]:
        gen = AnchorGenerator(sizes, ratios, strides, t)
        out = gen(images, maps)
        assert len(out) == len(c["images"]) and all(len(per_img) == len(c["grids"]) for per_img in out)
        anchors = [lvl.bbox.numpy() for lvl in out[0]]
        for per_img, size in zip(out, c["images"]):
            for lvl, first in zip(per_img, out[0]):
                assert lvl.bbox is first.bbox and lvl.mode == "xyxy" and tuple(lvl.size) == tuple(size)
                vis = lvl.get_field("visibility")
                assert vis.dtype == (torch.bool if t >= 0 else torch.uint8) and vis.shape == (len(lvl.bbox),)
        plane = np.stack([np.concatenate([lvl.get_field("visibility").numpy().astype(np.uint8) for lvl in per_img]) for per_img in out])
        for a, m in zip(anchors, np_anchors(c)):
            assert a.dtype == np.float32 and np.array_equal(a, m), "synth.anchor_grid differs from the reference's AnchorGenerator"
        z["anchor_sha256"] = np.array(sha256(anchors))
        z["visibility_sha256_t%d" % t] = np.array(sha256([plane]))
        z["visibility_dtype_t%d" % t] = np.array(str(out[0][0].get_field("visibility").dtype))
        for l, cell in enumerate(gen.cell_anchors):
            assert cell.dtype == torch.float32
            z["cell_%d" % l] = cell.numpy()
        if not c.get("big"):
            z["visibility_t%d" % t] = plane
            for l, a in enumerate(anchors):
                z["anchors_%d" % l] = a
    return z


def main():
    import_reference()
    if not hasattr(np, "float"):
        np.float = float   # the reference predates numpy 1.24
    os.makedirs(OUT, exist_ok=True)
    rows = 0
    for name, c in CASES.items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        z = run_case(c)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **z)
        stored = sum(len(v) for k, v in z.items() if k.startswith("anchors_"))
        rows += stored
        print(name, "levels", len(c["grids"]), "anchor rows stored", stored, os.path.getsize(path), "bytes")
    print("anchor rows stored in all:", rows)


if __name__ == "__main__":
    main()
