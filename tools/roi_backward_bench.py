"""Times the ROI pooling backward at the training shape: 12 images x 36 boxes, 256 channels, 4 pyramid levels of a 1216 x 800 image + the
stride-16 depth map, pooled 8, ratio 2.  Default entry (the caller's zero fill + the atomic scatter) against veto_roi_pool_backward_ordered
(the gather, which writes every element), alternating; profiles/train_deterministic.txt section 3.  usage: tools/roi_backward_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from veto_amd import poolers, synth

dev = torch.device("cuda:0")
W, H, B, C = 1216, 800, 12, 256
rng = np.random.RandomState(5)
boxes = [synth.roi_test_boxes(rng, 36, W, H) for _ in range(B)]
rois = torch.from_numpy(np.concatenate([np.concatenate([np.full((36, 1), i, dtype=np.float32), b], 1) for i, b in enumerate(boxes)])).to(dev)
shapes = [(B, C, H >> (2 + l), W >> (2 + l)) for l in range(4)]
dshape = (B, C, H >> 4, W >> 4)
scales = (0.25, 0.125, 0.0625, 0.03125)
g_rgb = torch.randn(len(rois), C, 8, 8, device=dev)
g_dep = torch.randn(len(rois), C, 8, 8, device=dev)
for ordered in (False, True, False, True):
    for _ in range(3):
        out = poolers._roi_pool_backward(shapes, scales, rois, B, 8, 2, g_rgb, dshape, g_dep, ordered=ordered)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        out = poolers._roi_pool_backward(shapes, scales, rois, B, 8, 2, g_rgb, dshape, g_dep, ordered=ordered)
    b.record()
    torch.cuda.synchronize()
    print("%s entry, map allocation and fill included: %.3f ms per call (map bytes %.2f GB)"
          % ("ordered" if ordered else "default", a.elapsed_time(b) / 10, sum(int(np.prod(s)) for s in shapes + [dshape]) * 4 / 2 ** 30))
    del out
