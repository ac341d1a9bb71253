"""Host restatement of the training path's dropout masks (include/veto_amd.h, veto_train_opts_t; veto_amd/csrc/common.h,
dropout_keep; veto_amd/csrc/abi_train.hip, drop_site).  TEST INFRASTRUCTURE ONLY: imported by oracle/train_oracle.py and tests/.

The masks are a counter-based hash of (seed, site, element index), nothing is drawn: element `idx` of a site is kept iff the top
24 bits of splitmix64(site seed + idx * 0x9E3779B97F4A7C15) reach the threshold int(float32(p) * 2^24); kept values are scaled by the
float32 1 / (1 - p).  The reference draws its masks from torch's generator, so these equal its masks in distribution only: what
is restated here is the library's own documented contract, pinned to the device bit for bit by
tests/test_train_scale_gpu.py::test_layernorm_backward_split_form_applies_the_dropout_mask.

Sites and element numbering (the header states them in one place):
  1      Dropout behind the ReLU of pos_embed:  element (n, k) of [n_obj, 128]       -> n * 128 + k
  2      pos_drop on the assembled tokens:      element (row, col) of [n_pair*19, 576] -> row * 576 + col, row = pair * 19 + token
  3 + l  Dropout behind to_out of layer l:      as site 2
"""
import numpy as np
import torch

SITE_STRIDE = 0x632BE59BD9B4E019
SITE_POS, SITE_EMB, SITE_ATTN0 = 1, 2, 3
_M64 = (1 << 64) - 1


def keep_mask(seed, rows, cols, thresh, row0=0, row_step=1):
    """bool [rows, cols]: element (r, c) is element index ((row0 + r) * row_step) * cols + c of the site whose 64-bit seed is `seed`."""
    r = (np.uint64(row0) + np.arange(rows, dtype=np.uint64)) * np.uint64(row_step)
    idx = (r[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]).reshape(-1)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return torch.from_numpy(((z >> np.uint64(40)) >= np.uint64(thresh)).reshape(rows, cols))


def threshold(p):
    """The device's threshold: (unsigned)(p * 16777216.0f) on the float32 p."""
    return int(np.float32(p) * np.float32(16777216.0))


def scale(p):
    """The device's scale: 1.f / (1.f - p) on the float32 p."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


class Dropout:
    """What veto_train_opts_t carries: the three rates and the 64-bit seed.  `site_seeds` / `row_shift` exist for the tests' deliberately
    wrong references only: {site: another step seed for that site alone}, {site: rows by which that site's mask is displaced},
    {site: d} numbers that site by row // d (d = 19: by pair, i.e. by the rows of a compact CLS-row matrix, instead of by token row)."""

    def __init__(self, p_pos=0.0, p_emb=0.0, p_attn=0.0, seed=0, site_seeds=None, row_shift=None, row_div=None):
        self.p_pos, self.p_emb, self.p_attn, self.seed = float(p_pos), float(p_emb), float(p_attn), int(seed)
        self.site_seeds, self.row_shift, self.row_div = dict(site_seeds or {}), dict(row_shift or {}), dict(row_div or {})

    def rate(self, site):
        return self.p_pos if site == SITE_POS else self.p_emb if site == SITE_EMB else self.p_attn

    def site_seed(self, site):
        return (self.site_seeds.get(site, self.seed) + site * SITE_STRIDE) & _M64

    def factor(self, site, rows, cols, dtype, row0=0):
        """keep / (1 - p) of the site for rows row0 .. row0 + rows - 1 as a [rows, cols] tensor, or None where the site is off (p == 0)."""
        p = self.rate(site)
        if not p > 0.0:
            return None
        d = self.row_div.get(site, 1)
        assert rows % d == 0 and row0 % d == 0
        keep = keep_mask(self.site_seed(site), rows // d, cols, threshold(p), row0 // d + self.row_shift.get(site, 0)).repeat_interleave(d, 0)
        return keep.to(dtype) * scale(p)
