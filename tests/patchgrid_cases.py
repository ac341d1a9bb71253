"""Cases and float64 restatements for the patch grids (POOLER_RESOLUTION, PATCH_SIZE) = (4, 1), (8, 2), (12, 3), (16, 4): shared by
tests/test_patchgrid_host.py (CPU) and tests/test_patchgrid_gpu.py.

Fixtures: tests/golden/patchgrid/*.npz, written by tests/golden/make_golden_patchgrid.py from the real reference; inputs are
regenerated here from the portable RNG of veto_amd.synth at the matching sizes.

Patch stage.  A patch token of pair (s, o) is  proj(cat(patches(s), patches(o))) + pos_embedding  (model_veto.py:99-113), with the
feature order of einops 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' and the reference's crossed naming: proj_d (512 wide) acts on the
DEPTH maps, proj_v (64 wide) on the RGB maps.  The library computes it per object (subject table with the bias + object table) from
split-bf16 operands in one GEMM of K = 512 p^2 (256 p^2 depth + 256 p^2 rgb features per object row; a table column multiplies
one modality, the other half of its weight row is exact zeros).

Error bound of a table element, derived as tests/prelude_cases.split_gemm_bound derives its own -- operand half steps (the
residuals of the two bf16 splits and the dropped lo x lo product) plus the float32 accumulation of the kept products,
gamma(3 K) sum |a||w| -- with K = 512 p^2, the GEMM's reduction length, in place of the 1024 live k's prelude_cases counts at p = 2.
"""
import os

import numpy as np
import torch

import prelude_cases as pc
from oracle import veto_oracle as vo
from veto_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchgrid")
GRIDS = ((4, 1), (8, 2), (12, 3), (16, 4))            # what the library runs
NEW_GRIDS = ((4, 1), (12, 3), (16, 4))                # ... and what it did not run before
REFUSED = ((8, 4), (8, 1), (16, 2), (7, 2))           # resolution != 4 * patch: another token count
KINDS = ("predcls", "sgcls", "meet")
T = pc.T
U = pc.U


def golden_name(res, patch, kind):
    return "r%dp%d_%s" % (res, patch, kind)


_CACHE = {}


def load(name):
    """(fixture, state dict, batch, OracleConfig, pair lists) of one eval fixture, inputs regenerated at the fixture's patch size"""
    if name in _CACHE:
        return _CACHE[name]
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    patch = int(name[name.index("p") + 1:name.index("_")])
    layers, heads, meet = int(g["layers"]), int(g["heads"]), bool(int(g["meet"]))
    num_objs = [int(x) for x in g["num_objs"]]
    if meet:
        groups = [int(x) for x in g["group_sizes"]]
        sd = synth.meet_state_dict(0, groups, layers=layers, patch=patch)
    else:
        groups = None
        sd = synth.predictor_state_dict(0, layers=layers, patch=patch)
    batch = synth.synthetic_batch(7, len(num_objs), num_objs, patch=patch)
    cfg = vo.OracleConfig(layers=layers, heads=heads, patch=patch, mode=str(g["mode"]), meet_groups=groups, prefix="model." if meet else "")
    counts = [int(x) for x in g["pair_counts"]]
    pairs = np.split(g["pair_idx"], np.cumsum(counts)[:-1])
    _CACHE[name] = (g, sd, batch, cfg, pairs)
    return _CACHE[name]


def golden_logits(g, cfg):
    """[P, num_out]: the vanilla logits, or the MEET groups' side by side in the order of the library's rel_out rows"""
    if cfg.meet_groups is None:
        return g["rel_dists"]
    return np.concatenate([g["rel_group_%d" % k] for k in range(len(cfg.meet_groups))], axis=1)


def train_case():
    """(fixture, state dict, OracleConfig, batch, pair lists) of the (16, 4) training fixture"""
    g = dict(np.load(os.path.join(GOLDEN_DIR, "r16p4_train.npz")))
    layers, heads = int(g["layers"]), int(g["heads"])
    num_objs = [int(x) for x in g["num_objs"]]
    sd = synth.predictor_state_dict(0, layers=layers, patch=4)
    batch = synth.synthetic_batch(7, len(num_objs), num_objs, patch=4)
    cfg = vo.OracleConfig(layers, heads, patch=4, mode=str(g["mode"]))
    return g, sd, cfg, batch, [vo.enumerate_test_pairs(n) for n in num_objs]


# ---- patchify ---------------------------------------------------------------------------------------------------------------------------
def patchify_np(x, p, wrong=()):
    """[N, C, 4p, 4p] -> [N, 16, p p C], feature (p1 p + p2) C + c: 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'.
    wrong: 'c_first' = (c p1 p2) features, 'p_swapped' = (p2 p1 c)."""
    n, c, hh, ww = x.shape
    assert hh == 4 * p and ww == 4 * p
    v = x.reshape(n, c, 4, p, 4, p)                       # n c h p1 w p2
    if "c_first" in wrong:
        return v.transpose(0, 2, 4, 1, 3, 5).reshape(n, 16, c * p * p)
    if "p_swapped" in wrong:
        return v.transpose(0, 2, 4, 5, 3, 1).reshape(n, 16, p * p * c)
    return v.transpose(0, 2, 4, 3, 5, 1).reshape(n, 16, p * p * c)


def split_gemm_bound(A, W, K):
    """prelude_cases.split_gemm_bound with the accumulation length given: K = the reduction length of the device GEMM"""
    aa, aw = np.abs(A), np.abs(W)
    al, wl = pc._hu(aa), pc._hu(aw)
    ra, rw = pc._hu(al), pc._hu(wl)
    fmt = np.concatenate([ra, aa, ra, al], axis=1) @ np.concatenate([aw, rw, rw, wl], axis=1).T
    return fmt + pc.gamma(3 * K) * (aa @ aw.T + fmt)


def patch_tables(sd, batch, p, prefix="", wrong=()):
    """Per-object patch tables in float64 and their bounds: (TS [N, 16, 576] subject half with the bias, TO object half, dTS, dTO);
    columns [depth -> proj_d 512 | rgb -> proj_v 64].  wrong: patchify_np's mistakes, or 'rgb_first' (proj_d on the RGB maps)."""
    t = prefix + T
    dep_map, rgb_map = batch["roi_depth_features"], batch["roi_features"]
    if "rgb_first" in wrong:
        dep_map, rgb_map = rgb_map, dep_map
    F = 256 * p * p
    dep = patchify_np(dep_map.astype(np.float64), p, wrong).reshape(-1, F)
    rgb = patchify_np(rgb_map.astype(np.float64), p, wrong).reshape(-1, F)
    N = dep.shape[0] // 16
    wd = np.asarray(sd[t + "patch_embed.proj_d.weight"], dtype=np.float64).reshape(512, p * p, 2, 256)   # [out, (p1 p2), subject | object, c]
    wv = np.asarray(sd[t + "patch_embed.proj_v.weight"], dtype=np.float64).reshape(64, p * p, 2, 256)
    bias = np.concatenate([np.asarray(sd[t + "patch_embed.proj_d.bias"], dtype=np.float64), np.asarray(sd[t + "patch_embed.proj_v.bias"], dtype=np.float64)])
    tabs, bounds = [], []
    for half in (0, 1):
        Wd, Wv = wd[:, :, half, :].reshape(512, F), wv[:, :, half, :].reshape(64, F)
        tab = np.concatenate([dep @ Wd.T, rgb @ Wv.T], axis=1)
        d = np.concatenate([split_gemm_bound(dep, Wd, 2 * F), split_gemm_bound(rgb, Wv, 2 * F)], axis=1)
        if half == 0:
            tab = tab + bias
            d = d + U * np.abs(tab)                                     # the bias add of the GEMM epilogue
        tabs.append(tab.reshape(N, 16, pc.DIM))
        bounds.append(d.reshape(N, 16, pc.DIM))
    return tabs[0], tabs[1], bounds[0], bounds[1]


def patch_tokens(sd, batch, pairs, p, prefix="", wrong=()):
    """(tokens 1..16 of every pair [P, 16, 576] float64, their bound) in the library's per-object form, as prelude_cases.restate"""
    subj, obj = vo.build_pair_indices(pairs, batch["num_objs"])
    TS, TO, dTS, dTO = patch_tables(sd, batch, p, prefix, wrong)
    pe = np.asarray(sd[prefix + T + "pos_embedding"], dtype=np.float64).reshape(pc.DIM)
    pre = TS[subj] + TO[obj]
    dpre = dTS[subj] + dTO[obj]
    dpre = dpre + U * (np.abs(pre) + dpre)
    return pre + pe, dpre + U * (np.abs(pre + pe) + dpre)


def oracle_patch_tokens(sd, cfg, batch, pairs, dtype=torch.float64):
    """oracle/veto_oracle.py's own token rows 1..16 (per pair, the reference's form)"""
    _, _, _, inter = vo.forward(sd, cfg, batch, rel_pair_idxs=pairs, dtype=dtype, return_intermediates=True)
    return inter["tokens"][:, 1:17].numpy()
