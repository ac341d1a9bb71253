"""Prints what every veto_*_workspace_bytes that needs no handle (and so no GPU) returns for a fixed list of arguments: non-positive
and one-element sizes, sizes one below and one above a multiple of 64 elements (where the 256-byte rounding of a region changes),
both filter_duplicates forms, 1 and 5 pyramid levels, both forms of veto_debug_wgrad, and optimizer tables whose chunk table ends
on and off a 256-byte boundary.  Two builds of the library lay their workspaces out alike when their outputs are identical:
    VETO_AMD_LIB=<one build> python tools/abi_workspace_sizes.py > a.txt;  VETO_AMD_LIB=<the other> ... > b.txt;  cmp a.txt b.txt"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veto_amd import native  # noqa: E402

SIZES = (-1, 0, 1, 63, 64, 65, 1000)


def rpn_args(n_img, levels, pre_nms_top_n):
    a = native.VetoRpnArgs()
    a.struct_size, a.n_img, a.n_lvl, a.pre_nms_top_n = ctypes.sizeof(a), n_img, len(levels), pre_nms_top_n
    for l, (A, H, W) in enumerate(levels):
        a.level_a[l], a.level_h[l], a.level_w[l] = A, H, W
    return a


def rpn_loss_args(n_img, levels, n_tgt, batch):
    a = native.VetoRpnLossArgs()
    a.struct_size, a.n_img, a.n_lvl, a.n_tgt, a.batch_size_per_image = ctypes.sizeof(a), n_img, len(levels), n_tgt, batch
    for l, (A, H, W) in enumerate(levels):
        a.level_a[l], a.level_h[l], a.level_w[l] = A, H, W
    return a


def box_loss_args(n_rows, n_cls, cls_agnostic):
    a = native.VetoBoxLossArgs()
    a.struct_size, a.n_rows, a.n_cls, a.cls_agnostic = ctypes.sizeof(a), n_rows, n_cls, cls_agnostic
    a.n_reg_cols = 8 if cls_agnostic else 4 * n_cls
    a.ld_logits, a.ld_reg = n_cls, a.n_reg_cols
    return a


def optim_args(numels):
    """One tensor per entry; a negative entry is a tensor of that many elements without a gradient (it takes no chunk)."""
    rows = (native.VetoOptimTensor * max(len(numels), 1))()
    for t, n in zip(rows, numels):
        t.numel, t.grad = abs(n), (256 if n > 0 else None)
    a = native.VetoOptimArgs()
    a.struct_size, a.tensor_size, a.n_tensors = ctypes.sizeof(a), ctypes.sizeof(native.VetoOptimTensor), len(numels)
    a.mode, a.tensors = native.VETO_OPTIM_CLIP_STEP, rows
    return a, rows


LEVELS_1 = [(15, 13, 17)]
LEVELS_5 = [(3, 50, 63), (3, 25, 32), (3, 13, 16), (3, 7, 8), (3, 4, 4)]
C = native.VETO_OPTIM_CHUNK
OPTIM_TABLES = [[], [1], [C], [C + 1], [63, 64, 65], [31 * C], [32 * C], [33 * C], [5, -7, 3 * C + 1, 0, 12 * C],
                [1000] * 31 + [-1000], [1000] * 33, [C + 1] * 100]


def main():
    lib = native.load_library()

    def show(name, args, value=None):
        print("%s(%s) = %d" % (name, ", ".join(str(x) for x in args), getattr(lib, name)(*args) if value is None else value))

    for n in SIZES:
        for name in ("veto_debug_ffn_workspace_bytes", "veto_debug_outproj_workspace_bytes", "veto_debug_layer_tail_workspace_bytes",
                     "veto_debug_qkv_attn_workspace_bytes", "veto_debug_layernorm_backward_workspace_bytes", "veto_ce_loss_workspace_bytes"):
            show(name, (n,))
    for m, n, k in itertools.product((0, 1, 63, 65), (0, 1, 192, 193), (-1, 32, 95, 97)):
        show("veto_debug_gemm_workspace_bytes", (m, n, k))
    for m, n, k, ks in itertools.product((0, 1, 63, 65, 4097), (0, 1, 31, 32, 33, 576), (0, 192, 384), (0, 3)):
        show("veto_debug_wgrad_workspace_bytes", (m, n, k, ks))       # n % 32 == 0 and not
        show("veto_debug_wgrad_ordered_workspace_bytes", (m, n, k, ks))
    for rows, cls in itertools.product(SIZES, (0, 1, 2, 51, 151)):
        show("veto_postprocess_workspace_bytes", (rows, cls))
        show("veto_obj_decode_workspace_bytes", (rows, cls))
        show("veto_detect_relsample_workspace_bytes", (rows, min(cls, 4)))
        for dup in (0, 1):
            show("veto_box_postprocess_workspace_bytes", (rows, cls, dup))
    for n_img, pairs, gts, cls in itertools.product((0, 1, 3), (-1, 0, 1, 63, 65), (0, 1, 63, 65), (1, 2, 51)):
        show("veto_sgg_eval_workspace_bytes", (n_img, pairs, gts, cls))
    for n_img, levels, top_n in itertools.product((0, 1, 3), (LEVELS_1, LEVELS_5), (0, 1, 63, 65, 1000, 6000)):
        a = rpn_args(n_img, levels, top_n)
        show("veto_rpn_proposals_workspace_bytes", (n_img, "%d levels" % len(levels), top_n), lib.veto_rpn_proposals_workspace_bytes(ctypes.byref(a)))
    for n_img, levels, n_tgt, batch in itertools.product((0, 1, 3), (LEVELS_1, LEVELS_5), (-1, 0, 1, 63, 65), (0, 1, 63, 256)):
        a = rpn_loss_args(n_img, levels, n_tgt, batch)
        show("veto_rpn_loss_workspace_bytes", (n_img, "%d levels" % len(levels), n_tgt, batch), lib.veto_rpn_loss_workspace_bytes(ctypes.byref(a)))
    a = rpn_args(1, LEVELS_1, 100)
    a.struct_size -= 8
    show("veto_rpn_proposals_workspace_bytes", ("short struct",), lib.veto_rpn_proposals_workspace_bytes(ctypes.byref(a)))
    a = rpn_loss_args(1, LEVELS_1, 1, 256)
    a.struct_size -= 8
    show("veto_rpn_loss_workspace_bytes", ("short struct",), lib.veto_rpn_loss_workspace_bytes(ctypes.byref(a)))
    for rows, cls, agnostic in itertools.product((-1, 0, 1, 15, 16, 17, 512), (1, 2, 151), (0, 1)):
        a = box_loss_args(rows, cls, agnostic)
        show("veto_box_loss_workspace_bytes", (rows, cls, agnostic), lib.veto_box_loss_workspace_bytes(ctypes.byref(a)))
    for numels in OPTIM_TABLES:
        a, rows = optim_args(numels)
        label = numels if len(numels) < 10 else "%d tensors of %d, ..., %d" % (len(numels), numels[0], numels[-1])
        show("veto_optim_step_workspace_bytes", (label,), lib.veto_optim_step_workspace_bytes(ctypes.byref(a)))


if __name__ == "__main__":
    main()
