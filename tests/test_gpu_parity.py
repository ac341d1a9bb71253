"""Parity tests proper: the HIP path, called through the C ABI, against (1) the golden outputs of
the real reference, (2) the CPU oracle on other seeded inputs, (3) size-independent properties at
BASELINE.json's full size.  Tolerance: 1e-3 max-abs on fp32 logits (north_star), pair indexing
bit-exact."""
import numpy as np
import pytest
import torch

from conftest import (golden_names, golden_pairs, load_golden, load_post_golden, load_postmeet_golden, load_postvote_golden,
                      post_golden_names, postmeet_golden_names, postvote_golden_names)

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(model, batch, mode, device, pairs=None, debug=False):
    from veto_amd import testing
    from veto_amd.pairs import prepare_test_pairs
    props = testing.make_proposals(batch, mode, device)
    if pairs is None:
        pairs = prepare_test_pairs(device, props)
    rgb = torch.from_numpy(batch["roi_features"]).to(device)
    dep = torch.from_numpy(batch["roi_depth_features"]).to(device)
    model.debug_outputs = debug
    with torch.no_grad():
        out = model(props, pairs, None, None, roi_features=rgb, roi_depth_features=dep)
    torch.cuda.synchronize()
    return out, pairs


# ---------------------------------------------------------------------------------------------------
def test_library_loaded_is_in_tree():
    from veto_amd import native
    lib = native.load_library()
    assert native.library_path().endswith("veto_amd/csrc/libveto_amd.so")
    assert b"gfx950" in lib.veto_version()


@pytest.mark.parametrize("m,n,k", [(256, 192, 32), (300, 384, 576), (1000, 1728, 576), (777, 576, 1152),
                                   (6912, 1152, 2048)])
def test_split_gemm_against_fp64(m, n, k):
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).to(dev)
    w = torch.randn(n, k, generator=g).to(dev)
    bias = torch.randn(n, generator=g).to(dev)
    ref = (a.double() @ w.double().t() + bias.double())
    ws = torch.empty(lib.veto_debug_gemm_workspace_bytes(m, n, k), dtype=torch.uint8, device=dev)
    for precision, tol in ((native.VETO_PRECISE, 3e-5), (native.VETO_MIXED, 1.5e-5), (native.VETO_FAST, 2e-2)):
        if precision == native.VETO_MIXED and k % 64 != 0:
            continue   # mixed rows come in blocks of 64 k's
        c = torch.full((m, n), float("nan"), device=dev)
        native.check(lib.veto_debug_gemm(None, a.data_ptr(), w.data_ptr(), bias.data_ptr(), c.data_ptr(), m, n, k,
                                         precision, ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        # error relative to sum_k |a||w| (the natural scale of a rounded dot product)
        scale = (a.abs().double() @ w.abs().double().t()).clamp_min(1e-6)
        rel = ((c.double() - ref).abs() / scale).max().item()
        assert rel < tol, (m, n, k, precision, rel)


def test_mixed_gemm_saturates_gracefully_on_outliers():
    """The e4m3 correction planes of the mixed format clamp instead of overflowing (v_cvt_pk_fp8_f32 itself would produce NaN
    above 448): activations far outside the fixed scaling range (|a| > 28) and a weight tensor whose exponent is set by one
    huge entry must give finite results whose error is that of the fp16 main product at worst (2^-11 relative), and the
    well-scaled rows of the same call keep the full 2^-16 class."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    m, n, k = 512, 384, 576
    g = torch.Generator(device="cpu").manual_seed(5)
    a = torch.randn(m, k, generator=g)
    a[7] *= 300.0                      # one row of large activations
    a[100, 13] = 6.0e4                 # near the fp16 maximum
    w = torch.randn(n, k, generator=g) * 0.04
    w[3, 5] = 3.0                      # sets the tensor's e4m3 exponent: every other weight then uses few e4m3 bits
    a, w = a.to(dev), w.to(dev)
    ref = a.double() @ w.double().t()
    scale = (a.abs().double() @ w.abs().double().t()).clamp_min(1e-6)
    ws = torch.empty(lib.veto_debug_gemm_workspace_bytes(m, n, k), dtype=torch.uint8, device=dev)
    c = torch.full((m, n), float("nan"), device=dev)
    native.check(lib.veto_debug_gemm(None, a.data_ptr(), w.data_ptr(), None, c.data_ptr(), m, n, k, native.VETO_MIXED, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    assert torch.isfinite(c).all()
    rel = (c.double() - ref).abs() / scale
    assert rel.max().item() < 2.0 ** -10, rel.max().item()
    ok = torch.ones(m, dtype=torch.bool, device=dev)
    ok[7] = ok[100] = False
    assert rel[ok].max().item() < 2e-4, rel[ok].max().item()       # (the coarse weight exponent costs correction bits, not the main term)


@pytest.mark.parametrize("m", [1, 127, 128, 129, 1000, 33000])
def test_fused_feedforward_matches_two_launch_form_and_fp64(m):
    """The fused FeedForward kernel (ffn_fused.hip: fc1 -> GELU -> fc2 + residual, hidden activation kept on the CU;
    model_veto.py:137-143 + the residual of :21) against an fp64 reference and against the two-launch form (same operands and
    summation order; the compiler contracts x * sigmoid(g(x)) into the fp16 conversion differently in the two kernels, so the
    two agree to the rounding of the hidden activation, not bit for bit): panel edges (127 / 128 / 129 rows), a single row, and
    more panels than CUs.  Row r of the result must not depend on the rows around it: the first rows of the 33 000-row
    call equal the 1 000-row call of the same data bit for bit."""
    import ctypes
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m)
    a = torch.randn(m, 576, generator=g).to(dev)
    x0 = torch.randn(m, 576, generator=g).to(dev)
    w1 = (torch.randn(1152, 576, generator=g) * 0.04).to(dev)
    b1 = (torch.randn(1152, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(576, 1152, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(576, generator=g) * 0.1).to(dev)
    hid = torch.nn.functional.gelu(a.double() @ w1.double().t() + b1.double())
    ref = x0.double() + hid @ w2.double().t() + b2.double()
    scale = (hid.abs() @ w2.double().abs().t()).clamp_min(1e-6)
    ws = torch.empty(lib.veto_debug_ffn_workspace_bytes(m), dtype=torch.uint8, device=dev)
    out = []
    for mode in (0, 1):
        x = x0.clone()
        native.check(lib.veto_debug_ffn(None, a.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), x.data_ptr(),
                                        m, mode, 1, 1, None, ws.data_ptr(), ws.numel(), None, None, None))
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
        rel = ((x.double() - ref).abs() / scale).max().item()
        assert rel < 1e-4, (m, mode, rel)     # the hidden activation is rounded to 2^-16 on its way into fc2
        out.append(x)
    assert ((out[0].double() - out[1].double()).abs() / scale).max().item() < 1e-4
    if m > 1000:   # batch invariance of the fused kernel: the same rows inside a smaller call
        k = 1000
        xs = x0[:k].clone()
        ws2 = torch.empty(lib.veto_debug_ffn_workspace_bytes(k), dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_ffn(None, a[:k].contiguous().data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                        xs.data_ptr(), k, 1, 1, 1, None, ws2.data_ptr(), ws2.numel(), None, None, None))
        torch.cuda.synchronize()
        assert torch.equal(xs, out[1][:k])


def _decode_mixed_rows(raw, k):
    """[rows, 4k] uint8 mixed ACTIVATION rows (veto_amd/csrc/common.h) -> (h fp16 plane, h + X * 2^-11, Y) as float64 [rows, k]."""
    rows = raw.shape[0]
    blk = raw.reshape(rows, k // 64, 256)
    h = blk[:, :, :128].contiguous().view(torch.float16).reshape(rows, k).double()
    grp = blk[:, :, 128:].reshape(rows, k // 64, 16, 8)
    x = grp[..., :4].contiguous().view(torch.float8_e4m3fn).double().reshape(rows, k)
    y = grp[..., 4:].contiguous().view(torch.float8_e4m3fn).double().reshape(rows, k)
    return h, h + x * 2.0 ** -11, y


@pytest.mark.parametrize("m", [129, 5000])
def test_fused_feedforward_layernorm_epilogue(m):
    """The next layer's LayerNorm written by the fused FeedForward epilogue as mixed rows (model_veto.py:125-132 behind :137-143):
    the rows are decoded plane by plane -- fp16 value, e4m3 residual (2^11), e4m3 value -- and compared with the LayerNorm of the
    kernel's own fp32 result, and with the rows a LayerNorm launch writes behind the two-launch form."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m)
    a = torch.randn(m, 576, generator=g).to(dev)
    x0 = (torch.randn(m, 576, generator=g) + 0.7).to(dev)          # a row mean away from zero
    w1 = (torch.randn(1152, 576, generator=g) * 0.04).to(dev)
    b1 = (torch.randn(1152, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(576, 1152, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(576, generator=g) * 0.1).to(dev)
    lw = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev)
    lb = (0.2 * torch.randn(576, generator=g)).to(dev)
    ws = torch.empty(lib.veto_debug_ffn_workspace_bytes(m), dtype=torch.uint8, device=dev)
    planes = []
    for mode in (0, 1):
        x = x0.clone()
        rows = torch.zeros(m, 4 * 576, dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_ffn(None, a.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), x.data_ptr(),
                                        m, mode, 1, 1, None, ws.data_ptr(), ws.numel(), lw.data_ptr(), lb.data_ptr(), rows.data_ptr()))
        torch.cuda.synchronize()
        ref = torch.nn.functional.layer_norm(x.double(), (576,), lw.double(), lb.double(), 1e-5)
        h, hx, y = _decode_mixed_rows(rows, 576)
        assert (h - ref).abs().max().item() <= 2.0 ** -11 * ref.abs().max().item() * 1.01 + 1e-6, mode      # fp16 plane
        assert ((hx - ref).abs() / ref.abs().clamp_min(0.05)).max().item() < 2.0 ** -14, mode                # + e4m3 residual
        assert ((y - ref).abs() / ref.abs().clamp_min(0.05)).max().item() < 2.0 ** -3, mode                  # e4m3 value (4 bits)
        planes.append(hx)
    assert (planes[0] - planes[1]).abs().max().item() < 2e-4


@pytest.mark.parametrize("m", [1, 129, 5000, 40000])
def test_fused_out_projection_residual_layernorm(m):
    """The attention out projection + residual (+ the FeedForward PreNorm as mixed rows) on the full-row panel kernel
    (ffn_fused.hip MODE 1; model_veto.py:96, :20, :125-132) against fp64 and against the GEMM launch + LayerNorm launch."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m + 7)
    a = torch.randn(m, 576, generator=g).to(dev)
    x0 = (torch.randn(m, 576, generator=g) - 0.4).to(dev)
    w = (torch.randn(576, 576, generator=g) * 0.05).to(dev)
    b = (torch.randn(576, generator=g) * 0.1).to(dev)
    lw = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev)
    lb = (0.2 * torch.randn(576, generator=g)).to(dev)
    ref = x0.double() + a.double() @ w.double().t() + b.double()
    scale = (a.abs().double() @ w.abs().double().t()).clamp_min(1e-6)
    ws = torch.empty(lib.veto_debug_outproj_workspace_bytes(m), dtype=torch.uint8, device=dev)
    xs, planes = [], []
    for mode in (0, 1):
        x = x0.clone()
        rows = torch.zeros(m, 4 * 576, dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_outproj(None, a.data_ptr(), w.data_ptr(), b.data_ptr(), x.data_ptr(), m, mode, 1, 1, None,
                                            ws.data_ptr(), ws.numel(), lw.data_ptr(), lb.data_ptr(), rows.data_ptr()))
        torch.cuda.synchronize()
        assert ((x.double() - ref).abs() / scale).max().item() < 1.5e-5, mode
        lnref = torch.nn.functional.layer_norm(x.double(), (576,), lw.double(), lb.double(), 1e-5)
        h, hx, y = _decode_mixed_rows(rows, 576)
        assert ((hx - lnref).abs() / lnref.abs().clamp_min(0.05)).max().item() < 2.0 ** -14, mode
        xs.append(x)
        planes.append(hx)
    # same operands and k order; the panel kernel starts its accumulators at the residual row where the GEMM launch adds it last:
    # the two differ by fp32 roundings of the sum
    assert ((xs[0] - xs[1]).abs() / (xs[0].abs() + scale.float())).max().item() < 2e-6
    assert (planes[0] - planes[1]).abs().max().item() < 2e-4


@pytest.mark.parametrize("m", [1, 129, 5000, 40000])
def test_fused_layer_tail(m):
    """Everything of a layer behind its attention in one launch (ffn_fused.hip MODE 2: out projection + residual + LayerNorm2 +
    FeedForward + residual + the next LayerNorm; model_veto.py:96, :20-21, :125-143) against fp64 and against the two panel launches
    it replaces.  The LayerNorm2 rows are written and re-read by the same CU within the launch (L1 invalidate in between): 40 000
    rows = more panels than CUs, so every workgroup goes through that hand-off several times."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m + 11)
    a = torch.randn(m, 576, generator=g).to(dev)
    x0 = (torch.randn(m, 576, generator=g) + 0.3).to(dev)
    wo = (torch.randn(576, 576, generator=g) * 0.05).to(dev)
    bo = (torch.randn(576, generator=g) * 0.1).to(dev)
    l2w = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev)
    l2b = (0.2 * torch.randn(576, generator=g)).to(dev)
    w1 = (torch.randn(1152, 576, generator=g) * 0.04).to(dev)
    b1 = (torch.randn(1152, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(576, 1152, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(576, generator=g) * 0.1).to(dev)
    lw = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev)
    lb = (0.2 * torch.randn(576, generator=g)).to(dev)
    x1 = x0.double() + a.double() @ wo.double().t() + bo.double()
    hin = torch.nn.functional.layer_norm(x1, (576,), l2w.double(), l2b.double(), 1e-5)
    ref = x1 + torch.nn.functional.gelu(hin @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
    ws = torch.empty(lib.veto_debug_layer_tail_workspace_bytes(m), dtype=torch.uint8, device=dev)
    xs, planes = [], []
    for mode in (0, 1):
        x = x0.clone()
        rows = torch.zeros(m, 4 * 576, dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_layer_tail(None, a.data_ptr(), wo.data_ptr(), bo.data_ptr(), l2w.data_ptr(), l2b.data_ptr(), w1.data_ptr(),
                                               b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), x.data_ptr(), m, mode, 1, None, ws.data_ptr(),
                                               ws.numel(), lw.data_ptr(), lb.data_ptr(), rows.data_ptr()))
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
        err = (x.double() - ref).abs().max().item()
        assert err < 3e-4, (m, mode, err)
        lnref = torch.nn.functional.layer_norm(x.double(), (576,), lw.double(), lb.double(), 1e-5)
        h, hx, y = _decode_mixed_rows(rows, 576)
        assert ((hx - lnref).abs() / lnref.abs().clamp_min(0.05)).max().item() < 2.0 ** -14, mode
        xs.append(x)
    assert (xs[0] - xs[1]).abs().max().item() < 3e-4


def _attention_fp64(a, wqkv, n_pair, heads):
    """model_veto.py:85-96 on LayerNorm'ed rows a [19 n_pair, 576], fp64."""
    dh = 576 // heads
    qkv = (a.double() @ wqkv.double().t()).reshape(n_pair, 19, 3, heads, dh)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))            # [pair, head, token, dh]
    att = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
    return (att @ v).permute(0, 2, 1, 3).reshape(n_pair * 19, 576)


@pytest.mark.parametrize("heads", [8, 6])
@pytest.mark.parametrize("n_pair,sharp", [(1, 1.0), (16, 1.0), (37, 3.0), (1260, 1.0), (4099, 2.0)])
def test_fused_qkv_attention(n_pair, sharp, heads):
    """QKV projection + per-pair attention in one launch (qkv_attn_fused.hip; model_veto.py:78-96) against fp64 and against the two
    launches it replaces, on pair counts that leave partial 16-pair tiles, fewer tiles than workgroups and several tiles per
    workgroup; `sharp` scales q and k so that the softmax is far from uniform (scores of +-30)."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(n_pair * 10 + heads)
    m = n_pair * 19
    a = torch.randn(m, 576, generator=g).to(dev)
    wqkv = (torch.randn(1728, 576, generator=g) * 0.05)
    wqkv[:1152] *= sharp
    wqkv = wqkv.to(dev)
    ref = _attention_fp64(a, wqkv, n_pair, heads)
    ws = torch.empty(lib.veto_debug_qkv_attn_workspace_bytes(n_pair), dtype=torch.uint8, device=dev)
    outs, errs = [], []
    for mode in (1, 0):
        rows = torch.zeros(m, 4 * 576, dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_qkv_attn(None, a.data_ptr(), wqkv.data_ptr(), n_pair, heads, mode, 1, None, ws.data_ptr(), ws.numel(),
                                             rows.data_ptr()))
        torch.cuda.synchronize()
        h, hx, y = _decode_mixed_rows(rows, 576)
        assert torch.isfinite(hx).all()
        errs.append((hx - ref).abs().max().item())
        outs.append(hx)
    # a score carries the 2^-16 of its operands times sum |q||k|, so the error grows with the sharpness: the bar is the plain case's,
    # scaled, and the two-launch form's own error (the fused form keeps q / k / v in fp32 up to the bf16 hi / lo split, the two-launch
    # form rounds them to 3-byte floats first: the fused form is the more accurate of the two)
    bar = 2e-4 * sharp ** 2 * max(1.0, ref.abs().max().item())
    assert errs[0] < bar and errs[0] < 1.5 * errs[1] + 2e-5, (n_pair, heads, errs)
    assert (outs[0] - outs[1]).abs().max().item() < 2 * bar


@pytest.mark.parametrize("m,n,k,kb_tiles,kb_steps", [(1000, 576, 576, 0, 0), (5000, 4608, 768, 3, 3), (3000, 768, 4608, 1, 36),
                                                      (300, 1152, 192, 2, 2)])
def test_gemm_block_diagonal_and_output_forms(m, n, k, kb_tiles, kb_steps):
    """The round-3 forms of the split-row GEMM (veto_debug_gemm_forms): block-diagonal weights -- column tile j multiplies only the
    k-steps of its block, the rest of w (here: garbage) is ignored -- and the split-row / 3-byte-float epilogues, against fp64.
    The second and third shapes are the two block products of the folded last layer (abi_forward.hip)."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(m + n)
    a = torch.randn(m, k, generator=g).to(dev)
    w = (torch.randn(n, k, generator=g) * 0.05).to(dev)
    wd = w.double()
    if kb_tiles:        # the reference multiplies by the block-diagonal part only; the kernel must never read the rest
        mask = torch.zeros(n, k, dtype=torch.bool, device=dev)
        for j in range(n // 192):
            k0 = (j // kb_tiles) * kb_steps * 32
            mask[j * 192:(j + 1) * 192, k0:k0 + kb_steps * 32] = True
        wd = wd * mask
        w = torch.where(mask, w, torch.full_like(w, float("nan")))
    ref = a.double() @ wd.t()
    scale = (a.abs().double() @ wd.abs().t()).clamp_min(1e-6)
    ws = torch.empty(lib.veto_debug_gemm_workspace_bytes(m, n, k), dtype=torch.uint8, device=dev)

    def run(form, out):
        native.check(lib.veto_debug_gemm_forms(None, a.data_ptr(), w.data_ptr(), out.data_ptr(), m, n, k, kb_tiles, kb_steps, form,
                                               ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()

    c = torch.full((m, n), float("nan"), device=dev)
    run(0, c)
    assert torch.isfinite(c).all()
    assert ((c.double() - ref).abs() / scale).max().item() < 2e-5
    sp = torch.zeros(m, 2 * n, dtype=torch.bfloat16, device=dev)
    run(1, sp)
    sp = sp.view(m, n // 32, 2, 32).double()
    dec = (sp[:, :, 0] + sp[:, :, 1]).reshape(m, n)                      # hi + lo: a 16-bit significand of the fp32 result
    assert ((dec - c.double()).abs() / c.abs().double().clamp_min(1e-20)).max().item() < 2.0 ** -16
    f24 = torch.zeros(m, 3 * n, dtype=torch.uint8, device=dev)
    run(2, f24)
    b = f24.view(m, n, 3).to(torch.int32)
    bits = (b[:, :, 0] << 8) | (b[:, :, 1] << 16) | (b[:, :, 2] << 24)
    dec24 = bits.view(torch.float32)
    rel = ((dec24.double() - c.double()).abs() / c.abs().double().clamp_min(1e-20)).max().item()
    assert rel <= 2.0 ** -16, rel                                        # round to nearest at 16 significand bits
    assert ((dec24.view(torch.int32) & 0xFF) == 0).all()
    if kb_tiles == 0:
        # non-finite results keep their class in the 3-byte form: Inf stays Inf of its sign, a NaN stays a NaN (the rounding increment
        # must not carry a NaN's mantissa into the exponent: it would be stored as +-0)
        a2 = a.clone()
        a2[0, 0], a2[1, 0], a2[2, 0] = float("inf"), float("-inf"), float("nan")
        w2 = w.clone()
        w2[:, 0] = w2[:, 0].abs() + 0.01
        native.check(lib.veto_debug_gemm_forms(None, a2.data_ptr(), w2.data_ptr(), f24.data_ptr(), m, n, k, 0, 0, 2, ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        b = f24.view(m, n, 3).to(torch.int32)
        d = ((b[:, :, 0] << 8) | (b[:, :, 1] << 16) | (b[:, :, 2] << 24)).view(torch.float32)
        assert torch.isnan(d[2]).all() and torch.isfinite(d[3:]).all()
        # (an Inf operand goes through the split-bf16 terms as Inf - Inf in the low plane: NaN or Inf, never a finite value)
        assert (~torch.isfinite(d[0])).all() and (~torch.isfinite(d[1])).all()


def test_fused_layer_tail_full_size_hand_off():
    """The layer-tail kernel at the headline size (287 280 rows: nine panels per workgroup, every CU streaming): the LayerNorm2
    rows a workgroup writes and re-reads within the launch must be the fresh ones in EVERY row (an L1 line of the rows they replace
    would be a stale hit), launch after launch.  Checked word by word against the two panel launches (which pass the rows through
    a kernel boundary), three times."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    m = 287280
    g = torch.Generator(device="cpu").manual_seed(99)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(dev)
    a, x0 = mk(m, 576), mk(m, 576)
    wo, bo = mk(576, 576, s=0.05), mk(576, s=0.1)
    l2w, l2b = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev), mk(576, s=0.2)
    w1, b1, w2, b2 = mk(1152, 576, s=0.04), mk(1152, s=0.1), mk(576, 1152, s=0.03), mk(576, s=0.1)
    lw, lb = (1.0 + 0.3 * torch.randn(576, generator=g)).to(dev), mk(576, s=0.2)
    ws = torch.empty(lib.veto_debug_layer_tail_workspace_bytes(m), dtype=torch.uint8, device=dev)

    def run(mode):
        x = x0.clone()
        rows = torch.zeros(m, 4 * 576, dtype=torch.uint8, device=dev)
        native.check(lib.veto_debug_layer_tail(None, a.data_ptr(), wo.data_ptr(), bo.data_ptr(), l2w.data_ptr(), l2b.data_ptr(), w1.data_ptr(),
                                               b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), x.data_ptr(), m, mode, 1, None, ws.data_ptr(),
                                               ws.numel(), lw.data_ptr(), lb.data_ptr(), rows.data_ptr()))
        torch.cuda.synchronize()
        return x, rows

    ref_x, ref_rows = run(0)
    first = None
    for rep in range(3):
        x, rows = run(1)
        assert torch.isfinite(x).all()
        assert (x - ref_x).abs().max().item() < 3e-4, rep          # a stale LayerNorm2 row would be off by O(1)
        if first is None:
            first = (x, rows)
        else:
            assert torch.equal(x, first[0]) and torch.equal(rows, first[1])     # and the launch is deterministic


@pytest.mark.parametrize("n", [1, 2, 3, 10, 36, 50])
def test_enumerate_pairs_bit_exact(n):
    from veto_amd.pairs import prepare_test_pairs
    from veto_amd.structures import BoxList
    dev = _dev()
    p = BoxList(torch.zeros(n, 4), (800, 600))
    p.add_field("pred_scores", torch.linspace(1.0, 0.1, n))
    got = prepare_test_pairs(dev, [p])[0].cpu()
    cand = torch.ones((n, n)) - torch.eye(n)
    ref = torch.nonzero(cand).view(-1, 2)
    if len(ref) == 0:
        ref = torch.zeros((1, 2), dtype=torch.int64)
    if len(ref) > 2048:
        # sampling.py:41-45: top MAX_PROPOSAL_PAIR by score product; ties ((i,j) vs (j,i)) may be
        # ordered differently by a device sort, so compare the selected score multiset
        q = p.get_field("pred_scores")
        sel = lambda idx: torch.sort(q[idx[:, 0]] * q[idx[:, 1]], descending=True)[0]
        assert got.shape == (2048, 2)
        assert torch.equal(sel(got), sel(ref)[:2048])
    else:
        assert torch.equal(got, ref)


@pytest.mark.parametrize("precision", ["mixed", "precise"])
@pytest.mark.parametrize("name", golden_names())
def test_golden_parity(name, precision):
    """HIP path vs the committed outputs of the real reference, in both parity-grade precision modes; the fixtures include the
    full-size workloads: sgcls 12 x 36 (cfg-4 per GPU), L6/H6 12 x 36, MEET VG / GQA at 36 objects, a ragged 12-image batch with
    1..64 objects and the reference's own 2048-pair cap."""
    from veto_amd import testing
    dev = _dev()
    g, sd, batch = load_golden(name)
    meet, mode = bool(int(g["meet"])), str(g["mode"])
    cfg = testing.make_config(g["_layers"], g["_heads"], mode, meet, str(g["dataset"]), precision=precision)
    experts = bool(int(g.get("experts", 0)))
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = experts
    model = testing.make_predictor(cfg, sd, dev)
    given = [torch.from_numpy(p).to(dev) for p in golden_pairs(g)] if int(g["capped_pairs"]) else None
    out, pairs = _run(model, batch, mode, dev, pairs=given, debug=True)
    assert np.array_equal(torch.cat(pairs).cpu().numpy(), g["pair_idx"])
    obj_dists, rel = out[0], out[1]
    assert np.array_equal(torch.cat([o.argmax(1) for o in obj_dists]).cpu().numpy(), g["obj_dists_argmax"])
    assert [tuple(o.shape) for o in obj_dists] == [(n, g["_n_obj"]) for n in batch["num_objs"]]
    if meet:
        assert out[3] == [int(x) for x in g["incre_idx_list"]]
        keys = ["group_%d%d" % (k, e) for k in range(len(g["group_sizes"])) for e in (1, 2, 3)] if experts \
            else ["group_%d" % k for k in range(len(g["group_sizes"]))]
        assert sorted(rel.keys()) == sorted(keys)
        for k in keys:
            err = np.abs(rel[k].cpu().numpy() - g["rel_" + k]).max()
            assert err <= LOGIT_TOL, (name, k, err)
    else:
        assert out[2] == {} and out[3] is None and out[4] is None and out[5] is None
        got = torch.cat(list(rel)).cpu().numpy()
        assert [r.shape[0] for r in rel] == [int(x) for x in g["pair_counts"]]
        if not int(g["capped_pairs"]):
            assert [r.shape[0] for r in rel] == [max(n * (n - 1), 1) for n in batch["num_objs"]]
        err = np.abs(got - g["rel_dists"]).max()
        print("%s [%s]: logit max-abs-err %.3e" % (name, precision, err))
        assert err <= LOGIT_TOL, (name, err)
        assert err <= 3e-4, (name, err)     # the margin both modes are expected to keep (measured: 2-3e-5 / 4-9e-5)
        step = int(g["tokens_step"])
        tok = model.last_debug["tokens"][::step, :, ::9].cpu().numpy()
        assert np.abs(tok - g["tokens_sample"]).max() <= 2e-4
        assert (got.argmax(1) == g["rel_dists"].argmax(1)).mean() > 0.99


@pytest.mark.parametrize("layers,heads,num_objs,relu_like", [(2, 8, [7, 12], True), (3, 6, [9, 4, 1, 6], False),
                                                             (1, 8, [5], False), (2, 4, [6, 6], False), (2, 12, [5, 8], False)])
def test_oracle_parity_other_inputs(layers, heads, num_objs, relu_like):
    """HIP path vs the CPU oracle on inputs no golden covers (other seeds, ragged batches, L=1; 12 heads: the block form of the
    folded last layer at the padded head width 64, 4 heads: its product form)."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    dev = _dev()
    sd = synth.predictor_state_dict(3, layers=layers)
    batch = synth.synthetic_batch(11, len(num_objs), num_objs, relu_like=relu_like)
    cfg = testing.make_config(layers, heads)
    model = testing.make_predictor(cfg, sd, dev)
    out, pairs = _run(model, batch, "predcls", dev, debug=True)
    ref, subj, obj, inter = vo.forward(sd, vo.OracleConfig(layers=layers, heads=heads), batch,
                                       return_intermediates=True)
    assert np.array_equal(model.last_debug["subj_inds"].cpu().numpy(), subj)
    assert np.array_equal(model.last_debug["obj_inds"].cpu().numpy(), obj)
    tok_err = (model.last_debug["tokens"].cpu() - inter["tokens"]).abs().max().item()
    assert tok_err <= 2e-4, tok_err
    cls_err = (model.last_debug["cls"].cpu() - inter["cls"]).abs().max().item()
    err = (torch.cat(list(out[1])).cpu() - ref).abs().max().item()
    print("L%d H%d: tokens %.2e cls %.2e logits %.2e" % (layers, heads, tok_err, cls_err, err))
    assert err <= LOGIT_TOL, err
    # The classifier's input, against the float64 oracle.  Yardstick: the float32 oracle's own error against the float64 one on this
    # case (what the L layers cost in plain float32).  The device multiplies operands of a 2^-16-class format (fp16 + e4m3 residual:
    # a 16-bit significand) where the float32 oracle multiplies 2^-24 ones, and both accumulate in float32 over the same reductions,
    # so the factor allowed is the ratio of the two formats' steps, 2^(24 - 16) = 256, not the 4 of a float32 kernel; the floor is 4
    # float32 ulps of the largest element.
    _, _, _, inter64 = vo.forward(sd, vo.OracleConfig(layers=layers, heads=heads), batch, dtype=torch.float64, return_intermediates=True)
    yard = (inter["cls"].double() - inter64["cls"]).abs().max().item()
    cls_err64 = (model.last_debug["cls"].cpu().double() - inter64["cls"]).abs().max().item()
    allowed = 256 * yard + 4 * 2.0 ** -23 * inter64["cls"].abs().max().item()
    print("L%d H%d: cls against float64 %.2e, float32 oracle %.2e, allowed %.2e" % (layers, heads, cls_err64, yard, allowed))
    assert cls_err64 <= allowed, (cls_err64, yard)


@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_parity_under_sharp_attention(precision):
    """The random-init fixtures have nearly uniform attention (mean max-probability of a softmax row 0.07), which hides errors
    in the q / k path.  With the q and k rows of every to_qkv weight scaled by 5 the softmax is as sharp as a trained one (0.70);
    the HIP path must still sit well inside the tolerance against the fp64 oracle (tools/precision_study.py --sharp shows that
    fp16 storage of q / k would not: 1.4e-3)."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    dev = _dev()
    layers, heads = 4, 8
    sd = dict(synth.predictor_state_dict(0, layers=layers))
    for l in range(layers):
        k = "fusion_transformer.transformer.layers.%d.0.fn.to_qkv.weight" % l
        w = np.array(sd[k]).copy()
        w[:2 * 576] *= 5.0
        sd[k] = w
    batch = synth.synthetic_batch(7, 2, [12, 9])
    model = testing.make_predictor(testing.make_config(layers, heads, precision=precision), sd, dev)
    out, _ = _run(model, batch, "predcls", dev)
    ref, _, _ = vo.forward(sd, vo.OracleConfig(layers=layers, heads=heads), batch, dtype=torch.float64)
    err = (torch.cat(list(out[1])).cpu().double() - ref).abs().max().item()
    print("sharp attention [%s]: logit max-abs-err %.3e" % (precision, err))
    assert err <= 3e-4, err


def _trained_like_state_dict(layers, hidden_factor=300.0):
    """The synthetic weights re-parameterised the way training leaves a transformer (same function): LayerNorm gains x 8 with shifted
    biases, 3 % of the hidden units x 30 and six x `hidden_factor`, one outlier entry per Linear weight."""
    from veto_amd import synth
    sd = {k: np.array(v).copy() for k, v in synth.predictor_state_dict(0, layers=layers).items()}
    rng = np.random.RandomState(3)
    T = "fusion_transformer.transformer.layers.%d."
    for l in range(layers):
        for norm, lin in (("0.norm", "0.fn.to_qkv"), ("1.norm", "1.fn.net.0")):
            sd[(T % l) + norm + ".weight"] *= 8.0
            sd[(T % l) + norm + ".bias"] += 3.0 * rng.randn(576).astype(np.float32)
            sd[(T % l) + lin + ".weight"] /= 8.0
        w1, b1, w2 = (T % l) + "1.fn.net.0.weight", (T % l) + "1.fn.net.0.bias", (T % l) + "1.fn.net.3.weight"
        units = rng.permutation(1152)
        for sel, f in ((units[:35], 30.0), (units[35:41], hidden_factor)):
            sd[w1][sel] *= f
            sd[b1][sel] *= f
            sd[w2][:, sel] /= f
        for name in ("0.fn.to_qkv", "0.fn.to_out.0", "1.fn.net.0", "1.fn.net.3"):
            w = sd[(T % l) + name + ".weight"]
            w[rng.randint(w.shape[0]), rng.randint(w.shape[1])] = 20.0 * np.abs(w).max()
    return sd


@pytest.mark.parametrize("precision", ["mixed", "precise"])
def test_parity_on_trained_like_activations(precision):
    """Random-init weights keep every activation small (max |LayerNorm out| 5.6, max |GELU hidden| 2.6 on the fixtures); trained
    transformers do not.  The same FUNCTION is re-parameterised the way training leaves it: LayerNorm gains x 8 with shifted
    biases (the consuming to_qkv / fc1 weights / 8), 3 % of the FeedForward hidden units x 30 and a handful x 300 (their fc2
    columns scaled back), and one outlier entry (20 x the maximum) in every Linear weight.  LayerNorm outputs then reach +-40,
    hidden activations several hundred, a few exceed the e4m3 range of the mixed operand format (448: they degrade to the fp16
    class, element by element) -- the fixed activation exponents of round 2 saturated at 28.  Against the fp64 oracle."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    dev = _dev()
    layers, heads = 4, 8
    sd = _trained_like_state_dict(layers)
    batch = synth.synthetic_batch(11, 2, [12, 9])
    model = testing.make_predictor(testing.make_config(layers, heads, precision=precision), sd, dev)
    out, _ = _run(model, batch, "predcls", dev)
    ref, _, _ = vo.forward(sd, vo.OracleConfig(layers=layers, heads=heads), batch, dtype=torch.float64)
    got = torch.cat(list(out[1])).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print("trained-like activations [%s]: logit max-abs-err %.3e (max |logit| %.2f)" % (precision, err, ref.abs().max().item()))
    assert err <= 3e-4, err


def test_saturation_audit_counts_what_the_mixed_format_clamps():
    """veto_forward_saturation (VETO_AMD.COUNT_SATURATION) makes the silent part of the mixed operand format visible: elements beyond
    |a| = 448 lose their e4m3 correction terms, beyond 65504 their fp16 value clamps.  On the fixtures nothing is clamped; with the
    trained-like weights a few of the hidden units scaled x 300 are (value plane), and the logits of the audit forward
    (launch-per-stage form) agree with the default forward.  Hidden units scaled x 60000 overflow fp16 itself."""
    from veto_amd import synth, testing
    dev = _dev()
    layers, heads = 4, 8
    batch = synth.synthetic_batch(11, 2, [12, 9])
    cfg = testing.make_config(layers, heads)
    cfg.VETO_AMD.COUNT_SATURATION = True

    g, sd0, gbatch = load_golden("predcls_n10_l4h8")
    model = testing.make_predictor(cfg, sd0, dev)
    out, _ = _run(model, gbatch, "predcls", dev)
    assert np.abs(torch.cat(list(out[1])).cpu().numpy() - g["rel_dists"]).max() <= LOGIT_TOL
    rep = model.last_saturation
    assert len(rep) == layers and all(set(r) == {"qkv_in", "attn_out", "ffn_in", "hidden"} for r in rep)
    n_rows = 90 * 19
    for l in range(layers - 1):
        assert rep[l]["attn_out"]["elements"] == n_rows * 576 and rep[l]["hidden"]["elements"] == n_rows * 1152, rep[l]
        assert rep[l]["qkv_in"]["elements"] == (90 * 2 * 576 if l == 0 else n_rows * 576), rep[l]
    # the last layer: attention on split-bf16 operands, FeedForward on the 90 CLS rows as mixed rows (the classifier's input: audited too)
    last = rep[layers - 1]
    assert last["qkv_in"]["elements"] == 0 and last["attn_out"]["elements"] == 0, last
    assert last["ffn_in"]["elements"] == 90 * 576 and last["hidden"]["elements"] == 90 * 1152, last
    assert all(v["f16_saturated"] == 0 and v["value_saturated"] == 0 and v["resid_saturated"] == 0 for r in rep for v in r.values()), rep

    sd = _trained_like_state_dict(layers)
    plain = testing.make_predictor(testing.make_config(layers, heads), sd, dev)
    ref, _ = _run(plain, batch, "predcls", dev)
    model = testing.make_predictor(cfg, sd, dev)
    out, _ = _run(model, batch, "predcls", dev)
    assert (torch.cat(list(out[1])) - torch.cat(list(ref[1]))).abs().max().item() <= 1e-4
    rep = model.last_saturation
    print("saturation audit, trained-like weights:", [{k: (v["value_saturated"], v["resid_saturated"]) for k, v in r.items()} for r in rep])
    hid = [rep[l]["hidden"] for l in range(layers)]      # (the last layer's CLS rows included: its hidden units are scaled like the others')
    # (the residual plane clamps only where the fp16 rounding error itself exceeds 448 / 2^11 = 0.22, i.e. for some |a| >= 512)
    assert sum(h["value_saturated"] for h in hid) > 0, rep
    assert all(h["f16_saturated"] == 0 and h["value_saturated"] < 0.01 * h["elements"] for h in hid), rep

    model = testing.make_predictor(cfg, _trained_like_state_dict(layers, hidden_factor=60000.0), dev)
    _run(model, batch, "predcls", dev)
    assert sum(r["hidden"]["f16_saturated"] for r in model.last_saturation) > 0, model.last_saturation
    # ... and the audit sees it in the LAST layer too, whose FeedForward runs on the pairs' CLS rows as mixed operands (round 6: those rows
    # are the classifier's input, and rounds 2-5 reported zeros for them)
    assert model.last_saturation[layers - 1]["hidden"]["f16_saturated"] > 0, model.last_saturation[layers - 1]


@pytest.mark.parametrize("name", ["predcls_n10_l4h8", "predcls_n36_l4h8", "predcls_b12_n36_l6h6"])
def test_fast_mode_error_is_reported_not_trusted(name):
    """VETO_FAST (round 6): VETO_MIXED's launches with the correction stages of the two fused token-row launches skipped -- the fp16 main
    product alone.  Its error is an fp16 GEMM's (pure fp16 operands: 1.6-2.1e-3, tools/precision_study.py): far from the mixed mode's
    5e-5 -- the stages really are skipped -- and far from garbage -- the shortened stage streams of both kernels (eight and six heads,
    one panel and many) still multiply every fp16 slice exactly once."""
    from veto_amd import testing
    dev = _dev()
    g, sd, batch = load_golden(name)
    cfg = testing.make_config(int(g["_layers"]), int(g["_heads"]), precision="fast")
    model = testing.make_predictor(cfg, sd, dev)
    out, _ = _run(model, batch, "predcls", dev)
    err = np.abs(torch.cat(list(out[1])).cpu().numpy() - g["rel_dists"]).max()
    print("%s: fast (fp16 single pass) logit max-abs-err %.3e" % (name, err))
    assert 2e-4 < err < 1e-2, err


def test_full_size_properties():
    """BASELINE.json cfg-2 size (12 img x 36 obj = 15120 pairs, L4/H8): results must not depend on
    batching, pair order or workspace chunking -- each pair's logits are a function of its own
    subject/object only.  All three are bit-exact properties of the HIP path."""
    from veto_amd import synth, testing
    from veto_amd.pairs import prepare_test_pairs
    dev = _dev()
    sd = synth.predictor_state_dict(0, layers=4)
    batch = synth.synthetic_batch(7, 12, 36)
    model = testing.make_predictor(testing.make_config(4, 8), sd, dev)
    out, pairs = _run(model, batch, "predcls", dev)
    full = torch.cat(list(out[1]))
    assert full.shape == (15120, 51) and torch.isfinite(full).all()

    # (1) image 0 alone == image 0 inside the batch; and it matches the 36-object golden
    one = synth.synthetic_batch(7, 1, 36)
    g, _, gbatch = load_golden("predcls_n36_l4h8")
    out1, _ = _run(model, one, "predcls", dev)
    assert np.abs(out1[1][0].cpu().numpy() - g["rel_dists"]).max() <= LOGIT_TOL
    # synthetic_batch draws per-object streams by global index, so image 0 of the batch has the same objects
    assert np.array_equal(batch["roi_features"][:36], one["roi_features"])
    assert torch.equal(out[1][0], out1[1][0])

    # (2) permuting the pair list permutes the logits
    perm = torch.randperm(1260, generator=torch.Generator().manual_seed(5)).to(dev)
    ppairs = [pairs[0][perm]] + list(pairs[1:])
    outp, _ = _run(model, batch, "predcls", dev, pairs=ppairs)
    assert torch.equal(outp[1][0], out[1][0][perm])

    # (3) chunked workspace (4 passes) == single pass
    modelc = testing.make_predictor(testing.make_config(4, 8, max_chunk_pairs=4000), sd, dev)
    outc, _ = _run(modelc, batch, "predcls", dev)
    assert torch.equal(torch.cat(list(outc[1])), full)


def _flat(rel):
    """Predicate logits as one [P, n] tensor: list of per-image tensors (vanilla) or dict of group heads (MEET)."""
    if isinstance(rel, dict):
        return torch.cat([rel[k] for k in sorted(rel)], 1)
    return torch.cat(list(rel))


@pytest.mark.parametrize("mode,meet,dataset,layers,heads,precision", [
    ("sgcls", False, "VG", 4, 8, "mixed"),        # cfg-4 per-GPU workload
    ("predcls", False, "VG", 6, 6, "mixed"),      # the shipped architecture
    ("predcls", True, "VG", 6, 6, "mixed"),       # cfg-5 heads, VG
    ("sgcls", True, "GQA", 4, 8, "mixed"),        # GQA heads, hard-label sgcls embedding of the MEET trunk
    ("predcls", False, "VG", 4, 8, "precise"),
])
def test_full_size_properties_other_modes(mode, meet, dataset, layers, heads, precision):
    """12 images x 36 objects in the modes round 1 only ran small: every pair's logits depend on its own subject / object only,
    so the batch result must equal -- bit for bit -- the single-image result, a permuted pair list must give permuted logits,
    and a workspace chunk size that cuts inside images must change nothing (table layer 0, folded last layer and the chunk loop
    all take part at this size)."""
    from veto_amd import synth, testing
    from veto_amd.meet_tables import NUM_CLASSES
    dev = _dev()
    n_objc = NUM_CLASSES[dataset][0]
    if meet:
        from conftest import GQA_MEET_GROUPS, VG_MEET_GROUPS
        sd = synth.meet_state_dict(0, VG_MEET_GROUPS if dataset == "VG" else GQA_MEET_GROUPS, layers=layers, num_obj_cls=n_objc)
    else:
        sd = synth.predictor_state_dict(0, layers=layers, num_obj_cls=n_objc, num_rel_cls=NUM_CLASSES[dataset][1])
    batch = synth.synthetic_batch(7, 12, 36, num_obj_cls=n_objc)
    model = testing.make_predictor(testing.make_config(layers, heads, mode, meet, dataset, precision=precision), sd, dev)
    out, pairs = _run(model, batch, mode, dev)
    full = _flat(out[1])
    assert full.shape[0] == 15120 and torch.isfinite(full).all()
    one = synth.synthetic_batch(7, 1, 36, num_obj_cls=n_objc)
    out1, _ = _run(model, one, mode, dev)
    assert torch.equal(_flat(out1[1]), full[:1260])
    perm = torch.randperm(1260, generator=torch.Generator().manual_seed(5)).to(dev)
    outp, _ = _run(model, batch, mode, dev, pairs=[pairs[0]] + [pairs[1][perm]] + list(pairs[2:]))
    assert torch.equal(_flat(outp[1])[1260:2520], full[1260:2520][perm])
    modelc = testing.make_predictor(testing.make_config(layers, heads, mode, meet, dataset, precision=precision, max_chunk_pairs=3333), sd, dev)
    outc, _ = _run(modelc, batch, mode, dev)
    assert torch.equal(_flat(outc[1]), full)


def test_ragged_capped_batch_properties():
    """The ragged 12-image fixture (1 .. 64 objects, three images cut to 2048 pairs by the reference's own selection): chunking
    invariance with a chunk size that splits the capped images, and image-by-image == batch, bit for bit."""
    from veto_amd import testing
    dev = _dev()
    g, sd, batch = load_golden("ragged12_capped_l4h8")
    given = [torch.from_numpy(p).to(dev) for p in golden_pairs(g)]
    model = testing.make_predictor(testing.make_config(4, 8), sd, dev)
    out, _ = _run(model, batch, "predcls", dev, pairs=given)
    full = torch.cat(list(out[1]))
    assert [int(r.shape[0]) for r in out[1]] == [int(x) for x in g["pair_counts"]]
    modelc = testing.make_predictor(testing.make_config(4, 8, max_chunk_pairs=1000), sd, dev)
    outc, _ = _run(modelc, batch, "predcls", dev, pairs=given)
    assert torch.equal(torch.cat(list(outc[1])), full)
    # image 2 (64 objects, capped) on its own
    from conftest import subset_images
    sub, sub_pairs, rows = subset_images(g, batch, [2])
    outs, _ = _run(model, sub, "predcls", dev, pairs=[torch.from_numpy(sub_pairs[0]).to(dev)])
    assert torch.equal(outs[1][0], full[torch.from_numpy(rows).to(dev)])


def test_cpu_tensors_fail_loudly():
    from veto_amd import synth, testing
    g, sd, batch = load_golden("predcls_n10_l4h8")
    model = testing.make_predictor(testing.make_config(4, 8), sd, _dev())
    props = testing.make_proposals(batch, "predcls", "cpu")
    pairs = [torch.zeros((1, 2), dtype=torch.int64)]
    with pytest.raises(RuntimeError):
        model(props, pairs, None, None, roi_features=torch.from_numpy(batch["roi_features"]),
              roi_depth_features=torch.from_numpy(batch["roi_depth_features"]))
    model.train()          # training mode has no CPU path either
    with pytest.raises(RuntimeError, match="HIP device"):
        model(props, pairs, [torch.tensor([1])], None, roi_features=torch.from_numpy(batch["roi_features"]),
              roi_depth_features=torch.from_numpy(batch["roi_depth_features"]))


def _check_sorted_output(res, ref_scores_sorted, ref_pairs, ref_labels, ref_prob, tol=2e-6):
    """Scores must match; the order may differ only where the reference's keys are within rounding."""
    got_pairs, got_prob = res.get_field("rel_pair_idxs").cpu().numpy(), res.get_field("pred_rel_scores").cpu().numpy()
    got_labels = res.get_field("pred_rel_labels").cpu().numpy()
    assert got_pairs.shape == ref_pairs.shape
    same = (got_pairs == ref_pairs).all(1)
    if not same.all():   # a swap is legitimate only between (near-)equal sort keys
        bad = np.nonzero(~same)[0]
        assert np.abs(ref_scores_sorted[bad][:, None] - ref_scores_sorted[bad][None, :]).min(1).max() <= tol
        key = lambda p: p[:, 0] * 4096 + p[:, 1]
        assert np.array_equal(np.sort(key(got_pairs)), np.sort(key(ref_pairs)))
    assert np.abs(got_prob[same] - ref_prob[same]).max() <= tol
    assert np.array_equal(got_labels[same], ref_labels[same])


@pytest.mark.parametrize("name", post_golden_names())
def test_postprocessor_golden_parity(name):
    """HIP PostProcessor (veto_postprocess) vs the committed outputs of the real reference PostProcessor."""
    from oracle import veto_oracle as vo
    from veto_amd.postprocess import PostProcessor
    from veto_amd.structures import BoxList
    dev = _dev()
    g, rel_logits, obj_logits, pairs, num_objs = load_post_golden(name)
    boxes = [BoxList(torch.zeros(n, 4), (800, 600)).to(dev) for n in num_objs]
    post = PostProcessor(False, use_gt_box=True)
    P = [len(p) for p in pairs]
    res = post((list(torch.from_numpy(rel_logits).to(dev).split(P)), list(torch.from_numpy(obj_logits).to(dev).split(num_objs))),
               [torch.from_numpy(p).to(dev) for p in pairs], boxes)
    torch.cuda.synchronize()
    ref = vo.postprocess(rel_logits, obj_logits, pairs, num_objs)
    for i, r in enumerate(res):
        assert np.array_equal(r.get_field("pred_labels").cpu().numpy(), g["pred_labels_%d" % i])
        assert np.abs(r.get_field("pred_scores").cpu().numpy() - g["pred_scores_%d" % i]).max() <= 1e-6
        _check_sorted_output(r, ref[i]["triple_scores"].numpy(), g["rel_pair_idxs_%d" % i], g["pred_rel_labels_%d" % i],
                             g["pred_rel_scores_%d" % i])
        ts = post.last_triple_scores[i].cpu().numpy()
        assert (np.diff(ts) <= 0).all()                       # sortedness


def test_postprocessor_full_size_properties():
    """12 images x 1260 pairs: sorted keys, a permutation of the input pairs, probabilities sum to 1,
    ties broken by index (two identical logit rows keep their input order)."""
    from veto_amd import synth
    from veto_amd.postprocess import PostProcessor
    from veto_amd.structures import BoxList
    from oracle import veto_oracle as vo
    dev = _dev()
    num_objs = [36] * 12
    pairs = [torch.from_numpy(vo.enumerate_test_pairs(36)).to(dev) for _ in num_objs]
    rel = torch.from_numpy(synth.normal(5, "rel", (15120, 51), 0.0, 2.0)).to(dev)
    rel[101] = rel[100]                                        # an exact tie inside image 0
    obj = torch.from_numpy(synth.normal(5, "obj", (432, 151), 0.0, 3.0)).to(dev)
    boxes = [BoxList(torch.zeros(36, 4), (800, 600)).to(dev) for _ in num_objs]
    post = PostProcessor(False, use_gt_box=True)
    res = post((rel, obj), pairs, boxes)
    torch.cuda.synchronize()
    for i, r in enumerate(res):
        ts = post.last_triple_scores[i]
        assert (ts[1:] <= ts[:-1]).all()
        p = r.get_field("rel_pair_idxs")
        assert torch.equal(torch.sort(p[:, 0] * 64 + p[:, 1])[0], torch.sort(pairs[i][:, 0] * 64 + pairs[i][:, 1])[0])
        assert (r.get_field("pred_rel_scores").sum(1) - 1).abs().max() < 1e-5
        assert (r.get_field("pred_rel_labels") >= 1).all() and (r.get_field("pred_labels") >= 1).all()
    p0 = res[0].get_field("rel_pair_idxs")
    key = (p0[:, 0] * 64 + p0[:, 1]).tolist()
    k100, k101 = int(pairs[0][100, 0] * 64 + pairs[0][100, 1]), int(pairs[0][101, 0] * 64 + pairs[0][101, 1])
    if (post.last_triple_scores[0][key.index(k100)] == post.last_triple_scores[0][key.index(k101)]):
        assert key.index(k100) < key.index(k101)


@pytest.mark.parametrize("name", postmeet_golden_names())
def test_postprocessor_meet_golden_parity(name):
    """HIP MEET merge (veto_postprocess_meet) vs the committed outputs of the reference's MEET branch."""
    from oracle import veto_oracle as vo
    from veto_amd.postprocess import PostProcessor
    from veto_amd.structures import BoxList
    dev = _dev()
    g, rel, obj_logits, pairs, n = load_postmeet_golden(name)
    incre = [int(x) for x in g["incre_idx_list"]]
    post = PostProcessor(False, use_gt_box=True)
    box = BoxList(torch.zeros(n, 4), (800, 600)).to(dev)
    res = post(({k: torch.from_numpy(v).to(dev) for k, v in rel.items()}, [torch.from_numpy(obj_logits).to(dev)]),
               [torch.from_numpy(pairs).to(dev)], [box], incre_idx_list=incre, ensemble=True)[0]
    torch.cuda.synchronize()
    ref = vo.postprocess_meet(rel, obj_logits, pairs, incre, len(incre))
    assert np.array_equal(res.get_field("pred_labels").cpu().numpy(), g["pred_labels"])
    assert np.abs(res.get_field("pred_scores").cpu().numpy() - g["pred_scores"]).max() <= 1e-6
    assert res.get_field("rel_pair_idxs").dtype == torch.float32
    # rows are (pair, group) items: compare on (pair, label, row sum pattern) where the order agrees
    got_pairs = res.get_field("rel_pair_idxs").cpu().numpy()
    same = (got_pairs == g["rel_pair_idxs"]).all(1) & (res.get_field("pred_rel_labels").cpu().numpy() == g["pred_rel_labels"])
    ts = ref["triple_scores"].numpy()
    if not same.all():
        bad = np.nonzero(~same)[0]
        assert np.abs(ts[bad][:, None] - ts[bad][None, :] + np.eye(len(bad))).min(1).max() <= 2e-6
    assert same.mean() > 0.95
    assert np.abs(res.get_field("pred_rel_scores").cpu().numpy()[same] - g["pred_rel_scores"][same]).max() <= 2e-6
    got_ts = post.last_triple_scores[0].cpu().numpy()
    assert (np.diff(got_ts) <= 0).all() and np.abs(np.sort(got_ts) - np.sort(ts)).max() <= 2e-6
    with pytest.raises(ValueError):
        post(({k: torch.from_numpy(v).to(dev) for k, v in rel.items()}, [torch.from_numpy(obj_logits).to(dev)] * 2),
             [torch.from_numpy(pairs).to(dev)] * 2, [box, box], incre_idx_list=incre, ensemble=True)


@pytest.mark.parametrize("name", postvote_golden_names())
def test_postprocessor_vote_golden_parity(name):
    """HIP expert voting (veto_postprocess_vote) vs the committed outputs of the reference's EXPERT_GROUP
    branch (inference.py:93-283): same kept rows, same order (up to score near-ties), same probabilities."""
    from oracle import veto_oracle as vo
    from veto_amd import testing
    from veto_amd.postprocess import PostProcessor
    from veto_amd.structures import BoxList
    dev = _dev()
    g, rel, obj_logits, pairs, n = load_postvote_golden(name)
    incre = [int(x) for x in g["incre_idx_list"]]
    cfg = testing.make_config(1, 8, meet=True, dataset=str(g["dataset"]))
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = True
    cfg.ENSEMBLE_LEARNING.VOTING = str(g["voting"])
    post = PostProcessor(False, use_gt_box=True, cfg=cfg)
    box = BoxList(torch.zeros(n, 4), (800, 600)).to(dev)
    res = post(({k: torch.from_numpy(v).to(dev) for k, v in rel.items()}, [torch.from_numpy(obj_logits).to(dev)]),
               [torch.from_numpy(pairs).to(dev)], [box], incre_idx_list=incre, ensemble=True)[0]
    ref = vo.postprocess_vote(rel, obj_logits, pairs, incre, len(incre), voting=str(g["voting"]))
    assert np.array_equal(res.get_field("pred_labels").cpu().numpy(), g["pred_labels"])
    assert res.get_field("rel_pair_idxs").dtype == torch.float32
    got_pairs = res.get_field("rel_pair_idxs").cpu().numpy()
    assert got_pairs.shape == g["rel_pair_idxs"].shape                      # the same number of rows survive the vote
    same = (got_pairs == g["rel_pair_idxs"]).all(1) & (res.get_field("pred_rel_labels").cpu().numpy() == g["pred_rel_labels"])
    ts = ref["triple_scores"].numpy()
    if not same.all():
        bad = np.nonzero(~same)[0]
        assert np.abs(ts[bad][:, None] - ts[bad][None, :] + np.eye(len(bad))).min(1).max() <= 2e-6
    assert same.mean() > 0.95
    assert np.abs(res.get_field("pred_rel_scores").cpu().numpy()[same] - g["pred_rel_scores"][same]).max() <= 2e-6
    got_ts = post.last_triple_scores[0].cpu().numpy()
    assert (got_ts >= 0).all() and (np.diff(got_ts) <= 0).all() and np.abs(np.sort(got_ts) - np.sort(ts)).max() <= 2e-6


def test_expert_group_predictor_into_voting_postprocessor():
    """VETOPredictor_MEET with EXPERT_GROUP (15 heads) -> PostProcessor voting, on the device, against the
    oracle chain at a size no golden covers."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    from veto_amd.postprocess import PostProcessor
    dev = _dev()
    groups = [4, 6, 9, 19, 12]
    sd = synth.meet_state_dict(5, groups, layers=2, experts=3)
    batch = synth.synthetic_batch(17, 1, [14])
    cfg = testing.make_config(2, 8, "sgcls", meet=True)
    cfg.ENSEMBLE_LEARNING.EXPERT_GROUP = True
    cfg.ENSEMBLE_LEARNING.VOTING = "C"
    model = testing.make_predictor(cfg, sd, dev)
    out, pairs = _run(model, batch, "sgcls", dev)
    ocfg = vo.OracleConfig(layers=2, heads=8, mode="sgcls", meet_groups=groups, prefix="model.", experts=3)
    logits, _, _ = vo.forward(sd, ocfg, batch)
    col, ref_rel = 0, {}
    for e in range(3):
        for k, gk in enumerate(groups):
            ref_rel["group_%d%d" % (k, e + 1)] = logits[:, col:col + gk + 2].numpy()
            col += gk + 2
    for k, v in ref_rel.items():
        assert np.abs(out[1][k].cpu().numpy() - v).max() <= LOGIT_TOL
    post = PostProcessor(False, use_gt_box=True, cfg=cfg)
    props = testing.make_proposals(batch, "sgcls", dev)
    obj_logits = torch.from_numpy(batch["predict_logits"]).to(dev)
    res = post((out[1], [obj_logits]), pairs, props, incre_idx_list=out[3], ensemble=True)[0]
    ref = vo.postprocess_vote(ref_rel, batch["predict_logits"], pairs[0].cpu().numpy(), out[3], 51, voting="C")
    # the vote itself is discrete: the kept (pair, group-local label) multiset must agree unless two experts'
    # top probabilities are within the logit noise of each other
    got = sorted(zip(res.get_field("rel_pair_idxs").cpu().numpy().astype(int).tolist(), res.get_field("pred_rel_labels").cpu().tolist(),
                     np.round(res.get_field("pred_rel_scores").cpu().numpy().sum(1), 3).tolist()), key=str)
    want = sorted(zip(ref["rel_pair_idxs"].numpy().astype(int).tolist(), ref["pred_rel_labels"].tolist(),
                      np.round(ref["pred_rel_scores"].numpy().sum(1), 3).tolist()), key=str)
    assert abs(len(got) - len(want)) <= 2 and len(set(map(str, got)) & set(map(str, want))) >= 0.98 * len(want)


def test_relation_head_chain_against_oracle_chain():
    """proposals + ROI maps -> pairs -> predictor -> PostProcessor, all on the device, against the
    oracle's predictor + postprocess chain (predcls: one-hot +-1000 object logits, obj scores == 1)."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    from veto_amd.relation_head import VETORelationHead
    dev = _dev()
    num_objs = [8, 5]
    sd = synth.predictor_state_dict(3, layers=2)
    batch = synth.synthetic_batch(13, 2, num_objs)
    cfg = testing.make_config(2, 8)
    head = VETORelationHead(cfg)
    head.predictor = testing.make_predictor(cfg, sd, dev)
    head.eval()
    props = testing.make_proposals(batch, "predcls", dev)
    _, result, losses = head.forward_pooled(props, torch.from_numpy(batch["roi_features"]).to(dev),
                             torch.from_numpy(batch["roi_depth_features"]).to(dev))
    torch.cuda.synchronize()
    assert losses == {}
    logits, _, _ = vo.forward(sd, vo.OracleConfig(layers=2, heads=8), batch)
    pairs = [vo.enumerate_test_pairs(n) for n in num_objs]
    onehot = np.full((sum(num_objs), 151), -1000.0, dtype=np.float32)
    onehot[np.arange(sum(num_objs)), batch["labels"]] = 1000.0
    ref = vo.postprocess(logits.numpy(), onehot, pairs, num_objs)
    for r, o in zip(result, ref):
        assert torch.equal(r.get_field("pred_labels").cpu(), o["pred_labels"])
        assert (r.get_field("pred_scores").cpu() - 1).abs().max() < 1e-6
        got_p, ref_p = r.get_field("rel_pair_idxs").cpu().numpy(), o["rel_pair_idxs"].numpy()
        same = (got_p == ref_p).all(1)
        assert same.mean() > 0.9   # near-ties (logit noise 3e-5) may swap neighbours
        assert np.abs(r.get_field("pred_rel_scores").cpu().numpy()[same] - o["pred_rel_scores"].numpy()[same]).max() < 1e-4
        assert np.array_equal(r.get_field("pred_rel_labels").cpu().numpy()[same], o["pred_rel_labels"].numpy()[same])


def test_repeated_runs_are_bit_identical():
    """The GEMM's LDS-DMA / barrier protocol has no data race: 25 back-to-back forwards at full size,
    interleaved with an unrelated memory-bound kernel, give bit-identical logits every time."""
    from veto_amd import synth, testing
    dev = _dev()
    sd = synth.predictor_state_dict(0, layers=4)
    batch = synth.synthetic_batch(7, 12, 36)
    model = testing.make_predictor(testing.make_config(4, 8), sd, dev)
    out, pairs = _run(model, batch, "predcls", dev)
    first = torch.cat(list(out[1])).clone()
    junk = torch.empty(64 << 20, device=dev)
    for i in range(25):
        junk.normal_()                                   # perturbs cache state and timing between runs
        out, _ = _run(model, batch, "predcls", dev, pairs=pairs)
        assert torch.equal(torch.cat(list(out[1])), first), i


def test_large_image_with_pair_cap_against_oracle():
    """One image with 64 objects in sgcls: 4032 candidate pairs, cut to MAX_PROPOSAL_PAIR = 2048 by score product
    (sampling.py:41-45); the selected pairs (whatever order the device sort gives to ties) go through the
    predictor and must match the oracle on exactly those pairs."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    from veto_amd.pairs import prepare_test_pairs
    dev = _dev()
    sd = synth.predictor_state_dict(6, layers=2)
    batch = synth.synthetic_batch(19, 1, [64])
    cfg = testing.make_config(2, 8, "sgcls")
    model = testing.make_predictor(cfg, sd, dev)
    props = testing.make_proposals(batch, "sgcls", dev)
    props[0].add_field("pred_scores", torch.from_numpy(synth.uniform(19, "cap.scores", (64,), 0.05, 1.0)).to(dev))
    pairs = prepare_test_pairs(dev, props)
    assert pairs[0].shape == (2048, 2) and (pairs[0][:, 0] != pairs[0][:, 1]).all()
    q = props[0].get_field("pred_scores")
    kept = (q[pairs[0][:, 0]] * q[pairs[0][:, 1]]).min().item()
    allp = torch.nonzero(torch.ones(64, 64, device=dev) - torch.eye(64, device=dev))
    assert ((q[allp[:, 0]] * q[allp[:, 1]]) > kept).sum().item() <= 2048      # nothing better was left out
    out, _ = _run(model, batch, "sgcls", dev, pairs=pairs)
    ref, _, _ = vo.forward(sd, vo.OracleConfig(layers=2, heads=8, mode="sgcls"), batch, rel_pair_idxs=[pairs[0].cpu().numpy()])
    err = (torch.cat(list(out[1])).cpu() - ref).abs().max().item()
    assert err <= LOGIT_TOL, err


@pytest.mark.parametrize("m,n,k,ks", [(1000, 100, 192, 1), (5000, 576, 576, 0), (40000, 1728, 576, 0), (9999, 1152, 384, 7)])
def test_wgrad_gemm_against_fp64(m, n, k, ks):
    """dw = dy^T . x (reduction over the rows) through the split-K / atomic form of the production GEMM and the
    transposing split kernel: the weight-gradient shape of every Linear layer."""
    from veto_amd import native
    dev = _dev()
    lib = native.load_library()
    g = torch.Generator(device="cpu").manual_seed(m + n + k)
    dy = torch.randn(m, n, generator=g).to(dev)
    x = torch.randn(m, k, generator=g).to(dev)
    ref = dy.double().t() @ x.double()
    ws = torch.empty(lib.veto_debug_wgrad_workspace_bytes(m, n, k, ks), dtype=torch.uint8, device=dev)
    dw = torch.full((n, k), float("nan"), device=dev)
    native.check(lib.veto_debug_wgrad(None, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), m, n, k, ks, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    scale = (dy.abs().double().t() @ x.abs().double()).clamp_min(1e-6)
    rel = ((dw.double() - ref).abs() / scale).max().item()
    assert rel < 2e-5, (m, n, k, ks, rel)


def test_restructured_first_and_last_layer_match_the_plain_path(tmp_path):
    """The per-object form of layer 0 (VETO_QKV0_TABLES) and the folded last layer (VETO_CLS_FOLD) are exact algebra: the
    logits with both switched off (plain LayerNorm -> QKV GEMM -> attention in every layer) agree with the default path far
    inside the parity tolerance.  The knobs are read once per process, hence two child processes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from conftest import load_golden\n"
            "from veto_amd import testing\n"
            "from veto_amd.pairs import prepare_test_pairs\n"
            "g, sd, batch = load_golden('predcls_n36_l4h8')\n"
            "dev = torch.device('cuda:0')\n"
            "model = testing.make_predictor(testing.make_config(4, 8), sd, dev)\n"
            "props = testing.make_proposals(batch, 'predcls', dev)\n"
            "pairs = prepare_test_pairs(dev, props)\n"
            "with torch.no_grad():\n"
            "    out = model(props, pairs, None, None, roi_features=torch.from_numpy(batch['roi_features']).to(dev),\n"
            "                roi_depth_features=torch.from_numpy(batch['roi_depth_features']).to(dev))\n"
            "np.save(sys.argv[1], torch.cat(list(out[1])).cpu().numpy())\n") % (root, os.path.join(root, "tests"))
    outs = []
    # ... and the forms behind the other knobs of the default (mixed) path: the folded last layer with its products as two dense
    # GEMMs instead of four block-structured ones and its attention on the vector ALU, fp32 q / k / v instead of 3-byte floats, one
    # launch per panel phase
    variants = (("default", {}), ("plain", {"VETO_QKV0_TABLES": "0", "VETO_CLS_FOLD": "0"}),
                ("round2-forms", {"VETO_FOLD_BLOCKS": "0", "VETO_QKV_F24": "0", "VETO_TAIL_FUSED": "0", "VETO_FFN_LATE": "0", "VETO_CLS_MFMA": "0"}),
                ("two-launch-attention", {"VETO_QKV_ATTN_FUSED": "0"}),
                # the residual stream between the layers as 3-byte floats (round 6: measured null, kept as a variant): a 16-bit significand
                # in the stream itself, so it sits further from the default than the exact re-formulations above
                ("x-f24", {"VETO_X_F24": "1"}))
    for tag, env in variants:
        path = str(tmp_path / (tag + ".npy"))
        subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, **env), timeout=600)
        outs.append(np.load(path))
    g, _, _ = load_golden("predcls_n36_l4h8")
    for (tag, _), o in zip(variants[1:], outs[1:]):
        assert np.abs(outs[0] - o).max() < (3e-4 if tag == "x-f24" else 1e-4), tag
    for o in outs:
        assert np.abs(o - g["rel_dists"]).max() <= LOGIT_TOL


def test_oracle_parity_large_feature_scale():
    """ROI maps 40x larger and shifted (row means far from zero): the per-object form of layer 0 subtracts row means before its
    GEMMs and must stay as accurate as LayerNorm on the assembled tokens."""
    from oracle import veto_oracle as vo
    from veto_amd import synth, testing
    dev = _dev()
    sd = synth.predictor_state_dict(5, layers=3)
    batch = synth.synthetic_batch(13, 2, [8, 5], relu_like=True)
    for key in ("roi_features", "roi_depth_features"):
        batch[key] = (batch[key] * 40.0 + 15.0).astype(np.float32)
    model = testing.make_predictor(testing.make_config(3, 8), sd, dev)
    out, _ = _run(model, batch, "predcls", dev)
    ref, _, _ = vo.forward(sd, vo.OracleConfig(layers=3, heads=8), batch)
    err = (torch.cat(list(out[1])).cpu() - ref).abs().max().item()
    print("scaled features: logit max-abs-err %.2e (|logit| max %.2f)" % (err, ref.abs().max().item()))
    assert err <= LOGIT_TOL, err


def test_gemm_bias_slices_with_single_kstep_tiles():
    """K = 32 makes a tile ONE stage, so the loader waves run two TILES ahead of the epilogue that reads the bias slice in LDS:
    many such tiles per workgroup (M = 256 * 600, N = 192 * 2) must still pick up the right 192 bias values each."""
    from veto_amd import native
    lib = native.load_library()
    dev = _dev()
    m, n, k = 256 * 600, 384, 32
    g = torch.Generator(device="cpu").manual_seed(9)
    a = torch.randn(m, k, generator=g).to(dev)
    w = torch.randn(n, k, generator=g).to(dev)
    bias = (torch.arange(n, dtype=torch.float32) * 10.0).to(dev)      # distinct per column and per N-tile
    ws = torch.empty(lib.veto_debug_gemm_workspace_bytes(m, n, k), dtype=torch.uint8, device=dev)
    c = torch.full((m, n), float("nan"), device=dev)
    native.check(lib.veto_debug_gemm(None, a.data_ptr(), w.data_ptr(), bias.data_ptr(), c.data_ptr(), m, n, k, native.VETO_PRECISE, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    ref = a.double() @ w.double().t() + bias.double()
    assert ((c.double() - ref).abs().max().item()) < 1e-2


def test_workspace_is_one_per_device_and_stream_and_only_grows():
    """The call path's scratch memory (native.Launch.workspace): calls on two side streams give the default stream's bits, each
    stream has its own workspace tensor, and a smaller call on a stream re-uses that stream's tensor.  Vanilla PostProcessor
    (1 image, 3 objects, 6 pairs, 51 predicates) and SGGEvaluator.evaluate (1 image, 2 GT relations, 6 predictions)."""
    from veto_amd import native, synth
    from veto_amd.evaluation import SGGEvaluator
    from veto_amd.postprocess import PostProcessor
    from veto_amd.structures import BoxList
    dev = _dev()
    pair_list = [(a, b) for a in range(3) for b in range(3) if a != b]
    rel = torch.from_numpy(synth.normal(11, "ws.rel", (6, 51), 0.0, 2.0)).to(dev)
    obj = torch.from_numpy(synth.normal(11, "ws.obj", (3, 151), 0.0, 3.0)).to(dev)
    pairs = torch.tensor(pair_list, dtype=torch.int64, device=dev)
    image = {"gt_rels": np.array([[0, 1, 5], [2, 0, 17]]), "gt_classes": np.array([3, 7, 9]),
             "gt_boxes": np.array([[0, 0, 50, 50], [60, 10, 120, 90], [20, 100, 80, 160]], dtype=np.float32),
             "pred_rel_inds": np.array(pair_list), "rel_scores": torch.softmax(rel, 1).cpu().numpy(),
             "pred_classes": np.array([3, 7, 9]), "obj_scores": np.ones(3, dtype=np.float32)}
    image["pred_boxes"] = image["gt_boxes"]
    evaluator = SGGEvaluator("sgcls", 51, np.array([[9, 3, 17]]), device=dev)

    def post(n_pair=6):
        box = BoxList(torch.zeros(3, 4), (800, 600)).to(dev)
        r = PostProcessor(False, use_gt_box=True)((rel[:n_pair], obj), [pairs[:n_pair]], [box])[0]
        return [r.get_field(k) for k in ("pred_labels", "pred_scores", "rel_pair_idxs", "pred_rel_scores", "pred_rel_labels")]

    def evaluate():
        res = evaluator.evaluate([image])
        flat = [np.array([res[k][n] for n in (20, 50, 100)]) for k in ("recall", "recall_nogc", "zeroshot_recall", "accuracy",
                                                                       "mean_recall", "ng_mean_recall")]
        return flat + [res["per_image"][0][k] for k in ("gc_rank", "ng_rank", "acc_rank", "zeroshot")]

    want_post, want_eval = post(), evaluate()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for s in streams:
        with torch.cuda.stream(s):
            got_post, got_eval = post(), evaluate()
        s.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got_post, want_post))
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got_eval, want_eval))
    keys = [(s.device_index, s.cuda_stream) for s in streams]
    ws = [native._WORKSPACES[k] for k in keys]
    assert ws[0] is not ws[1] and ws[0].data_ptr() != ws[1].data_ptr()
    assert (dev.index, 0) in native._WORKSPACES and native._WORKSPACES[(dev.index, 0)] is not ws[0]   # the default stream's own
    with torch.cuda.stream(streams[0]):
        small = post(n_pair=2)
    streams[0].synchronize()
    assert native._WORKSPACES[keys[0]] is ws[0]
    assert small[2].shape == (2, 2)
