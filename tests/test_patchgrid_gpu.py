"""The patch grids (POOLER_RESOLUTION, PATCH_SIZE) = (4, 1), (12, 3), (16, 4) on the device, and the unchanged default (8, 2): logits
against the real reference's (tests/golden/patchgrid/), the patch stage per element against float64 inside a derived bound, a
training step against oracle/train_oracle.py in the ordered mode (twice, bit-equal), chunked and batched calls, workspace sizes,
veto_create's refusals, and the default grid's bits against hashes taken from a build of the parent commit.

Eval calls go through veto_forward with a hand-filled veto_inputs_t.  Every workspace is exactly veto_workspace_bytes long, filled
with a sentinel and followed by guard cells; out_logits and the debug outputs likewise (tests/test_prelude_gpu.py's Guarded)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import patchgrid_cases as pg

pytestmark = pytest.mark.gpu

GUARD = 64
SENT32 = 0x7fc5a5a5
SENT64 = 0x5a5a5a5a5a5a5a5a
LOGIT_TOL = 1e-3            # the project's logit bar
GRAD_TOL = 2e-3             # tests/test_train_scale_gpu.py
HASH_FILE = os.path.join(os.path.dirname(pg.GOLDEN_DIR), "patchgrid_parent_hashes.txt")


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Guarded:
    """numel elements of sentinel, GUARD more behind them"""

    def __init__(self, numel, dtype, dev):
        self.numel, self.wide = numel, dtype == torch.int64
        self.raw = torch.full((numel + GUARD,), SENT64 if self.wide else SENT32, dtype=torch.int64 if self.wide else torch.int32, device=dev)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def bits(self, what):
        raw = self.raw.cpu().numpy()
        sent = SENT64 if self.wide else SENT32
        assert (raw[self.numel:] == sent).all(), "%s: guard cells behind the buffer were written" % what
        left = int((raw[:self.numel] == sent).sum())
        assert left == 0, "%s: %d of %d elements were never written" % (what, left, self.numel)
        return raw[:self.numel]


def engine_weights(sd, prefix=""):
    """The state dict under the names the handle expects: the predictor's prefix stripped, the MEET heads row-concatenated"""
    w = {k[len(prefix):]: np.asarray(v) for k, v in sd.items() if k.startswith(prefix)}
    k = 0
    heads_w, heads_b = [], []
    while "rel_out.%d.weight" % k in w:
        heads_w.append(w["rel_out.%d.weight" % k])
        heads_b.append(w["rel_out.%d.bias" % k])
        k += 1
    if heads_w:
        w["rel_out.weight"], w["rel_out.bias"] = np.concatenate(heads_w, 0), np.concatenate(heads_b, 0)
    return w


def make_engine(sd, res, patch, layers, heads, num_out, precision="mixed", chunk=0, prefix=""):
    from veto_amd import native
    dev = _dev()
    eng = native.Engine(layers, heads, 151, num_out, precision={"mixed": native.VETO_MIXED, "precise": native.VETO_PRECISE}[precision],
                        device=0, max_chunk_pairs=chunk, patch=patch, resolution=res)
    w = engine_weights(sd, prefix)
    stream = torch.cuda.current_stream(dev).cuda_stream
    held = []
    for name, numel in eng.weight_specs():
        t = torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dev).reshape(-1)
        assert t.numel() == numel, (name, t.numel(), numel)
        held.append(t)
        eng.load_weight(name, t.data_ptr(), numel, stream)
    torch.cuda.synchronize()
    return eng


def run(eng, batch, pairs, num_out, sgcls=False, tokens=True, what="call"):
    """One veto_forward; dict(logits [P, num_out] float32, subj, obj int64 [P], tokens [P, 19, 576]).  The workspace is exactly
    veto_workspace_bytes long inside a longer sentinel-filled buffer: nothing behind it may change."""
    from veto_amd import native
    dev = _dev()
    num_objs = [int(n) for n in batch["num_objs"]]
    N, P = sum(num_objs), int(sum(len(p) for p in pairs))

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    rgb, dep, boxes = up(batch["roi_features"]), up(batch["roi_depth_features"]), up(batch["boxes"])
    pr = up(np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs]))
    ooff = up(np.concatenate([[0], np.cumsum(num_objs)]).astype(np.int32))
    poff = up(np.concatenate([[0], np.cumsum([len(p) for p in pairs])]).astype(np.int32))
    lab = None if sgcls else up(batch["labels"].astype(np.int64))
    lg = up(batch["predict_logits"].astype(np.float32)) if sgcls else None
    need = eng.workspace_bytes(N, P)
    assert need > 0
    ws = torch.full((need + 4096,), 0x5a, dtype=torch.uint8, device=dev)
    f32, i64 = torch.float32, torch.int64
    bufs = {"logits": Guarded(P * num_out, f32, dev), "subj": Guarded(P, i64, dev), "obj": Guarded(P, i64, dev)}
    if tokens:
        bufs["tokens"] = Guarded(P * 19 * 576, f32, dev)
    inp = native.VetoInputs(struct_size=ctypes.sizeof(native.VetoInputs), n_obj=N, n_pair=P, n_img=len(num_objs),
                            roi_rgb=rgb.data_ptr(), roi_depth=dep.data_ptr(), boxes=boxes.data_ptr(), box_mode=0,
                            obj_labels=lab.data_ptr() if lab is not None else None, obj_logits=lg.data_ptr() if lg is not None else None,
                            rel_pairs=pr.data_ptr(), img_obj_offset=ooff.data_ptr(), img_pair_offset=poff.data_ptr(), bn_batch_stats=None)
    dbg = native.VetoDebugOutputs(struct_size=ctypes.sizeof(native.VetoDebugOutputs), subj_inds=bufs["subj"].ptr, obj_inds=bufs["obj"].ptr,
                                  tokens=bufs["tokens"].ptr if tokens else None, cls=None)
    eng.forward(torch.cuda.current_stream(dev).cuda_stream, inp, ws.data_ptr(), need, bufs["logits"].ptr, dbg)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5a).all()), "%s: bytes behind veto_workspace_bytes were written" % what
    r = {k: b.bits("%s / %s" % (what, k)) for k, b in bufs.items()}
    out = {"logits": r["logits"].view(np.float32).reshape(P, num_out), "subj": r["subj"], "obj": r["obj"]}
    if tokens:
        out["tokens"] = r["tokens"].view(np.float32).reshape(P, 19, 576)
    return out


# ---- logits against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["mixed", "precise"])
@pytest.mark.parametrize("name", [pg.golden_name(r, p, k) for r, p in pg.NEW_GRIDS for k in pg.KINDS])
def test_logits_against_the_reference(name, precision):
    """veto_forward at (4, 1), (12, 3), (16, 4) -- predcls, sgcls (with the placeholder pair of a one-object image; NHEADS 6 at
    (12, 3)) and MEET -- against the logits of the real reference within 1e-3; the global pair indices bit for bit."""
    from oracle import veto_oracle as vo
    g, sd, batch, cfg, pairs = pg.load(name)
    ref = pg.golden_logits(g, cfg)
    eng = make_engine(sd, 4 * cfg.patch, cfg.patch, cfg.layers, cfg.heads, ref.shape[1], precision, prefix=cfg.prefix)
    got = run(eng, batch, pairs, ref.shape[1], sgcls=cfg.mode == "sgcls" and cfg.meet_groups is None, tokens=False, what=name)
    eng.close()
    subj, obj = vo.build_pair_indices(pairs, batch["num_objs"])
    assert np.array_equal(got["subj"], subj) and np.array_equal(got["obj"], obj)
    err = float(np.abs(got["logits"] - ref).max())
    print("PATCHGRID logits %s %s: max-abs-err %.3e of %.0e" % (name, precision, err, LOGIT_TOL))
    assert np.isfinite(got["logits"]).all() and err <= LOGIT_TOL, (name, precision, err)


# ---- the patch stage per element --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,patch", pg.GRIDS)
def test_patch_tokens_against_fp64(res, patch):
    """patchify_kernel<p> + gemm_patch with K = 512 p^2 (512, 2048, 4608, 8192): the 16 patch tokens of every pair against the float64
    restatement of tests/patchgrid_cases.py, per element inside its derived bound (operand half steps + gamma(3 K)); the float32
    oracle's distance on the same bound is printed beside it.  Twice: the second call repeats the first bit for bit."""
    from veto_amd import synth
    from oracle import veto_oracle as vo
    sd = synth.predictor_state_dict(0, layers=2, patch=patch)
    batch = synth.synthetic_batch(7, 2, [3, 5], patch=patch)
    pairs = [vo.enumerate_test_pairs(n) for n in batch["num_objs"]]
    eng = make_engine(sd, res, patch, 2, 8, 51)
    a = run(eng, batch, pairs, 51, what="(%d, %d)" % (res, patch))
    b = run(eng, batch, pairs, 51, what="(%d, %d) again" % (res, patch))
    eng.close()
    assert np.array_equal(a["tokens"].view(np.uint32), b["tokens"].view(np.uint32)) and np.array_equal(a["logits"].view(np.uint32), b["logits"].view(np.uint32))
    ref, bound = pg.patch_tokens(sd, batch, pairs, patch)
    got = a["tokens"][:, 1:17].astype(np.float64)
    assert np.isfinite(got).all()
    f32 = pg.oracle_patch_tokens(sd, vo.OracleConfig(layers=2, heads=8, patch=patch), batch, pairs, dtype=torch.float32).astype(np.float64)
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    print("PATCHGRID patch stage (%d, %d) K %d: measured max-abs-err %.3e, derived bound at that element %.3e, worst ratio %.4f of the bound "
          "(float32 oracle: err %.3e, ratio %.4f)" % (res, patch, 512 * patch * patch, err.max(), bound.reshape(-1)[err.argmax()], ratio,
                                                      np.abs(f32 - ref).max(), (np.abs(f32 - ref) / bound).max()))
    assert ratio <= 1.0, ratio


# ---- chunked and batched ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,patch", pg.NEW_GRIDS)
def test_an_image_in_a_chunked_batch_equals_the_image_alone(res, patch):
    """Three images of 3, 2 and 5 objects, the middle one WITHOUT pairs, with max_chunk_pairs 7 (6 + 0 + 20 pairs: the first chunk
    ends one pair into the last image, the others inside it): the last image's logits equal those of a call with that image alone and
    no chunking, bit for bit."""
    from veto_amd import synth
    from oracle import veto_oracle as vo
    sd = synth.predictor_state_dict(0, layers=2, patch=patch)
    batch = synth.synthetic_batch(7, 3, [3, 2, 5], patch=patch)
    pairs = [vo.enumerate_test_pairs(3), np.zeros((0, 2), dtype=np.int64), vo.enumerate_test_pairs(5)]
    chunked = make_engine(sd, res, patch, 2, 8, 51, chunk=7)
    whole = run(chunked, batch, pairs, 51, tokens=False, what="batch of three")
    chunked.close()
    alone = {k: (v[5:] if isinstance(v, np.ndarray) and len(v) == 10 else v) for k, v in batch.items()}
    alone["num_objs"] = [5]
    plain = make_engine(sd, res, patch, 2, 8, 51)
    one = run(plain, alone, [pairs[2]], 51, tokens=False, what="the image alone")
    plain.close()
    assert np.array_equal(whole["logits"][6:].view(np.uint32), one["logits"].view(np.uint32))
    assert np.array_equal(whole["subj"][6:] - 5, one["subj"]) and np.array_equal(whole["obj"][6:] - 5, one["obj"])


# ---- workspaces -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,patch", pg.GRIDS)
def test_workspace_sizes_follow_the_patch_size(res, patch):
    """veto_workspace_bytes / veto_train_workspace_bytes grow by exactly the patch rows (and, in training, the transposed weight and
    its gradients) of the handle's patch size; that they are sufficient is what every call of this file checks with its guards."""
    from veto_amd import native
    lib = native.load_library()
    sizes = {}
    for r, p in ((8, 2), (res, patch)):
        eng = native.Engine(2, 8, 151, 51, precision=native.VETO_MIXED, device=0, patch=p, resolution=r)
        sizes[p] = (eng.workspace_bytes(8, 26), lib.veto_train_workspace_bytes(eng.handle, 8, 26))
        eng.close()
    K, K2 = 512 * patch * patch, 2048
    TR = lambda k: (k + 191) // 192 * 192
    al = lambda b: (b + 255) // 256 * 256
    assert sizes[patch][0] - sizes[2][0] == 256 * 2 * (K - K2) * 2
    train = lambda k: al(256 * 2 * k * 2) + al(k * 1152 * 4) + al(TR(k) * 2 * 1152 * 2) + al(256 * TR(k) * 4)
    assert sizes[patch][1] - sizes[2][1] == train(K) - train(K2)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,patch", pg.REFUSED + ((8, 0), (20, 5)))
def test_veto_create_refuses_other_grids(res, patch):
    """An argument check: nothing is allocated or launched."""
    from veto_amd import native
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(native.VetoError) as e:
        native.Engine(2, 8, 151, 51, precision=native.VETO_MIXED, device=0, patch=patch, resolution=res)
    msg = str(e.value)
    assert all("(%d, %d)" % q in msg for q in pg.GRIDS) and "19 tokens" in msg, msg
    assert torch.cuda.mem_get_info()[0] == before


# ---- training ---------------------------------------------------------------------------------------------------------------------------
def train_step(res, patch, layers=2, heads=8, num_objs=(3, 5), sd_seed=2, batch_seed=13):
    """One ordered-mode training step of VETOPredictor on the device: ({name: gradient}, {input: gradient}, losses, the inputs)"""
    import test_train_scale_gpu as ts
    from veto_amd import synth, testing
    dev = _dev()
    cfg = testing.make_config(layers, heads, "predcls", False, "VG", patch=patch, resolution=res)
    cfg.VETO_AMD.DETERMINISTIC = True
    sd = synth.predictor_state_dict(sd_seed, layers=layers, patch=patch)
    model = testing.make_predictor(cfg, sd, dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    batch = synth.synthetic_batch(batch_seed, len(num_objs), list(num_objs), patch=patch)
    pairs = ts.all_pairs(num_objs)
    labels = ts.uniform_labels(pairs)
    props = testing.make_proposals(batch, "predcls", dev)
    roi = {k: torch.from_numpy(batch[k]).to(dev).requires_grad_(True) for k in ("roi_features", "roi_depth_features")}
    out = model(props, [torch.from_numpy(p).to(dev) for p in pairs], [torch.from_numpy(l).to(dev) for l in labels], None, **roi)
    sum(out[2].values()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
    return grads, {k: v.grad.detach().cpu() for k, v in roi.items()}, {k: float(v.detach()) for k, v in out[2].items()}, (sd, batch, pairs, labels)


def _hash(tensors):
    h = hashlib.sha256()
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(np.ascontiguousarray(tensors[k].numpy() if isinstance(tensors[k], torch.Tensor) else tensors[k]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("res,patch", [(4, 1), (16, 4)])
def test_training_step_against_the_oracle(res, patch):
    """Forward, losses and every gradient -- proj_d / proj_v (the weight-gradient GEMM over 512 p^2 rows and its scatter), the ROI map
    gradients (the input-gradient GEMM over the padded transposed weight and unpatchify<p>) -- against train_oracle.train_step in
    float64 under the element-wise bound of tests/test_train_scale_gpu.py; the ordered mode run twice gives the same bits."""
    import test_train_scale_gpu as ts
    from oracle import train_oracle as to
    from oracle import veto_oracle as vo
    grads, dmaps, losses, (sd, batch, pairs, labels) = train_step(res, patch)
    grads2, dmaps2, losses2, _ = train_step(res, patch)
    assert losses == losses2 and _hash(grads) == _hash(grads2) and _hash(dmaps) == _hash(dmaps2), "the ordered mode did not repeat its bits"
    ref = to.train_step(sd, vo.OracleConfig(2, 8, patch=patch), batch, pairs, np.concatenate(labels), None)
    for k, v in losses.items():
        assert abs(v - ref["losses"][k]) < 2e-4 * max(1.0, abs(ref["losses"][k])), (k, v, ref["losses"][k])
    assert set(ref["grads"]) <= set(grads)
    res_ = {n: ts._errors(grads[n], want) for n, want in ref["grads"].items()}
    for k in dmaps:
        assert tuple(dmaps[k].shape) == (8, 256, res, res)
        res_["d_" + k] = ts._errors(dmaps[k], ref["d_" + k])
    worst = max(res_.items(), key=lambda kv: max(kv[1]))
    pe = {n: v for n, v in res_.items() if "patch_embed" in n or n.startswith("d_roi")}
    print("PATCHGRID train (%d, %d): worst element %.2e norm %.2e at %s | patch side: %s" % (
        res, patch, worst[1][0], worst[1][1], worst[0], "  ".join("%s %.1e %.1e" % (n.split("transformer.")[-1], e, ne) for n, (e, ne) in sorted(pe.items()))))
    for n, (e, ne) in res_.items():
        assert e < GRAD_TOL and ne < GRAD_TOL, (n, e, ne)


# ---- the default grid keeps its bits ----------------------------------------------------------------------------------------------------
def default_hashes():
    """SHA-256 of the (8, 2) results the parent commit already produced: the logits of the predcls_n10_l4h8 fixture's batch in both
    precision modes, and the ordered-mode gradients (parameters and ROI maps) of one training step"""
    from conftest import load_golden
    g, sd, batch = load_golden("predcls_n10_l4h8")
    pairs = [np.asarray(p) for p in np.split(g["pair_idx"], np.cumsum([int(x) for x in g["pair_counts"]])[:-1])]
    out = {}
    for precision in ("mixed", "precise"):
        eng = make_engine(sd, 8, 2, int(g["layers"]), int(g["heads"]), 51, precision)
        out["logits_" + precision] = _hash({"logits": run(eng, batch, pairs, 51, tokens=False)["logits"]})
        eng.close()
    grads, dmaps, _, _ = train_step(8, 2, layers=4, num_objs=(10,))
    out["train_ordered_grads"] = _hash(grads)
    out["train_ordered_map_grads"] = _hash(dmaps)
    return out


def test_default_grid_keeps_the_parent_commits_bits():
    """(8, 2): the p = 2 instantiations do the parent's arithmetic in the parent's order.  The hashes in
    tests/golden/patchgrid_parent_hashes.txt were taken with this function from a library built from the parent commit, on an MI355X
    (profiles/patchgrid_parity.txt says how); its two training hashes were taken again when the relation loss's gradient changed in its
    last bits (the file and profiles/ce_loss_parity.txt say why)."""
    want = dict(line.split() for line in open(HASH_FILE) if line.strip() and not line.startswith("#"))
    got = default_hashes()
    assert set(got) == set(want)
    for k in sorted(got):
        assert got[k] == want[k], "%s: the bits of the default patch grid changed" % k
