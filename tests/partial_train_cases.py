"""The cases of the partial training step (include/veto_amd.h, veto_train_plan_t): shapes, plans, the eval-mode settings and the
float64 reference they are held to.  tests/test_partial_train_gpu.py runs them on the device, tests/test_partial_train_host.py asserts
their premises on the CPU.  No test lives here.

Shapes.  Token rows = pairs x 19.  "l2h8-3img": 3, 7 and 2 objects with every ordered pair of the first two images and ONE pair of the
third: 49 pairs, 931 token rows -- no multiple of 64 (the LayerNorm backward's block) or of 256 (the GEMM's row tile), four row tiles.
"l3h6-2img": 4 and 6 objects, 42 pairs, 798 rows; "l3h6-1img": 5 objects, 20 pairs, 380 rows.  "l6h6-1img": the same image under six
layers, the smallest depth at which three or more layers under the lowest consumer share two sets of buffers in the forward.

Plans are sets of engine weight names (veto_weight_info).  `mid` is layer (L - 1) // 2: the middle layer at L3, the first at L2.
"last_heads" is the issue's "last layer plus heads" with its count of 4 weight-gradient and 3 input-gradient GEMMs: the four Linears of
the last layer with their biases, its LayerNorm2 and the heads.  LayerNorm1 of that layer sits BEHIND the QKV projection in the backward
chain (fc2, fc1, LN2, out, attention, qkv, LN1), so its gain needs the projection's input gradient: "last_all_heads" adds it and costs
the fourth input-gradient GEMM.
"""
import collections
import functools

import numpy as np
import torch

RATES = (0.1, 0.35, 0.35)      # p_pos, p_emb, p_attn: the reference's
STEP_SEED = 0x5EEDFACE12345
T = "fusion_transformer.transformer."
LINEARS = ("0.fn.to_qkv.weight", "0.fn.to_out.0.weight", "0.fn.to_out.0.bias", "1.fn.net.0.weight", "1.fn.net.0.bias", "1.fn.net.3.weight",
           "1.fn.net.3.bias")
NORMS = ("0.norm.weight", "0.norm.bias", "1.norm.weight", "1.norm.bias")
HEADS = ("rel_out.weight", "rel_out.bias")
BUFFERS = ("pos_embed.0.running_mean", "pos_embed.0.running_var")

Shape = collections.namedtuple("Shape", "tag layers heads num_objs single_pair_last batch_seed")
SHAPES = {s.tag: s for s in [Shape("l2h8-3img", 2, 8, (3, 7, 2), True, 14), Shape("l3h6-2img", 3, 6, (4, 6), False, 14),
                             Shape("l3h6-1img", 3, 6, (5,), False, 13), Shape("l6h6-1img", 6, 6, (5,), False, 13)]}


def shape_pairs_labels(shape):
    from oracle import veto_oracle as vo
    from veto_amd import synth
    pairs = [vo.enumerate_test_pairs(n) for n in shape.num_objs]
    if shape.single_pair_last:
        pairs[-1] = np.array([[1, 0]], dtype=np.int64)
    lab = synth.integers(7, "partial.labels", (sum(len(p) for p in pairs),), 0, 51)
    return pairs, list(np.split(lab, np.cumsum([len(p) for p in pairs])[:-1]))


def shape_batch(shape):
    from veto_amd import synth
    return synth.synthetic_batch(shape.batch_seed, len(shape.num_objs), list(shape.num_objs))


@functools.lru_cache(maxsize=None)
def state_dict(layers, meet=False):
    from conftest import VG_MEET_GROUPS
    from veto_amd import synth
    return synth.meet_state_dict(2, VG_MEET_GROUPS, layers=layers) if meet else synth.predictor_state_dict(2, layers=layers)


def weight_names(layers):
    """The engine's tensors that are parameters, in no particular order (the buffers of pos_embed.0 are BUFFERS)."""
    names = ["obj_embed.weight", "class_projection.0.weight", "class_projection.0.bias", "location_projection.0.weight",
             "location_projection.0.bias", "pos_embed.0.weight", "pos_embed.0.bias", "pos_embed.1.weight", "pos_embed.1.bias",
             T + "cls_token", T + "pos_embedding"]
    names += [T + "patch_embed.proj_%s.%s" % (p, k) for p in "dv" for k in ("weight", "bias")]
    names += [T + "layers.%d.%s" % (l, k) for l in range(layers) for k in LINEARS + NORMS]
    return names + list(HEADS)


def layer(l, keys=LINEARS + NORMS):
    return {T + "layers.%d.%s" % (l, k) for k in keys}


Plan = collections.namedtuple("Plan", "trainable maps wgrad dgrad")      # wgrad / dgrad: the launch counts (None: not stated)


def plans(layers):
    L, mid = layers, (layers - 1) // 2
    every = set(weight_names(L))
    return {
        "heads": Plan(set(HEADS), False, 0, 0),
        "last_heads": Plan(layer(L - 1, LINEARS + NORMS[2:]) | set(HEADS), False, 4, 3),
        "last_all_heads": Plan(layer(L - 1) | set(HEADS), False, 4, 4),
        "fc2_mid": Plan(layer(mid, LINEARS[5:7]), False, 1, 4 * (L - 1 - mid)),
        "qkv_mid": Plan(layer(mid, LINEARS[0:1]), False, 1, 4 * (L - 1 - mid) + 3),
        "ln_gains": Plan({T + "layers.%d.%s" % (l, k) for l in range(L) for k in (NORMS[0], NORMS[2])}, False, 0, 4 * L),
        "obj_embed": Plan({"obj_embed.weight"}, False, 0, 4 * L),
        "no_heads": Plan(every - set(HEADS), True, 4 * L, 4 * L),
        "maps_only": Plan(set(), True, 0, 4 * L),
        "full": Plan(every, True, 4 * L, 4 * L),
    }


def frozen_prefix(layers, k):
    """Layers k .. L-1 and the heads trainable, everything under layer k frozen (k == L: the heads alone)."""
    out = set(HEADS)
    for l in range(k, layers):
        out |= layer(l)
    return out


# ---- the float64 reference of a step with per-site settings -----------------------------------------------------------------------------
def oracle_step(shape, seed, p_pos, p_emb, p_attn_layers, bn_eval=False, dtype=torch.float64):
    """One training step (plain CE over every pair row) composed from oracle/veto_oracle.py's own pieces: position_embedding with
    batch_stats = not bn_eval, pair_tokens, encoder_layer(drop = that layer's factor) per layer, under the library's masks for `seed`
    (oracle/dropout.py).  Returns {"logits", "loss", "grads": {state-dict key: gradient}, "d_roi_features", "d_roi_depth_features"}."""
    from oracle import dropout as od
    from oracle import veto_oracle as vo
    sd, batch = state_dict(shape.layers), shape_batch(shape)
    pairs, labels = shape_pairs_labels(shape)
    cfg = vo.OracleConfig(shape.layers, shape.heads)
    p = {}
    for k, v in sd.items():
        if "criterion" in k or k.endswith("num_batches_tracked"):
            continue
        t = vo._t(np.asarray(v), dtype).clone()
        p[k] = t.requires_grad_(True) if not k.endswith(("running_mean", "running_var")) else t
    rgb = vo._t(batch["roi_features"], dtype).clone().requires_grad_(True)
    dep = vo._t(batch["roi_depth_features"], dtype).clone().requires_grad_(True)
    subj, obj = vo.build_pair_indices(pairs, batch["num_objs"])
    s, o = torch.from_numpy(subj), torch.from_numpy(obj)
    P, n_obj = len(subj), len(batch["boxes"])

    def factor(site, rate, rows, cols):
        return od.Dropout(rate, rate, rate, seed=seed).factor(site, rows, cols, dtype)

    def tokens(site, rate):
        f = factor(site, rate, P * 19, cfg.dim)
        return None if f is None else f.reshape(P, 19, cfg.dim)
    emb, _ = vo.object_embeddings(p, cfg, batch["labels"], None, None, dtype)
    pos = vo.position_embedding(p, cfg, batch["boxes"], dtype, batch_stats=not bn_eval, drop=factor(od.SITE_POS, p_pos, n_obj, 128))
    x = vo.pair_tokens(p, cfg, emb, pos, rgb, dep, s, o, dtype, drop=tokens(od.SITE_EMB, p_emb))
    for l in range(cfg.layers):
        x = vo.encoder_layer(p, cfg, x, l, dtype, drop=tokens(od.SITE_ATTN0 + l, p_attn_layers[l]))
    Wh, bh = vo.head_weights(p, cfg, dtype)
    z = x[:, 0] @ Wh.t() + bh
    loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(np.concatenate(labels)).long())
    loss.backward()
    return {"logits": z.detach(), "loss": float(loss.detach()), "grads": {k: v.grad.detach() for k, v in p.items() if v.grad is not None},
            "d_roi_features": rgb.grad.detach(), "d_roi_depth_features": dep.grad.detach()}


# the eval-mode settings: (which modules are in eval(), the rates the step must then run at given the modules' p = RATES)
EvalCase = collections.namedtuple("EvalCase", "tag shape attn_eval pos_drop_eval bn_eval")
EVAL_CASES = {c.tag: c for c in [EvalCase("attn-mid-off", "l3h6-2img", (1,), False, False), EvalCase("pos-drop-off", "l2h8-3img", (), True, False),
                                 EvalCase("bn-eval", "l2h8-3img", (), False, True)]}


def eval_case_rates(case, honour_eval=True):
    """(p_pos, p_emb, [p_attn per layer]) the step runs at; honour_eval False: the WRONG reference that leaves the masks of the modules in
    eval() on."""
    L = SHAPES[case.shape].layers
    attn = [0.0 if (l in case.attn_eval and honour_eval) else RATES[2] for l in range(L)]
    return RATES[0], 0.0 if (case.pos_drop_eval and honour_eval) else RATES[1], attn
