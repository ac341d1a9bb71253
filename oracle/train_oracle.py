"""CPU restatement of the training-time losses, of the MEET expert sampling (the
parts named there: "weighted CE (BETA_LOSS ...), MEET per-group CE with ... expert sampling") and, in `train_step`, of
the whole training step: the training-mode forward over oracle/veto_oracle.py's pieces and, through torch autograd in
float64, the gradient of the summed losses for every parameter and for the two ROI inputs.

TEST INFRASTRUCTURE ONLY: imported by tests/ and nothing else; the product path is veto_amd/csrc/losses.hip behind
veto_ce_loss / veto_meet_sample.

PARITY PINNED: tests/golden/train_*.npz hold, from the reference predictor run in training mode here
(tests/golden/make_golden.py::run_train_losses): the classifier logits it produced, the labels, the losses it
returned and, for MEET, its expert sampling drawn from Python's `random` seeded with 1, and the gradients its
autograd produced (norm and a strided sample per parameter and per ROI input): tests/test_train_oracle.py holds
`train_step` to every one of them.
"""
import numpy as np
import torch

from . import dropout as od
from . import veto_oracle as vo


def weighted_ce(logits, labels, weight=None):
    """nn.CrossEntropyLoss(weight=w)(logits, labels), reduction 'mean' (roi_relation_predictors.py:4067-4068,4133):
    sum_i w[y_i] * (logsumexp(z_i) - z_i[y_i]) / sum_i w[y_i].  Returns (loss, dlogits) in float64."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    w = np.ones(z.shape[1]) if weight is None else np.asarray(weight, dtype=np.float64)
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    wi = w[y]
    loss = float((wi * (lse - z[np.arange(len(y)), y])).sum() / wi.sum())
    p = np.exp(z - lse[:, None])
    p[np.arange(len(y)), y] -= 1.0
    return loss, p * (wi / wi.sum())[:, None]


class PyRandomStream:
    """The exact stream of Python's `random` module (MT19937, CPython's random_random / getrandbits /
    _randbelow_with_getrandbits) on top of 32-bit words, so that it can be replayed from a block of raw words."""

    def __init__(self, words):
        self.words, self.pos = words, 0

    def _u32(self):
        v = int(self.words[self.pos])
        self.pos += 1
        return v

    def random(self):
        a, b = self._u32() >> 5, self._u32() >> 6
        return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0)

    def randint0(self, n):          # random.randint(0, n - 1)
        k = n.bit_length()
        r = self._u32() >> (32 - k)
        while r >= n:
            r = self._u32() >> (32 - k)
        return r


def meet_sampling(labels, incre_idx_list, sample_rate_matrix, num_groups, stream):
    """VETOPredictor_MEET.forward, training branch, ZERO_LABEL_PADDING_MODE 'rand_insert'
    (roi_relation_predictors.py:3940-3969): per relation, in order: a background label goes to ONE random group
    (random.randint); a foreground label with group id g = incre_idx_list[label] draws u = random.random() and walks
    a = G .. 1: the first a with u <= sample_rate_matrix[a-1][label] or a < g puts the relation into groups 0..a-1.
    Returns the list of per-group row index lists (cur_chosen_matrix)."""
    chosen = [[] for _ in range(num_groups)]
    for i, lab in enumerate(labels):
        lab = int(lab)
        if lab == 0:
            chosen[stream.randint0(num_groups)].append(i)
            continue
        g = incre_idx_list[lab]
        u = stream.random()
        for j in range(num_groups):
            a = num_groups - j
            if u <= sample_rate_matrix[a - 1][lab] or a < g:
                for k in range(a):
                    chosen[k].append(i)
                break
    return chosen


def meet_group_labels(labels, rows, incre_idx_list, k):
    """Ensemble.forward :3812-3821: inside group k own classes map to 1.. (their position in the group's class
    list + 1), every other foreground class to g_k + 1, background stays 0."""
    own = [c for c, x in enumerate(incre_idx_list) if x == k + 1]
    out = []
    for i in rows:
        lab = int(labels[i])
        out.append(0 if lab == 0 else (own.index(lab) + 1 if lab in own else len(own) + 1))
    return np.array(out, dtype=np.int64)


def _ce_terms(logits, labels, weight):
    """(per-row w[y] * nll, per-row w[y]) of nn.CrossEntropyLoss(weight=w); a negative label is an ignored row."""
    keep = labels >= 0
    y = labels.clamp(min=0)
    nll = torch.logsumexp(logits, 1) - logits.gather(1, y[:, None])[:, 0]
    w = torch.ones_like(nll) if weight is None else weight[y]
    w = w * keep.to(w.dtype)
    return w * nll, w


def _loss_plan(cfg, labels, loss, dtype):
    """The loss dict as a list of (name, first logit column, column count, rows, targets, class weights): the vanilla head's one
    (weighted) CE over every row, or per MEET head the CE over that group's chosen rows with the group-local labels
    (Ensemble.forward :3806-3846; every expert of a group sees the same rows and labels)."""
    labels = torch.as_tensor(np.asarray(labels)).long()
    loss = loss or {}
    if cfg.meet_groups is None:
        w = loss.get("weight")
        w = None if w is None else torch.as_tensor(np.asarray(w)).to(dtype)
        n_out = int(loss["num_out"]) if "num_out" in loss else None
        return [("rel_loss", 0, n_out, torch.arange(len(labels)), labels, w)]
    incre = [int(x) for x in loss["incre_idx_list"]]
    plan, col = [], 0
    for e in range(max(1, cfg.experts)):
        for k, g in enumerate(cfg.meet_groups):
            rows = np.asarray(loss["chosen"][k], dtype=np.int64)
            name = "group_%d%d_CE_loss" % (k, e + 1) if cfg.experts else "group_%d_CE_loss" % k
            plan.append((name, col, g + 2, torch.from_numpy(rows),
                         torch.from_numpy(meet_group_labels(labels.numpy(), rows, incre, k)), None))
            col += g + 2
    return plan


def train_step(sd, cfg, batch, rel_pair_idxs, labels, loss=None, dtype=torch.float64, pair_chunk=256, dropout=None):
    """One training step of VETOPredictor / VETOPredictor_MEET (roi_relation_predictors.py:4074-4136, :3752-3853,
    :3909-3995): the forward of veto_oracle.forward except that pos_embed.0 normalises with the BATCH statistics (biased
    variance) and that the three dropout sites of the path carry the masks `dropout` names, the losses, and autograd of their
    sum (the trainer sums the loss dict).

    dropout: None (dropout off: every golden and tests/test_train_oracle.py), or an oracle.dropout.Dropout with the meaning of
            veto_train_opts_t (include/veto_amd.h): p_pos / p_emb / p_attn and the step's 64-bit seed.  The masks are the
            LIBRARY's counter-based ones, element for element (the reference draws from torch's generator and cannot be matched
            bit for bit): keep * x / (1 - p) behind the ReLU of pos_embed (site 1, element n * 128 + k), on the assembled tokens
            (pos_drop, site 2, element row * 576 + col with row = GLOBAL pair row * 19 + token: not the chunk's) and on
            (attn_out Wo^T + bo) of layer l before the residual add (site 3 + l, numbered as site 2); a site with p == 0 leaves
            x untouched.
    labels: relation label per pair row, concatenated over the images.
    loss:   None (plain CE), {"weight": class weights} (BETA_LOSS), or for cfg.meet_groups
            {"chosen": per-group row lists (cur_chosen_matrix), "incre_idx_list": ...}.
    Returns a dict: "losses" {name: float}, "logits" [P, n_out], "grads" {state-dict key: gradient} for every parameter the
    loss depends on (EXPERT_GROUP: `rel_out.k` is the last expert's head, listed under both of its names),
    "d_roi_features" / "d_roi_depth_features", and "bn_batch_stats" (mean, biased var, unbiased var of the box features: the
    running update takes the unbiased one).

    Memory is bounded by `pair_chunk`: the per-object prelude (object embeddings, position embedding with its BatchNorm)
    is built once and cut out of the graph; every chunk of pairs back-propagates its share of the summed loss into the
    parameters and into the prelude's outputs, whose accumulated gradient goes through the prelude once at the end.  The
    chunk size does not change the result beyond float64 summation order (tests/test_train_oracle.py)."""
    num_objs = batch["num_objs"]
    subj, obj = vo.build_pair_indices(rel_pair_idxs, num_objs)
    subj_t, obj_t = torch.from_numpy(subj), torch.from_numpy(obj)
    P = len(subj)
    skip = ("running_mean", "running_var", "num_batches_tracked")
    p = {k: vo._t(np.asarray(v) if not torch.is_tensor(v) else v, dtype).clone().requires_grad_(True)
         for k, v in sd.items() if k.startswith(cfg.prefix) and not k.endswith(skip) and "criterion" not in k}
    if cfg.experts:     # rel_out.k IS rel_out_group.<last>.k
        for k in range(len(cfg.meet_groups)):
            for part in (".weight", ".bias"):
                p.pop(cfg.prefix + "rel_out.%d%s" % (k, part), None)
    rgb = vo._t(batch["roi_features"], dtype).clone().requires_grad_(True)
    dep = vo._t(batch["roi_depth_features"], dtype).clone().requires_grad_(True)

    emb, _ = vo.object_embeddings(p, cfg, batch["labels"], batch.get("predict_logits"), batch.get("pred_labels"), dtype)
    n_obj = len(np.asarray(batch["boxes"]))
    pos = vo.position_embedding(p, cfg, batch["boxes"], dtype, batch_stats=True,
                                drop=None if dropout is None else dropout.factor(od.SITE_POS, n_obj, 128, dtype))
    emb_c, pos_c = emb.detach().requires_grad_(True), pos.detach().requires_grad_(True)

    plan = _loss_plan(cfg, labels, loss, dtype)
    # denominators first: sum of w[y] over a loss's rows depends on the labels alone
    denom = []
    for name, c0, nc, rows, tgt, w in plan:
        keep = (tgt >= 0).to(dtype)
        denom.append(float((keep if w is None else w[tgt.clamp(min=0)] * keep).sum()))
    # row -> position in each loss's row list (-1: not chosen); a row is chosen at most once per group
    where = []
    for name, c0, nc, rows, tgt, w in plan:
        idx = torch.full((P,), -1, dtype=torch.long)
        idx[rows] = torch.arange(len(rows))
        where.append(idx)
    totals = [0.0] * len(plan)
    logits_out = []
    for a in range(0, P, pair_chunk):
        s, o = subj_t[a:a + pair_chunk], obj_t[a:a + pair_chunk]
        def site(k):      # the factor of token-row site k for this chunk's pairs: rows a * 19 .. of the whole step's numbering
            f = None if dropout is None else dropout.factor(k, len(s) * 19, cfg.dim, dtype, row0=a * 19)
            return None if f is None else f.reshape(len(s), 19, cfg.dim)
        x = vo.pair_tokens(p, cfg, emb_c, pos_c, rgb, dep, s, o, dtype, drop=site(od.SITE_EMB))
        for l in range(cfg.layers):
            x = vo.encoder_layer(p, cfg, x, l, dtype, drop=site(od.SITE_ATTN0 + l))
        Wh, bh = vo.head_weights(p, cfg, dtype)
        z = x[:, 0] @ Wh.t() + bh
        logits_out.append(z.detach())
        part = None
        for j, (name, c0, nc, rows, tgt, w) in enumerate(plan):
            at = where[j][a:a + pair_chunk]
            local = torch.nonzero(at >= 0)[:, 0]
            if len(local) == 0 or denom[j] == 0.0:
                continue
            zz = z[local, c0:(c0 + nc if nc is not None else z.shape[1])]
            terms, _ = _ce_terms(zz, tgt[at[local]], w)
            contrib = terms.sum() / denom[j]
            totals[j] += float(contrib.detach())
            part = contrib if part is None else part + contrib
        if part is not None:
            part.backward()
    torch.autograd.backward([emb, pos], [emb_c.grad if emb_c.grad is not None else torch.zeros_like(emb),
                                         pos_c.grad if pos_c.grad is not None else torch.zeros_like(pos)])
    losses = {name: (totals[j] if denom[j] > 0 else float("nan")) for j, (name, *_r) in enumerate(plan)}
    if cfg.mode != "predcls":   # :4129-4132 / :3823-3827: no parameter is behind it
        fg = torch.as_tensor(np.asarray(batch["labels"])).long()
        if cfg.meet_groups is None:
            src = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(batch["pred_labels"])).long(), p[cfg.prefix + "obj_embed.weight"].shape[0])
        else:
            src = vo._t(batch["predict_logits"], dtype)
        t, wsum = _ce_terms(src.to(dtype), fg, None)
        losses["obj_loss"] = float(t.sum() / wsum.sum())
    grads = {k: v.grad.detach() for k, v in p.items() if v.grad is not None}
    if cfg.experts:
        for k in range(len(cfg.meet_groups)):
            for part in (".weight", ".bias"):
                grads[cfg.prefix + "rel_out.%d%s" % (k, part)] = grads[cfg.prefix + "rel_out_group.%d.%d%s" % (cfg.experts - 1, k, part)]
    feat = vo.center_xywh_from_xyxy(vo._t(batch["boxes"], dtype))
    return {"losses": losses, "logits": torch.cat(logits_out), "grads": grads,
            "d_roi_features": rgb.grad.detach() if rgb.grad is not None else torch.zeros_like(rgb),
            "d_roi_depth_features": dep.grad.detach() if dep.grad is not None else torch.zeros_like(dep),
            "bn_batch_stats": (feat.mean(0), feat.var(0, unbiased=False), feat.var(0, unbiased=True) if len(feat) > 1 else None)}
