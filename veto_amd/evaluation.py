"""MI355X-native relation evaluation.

Host-side counterpart of the reference's per-image routine `evaluate_relation_of_one_image`
(pysgg/data/datasets/evaluation/vg/vg_eval.py:459-566) and of the evaluator classes it drives
(sgg_eval.py: SGRecall, SGNoGraphConstraintRecall, SGZeroShotRecall, SGPairAccuracy, SGMeanRecall,
SGNGMeanRecall) for the GT-box modes predcls / sgcls and for sgdet, where the predicted objects are the detector's (their
count differs from the GT count) and SGPairAccuracy records nothing, so A@K is NaN as in the reference
(sgg_eval.py:356, vg_eval.py:500-525).  The reference pulls every BoxList to the host and loops
in numpy; here the sorted predictions stay on the device, one launch (veto_sgg_eval) scores all images of the
batch, and only the final numbers (and, for inspection, the per-relation match ranks) come back.

`SGGEvaluator.evaluate(images)` takes per-image dicts with the reference's local_container names
(gt_rels, gt_classes, gt_boxes, pred_rel_inds, rel_scores, pred_classes, pred_boxes, obj_scores);
`evaluate_boxlists(groundtruths, predictions)` takes the BoxLists the reference's loop is fed with.
The result dict follows the reference's result_dict ('<mode>_recall' -> {20, 50, 100}, ...).

Over a split there are two ways to feed it.  update() / update_boxlists() read each batch's ranks back and finalize() folds them on
the host.  accumulate() / accumulate_boxlists() leave the per-relation records (three ranks, the zero-shot flag, the GT predicate)
in device buffers and read nothing back; finalize() then folds them in one veto_sgg_eval_fold call and makes one copy.  The fold's
summation order depends on the image sequence alone, so state() / load_state() (and distributed.all_gather_eval_state between
them) merge the records of several ranks into the bits of a single-rank run.

`DetectionEvaluator` is the "bbox" branch of the same routine (vg_eval.py:67-182): box mAP by pycocotools' COCOeval rules, fed
batch by batch like SGGEvaluator.update / finalize; `do_box_evaluation` is its drop-in form."""
import ctypes

import numpy as np
import torch

from . import native

KS = (20, 50, 100)
NO_MATCH = 0x3fffffff
RECORD_FIELDS = ("gc_rank", "ng_rank", "acc_rank", "zeroshot_flag", "gt_predicate")      # rows of SGGEvaluator's device records


def _t(x, dtype, device):
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    return x.to(device=device, dtype=dtype)


class SGGEvaluator:
    def __init__(self, mode, num_rel_category, zeroshot_triplet, iou_thres=0.5, device="cuda", reserve=4096):
        if mode not in ("predcls", "sgcls", "sgdet"):
            raise NotImplementedError("veto_amd.SGGEvaluator covers predcls / sgcls / sgdet, got %r" % (mode,))
        self.mode, self.num_rel, self.iou_thres = mode, int(num_rel_category), float(iou_thres)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("veto_amd.SGGEvaluator runs only on a HIP device (got %s)" % self.device)
        self.zeroshot = _t(zeroshot_triplet, torch.int64, self.device).reshape(-1, 3).contiguous()
        self._reserve_rows = max(int(reserve), 1)      # first capacity of the device-resident records (accumulate())
        self.reset()

    # ---- dataset-level accumulation (the reference's evaluators keep per-image lists over the WHOLE split and fold them once,
    # sgg_eval.py:133-136,209,331-336,420-466; per-batch results cannot be averaged into mR@K / A@K afterwards) --------------
    def reset(self):
        """Forgets everything accumulated by update() or accumulate()."""
        self._acc = []        # per evaluated image: (gc_rank, ng_rank, acc_rank, zeroshot flags, GT predicate of every GT relation)
        self._fed = None      # "update" (host lists in _acc) or "accumulate" (device records): one of the two between resets
        self._rec = None      # [5, capacity] int32 on the device: the RECORD_FIELDS of every GT relation seen by accumulate()
        self._rows = 0
        self._img_g, self._img_p = [], []      # per image: GT relations, predicted pairs
        self._scratch = {}    # images per batch -> the per-batch outputs nobody reads on this path

    def _feed(self, how):
        if self._fed not in (None, how):
            raise ValueError("veto_amd.SGGEvaluator: %s*() after %s*(); reset() first" % (how, self._fed))
        self._fed = how

    def update(self, images):
        """Scores one batch on the device (same launch as evaluate()) and keeps its per-relation match ranks for finalize().
        Returns the batch's own result dict."""
        self._feed("update")
        res = self.evaluate(images)
        for im, r in zip(images, res["per_image"]):
            if r is None:
                continue
            gt_pred = _t(im["gt_rels"], torch.int64, "cpu").reshape(-1, 3)[:, 2].numpy()
            self._acc.append((r["gc_rank"], r["ng_rank"], r["acc_rank"], r["zeroshot"], gt_pred))
        return res

    def update_boxlists(self, groundtruths, predictions):
        self._feed("update")
        res = self.evaluate_boxlists(groundtruths, predictions)
        for gt, r in zip(groundtruths, res["per_image"]):
            if r is None:
                continue
            gt_pred = _t(gt.get_field("relation_tuple"), torch.int64, "cpu").reshape(-1, 3)[:, 2].numpy()
            self._acc.append((r["gc_rank"], r["ng_rank"], r["acc_rank"], r["zeroshot"], gt_pred))
        return res

    def finalize(self):
        """Folds every image seen by update() the way the reference does at the end of the split: np.mean of the per-image
        recalls, A@K = mean(hits) / mean(counts), mean recall from the per-image per-class hit ratios.  After accumulate() the same
        fold runs on the device over the resident records (_finalize_records)."""
        if getattr(self, "_fed", None) == "accumulate":
            return self._finalize_records()
        C = self.num_rel
        res = {"images_evaluated": len(self._acc)}
        lists = {n: {k: [] for k in KS} for n in ("recall", "recall_nogc", "zeroshot_recall", "acc_hit", "acc_cnt")}
        coll = {n: {k: [[] for _ in range(C)] for k in KS} for n in ("mean_recall", "ng_mean_recall")}
        n_zs = 0
        for gc, ng, ac, zs, gt_pred in self._acc:
            G = len(gc)
            n_zs += bool(zs.any())
            for k in KS:
                hit, nghit = gc < k, ng < k
                lists["recall"][k].append(float(hit.sum()) / float(G))
                lists["recall_nogc"][k].append(float(nghit.sum()) / float(G))
                if zs.any():
                    lists["zeroshot_recall"][k].append(float((hit & zs).sum()) / float(zs.sum()))
                if self.mode != "sgdet":   # sgg_eval.py:356: SGPairAccuracy records nothing in sgdet -> A@K = NaN
                    lists["acc_hit"][k].append(float((ac < k).sum()))
                    lists["acc_cnt"][k].append(float(G))
                for name, h in (("mean_recall", hit), ("ng_mean_recall", nghit)):
                    cnt = np.bincount(gt_pred, minlength=C)
                    hc = np.bincount(gt_pred[h], minlength=C)
                    for n in np.nonzero(cnt[1:])[0] + 1:
                        coll[name][k][n].append(float(hc[n]) / float(cnt[n]))
        res["images_with_zeroshot"] = n_zs
        for name in ("recall", "recall_nogc", "zeroshot_recall"):
            res[name] = {k: (float(np.mean(v)) if len(v) else float("nan")) for k, v in lists[name].items()}
            res[name + "_list"] = lists[name]
        res["accuracy"] = {k: (float(np.mean(lists["acc_hit"][k]) / np.mean(lists["acc_cnt"][k])) if lists["acc_cnt"][k] else float("nan"))
                           for k in KS}
        for name in ("mean_recall", "ng_mean_recall"):
            res[name + "_list"] = {k: [float(np.mean(coll[name][k][n + 1])) if coll[name][k][n + 1] else 0.0 for n in range(C - 1)]
                                   for k in KS}
            res[name] = {k: sum(res[name + "_list"][k]) / float(C - 1) for k in KS}
        return res

    # ---- the same over device-resident records: no read-back per batch, one fold and one copy at the end of the split ------------
    def _reserve(self, rows):
        cap = 0 if self._rec is None else self._rec.shape[1]
        if rows <= cap:
            return
        # zeros: the flag rows of an image that is not evaluated are never written, and state() hands them out
        grown = torch.zeros((len(RECORD_FIELDS), max(rows, 2 * cap, self._reserve_rows)), dtype=torch.int32, device=self.device)
        if self._rows:
            grown[:, :self._rows] = self._rec[:, :self._rows]
        self._rec = grown

    def accumulate(self, images):
        """Scores one batch like update(), with the per-relation ranks and flags written straight into the evaluator's device
        buffers, and the GT predicates copied beside them on the device.  No device-to-host copy, no stream synchronisation;
        returns None.  finalize() folds the records of the whole split."""
        self._feed("accumulate")
        if not len(images):
            return None
        f, n_g, n_p = self._pack(images, record=True)
        n_img, sum_g, sum_p, r0 = len(images), sum(n_g), sum(n_p), self._rows
        if r0 + sum_g >= 1 << 31 or len(self._img_g) + n_img >= 1 << 31:
            raise ValueError("veto_amd.SGGEvaluator: a split holds fewer than 2^31 GT relations and images")
        self._reserve(r0 + sum_g + 1)      # + 1: a batch without a GT relation still hands the launch a valid pointer
        sc = self._scratch.get(n_img)
        if sc is None:
            i32 = torch.int32
            sc = self._scratch[n_img] = (torch.zeros((n_img, 100), dtype=i32, device=self.device),
                                         torch.zeros((n_img, 100), dtype=i32, device=self.device),
                                         torch.zeros(n_img, dtype=i32, device=self.device),
                                         torch.empty(18 + 6 * (self.num_rel - 1) + 2, dtype=torch.float64, device=self.device))
        rec = self._rec
        self._launch(f, sum_g, sum_p, gc_rank=rec[0, r0:], ng_rank=rec[1, r0:], acc_rank=rec[2, r0:], zeroshot_flag=rec[3, r0:],
                     ng_rows=sc[0], ng_cols=sc[1], ng_count=sc[2], metrics=sc[3])
        if sum_g:
            rec[4, r0:r0 + sum_g] = f["gt_rels"][:sum_g, 2]
        self._img_g += n_g
        self._img_p += n_p
        self._rows = r0 + sum_g
        return None

    def accumulate_boxlists(self, groundtruths, predictions):
        return self.accumulate(self._boxlist_images(groundtruths, predictions))

    def _finalize_records(self):
        """veto_sgg_eval_fold over the resident records, then ONE device-to-host copy: the metrics and the per-image quotients
        share a buffer.  The records stay, so a second call returns the same bits."""
        dev, C, n_img = self.device, self.num_rel, len(self._img_g)
        Cf, n_m = C - 1, 18 + 6 * (C - 1) + 2
        call = native.Launch(dev, "veto_amd.SGGEvaluator runs only on a HIP device")
        self._reserve(1)
        counts = np.zeros((2, n_img + 1), dtype=np.int64)
        np.cumsum(np.asarray(self._img_g, dtype=np.int64), out=counts[0, 1:])
        counts[1, :n_img] = self._img_p
        counts = torch.from_numpy(counts.astype(np.int32)).to(dev)      # the one upload: offsets | pair counts
        out = torch.empty(n_m + 12 * n_img, dtype=torch.float64, device=dev)
        rec = self._rec
        a = call.args(native.VetoSggEvalFoldArgs, n_img=n_img, n_rel_cls=C, mode=1 if self.mode == "sgdet" else 0,
                      n_gt_total=self._rows, img_gt_offset=counts[0], img_pair_count=counts[1], gt_predicate=rec[4],
                      gc_rank=rec[0], ng_rank=rec[1], acc_rank=rec[2], zeroshot_flag=rec[3], metrics=out,
                      per_image=out[n_m:] if n_img else None)
        ws = call.workspace(call.lib.veto_sgg_eval_fold_workspace_bytes(n_img, C))
        call.run("veto_sgg_eval_fold", ctypes.byref(a), ws.data_ptr(), ws.numel())
        h = out.cpu().numpy()
        m, per = h[:n_m], h[n_m:].reshape(n_img, 12)
        res = {"images_evaluated": int(m[18 + 6 * Cf]), "images_with_zeroshot": int(m[18 + 6 * Cf + 1])}
        for j, name in enumerate(("recall", "recall_nogc", "zeroshot_recall", "accuracy", "mean_recall", "ng_mean_recall")):
            res[name] = {k: float(m[3 * j + i]) for i, k in enumerate(KS)}
        for kind, name in enumerate(("mean_recall_list", "ng_mean_recall_list")):
            res[name] = {k: m[18 + (kind * 3 + i) * Cf: 18 + (kind * 3 + i + 1) * Cf].tolist() for i, k in enumerate(KS)}
        for j, name in enumerate(("recall_list", "recall_nogc_list", "zeroshot_recall_list")):      # NaN: the image is not in the list
            res[name] = {k: per[~np.isnan(per[:, 3 * j + i]), 3 * j + i].tolist() for i, k in enumerate(KS)}
        return res

    def state(self):
        """The records as a dict of tensors trimmed to their rows (RECORD_FIELDS: [sum G] int32 each) plus the per-image counts
        'gt_count' and 'pair_count' ([images] int64): what load_state() and distributed.all_gather_eval_state() take."""
        self._feed("accumulate")
        self._reserve(1)
        st = {name: self._rec[i, :self._rows].clone() for i, name in enumerate(RECORD_FIELDS)}
        st["gt_count"] = torch.tensor(self._img_g, dtype=torch.int64).to(self.device)
        st["pair_count"] = torch.tensor(self._img_p, dtype=torch.int64).to(self.device)
        return st

    def load_state(self, states):
        """Replaces the records by the concatenation of `states` (dicts as state() returns them, on any device) in list order:
        with the contiguous shards of distributed.shard_images, rank-major order is dataset order and finalize() returns the
        bits of a single-rank run."""
        states = list(states)
        for st in states:
            rows = [int(st[name].numel()) for name in RECORD_FIELDS]
            if len(set(rows)) != 1 or st["gt_count"].numel() != st["pair_count"].numel() or int(st["gt_count"].sum()) != rows[0]:
                raise ValueError("veto_amd.SGGEvaluator.load_state: the fields of a state disagree about its rows")
        self.reset()
        self._fed = "accumulate"
        for st in states:
            self._img_g += [int(x) for x in st["gt_count"].tolist()]
            self._img_p += [int(x) for x in st["pair_count"].tolist()]
        rows = sum(self._img_g)
        if rows >= 1 << 31 or len(self._img_g) >= 1 << 31:
            raise ValueError("veto_amd.SGGEvaluator: a split holds fewer than 2^31 GT relations and images")
        self._reserve(rows + 1)
        for i, name in enumerate(RECORD_FIELDS):
            if rows:
                self._rec[i, :rows] = torch.cat([_t(st[name], torch.int32, self.device).reshape(-1) for st in states])
        self._rows = rows

    def evaluate_boxlists(self, groundtruths, predictions):
        """vg_eval.py:470-498: unpack the fields of the GT / prediction BoxLists."""
        return self.evaluate(self._boxlist_images(groundtruths, predictions))

    @staticmethod
    def _boxlist_images(groundtruths, predictions):
        images = []
        for gt, pr in zip(groundtruths, predictions):
            images.append({
                "gt_rels": gt.get_field("relation_tuple"), "gt_classes": gt.get_field("labels"), "gt_boxes": gt.convert("xyxy").bbox,
                "pred_rel_inds": pr.get_field("rel_pair_idxs"), "rel_scores": pr.get_field("pred_rel_scores"),
                "pred_classes": pr.get_field("pred_labels"), "pred_boxes": pr.convert("xyxy").bbox,
                "obj_scores": pr.get_field("pred_scores")})
        return images

    def _pack(self, images, record=False):
        """The batch as veto_sgg_eval takes it: concatenated device tensors, the offset arrays and the per-image counts.
        record: keep the caller's device tensors alive on the current stream (a path that never synchronises may read them while
        the stream that made them has moved on and released them)."""
        dev = self.device
        i64, f32 = torch.int64, torch.float32
        stream = torch.cuda.current_stream(dev)
        def cat(key, dtype, shape):
            parts = [_t(im[key], dtype, dev).reshape(shape) for im in images]
            if record:
                for p in parts:
                    p.record_stream(stream)
            t = torch.cat(parts, 0).contiguous()
            # an all-empty field still needs a valid device pointer for the ABI's argument check
            return t if t.numel() else torch.zeros((1,) + tuple(abs(d) for d in shape[1:]), dtype=dtype, device=dev)
        gt_rels = cat("gt_rels", i64, (-1, 3))
        gt_classes, gt_boxes = cat("gt_classes", i64, (-1,)), cat("gt_boxes", f32, (-1, 4))
        pred_pairs, rel_scores = cat("pred_rel_inds", i64, (-1, 2)), cat("rel_scores", f32, (-1, self.num_rel))
        if self.mode == "predcls":   # vg_eval.py:517-520
            pred_classes, pred_boxes = gt_classes, gt_boxes
            obj_scores = torch.ones(gt_classes.shape[0], dtype=f32, device=dev)
        else:
            pred_classes, pred_boxes = cat("pred_classes", i64, (-1,)), cat("pred_boxes", f32, (-1, 4))
            obj_scores = cat("obj_scores", f32, (-1,))
            if self.mode == "sgcls" and pred_boxes.shape[0] != gt_boxes.shape[0]:
                raise ValueError("sgcls: the number of predicted boxes must equal the number of GT boxes")
        rows = lambda x, width: int(x.numel() // width) if isinstance(x, torch.Tensor) else int(np.asarray(x).size // width)
        n_g = [rows(im["gt_rels"], 3) for im in images]
        n_o = [int(len(im["gt_classes"])) for im in images]
        n_p = [rows(im["pred_rel_inds"], 2) for im in images]
        pred_off = None
        if self.mode == "sgdet":   # the detector's objects: their own count per image (vg_eval.py:491-495)
            n_q = [rows(im["pred_classes"], 1) for im in images]
            if [rows(im["pred_boxes"], 4) for im in images] != n_q or [rows(im["obj_scores"], 1) for im in images] != n_q:
                raise ValueError("sgdet: pred_classes, pred_boxes and obj_scores must have one row per predicted object")
            pred_off = native.device_offsets(n_q, device=dev)[0]
        off = native.device_offsets(n_g, n_o, n_p, device=dev)
        fields = dict(n_img=len(images), n_rel_cls=self.num_rel, n_zeroshot=int(self.zeroshot.shape[0]), iou_thres=self.iou_thres,
                      gt_offset=off[0], obj_offset=off[1], pair_offset=off[2], gt_rels=gt_rels, gt_classes=gt_classes,
                      gt_boxes=gt_boxes, pred_pairs=pred_pairs, rel_scores=rel_scores, pred_classes=pred_classes,
                      pred_boxes=pred_boxes, obj_scores=obj_scores, zeroshot=self.zeroshot,
                      reserved0=1 if pred_off is not None else 0, pred_obj_offset=pred_off)
        return fields, n_g, n_p

    def _launch(self, f, sum_g, sum_p, gc_rank, ng_rank, acc_rank, zeroshot_flag, ng_rows, ng_cols, ng_count, metrics):
        """veto_sgg_eval on a batch packed by _pack(), writing to the given output tensors."""
        call = native.Launch(self.device, "veto_amd.SGGEvaluator runs only on a HIP device")
        a = call.args(native.VetoSggEvalArgs, n_img=f["n_img"], n_rel_cls=f["n_rel_cls"], n_zeroshot=f["n_zeroshot"],
                      iou_thres=f["iou_thres"], gt_offset=f["gt_offset"], obj_offset=f["obj_offset"], pair_offset=f["pair_offset"],
                      gt_rels=f["gt_rels"], gt_classes=f["gt_classes"], gt_boxes=f["gt_boxes"], pred_pairs=f["pred_pairs"],
                      rel_scores=f["rel_scores"], pred_classes=f["pred_classes"], pred_boxes=f["pred_boxes"],
                      obj_scores=f["obj_scores"], zeroshot=f["zeroshot"], reserved0=f["reserved0"],
                      pred_obj_offset=f["pred_obj_offset"], gc_rank=gc_rank, ng_rank=ng_rank, acc_rank=acc_rank,
                      zeroshot_flag=zeroshot_flag, ng_rows=ng_rows, ng_cols=ng_cols, ng_count=ng_count, metrics=metrics)
        ws = call.workspace(call.lib.veto_sgg_eval_workspace_bytes(f["n_img"], sum_p, sum_g, self.num_rel))
        call.run("veto_sgg_eval", ctypes.byref(a), sum_p, sum_g, ws.data_ptr(), ws.numel())

    def evaluate(self, images):
        dev = self.device
        i32 = torch.int32
        fields, n_g, n_p = self._pack(images)
        n_img, sum_g, sum_p, C = len(images), sum(n_g), sum(n_p), self.num_rel
        out = {k: torch.empty(max(sum_g, 1), dtype=i32, device=dev) for k in ("gc_rank", "ng_rank", "acc_rank", "zeroshot_flag")}
        ng_rows = torch.zeros((n_img, 100), dtype=i32, device=dev)
        ng_cols = torch.zeros((n_img, 100), dtype=i32, device=dev)
        ng_count = torch.zeros(n_img, dtype=i32, device=dev)
        metrics = torch.empty(18 + 6 * (C - 1) + 2, dtype=torch.float64, device=dev)
        self._launch(fields, sum_g, sum_p, ng_rows=ng_rows, ng_cols=ng_cols, ng_count=ng_count, metrics=metrics, **out)
        m = metrics.cpu().numpy()
        Cf = C - 1
        res = {"images_evaluated": int(m[18 + 6 * Cf]), "images_with_zeroshot": int(m[18 + 6 * Cf + 1])}
        for j, name in enumerate(("recall", "recall_nogc", "zeroshot_recall", "accuracy", "mean_recall", "ng_mean_recall")):
            res[name] = {k: float(m[3 * j + i]) for i, k in enumerate(KS)}
        if self.mode == "sgdet":
            res["accuracy"] = {k: float("nan") for k in KS}
        for kind, name in enumerate(("mean_recall_list", "ng_mean_recall_list")):
            res[name] = {k: m[18 + (kind * 3 + i) * Cf: 18 + (kind * 3 + i + 1) * Cf].tolist() for i, k in enumerate(KS)}
        # per-image views (what the reference keeps as lists in its result_dict), from the match ranks
        host = {k: v.cpu().numpy() for k, v in out.items()}
        ngc, ngr, ngk = ng_count.cpu().numpy(), ng_rows.cpu().numpy(), ng_cols.cpu().numpy()
        res["per_image"] = []
        lists = {n: {k: [] for k in KS} for n in ("recall_list", "recall_nogc_list", "zeroshot_recall_list")}
        g0 = 0
        for i in range(n_img):
            G = n_g[i]
            if G == 0 or n_p[i] == 0:
                res["per_image"].append(None)
                g0 += G
                continue
            sl = slice(g0, g0 + G)
            zs = host["zeroshot_flag"][sl].astype(bool)
            res["per_image"].append({"gc_rank": host["gc_rank"][sl].astype(np.int64), "ng_rank": host["ng_rank"][sl].astype(np.int64),
                                     "acc_rank": host["acc_rank"][sl].astype(np.int64), "zeroshot": zs,
                                     "ng_rows": ngr[i, :ngc[i]], "ng_cols": ngk[i, :ngc[i]]})
            for k in KS:
                hit = host["gc_rank"][sl] < k
                lists["recall_list"][k].append(float(hit.sum()) / float(G))
                lists["recall_nogc_list"][k].append(float((host["ng_rank"][sl] < k).sum()) / float(G))
                if zs.any():
                    lists["zeroshot_recall_list"][k].append(float((hit & zs).sum()) / float(zs.sum()))
            g0 += G
        res.update(lists)
        return res

    def generate_print_string(self, res):
        """The lines the reference logs (sgg_eval.py generate_print_string of the six evaluators).  sgdet: the A@K line reads
        nan, as the reference's mean over an empty list does."""
        fmt = lambda tag, d: "".join(" %s @ %d: %.4f; " % (tag, k, d[k]) for k in KS)
        m = self.mode
        return ("SGG eval: " + fmt(" R", res["recall"]) + " for mode=%s, type=Recall(Main).\n" % m +
                "SGG eval: " + fmt("ngR", res["recall_nogc"]) + " for mode=%s, type=No Graph Constraint Recall(Main).\n" % m +
                "SGG eval: " + fmt(" zR", res["zeroshot_recall"]) + " for mode=%s, type=Zero Shot Recall.\n" % m +
                "SGG eval: " + fmt(" mR", res["mean_recall"]) + " for mode=%s, type=Mean Recall.\n" % m +
                "SGG eval: " + fmt("ng-mR", res["ng_mean_recall"]) + " for mode=%s, type=No Graph Constraint Mean Recall.\n" % m +
                "SGG eval: " + fmt("  A", res["accuracy"]) + " for mode=%s, type=TopK Accuracy.\n" % m)


# ---- detection (box mAP) evaluation: the "bbox" branch of do_vg_evaluation (vg_eval.py:67-182) ------------------------------------
# COCOeval's Params for iouType 'bbox', formed as pycocotools forms them so that the device gets numpy's bits
DET_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
DET_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
DET_MAX_DETS = (1, 10, 100)
DET_AREA_RNGS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
DET_STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl")      # COCOResults('bbox'): stats[0..5]


class DetectionEvaluator:
    """COCOeval.evaluate() / accumulate() / summarize() over a split, on the device (veto_det_eval_match per batch,
    veto_det_eval_accumulate once).  update() appends one record per detection to device buffers that grow geometrically and reads
    nothing back; finalize() returns precision [10, 101, C-1, 4, 3], recall [10, C-1, 4, 3], stats [12], 'mAp' (= stats[1], AP at
    IoU 0.5: what the reference calls mAp), 'recall@100_iou0.5' and COCOResults('bbox')'s six names.

    first_gt_id: the annotation id of the split's first GT box.  vg_eval.py:78 numbers from 0 and COCOeval tests the id for truth,
    so with 0 (the default: the reference's numbers) a detection matched to the very first GT box of the split counts as unmatched;
    1 is the COCO-correct count.

    Limits (include/veto_amd.h): 2..1024 classes, 1024 GT boxes and 1024 detections per image, fewer than 2^31 detections per
    split.  Labels must lie in 1..C-1: labels given on the host are checked in update(); labels that already live on the device
    are checked there and reported by finalize().  Scores must be finite."""

    def __init__(self, num_classes, device="cuda", first_gt_id=0):
        self.num_classes, self.first_gt_id = int(num_classes), int(first_gt_id)
        if not 2 <= self.num_classes <= 1024:
            raise ValueError("veto_amd.DetectionEvaluator: num_classes %d outside 2..1024" % self.num_classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("veto_amd.DetectionEvaluator runs only on a HIP device (got %s)" % self.device)
        self.reset()

    def reset(self):
        """Forgets everything accumulated by update()."""
        self._rows = self._gts = 0
        self._rec = None                      # [3, capacity] int64: the key / match / ignore words of every record
        self._gt_counts = torch.zeros((self.num_classes - 1, 4), dtype=torch.int64, device=self.device)
        self._label_errors = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _reserve(self, rows):
        cap = 0 if self._rec is None else self._rec.shape[1]
        if rows <= cap:
            return
        grown = torch.empty((3, max(rows, 2 * cap, 4096)), dtype=torch.int64, device=self.device)
        if self._rows:
            grown[:, :self._rows] = self._rec[:, :self._rows]
        self._rec = grown

    def _labels(self, x, what):
        if not (isinstance(x, torch.Tensor) and x.device.type == "cuda"):      # on the host: refuse here
            lab = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1)
            if lab.size and (lab.min() < 1 or lab.max() >= self.num_classes):
                raise ValueError("veto_amd.DetectionEvaluator: %s outside 1..%d" % (what, self.num_classes - 1))
        return _t(x, torch.int64, self.device).reshape(-1)

    def update(self, images):
        """Matches one batch (dicts with gt_boxes, gt_classes, pred_boxes, pred_classes, obj_scores) and appends its records."""
        if not len(images):
            return
        dev = self.device
        call = native.Launch(dev, "veto_amd.DetectionEvaluator runs only on a HIP device")
        f32 = torch.float32
        gt_labels = [self._labels(im["gt_classes"], "gt_classes") for im in images]
        det_labels = [self._labels(im["pred_classes"], "pred_classes") for im in images]
        gt_boxes = [_t(im["gt_boxes"], f32, dev).reshape(-1, 4) for im in images]
        det_boxes = [_t(im["pred_boxes"], f32, dev).reshape(-1, 4) for im in images]
        det_scores = [_t(im["obj_scores"], f32, dev).reshape(-1) for im in images]
        n_g, n_d = [int(x.shape[0]) for x in gt_labels], [int(x.shape[0]) for x in det_labels]
        if [int(x.shape[0]) for x in gt_boxes] != n_g or [int(x.shape[0]) for x in det_boxes] != n_d or \
                [int(x.shape[0]) for x in det_scores] != n_d:
            raise ValueError("veto_amd.DetectionEvaluator: one box per label and one score per detection")
        n_img, sum_g, sum_d = len(images), sum(n_g), sum(n_d)
        self._reserve(max(self._rows + sum_d, 1))      # a batch without a detection still counts its GT boxes
        off = native.device_offsets(n_g, n_d, device=dev)
        host_g = (ctypes.c_int32 * (n_img + 1))(0, *np.cumsum(n_g).tolist())
        host_d = (ctypes.c_int32 * (n_img + 1))(0, *np.cumsum(n_d).tolist())
        a = call.args(native.VetoDetEvalMatchArgs, n_img=n_img, n_cls=self.num_classes, n_gt=sum_g, n_det=sum_d,
                      first_gt_id=self.first_gt_id + self._gts, row_offset=self._rows,
                      iou_thrs=(ctypes.c_double * 10)(*DET_IOU_THRS.tolist()),
                      area_rngs=(ctypes.c_double * 8)(*[float(v) for r in DET_AREA_RNGS for v in r]),
                      gt_offset=off[0], det_offset=off[1],
                      gt_offset_host=ctypes.cast(host_g, ctypes.c_void_p), det_offset_host=ctypes.cast(host_d, ctypes.c_void_p),
                      gt_boxes=torch.cat(gt_boxes).contiguous(), gt_labels=torch.cat(gt_labels).contiguous(),
                      det_boxes=torch.cat(det_boxes).contiguous(), det_scores=torch.cat(det_scores).contiguous(),
                      det_labels=torch.cat(det_labels).contiguous(),
                      rec_key=self._rec[0], rec_match=self._rec[1], rec_ignore=self._rec[2],
                      gt_counts=self._gt_counts, label_errors=self._label_errors)
        ws = call.workspace(call.lib.veto_det_eval_match_workspace_bytes(n_img, sum_g, sum_d))
        call.run("veto_det_eval_match", ctypes.byref(a), ws.data_ptr(), ws.numel())
        self._rows += sum_d
        self._gts += sum_g

    def update_boxlists(self, groundtruths, predictions, mode="sgdet"):
        """vg_eval.py:70-108: the fields of the GT / prediction BoxLists; predcls: the labels are the GT 'labels', the scores 1."""
        images = []
        for gt, pr in zip(groundtruths, predictions):
            boxes = pr.convert("xyxy").bbox
            if mode == "predcls":
                labels = pr.get_field("labels")
                scores = torch.ones(int(labels.shape[0]), dtype=torch.float32, device=labels.device)
            else:
                labels, scores = pr.get_field("pred_labels"), pr.get_field("pred_scores")
            images.append({"gt_boxes": gt.convert("xyxy").bbox, "gt_classes": gt.get_field("labels"), "pred_boxes": boxes,
                           "pred_classes": labels, "obj_scores": scores})
        self.update(images)

    def finalize(self):
        """Sorts and folds every record appended since reset(); the one place that reads anything back.

        Raises ValueError when a label outside 1..C-1 was met on the device.  The kernel has left those boxes out, so the tables
        of this split are not returned and the error stays set: every later finalize() raises again until reset()."""
        dev, K = self.device, self.num_classes - 1
        call = native.Launch(dev, "veto_amd.DetectionEvaluator runs only on a HIP device")
        self._reserve(1)
        f64 = torch.float64
        precision = torch.empty((10, 101, K, 4, 3), dtype=f64, device=dev)
        recall = torch.empty((10, K, 4, 3), dtype=f64, device=dev)
        tail = torch.empty(13, dtype=f64, device=dev)       # stats [12] | recall50_100
        a = call.args(native.VetoDetEvalAccumulateArgs, n_cls=self.num_classes, n_rec=self._rows,
                      iou_thrs=(ctypes.c_double * 10)(*DET_IOU_THRS.tolist()), rec_thrs=(ctypes.c_double * 101)(*DET_REC_THRS.tolist()),
                      rec_key=self._rec[0], rec_match=self._rec[1], rec_ignore=self._rec[2], gt_counts=self._gt_counts,
                      precision=precision, recall=recall, stats=tail, recall50_100=tail[12:])
        ws = call.workspace(call.lib.veto_det_eval_accumulate_workspace_bytes(self._rows, self.num_classes))
        call.run("veto_det_eval_accumulate", ctypes.byref(a), ws.data_ptr(), ws.numel())
        bad = int(self._label_errors.item())
        if bad:
            raise ValueError("veto_amd.DetectionEvaluator: %d labels outside 1..%d were met on the device" % (bad, K))
        t = tail.cpu().numpy()
        res = {"precision": precision.cpu().numpy(), "recall": recall.cpu().numpy(), "stats": t[:12].copy(),
               "mAp": float(t[1]), "recall@100_iou0.5": float(t[12])}
        res.update({name: float(t[i]) for i, name in enumerate(DET_STAT_NAMES)})
        return res

    def evaluate(self, images):
        self.reset()
        self.update(images)
        return self.finalize()

    def evaluate_boxlists(self, groundtruths, predictions, mode="sgdet"):
        self.reset()
        self.update_boxlists(groundtruths, predictions, mode)
        return self.finalize()


def do_box_evaluation(groundtruths, predictions, mode, num_classes, device="cuda", first_gt_id=0):
    """The "bbox" branch of do_vg_evaluation: (mAp, result_str, coco_res_to_save) with the two lines of vg_eval.py:176-178."""
    res = DetectionEvaluator(num_classes, device=device, first_gt_id=first_gt_id).evaluate_boxlists(groundtruths, predictions, mode)
    result_str = "Detection evaluation mAp=%.4f\n" % res["mAp"]
    result_str += "recall@%d IOU:0.5 %.4f\n" % (DET_MAX_DETS[-1], res["recall@100_iou0.5"])
    return res["mAp"], result_str, {"bbox/%s" % name: res[name] for name in DET_STAT_NAMES}
