"""The detection (box mAP) evaluator on the device against the numpy restatement of COCOeval (tests/det_eval_cases.py; its
premises are asserted by test_det_eval_host.py; it has never been run against pycocotools): precision and recall bit for bit,
stats and recall@100 within 1e-12 (numpy's pairwise mean against a fixed-order sum), every call twice with the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import det_eval_cases as dc
from veto_amd import native
from veto_amd.evaluation import DET_AREA_RNGS, DET_IOU_THRS, DET_REC_THRS, DetectionEvaluator, do_box_evaluation
from veto_amd.structures import BoxList

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run_case(case, batches=None):
    ev = DetectionEvaluator(case["num_classes"], device=DEV, first_gt_id=case["first_gt_id"])
    for batch in case["batches"] if batches is None else batches:
        ev.update(batch)
    return ev.finalize()


def compare(name, got, want):
    p_eq = int((got["precision"] == want["precision"]).sum())
    r_eq = int((got["recall"] == want["recall"]).sum())
    err = max(float(np.abs(got["stats"] - want["stats"]).max()), abs(got["recall@100_iou0.5"] - want["recall50_100"]))
    print("det_eval %-22s precision %d / %d equal, recall %d / %d equal, stats error %.3e"
          % (name, p_eq, want["precision"].size, r_eq, want["recall"].size, err))
    assert got["precision"].shape == want["precision"].shape and got["recall"].shape == want["recall"].shape
    assert p_eq == want["precision"].size and r_eq == want["recall"].size
    assert err <= 1e-12
    assert got["mAp"] == got["stats"][1] and got["AP75"] == got["stats"][2] and got["APl"] == got["stats"][5]


@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_evaluator_matches_the_restatement_bit_for_bit(name):
    case = dc.cases()[name]
    got, again = run_case(case), run_case(case)
    for key in ("precision", "recall", "stats"):
        assert np.array_equal(got[key], again[key]), key
    assert got["recall@100_iou0.5"] == again["recall@100_iou0.5"]
    compare(name, got, dc.expected(name))


def test_batching_does_not_change_a_bit():
    case = dc.cases()["realistic"]
    four, one = run_case(case), run_case(case, batches=[dc.flat_images(case)])
    for key in ("precision", "recall", "stats"):
        assert np.array_equal(four[key], one[key]), key
    ev = DetectionEvaluator(case["num_classes"], device=DEV)        # the one-shot form, with the inputs already on the device
    on_dev = [{k: torch.as_tensor(v).to(DEV) for k, v in im.items()} for im in dc.flat_images(case)]
    shot = ev.evaluate(on_dev)
    assert np.array_equal(shot["precision"], four["precision"]) and np.array_equal(shot["stats"], four["stats"])


def test_library_sizes_are_the_ones_the_cases_are_built_for():
    lib = native.load_library()
    v = [ctypes.c_int32() for _ in range(4)]
    assert lib.veto_det_eval_limits(*[ctypes.byref(x) for x in v]) == 0
    assert v[0].value >= 256 and v[1].value >= 1024
    assert (v[2].value, v[3].value) == (dc.SCAN_CHUNK, dc.SORT_TILE)


class Raw:
    """The two entry points called directly on one batch, with the caller's own buffers."""

    def __init__(self, images, n_cls, first_gt_id=0, rows=None):
        cat = lambda key, dtype, shape: torch.cat([torch.as_tensor(np.asarray(im[key])).reshape(shape) for im in images]).to(DEV, dtype).contiguous()
        self.n_g = [len(im["gt_classes"]) for im in images]
        self.n_d = [len(im["obj_scores"]) for im in images]
        self.t = dict(gt_boxes=cat("gt_boxes", torch.float32, (-1, 4)), gt_labels=cat("gt_classes", torch.int64, (-1,)),
                      det_boxes=cat("pred_boxes", torch.float32, (-1, 4)), det_scores=cat("obj_scores", torch.float32, (-1,)),
                      det_labels=cat("pred_classes", torch.int64, (-1,)))
        n_img, self.n_gt, self.n_det = len(images), sum(self.n_g), sum(self.n_d)
        self.n_cls = n_cls
        self.off = native.device_offsets(self.n_g, self.n_d, device=DEV)
        self.host_g = (ctypes.c_int32 * (n_img + 1))(0, *np.cumsum(self.n_g).tolist())
        self.host_d = (ctypes.c_int32 * (n_img + 1))(0, *np.cumsum(self.n_d).tolist())
        self.rec = torch.zeros((3, max(self.n_det if rows is None else rows, 1)), dtype=torch.int64, device=DEV)
        self.counts = torch.zeros((max(n_cls - 1, 1), 4), dtype=torch.int64, device=DEV)
        self.errors = torch.zeros(1, dtype=torch.int32, device=DEV)
        a = native.VetoDetEvalMatchArgs(struct_size=ctypes.sizeof(native.VetoDetEvalMatchArgs), n_img=n_img, n_cls=n_cls,
                                        n_gt=self.n_gt, n_det=self.n_det, first_gt_id=first_gt_id, row_offset=0)
        a.iou_thrs = (ctypes.c_double * 10)(*DET_IOU_THRS.tolist())
        a.area_rngs = (ctypes.c_double * 8)(*[float(v) for r in DET_AREA_RNGS for v in r])
        a.gt_offset, a.det_offset = self.off[0].data_ptr(), self.off[1].data_ptr()
        a.gt_offset_host, a.det_offset_host = ctypes.addressof(self.host_g), ctypes.addressof(self.host_d)
        for k, v in self.t.items():
            setattr(a, k, v.data_ptr() if v.numel() else None)
        a.rec_key, a.rec_match, a.rec_ignore = (self.rec[i].data_ptr() for i in range(3))
        a.gt_counts, a.label_errors = self.counts.data_ptr(), self.errors.data_ptr()
        self.args = a
        self.lib = native.load_library()
        need = self.lib.veto_det_eval_match_workspace_bytes(n_img, self.n_gt, self.n_det)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        self.ws_need = need

    def match(self, ws_bytes=None):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return self.lib.veto_det_eval_match(stream, ctypes.byref(self.args), self.ws.data_ptr(), self.ws_need if ws_bytes is None else ws_bytes)

    def accumulate_args(self):
        K = self.n_cls - 1
        self.out = dict(precision=torch.empty((10, 101, K, 4, 3), dtype=torch.float64, device=DEV),
                        recall=torch.empty((10, K, 4, 3), dtype=torch.float64, device=DEV),
                        stats=torch.empty(12, dtype=torch.float64, device=DEV), recall50_100=torch.empty(1, dtype=torch.float64, device=DEV))
        b = native.VetoDetEvalAccumulateArgs(struct_size=ctypes.sizeof(native.VetoDetEvalAccumulateArgs), n_cls=self.n_cls, n_rec=self.n_det)
        b.iou_thrs = (ctypes.c_double * 10)(*DET_IOU_THRS.tolist())
        b.rec_thrs = (ctypes.c_double * 101)(*DET_REC_THRS.tolist())
        b.rec_key, b.rec_match, b.rec_ignore = (self.rec[i].data_ptr() for i in range(3))
        b.gt_counts = self.counts.data_ptr()
        for k, v in self.out.items():
            setattr(b, k, v.data_ptr())
        return b

    def accumulate(self, b, ws_short=0):
        need = self.lib.veto_det_eval_accumulate_workspace_bytes(b.n_rec, b.n_cls)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.veto_det_eval_accumulate(stream, ctypes.byref(b), ws.data_ptr(), need - ws_short)
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("name", ["segments_%d" % (dc.SORT_TILE + 1), "score_ties", "gt_only_split"])
def test_raw_abi_matches_the_restatement(name):
    case = dc.cases()[name]
    want = dc.expected(name)
    results = []
    for _ in range(2):
        raw = Raw(dc.flat_images(case), case["num_classes"], case["first_gt_id"])
        assert raw.match() == 0, raw.lib.veto_last_error()
        assert raw.accumulate(raw.accumulate_args()) == 0, raw.lib.veto_last_error()
        assert int(raw.errors.item()) == 0
        results.append({k: v.cpu().numpy() for k, v in raw.out.items()})
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), k
    assert np.array_equal(results[0]["precision"], want["precision"]) and np.array_equal(results[0]["recall"], want["recall"])
    assert np.abs(results[0]["stats"] - want["stats"]).max() <= 1e-12 and abs(results[0]["recall50_100"][0] - want["recall50_100"]) <= 1e-12


def _boxes(n, cls=1):
    return dc.image(gt=[(cls, 0, 0, 9, 9)] * n[0], det=[(cls, .5, 0, 0, 9, 9)] * n[1])


def test_refusals_launch_nothing():
    lib = native.load_library()
    err = lambda: lib.veto_last_error().decode()
    max_gt, max_det = ctypes.c_int32(), ctypes.c_int32()
    lib.veto_det_eval_limits(ctypes.byref(max_gt), ctypes.byref(max_det), None, None)
    ok = Raw([_boxes((max_gt.value, max_det.value))], 3)              # exactly at the limits: accepted
    assert ok.match() == 0, err()
    torch.cuda.synchronize()
    untouched = torch.full((3, max_det.value + 1), 7, dtype=torch.int64, device=DEV)

    def refused(raw, needle, **fields):
        raw.rec = untouched.clone()
        raw.args.rec_key, raw.args.rec_match, raw.args.rec_ignore = (raw.rec[i].data_ptr() for i in range(3))
        for k, v in fields.items():
            setattr(raw.args, k, v)
        assert raw.match() < 0
        assert needle in err(), err()
        torch.cuda.synchronize()
        assert bool((raw.rec == 7).all()) and int(raw.counts.sum()) == 0      # nothing was launched

    refused(Raw([_boxes((max_gt.value + 1, 1))], 3), "limit is %d" % max_gt.value)
    refused(Raw([_boxes((1, max_det.value + 1))], 3), "limit is %d" % max_det.value)
    refused(Raw([_boxes((1, 1))], 3), "n_cls", n_cls=1)
    refused(Raw([_boxes((1, 1))], 3), "n_cls", n_cls=1025)
    refused(Raw([_boxes((1, 1))], 3), "2^31", row_offset=(1 << 31) - 1)
    refused(Raw([_boxes((1, 1))], 3), "size mismatch", struct_size=ctypes.sizeof(native.VetoDetEvalMatchArgs) - 8)
    raw = Raw([_boxes((1, 1))], 3)
    raw.rec = untouched.clone()
    raw.args.rec_key, raw.args.rec_match, raw.args.rec_ignore = (raw.rec[i].data_ptr() for i in range(3))
    assert raw.match(raw.ws_need - 1) == -4 and "workspace too small" in err()
    torch.cuda.synchronize()
    assert bool((raw.rec == 7).all())
    # accumulate: a short struct, the record limit, a workspace one byte too small; the outputs stay as they were
    raw = Raw([_boxes((1, 1))], 3)
    assert raw.match() == 0
    for change, needle in ((dict(struct_size=8), "size mismatch"), (dict(n_rec=1 << 31), "n_rec"), (dict(n_cls=1025), "n_cls")):
        b = raw.accumulate_args()
        for k, v in change.items():
            setattr(b, k, v)
        raw.out["stats"].fill_(7.0)
        assert raw.accumulate(b) < 0 and needle in err(), err()
        assert bool((raw.out["stats"] == 7.0).all())
    b = raw.accumulate_args()
    raw.out["stats"].fill_(7.0)
    assert raw.accumulate(b, ws_short=1) == -4 and "workspace too small" in err()
    assert bool((raw.out["stats"] == 7.0).all())
    assert lib.veto_det_eval_accumulate_workspace_bytes(1 << 31, 3) == 0 and lib.veto_det_eval_accumulate_workspace_bytes(10, 1025) == 0


def test_labels_outside_the_classes_are_refused():
    ev = DetectionEvaluator(3, device=DEV)
    for bad in (0, 3):
        with pytest.raises(ValueError, match="outside 1..2"):
            ev.update([dc.image(gt=[(1, 0, 0, 9, 9)], det=[(bad, .5, 0, 0, 9, 9)])])
        with pytest.raises(ValueError, match="outside 1..2"):
            ev.update([dc.image(gt=[(bad, 0, 0, 9, 9)], det=[(1, .5, 0, 0, 9, 9)])])
    assert ev._rows == 0 and int(ev._gt_counts.sum()) == 0                   # nothing was launched
    for n_cls in (1, 1025):
        with pytest.raises(ValueError, match="num_classes"):
            DetectionEvaluator(n_cls, device=DEV)
    # labels that already live on the device cannot be seen from the host: the kernel leaves them out and finalize reports them
    im = {k: torch.as_tensor(v).to(DEV) for k, v in dc.image(gt=[(1, 0, 0, 9, 9)], det=[(3, .5, 0, 0, 9, 9), (1, .4, 0, 0, 9, 9)]).items()}
    ev.update([im])
    with pytest.raises(ValueError, match="1 labels outside"):
        ev.finalize()
    with pytest.raises(ValueError, match="1 labels outside"):                # the error stays set ...
        ev.finalize()
    ev.reset()                                                               # ... until reset()
    assert np.all(ev.finalize()["stats"] == -1.0)


def _boxlists(images):
    gts, preds = [], []
    for im in images:
        gt = BoxList(torch.as_tensor(im["gt_boxes"]).to(DEV), (1000, 1000))
        gt.add_field("labels", torch.as_tensor(im["gt_classes"]).to(DEV))
        pr = BoxList(torch.as_tensor(im["pred_boxes"]).to(DEV), (1000, 1000))
        pr.add_field("pred_labels", torch.as_tensor(im["pred_classes"]).to(DEV))
        pr.add_field("pred_scores", torch.as_tensor(im["obj_scores"]).to(DEV))
        gts.append(gt)
        preds.append(pr)
    return gts, preds


@pytest.mark.parametrize("name", ["gt_only_first_batch", "gt_only_split"])
def test_one_shot_forms_without_a_detection_in_the_first_batch(name):
    case = dc.cases()[name]
    want = dc.expected(name)
    ev = DetectionEvaluator(case["num_classes"], device=DEV, first_gt_id=case["first_gt_id"])
    compare(name + " (first batch alone)", ev.evaluate(case["batches"][0]),
            dc.np_coco_eval(case["batches"][0], case["num_classes"], case["first_gt_id"]))
    compare(name + " (one shot)", ev.evaluate(dc.flat_images(case)), want)
    m_ap, text, _ = do_box_evaluation(*_boxlists(dc.flat_images(case)), "sgdet", case["num_classes"], device=DEV)
    assert abs(m_ap - want["stats"][1]) <= 1e-12
    assert text == "Detection evaluation mAp=%.4f\nrecall@%d IOU:0.5 %.4f\n" % (want["stats"][1], 100, want["recall50_100"])


def test_do_box_evaluation_prints_the_reference_lines():
    case = dc.cases()["empties"]
    want = dc.expected("empties")
    gts, preds, preds_predcls = [], [], []
    for im in dc.flat_images(case):
        gt = BoxList(torch.as_tensor(im["gt_boxes"]).to(DEV), (1000, 1000))
        gt.add_field("labels", torch.as_tensor(im["gt_classes"]).to(DEV))
        pr = BoxList(torch.as_tensor(im["pred_boxes"]).to(DEV), (1000, 1000))
        pr.add_field("pred_labels", torch.as_tensor(im["pred_classes"]).to(DEV))
        pr.add_field("pred_scores", torch.as_tensor(im["obj_scores"]).to(DEV))
        gts.append(gt)
        preds.append(pr)
        pc = BoxList(torch.as_tensor(im["gt_boxes"]).to(DEV), (1000, 1000))    # predcls: the GT boxes with the GT 'labels', scores 1
        pc.add_field("labels", torch.as_tensor(im["gt_classes"]).to(DEV))
        preds_predcls.append(pc)
    m_ap, text, saved = do_box_evaluation(gts, preds, "sgdet", case["num_classes"], device=DEV)
    assert abs(m_ap - want["stats"][1]) <= 1e-12
    assert text == "Detection evaluation mAp=%.4f\nrecall@%d IOU:0.5 %.4f\n" % (want["stats"][1], 100, want["recall50_100"])
    assert list(saved) == ["bbox/AP", "bbox/AP50", "bbox/AP75", "bbox/APs", "bbox/APm", "bbox/APl"]
    assert all(abs(saved["bbox/" + n] - want["stats"][i]) <= 1e-12 for i, n in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl")))
    images = [{"gt_boxes": im["gt_boxes"], "gt_classes": im["gt_classes"], "pred_boxes": im["gt_boxes"], "pred_classes": im["gt_classes"],
               "obj_scores": np.ones(len(im["gt_classes"]), np.float32)} for im in dc.flat_images(case)]
    want_predcls = dc.np_coco_eval(images, case["num_classes"], 0)
    m_ap, text, _ = do_box_evaluation(gts, preds_predcls, "predcls", case["num_classes"], device=DEV)
    assert abs(m_ap - want_predcls["stats"][1]) <= 1e-12 and text.startswith("Detection evaluation mAp=%.4f\n" % want_predcls["stats"][1])
