"""The control of profiles/train_deterministic.txt (section 4): the full-size step (12 x 36 objects, 15 120 pairs, L2 / H8, dropout at the reference's rates)
three times from one state in the default mode and, where the tree has it, in the ordered mode: how many gradient tensors differ in any
bit between runs; workspace bytes; a hash of the (deterministic) forward for a tree-to-tree comparison.

With --shape IMAGESxOBJECTS --layers L: the tree-to-tree control of a change that must not move a bit (profiles/train_host_stages.txt).
Per mode, one step each without dropout, with dropout at the reference's rates and (dropout on) under the "heads", "last_heads" and
"last_all_heads" plans of tests/partial_train_cases.py, every one printed as ONE sha256 over all parameter gradients and d_roi_*, the
loss bits and a hash of the forward; then the training workspace sizes at this shape and at 432 objects / 15 120 pairs.  The ordered
mode's lines of two trees are equal when the trees compute the same; the default mode's gradient hash moves from run to run (float atomics).
usage: tools/train_repeat_control.py [root of the tree to import veto_amd from; default: this one] [--shape 2x6 --layers 4]"""
import argparse
import ctypes
import hashlib
import os
import random
import sys

ap = argparse.ArgumentParser()
ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--shape", help="IMAGESxOBJECTS per image, e.g. 1x2")
ap.add_argument("--layers", type=int, default=2)
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
import numpy as np
import torch
from veto_amd import native, synth, testing
from veto_amd.pairs import prepare_test_pairs

dev = torch.device("cuda:0")
has_knob = hasattr(native, "ordered_mode")
n_img, n_obj_img = [int(v) for v in args.shape.split("x")] if args.shape else (12, 36)
layers = args.layers if args.shape else 2
tree = os.path.basename(root) or root


def build(knob):
    cfg = testing.make_config(layers, 8)
    if has_knob:
        cfg.VETO_AMD.DETERMINISTIC = knob
    return cfg, testing.make_predictor(cfg, synth.predictor_state_dict(0, layers=layers), dev).train()


batch = synth.synthetic_batch(7, n_img, n_obj_img)
props = testing.make_proposals(batch, "predcls", dev)
pairs = prepare_test_pairs(dev, props)
n = sum(int(p.shape[0]) for p in pairs)
labels = torch.from_numpy(synth.integers(5, "bench.labels", (n,), 0, 51)).to(dev)
rel_labels = list(labels.split([int(p.shape[0]) for p in pairs]))


def run(model, maps=True):
    roi = {k: torch.from_numpy(batch[k]).to(dev).requires_grad_(maps) for k in ("roi_features", "roi_depth_features")}
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(3)
    random.seed(1)
    out = model(props, pairs, rel_labels, None, **roi)
    loss = out[2]["rel_loss"]
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().cpu().numpy().tobytes(), "logits": out[1][0].detach().cpu().numpy().tobytes() if isinstance(out[1], (list, tuple)) and len(out[1]) and torch.is_tensor(out[1][0]) else b""}
    res.update({"grad." + k: p.grad.cpu().numpy().tobytes() for k, p in model.named_parameters() if p.grad is not None})
    res.update({"d_" + k: v.grad.cpu().numpy().tobytes() for k, v in roi.items() if v.grad is not None})
    return res


def workspace_line(model, n_obj, n_pair, plans):
    eng, lib = model._ensure_engine(dev), native.load_library()
    line = "workspace bytes at %d objects / %d pairs (L%d): veto_train_workspace_bytes %d" % (n_obj, n_pair, layers, lib.veto_train_workspace_bytes(eng.handle, n_obj, n_pair))
    if has_knob:
        on = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts), deterministic=1)
        line += "; veto_train_workspace_bytes_opts(deterministic=1) %d" % lib.veto_train_workspace_bytes_opts(eng.handle, n_obj, n_pair, ctypes.byref(on))
        names = [name for name, _ in eng.weight_specs()]
        for tag, plan in plans:
            flags = (ctypes.c_uint8 * len(names))(*[1 if name in plan.trainable else 0 for name in names])
            p = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan), bn_eval=0, d_roi=int(plan.maps), trainable=ctypes.cast(flags, ctypes.c_void_p), p_attn_layer=None)
            line += "; _plan(%s, deterministic=1) %d" % (tag, lib.veto_train_workspace_bytes_plan(eng.handle, n_obj, n_pair, ctypes.byref(on), ctypes.byref(p)))
    return line


def shape_control():
    sys.path.insert(0, os.path.join(root, "tests"))
    import partial_train_cases as pc
    plans = [(tag, pc.plans(layers)[tag]) for tag in ("heads", "last_heads", "last_all_heads")]
    for knob in (False, True):
        cfg, model = build(knob)
        dropouts = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
        cases = [("no-dropout", None, False), ("dropout", None, True)] + [("plan:" + tag, plan, True) for tag, plan in plans]
        for tag, plan, drop in cases:
            model.train()
            for m in dropouts:
                m.train(drop)
            for name, p in model.named_parameters():
                p.requires_grad_(plan is None or name in plan.trainable)
            r = run(model, maps=plan is None or plan.maps)
            grads = sorted(k for k in r if k.startswith(("grad.", "d_")))
            print("%s mode=%s %dx%d L%d %-19s: %3d gradients sha256 %s loss bits %s fwd-hash %s" % (
                tree, "ordered" if knob else "default", n_img, n_obj_img, layers, tag, len(grads),
                hashlib.sha256(b"".join(k.encode() + r[k] for k in grads)).hexdigest()[:32], r["loss"].hex(), hashlib.sha1(r["loss"] + r["logits"]).hexdigest()[:16]))
        if knob:
            print(workspace_line(model, n_img * n_obj_img, n, plans))
            print(workspace_line(model, 432, 15120, plans))
        del model
        torch.cuda.empty_cache()


def full_size_control():
    for knob in ([False, True] if has_knob else [False]):
        cfg, model = build(knob)
        runs = [run(model) for _ in range(3)]
        grads = [k for k in runs[0] if k.startswith(("grad.", "d_"))]
        differ = [k for k in grads if runs[1][k] != runs[0][k] or runs[2][k] != runs[0][k]]
        print("%s mode=%s: full-size step x 3: %d of %d gradient tensors differ in some bit between runs; loss bits equal %s; loss %s fwd-hash %s"
              % (tree, "ordered" if knob else "default", len(differ), len(grads),
                 runs[0]["loss"] == runs[1]["loss"] == runs[2]["loss"], np.frombuffer(runs[0]["loss"], dtype=np.float32)[0],
                 hashlib.sha1(runs[0]["loss"] + runs[0]["logits"]).hexdigest()[:16]))
        if differ:
            print("  differing: " + " ".join(sorted(differ)[:12]) + (" ..." if len(differ) > 12 else ""))
        print(workspace_line(model, 432, n, []))
        del model
        torch.cuda.empty_cache()


shape_control() if args.shape else full_size_control()
