"""The control of profiles/train_deterministic.txt (section 4): the full-size step (12 x 36 objects, 15 120 pairs, L2 / H8, dropout at the reference's rates)
three times from one state in the default mode and, where the tree has it, in the ordered mode: how many gradient tensors differ in any
bit between runs; workspace bytes; a hash of the (deterministic) forward for a tree-to-tree comparison.
usage: tools/train_repeat_control.py [root of the tree to import veto_amd from; default: this one]"""
import ctypes
import hashlib
import os
import sys

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
from veto_amd import native, synth, testing
from veto_amd.pairs import prepare_test_pairs

dev = torch.device("cuda:0")
has_knob = hasattr(native, "ordered_mode")


def build(knob):
    cfg = testing.make_config(2, 8)
    if has_knob:
        cfg.VETO_AMD.DETERMINISTIC = knob
    return cfg, testing.make_predictor(cfg, synth.predictor_state_dict(0, layers=2), dev).train()


batch = synth.synthetic_batch(7, 12, 36)
props = testing.make_proposals(batch, "predcls", dev)
pairs = prepare_test_pairs(dev, props)
n = sum(int(p.shape[0]) for p in pairs)
labels = torch.from_numpy(synth.integers(5, "bench.labels", (n,), 0, 51)).to(dev)
rel_labels = list(labels.split([int(p.shape[0]) for p in pairs]))


def run(model):
    roi = {k: torch.from_numpy(batch[k]).to(dev).requires_grad_(True) for k in ("roi_features", "roi_depth_features")}
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(3)
    out = model(props, pairs, rel_labels, None, **roi)
    loss = out[2]["rel_loss"]
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().cpu().numpy().tobytes(), "logits": out[1][0].detach().cpu().numpy().tobytes() if isinstance(out[1], (list, tuple)) and len(out[1]) and torch.is_tensor(out[1][0]) else b""}
    res.update({"grad." + k: p.grad.cpu().numpy().tobytes() for k, p in model.named_parameters() if p.grad is not None})
    res.update({"d_" + k: v.grad.cpu().numpy().tobytes() for k, v in roi.items()})
    return res


for knob in ([False, True] if has_knob else [False]):
    cfg, model = build(knob)
    runs = [run(model) for _ in range(3)]
    grads = [k for k in runs[0] if k.startswith(("grad.", "d_"))]
    differ = [k for k in grads if runs[1][k] != runs[0][k] or runs[2][k] != runs[0][k]]
    print("%s mode=%s: full-size step x 3: %d of %d gradient tensors differ in some bit between runs; loss bits equal %s; loss %s fwd-hash %s"
          % (os.path.basename(root) or root, "ordered" if knob else "default", len(differ), len(grads),
             runs[0]["loss"] == runs[1]["loss"] == runs[2]["loss"], np.frombuffer(runs[0]["loss"], dtype=np.float32)[0],
             hashlib.sha1(runs[0]["loss"] + runs[0]["logits"]).hexdigest()[:16]))
    if differ:
        print("  differing: " + " ".join(sorted(differ)[:12]) + (" ..." if len(differ) > 12 else ""))
    eng = model._ensure_engine(dev)
    lib = native.load_library()
    line = "workspace bytes at 432 objects / %d pairs (L2): veto_train_workspace_bytes %d" % (n, lib.veto_train_workspace_bytes(eng.handle, 432, n))
    if has_knob:
        on = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts), deterministic=1)
        line += "; veto_train_workspace_bytes_opts(deterministic=1) %d" % lib.veto_train_workspace_bytes_opts(eng.handle, 432, n, ctypes.byref(on))
    print(line)
    del model
    torch.cuda.empty_cache()
