"""Times one training step (veto_forward_train + losses + veto_backward through autograd) of VETOPredictor on the
BASELINE cfg-2 batch shape (12 images x 36 objects = 15 120 pairs, 4 layers, 8 heads), dropout at the reference's rates.
usage: tools/train_bench.py [steps] [--freeze heads|lastK] [--eval-frozen | --frozen-fused]
--freeze heads: every parameter but the classifier frozen (requires_grad = False); --freeze lastK (last1, last2, ...): the last K
transformer layers and the classifier trainable, everything under them frozen.  The step then runs under a veto_train_plan_t.
--eval-frozen (with --freeze): the frozen sub-modules are also put in eval(), as the reference's fix_eval_modules does: pos_embed on
its running statistics, no dropout under the lowest trainable layer.  --frozen-fused: that, and VETO_AMD.FROZEN_FUSED on, so that
the frozen region runs through the fused inference launches (the decision is printed)."""
import argparse, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from veto_amd import synth, testing
from veto_amd.pairs import prepare_test_pairs

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=5)
ap.add_argument("--freeze", default=None, help="heads, or lastK (K = 1, 2, ...)")
ap.add_argument("--eval-frozen", action="store_true", help="eval() on the frozen sub-modules")
ap.add_argument("--frozen-fused", action="store_true", help="--eval-frozen with VETO_AMD.FROZEN_FUSED on")
args = ap.parse_args()
steps = args.steps
if args.freeze is not None and not re.fullmatch(r"heads|last[1-9]", args.freeze):
    ap.error("--freeze takes heads or lastK")
if (args.eval_frozen or args.frozen_fused) and args.freeze is None:
    ap.error("--eval-frozen / --frozen-fused need --freeze")
dev = torch.device("cuda:0")
cfg = testing.make_config(4, 8)
cfg.VETO_AMD.FROZEN_FUSED = bool(args.frozen_fused)
model = testing.make_predictor(cfg, synth.predictor_state_dict(0, layers=4), dev).train()
batch = synth.synthetic_batch(7, 12, 36)
props = testing.make_proposals(batch, "predcls", dev)
pairs = prepare_test_pairs(dev, props)
n = sum(int(p.shape[0]) for p in pairs)
labels = torch.from_numpy(synth.integers(5, "bench.labels", (n,), 0, 51)).to(dev)
rel_labels = list(labels.split([int(p.shape[0]) for p in pairs]))
kw = dict(roi_features=torch.from_numpy(batch["roi_features"]).to(dev), roi_depth_features=torch.from_numpy(batch["roi_depth_features"]).to(dev))
if args.freeze is not None:
    keep = 0 if args.freeze == "heads" else int(args.freeze[4:])
    tail = tuple(".layers.%d." % l for l in range(4 - keep, 4))
    for name, prm in model.named_parameters():
        prm.requires_grad_(name.startswith("rel_out.") or any(t in name for t in tail))
    if args.eval_frozen or args.frozen_fused:
        tr = model.fusion_transformer.transformer
        for m in [model.pos_embed, tr.pos_drop] + [tr.layers[l] for l in range(4 - keep)]:
            m.eval()
opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4)


def step():
    opt.zero_grad(set_to_none=True)
    loss = model(props, pairs, rel_labels, None, **kw)[2]["rel_loss"]
    loss.backward()
    opt.step()
    return loss


for _ in range(2):
    step()
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
t_f = t_b = 0.0
t0 = time.perf_counter()
for _ in range(steps):
    opt.zero_grad(set_to_none=True)
    ev[0].record()
    loss = model(props, pairs, rel_labels, None, **kw)[2]["rel_loss"]
    ev[1].record()
    loss.backward()
    ev[2].record()
    opt.step()
    torch.cuda.synchronize()
    t_f += ev[0].elapsed_time(ev[1]); t_b += ev[1].elapsed_time(ev[2])
dt = (time.perf_counter() - t0) / steps
print("training step: %.1f ms (forward+loss %.1f ms, backward %.1f ms, rest = optimizer) -> %.0f pairs/s; loss %.4f; peak memory %.1f GB" %
      (dt * 1e3, t_f / steps, t_b / steps, n / dt, float(loss.detach()), torch.cuda.max_memory_allocated() / 2 ** 30))
print("frozen-fused: %s (%s)" % model.last_frozen_fused)
ws = model.__dict__.get("_train_ws")
print("trainable tensors: %d of %d; training workspace: %d bytes" % (sum(p.requires_grad for p in model.parameters()), len(list(model.parameters())),
                                                                 ws.numel() if torch.is_tensor(ws) else 0))
