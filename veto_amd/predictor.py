"""MI355X-native `VETOPredictor` / `VETOPredictor_MEET` behind the reference's plugin API.

Mirrors pysgg/modeling/roi_heads/relation_head/roi_relation_predictors.py:3876-4139:
  * registered under the same names in a registry of the same protocol (veto_amd.registry),
  * same constructor `Predictor(config, in_channels)` and the same `forward` signature,
  * same 6-tuple return (SURVEY.md section 8b "Return"),
  * same state-dict key names, so reference checkpoints load unchanged.

The modules below are PARAMETER CONTAINERS: the arithmetic of the eval forward runs in
libveto_amd.so (hand-written HIP, include/veto_amd.h) on the tensors' own device and stream.
There is no PyTorch or CPU fallback; if the library is missing, or the inputs are not on a HIP
device, forward raises.
"""
import ctypes
import os
import weakref
import warnings

import torch
from torch import nn

from . import meet_tables, native
from .registry import ROI_RELATION_PREDICTOR

_STATISTICS_PROVIDER = None
_EMBEDDING_PROVIDER = None


def set_statistics_provider(fn):
    """fn(config) -> {'obj_classes': [...], 'rel_classes': [...]} (replaces the reference's
    pysgg.data.get_dataset_statistics, data/build.py:27-77, when pysgg is not importable)."""
    global _STATISTICS_PROVIDER
    _STATISTICS_PROVIDER = fn


def set_embedding_provider(fn):
    """fn(obj_classes, wv_dir, wv_dim) -> FloatTensor [len(obj_classes), wv_dim] (replaces
    utils_motifs.obj_edge_vectors, utils_motifs.py:151-171)."""
    global _EMBEDDING_PROVIDER
    _EMBEDDING_PROVIDER = fn


def _dataset_statistics(config):
    if _STATISTICS_PROVIDER is not None:
        return _STATISTICS_PROVIDER(config)
    try:
        from pysgg.data import get_dataset_statistics  # type: ignore
        return get_dataset_statistics(config)
    except ImportError:
        n_obj, n_rel = meet_tables.NUM_CLASSES[config.GLOBAL_SETTING.DATASET_CHOICE]
        return {"obj_classes": ["obj_%d" % i for i in range(n_obj)],
                "rel_classes": ["rel_%d" % i for i in range(n_rel)]}


def _embedding_vectors(obj_classes, wv_dir, wv_dim):
    if _EMBEDDING_PROVIDER is not None:
        return _EMBEDDING_PROVIDER(obj_classes, wv_dir, wv_dim)
    try:
        from pysgg.modeling.roi_heads.relation_head.utils_motifs import obj_edge_vectors  # type: ignore
        return obj_edge_vectors(obj_classes, wv_dir=wv_dir, wv_dim=wv_dim)
    except ImportError:
        warnings.warn("veto_amd: GloVe loader unavailable; obj_embed initialised N(0,1) "
                      "(load a checkpoint or call set_embedding_provider)")
        return torch.randn(len(obj_classes), wv_dim)


def _mode(config):
    rh = config.MODEL.ROI_RELATION_HEAD
    if rh.USE_GT_BOX:
        return "predcls" if rh.USE_GT_OBJECT_LABEL else "sgcls"
    return "sgdet"


def _precision(config):
    ext = getattr(config, "VETO_AMD", None)
    name = getattr(ext, "PRECISION", "mixed") if ext is not None else "mixed"
    modes = {"precise": native.VETO_PRECISE, "fast": native.VETO_FAST, "mixed": native.VETO_MIXED}
    if name not in modes:
        raise ValueError("VETO_AMD.PRECISION must be one of %s, got %r" % (sorted(modes), name))
    return modes[name]


def _max_chunk(config):
    ext = getattr(config, "VETO_AMD", None)
    return int(getattr(ext, "MAX_CHUNK_PAIRS", 0)) if ext is not None else 0


# ---------------------------------------------------------------------------------------------------
# Parameter containers with the reference's attribute names (=> identical state-dict keys).
# ---------------------------------------------------------------------------------------------------

class _Holder(nn.Module):
    """A module that only owns sub-modules/parameters; the compute lives in the HIP library."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the forward pass runs in libveto_amd.so")


def _attention_params(dim, dropout):
    m = _Holder()
    m.to_qkv = nn.Linear(dim, 3 * dim, bias=False)
    m.to_out = nn.Sequential(nn.Linear(dim, dim), nn.Dropout(dropout))
    return m


def _feedforward_params(dim, hidden):
    m = _Holder()
    m.net = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(0.0), nn.Linear(hidden, dim),
                          nn.Dropout(0.0))
    return m


def _prenorm(dim, fn):
    m = _Holder()
    m.norm = nn.LayerNorm(dim)
    m.fn = fn
    return m


# (POOLER_RESOLUTION, PATCH_SIZE) the library runs: a 4 x 4 grid of patches, so that a pair is 19 tokens (include/veto_amd.h)
SUPPORTED_PATCH_GRIDS = ((4, 1), (8, 2), (12, 3), (16, 4))


def patch_grid(config):
    """(POOLER_RESOLUTION, PATCH_SIZE) of the config; ValueError naming the supported pairs for any other."""
    rh = config.MODEL.ROI_RELATION_HEAD
    pair = (rh.POOLER_RESOLUTION, rh.VETOTRANSFORMER.PATCH_SIZE)
    if pair not in SUPPORTED_PATCH_GRIDS:
        raise ValueError("veto_amd: ROI_RELATION_HEAD.POOLER_RESOLUTION %r with VETOTRANSFORMER.PATCH_SIZE %r is not supported: the fused "
                         "launches hold 19 tokens per pair (a 4 x 4 patch grid), so (POOLER_RESOLUTION, PATCH_SIZE) must be one of %s"
                         % (pair[0], pair[1], ", ".join("(%d, %d)" % q for q in SUPPORTED_PATCH_GRIDS)))
    return int(pair[0]), int(pair[1])


def _transformer_params(config, in_channels):
    vt = config.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER
    dim, patch = vt.T_INPUT_DIM, vt.PATCH_SIZE
    if dim != 576:
        # same constraint as the reference: proj_d (512) + proj_v (64) are hard-wired, so any other
        # T_INPUT_DIM fails at the token concat (model_veto.py:105-113)
        raise ValueError("VETOTRANSFORMER.T_INPUT_DIM must be 576, got %d" % dim)
    inner = _Holder()
    inner.patch_embed = _Holder()
    pdim = in_channels * 2 * patch * patch
    inner.patch_embed.proj_d = nn.Linear(pdim, 512)
    inner.patch_embed.proj_v = nn.Linear(pdim, 64)
    inner.cls_token = nn.Parameter(torch.randn(1, 1, dim))
    inner.pos_embedding = nn.Parameter(torch.randn(1, 1, dim))
    inner.pos_drop = nn.Dropout(vt.EMB_DROPOUT)
    inner.layers = nn.ModuleList(
        nn.ModuleList([_prenorm(dim, _attention_params(dim, vt.T_DROPOUT)),
                       _prenorm(dim, _feedforward_params(dim, 2 * dim))])
        for _ in range(vt.ENC_LAYERS))
    outer = _Holder()
    outer.transformer = inner
    outer.to_cls_token = nn.Identity()
    return outer


def _xavier_linear(in_f, out_f):
    lin = nn.Linear(in_f, out_f, bias=True)
    nn.init.xavier_normal_(lin.weight)
    return lin


def _build_trunk(m, config, num_obj_cls, with_embed2):
    """Adds the modules shared by VETOPredictor (:4014-4053) and Ensemble (:3668-3704) to `m`."""
    dim = config.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.T_INPUT_DIM
    embed_dim = 200
    if with_embed2:
        m.obj_embed2 = nn.Embedding(num_obj_cls, embed_dim)
    m.obj_embed = nn.Embedding(num_obj_cls, embed_dim)
    m.class_projection = nn.Sequential(nn.Linear(2 * embed_dim, dim), nn.ReLU(inplace=True))
    m.bbox_embed = nn.Sequential(nn.Linear(9, 32), nn.ReLU(inplace=True), nn.Dropout(0.1),
                                 nn.Linear(32, 128), nn.ReLU(inplace=True), nn.Dropout(0.1))
    m.pos_embed = nn.Sequential(nn.BatchNorm1d(4, momentum=0.001), nn.Linear(4, 128), nn.ReLU(inplace=True),
                                nn.Dropout(0.1))
    m.location_projection = nn.Sequential(nn.Linear(256, dim), nn.ReLU(inplace=True))
    m.fusion_transformer = _transformer_params(config, in_channels=256)


_TRUNK_KEYS = None


def cached_offsets(n_objs, n_pairs, device):
    """Per-image exclusive prefix sums (objects, pairs) as int32 device tensors: two rows of native.device_offsets."""
    off = native.device_offsets(n_objs, n_pairs, device=device)
    return off[0], off[1]


class _NativeForward:
    """Shared device-side plumbing: engine lifetime, weight upload, workspace, one C-ABI forward."""

    def _native_init(self, config, trunk, num_obj_cls, head_modules):
        vt = config.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER
        self._layers, self._heads = int(vt.ENC_LAYERS), int(vt.NHEADS)
        self._resolution, self._patch = patch_grid(config)
        self._num_obj_cls = num_obj_cls
        self._head_modules = head_modules
        self._num_out = sum(h.out_features for h in head_modules)
        self._precision = _precision(config)
        self._max_chunk = _max_chunk(config)
        # VETO_AMD.COUNT_SATURATION: eval forwards go through veto_forward_saturation (slower: launch per stage, one stream
        # synchronisation) and leave the per-layer counts of clamped mixed-row elements in `self.last_saturation`
        self._count_saturation = bool(getattr(getattr(config, "VETO_AMD", None), "COUNT_SATURATION", False))
        self._deterministic = bool(getattr(getattr(config, "VETO_AMD", None), "DETERMINISTIC", False))
        self.last_saturation = None
        # VETO_AMD.FROZEN_FUSED: eligible training steps run their frozen region through the fused inference launches
        # (frozen_fused_eligibility); what the last training step decided, and why: (bool, reason)
        self._frozen_fused = bool(getattr(getattr(config, "VETO_AMD", None), "FROZEN_FUSED", False))
        self.last_frozen_fused = (False, "no training step has run")
        object.__setattr__(self, "_trunk", trunk)  # not a sub-module registration
        self._engine = None
        self._engine_device = None
        self._uploaded = None
        self._tensor_versions = {}      # per engine weight: the (data_ptr, _version) of its module tensors at their last upload
        self._forced = set()            # refresh_weights(names): uploaded next time whatever their version
        self._workspace = None
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.refresh_weights())

    def _weight_tensors(self):
        t = self._trunk
        sd = {k: v for k, v in t.state_dict().items()}
        out = {k: sd[k] for k in sd if k.startswith(("obj_embed.", "class_projection.0.", "pos_embed.",
                                                     "location_projection.0.", "fusion_transformer."))}
        out.pop("pos_embed.0.num_batches_tracked", None)
        heads = self._head_modules
        out["rel_out.weight"] = torch.cat([h.weight for h in heads], 0) if len(heads) > 1 else heads[0].weight
        out["rel_out.bias"] = torch.cat([h.bias for h in heads], 0) if len(heads) > 1 else heads[0].bias
        return out

    def _weights_version(self):
        return tuple((p.data_ptr(), p._version) for p in list(self._trunk.parameters()) + list(self._trunk.buffers()))

    def refresh_weights(self, names=None):
        """Forces the next call to re-upload every weight (and rebuild the engine's derived operands: split / mixed rows,
        Wqkv diag(gamma), Mcat, Ncat).  Weight changes are detected through (data_ptr, Tensor._version), which writes
        through `.data` (`p.data.copy_()`, EMA updates, hand-written optimisers, some checkpoint loaders) do NOT bump:
        call this after such a write in eval mode.  In training mode and after load_state_dict it happens by itself.

        names: an optional list of state-dict names (the engine's: veto_weight_info; the heads are "rel_out.weight" /
        "rel_out.bias") -- only these are known to have changed.  A frozen-fused training step (VETO_AMD.FROZEN_FUSED), which
        uploads a tensor only when its (data_ptr, _version) changed since its last upload, then uploads just these besides,
        and the engine rebuilds just the operands that read them; every other path re-uploads everything, as without names.
        The caveat above holds there too: a frozen tensor written through `.data` between two frozen-fused steps is NOT seen;
        name it here."""
        self._uploaded = None
        if names is None:
            self._tensor_versions = {}
        else:
            self._forced.update(names)

    invalidate = refresh_weights

    def _module_tensors(self):
        """{engine weight name: the module tensors it is made of, in row order} (rel_out.*: one per head)."""
        keep = ("obj_embed.", "class_projection.0.", "pos_embed.", "location_projection.0.", "fusion_transformer.")
        t = self._trunk
        out = {k: (v,) for k, v in list(t.named_parameters()) + list(t.named_buffers())
               if k.startswith(keep) and k != "pos_embed.0.num_batches_tracked"}
        out["rel_out.weight"] = tuple(h.weight for h in self._head_modules)
        out["rel_out.bias"] = tuple(h.bias for h in self._head_modules)
        return out

    def _upload_changed(self, device):
        """The frozen-fused step's upload: the tensors whose (data_ptr, _version) changed since their last upload (the trainable
        ones after an optimizer step; frozen ones normally never) and the ones refresh_weights(names) named."""
        eng = self._engine
        src = self._module_tensors()
        stamp = {n: tuple((t.data_ptr(), t._version) for t in ts) for n, ts in src.items()}
        stream = torch.cuda.current_stream(device)
        keep = []
        for name, numel in eng.weight_specs():
            if self._tensor_versions.get(name) == stamp[name] and name not in self._forced:
                continue
            ts = src[name]
            t = (ts[0] if len(ts) == 1 else torch.cat(ts, 0)).detach().to(device=device, dtype=torch.float32).contiguous()
            if t.numel() != numel:
                raise RuntimeError("veto_amd: weight %s has %d elements, expected %d" % (name, t.numel(), numel))
            keep.append(t)
            eng.load_weight(name, t.data_ptr(), numel, stream.cuda_stream)
        if keep:
            stream.synchronize()  # `keep` may be freed after this
        self._tensor_versions = stamp
        self._forced = set()
        self._uploaded = self._weights_version()      # (everything the engine holds is current: an eval forward may trust it)

    def _ensure_engine(self, device, per_tensor=False):
        if device.type != "cuda":
            raise RuntimeError("veto_amd: the predictor runs only on a HIP device (got %s); there is no CPU path" % device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._engine is None or self._engine_device != idx:
            if self._engine is not None:
                self._engine.close()
            self._engine = native.Engine(self._layers, self._heads, self._num_obj_cls, self._num_out,
                                         precision=self._precision, device=idx, max_chunk_pairs=self._max_chunk,
                                         patch=self._patch, resolution=self._resolution)
            self._engine_device = idx
            self._uploaded = None
            self._tensor_versions = {}
        if per_tensor:
            self._upload_changed(device)
            return self._engine
        ver = self._weights_version()
        if self._trunk.training:
            self._uploaded = None      # a training step changes the weights: never trust the version stamp there
        if self._uploaded != ver:
            tensors = self._weight_tensors()
            stream = torch.cuda.current_stream(device).cuda_stream
            keep = []
            for name, numel in self._engine.weight_specs():
                t = tensors[name].detach().to(device=device, dtype=torch.float32).contiguous()
                if t.numel() != numel:
                    raise RuntimeError("veto_amd: weight %s has %d elements, expected %d" % (name, t.numel(), numel))
                keep.append(t)
                self._engine.load_weight(name, t.data_ptr(), numel, stream)
            torch.cuda.current_stream(device).synchronize()  # `keep` may be freed after this
            self._uploaded = ver
            self._tensor_versions, self._forced = {}, set()      # (no per-tensor stamps were taken: a frozen-fused step uploads all once)
        return self._engine

    @staticmethod
    def _rate(drop):
        """The rate a dropout site runs at: its module's p, or 0 while the module is in eval() (as nn.Dropout behaves)."""
        return float(drop.p) if drop.training else 0.0

    def _attn_rates(self):
        return [self._rate(layer[0].fn.to_out[1]) for layer in self._trunk.fusion_transformer.transformer.layers]

    def _train_opts(self):
        """Dropout probabilities of the three sites the training path implements, read from the mirror modules (so that
        `module.p = 0` and `module.eval()` behave as in torch), plus a fresh seed drawn from torch's generator.  Attention
        rates that differ between the layers travel in the plan (_train_plan); p_attn is then not read."""
        t = self._trunk
        tr = t.fusion_transformer.transformer
        o = native.VetoTrainOpts(struct_size=ctypes.sizeof(native.VetoTrainOpts))
        o.p_pos = self._rate(t.pos_embed[3])
        o.p_emb = self._rate(tr.pos_drop)
        ps = set(self._attn_rates())
        o.p_attn = ps.pop() if len(ps) == 1 else 0.0
        others = [n for n, m in t.named_modules() if isinstance(m, nn.Dropout) and m.p > 0 and
                  not (n == "pos_embed.3" or n.endswith("pos_drop") or n.endswith("fn.to_out.1"))]
        others = [n for n in others if not n.startswith("bbox_embed")]        # bbox_embed is not on the VETO path
        if others:
            raise NotImplementedError("veto_amd: dropout is built for pos_embed, pos_drop and the attention output only; "
                                      "these modules also have p > 0: %s" % ", ".join(others[:6]))
        o.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        o.deterministic = int(native.ordered_mode(self._deterministic))
        return o

    def _run_native_train(self, proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits):
        """Forward in training mode: BatchNorm1d(4) of pos_embed on batch statistics (and its running statistics
        updated the way nn.BatchNorm1d(momentum=0.001) does, roi_relation_predictors.py:4042-4047)."""
        device = roi_features.device
        stats = torch.empty(12, dtype=torch.float32, device=device)
        if any(isinstance(m, nn.Dropout) and m.p > 0 for n, m in self._trunk.named_modules() if not n.startswith("bbox_embed")):
            raise NotImplementedError("veto_amd: the forward-only training pass (VETO_AMD.TRAIN_FORWARD_ONLY) runs without dropout")
        out = self._run_native(proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits, bn_batch_stats=stats)
        bn = self._trunk.pos_embed[0]
        with torch.no_grad():
            m = bn.momentum
            bn.running_mean.mul_(1 - m).add_(stats[0:4].to(bn.running_mean.device), alpha=m)
            bn.running_var.mul_(1 - m).add_(stats[8:12].to(bn.running_var.device), alpha=m)
            bn.num_batches_tracked += 1
        return out

    def _prepare_inputs(self, proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits, bn_batch_stats=None,
                        per_tensor=False):
        """Validates the call and flattens it into a veto_inputs_t.  Returns (call, inp, n_objs, n_pairs, eng); `call` keeps the
        tensors the struct points into.  per_tensor: a frozen-fused step's upload (_upload_changed)."""
        device = roi_features.device
        want = (256, self._resolution, self._resolution)
        if tuple(roi_features.shape[1:]) != want or tuple(roi_depth_features.shape[1:]) != want:
            raise ValueError("roi features must be [N, %d, %d, %d] (POOLER_RESOLUTION %d), got %s / %s"
                             % (want + (self._resolution, tuple(roi_features.shape), tuple(roi_depth_features.shape))))
        eng = self._ensure_engine(device, per_tensor)
        call = native.Launch(device, "veto_amd: the predictor runs only on a HIP device")
        n_objs = [len(p) for p in proposals]
        n_pairs = [int(p.shape[0]) for p in rel_pair_idxs]
        if roi_features.shape[0] != sum(n_objs) or roi_depth_features.shape[0] != sum(n_objs):
            raise ValueError("roi feature rows (%d) != total proposals (%d)" % (roi_features.shape[0], sum(n_objs)))
        f32 = dict(device=device, dtype=torch.float32)
        rgb = roi_features.detach().to(**f32).contiguous()
        dep = roi_depth_features.detach().to(**f32).contiguous()
        boxes = torch.cat([p.bbox for p in proposals], 0).to(**f32).contiguous()
        pairs = torch.cat([p.reshape(-1, 2) for p in rel_pair_idxs], 0).to(device=device, dtype=torch.int64).contiguous()
        off = native.device_offsets(n_objs, n_pairs, device=device)
        lab = labels.to(device=device, dtype=torch.int64).contiguous() if labels is not None else None
        lg = logits.detach().to(**f32).contiguous() if logits is not None else None
        inp = call.args(native.VetoInputs, n_obj=sum(n_objs), n_pair=sum(n_pairs), n_img=len(proposals), roi_rgb=rgb, roi_depth=dep,
                        boxes=boxes, box_mode=0 if proposals[0].mode == "xyxy" else 1, obj_labels=lab, obj_logits=lg, rel_pairs=pairs,
                        img_obj_offset=off[0], img_pair_offset=off[1], bn_batch_stats=bn_batch_stats)
        return call, inp, n_objs, n_pairs, eng

    def _run_native(self, proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits,
                    debug=False, bn_batch_stats=None):
        call, inp, n_objs, n_pairs, eng = self._prepare_inputs(proposals, rel_pair_idxs, roi_features, roi_depth_features,
                                                               labels, logits, bn_batch_stats)
        device, n_pair = call.device, inp.n_pair
        f32 = dict(device=device, dtype=torch.float32)
        # the workspace follows the module's lifetime (it is large), not the shared per-stream cache
        need = eng.workspace_bytes(inp.n_obj, n_pair)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
            self._workspace = None
            self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
        out = torch.empty((n_pair, self._num_out), **f32)
        dbg, extras = None, None
        if debug:
            extras = {"subj_inds": torch.empty(n_pair, dtype=torch.int64, device=device),
                      "obj_inds": torch.empty(n_pair, dtype=torch.int64, device=device),
                      "tokens": torch.empty((n_pair, 19, 576), **f32),
                      "cls": torch.empty((n_pair, 576), **f32)}
            dbg = call.args(native.VetoDebugOutputs, **extras)
        stream = call.stream.cuda_stream
        # (the audit is of the VETO_MIXED operands: the ABI refuses it on a handle that computes in another mode)
        if self._count_saturation and self._precision == native.VETO_MIXED and bn_batch_stats is None and not debug:
            self.last_saturation = eng.forward_saturation(stream, inp, self._workspace.data_ptr(), self._workspace.numel(), out.data_ptr())
        else:
            eng.forward(stream, inp, self._workspace.data_ptr(), self._workspace.numel(), out.data_ptr(), dbg)
        call.record()
        self.last_debug = extras
        return out, n_objs, n_pairs

    # ---- training path with gradients (veto_forward_train / veto_backward) ---------------------------------------
    def _train_param_spec(self):
        """[(Parameter, engine weight name, first row, row count or None)] for every tensor the backward fills."""
        trunk = dict(self._trunk.named_parameters())
        spec = []
        for name, prm in trunk.items():
            if name.startswith(("obj_embed.", "class_projection.0.", "pos_embed.", "location_projection.0.", "fusion_transformer.")):
                spec.append((prm, name, 0, None))
        row = 0
        for head in self._head_modules:
            spec.append((head.weight, "rel_out.weight", row, head.out_features))
            spec.append((head.bias, "rel_out.bias", row, head.out_features))
            row += head.out_features
        return spec

    def frozen_fused_eligibility(self, want_maps=False):
        """Does a training step of the module as it stands run its frozen region through the fused inference launches
        (veto_train_plan_t.frozen_fused)?  A pure function of the module's state (no device, no engine; besides it only the
        VETO_X_F24 knob of the environment is read): (eligible, reason, k),
        k the lowest transformer layer with a trainable parameter (the layer count when only the heads are trainable).  The
        frozen region is everything under layer k; it must compute what the inference forward computes: pos_embed[0] on its
        running statistics, its dropout sites at rate 0, no gradient asked of anything inside it.  want_maps: a ROI map
        requires grad."""
        layers = self._layers
        if not self._frozen_fused:
            return False, "VETO_AMD.FROZEN_FUSED is off", layers
        if self._precision == native.VETO_FAST:
            return False, "VETO_AMD.PRECISION is fast (logit error above the 1e-3 bar)", layers
        if os.environ.get("VETO_X_F24") == "1":      # (the library refuses the flag under this A/B knob: the hand-off takes fp32 rows)
            return False, "VETO_X_F24=1 is set", layers
        if want_maps:
            return False, "a ROI map requires grad", layers
        k, prefix = layers, "fusion_transformer.transformer.layers."
        for prm, name, _, _ in self._train_param_spec():
            if not prm.requires_grad or name.startswith("rel_out."):
                continue
            if not name.startswith(prefix):
                return False, "the prelude parameter %s requires grad" % name, layers
            k = min(k, int(name[len(prefix):].split(".", 1)[0]))
        if k == 0:
            return False, "layer 0 has a trainable parameter (k = 0)", 0
        t = self._trunk
        if t.pos_embed[0].training:
            return False, "pos_embed[0] is in training mode (batch statistics)", k
        for what, drop in (("pos_embed[3]", t.pos_embed[3]), ("pos_drop", t.fusion_transformer.transformer.pos_drop)):
            if self._rate(drop) > 0:
                return False, "the Dropout %s of the frozen region runs at p = %g" % (what, self._rate(drop)), k
        for l, p in enumerate(self._attn_rates()[:k]):
            if p > 0:
                return False, "the attention Dropout of frozen layer %d runs at p = %g" % (l, p), k
        return True, "frozen region: the prelude and layers 0..%d" % (k - 1), k

    def _train_plan(self, eng, spec, want_maps):
        """The veto_train_plan_t of this step, or None when every parameter is trainable, pos_embed[0] is in training mode and
        the layers share one attention dropout rate: the step then runs through the entry points without a plan, as it always
        did.  An eligible step (frozen_fused_eligibility) sets the plan's frozen_fused; the decision and its reason stay in
        self.last_frozen_fused.  Returns (plan, the ctypes arrays it points into)."""
        fused, reason, _ = self.frozen_fused_eligibility(want_maps)
        self.last_frozen_fused = (fused, reason)
        flags = {}
        for prm, name, _, _ in spec:      # (the heads of a MEET list share rel_out.*: one trainable head sets the flag)
            flags[name] = flags.get(name, False) or bool(prm.requires_grad)
        rates = self._attn_rates()
        bn_eval = not self._trunk.pos_embed[0].training
        if all(flags.values()) and not bn_eval and len(set(rates)) == 1:
            return None, None
        names = [n for n, _ in eng.weight_specs()]
        trainable = (ctypes.c_uint8 * len(names))(*[1 if flags.get(n, False) else 0 for n in names])
        p_layer = (ctypes.c_float * len(rates))(*rates)
        plan = native.VetoTrainPlan(struct_size=ctypes.sizeof(native.VetoTrainPlan), bn_eval=int(bn_eval),
                                    trainable=ctypes.cast(trainable, ctypes.c_void_p), p_attn_layer=ctypes.cast(p_layer, ctypes.c_void_p),
                                    d_roi=int(bool(want_maps)), frozen_fused=int(fused))
        return plan, (trainable, p_layer)

    def _run_native_train_grad(self, proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits=None):
        """Training-mode forward whose result carries an autograd graph: logits [sum P, num_out]."""
        spec = self._train_param_spec()
        # roi_features / roi_depth_features are differentiable inputs: veto_backward returns their gradients (the reference trains
        # its depth backbone through roi_depth_features, tools/relation_train_net.py:166-170)
        return _TrainFn.apply(self, (proposals, rel_pair_idxs, labels, logits), roi_features, roi_depth_features, *[s[0] for s in spec])


class _WsToken:
    """Ownership of the cached training workspace by one (forward, backward) pair; see _TrainFn.forward."""
    __slots__ = ("done", "__weakref__")

    def __init__(self):
        self.done = False


class _TrainFn(torch.autograd.Function):
    """logits = VETO trunk + heads in training mode; backward fills the gradients of every trainable parameter through
    veto_backward (veto_backward_plan when a parameter is frozen or a sub-module is in eval mode: _NativeForward._train_plan)
    and returns None for the frozen ones.  The parameters are inputs only so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, owner, call, roi_features, roi_depth_features, *params):
        proposals, rel_pair_idxs, labels, obj_logits = call
        device = roi_features.device
        bn = owner._trunk.pos_embed[0]
        # (an eval-mode BatchNorm normalises with its running statistics and leaves them alone: no batch statistics then)
        stats = torch.empty(12, dtype=torch.float32, device=device) if bn.training else None
        want_maps = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        # (a frozen-fused step uploads only the tensors that changed: decided from the module's state, before the engine is touched)
        launch, inp, n_objs, n_pairs, eng = owner._prepare_inputs(proposals, rel_pair_idxs, roi_features, roi_depth_features,
                                                                labels, obj_logits, stats,
                                                                per_tensor=owner.frozen_fused_eligibility(want_maps)[0])
        opts = owner._train_opts()
        ctx.spec = owner._train_param_spec()
        plan, ctx.plan_arrays = owner._train_plan(eng, ctx.spec, want_maps)
        ctx.plan = plan
        plan_ref = ctypes.byref(plan) if plan is not None else None
        if plan is None:
            need = launch.lib.veto_train_workspace_bytes_opts(eng.handle, inp.n_obj, inp.n_pair, ctypes.byref(opts))
        else:
            need = launch.lib.veto_train_workspace_bytes_plan(eng.handle, inp.n_obj, inp.n_pair, ctypes.byref(opts), plan_ref)
            if need == 0:
                raise native.VetoError("veto_amd: %s" % launch.lib.veto_last_error().decode())
        # tens of GB: keep one workspace on the module and hand it to the next step once its backward has run (an
        # allocation of this size goes to the driver every time, and releasing it synchronises the device)
        # The cached workspace belongs to at most one forward whose backward has not run yet.  Ownership is a token held by
        # that forward's autograd context and seen here through a weak reference: a forward that never gets a backward
        # (torch.no_grad(), a loss-only validation pass, an exception in between) drops its context, the token dies with it
        # and the workspace is free again -- no sticky flag.
        ws = owner.__dict__.get("_train_ws")
        holder = owner.__dict__.get("_train_ws_owner")
        busy = holder is not None and holder() is not None and not holder().done
        if ws is None or ws.numel() < need or ws.device != device or busy:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            if not busy:
                owner.__dict__["_train_ws"] = ws
        ctx.ws_token = None
        if ws is owner.__dict__.get("_train_ws"):
            ctx.ws_token = _WsToken()
            owner.__dict__["_train_ws_owner"] = weakref.ref(ctx.ws_token)
        out = torch.empty((inp.n_pair, owner._num_out), dtype=torch.float32, device=device)
        if plan is None:
            launch.run("veto_forward_train", ctypes.byref(inp), ctypes.byref(opts), ws.data_ptr(), ws.numel(), out.data_ptr(), handle=eng.handle)
        else:
            launch.run("veto_forward_train_plan", ctypes.byref(inp), ctypes.byref(opts), plan_ref, ws.data_ptr(), ws.numel(), out.data_ptr(),
                       handle=eng.handle)
        ctx.opts = opts
        if stats is not None:
            with torch.no_grad():    # nn.BatchNorm1d(momentum=0.001) running statistics
                m = bn.momentum
                bn.running_mean.mul_(1 - m).add_(stats[0:4].to(bn.running_mean.device), alpha=m)
                bn.running_var.mul_(1 - m).add_(stats[8:12].to(bn.running_var.device), alpha=m)
                bn.num_batches_tracked += 1
        ctx.owner, ctx.inp, ctx.launch, ctx.ws, ctx.eng = owner, inp, launch, ws, eng   # (launch: the tensors `inp` points into)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        owner, eng = ctx.owner, ctx.eng
        device = dlogits.device
        launch = native.Launch(device, "veto_amd: the predictor runs only on a HIP device")
        dlogits = dlogits.detach().to(torch.float32).contiguous()
        flat = torch.empty(launch.lib.veto_grad_floats(eng.handle), dtype=torch.float32, device=device)
        d_rgb = d_dep = None
        n_obj = ctx.inp.n_obj
        if ctx.needs_input_grad[2]:
            d_rgb = torch.empty((n_obj, 256, owner._resolution, owner._resolution), dtype=torch.float32, device=device)
        if ctx.needs_input_grad[3]:
            d_dep = torch.empty((n_obj, 256, owner._resolution, owner._resolution), dtype=torch.float32, device=device)
        ctx.opts.d_roi_rgb, ctx.opts.d_roi_depth = launch.ptr(d_rgb), launch.ptr(d_dep)
        if ctx.plan is None:
            launch.run("veto_backward", ctypes.byref(ctx.inp), ctypes.byref(ctx.opts), ctx.ws.data_ptr(), ctx.ws.numel(),
                       launch.ptr(dlogits), flat.data_ptr(), handle=eng.handle)
        else:      # (only the regions of `flat` that belong to trainable tensors are written, and only those are read below)
            launch.run("veto_backward_plan", ctypes.byref(ctx.inp), ctypes.byref(ctx.opts), ctypes.byref(ctx.plan), ctx.ws.data_ptr(),
                       ctx.ws.numel(), launch.ptr(dlogits), flat.data_ptr(), handle=eng.handle)
        if ctx.ws_token is not None:
            ctx.ws_token.done = True
        offsets = eng.weight_offsets()
        grads = []
        for prm, name, row0, rows in ctx.spec:
            if not prm.requires_grad:      # frozen: autograd did not ask, and under a plan the region was never written
                grads.append(None)
                continue
            off, numel = offsets[name]
            if rows is None:
                g = flat[off:off + numel]
            else:
                per_row = prm.numel() // rows
                g = flat[off + row0 * per_row: off + (row0 + rows) * per_row]
            grads.append(g.view_as(prm).to(prm.device))
        return (None, None, d_rgb, d_dep) + tuple(grads)


def _cat_field(proposals, name):
    return torch.cat([p.get_field(name) for p in proposals], 0)




@ROI_RELATION_PREDICTOR.register("VETOPredictor")
class VETOPredictor(nn.Module, _NativeForward):
    def __init__(self, config, in_channels):
        super().__init__()
        self.mode = _mode(config)
        statistics = _dataset_statistics(config)
        self.obj_classes, self.rel_classes = statistics["obj_classes"], statistics["rel_classes"]
        self.num_obj_cls, self.num_rel_cls = len(self.obj_classes), len(self.rel_classes)
        self.embed_dim = 200
        _build_trunk(self, config, self.num_obj_cls, with_embed2=True)
        vecs = _embedding_vectors(self.obj_classes, getattr(config, "GLOVE_DIR", ""), self.embed_dim)
        with torch.no_grad():
            self.obj_embed.weight.copy_(vecs)
        dim = config.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.T_INPUT_DIM
        self.rel_out = _xavier_linear(dim, self.num_rel_cls)
        self.beta_loss = bool(config.GLOBAL_SETTING.BETA_LOSS)
        weights = torch.ones(self.num_rel_cls)
        if self.beta_loss:
            weights = class_balanced_weights(getattr(config.GLOBAL_SETTING, "REL_COUNTS", None), self.num_rel_cls)
        self.criterion_loss_rel = nn.CrossEntropyLoss(weight=weights)
        self.criterion_loss = nn.CrossEntropyLoss()
        self._native_init(config, self, self.num_obj_cls, [self.rel_out])
        self._train_forward_only = bool(getattr(getattr(config, "VETO_AMD", None), "TRAIN_FORWARD_ONLY", False))

    def forward(self, proposals, rel_pair_idxs, rel_labels, logger, roi_features=None,
                roi_depth_features=None, rel_binarys=None):
        if self.mode == "predcls":
            labels = _cat_field(proposals, "labels").long()
            logits = None
            obj_label_for_dist = labels
        else:
            logits = _cat_field(proposals, "predict_logits").detach()
            obj_label_for_dist = _cat_field(proposals, "pred_labels").detach().long()
            labels = None
        if self.training:   # :4127-4136: losses only
            from .losses import ce_loss, relation_ce_loss
            target = torch.cat(list(rel_labels), 0)
            w = self.criterion_loss_rel.weight
            add_losses = {}
            if self._train_forward_only:
                rel, _, _ = self._run_native_train(proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits)
                add_losses["rel_loss"] = relation_ce_loss(rel, target, weight=w)[0][0]
            else:
                rel = self._run_native_train_grad(proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, logits)
                add_losses["rel_loss"] = ce_loss(rel, target, weight=w)
            if self.mode != "predcls":   # :4129-4132: CE over obj_dists, which is the ONE-HOT of pred_labels here
                fg = _cat_field(proposals, "labels").long()
                onehot = nn.functional.one_hot(obj_label_for_dist.to(rel.device), self.num_obj_cls).float()
                add_losses["obj_loss"] = relation_ce_loss(onehot, fg)[0][0]
            return None, None, add_losses, None, None, None
        rel, n_objs, n_pairs = self._run_native(proposals, rel_pair_idxs, roi_features, roi_depth_features,
                                                labels, logits, debug=getattr(self, "debug_outputs", False))
        obj_dists = nn.functional.one_hot(obj_label_for_dist.to(rel.device), self.num_obj_cls).float()
        return obj_dists.split(n_objs, dim=0), rel.split(n_pairs, dim=0), {}, None, None, None


def class_balanced_weights(counts, num_cls, beta=0.999):
    """BETA_LOSS class weights (roi_relation_predictors.py:4058-4066). The reference reads a
    hard-coded absolute pickle path; here the 51 counts come from GLOBAL_SETTING.REL_COUNTS."""
    if counts is None:
        raise ValueError("GLOBAL_SETTING.BETA_LOSS needs GLOBAL_SETTING.REL_COUNTS (the predicate counts of "
                         "the reference's pred_counts.pkl)")
    c = torch.as_tensor(counts, dtype=torch.float64)
    if c.numel() != num_cls:
        raise ValueError("REL_COUNTS must have %d entries" % num_cls)
    c = torch.sort(c, descending=True)[0]
    w = (1.0 - beta) / (1.0 - beta ** c)
    return (w * (num_cls / w.sum())).float()


class _EnsembleParams(_Holder):
    """Parameter tree of the reference's `Ensemble` (roi_relation_predictors.py:3661-3744)."""

    def __init__(self, config, num_obj_cls, sizes, obj_classes, experts_per_group=1, expert_group=False):
        super().__init__()
        _build_trunk(self, config, num_obj_cls, with_embed2=False)
        vecs = _embedding_vectors(obj_classes, getattr(config, "GLOVE_DIR", ""), 200)
        with torch.no_grad():
            self.obj_embed.weight.copy_(vecs)
        dim = config.MODEL.ROI_RELATION_HEAD.VETOTRANSFORMER.T_INPUT_DIM
        self.rel_out_group = nn.ModuleList([])
        if expert_group:
            # :3717-3723: experts_per_group lists of K heads; `rel_out` stays bound to the LAST list, so the
            # state dict holds it twice (rel_out.{k} and rel_out_group.{E-1}.{k} are the same tensors)
            for _ in range(experts_per_group):
                self.rel_out = nn.ModuleList(_xavier_linear(dim, g + 2) for g in sizes)
                self.rel_out_group.append(self.rel_out)
        else:
            self.rel_out = nn.ModuleList(_xavier_linear(dim, g + 2) for g in sizes)
        self.CE_loss = nn.CrossEntropyLoss()
        self.criterion_loss = nn.CrossEntropyLoss()


@ROI_RELATION_PREDICTOR.register("VETOPredictor_MEET")
class VETOPredictor_MEET(nn.Module, _NativeForward):
    def __init__(self, config, in_channels):
        super().__init__()
        self.mode = _mode(config)
        statistics = _dataset_statistics(config)
        self.params = {"statistics": statistics, "obj_classes": statistics["obj_classes"],
                       "rel_classes": statistics["rel_classes"]}
        dataset = config.GLOBAL_SETTING.DATASET_CHOICE
        self.group_split_mode = config.GCL_SETTING.GROUP_SPLIT_MODE
        self.max_group_element_number_list = meet_tables.group_sizes(dataset, self.group_split_mode)
        self.incre_idx_list = meet_tables.incre_idx_list(self.max_group_element_number_list)
        self.num_groups = len(self.max_group_element_number_list)
        # :3901-3903: three experts per group unless ENSEMBLE_LEARNING.EXPERT_GROUP is off
        self.expert_group = bool(config.ENSEMBLE_LEARNING.EXPERT_GROUP)
        self.experts_per_group = 3 if self.expert_group else 1
        self.num_obj_cls = len(self.params["obj_classes"])
        self.model = _EnsembleParams(config, self.num_obj_cls, self.max_group_element_number_list,
                                     self.params["obj_classes"], self.experts_per_group, self.expert_group)
        # head columns of the one fused GEMV: expert-major, then group (all heads read the same CLS row)
        if self.expert_group:
            heads = [h for lst in self.model.rel_out_group for h in lst]
        else:
            heads = list(self.model.rel_out)
        self._native_init(config, self.model, self.num_obj_cls, heads)
        self._train_forward_only = bool(getattr(getattr(config, "VETO_AMD", None), "TRAIN_FORWARD_ONLY", False))
        self._dataset, self._sampler = dataset, None
        self._zero_label_padding_mode = str(config.GCL_SETTING.ZERO_LABEL_PADDING_MODE)
        self.nms_thresh = float(config.TEST.RELATION.LATER_NMS_PREDICTION_THRES)   # Ensemble.__init__ :3670

    def forward(self, proposals, rel_pair_idxs, rel_labels, logger, roi_features=None,
                roi_depth_features=None, rel_binarys=None):
        if self.mode == "predcls":
            labels = _cat_field(proposals, "labels").long()
            dist_labels = labels
        else:
            dist_labels = _cat_field(proposals, "pred_labels").detach().long()
            if self.mode == "sgdet" and not self.training:
                # :3778-3781: the decoder's class-aware NMS over softmax(one_hot(pred_labels)), on the device
                from .sgdet import decode_objects
                boxes_per_cls = torch.cat([p.get_field("boxes_per_cls").reshape(len(p), -1, 4) for p in proposals], 0)
                labels, _, _ = decode_objects(dist_labels, boxes_per_cls.to(dist_labels.device), [len(p) for p in proposals],
                                              self.nms_thresh, mode="meet", want_scores=False, want_boxes=False)
            else:
                # obj_dists[:, 1:].max(1)[1] + 1 over a one-hot (:3776-3784): the label itself, or 1 for label 0 (sgcls, and
                # sgdet in training, where the reference skips the decoder NMS)
                labels = torch.where(dist_labels > 0, dist_labels, torch.ones_like(dist_labels))
        if self.training:
            # :3930-3969 expert sampling, :3806-3846 group label remap + per-group CE
            from .losses import MeetTrainingSampler, ce_loss, relation_ce_loss
            if self._train_forward_only:
                rel, _, _ = self._run_native_train(proposals, rel_pair_idxs, roi_features, roi_depth_features, labels, None)
            else:
                rel = self._run_native_train_grad(proposals, rel_pair_idxs, roi_features, roi_depth_features, labels)
            if self._sampler is None or self._sampler.device != rel.device:
                self._sampler = MeetTrainingSampler(self._dataset, self.max_group_element_number_list, device=rel.device,
                                                    zero_label_padding_mode=self._zero_label_padding_mode)
            chosen, group_labels = self._sampler.sample(torch.cat(list(rel_labels), 0))
            add_losses, col = {}, 0
            for e in range(self.experts_per_group):      # :3833-3846: every expert of a group sees the same rows and labels
                for k, g in enumerate(self.max_group_element_number_list):
                    sl = rel[:, col:col + g + 2]
                    key = "group_%d%d_CE_loss" % (k, e + 1) if self.expert_group else "group_%d_CE_loss" % k
                    add_losses[key] = relation_ce_loss(sl, group_labels[k], rows=chosen[k])[0][0] \
                        if self._train_forward_only else ce_loss(sl, group_labels[k], rows=chosen[k])
                    col += g + 2
            if self.mode != "predcls":   # :3823-3827
                obj_logits = _cat_field(proposals, "predict_logits").detach()
                add_losses["obj_loss"] = relation_ce_loss(obj_logits.to(rel.device), _cat_field(proposals, "labels").long())[0][0]
            return None, None, add_losses, self.incre_idx_list, [chosen], None
        rel, n_objs, n_pairs = self._run_native(proposals, rel_pair_idxs, roi_features, roi_depth_features,
                                                labels, None, debug=getattr(self, "debug_outputs", False))
        rel_dists, col = {}, 0
        for e in range(self.experts_per_group):
            for k, g in enumerate(self.max_group_element_number_list):
                # :3833-3841: 'group_<k><expert 1..3>' with EXPERT_GROUP, 'group_<k>' without
                key = "group_%d%d" % (k, e + 1) if self.expert_group else "group_%d" % k
                rel_dists[key] = rel[:, col:col + g + 2]
                col += g + 2
        obj_dists = nn.functional.one_hot(dist_labels.to(rel.device), self.num_obj_cls).float().split(n_objs, dim=0)
        return obj_dists, rel_dists, {}, self.incre_idx_list, None, {}
