"""Name -> predictor registry with the same protocol as the reference's
pysgg/utils/registry.py:9-45 (`registry.ROI_RELATION_PREDICTOR`, modeling/registry.py:16):
a dict whose `register(name)` works as a decorator or as a direct call.

The reference's `register` asserts the name is not taken (utils/registry.py:4-6), so a drop-in
replacement cannot simply register itself next to the original; `install()` overwrites the two
VETO entries of an existing pysgg registry instead ("Registration").
"""


class Registry(dict):
    def register(self, name, module=None):
        if module is not None:
            self._add(name, module)
            return module

        def deco(fn):
            self._add(name, fn)
            return fn

        return deco

    def _add(self, name, module):
        if name in self:
            raise AssertionError("%r is already registered" % (name,))
        self[name] = module


ROI_RELATION_PREDICTOR = Registry()


def make_roi_relation_predictor(cfg, in_channels):
    """Same lookup as roi_relation_predictors.py:4152-4154."""
    func = ROI_RELATION_PREDICTOR[cfg.MODEL.ROI_RELATION_HEAD.PREDICTOR]
    return func(cfg, in_channels)


def install(target_registry=None):
    """Point the reference's registry at the MI355X predictors.

    With no argument, imports `pysgg.modeling.registry` (the reference must be importable).
    Returns the registry that was patched."""
    from . import predictor  # noqa: F401  (registers into ROI_RELATION_PREDICTOR)
    if target_registry is None:
        from pysgg.modeling import registry as ref_registry  # type: ignore
        target_registry = ref_registry.ROI_RELATION_PREDICTOR
    for name in ("VETOPredictor", "VETOPredictor_MEET"):
        dict.__setitem__(target_registry, name, ROI_RELATION_PREDICTOR[name])
    return target_registry


def install_detector_ops():
    """Point the reference's detector at the device decoder: `pysgg.layers.nms` and `boxlist_ops._box_nms` (boxlist_nms:
    the box head's and the RPN's NMS) become veto_amd.layers.nms, and `box_head.inference.make_roi_box_post_processor`
    returns veto_amd.boxhead.PostProcessor.  `pysgg` must be importable.  Independent of install().  Returns the patched
    (module, name) pairs."""
    import importlib
    from . import boxhead, layers
    patched = []
    for mod, name, value in (("pysgg.layers", "nms", layers.nms),
                             ("pysgg.structures.boxlist_ops", "_box_nms", layers.nms),
                             ("pysgg.modeling.roi_heads.box_head.inference", "make_roi_box_post_processor",
                              boxhead.make_roi_box_post_processor)):
        setattr(importlib.import_module(mod), name, value)
        patched.append((mod, name))
    # box_head.py binds the factory by name when it is imported (box_head.py:8): re-point that binding too if it exists
    import sys
    head = sys.modules.get("pysgg.modeling.roi_heads.box_head.box_head")
    if head is not None and hasattr(head, "make_roi_box_post_processor"):
        head.make_roi_box_post_processor = boxhead.make_roi_box_post_processor
    return patched


def install_rpn_ops():
    """Point the reference's RPN at the device proposal selector: `pysgg.modeling.rpn.inference.make_rpn_postprocessor`
    returns veto_amd.rpn.RPNPostProcessor.  `pysgg` must be importable.  Independent of install() and
    install_detector_ops().  Returns the patched (module, name) pairs."""
    import importlib
    import sys
    from . import rpn
    setattr(importlib.import_module("pysgg.modeling.rpn.inference"), "make_rpn_postprocessor", rpn.make_rpn_postprocessor)
    patched = [("pysgg.modeling.rpn.inference", "make_rpn_postprocessor")]
    # rpn.py binds the factory by name when it is imported (rpn.py:10): re-point that binding too if it exists
    head = sys.modules.get("pysgg.modeling.rpn.rpn")
    if head is not None and hasattr(head, "make_rpn_postprocessor"):
        head.make_rpn_postprocessor = rpn.make_rpn_postprocessor
        patched.append(("pysgg.modeling.rpn.rpn", "make_rpn_postprocessor"))
    return patched


def install_box_sampling_ops():
    """Point the reference's box head at the device sampler: `pysgg.modeling.roi_heads.box_head.sampling.make_roi_box_samp_processor`
    returns veto_amd.boxsampling.FastRCNNSampling (assign_label_to_proposals, prepare_targets, subsample).  `pysgg` must be
    importable.  Independent of install(), install_detector_ops() and install_rpn_ops().  Returns the patched (module, name)
    pairs."""
    import importlib
    import sys
    from . import boxsampling
    setattr(importlib.import_module("pysgg.modeling.roi_heads.box_head.sampling"), "make_roi_box_samp_processor",
            boxsampling.make_roi_box_samp_processor)
    patched = [("pysgg.modeling.roi_heads.box_head.sampling", "make_roi_box_samp_processor")]
    # box_head.py binds the factory by name when it is imported (box_head.py:9): re-point that binding too if it exists
    head = sys.modules.get("pysgg.modeling.roi_heads.box_head.box_head")
    if head is not None and hasattr(head, "make_roi_box_samp_processor"):
        head.make_roi_box_samp_processor = boxsampling.make_roi_box_samp_processor
        patched.append(("pysgg.modeling.roi_heads.box_head.box_head", "make_roi_box_samp_processor"))
    return patched


def install_rpn_loss_ops():
    """Point the reference's RPN at the device loss: `pysgg.modeling.rpn.loss.make_rpn_loss_evaluator` returns
    veto_amd.rpnloss.RPNLossComputation (anchor matching, fg/bg sampling, both losses and their gradients in one call).  `pysgg`
    must be importable.  Independent of install(), install_detector_ops(), install_rpn_ops() and install_box_sampling_ops().
    Returns the patched (module, name) pairs."""
    import importlib
    import sys
    from . import rpnloss
    setattr(importlib.import_module("pysgg.modeling.rpn.loss"), "make_rpn_loss_evaluator", rpnloss.make_rpn_loss_evaluator)
    patched = [("pysgg.modeling.rpn.loss", "make_rpn_loss_evaluator")]
    # rpn.py binds the factory by name when it is imported (rpn.py:9): re-point that binding too if it exists
    head = sys.modules.get("pysgg.modeling.rpn.rpn")
    if head is not None and hasattr(head, "make_rpn_loss_evaluator"):
        head.make_rpn_loss_evaluator = rpnloss.make_rpn_loss_evaluator
        patched.append(("pysgg.modeling.rpn.rpn", "make_rpn_loss_evaluator"))
    return patched


_ANCHOR_ORIGINALS = []   # (module, name, what install_anchor_ops replaced), for uninstall_anchor_ops


def install_anchor_ops():
    """Point the reference's RPN at the device anchor generator: `pysgg.modeling.rpn.anchor_generator.make_anchor_generator`,
    `make_anchor_generator_retinanet` and the class `AnchorGenerator` become veto_amd.rpn's (one launch per forward for the anchors
    of every level and the visibility of every image, the anchors cached per grid shape).  Modules that bound one of them by name
    when they were imported (`from .anchor_generator import make_anchor_generator`, rpn/rpn.py:9;
    `make_anchor_generator_retinanet`, rpn/retinanet/retinanet.py:8) are re-pointed too.  `pysgg` must be importable.
    Independent of the other installers.  Returns the patched (module, name) pairs; uninstall_anchor_ops() puts the originals
    back."""
    import importlib
    import sys
    import types
    from . import rpn
    patched = []
    module = importlib.import_module("pysgg.modeling.rpn.anchor_generator")
    for name in ("make_anchor_generator", "make_anchor_generator_retinanet", "AnchorGenerator"):
        value, original = getattr(rpn, name), getattr(module, name)
        if original is value:
            continue
        targets = [(module.__name__, module)] + sorted((n, m) for n, m in list(sys.modules.items())
                                                       if isinstance(m, types.ModuleType) and m is not module and vars(m).get(name) is original)
        for n, m in targets:
            if vars(m).get(name) is original:
                setattr(m, name, value)
                _ANCHOR_ORIGINALS.append((m, name, original))
                patched.append((n, name))
    return patched


def uninstall_anchor_ops():
    """Undo install_anchor_ops: every name it replaced gets its original back.  Returns how many."""
    n = len(_ANCHOR_ORIGINALS)
    while _ANCHOR_ORIGINALS:
        module, name, original = _ANCHOR_ORIGINALS.pop()
        setattr(module, name, original)
    return n


def install_box_loss_ops():
    """Point the reference's box head at the device loss: `pysgg.modeling.roi_heads.box_head.loss.make_roi_box_loss_evaluator`
    returns veto_amd.boxloss.FastRCNNLossComputation (both losses and their gradients in one call).  `pysgg` must be importable.
    Independent of install(), install_detector_ops(), install_rpn_ops(), install_box_sampling_ops() and install_rpn_loss_ops().
    Returns the patched (module, name) pairs."""
    import importlib
    import sys
    from . import boxloss
    setattr(importlib.import_module("pysgg.modeling.roi_heads.box_head.loss"), "make_roi_box_loss_evaluator",
            boxloss.make_roi_box_loss_evaluator)
    patched = [("pysgg.modeling.roi_heads.box_head.loss", "make_roi_box_loss_evaluator")]
    # box_head.py binds the factory by name when it is imported (box_head.py:6): re-point that binding too if it exists
    head = sys.modules.get("pysgg.modeling.roi_heads.box_head.box_head")
    if head is not None and hasattr(head, "make_roi_box_loss_evaluator"):
        head.make_roi_box_loss_evaluator = boxloss.make_roi_box_loss_evaluator
        patched.append(("pysgg.modeling.roi_heads.box_head.box_head", "make_roi_box_loss_evaluator"))
    return patched


def install_pooler_ops():
    """Point the reference's ROI pooling at the device kernels: `pysgg.layers.ROIAlign` (and `pysgg.layers.roi_align.ROIAlign`,
    which it was imported from) become veto_amd.poolers.ROIAlign and `pysgg.modeling.poolers.Pooler` becomes veto_amd.poolers.Pooler -- the box head's 7 x 7
    pooler included, whose `pysgg._C.roi_align_forward` has no HIP build.  Modules that bound one of the originals by name when
    they were imported (`from pysgg.modeling.poolers import Pooler`, roi_box_feature_extractors.py:8; `from pysgg.layers import
    ROIAlign`, poolers.py:6) are re-pointed too.  sampling_ratio 0, the default of pysgg/config/defaults.py, is served (the adaptive
    grid, veto_roi_pool_adaptive); its backward raises in the ordered mode.  Pooler(cat_all_levels=True) and Pooler.forward(union=True) keep raising.
    `pysgg` must be importable.  Independent of the other installers.  Returns the patched (module, name) pairs."""
    import importlib
    import sys
    import types
    from . import poolers
    patched = []
    for mod, name, value in (("pysgg.layers", "ROIAlign", poolers.ROIAlign),
                             ("pysgg.modeling.poolers", "Pooler", poolers.Pooler)):
        module = importlib.import_module(mod)
        original = getattr(module, name)
        if original is value:
            continue
        targets = [(mod, module)] + sorted((n, m) for n, m in list(sys.modules.items())
                                           if isinstance(m, types.ModuleType) and m is not module and vars(m).get(name) is original)
        for n, m in targets:
            if vars(m).get(name) is original:
                setattr(m, name, value)
                patched.append((n, name))
    return patched


_SOLVER_ORIGINALS = []   # (module, name, what install_solver_ops replaced), for uninstall_solver_ops


def install_solver_ops():
    """Point the reference's training loop at the device optimizer: `pysgg.solver.build.make_optimizer` and
    `pysgg.solver.make_optimizer` return veto_amd.solver.Adam, and `pysgg.utils.checkpoint.clip_grad_norm` is
    veto_amd.solver.clip_grad_norm.  Modules that bound one of the originals by name when they were imported
    (`from pysgg.solver import make_optimizer`, tools/relation_train_net.py:27-29) are re-pointed too.  `pysgg` must be
    importable.  Independent of the other installers.  Returns the patched (module, name) pairs; uninstall_solver_ops() puts
    the originals back."""
    import importlib
    import sys
    import types
    from . import solver
    patched = []
    for mod, name, value in (("pysgg.solver.build", "make_optimizer", solver.make_optimizer),
                             ("pysgg.solver", "make_optimizer", solver.make_optimizer),
                             ("pysgg.utils.checkpoint", "clip_grad_norm", solver.clip_grad_norm)):
        module = importlib.import_module(mod)
        original = getattr(module, name)
        if original is value:
            continue
        targets = [(mod, module)] + sorted((n, m) for n, m in list(sys.modules.items())
                                           if isinstance(m, types.ModuleType) and m is not module and vars(m).get(name) is original)
        for n, m in targets:
            if vars(m).get(name) is original:
                setattr(m, name, value)
                _SOLVER_ORIGINALS.append((m, name, original))
                patched.append((n, name))
    return patched


def uninstall_solver_ops():
    """Undo install_solver_ops: every name it replaced gets its original back.  Returns how many."""
    n = len(_SOLVER_ORIGINALS)
    while _SOLVER_ORIGINALS:
        module, name, original = _SOLVER_ORIGINALS.pop()
        setattr(module, name, original)
    return n
