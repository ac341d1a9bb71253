"""The optimizer side of a training iteration on the HIP device: the caller side of veto_optim_step.

The reference's loop (tools/relation_train_net.py:470-483) runs, after loss.backward(), `clip_grad_norm`
(pysgg/utils/checkpoint.py:180-219: one norm per parameter, a read-back of the coefficient, one mul_ per parameter) and the step
of the torch.optim.Adam that `make_optimizer` builds with one param group per parameter (pysgg/solver/build.py:7-34), which
torch therefore steps one tensor at a time.  Here all of it is one call over a table of tensors: two launches for norms, clip and
step together, one for the step alone, whatever the number of tensors, and no device->host copy.  The arithmetic, the order of
the norm's summation and the NaN / Inf cases: include/veto_amd.h.

`optim_call` is the one ABI call.  `Adam` is a torch.optim.Optimizer with torch.optim.Adam's param-group keys and state
(`step`, `exp_avg`, `exp_avg_sq`), so state_dict() / load_state_dict() interchange with it both ways; `clip_grad_norm` and
`make_optimizer` have the reference's signatures (registry.install_solver_ops points the reference at them)."""
import ctypes

import torch

from . import native

CHUNK = native.VETO_OPTIM_CHUNK      # elements of one tensor per workgroup (VETO_OPTIM_CHUNK)
MAX_TENSORS = 4096
MAX_NUMEL = (1 << 31) - 1
NORMS, CLIP, STEP, CLIP_STEP = native.VETO_OPTIM_NORMS, native.VETO_OPTIM_CLIP, native.VETO_OPTIM_STEP, native.VETO_OPTIM_CLIP_STEP
_WHAT = "veto_amd.solver runs on a HIP device only"


def _check_tensor(t, what, device=None, numel=None):
    """A dense contiguous fp32 tensor (on `device`, of `numel` elements, where given); needs neither the device nor the library."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
    if t.layout != torch.strided:
        raise ValueError("%s is %s: only dense tensors are supported" % (what, t.layout))
    if t.dtype != torch.float32:
        raise ValueError("%s is %s: only float32 is supported" % (what, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s is not contiguous" % what)
    if t.numel() > MAX_NUMEL:
        raise ValueError("%s has %d elements, the limit is %d" % (what, t.numel(), MAX_NUMEL))
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, the others on %s: one HIP device is supported" % (what, t.device, device))
    if numel is not None and t.numel() != numel:
        raise ValueError("%s has %d elements, its parameter %d" % (what, t.numel(), numel))


def _hip_device(device):
    if device.type != "cuda":
        raise ValueError("%s (got %s)" % (_WHAT, device))
    return device


def optim_call(rows, mode, max_norm=0.0, table=None, checked=False):
    """One veto_optim_step call.  rows: a sequence of (param, grad, exp_avg, exp_avg_sq, step, lr, weight_decay, beta1, beta2,
    eps), all tensors contiguous fp32 on one HIP device.  grad None: the tensor takes no part (its other tensors may be None
    too).  In the modes that only take norms (NORMS, CLIP) param and state may be None and the scalars are not read.  `step` is
    the count including this update.  table: a native.VetoOptimTensor array of at least len(rows) to fill instead of a new one
    (the library has copied what it needs when the call returns).  Every tensor of every row is checked here (dense contiguous
    fp32 on the one device, state and gradient of the parameter's size) unless checked=True says that the caller has done so.
    Returns {} for STEP, else device tensors: norms [len(rows)], total_norm and coef (0-dim; coef is the applied coefficient).
    CLIP scales the gradients in place; CLIP_STEP leaves them as they are.  No device->host copy and no synchronisation.
    Gradients are kept alive on the stream by record_stream; parameters and state belong to the caller for as long as it steps."""
    n = len(rows)
    if not 1 <= n <= MAX_TENSORS:
        raise ValueError("%d tensors: 1..%d are supported" % (n, MAX_TENSORS))
    if mode not in (NORMS, CLIP, STEP, CLIP_STEP):
        raise ValueError("unknown mode %r" % (mode,))
    max_norm = float(max_norm)
    if mode in (CLIP, CLIP_STEP) and not max_norm > 0:
        raise ValueError("max_norm must be > 0 to clip, got %r" % max_norm)
    device = next((t.device for r in rows for t in r[:4] if t is not None), None)
    if device is None:
        raise ValueError("no tensor in the table")
    _hip_device(device)
    if not checked:
        steps = mode in (STEP, CLIP_STEP)
        for i, r in enumerate(rows):
            p, g, m, v = r[:4]
            size = next((t.numel() for t in (p, g) if t is not None), None)
            for t, what in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
                if t is not None:
                    _check_tensor(t, "row %d: %s" % (i, what), device, size)
                elif steps and g is not None and g.numel() and what != "grad":
                    raise ValueError("row %d: %s is missing in a mode that steps" % (i, what))
    call = native.Launch(device, _WHAT)
    if table is None:
        table = (native.VetoOptimTensor * n)()
    for e, (p, g, m, v, step, lr, wd, b1, b2, eps) in zip(table, rows):
        e.param = p.data_ptr() if p is not None else None
        e.exp_avg = m.data_ptr() if m is not None else None
        e.exp_avg_sq = v.data_ptr() if v is not None else None
        if g is not None and g.numel():
            e.grad = call.ptr(g)
            e.numel = g.numel()
        else:
            e.grad = None
            e.numel = p.numel() if p is not None else 0
        e.step, e.lr, e.weight_decay, e.beta1, e.beta2, e.eps = int(step), lr, wd, b1, b2, eps
    out = {}
    a = native.VetoOptimArgs(struct_size=ctypes.sizeof(native.VetoOptimArgs), tensor_size=ctypes.sizeof(native.VetoOptimTensor),
                             n_tensors=n, mode=mode, max_norm=max_norm, tensors=table)
    if mode != STEP:
        buf = torch.empty(n + 2, dtype=torch.float32, device=device)      # norms | total_norm | coef: one allocation
        out = {"norms": buf[:n], "total_norm": buf[n], "coef": buf[n + 1]}
        a.norms, a.total_norm, a.coef = buf.data_ptr(), buf.data_ptr() + 4 * n, buf.data_ptr() + 4 * (n + 1)
        call._tensors.append(buf)
    need = call.lib.veto_optim_step_workspace_bytes(ctypes.byref(a))      # (0: the sizes are out of range, the call says which)
    ws = call.workspace(need)
    call.run("veto_optim_step", ctypes.byref(a), ws.data_ptr(), ws.numel())
    return out


def _grad_of(p, what):
    g = p.grad
    if g is None:
        return None
    if g.is_sparse:
        raise ValueError("%s has a sparse gradient: only dense gradients are supported" % what)
    _check_tensor(g, "the gradient of %s" % what, p.device, p.numel())
    return g


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (single-tensor form, coupled weight decay) whose step is one veto_optim_step call over every parameter
    with a gradient.  Param-group keys, per-parameter state and the meaning of `step` (a CPU float32 0-dim tensor, incremented
    only when the parameter has a gradient) are torch's, so a state_dict moves between the two classes in both directions.
    group["lr"] and the other hyper-parameters are read at every call: LR schedulers work unchanged.
    Refused: amsgrad, maximize, capturable, differentiable, decoupled_weight_decay, a closure, parameters that are not contiguous
    float32 on one HIP device, sparse or non-float32 gradients, more than 4096 parameters with a gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("lr and betas must be Python numbers (a tensor would have to be read back at every step)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %r" % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %r" % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._table = None
        self._cache = {}
        self._check_groups()

    def _check_groups(self):
        """What needs neither the device nor the library: the flags of every group, and every parameter dense contiguous float32."""
        for group in self.param_groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"):
                if group.get(flag):
                    raise ValueError("veto_amd.solver.Adam does not support %s=True" % flag)
            for p in group["params"]:
                _check_tensor(p, "a parameter")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_groups()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._table = None
        self._cache = {}
        for group in self.param_groups:       # as torch.optim.Adam.__setstate__: older state dicts lack the newer keys
            for key, value in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                               ("differentiable", False), ("fused", None), ("decoupled_weight_decay", False)):
                group.setdefault(key, value)

    def _state_of(self, p):
        """torch.optim.Adam._init_group: lazy, `step` on the host."""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not torch.is_tensor(state["step"]):
            state["step"] = torch.tensor(float(state["step"]), dtype=torch.float32)
        return state

    def _bind(self, p, device):
        """The state of p as a call uses it, checked once per set of state tensors: (step tensor, its numpy view, exp_avg,
        exp_avg_sq).  The view shares the tensor's memory, so counting a step costs no tensor operation."""
        state = self._state_of(p)
        _check_tensor(state["exp_avg"], "exp_avg", device, p.numel())
        _check_tensor(state["exp_avg_sq"], "exp_avg_sq", device, p.numel())
        step = state["step"]
        if step.device.type != "cpu" or step.dtype != torch.float32 or step.dim() != 0:
            raise ValueError("state['step'] must be a 0-dim float32 tensor on the host (capturable=False), got %s %s on %s"
                             % (tuple(step.shape), step.dtype, step.device))
        return (step, step.numpy(), state["exp_avg"], state["exp_avg_sq"])

    def _rows(self):
        """Every check first, for every parameter with a gradient (nothing has changed when one fails); then the rows of the call,
        each with its step count including this update, and the bound state records (_bind) to count the steps on.  This loop is the host cost of a step: the checks are one condition per
        parameter, and whatever they refuse is named by the slow path."""
        f32, strided = torch.float32, torch.strided
        todo, device = [], None
        for group in self.param_groups:
            if group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or group["decoupled_weight_decay"]:
                self._check_groups()
            b1, b2 = group["betas"]
            hyper = (float(group["lr"]), float(group["weight_decay"]), float(b1), float(b2), float(group["eps"]))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if device is None:
                    device = p.device
                if not (g.dtype is f32 and g.layout is strided and g.is_contiguous() and g.device == device and p.dtype is f32
                        and p.is_contiguous() and p.device == device and g.numel() == p.numel()):
                    _check_tensor(p, "a parameter", device)
                    _grad_of(p, "a parameter")
                    raise ValueError("a parameter or its gradient is not a dense contiguous float32 tensor on %s" % device)
                todo.append((p, g, hyper))
        if device is not None:
            _hip_device(device)
        if len(todo) > MAX_TENSORS:
            raise ValueError("%d parameters with a gradient: the limit of one call is %d" % (len(todo), MAX_TENSORS))
        cache, states, bound = self._cache, self.state, []
        for p, g, hyper in todo:
            st, c = states[p], cache.get(p)
            if c is None or c[0] is not st.get("step") or c[2] is not st.get("exp_avg") or c[3] is not st.get("exp_avg_sq"):
                c = cache[p] = self._bind(p, device)
            bound.append(c)
        # (torch counts the step before the update; here the count is written back only once the call has been accepted, so a
        # refused or failed call leaves every step as it was)
        return [(p, g, c[2], c[3], int(c[1]) + 1) + hyper for (p, g, hyper), c in zip(todo, bound)], bound

    def _apply(self, mode, max_norm):
        rows, bound = self._rows()
        if not rows:
            return None
        if self._table is None or len(self._table) < len(rows):
            self._table = (native.VetoOptimTensor * len(rows))()
        out = optim_call(rows, mode, max_norm, table=self._table, checked=True)
        for r, c in zip(rows, bound):                      # the update is enqueued: now the steps count
            c[1][...] = r[4]
        # the parameters were written through raw pointers: tell autograd (and VETOPredictor._weights_version) that they changed
        torch.autograd.graph.increment_version([r[0] for r in rows])
        self._opt_called = True                            # what an LR scheduler looks at to see that a step came before its own
        return out

    @torch.no_grad()
    def step(self, closure=None):
        """The Adam step of every parameter with a gradient: one launch."""
        if closure is not None:
            raise ValueError("veto_amd.solver.Adam takes no closure")
        self._apply(STEP, 0.0)
        return None

    @torch.no_grad()
    def clip_and_step(self, max_norm):
        """clip_grad_norm(clip=True) and step() in one call: the global norm over every gradient, the coefficient, and the Adam
        step with each gradient scaled in registers.  The gradients in memory stay UNSCALED.  Returns the total norm as a 0-dim
        device tensor (0 when no parameter has a gradient).  Two launches, no device->host copy."""
        max_norm = float(max_norm)
        if not max_norm > 0:
            raise ValueError("max_norm must be > 0, got %r" % max_norm)
        out = self._apply(CLIP_STEP, max_norm)
        if out is None:
            p = next((p for group in self.param_groups for p in group["params"]), None)
            return torch.zeros((), dtype=torch.float32, device=p.device if p is not None else "cpu")
        self.last_norms, self.last_coef = out["norms"], out["coef"]
        return out["total_norm"]


def clip_grad_norm(named_parameters, max_norm, logger, clip=False, verbose=False):
    """checkpoint.py:180-219 with its signature.  The norm over all gradients as one vector; with clip=True every gradient is
    multiplied in place by max_norm / (total_norm + 1e-6) where that is below 1.  Returns the total norm as a 0-dim device
    tensor.  At most two launches and, unless verbose, no device->host copy; verbose=True makes one copy of the norms and logs
    the reference's lines."""
    max_norm = float(max_norm)
    if clip and not max_norm > 0:
        raise ValueError("max_norm must be > 0 to clip, got %r" % max_norm)
    named = [(n, p) for n, p in named_parameters]
    device = None
    rows, names = [], []
    for n, p in named:
        g = _grad_of(p, n)
        if g is None:
            continue
        if device is None:
            device = g.device
        elif g.device != device:
            raise ValueError("the gradient of %s is on %s, the others on %s: one HIP device is supported" % (n, g.device, device))
        rows.append((None, g, None, None, 1, 0.0, 0.0, 0.0, 0.0, 0.0))
        names.append((n, p.size()))
    if device is not None:
        _hip_device(device)
    if not rows:                                           # the reference returns the number 0.0
        return torch.zeros((), dtype=torch.float32, device=named[0][1].device if named else "cpu")
    if len(rows) > MAX_TENSORS:
        raise ValueError("%d gradients: the limit of one call is %d" % (len(rows), MAX_TENSORS))
    out = optim_call(rows, CLIP if clip else NORMS, max_norm)
    if verbose:
        host = torch.cat([out["norms"], out["total_norm"].reshape(1)]).cpu()      # the one copy
        total = float(host[-1])
        logger.info('---Total norm {:.5f} clip coef {:.5f}-----------------'.format(total, max_norm / (total + 1e-6)))
        for (name, shape), norm in zip(names, host[:-1].tolist()):
            logger.info("{:<50s}: {:f}, ({})".format(name, norm, shape))
        logger.info('-------------------------------')
    return out["total_norm"]


def _first(items, name):
    """The first of `items` (None: no rule) that occurs in `name`, else None."""
    return next((item for item in items or () if item in name), None)


def optimizer_groups(cfg, model, logger, slow_heads=None, except_weight_decay=None, slow_ratio=5.0, rl_factor=1.0):
    """One param group per trainable parameter, in named_parameters() order, with the lr and weight_decay that the reference's
    make_optimizer gives it (tests/test_optim_host.py pins the table and the log to the reference's own, name by name).  Keys
    read: SOLVER.BASE_LR, SOLVER.BIAS_LR_FACTOR, SOLVER.WEIGHT_DECAY, SOLVER.WEIGHT_DECAY_BIAS.  The rules, all on substrings of
    the parameter's name: "bias" takes the bias pair; any item of except_weight_decay sets weight_decay to 0 and EVERY matching
    item is logged; the FIRST matching item of slow_heads divides lr by slow_ratio, once, and is logged once; lr is then
    multiplied by rl_factor."""
    so = cfg.SOLVER
    groups = []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        is_bias = "bias" in name
        lr = so.BASE_LR * so.BIAS_LR_FACTOR if is_bias else so.BASE_LR
        weight_decay = so.WEIGHT_DECAY_BIAS if is_bias else so.WEIGHT_DECAY
        exempt = sum(1 for item in except_weight_decay or () if item in name)
        for _ in range(exempt):
            logger.info("NO WEIGHT DECAY: %s." % name)
        if exempt:
            weight_decay = 0.0
        if _first(slow_heads, name) is not None:
            logger.info("SLOW HEADS: %s is slow down by ratio of %s." % (name, slow_ratio))
            lr = lr / slow_ratio
        groups.append(dict(params=[param], lr=lr * rl_factor, weight_decay=weight_decay))
    return groups


def make_optimizer(cfg, model, logger, slow_heads=None, except_weight_decay=None, slow_ratio=5.0, rl_factor=1.0):
    """The reference's make_optimizer (solver/build.py:7-34) by signature and by the groups it makes; returns
    veto_amd.solver.Adam over them, with SOLVER.BASE_LR as the default lr, where the reference returns torch.optim.Adam."""
    return Adam(optimizer_groups(cfg, model, logger, slow_heads, except_weight_decay, slow_ratio, rl_factor), lr=cfg.SOLVER.BASE_LR)
