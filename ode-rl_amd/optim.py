"""`FusedAdam`: torch.optim.Adam semantics (the reference's optimizer, train_test.py:24) with ONE HIP launch per step for all
parameter tensors (csrc/optim_step.hip) instead of torch's per-op foreach launches.  State layout and `state_dict()` are those of
torch.optim.Adam (`step`, `exp_avg`, `exp_avg_sq`), so the reference's pickled optimizer state (helpers/utils.py:218-222)
loads into it and vice versa.

Gradient clipping by global norm (the reference's `opt.clip`, train_test.py:187-195) on the device: `clip_grad_norm_` stands in for
torch.nn.utils.clip_grad_norm_, and `FusedAdam(max_grad_norm=...)` folds the scaling into the optimizer launch.  Neither reads
anything back to the host.

`FusedAdamax` is the same for torch.optim.Adamax (csrc/optim_step.hip), the optimizer of Vid-ODE's recipe (Vid-ODE/main.py:187), and
`decay_learning_rate` that recipe's per-epoch decay (main.py:214)."""
import ctypes

import torch

from . import _lib
from .hip_ops import _ptr, _stream, require_device_tensor, workspace


_GROUPS = object()   # step(max_grad_norm=...) left out: the parameter groups' setting holds


def _clip_off(max_norm):
    """None and -1 (the reference's `clip == -1`) switch clipping off; anything else must be a norm bound >= 0."""
    if max_norm is None or max_norm == -1:
        return True
    if not float(max_norm) >= 0:
        raise ValueError(f"max_grad_norm must be None, -1 (off) or >= 0 (got {max_norm})")
    return False


def _tables(*lists):
    """Host arrays of device pointers, one per list of tensors, and the element counts of the first list."""
    n = len(lists[0])
    arrs = [(ctypes.c_void_p * n)(*[x.data_ptr() for x in xs]) for xs in lists]
    return arrs, (ctypes.c_longlong * n)(*[x.numel() for x in lists[0]]), n


def _grad_norm(grads, max_norm):
    """(total_norm, coef, clipped_norm) as one fresh (3,) device tensor -- csrc/optim_step.hip's two-stage sum of squares over `grads` -- and
    the host tables (pointers, element counts, n) it was called with."""
    lib = _lib.load()
    (g,), numel, n = _tables(grads)
    dev = grads[0].device
    nbytes = lib.odehip_grad_norm_workspace_bytes(n, numel)
    ws = workspace("grad_norm", nbytes, dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.check(lib.odehip_grad_norm(g, numel, n, float(max_norm), _ptr(ws), nbytes, _ptr(out3), _stream()))
    return out3, (g, numel, n)


def _on_hip_path(g):
    return g.is_cuda and g.dtype == torch.float32 and g.layout == torch.strided and g.is_contiguous()


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) with error_if_nonfinite=False: scales every `p.grad` in place by
    min(max_norm / (total_norm + 1e-6), 1) and returns total_norm, the norm BEFORE clipping, as a device scalar.  Parameters without
    a gradient are skipped; no gradients at all returns tensor(0.).  CUDA float32 dense contiguous gradients on one device take the HIP
    kernels (sum of squares in float64, no host synchronisation, ceil(n / 24) launches each for the norm and the scaling plus one for
    the coefficient); anything else is handed to torch's function."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only norm_type=2 is supported (got {norm_type})")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    grads = [p.grad for p in params]
    if not all(_on_hip_path(g) and g.device == grads[0].device for g in grads):
        return torch.nn.utils.clip_grad_norm_(params, float(max_norm))
    out3, (g, numel, n) = _grad_norm(grads, max_norm)
    _lib.check(_lib.load().odehip_grad_scale(g, numel, n, _ptr(out3[1:]), _stream()))
    return out3[0]


class _FusedOptimizer(torch.optim.Optimizer):
    """What FusedAdam and FusedAdamax share: everything about a step but the arithmetic of its kernel.  A subclass names the second
    state tensor (`_second`, torch's key for it), its two C entry points (`_step_fn`, `_clipped_fn`), which take the same arguments, and torch's name
    for the algorithm (`_kind`).

    max_grad_norm: None or -1 = no clipping (the step is the one launch per 24 tensors it always was); a bound >= 0 clips the
    gradients of ALL parameter groups together by their global L2 norm inside the step -- norm, coefficient, then the update launch
    reading the coefficient from the device -- and leaves `p.grad` scaled, as torch.nn.utils.clip_grad_norm_ before the step would.
    `last_grad_norm` / `last_clipped_norm`: the norm before / after clipping of the last clipped step (device scalars; tensor(0.) when that step had no gradient; None before)."""

    _kind = _second = _step_fn = _clipped_fn = None

    def __init__(self, params, lr, betas, eps, weight_decay, max_grad_norm):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError(f"invalid {self._kind} hyper-parameter")
        _clip_off(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self.last_grad_norm = None
        self.last_clipped_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:   # a torch.optim state dict has no such key
            group.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("last_grad_norm", None)
        self.__dict__.setdefault("last_clipped_norm", None)

    def _max_grad_norm(self):
        bounds = {None if _clip_off(g["max_grad_norm"]) else float(g["max_grad_norm"]) for g in self.param_groups}
        if len(bounds) > 1:
            raise ValueError(f"{type(self).__name__}: the norm is taken over all parameter groups, so they must share max_grad_norm (got {sorted(map(str, bounds))})")
        return bounds.pop() if bounds else None

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_GROUPS):
        """max_grad_norm: overrides the groups' setting for this call (None / -1: off); left out, the groups' setting holds."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        name = type(self).__name__
        if max_grad_norm is _GROUPS:
            max_grad_norm = self._max_grad_norm()
        elif _clip_off(max_grad_norm):
            max_grad_norm = None
        work = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            steps = set()
            keep = []
            for p in ps:
                require_device_tensor(p, "parameter")
                if not p.is_contiguous() or p.grad.is_sparse:
                    raise RuntimeError(f"{name} needs dense, contiguous parameters")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st[self._second] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = st["step"] + 1 if torch.is_tensor(st["step"]) else torch.tensor(float(st["step"]) + 1)
                steps.add(int(st["step"]))
                if max_grad_norm is not None:
                    require_device_tensor(p.grad, "gradient")
                keep.append(p.grad.contiguous())
            if len(steps) != 1:
                raise RuntimeError(f"{name}: parameters of one group must share their step count")
            # a tensor of 0 elements has no memory (a null pointer) and nothing to update: its state above is all torch gives it
            live = [(p, g) for p, g in zip(ps, keep) if p.numel() > 0]
            if live:
                work.append((group, [p for p, _ in live], [g for _, g in live], steps.pop()))
        coef = None
        if max_grad_norm is not None and work:
            out3, _ = _grad_norm([g for _, _, gs, _ in work for g in gs], max_grad_norm)
            self.last_grad_norm, coef, self.last_clipped_norm = out3[0], out3[1:2], out3[2]
        elif max_grad_norm is not None:   # nothing to clip: torch's clip_grad_norm_ returns tensor(0.) for no gradients
            self.last_grad_norm, self.last_clipped_norm = torch.tensor(0.0), torch.tensor(0.0)
        for group, ps, keep, step in work:
            (pa, ga, ma, va), numel, n = _tables(ps, keep, [self.state[p]["exp_avg"] for p in ps], [self.state[p][self._second] for p in ps])
            hyper = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                     float(group["weight_decay"]), step)
            if coef is None:
                _lib.check(getattr(lib, self._step_fn)(pa, ga, ma, va, numel, n, *hyper, _stream()))
            else:
                _lib.check(getattr(lib, self._clipped_fn)(pa, ga, ma, va, numel, n, *hyper, _ptr(coef), _stream()))
                for p, g in zip(ps, keep):
                    if g is not p.grad:   # the kernel scaled a contiguous copy
                        p.grad.copy_(g)
            for p in ps:   # the kernel wrote through raw pointers: tell autograd (and the packed-weight caches keyed on _version)
                torch.autograd.graph.increment_version(p)
        return loss


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam (amsgrad off) in one launch per 24 tensors (csrc/optim_step.hip); clipping, state and step: `_FusedOptimizer`."""

    _kind, _second, _step_fn, _clipped_fn = "Adam", "exp_avg_sq", "odehip_adam_step", "odehip_adam_step_clipped"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm)


class FusedAdamax(_FusedOptimizer):
    """torch.optim.Adamax in one launch per 24 tensors (csrc/optim_step.hip), with torch's defaults: Vid-ODE's optimizer
    (Vid-ODE/main.py:187).  State per parameter is torch's (`step`, `exp_avg`, `exp_inf`), so state dicts go both ways; `exp_inf` is
    torch's bit for bit, and a NaN gradient gives NaN there and in the parameter, never a finite update.  Clipping, `step(closure,
    max_grad_norm=)`, `last_grad_norm` / `last_clipped_norm`: `_FusedOptimizer`.  torch's `maximize`, `foreach`, `differentiable`
    and `capturable` are refused as arguments (TypeError), and a state dict that switches `maximize`, `differentiable` or `capturable`
    on does not load (ValueError): none of them is ignored."""

    _kind, _second, _step_fn, _clipped_fn = "Adamax", "exp_inf", "odehip_adamax_step", "odehip_adamax_step_clipped"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, **unsupported):
        if unsupported:
            raise TypeError(f"FusedAdamax takes no {sorted(unsupported)}: of torch.optim.Adamax's options it implements lr, betas, eps and "
                            "weight_decay (maximize, foreach, differentiable and capturable are refused, not ignored)")
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm)

    def __setstate__(self, state):
        for group in state.get("param_groups", ()):   # a torch.optim.Adamax state dict carries its options: the defaults load, others do not
            on = [k for k in ("maximize", "differentiable", "capturable") if group.get(k)]
            if on:
                raise ValueError(f"FusedAdamax: the state sets {on}, which this optimizer does not implement")
        super().__setstate__(state)


def decay_learning_rate(optimizer, decay_rate=0.999, lowest=1e-3):
    """Vid-ODE's learning-rate decay (Vid-ODE/utils.py:120 `update_learning_rate`, called once per epoch at main.py:214 with
    decay_rate=0.99, lowest=lr / 10): lr = max(lr * decay_rate, lowest) in every parameter group of any torch.optim.Optimizer.
    Host only -- the rate is an argument of each step's launch, so nothing is rebuilt.  Returns the new rates, one per group."""
    for group in optimizer.param_groups:
        group["lr"] = max(group["lr"] * decay_rate, lowest)
    return [group["lr"] for group in optimizer.param_groups]
