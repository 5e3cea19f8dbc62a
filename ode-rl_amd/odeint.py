"""`odeint(func, y0, t, rtol=, atol=, method=)` -- the call surface of torchdiffeq that the reference
consumes (/root/reference/modules/DiffEqSolver.py:37,45-46), executed by the HIP library.

Supported `func`: an `ODEFunc` (or any module exposing `gradient_net`, an nn.Sequential of stride-1
'same' Conv2d layers separated by ReLU or by Tanh, optionally followed by one Tanh head, as built by
`helpers.utils.create_convnet` with nonlinear='relu' / 'tanh' and final_act=False / True).  The dynamics are
autonomous (`ODEFunc.forward` ignores t: modules/DiffEqSolver.py:77), so `t` only sets step sizes.

Semantics follow torchdiffeq 0.2.1: solution[0] = y0, float64 time, 'rk4' = 3/8 rule with one step per
output interval -- or, with options={"grid_constructor": fn}, steps on the grid fn(func, y0, t) with the outputs interpolated
linearly --, strictly decreasing t integrates the negated dynamics on -t.  Under autograd a decreasing t raises NotImplementedError
until ode_rl_amd.set_reverse_time_grads(True); then every method differentiates that negated solve (fp32 mode), with or without an
internal grid, and `odeint_adjoint` takes a decreasing t for the fixed-grid methods without one (autograd.odeint_adjoint).
"""
import torch
import torch.nn as nn

from . import _lib, hip_ops

FIXED_GRID = ("euler", "midpoint", "rk4")
ADAPTIVE = ("dopri5", "bosh3")   # embedded FSAL pairs, one driver (csrc/dopri5_control.h holds their tableaus)
last_stats = hip_ops.LazyStats()  # nfe / n_accept / n_reject of the most recent dopri5 call (instrumentation; fills itself after an asynchronous solve)


def _host_times(t):
    return hip_ops.host_times(t)


def _check_monotone(t):
    if len(t) > 1:
        d = t[1:] - t[:-1]
        if not (bool((d > 0).all()) or bool((d < 0).all())):
            raise AssertionError("t must be strictly increasing or decreasing")


def conv_stack_of(func):
    """Find (and cache on the module) the packed conv stack behind an ODEFunc-like module."""
    cached = getattr(func, "_hip_stack", None)
    if cached is not None:
        return cached
    net = getattr(func, "gradient_net", None)
    if net is None and isinstance(func, nn.Sequential):
        net = func
    if not isinstance(net, nn.Sequential):
        raise TypeError("odeint(HIP): `func` must expose `gradient_net` (nn.Sequential of Conv2d/ReLU/Tanh as built by "
                        "create_convnet); arbitrary Python dynamics are not supported and there is no CPU fallback")
    # create_convnet: conv, act, conv, act, ..., conv [, Tanh]  with act all ReLU or all Tanh (helpers/utils.py, nonlinear=)
    mods = list(net)
    final_tanh = len(mods) > 1 and isinstance(mods[-1], nn.Tanh) and isinstance(mods[-2], nn.Conv2d)
    body = mods[:-1] if final_tanh else mods
    convs = [m for m in body if isinstance(m, nn.Conv2d)]
    acts = [m for m in body if not isinstance(m, nn.Conv2d)]
    for m in acts:
        if type(m) not in (nn.ReLU, nn.Tanh):
            raise TypeError(f"odeint(HIP): unsupported layer {m} in gradient_net (Conv2d separated by ReLU or Tanh, "
                            "optionally followed by one Tanh)")
    if len({type(m) for m in acts}) > 1:
        raise TypeError("odeint(HIP): the hidden activations of gradient_net must be all ReLU or all Tanh")
    if not convs or not isinstance(body[0], nn.Conv2d) or not isinstance(body[-1], nn.Conv2d) or any(
            isinstance(m, nn.Conv2d) == isinstance(n, nn.Conv2d) for m, n in zip(body, body[1:])):
        raise TypeError("odeint(HIP): every hidden Conv2d must be followed by exactly one activation (ReLU or Tanh)")
    act = _lib.ACT_TANH if acts and isinstance(acts[0], nn.Tanh) else _lib.ACT_RELU
    stack = hip_ops.PackedConvStack(convs, final_tanh, act)
    try:
        object.__setattr__(func, "_hip_stack", stack)
    except Exception:
        pass
    return stack


def check_options(method, options, where="odeint"):
    """torchdiffeq's `options` that this path implements.  Fixed-grid methods, in `odeint` and -- once
    set_adjoint_grids(True) has switched them on; refused as before otherwise -- in `odeint_adjoint`: `grid_constructor` (an internal grid of the caller's; the requested times are filled by linear interpolation) and `interp:
    "linear"` next to it; `step_size` stays refused -- `step_size_grid(step_size)` builds torchdiffeq's grid for it --, as do `perturb`
    and any other `interp`: they would change the result and are refused rather than ignored.  dopri5 and bosh3: `first_step` and
    `max_num_steps`.  Looks at no tensor."""
    options = options or {}
    if method in FIXED_GRID:
        known = {"grid_constructor", "interp"} if where == "odeint" or hip_ops.adjoint_grids_enabled() else set()
    else:
        known = {"first_step", "max_num_steps"}
    unknown = set(options) - known
    if unknown:
        hint = ""
        if method in FIXED_GRID and not known and unknown & {"step_size", "grid_constructor", "interp"}:
            hint = (": internal grids under odeint_adjoint are opt-in -- torchdiffeq's adjoint builds a new grid for every backward "
                    "interval, anchored at its later time, and so does this path after ode_rl_amd.set_adjoint_grids(True)")
        elif "step_size" in unknown and method in FIXED_GRID:
            hint = ': for a step size pass options={"grid_constructor": ode_rl_amd.step_size_grid(step_size)}'
        raise ValueError(f"{where}(HIP): unsupported {method} options {sorted(unknown)}{hint}")
    if method in FIXED_GRID:
        if "grid_constructor" in options and not callable(options["grid_constructor"]):
            raise TypeError(f"{where}(HIP): options['grid_constructor'] must be callable as grid_constructor(func, y0, t), got "
                            f"{type(options['grid_constructor']).__name__}")
        if options.get("interp", "linear") != "linear":
            raise ValueError(f"{where}(HIP): unsupported interp {options['interp']!r}: only \"linear\" is implemented")


def step_size_grid(step_size):
    """The grid constructor of torchdiffeq's `options={"step_size": h}` (_grid_constructor_from_step_size), for
    `options={"grid_constructor": step_size_grid(h)}`: steps of h from t[0], the last one cut short at t[-1]; float64."""
    step_size = float(step_size)
    if not step_size > 0:
        raise ValueError(f"step_size_grid: step_size must be positive, got {step_size!r}")

    def grid_constructor(func, y0, t):
        t = torch.as_tensor(t).detach().to("cpu", torch.float64)
        niters = torch.ceil((t[-1] - t[0]) / step_size + 1).item()
        grid = torch.arange(0, niters, dtype=torch.float64) * step_size + t[0]
        grid[-1] = t[-1]
        return grid
    return grid_constructor


def internal_grid(func, y0, th, options):
    """The float64 host grid the fixed-grid solver steps through, from options["grid_constructor"](func, y0, t) with the (already
    increasing) host times `th`, checked as torchdiffeq asserts; None without a constructor."""
    ctor = (options or {}).get("grid_constructor")
    if ctor is None:
        return None
    grid = hip_ops.host_times(ctor(func, y0, th))
    if len(grid) < 1 or not bool(grid[0] == th[0]) or not bool(grid[-1] == th[-1]):
        raise AssertionError("the grid of grid_constructor must start at t[0] and end at t[-1]")
    if len(grid) > 1 and not bool((grid[1:] > grid[:-1]).all()):
        raise AssertionError("the grid of grid_constructor must be strictly increasing")
    return grid


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None):
    if method is None:
        method = "dopri5"
    if method not in FIXED_GRID + ADAPTIVE:
        raise ValueError('Invalid method "{}". Must be one of euler, midpoint, rk4, dopri5, bosh3'.format(method))
    check_options(method, options)
    hip_ops.require_device_tensor(y0, "y0")
    if torch.is_grad_enabled() and (y0.requires_grad or any(p.requires_grad for p in func.parameters())):
        from .autograd import odeint_with_grad
        return odeint_with_grad(func, y0, t, rtol, atol, method, options)
    return odeint_forward(func, y0, t, rtol, atol, method, options)


def odeint_forward(func, y0, t, rtol, atol, method, options=None):
    th = _host_times(t)
    _check_monotone(th)
    negate = False
    if len(th) > 1 and bool(th[0] > th[1]):  # torchdiffeq: strictly decreasing t => integrate -f on -t
        th = -th
        negate = True
    stack = conv_stack_of(func)
    if method in FIXED_GRID:
        check_options(method, options)
        grid = internal_grid(func, y0, th, options)   # of -t for a decreasing t: torchdiffeq flips time before it builds the solver
        if grid is not None:
            return hip_ops.odeint_fixed_on_grid(stack, method, y0, th, grid, negate=negate)
        return hip_ops.odeint_fixed(stack, method, y0, th, negate=negate)
    check_options(method, options)
    return run_dopri5(stack, y0, th, dopri5_cfg(rtol, atol, options, method), negate=negate)[0]


def dopri5_cfg(rtol, atol, options, method="dopri5"):
    """Tolerances, the adaptive method and the `options` this path implements for it, as run_dopri5 and the autograd Functions take
    them."""
    options = options or {}
    return dict(rtol=float(rtol), atol=float(atol), first_step=float(options.get("first_step") or 0.0),
                max_num_steps=int(options.get("max_num_steps") or 0), method=method)


def run_dopri5(stack, y0, th, cfg, save=False, negate=False):
    """One adaptive forward (cfg["method"]: dopri5 or bosh3) -> (out, pending, stats, saved).  With hip_ops.set_async_dopri5 on (and not for the negated dynamics) the
    solve is only enqueued: `pending` is its PendingDopri5, bound to last_stats -- the stats are read when somebody looks at them --
    and stats / saved are None.  Otherwise pending is None and last_stats holds the stats.  save: keep the activations of the accepted
    steps for the backward pass (hip_ops.odeint_dopri5_saving); `saved` is then what odeint_dopri5_backward_saved takes, or None."""
    steps = dict(first_step=cfg["first_step"], max_steps=cfg["max_num_steps"], method=cfg.get("method", "dopri5"))
    saved = None
    if save:   # (a negated solve never starts asynchronously: odeint_dopri5_saving)
        out, stats, saved = hip_ops.odeint_dopri5_saving(stack, y0, th, cfg["rtol"], cfg["atol"], negate=negate, **steps)
    elif hip_ops._async_dopri5 and not negate:
        out, stats = hip_ops.odeint_dopri5_start(stack, y0, th, cfg["rtol"], cfg["atol"], **steps)
    else:
        out, stats = hip_ops.odeint_dopri5(stack, y0, th, cfg["rtol"], cfg["atol"], negate=negate, **steps)
    if isinstance(stats, hip_ops.PendingDopri5):
        last_stats._bind(stats)
        return out, stats, None, None
    last_stats.clear()
    last_stats.update(stats)
    return out, None, stats, saved
