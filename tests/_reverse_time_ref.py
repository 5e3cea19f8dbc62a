"""Reference for gradients through solves on a strictly decreasing t (tests/test_reverse_time_cpu.py, tests/test_hip_reverse_time.py).

torchdiffeq solves a decreasing t as the negated dynamics on -t.  The reference says exactly that, from outside: autograd through
the oracle's solvers on `lambda s, y: -f(-s, y)` over `-t` -- oracle/torchdiffeq_ref.py for euler / midpoint / rk4, its restatement
for the adaptive tableaus (tests/_adaptive_ref.py, which also runs in float32 and reports the step counts) for dopri5 and bosh3, and
the restated `integrate` loop (tests/_grid_ref.py) on the grid of -t for an internal grid.  None of them is handed a decreasing t, so
the sign conventions under test are not the reference's own."""
import torch
import torch.nn.functional as F

import _adaptive_ref
import _grid_ref
from oracle import torchdiffeq_ref

FIXED = ("euler", "midpoint", "rk4")


def negated(f):
    return lambda s, y: -f(-s, y)


def dynamics_of(func, params):
    """The dynamics of an ODEFunc-like module as a closure on `params` = [w0, w1, ..., b0, b1, ...] (any dtype)."""
    net = list(func.gradient_net)
    head = isinstance(net[-1], torch.nn.Tanh)
    body = net[:-1] if head else net
    n = sum(isinstance(m, torch.nn.Conv2d) for m in body)
    act = torch.tanh if any(isinstance(m, torch.nn.Tanh) for m in body) else torch.relu
    ws, bs = params[:n], params[n:]

    def fn(t, y):
        x = y
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
            if i < n - 1:
                x = act(x)
        return torch.tanh(x) if head else x
    return fn


def leaf_params(func, dtype):
    convs = [m for m in func.gradient_net if isinstance(m, torch.nn.Conv2d)]
    return [c.weight.detach().cpu().to(dtype).requires_grad_(True) for c in convs] + \
           [c.bias.detach().cpu().to(dtype).requires_grad_(True) for c in convs]


def solve(f, y0, t, method, step_size=None, stats=None, rtol=1e-7, atol=1e-9, first_step=None):
    """The solution at the strictly decreasing float64 times t: the negated dynamics on -t."""
    t = torch.as_tensor(t, dtype=torch.float64)
    assert len(t) > 1 and bool((t[1:] < t[:-1]).all()), "the reference is for strictly decreasing t"
    g, s = negated(f), -t
    if method in FIXED:
        if step_size is not None:
            return _grid_ref.integrate_on_grid(g, y0, s, _grid_ref.step_size_grid_ref(s, step_size), method)
        return torchdiffeq_ref.odeint(g, y0, s, method=method)
    options = None if first_step is None else {"first_step": first_step}
    return _adaptive_ref.odeint(g, y0, s, rtol=rtol, atol=atol, method=method, options=options, stats=stats)


def solve_with_grads(make_f, params, y0, t, gout, method, **kw):
    """(solution, [grad y0] + grads of params) with the loss sum(solution * gout); make_f(params) -> f(t, y)."""
    y = y0.detach().clone().requires_grad_(True)
    sol = solve(make_f(params), y, t, method, **kw)
    grads = torch.autograd.grad(sol, [y] + list(params), gout.to(sol.dtype))
    return sol.detach(), [g.detach() for g in grads]


def module_reference(func, y0, t, gout, method, dtype=torch.float64, **kw):
    """solve_with_grads for an ODEFunc-like module: gradients ordered [y0, w0.., b0..], in `dtype` on the CPU."""
    params = leaf_params(func, dtype)
    return solve_with_grads(lambda p: dynamics_of(func, p), params, y0.detach().cpu().to(dtype), t, gout.detach().cpu(), method, **kw)
