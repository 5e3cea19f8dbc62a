"""odeint_adjoint on internal grids (options={"grid_constructor": fn}) on the GPU, against the float64 restatement of torchdiffeq's
adjoint with options (tests/_grid_adjoint_ref.py): every backward interval is stepped through the grid its flipped end points build,
y is carried through the interior points and reset, with grad_out added, at the output times only.

Cases: B = 2, t = (0, 0.25, 0.7) -- two intervals that step_size_grid(0.2) cuts into 2 and 3 unequal sub-steps, anchored at the later
time -- and one constructor with unequal sub-steps of its own.  Stacks: 64-channel ReLU (the trajectory walks), 64-192-192-64 ReLU
(_solver_stack_cases B1's shape: per-layer Winograd and direct kernels, the shared epilogue), 64-channel Tanh with a Tanh head.
Tolerance: rel-L2 <= 1e-4 per gradient tensor, the bound tests/test_hip_backward.py holds the one-step adjoint to against the oracle
(_solver_stack_cases.GRAD_FLOOR)."""
import pytest
import torch

import _grid_adjoint_ref as gar
import _solver_stack_cases as sc
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

T3 = torch.tensor([0.0, 0.25, 0.7], dtype=torch.float64)


@pytest.fixture(autouse=True)
def _adjoint_grids_on():
    """odeint_adjoint takes internal grids only after set_adjoint_grids(True); the tests leave the switch as they found it."""
    import ode_rl_amd
    was = ode_rl_amd.set_adjoint_grids(True)
    yield
    ode_rl_amd.set_adjoint_grids(was)


CASES = gar.CASES
_spec, _grid, _reference = gar.case_spec, gar.case_grid, gar.case_reference


def _device_run(dev, spec, method, options, f=None):
    """(sol, gradients by name) of odeint_adjoint(..., options=options) and its backward pass."""
    import ode_rl_amd
    f = f if f is not None else sc.device_func(dev, spec)
    f.zero_grad()
    z = spec["z0"].to(dev).requires_grad_(True)
    sol = ode_rl_amd.odeint_adjoint(f, z, T3, method=method, **({"options": options} if options is not None else {}))
    sol.backward(spec["gout"].to(dev))
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    out = {"z0": z.grad.clone()}
    out.update({f"w{i}": c.weight.grad.clone() for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad.clone() for i, c in enumerate(convs)})
    return sol.detach(), out


@pytest.mark.parametrize("stack,method,grid,batch", CASES, ids=[f"{s}.{m}.{g}.B{b}" for s, m, g, b in CASES])
def test_gradients_match_the_restatement(cuda, stack, method, grid, batch):
    import ode_rl_amd
    spec = _spec(stack, batch)
    ref = _reference(stack, method, grid, batch)
    options = {"grid_constructor": _grid(grid)}
    f = sc.device_func(cuda, spec)
    sol, got = _device_run(cuda, spec, method, options, f)
    with torch.no_grad():
        plain = ode_rl_amd.odeint(f, spec["z0"].to(cuda), T3, method=method, options=options)
    assert torch.equal(sol, plain)                                       # the forward IS odeint's gridded solve
    inc = record(f"grid_adjoint.{stack}.{method}.{grid}.B{batch}.sol", rel_l2(sol, ref["sol"]))
    assert inc <= 1e-4, inc                                              # the solution bound of the gridded odeint (test_hip_grid_options.py)
    assert sorted(got) == sorted(k for k in ref if k != "sol")
    errs = {k: record(f"grid_adjoint.{stack}.{method}.{grid}.B{batch}.{k}", rel_l2(got[k], ref[k])) for k in got}
    print(f"grid adjoint {stack} {method} {grid} B={batch}: solution {inc:.3e},gradients {errs}")
    for k, e in errs.items():
        assert e <= sc.GRAD_FLOOR, (k, e)


def test_degenerate_grids_are_the_one_step_adjoint_bit_for_bit(cuda):
    """A constructor that returns t itself: forward and backward are the calls without options.  A step size no smaller than any
    interval: every backward grid is its two end points, so on the same trajectory the backward is the one-step adjoint's (the
    FORWARD grid of such a step size skips t[1], so the trajectories of the public calls differ and are not compared)."""
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    from ode_rl_amd.odeint import conv_stack_of
    spec = _spec("walk", 2)
    f = sc.device_func(cuda, spec)
    for method in ("euler", "midpoint", "rk4"):
        sol0, g0 = _device_run(cuda, spec, method, None, f)
        sol1, g1 = _device_run(cuda, spec, method, {"grid_constructor": lambda func, y0, t: t}, f)
        assert torch.equal(sol0, sol1) and all(torch.equal(g0[k], g1[k]) for k in g0)
        gout = spec["gout"].to(cuda)
        a = hip_ops.odeint_adjoint_backward(conv_stack_of(f), method, T3, sol0, gout)
        a = [a[0].clone()] + [g.clone() for g in a[1]] + [g.clone() for g in a[2]]
        for h in (0.45, 1.0):
            b = hip_ops.odeint_adjoint_on_grid_backward(conv_stack_of(f), method, T3, sol0, gout, f, {"grid_constructor": ode_rl_amd.step_size_grid(h)})
            assert all(torch.equal(x, y) for x, y in zip(a, [b[0]] + list(b[1]) + list(b[2])))


def test_the_new_entry_on_a_grid_without_interior_points_is_the_old_entry(cuda):
    """The C entry itself, handed the output times as its grid: the same sweep, the trajectory behind the layout instead of inside it."""
    import ctypes
    from ode_rl_amd import _lib, hip_ops
    from ode_rl_amd.odeint import conv_stack_of
    spec = _spec("walk", 2)
    f = sc.device_func(cuda, spec)
    stack = conv_stack_of(f)
    with torch.no_grad():
        import ode_rl_amd
        sol = ode_rl_amd.odeint(f, spec["z0"].to(cuda), T3, method="rk4")
    gout = spec["gout"].to(cuda)
    want = hip_ops.odeint_adjoint_backward(stack, "rk4", T3, sol, gout)
    want = [want[0].clone()] + [g.clone() for g in want[1]] + [g.clone() for g in want[2]]
    desc, dg, lib = stack.refresh(), stack.dgrad_desc(), _lib.load()
    tarr = hip_ops._c_times(T3)
    nbytes = lib.odehip_odeint_adjoint_grid_workspace_bytes(ctypes.byref(desc), 2, 3, 3, 2)
    ws = hip_ops.alloc_workspace(nbytes, cuda)
    grads, gw_arr, gb_arr = hip_ops._stack_grads(stack, 2, cuda)
    _lib.check(lib.odehip_odeint_adjoint_backward_on_grid(ctypes.byref(desc), ctypes.byref(dg), 2, tarr, 3, tarr, 3, (ctypes.c_int * 3)(0, 1, 2), 2,
                                                          hip_ops._ptr(sol), hip_ops._ptr(gout), hip_ops._ptr(grads[0]), gw_arr, gb_arr,
                                                          hip_ops._ptr(ws), ws.numel(), hip_ops._stream()))
    assert all(torch.equal(x, y) for x, y in zip(want, [grads[0]] + list(grads[1]) + list(grads[2])))


def test_grid_constructor_calls_limits_and_bf16(cuda):
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    spec = _spec("walk", 2)
    f = sc.device_func(cuda, spec)
    calls = []

    def recording(func, y0, t):
        calls.append(t.tolist())
        return ode_rl_amd.step_size_grid(0.2)(func, y0, t)
    z = spec["z0"].to(cuda).requires_grad_(True)
    sol = ode_rl_amd.odeint_adjoint(f, z, T3, method="rk4", options={"grid_constructor": recording})
    assert calls == [[0.0, 0.25, 0.7]]                                   # the forward solve's grid
    sol.backward(spec["gout"].to(cuda))
    assert calls[1:] == [[-0.7, -0.25], [-0.25, -0.0]]                   # T - 1 backward intervals, i = T-1 .. 1, flipped
    assert hip_ops.last_adjoint_grid["points"] == 6

    # 700 sub-steps: the forward (nothing kept) runs, rk4's backward would need 2800 evaluations -- refused before any launch, and
    # the next valid call computes what it computed before
    fine = {"grid_constructor": ode_rl_amd.step_size_grid(0.001)}
    sol0, g0 = _device_run(cuda, spec, "rk4", {"grid_constructor": ode_rl_amd.step_size_grid(0.2)}, f)
    z = spec["z0"].to(cuda).requires_grad_(True)
    sol = ode_rl_amd.odeint_adjoint(f, z, T3, method="rk4", options=fine)
    with pytest.raises(ValueError, match=r"2800 evaluations.*at most 2048"):
        sol.backward(spec["gout"].to(cuda))
    sol1, g1 = _device_run(cuda, spec, "rk4", {"grid_constructor": ode_rl_amd.step_size_grid(0.2)}, f)
    assert torch.equal(sol0, sol1) and all(torch.equal(g0[k], g1[k]) for k in g0)

    hip_ops.set_compute_dtype("bf16")
    try:
        with pytest.raises(TypeError, match="bf16"):
            ode_rl_amd.odeint_adjoint(f, z, T3, method="rk4", options={"grid_constructor": ode_rl_amd.step_size_grid(0.2)})
    finally:
        hip_ops.set_compute_dtype(None)

    ode_rl_amd.set_adjoint_grids(False)                                  # switched off: the refusal of old, before any launch
    try:
        with pytest.raises(ValueError, match="grid_constructor.*set_adjoint_grids"):
            ode_rl_amd.odeint_adjoint(f, z, T3, method="rk4", options={"grid_constructor": ode_rl_amd.step_size_grid(0.2)})
    finally:
        ode_rl_amd.set_adjoint_grids(True)
