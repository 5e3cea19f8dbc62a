"""Gradients through solves on a strictly decreasing t on the GPU (ode_rl_amd.set_reverse_time_grads).

References and bounds -- none of them invented here:
  parity   float64 autograd through the oracle on `lambda s, y: -f(-s, y)` over -t (tests/_reverse_time_ref.py).  Fixed grid: every
           tensor <= 1e-4 rel-L2, the bound of the increasing-grid tests (tests/test_hip_grid_options.py, DESIGN row a7).  Adaptive:
           max(4 * d32, 1e-4) with d32 the float32 restatement's own distance to float64 on the same case, and the restatement's
           (nfe, n_accept, n_reject); first_step as tests/_bosh3_cases.py, so that no gradient runs through the step heuristic.
  mirror   g = f with the last conv's weight and bias negated (tanh is odd, so this holds under a Tanh head too): odeint(f, z0, t) on
           the decreasing t and odeint(g, z0, -t) are the same solve.  Solutions within 4 * 2^-24 of the largest magnitude, gradients
           <= 1e-6 rel-L2 (the last layer's negated), equal step counts.  Needs no oracle.
  adjoint  euler / midpoint / rk4 against the oracle's float64 adjoint on the negated dynamics: <= 1e-4, the bound
           tests/test_hip_adjoint_paths.py holds the increasing case to; and the mirror identity at 1e-6.
           The adjoint against odeint + backward() on the same grid differs by the method's truncation error: midpoint and rk4 are
           held to 1e-4 on the kink-free dynamics, euler -- of order one there on these steps -- must close the gap at first order
           when the grid is refined (the gap is C h + O(h^2), so halving h gives a ratio of 1/2 + O(h): 0.4 .. 0.6 asserted).
Weights: the solutions of the vigorous 64-channel weights and of the V stack of tests/test_hip_grid_options.py (the methods differ on
them) against the reference for every method; solutions AND gradients on the Tanh-head stack (smooth) and on the kink-free ReLU
dynamics of tests/_grid_ref.py -- on other ReLU weights a mask element may flip between two correct implementations, which is why every
gradient test held to 1e-4 here is kink-free (tests/test_hip_backward.py); the vigorous weights' gradients are held to the float32
restatement's own distance in the rejecting adaptive case, and to the mirror identity for every method."""
import copy
import functools

import pytest
import torch

import _grid_ref
import _reverse_time_ref as rt
from conftest import record, rel_l2
from test_hip_grid_options import _v_stack, _vigorous_f, _z0

pytestmark = pytest.mark.gpu

T4 = (0.9, 0.6, 0.55, 0.1)
T2 = (0.3, 0.0)
TOL = dict(rtol=1e-3, atol=1e-4)   # tests/_bosh3_cases.py
FIRST_STEP = 0.02
CASES = [("euler", None), ("midpoint", None), ("rk4", None), ("rk4", 0.11), ("dopri5", None), ("bosh3", None)]


@pytest.fixture(autouse=True)
def _switch_on():
    import ode_rl_amd
    was = ode_rl_amd.set_reverse_time_grads(True)
    yield
    ode_rl_amd.set_reverse_time_grads(was)


def _t(times):
    return torch.tensor(times, dtype=torch.float64)


def _kink_free():
    return _grid_ref.kink_free()[0]


def _tanh_head(channels=64):
    import ode_rl_amd
    torch.manual_seed(6)
    f = ode_rl_amd.ODEFunc(n_inputs=channels, n_outputs=channels, n_layers=3, n_units=channels, downsize=False, nonlinear="tanh", final_act=True)
    with torch.no_grad():
        for p in f.parameters():
            p.mul_(2.0)
    return f


STACKS = {"A": lambda: _vigorous_f()[0], "V": lambda: _v_stack()[0], "tanh": _tanh_head, "kf": _kink_free}


def _channels(f):
    return [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)][0].in_channels


def _kwargs(method, step):
    import ode_rl_amd
    if step is not None:
        return {"method": method, "options": {"grid_constructor": ode_rl_amd.step_size_grid(step)}}
    if method in ("dopri5", "bosh3"):
        return dict(method=method, options={"first_step": FIRST_STEP}, **TOL)
    return {"method": method}


def _gout(n_times, batch, channels, seed=8):
    return torch.randn(n_times, batch, channels, 16, 16, generator=torch.Generator().manual_seed(seed))


def _run(f, z0, t, gout, cuda, adjoint=False, **kw):
    """(solution, [grad z0, grad w.., grad b..], stats of an adaptive forward) on the device."""
    import ode_rl_amd
    f.zero_grad()
    zd = z0.to(cuda).requires_grad_(True)
    sol = (ode_rl_amd.odeint_adjoint if adjoint else ode_rl_amd.odeint)(f, zd, t, **kw)
    st = dict(ode_rl_amd.last_stats) if kw.get("method") in ("dopri5", "bosh3") else {}
    sol.backward(gout.to(cuda))
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    grads = [zd.grad] + [c.weight.grad for c in convs] + [c.bias.grad for c in convs]
    return sol.detach(), [g.detach().clone() for g in grads], (st.get("nfe"), st.get("n_accept"), st.get("n_reject"))


def _mirror(f):
    stack = f.__dict__.pop("_hip_stack", None)   # the packed images cached on a module that has run (ctypes: not copyable)
    try:
        g = copy.deepcopy(f)
    finally:
        if stack is not None:
            object.__setattr__(f, "_hip_stack", stack)
    last = [m for m in g.gradient_net if isinstance(m, torch.nn.Conv2d)][-1]
    with torch.no_grad():
        last.weight.neg_()
        last.bias.neg_()
    return g


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def _reference(stack, batch, times, method, step, dtype):
    f = STACKS[stack]()
    c = _channels(f)
    stats = {}
    kw = {"step_size": step} if step is not None else {}
    if method in ("dopri5", "bosh3"):
        kw = dict(stats=stats, first_step=FIRST_STEP, **TOL)
    sol, grads = rt.module_reference(f, _z0(batch, c, seed=7), _t(times), _gout(len(times), batch, c), method, dtype=dtype, **kw)
    return sol, grads, (stats.get("nfe"), stats.get("n_accept"), stats.get("n_reject"))


@pytest.mark.parametrize("method,step", CASES)
@pytest.mark.parametrize("stack,batch,times", [("kf", 3, T4), ("kf", 17, T2), ("tanh", 3, T4), ("tanh", 17, T2), ("A", 3, T4), ("A", 17, T2),
                                               ("V", 2, T4)])
def test_solution_and_gradients_match_float64_autograd_on_the_negated_dynamics(cuda, stack, batch, times, method, step):
    """kf and tanh: the solution and every gradient tensor.  A and V (ReLU weights with kinks): the solution of the same call."""
    with_grads = stack in ("kf", "tanh")
    f = STACKS[stack]().to(cuda)
    c = _channels(f)
    sol, got, counts = _run(f, _z0(batch, c, seed=7), _t(times), _gout(len(times), batch, c), cuda, **_kwargs(method, step))
    ref_sol, ref_g, ref_counts = _reference(stack, batch, times, method, step, torch.float64)
    assert torch.equal(sol[0].cpu(), _z0(batch, c, seed=7))
    name = f"reverse.{stack}.B{batch}.T{len(times)}.{method}{'' if step is None else '.grid'}"
    errs = [record(f"{name}.sol", rel_l2(sol, ref_sol))]
    if with_grads:
        errs += [record(f"{name}.g{i}", rel_l2(a, b)) for i, (a, b) in enumerate(zip(got, ref_g))]
    assert len(got) == len(ref_g) and all(float(g.abs().max()) > 0 for g in got)
    bound = 1e-4
    if method in ("dopri5", "bosh3"):
        s32, g32, counts32 = _reference(stack, batch, times, method, step, torch.float32)
        d32 = max([rel_l2(s32, ref_sol)] + ([rel_l2(a, b) for a, b in zip(g32, ref_g)] if with_grads else []))
        bound = max(4 * record(f"{name}.d32", d32), 1e-4)
        assert counts == counts32, (counts, counts32, ref_counts)
    assert max(errs) <= bound, (errs, bound)


@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_an_adaptive_solve_that_rejects_steps_matches_the_restatement(cuda, method):
    """The vigorous weights with a first step of the whole span, 0.8: the controller rejects twice (float32 and float64 restatement
    alike) before it accepts; the device must accept and reject the same attempts.  Bounds from the float32 restatement's distance."""
    import ode_rl_amd
    f, _ = _vigorous_f()
    z0, gout, t = _z0(3, seed=7), _gout(4, 3, 64), _t(T4)
    kw = dict(method=method, options={"first_step": 0.8}, **TOL)
    sol, got, counts = _run(f.to(cuda), z0, t, gout, cuda, **kw)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        stats = {}
        s, g = rt.module_reference(f, z0, t, gout, method, dtype=dtype, stats=stats, first_step=0.8, **TOL)
        ref[dtype] = (s, g, (stats["nfe"], stats["n_accept"], stats["n_reject"]))
    assert counts[2] >= 1 and ref[torch.float64][2][2] >= 1, (counts, ref[torch.float64][2])
    assert counts == ref[torch.float32][2] == ref[torch.float64][2]
    d32 = record(f"reverse.reject.{method}.d32.sol", rel_l2(ref[torch.float32][0], ref[torch.float64][0]))
    assert record(f"reverse.reject.{method}.sol", rel_l2(sol, ref[torch.float64][0])) <= max(4 * d32, 1e-4)
    for i, (a, b32, b64) in enumerate(zip(got, ref[torch.float32][1], ref[torch.float64][1])):
        d = record(f"reverse.reject.{method}.d32.g{i}", rel_l2(b32, b64))
        assert record(f"reverse.reject.{method}.g{i}", rel_l2(a, b64)) <= max(4 * d, 1e-4), i


# ---------------------------------------------------------------------------------------------------------------- 2. mirror
@pytest.mark.parametrize("method,step", CASES)
@pytest.mark.parametrize("stack,batch,times", [("A", 3, T4), ("A", 17, T2), ("V", 2, T4), ("tanh", 3, T4), ("tanh", 17, T2)])
def test_a_decreasing_solve_is_the_increasing_solve_of_the_mirrored_dynamics(cuda, stack, batch, times, method, step):
    f = STACKS[stack]().to(cuda)
    g = _mirror(f)
    c = _channels(f)
    z0, gout, t = _z0(batch, c, seed=7), _gout(len(times), batch, c), _t(times)
    kw = _kwargs(method, step)
    if method in ("dopri5", "bosh3"):
        kw = dict(method=method, **TOL)   # the heuristic's first step too: it sees the same slopes on both sides
    sol_f, gf, counts_f = _run(f, z0, t, gout, cuda, **kw)
    sol_g, gg, counts_g = _run(g, z0, -t, gout, cuda, **kw)
    name = f"mirror.{stack}.B{batch}.T{len(times)}.{method}{'' if step is None else '.grid'}"
    assert counts_f == counts_g
    assert float((sol_f - sol_g).abs().max()) <= 4 * 2.0 ** -24 * float(sol_g.abs().max())
    n_conv = (len(gf) - 1) // 2
    flipped = {n_conv, 2 * n_conv}   # the last conv's weight and bias
    bitwise = torch.equal(sol_f, sol_g)
    errs = []
    for i, (a, b) in enumerate(zip(gf, gg)):
        b = -b if i in flipped else b
        bitwise = bitwise and torch.equal(a, b)
        errs.append(rel_l2(a, b))
    record(f"{name}.bitwise", float(bitwise))
    assert record(f"{name}.worst", max(errs)) <= 1e-6, errs
    assert all(float(x.abs().max()) > 0 for x in gf)


# ---------------------------------------------------------------------------------------------------------------- 3. adjoint
@functools.lru_cache(maxsize=None)
def _adjoint_reference(stack, method, batch, times):
    from oracle import torchdiffeq_ref
    f = STACKS[stack]()
    params = rt.leaf_params(f, torch.float64)
    t = _t(times)
    _, gz, gp = torchdiffeq_ref.odeint_adjoint(rt.negated(rt.dynamics_of(f, params)), _z0(batch, 64, seed=7).double(), -t, params,
                                              _gout(len(times), batch, 64).double(), method=method)
    return [gz.detach()] + [g.detach() for g in gp]


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("stack,batch,times", [("kf", 3, T4), ("kf", 17, T2), ("tanh", 3, T4), ("tanh", 17, T2)])
def test_the_adjoint_on_a_decreasing_grid(cuda, stack, method, batch, times):
    f = STACKS[stack]().to(cuda)
    z0, gout, t = _z0(batch, 64, seed=7), _gout(len(times), batch, 64), _t(times)
    sol, got, _ = _run(f, z0, t, gout, cuda, adjoint=True, method=method)
    ref = _adjoint_reference(stack, method, batch, times)
    name = f"reverse.adjoint.{stack}.B{batch}.T{len(times)}.{method}"
    errs = [record(f"{name}.g{i}", rel_l2(a, b)) for i, (a, b) in enumerate(zip(got, ref))]
    assert len(errs) == len(ref) == len(got) and max(errs) <= 1e-4, errs
    # the forward is odeint's own negated solve
    plain_sol, plain_g, _ = _run(f, z0, t, gout, cuda, method=method)
    assert torch.equal(sol, plain_sol)
    # against odeint + backward(): apart by the method's truncation error (module docstring); the Tanh stack's is recorded
    gap = record(f"{name}.vs_autograd", max(rel_l2(a, b) for a, b in zip(got, plain_g)))
    if stack == "kf" and method in ("midpoint", "rk4"):
        assert gap <= 1e-4
    # ... and the mirrored dynamics on -t give the same adjoint gradients
    _, mirrored, _ = _run(_mirror(f), z0, -t, gout, cuda, adjoint=True, method=method)
    n_conv = (len(got) - 1) // 2
    worst = max(rel_l2(a, -b if i in (n_conv, 2 * n_conv) else b) for i, (a, b) in enumerate(zip(got, mirrored)))
    assert record(f"{name}.mirror", worst) <= 1e-6


def test_the_euler_adjoint_closes_on_autograd_at_first_order(cuda):
    """Continuous adjoint and discrete backward of euler differ by C h + O(h^2): on [0.3, 0] in 16 and in 32 equal steps, the loss on
    the last frame alone, the gap halves up to O(h)."""
    f = _kink_free().to(cuda)
    z0 = _z0(3, 64, seed=7)
    gaps = []
    for n in (16, 32):
        t = torch.linspace(0.3, 0.0, n + 1, dtype=torch.float64)
        gout = torch.zeros(n + 1, 3, 64, 16, 16)
        gout[-1] = _gout(1, 3, 64)[0]
        _, adj, _ = _run(f, z0, t, gout, cuda, adjoint=True, method="euler")
        _, bwd, _ = _run(f, z0, t, gout, cuda, method="euler")
        gaps.append(record(f"reverse.adjoint.euler.refine.N{n}", max(rel_l2(a, b) for a, b in zip(adj, bwd))))
    assert gaps[0] > 1e-4 and 0.4 <= record("reverse.adjoint.euler.refine.ratio", gaps[1] / gaps[0]) <= 0.6, gaps


# ---------------------------------------------------------------------------------------------------------------- 4. determinism, isolation
@pytest.mark.parametrize("method,step", [("rk4", None), ("rk4", 0.11), ("dopri5", None)])
def test_two_runs_are_bitwise_equal(cuda, method, step):
    f, _ = _vigorous_f()
    f = f.to(cuda)
    z0, gout = _z0(3, seed=7), _gout(4, 3, 64)
    a = _run(f, z0, _t(T4), gout, cuda, **_kwargs(method, step))
    b = _run(f, z0, _t(T4), gout, cuda, **_kwargs(method, step))
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]


def test_the_switch_leaves_increasing_grids_alone_and_the_walks_count_alike(cuda):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f, _ = _vigorous_f()
    f = f.to(cuda)
    z0, gout, up = _z0(3, seed=7), _gout(4, 3, 64), _t(tuple(-x for x in T4))
    ode_rl_amd.set_reverse_time_grads(False)
    before = _run(f, z0, up, gout, cuda, method="rk4")
    n0 = lib.odehip_persistent_trajectory_launches()
    _run(f, z0, up, gout, cuda, method="rk4")
    per_step_up = lib.odehip_persistent_trajectory_launches() - n0
    ode_rl_amd.set_reverse_time_grads(True)
    n0 = lib.odehip_persistent_trajectory_launches()
    _run(f, z0, _t(T4), gout, cuda, method="rk4")
    per_step_down = lib.odehip_persistent_trajectory_launches() - n0
    assert per_step_down == per_step_up and per_step_up >= 1
    ode_rl_amd.set_reverse_time_grads(False)
    after = _run(f, z0, up, gout, cuda, method="rk4")
    assert torch.equal(before[0], after[0]) and all(torch.equal(x, y) for x, y in zip(before[1], after[1]))
    # a head stack's reverse sweep records no walk, on either grid: the counter stands still across backward()
    h = _tanh_head().to(cuda)
    ode_rl_amd.set_reverse_time_grads(True)
    forward_counts = []
    for t in (up, _t(T4)):
        n0 = lib.odehip_persistent_trajectory_launches()
        sol = ode_rl_amd.odeint(h, z0.to(cuda).requires_grad_(True), t, method="rk4")
        torch.cuda.synchronize()
        n1 = lib.odehip_persistent_trajectory_launches()
        sol.backward(gout.to(cuda))
        torch.cuda.synchronize()
        assert lib.odehip_persistent_trajectory_launches() == n1
        forward_counts.append(n1 - n0)
    assert forward_counts[0] == forward_counts[1]


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing(cuda):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f, _ = _vigorous_f()
    f = f.to(cuda)
    z, t = _z0(2).to(cuda).requires_grad_(True), _t(T4)
    n0 = lib.odehip_persistent_trajectory_launches()
    ode_rl_amd.set_reverse_time_grads(False)
    with pytest.raises(NotImplementedError, match="reversed-time.*set_reverse_time_grads"):
        ode_rl_amd.odeint(f, z, t, method="rk4")
    with pytest.raises(NotImplementedError, match="decreasing time grids are not supported.*set_reverse_time_grads"):
        ode_rl_amd.odeint_adjoint(f, z, t, method="rk4")
    ode_rl_amd.set_reverse_time_grads(True)
    for method in ("dopri5", "bosh3"):
        for opts in ({}, {"norm": "seminorm"}):
            with pytest.raises(NotImplementedError, match=f"decreasing t under method '{method}'"):
                ode_rl_amd.odeint_adjoint(f, z, t, method=method, adjoint_options=opts, **TOL)
    was = ode_rl_amd.set_adjoint_grids(True)
    try:
        with pytest.raises(NotImplementedError, match="decreasing t with options\\['grid_constructor'\\]"):
            ode_rl_amd.odeint_adjoint(f, z, t, method="rk4", options={"grid_constructor": ode_rl_amd.step_size_grid(0.11)})
    finally:
        ode_rl_amd.set_adjoint_grids(was)
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        for call in (ode_rl_amd.odeint, ode_rl_amd.odeint_adjoint):
            with pytest.raises(TypeError, match="decreasing t.*bf16"):
                call(f, z, t, method="rk4")
    finally:
        ode_rl_amd.set_compute_dtype(None)
    assert lib.odehip_persistent_trajectory_launches() == n0 and z.grad is None
