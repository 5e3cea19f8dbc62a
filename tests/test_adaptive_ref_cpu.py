"""tests/_adaptive_ref.py pinned on the CPU.

  dopri5 tableau   reproduces oracle.torchdiffeq_ref.odeint bit for bit (solution, nfe / accepted / rejected, every dt and error
                   ratio) on two fixture stacks of _solver_stack_cases.py: F1 (no rejected step) and F6 (rejecting), and with
                   first_step / on a decreasing grid.  The generic code path is therefore the oracle's arithmetic.
  bosh3 tableau    equals scipy's RK23 (A, B, C = beta, c_sol, alpha; E = -c_error); one accepted step ends where
                   solve_ivp(method="RK23") ends on a linear system, to rounding; order conditions: y = t^3 is integrated exactly by
                   the solution weights, the error estimate vanishes on y = t^2 (the embedded pair is second order), the observed
                   convergence order on a linear system against expm is 3.
  adjoint          with the dopri5 tableau, odeint_adjoint reproduces oracle.torchdiffeq_ref.odeint_adjoint bit for bit under both norms
                   (trajectory, every gradient, nfe / accepted / rejected and every error ratio of the backward solves)."""
import math

import numpy as np
import pytest
import torch

import _adaptive_ref as ar
import _solver_stack_cases as sc
from oracle import torchdiffeq_ref as ref


@pytest.mark.parametrize("case,options", [("F1.dopri5", None), ("F6.dopri5", None), ("F6.dopri5", {"first_step": 0.05}),
                                          ("F8.F4.dopri5.decreasing", None)])
def test_dopri5_tableau_reproduces_the_oracle_bit_for_bit(case, options):
    spec = sc.forward_case(case)
    for dtype in (torch.float32, torch.float64):
        ws, bs = sc._params(spec, dtype)
        f = sc.dynamics(spec, ws, bs)
        s_o, s_a = {}, {}
        with torch.no_grad():
            want = ref.odeint(f, spec["z0"].to(dtype), spec["t"], method="dopri5", stats=s_o, options=options, **sc.DOPRI5_TOL)
            got = ar.odeint(f, spec["z0"].to(dtype), spec["t"], method="dopri5", stats=s_a, options=options, **sc.DOPRI5_TOL)
        assert torch.equal(got, want)
        for key in ("nfe", "dts", "ratios", "steps_per_output"):
            assert s_a[key] == s_o[key], key
        assert (s_a["n_accept"], s_a["n_reject"]) == (s_o.get("n_accept", 0), s_o.get("n_reject", 0))
        assert len(s_a["accepted"]) == s_a["n_accept"]
    if case.startswith("F6") and options is None:
        assert s_o["n_reject"] >= 1   # the rejecting case rejects


def test_bosh3_tableau_is_scipys_rk23():
    rk = pytest.importorskip("scipy.integrate").RK23
    tb = ar.BOSH3
    assert rk.n_stages == 3 and rk.order == 3 == tb.order and rk.error_estimator_order == 2
    np.testing.assert_array_equal(rk.C, np.array([0.0] + tb.alpha[:-1]))
    assert tb.alpha[-1] == 1.0
    for i, row in enumerate(tb.beta[:-1]):
        np.testing.assert_array_equal(rk.A[i + 1, :len(row)], np.array(row))
        assert not rk.A[i + 1, len(row):].any()
    np.testing.assert_array_equal(rk.B, np.array(tb.c_sol[:3]))
    np.testing.assert_array_equal(np.array(tb.beta[-1]), rk.B)       # FSAL: the last beta row is the solution row
    np.testing.assert_allclose(rk.E, -np.array(tb.c_error), rtol=0, atol=1e-16)   # scipy: y_new - y_hat with the opposite sign
    np.testing.assert_allclose(sum(tb.c_error), 0.0, atol=1e-16)


A_LIN = torch.tensor([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.1, 0.0, -1.0]], dtype=torch.float64)
Y_LIN = torch.tensor([1.0, -0.5, 0.25], dtype=torch.float64)


def _lin(t, y):
    return A_LIN @ y


def test_one_bosh3_step_ends_where_scipys_rk23_ends():
    solve_ivp = pytest.importorskip("scipy.integrate").solve_ivp
    h = 0.05
    sol = solve_ivp(lambda t, y: A_LIN.numpy() @ y, (0.0, h), Y_LIN.numpy(), method="RK23", first_step=h, rtol=1e-3, atol=1e-6)
    assert sol.t.tolist() == [0.0, h]   # one accepted step of exactly h
    t0, dt = torch.tensor(0.0, dtype=torch.float64), torch.tensor(h, dtype=torch.float64)
    y1, f1, err, k = ar.rk_step(ar.BOSH3, _lin, Y_LIN, _lin(t0, Y_LIN), t0, dt, t0 + dt)
    np.testing.assert_allclose(y1.numpy(), sol.y[:, -1], rtol=0, atol=4e-16)
    assert torch.equal(f1, k[-1]) and torch.allclose(f1, _lin(t0 + dt, y1), rtol=0, atol=1e-15)   # FSAL: f1 = f(y1) = k4
    # the whole solver, first_step = h and tolerances the step passes, ends its first step there too
    stats = {}
    out = ar.odeint(_lin, Y_LIN, torch.tensor([0.0, h], dtype=torch.float64), rtol=1e-3, atol=1e-6, method="bosh3",
                    options={"first_step": h}, stats=stats)
    assert (stats["nfe"], stats["n_accept"], stats["n_reject"]) == (4, 1, 0)
    # (through the quartic dense output at x = 1: its coefficients weigh y_mid with 32, so the sum cancels to 32 eps |y| <= 7e-15)
    np.testing.assert_allclose(out[1].numpy(), sol.y[:, -1], rtol=0, atol=32 * 2.3e-16)


def test_bosh3_order_conditions():
    tb = ar.BOSH3
    t0, dt = torch.tensor(0.3, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)
    y0 = torch.tensor([t0 ** 3], dtype=torch.float64)
    cubic = lambda t, y: torch.stack([3 * t ** 2])   # noqa: E731
    y1, _, err3, _ = ar.rk_step(tb, cubic, y0, cubic(t0, y0), t0, dt, t0 + dt)
    assert abs(float(y1) - 1.0) <= 4e-16          # third order: t^3 exactly (1.0 = (0.3 + 0.7)^3)
    assert abs(float(err3)) > 1e-3                # ... which the second-order companion does not manage
    y0 = torch.tensor([t0 ** 2], dtype=torch.float64)
    quad = lambda t, y: torch.stack([2 * t])      # noqa: E731
    y1, _, err2, _ = ar.rk_step(tb, quad, y0, quad(t0, y0), t0, dt, t0 + dt)
    assert abs(float(y1) - 1.0) <= 4e-16 and abs(float(err2)) <= 4e-16   # both orders integrate t^2: the estimate vanishes


def test_bosh3_converges_with_order_three():
    exact = torch.linalg.matrix_exp(A_LIN) @ Y_LIN

    def solve(n):
        y, t, dt = Y_LIN, torch.tensor(0.0, dtype=torch.float64), torch.tensor(1.0 / n, dtype=torch.float64)
        f = _lin(t, y)
        for _ in range(n):
            y, f, _, _ = ar.rk_step(ar.BOSH3, _lin, y, f, t, dt, t + dt)
            t = t + dt
        return float((y - exact).norm())
    errs = [solve(n) for n in (20, 40, 80)]
    orders = [math.log2(a / b) for a, b in zip(errs, errs[1:])]
    print("errors", errs, "observed orders", orders)
    assert all(2.8 <= o <= 3.2 for o in orders), orders


def test_dense_output_of_bosh3_passes_through_its_three_points():
    """The quartic of interp_fit goes through y0 at x = 0, y1 at x = 1 and y_mid = y0 + dt k2 / 2 at x = 1 / 2, with slope dt f0 at 0."""
    tb = ar.BOSH3
    t0, dt = torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.37, dtype=torch.float64)
    y1, _, _, k = ar.rk_step(tb, _lin, Y_LIN, _lin(t0, Y_LIN), t0, dt, t0 + dt)
    coeffs = ar.interp_fit(tb, Y_LIN, y1, k, dt)
    at = lambda x: ref._interp_evaluate(coeffs, t0, t0 + dt, t0 + x * dt)   # noqa: E731
    assert torch.equal(at(0.0), Y_LIN)
    assert float((at(1.0) - y1).abs().max()) <= 32 * 2.3e-16 * 2
    assert float((at(0.5) - (Y_LIN + dt * 0.5 * k[1])).abs().max()) <= 32 * 2.3e-16 * 2
    assert torch.equal(coeffs[1], dt * k[0])


@pytest.mark.parametrize("norm", ["mixed", "seminorm"])
def test_adjoint_with_the_dopri5_tableau_reproduces_the_oracle_bit_for_bit(norm):
    import _bosh3_cases as bc
    spec = bc.backward_spec("GT")
    for dtype in (torch.float32, torch.float64):
        out = []
        for mod in (ref, ar):
            ws, bs = sc._params(spec, dtype, requires_grad=True)
            stats = {}
            ys, gz, gp = mod.odeint_adjoint(sc.dynamics(spec, ws, bs), spec["z0"].to(dtype), spec["t"], ws + bs, spec["gout"].to(dtype),
                                            method="dopri5", stats=stats, adjoint_norm=norm, **sc.DOPRI5_TOL)
            out.append((ys, gz, gp, stats))
        (ys_o, gz_o, gp_o, s_o), (ys_a, gz_a, gp_a, s_a) = out
        assert torch.equal(ys_a, ys_o) and torch.equal(gz_a, gz_o) and all(torch.equal(a, b) for a, b in zip(gp_a, gp_o))
        for key in ("nfe", "n_accept", "dts", "ratios"):
            assert s_a[key] == s_o[key], key
        assert s_a["n_reject"] == s_o.get("n_reject", 0) and s_a["n_accept"] >= 2
