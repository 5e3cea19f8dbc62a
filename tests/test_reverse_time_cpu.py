"""Gradients through solves on a decreasing t, as far as a machine without a GPU can check them: the opt-in switch, the refusals that
stay as they were with it off, the argument checks of the new C entries (all before any HIP call), and the float64 reference of the
GPU tests (tests/_reverse_time_ref.py) against a closed form."""
import ctypes
import math

import pytest
import torch

import _reverse_time_ref as rt

T_DEC = torch.tensor([0.9, 0.6, 0.55, 0.1], dtype=torch.float64)


def _f():
    import ode_rl_amd
    return ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)


@pytest.fixture
def switch_off():
    import ode_rl_amd
    was = ode_rl_amd.set_reverse_time_grads(False)
    yield
    ode_rl_amd.set_reverse_time_grads(was)


def test_the_switch_defaults_to_off_and_returns_the_previous_value():
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    assert "set_reverse_time_grads" in ode_rl_amd.__all__
    assert hip_ops.reverse_time_grads_enabled() is False
    assert ode_rl_amd.set_reverse_time_grads(True) is False and hip_ops.reverse_time_grads_enabled() is True
    assert ode_rl_amd.set_reverse_time_grads(True) is True
    assert ode_rl_amd.set_reverse_time_grads(False) is True and hip_ops.reverse_time_grads_enabled() is False
    assert ode_rl_amd.set_reverse_time_grads(0) is False


def test_switched_off_the_refusal_of_odeint_keeps_its_text_and_names_the_switch(switch_off):
    """odeint_with_grad looks at t before it looks at a tensor's device (odeint itself refuses a CPU y0 first)."""
    from ode_rl_amd import autograd
    z = torch.zeros(1, 64, 16, 16, requires_grad=True)
    for method, options in (("rk4", None), ("euler", {"grid_constructor": lambda f, y, t: t.clone()}), ("dopri5", None), ("bosh3", None)):
        with pytest.raises(NotImplementedError, match="reversed-time") as e:
            autograd.odeint_with_grad(_f(), z, T_DEC, 1e-3, 1e-4, method, options)
        assert str(e.value).startswith("odeint(HIP): reversed-time integration is not implemented yet")
        assert "set_reverse_time_grads(True)" in str(e.value)


def test_switched_on_bf16_mode_is_a_type_error_before_any_tensor_is_looked_at():
    import ode_rl_amd
    from ode_rl_amd import autograd
    z = torch.zeros(1, 64, 16, 16, requires_grad=True)
    was = ode_rl_amd.set_reverse_time_grads(True)
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        with pytest.raises(TypeError, match="decreasing t.*bf16"):
            autograd.odeint_with_grad(_f(), z, T_DEC, 1e-3, 1e-4, "rk4", None)
    finally:
        ode_rl_amd.set_compute_dtype(None)
        ode_rl_amd.set_reverse_time_grads(was)


def _fake_stack(L, channels=(64, 64, 64), fused=False, bf16=False):
    d = L.ConvStack()
    d.n_convs, d.ks = len(channels) - 1, 3
    for i, c in enumerate(channels):
        d.channels[i] = c
    for l in range(d.n_convs):
        d.w_packed[l] = d.bias[l] = 4096
        if bf16:
            d.w_bf16[l] = 4096
    if fused:
        d.w_fused = 4096
    return d


def test_the_existing_c_entry_refuses_as_before_and_the_new_entries_check_their_arguments():
    import ode_rl_amd
    L = ode_rl_amd._lib
    lib = L.load()
    assert lib.odehip_version() == 13   # pure additions
    p, ptrs = ctypes.c_void_p(4096), (ctypes.c_void_p * 8)(*([4096] * 8))
    up, down = (ctypes.c_double * 3)(0.0, 0.4, 1.0), (ctypes.c_double * 3)(1.0, 0.4, 0.0)
    f, fmt = _fake_stack(L), ctypes.c_int(0)
    err = lambda: lib.odehip_last_error().decode()
    assert lib.odehip_odeint_fixed(ctypes.byref(f), L.RK4, p, up, 3, 2, p, 1, 1, p, 1 << 30, ctypes.byref(fmt), None) == -1
    assert "odeint_fixed: backward through negated dynamics is not supported" in err()

    fwd, bwd, adj = lib.odehip_odeint_fixed_negated_saving, lib.odehip_odeint_fixed_negated_backward, lib.odehip_odeint_adjoint_backward_negated
    assert fwd(ctypes.byref(f), L.RK4, p, down, 3, 2, p, p, 1 << 30, None) == -1 and "strictly increasing" in err()   # the caller passes -t
    assert fwd(ctypes.byref(f), L.DOPRI5, p, up, 3, 2, p, p, 1 << 30, None) == -1 and "not a fixed-grid method" in err()
    assert fwd(ctypes.byref(f), L.RK4, None, up, 3, 2, p, p, 1 << 30, None) == -1 and "odeint_fixed_negated_saving: null pointer" in err()
    assert fwd(ctypes.byref(f), L.RK4, p, up, 3, 2, p, p, 1024, None) == -1 and "workspace too small" in err()
    for bad in (_fake_stack(L, fused=True), _fake_stack(L, bf16=True)):
        assert fwd(ctypes.byref(bad), L.RK4, p, up, 3, 2, p, p, 1 << 30, None) == -1 and "fp32 stacks only" in err()
        assert bwd(ctypes.byref(bad), ctypes.byref(bad), L.RK4, up, 3, 2, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "fp32 stacks only" in err()
        assert adj(ctypes.byref(bad), ctypes.byref(bad), L.RK4, up, 3, 2, p, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "fp32 stacks only" in err()
    odd = _fake_stack(L, channels=(32, 32))
    assert fwd(ctypes.byref(odd), L.EULER, p, up, 3, 2, p, p, 1 << 30, None) == -1 and "multiples of 64" in err()
    assert bwd(ctypes.byref(f), ctypes.byref(f), L.RK4, up, 3, 2, None, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "null pointer" in err()
    assert bwd(ctypes.byref(f), ctypes.byref(f), L.RK4, up, 3, 2, p, p, ptrs, ptrs, p, 1024, None) == -1 and "workspace too small" in err()
    assert adj(ctypes.byref(f), ctypes.byref(f), L.RK4, down, 3, 2, p, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "strictly increasing" in err()
    assert adj(ctypes.byref(f), ctypes.byref(f), L.RK4, up, 3, 2, p, p, p, ptrs, ptrs, p, 1024, None) == -1 and "workspace too small" in err()

    saved, stats, log = ctypes.c_int(7), (ctypes.c_int * 4)(), (ctypes.c_double * 8)(0.0, 0.4, 0.4, 0.6, 0, 0, 0, 0)
    sav = lib.odehip_odeint_adaptive_saving_negated
    assert sav(L.BOSH3, ctypes.byref(f), p, up, 3, 2, 1e-3, 1e-4, 0.0, 0, p, stats, log, 4, 0, ctypes.byref(saved), p, 1 << 30, None) == -1
    assert "max_accept must be positive" in err()
    assert sav(9, ctypes.byref(f), p, up, 3, 2, 1e-3, 1e-4, 0.0, 0, p, stats, log, 4, 8, ctypes.byref(saved), p, 1 << 30, None) == -1
    assert "unknown adaptive method code 9" in err() and saved.value == 0
    assert sav(L.DOPRI5, ctypes.byref(_fake_stack(L, fused=True)), p, up, 3, 2, 1e-3, 1e-4, 0.0, 0, p, stats, log, 4, 8, ctypes.byref(saved), p,
               1 << 30, None) == -1 and "fp32 stacks only" in err()
    assert sav(L.DOPRI5, ctypes.byref(f), p, up, 3, 2, 1e-3, 1e-4, 0.0, 0, p, stats, log, 4, 8, ctypes.byref(saved), p, 1024, None) == -1
    assert "workspace too small" in err()
    bad = _fake_stack(L, bf16=True)
    back, back_saved = lib.odehip_odeint_adaptive_backward_negated, lib.odehip_odeint_adaptive_backward_saved_negated
    assert back(L.DOPRI5, ctypes.byref(bad), ctypes.byref(bad), up, 3, 2, log, 2, p, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "fp32 stacks only" in err()
    assert back(L.DOPRI5, ctypes.byref(f), ctypes.byref(f), up, 3, 2, log, 2, None, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "null pointer" in err()
    assert back(L.DOPRI5, ctypes.byref(f), ctypes.byref(f), down, 3, 2, log, 2, p, p, p, ptrs, ptrs, p, 1 << 30, None) == -1 and "strictly increasing" in err()
    assert back_saved(L.BOSH3, ctypes.byref(bad), ctypes.byref(bad), up, 3, 2, log, 2, p, p, ptrs, ptrs, 8, p, 1 << 30, None) == -1 and "fp32 stacks only" in err()
    assert back_saved(L.BOSH3, ctypes.byref(f), ctypes.byref(f), up, 3, 2, log, 9, p, p, ptrs, ptrs, 8, p, 1 << 30, None) == -1 and "n_steps <= max_accept" in err()


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_the_reference_reproduces_a_closed_form(method):
    """dz/dt = a z on t = [1, 0.4, 0]: z(t) = z0 exp(a (t - 1)).  With the loss sum_j g_j z(t_j): dL/dz0 = sum_j g_j exp(a (t_j - 1)) and
    dL/da = sum_j g_j (t_j - 1) z(t_j).  a = 0.1: one 3/8-rule step of 0.6 is off by (a h)^5 / 120 = 6e-9, far inside the 1e-6 asked."""
    a0, z0, t, g = 0.1, 1.7, torch.tensor([1.0, 0.4, 0.0], dtype=torch.float64), [0.3, -1.1, 0.8]
    a = torch.tensor(a0, dtype=torch.float64, requires_grad=True)
    sol, (gz, ga) = rt.solve_with_grads(lambda p: (lambda tt, y: p[0] * y), [a], torch.tensor([z0], dtype=torch.float64), t,
                                        torch.tensor(g, dtype=torch.float64).view(3, 1), method, rtol=1e-10, atol=1e-12)
    z = [z0 * math.exp(a0 * (tj - 1.0)) for tj in t.tolist()]
    want_gz = sum(gj * zj / z0 for gj, zj in zip(g, z))
    want_ga = sum(gj * (tj - 1.0) * zj for gj, tj, zj in zip(g, t.tolist(), z))
    assert max(abs(float(sol[j]) - z[j]) / abs(z[j]) for j in range(3)) <= 1e-6
    assert abs(float(gz) - want_gz) <= 1e-6 * abs(want_gz)
    assert abs(float(ga) - want_ga) <= 1e-6 * abs(want_ga)


def test_the_reference_on_a_grid_is_the_plain_reference_when_the_step_covers_every_interval():
    """step_size >= every interval of -t: the grid of -t is -t itself (the last step cut short), so both routes are one loop."""
    a = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    t, y0, g = torch.tensor([1.0, 0.6, 0.2], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64), torch.ones(3, 1, dtype=torch.float64)
    make = lambda p: (lambda tt, y: p[0] * y)
    plain = rt.solve_with_grads(make, [a], y0, t, g, "midpoint")
    grid = rt.solve_with_grads(make, [a], y0, t, g, "midpoint", step_size=0.4)
    assert torch.allclose(plain[0], grid[0], rtol=1e-13, atol=0) and all(torch.allclose(x, y, rtol=1e-12, atol=0) for x, y in zip(plain[1], grid[1]))
    finer = rt.solve_with_grads(make, [a], y0, t, g, "midpoint", step_size=0.11)
    assert not torch.allclose(plain[0], finer[0], rtol=1e-9, atol=0)
