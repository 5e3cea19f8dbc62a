"""Fixed-grid solvers on an internal grid (options={"grid_constructor": fn}, ode_rl_amd.step_size_grid), the parts that need no GPU:
torchdiffeq's step-size grid, the emit table the library builds on the host (csrc/grid_interp.hip: odehip_grid_emit_table) against
known answers and against its Python restatement (tests/_grid_ref.py), the validation of grids and options, and the routing of
`odeint` down to the point where it looks at a tensor."""
import ctypes

import pytest
import torch

import _grid_ref

T3 = [0.0, 0.5, 1.0]


def _f():
    import ode_rl_amd
    return ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)


@pytest.mark.parametrize("step,want", [(0.3, [0.0, 0.3, 0.6, 0.9, 1.0]),          # the last step is cut short
                                       (0.25, [0.0, 0.25, 0.5, 0.75, 1.0]),       # divides the span exactly
                                       (2.0, [0.0, 1.0])])                        # larger than the span: [t0, tT]
def test_step_size_grid_known_answers(step, want):
    import ode_rl_amd
    t = torch.tensor(T3, dtype=torch.float64)
    grid = ode_rl_amd.step_size_grid(step)(None, None, t)
    assert grid.dtype == torch.float64 and grid[0] == t[0] and grid[-1] == t[-1]
    torch.testing.assert_close(grid, torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.equal(grid, _grid_ref.step_size_grid_ref(t, step))
    # an offset, float32 t: converted to float64 first, the grid still ends on t[-1] exactly
    t32 = torch.tensor([0.1, 0.25, 0.7], dtype=torch.float32)
    g32 = ode_rl_amd.step_size_grid(step)(None, None, t32)
    assert g32.dtype == torch.float64 and g32[0] == t32[0].double() and g32[-1] == t32[-1].double()
    assert "step_size_grid" in ode_rl_amd.__all__


def test_step_size_grid_refuses_nonpositive_steps():
    import ode_rl_amd
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="step_size"):
            ode_rl_amd.step_size_grid(bad)


# (grid, t, first, slope (float64 quotient, rounded to fp32 by the table), exact)
TABLES = {
    "finer_unaligned": ([0.0, 0.3, 0.6, 0.9, 1.0], T3, [1, 1, 2, 2, 3], [0.0, (0.5 - 0.3) / (0.6 - 0.3), 1.0], [True, False, True]),
    # one interval emits three outputs, two emit none
    "coarser_multi": ([0.0, 0.4, 0.5, 0.6, 2.0], [0.0, 0.1, 0.2, 0.3, 2.0], [1, 4, 4, 4, 5], [0.0, 0.1 / 0.4, 0.2 / 0.4, 0.3 / 0.4, 1.0],
                      [True, False, False, False, True]),
    "identity": (T3, T3, [1, 2, 3], [0.0, 1.0, 1.0], [True, True, True]),
    "interior_hit": ([0.0, 0.25, 0.5, 1.0], [0.0, 0.5, 0.75, 1.0], [1, 1, 2, 4], [0.0, 1.0, (0.75 - 0.5) / (1.0 - 0.5), 1.0],
                     [True, True, False, True]),
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_emit_table_known_answers(name):
    from ode_rl_amd import hip_ops
    grid, t, first, slope, exact = TABLES[name]
    table = hip_ops.grid_emit_table(torch.tensor(grid, dtype=torch.float64), torch.tensor(t, dtype=torch.float64))
    assert table.first == first and table.first[0] == 1 and table.first[-1] == len(t)
    assert table.exact == exact
    assert table.slope == [float(torch.tensor(s, dtype=torch.float64).to(torch.float32)) for s in slope]
    assert (table.first, table.slope, table.exact) == _grid_ref.emit_table_ref(grid, t)


def test_c_table_builder_agrees_with_the_restatement_on_random_grids():
    from ode_rl_amd import hip_ops
    g = torch.Generator().manual_seed(3)
    for n_grid, n_times in [(2, 9), (9, 2), (17, 17), (40, 7), (7, 40), (33, 5)]:
        pts = torch.rand(n_grid + n_times, generator=g, dtype=torch.float64).sort().values
        pick = torch.randperm(n_grid + n_times - 2, generator=g)[:n_times - 2] + 1
        t = torch.cat([pts[:1], pts[pick].sort().values, pts[-1:]])
        grid = torch.cat([pts[:1], pts[torch.randperm(n_grid + n_times - 2, generator=g)[:n_grid - 2] + 1].sort().values, pts[-1:]])
        table = hip_ops.grid_emit_table(grid, t)   # the two draws overlap: some outputs fall exactly on interior grid points
        assert (table.first, table.slope, table.exact) == _grid_ref.emit_table_ref(grid, t)
        assert all(a <= b for a, b in zip(table.first, table.first[1:]))


def test_grid_validation():
    from ode_rl_amd import hip_ops
    t = torch.tensor(T3, dtype=torch.float64)
    for bad in ([0.0, 0.5, 0.9], [0.1, 0.5, 1.0]):                      # the end points must be t's
        with pytest.raises(AssertionError, match="start at t\\[0\\] and end at t\\[-1\\]"):
            hip_ops.grid_emit_table(torch.tensor(bad, dtype=torch.float64), t)
    for bad in ([0.0, 0.6, 0.4, 1.0], [0.0, 0.5, 0.5, 1.0]):            # strictly increasing
        with pytest.raises(AssertionError, match="strictly increasing"):
            hip_ops.grid_emit_table(torch.tensor(bad, dtype=torch.float64), t)
    with pytest.raises(AssertionError, match="one dimensional"):
        hip_ops.grid_emit_table(torch.zeros(2, 2, dtype=torch.float64), t)
    # a grid that is not float64 is converted as host_times converts t
    table = hip_ops.grid_emit_table(torch.tensor([0.0, 0.25, 1.0], dtype=torch.float32), t)
    assert table.first == [1, 1, 3] and table.exact == [True, False, True]


def test_the_launches_refuse_bad_arguments_before_any_hip_call():
    """Null pointers, a table that does not cover T, and G < 2 with T > 1: ODEHIP_EINVAL with a message, checkable without a GPU."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    first, slope, exact = (ctypes.c_int * 3)(1, 2, 3), (ctypes.c_float * 3)(0, 1, 1), (ctypes.c_int * 3)(1, 1, 1)
    p = ctypes.c_void_p(4096)
    nbytes = lib.odehip_grid_table_bytes(3, 3)
    assert nbytes >= (3 + 3 * 3) * 4 and nbytes % 16 == 0
    for fn in (lib.odehip_grid_emit, lib.odehip_grid_scatter):
        assert fn(None, p, first, slope, exact, 3, 3, 1024, p, nbytes, None) == -1 and b"null" in lib.odehip_last_error()
        assert fn(p, p, first, slope, exact, 3, 3, 1024, None, nbytes, None) == -1 and b"null" in lib.odehip_last_error()
        assert fn(p, p, first, slope, exact, 1, 3, 1024, p, nbytes, None) == -1 and b"cannot serve" in lib.odehip_last_error()
        assert fn(p, p, first, slope, exact, 3, 3, 1024, p, nbytes - 4, None) == -1 and b"are needed" in lib.odehip_last_error()
        assert fn(p, p, first, slope, exact, 3, 3, 1022, p, nbytes, None) == -1 and b"multiple of 4" in lib.odehip_last_error()
        short = (ctypes.c_int * 3)(1, 2, 2)    # covers two of the three outputs
        assert fn(p, p, short, slope, exact, 3, 3, 1024, p, nbytes, None) == -1 and b"does not cover" in lib.odehip_last_error()
        back = (ctypes.c_int * 3)(1, 0, 3)
        assert fn(p, p, back, slope, exact, 3, 3, 1024, p, nbytes, None) == -1 and b"not monotone" in lib.odehip_last_error()
        assert fn(p, p, first, slope, exact, 3, 5000, 1024, p, 1 << 20, None) == -1 and b"at most 4096" in lib.odehip_last_error()
    d = (ctypes.c_double * 3)(0.0, 0.5, 1.0)
    assert lib.odehip_grid_emit_table(d, 3, None, 3, first, slope, exact) == -1 and b"null" in lib.odehip_last_error()
    assert lib.odehip_grid_emit_table(d, 1, d, 3, first, slope, exact) == -1 and b"cannot serve" in lib.odehip_last_error()


def test_options_are_checked_before_any_tensor_is_looked_at():
    import ode_rl_amd
    f, z, t = _f(), torch.zeros(1, 64, 16, 16), torch.tensor([0.0, 1.0])
    grid = ode_rl_amd.step_size_grid(0.05)
    for method in ("euler", "midpoint", "rk4"):
        with pytest.raises(ValueError, match="interp"):
            ode_rl_amd.odeint(f, z, t, method=method, options={"grid_constructor": grid, "interp": "cubic"})
        with pytest.raises(TypeError, match="callable"):
            ode_rl_amd.odeint(f, z, t, method=method, options={"grid_constructor": 0.05})
        with pytest.raises(ValueError, match="perturb"):
            ode_rl_amd.odeint(f, z, t, method=method, options={"grid_constructor": grid, "perturb": True})
    with pytest.raises(ValueError, match="step_size_grid"):      # the refusal of step_size stays and now names the helper
        ode_rl_amd.odeint(f, z, t, method="rk4", options={"step_size": 0.05})
    with pytest.raises(ValueError, match="grid_constructor"):     # the adaptive solver has no grid to construct
        ode_rl_amd.odeint(f, z, t, method="dopri5", options={"grid_constructor": grid})


def test_gridded_odeint_reaches_the_tensor_check():
    """Every option accepted: the next thing looked at is the tensor, and there is no CPU fallback."""
    import ode_rl_amd
    f, z, t = _f(), torch.zeros(1, 64, 16, 16), torch.tensor([0.0, 1.0])
    for options in ({"grid_constructor": ode_rl_amd.step_size_grid(0.05)},
                    {"grid_constructor": ode_rl_amd.step_size_grid(0.05), "interp": "linear"}, {"interp": "linear"}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ode_rl_amd.odeint(f, z, t, method="rk4", options=options)
    solver = ode_rl_amd.DiffEqSolver(f, "rk4", options={"grid_constructor": ode_rl_amd.step_size_grid(0.05)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solver(z, t)


def test_odeint_adjoint_still_refuses_internal_grids():
    import ode_rl_amd
    f, z, t = _f(), torch.zeros(1, 64, 16, 16), torch.tensor([0.0, 1.0])
    with pytest.raises(ValueError, match="grid_constructor"):
        ode_rl_amd.odeint_adjoint(f, z, t, method="rk4", options={"grid_constructor": ode_rl_amd.step_size_grid(0.05)})
    with pytest.raises(ValueError, match="interp"):
        ode_rl_amd.odeint_adjoint(f, z, t, method="euler", options={"interp": "linear"})


def test_models_read_decode_step_size():
    import argparse
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    from ode_rl_amd.models.VidODE import VidODE
    base = dict(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3, neural_ode_n_units=64,
                neural_ode_decoder_out_ch=64, decode_diff_method="rk4", mem=False, z_sample=False, n_layers=2)
    t = torch.tensor(T3, dtype=torch.float64)
    for cls in (ODEConvGRU, VidODE):
        assert cls(argparse.Namespace(**base), torch.device("cpu")).diffeq_solver.options is None
        options = cls(argparse.Namespace(decode_step_size=0.3, **base), torch.device("cpu")).diffeq_solver.options
        assert sorted(options) == ["grid_constructor"]
        assert torch.equal(options["grid_constructor"](None, None, t), _grid_ref.step_size_grid_ref(t, 0.3))
