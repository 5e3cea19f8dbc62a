"""odeint(method="bosh3") on the device against tests/_adaptive_ref.py (cases and their CPU-proved conditions: tests/_bosh3_cases.py,
tests/test_bosh3_cases_cpu.py).

Forward    same (nfe, n_accept, n_reject) as the float32 restatement; trajectory increments within max(4 x d32, DOPRI5_FLOOR) of the
           float64 restatement, frame by frame (d32: the float32 restatement's own distance; the floor is the dopri5 floor of
           test_hip_solver_stacks.py -- the same quartic dense output cancels in fp32); reruns bitwise equal; the asynchronous solve
           (set_async_dopri5) bitwise equal to the synchronous one; first_step and max_num_steps honoured, a solve that runs out of
           max_num_steps raises AssertionError as dopri5's does.
Backward   every gradient tensor of odeint(...).backward against float64 autograd through the restatement, within
           max(4 x d32, GRAD_FLOOR): with the activations kept by the saving forward (64-channel stack, adaptive walk), re-integrated
           when the saving slots run out, and on stacks that never save.
bosh3 is not dopri5: on the vigorous fixture the device's two methods differ by >= 1e-5, and each sits next to its own restatement.
Adjoint    odeint_adjoint(method="bosh3") under the mixed norm and the seminorm against the restatement's adjoint in float64: the same
           (nfe, n_accept, n_reject) of the backward solves in last_adjoint_stats, every gradient within max(4 x d32, GRAD_FLOOR); a
           max_accept too small for the accepted steps is ValueError.  Both norms run the host-driven loop.
Not built: bf16 compute mode raises TypeError.

Every test here fails on a library without bosh3 with ValueError('Invalid method "bosh3"')."""
import pytest
import torch

import _adaptive_ref as ar
import _bosh3_cases as bc
import _convgru_ref as cref
import _solver_stack_cases as sc
from conftest import record, rel_l2, vigorous_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forward_refs():
    out = {}
    for name in bc.FORWARD:
        spec = bc.forward_spec(name)
        out[name] = (spec, bc.forward_reference(spec, torch.float64), bc.forward_reference(spec, torch.float32))
    return out


@pytest.mark.parametrize("name", sorted(bc.FORWARD))
def test_trajectory_and_step_counts_match_the_restatement(cuda, forward_refs, name):
    spec, (r64, s64), (r32, s32) = forward_refs[name]
    f = sc.device_func(cuda, spec)
    sol, counts = bc.device_forward(cuda, spec, f=f)
    assert counts == bc.counts(s32) == bc.counts(s64), (counts, bc.counts(s32))
    assert torch.equal(sol[0].cpu(), spec["z0"])
    i64, i32, got = sc.increments(r64, spec["z0"]), sc.increments(r32, spec["z0"]), sc.increments(sol, spec["z0"])
    tol, d32 = cref.bound(i32, i64, sc.DOPRI5_FLOOR)
    e = record(f"bosh3.{name}.increments", rel_l2(got, i64))
    print(f"{name}: rel-L2 of the increments {e:.3e}, d32 {d32:.3e}, bound {tol:.3e}, counts {counts}")
    assert e <= tol
    for j in range(got.shape[0]):
        e_j = rel_l2(got[j], i64[j])
        print(f"  frame {j + 1}: {e_j:.3e}")
        assert e_j <= cref.bound(i32[j], i64[j], sc.DOPRI5_FLOOR)[0], (name, j, e_j)
    again, counts2 = bc.device_forward(cuda, spec, f=f)
    assert counts2 == counts and torch.equal(again, sol)   # a rerun is bitwise equal


@pytest.mark.parametrize("name", ["R1", "R3", "W2"])
def test_asynchronous_solve_is_bitwise_the_synchronous_one(cuda, forward_refs, name):
    import ode_rl_amd
    spec = forward_refs[name][0]
    f = sc.device_func(cuda, spec)
    sync, counts = bc.device_forward(cuda, spec, f=f)
    was = ode_rl_amd.set_async_dopri5(True)
    try:
        asyn, counts_async = bc.device_forward(cuda, spec, f=f)
    finally:
        ode_rl_amd.set_async_dopri5(was)
    assert counts_async == counts and torch.equal(asyn, sync)


def test_first_step_and_max_num_steps_are_honoured(cuda, forward_refs):
    import ode_rl_amd
    spec = forward_refs["R1"][0]
    f = sc.device_func(cuda, spec)
    opts = {"first_step": 0.01}
    r32, s32 = bc.forward_reference(spec, torch.float32, options=opts)
    r64, s64 = bc.forward_reference(spec, torch.float64, options=opts)
    assert bc.counts(s32) == bc.counts(s64) and s32["nfe"] == 1 + 3 * (s32["n_accept"] + s32["n_reject"])
    sol, counts = bc.device_forward(cuda, spec, options=opts, f=f)
    assert counts == bc.counts(s32)
    assert ode_rl_amd.last_stats["accepted"][0] == (0.0, 0.01)
    i64 = sc.increments(r64, spec["z0"])
    assert rel_l2(sc.increments(sol, spec["z0"]), i64) <= cref.bound(sc.increments(r32, spec["z0"]), i64, sc.DOPRI5_FLOOR)[0]
    # the restatement needs max(steps_per_output) attempts for one output time: one fewer fails, on both sides, that many pass
    need = max(s32["steps_per_output"])
    assert need >= 2
    with pytest.raises(AssertionError):
        bc.forward_reference(spec, torch.float32, options={"first_step": 0.01, "max_num_steps": need - 1})
    with pytest.raises(AssertionError):
        bc.device_forward(cuda, spec, options={"first_step": 0.01, "max_num_steps": need - 1}, f=f)
    ok, counts_ok = bc.device_forward(cuda, spec, options={"first_step": 0.01, "max_num_steps": need}, f=f)
    assert counts_ok == counts and torch.equal(ok, sol)


def _check_gradients(name, spec, got, tag):
    g64, _, s64 = bc.backward_reference(spec, torch.float64)
    g32, _, _ = bc.backward_reference(spec, torch.float32)
    for k in sorted(g64):
        tol, d32 = cref.bound(g32[k], g64[k], sc.GRAD_FLOOR)
        e = record(f"bosh3.{name}.{tag}.grad.{k}", rel_l2(got[k], g64[k]))
        print(f"{name} {tag} {k}: {e:.3e} (d32 {d32:.3e}, bound {tol:.3e})")
        assert e <= tol, (name, tag, k, e)
    return s64


@pytest.mark.parametrize("name", sorted(bc.BACKWARD))
def test_gradients_match_float64_autograd_through_the_restatement(cuda, name):
    spec = bc.backward_spec(name)
    got, st = bc.device_backward(cuda, spec)
    s64 = _check_gradients(name, spec, got, "sweep")
    assert (st["nfe"], st["n_accept"], st["n_reject"]) == bc.counts(s64)
    if name == "G64":
        assert st["saved"]   # the 64-channel stack keeps its activations: the backward was the reverse sweep alone


def test_gradients_when_the_saving_slots_run_out(cuda, monkeypatch):
    """One saving slot for a forward that accepts three steps: nothing is handed to the backward pass, which re-integrates the logged
    steps -- the same gradients."""
    from ode_rl_amd import hip_ops
    spec = bc.backward_spec("G64")
    monkeypatch.setattr(hip_ops, "_dopri5_save_slots", 1)
    got, st = bc.device_backward(cuda, spec)
    assert st["n_accept"] >= 2 and not st["saved"]
    _check_gradients("G64", spec, got, "reintegrated")


def test_bosh3_is_not_dopri5(cuda):
    import ode_rl_amd
    from oracle import reference_modules as rm
    sd, z0, t, _ = vigorous_case()
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)
    f.load_state_dict(sd)
    f = f.to(cuda)
    ws, bs = rm.split_convnet_state(sd, "gradient_net.")
    fr = rm.ode_func([w.double() for w in ws], [b.double() for b in bs])
    sols = {}
    with torch.no_grad():
        for m in ("bosh3", "dopri5"):
            sols[m] = ode_rl_amd.odeint(f, z0.to(cuda), t.to(cuda), method=m, **bc.TOL).cpu()
            want = ar.odeint(fr, z0.double(), t, method=m, **bc.TOL)
            e = record(f"bosh3.traj_vig.{m}", rel_l2(sols[m][-1], want[-1]))
            assert e <= sc.DOPRI5_FLOOR, (m, e)
    d = rel_l2(sols["bosh3"][-1], sols["dopri5"][-1])
    print("device bosh3 vs device dopri5, last frame:", d)
    assert d >= 1e-5


def test_diffeqsolver_passes_the_method_through(cuda, forward_refs):
    import ode_rl_amd
    spec, (r64, _), (r32, _) = forward_refs["R3"]
    f = sc.device_func(cuda, spec)
    solver = ode_rl_amd.DiffEqSolver(f, "bosh3", odeint_rtol=bc.TOL["rtol"], odeint_atol=bc.TOL["atol"], device=cuda)
    with torch.no_grad():
        sol = solver(spec["z0"].to(cuda), spec["t"].to(cuda))
    i64 = sc.increments(r64, spec["z0"])
    assert rel_l2(sc.increments(sol, spec["z0"]), i64) <= cref.bound(sc.increments(r32, spec["z0"]), i64, sc.DOPRI5_FLOOR)[0]
    assert ode_rl_amd.last_stats["n_reject"] >= 1


def test_what_is_not_built_is_refused_by_name(cuda, forward_refs):
    import ode_rl_amd
    spec = forward_refs["R1"][0]
    f = sc.device_func(cuda, spec)
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        with pytest.raises(TypeError, match="bosh3.*bf16"):
            bc.device_forward(cuda, spec, f=f)
    finally:
        ode_rl_amd.set_compute_dtype(None)
    with pytest.raises(ValueError, match="Invalid method"):
        ode_rl_amd.odeint(f, spec["z0"].to(cuda), spec["t"], method="adaptive_heun")


@pytest.mark.parametrize("norm", ["mixed", "seminorm"])
@pytest.mark.parametrize("name", sorted(bc.BACKWARD))
def test_adjoint_matches_the_restatements_adjoint(cuda, name, norm):
    spec = bc.backward_spec(name)
    g64, s64 = bc.adjoint_reference(spec, torch.float64, norm)
    g32, _ = bc.adjoint_reference(spec, torch.float32, norm)
    got, st = bc.device_adjoint(cuda, spec, norm)
    assert (st["nfe"], st["n_accept"], st["n_reject"]) == bc.counts(s64), (st, bc.counts(s64))
    for k in sorted(g64):
        tol, d32 = cref.bound(g32[k], g64[k], sc.GRAD_FLOOR)
        e = record(f"bosh3.{name}.adjoint.{norm}.grad.{k}", rel_l2(got[k], g64[k]))
        print(f"{name} adjoint {norm} {k}: {e:.3e} (d32 {d32:.3e}, bound {tol:.3e})")
        assert e <= tol, (name, norm, k, e)


def test_adjoint_max_accept_bounds_the_accepted_steps(cuda):
    spec = bc.backward_spec("GT")
    _, s64 = bc.adjoint_reference(spec, torch.float64, "seminorm")
    # the workspace holds max_accept + 1 slots (adjoint_layout.h, as for dopri5): n_accept - 1 is exactly enough, one fewer is not
    got, st = bc.device_adjoint(cuda, spec, "seminorm", max_accept=s64["n_accept"] - 1)
    assert st["n_accept"] == s64["n_accept"] >= 3
    with pytest.raises(ValueError, match="max_accept"):
        bc.device_adjoint(cuda, spec, "seminorm", max_accept=s64["n_accept"] - 2)


def test_upstream_diffeqsolver_passes_the_method_through(cuda, forward_refs):
    from ode_rl_amd.models.conv_odegru import DiffeqSolver
    spec, (r64, _), (r32, _) = forward_refs["R1"]
    f = sc.device_func(cuda, spec)
    solver = DiffeqSolver(64, f, "bosh3", 64, odeint_rtol=bc.TOL["rtol"], odeint_atol=bc.TOL["atol"], device=cuda)
    with torch.no_grad():
        sol = solver(spec["z0"].to(cuda), spec["t"].to(cuda)).permute(1, 0, 2, 3, 4)   # batch-first -> time-first
    i64 = sc.increments(r64, spec["z0"])
    assert rel_l2(sc.increments(sol, spec["z0"]), i64) <= cref.bound(sc.increments(r32, spec["z0"]), i64, sc.DOPRI5_FLOOR)[0]
