"""The solvers on stacks whose layers run the DIRECT convolution kernels (csrc/conv_q4.hip), against the float64 oracle.

A convolution kernel also carries the solver's arithmetic in its epilogue, and that arithmetic exists twice in csrc/conv_common.h:
emit_quad() behind the Winograd kernels, epilogue() behind the 32x32-accumulator kernels.  Every other trajectory test builds its
dynamics from 32 / 64 / 128-channel 3x3 layers, whose last layer and input-gradient layers are Winograd layers: the stage combine
(combine 1, with the dopri5 error partials), the activation-mask backward (combine 2) and the reverse-sweep targets (combine 3) of
epilogue() run there under no fp32 bound.  The stacks of tests/_solver_stack_cases.py put a direct kernel where those branches are taken:

  F1  32 -> 96 -> 96 -> 32, 3x3     ring kernel as last layer (6 chunks): order-0 and order-1 combine, k_out, out2_nchw, partials at C = 32
  F2  64 -> 192 -> 64, 3x3          ring with 12 chunks as last layer
  F3  256 -> 256, one 3x3 conv      first = last layer, 16 chunks, cout 256
  F4  32 -> 32 -> 32, 5x5           conv_ring_kernel<5,1,4> with combine (launch_wino5 declines a stage combine)
  F5  128 -> 128 -> 128, 5x5, B 33  conv_ring_kernel<5,1,2,2> (264 workgroups) with combine
  F6  64 -> 32 -> 64, 1x1           1x1 ring with combine
  F7  F1 with Tanh layers and head  act_fwd in epilogue()
  F8  F1, F4 on a decreasing t      k_scale = -1
  B1  64 -> 192 -> 192 -> 64        ring input-gradient layers with combine 2 (192 -> 192) and combine 3 (192 -> 64); weight gradients at 192
  B2  192 -> 64 -> 192              ring input-gradient layer with combine 2 as the chain's first row, Winograd combine 3 next to it
  B3  B1 with Tanh hidden layers    act_bwd Tanh in epilogue()

Bounds (tests/_convgru_ref.py::bound): max(4 * d32, floor) with d32 the float32 restatement's own distance from the float64 one and the
project's floors -- increments of a fixed-grid trajectory 3e-6, of a dopri5 trajectory 5e-5, a gradient tensor 1e-4.
tests/test_solver_stack_cases_cpu.py asserts 4 * d32 <= floor for every case, so the floor is the bound.  dopri5 runs at rtol 1e-3,
atol 1e-4 and must take the oracle's (n_accept, n_reject); F4 and F6 reject steps.

Every forward case is also run twice (bitwise equal) and on a rotated batch.  A fixed-grid solve treats every sample on its own, so
the rotated run must equal the rotated result bit for bit (a misplaced `off` cannot).  dopri5 couples the samples through ONE error
norm over the whole batch (torchdiffeq's rms norm), summed in float32 in a fixed order of per-wave partials: a rotation reorders that
sum, the ratio moves in its last bits and so does every later step size.  There the rotated run must take the same (n_accept,
n_reject) and stay within the dopri5 floor of the first run; a partial that is lost or counted twice changes the norm by 1 / (number
of partials) or more and fails the step counts against the oracle."""
import pytest
import torch

import _convgru_ref as ref
import _solver_stack_cases as sc
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

_REFS = {}


def _forward_reference(case):
    """(spec, float64 trajectory, its step counts, float32 trajectory), computed once per case; the stack's values once per stack."""
    if case not in _REFS:
        stack = sc.FORWARD_CASES[case][0]
        if ("stack", stack) not in _REFS:
            _REFS[("stack", stack)] = sc.forward_stack(stack)
        spec = sc.forward_case(case, {stack: _REFS[("stack", stack)]})
        r64, c64 = sc.forward_reference(spec, torch.float64)
        r32, _ = sc.forward_reference(spec, torch.float32)
        _REFS[case] = (spec, r64, c64, r32)
    return _REFS[case]


def _backward_reference(case):
    if case not in _REFS:
        spec = sc.backward_case(case)
        g64, margin, c64 = sc.backward_reference(spec, torch.float64)
        g32, _, _ = sc.backward_reference(spec, torch.float32)
        _REFS[case] = (spec, g64, margin, c64, g32)
    return _REFS[case]


@pytest.mark.parametrize("case", list(sc.FORWARD_CASES))
def test_trajectory_matches_the_float64_oracle(cuda, case):
    spec, r64, c64, r32 = _forward_reference(case)
    z0, adaptive = spec["z0"], spec["method"] == "dopri5"
    floor = sc.DOPRI5_FLOOR if adaptive else sc.FIXED_FLOOR
    f = sc.device_func(cuda, spec)
    sol, counts = sc.device_forward(cuda, spec, f)
    assert sol.shape == r64.shape and torch.equal(sol[0].cpu(), z0)    # solution[0] = y0 exactly
    assert bool(torch.isfinite(sol).all())
    i64 = sc.increments(r64, z0)
    tol, d32 = ref.bound(sc.increments(r32, z0), i64, floor)
    err = rel_l2(sc.increments(sol, z0), i64)
    record(f"stacks.{case}.d32", d32)
    record(f"stacks.{case}.hip", err)
    print(f"{case}: float32 restatement {d32:.3e}, HIP {err:.3e}, bound {tol:.3e}, steps {counts} (oracle {c64})")
    assert err <= tol, (case, err, d32, tol)
    for j in range(i64.shape[0]):    # ... and every frame on its own: a late frame cannot hide an early one
        e_j = rel_l2(sc.increments(sol, z0)[j], i64[j])
        assert e_j <= ref.bound(sc.increments(r32, z0)[j], i64[j], floor)[0], (case, j, e_j)
    if adaptive:
        assert counts == c64, (case, counts, c64)

    again, counts_again = sc.device_forward(cuda, spec, f)
    assert torch.equal(again, sol) and counts_again == counts, case    # bitwise reproducible

    batch = z0.shape[0]
    if batch > 1:
        perm = torch.arange(batch).roll(1)
        moved, counts_moved = sc.device_forward(cuda, spec, f, z0=z0[perm].contiguous())
        if adaptive:
            e_perm = rel_l2(sc.increments(moved, z0[perm]), sc.increments(sol[:, perm.to(sol.device)], z0[perm]))
            record(f"stacks.{case}.rotated", e_perm)
            assert counts_moved == counts and e_perm <= sc.DOPRI5_FLOOR, (case, counts_moved, counts, e_perm)
        else:
            assert torch.equal(moved, sol[:, perm.to(sol.device)]), case    # samples are independent, bit for bit


@pytest.mark.parametrize("case", list(sc.BACKWARD_CASES))
def test_gradients_match_the_float64_oracle(cuda, case):
    """Gradients of z0, every weight and every bias: float64 autograd through the oracle's solver ("discrete"), or the oracle's adjoint
    ("adjoint"); each third of a 192-channel axis of a weight gradient also on its own."""
    spec, g64, margin, c64, g32 = _backward_reference(case)
    if spec["act"] == "relu":
        assert margin >= 0.5, margin    # kink-free: a condition on the reference alone
    got, counts = sc.device_backward(cuda, spec)
    assert got.keys() == g64.keys(), (sorted(got), sorted(g64))
    if counts is not None:
        assert counts == c64, (case, counts, c64)
    failed = []
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), (case, name)
        for suffix, cut in [("", lambda t: t)] + list(sc.third_views(name, g64[name]).items()):
            a64 = cut(g64[name])
            assert float(a64.abs().max()) > 0.0, (case, name + suffix)
            tol, d32 = ref.bound(cut(g32[name]), a64, sc.GRAD_FLOOR)
            err = rel_l2(cut(g), a64)
            record(f"stacks.{case}.{name}{suffix}.d32", d32)
            record(f"stacks.{case}.{name}{suffix}.hip", err)
            print(f"{case} {name}{suffix}: float32 restatement {d32:.3e}, HIP {err:.3e}, bound {tol:.3e}")
            if not err <= tol:
                failed.append((name + suffix, err, d32, tol))
    assert not failed, (case, failed)
