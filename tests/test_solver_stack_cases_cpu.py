"""Conditions on the REFERENCE of the solver-stack cases (tests/_solver_stack_cases.py), checked without a GPU, so that the bounds of
tests/test_hip_solver_stacks.py mean what they say:

  * for every case 4 * d32 <= the floor of its family (d32: the float32 restatement's distance from the float64 one), so that the
    floor -- 3e-6 fixed grid, 5e-5 dopri5, 1e-4 gradients -- is the effective bound of max(4 * d32, floor);
  * the ReLU stacks of the backward cases are kink-free (margin >= 0.5);
  * for dopri5 the float32 and the float64 oracle take the same (n_accept, n_reject), with n_accept >= 3, and at least one forward
    case rejects a step;
  * no float64 reference tensor is all zero (also not a third of a 192-channel weight gradient).

A seed that fails one of these is replaced by another seed; nothing is widened."""
import pytest
import torch

import _solver_stack_cases as sc
from conftest import rel_l2

_CACHE = {}


def _forward(name):
    if name not in _CACHE:
        stack = sc.FORWARD_CASES[name][0]
        if ("stack", stack) not in _CACHE:
            _CACHE[("stack", stack)] = sc.forward_stack(stack)
        spec = sc.forward_case(name, {stack: _CACHE[("stack", stack)]})
        _CACHE[name] = (spec, sc.forward_reference(spec, torch.float64), sc.forward_reference(spec, torch.float32))
    return _CACHE[name]


def _backward(name):
    if name not in _CACHE:
        spec = sc.backward_case(name)
        _CACHE[name] = (spec, sc.backward_reference(spec, torch.float64), sc.backward_reference(spec, torch.float32))
    return _CACHE[name]


def test_the_tables_hold_the_cases_the_kernels_need():
    """Each stack reaches the kernel its row names: what launch_conv (csrc/conv_q4.hip) does with the LAST layer's shape."""
    wino3 = (16, 32, 48, 64, 128)   # launch_wino takes a 3x3 layer of these input widths; every other one runs a direct kernel
    for name, (channels, ks, _, _, batch, _, _, _, _) in sc.FORWARD_STACKS.items():
        assert all(c % 32 == 0 for c in channels) and channels[0] == channels[-1], name
        if ks == 3:
            assert channels[-2] not in wino3, name
    assert sc.FORWARD_STACKS["F5"][4] * (128 // 32) * 2 > 256    # conv_ring_kernel<5,1,2,2>
    assert sc.FORWARD_STACKS["F4"][4] * (32 // 32) * 2 <= 256    # conv_ring_kernel<5,1,4>
    for name, (channels, _, _, _, _) in sc.BACKWARD_STACKS.items():
        assert all(c % 64 == 0 for c in channels) and channels[0] == channels[-1] and 192 in channels, name
    assert {m for s, m, _ in sc.FORWARD_CASES.values() if s == "F1"} == {"euler", "midpoint", "rk4", "dopri5"}
    assert sum(1 for _, _, dec in sc.FORWARD_CASES.values() if dec) == 4


@pytest.mark.parametrize("case", list(sc.FORWARD_CASES))
def test_forward_reference_conditions(case):
    spec, (r64, c64), (r32, c32) = _forward(case)
    z0 = spec["z0"]
    floor = sc.DOPRI5_FLOOR if spec["method"] == "dopri5" else sc.FIXED_FLOOR
    i64, i32 = sc.increments(r64, z0), sc.increments(r32, z0)
    assert torch.equal(r64[0], z0.double())
    for frame in i64:
        assert float(frame.abs().max()) > 0.0
    d32 = rel_l2(i32, i64)
    assert 4.0 * d32 <= floor, (case, d32)
    moved = float(i64[-1].norm() / z0.double().norm())
    assert 0.3 <= moved <= 3.0, (case, moved)    # one unit of time changes the state by order 1
    if spec["method"] == "dopri5":
        assert c32 == c64 and c64[0] >= 3, (case, c64, c32)


def test_a_forward_case_rejects_a_step():
    rejecting = [c for c, (_, m, _) in sc.FORWARD_CASES.items() if m == "dopri5" and _forward(c)[1][1][1] >= 1]
    assert rejecting, "no dopri5 case rejects a step"


@pytest.mark.parametrize("case", list(sc.BACKWARD_CASES))
def test_backward_reference_conditions(case):
    spec, (g64, margin, c64), (g32, _, c32) = _backward(case)
    if spec["act"] == "relu":
        assert margin >= 0.5, (case, margin)
    if spec["method"] == "dopri5":
        assert c32 == c64 and c64[0] >= 3, (case, c64, c32)
    n_conv = len(spec["channels"]) - 1
    assert sorted(g64) == sorted(["z0"] + [f"w{i}" for i in range(n_conv)] + [f"b{i}" for i in range(n_conv)])
    n_views = 0
    for name, a64 in g64.items():
        parts = [("", lambda t: t)] + list(sc.third_views(name, a64).items())
        n_views += len(parts) - 1
        for suffix, cut in parts:
            assert float(cut(a64).abs().max()) > 0.0, (case, name + suffix)
            d32 = rel_l2(cut(g32[name]), cut(a64))
            assert 4.0 * d32 <= sc.GRAD_FLOOR, (case, name + suffix, d32)
    assert n_views >= 6, (case, n_views)    # every stack has 192-channel axes
