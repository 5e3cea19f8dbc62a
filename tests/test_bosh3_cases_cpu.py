"""The bosh3 cases (tests/_bosh3_cases.py) checked on the CPU, references alone: every condition test_hip_bosh3.py relies on is proved
here from the restatement (tests/_adaptive_ref.py) in float64 and float32, so that a device failure cannot be the case's fault.

  counts      float32 and float64 take the same (nfe, accepted, rejected); nfe = 2 + 3 attempts (1 + 3 attempts with first_step)
  margins     every error ratio is at least 3 % away from 1 in both precisions: a fp32 implementation that sums in another order decides
              every attempt the same way
  R3          rejects at least one step;  R1: an accepted step with two output times and one with none;  T2: decreasing t
  bounds      4 x d32 (the float32 restatement's own rel-L2 distance from the float64 one) is below the floor of the stack family
              (_solver_stack_cases.DOPRI5_FLOOR for trajectory increments, GRAD_FLOOR for gradient tensors): the floor is the bound
  nothing is all zero: every frame's increment, every gradient tensor
  backward    the stacks are kink-free: the smallest hidden pre-activation stays >= 0.1 away from 0 on every attempt
  adjoint     both norms on every backward stack: float32 and float64 take the same counts in the backward solves, with the same 3 %
              margin on every error ratio; the mixed norm takes other steps than the seminorm somewhere (the parameter block steers)
  bosh3 is not dopri5: on the vigorous fixture the two restatements differ by >= 1e-5 at these tolerances"""
import pytest
import torch

import _bosh3_cases as bc
import _convgru_ref as cref
import _solver_stack_cases as sc
from conftest import rel_l2, vigorous_case


@pytest.fixture(scope="module")
def forward_refs():
    out = {}
    for name in bc.FORWARD:
        spec = bc.forward_spec(name)
        out[name] = (spec, bc.forward_reference(spec, torch.float64), bc.forward_reference(spec, torch.float32))
    return out


@pytest.mark.parametrize("name", sorted(bc.FORWARD))
def test_forward_case_conditions(forward_refs, name):
    spec, (r64, s64), (r32, s32) = forward_refs[name]
    assert bc.counts(s64) == bc.counts(s32)
    assert s64["nfe"] == 2 + 3 * (s64["n_accept"] + s64["n_reject"])
    for st in (s64, s32):
        assert all(abs(r - 1.0) >= 0.03 for r in st["ratios"]), st["ratios"]
    i64, i32 = sc.increments(r64, spec["z0"]), sc.increments(r32, spec["z0"])
    tol, d32 = cref.bound(i32, i64, sc.DOPRI5_FLOOR)
    print(name, "counts", bc.counts(s64), "outputs per step", bc.outputs_per_step(spec, s64), "d32", d32)
    assert tol == sc.DOPRI5_FLOOR
    for j in range(i64.shape[0]):
        assert float(i64[j].norm()) > 1e-2 * float(spec["z0"].norm()), j   # every frame has moved
        assert cref.bound(i32[j], i64[j], sc.DOPRI5_FLOOR)[0] == sc.DOPRI5_FLOOR


def test_the_cases_cover_what_they_are_there_for(forward_refs):
    spec, (_, s64), _ = forward_refs["R3"]
    assert s64["n_reject"] >= 1
    spec, (_, s64), _ = forward_refs["R1"]
    per = bc.outputs_per_step(spec, s64)
    assert max(per) >= 2 and min(per) == 0 and sum(per) == len(spec["t"]) - 1
    spec, _, _ = forward_refs["T2"]
    assert bool((spec["t"][1:] < spec["t"][:-1]).all()) and spec["final_act"] and spec["act"] == "tanh"
    assert {tuple(forward_refs[n][0]["z0"].shape[:2]) for n in ("R1", "R3", "W2")} == {(1, 64), (3, 64), (2, 128)}
    assert all(3 <= len(forward_refs[n][0]["t"]) <= 5 for n in forward_refs)


@pytest.mark.parametrize("name", sorted(bc.BACKWARD))
def test_backward_case_conditions(name):
    spec = bc.backward_spec(name)
    g64, m64, s64 = bc.backward_reference(spec, torch.float64)
    g32, m32, s32 = bc.backward_reference(spec, torch.float32)
    assert bc.counts(s64) == bc.counts(s32) and s64["n_accept"] >= 2
    assert s64["nfe"] == 1 + 3 * (s64["n_accept"] + s64["n_reject"])
    for st in (s64, s32):
        assert all(abs(r - 1.0) >= 0.03 for r in st["ratios"]), st["ratios"]
    assert min(m64, m32) >= 0.1, (m64, m32)
    for k in g64:
        tol, d32 = cref.bound(g32[k], g64[k], sc.GRAD_FLOOR)
        print(name, k, "d32", d32)
        assert tol == sc.GRAD_FLOOR and float(g64[k].norm()) > 0
    if name == "G64":   # the reverse sweep meets a step with two outputs (their dense-output weights add up in one seed)
        assert max(bc.outputs_per_step(spec, s64)) >= 2


def test_bosh3_and_dopri5_differ_on_the_vigorous_fixture():
    from oracle import reference_modules as rm
    import _adaptive_ref as ar
    sd, z0, t, _ = vigorous_case()
    ws, bs = rm.split_convnet_state(sd, "gradient_net.")
    f = rm.ode_func([w.double() for w in ws], [b.double() for b in bs])
    with torch.no_grad():
        a = ar.odeint(f, z0.double(), t, method="bosh3", **bc.TOL)
        b = ar.odeint(f, z0.double(), t, method="dopri5", **bc.TOL)
    d = rel_l2(a[-1], b[-1])
    print("bosh3 vs dopri5 on traj_vig, last frame:", d)
    assert d >= 1e-5


def test_adjoint_case_conditions():
    differs = False
    for name in sorted(bc.BACKWARD):
        spec = bc.backward_spec(name)
        per_norm = {}
        for norm in ("mixed", "seminorm"):
            g64, s64 = bc.adjoint_reference(spec, torch.float64, norm)
            g32, s32 = bc.adjoint_reference(spec, torch.float32, norm)
            assert bc.counts(s64) == bc.counts(s32) and s64["n_accept"] >= len(spec["t"]) - 1
            for st in (s64, s32):
                assert all(abs(r - 1.0) >= 0.03 for r in st["ratios"]), (name, norm, st["ratios"])
            for k in g64:
                assert float(g64[k].norm()) > 0
                print(name, norm, k, "d32", cref.bound(g32[k], g64[k], sc.GRAD_FLOOR)[1])
            per_norm[norm] = bc.counts(s64)
        differs = differs or per_norm["mixed"] != per_norm["seminorm"]
    assert differs
