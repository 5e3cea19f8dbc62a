"""The fixed-grid tableau proves itself without a device.

tests/fixed_tableau_check.cpp includes ode-rl_amd/csrc/fixed_tableau.h -- the one place the euler / midpoint / rk4 (3/8 rule)
coefficients and the forward, reverse-sweep and adjoint plans derived from them live -- and applies the plans to y' = lambda y in
double, as the conv epilogues would.  Compared, to 1e-6 relative (the only error is the fp32 rounding of a few coefficients,
<= 2^-24 each), for z = h lambda in [-1, 1]:
  forward   y1 = R(z) y
  reverse   dy1/dy0 = R(z), dy1/dlambda = sum_s gk_s x_s = h R'(z) y
  adjoint   a_next = R(z) a, and sum_s scales_s A_s Y_s against the same sum formed directly from the tableau's stage
            polynomials, sum_s h b_s P_s(z) P_s(-z) y1 a: the adjoint is optimise-then-discretise, so its parameter sum equals
            h R'(z) y only up to the method's order (Euler: h (1 + z) y against h y), not to 1e-6
and the structural rules: zero weights give no source or target, at most four targets, the target order the drivers rely on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixed_tableau_plans_reproduce_the_methods(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "fixed_tableau_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "fixed_tableau_check.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "fixed_tableau: ok" in res.stdout, res.stdout + res.stderr
