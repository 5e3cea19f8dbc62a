"""The weight-gradient paths of csrc/wgrad*.hip that no other test runs, against float64 autograd on the CPU.

  * the direct fp32 kernels behind ODEHIP_WGRAD_WINO=0 / ODEHIP_WGRAD_WINO5=0 (wgrad_tile_kernel<3,0,3> with wgrad_reduce_kernel<4>; the
    three 5x5 parts with wgrad_reduce_kernel<1>).  The library reads both switches once per process, so every case runs in a child
    process (tests/_wgrad_worker.py), once per environment: "default" and "off".
  * slab counts batch * esplit of 4 .. 68: every tail predicate of slab_sum4_kernel and wgrad_reduce_kernel<4> (section A1).
  * stacks with a 128-channel hidden layer: two steps of the co0 and ci0 tile loops (A4).
  * ConvGRU cells with input_dim != hidden_dim (the halves of the two weight gradients sit at channel offset input_dim, compared
    separately so that a misplaced half cannot be averaged away) and with kernel sizes 3 and 1 (B).

Bound (tests/_convgru_ref.py::bound): per gradient tensor, d32 = rel-L2 of the float32 restatement from the float64 one on the same
inputs; the HIP result must be within max(4 * d32, 1e-4) of the float64 result (1e-4: the project's gradient bound).  The dynamics are
kink-free (ReLU margin >= 0.5 in the float64 restatement, asserted), so the gradient is a smooth function of the inputs.

bf16 compute mode: hip_ops._bf16_cell_ok rejects (128, 64, 5) (input_dim + hidden_dim > 128), so the per-step driver must fall back to
the fp32 path (same bound as above) and the whole-sequence driver must reject the cell with its clean error."""
import os
import subprocess
import sys

import pytest
import torch

import _convgru_ref as ref
import _wgrad_cases as wc
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

BOTH, DEFAULT = ("default", "off"), ("default",)
ENVS = {"default": {}, "off": {"ODEHIP_WGRAD_WINO": "0", "ODEHIP_WGRAD_WINO5": "0"}}

# name -> (n_layers, n_units, method, T, B, seed); every stack runs in both environments.  Seeds: the float64 restatement of each has
# a ReLU margin >= 0.5 (asserted below).
STACKS = {f"euler.T2.B{b}": (3, 64, "euler", 2, b, 40 + b) for b in (1, 2, 3, 4, 5, 9, 13, 17)}   # n_eval = 1, esplit = 4: 4 B slabs
STACKS["rk4.T4.B3"] = (3, 64, "rk4", 4, 3, 61)            # n_eval = 12 = esplit: 36 slabs, one evaluation per workgroup
STACKS["rk4.T3.B3"] = (3, 64, "rk4", 3, 3, 62)            # n_eval = 8 = esplit
STACKS["wide128.euler.T3.B2"] = (1, 128, "euler", 3, 2, 63)   # 64 -> 128, 128 -> 128, 128 -> 64

# name -> ((I, H, ks), driver, with h0, environments, compute dtype); B = 2, T = 2.  Cases of one shape share inputs and reference.
CELLS = {}
for _shape in ((128, 64, 5), (64, 128, 5)):
    for _driver in ("step", "rollout"):
        CELLS[f"{_driver}.I{_shape[0]}.H{_shape[1]}.k5"] = (_shape, _driver, True, BOTH, None)
CELLS["rollout.I128.H64.k5.no_h0"] = ((128, 64, 5), "rollout", False, BOTH, None)    # the state halves start at step 1
for _shape in ((64, 64, 3), (128, 64, 3), (64, 128, 1)):
    CELLS[f"step.I{_shape[0]}.H{_shape[1]}.k{_shape[2]}"] = (_shape, "step", True, DEFAULT, None)
CELLS["step.I128.H64.k5.bf16_mode"] = ((128, 64, 5), "step", True, DEFAULT, "bf16")
REJECTED = {"rollout.I128.H64.k5.bf16_mode": ((128, 64, 5), "rollout", True, DEFAULT, "bf16")}


SHAPE_SEEDS = {(128, 64, 5): 71, (64, 128, 5): 72, (64, 64, 3): 73, (128, 64, 3): 74, (64, 128, 1): 75}


def _cell_spec(name):
    (i, h, ks), driver, state, _, mode = {**CELLS, **REJECTED}[name]
    return wc.cell_case(i, h, ks, driver, 2, 2, SHAPE_SEEDS[(i, h, ks)], state=state, compute_dtype=mode, expect_rejected=name in REJECTED)


@pytest.fixture(scope="module")
def specs():
    out = {name: wc.stack_case(*args) for name, args in STACKS.items()}
    out.update({name: _cell_spec(name) for name in list(CELLS) + list(REJECTED)})
    return out


def _worker_run(env_name, specs, tmp_path_factory):
    d = tmp_path_factory.mktemp(f"wgrad_{env_name}")
    cases = {name: s for name, s in specs.items() if name in STACKS or env_name in {**CELLS, **REJECTED}[name][3]}
    torch.save(cases, d / "cases.pt")
    env = {k: v for k, v in os.environ.items() if k not in ("ODEHIP_WGRAD_WINO", "ODEHIP_WGRAD_WINO5")}
    env.update(ENVS[env_name])
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_wgrad_worker.py")
    try:
        r = subprocess.run([sys.executable, worker, str(d / "cases.pt"), str(d / "out.pt")], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"worker ({env_name}) timed out: {(e.stdout or b'')[-1500:]!r} {(e.stderr or b'')[-3000:]!r}")
    assert r.returncode == 0, f"worker ({env_name}) exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    return torch.load(d / "out.pt")


@pytest.fixture(scope="module")
def run_default(cuda, specs, tmp_path_factory):
    return _worker_run("default", specs, tmp_path_factory)


@pytest.fixture(scope="module")
def run_off(cuda, specs, tmp_path_factory):
    return _worker_run("off", specs, tmp_path_factory)


@pytest.fixture
def results(request):
    return lambda env_name: request.getfixturevalue("run_" + env_name)


_REFS = {}


def _reference(key, make):
    """The float64 and float32 restatements of a case, computed once and shared between the environments and drivers."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _compare(tag, got, r32, r64, views=None):
    """Every tensor of `got` against the bound; views: {suffix: function} of extra slices to compare on their own."""
    assert got.keys() == r64.keys(), (sorted(got), sorted(r64))
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), (tag, name)
    failed = []
    for name in got:
        parts = [("", lambda t: t)] + (list(views(name).items()) if views else [])
        for suffix, cut in parts:
            g, a32, a64 = cut(got[name]), cut(r32[name]), cut(r64[name])
            assert float(a64.abs().max()) > 0.0, (tag, name + suffix)
            tol, d32 = ref.bound(a32, a64, 1e-4)
            err = rel_l2(g, a64)
            record(f"wgrad.{tag}.{name}{suffix}.d32", d32)
            record(f"wgrad.{tag}.{name}{suffix}.hip", err)
            record(f"wgrad.{tag}.{name}{suffix}.bound", tol)
            print(f"{tag} {name}{suffix}: float32 restatement {d32:.3e}, HIP {err:.3e}, bound {tol:.3e}")
            if not err <= tol:
                failed.append((name + suffix, err, d32, tol))
    assert not failed, (tag, failed)


# ---- A. 3x3 dynamics stacks: odeint(...).backward(gout)
@pytest.mark.parametrize("case", list(STACKS))
@pytest.mark.parametrize("env_name", BOTH)
def test_stack_weight_gradients(results, specs, env_name, case):
    spec = specs[case]
    (r64, margin), (r32, _) = _reference(case, lambda: (wc.stack_reference(spec, torch.float64), wc.stack_reference(spec, torch.float32)))
    assert margin >= 0.5, margin   # kink-free: a condition on the reference alone
    _compare(f"{env_name}.{case}", results(env_name)[case]["grads"], r32, r64)


# ---- B. ConvGRU cells
def _cell_reference(name, specs):
    shape, _, state, _, _ = CELLS[name]
    spec = specs[name]
    return _reference(("cell", shape, state), lambda: (wc.cell_reference(spec, torch.float64), wc.cell_reference(spec, torch.float32)))


def _half_views(input_dim):
    def views(name):
        if name in ("conv_gates.0.weight", "conv_can.0.weight"):
            return {"[frame half]": lambda t: t[:, :input_dim], "[state half]": lambda t: t[:, input_dim:]}
        return {}
    return views


@pytest.mark.parametrize("env_name,case", [(e, c) for c, v in CELLS.items() if v[4] is None for e in v[3]])
def test_cell_weight_gradients(results, specs, env_name, case):
    r64, r32 = _cell_reference(case, specs)
    _compare(f"{env_name}.{case}", results(env_name)[case]["grads"], r32, r64, _half_views(CELLS[case][0][0]))


def test_cell_bf16_mode_falls_back_to_fp32_where_the_bf16_kernels_do_not_serve(results, specs):
    """(128, 64, 5) in bf16 compute mode: the bf16 ring kernels hold at most 128 input channels, so the per-step driver runs the fp32
    path (it meets the fp32 bound, which bf16 operands -- 8 mantissa bits -- cannot) and the sequence driver rejects the cell."""
    from ode_rl_amd import hip_ops
    assert not hip_ops._bf16_cell_ok(128, 64, 5)
    out = results("default")
    case = "step.I128.H64.k5.bf16_mode"
    r64, r32 = _cell_reference(case, specs)
    _compare(f"default.{case}", out[case]["grads"], r32, r64, _half_views(128))
    err = out["rollout.I128.H64.k5.bf16_mode"]["error"]
    assert err.startswith("ValueError: ConvGRU sequence: bf16 compute needs"), err
