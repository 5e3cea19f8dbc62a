"""The fp32 trajectory walks where a group of four workgroups carries two samples, or a second pass (csrc/conv_wino.hip:
wino_persist_kernel, wino_persist_d_kernel, wino_persist_v_kernel).  The loop of persist_walk<ADAPT> and persist_walk_v is

    for (b = group; b < batch; b += 2 * n_groups) { n_interleaved = b + n_groups < batch ? 2 : 1; ... }

with 64 groups: up to B = 64 a group walks one sample; up to 128 two, layer by layer in turn, through the same LDS and the same row
cursor; above 128 it runs the loop again.  Batches 65, 128 / 130, 129 and 193 are the smallest of each regime
(tests/_interleaved_cases.py says which groups do what at each).  Between two rows of a sample the group's LDS, U ring and accumulators
have carried the other sample, a row with dep_back waits for l - 1 of ITS sample, and a per-call table is read twice: so the rows that
matter are those of the saving forward, the reverse sweep, the adjoints and the adaptive tables, none of which the suite ran above
B = 64 before.

Every case of _interleaved_cases.CASES asserts
  1. the walk ran: odehip_persistent_trajectory_launches() grows by the driver's launches (fixed grids: 1 forward, 2 for a training
     step or an adjoint; adaptive: one per attempt, at least one), the strip kernel does not run (B > 64), the error word stays 0;
  2. trajectory, grad_z0, every weight and every bias gradient (and the adaptive solvers' nfe, n_accept, n_reject, accepted) equal,
     bit for bit, one launch per layer (odehip_set_persistent_trajectory(0)), which ran FIRST (a dopri5 training step is two
     algorithms, compared one by one: _check_dopri5_backward);
  3. every compared tensor is finite and nonzero; frame 0 is z0 and the last frame differs from z0 FOR EVERY SAMPLE (a norm over the
     batch would hide one stale sample out of 193);
  4. a second call gives the same bits (the cached table, the zeroed flag area, the staging ring).
The library's outputs are torch.empty: before every walk run, blocks of the outputs' sizes are filled with NaN and handed back to the
allocator.  That is best effort (nothing makes the allocator hand those blocks out next); what a never-written sample cannot pass is 3.
and, with the reference's outputs still alive in blocks of their own, 2.

Further: the two drivers of the adaptive adjoint against each other with the comparison of tests/test_hip_adjoint_paths.py; samples
{0, 63, 64, 127, 128, 192} of a B = 193 training step against the same six as a batch of six under one launch per layer (the per-layer
kernels index the sample by blockIdx.y and share nothing between samples: this check cannot go wrong alike with 2.); and the weight
and bias gradients of B = 129 -- slabs summed over all evaluations and samples, which 2. and the independence check cannot see wrong in
both paths alike -- against float64 autograd through the oracle on the CPU."""
import functools
import os

import pytest
import torch

import _interleaved_cases as ic
import _solver_stack_cases as sc
from conftest import record, rel_l2
from test_hip_adjoint_paths import _on_host_loop

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _persistent_on():
    return os.environ.get("ODEHIP_PERSISTENT", "1") != "0"


def _poison(*tensors):
    """Three NaN-filled blocks of every tensor's size go back to the allocator: the next outputs of these sizes are likely to start as
    NaN.  Best effort: the caching allocator promises nothing about which block it hands out."""
    for t in tensors:
        blocks = [torch.full_like(t, NAN) for _ in range(3)]
        torch.cuda.synchronize()
        del blocks


def _run(cuda, f, z0, t, go, driver, method, backward_persistent=None):
    """One library call (and its backward pass): ({name: tensor on the device}, stats of the call).  backward_persistent: what
    odehip_set_persistent_trajectory is given for the backward pass alone."""
    import ode_rl_amd
    kw = ic.solver_kwargs(driver, method)
    stats = {}
    if driver == "forward":
        with torch.no_grad():
            out = {"traj": ode_rl_amd.odeint(f, z0, t, method=method, **kw)}
    else:
        f.zero_grad()
        z = z0.detach().requires_grad_(True)
        sol = (ode_rl_amd.odeint_adjoint if driver == "adjoint" else ode_rl_amd.odeint)(f, z, t, method=method, **kw)
        if method in ic.ADAPTIVE:
            stats["forward"] = dict(ode_rl_amd.last_stats)
        if backward_persistent is None:
            sol.backward(go)
        else:
            lib = ode_rl_amd._lib.load()
            was = lib.odehip_set_persistent_trajectory(backward_persistent)
            try:
                sol.backward(go)
                torch.cuda.synchronize()
            finally:
                lib.odehip_set_persistent_trajectory(was)
        convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
        out = {"traj": sol.detach(), "grad_z0": z.grad}
        out.update({f"grad_w{i}": c.weight.grad for i, c in enumerate(convs)})
        out.update({f"grad_b{i}": c.bias.grad for i, c in enumerate(convs)})
        for c in convs:   # the next run must allocate gradients of its own
            c.weight.grad = c.bias.grad = None
        if driver == "adjoint" and method in ic.ADAPTIVE:
            stats["adjoint"] = dict(ode_rl_amd.last_adjoint_stats)
    if driver == "forward" and method in ic.ADAPTIVE:
        stats["forward"] = dict(ode_rl_amd.last_stats)
    torch.cuda.synchronize()
    return out, stats


def _counted(lib, fn):
    """(fn(), launches of the persistent walks, launches of the strip kernel)"""
    n0, s0 = lib.odehip_persistent_trajectory_launches(), lib.odehip_strip_walk_launches()
    res = fn()
    return res, lib.odehip_persistent_trajectory_launches() - n0, lib.odehip_strip_walk_launches() - s0


def _expected_launches(stack, driver, method):
    """What the driver launches: (count, exact)"""
    if method in ic.ADAPTIVE:
        return (2 if driver == "train" else 1), False   # one per attempt (+ the one-walk backward): at least
    if driver == "train" and ic.STACKS[stack][2]:
        return 1, True   # the reverse sweep over a Tanh head is not recorded (PersistScope::begin): the saving forward alone
    return (1 if driver == "forward" else 2), True


def _deterministic(stats):
    """The part of an adaptive call's stats that is arithmetic (`attempts_enqueued` is how far the host ran ahead: timing)."""
    fwd = {k: stats["forward"][k] for k in ("nfe", "n_accept", "n_reject", "accepted")} if "forward" in stats else None
    adj = {k: stats["adjoint"][k] for k in ("nfe", "n_accept", "n_reject")} if "adjoint" in stats else None
    return fwd, adj


def _assert_not_vacuous(name, out, z0):
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), (name, k, "not finite")
        assert float(v.abs().max()) > 0.0, (name, k, "all zero")
    traj = out["traj"]
    assert torch.equal(traj[0], z0), (name, "frame 0 is not z0")
    moved = (traj[-1] != z0).flatten(1).any(dim=1)
    assert bool(moved.all()), (name, "samples whose last frame is z0", (~moved).nonzero().flatten().tolist())
    if "grad_z0" in out:
        seen = (out["grad_z0"] != 0).flatten(1).any(dim=1)
        assert bool(seen.all()), (name, "samples without an input gradient", (~seen).nonzero().flatten().tolist())


def _assert_same_bits(name, tag, got, ref):
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        if not torch.equal(got[k], ref[k]):
            d = got[k] != ref[k]
            rows = d.flatten(2).any(dim=2).any(dim=0) if k == "traj" else (d.flatten(1).any(dim=1) if k == "grad_z0" else None)
            where = f"samples {rows.nonzero().flatten().tolist()[:16]}" if rows is not None else f"{int(d.sum())} elements"
            raise AssertionError(f"{name}: {k} differs from {tag} in {where}")


SAVED_VS_REINTEGRATED = 1e-5   # tests/test_hip_backward.py::test_dopri5_saving_forward_equals_reintegration, kink-free dynamics


def _check_dopri5_backward(cuda, lib, name, stack, f, z0, t, go):
    """A dopri5 training step is two algorithms: with the walk, the forward keeps the activations of the accepted steps and the backward
    is ONE walk over them; without it nothing is kept and the backward re-integrates.  The two round the stage-2 input of a step
    differently (tests/test_hip_backward.py::test_dopri5_saving_forward_equals_reintegration; beta21 = 1/5 -- bosh3's 1/2 is exact and
    its two paths agree bit for bit), so under odehip_set_persistent_trajectory(0) for the whole step the trajectory and the step
    sequence are equal bit for bit and the gradients are not, at any batch.  "One launch per layer" for each algorithm on its own:
      saved           the walk's forward, then the backward with the switch at 0: its recorded rows are replayed as ordinary launches
      re-integrating  ODEHIP_DOPRI5_SAVE=0: the whole step on the walks against the whole step with the switch at 0.
    Both sides of "saved" read the slots the walk's forward wrote, so a slot written wrongly for sample 64 or 128 would be wrong alike
    in both.  What ties them to a path that never saw those slots is the distance of the saved path's gradients from the
    re-integrating step under one launch per layer: every weight and bias gradient, and grad_z0 SAMPLE BY SAMPLE (the largest
    per-sample rel-L2), recorded for every case and, on the kink-free stack, where the two algorithms differ by round-off alone, held
    to the existing test's 1e-5.  (On the ReLU stack mask elements flip between them: 1e-4 .. 1e-3, recorded, not bounded.)"""
    def step(**kw):
        return _counted(lib, lambda: _run(cuda, f, z0, t, go, "train", "dopri5", **kw))

    def reintegrating(fn):
        os.environ["ODEHIP_DOPRI5_SAVE"] = "0"
        try:
            return fn()
        finally:
            os.environ.pop("ODEHIP_DOPRI5_SAVE")

    was = lib.odehip_set_persistent_trajectory(0)
    try:
        (ref, ref_stats), n_ref, _ = step()
        lib.odehip_set_persistent_trajectory(1)
        (saved_ref, _), n_fwd, s0 = step(backward_persistent=0)
        _poison(*ref.values())
        (got, stats), n_walk, s1 = step()
        _poison(*ref.values())
        (again, stats2), n_walk2, s2 = step()
        _poison(*ref.values())
        (re_got, re_stats), n_re, s3 = reintegrating(step)
    finally:
        lib.odehip_set_persistent_trajectory(was)
    print(f"{name}: persistent launches {n_walk} (forward alone {n_fwd}, re-integrating {n_re}), stats {_deterministic(stats)}")
    assert lib.odehip_persistent_error(0) == 0, "a capped wait of a persistent launch gave up"
    assert n_ref == 0 and s0 + s1 + s2 + s3 == 0
    if _persistent_on():
        assert n_fwd >= 1 and n_walk == n_fwd + 1 and n_walk2 == n_walk and n_re >= 2, (n_fwd, n_walk, n_walk2, n_re)
        assert stats["forward"]["saved"] and not re_stats["forward"]["saved"] and not ref_stats["forward"]["saved"]
    for out in (ref, saved_ref, got, re_got):
        _assert_not_vacuous(name, out, z0)
    assert stats["forward"]["n_accept"] >= ic.MIN_ACCEPT, stats
    # the forward: trajectory and step sequence of one launch per layer
    assert torch.equal(got["traj"], ref["traj"]) and _deterministic(stats) == _deterministic(ref_stats), (stats, ref_stats)
    # the one-walk backward over the kept activations against its rows as ordinary launches
    _assert_same_bits(name, "the backward as one launch per layer", got, saved_ref)
    _assert_same_bits(name, "the first call", again, got)
    assert _deterministic(stats2) == _deterministic(stats)
    # the re-integrating step on the walks against one launch per layer
    _assert_same_bits(name, "one launch per layer (re-integrating)", re_got, ref)
    assert _deterministic(re_stats) == _deterministic(ref_stats)
    # the saved path against the re-integrating step under one launch per layer: a reference that never read the walk's saved slots
    errs = {}
    for k in sorted(k for k in ref if k != "traj"):
        if k == "grad_z0":
            d, r = (got[k].double() - ref[k].double()).flatten(1).norm(dim=1), ref[k].double().flatten(1).norm(dim=1)
            errs[k] = float((d / r).max())
            print(f"{name}: grad_z0 of sample {int((d / r).argmax())} is the farthest from the re-integrating step")
        else:
            errs[k] = rel_l2(got[k], ref[k])
        record(f"interleaved.{name}.saved_vs_reintegrated.{k}", errs[k])
    print(f"{name}: saved path against the re-integrating step under one launch per layer {errs}")
    if stack == "kinkfree":
        assert max(errs.values()) <= SAVED_VS_REINTEGRATED, errs


@pytest.mark.parametrize("name", list(ic.CASES))
def test_walk_is_bit_identical_to_per_layer_launches(cuda, name):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    stack, driver, method, batch = ic.CASES[name]
    first, second, solo = ic.regime(batch)
    assert batch > ic.N_GROUPS and len(first) == 2, "the case leaves every group one sample"
    f = ic.func(stack).to(cuda)
    z0 = ic.z0(stack, batch).to(cuda)
    t = ic.times(method)
    go = None if driver == "forward" else ic.gout(stack, batch, len(t)).to(cuda)
    adaptive_adjoint = driver == "adjoint" and method in ic.ADAPTIVE
    if driver == "train" and method == "dopri5":
        return _check_dopri5_backward(cuda, lib, name, stack, f, z0, t, go)

    def run():
        call = lambda: _run(cuda, f, z0, t, go, driver, method)   # noqa: E731
        return _on_host_loop(call) if adaptive_adjoint else call()

    was = lib.odehip_set_persistent_trajectory(0)
    try:
        (ref, ref_stats), n_ref, _ = _counted(lib, run)
        assert n_ref == 0, "a persistent walk ran under odehip_set_persistent_trajectory(0)"
        lib.odehip_set_persistent_trajectory(1)
        _poison(*ref.values())
        (got, stats), n_walk, n_strip = _counted(lib, run)
        _poison(*ref.values())
        (again, stats2), n_walk2, n_strip2 = _counted(lib, run)
    finally:
        lib.odehip_set_persistent_trajectory(was)
    print(f"{name}: group 0 walks {first} then {second}, {solo} groups solo; persistent launches {n_walk}, stats {_deterministic(stats)}")
    # 1. the walk under test ran, the strip kernel did not, no wait gave up
    assert lib.odehip_persistent_error(0) == 0, "a capped wait of a persistent launch gave up"
    assert n_strip == 0 and n_strip2 == 0, "the host chose the strip walk above one sample per group"
    if _persistent_on():
        want, exact = _expected_launches(stack, driver, method)
        assert (n_walk == want and n_walk2 == want) if exact else (n_walk >= want and n_walk2 >= want), (n_walk, n_walk2, want)
    # 3. nothing compared is vacuous
    _assert_not_vacuous(name, ref, z0)
    _assert_not_vacuous(name, got, z0)
    if method in ic.ADAPTIVE:
        assert stats["forward"]["n_accept"] >= ic.MIN_ACCEPT, stats
        if adaptive_adjoint:
            assert stats["adjoint"]["n_accept"] >= ic.MIN_ACCEPT and stats["adjoint"]["controller"] == "host", stats
    # 2. bit identity with one launch per layer
    _assert_same_bits(name, "one launch per layer", got, ref)
    assert _deterministic(stats) == _deterministic(ref_stats), (stats, ref_stats)
    # 4. and with itself
    _assert_same_bits(name, "the first call", again, got)
    assert _deterministic(stats2) == _deterministic(stats), (stats2, stats)


@pytest.mark.parametrize("name", ic.ADJOINT_CASES)
def test_device_steered_adjoint_equals_host_loop(cuda, name):
    """The comparison of tests/test_hip_adjoint_paths.py::test_device_controller_equals_host_loop, here with two samples per group and a
    second pass: the device-steered walk reads {first row, rows} again in the second pass, its rows carry relocatable pointers, dep_back
    and norm rows whose partials two samples of a group write in turn."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    stack, driver, method, batch = ic.CASES[name]
    f = ic.func(stack).to(cuda)
    z0 = ic.z0(stack, batch).to(cuda)
    t = ic.times(method)
    go = ic.gout(stack, batch, len(t)).to(cuda)
    n0, s0 = lib.odehip_persistent_trajectory_launches(), lib.odehip_strip_walk_launches()
    dev, dev_st = _run(cuda, f, z0, t, go, driver, method)
    _poison(*dev.values())
    dev2, dev2_st = _run(cuda, f, z0, t, go, driver, method)
    n_walk, n_strip = lib.odehip_persistent_trajectory_launches() - n0, lib.odehip_strip_walk_launches() - s0
    host, host_st = _on_host_loop(lambda: _run(cuda, f, z0, t, go, driver, method))
    assert lib.odehip_persistent_error(0) == 0, "a capped wait of a persistent launch gave up"
    assert n_strip == 0
    if _persistent_on() and os.environ.get("ODEHIP_ADJOINT_DEVICE") != "0":
        assert n_walk >= 2 and dev_st["adjoint"]["controller"] == "device", (n_walk, dev_st)
    assert host_st["adjoint"]["controller"] == "host", host_st
    _assert_not_vacuous(name, dev, z0)
    grads = sorted(k for k in dev if k != "traj")
    # the forward solve is the same code in both runs
    assert torch.equal(dev["traj"], host["traj"]) and dev_st["forward"]["nfe"] == host_st["forward"]["nfe"]
    # deterministic: bitwise
    assert all(torch.equal(dev[k], dev2[k]) for k in grads)
    # one interval = one fresh solve: 2 evaluations for the initial step + one per stage (dopri5's seventh is the next step's first) per attempt
    per_attempt = 6 if method == "dopri5" else 3
    a_dev, a_host = dev_st["adjoint"], host_st["adjoint"]
    for st in (a_dev, a_host):
        assert st["nfe"] == 2 * (len(t) - 1) + per_attempt * (st["n_accept"] + st["n_reject"]) and st["n_accept"] >= len(t) - 1
        assert st["n_accept"] >= ic.MIN_ACCEPT, st
    assert (a_dev["nfe"], a_dev["n_accept"], a_dev["n_reject"]) == (a_host["nfe"], a_host["n_accept"], a_host["n_reject"]), (a_dev, a_host)
    errs = [record(f"interleaved.{name}.dev_vs_host.{k}", rel_l2(dev[k], host[k])) for k in grads]
    print(f"{name}: stats {a_dev}, dev vs host {errs}")
    assert max(errs) <= 1e-6, errs


def test_samples_of_every_slot_and_pass_are_independent_of_the_batch(cuda):
    """rk4 training step at B = 193 on the walk; the six samples alone under one launch per layer."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    batch, idx = ic.INDEPENDENT_BATCH, list(ic.INDEPENDENT_SAMPLES)
    f = ic.func("relu").to(cuda)
    z0 = (ic.z0("relu", batch) * 1.25).to(cuda)   # not the inputs of the B = 193 cases above
    t = ic.times("rk4")
    go = ic.gout("relu", batch, len(t)).to(cuda)
    was = lib.odehip_set_persistent_trajectory(0)
    try:
        (six, _), n_six, _ = _counted(lib, lambda: _run(cuda, f, z0[idx].contiguous(), t, go[:, idx].contiguous(), "train", "rk4"))
        lib.odehip_set_persistent_trajectory(1)
        full_shapes = [torch.empty(len(t), batch, 64, 16, 16, device=cuda), torch.empty(batch, 64, 16, 16, device=cuda)]
        _poison(*full_shapes)
        del full_shapes
        (full, _), n_walk, n_strip = _counted(lib, lambda: _run(cuda, f, z0, t, go, "train", "rk4"))
    finally:
        lib.odehip_set_persistent_trajectory(was)
    assert lib.odehip_persistent_error(0) == 0 and n_six == 0 and n_strip == 0
    if _persistent_on():
        assert n_walk == 2
    _assert_not_vacuous("independence", full, z0)
    for j, b in enumerate(idx):
        assert torch.equal(full["traj"][:, b], six["traj"][:, j]), f"trajectory of sample {b}"
        assert torch.equal(full["grad_z0"][b], six["grad_z0"][j]), f"grad_z0 of sample {b}"


@functools.lru_cache(maxsize=None)
def _f64():
    spec = ic.f64_case()
    return (spec,) + ic.f64_reference(spec)


def test_gradients_of_a_two_pass_batch_against_float64_autograd(cuda):
    """Kink-free three-conv stack (_wgrad_cases.stack_case), B = 129, midpoint, two time points: trajectory increments within FIXED_FLOOR,
    grad_z0 and every weight and bias gradient within GRAD_FLOOR of float64 autograd through oracle.torchdiffeq_ref.
    Observed on an MI355X: increments 1.6e-7; grad_z0 3.5e-8, weights 4.5e-7 / 3.6e-7 / 2.4e-7, biases 4.0e-7 / 3.0e-7 / 1.4e-7."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    spec, ref_sol, ref, margin = _f64()
    assert margin > 0.5, margin
    f = ode_rl_amd.ODEFunc(64, 64, 1, 64, False, "relu", final_act=False)
    f.load_state_dict(spec["sd"])
    f = f.to(cuda)
    z0 = spec["z0"].to(cuda)
    _poison(torch.empty(len(spec["t"]), ic.F64_BATCH, 64, 16, 16, device=cuda), z0)
    (got, _), n_walk, n_strip = _counted(lib, lambda: _run(cuda, f, z0, spec["t"], spec["gout"].to(cuda), "train", spec["method"]))
    assert lib.odehip_persistent_error(0) == 0 and n_strip == 0
    if _persistent_on():
        assert n_walk == 2
    _assert_not_vacuous("float64", got, z0)
    inc = record("interleaved.f64.increment", rel_l2(sc.increments(got["traj"], spec["z0"]), sc.increments(ref_sol, spec["z0"])))
    print(f"B = {ic.F64_BATCH} {spec['method']}: trajectory increments {inc:.3e}")
    errs = {}
    for k in sorted(ref):
        assert float(ref[k].abs().max()) > 0.0, k
        errs[k] = record(f"interleaved.f64.grad.{k}", rel_l2(got[f"grad_{k}"], ref[k]))
        print(f"B = {ic.F64_BATCH} {spec['method']}: grad {k} {errs[k]:.3e}")
    assert inc <= sc.FIXED_FLOOR, inc
    assert max(errs.values()) <= sc.GRAD_FLOOR, errs
