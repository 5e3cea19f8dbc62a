"""The two drivers of the seminorm dopri5 adjoint at sizes that take seconds: the device-steered controller on the adaptive persistent
walk (csrc/adjoint_device.hip) against the host-driven loop (csrc/adjoint_dopri5.hip).  Both read one slot geometry
(csrc/adjoint_layout.h); the full-size comparison is tests/test_hip_baseline_configs.py (B = 64, T = 10).

Kink-free 64-channel dynamics (tests/test_hip_backward.py::_kink_free: no pre-activation near a ReLU kink, so no mask element can flip
between two correct fp32 paths), t = [0.5, 0.55, 0.6], rtol = atol = 1e-5.  Batch 2 runs the sixteen-workgroup walk, batch 17 the
four-workgroup one.  Bounds are those of test_config2_full_size_device_controller_equals_host_loop: forward bitwise, two device runs
bitwise, equal (nfe, n_accept, n_reject), every gradient rel-L2 <= 1e-6 between the paths.

Two paths that share a wrong geometry would still agree with each other, so batch 2 is also held against the oracle's adjoint with the
bound test_config2_batch64_adjoint_against_the_oracle uses for these dynamics, grid and tolerances: every gradient <= 1e-4, the
accepted-step count within 2 (at rtol 1e-5 the error estimate sits at fp32 round-off and depends on the convolution's summation
order)."""
import os

import pytest
import torch

from conftest import record, rel_l2
from test_hip_backward import _kink_free

pytestmark = pytest.mark.gpu

T_GRID = [0.5, 0.55, 0.6]
RTOL = ATOL = 1e-5


def _needs_device_path():
    if os.environ.get("ODEHIP_PERSISTENT") == "0" or os.environ.get("ODEHIP_ADJOINT_DEVICE") == "0":
        pytest.skip("needs the device-controlled adjoint")


def _inputs(batch):
    f, sd = _kink_free()
    g = torch.Generator().manual_seed(100 + batch)
    z0 = torch.randn(batch, 64, 16, 16, generator=g) * 0.5
    t = torch.tensor(T_GRID, dtype=torch.float64)
    gout = torch.randn(len(T_GRID), batch, 64, 16, 16, generator=g)
    return f, sd, z0, t, gout


def _adjoint_step(f, z0, t, gout, **adjoint_options):
    import ode_rl_amd
    f.zero_grad()
    z = z0.clone().requires_grad_(True)
    sol = ode_rl_amd.odeint_adjoint(f, z, t, rtol=RTOL, atol=ATOL, method="dopri5", adjoint_options={"norm": "seminorm", **adjoint_options})
    fwd = dict(ode_rl_amd.last_stats)
    sol.backward(gout)
    st = dict(ode_rl_amd.last_adjoint_stats)
    return sol.detach().clone(), z.grad.clone(), [p.grad.clone() for p in f.parameters()], fwd, st


def _on_host_loop(fn):
    os.environ["ODEHIP_ADJOINT_DEVICE"] = "0"
    try:
        return fn()
    finally:
        os.environ.pop("ODEHIP_ADJOINT_DEVICE")


@pytest.mark.parametrize("batch", [2, 17])
def test_device_controller_equals_host_loop(cuda, batch):
    _needs_device_path()
    f, _, z0, t, gout = _inputs(batch)
    f, z0, gout = f.to(cuda), z0.to(cuda), gout.to(cuda)
    dev = _adjoint_step(f, z0, t, gout)
    dev2 = _adjoint_step(f, z0, t, gout)
    host = _on_host_loop(lambda: _adjoint_step(f, z0, t, gout))
    # the forward solve is the same code in both runs
    assert torch.equal(dev[0], host[0]) and dev[3]["nfe"] == host[3]["nfe"]
    # deterministic: bitwise
    assert torch.equal(dev[1], dev2[1]) and all(torch.equal(a, b) for a, b in zip(dev[2], dev2[2]))
    # one interval = one fresh solve: 2 evaluations for the initial step + 6 per attempted step
    for st in (dev[4], host[4]):
        assert st["nfe"] == 2 * (len(t) - 1) + 6 * (st["n_accept"] + st["n_reject"]) and st["n_accept"] >= len(t) - 1
    assert (dev[4]["nfe"], dev[4]["n_accept"], dev[4]["n_reject"]) == (host[4]["nfe"], host[4]["n_accept"], host[4]["n_reject"]), (dev[4], host[4])
    record(f"adjoint_paths.B{batch}.n_accept", dev[4]["n_accept"])
    record(f"adjoint_paths.B{batch}.n_reject", dev[4]["n_reject"])
    errs = [record(f"adjoint_paths.B{batch}.dev_vs_host.grad_z0", rel_l2(dev[1], host[1]))]
    errs += [record(f"adjoint_paths.B{batch}.dev_vs_host.grad_p{i}", rel_l2(a, b)) for i, (a, b) in enumerate(zip(dev[2], host[2]))]
    print(f"batch {batch}: stats {dev[4]}, dev vs host {errs}")
    assert max(errs) <= 1e-6, errs
    assert all(bool(torch.isfinite(g).all()) for g in [dev[1]] + dev[2])


def test_both_paths_against_the_oracle(cuda):
    _needs_device_path()
    from oracle import reference_modules as rm
    from oracle import torchdiffeq_ref
    batch = 2
    f, sd, z0, t, gout = _inputs(batch)
    ws, bs = rm.split_convnet_state(sd, "gradient_net.")
    ws = [w.clone().requires_grad_(True) for w in ws]
    bs = [b.clone().requires_grad_(True) for b in bs]
    stats = {}
    _, ref_gz, ref_gp = torchdiffeq_ref.odeint_adjoint(rm.ode_func(ws, bs), z0, t, ws + bs, gout, rtol=RTOL, atol=ATOL, method="dopri5",
                                                       stats=stats, adjoint_norm="seminorm")
    f, z0, gout = f.to(cuda), z0.to(cuda), gout.to(cuda)
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    for path in ("device", "host"):
        got = _adjoint_step(f, z0, t, gout) if path == "device" else _on_host_loop(lambda: _adjoint_step(f, z0, t, gout))
        assert abs(got[4]["n_accept"] - stats["n_accept"]) <= 2, (got[4], stats)
        errs = [record(f"adjoint_paths.B{batch}.{path}_vs_oracle.grad_z0", rel_l2(got[1], ref_gz))]
        for i, (c, gw, gb) in enumerate(zip(convs, ref_gp[:5], ref_gp[5:])):
            errs += [record(f"adjoint_paths.B{batch}.{path}_vs_oracle.grad_w{i}", rel_l2(c.weight.grad, gw)),
                     record(f"adjoint_paths.B{batch}.{path}_vs_oracle.grad_b{i}", rel_l2(c.bias.grad, gb))]
        print(f"{path} vs oracle: {errs}")
        assert max(errs) <= 1e-4, (path, errs)


def test_too_few_slots_is_the_same_error_on_both_paths(cuda):
    """Three output times need two accepted steps; max_accept = 1 leaves room for one."""
    _needs_device_path()
    f, _, z0, t, gout = _inputs(2)
    f, z0, gout = f.to(cuda), z0.to(cuda), gout.to(cuda)
    with pytest.raises(ValueError, match="more than max_accept") as dev:
        _adjoint_step(f, z0, t, gout, max_accept=1)
    with pytest.raises(ValueError, match="more than max_accept") as host:
        _on_host_loop(lambda: _adjoint_step(f, z0, t, gout, max_accept=1))
    assert str(dev.value) == str(host.value), (str(dev.value), str(host.value))
