"""The row-strip walk (wino_persist_strip_kernel): fixed-grid trajectories of a 64-channel stack whose batch gives every group of four
workgroups one sample.  A workgroup owns all 64 output channels of four rows, so every accumulator element sees the MFMA sequence of
the other walks and of the per-layer kernel, and the epilogue is the shared one: the strip walk must agree BIT FOR BIT with one
launch per layer (odehip_set_persistent_trajectory(0), the ODEHIP_PERSISTENT=0 path) and with the co-tile x image-half walk
(odehip_set_strip_walk(0), the ODEHIP_STRIP_WALK=0 path).  Every case asserts through odehip_strip_walk_launches that the strip kernel
really ran (and did not run when it was switched off).

Shapes: batches 17 and 20 (the first above the sixteen-workgroup walk's 16; 20 leaves the groups of several XCDs without a sample)
and 64 (every group busy: the headline's batch); three time points; two hidden layers, so plain rows follow a stage-combine row
and each other.  Boundary cases: an input that is nonzero only on the image border (the zero padding comes from the DMA's range check,
which a strip's six-row raw tile addresses differently) and one that is nonzero only in the halo rows between strips."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

T = (0.1, 0.25, 0.7)


def _func(act="relu", head=False, n_layers=2):
    import ode_rl_amd
    torch.manual_seed(5)
    f = ode_rl_amd.ODEFunc(64, 64, n_layers, 64, False, act, final_act=head)
    g = torch.Generator().manual_seed(31)
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():   # a scale of its own for every output and input channel: a swapped co block or ci quad cannot cancel
        for c in convs:
            co, ci = c.weight.shape[:2]
            c.weight.mul_((0.5 + torch.rand(co, generator=g))[:, None, None, None] * (0.5 + torch.rand(ci, generator=g))[None, :, None, None])
    return f


def _z0(batch, kind="random"):
    g = torch.Generator().manual_seed(200 + batch)
    z = torch.randn(batch, 64, 16, 16, generator=g) * 0.5
    if kind == "border":      # rows 0 and 15, columns 0 and 15
        m = torch.zeros(16, 16)
        m[0, :] = m[15, :] = 1.0
        m[:, 0] = m[:, 15] = 1.0
        z = z * m
    elif kind == "halo":      # the rows a strip reads from its neighbours, and the neighbours' rows next to them
        m = torch.zeros(16, 16)
        for r in (3, 4, 7, 8, 11, 12):
            m[r, :] = 1.0
        z = z * m
    return z


def _switches_on():
    return os.environ.get("ODEHIP_PERSISTENT", "1") != "0" and os.environ.get("ODEHIP_STRIP_WALK", "1") != "0"


def _solve(lib, f, z0, method, cuda, persistent, strip, train=False, gout=None):
    """([trajectory, gradients...], launches of the strip kernel) under the given switches."""
    import ode_rl_amd
    t = torch.tensor(T, dtype=torch.float64)
    was_p = lib.odehip_set_persistent_trajectory(persistent)
    was_s = lib.odehip_set_strip_walk(strip)
    try:
        n0 = lib.odehip_strip_walk_launches()
        if not train:
            with torch.no_grad():
                out = [ode_rl_amd.odeint(f, z0.to(cuda), t, method=method).clone()]
        else:
            f.zero_grad()
            zd = z0.to(cuda).requires_grad_(True)
            sol = ode_rl_amd.odeint(f, zd, t, method=method)
            sol.backward(gout.to(cuda))
            convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
            out = [sol.detach().clone(), zd.grad.clone()] + [c.weight.grad.clone() for c in convs] + [c.bias.grad.clone() for c in convs]
        torch.cuda.synchronize()
        return out, lib.odehip_strip_walk_launches() - n0
    finally:
        lib.odehip_set_strip_walk(was_s)
        lib.odehip_set_persistent_trajectory(was_p)


@functools.lru_cache(maxsize=None)
def _per_layer(method, batch, kind, act, head):
    """One launch per layer: the reference every walk is compared with, computed once per case."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    cuda = torch.device("cuda:0")
    out, n = _solve(lib, _func(act, head).to(cuda), _z0(batch, kind), method, cuda, 0, 1)
    assert n == 0
    return out[0]


def _check_forward(cuda, method, batch, kind="random", act="relu", head=False):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f = _func(act, head).to(cuda)
    z0 = _z0(batch, kind)
    layer = _per_layer(method, batch, kind, act, head)
    (halves,), n_halves = _solve(lib, f, z0, method, cuda, 1, 0)
    (strip,), n_strip = _solve(lib, f, z0, method, cuda, 1, 1)
    assert n_halves == 0, "the strip kernel ran although it was switched off"
    if _switches_on():
        assert n_strip >= 1, "the strip kernel did not run"
    assert torch.equal(strip[0].cpu(), z0)
    assert torch.isfinite(strip).all() and float(strip[-1].abs().max()) > 0
    assert torch.equal(strip, layer)
    assert torch.equal(strip, halves)


@pytest.mark.parametrize("batch", [17, 20, 64])
@pytest.mark.parametrize("method", ["rk4", "midpoint", "euler"])
def test_forward_is_bit_identical_to_per_layer_launches_and_to_the_other_walk(cuda, method, batch):
    _check_forward(cuda, method, batch)


def test_forward_and_backward_are_bit_identical_to_per_layer_launches(cuda):
    """A training step at B = 17: the saving forward, then the reverse sweep with its ReLU-mask and target rows."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f = _func().to(cuda)
    z0 = _z0(17)
    gout = torch.randn(len(T), 17, 64, 16, 16, generator=torch.Generator().manual_seed(7))
    layer, n_layer = _solve(lib, f, z0, "rk4", cuda, 0, 1, train=True, gout=gout)
    strip, n_strip = _solve(lib, f, z0, "rk4", cuda, 1, 1, train=True, gout=gout)
    assert n_layer == 0
    if _switches_on():
        assert n_strip >= 2, "the saving forward and the reverse sweep did not both take the strip kernel"
    assert len(strip) == len(layer) == 2 + 2 * sum(isinstance(m, torch.nn.Conv2d) for m in f.gradient_net)
    for a, b in zip(strip, layer):
        assert float(a.abs().max()) > 0
        assert torch.equal(a, b)


def test_tanh_dynamics_with_a_tanh_head(cuda):
    _check_forward(cuda, "rk4", 17, act="tanh", head=True)


@pytest.mark.parametrize("kind", ["border", "halo"])
def test_boundary_and_halo_rows(cuda, kind):
    _check_forward(cuda, "rk4", 17, kind=kind)
