"""GPU parity of Tanh dynamics: hidden Tanh layers (create_convnet's nonlinear='tanh') and the Tanh head (final_act=True) on
every path that evaluates a conv stack -- f, the fixed-grid solvers on each kernel path, the persistent walks, dopri5 (sync and
async), discretise-then-optimise gradients, odeint_adjoint, decreasing t, the encoder -- against the reference fixture
(tests/golden/tanh.npz) and the oracle.  Tanh has no kink, so the gradient comparisons need no margin conditions."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, procedural_state_dict, procedural_tensor, rel_l2

pytestmark = pytest.mark.gpu

STACKS = {   # name -> (ODEFunc arguments, nonlinear, final_act)
    "A_tanh": ((64, 64, 3, 64), "tanh", False),
    "A_head": ((64, 64, 3, 64), "relu", True),
    "A_tanh_head": ((64, 64, 3, 64), "tanh", True),
    "V_tanh_head": ((128, 128, 2, 64), "tanh", True),
    "S_tanh_head": ((32, 32, 3, 32), "tanh", True),
}


def _func(name, seed=0, kink_free=False):
    import ode_rl_amd
    args, act, head = STACKS[name]
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(*args, False, act, final_act=head)
    if kink_free:   # ReLU hidden layers: pre-activations far from 0 (tests/test_hip_backward.py), so no mask can flip
        convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
        with torch.no_grad():
            for c in convs[:-1]:
                c.weight.mul_(0.15)
                c.bias.copy_(torch.where(torch.arange(c.out_channels) % 2 == 0, 2.5, -2.5))
    return f


def _oracle_f(f, params=None, backwards=False):
    """The dynamics of an ODEFunc as a closure on (optionally grad-requiring copies of) its parameters."""
    net = list(f.gradient_net)
    head = isinstance(net[-1], torch.nn.Tanh)
    convs = [m for m in net if isinstance(m, torch.nn.Conv2d)]
    act = torch.tanh if any(isinstance(m, torch.nn.Tanh) for m in (net[:-1] if head else net)) else torch.relu
    if params is None:
        params = [c.weight.detach().cpu() for c in convs] + [c.bias.detach().cpu() for c in convs]
    n = len(convs)
    ws, bs = params[:n], params[n:]

    def fn(t, y):
        x = y
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
            if i < n - 1:
                x = act(x)
        if head:
            x = torch.tanh(x)
        return -x if backwards else x
    return fn


def _leaf_params(f):
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    return [c.weight.detach().cpu().clone().requires_grad_(True) for c in convs] + \
           [c.bias.detach().cpu().clone().requires_grad_(True) for c in convs]


def _param_grads(f):
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    return [c.weight.grad for c in convs] + [c.bias.grad for c in convs]


@pytest.mark.parametrize("key,args,act,head,seed", [("fA_tanh", (64, 64, 3, 64), "tanh", False, 40),
                                                    ("fA_head", (64, 64, 3, 64), "relu", True, 41),
                                                    ("fV_head", (128, 128, 2, 64), "tanh", True, 42)])
def test_f_matches_reference_fixture(cuda, key, args, act, head, seed):
    """Procedural weights and input (rebuilt bit for bit from tests/golden/make_golden_tanh.py's seeds) against the reference's f."""
    import ode_rl_amd
    g = load_golden("tanh.npz")
    f = ode_rl_amd.ODEFunc(*args, False, act, final_act=head)
    f.load_state_dict(procedural_state_dict(f.state_dict(), seed))
    f = f.to(cuda)
    y = procedural_tensor((1, args[0], 16, 16), seed + 100, -1, 1).to(cuda)
    ref = torch.from_numpy(g[key + ".out"])
    with torch.no_grad():
        assert rel_l2(f(0.0, y), ref) <= 5e-6
        assert rel_l2(f(0.0, y, backwards=True), -ref) <= 5e-6


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("name,batch,T", [("A_tanh", 64, 10), ("A_tanh_head", 4, 6), ("V_tanh_head", 2, 4), ("S_tanh_head", 3, 4)],
                         ids=["persistent", "walk16", "wide", "per_layer"])
def test_fixed_grid_matches_oracle(cuda, method, name, batch, T):
    import ode_rl_amd
    from oracle import torchdiffeq_ref
    f = _func(name, seed=1)
    c = STACKS[name][0][0]
    z0 = torch.randn(batch, c, 16, 16, generator=torch.Generator().manual_seed(2)) * 0.5
    t = torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T)
    with torch.no_grad():
        ref = torchdiffeq_ref.odeint(_oracle_f(f), z0, t, method=method)
        got = ode_rl_amd.odeint(f.to(cuda), z0.to(cuda), t, method=method).cpu()
    assert torch.equal(got[0], z0)
    assert rel_l2(got[1:] - z0, ref[1:] - z0) <= 1e-5


@pytest.mark.parametrize("name,batch", [("A_tanh", 64), ("A_head", 64), ("A_tanh_head", 4)])
def test_persistent_trajectory_is_bit_identical_to_per_layer_launches(cuda, name, batch):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f = _func(name, seed=5).to(cuda)
    z0 = torch.randn(batch, 64, 16, 16, device=cuda) * 0.5
    t = torch.arange(10, 20, dtype=torch.float64, device=cuda) / 20
    was = lib.odehip_set_persistent_trajectory(0)
    try:
        with torch.no_grad():
            ref = ode_rl_amd.odeint(f, z0, t, method="rk4")
            lib.odehip_set_persistent_trajectory(1)
            n0 = lib.odehip_persistent_trajectory_launches()
            out = ode_rl_amd.odeint(f, z0, t, method="rk4")
            torch.cuda.synchronize()
        if os.environ.get("ODEHIP_PERSISTENT", "1") != "0":   # switched off for the process: the switch above does not re-enable it
            assert lib.odehip_persistent_trajectory_launches() > n0, "the persistent path did not run"
        assert torch.equal(out, ref)
    finally:
        lib.odehip_set_persistent_trajectory(was)


@pytest.mark.parametrize("name,batch", [("A_tanh_head", 3), ("A_tanh", 20)])
def test_dopri5_matches_oracle_and_async(cuda, name, batch):
    import ode_rl_amd
    from oracle import torchdiffeq_ref
    f = _func(name, seed=3)
    z0 = torch.randn(batch, 64, 16, 16, generator=torch.Generator().manual_seed(4)) * 0.5
    t = torch.tensor([0.0, 0.05, 0.3, 0.31, 0.75], dtype=torch.float64)
    ost = {}
    with torch.no_grad():
        ref = torchdiffeq_ref.odeint(_oracle_f(f), z0, t, rtol=1e-4, atol=1e-5, method="dopri5", stats=ost)
        f = f.to(cuda)
        got = ode_rl_amd.odeint(f, z0.to(cuda), t, rtol=1e-4, atol=1e-5, method="dopri5")
        st = dict(ode_rl_amd.last_stats)
        assert (st["nfe"], st["n_accept"], st["n_reject"]) == (ost["nfe"], ost.get("n_accept", 0), ost.get("n_reject", 0))
        assert rel_l2(got, ref) <= 1e-4
        was = ode_rl_amd.set_async_dopri5(True)
        try:
            got_async = ode_rl_amd.odeint(f, z0.to(cuda), t, rtol=1e-4, atol=1e-5, method="dopri5")
            assert torch.equal(got_async, got)
            assert dict(ode_rl_amd.last_stats)["nfe"] == st["nfe"]
        finally:
            ode_rl_amd.set_async_dopri5(was)


def _check_grads(got_z, got_p, ref_z, ref_p, tol=1e-4):
    assert rel_l2(got_z, ref_z) <= tol
    for i, (a, b) in enumerate(zip(got_p, ref_p)):
        assert a is not None and rel_l2(a, b) <= tol, i


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4", "dopri5"])
@pytest.mark.parametrize("name", ["A_tanh", "A_tanh_head", "A_head", "V_tanh_head"])
def test_backward_matches_autograd_through_oracle(cuda, name, method):
    import ode_rl_amd
    from oracle import torchdiffeq_ref
    f = _func(name, seed=7, kink_free=(name == "A_head"))
    c = STACKS[name][0][0]
    g = torch.Generator().manual_seed(8)
    z0 = torch.randn(3, c, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.25, 0.3, 0.7], dtype=torch.float64)
    gout = torch.randn(4, 3, c, 16, 16, generator=g)
    kw = dict(rtol=1e-4, atol=1e-5) if method == "dopri5" else {}
    params = _leaf_params(f)
    z = z0.clone().requires_grad_(True)
    sol = torchdiffeq_ref.odeint(_oracle_f(f, params), z, t, method=method, **kw)
    ref = torch.autograd.grad(sol, [z] + params, gout)
    f = f.to(cuda)
    zd = z0.to(cuda).requires_grad_(True)
    out = ode_rl_amd.odeint(f, zd, t, method=method, **kw)
    assert rel_l2(out, sol.detach()) <= 1e-4
    (out * gout.to(cuda)).sum().backward()
    _check_grads(zd.grad, _param_grads(f), ref[0], ref[1:])


@pytest.mark.parametrize("method,norm", [("rk4", None), ("euler", None), ("dopri5", "seminorm"), ("dopri5", "mixed")])
@pytest.mark.parametrize("name", ["A_tanh_head", "A_tanh"])
def test_adjoint_matches_oracle_adjoint(cuda, name, method, norm):
    import ode_rl_amd
    from oracle import torchdiffeq_ref
    f = _func(name, seed=9)
    g = torch.Generator().manual_seed(10)
    z0 = torch.randn(3, 64, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.25, 0.3, 0.7], dtype=torch.float64)
    gout = torch.randn(4, 3, 64, 16, 16, generator=g)
    kw = dict(rtol=1e-3, atol=1e-4) if method == "dopri5" else {}
    params = _leaf_params(f)
    stats = {}
    ref_sol, ref_gz, ref_gp = torchdiffeq_ref.odeint_adjoint(_oracle_f(f, params), z0, t, params, gout, method=method, stats=stats,
                                                             **kw, **({"adjoint_norm": norm} if norm else {}))
    f = f.to(cuda)
    zd = z0.to(cuda).requires_grad_(True)
    opts = {"adjoint_options": {"norm": norm}} if norm == "seminorm" else {}
    sol = ode_rl_amd.odeint_adjoint(f, zd, t, method=method, **kw, **opts)
    assert rel_l2(sol, ref_sol) <= 1e-4
    sol.backward(gout.to(cuda))
    if method == "dopri5":
        got = ode_rl_amd.last_adjoint_stats
        assert (got["nfe"], got["n_accept"], got["n_reject"]) == (stats["nfe"], stats["n_accept"], stats.get("n_reject", 0)), (got, stats)
    _check_grads(zd.grad, _param_grads(f), ref_gz, ref_gp)


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_decreasing_t_and_backwards(cuda, method):
    """Strictly decreasing t integrates -f on -t (torchdiffeq); backwards=True returns -f -- the sign comes after the Tanh head."""
    import ode_rl_amd
    from oracle import torchdiffeq_ref
    f = _func("A_tanh_head", seed=11)
    z0 = torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(12)) * 0.5
    t = torch.tensor([0.7, 0.5, 0.3, 0.1], dtype=torch.float64)
    kw = dict(rtol=1e-4, atol=1e-5) if method == "dopri5" else {}
    with torch.no_grad():
        ref = torchdiffeq_ref.odeint(_oracle_f(f), z0, t, method=method, **kw)
        ref_b = _oracle_f(f, backwards=True)(0.0, z0)
        f = f.to(cuda)
        out = ode_rl_amd.odeint(f, z0.to(cuda), t, method=method, **kw)
        assert rel_l2(out[1:].cpu() - z0, ref[1:] - z0) <= 1e-5
        assert rel_l2(f(0.0, z0.to(cuda), backwards=True), ref_b) <= 5e-6
        solver = ode_rl_amd.DiffEqSolver(f, method, device=cuda)
        assert rel_l2(solver(z0.to(cuda), t.to(cuda)).cpu()[1:] - z0, ref[1:] - z0) <= 1e-4


def test_encoder_matches_reference_fixture(cuda):
    import ode_rl_amd
    g = load_golden("tanh.npz")
    f = ode_rl_amd.ODEFunc(n_inputs=32, n_outputs=32, n_layers=3, n_units=32, downsize=False, nonlinear="tanh", final_act=True)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), 32)
    enc.load_state_dict(procedural_state_dict(enc.state_dict(), 43))
    enc = enc.to(cuda)
    inp = procedural_tensor((4, 1, 32, 16, 16), 143, -1, 1).to(cuda)
    t = torch.arange(4, dtype=torch.float64, device=cuda) / 8
    with torch.no_grad():
        mean, std = enc(inp, t)
        _, latent = enc.run_ode_conv_gru(inp, t)
    assert rel_l2(latent, torch.from_numpy(g["enc_tanh.latent"])) <= 5e-5
    assert rel_l2(mean, torch.from_numpy(g["enc_tanh.mean"])) <= 5e-5
    assert rel_l2(std, torch.from_numpy(g["enc_tanh.std"])) <= 5e-5


@pytest.mark.parametrize("ch,act", [(64, "tanh"), (64, "relu")])   # (the training path takes 64-channel multiples)
def test_encoder_backward_matches_autograd_through_oracle(cuda, ch, act):
    import ode_rl_amd
    from oracle import reference_modules as rm
    torch.manual_seed(13)
    f = ode_rl_amd.ODEFunc(n_inputs=ch, n_outputs=ch, n_layers=3, n_units=ch, downsize=False, nonlinear=act, final_act=True)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), ch)
    alt = torch.where(torch.arange(ch) % 2 == 0, 2.5, -2.5)
    with torch.no_grad():
        if act == "relu":
            for i in (0, 2, 4, 6):
                f.gradient_net[i].weight.mul_(0.15)
                f.gradient_net[i].bias.copy_(alt)
        enc.transform_z0[0].weight.mul_(0.3)   # the 1x1 head's ReLU away from its kink
        enc.transform_z0[0].bias.copy_(alt)
        for k, p in enc.cgru_cell.state_dict().items():
            if ".1." in k:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if k.endswith("weight") else 0.0))
    g = torch.Generator().manual_seed(14)
    T, B = 3, 2
    inputs = torch.randn(T, B, ch, 16, 16, generator=g) * 0.5
    t = torch.arange(T, dtype=torch.float64) / 8
    gmean, gstd = torch.randn(B, ch, 16, 16, generator=g), torch.randn(B, ch, 16, 16, generator=g)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    n = sum(1 for k in sd if k.startswith("ode_func.gradient_net.") and k.endswith(".weight"))
    ws = [sd[f"ode_func.gradient_net.{2 * i}.weight"] for i in range(n)]
    bs = [sd[f"ode_func.gradient_net.{2 * i}.bias"] for i in range(n)]
    cell = {k[len("cgru_cell."):]: v for k, v in sd.items() if k.startswith("cgru_cell.")}
    head = {k[len("transform_z0."):]: v for k, v in sd.items() if k.startswith("transform_z0.")}
    x = inputs.clone().requires_grad_(True)
    rmean, rstd, _ = rm.ode_convgru_encode(x, t, _oracle_f(f, ws + bs), cell, head)
    names = list(sd)
    grads = torch.autograd.grad([rmean, rstd], [x] + [sd[k] for k in names], [gmean, gstd])
    enc = enc.to(cuda)
    xd = inputs.to(cuda).requires_grad_(True)
    mean, std = enc(xd, t.to(cuda))
    assert rel_l2(mean, rmean.detach()) <= 5e-5 and rel_l2(std, rstd.detach()) <= 5e-5
    torch.autograd.backward([mean, std], [gmean.to(cuda), gstd.to(cuda)])
    assert rel_l2(xd.grad, grads[0]) <= 2e-4
    bad = {}
    for name, gr in zip(names, grads[1:]):
        p = dict(enc.named_parameters()).get(name)
        if p is not None and rel_l2(p.grad, gr) > 2e-4:
            bad[name] = rel_l2(p.grad, gr)
    assert not bad, bad


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_nan_in_y0_reaches_outputs_and_gradients(cuda, method):
    import ode_rl_amd
    f = _func("A_tanh_head", seed=15).to(cuda)
    z0 = torch.randn(2, 64, 16, 16, device=cuda) * 0.5
    z0[1, 3, 4, 5] = float("nan")
    t = torch.tensor([0.0, 0.1, 0.2], dtype=torch.float64)
    if method == "dopri5":
        with pytest.raises(Exception):   # a non-finite state stops the adaptive solver (ODEHIP_ENAN), as the reference asserts
            ode_rl_amd.odeint(f, z0.requires_grad_(True), t, method=method)
        return
    zd = z0.requires_grad_(True)
    out = ode_rl_amd.odeint(f, zd, t, method=method)
    assert bool(torch.isnan(out[1:, 1]).any()) and bool(torch.isfinite(out[:, 0]).all())
    out.sum().backward()
    assert bool(torch.isnan(zd.grad[1]).any())
    assert all(bool(torch.isnan(p).any()) for p in _param_grads(f))


def test_bf16_mode_refuses_tanh_stacks_before_launching(cuda):
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    for name in ("A_tanh", "A_head"):
        f = _func(name, seed=16).to(cuda)
        z0 = torch.randn(2, 64, 16, 16, device=cuda)
        t = torch.tensor([0.0, 0.1], dtype=torch.float64)
        with torch.no_grad():
            ref = ode_rl_amd.odeint(f, z0, t, method="rk4")   # an fp32 call first: the stack is cached
        torch.cuda.synchronize()
        n0 = lib.odehip_persistent_trajectory_launches()
        was = ode_rl_amd.hip_ops._global_mode
        ode_rl_amd.set_compute_dtype("bf16")
        try:
            with pytest.raises(TypeError, match="bf16"):
                ode_rl_amd.odeint(f, z0, t, method="rk4")
            with pytest.raises(TypeError, match="bf16"), torch.no_grad():
                f(0.0, z0)
        finally:
            ode_rl_amd.set_compute_dtype(was)
        assert lib.odehip_persistent_trajectory_launches() == n0
        with pytest.raises(TypeError, match="bf16"), torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            ode_rl_amd.odeint(f, z0, t, method="rk4")
        with torch.no_grad():
            assert torch.equal(ode_rl_amd.odeint(f, z0, t, method="rk4"), ref)
