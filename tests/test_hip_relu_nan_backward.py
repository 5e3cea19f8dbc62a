"""NaN semantics of the backward passes against torch in float64 (bf16 paths: against the oracle's bf16 emulation).

torch's ReLU backward is threshold_backward, `y <= 0 ? 0 : g`: where the activation is NaN the gradient PASSES.  The forward ReLUs of
the library propagate NaN (relu_f); a backward mask `y > 0 ? g : 0` would turn a NaN forward pass into a finite, zero update.  The rule
checked here: wherever torch's result is NaN the HIP result is NaN, wherever torch's is a number the HIP result is a number within the
tolerance of the existing finite test of that path (rel-L2 over the finite entries).

The inputs are built so that the NaN pattern cannot depend on a Winograd tile: a NaN BIAS in one hidden channel makes that whole channel
map NaN, so the NaN masks must be EQUAL, not only a superset.  Weights and biases otherwise are kink-free (biases +-2.5 on alternating
channels keep every finite pre-activation far from 0), so no mask element can flip between two correct fp32 implementations.  With one
hidden channel c of conv l NaN, everything after conv l+1 is NaN in the forward pass, yet torch's gradient w.r.t. the input and the
bias gradients stay finite and dW_l[c], db_l[c] are finite and non-zero -- the entries a laundering mask zeroes.  dopri5 is not here:
its forward already stops on a non-finite state (tests/test_hip_solver_failures.py).  No NaN goes near the warp chain's flow or any
other kernel that turns data into an address."""
import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAN_LAYER, NAN_CH = 1, 6     # conv 1 (a hidden layer of every stack here), channel 6 (its bias is +2.5: active without the NaN)


def check_nan_rule(got, ref, tol, what):
    """got (HIP, any device) against ref (torch): equal NaN masks, finite entries within rel-L2 tol."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, what
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), (f"{what}: NaN masks differ: {int((gn & ~rn).sum())} NaN where torch has a number, "
                                 f"{int((rn & ~gn).sum())} numbers where torch has NaN (of {ref.numel()})")
    fin = ~rn
    assert bool(torch.isfinite(ref[fin]).all()) and bool(torch.isfinite(got[fin]).all()), what
    if bool(fin.any()) and float(ref[fin].norm()) > 0:
        e = rel_l2(got[fin], ref[fin])
        assert e <= tol, f"{what}: rel-L2 {e:.3e} over the finite entries > {tol}"
    else:
        assert torch.equal(got[fin], ref[fin]), what


def _kink_free_f(ch=64, units=64, n_layers=3, seed=0, nan_sign=1.0):
    import ode_rl_amd
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(ch, ch, n_layers, units, False, "relu", final_act=False)
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        for c in convs[:-1]:
            c.weight.mul_(0.15)
            c.bias.copy_(torch.where(torch.arange(c.out_channels) % 2 == 0, 2.5, -2.5))
        convs[-1].weight.mul_(4.0)
        convs[NAN_LAYER].bias[NAN_CH] = math.copysign(float("nan"), nan_sign)
    return f


def _oracle_grads(f, z0, t, gout, method, compute_dtype="f32", adjoint=False):
    from oracle import reference_modules as rm
    from oracle import torchdiffeq_ref
    dt = torch.float64 if compute_dtype == "f32" else torch.float32
    ws, bs = rm.split_convnet_state({k: v.detach().clone() for k, v in f.state_dict().items()}, "gradient_net.")
    ws = [w.to(dt).requires_grad_(True) for w in ws]
    bs = [b.to(dt).requires_grad_(True) for b in bs]
    func = rm.ode_func(ws, bs, compute_dtype=compute_dtype)
    if adjoint:
        sol, gz, gp = torchdiffeq_ref.odeint_adjoint(func, z0.detach().clone().to(dt), t, ws + bs, gout.to(dt), method=method)
        return sol, gz, list(gp[:len(ws)]), list(gp[len(ws):])
    z = z0.detach().clone().to(dt).requires_grad_(True)
    sol = torchdiffeq_ref.odeint(func, z, t, method=method)
    g = torch.autograd.grad(sol, [z] + ws + bs, gout.to(dt))
    return sol.detach(), g[0], list(g[1:1 + len(ws)]), list(g[1 + len(ws):])


def _run_hip(cuda, f, z0, t, gout, method, adjoint=False):
    import ode_rl_amd
    f = f.to(cuda)
    f.zero_grad()
    zd = z0.detach().to(cuda).requires_grad_(True)
    fn = ode_rl_amd.odeint_adjoint if adjoint else ode_rl_amd.odeint
    sol = fn(f, zd, t, method=method)
    sol.backward(gout.to(cuda))
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    return sol.detach(), zd.grad, [c.weight.grad for c in convs], [c.bias.grad for c in convs]


def _compare(got, ref, tol, tag):
    sol, gz, gw, gb = got
    rsol, rgz, rgw, rgb = ref
    # informative: the forward is NaN after the first evaluation, the gradients a laundering mask would zero are numbers in torch
    assert bool(torch.isnan(rsol[1:]).all())
    assert bool(torch.isfinite(rgb[NAN_LAYER][NAN_CH])) and float(rgb[NAN_LAYER][NAN_CH].abs()) > 0
    assert bool(torch.isfinite(rgz).all())
    check_nan_rule(sol, rsol, tol, f"{tag} trajectory")
    check_nan_rule(gz, rgz, tol, f"{tag} grad_z")
    for l, (a, b) in enumerate(zip(gw, rgw)):
        check_nan_rule(a, b, tol, f"{tag} dW{l}")
    for l, (a, b) in enumerate(zip(gb, rgb)):
        check_nan_rule(a, b, tol, f"{tag} db{l}")


@pytest.mark.parametrize("persistent", [0, 1], ids=["per_layer", "persistent"])
@pytest.mark.parametrize("batch", [2, 3, 20])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_fixed_grid_backward_passes_the_gradient_of_a_nan_channel(cuda, method, batch, persistent):
    """One informative step (T = 2) of each fixed-grid method through loss.backward(), 64-channel stack; euler is a single evaluation
    of f and its backward.  Batch 3 takes the sixteen-workgroup walk, batch 20 the whole-trajectory walk, persistent=0 the per-layer
    launches.  The dW of the layers behind the NaN channel are NaN in their input-channel slice c, as in torch."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f = _kink_free_f(seed=batch)
    g = torch.Generator().manual_seed(31 + batch)
    z0 = torch.randn(batch, 64, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.3], dtype=torch.float64)
    gout = torch.randn(2, batch, 64, 16, 16, generator=g)
    ref = _oracle_grads(f, z0, t, gout, method)
    was = lib.odehip_set_persistent_trajectory(persistent)
    try:
        got = _run_hip(cuda, f, z0, t, gout, method)
    finally:
        lib.odehip_set_persistent_trajectory(was)
    _compare(got, ref, 1e-4, f"{method} B{batch} persistent={persistent}")


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_vidode_stack_backward_passes_the_gradient_of_a_nan_channel(cuda, method):
    """VidODE's 128 -> 64 -> 64 -> 128 dynamics, one step."""
    f = _kink_free_f(ch=128, units=64, n_layers=2, seed=9)
    g = torch.Generator().manual_seed(9)
    z0 = torch.randn(2, 128, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.3], dtype=torch.float64)
    gout = torch.randn(2, 2, 128, 16, 16, generator=g)
    ref = _oracle_grads(f, z0, t, gout, method)   # (first: _run_hip moves f to the device)
    _compare(_run_hip(cuda, f, z0, t, gout, method), ref, 1e-4, f"vidode {method}")


@pytest.mark.parametrize("ch", [64, 128])
def test_fixed_grid_adjoint_passes_the_gradient_of_a_nan_channel(cuda, ch):
    """odeint_adjoint (rk4): the reverse solve re-integrates from the NaN final state, so every activation of the reverse pass is NaN;
    torch's adjoint and the parameters' bias gradients stay numbers (every mask passes), the weight gradients are NaN."""
    f = _kink_free_f(ch=ch, units=64, n_layers=3 if ch == 64 else 2, seed=4)
    g = torch.Generator().manual_seed(4)
    z0 = torch.randn(2, ch, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.3], dtype=torch.float64)
    gout = torch.randn(2, 2, ch, 16, 16, generator=g)
    ref = _oracle_grads(f, z0, t, gout, "rk4", adjoint=True)
    got = _run_hip(cuda, f, z0, t, gout, "rk4", adjoint=True)
    _compare(got, ref, 1e-4, f"adjoint C{ch}")


@pytest.mark.parametrize("ch,T,B", [(64, 3, 2), (64, 1, 3), (128, 2, 1)])
def test_encoder_backward_passes_the_gradient_of_a_nan_head_channel(cuda, ch, T, B):
    """The encoder (reverse-time Euler + ConvGRU + 1x1 head), shapes of test_hip_encoder_backward.py, with a NaN bias in one channel
    of the head's hidden 1x1 convolution: mean and std are NaN everywhere; the std gradient passes |.|, whose torch derivative at NaN
    is 0 (the ConvGRU backward's abs: a regression guard), so every gradient below the head's ReLU is a number in torch."""
    import test_hip_encoder_backward as teb
    enc = teb._build(ch)
    with torch.no_grad():
        enc.transform_z0[0].bias[NAN_CH] = float("nan")
    g = torch.Generator().manual_seed(11)
    inputs = torch.randn(T, B, ch, 16, 16, generator=g) * 0.5
    t = torch.arange(T, dtype=torch.float64) / 8
    gmean = torch.randn(B, ch, 16, 16, generator=g)
    gstd = torch.randn(B, ch, 16, 16, generator=g)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in enc.state_dict().items()}
    from oracle import reference_modules as rm
    ws, bs = rm.split_convnet_state(sd, "ode_func.gradient_net.")
    cell = {k[len("cgru_cell."):]: v for k, v in sd.items() if k.startswith("cgru_cell.")}
    head = {k[len("transform_z0."):]: v for k, v in sd.items() if k.startswith("transform_z0.")}
    x = inputs.double().requires_grad_(True)
    mean, std, _ = rm.ode_convgru_encode(x, t, rm.ode_func(ws, bs), cell, head)
    names = list(sd)
    rg = torch.autograd.grad([mean, std], [x] + [sd[k] for k in names], [gmean.double(), gstd.double()])
    assert bool(torch.isnan(mean).all()) and bool(torch.isfinite(rg[0]).all())
    assert bool(torch.isfinite(rg[1 + names.index("transform_z0.0.bias")][NAN_CH]))

    enc = enc.to(cuda)
    xd = inputs.to(cuda).requires_grad_(True)
    m, s = enc(xd, t.to(cuda))
    check_nan_rule(m, mean, 5e-5, "encoder mean")
    check_nan_rule(s, std, 5e-5, "encoder std")
    torch.autograd.backward([m, s], [gmean.to(cuda), gstd.to(cuda)])
    check_nan_rule(xd.grad, rg[0], 2e-4, "encoder grad_x")
    params = dict(enc.named_parameters())
    for k, r in zip(names, rg[1:]):
        if k in params:
            check_nan_rule(params[k].grad, r, 2e-4, f"encoder {k}")


@pytest.mark.parametrize("nan_sign", [1.0, -1.0], ids=["pos_nan", "neg_nan"])
@pytest.mark.parametrize("persistent", [0, 1], ids=["per_evaluation", "whole_trajectory"])
def test_bf16_backward_passes_the_gradient_of_a_nan_channel(cuda, persistent, nan_sign):
    """bf16 mode, rk4 training step: persistent=0 runs the per-evaluation stack (fstack_bf16.hip, masks on fp32 values), persistent=1
    the whole-trajectory reverse sweep (btraj_bf16.hip, masks on the saved bf16 bits -- a NaN with its sign bit set must pass too),
    against the oracle's bf16 emulation (fp32) at the bounds of tests/test_hip_bf16.py (gradients 5e-3)."""
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    f = _kink_free_f(seed=5, nan_sign=nan_sign)
    assert (torch.signbit(f.gradient_net[2 * NAN_LAYER].bias[NAN_CH]).item()) == (nan_sign < 0)
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(3, 64, 16, 16, generator=g) * 0.5
    t = torch.tensor([0.1, 0.25, 0.3], dtype=torch.float64)
    gout = torch.randn(3, 3, 64, 16, 16, generator=g)
    ref = _oracle_grads(f, z0, t, gout, "rk4", compute_dtype="bf16")
    ode_rl_amd.set_compute_dtype("bf16")
    was = lib.odehip_set_persistent_trajectory(persistent)
    try:
        n0 = lib.odehip_persistent_trajectory_launches()
        got = _run_hip(cuda, f, z0, t, gout, "rk4")
        if persistent and os.environ.get("ODEHIP_PERSISTENT", "1") != "0":
            assert lib.odehip_persistent_trajectory_launches() > n0, "the whole-trajectory path did not run"
    finally:
        lib.odehip_set_persistent_trajectory(was)
        ode_rl_amd.set_compute_dtype(None)
    _compare(got, ref, 5e-3, f"bf16 persistent={persistent} sign={nan_sign}")


# ---- VidODE's flow decoder: fused BatchNorm + ReLU (+ x2 upsampling)
@pytest.mark.parametrize("where", ["x", "gamma"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("upsample", [True, False])
@pytest.mark.parametrize("shape", [(3, 8, 4, 8), (5, 128, 32, 32), (2, 64, 64, 64)])
def test_bn_relu_up_backward_passes_the_gradient_of_a_nan_activation(cuda, shape, upsample, training, where):
    """Shapes and bounds of test_bn_relu_up_matches_torch (gradients 2e-5) with one NaN in x or in gamma.  Train mode and a NaN in x:
    the batch statistics of its channel are NaN, so is every pre-activation of it; torch then returns NaN grad_x and dgamma for that
    channel but a finite dbeta.  A NaN gamma makes its channel NaN in both modes while dgamma and dbeta stay finite."""
    from ode_rl_amd.autograd import bn_relu_up
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 7 + c + (2 if upsample else 0) + (1 if training else 0))
    x = torch.randn(*shape, generator=g) * 1.5 + 0.3
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    bn.train(training)
    ch = c // 2
    with torch.no_grad():
        ref_bn = copy.deepcopy(bn).double()
        pre = ref_bn(x.double())
        x = x + (pre.abs() < 1e-4).float() * 0.01     # off the kink, as the finite test
        if where == "x":
            x[n - 1, ch, h // 2, w // 2 + 1] = float("nan")
        else:
            bn.weight[ch] = float("nan")
    ref_bn = copy.deepcopy(bn).double()
    xr = x.double().requires_grad_(True)
    ref = torch.relu(ref_bn(xr))
    if upsample:
        ref = F.interpolate(ref, scale_factor=2, mode="bilinear", align_corners=False)
    gout = torch.randn(ref.shape, generator=g)
    ref.backward(gout.double())
    assert bool(torch.isfinite(ref_bn.bias.grad).all())          # the entries a laundering mask would zero are numbers in torch
    bnd = copy.deepcopy(bn).to(cuda)
    xd = x.to(cuda).requires_grad_(True)
    out = bn_relu_up(xd, bnd, upsample)
    check_nan_rule(out, ref, 2e-6, "bn_relu_up out")
    out.backward(gout.to(cuda))
    check_nan_rule(xd.grad, xr.grad, 2e-5, "bn_relu_up grad_x")
    check_nan_rule(bnd.weight.grad, ref_bn.weight.grad, 2e-5, "bn_relu_up dgamma")
    check_nan_rule(bnd.bias.grad, ref_bn.bias.grad, 2e-5, "bn_relu_up dbeta")


# ---- regression guards: backward passes whose NaN semantics already match torch
@pytest.mark.parametrize("where", ["x", "grad"])
def test_upsample2x_backward_propagates_nan_as_torch(cuda, where):
    from ode_rl_amd.autograd import upsample2x
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 16, 16, generator=g)
    gout = torch.randn(2, 8, 32, 32, generator=g)
    if where == "x":
        x[1, 3, 5, 6] = float("nan")
    else:
        gout[0, 2, 9, 17] = float("nan")
    xr = x.double().requires_grad_(True)
    ref = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    ref.backward(gout.double())
    xd = x.to(cuda).requires_grad_(True)
    out = upsample2x(xd)
    check_nan_rule(out, ref, 1e-6, "upsample2x out")
    out.backward(gout.to(cuda))
    check_nan_rule(xd.grad, xr.grad, 1e-6, "upsample2x grad")


def test_fused_adam_with_a_nan_gradient_matches_torch_adam(cuda):
    """Against torch.optim.Adam in fp32 (the arithmetic order of tests/test_hip_train_loop.py): the NaN element and its moments become
    NaN, every other element follows torch."""
    from ode_rl_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(3, 64, generator=g)
    grads = [torch.randn(3, 64, generator=g) for _ in range(3)]
    grads[1][1, 17] = float("nan")
    a = torch.nn.Parameter(p0.clone())
    b = torch.nn.Parameter(p0.to(cuda))
    oa = torch.optim.Adam([a], lr=1e-2, weight_decay=0.01, foreach=False)
    ob = FusedAdam([b], lr=1e-2, weight_decay=0.01)
    for gr in grads:
        a.grad, b.grad = gr.clone(), gr.to(cuda)
        oa.step()
        ob.step()
        check_nan_rule(b, a, 1e-6, "FusedAdam param")
    assert bool(torch.isnan(a[1, 17])) and int(torch.isnan(a).sum()) == 1
    for k in ("exp_avg", "exp_avg_sq"):   # (the moments round differently from torch's at ~1e-5; the masks are what is checked here)
        check_nan_rule(ob.state[b][k], oa.state[a][k], 1e-4, f"FusedAdam {k}")
