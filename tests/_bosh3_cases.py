"""Cases of the bosh3 tests (test_bosh3_cases_cpu.py, test_hip_bosh3.py): stacks the adaptive drivers take -- the 64-channel 3-conv
ReLU stack (the persistent adaptive walk), 128 -> 64 -> 64 -> 128 (one launch per layer) and a Tanh stack with a Tanh head -- in the
spec format of _solver_stack_cases.py, whose dynamics / device helpers they reuse.  The references are tests/_adaptive_ref.py in
float64 and float32.

What each case is there for is a CONDITION that test_bosh3_cases_cpu.py proves from the restatement:
  every case     float32 and float64 take the same (accepted, rejected) counts; no frame, slope or gradient is all zero
  R3             n_reject >= 1 (the first layer's bias shifted down, as F4 / F6 of _solver_stack_cases.py)
  R1             two output times inside one accepted step, and an accepted step that contains no output time
  T2             a decreasing t
Tolerances: _solver_stack_cases.DOPRI5_TOL (rtol 1e-3, atol 1e-4), the loose end the models solve at."""
import torch

import _adaptive_ref as ar
import _solver_stack_cases as sc

TOL = sc.DOPRI5_TOL

# name -> (channels, hidden activation, Tanh head, B, times, gain, first-layer bias shift, seed)
FORWARD = {
    "R1": ((64, 64, 64, 64), "relu", False, 1, [0.0, 0.3, 0.45, 0.7, 1.0], 6.0, 0.0, 31),
    "R3": ((64, 64, 64, 64), "relu", False, 3, [0.0, 0.4, 1.0], 20.0, -1.0, 32),
    "W2": ((128, 64, 64, 128), "relu", False, 2, [0.0, 0.3, 0.6, 1.0], 6.0, 0.0, 33),
    "T2": ((64, 64, 64), "tanh", True, 2, [1.0, 0.7, 0.2, 0.0], 8.0, 0.0, 34),
}
# kink-free backward stacks (B1 - B3's construction): name -> (channels, hidden activation, B, times, seed)
BACKWARD = {
    "G64": ((64, 64, 64, 64), "relu", 2, [0.1, 0.25, 0.3, 0.7], 41),    # saving forward + reverse sweep on the adaptive walk
    "G128": ((128, 64, 128), "relu", 2, [0.1, 0.4, 0.7], 42),           # nothing saved: the backward re-integrates, one launch per layer
    "GT": ((64, 64, 64), "tanh", 2, [0.1, 0.3, 0.7], 43),               # Tanh hidden layer
}
# torchdiffeq's first_step option under autograd, so that no gradient runs through the step heuristic.  0.02: the controller's tenfold
# growth then tries 0.2, which these dynamics accept -- from 0.005 it would try 0.5, a rejected attempt that throws the state across
# the ReLU kinks the stacks are built to stay away from
FIRST_STEP = 0.02


def forward_spec(name):
    from conftest import procedural_state_dict, procedural_tensor
    channels, act, final_act, B, times, gain, shift, seed = FORWARD[name]
    sd = procedural_state_dict(sc._shapes(channels, 3), seed)
    sd["gradient_net.0.bias"] = sd["gradient_net.0.bias"] + shift
    last = 2 * (len(channels) - 2)
    sd[f"gradient_net.{last}.weight"] = sd[f"gradient_net.{last}.weight"] * gain
    sd[f"gradient_net.{last}.bias"] = sd[f"gradient_net.{last}.bias"] * gain
    return {"channels": channels, "ks": 3, "act": act, "final_act": final_act, "sd": sd, "method": "bosh3",
            "t": torch.tensor(times, dtype=torch.float64), "z0": procedural_tensor((B, channels[0], 16, 16), 1000 + seed, -1.0, 1.0)}


def backward_spec(name):
    from conftest import procedural_state_dict, procedural_tensor
    channels, act, B, times, seed = BACKWARD[name]
    sd = procedural_state_dict(sc._shapes(channels, 3), seed)
    n_conv = len(channels) - 1
    for i in range(n_conv):
        w, b = f"gradient_net.{2 * i}.weight", f"gradient_net.{2 * i}.bias"
        if i < n_conv - 1:
            sd[w] = sd[w] * 0.15
            sd[b] = torch.where(torch.arange(sd[b].numel()) % 2 == 0, 2.5, -2.5).to(torch.float32)
        else:
            sd[w] = sd[w] * 4.0
    T = len(times)
    return {"channels": channels, "ks": 3, "act": act, "final_act": False, "sd": sd, "method": "bosh3",
            "t": torch.tensor(times, dtype=torch.float64), "z0": procedural_tensor((B, channels[0], 16, 16), 1000 + seed, -1.0, 1.0),
            "gout": procedural_tensor((T, B, channels[0], 16, 16), 2000 + seed, -1.0, 1.0)}


def forward_reference(spec, dtype, method=None, options=None):
    """(trajectory, stats) of the restatement in `dtype`; stats: nfe, n_accept, n_reject, accepted [(t0, dt)], dts, ratios."""
    ws, bs = sc._params(spec, dtype)
    stats = {}
    with torch.no_grad():
        sol = ar.odeint(sc.dynamics(spec, ws, bs), spec["z0"].to(dtype), spec["t"], method=method or spec["method"], stats=stats,
                        options=options, **TOL)
    return sol, stats


def counts(stats):
    return (stats["nfe"], stats["n_accept"], stats["n_reject"])


def backward_reference(spec, dtype):
    """(gradients by name, smallest |pre-activation| of a hidden layer, stats): autograd in `dtype` through the restatement."""
    ws, bs = sc._params(spec, dtype, requires_grad=True)
    margin = [float("inf")]
    f = sc.dynamics(spec, ws, bs, margin)
    stats = {}
    z = spec["z0"].detach().to(dtype).requires_grad_(True)
    sol = ar.odeint(f, z, spec["t"], method="bosh3", stats=stats, options={"first_step": FIRST_STEP}, **TOL)
    grads = torch.autograd.grad(sol, [z] + ws + bs, spec["gout"].to(dtype))
    out = {"z0": grads[0].detach()}
    out.update({f"w{i}": g.detach() for i, g in enumerate(grads[1:1 + len(ws)])})
    out.update({f"b{i}": g.detach() for i, g in enumerate(grads[1 + len(ws):])})
    return out, margin[0], stats


def adjoint_reference(spec, dtype, norm):
    """(gradients by name, (nfe, n_accept, n_reject) of the backward solves) of the restatement's adjoint in `dtype`."""
    ws, bs = sc._params(spec, dtype, requires_grad=True)
    stats = {}
    _, gz, gp = ar.odeint_adjoint(sc.dynamics(spec, ws, bs), spec["z0"].to(dtype), spec["t"], ws + bs, spec["gout"].to(dtype),
                                  method="bosh3", stats=stats, adjoint_norm=norm, **TOL)
    out = {"z0": gz.detach()}
    out.update({f"w{i}": g.detach() for i, g in enumerate(gp[:len(ws)])})
    out.update({f"b{i}": g.detach() for i, g in enumerate(gp[len(ws):])})
    return out, stats


def device_adjoint(dev, spec, norm, max_accept=None):
    """(gradients by name on the CPU, last_adjoint_stats) of odeint_adjoint(method="bosh3") and its backward pass."""
    import torch.nn as nn
    import ode_rl_amd
    f = sc.device_func(dev, spec)
    z = spec["z0"].to(dev).requires_grad_(True)
    opts = {} if norm == "mixed" else {"norm": "seminorm"}
    if max_accept is not None:
        opts["max_accept"] = max_accept
    sol = ode_rl_amd.odeint_adjoint(f, z, spec["t"], method="bosh3", adjoint_options=opts, **TOL)
    sol.backward(spec["gout"].to(dev))
    st = dict(ode_rl_amd.last_adjoint_stats)
    convs = [m for m in f.gradient_net if isinstance(m, nn.Conv2d)]
    out = {"z0": z.grad}
    out.update({f"w{i}": c.weight.grad for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad for i, c in enumerate(convs)})
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, st


def outputs_per_step(spec, stats):
    """For every accepted step of a run, how many output times lie in (t0, t0 + dt] (on -t for a decreasing grid)."""
    t = spec["t"]
    t = -t if bool(t[0] > t[1]) else t
    return [sum(1 for x in t[1:].tolist() if t0 < x <= t0 + dt) for t0, dt in stats["accepted"]]


# ---------------------------------------------------------------------------------------------------------------- device side
def device_forward(dev, spec, method="bosh3", options=None, f=None):
    """(trajectory on the device, (nfe, n_accept, n_reject)) of one library call."""
    import ode_rl_amd
    f = f if f is not None else sc.device_func(dev, spec)
    with torch.no_grad():
        sol = ode_rl_amd.odeint(f, spec["z0"].to(dev), spec["t"], method=method, options=options, **TOL)
    st = dict(ode_rl_amd.last_stats)
    return sol, (st["nfe"], st["n_accept"], st["n_reject"])


def device_backward(dev, spec):
    """(gradients by name on the CPU, stats of the forward) of odeint(method="bosh3") under autograd and its backward pass."""
    import torch.nn as nn
    import ode_rl_amd
    f = sc.device_func(dev, spec)
    z = spec["z0"].to(dev).requires_grad_(True)
    sol = ode_rl_amd.odeint(f, z, spec["t"], method="bosh3", options={"first_step": FIRST_STEP}, **TOL)
    st = dict(ode_rl_amd.last_stats)
    sol.backward(spec["gout"].to(dev))
    convs = [m for m in f.gradient_net if isinstance(m, nn.Conv2d)]
    out = {"z0": z.grad}
    out.update({f"w{i}": c.weight.grad for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad for i, c in enumerate(convs)})
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, st
