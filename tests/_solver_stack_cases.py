"""Cases of the solver-stack tests (test_solver_stack_cases_cpu.py, test_hip_solver_stacks.py): dynamics whose LAST layer and whose
input-gradient layers run the direct convolution kernels (csrc/conv_q4.hip), so that the solver arithmetic of their epilogue
(csrc/conv_common.h: epilogue(), combine 1 / 2 / 3) is what produces the numbers compared.

A case is a plain dict of CPU tensors and settings (a "spec"), built from procedural values alone.  The CPU side restates each spec in
float64 and float32 with oracle.torchdiffeq_ref and F.conv2d; the device side runs it through the library once.

Forward stacks (FORWARD_STACKS): channels, kernel size, hidden activation, Tanh head, batch, number of time points, gain, hidden bias
shift, seed.  `gain` multiplies the last layer's weights and bias so that |f(z0)| is of the order of |z0|: one unit of time then
changes the state by order 1 (the stage combine contributes visibly; dopri5 takes several steps).  The smooth dynamics of a random
stack never make dopri5 reject a step; a negative shift of the first layer's bias (F4, F6) starts most hidden units switched off, so
the state drifts almost linearly, the controller grows the step tenfold and then meets the units switching on: rejected steps.
Forward cases (FORWARD_CASES): stack, method, time direction.

Backward stacks (BACKWARD_STACKS) are 3x3 and kink-free as _wgrad_cases.stack_case builds them: hidden biases of +-2.5 on alternating
channels, weights x 0.15, last layer x 4."""
import torch
import torch.nn as nn
import torch.nn.functional as F

FIXED_FLOOR = 3e-6     # increments of a fixed-grid trajectory (tests/test_hip_odeint.py: VIGOROUS_TOL)
DOPRI5_FLOOR = 5e-5    # increments of a dopri5 trajectory: the quartic dense output cancels in fp32
GRAD_FLOOR = 1e-4      # every gradient tensor (the project's gradient bound)
DOPRI5_TOL = dict(rtol=1e-3, atol=1e-4)   # at rtol >= 1e-4 the step sequence is the oracle's

# name -> (channels, ks, hidden activation, Tanh head, B, T, gain, hidden bias shift, seed)
FORWARD_STACKS = {
    "F1": ((32, 96, 96, 32), 3, "relu", False, 3, 3, 12.0, 0.0, 11),    # 3x3 ring as last layer: cin 96, 6 chunks; partials at C = 32
    "F2": ((64, 192, 64), 3, "relu", False, 2, 3, 6.0, 0.0, 12),        # ring with 12 chunks as last layer
    "F3": ((256, 256), 3, "relu", False, 1, 2, 1.5, 0.0, 13),           # first = last layer, 16 chunks, cout 256
    "F4": ((32, 32, 32), 5, "relu", False, 2, 3, 15.0, -0.5, 14),       # conv_ring_kernel<5,1,4> with combine
    "F5": ((128, 128, 128), 5, "relu", False, 33, 2, 6.0, 0.0, 15),     # conv_ring_kernel<5,1,2,2>: 33 * 4 * 2 = 264 workgroups > 256
    "F6": ((64, 32, 64), 1, "relu", False, 3, 3, 30.0, -1.0, 16),       # 1x1 ring with combine
    "F7": ((32, 96, 96, 32), 3, "tanh", True, 3, 3, 8.0, 0.0, 17),      # F1's stack, Tanh hidden layers and a Tanh head: act_fwd in epilogue()
}
# name -> (stack, method, decreasing t)
FORWARD_CASES = {}
for _m in ("euler", "midpoint", "rk4", "dopri5"):
    FORWARD_CASES[f"F1.{_m}"] = ("F1", _m, False)
for _m in ("rk4", "dopri5"):
    FORWARD_CASES[f"F2.{_m}"] = ("F2", _m, False)
FORWARD_CASES["F3.midpoint"] = ("F3", "midpoint", False)
for _m in ("rk4", "dopri5"):
    FORWARD_CASES[f"F4.{_m}"] = ("F4", _m, False)
FORWARD_CASES["F5.euler"] = ("F5", "euler", False)
for _m in ("rk4", "dopri5"):
    FORWARD_CASES[f"F6.{_m}"] = ("F6", _m, False)
FORWARD_CASES["F7.rk4"] = ("F7", "rk4", False)
for _s in ("F1", "F4"):                                            # F8: k_scale = -1
    for _m in ("rk4", "dopri5"):
        FORWARD_CASES[f"F8.{_s}.{_m}.decreasing"] = (_s, _m, True)

# name -> (channels, hidden activation, B, T, seed)
BACKWARD_STACKS = {
    "B1": ((64, 192, 192, 64), "relu", 2, 3, 21),   # ring dgrad with combine 2 (192 -> 192) and combine 3 (192 -> 64); wgrad tiles at 192
    "B2": ((192, 64, 192), "relu", 2, 3, 22),       # ring dgrad with combine 2 as the chain's first row, Winograd combine 3 next to it
    "B3": ((64, 192, 192, 64), "tanh", 2, 3, 23),   # B1 with Tanh hidden layers: act_bwd Tanh in epilogue()
}
# name -> (stack, driver, method); drivers: "discrete" = odeint(...).backward, "adjoint" = odeint_adjoint(...).backward
BACKWARD_CASES = {
    "B1.rk4.discrete": ("B1", "discrete", "rk4"),
    "B1.euler.adjoint": ("B1", "adjoint", "euler"),
    "B1.dopri5.adjoint": ("B1", "adjoint", "dopri5"),
    "B2.rk4.discrete": ("B2", "discrete", "rk4"),
    "B2.dopri5.discrete": ("B2", "discrete", "dopri5"),
    "B3.rk4.discrete": ("B3", "discrete", "rk4"),
}
BACKWARD_FIRST_STEP = 0.005   # dopri5 under autograd: torchdiffeq's first_step option, so that no gradient runs through the step heuristic


class StackFunc(nn.Module):
    """The smallest module the library's odeint accepts: `gradient_net`, Conv2d layers ('same') separated by ReLU or Tanh."""

    def __init__(self, channels, ks, act="relu", final_act=False):
        super().__init__()
        layers = []
        n = len(channels) - 1
        for i in range(n):
            layers.append(nn.Conv2d(channels[i], channels[i + 1], ks, padding=ks // 2))
            if i < n - 1:
                layers.append(nn.Tanh() if act == "tanh" else nn.ReLU())
        if final_act:
            layers.append(nn.Tanh())
        self.gradient_net = nn.Sequential(*layers)

    def forward(self, t, y):
        return self.gradient_net(y)


def _shapes(channels, ks):
    sd = {}
    for i in range(len(channels) - 1):
        sd[f"gradient_net.{2 * i}.weight"] = torch.zeros(channels[i + 1], channels[i], ks, ks)
        sd[f"gradient_net.{2 * i}.bias"] = torch.zeros(channels[i + 1])
    return sd


def _times(T, decreasing=False):
    t = torch.tensor([0.0, 0.4, 1.0][:T] if T > 2 else [0.0, 0.7], dtype=torch.float64)
    return (1.0 - t) if decreasing else t


def forward_stack(name):
    """The spec of a forward stack without method and time grid (forward_case adds them): shared by the cases of the stack."""
    from conftest import procedural_state_dict, procedural_tensor
    channels, ks, act, final_act, B, T, gain, shift, seed = FORWARD_STACKS[name]
    sd = procedural_state_dict(_shapes(channels, ks), seed)
    sd["gradient_net.0.bias"] = sd["gradient_net.0.bias"] + shift
    last = 2 * (len(channels) - 2)
    sd[f"gradient_net.{last}.weight"] = sd[f"gradient_net.{last}.weight"] * gain
    sd[f"gradient_net.{last}.bias"] = sd[f"gradient_net.{last}.bias"] * gain
    return {"channels": channels, "ks": ks, "act": act, "final_act": final_act, "sd": sd, "T": T,
            "z0": procedural_tensor((B, channels[0], 16, 16), 1000 + seed, -1.0, 1.0)}


def forward_case(name, stacks=None):
    stack, method, decreasing = FORWARD_CASES[name]
    base = stacks[stack] if stacks is not None else forward_stack(stack)
    spec = dict(base)
    spec.update(method=method, t=_times(base["T"], decreasing))
    return spec


def backward_stack(name):
    from conftest import procedural_state_dict, procedural_tensor
    channels, act, B, T, seed = BACKWARD_STACKS[name]
    sd = procedural_state_dict(_shapes(channels, 3), seed)
    n_conv = len(channels) - 1
    for i in range(n_conv):
        w, b = f"gradient_net.{2 * i}.weight", f"gradient_net.{2 * i}.bias"
        if i < n_conv - 1:
            sd[w] = sd[w] * 0.15
            sd[b] = torch.where(torch.arange(sd[b].numel()) % 2 == 0, 2.5, -2.5).to(torch.float32)
        else:
            sd[w] = sd[w] * 4.0
    return {"channels": channels, "ks": 3, "act": act, "final_act": False, "sd": sd, "T": T,
            "z0": procedural_tensor((B, channels[0], 16, 16), 1000 + seed, -1.0, 1.0),
            "t": torch.tensor([0.1, 0.25, 0.3, 0.7][:T], dtype=torch.float64),
            "gout": procedural_tensor((T, B, channels[0], 16, 16), 2000 + seed, -1.0, 1.0)}


def backward_case(name, stacks=None):
    stack, driver, method = BACKWARD_CASES[name]
    base = stacks[stack] if stacks is not None else backward_stack(stack)
    spec = dict(base)
    spec.update(driver=driver, method=method)
    return spec


# ------------------------------------------------------------------------------------------------------------------- CPU side
def dynamics(spec, ws, bs, margin=None):
    """f(t, y) of a spec on the given weights (any dtype): F.conv2d, the hidden activation between the layers, the Tanh head.
    margin: a one-element list that receives the smallest |pre-activation| of a hidden layer."""
    pad = spec["ks"] // 2
    act = torch.tanh if spec["act"] == "tanh" else torch.relu

    def f(tt, y):
        x = y
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = F.conv2d(x, w, b, padding=pad)
            if i < len(ws) - 1:
                if margin is not None:
                    margin[0] = min(margin[0], float(x.detach().abs().min()))
                x = act(x)
        return torch.tanh(x) if spec["final_act"] else x
    return f


def _params(spec, dtype, requires_grad=False):
    from oracle import reference_modules as rm
    ws, bs = rm.split_convnet_state(spec["sd"], "gradient_net.")
    ws = [w.detach().to(dtype).requires_grad_(requires_grad) for w in ws]
    bs = [b.detach().to(dtype).requires_grad_(requires_grad) for b in bs]
    return ws, bs


def forward_reference(spec, dtype):
    """(trajectory, stats) of the oracle in `dtype`; stats holds n_accept / n_reject for dopri5."""
    from oracle import torchdiffeq_ref
    ws, bs = _params(spec, dtype)
    stats = {}
    kw = DOPRI5_TOL if spec["method"] == "dopri5" else {}
    with torch.no_grad():
        sol = torchdiffeq_ref.odeint(dynamics(spec, ws, bs), spec["z0"].to(dtype), spec["t"], method=spec["method"], stats=stats, **kw)
    return sol, (stats.get("n_accept", 0), stats.get("n_reject", 0))


def increments(sol, z0):
    """What the forward tests compare (as tests/test_hip_odeint.py does): sol[1:] - z0, so that an unchanged z0 hides nothing."""
    return sol[1:].detach().double().cpu() - z0.double()


def backward_reference(spec, dtype):
    """(gradients by name {"z0", "w0".., "b0"..}, ReLU margin, stats) in `dtype`: float64 autograd through the oracle's solver for the
    "discrete" driver, the oracle's adjoint (seminorm for dopri5) for the "adjoint" driver."""
    from oracle import torchdiffeq_ref
    ws, bs = _params(spec, dtype, requires_grad=True)
    margin = [float("inf")]
    f = dynamics(spec, ws, bs, margin)
    gout = spec["gout"].to(dtype)
    stats = {}
    if spec["driver"] == "adjoint":
        kw = dict(adjoint_norm="seminorm", **DOPRI5_TOL) if spec["method"] == "dopri5" else {}
        _, gz, gp = torchdiffeq_ref.odeint_adjoint(f, spec["z0"].to(dtype), spec["t"], ws + bs, gout, method=spec["method"], stats=stats, **kw)
        grads = [gz] + list(gp)
    else:
        kw = dict(options={"first_step": BACKWARD_FIRST_STEP}, **DOPRI5_TOL) if spec["method"] == "dopri5" else {}
        z = spec["z0"].detach().to(dtype).requires_grad_(True)
        sol = torchdiffeq_ref.odeint(f, z, spec["t"], method=spec["method"], stats=stats, **kw)
        grads = torch.autograd.grad(sol, [z] + ws + bs, gout)
    out = {"z0": grads[0].detach()}
    out.update({f"w{i}": g.detach() for i, g in enumerate(grads[1:1 + len(ws)])})
    out.update({f"b{i}": g.detach() for i, g in enumerate(grads[1 + len(ws):])})
    return out, margin[0], (stats.get("n_accept", 0), stats.get("n_reject", 0))


def third_views(name, tensor):
    """{suffix: function}: each third of every 192-channel axis of a weight gradient on its own, so that a misplaced tile cannot average
    away in the whole tensor's norm."""
    views = {}
    if name.startswith("w"):
        for axis in (0, 1):
            if tensor.shape[axis] == 192:
                for k in range(3):
                    views[f"[axis {axis}, third {k}]"] = (lambda t, axis=axis, k=k: t.narrow(axis, 64 * k, 64))
    return views


# ---------------------------------------------------------------------------------------------------------------- device side
def device_func(dev, spec):
    f = StackFunc(spec["channels"], spec["ks"], spec["act"], spec["final_act"])
    f.load_state_dict(spec["sd"])
    return f.to(dev)


def device_forward(dev, spec, f=None, z0=None):
    """(trajectory on the device, (n_accept, n_reject)) of one library call."""
    import ode_rl_amd
    f = f if f is not None else device_func(dev, spec)
    z0 = spec["z0"] if z0 is None else z0
    kw = DOPRI5_TOL if spec["method"] == "dopri5" else {}
    with torch.no_grad():
        sol = ode_rl_amd.odeint(f, z0.to(dev), spec["t"], method=spec["method"], **kw)
    counts = (0, 0)
    if spec["method"] == "dopri5":
        st = dict(ode_rl_amd.last_stats)
        counts = (st["n_accept"], st["n_reject"])
    return sol, counts


def device_backward(dev, spec):
    """Gradients by name of one library call and its backward pass, and the dopri5 adjoint's (n_accept, n_reject)."""
    import ode_rl_amd
    f = device_func(dev, spec)
    z = spec["z0"].to(dev).requires_grad_(True)
    counts = None
    if spec["driver"] == "adjoint":
        kw = dict(adjoint_options={"norm": "seminorm"}, **DOPRI5_TOL) if spec["method"] == "dopri5" else {}
        sol = ode_rl_amd.odeint_adjoint(f, z, spec["t"], method=spec["method"], **kw)
    else:
        kw = dict(options={"first_step": BACKWARD_FIRST_STEP}, **DOPRI5_TOL) if spec["method"] == "dopri5" else {}
        sol = ode_rl_amd.odeint(f, z, spec["t"], method=spec["method"], **kw)
    sol.backward(spec["gout"].to(dev))
    if spec["driver"] == "adjoint" and spec["method"] == "dopri5":
        st = ode_rl_amd.last_adjoint_stats
        counts = (st["n_accept"], st["n_reject"])
    convs = [m for m in f.gradient_net if isinstance(m, nn.Conv2d)]
    out = {"z0": z.grad}
    out.update({f"w{i}": c.weight.grad for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad for i, c in enumerate(convs)})
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, counts
