"""Cases of the weight-gradient tests (test_hip_wgrad.py, _wgrad_worker.py) and of tools/wgrad_ab.py: one set of builders.

A case is a plain dict of CPU tensors and settings (a "spec").  The CPU side builds specs from procedural values and restates each in
float64 / float32 (oracle.torchdiffeq_ref for the 3x3 dynamics stacks, oracle.reference_modules.convgru_cell looped for the cells); the
device side (`run_on_device`) runs a spec through the library once and returns its gradients by name."""
import torch

CELL_NAMES = ["conv_gates.0.weight", "conv_gates.0.bias", "conv_gates.1.weight", "conv_gates.1.bias",
              "conv_can.0.weight", "conv_can.0.bias", "conv_can.1.weight", "conv_can.1.bias"]


# ---------------------------------------------------------------------------------------------------------------- device side
def stack_grads(dev, spec):
    """odeint(...).backward(gout) through a 3x3 dynamics stack: {"z0", "w0".., "b0"..}.  spec["sd"] None: the module's own initialisation."""
    import ode_rl_amd
    f = ode_rl_amd.ODEFunc(64, 64, spec["n_layers"], spec["n_units"], False, "relu", final_act=False)
    if spec.get("sd") is not None:
        f.load_state_dict(spec["sd"])
    f = f.to(dev)
    z = spec["z0"].to(dev).requires_grad_(True)
    ode_rl_amd.odeint(f, z, spec["t"], method=spec["method"]).backward(spec["gout"].to(dev))
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    out = {"z0": z.grad}
    out.update({f"w{i}": c.weight.grad for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad for i, c in enumerate(convs)})
    return out


def cell_grads(dev, spec):
    """T steps of a ConvGRU cell under a fixed weighting of every state, by the per-step driver ("step", convgru_backward.hip) or the
    whole-sequence one ("rollout", convgru_sequence.hip): {"x", "h0" (if given), the eight parameters}."""
    import ode_rl_amd
    cell = ode_rl_amd.ConvGRUCell((16, 16), spec["I"], spec["H"], spec["ks"])
    if spec.get("sd") is not None:
        cell.load_state_dict(spec["sd"])
    cell = cell.to(dev)
    x = spec["x"].to(dev).requires_grad_(True)
    h0 = None if spec["h0"] is None else spec["h0"].to(dev).requires_grad_(True)
    if spec["driver"] == "step":
        hs, last = cell(input_tensor=x, h_cur=h0, seq_len=spec["T"])
    else:
        hs, last = cell.rollout(x, h0, spec["T"])
    ((hs * spec["gw"].to(dev)).sum() + (last * spec["gl"].to(dev)).sum()).backward()
    out = {"x": x.grad}
    if h0 is not None:
        out["h0"] = h0.grad
    ps = dict(cell.named_parameters())
    out.update({k: ps[k].grad for k in CELL_NAMES})
    return out


def run_on_device(dev, spec):
    """{"grads": {name: CPU tensor}}, or {"error": text} for a spec that expects the library's argument checks to reject it."""
    import ode_rl_amd
    mode = spec.get("compute_dtype")
    if mode is not None:
        ode_rl_amd.set_compute_dtype(mode)
    try:
        fn = stack_grads if spec["kind"] == "stack" else cell_grads
        if spec.get("expect_rejected"):
            try:
                fn(dev, spec)
            except ValueError as e:
                return {"error": f"ValueError: {e}"}
            raise AssertionError("the library accepted a case that expects a rejection")
        grads = fn(dev, spec)
        torch.cuda.synchronize()
        return {"grads": {k: v.detach().cpu() for k, v in grads.items()}}
    finally:
        if mode is not None:
            ode_rl_amd.set_compute_dtype(None)


# ------------------------------------------------------------------------------------------------------------------- CPU side
def stack_case(n_layers, n_units, method, T, B, seed):
    """Kink-free dynamics as in test_backward_strict_on_kink_free_dynamics: weights x 0.15 and hidden biases of +-2.5 on alternating
    channels (half the channels always active, half always masked), last layer x 4; procedural values throughout."""
    import ode_rl_amd
    from conftest import procedural_state_dict, procedural_tensor
    shapes = ode_rl_amd.ODEFunc(64, 64, n_layers, n_units, False, "relu", final_act=False).state_dict()
    sd = procedural_state_dict(shapes, seed)
    n_conv = len([k for k in sd if k.endswith(".weight")])
    for i in range(n_conv):
        w, b = f"gradient_net.{2 * i}.weight", f"gradient_net.{2 * i}.bias"
        if i < n_conv - 1:
            sd[w] = sd[w] * 0.15
            sd[b] = torch.where(torch.arange(sd[b].numel()) % 2 == 0, 2.5, -2.5).to(torch.float32)
        else:
            sd[w] = sd[w] * 4.0
    return {"kind": "stack", "n_layers": n_layers, "n_units": n_units, "method": method, "sd": sd,
            "z0": procedural_tensor((B, 64, 16, 16), 1000 + seed, -1.0, 1.0),
            "t": torch.tensor([0.1, 0.25, 0.3, 0.7][:T], dtype=torch.float64),
            "gout": procedural_tensor((T, B, 64, 16, 16), 2000 + seed, -1.0, 1.0)}


def stack_reference(spec, dtype):
    """Autograd through the restated solver in `dtype`: (gradients by name, ReLU margin = the smallest |pre-activation| of a hidden layer)."""
    import torch.nn.functional as F
    from oracle import reference_modules as rm
    from oracle import torchdiffeq_ref
    ws, bs = rm.split_convnet_state(spec["sd"], "gradient_net.")
    ws = [w.detach().to(dtype).requires_grad_(True) for w in ws]
    bs = [b.detach().to(dtype).requires_grad_(True) for b in bs]
    margin = [float("inf")]

    def f(tt, y):
        x = y
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = F.conv2d(x, w, b, padding=1)
            if i < len(ws) - 1:
                margin[0] = min(margin[0], float(x.detach().abs().min()))
                x = torch.relu(x)
        return x
    z = spec["z0"].detach().to(dtype).requires_grad_(True)
    sol = torchdiffeq_ref.odeint(f, z, spec["t"], method=spec["method"])
    grads = torch.autograd.grad(sol, [z] + ws + bs, spec["gout"].to(dtype))
    out = {"z0": grads[0]}
    out.update({f"w{i}": g for i, g in enumerate(grads[1:1 + len(ws)])})
    out.update({f"b{i}": g for i, g in enumerate(grads[1 + len(ws):])})
    return out, margin[0]


def cell_case(I, H, ks, driver, T, B, seed, state=True, compute_dtype=None, expect_rejected=False):
    import _convgru_ref as ref
    from conftest import procedural_tensor
    return {"kind": "cell", "I": I, "H": H, "ks": ks, "driver": driver, "T": T, "sd": ref.cell_state_dict(I, H, seed, ks),
            "x": procedural_tensor((T, B, I, 16, 16), 3000 + seed, -1.0, 1.0),
            "h0": procedural_tensor((B, H, 16, 16), 4000 + seed, -0.8, 0.8) if state else None,
            "gw": procedural_tensor((T, B, H, 16, 16), 5000 + seed, -1.0, 1.0), "gl": procedural_tensor((B, H, 16, 16), 6000 + seed, -1.0, 1.0),
            "compute_dtype": compute_dtype, "expect_rejected": expect_rejected}


def cell_reference(spec, dtype, compute_dtype="f32"):
    """Autograd through oracle.reference_modules.convgru_cell looped over the sequence, in `dtype` (a zero state where h0 is None)."""
    from oracle import reference_modules as rm
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in spec["sd"].items()}
    x = spec["x"].detach().to(dtype).requires_grad_(True)
    h0 = None if spec["h0"] is None else spec["h0"].detach().to(dtype).requires_grad_(True)
    h = h0 if h0 is not None else torch.zeros(x.shape[1], spec["H"], 16, 16, dtype=dtype)
    hs = []
    for t in range(spec["T"]):
        h = rm.convgru_cell(x[t], h, p, compute_dtype=compute_dtype)
        hs.append(h)
    hs = torch.stack(hs)
    loss = (hs * spec["gw"].to(dtype)).sum() + (hs[-1] * spec["gl"].to(dtype)).sum()
    leaves = [("x", x)] + ([("h0", h0)] if h0 is not None else []) + [(k, p[k]) for k in CELL_NAMES]
    grads = torch.autograd.grad(loss, [v for _, v in leaves])
    return {k: g for (k, _), g in zip(leaves, grads)}
