"""Cases of tests/test_hip_interleaved_walks.py: the fp32 trajectory walks (csrc/conv_wino.hip: persist_walk<ADAPT>, persist_walk_v) at the
batches where a group of four workgroups carries two samples, or runs its outer loop a second time.

256 workgroups are 64 groups; a group walks samples b and b + 64 layer by layer in turn, then b + 128 and b + 192.  The smallest batches of
each regime:
   65   group 0 walks samples 0 and 64 interleaved, the other 63 groups one sample (solo): the launch mixes both
  128   every group interleaved (130 on the wide walk, whose existing forward cases use it)
  129   every group interleaved in pass one; group 0 alone makes a second pass, solo, for sample 128
  193   group 0's second pass is itself interleaved (samples 128 and 192)

Dynamics: the shallowest stacks the walks take.  64 channels: ODEFunc(64, 64, 1, 64) = three convs, every output and input channel with
a weight scale of its own (tests/test_hip_strip_walk.py::_func), the last layer times `gain` so that the state moves by order 1 per unit
of time and the adaptive solvers take several steps.  "kinkfree": the same three convs as _wgrad_cases.stack_case builds them (hidden
biases +-2.5 on alternating channels, weights x 0.15, last layer x 4) under the same channel scales -- no pre-activation near a ReLU
kink, which the comparison of the two adjoint drivers needs (their step sizes differ in the last bits: a mask element that flipped
between them would not be round-off).  Wide: 128 -> 64 -> 64 -> 128 of tests/test_hip_vidode_shapes.py::_f_v.

Every sample has an input of its own: z0 = randn(seed 200 + B) * 0.5."""
import torch

N_GROUPS = 64
T_FIXED = (0.1, 0.25, 0.7)            # three non-uniform time points
T_ADAPTIVE = (0.0, 0.4, 1.0)
ADAPTIVE_TOL = dict(rtol=1e-4, atol=1e-5)
FIRST_STEP = 0.02                      # dopri5 under autograd (tests/_bosh3_cases.py: FIRST_STEP)
MIN_ACCEPT = 3

# stack -> (channels of the state, hidden activation, Tanh head, gain of the last layer).  Accepted steps of the float32 restatement
# (tests/_adaptive_ref.py on cpu_spec(), at B = 4, 65 and 129 alike) on T_ADAPTIVE at ADAPTIVE_TOL: relu 5 (dopri5), 12 (bosh3), 6 (dopri5
# from FIRST_STEP); wide 4; kinkfree forward 3 (dopri5, also from FIRST_STEP) and 4 (bosh3), seminorm adjoint 5 and 6 -- the tests assert >= MIN_ACCEPT
STACKS = {
    "relu": (64, "relu", False, 6.0),
    "tanh": (64, "tanh", True, 6.0),          # Tanh head: its reverse sweep is not recorded (one launch per layer), the saving forward is
    "tanh_hidden": (64, "tanh", False, 6.0),  # Tanh hidden layers alone: act_bwd's Tanh mask in the walk's reverse sweep
    "kinkfree": (64, "relu", False, 1.0),
    "wide": (128, "relu", False, 6.0),
}

# name -> (stack, driver, method, batch); drivers:
#   forward   odeint under no_grad
#   train     odeint(...).backward(gout): the saving forward and the reverse sweep (dopri5: first_step given, the one-walk backward;
#             what "one launch per layer" is for it: test_hip_interleaved_walks.py::_check_dopri5_backward)
#   adjoint   odeint_adjoint(...).backward(gout); adaptive methods under the seminorm, on the host loop
CASES = {
    "fixed_forward.rk4.B129": ("relu", "forward", "rk4", 129),
    "fixed_forward.rk4.B193": ("relu", "forward", "rk4", 193),
    "train.rk4.B65": ("relu", "train", "rk4", 65),
    "train.rk4.B129": ("relu", "train", "rk4", 129),
    "train.midpoint.B193": ("relu", "train", "midpoint", 193),
    "train.tanh.rk4.B65": ("tanh", "train", "rk4", 65),
    "train.tanh_hidden.rk4.B65": ("tanh_hidden", "train", "rk4", 65),
    "fixed_adjoint.rk4.B65": ("relu", "adjoint", "rk4", 65),
    "fixed_adjoint.euler.B129": ("relu", "adjoint", "euler", 129),
    "adaptive_forward.dopri5.B129": ("relu", "forward", "dopri5", 129),
    "adaptive_forward.bosh3.B65": ("relu", "forward", "bosh3", 65),
    "dopri5_backward.B65": ("relu", "train", "dopri5", 65),
    "dopri5_backward.B129": ("relu", "train", "dopri5", 129),
    "dopri5_backward.kinkfree.B65": ("kinkfree", "train", "dopri5", 65),     # the saved path held to the re-integrating one: round-off alone
    "dopri5_backward.kinkfree.B129": ("kinkfree", "train", "dopri5", 129),
    "adaptive_adjoint.dopri5.B65": ("kinkfree", "adjoint", "dopri5", 65),
    "adaptive_adjoint.dopri5.B129": ("kinkfree", "adjoint", "dopri5", 129),
    "adaptive_adjoint.bosh3.B65": ("kinkfree", "adjoint", "bosh3", 65),
    "wide.train.rk4.B65": ("wide", "train", "rk4", 65),
    "wide.train.rk4.B130": ("wide", "train", "rk4", 130),
    "wide.adaptive_forward.dopri5.B130": ("wide", "forward", "dopri5", 130),
}
ADAPTIVE = ("dopri5", "bosh3")
ADJOINT_CASES = [k for k, v in CASES.items() if v[1] == "adjoint" and v[2] in ADAPTIVE]

INDEPENDENT_BATCH = 193
INDEPENDENT_SAMPLES = (0, 63, 64, 127, 128, 192)   # one sample of each slot (first / second of a group) of each pass, and both ends

F64_BATCH, F64_SEED = 129, 71   # the float64 comparison: _wgrad_cases.stack_case(1, 64, F64_METHOD, 2, F64_BATCH, F64_SEED)
F64_METHOD = "midpoint"


def regime(batch):
    """(samples group 0 walks in its first pass, in its second pass, number of groups that walk one sample only in pass one)"""
    first = [b for b in (0, N_GROUPS) if b < batch]
    second = [b for b in (2 * N_GROUPS, 3 * N_GROUPS) if b < batch]
    solo = sum(1 for g in range(N_GROUPS) if g < batch and g + N_GROUPS >= batch)
    return first, second, solo


def _scale_channels(convs):
    """a scale of its own for every output and input channel: a swapped co tile or ci chunk cannot cancel"""
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for c in convs:
            co, ci = c.weight.shape[:2]
            c.weight.mul_((0.5 + torch.rand(co, generator=g))[:, None, None, None] * (0.5 + torch.rand(ci, generator=g))[None, :, None, None])


def func(stack):
    """The dynamics module of a stack (on the CPU)."""
    import ode_rl_amd
    channels, act, head, gain = STACKS[stack]
    if stack == "wide":
        from test_hip_vidode_shapes import _f_v
        f, _ = _f_v()
    else:
        torch.manual_seed(5)
        f = ode_rl_amd.ODEFunc(64, 64, 1, 64, False, act, final_act=head)
    convs = [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == (4 if stack == "wide" else 3)
    if stack == "kinkfree":
        from conftest import procedural_state_dict
        f.load_state_dict(procedural_state_dict(f.state_dict(), 83))
        with torch.no_grad():
            for c in convs[:-1]:
                c.weight.mul_(0.15)
                c.bias.copy_(torch.where(torch.arange(64) % 2 == 0, 2.5, -2.5))
            convs[-1].weight.mul_(4.0)
    if stack != "wide":
        _scale_channels(convs)
    with torch.no_grad():
        convs[-1].weight.mul_(gain)
        convs[-1].bias.mul_(gain)
    return f


def z0(stack, batch):
    return torch.randn(batch, STACKS[stack][0], 16, 16, generator=torch.Generator().manual_seed(200 + batch)) * 0.5


def times(method):
    return torch.tensor(T_ADAPTIVE if method in ADAPTIVE else T_FIXED, dtype=torch.float64)


def gout(stack, batch, n_times):
    return torch.randn(n_times, batch, STACKS[stack][0], 16, 16, generator=torch.Generator().manual_seed(300 + batch))


def solver_kwargs(driver, method):
    """What the library call of a case is given besides (f, z0, t, method=)."""
    if method not in ADAPTIVE:
        return {}
    kw = dict(ADAPTIVE_TOL)
    if driver == "train":
        kw["options"] = {"first_step": FIRST_STEP}
    if driver == "adjoint":
        kw["adjoint_options"] = {"norm": "seminorm"}
    return kw


def cpu_spec(stack):
    """The stack as a spec of tests/_solver_stack_cases.py (dynamics(), _params()): its float32 / float64 restatement on the CPU."""
    _, act, head, _ = STACKS[stack]
    return {"ks": 3, "act": act, "final_act": head, "sd": {k: v.detach().clone() for k, v in func(stack).state_dict().items()}}


def f64_case():
    import _wgrad_cases as wc
    return wc.stack_case(1, 64, F64_METHOD, 2, F64_BATCH, F64_SEED)


def f64_reference(spec):
    """(trajectory, gradients by name, ReLU margin) of float64 autograd through the oracle's solver: _wgrad_cases.stack_reference, which
    does not return the trajectory."""
    import _solver_stack_cases as sc
    from oracle import torchdiffeq_ref
    s = {"ks": 3, "act": "relu", "final_act": False, "sd": spec["sd"]}
    ws, bs = sc._params(s, torch.float64, requires_grad=True)
    margin = [float("inf")]
    z = spec["z0"].detach().double().requires_grad_(True)
    sol = torchdiffeq_ref.odeint(sc.dynamics(s, ws, bs, margin), z, spec["t"], method=spec["method"])
    grads = torch.autograd.grad(sol, [z] + ws + bs, spec["gout"].double())
    out = {"z0": grads[0]}
    out.update({f"w{i}": g for i, g in enumerate(grads[1:1 + len(ws)])})
    out.update({f"b{i}": g for i, g in enumerate(grads[1 + len(ws):])})
    return sol.detach(), out, margin[0]
