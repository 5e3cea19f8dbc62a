"""odeint_adjoint against autograd on an internal grid, at the shape of BASELINE config 2: stack A (64 channels, 5 convolutions),
B = 64, T = 10, rk4, fp32, every interval cut into four equal sub-steps (37 grid points forward and backward; a constructor of its
own: step_size_grid(0.0125) follows torchdiffeq's formula, whose ceil() appends a point one rounding error short of an interval's
end wherever h divides the interval, and internal_grid refuses a grid that does not increase).
  autograd   odeint(..., options=).backward(): the saving forward keeps every activation of the grid in a private workspace
  adjoint    odeint_adjoint(..., options=).backward(): the forward keeps the trajectory; the backward re-integrates on the backward grid
Reported per path: device time of forward + backward (median over 7 groups of 10 calls between HIP events after warm-up), the bytes
torch holds between forward and backward (memory_allocated after the forward minus before it), the peak over the whole step
(max_memory_allocated minus the level before) and the solver workspace sizes the library asks for.  Reported, not gated.
  python tools/grid_adjoint_bench.py [--out FILE] [--batch 64]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402
from ode_rl_amd import _lib, hip_ops  # noqa: E402
from ode_rl_amd.odeint import conv_stack_of  # noqa: E402
from eval_bench import device_ms  # noqa: E402


def quarter_grid(func, y0, t):
    """Every interval of t cut into four equal sub-steps; the points of t themselves bit for bit."""
    k = torch.arange(4, dtype=torch.float64) / 4
    return torch.cat([t[i] + (t[i + 1] - t[i]) * k for i in range(len(t) - 1)] + [t[-1:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_adjoint_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    ode_rl_amd.set_adjoint_grids(True)
    torch.manual_seed(0)
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False).to(dev)
    z0 = (torch.randn(a.batch, 64, 16, 16, generator=torch.Generator().manual_seed(1234)) * 0.5).to(dev)
    t = torch.arange(10, 20, dtype=torch.float64) / 20
    options = {"grid_constructor": quarter_grid}
    gout = torch.randn(10, a.batch, 64, 16, 16, device=dev)
    zg = z0.clone().requires_grad_(True)
    solvers = {"autograd": ode_rl_amd.odeint, "adjoint": ode_rl_amd.odeint_adjoint}
    lib, desc = _lib.load(), conv_stack_of(f).refresh()
    launches = lib.odehip_persistent_trajectory_launches

    def step(solve, probe=None):
        f.zero_grad()
        zg.grad = None
        sol = solve(f, zg, t, method="rk4", options=options)
        if probe is not None:
            torch.cuda.synchronize()
            probe["held_between_forward_and_backward"] = torch.cuda.memory_allocated()
        sol.backward(gout)

    rec = {"device": torch.cuda.get_device_name(0), "shape": {"stack": "A", "B": a.batch, "T": 10, "method": "rk4", "dtype": "fp32",
                                                               "sub_steps_per_interval": 4},
           "method": "median of 7 groups of 10 calls between HIP events after warm-up; bytes from torch's allocator"}
    for name, solve in solvers.items():
        step(solve)                                                       # warm-up: the shared workspaces exist from here on
        torch.cuda.synchronize()
        n0 = launches()
        step(solve)
        torch.cuda.synchronize()
        walks = launches() - n0
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        probe = {}
        step(solve, probe)
        torch.cuda.synchronize()
        med, lo, hi = device_ms(lambda: step(solve), n=10)
        rec[name] = {"forward_backward_ms_median": med, "ms_min": lo, "ms_max": hi, "persistent_launches_per_step": int(walks),
                     "bytes_held_between_forward_and_backward": int(probe["held_between_forward_and_backward"] - base),
                     "bytes_peak_over_the_step": int(torch.cuda.max_memory_allocated() - base)}
    g = hip_ops.last_adjoint_grid["points"]
    rec["grid_points"] = {"forward": len(options["grid_constructor"](None, None, t)), "backward": g}
    rec["workspace_bytes"] = {
        "autograd_private_saving_workspace": int(lib.odehip_odeint_workspace_bytes(ctypes.byref(desc), a.batch, rec["grid_points"]["forward"], 2, 1)),
        "adjoint_shared_backward_workspace": int(hip_ops.last_adjoint_grid["workspace_bytes"]),
        "adjoint_one_step_per_interval_workspace": int(lib.odehip_odeint_workspace_bytes(ctypes.byref(desc), a.batch, 10, 2, 1)),
        "trajectory": int(gout.numel() * 4)}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
