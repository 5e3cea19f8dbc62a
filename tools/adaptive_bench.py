"""dopri5 against bosh3 at the models' own tolerances (DiffEqSolver's rtol 1e-4 / atol 1e-5): time per solve, step counts and error.

Two workloads, the dynamics as bench.py builds them (default initialisation, seed 0): BASELINE configs[0] (5 x conv 64 -> 64, B = 4) and
the Vid-ODE decode shape (128 -> 64 -> 64 -> 128, B = 8), T = 10 output times with intervals of 1 / (2 T).  For each, forward (no_grad) and
forward + backward (loss.backward() through the solver), `--runs` alternating runs per method (dopri5, bosh3, dopri5, ...) in ONE
process; a run is `--solves` solves after two warm-up solves, each timed from enqueue to the end of the device work, and reports their
median.  The error is the rel-L2 distance of the trajectory's increments from a float64 solution at rtol 1e-10 / atol 1e-12 computed on
the CPU with tests/_adaptive_ref.py's dopri5.  One JSON document on stdout / in --out (profiles/bosh3.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

WORKLOADS = {   # name -> (C0, n_layers of ODEFunc, batch)
    "configs[0] (5 x conv 64->64, B=4)": (64, 3, 4),
    "Vid-ODE decode (128->64->64->128, B=8)": (128, 2, 8),
}
RTOL, ATOL = 1e-4, 1e-5


def reference_increments(state, z0, t):
    import torch.nn.functional as F
    import _adaptive_ref as ar
    keys = sorted((k for k in state if k.endswith("weight")), key=lambda k: int(k.split(".")[1]))
    ws = [state[k].double() for k in keys]
    bs = [state[k.replace("weight", "bias")].double() for k in keys]

    def f(tt, y):
        for i, (w, b) in enumerate(zip(ws, bs)):
            y = F.conv2d(y, w, b, padding=1)
            if i < len(ws) - 1:
                y = torch.relu(y)
        return y
    with torch.no_grad():
        sol = ar.odeint(f, z0.double(), t, rtol=1e-10, atol=1e-12, method="dopri5")
    return sol[1:] - z0.double()


def one_run(ode_rl_amd, f, z0, t, method, backward, solves):
    times, stats, sol = [], None, None
    for i in range(solves + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if backward:
            z = z0.clone().requires_grad_(True)
            sol = ode_rl_amd.odeint(f, z, t, rtol=RTOL, atol=ATOL, method=method)
            stats = dict(ode_rl_amd.last_stats)
            sol.square().mean().backward()
        else:
            with torch.no_grad():
                sol = ode_rl_amd.odeint(f, z0, t, rtol=RTOL, atol=ATOL, method=method)
            stats = dict(ode_rl_amd.last_stats)
        torch.cuda.synchronize()
        if i >= 2:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), stats, sol.detach()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--solves", type=int, default=20)
    p.add_argument("--frames", type=int, default=10)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import ode_rl_amd
    dev = torch.device("cuda:0")
    T = a.frames
    t_cpu = torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T)
    doc = {"rtol": RTOL, "atol": ATOL, "frames": T, "runs": a.runs, "solves_per_run": a.solves, "device": torch.cuda.get_device_name(0),
           "workloads": {}}
    for name, (c0, n_layers, batch) in WORKLOADS.items():
        torch.manual_seed(0)
        f = ode_rl_amd.ODEFunc(n_inputs=c0, n_outputs=c0, n_layers=n_layers, n_units=64, downsize=False, nonlinear="relu", final_act=False)
        state = {k: v.detach().clone() for k, v in f.state_dict().items()}
        f = f.to(dev)
        z0_cpu = torch.randn(batch, c0, 16, 16, generator=torch.Generator().manual_seed(1234)) * 0.5
        z0, t = z0_cpu.to(dev), t_cpu.to(dev)
        ref = reference_increments(state, z0_cpu, t_cpu)
        entry = {}
        for leg, backward in (("forward", False), ("forward+backward", True)):
            per = {m: {"median_ms_per_solve": []} for m in ("dopri5", "bosh3")}
            for _ in range(a.runs):
                for m in ("dopri5", "bosh3"):
                    ms, st, sol = one_run(ode_rl_amd, f, z0, t, m, backward, a.solves)
                    per[m]["median_ms_per_solve"].append(round(ms, 4))
                    per[m].update(nfe=st["nfe"], n_accept=st["n_accept"], n_reject=st["n_reject"],
                                  rel_l2_error=float(((sol[1:].double().cpu() - z0_cpu.double()) - ref).norm() / ref.norm()))
            for m in per:
                v = per[m]["median_ms_per_solve"]
                per[m].update(median_of_runs_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
            d, b = per["dopri5"], per["bosh3"]
            separated = d["max_ms"] < b["min_ms"] or b["max_ms"] < d["min_ms"]
            per["faster"] = ("dopri5" if d["median_of_runs_ms"] < b["median_of_runs_ms"] else "bosh3") if separated else "neither (the runs overlap)"
            entry[leg] = per
        doc["workloads"][name] = entry
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
