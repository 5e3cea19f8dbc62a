"""The seminorm adjoint's two drivers, timed for both adaptive methods: the device-steered controller (csrc/adjoint_device.hip) against
the host-driven loop (csrc/adjoint_dopri5.hip; ODEHIP_ADJOINT_DEVICE=0, which the library reads per call).

Workload: BASELINE configs[2]'s shape as bench.py builds it (5 x conv 64 -> 64, default initialisation, seed 0, B = 64, T = 10 output
times with intervals of 1 / (2 T), DiffEqSolver's rtol 1e-4 / atol 1e-5); a step is odeint_adjoint(..., adjoint_options={"norm":
"seminorm"}) and its backward pass.  The protocol of tools/adaptive_bench.py: `--runs` alternating runs per leg (bosh3 device, bosh3
host, dopri5 device, dopri5 host, bosh3 device, ...) in ONE process; a run is `--steps` training steps after two warm-up steps, each
timed from enqueue to the end of the device work, and reports their median.  One JSON document on stdout / in --out
(profiles/bosh3_device_adjoint.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RTOL, ATOL = 1e-4, 1e-5


def one_run(ode_rl_amd, f, z0, t, gout, method, controller, steps):
    if controller == "host":
        os.environ["ODEHIP_ADJOINT_DEVICE"] = "0"
    try:
        times, st = [], None
        for i in range(steps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.zero_grad()
            z = z0.detach().requires_grad_(True)
            sol = ode_rl_amd.odeint_adjoint(f, z, t, rtol=RTOL, atol=ATOL, method=method, adjoint_options={"norm": "seminorm"})
            sol.backward(gout)
            torch.cuda.synchronize()
            st = dict(ode_rl_amd.last_adjoint_stats)
            if i >= 2:
                times.append((time.perf_counter() - t0) * 1e3)
        if st["controller"] != controller:
            raise RuntimeError(f"{method}: asked for the {controller} controller, {st['controller']} ran")
        return statistics.median(times), st
    finally:
        os.environ.pop("ODEHIP_ADJOINT_DEVICE", None)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--frames", type=int, default=10)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import ode_rl_amd
    dev = torch.device("cuda:0")
    T = a.frames
    torch.manual_seed(0)
    f = ode_rl_amd.ODEFunc(n_inputs=64, n_outputs=64, n_layers=3, n_units=64, downsize=False, nonlinear="relu", final_act=False).to(dev)
    z0 = (torch.randn(a.batch, 64, 16, 16, generator=torch.Generator().manual_seed(1234)) * 0.5).to(dev)
    t = (torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T)).to(dev)
    gout = torch.randn(T, a.batch, 64, 16, 16, generator=torch.Generator().manual_seed(99)).to(dev)
    legs = [(m, c) for m in ("bosh3", "dopri5") for c in ("device", "host")]
    per = {f"{m} {c}": {"median_ms_per_step": []} for m, c in legs}
    for _ in range(a.runs):
        for m, c in legs:
            ms, st = one_run(ode_rl_amd, f, z0, t, gout, m, c, a.steps)
            e = per[f"{m} {c}"]
            e["median_ms_per_step"].append(round(ms, 4))
            e.update(backward_nfe=st["nfe"], backward_n_accept=st["n_accept"], backward_n_reject=st["n_reject"])
    for e in per.values():
        v = e["median_ms_per_step"]
        e.update(median_of_runs_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    verdict = {}
    for m in ("bosh3", "dopri5"):
        d, h = per[f"{m} device"], per[f"{m} host"]
        if d["max_ms"] < h["min_ms"]:
            verdict[m] = "device faster (the runs do not overlap)"
        elif h["max_ms"] < d["min_ms"]:
            verdict[m] = "host faster (the runs do not overlap)"
        else:
            verdict[m] = "neither (the runs overlap)"
    doc = {"workload": f"configs[2] shape: 5 x conv 64->64, B={a.batch}, T={T}, seminorm adjoint training step", "rtol": RTOL, "atol": ATOL,
           "runs": a.runs, "steps_per_run": a.steps, "device": torch.cuda.get_device_name(0), "legs": per, "faster": verdict}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
