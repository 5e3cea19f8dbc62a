"""Cost of Tanh dynamics against ReLU on the headline shape (BASELINE configs[1]: rk4, B=64, 64 channels, 10 output times, 5 convs
per evaluation): forward trajectory and forward + backward, per variant, interleaved rounds, median ms.
  python tools/tanh_cost.py [--batch 64] [--steps 40] [--rounds 5] > profiles/tanh_cost.json"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"relu": ("relu", False), "tanh": ("tanh", False), "relu_head": ("relu", True), "tanh_head": ("tanh", True)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--frames", type=int, default=10)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    import ode_rl_amd
    dev = torch.device("cuda", 0)
    z0 = torch.randn(a.batch, 64, 16, 16, device=dev) * 0.5
    t = torch.arange(a.frames, 2 * a.frames, dtype=torch.float64) / (2 * a.frames)
    gout = torch.randn(a.frames, a.batch, 64, 16, 16, device=dev)
    funcs = {}
    for name, (act, head) in VARIANTS.items():
        torch.manual_seed(0)
        funcs[name] = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, act, final_act=head).to(dev)

    def fwd(f):
        with torch.no_grad():
            ode_rl_amd.odeint(f, z0, t, method="rk4")

    def train(f):
        z = z0.clone().requires_grad_(True)
        ode_rl_amd.odeint(f, z, t, method="rk4").backward(gout)

    legs = {"forward": fwd, "train": train}
    times = {(leg, n): [] for leg in legs for n in funcs}
    for leg, fn in legs.items():
        for f in funcs.values():
            for _ in range(5):
                fn(f)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            for n, f in funcs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn(f)
                torch.cuda.synchronize()
                times[(leg, n)].append((time.perf_counter() - t0) / a.steps * 1e3)
    n_layers = (a.frames - 1) * 4 * 5
    out = {"shape": {"batch": a.batch, "channels": 64, "frames": a.frames, "method": "rk4", "conv_layers_per_trajectory": n_layers},
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "ms_median": {}, "spread_ms": {}}
    for (leg, n), v in times.items():
        out["ms_median"][f"{leg}.{n}"] = round(statistics.median(v), 4)
        out["spread_ms"][f"{leg}.{n}"] = round(max(v) - min(v), 4)
    for n in funcs:
        if n != "relu":
            d = out["ms_median"][f"forward.{n}"] - out["ms_median"]["forward.relu"]
            out.setdefault("forward_delta_us_per_layer", {})[n] = round(d * 1e3 / n_layers, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
