"""Cost of Tanh dynamics in bf16 compute mode next to ReLU, at bench.py's bf16 size (rk4, B = 128, 40 frames, the 64-channel
stack): one inference trajectory and one training step (forward + backward) per activation, the median of `--reps` timed
repetitions of `--steps` calls each.  Prints one JSON line.  (bench.py itself times the ReLU stack only; the ReLU figures here
are for the ratio, the record's ReLU numbers come from bench.py through tools/ab_bench.sh.)

  python tools/bf16_tanh_cost.py [--batch 128] [--frames 40] [--steps 20] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--frames", type=int, default=40)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    import ode_rl_amd
    dev = torch.device("cuda:0")
    ode_rl_amd.set_compute_dtype("bf16")
    ode_rl_amd.set_bf16_tanh(True)
    z0 = torch.randn(a.batch, 64, 16, 16, device=dev) * 0.5
    t = torch.arange(a.frames, 2 * a.frames, dtype=torch.float64) / (2 * a.frames)
    gout = torch.randn(a.frames, a.batch, 64, 16, 16, device=dev)
    out = {"batch": a.batch, "frames": a.frames, "method": "rk4", "dtype": "bf16", "steps": a.steps, "reps": a.reps}
    for act in ("relu", "tanh"):
        torch.manual_seed(0)
        f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, act, final_act=False).to(dev)

        def infer():
            with torch.no_grad():
                ode_rl_amd.odeint(f, z0, t, method="rk4")

        def train():
            f.zero_grad(set_to_none=True)
            z = z0.clone().requires_grad_(True)
            ode_rl_amd.odeint(f, z, t, method="rk4").backward(gout)

        for name, fn in (("infer", infer), ("train", train)):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / a.steps)
            out[f"{act}_{name}_ms"] = round(statistics.median(ms), 4)
            out[f"{act}_{name}_ms_all"] = [round(v, 4) for v in ms]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
