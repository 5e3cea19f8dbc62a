"""ODEConvGRUCell.forward alone (BASELINE shape: B=64, T_in=10, 64 channels) -- timing and, under rocprofv3, the kernel breakdown.
  python tools/encoder_bench.py [--batch 64] [--frames 10] [--steps 20] [--dtype f32|bf16] [--backward]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--frames", type=int, default=10)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--channels", type=int, default=64)
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    p.add_argument("--backward", action="store_true", help="time forward + backward (gradient through mean and std)")
    a = p.parse_args()
    import ode_rl_amd
    if a.dtype == "bf16":
        ode_rl_amd.set_compute_dtype("bf16")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    C = a.channels
    f = ode_rl_amd.ODEFunc(C, C, 3 if C == 64 else 2, 64, False, "relu", final_act=False)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), C).to(dev)
    x = torch.randn(a.frames, a.batch, C, 16, 16, device=dev) * 0.5
    t = torch.arange(a.frames, dtype=torch.float64, device=dev) / (2 * a.frames)
    gm, gs = torch.randn(a.batch, C, 16, 16, device=dev), torch.randn(a.batch, C, 16, 16, device=dev)

    def step():
        if not a.backward:
            with torch.no_grad():
                return enc(x, t)
        enc.zero_grad(set_to_none=True)
        mean, std = enc(x, t)
        torch.autograd.backward([mean, std], [gm, gs])

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    print(json.dumps({"what": "ODEConvGRUCell.forward" + (" + backward" if a.backward else ""), "batch": a.batch, "frames": a.frames, "channels": C, "dtype": a.dtype, "ms": ms}))


if __name__ == "__main__":
    main()
