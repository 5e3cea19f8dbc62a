"""Clipped optimizer step on the ODEConvGRU model's parameter set (40 tensors, 1.04 M parameters), on the same GPU:
  * fused       FusedAdam(max_grad_norm=c).step(): sum of squares -> coefficient -> Adam reading the coefficient (csrc/optim_step.hip)
  * torch_clip  torch.nn.utils.clip_grad_norm_(params, c) followed by the unclipped FusedAdam.step()
  * hip_clip    ode_rl_amd.optim.clip_grad_norm_(params, c) followed by the unclipped FusedAdam.step()
  * unclipped   FusedAdam.step() alone (what clipping adds is the difference)
For each: device kernels of one call by torch.profiler (memcpy / memset not counted), whether the call runs under
torch.cuda.set_sync_debug_mode("error"), and the device time, median (min, max) over 7 groups of 50 calls between HIP events after 10
warm-up calls, the variants alternating group by group; for the fused variant also the mean device time of each kernel (torch.profiler).  The gradients are refilled from a fixed tensor before every call by one
foreach copy, inside the timed window of every variant alike (a clipped step scales them in place).  Reported, not gated.
  python tools/clip_bench.py [--out FILE] [--clip 0.5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402,F401
from eval_bench import kernel_launches  # noqa: E402
from ode_rl_amd.models.ODEConvGRU import ODEConvGRU  # noqa: E402
from ode_rl_amd.optim import FusedAdam, clip_grad_norm_  # noqa: E402


def model_gradients(dev):
    """(parameters, fixed gradients) of the ODEConvGRU model the benchmark and the tests build"""
    opt = argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3, neural_ode_n_units=64,
                             neural_ode_decoder_out_ch=64, decode_diff_method="dopri5", mem=False, z_sample=False)
    torch.manual_seed(0)
    base = [p.detach() for p in ODEConvGRU(opt, torch.device("cpu")).to(dev).parameters()]
    g = torch.Generator().manual_seed(1)
    return base, [torch.randn(p.shape, generator=g).to(dev) for p in base]


def variant(name, base, fixed, clip):
    """one call of variant `name` on its own copy of the parameters: refill the gradients, clip, step"""
    ps = [torch.nn.Parameter(p.clone()) for p in base]
    for p in ps:
        p.grad = torch.empty_like(p)
    grads = [p.grad for p in ps]
    adam = FusedAdam(ps, lr=1e-3, max_grad_norm=clip if name == "fused" else None)

    def call():
        torch._foreach_copy_(grads, fixed)
        if name == "torch_clip":
            torch.nn.utils.clip_grad_norm_(ps, clip)
        elif name == "hip_clip":
            clip_grad_norm_(ps, clip)
        adam.step()
    return call


def refill_only(fixed):
    grads = [torch.empty_like(p) for p in fixed]
    return lambda: torch._foreach_copy_(grads, fixed)


def kernel_us(fn, reps=20):
    """{kernel name: mean device time in us per launch} over `reps` calls, by torch.profiler (tracing on: for the split of a call
    among its kernels, not for its total)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            t = getattr(e, "device_time", None)
            acc.setdefault(e.name, []).append(float(t if t is not None else e.cuda_time))
    return {k: {"launches_per_call": len(v) / reps, "us_mean": sum(v) / len(v)} for k, v in acc.items()}


def runs_without_sync(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn()
        return True
    except RuntimeError:
        return False
    finally:
        torch.cuda.set_sync_debug_mode("default")


def alternating_ms(calls, n=50, warm=10, reps=7):
    """{name: (median, min, max)} of the mean of n back-to-back calls between two events, the variants taking turns group by group"""
    for fn in calls.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / n)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--clip", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    base, fixed = model_gradients(dev)
    calls = {name: variant(name, base, fixed, a.clip) for name in ("fused", "torch_clip", "hip_clip", "unclipped")}
    rec = {"device": torch.cuda.get_device_name(0), "tensors": len(base), "parameters": sum(p.numel() for p in base), "clip": a.clip,
           "method": "one gradient refill (a foreach copy) + the step; median (min, max) of 7 groups of 50 calls between HIP events after 10 "
                     "warm-up calls, variants alternating; launches of one call by torch.profiler (memcpy / memset not counted; the refill's "
                     "kernels are counted in every variant and listed under refill_launches)",
           "variants": {}}
    rec["refill_launches"] = kernel_launches(refill_only(fixed))[0]
    times = alternating_ms(calls)
    for name, fn in calls.items():
        n, names = kernel_launches(fn)
        med, lo, hi = times[name]
        rec["variants"][name] = {"us_median": med * 1e3, "us_min": lo * 1e3, "us_max": hi * 1e3, "launches": n, "kernels": names,
                                 "runs_under_sync_debug_error": runs_without_sync(fn)}
        print(json.dumps({name: rec["variants"][name]}), flush=True)
    rec["fused_kernel_us"] = kernel_us(calls["fused"])
    print(json.dumps({"fused_kernel_us": rec["fused_kernel_us"]}), flush=True)
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
