"""Evaluation metrics (csrc/frame_metrics.hip) against two other ways to get the same numbers, on the evaluation shapes:
  * `frame_metrics`: the hand-written launch pair;
  * stock torch ops on the device: the five moment maps stacked, F.conv2d with the 11-tap window along rows and columns;
  * the reference's way restated on the host: per predicted frame F.mse_loss(...).item(), a device -> host copy of the frame batch
    and the float32 SSIM restatement (tests/_metrics_ref.py) once per sample.
Device times are medians over repeated groups of calls between HIP events after a warm-up; the host path is a wall clock around whole
passes that end synchronised.  Launch counts come from torch.profiler (kernels of one call).
Usage: python tools/eval_bench.py [--out FILE]   (shapes (B, T, C) = (4, 180, 1) and (64, 10, 1))"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ode_rl_amd  # noqa: E402
import _metrics_ref as mr  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8e12   # MI355X specification


def device_ms(fn, n=50, warm=10, reps=7):
    """median over `reps` of the mean of n back-to-back calls between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_launches(fn):
    """device kernels of ONE call, by torch.profiler; None if the profiler reports none (not measured)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
             and "memset" not in e.name.lower()]
    return (len(names), sorted(set(names))) if names else (None, [])


def torch_metrics(pred, truth, R, taps):
    """the same five outputs from stock torch ops"""
    b, t, c, h, w = pred.shape
    x, y = pred.reshape(-1, 1, h, w), truth.reshape(-1, 1, h, w)
    m = torch.cat([x, y, x * x, y * y, x * y], 1)
    f = F.conv2d(F.conv2d(m, taps.view(1, 1, 1, -1).expand(5, 1, 1, -1), groups=5), taps.view(1, 1, -1, 1).expand(5, 1, -1, 1), groups=5)
    ux, uy, uxx, uyy, uxy = f.unbind(1)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    ssim_bt = s.mean(dim=(1, 2)).view(b, t, c).mean(2)
    sse = ((pred - truth) ** 2).sum(dim=(2, 3, 4))
    mse = sse.sum(0) / (b * c * h * w)
    return mse, 10 * torch.log10(R * R / mse), ssim_bt.mean(0), sse, ssim_bt


def host_reference_pass(pred, truth):
    """the reference's test() loop body for one batch (train_test.py:104-117) on frames in [-0.5, 0.5]"""
    out = []
    for t in range(pred.shape[1]):
        p, g = pred[:, t], truth[:, t]
        mse = F.mse_loss(p, g).item()
        psnr = 10 * math.log10(1 / mse)
        p255, g255 = ((p + 0.5) * 255.0).squeeze(1).cpu().numpy(), ((g + 0.5) * 255.0).squeeze(1).cpu().numpy()
        ssim = sum(mr.ssim_ref(a, b, 255.0, np.float32) for a, b in zip(p255, g255)) / p.shape[0]
        out.append((mse, psnr, ssim))
    return out


def bench_shape(b, t, c, dev):
    pred_h, truth_h = mr.make_frames(b, t, c, seed=b + t)
    pred, truth = torch.from_numpy(pred_h).to(dev), torch.from_numpy(truth_h).to(dev)
    k = torch.arange(-5, 6, dtype=torch.float64)
    taps = torch.exp(-k * k / (2 * 1.5 ** 2))
    taps = (taps / taps.sum()).float().to(dev)
    rec = {"shape_BTC": [b, t, c], "operand_bytes": 2 * pred.numel() * 4}
    hip = lambda: ode_rl_amd.frame_metrics(pred, truth, 1.0)          # noqa: E731
    stock = lambda: torch_metrics(pred, truth, 1.0, taps)             # noqa: E731
    for name, fn in (("frame_metrics", hip), ("torch_ops", stock)):
        med, lo, hi = device_ms(fn)
        n, names = kernel_launches(fn)
        rec[name] = {"device_us_median": med * 1e3, "device_us_min": lo * 1e3, "device_us_max": hi * 1e3, "kernel_launches": n, "kernels": names}
    a, s = hip(), stock()
    rec["torch_ops_vs_frame_metrics_max_abs_ssim"] = float((a.ssim_per_sample - s[4]).abs().max())
    bound_us = rec["operand_bytes"] / HBM_PEAK_BYTES_PER_S * 1e6
    rec["hbm_bound_us"] = bound_us
    rec["frame_metrics_fraction_of_hbm_bound"] = bound_us / rec["frame_metrics"]["device_us_median"]
    p05, t05 = pred - 0.5, truth - 0.5
    host_reference_pass(p05, t05)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_reference_pass(p05, t05)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    rec["host_reference_way"] = {"wall_ms_median": float(np.median(ts)) * 1e3, "host_syncs": 3 * t, "ssim_calls": b * t * c}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "method": "device: median of 7 groups of 50 calls between HIP events after 10 warm-up calls; host: median wall clock of 3 passes",
           "shapes": [bench_shape(4, 180, 1, dev), bench_shape(64, 10, 1, dev)]}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
