"""Upstream Vid-ODE's evaluation protocol on the device (csrc/png_metrics.hip) timed on the evaluation shapes:
  * `png_metrics` without and with the byte outputs, and `PngEvaluation.update` (the second, accumulating launch included);
  * `frame_metrics` (the ODE-RL protocol) on the same frames, where it accepts them (S = 64);
  * upstream's host route for ONE batch as context: device -> host copy, quantisation, PIL convert('L') per image (the integer
    restatement where Pillow is missing), scipy's Gaussian SSIM per image (what scikit-image calls).  No PNG encoding or file I/O.
Per shape and call: the median over repeated groups of back-to-back calls between HIP events ("device_us": what a caller who enqueues
call after call pays per call), the host's own time to enqueue one call ("enqueue_us": wall clock around the same loop before it
synchronises) and the verdict derived from the two -- a call whose event time is within 15 % of its enqueue time is bound by launch
and host enqueue, any other by the kernel.  Nothing is asserted: the numbers are recorded.
Usage: python tools/png_metrics_bench.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ode_rl_amd  # noqa: E402
import _metrics_ref as mr  # noqa: E402
import _png_metrics_ref as ref  # noqa: E402

SHAPES = [(4, 10, 1, 64), (64, 10, 3, 64), (4, 10, 3, 128), (64, 10, 3, 128)]
HOST_SHAPES = [(4, 10, 1, 64), (4, 10, 3, 128)]


def timed(fn, n=50, warm=10, reps=7):
    """(median device us per call between events, median host enqueue us per call) over `reps` groups of n back-to-back calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        host.append((time.perf_counter() - t0) / n * 1e6)
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) / n * 1e3)
    d, h = float(np.median(dev)), float(np.median(host))
    return {"device_us": d, "device_us_min": float(min(dev)), "device_us_max": float(max(dev)), "enqueue_us": h,
            "bound_by": "launch and host enqueue" if d <= 1.15 * h else "the kernel"}


def host_route(pred, truth, input_norm):
    """upstream's way for one batch, wall clock in ms; also returns the means it finds"""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pb, tb = ref.rgb_bytes(pred.cpu(), input_norm).numpy(), ref.rgb_bytes(truth.cpu(), input_norm).numpy()
    ssim, mse = [], []
    for i in range(pb.shape[0]):
        for j in range(pb.shape[1]):
            if Image is not None:
                lp, lt = (np.asarray(Image.fromarray(v, "RGB").convert("L")) for v in (pb[i, j], tb[i, j]))
            else:
                lp, lt = ref.luma(pb[i, j]), ref.luma(tb[i, j])
            ssim.append(mr.ssim_ref(lt, lp, 255.0, np.float64))
            d = pb[i, j].astype(np.float32) / 255 - tb[i, j].astype(np.float32) / 255
            mse.append(float((d * d).mean()))
    ms = (time.perf_counter() - t0) * 1e3
    return {"wall_ms": ms, "luma_by": "Pillow" if Image is not None else "integer restatement", "avg_ssim": float(np.mean(ssim)),
            "avg_mse": float(np.mean(mse))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_metrics.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for b, t, c, s in SHAPES:
        g = torch.Generator().manual_seed(b + t + c + s)
        truth = (torch.rand((b, t, c, s, s), generator=g) * 2 - 1).to(dev)
        pred = (truth + 0.1 * torch.randn((b, t, c, s, s), generator=g).to(dev)).clamp(-1.2, 1.2)
        ev = ode_rl_amd.PngEvaluation(dev)
        rec = {"B": b, "T": t, "C": c, "S": s, "images": b * t, "input_MB": 2 * pred.numel() * 4 / 1e6,
               "png_metrics": timed(lambda: ode_rl_amd.png_metrics(pred, truth, True)),
               "png_metrics_with_bytes": timed(lambda: ode_rl_amd.png_metrics(pred, truth, True, return_bytes=True)),
               "png_evaluation_update": timed(lambda: ev.update(pred, truth, True))}
        if s == 64:
            p01, x01 = (pred + 1) / 2, (truth + 1) / 2
            rec["frame_metrics"] = timed(lambda: ode_rl_amd.frame_metrics(p01, x01, 1.0))
        if (b, t, c, s) in HOST_SHAPES:
            rec["upstream_host_route"] = host_route(pred, truth, True)
            m = ode_rl_amd.png_metrics(pred, truth, True)
            rec["upstream_host_route"]["device_minus_host_avg_ssim"] = float(m.ssim.mean()) - rec["upstream_host_route"]["avg_ssim"]
        print(json.dumps(rec))
        out["shapes"].append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
