"""One training batch of upstream Vid-ODE assembled three ways from the same clips, at upstream's shapes (sample_size 10, regular
extrapolation: 5 observed + 5 predicted frames; batch 4 and 64; 64 x 64 x 1 and 128 x 128 x 3), the batch `get_next_batch` hands to the
model (observed_data, data_to_predict, orignal_data_to_predict):
  * launch        VidODEBatches.render(plan, test_interp=False): one odehip_vidode_batch launch from the resident uint8 store
  * composition   the same dictionary from the same resident store in torch ops on the device: index, flip, permute, float, div,
                  normalise, mask multiplies, clone
  * host          upstream's route: per item a numpy gather, ToTensor, Normalize on the host, stack, split, a host->device copy, the
                  mask multiplies on the device (host clock around a synchronised call; the other two are HIP events)
`launch` and `composition` are timed per call between two HIP events with the index tables already on the device side of the call
(both upload theirs inside the window), the variants alternating, median (min, max) of `--calls` calls after `--warmup`.  An event
pair around a single call also times the host's enqueue work where the device outruns it; `launch_kernel_ms` is therefore also given
as the device time of `--burst` back-to-back launches of the same table over their count.  Bytes per batch are computed from the
shapes (uint8 read, float32 written, the table); the share of HBM bandwidth is those bytes over the kernel time over 8 TB/s.
The only requirement: launch <= composition in the same run.  Everything else is reported.
`--rotate D` adds a leg per shape with upstream's RandomRotation(D) in the batch (one angle per sample, drawn once): the rotated launch
(`rotate=D`, one odehip_vidode_batch_rotated launch), the unrotated launch for context, and the rotated batch composed in torch ops on
the same resident store (index, flip, permute, float, `affine_grid` + `grid_sample` with zeros outside, the clip to each frame's
minimum, div, normalise, mask multiplies, clone -- in float32, so it differs from the launch in the last digits), the three variants
alternating, same event pairs, same requirement: rotated launch <= rotated composition.
  python tools/vidode_data_bench.py [--rotate 10] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ode_rl_amd  # noqa: E402,F401
from ode_rl_amd import vidode_data  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [(4, 64, 64, 1), (64, 64, 64, 1), (4, 128, 128, 3), (64, 128, 128, 3)]
N_CLIPS, CLIP_LEN, SAMPLE = 64, 20, 10


def composition(store, flip_d, frames_d, mask_d, n_obs, norm):
    x = store.data[frames_d]                                           # (B, T, H, W, C) uint8
    x = torch.where(flip_d.view(-1, 1, 1, 1, 1), x.flip(3), x)
    x = x.permute(0, 1, 4, 2, 3).float().div(255)
    if norm:
        x = x.sub(0.5).div(0.5)
    m = mask_d.view(*mask_d.shape, 1, 1, 1)
    obs, orig = m[:, :n_obs] * x[:, :n_obs], x[:, n_obs:].clone()
    return obs, m[:, n_obs:] * orig, orig


def composition_rotated(store, flip_d, frames_d, mask_d, theta_d, n_obs, norm):
    x = store.data[frames_d]                                           # (B, T, H, W, C) uint8
    x = torch.where(flip_d.view(-1, 1, 1, 1, 1), x.flip(3), x)
    b, t, h, w, c = x.shape
    x = x.permute(0, 1, 4, 2, 3).reshape(b * t, c, h, w).float()
    grid = F.affine_grid(theta_d.repeat_interleave(t, 0), (b * t, c, h, w), align_corners=True)
    v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    v = torch.where(v != 0, torch.maximum(v, x.amin(dim=(1, 2, 3), keepdim=True)), v)
    v = v.div(255)
    if norm:
        v = v.sub(0.5).div(0.5)
    v = v.view(b, t, c, h, w)
    m = mask_d.view(*mask_d.shape, 1, 1, 1)
    obs, orig = m[:, :n_obs] * v[:, :n_obs], v[:, n_obs:].clone()
    return obs, m[:, n_obs:] * orig, orig


def rotation_theta(angle, h, w):
    """(B, 2, 3) float32 for `affine_grid(align_corners=True)`: output pixel -> source pixel of a rotation about the frame's centre."""
    a = np.deg2rad(np.asarray(angle, dtype=np.float64))
    ca, sa, cx, cy, z = np.cos(a), np.sin(a), w / 2 - 0.5, h / 2 - 0.5, np.zeros(len(a))
    return torch.from_numpy(np.stack([np.stack([ca, -sa * cy / cx, z], 1), np.stack([sa * cx / cy, ca, z], 1)], 1).astype(np.float32))


def rotate_leg(args, opt, store, plan, n_obs, degrees, dev):
    it_plain = vidode_data.VidODEBatches(opt, store, train=True, hflip=True, seed=0)
    it = vidode_data.VidODEBatches(opt, store, train=True, hflip=True, rotate=degrees, seed=0)
    plan = dict(plan, angle=np.random.RandomState(1).uniform(-degrees, degrees, size=len(plan["flip"])))
    theta = rotation_theta(plan["angle"], store.height, store.width)

    def launch():
        return it.render(plan, test_interp=False)

    def unrotated():
        return it_plain.render(plan, test_interp=False)

    def composed():
        frames_d = vidode_data._upload(torch.from_numpy(plan["frames"].astype(np.int64)), dev)
        mask_d = vidode_data._upload(torch.from_numpy(plan["mask"]), dev)
        flip_d = vidode_data._upload(torch.from_numpy(plan["flip"]), dev)
        return composition_rotated(store, flip_d, frames_d, mask_d, vidode_data._upload(theta, dev), n_obs, True)

    got, comp = launch(), composed()
    keys = ("observed_data", "data_to_predict", "orignal_data_to_predict")
    diffs = torch.cat([(got[k] - x).abs().flatten() for k, x in zip(keys, comp)])
    for _ in range(args.warmup):
        launch(), unrotated(), composed()
    torch.cuda.synchronize()
    t_launch, t_plain, t_comp = [], [], []
    for _ in range(args.calls):
        t_launch.append(event_ms(launch)[0])
        t_plain.append(event_ms(unrotated)[0])
        t_comp.append(event_ms(composed)[0])
    names, parts, _ = it.layout(plan, False)

    def burst():
        for _ in range(args.burst):
            it._launch(plan["flip"], parts, plan["angle"])

    burst_ms, _ = event_ms(burst)
    return {"degrees": degrees, "launch": stats(t_launch), "unrotated_launch": stats(t_plain), "composition": stats(t_comp),
            "launch_kernel_ms": burst_ms / args.burst, "burst": args.burst,
            "composition_over_launch": statistics.median(t_comp) / statistics.median(t_launch),
            "launch_over_unrotated": statistics.median(t_launch) / statistics.median(t_plain),
            "max_abs_diff_vs_composition": float(diffs.max()), "mean_abs_diff_vs_composition": float(diffs.mean()),
            "launch_not_slower_than_composition": statistics.median(t_launch) <= statistics.median(t_comp)}


def host_route(clips, plan, n_obs, norm, dev):
    items = []
    for c, rel, flip in zip(plan["clips"], plan["rel"], plan["flip"]):
        frames = clips[int(c)][rel]
        if flip:
            frames = frames[..., ::-1, :].copy()
        v = torch.from_numpy(np.rollaxis(frames, axis=-1, start=-3)).float().div(255)
        items.append(v.sub_(torch.FloatTensor([0.5]).view(1, 1, 1)).div_(torch.FloatTensor([0.5]).view(1, 1, 1)) if norm else v)
    data = torch.stack(items)
    mask = torch.from_numpy(plan["mask"]).unsqueeze(-1)
    obs, pred = data[:, :n_obs].clone().to(dev), data[:, n_obs:].clone().to(dev)
    orig = pred.clone()
    return mask[:, :n_obs].unsqueeze(-1).unsqueeze(-1).to(dev) * obs, mask[:, n_obs:].unsqueeze(-1).unsqueeze(-1).to(dev) * pred, orig


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "calls": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--rotate", type=float, help="degrees: add the rotated leg")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vidode_data_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "sample_size": SAMPLE, "mode": "regular extrapolation, input_norm, hflip",
              "outputs": ["observed_data", "data_to_predict", "orignal_data_to_predict"], "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for batch, h, w, c in SHAPES:
        rng = np.random.RandomState(h + c)
        clips = [rng.randint(0, 256, size=(CLIP_LEN, h, w, c)).astype(np.uint8) for _ in range(N_CLIPS)]
        store = vidode_data.ClipStore(clips, device=dev)
        opt = types.SimpleNamespace(window_size=SAMPLE, sample_size=SAMPLE, irregular=False, extrap=True, batch_size=batch, input_norm=True)
        it = vidode_data.VidODEBatches(opt, store, train=True, hflip=True, seed=0)
        random.seed(0)
        np.random.seed(0)
        plan, n_obs = it.draw(), it.n_observed
        plan["mask"][:, 1::3] = 0.0     # a mask with zeros, so the multiplies have something to do

        def launch():
            return it.render(plan, test_interp=False)

        def composed():
            frames_d = vidode_data._upload(torch.from_numpy(plan["frames"].astype(np.int64)), dev)
            mask_d = vidode_data._upload(torch.from_numpy(plan["mask"]), dev)
            flip_d = vidode_data._upload(torch.from_numpy(plan["flip"]), dev)
            return composition(store, flip_d, frames_d, mask_d, n_obs, True)

        got, comp = launch(), composed()
        keys = ("observed_data", "data_to_predict", "orignal_data_to_predict")
        diff = max(float((got[k] - x).abs().max()) for k, x in zip(keys, comp))
        hostd = host_route(clips, plan, n_obs, True, dev)
        host_equal = all(torch.equal(got[k], x) for k, x in zip(keys, hostd))
        for _ in range(args.warmup):
            launch(), composed()
        torch.cuda.synchronize()
        t_launch, t_comp = [], []
        for _ in range(args.calls):
            t_launch.append(event_ms(launch)[0])
            t_comp.append(event_ms(composed)[0])
        names, parts, _ = it.layout(plan, False)

        def burst():
            for _ in range(args.burst):
                it._launch(plan["flip"], parts)

        burst_ms, _ = event_ms(burst)
        t_host = []
        for _ in range(args.host_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(clips, plan, n_obs, True, dev)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) * 1e3)
        slots = sum(f.shape[1] for f, _ in parts) * batch
        table_bytes = 4 * (batch + 2 * slots)
        bytes_moved = slots * h * w * c * (1 + 4) + table_bytes + 1024
        kernel_ms = burst_ms / args.burst
        entry = {"batch": batch, "height": h, "width": w, "channels": c, "launch": stats(t_launch), "composition": stats(t_comp),
                 "host_route": stats(t_host), "launch_kernel_ms": kernel_ms, "burst": args.burst,
                 "composition_over_launch": statistics.median(t_comp) / statistics.median(t_launch),
                 "host_over_launch": statistics.median(t_host) / statistics.median(t_launch),
                 "bytes_per_batch": bytes_moved, "bytes_read_uint8": slots * h * w * c, "bytes_written_f32": 4 * slots * h * w * c,
                 "achieved_bytes_per_s": bytes_moved / (kernel_ms * 1e-3), "hbm_fraction_of_peak": bytes_moved / (kernel_ms * 1e-3) / HBM_PEAK,
                 "max_abs_diff_vs_composition": diff, "bitwise_equal_to_host_route": host_equal,
                 "launch_not_slower_than_composition": statistics.median(t_launch) <= statistics.median(t_comp)}
        if args.rotate is not None:
            entry["rotate"] = rotate_leg(args, opt, store, plan, n_obs, args.rotate, dev)
        print(json.dumps(entry))
        result["shapes"].append(entry)
        del store, it, clips
    result["requirement_met"] = all(e["launch_not_slower_than_composition"] and e.get("rotate", e)["launch_not_slower_than_composition"]
                                    for e in result["shapes"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if not result["requirement_met"]:
        raise SystemExit("vidode_data_bench: the launch is slower than the device composition")


if __name__ == "__main__":
    main()
