"""Sampled z0 (csrc/latent_sample.hip) against the torch composition of the same step on the same GPU, and what `opt.z_sample` costs a
training step:
  * `sample_z0` forward and forward + backward at (B, K) = (4, 1), (64, 1), (64, 3), C = 64;
  * torch: randn_like, addcmul, the KL formula, and autograd through them;
  * `train_batch`-style steps (zero_grad, forward, loss, backward, FusedAdam) of the ODEConvGRU at B = 4 and B = 64, rk4, 10 -> 10 frames,
    with z_sample off and on (K = 1).
Device times: median over 7 groups of 50 calls between HIP events after 10 warm-up calls; training steps: wall clock over --steps
synchronised steps.  Launch counts by torch.profiler (kernels of one call).  Reported, not gated.
  python tools/latent_bench.py [--out FILE] [--steps 10] [--only-step on|off]   (--only-step: ONE training step and nothing else, for
  a kernel trace of the step with z_sample on or off)"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402
from eval_bench import device_ms, kernel_launches  # noqa: E402


def torch_sample(mean, std, k):
    m, s = (mean.repeat(k, 1, 1, 1), std.repeat(k, 1, 1, 1)) if k > 1 else (mean, std)
    z0 = torch.addcmul(m, s, torch.randn_like(m))
    kl = (0.5 * (mean * mean + std * std - 1.0) - torch.log(std)).sum((1, 2, 3))
    return z0, kl


def bench_op(b, k, dev):
    g = torch.Generator().manual_seed(b + k)
    mean = torch.randn(b, 64, 16, 16, generator=g).to(dev).requires_grad_(True)
    std = (torch.rand(b, 64, 16, 16, generator=g) * 1.5 + 0.25).to(dev).requires_grad_(True)
    gz, gkl = torch.randn(k * b, 64, 16, 16, device=dev), torch.randn(b, device=dev)
    rec = {"B": b, "K": k, "C": 64}

    def fwd(fn):
        with torch.no_grad():
            return fn()

    def both(fn):
        z0, kl = fn()
        torch.autograd.grad([z0, kl], [mean, std], [gz, gkl])

    for name, fn in (("sample_z0", lambda: ode_rl_amd.sample_z0(mean, std, n_samples=k)), ("torch_ops", lambda: torch_sample(mean, std, k))):
        f_med, f_lo, f_hi = device_ms(lambda: fwd(fn))
        t_med, t_lo, t_hi = device_ms(lambda: both(fn))
        rec[name] = {"forward_us_median": f_med * 1e3, "forward_us_min": f_lo * 1e3, "forward_us_max": f_hi * 1e3,
                     "forward_backward_us_median": t_med * 1e3, "forward_backward_us_min": t_lo * 1e3, "forward_backward_us_max": t_hi * 1e3,
                     "forward_launches": kernel_launches(lambda: fwd(fn))[0], "forward_backward_launches": kernel_launches(lambda: both(fn))[0]}
    return rec


def make_step(batch, z_sample, dev):
    from ode_rl_amd.data import MovingMNISTSynthetic
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    from ode_rl_amd.optim import FusedAdam
    torch.manual_seed(0)
    opt = argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3, neural_ode_n_units=64,
                             neural_ode_decoder_out_ch=64, decode_diff_method="rk4", mem=False, z_sample=z_sample)
    m = ODEConvGRU(opt, torch.device("cpu")).to(dev).train()
    T = 10
    bd = next(MovingMNISTSynthetic(T, T, num_objects=[2], batch_size=batch, device=dev, seed=0))
    frames, truth = bd["observed_data"] + 0.5, bd["data_to_predict"] + 0.5
    ts = torch.arange(2 * T, dtype=torch.float64, device=dev) / (2 * T)
    tp = {"observed_tp": ts[:T], "tp_to_predict": ts[T:]}
    optim = FusedAdam(m.parameters(), lr=1e-4)

    def step():
        optim.zero_grad()
        loss = m.get_loss(m.get_prediction(frames, batch_dict=tp), truth)
        loss.backward()
        optim.step()
        return loss
    return step


def bench_step(batch, steps, dev):
    rec = {"batch": batch, "frames": "10 -> 10", "method": "rk4"}
    for z in (False, True):
        step = make_step(batch, z, dev)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        key = "z_sample_on" if z else "z_sample_off"
        rec[key] = {"train_step_ms": (time.perf_counter() - t0) / steps * 1e3, "kernel_launches": kernel_launches(step)[0], "last_loss": float(loss)}
    rec["extra_launches_with_z_sample"] = rec["z_sample_on"]["kernel_launches"] - rec["z_sample_off"]["kernel_launches"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only-step", choices=["on", "off"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    if a.only_step:
        step = make_step(4, a.only_step == "on", dev)
        print(json.dumps({"z_sample": a.only_step, "loss": float(step())}))
        return
    rec = {"device": torch.cuda.get_device_name(0),
           "method": "ops: median of 7 groups of 50 calls between HIP events after 10 warm-up calls; steps: wall clock per synchronised step",
           "ops": [bench_op(4, 1, dev), bench_op(64, 1, dev), bench_op(64, 3, dev)],
           "train_step": [bench_step(4, a.steps, dev), bench_step(64, a.steps, dev)]}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
