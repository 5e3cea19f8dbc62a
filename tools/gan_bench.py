"""The adversarial step (models/gan.py, train.train_batch_gan) with fused=True against fused=False -- the same discriminators with
InstanceNorm + LeakyReLU, the sequence assembly and the LSGAN terms as torch compositions -- on the same GPU, at Vid-ODE's shapes:
b = 8, t_in = t = 10, c = 1, 64 x 64, hence 80 images for netD_img and 80 sequences of 11 channels for netD_seq.
  * one discriminator pass each way, per discriminator: netD_adv_loss + backward to its parameters (the D update's work) and
    netG_adv_loss + backward to the prediction with the parameters frozen (the G update's share);
  * the pieces alone: norm + activation forward + backward at the three plane sizes of a pass, the sequence assembly + backward, one
    LSGAN term + backward;
  * one whole train_batch_gan step around a VidODE generator (rk4), both ways.
Device times: median (min, max) over 7 groups of N calls between HIP events after 10 warm-up calls, the two variants alternating
group by group so that drift hits both; launches of one call by torch.profiler.  Reported, not gated.
  python tools/gan_bench.py [--out FILE] [--batch 8] [--frames 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402
from eval_bench import kernel_launches  # noqa: E402


def ab(fused_fn, torch_fn, n=20, warm=10, reps=7):
    """{fused, torch_composition, speedup}: per-call device time of the two callables, alternating group by group"""
    fns = {"fused": fused_fn, "torch_composition": torch_fn}
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / n)
    rec = {}
    for k, fn in fns.items():
        launches, _ = kernel_launches(fn)
        rec[k] = {"us_median": float(np.median(ts[k])) * 1e3, "us_min": min(ts[k]) * 1e3, "us_max": max(ts[k]) * 1e3, "launches": launches}
    rec["speedup"] = rec["torch_composition"]["us_median"] / rec["fused"]["us_median"]
    return rec


def discriminator_passes(b, t, dev):
    from ode_rl_amd.models.gan import Discriminator
    g = torch.Generator().manual_seed(0)
    real, input_real = torch.rand(b, t, 1, 64, 64, generator=g).to(dev), torch.rand(b, t, 1, 64, 64, generator=g).to(dev)
    fake = torch.rand(b, t, 1, 64, 64, generator=g).to(dev).requires_grad_(True)
    rec = {}
    for tag, seq, in_ch in (("netD_img", False, 1), ("netD_seq", True, t + 1)):
        nets = {}
        for fused in (True, False):
            torch.manual_seed(1)
            nets[fused] = Discriminator(in_ch, dev, seq=seq, fused=fused).to(dev)
        nets[False].load_state_dict(nets[True].state_dict())

        def d_pass(net):
            def step():
                torch.autograd.grad(net.netD_adv_loss(real, fake, input_real if seq else None), list(net.parameters()))
            return step

        def g_pass(net):
            def step():
                for p in net.parameters():
                    p.requires_grad_(False)
                torch.autograd.grad(net.netG_adv_loss(real, fake, input_real if seq else None), fake)
                for p in net.parameters():
                    p.requires_grad_(True)
            return step

        rec[tag] = {"d_loss_and_backward": ab(d_pass(nets[True]), d_pass(nets[False])),
                    "g_loss_and_backward": ab(g_pass(nets[True]), g_pass(nets[False]))}
        print(json.dumps({tag: rec[tag]}), flush=True)
    return rec


def pieces(b, t, dev):
    g = torch.Generator().manual_seed(2)
    rec = {}
    n = b * t
    for name, shape in (("norm_act_128x32x32", (n, 128, 32, 32)), ("norm_act_128x16x16", (n, 128, 16, 16)), ("norm_act_256x8x8", (n, 256, 8, 8)),
                        ("norm_act_512x9x9", (n, 512, 9, 9))):
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(shape, generator=g).to(dev)
        row = ab(lambda: torch.autograd.grad(ode_rl_amd.instnorm_lrelu(x), x, gy),
                 lambda: torch.autograd.grad(F.leaky_relu(F.instance_norm(x), 0.2), x, gy), n=50)
        row["compulsory_bytes"] = 5 * 4 * x.numel()     # x read twice, y and grad_x written, grad_y read
        row["fused_bytes_per_s_whole_call"] = row["compulsory_bytes"] / (row["fused"]["us_median"] * 1e-6)
        rec[name] = row
    from ode_rl_amd.models.gan import Discriminator
    input_real = torch.rand(b, t, 1, 64, 64, generator=g).to(dev)
    frames = torch.rand(b, t, 1, 64, 64, generator=g).to(dev).requires_grad_(True)
    gout = torch.rand(b * t, t + 1, 64, 64, generator=g).to(dev)
    plain = Discriminator(t + 1, dev, seq=True, fused=False)
    rec["sequence_assembly"] = ab(lambda: torch.autograd.grad(ode_rl_amd.gan_sequences(input_real, frames), frames, gout),
                                  lambda: torch.autograd.grad(plain.rearrange_seq(None, frames, input_real), frames, gout), n=50)
    pred = torch.randn(b * t, 64, 10, 10, generator=g).to(dev).requires_grad_(True)
    rec["lsgan_term"] = ab(lambda: torch.autograd.grad(ode_rl_amd.lsgan_loss(pred, 1.0), pred),
                           lambda: torch.autograd.grad(torch.mean((pred - torch.ones_like(pred)) ** 2), pred), n=50)
    print(json.dumps(rec), flush=True)
    return rec


def whole_step(b, t, dev):
    from ode_rl_amd import train
    from ode_rl_amd.data import MovingMNISTSynthetic
    from ode_rl_amd.models.gan import create_netD
    from ode_rl_amd.models.VidODE import VidODE
    torch.manual_seed(0)
    opt = argparse.Namespace(n_downs=2, resolution=64, in_channels=1, n_layers=2, decode_diff_method="rk4")
    model = VidODE(opt, torch.device("cpu")).to(dev)
    batch = next(MovingMNISTSynthetic(t, t, num_objects=[2], batch_size=b, device=dev, seed=0))
    ts = torch.arange(2 * t, dtype=torch.float64, device=dev) / (2 * t)
    ones = torch.ones(b, t, 1, device=dev)
    bd = {"observed_tp": ts[:t], "tp_to_predict": ts[t:], "observed_mask": ones, "mask_predicted_data": ones,
          "observed_data": batch["observed_data"], "data_to_predict": batch["data_to_predict"]}
    opt_g = ode_rl_amd.FusedAdamax(model.parameters(), lr=1e-4)
    gan_opt = argparse.Namespace(input_dim=1, lr=1e-4, output_sequence=t, sample_size=2 * t, unequal=False, irregular=False, extrap=True)
    steps = {}
    for fused in (True, False):
        torch.manual_seed(3)
        img, seq, opt_d = create_netD(gan_opt, dev, fused=fused)
        steps[fused] = (lambda img=img, seq=seq, opt_d=opt_d: train.train_batch_gan(model, img, seq, bd, opt_g, opt_d))
    rec = ab(steps[True], steps[False], n=5, warm=3)
    plain = ode_rl_amd.FusedAdamax(model.parameters(), lr=1e-4)
    rec["train_batch_without_gan"] = ab(lambda: train.train_batch(model, bd, plain), lambda: train.train_batch(model, bd, plain), n=5, warm=3)["fused"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gan_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "frames_in": a.frames, "frames_out": a.frames,
           "method": "median (min, max) of 7 groups of N calls between HIP events after warm-up, fused and torch_composition alternating "
                     "group by group (N = 20 for discriminator passes, 50 for the pieces, 5 for whole steps); launches of one call by "
                     "torch.profiler (memcpy / memset not counted); torch_composition = the same modules built with fused=False",
           "discriminator_pass": discriminator_passes(a.batch, a.frames, dev), "pieces": pieces(a.batch, a.frames, dev),
           "train_batch_gan_step": whole_step(a.batch, a.frames, dev)}
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
