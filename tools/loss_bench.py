"""The training losses (csrc/frame_loss.hip) against the torch compositions the models ran before, on the same GPU:
  * kernel launches of one loss + backward with the tensors laid out as each model hands them over (ODEConvGRU and ConvGRU: a
    (T, B) buffer permuted to batch-first; VidODE: the intermediates as a channel slice, the last observed frame as a view), with
    ODEHIP_FUSED_LOSS unset and 0, by torch.profiler;
  * device time of loss + backward at (B, T) = (4, 10), (64, 10), (128, 40), one 64 x 64 channel, for both kinds, and at the large
    size the achieved bytes per second against the compulsory traffic (MSE: pred and truth read twice, grad_pred written once =
    5 N floats; L1 pair: pred, inter, truth twice -- the previous frame is the same truth tensor again -- read forward and backward,
    two gradients written = 10 N floats with all frames selected).
Device times: median (min, max) over 7 groups of 50 calls between HIP events after 10 warm-up calls.  Reported, not gated.
  python tools/loss_bench.py [--out FILE] [--sizes 4x10,64x10,128x40]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402
from eval_bench import device_ms, kernel_launches  # noqa: E402

LATENT = 64 * 256


def mse_case(b, t, dev, with_kl):
    """pred as the decoder leaves it: (T, B, 1, 64, 64) in memory, batch-first by a permute; get_loss reshapes it to (B T, 1, 64, 64),
    or with kl (B,) keeps the batch rows and makes it contiguous"""
    g = torch.Generator().manual_seed(b + t)
    buf = torch.rand(t, b, 1, 64, 64, generator=g).to(dev).requires_grad_(True)
    truth = torch.rand(b, t, 1, 64, 64, generator=g).to(dev)
    kl = (torch.rand(b, generator=g) * 300 + 5).to(dev).requires_grad_(True) if with_kl else None

    def step():
        pred = buf.permute(1, 0, 2, 3, 4)
        if with_kl:
            loss = ode_rl_amd.mse_kl_loss(pred.contiguous(), truth, kl=kl, kl_weight=1.0, latent_elems=LATENT)[0]
        else:
            loss = ode_rl_amd.mse_kl_loss(pred.reshape(b * t, 1, 64, 64), truth.reshape(b * t, 1, 64, 64))[0]
        torch.autograd.grad(loss, [buf] + ([kl] if with_kl else []))
    return step


def l1_case(b, t, dev):
    g = torch.Generator().manual_seed(b * t)
    pred = torch.rand(b, t, 1, 64, 64, generator=g).to(dev).requires_grad_(True)
    outputs = torch.rand(b, t, 4, 64, 64, generator=g).to(dev).requires_grad_(True)
    truth = torch.rand(b, t, 1, 64, 64, generator=g).to(dev)
    observed = torch.rand(b, 2, 1, 64, 64, generator=g).to(dev)
    mask = torch.ones(b, t, 1, device=dev)

    def step():
        loss = ode_rl_amd.vidode_l1_loss(pred, outputs[:, :, 2:3], truth, observed[:, -1], mask)[0]
        torch.autograd.grad(loss, [pred, outputs])
    return step


def ab(step):
    """{fused, torch}: time and launches of `step` with ODEHIP_FUSED_LOSS unset and 0"""
    rec = {}
    for name, value in (("fused", None), ("torch_composition", "0")):
        if value is None:
            os.environ.pop("ODEHIP_FUSED_LOSS", None)
        else:
            os.environ["ODEHIP_FUSED_LOSS"] = value
        med, lo, hi = device_ms(step)
        n, names = kernel_launches(step)
        rec[name] = {"us_median": med * 1e3, "us_min": lo * 1e3, "us_max": hi * 1e3, "launches": n, "kernels": names}
    os.environ.pop("ODEHIP_FUSED_LOSS", None)
    rec["speedup"] = rec["torch_composition"]["us_median"] / rec["fused"]["us_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--sizes", default="4x10,64x10,128x40")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0),
           "method": "loss + backward; median (min, max) of 7 groups of 50 calls between HIP events after 10 warm-up calls; launches of one "
                     "call by torch.profiler (memcpy / memset not counted); torch_composition = the same call with ODEHIP_FUSED_LOSS=0",
           "sizes": []}
    for size in a.sizes.split(","):
        b, t = (int(v) for v in size.split("x"))
        n = b * t * 4096
        row = {"B": b, "T": t, "elements": n,
               "mse": ab(mse_case(b, t, dev, False)), "mse_kl": ab(mse_case(b, t, dev, True)), "vidode_l1": ab(l1_case(b, t, dev))}
        # compulsory traffic of the fused calls themselves (the permuted pred costs one more copy each way, in both columns)
        for key, floats in (("mse", 5 * n), ("mse_kl", 5 * n), ("vidode_l1", 10 * n)):
            row[key]["compulsory_bytes"] = 4 * floats
            row[key]["fused_bytes_per_s_whole_call"] = 4 * floats / (row[key]["fused"]["us_median"] * 1e-6)
        rec["sizes"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
