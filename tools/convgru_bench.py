"""ConvGRU baseline: the sequence path (csrc/convgru_sequence.hip, ConvGRUCell.rollout) against the route the cell offered before it,
`ConvGRUCell.forward` in its Python loop (one C-ABI call, a fresh zero frame and a stack entry per step), same process, interleaved:
  * a rollout of the decoder cell (64 / 64, no input) at (T, B) = (190, 4), (10, 4), (10, 64), forward only;
  * the whole model's training step (forward, loss, backward, FusedAdam) at B = 4 and 64, the baseline route being the same model
    with both cells' `rollout` bound to `forward`.
Times are HIP events around groups of calls after a warm-up; per size the two routes alternate group by group and the median of
the groups is reported (with min and max).
Usage: python tools/convgru_bench.py [--out FILE] [--groups 7]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ode_rl_amd  # noqa: E402
from ode_rl_amd import train  # noqa: E402
from ode_rl_amd.models import ConvGRU  # noqa: E402
from ode_rl_amd.optim import FusedAdam  # noqa: E402


def interleaved_ms(fns, n, warm, groups):
    """{name: (median, min, max)} of the mean time of n back-to-back calls; the routes take turns group by group"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / n)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def record(times):
    out = {k: {"ms_median": m, "ms_min": lo, "ms_max": hi} for k, (m, lo, hi) in times.items()}
    out["step_loop_over_sequence"] = times["step_loop"][0] / times["sequence"][0]
    return out


def bench_rollout(T, B, dev, groups):
    torch.manual_seed(T + B)
    cell = ode_rl_amd.ConvGRUCell((16, 16), 64, 64, 5).to(dev)
    h = torch.randn(B, 64, 16, 16, device=dev) * 0.5
    with torch.no_grad():
        fns = {"sequence": lambda: cell.rollout(None, h, T), "step_loop": lambda: cell(None, h, T)}
        n = 3 if T > 100 else 20
        rec = record(interleaved_ms(fns, n, 3, groups))
        a, b = fns["sequence"]()[0], fns["step_loop"]()[0]
    rec.update(T=T, B=B, calls_per_group=n, bitwise_equal=bool(torch.equal(a, b)))
    return rec


def bench_train(B, dev, groups):
    opt = argparse.Namespace(convgru_out_ch=64, conv_encoder_out_ch=64, in_channels=1, phase="train", train_in_seq=10, train_out_seq=10,
                             test_in_seq=10, test_out_seq=190, batch_size=B, depth=1, resolution=64)
    g = torch.Generator().manual_seed(B)
    batch = {"observed_data": (torch.rand(B, 10, 1, 64, 64, generator=g) - 0.5).to(dev),
             "data_to_predict": (torch.rand(B, 10, 1, 64, 64, generator=g) - 0.5).to(dev)}
    fns = {}
    for name in ("sequence", "step_loop"):
        torch.manual_seed(7)
        model = ConvGRU(opt, dev)
        if name == "step_loop":   # the route of the parent commit: the cells' step-by-step forward
            for cell in (model.encoder.conv_gru_cells[0], model.decoder.conv_gru_cells[0]):
                cell.rollout = (lambda c: lambda x=None, h=None, seq_len=10, dim=0: c(x, h, seq_len, dim=dim))(cell)
        optim = FusedAdam(model.parameters(), lr=1e-4)
        fns[name] = (lambda m, o: lambda: train.train_batch(m, batch, o))(model, optim)
    rec = record(interleaved_ms(fns, 5, 3, groups))
    rec.update(B=B, calls_per_group=5)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--groups", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convgru_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0),
           "method": f"median of {a.groups} groups of back-to-back calls between HIP events after 3 warm-up calls; the two routes alternate "
                     "group by group in one process",
           "rollout_decoder_cell_64_64": [bench_rollout(T, B, dev, a.groups) for T, B in ((190, 4), (10, 4), (10, 64))],
           "train_step_model": [bench_train(B, dev, a.groups) for B in (4, 64)]}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
