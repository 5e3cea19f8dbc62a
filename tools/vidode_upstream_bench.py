"""Upstream Vid-ODE's model (ode_rl_amd.models.conv_odegru) fused against its torch composition (`fused=False`) on one GPU:

  * the encoder `Encoder_z0_ODE_ConvGRU` at upstream's shape (128 channels, dynamics of 64 units, 2 hidden layers), t = 10 frames:
    forward (no gradient) and forward + backward;
  * a whole training step `compute_all_losses` + backward of `VidODE` (init_dim 32, n_downs 2, 64 x 64 frames, 10 observed and 10
    predicted frames, dec_diff 'euler', BatchNorm in train());
  * the two two-source 3x3 convolutions of the plain cell on their own (gates: 256 -> 256, candidate: 256 -> 128 channels), timed as
    single launches; t of each, over the fused encoder forward, is the share of the step they take.  They run the direct kernel
    (the F(2x2,3x3) launch serves one source and at most 128 input channels); the share decides whether a two-source form is worth
    building.  The backward's input-gradient convolutions are one-source and not part of this figure.

Batches 4 (upstream's) and 64.  Every figure is the median of HIP-event times over --iters runs after --warmup.  Writes
profiles/vidode_upstream.json.

    python tools/vidode_upstream_bench.py [--iters 20] [--warmup 5] [--out profiles/vidode_upstream.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ode_rl_amd  # noqa: E402
from ode_rl_amd import hip_ops  # noqa: E402
from ode_rl_amd.models import conv_odegru  # noqa: E402

T, CH = 10, 128


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def opt():
    return types.SimpleNamespace(init_dim=32, n_downs=2, n_layers=2, input_size=64, input_dim=1, extrap=True, run_backwards=True,
                                 dec_diff="euler", slot_attention=False, nru=False, nru2=False)


def encoder(fused, dev, state=None):
    func = conv_odegru.ODEFunc(None, CH, CH, conv_odegru.create_convnet(CH, CH, n_layers=2, n_units=CH // 2))
    solver = conv_odegru.DiffeqSolver(CH, func, "euler", CH, odeint_rtol=1e-3, odeint_atol=1e-4, fused=fused)
    enc = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), CH, CH, (3, 3), 2, torch.FloatTensor, batch_first=True, bias=True,
                                             return_all_layers=True, z0_diffeq_solver=solver, run_backwards=True, fused=fused)
    if state is not None:
        enc.load_state_dict(state)
    return enc.to(dev)


def bench_encoder(batch, dev, iters, warmup):
    torch.manual_seed(0)
    base = encoder(True, dev)
    frames = torch.randn(batch, T, CH, 16, 16, device=dev)
    times = torch.linspace(0.0, 0.9, T, dtype=torch.float64)
    mask = torch.ones(batch, T, 1, device=dev)
    out = {}
    for fused in (True, False):
        enc = base if fused else encoder(False, dev, base.state_dict())
        tag = "fused" if fused else "composition"

        def fwd():
            with torch.no_grad():
                return enc(frames, times, mask=mask)

        def fwd_bwd():
            for p in enc.parameters():
                p.grad = None
            mean, std = enc(frames, times, mask=mask)
            (mean.sum() + std.sum()).backward()

        out[f"forward_ms.{tag}"] = median_ms(fwd, iters, warmup)
        out[f"forward_backward_ms.{tag}"] = median_ms(fwd_bwd, iters, warmup)
    # the two-source 3x3 convolutions of one cell step, as single launches
    cell = base.cell_list[0]
    x = hip_ops.nchw_to_q4(frames[:, 0].contiguous())
    h = hip_ops.nchw_to_q4(torch.randn(batch, CH, 16, 16, device=dev))
    wg, wc = hip_ops.pack_conv_weight(cell.conv_gates.weight.detach()), hip_ops.pack_conv_weight(cell.conv_can.weight.detach())
    bg, bc = cell.conv_gates.bias.detach(), cell.conv_can.bias.detach()
    gates = median_ms(lambda: hip_ops.conv_q4(x, wg, bg, 2 * CH, 3, src2=h), iters, warmup)
    cand = median_ms(lambda: hip_ops.conv_q4(x, wc, bc, CH, 3, src2=h), iters, warmup)
    out["two_source_conv3x3_ms"] = {"gates_256_to_256": gates, "candidate_256_to_128": cand, "per_encoder_forward": T * (gates + cand)}
    out["two_source_conv3x3_share_of_fused_forward"] = T * (gates + cand) / out["forward_ms.fused"]
    out["two_source_conv3x3_share_of_fused_forward_backward"] = T * (gates + cand) / out["forward_backward_ms.fused"]
    return out


def bench_model(batch, dev, iters, warmup):
    torch.manual_seed(0)
    base = conv_odegru.VidODE(opt(), dev).train()
    batch_dict = {"observed_data": torch.rand(batch, T, 1, 64, 64, device=dev), "data_to_predict": torch.rand(batch, T, 1, 64, 64, device=dev),
                  "observed_tp": torch.linspace(0.0, 0.45, T, dtype=torch.float64), "tp_to_predict": torch.linspace(0.5, 0.95, T, dtype=torch.float64),
                  "observed_mask": torch.ones(batch, T, 1), "mask_predicted_data": torch.ones(batch, T, 1)}
    out = {}
    for fused in (True, False):
        model = base
        if not fused:
            model = conv_odegru.VidODE(opt(), dev, fused=False).train()
            model.load_state_dict(base.state_dict())

        def step():
            for p in model.parameters():
                p.grad = None
            model.compute_all_losses(dict(batch_dict))["loss"].backward()

        out[f"train_step_ms.{'fused' if fused else 'composition'}"] = median_ms(step, iters, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vidode_upstream.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "frames": T, "encoder_channels": CH, "frame_size": 64, "iters": args.iters,
              "warmup": args.warmup, "timing": "median of HIP-event times, ms", "compute_dtype": ode_rl_amd.current_compute_dtype(), "batches": {}}
    for batch in (4, 64):
        r = {"encoder": bench_encoder(batch, dev, args.iters, args.warmup), "model": bench_model(batch, dev, args.iters, args.warmup)}
        result["batches"][str(batch)] = r
        print(batch, json.dumps(r))
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
