"""Cost of the observation mask in the ODE-ConvGRU encoder at the VidODE shape (128 channels, T = 10, B = 4 and B = 64): encode
(inference) and encode + backward (training), three ways -- no mask, an all-ones mask, every second frame unobserved.

  python tools/mask_bench.py [--steps 20] [--variants none,ones,alternate]         one process, one JSON line
  python tools/mask_bench.py --ab OTHER_TREE [--rounds 3] [--out profiles/encoder_mask.json]
      interleaved child processes on one box, as tools/ab_bench.sh does: per round OTHER_TREE (a built checkout of the commit to
      compare against, which need not know the mask: it runs `none` only) twice and this tree once.  The spread OTHER_TREE shows
      against itself is recorded next to the numbers; it is the margin for "not slower".
  python tools/mask_bench.py --skip OTHER_TREE [--rounds 3] [--out profiles/encoder_skip.json]
      what skipping the encoder steps that no sample observed saves: both cell flavours (the 5x5 GroupNorm cell, the norm-free 3x3 cell
      of models/conv_odegru.py), three masks (all observed, every second frame unobserved, 3 of 10 observed), each from the HOST (this
      tree skips) and from the DEVICE (nothing can skip), medians of HIP-event times.  Interleaved with OTHER_TREE (the parent commit:
      it skips nothing wherever the mask lives) as above; all observed must be no slower than the parent beyond the parent's spread
      against itself, alternating faster by more than that spread."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 10, 4), (128, 10, 64)]          # (channels, frames, batch)


def measure(tree, variants, steps):
    sys.path.insert(0, tree)
    import torch
    import ode_rl_amd
    dev = torch.device("cuda", 0)
    out = {}
    for C, T, B in SHAPES:
        torch.manual_seed(0)
        f = ode_rl_amd.ODEFunc(C, C, 2, C // 2, False, "relu", final_act=False)      # models/VidODE.py: n_layers = 2, n_units = ch / 2
        enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), C).to(dev)
        x = torch.randn(T, B, C, 16, 16, device=dev) * 0.5
        t = torch.arange(T, dtype=torch.float64, device=dev) / (2 * T)
        gm, gs = torch.randn(B, C, 16, 16, device=dev), torch.randn(B, C, 16, 16, device=dev)
        masks = {"none": None, "ones": torch.ones(B, T, 1, device=dev),
                 "alternate": (torch.arange(T, device=dev) % 2 == 0).float().expand(B, T).unsqueeze(-1).contiguous()}

        def encode(m):
            with torch.no_grad():
                enc(x, t, m)

        def train(m):
            enc.zero_grad(set_to_none=True)
            mean, std = enc(x, t, m)
            torch.autograd.backward([mean, std], [gm, gs])

        for v in variants:
            for what, fn in (("encode_ms", encode), ("encode_backward_ms", train)):
                for _ in range(3):
                    fn(masks[v])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn(masks[v])
                torch.cuda.synchronize()
                out[f"B{B}.{v}.{what}"] = (time.perf_counter() - t0) / steps * 1e3
    return out


SKIP_MASKS = {"all": [1] * 10, "alternate": [1, 0] * 5, "3of10": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]}


def measure_skip(tree, steps):
    """{B<batch>.<cell>.<mask>.<host|device>.<encode_ms|encode_backward_ms>: median HIP-event time of one call}, and the steps for which
    the last forward launched the cell where the tree reports it."""
    sys.path.insert(0, tree)
    import torch
    import ode_rl_amd
    from ode_rl_amd.models import conv_odegru
    dev = torch.device("cuda", 0)
    out = {}
    for C, T, B in SHAPES:
        torch.manual_seed(0)
        f = ode_rl_amd.ODEFunc(C, C, 2, C // 2, False, "relu", final_act=False)
        gn = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), C).to(dev)
        func = conv_odegru.ODEFunc(None, C, C, conv_odegru.create_convnet(C, C, n_layers=2, n_units=C // 2))    # upstream's set_ode_func_netED
        solver = conv_odegru.DiffeqSolver(C, func, "euler", C, odeint_rtol=1e-3, odeint_atol=1e-4)
        plain = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), C, C, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                                   return_all_layers=True, z0_diffeq_solver=solver, run_backwards=True).to(dev)
        x = torch.randn(T, B, C, 16, 16, device=dev) * 0.5
        xb = x.permute(1, 0, 2, 3, 4).contiguous()
        t = torch.arange(T, dtype=torch.float64) / (2 * T)
        gm, gs = torch.randn(B, C, 16, 16, device=dev), torch.randn(B, C, 16, 16, device=dev)
        calls = {"gn": (gn, lambda m: gn(x, t, m)), "plain": (plain, lambda m: plain(xb, t, mask=m))}
        for cell, (module, call) in calls.items():
            for name, row in SKIP_MASKS.items():
                host = torch.tensor([row] * B, dtype=torch.float32).unsqueeze(-1)
                for where, m in (("host", host), ("device", host.to(dev))):
                    def encode():
                        with torch.no_grad():
                            call(m)

                    def train():
                        module.zero_grad(set_to_none=True)
                        mean, std = call(m)
                        torch.autograd.backward([mean, std], [gm, gs])

                    for what, fn in (("encode_ms", encode), ("encode_backward_ms", train)):
                        for _ in range(3):
                            fn()
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                        for a, b in ev:
                            a.record()
                            fn()
                            b.record()
                        torch.cuda.synchronize()
                        out[f"B{B}.{cell}.{name}.{where}.{what}"] = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
                    out[f"B{B}.{cell}.{name}.{where}.cell_steps"] = getattr(module._packed(), "last_cell_steps", None)
    return out


def skip_ab(other, rounds, steps, out_path):
    def run(tree):
        line = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--measure-skip", "--steps", str(steps)], check=True,
                              stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1]
        print(tree, line, file=sys.stderr, flush=True)
        return json.loads(line)
    runs = {"other_a": [], "other_b": [], "this": []}
    for _ in range(rounds):
        runs["other_a"].append(run(other))
        runs["this"].append(run(HERE))
        runs["other_b"].append(run(other))
    med = lambda rows, k: sorted(r[k] for r in rows)[len(rows) // 2]
    res = {"what": "ODE-ConvGRU encoder forward (encode) and forward + backward at the VidODE shape, median HIP-event ms per call; `host`: the "
                   "mask where the loader leaves it (this tree skips the steps no sample observed), `device`: the same mask on the device "
                   "(nothing can skip)", "channels": 128, "frames": 10, "calls_per_window": steps, "rounds": rounds,
           "other_tree": "the parent commit: it skips nothing wherever the mask lives", "masks": SKIP_MASKS, "rows": []}
    for C, T, B in SHAPES:
        for cell in ("gn", "plain"):
            for what in ("encode_ms", "encode_backward_ms"):
                row = {"batch": B, "cell": cell, "what": what}
                spreads = []
                for name in SKIP_MASKS:
                    k = f"B{B}.{cell}.{name}.host.{what}"
                    base = [r[k] for r in runs["other_a"] + runs["other_b"]]
                    parent = sorted(base)[len(base) // 2]
                    row[name] = {"parent_host": parent, "parent_runs": base, "parent_spread_rel": (max(base) - min(base)) / parent,
                                 "host": med(runs["this"], k), "host_runs": [r[k] for r in runs["this"]],
                                 "device": med(runs["this"], k.replace(".host.", ".device.")),
                                 "cell_steps_host": runs["this"][0][f"B{B}.{cell}.{name}.host.cell_steps"],
                                 "cell_steps_device": runs["this"][0][f"B{B}.{cell}.{name}.device.cell_steps"]}
                    row[name]["host_vs_parent_rel"] = row[name]["host"] / parent - 1.0
                    row[name]["host_vs_device_rel"] = row[name]["host"] / row[name]["device"] - 1.0
                    spreads.append(row[name]["parent_spread_rel"])
                row["all_observed_not_slower_than_parent"] = row["all"]["host_vs_parent_rel"] <= row["all"]["parent_spread_rel"]
                row["alternate_faster_than_parent_by_more_than_its_spread"] = (-row["alternate"]["host_vs_parent_rel"] >
                                                                              row["alternate"]["parent_spread_rel"])
                res["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def child(tree, variants, steps):
    line = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--variants", variants, "--steps", str(steps)],
                          check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1]
    print(tree, variants, line, file=sys.stderr, flush=True)
    return json.loads(line)


def ab(other, rounds, steps, out_path):
    runs = {"other_a": [], "other_b": [], "this": []}
    for _ in range(rounds):
        runs["other_a"].append(child(other, "none", steps))
        runs["this"].append(child(HERE, "none,ones,alternate", steps))
        runs["other_b"].append(child(other, "none", steps))
    med = lambda rows, k: sorted(r[k] for r in rows)[len(rows) // 2]
    res = {"what": "ODEConvGRUCell.forward (encode) and forward + backward at the VidODE shape, ms per call", "channels": 128, "frames": 10,
           "steps_per_window": steps, "rounds": rounds, "other_tree": "the parent commit (no mask support): variant `none` only", "rows": []}
    for C, T, B in SHAPES:
        for what in ("encode_ms", "encode_backward_ms"):
            k = f"B{B}.none.{what}"
            base = [r[k] for r in runs["other_a"] + runs["other_b"]]
            other_med = sorted(base)[len(base) // 2]
            spread = (max(base) - min(base)) / other_med        # what the other tree shows against itself, all its runs of this session
            row = {"batch": B, "what": what, "parent_none": other_med, "parent_runs": base, "parent_spread_rel": spread}
            for v in ("none", "ones", "alternate"):
                row[v] = med(runs["this"], f"B{B}.{v}.{what}")
                row[v + "_runs"] = [r[f"B{B}.{v}.{what}"] for r in runs["this"]]
            row["none_vs_parent_rel"] = row["none"] / other_med - 1.0
            row["ones_vs_none_rel"] = row["ones"] / row["none"] - 1.0
            row["alternate_vs_none_rel"] = row["alternate"] / row["none"] - 1.0
            row["unmasked_not_slower_than_parent"] = row["none_vs_parent_rel"] <= spread
            row["masked_not_slower_than_unmasked"] = max(row["ones_vs_none_rel"], row["alternate_vs_none_rel"]) <= spread
            res["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--variants", default="none,ones,alternate")
    p.add_argument("--tree", default=HERE, help="the checkout to import ode_rl_amd from")
    p.add_argument("--ab", default=None, metavar="OTHER_TREE")
    p.add_argument("--skip", default=None, metavar="OTHER_TREE")
    p.add_argument("--measure-skip", action="store_true", help="one process, one JSON line: the measurements of --skip for --tree")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.skip:
        return skip_ab(os.path.abspath(a.skip), a.rounds, a.steps, a.out or os.path.join(HERE, "profiles", "encoder_skip.json"))
    if a.measure_skip:
        return print(json.dumps(measure_skip(os.path.abspath(a.tree), a.steps)))
    a.out = a.out or os.path.join(HERE, "profiles", "encoder_mask.json")
    if a.ab:
        return ab(os.path.abspath(a.ab), a.rounds, a.steps, a.out)
    print(json.dumps(measure(os.path.abspath(a.tree), a.variants.split(","), a.steps)))


if __name__ == "__main__":
    main()
