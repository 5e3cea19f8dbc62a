"""Bit identity of the weight-gradient paths of two builds of the library (csrc/wgrad*.hip).

  ODEHIP_LIB=<lib.so> python tools/wgrad_ab.py run <out.pt> [--off]     gradients of every case from fixed seeds, in this (fresh) process;
                                                                        --off: only the cases marked for it, with the Winograd-domain
                                                                        weight gradients switched off (the direct fp32 kernels)
  python tools/wgrad_ab.py compare <a.pt> <b.pt>                        torch.equal on every tensor; exit status 1 on a difference

Cases run through the builders of tests/_wgrad_cases.py (shared with tests/test_hip_wgrad.py) at the smallest shapes at which each
path can still go wrong; the sums are deterministic by design, so there is no tolerance."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _wgrad_cases as wc   # noqa: E402  (the one set of case builders, shared with tests/test_hip_wgrad.py)


def _stack_grads(dev, n_units, method, T, B, seed, n_layers=3):   # the module's own initialisation under a fixed seed
    import torch
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    spec = {"n_layers": n_layers, "n_units": n_units, "method": method, "sd": None, "z0": torch.randn(B, 64, 16, 16, generator=g) * 0.5,
            "t": torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T), "gout": torch.randn(T, B, 64, 16, 16, generator=g)}
    return list(wc.stack_grads(dev, spec).values())


def _module_grads(module, inputs, outputs):
    import torch
    g = torch.Generator().manual_seed(77)
    outputs = [o for o in outputs if o is not None and o.requires_grad]
    torch.autograd.backward(outputs, [torch.randn(o.shape, generator=g).to(o.device) for o in outputs])
    return [x.grad for x in inputs] + [p.grad for _, p in sorted(module.named_parameters())]


def _encoder_grads(dev, T=2, B=2, ch=64):   # ODE-ConvGRU encoder: 3x3 dynamics, the 5x5 cell (128 gate outputs, two input halves), 1x1 heads
    import torch
    import ode_rl_amd
    torch.manual_seed(3)
    f = ode_rl_amd.ODEFunc(n_inputs=ch, n_outputs=ch, n_layers=3, n_units=ch, downsize=False, nonlinear="relu", final_act=False)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), ch).to(dev)
    x = (torch.randn(T, B, ch, 16, 16, generator=torch.Generator().manual_seed(11)) * 0.5).to(dev).requires_grad_(True)
    mean, std = enc(x, (torch.arange(T, dtype=torch.float64) / 8).to(dev))
    return _module_grads(enc, [x], [mean, std])


def _cell_grads(dev, driver, ch=64):   # "step": the per-step driver (convgru_backward.hip); "rollout": the whole-sequence one (convgru_sequence.hip)
    import torch
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    spec = {"I": ch, "H": ch, "ks": 5, "driver": driver, "T": 2, "sd": None, "x": torch.randn(2, 2, ch, 16, 16, generator=g) * 0.5,
            "h0": torch.randn(2, ch, 16, 16, generator=g) * 0.5, "gw": torch.randn(2, 2, ch, 16, 16, generator=g),
            "gl": torch.randn(2, ch, 16, 16, generator=g)}
    return list(wc.cell_grads(dev, spec).values())


def run(out_path, off):
    if off:
        os.environ["ODEHIP_WGRAD_WINO"] = os.environ["ODEHIP_WGRAD_WINO5"] = "0"
    import torch
    import ode_rl_amd
    dev = torch.device("cuda:0")
    lib = ode_rl_amd._lib.load()
    res = {}
    # esplit = 4 > n_eval = 2: some workgroups write all-zero slabs
    res["stack64.euler.T3.B3"] = _stack_grads(dev, 64, "euler", 3, 3, 20)
    # a 128-channel hidden layer: the co0 and ci0 loops take two steps each
    res["stack128.euler.T2.B1"] = _stack_grads(dev, 128, "euler", 2, 1, 22, n_layers=1)
    res["encoder.C64.T2.B2"] = _encoder_grads(dev)
    res["cell_step.C64.B2"] = _cell_grads(dev, "step")
    res["cell_sequence.C64.T2.B2"] = _cell_grads(dev, "rollout")
    if not off:
        res["stack64.rk4.T3.B20"] = _stack_grads(dev, 64, "rk4", 3, 20, 21)   # esplit = 8 = n_eval
        ode_rl_amd.set_compute_dtype("bf16")
        was = lib.odehip_set_persistent_trajectory(0)
        try:
            res["bf16.stack64.per_evaluation.T3.B3"] = _stack_grads(dev, 64, "rk4", 3, 3, 23)    # bf16 operands rounded from fp32 saves
            lib.odehip_set_persistent_trajectory(1)
            res["bf16.stack64.whole_trajectory.T17.B3"] = _stack_grads(dev, 64, "rk4", 17, 3, 24)   # Q4h operands, two segments: accumulate
            res["bf16.encoder.C64.T2.B2"] = _encoder_grads(dev)
            res["bf16.cell_step.C64.B2"] = _cell_grads(dev, "step")
            res["bf16.cell_sequence.C64.T2.B2"] = _cell_grads(dev, "rollout")
        finally:
            lib.odehip_set_persistent_trajectory(was)
            ode_rl_amd.set_compute_dtype(None)
    torch.cuda.synchronize()
    saved = {k: [None if g is None else g.detach().cpu() for g in v] for k, v in res.items()}
    for k, v in saved.items():
        assert all(g is None or bool(torch.isfinite(g).all()) for g in v), k
    torch.save(saved, out_path)
    print(f"{ode_rl_amd._lib.LIB_PATH}: {len(saved)} cases, {sum(len(v) for v in saved.values())} tensors -> {out_path}")


def compare(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = 0
    for k in a:
        assert len(a[k]) == len(b[k]), k
        same = [(x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a[k], b[k])]
        bad += same.count(False)
        print(f"{k}: {len(same)} tensors, {same.count(True)} bitwise equal" + ("" if all(same) else f"  DIFFER at {[i for i, s in enumerate(same) if not s]}"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], "--off" in sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
