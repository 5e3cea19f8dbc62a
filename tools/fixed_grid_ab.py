"""Bit identity of the fixed-grid solve, its reverse sweep and its adjoint between two builds of the library (csrc/fixed_grid.hip,
fixed_tableau.h, fstack_bf16.hip, btraj_bf16.hip).

  ODEHIP_LIB=<lib.so> python tools/fixed_grid_ab.py run <out.pt>     every case from fixed seeds, in this (fresh) process
  python tools/fixed_grid_ab.py compare <a.pt> <b.pt>                torch.equal on every tensor; exit status 1 on a difference

Cases: a 64-channel, 3-layer ODEFunc; euler / midpoint / rk4; forward, forward on a decreasing grid (negated dynamics), saving
forward + backward, odeint_adjoint; the persistent walk on and off; B = 3 (sixteen-workgroup walk) and 20 (four-workgroup walk);
T = 2 and 4, T = 1 once per path; B = 20 at T = 2 with the strip walk switched off (the four-workgroup co-tile walk at one sample
per group); rk4 forward + backward at T = 2 with a batch two above the number of groups (two groups carry two samples); one
forward + backward on an internal grid; bf16: forward of the three methods, rk4 training
through the whole-trajectory launches at T = 4 and at T = 17 (the sweep cut into two segments).  The arithmetic is deterministic,
so there is no tolerance."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _case(dev, path, method, B, T, seed, options=None):
    import torch
    import ode_rl_amd
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    z0 = (torch.randn(B, 64, 16, 16, generator=g) * 0.5).to(dev)
    t = (torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T)).to(dev)
    gout = torch.randn(T, B, 64, 16, 16, generator=g).to(dev)
    if path in ("forward", "negate"):
        with torch.no_grad():
            return [ode_rl_amd.odeint(f, z0, t.flip(0) if path == "negate" else t, method=method)]
    z0.requires_grad_(True)
    if path == "adjoint":
        out = ode_rl_amd.odeint_adjoint(f, z0, t, method=method)
    else:
        out = ode_rl_amd.odeint(f, z0, t, method=method, options=options)
    out.backward(gout)
    return [out.detach(), z0.grad] + [p.grad for _, p in sorted(f.named_parameters())]


def run(out_path):
    import torch
    import ode_rl_amd
    dev = torch.device("cuda:0")
    lib = ode_rl_amd._lib.load()
    res = {}
    seed = 100
    paths = ("forward", "negate", "train", "adjoint")
    for persistent in (1, 0):
        was = lib.odehip_set_persistent_trajectory(persistent)
        try:
            for method in ("euler", "midpoint", "rk4"):
                for path in paths:
                    for B in (3, 20):
                        for T in (2, 4):
                            seed += 2
                            res[f"{path}.{method}.B{B}.T{T}.persistent{persistent}"] = _case(dev, path, method, B, T, seed)
        finally:
            lib.odehip_set_persistent_trajectory(was)
    for path in paths:
        seed += 2
        res[f"{path}.rk4.B3.T1"] = _case(dev, path, "rk4", 3, 1, seed)
    # the four-group co-tile walk at one sample per group (the strip walk takes these batches unless it is switched off) ...
    was = lib.odehip_set_strip_walk(0)
    try:
        n0 = lib.odehip_strip_walk_launches()
        for method in ("euler", "rk4"):
            for path in paths:
                seed += 2
                res[f"{path}.{method}.B20.T2.strip_off"] = _case(dev, path, method, 20, 2, seed)
        assert lib.odehip_strip_walk_launches() == n0, "the strip walk ran although it was switched off"
    finally:
        lib.odehip_set_strip_walk(was)
    # ... and with two samples in a group: a batch just above the number of groups (a group is four workgroups, the grid a
    # multiple of 32 workgroups), so two groups carry two samples
    n_groups = torch.cuda.get_device_properties(dev).multi_processor_count // 32 * 8
    res[f"train.rk4.B{n_groups + 2}.T2.two_samples_per_group"] = _case(dev, "train", "rk4", n_groups + 2, 2, 890)
    res["train.rk4.B3.T3.internal_grid"] = _case(dev, "train", "rk4", 3, 3, 900,
                                                 options={"grid_constructor": ode_rl_amd.step_size_grid(0.07)})
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        for method in ("euler", "midpoint", "rk4"):
            res[f"bf16.forward.{method}.B3.T4"] = _case(dev, "forward", method, 3, 4, 910)
        before = lib.odehip_persistent_trajectory_launches()
        res["bf16.train.rk4.B3.T4"] = _case(dev, "train", "rk4", 3, 4, 920)
        res["bf16.train.rk4.B3.T17.two_segments"] = _case(dev, "train", "rk4", 3, 17, 930)
        assert lib.odehip_persistent_trajectory_launches() > before, "the bf16 training cases did not take the whole-trajectory launch"
    finally:
        ode_rl_amd.set_compute_dtype(None)
    torch.cuda.synchronize()
    saved = {k: [x.detach().cpu() for x in v] for k, v in res.items()}
    for k, v in saved.items():
        assert all(bool(torch.isfinite(x).all()) for x in v), k
    torch.save(saved, out_path)
    print(f"{ode_rl_amd._lib.LIB_PATH}: {len(saved)} cases, {sum(len(v) for v in saved.values())} tensors -> {out_path}")


def compare(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = 0
    for k in a:
        assert len(a[k]) == len(b[k]), k
        same = [torch.equal(x, y) for x, y in zip(a[k], b[k])]
        bad += same.count(False)
        print(f"{k}: {len(same)} tensors, {same.count(True)} bitwise equal" + ("" if all(same) else f"  DIFFER at {[i for i, s in enumerate(same) if not s]}"))
    print(f"{len(a)} cases, {bad} tensors differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
