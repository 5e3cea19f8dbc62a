"""Bit identity of the adaptive (dopri5) solve, its two backward passes and its adjoints between two builds of the library
(csrc/dopri5.hip, dopri5_backward.hip, adjoint_dopri5.hip, adjoint_device.hip, dopri5_control.h).

  ODEHIP_LIB=<lib.so> python tools/dopri5_ab.py run <out.pt>     every case from fixed seeds, in this (fresh) process
  python tools/dopri5_ab.py compare <a.pt> <b.pt>                torch.equal on every tensor, == on every stats triple
                                                                 (nfe, n_accept, n_reject); exit status 1 on a difference

Cases: a 3-layer 64-channel ODEFunc on a 16x16 state, rtol 1e-3 / atol 1e-4; B = 3 (sixteen-workgroup walk) and 20; T = 1, 2, 4; the
persistent walk on and off.  Paths: forward; forward on a decreasing grid (negated dynamics); options={'first_step': 0.05}; saving
forward + backward from the saved slots; backward by re-integration (one slot: too few to save); asynchronous start / collect;
odeint_adjoint on the device-controlled path (seminorm), with ODEHIP_ADJOINT_DEVICE=0 (the host loop) and with the mixed norm.  Once
each: a Tanh head, a 32-channel stack (forward only: the per-layer path), vigorous dynamics with first_step 3.0 (rejected attempts),
output times 0.003 apart (one accepted step covers several).  `run` asserts from the library's own stats that rejections, a step
over two or more output times and an adjoint interval of more than one accepted step all occur.  The arithmetic is deterministic,
so there is no tolerance."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RTOL, ATOL = 1e-3, 1e-4
PATHS = ("forward", "negate", "first_step", "train_saved", "train_reintegrate", "train_async", "adjoint_device", "adjoint_host",
         "adjoint_mixed")


def _triple(st):
    return (int(st["nfe"]), int(st["n_accept"]), int(st["n_reject"]))


def _case(dev, path, B, T, seed, persistent, channels=64, head=False, vigorous=False, t=None, options=None, rtol=RTOL):
    """-> (tensors, stats triples, the forward's accepted (t0, dt) log or None)"""
    import torch
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(channels, channels, 3, channels, False, "relu", final_act=head)
    if vigorous:
        with torch.no_grad():
            [m for m in f.gradient_net if isinstance(m, torch.nn.Conv2d)][-1].weight.mul_(12.0)
    f = f.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    z0 = (torch.randn(B, channels, 16, 16, generator=g) * 0.5).to(dev)
    if t is None:
        t = torch.arange(T, 2 * T, dtype=torch.float64) / (2 * T)
    T = len(t)
    gout = torch.randn(T, B, channels, 16, 16, generator=g).to(dev)
    if path == "first_step":
        options = {"first_step": 0.05}
    atol = rtol * ATOL / RTOL
    if path in ("forward", "negate", "first_step"):
        with torch.no_grad():
            out = ode_rl_amd.odeint(f, z0, t.flip(0) if path == "negate" else t, rtol=rtol, atol=atol, method="dopri5", options=options)
        st = dict(ode_rl_amd.last_stats)
        return [out], [_triple(st)], st.get("accepted")
    z0.requires_grad_(True)
    slots, was_async, env = hip_ops._dopri5_save_slots, None, os.environ.get("ODEHIP_ADJOINT_DEVICE")
    try:
        if path == "train_reintegrate":
            hip_ops._dopri5_save_slots = 1
        if path == "train_async":
            was_async = ode_rl_amd.set_async_dopri5(True)
        if path == "adjoint_host":
            os.environ["ODEHIP_ADJOINT_DEVICE"] = "0"
        if path.startswith("adjoint"):
            adj = {} if path == "adjoint_mixed" else {"adjoint_options": {"norm": "seminorm"}}
            out = ode_rl_amd.odeint_adjoint(f, z0, t, rtol=rtol, atol=atol, method="dopri5", options=options, **adj)
        else:
            out = ode_rl_amd.odeint(f, z0, t, rtol=rtol, atol=atol, method="dopri5", options=options)
        out.backward(gout)
        st = dict(ode_rl_amd.last_stats)
        stats = [_triple(st)]
        if path == "train_saved" and T > 1 and persistent:
            assert st["saved"], "the saving forward did not save"
        if path == "train_reintegrate" and st["n_accept"] > 1:
            assert not st["saved"], "one slot was enough: the backward did not re-integrate"
        if path.startswith("adjoint") and T > 1:
            stats.append(_triple(ode_rl_amd.last_adjoint_stats))
    finally:
        hip_ops._dopri5_save_slots = slots
        if was_async is not None:
            ode_rl_amd.set_async_dopri5(was_async)
        if path == "adjoint_host":
            if env is None:
                os.environ.pop("ODEHIP_ADJOINT_DEVICE", None)
            else:
                os.environ["ODEHIP_ADJOINT_DEVICE"] = env
    return [out.detach(), z0.grad] + [p.grad for _, p in sorted(f.named_parameters())], stats, st.get("accepted")


def run(out_path):
    import torch
    import ode_rl_amd
    dev = torch.device("cuda:0")
    lib = ode_rl_amd._lib.load()
    res, stats, logs, grids = {}, {}, {}, {}
    seed = 200

    def add(name, *args, **kw):
        res[name], stats[name], logs[name] = _case(dev, *args, persistent, **kw)
        grids[name] = kw.get("t")

    close_t = torch.tensor([0.5, 0.503, 0.506, 0.509, 1.0], dtype=torch.float64)
    for persistent in (1, 0):
        was = lib.odehip_set_persistent_trajectory(persistent)
        try:
            for path in PATHS:
                for B in (3, 20):
                    for T in (1, 2, 4):
                        seed += 2
                        add(f"{path}.B{B}.T{T}.persistent{persistent}", path, B, T, seed)
            for path in ("forward", "train_saved", "adjoint_device"):
                add(f"{path}.tanh_head.B3.T4.persistent{persistent}", path, 3, 4, 810, head=True)
                add(f"{path}.rejections.B3.T4.persistent{persistent}", path, 3, 4, 820, vigorous=True, rtol=1e-4,
                    t=torch.tensor([0.0, 1.0, 2.5, 4.0], dtype=torch.float64), options={"first_step": 3.0})
                add(f"{path}.close_times.B3.T5.persistent{persistent}", path, 3, 5, 830, t=close_t)
            add(f"forward.32_channels.B3.T4.persistent{persistent}", "forward", 3, 4, 840, channels=32)
        finally:
            lib.odehip_set_persistent_trajectory(was)
    torch.cuda.synchronize()

    # the case set is not trivial, by the library's own account
    assert any(s[2] > 0 for v in stats.values() for s in v), "no case rejected an attempt"
    multi = [k for k, log in logs.items() if log is not None and grids[k] is not None and any(
        sum(1 for x in grids[k].tolist() if t0 < x <= t0 + dt) >= 2 for t0, dt in log)]
    assert multi, "no accepted step covers two or more output times"
    long_adj = [k for k, v in stats.items() if k.startswith("adjoint") and len(v) == 2 and v[1][1] > int(k.split(".T")[1].split(".")[0]) - 1]
    assert long_adj, "no adjoint interval took more than one accepted step"
    print(f"rejections in {sum(1 for v in stats.values() if any(s[2] > 0 for s in v))} cases; a step over >= 2 output times in "
          f"{len(multi)}; an adjoint interval of > 1 accepted step in {len(long_adj)}")

    saved = {k: [x.detach().cpu() for x in v] for k, v in res.items()}
    for k, v in saved.items():
        assert all(bool(torch.isfinite(x).all()) for x in v), k
    torch.save({"tensors": saved, "stats": stats}, out_path)
    print(f"{ode_rl_amd._lib.LIB_PATH}: {len(saved)} cases, {sum(len(v) for v in saved.values())} tensors -> {out_path}")


def compare(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert a["tensors"].keys() == b["tensors"].keys(), (sorted(a["tensors"]), sorted(b["tensors"]))
    bad = 0
    for k in a["tensors"]:
        ta, tb = a["tensors"][k], b["tensors"][k]
        assert len(ta) == len(tb), k
        same = [torch.equal(x, y) for x, y in zip(ta, tb)]
        stats_same = a["stats"][k] == b["stats"][k]
        bad += same.count(False) + (0 if stats_same else 1)
        print(f"{k}: {len(same)} tensors, {same.count(True)} bitwise equal, stats {a['stats'][k]}" + ("" if stats_same else f" != {b['stats'][k]}") +
              ("" if all(same) else f"  DIFFER at {[i for i, s in enumerate(same) if not s]}"))
    print(f"{len(a['tensors'])} cases, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
