"""odeint_adjoint(method="bosh3", adjoint_options={"norm": "seminorm"}) on the device-steered path (csrc/adjoint_device.hip), which
reads the call's tableau and so serves bosh3 as it serves dopri5.

Parity      64-channel stack of three 3x3 convs, ReLU, built as tests/_bosh3_cases.py builds its vigorous forward stacks (last layer
            scaled up, first layer's bias shifted down: units switch on and off along the trajectory), B = 3 on t = [0, 0.3, 0.5] (the
            sixteen-workgroup walk) and B = 20 on two output times (the four-workgroup walk).  Reference: tests/_adaptive_ref.py's
            adjoint with the seminorm, in float64; every gradient within max(4 x d32, GRAD_FLOOR) (d32: the float32 restatement's own
            distance), the bound of tests/test_hip_bosh3.py.  last_adjoint_stats carries the totals over the backward intervals, as
            the restatement's stats do: (nfe, n_accept, n_reject) must be equal, and nfe must be what one fresh solve per interval
            costs, 2 per interval + 3 per attempted step.  The inputs were chosen on the CPU so that the restatement REJECTS backward
            steps (B = 3: ratios 1.54 and 1.31 against accepted ones <= 0.74; B = 20: 1.62 and 1.38 against <= 0.61, in float32 and
            float64 alike); the tests assert it.
Controller  last_adjoint_stats["controller"] is "device" for bosh3 under the seminorm, "host" under the mixed norm and with
            ODEHIP_ADJOINT_DEVICE=0 (read per call).  Stacks take the path under bosh3 exactly where they do under dopri5: a Tanh
            hidden layer does, a Tanh head does not (both methods then run the host loop).
Two drivers device loop against host loop on the same inputs in one process: identical (nfe, n_accept, n_reject), every gradient within
            rel-L2 1e-6, the bound of tests/test_hip_adjoint_paths.py for dopri5.
max_accept  fewer slots than accepted steps: the error of dopri5's device path, which is the host loop's, under bosh3's name.
Cache       dopri5, bosh3, dopri5 at one shape in one process: the third result is bitwise the first (the table cache is keyed by
            content, so the two methods cannot share an entry).

On a library whose gate admits dopri5 only, every `controller == "device"` assertion for bosh3 fails (the field is missing or says
"host")."""
import os

import pytest
import torch

import _bosh3_cases as bc
import _convgru_ref as cref
import _solver_stack_cases as sc
from conftest import procedural_state_dict, procedural_tensor, record, rel_l2

pytestmark = pytest.mark.gpu

# name -> (channels, hidden activation, Tanh head, B, times, gain of the last layer, first-layer bias shift, seed)
CASES = {
    "B3": ((64, 64, 64, 64), "relu", False, 3, [0.0, 0.3, 0.5], 60.0, -1.5, 61),
    "B20": ((64, 64, 64, 64), "relu", False, 20, [0.0, 0.5], 40.0, -1.5, 61),
    "TH3": ((64, 64, 64), "tanh", True, 3, [0.0, 0.3, 0.5], 8.0, 0.0, 54),
}


def _needs_device_path():
    if os.environ.get("ODEHIP_PERSISTENT") == "0" or os.environ.get("ODEHIP_ADJOINT_DEVICE") == "0":
        pytest.skip("needs the device-controlled adjoint")


def _spec(name):
    channels, act, final_act, B, times, gain, shift, seed = CASES[name]
    sd = procedural_state_dict(sc._shapes(channels, 3), seed)
    sd["gradient_net.0.bias"] = sd["gradient_net.0.bias"] + shift
    last = 2 * (len(channels) - 2)
    sd[f"gradient_net.{last}.weight"] = sd[f"gradient_net.{last}.weight"] * gain
    sd[f"gradient_net.{last}.bias"] = sd[f"gradient_net.{last}.bias"] * gain
    T = len(times)
    return {"channels": channels, "ks": 3, "act": act, "final_act": final_act, "sd": sd, "method": "bosh3",
            "t": torch.tensor(times, dtype=torch.float64), "z0": procedural_tensor((B, channels[0], 16, 16), 1000 + seed, -1.0, 1.0),
            "gout": procedural_tensor((T, B, channels[0], 16, 16), 2000 + seed, -1.0, 1.0)}


@pytest.fixture(scope="module")
def refs():
    """name -> (spec, float64 gradients, float64 stats, float32 gradients, float32 stats) of the restatement's seminorm adjoint; computed
    once, read by every test."""
    cache = {}

    def get(name):
        if name not in cache:
            spec = _spec(name)
            g64, s64 = bc.adjoint_reference(spec, torch.float64, "seminorm")
            g32, s32 = bc.adjoint_reference(spec, torch.float32, "seminorm")
            cache[name] = (spec, g64, s64, g32, s32)
        return cache[name]
    return get


def _device_adjoint(dev, spec, method="bosh3", norm="seminorm", max_accept=None, f=None):
    """(gradients by name on the CPU, last_adjoint_stats) of odeint_adjoint(method=...) and its backward pass."""
    import torch.nn as nn
    import ode_rl_amd
    f = f if f is not None else sc.device_func(dev, spec)
    f.zero_grad()
    z = spec["z0"].to(dev).requires_grad_(True)
    opts = {} if norm == "mixed" else {"norm": "seminorm"}
    if max_accept is not None:
        opts["max_accept"] = max_accept
    sol = ode_rl_amd.odeint_adjoint(f, z, spec["t"], method=method, adjoint_options=opts, **bc.TOL)
    sol.backward(spec["gout"].to(dev))
    st = dict(ode_rl_amd.last_adjoint_stats)
    convs = [m for m in f.gradient_net if isinstance(m, nn.Conv2d)]
    out = {"z0": z.grad}
    out.update({f"w{i}": c.weight.grad for i, c in enumerate(convs)})
    out.update({f"b{i}": c.bias.grad for i, c in enumerate(convs)})
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}, st


def _check_against_reference(name, tag, got, st, ref):
    spec, g64, s64, g32, s32 = ref
    n_int = len(spec["t"]) - 1
    print(f"{name} {tag}: device {st}, restatement float64 {bc.counts(s64)}, float32 {bc.counts(s32)}")
    assert bc.counts(s64) == bc.counts(s32)
    assert (st["nfe"], st["n_accept"], st["n_reject"]) == bc.counts(s64), (st, bc.counts(s64))
    assert st["nfe"] == 2 * n_int + 3 * (st["n_accept"] + st["n_reject"]) and st["n_accept"] >= n_int   # a fresh solve per interval
    for k in sorted(g64):
        assert float(g64[k].abs().max()) > 0.0, k    # no layer of the case is dead
        tol, d32 = cref.bound(g32[k], g64[k], sc.GRAD_FLOOR)
        e = record(f"bosh3_device_adjoint.{name}.{tag}.grad.{k}", rel_l2(got[k], g64[k]))
        print(f"{name} {tag} {k}: {e:.3e} (d32 {d32:.3e}, bound {tol:.3e})")
        assert e <= tol, (name, tag, k, e)


@pytest.mark.parametrize("name", ["B3", "B20"])
def test_parity_with_the_restatements_adjoint_where_steps_are_rejected(cuda, refs, name):
    _needs_device_path()
    ref = refs(name)
    assert ref[2]["n_reject"] >= 1 and ref[4]["n_reject"] >= 1, "the case no longer rejects a backward step"
    got, st = _device_adjoint(cuda, ref[0])
    assert st["controller"] == "device", st
    _check_against_reference(name, "device", got, st, ref)


def test_the_host_loop_says_host(cuda, refs, monkeypatch):
    """Needs no device path: the mixed norm, and the seminorm with ODEHIP_ADJOINT_DEVICE=0 (read per call)."""
    spec = refs("B3")[0]
    f = sc.device_func(cuda, spec)
    for method in ("bosh3", "dopri5"):
        _, st = _device_adjoint(cuda, spec, method=method, norm="mixed", f=f)
        assert st["controller"] == "host", (method, st)
        assert set(st) >= {"nfe", "n_accept", "n_reject", "controller"}
    monkeypatch.setenv("ODEHIP_ADJOINT_DEVICE", "0")
    for method in ("bosh3", "dopri5"):
        _, st = _device_adjoint(cuda, spec, method=method, f=f)
        assert st["controller"] == "host", (method, st)


def test_which_controller_ran(cuda, refs, monkeypatch):
    _needs_device_path()
    spec = refs("B3")[0]
    f = sc.device_func(cuda, spec)
    for method in ("bosh3", "dopri5"):
        _, st = _device_adjoint(cuda, spec, method=method, f=f)
        assert st["controller"] == "device", (method, st)
        assert set(st) >= {"nfe", "n_accept", "n_reject", "controller"}
    monkeypatch.setenv("ODEHIP_ADJOINT_DEVICE", "0")
    _, st = _device_adjoint(cuda, spec, f=f)
    assert st["controller"] == "host", st
    monkeypatch.delenv("ODEHIP_ADJOINT_DEVICE")
    _, st = _device_adjoint(cuda, spec, f=f)
    assert st["controller"] == "device", st


def test_device_loop_against_host_loop(cuda, refs, monkeypatch):
    _needs_device_path()
    spec = refs("B3")[0]
    f = sc.device_func(cuda, spec)
    dev, st_dev = _device_adjoint(cuda, spec, f=f)
    dev2, st_dev2 = _device_adjoint(cuda, spec, f=f)
    monkeypatch.setenv("ODEHIP_ADJOINT_DEVICE", "0")
    host, st_host = _device_adjoint(cuda, spec, f=f)
    monkeypatch.delenv("ODEHIP_ADJOINT_DEVICE")
    assert (st_dev["controller"], st_host["controller"]) == ("device", "host")
    assert st_dev2 == st_dev and all(torch.equal(dev[k], dev2[k]) for k in dev)   # deterministic: bitwise
    assert (st_dev["nfe"], st_dev["n_accept"], st_dev["n_reject"]) == (st_host["nfe"], st_host["n_accept"], st_host["n_reject"]), (st_dev, st_host)
    assert st_dev["n_reject"] >= 1
    errs = {k: record(f"bosh3_device_adjoint.dev_vs_host.grad.{k}", rel_l2(dev[k], host[k])) for k in sorted(dev)}
    print(f"device {st_dev}, host {st_host}, device vs host {errs}")
    assert max(errs.values()) <= 1e-6, errs
    assert all(bool(torch.isfinite(g).all()) for g in dev.values())


def test_tanh_stacks_take_the_path_where_dopri5_does(cuda, refs):
    _needs_device_path()
    # Tanh head: no reverse sweep over it is recorded, so both methods run the host loop -- and bosh3's result is still the restatement's
    ref = refs("TH3")
    spec = ref[0]
    f = sc.device_func(cuda, spec)
    got, st = _device_adjoint(cuda, spec, f=f)
    _, st5 = _device_adjoint(cuda, spec, method="dopri5", f=f)
    assert st["controller"] == st5["controller"] == "host", (st, st5)
    _check_against_reference("TH3", "head", got, st, ref)
    # Tanh hidden layer, no head: the device path, for both
    spec = bc.backward_spec("GT")
    f = sc.device_func(cuda, spec)
    _, st = _device_adjoint(cuda, spec, f=f)
    _, st5 = _device_adjoint(cuda, spec, method="dopri5", f=f)
    assert st["controller"] == st5["controller"] == "device", (st, st5)


def test_max_accept_reached_is_the_error_of_dopri5s_device_path(cuda, refs, monkeypatch):
    _needs_device_path()
    spec, _, s64 = refs("B3")[:3]
    assert s64["n_accept"] > 2
    f = sc.device_func(cuda, spec)
    msgs = {}
    for method in ("bosh3", "dopri5"):
        with pytest.raises(ValueError, match="more than max_accept = 1 accepted steps") as e:
            _device_adjoint(cuda, spec, method=method, max_accept=1, f=f)
        msgs[method] = str(e.value)
    assert msgs["bosh3"] == msgs["dopri5"].replace("dopri5", "bosh3"), msgs
    monkeypatch.setenv("ODEHIP_ADJOINT_DEVICE", "0")
    with pytest.raises(ValueError, match="more than max_accept = 1 accepted steps") as e:
        _device_adjoint(cuda, spec, max_accept=1, f=f)
    monkeypatch.delenv("ODEHIP_ADJOINT_DEVICE")
    assert str(e.value) == msgs["bosh3"]
    # exactly enough slots (max_accept + 1 of them, adjoint_layout.h) is not an error, and the path is usable after the failures
    got, st = _device_adjoint(cuda, spec, max_accept=s64["n_accept"] - 1, f=f)
    assert st["controller"] == "device" and st["n_accept"] == s64["n_accept"]
    _check_against_reference("B3", "exact_slots", got, st, refs("B3"))


def test_the_two_methods_do_not_share_a_cached_table(cuda, refs):
    _needs_device_path()
    spec = refs("B3")[0]
    f = sc.device_func(cuda, spec)
    first, st1 = _device_adjoint(cuda, spec, method="dopri5", f=f)
    mid, st2 = _device_adjoint(cuda, spec, method="bosh3", f=f)
    third, st3 = _device_adjoint(cuda, spec, method="dopri5", f=f)
    assert st1["controller"] == st2["controller"] == st3["controller"] == "device"
    assert st3 == st1 and all(torch.equal(first[k], third[k]) for k in first)
    assert st2["nfe"] != st1["nfe"]                                   # bosh3 really ran in between: three evaluations per attempt
    _check_against_reference("B3", "between_dopri5", mid, st2, refs("B3"))
