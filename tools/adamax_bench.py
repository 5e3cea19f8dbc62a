"""The Adamax step on the parameter lists of ODEConvGRU (40 tensors, 1.04 M parameters) and VidODE (3.49 M parameters), on the same GPU:
  * fused           FusedAdamax.step()                      (csrc/optim_step.hip: one launch per 24 tensors)
  * fused_clip      FusedAdamax(max_grad_norm=c).step()     (sum of squares -> coefficient -> the update reading the coefficient)
  * foreach         torch.optim.Adamax(foreach=True).step()
  * foreach_clip    torch.nn.utils.clip_grad_norm_(params, c), then that step
  * single          torch.optim.Adamax(foreach=False).step()
  * single_clip     torch.nn.utils.clip_grad_norm_(params, c), then that step
For each: device kernels of one call by torch.profiler (memcpy / memset not counted), whether the call runs under
torch.cuda.set_sync_debug_mode("error"), and the device time, median (min, max) over 7 groups of 50 calls between HIP events after 10
warm-up calls, the variants alternating group by group.  The gradients are refilled from a fixed tensor before every call by one
foreach copy, inside the timed window of every variant alike (a clipped step scales them in place).  Reported, not gated.
  python tools/adamax_bench.py [--out FILE] [--clip 0.5]

Launches per step from a kernel trace (a run of its own, no counters, nothing timed in it):
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/adamax_bench.py --trace-run
  python tools/adamax_bench.py --count-trace DIR/**/*_kernel_trace.csv [--out FILE]    (merges into FILE if it exists)
--trace-run brackets TRACE_CALLS calls of every variant between two launches of a marker kernel none of them uses (grad_scale_kernel on
one element), in the order of `plan()`; --count-trace counts the kernels between each pair of markers in start order."""
import argparse
import csv
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ode_rl_amd  # noqa: E402,F401
from clip_bench import alternating_ms, model_gradients, runs_without_sync  # noqa: E402
from eval_bench import kernel_launches  # noqa: E402
from ode_rl_amd.optim import FusedAdamax  # noqa: E402

VARIANTS = ("fused", "fused_clip", "foreach", "foreach_clip", "single", "single_clip")
MODELS = ("ODEConvGRU", "VidODE")
TRACE_CALLS = 20
MARKER = "grad_scale_kernel"


def vidode_gradients(dev):
    """(parameters, fixed gradients) of the VidODE model of BASELINE configs[3]"""
    from ode_rl_amd.models.VidODE import VidODE
    opt = argparse.Namespace(n_downs=2, resolution=64, in_channels=1, n_layers=2, decode_diff_method="rk4")
    torch.manual_seed(0)
    base = [p.detach() for p in VidODE(opt, torch.device("cpu")).to(dev).parameters()]
    g = torch.Generator().manual_seed(1)
    return base, [torch.randn(p.shape, generator=g).to(dev) for p in base]


def variant(name, base, fixed, clip):
    """one call of variant `name` on its own copy of the parameters: refill the gradients, clip, step"""
    ps = [torch.nn.Parameter(p.clone()) for p in base]
    for p in ps:
        p.grad = torch.empty_like(p)
    grads = [p.grad for p in ps]
    kind, _, clipped = name.partition("_")
    if kind == "fused":
        opt = FusedAdamax(ps, max_grad_norm=clip if clipped else None)
    else:
        opt = torch.optim.Adamax(ps, foreach=kind == "foreach")

    def call():
        torch._foreach_copy_(grads, fixed)
        if clipped and kind != "fused":
            torch.nn.utils.clip_grad_norm_(ps, clip)
        opt.step()
    return call


def refill_only(fixed):
    grads = [torch.empty_like(p) for p in fixed]
    return lambda: torch._foreach_copy_(grads, fixed)


def plan():
    """the (model, variant) order of --trace-run; 'refill' is the gradient refill alone, which every variant's count contains"""
    return [(m, v) for m in MODELS for v in ("refill",) + VARIANTS]


def trace_run(dev, clip):
    from ode_rl_amd import _lib
    from ode_rl_amd.hip_ops import _stream
    lib = _lib.load()
    one, coef = torch.ones(1, device=dev), torch.ones(1, device=dev)
    arr, numel = (ctypes.c_void_p * 1)(one.data_ptr()), (ctypes.c_longlong * 1)(1)

    def marker():
        _lib.check(lib.odehip_grad_scale(arr, numel, 1, coef.data_ptr(), _stream()))

    sets = {"ODEConvGRU": model_gradients(dev), "VidODE": vidode_gradients(dev)}
    for model, name in plan():
        base, fixed = sets[model]
        call = refill_only(fixed) if name == "refill" else variant(name, base, fixed, clip)
        for _ in range(3):
            call()
        marker()
        for _ in range(TRACE_CALLS):
            call()
        marker()
    torch.cuda.synchronize()


def count_trace(paths):
    """{model: {variant: kernels per call}} from kernel-trace CSVs of one --trace-run (the process's rows may be split over files)"""
    rows = []
    for path in paths:
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    if len(marks) != 2 * len(plan()):
        raise SystemExit(f"count-trace: {len(marks)} marker launches in the trace, {2 * len(plan())} expected")
    out = {m: {} for m in MODELS}
    for k, (model, name) in enumerate(plan()):
        inside = rows[marks[2 * k] + 1:marks[2 * k + 1]]
        out[model][name] = {"launches_per_call": len(inside) / TRACE_CALLS,
                            "kernels": sorted({r["Kernel_Name"].split("(")[0][:80] for r in inside})}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to this file")
    ap.add_argument("--clip", type=float, default=0.5)
    ap.add_argument("--trace-run", action="store_true", help="only run the bracketed calls, for a kernel trace")
    ap.add_argument("--count-trace", nargs="+", default=None, metavar="CSV", help="count launches per call in kernel-trace CSVs")
    a = ap.parse_args()
    if a.count_trace:
        rec = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as fh:
                rec = json.load(fh)
        rec["kernel_trace"] = {"method": f"rocprofv3 --kernel-trace of --trace-run: kernels between two marker launches around {TRACE_CALLS} calls, "
                                         "divided by the calls; every variant's count contains the refill's", "models": count_trace(a.count_trace)}
        text = json.dumps(rec, indent=1)
        print(json.dumps(rec["kernel_trace"]))
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("adamax_bench needs a GPU: nothing here can be timed on the CPU")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev, a.clip)
        return
    rec = {"device": torch.cuda.get_device_name(0), "clip": a.clip,
           "method": "one gradient refill (a foreach copy) + [torch's clip_grad_norm_ +] the step; median (min, max) of 7 groups of 50 calls "
                     "between HIP events after 10 warm-up calls, variants alternating; launches of one call by torch.profiler (memcpy / "
                     "memset not counted; the refill's kernels are counted in every variant and listed under refill_launches)",
           "models": {}}
    for model, (base, fixed) in (("ODEConvGRU", model_gradients(dev)), ("VidODE", vidode_gradients(dev))):
        calls = {name: variant(name, base, fixed, a.clip) for name in VARIANTS}
        row = {"tensors": len(base), "parameters": sum(p.numel() for p in base), "refill_launches": kernel_launches(refill_only(fixed))[0],
               "variants": {}}
        times = alternating_ms(calls)
        for name, fn in calls.items():
            n, names = kernel_launches(fn)
            med, lo, hi = times[name]
            row["variants"][name] = {"us_median": med * 1e3, "us_min": lo * 1e3, "us_max": hi * 1e3, "launches": n, "kernels": names,
                                     "runs_under_sync_debug_error": runs_without_sync(fn)}
            print(json.dumps({model: {name: row["variants"][name]}}), flush=True)
        rec["models"][model] = row
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
