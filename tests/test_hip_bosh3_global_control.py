"""bosh3 under exact-global step control (ode_rl_amd.dist.enable_global_step_control; C ABI odehip_set_norm_allreduce_counted), modelled on
tests/test_hip_dist_gpu.py, which does the same for dopri5: two ranks (sharing the one GPU of the test box, gloo collectives) integrate
their shards of a batch of 4 -- split 2 + 2 and 3 + 1 -- with odeint(method="bosh3") and run loss.backward(), and must reproduce the
single-process run on the full batch: identical accepted-step logs on the two ranks, the full-batch solve's step counts, its step
sizes to 1e-5, trajectories to rel-L2 1e-5 and gradients to 1e-4 (only the summation order of the error norm differs) -- the dopri5
test's bounds.  Each rank is a fresh child process under its own `timeout -k 10`; the parent checks both exit codes before it does
anything else.

One single-process case installs a ctypes callback through the C ABI (world 1, the buffer left as it is): the solve must succeed with
the (nfe, n_accept, n_reject) of the hook-free solve.  The hook is installed with odehip_set_norm_allreduce_counted, the call whose
contract covers every adaptive method and sums the element count over the ranks (the 3 + 1 split needs that); under the older
odehip_set_norm_allreduce, whose contract is dopri5's with equal shards, bosh3 stays refused (tests/test_adaptive_abi_cpu.py), and the
same case says so.

On a library without the counted hook the two-rank cases fail with ValueError ("... is not implemented for bosh3") and the C-ABI
case with AttributeError (no such symbol)."""
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
CHILD_SECONDS = 240


def _case():
    """The dynamics, inputs and grid of the dopri5 test: the last two samples are three times as large, so a shard's own error norm is
    not the batch's."""
    import ode_rl_amd
    torch.manual_seed(0)
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)
    with torch.no_grad():
        for i in (0, 2, 4, 6):
            f.gradient_net[i].weight.mul_(0.15)
            f.gradient_net[i].bias.copy_(torch.where(torch.arange(64) % 2 == 0, 2.5, -2.5))
        f.gradient_net[8].weight.mul_(4.0)
    g = torch.Generator().manual_seed(3)
    z0 = torch.randn(4, 64, 16, 16, generator=g) * 0.5
    z0[2:] *= 3.0
    t = torch.tensor([0.0, 0.3, 0.5, 1.0], dtype=torch.float64)
    gout = torch.randn(4, 4, 64, 16, 16, generator=g)
    return f, z0, t, gout


@pytest.fixture(scope="module")
def full_batch(cuda):
    """The single-process solve of the whole batch and its backward pass: computed once, read by both splits."""
    import ode_rl_amd
    f, z0, t, gout = _case()
    state = {k: v.clone() for k, v in f.state_dict().items()}
    fd = f.to(cuda)
    zd = z0.to(cuda).requires_grad_(True)
    sol = ode_rl_amd.odeint(fd, zd, t, rtol=RTOL, atol=ATOL, method="bosh3")
    stats = dict(ode_rl_amd.last_stats)
    sol.backward(gout.to(cuda))
    with torch.no_grad():
        ode_rl_amd.odeint(fd, z0[:2].to(cuda), t, rtol=RTOL, atol=ATOL, method="bosh3")
    alone = list(ode_rl_amd.last_stats["accepted"])
    torch.cuda.synchronize()
    return {"state": state, "z0": z0, "t": t, "gout": gout, "sol": sol.detach().cpu(), "gz": zd.grad.cpu(),
            "gp": [p.grad.cpu() for p in fd.parameters()], "stats": stats, "alone": alone}


@pytest.mark.parametrize("split", [(2, 2), (3, 1)])
def test_two_ranks_exact_global_bosh3_match_single_process(cuda, tmp_path, full_batch, split):
    full = full_batch
    torch.save({"state": full["state"], "z0": full["z0"], "gout": full["gout"], "t": full["t"], "rtol": RTOL, "atol": ATOL}, tmp_path / "in.pt")
    with socket.socket() as sk:   # a free rendezvous port on the loopback
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # two ranks share ONE card here: the persistent launches (every CU, workgroups waiting for each other) assume one process per
    # GPU, so the ranks use one launch per layer -- the results are bit-identical either way
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", ODEHIP_PERSISTENT="0")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dist_bosh3_worker.py")
    bounds = [(0, split[0]), (split[0], 4)]
    procs = [subprocess.Popen(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, worker, str(tmp_path / f"out{r}.pt"),
                               str(tmp_path / "in.pt"), str(lo), str(hi)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
             for r, (lo, hi) in enumerate(bounds)]
    codes = [p.wait() for p in procs]   # (each child ends by itself or by its own time limit)
    assert codes == [0, 0], codes

    outs = [torch.load(tmp_path / f"out{r}.pt") for r in range(2)]
    st = full["stats"]
    assert outs[0]["accepted"] == outs[1]["accepted"]   # every rank took the same decisions on the same all-reduced numbers
    for o in outs:
        assert (o["nfe"], o["n_accept"], o["n_reject"]) == (st["nfe"], st["n_accept"], st["n_reject"]), (o["n_accept"], o["n_reject"], st)
        assert o["nfe"] == 2 + 3 * (o["n_accept"] + o["n_reject"])   # three evaluations per attempt: it is bosh3 that ran
        assert len(o["accepted"]) == len(st["accepted"])
        assert all(abs(a[1] - b[1]) <= 1e-5 * abs(b[1]) for a, b in zip(o["accepted"], st["accepted"]))
    assert rel_l2(torch.cat([o["sol"] for o in outs], 1), full["sol"]) <= 1e-5
    assert rel_l2(torch.cat([o["gz"] for o in outs], 0), full["gz"]) <= 1e-4
    for k, g in enumerate(full["gp"]):
        assert rel_l2(outs[0]["gp"][k], g) <= 1e-4      # summed over ranks == full-batch gradient
        assert torch.equal(outs[0]["gp"][k], outs[1]["gp"][k])
    # and per-shard control really would have differed: the first two samples alone take a different step sequence
    alone, acc = full["alone"], st["accepted"]
    assert len(alone) != len(acc) or any(abs(a[1] - b[1]) > 1e-3 * abs(b[1]) for a, b in zip(alone, acc))


def test_hook_through_the_c_abi_in_one_process(cuda, full_batch):
    import ode_rl_amd
    from ode_rl_amd import _lib
    full = full_batch
    f, z0, t, _ = _case()
    f.load_state_dict(full["state"])
    fd = f.to(cuda)
    calls = []

    def _cb(ptr, n, stream, user):   # world 1: the sums are already the batch's
        calls.append(n)
        return 0
    cb = _lib.ALLREDUCE_FN(_cb)
    scratch = torch.zeros(8, dtype=torch.float32, device=cuda)
    lib = _lib.load()
    _lib.check(lib.odehip_set_norm_allreduce_counted(ctypes.cast(cb, ctypes.c_void_p), None, 1, scratch.data_ptr()))
    try:
        with torch.no_grad():
            sol = ode_rl_amd.odeint(fd, z0.to(cuda), t, rtol=RTOL, atol=ATOL, method="bosh3")
        st = dict(ode_rl_amd.last_stats)
        torch.cuda.synchronize()
        # the older call installs the older contract: dopri5 only
        _lib.check(lib.odehip_set_norm_allreduce(ctypes.cast(cb, ctypes.c_void_p), None, 1, scratch.data_ptr()))
        n_calls = len(calls)
        with pytest.raises(ValueError, match="is not implemented for bosh3"), torch.no_grad():
            ode_rl_amd.odeint(fd, z0.to(cuda), t, rtol=RTOL, atol=ATOL, method="bosh3")
        assert len(calls) == n_calls
    finally:
        _lib.check(lib.odehip_set_norm_allreduce(None, None, 1, None))
    want = full["stats"]
    assert (st["nfe"], st["n_accept"], st["n_reject"]) == (want["nfe"], want["n_accept"], want["n_reject"]), (st, want)
    # the batch's element count, d0 and d1 together, d2, then one error norm per attempted step: nothing that depends on the stage count
    assert calls == [1, 2, 1] + [1] * (st["n_accept"] + st["n_reject"]), calls
    assert rel_l2(sol.cpu(), full["sol"]) <= 1e-5
