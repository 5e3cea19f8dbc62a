"""Cross-rank BatchNorm statistics under batch sharding (ode_rl_amd.dist.sync_batchnorm; csrc/bn_relu_up.hip cut in two around one
all-reduce each way).  Two ranks share the one GPU of the test box (gloo collectives, as tests/test_hip_dist_gpu.py) and must reproduce
the single-process run on the full batch; ONE two-rank job serves every test of the file.

Bounds.  Op level: rel-L2 <= 1e-5 for forward quantities, <= 1e-4 for gradients (those of tests/test_hip_dist_gpu.py: the sums are
float64, only fp32 round-off remains).  Model level: the noise floor of the model at fp32 is measured in the same test -- the largest
rel-L2, over everything compared, between the single-process fused run and the `fused=False` torch composition on the same inputs --
and the sharded run must agree with the single-process fused run within 4 x that floor, and never asked for less than 1e-5.  The
observed values go through conftest.record."""
import os
import socket
import subprocess
import sys
import time

import pytest
import torch
import torch.distributed as dist

import _syncbn_gpu_cases as cases
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

RANK_SECONDS = 240   # a rank's own limit (`timeout -k 10`); the parent gives up a little later


@pytest.fixture(scope="module")
def two_ranks(cuda, tmp_path_factory):
    """(blob, [what rank 0 wrote, what rank 1 wrote]).  A rank that fails takes the other down with it; nothing is started afterwards
    (pytest hands a failed module fixture's error to every test that asks for it)."""
    from ode_rl_amd.dist import sync_batchnorm  # noqa: F401  (without the feature the file stops here)
    tmp = tmp_path_factory.mktemp("syncbn")
    blob = cases.make_blob()
    torch.save(blob, tmp / "in.pt")
    with socket.socket() as sk:   # a free rendezvous port on the loopback
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    # two ranks on ONE card: one launch per layer in place of the persistent launches, which assume one process per GPU
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", ODEHIP_PERSISTENT="0")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_syncbn_gpu_worker.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", str(RANK_SECONDS), sys.executable, worker, str(tmp / f"out{r}.pt"), str(tmp / "in.pt")],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    deadline, codes = time.monotonic() + RANK_SECONDS + 20, [None, None]
    try:
        while None in codes and time.monotonic() < deadline and not any(codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    try:
                        codes[r] = p.wait(timeout=0.2)
                    except subprocess.TimeoutExpired:
                        pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0, 0], f"exit codes of the two ranks: {codes}"
    return blob, [torch.load(tmp / f"out{r}.pt") for r in range(2)]


# ---- the fused pass ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conv_bias", [False, True])
@pytest.mark.parametrize("upsample", [False, True])
def test_sharded_pass_matches_the_full_batch(cuda, two_ranks, upsample, conv_bias):
    blob, outs = two_ranks
    case, tag = (upsample, conv_bias), f"syncbn.op[up={int(upsample)},bias={int(conv_bias)}]"
    full = cases.run_op(blob, case, 0, cases.OP_SHAPE[0], cuda, None)
    sync, local = [o[(case, True)] for o in outs], [o[(case, False)] for o in outs]
    assert [s["out"].shape[0] for s in sync] == [2, 1]
    errs = {k: record(f"{tag}.{k}", rel_l2(torch.cat([s[k] for s in sync]), full[k])) for k in ("out", "dx")}
    for k in ("dgamma", "dbeta") + (("dconv_bias",) if conv_bias else ()):   # local sums: the gradient all-reduce adds them up
        errs[k] = record(f"{tag}.{k}", rel_l2(sync[0][k] + sync[1][k], full[k]))
    for k in ("running_mean", "running_var"):
        errs[k] = record(f"{tag}.{k}", rel_l2(sync[0][k], full[k]))
    print(tag, errs)
    assert all(errs[k] <= 1e-5 for k in ("out", "running_mean", "running_var")), errs
    assert all(errs[k] <= 1e-4 for k in errs if k.startswith("d")), errs
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(sync[0][k], sync[1][k]), k                        # every rank ends with the same buffers, bit for bit
    assert torch.equal(sync[0]["num_batches_tracked"], full["num_batches_tracked"])
    # and the test can see the defect: the same shards with their own statistics are far from the full batch
    for k in ("out", "dx"):
        assert record(f"{tag}.local_statistics.{k}", rel_l2(torch.cat([s[k] for s in local]), full[k])) > 1e-3, k


@pytest.fixture
def one_rank_group(tmp_path):
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("case", cases.OP_CASES, ids=lambda c: f"up{int(c[0])}-bias{int(c[1])}")
def test_one_rank_with_the_switch_on_is_bitwise_the_switch_off(cuda, one_rank_group, case):
    blob = cases.make_blob()
    off = cases.run_op(blob, case, 0, cases.OP_SHAPE[0], cuda, None)
    on = cases.run_op(blob, case, 0, cases.OP_SHAPE[0], cuda, one_rank_group)
    assert set(on) == set(off)
    for k in off:
        assert torch.equal(on[k], off[k]), k


def test_eval_mode_issues_no_collective(cuda, monkeypatch):
    from ode_rl_amd.autograd import bn_relu_up

    def no_collective(*a, **k):
        raise AssertionError("eval() BatchNorm uses the running statistics: nothing to reduce")
    monkeypatch.setattr(dist, "all_reduce", no_collective)
    blob = cases.make_blob()
    got = []
    for group in (None, object()):   # never looked at
        bn = torch.nn.BatchNorm2d(cases.OP_SHAPE[1])
        bn.load_state_dict(blob["op.bn"])
        bn = bn.to(cuda).eval()
        x = blob["op.x"].to(cuda).requires_grad_(True)
        y = bn_relu_up(x, bn, True, group=group)
        y.backward(blob["op.gout", True].to(cuda))
        got.append((y.detach(), x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.num_batches_tracked))
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_an_empty_shard_is_refused_before_any_collective(cuda, monkeypatch):
    from ode_rl_amd.autograd import bn_relu_up
    monkeypatch.setattr(dist, "all_reduce", lambda *a, **k: pytest.fail("a collective was issued"))
    bn = torch.nn.BatchNorm2d(8).to(cuda).train()
    with pytest.raises(ValueError, match="empty"):
        bn_relu_up(torch.zeros(0, 8, 4, 4, device=cuda), bn, False, group=object())
    assert int(bn.num_batches_tracked) == 0


def test_marked_model_refuses_the_module_by_module_fallbacks(cuda, one_rank_group):
    """A width not divisible by 4 and autocast are decided per call, on the device: a marked train() BatchNorm raises there."""
    from ode_rl_amd.dist import sync_batchnorm
    from ode_rl_amd.models.VidODE import Decoder, Encoder
    enc, dec = Encoder(1, 8, 1).to(cuda).train(), Decoder(16, 4, 1).to(cuda).train()
    sync_batchnorm(torch.nn.ModuleList([enc, dec]))
    assert enc(torch.zeros(2, 1, 8, 8, device=cuda)).shape == (2, 16, 4, 4)          # widths 8 and 4: fused
    with pytest.raises(RuntimeError, match="cross-rank statistics"):
        enc(torch.zeros(2, 1, 8, 12, device=cuda))                                    # the second level is 6 wide
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(RuntimeError, match="cross-rank statistics"):
        dec(torch.zeros(2, 16, 4, 4, device=cuda))


# ---- the models -------------------------------------------------------------------------------------------------------------------------

def _flat(res, skip=()):
    """{name: tensor} of everything a run returned that is compared by value."""
    out = {k: v for k, v in res.items() if torch.is_tensor(v)}
    out.update({"grad." + k: v for k, v in res.get("grads", {}).items() if k not in skip})
    out.update({k: v for k, v in res["buffers"].items() if not k.endswith("num_batches_tracked")})
    return out


def _check_model(tag, single, comp, ranks, gathered, skip=()):
    """single / comp: the full batch, fused and as the torch composition; ranks: what the two ranks got; gathered: per-sample results."""
    one, two = _flat(single, skip), _flat(comp, skip)
    assert set(one) == set(two)
    floors = {k: rel_l2(one[k], two[k]) for k in one}
    floor = record(f"{tag}.noise_floor", max(floors.values()))
    bound = max(4.0 * floor, 1e-5)
    r0, r1 = (_flat(r, skip) for r in ranks)
    errs = {k: rel_l2(torch.cat([r0[k], r1[k]]) if k in gathered else r0[k], one[k]) for k in one}
    worst = record(f"{tag}.sharded_vs_single", max(errs.values()))
    print(f"{tag}: noise floor {floor:.3e} ({max(floors, key=floors.get)}), bound {bound:.3e}, sharded vs single process {worst:.3e} "
          f"({max(errs, key=errs.get)})")
    assert worst <= bound, {k: (errs[k], floors[k]) for k in errs if errs[k] > bound}
    for k in one:                                    # after the collectives every rank holds the same gradients and buffers, bit for bit
        if k not in gathered:
            assert torch.equal(r0[k], r1[k]), k
    for k, v in single["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert torch.equal(ranks[0]["buffers"][k], v) and torch.equal(ranks[1]["buffers"][k], v), k


def test_sharded_training_step_of_upstream_vidode_matches_the_full_batch(cuda, two_ranks):
    """conv_odegru.VidODE at init_dim 32, n_downs 2, 64 x 64, n_layers 2, euler, extrapolation, 2 observed + 2 predicted frames, batch 4 as
    2 + 2: compute_all_losses -> backward -> allreduce_gradients against the single-process batch-4 step -- pred_y, every parameter
    gradient, every BatchNorm buffer."""
    blob, outs = two_ranks
    with cases.repeatable_library_convolutions():
        single = cases.upstream_step(cases.upstream_model(blob, cuda), blob["upstream.batch"], lambda: None)
        comp = cases.upstream_step(cases.upstream_model(blob, cuda, fused=False), blob["upstream.batch"], lambda: None)
    assert len(single["grads"]) > 20 and len(single["buffers"]) == 15
    _check_model("syncbn.upstream", single, comp, [o["upstream"] for o in outs], {"pred_y"}, skip=cases.BN_FED_BIASES)
    for k in cases.BN_FED_BIASES:   # exactly zero with batch statistics, on one device and on two
        assert all(torch.count_nonzero(r["grads"][k]) == 0 for r in (single, outs[0]["upstream"], outs[1]["upstream"])), k


def test_sharded_forward_of_the_rk4_vidode_matches_the_full_batch(cuda, two_ranks):
    """models/VidODE.py's model, decoder solved with rk4, train() forward only: prediction, flows and every BatchNorm buffer."""
    blob, outs = two_ranks
    with cases.repeatable_library_convolutions():
        single = cases.rk4_forward(cases.rk4_model(blob, cuda), blob["rk4.frames"], cuda)
        comp = cases.rk4_forward(cases.rk4_model(blob, cuda, fused=False), blob["rk4.frames"], cuda)
    assert len(single["buffers"]) == 15
    _check_model("syncbn.rk4", single, comp, [o["rk4"] for o in outs], {"pred_x", "optical_flow"})
