"""Worker of tests/test_hip_sync_batchnorm.py: one rank of a 2-rank job that shares ONE GPU (gloo for the collectives).  Runs its shard
of every case of the blob -- the fused BatchNorm pass with and without cross-rank statistics, one training step of upstream Vid-ODE's
model and one forward of models/VidODE.py's -- and writes what it got to a file."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _syncbn_gpu_cases as cases  # noqa: E402  (tests/ is the script's directory)


def main():
    out_path, blob = sys.argv[1], torch.load(sys.argv[2])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    from ode_rl_amd import dist as odist
    dev = torch.device("cuda", 0)
    res = {}
    for case in cases.OP_CASES:
        lo, hi = odist.shard_bounds(cases.OP_SHAPE[0], rank, world)
        for sync in (True, False):
            res[(case, sync)] = cases.run_op(blob, case, lo, hi, dev, dist.group.WORLD if sync else None)
    with cases.repeatable_library_convolutions():
        model = cases.upstream_model(blob, dev)
        odist.sync_batchnorm(model)
        res["upstream"] = cases.upstream_step(model, {k: odist.shard_batch(v, rank, world) if k in cases.SHARDED else v
                                                      for k, v in blob["upstream.batch"].items()},
                                              lambda: odist.allreduce_gradients(model.parameters()))
        model = cases.rk4_model(blob, dev)
        odist.sync_batchnorm(model)
        res["rk4"] = cases.rk4_forward(model, odist.shard_batch(blob["rk4.frames"], rank, world), dev)
    torch.save(res, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
