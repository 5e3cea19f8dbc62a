"""Worker of tests/test_hip_bosh3_global_control.py: one rank of a 2-rank job that shares ONE GPU (gloo for the collectives).
Integrates rows [lo, hi) of the batch with bosh3 under exact-global step control, then backward; writes results to a file.
argv: out file, in file, lo, hi."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    out_path, lo, hi = sys.argv[1], int(sys.argv[3]), int(sys.argv[4])
    dist.init_process_group("gloo")
    import ode_rl_amd
    from ode_rl_amd import dist as odist
    dev = torch.device("cuda", 0)
    blob = torch.load(sys.argv[2])
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)
    f.load_state_dict(blob["state"])
    f = f.to(dev)
    z0 = blob["z0"][lo:hi].to(dev).requires_grad_(True)
    gout = blob["gout"][:, lo:hi].to(dev)
    t = blob["t"]
    odist.enable_global_step_control(dev)
    try:
        sol = ode_rl_amd.odeint(f, z0, t, rtol=blob["rtol"], atol=blob["atol"], method="bosh3")
        stats = dict(ode_rl_amd.last_stats)
        sol.backward(gout)
    finally:
        odist.disable_global_step_control()
    odist.allreduce_gradients(f.parameters(), average=False)
    torch.save({"sol": sol.detach().cpu(), "gz": z0.grad.cpu(), "gp": [p.grad.cpu() for p in f.parameters()],
                "nfe": stats["nfe"], "n_accept": stats["n_accept"], "n_reject": stats["n_reject"], "accepted": stats["accepted"]}, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
