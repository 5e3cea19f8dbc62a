"""Generate tests/golden/tanh.npz: Tanh dynamics from the REFERENCE's own classes (dev container only; never runs on the GPU box).

The reference's `ODEFunc` defaults to final_act=True (a Tanh head) and its `create_convnet` to nonlinear='tanh'.  This fixture
pins those stacks, built by the reference itself, with the import stubs of make_golden.py (imported, not copied).  Weights and
inputs are procedural (tests/conftest.py: a closed form of the indices that the GPU tests rebuild bit for bit), so only OUTPUTS are stored:
  fA_tanh:   ODEFunc(64, 64, 3, 64, nonlinear='tanh', final_act=False)   -- Tanh hidden layers, the 64-channel A shape
  fA_head:   ODEFunc(64, 64, 3, 64)                                      -- the constructor's defaults: ReLU + Tanh head
  fV_head:   create_convnet(128, 128, 2, 64) with its defaults           -- Tanh hidden layers + Tanh head, 128 -> 64 -> 64 -> 128
  enc_tanh:  ODEConvGRUCell whose f_enc is ODEFunc(32, 32, 3, 32, nonlinear='tanh', final_act=True)

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tanh.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (its stubs; importing it generates nothing)
from conftest import procedural_state_dict, procedural_tensor  # noqa: E402  (make_golden put tests/ on the path)


def main():
    make_golden._install_stubs()
    from modules.DiffEqSolver import ODEFunc  # reference
    from modules.ODEConvGRUCell import ODEConvGRUCell  # reference
    from helpers.utils import create_convnet  # reference

    torch.set_grad_enabled(False)
    dev = torch.device("cpu")
    out = {}
    for key, args, kw, seed in (("fA_tanh", (64, 64, 3, 64), dict(downsize=False, nonlinear="tanh", final_act=False), 40),
                                ("fA_head", (64, 64, 3, 64), {}, 41)):   # {}: the defaults, nonlinear='relu', final_act=True
        f = ODEFunc(*args, device=dev, **kw)
        f.load_state_dict(procedural_state_dict(f.state_dict(), seed))
        y = procedural_tensor((1, 64, 16, 16), seed + 100, -1, 1)
        out[key + ".out"] = f(0.0, y).numpy()
    assert isinstance(ODEFunc(64, 64, 3, 64).gradient_net[-1], torch.nn.Tanh)

    net = create_convnet(128, 128, 2, 64)   # the defaults: nonlinear='tanh', final_act=True
    assert isinstance(net[1], torch.nn.Tanh) and isinstance(net[-1], torch.nn.Tanh)
    f = ODEFunc(net=net, device=dev)
    f.load_state_dict(procedural_state_dict(f.state_dict(), 42))
    out["fV_head.out"] = f(0.0, procedural_tensor((1, 128, 16, 16), 142, -1, 1)).numpy()

    fE = ODEFunc(n_inputs=32, n_outputs=32, n_layers=3, n_units=32, downsize=False, nonlinear="tanh", final_act=True, device=dev)
    enc = ODEConvGRUCell(fE, None, (16, 16), 32, device=dev)
    enc.load_state_dict(procedural_state_dict(enc.state_dict(), 43))
    inp = procedural_tensor((4, 1, 32, 16, 16), 143, -1, 1)
    tt = torch.tensor(np.arange(4) / 8)
    mean, std = enc(inp, tt)
    _, latent = enc.run_ode_conv_gru(inp, tt)
    out.update({"enc_tanh.mean": mean.numpy(), "enc_tanh.std": std.numpy(), "enc_tanh.latent": latent.numpy()})

    np.savez_compressed(os.path.join(HERE, "tanh.npz"), **out)


if __name__ == "__main__":
    main()
