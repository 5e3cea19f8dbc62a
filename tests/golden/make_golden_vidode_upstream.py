"""Generate tests/golden/vidode_upstream.npz (dev container only; never runs on the GPU box).

Imports upstream Vid-ODE's own classes from the REFERENCE checkout (read-only, never copied): `models.conv_odegru.VidODE`,
`models.base_conv_gru.ConvGRUCell` / `Encoder_z0_ODE_ConvGRU`, `models.ode_func`, `models.layers`.  Three modules they import are not
needed or not available here and are stubbed before the import: `torchdiffeq` (absent from the image; its `odeint` is the project's
oracle restatement, oracle/torchdiffeq_ref.py), `utils` (the reference's utils.py pulls in plotting packages; the model uses
`utils.Tracker` and `utils.get_device` only) and `wandb`.

The weights and inputs are PROCEDURAL (tests/_vidode_upstream_ref.py: index formulas), so the file holds arrays of outputs only: the
sorted state_dict keys and the parameter count of upstream's VidODE, one masked ConvGRUCell step, the encoder's (mean, std) for both
values of run_backwards, and compute_all_losses in extrapolation and interpolation mode (BatchNorm in train(), dec_diff = 'euler').
Time steps go in as float64 tensors.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vidode_upstream.py REFERENCE_ROOT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
sys.dont_write_bytecode = True

import _vidode_upstream_ref as ref  # noqa: E402
from oracle import torchdiffeq_ref  # noqa: E402


def stub_modules():
    td = types.ModuleType("torchdiffeq")
    td.odeint = torchdiffeq_ref.odeint
    ut = types.ModuleType("utils")

    class Tracker:
        def write_info(self, key, value):
            pass

    ut.Tracker = Tracker
    ut.get_device = lambda t: t.device
    sys.modules.update({"torchdiffeq": td, "utils": ut, "wandb": types.ModuleType("wandb")})


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_vidode_upstream.py REFERENCE_ROOT")
    stub_modules()
    sys.path.insert(0, os.path.join(sys.argv[1], "Vid-ODE"))
    from models import base_conv_gru, conv_odegru, layers, ode_func
    out = {}
    tracker = sys.modules["utils"].Tracker()

    # one masked cell step
    sd, x, h = ref.cell_case(64)
    cell = base_conv_gru.ConvGRUCell((16, 16), 64, 64, (3, 3), True, torch.FloatTensor)
    cell.load_state_dict(sd)
    with torch.no_grad():
        out["cell.h_next"] = cell(x, h, torch.tensor(ref.CELL_MASK)).numpy()

    # the encoder, both visiting orders
    sd, frames = ref.encoder_case(64, 2)
    func = ode_func.ODEFunc(None, 64, 64, layers.create_convnet(64, 64, n_layers=1, n_units=64))
    solver = ode_func.DiffeqSolver(64, func, "euler", 64, odeint_rtol=1e-3, odeint_atol=1e-4)
    for rb in (True, False):
        enc = base_conv_gru.Encoder_z0_ODE_ConvGRU((16, 16), 64, 64, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                                   return_all_layers=True, z0_diffeq_solver=solver, run_backwards=rb)
        enc.load_state_dict(sd)
        with torch.no_grad():
            mean, std = enc(frames, torch.tensor(ref.ENC_TIMES, dtype=torch.float64), mask=torch.tensor(ref.ENC_MASK).unsqueeze(-1),
                            tracker=tracker)
        out[f"enc.rb{int(rb)}.mean"], out[f"enc.rb{int(rb)}.std"] = mean.numpy(), std.numpy()

    # the model
    for extrap in (True, False):
        torch.manual_seed(0)
        model = conv_odegru.VidODE(ref.model_opt(extrap), "cpu")
        ref_sd = model.state_dict()
        if extrap:
            out["keys"] = np.array(sorted(ref_sd.keys()))
            out["n_params"] = np.array([sum(p.numel() for p in model.parameters())], dtype=np.int64)
        model.load_state_dict(ref.model_state_dict(ref_sd))
        model.train()
        with torch.no_grad():
            res = model.compute_all_losses(dict(ref.model_batch()))
        tag = "extrap" if extrap else "interp"
        out[f"{tag}.loss"] = res["loss"].numpy().reshape(1)
        out[f"{tag}.pred_y"] = res["pred_y"].numpy()
    path = os.path.join(HERE, "vidode_upstream.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
