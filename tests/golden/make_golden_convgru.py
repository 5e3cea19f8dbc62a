"""Generate tests/golden/convgru_model.npz (dev container only; never runs on the GPU box).

Imports the REFERENCE's own `models.ConvGRU.ConvGRU` from /root/reference (read-only, never copied) under the import stubs of
make_golden.py, plus what this model needs on a CPU-only box: the reference's ConvGRUCell.forward calls
`.cuda()` on the zero tensors it creates, so `torch.Tensor.cuda` is made the identity for the run.  `modules/ImpalaCNN.py`, which
the model file imports, needs nothing beyond those stubs.

The weights are PROCEDURAL (conftest.procedural_state_dict, seed 21): the two cells alone are 2 x 2.46 MB, so the fixture stores
only the key list, the parameter count, the inputs and the prediction; the test rebuilds the same weights from the formula.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convgru.py
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (sets up sys.path for conftest / oracle)
from conftest import procedural_state_dict, procedural_tensor  # noqa: E402

SEED = 21


def convgru_opt(phase="train", batch_size=2, test_out_seq=190):
    """The options the reference's ConvGRU reads (configs.yaml train_/test_mmnist_cgru_len20 and its defaults)."""
    return argparse.Namespace(convgru_out_ch=64, conv_encoder_out_ch=64, in_channels=1, phase=phase, train_in_seq=10, train_out_seq=10,
                              test_in_seq=10, test_out_seq=test_out_seq, batch_size=batch_size, depth=1, resolution=64)


def main():
    make_golden._install_stubs()
    torch.Tensor.cuda = lambda self, *a, **k: self   # ConvGRUCell.forward: torch.zeros(...).cuda() on a CPU box
    from models.ConvGRU import ConvGRU
    torch.manual_seed(0)
    model = ConvGRU(convgru_opt(), "cpu").eval()
    ref_sd = model.state_dict()
    model.load_state_dict(procedural_state_dict(ref_sd, SEED))
    inputs = procedural_tensor((2, 10, 1, 64, 64), 2100 + SEED, 0.0, 1.0)
    with torch.no_grad():
        pred = model(inputs)
    assert tuple(pred.shape) == (2, 10, 1, 64, 64)
    np.savez_compressed(os.path.join(HERE, "convgru_model.npz"), keys=np.array(list(ref_sd.keys())),
                        shapes=np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()]),
                        n_params=np.array([sum(p.numel() for p in model.parameters())], dtype=np.int64), seed=np.array([SEED]),
                        inputs=inputs.numpy(), pred=pred.numpy())
    print("convgru_model.npz:", len(ref_sd), "keys,", int(sum(p.numel() for p in model.parameters())), "parameters, pred range",
          float(pred.min()), float(pred.max()))


if __name__ == "__main__":
    main()
