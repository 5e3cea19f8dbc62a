"""Generate tests/golden/gan.npz (dev container only; never runs on the GPU box).

Loads the REFERENCE's own `Vid-ODE/models/gan.py` (read-only, never copied) by file path -- it imports nothing but torch -- and
runs its `Discriminator` on the CPU: `netD_img` (in_ch = c) and an extrapolating `netD_seq` with t_in = t (in_ch = (t + 1) c), their
`forward`, `netD_adv_loss` and `netG_adv_loss`.

Two of its paths cannot run on a CPU-only box and are covered by the restatement in tests/_gan_ref.py alone: the interpolation form
(`rearrange_seq_interp` calls `.cuda()`), and the zero-padding branch of `get_real_fake_seqs` (`.to(input_real.get_device())`, which
is -1 on the CPU); with t_in = t no row is padded, so the extrapolating case here never reaches it.

The weights are PROCEDURAL (tests/_gan_ref.py `state_dict`: an index formula): the discriminator has 2.7 M parameters whatever the
image size, so the fixture stores the key list and shapes, and the test rebuilds the same weights.  Inputs are 16 x 16.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gan.py REFERENCE_ROOT   (the checkout of the reference repository)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import _gan_ref  # noqa: E402
from conftest import procedural_tensor  # noqa: E402

SEED_IMG, SEED_SEQ = 31, 32
B, T, C, H = 2, 3, 2, 16


def inputs():
    """(real, fake, input_real), each (B, T, C, H, H) in [0, 1): what the test regenerates."""
    return tuple(procedural_tensor((B, T, C, H, H), 3100 + k, 0.0, 1.0) for k in range(3))


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_gan.py REFERENCE_ROOT")
    root = sys.argv[1]
    spec = importlib.util.spec_from_file_location("reference_gan", os.path.join(root, "Vid-ODE", "models", "gan.py"))
    gan = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gan)
    real, fake, input_real = inputs()
    out = {}
    for tag, seq, in_ch, seed in (("img", False, C, SEED_IMG), ("seq", True, (T + 1) * C, SEED_SEQ)):
        net = gan.Discriminator(in_ch=in_ch, device="cpu", seq=seq, is_extrap=True)
        ref_sd = net.state_dict()
        if tag == "img":
            out["keys"] = np.array(list(ref_sd.keys()))
        out[f"{tag}.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
        assert {k: tuple(v.shape) for k, v in ref_sd.items()} == _gan_ref.shapes(in_ch)
        net.load_state_dict(_gan_ref.state_dict(in_ch, seed))
        with torch.no_grad():
            x = net.rearrange_seq(real, fake, input_real, only_fake=True) if seq else fake.view(-1, C, H, H)
            out[f"{tag}.forward"] = net(x).numpy()
            out[f"{tag}.d_loss"] = net.netD_adv_loss(real, fake, input_real if seq else None).numpy().reshape(1)
            out[f"{tag}.g_loss"] = net.netG_adv_loss(real if seq else None, fake, input_real if seq else None).numpy().reshape(1)
        if seq:
            out["seq.rows"] = x.numpy()
    out["n_params"] = np.array([sum(int(np.prod(s)) for s in _gan_ref.shapes(C).values())], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "gan.npz"), **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "gan.npz")))


if __name__ == "__main__":
    main()
