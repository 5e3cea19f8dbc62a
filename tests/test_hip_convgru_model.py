"""The ConvGRU baseline end to end on the GPU: forward against the fixture the reference's own class wrote (procedural weights), a
training step through train_batch, evaluation on 10 -> 190 frames."""
import argparse

import pytest
import torch

import _convgru_ref as ref
from conftest import load_golden, procedural_state_dict, record, rel_l2

pytestmark = pytest.mark.gpu


def _opt(**kw):
    o = dict(convgru_out_ch=64, conv_encoder_out_ch=64, in_channels=1, phase="train", train_in_seq=10, train_out_seq=10, test_in_seq=10,
             test_out_seq=190, batch_size=2, depth=1, resolution=64)
    o.update(kw)
    return argparse.Namespace(**o)


def _model(cuda, seed, **kw):
    from ode_rl_amd.models import ConvGRU
    model = ConvGRU(_opt(**kw), torch.device("cpu"))
    sd = procedural_state_dict(model.state_dict(), seed)
    model.load_state_dict(sd)
    return model.to(cuda), sd


def test_forward_matches_the_reference_fixture(cuda):
    g = load_golden("convgru_model.npz")
    model, sd = _model(cuda, int(g["seed"][0]))
    inputs, want = torch.from_numpy(g["inputs"]), torch.from_numpy(g["pred"])
    with torch.no_grad():
        got = model(inputs.to(cuda))
        r64 = ref.model_forward(ref.cast(sd, torch.float64), inputs.double(), 10, 10)
        r32 = ref.model_forward(sd, inputs, 10, 10)
    assert got.shape == want.shape == (2, 10, 1, 64, 64)
    tol, d32 = ref.bound(r32, r64, 2e-5)
    tol += 2e-6                                  # the fused frame codec's own bound
    err_fix, err64, fix64 = rel_l2(got, want), rel_l2(got, r64), rel_l2(want, r64)
    record("convgru_model_d32", d32)
    record("convgru_model_hip_vs_fixture", err_fix)
    record("convgru_model_hip_vs_float64", err64)
    print(f"model: float32 restatement {d32:.3e}, fixture vs float64 {fix64:.3e}, HIP vs fixture {err_fix:.3e}, HIP vs float64 {err64:.3e}, bound {tol:.3e}")
    assert fix64 <= tol, fix64                   # the restatement IS the reference's model
    assert err_fix <= tol and err64 <= tol, (err_fix, err64, tol)


def _batch(b, t_in, t_out, seed):
    g = torch.Generator().manual_seed(seed)
    return {"observed_data": torch.rand(b, t_in, 1, 64, 64, generator=g) - 0.5, "data_to_predict": torch.rand(b, t_out, 1, 64, 64, generator=g) - 0.5,
            "observed_tp": None, "tp_to_predict": None}


def test_train_batch_is_finite_and_repeatable(cuda):
    from ode_rl_amd import train
    from ode_rl_amd.optim import FusedAdam
    batch = _batch(2, 10, 10, 5)
    runs = []
    for _ in range(2):
        model, _ = _model(cuda, 22)
        optim = FusedAdam(model.parameters(), lr=1e-3)
        losses = [float(train.train_batch(model, batch, optim)[2]) for _ in range(3)]
        runs.append((losses, [p.detach().clone() for p in model.parameters()]))
    (la, pa), (lb, pb) = runs
    assert all(l == l and abs(l) < float("inf") for l in la) and la == lb, (la, lb)
    assert la[-1] < la[0], la
    assert all(bool(torch.isfinite(p).all()) for p in pa) and all(torch.equal(p, q) for p, q in zip(pa, pb))


def test_evaluate_on_190_frames(cuda):
    from ode_rl_amd import train
    model, _ = _model(cuda, 23, phase="test")
    out = train.evaluate(model, [_batch(2, 10, 190, 6), _batch(2, 10, 190, 7)])
    for k in ("mse", "psnr", "ssim"):
        assert out[k].shape == (190,) and bool(torch.isfinite(out[k]).all()), k
    assert out["loss"] == out["loss"] and model.training
