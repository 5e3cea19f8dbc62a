"""Evaluation metrics, the part that needs no GPU: the CPU restatement of scikit-image's SSIM (tests/_metrics_ref.py) is pinned
against an independent direct form and closed-form cases; the new C-ABI export is in step with the header and refuses bad arguments
before any HIP call; `frame_metrics` has no CPU fallback; `train.evaluate` / `train.test_batch` do the reference's bookkeeping
(eval mode restored, no_grad, the [-0.5, 0.5] <-> [0, 1] shifts, means over batches, PSNR averaged per batch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _metrics_ref as mr
from conftest import ROOT


def _pairs():
    pred, truth = mr.make_frames(1, 4, 1, seed=11)   # t = 0..3 -> the four degradations in order
    return [(mr.DEGRADATIONS[t], pred[0, t, 0], truth[0, t, 0]) for t in range(4)]


def test_restatement_is_exactly_one_on_identical_images():
    for _, _, x in _pairs():
        assert mr.ssim_ref(x, x, 1.0) == 1.0
        assert mr.ssim_ref(x * 255.0, x * 255.0, 255.0) == 1.0


def test_restatement_on_constant_images_has_the_closed_form():
    for a, b, R in ((0.25, 0.75, 1.0), (0.0, 1.0, 1.0), (40.0, 200.0, 255.0)):
        c1 = (0.01 * R) ** 2
        got = mr.ssim_ref(np.full((64, 64), a), np.full((64, 64), b), R)
        # variances and covariance vanish: the contrast term is C2 / C2 = 1
        assert abs(got - (2 * a * b + c1) / (a * a + b * b + c1)) <= 1e-12


def test_restatement_matches_the_direct_form_and_is_symmetric():
    seen = []
    for kind, p, x in _pairs():
        for R, s in ((1.0, 1.0), (255.0, 255.0)):
            ref = mr.ssim_ref(p * s, x * s, R)
            assert abs(ref - mr.ssim_direct(p * s, x * s, R)) <= 1e-12, kind
            assert abs(ref - mr.ssim_ref(x * s, p * s, R)) <= 1e-12, kind
        seen.append(ref)
    assert min(seen) < 0.1 and max(seen) > 0.5, seen   # the degradations spread over the range: nothing sits near 1


def test_fp32_restatement_is_close_to_fp64():
    """scipy on float32 arrays (the reference's own path: its frames are float32) against float64: the basis of the GPU tolerance."""
    for kind, p, x in _pairs():
        assert abs(mr.ssim_ref(p * 255.0, x * 255.0, 255.0, np.float32) - mr.ssim_ref(p * 255.0, x * 255.0, 255.0)) <= 2e-6, kind


def test_metrics_ref_shapes_and_psnr_of_a_perfect_prediction():
    pred, truth = mr.make_frames(2, 3, 3, seed=5)
    pred[:, 1] = truth[:, 1]
    m = mr.metrics_ref(pred, truth, 1.0)
    assert m["sse"].shape == (2, 3) and m["ssim_per_sample"].shape == (2, 3) and m["mse"].shape == (3,)
    assert m["mse"][1] == 0.0 and m["psnr"][1] == np.inf and m["ssim"][1] == 1.0
    assert np.isfinite(m["psnr"][[0, 2]]).all() and (m["ssim"][[0, 2]] < 0.95).all()


def test_header_and_ctypes_table_declare_frame_metrics():
    import ode_rl_amd
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "odecgru_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+odehip_frame_metrics\s*\(([^)]*)\)\s*;", src)
    assert decl, "odehip_frame_metrics is not declared in the header"
    params = [p.strip() for p in decl.group(1).split(",")]
    kinds = ["p" if "*" in p else ("f" if p.startswith("float") else "i") for p in params]
    res, args = ode_rl_amd._lib.SIGNATURES["odehip_frame_metrics"]
    table = ["p" if a is ctypes.c_void_p else ("f" if a is ctypes.c_float else "i") for a in args]
    assert res is ctypes.c_int and kinds == table, (kinds, table)
    lib = ode_rl_amd._lib.load()
    assert hasattr(lib, "odehip_frame_metrics")
    assert lib.odehip_version() == 13 == ode_rl_amd._lib.ABI_VERSION
    assert int(re.search(r"#define\s+ODEHIP_ABI_VERSION\s+(\d+)", src).group(1)) == 13


def test_argument_errors_without_gpu():
    """Checked before any HIP call, so on a box without a GPU too: -1 and a message that names the problem."""
    import ode_rl_amd
    L = ode_rl_amd._lib
    lib = L.load()
    p = ctypes.c_void_p(64)

    def call(pred=p, truth=p, b=2, t=3, c=1, h=64, w=64, r=1.0, outs=(p, p, p, p, p)):
        rc = lib.odehip_frame_metrics(pred, truth, b, t, c, h, w, r, *outs, None)
        return rc, lib.odehip_last_error().decode()

    for kw in ({"pred": None}, {"truth": None}, {"outs": (p, p, None, p, p)}, {"outs": (None, p, p, p, p)}):
        rc, msg = call(**kw)
        assert rc == -1 and "null" in msg, (kw, msg)
    rc, msg = call(h=32, w=32)
    assert rc == -1 and "32 x 32" in msg and "shape" in msg, msg
    rc, msg = call(w=48)
    assert rc == -1 and "64 x 48" in msg, msg
    rc, msg = call(c=2)
    assert rc == -1 and "channels 2" in msg, msg
    rc, msg = call(t=0)
    assert rc == -1 and "n_frames (0)" in msg, msg
    rc, msg = call(b=0)
    assert rc == -1 and "batch (0)" in msg, msg
    for r in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(r=r)
        assert rc == -1 and "data_range" in msg, (r, msg)
    with pytest.raises(ValueError, match="data_range"):
        L.check(rc)


def test_frame_metrics_has_no_cpu_fallback():
    import ode_rl_amd
    x = torch.zeros(1, 1, 1, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ode_rl_amd.frame_metrics(x, x)
    with pytest.raises(TypeError):
        ode_rl_amd.frame_metrics(x.numpy(), x)
    assert ode_rl_amd.frame_metrics is ode_rl_amd.metrics.frame_metrics


# ---- train.test_batch / train.evaluate with a stub model and a stubbed frame_metrics -----------------------------------------

class _StubModel(torch.nn.Module):
    """get_prediction: the last observed frame times `gain`, repeated; records what it was called with."""

    def __init__(self, fail_at=None):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(0.5))
        self.calls = []
        self.fail_at = fail_at

    def get_prediction(self, inputs, batch_dict=None):
        self.calls.append({"training": self.training, "grad": torch.is_grad_enabled(), "min": float(inputs.min()), "max": float(inputs.max()),
                           "batch_dict": batch_dict})
        if self.fail_at is not None and len(self.calls) > self.fail_at:
            raise RuntimeError("stub model failure")
        t_out = batch_dict["data_to_predict"].shape[1]
        return (inputs[:, -1:] * self.gain).expand(-1, t_out, -1, -1, -1)

    def get_loss(self, pred, truth):
        return torch.nn.functional.mse_loss(pred, truth)


def _batch(seed, b=2, t_in=2, t_out=3):
    g = torch.Generator().manual_seed(seed)
    return {"observed_data": torch.rand(b, t_in, 1, 64, 64, generator=g) - 0.5, "data_to_predict": torch.rand(b, t_out, 1, 64, 64, generator=g) - 0.5}


def _stub_frame_metrics(seen):
    from ode_rl_amd.metrics import FrameMetrics

    def fm(pred, truth, data_range=1.0):
        seen.append({"pred": pred.clone(), "truth": truth.clone(), "R": data_range, "grad": torch.is_grad_enabled(),
                     "requires_grad": pred.requires_grad})
        sse = ((pred - truth) ** 2).sum(dim=(2, 3, 4))
        mse = sse.sum(0) / (pred.shape[0] * pred[0, 0].numel())
        return FrameMetrics(mse, 10 * torch.log10(data_range ** 2 / mse), 1 - mse, sse, 1 - sse / pred[0, 0].numel())
    return fm


def test_test_batch_shifts_to_unit_range_and_back():
    from ode_rl_amd import train
    model = _StubModel()
    bd = _batch(1)
    pred, truth, loss = train.test_batch(model, bd)
    call = model.calls[0]
    assert 0.0 <= call["min"] and call["max"] <= 1.0 and call["max"] > 0.5 and call["batch_dict"] is bd
    assert torch.equal(truth, (bd["data_to_predict"] + 0.5) - 0.5)
    assert torch.equal(pred, ((bd["observed_data"][:, -1:] + 0.5) * 0.5).expand(-1, 3, -1, -1, -1) - 0.5)
    want = torch.nn.functional.mse_loss(pred + 0.5, truth + 0.5)
    assert isinstance(loss, torch.Tensor) and abs(float(loss.detach()) - float(want.detach())) <= 1e-7


def test_evaluate_averages_over_batches_and_restores_training_mode(monkeypatch):
    import ode_rl_amd
    from ode_rl_amd import train
    seen = []
    monkeypatch.setattr(ode_rl_amd.metrics, "frame_metrics", _stub_frame_metrics(seen))
    model = _StubModel()
    model.train()
    batches = [_batch(2), _batch(3), _batch(4)]
    res = train.evaluate(model, iter(batches))
    assert model.training, "the training mode was not restored"
    assert len(model.calls) == 3 and all(not c["training"] and not c["grad"] for c in model.calls)
    assert all(s["R"] == 1.0 and not s["grad"] and not s["requires_grad"] for s in seen)
    for s, bd in zip(seen, batches):   # frame_metrics sees [0, 1] frames: (x + 0.5 - 0.5) + 0.5
        assert torch.equal(s["truth"], ((bd["data_to_predict"] + 0.5) - 0.5) + 0.5)
        assert 0.0 <= float(s["pred"].min()) and float(s["pred"].max()) <= 1.0
    mse = torch.stack([((s["pred"] - s["truth"]) ** 2).mean(dim=(0, 2, 3, 4)) for s in seen])       # (batches, T)
    psnr_per_batch = 10 * torch.log10(1.0 / mse)
    assert res["mse"].shape == (3,) and res["mse"].device.type == "cpu"
    assert torch.allclose(res["mse"], mse.mean(0), rtol=1e-5, atol=0)
    assert torch.allclose(res["psnr"], psnr_per_batch.mean(0), rtol=0, atol=1e-4)
    assert torch.allclose(res["ssim"], (1 - mse).mean(0), rtol=1e-5, atol=0)
    losses = [float(torch.nn.functional.mse_loss(s["pred"], s["truth"])) for s in seen]
    assert abs(res["loss"] - sum(losses) / 3) <= 1e-6
    assert res["avg_mse"] == float(res["mse"][-1]) and res["avg_psnr"] == float(res["psnr"][-1]) and res["avg_ssim"] == float(res["ssim"][-1])
    model.eval()
    train.evaluate(model, batches[:1])
    assert not model.training, "an eval-mode model must stay in eval mode"


def test_evaluate_psnr_is_the_mean_of_per_batch_psnrs(monkeypatch):
    """One batch predicted almost perfectly (mse 1e-4: 40 dB), one badly: the mean of the two PSNRs is far from the PSNR of the mean MSE."""
    import ode_rl_amd
    from ode_rl_amd import train
    monkeypatch.setattr(ode_rl_amd.metrics, "frame_metrics", _stub_frame_metrics([]))
    model = _StubModel()
    good, bad = _batch(5), _batch(6)
    good["data_to_predict"] = ((good["observed_data"][:, -1:] + 0.5) * 0.5 + 0.01).expand(-1, 3, -1, -1, -1) - 0.5
    res = train.evaluate(model, [good, bad])
    mse_bad = 2 * float(res["mse"][0]) - 1e-4
    assert abs(float(res["psnr"][0]) - 0.5 * (40.0 + 10 * math.log10(1 / mse_bad))) <= 1e-2
    assert float(res["psnr"][0]) - 10 * math.log10(1 / float(res["mse"][0])) > 5.0


def test_evaluate_restores_training_mode_when_the_model_raises(monkeypatch):
    import ode_rl_amd
    from ode_rl_amd import train
    monkeypatch.setattr(ode_rl_amd.metrics, "frame_metrics", _stub_frame_metrics([]))
    model = _StubModel(fail_at=1)
    model.train()
    with pytest.raises(RuntimeError, match="stub model failure"):
        train.evaluate(model, [_batch(7), _batch(8)])
    assert model.training and torch.is_grad_enabled()
    with pytest.raises(ValueError, match="no batches"):
        train.evaluate(model, [])
    assert model.training
