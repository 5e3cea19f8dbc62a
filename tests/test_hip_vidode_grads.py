"""VidODE's training step end to end: get_prediction -> get_loss -> backward() once on the device, every parameter gradient, the forward,
the loss and the BatchNorm buffers against tests/_vidode_ref.py in float64 (autograd through the oracle modules; pinned to the reference's
own forward by tests/test_vidode_ref_cpu.py).  The joints this holds together only show in the backward direction: pred_outputs fed by
the warp composite AND the intermediates slice of the loss, each latent frame feeding two decoder calls, the BatchNorm encoder run twice,
the convolution bias folded into the fused BatchNorm pass, mask_predicted_data leaving all-zero gradient frames inside the trajectory,
observed_mask in the 128-channel encoder backward, the permutes (or, as written, the `.view`) around cell and solver.

Cases (tests/_vidode_grad_cases.py): A train rk4 c=1 B=2 3/3; B train rk4 c=3 B=3 3/3 with both masks; C train dopri5 3/2; D eval rk4;
E eval rk4 as written (B == T == 3).  Bounds: forward 5e-5 (the whole-model bound of tests/test_hip_vidode.py), loss 1e-5 |loss| + 1e-7 and
gradients max(4 d32, 1e-3) with d32 the float32 restatement's own distance from float64 (tests/test_hip_train_end_to_end.py,
tests/_convgru_ref.py::bound); the reference alone must have d32 <= 2.5e-4, so no bound exceeds 1e-3.
The float64 restatement is the slow part: 0.5-0.8 s per case on 16 CPU threads (5-14 s on 8 busy ones), the float32 one 0.1 s (0.5-5 s);
both are computed once per case.  Observed: profiles/vidode_grads_observed.json."""
import copy
import functools

import pytest
import torch

import _vidode_grad_cases as cases
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

ALL = sorted(cases.CASES)
TRAIN = [c for c in ALL if cases.training(c)]
ENCODER_BN = ("conv_encoder.cnn_encoder.1.", "conv_encoder.cnn_encoder.4.", "conv_encoder.cnn_encoder.7.")
DECODER_BN = ("conv_decoder.cnn_decoder.2.", "conv_decoder.cnn_decoder.6.")


@functools.lru_cache(maxsize=None)
def _device_step(case):
    """The one training step of the case on the device: forward values, loss, gradients and buffers, all detached."""
    import ode_rl_amd
    cuda = torch.device("cuda:0")
    model = copy.deepcopy(cases.build_model(case)).to(cuda)
    bd = {k: v.to(cuda) for k, v in cases.batch(case).items()}
    # the codec's convolutions are library calls whose default algorithms differ from run to run in the last bits (tests/test_hip_encoder_mask.py::
    # reproducible_library_convolutions), enough to move a BatchNorm pre-activation across zero: the deterministic ones, so that a run repeats
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        pred = model.get_prediction(bd["observed_data"], bd)
        accepted = dict(ode_rl_amd.last_stats).get("n_accept") if cases.opt_of(case).decode_diff_method == "dopri5" else None
        loss = model.get_loss(pred, bd["data_to_predict"])
        loss.backward()
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
    return {"pred_x": pred.detach(), "pred_intermediates": model.extra_info["pred_intermediates"].detach(), "loss": float(loss),
            "grads": {k: (None if p.grad is None else p.grad.detach()) for k, p in model.named_parameters()},
            "buffers": {k: v.detach().clone() for k, v in model.named_buffers()}, "n_accept": accepted}


def _weight_of(label):
    return label.replace("[std]", "").replace(".bias", ".weight")


@pytest.mark.parametrize("case", ALL)
def test_the_reference_alone_meets_the_conditions_of_the_bounds(case):
    """Nothing of the device here: every compared gradient of the float32 restatement lies within 2.5e-4 of the float64 one (so that
    4 d32 never exceeds the 1e-3 floor) and has a non-zero norm; the gradients that are zero by construction are, in float64, below 1e-10
    of their convolution's weight gradient; dopri5 accepts the same number of steps in both precisions."""
    r64, r32 = cases.reference(case, torch.float64), cases.reference(case, torch.float32)
    by_norm64, zero64 = cases.compared(case, r64["grads"])
    by_norm32, _ = cases.compared(case, r32["grads"])
    assert sorted(r64["grads"]) == sorted(cases.state(case)[0])
    for (label, g64), (_, g32) in zip(by_norm64, by_norm32):
        assert float(g64.norm()) > 0, label
        assert record(f"vidode_grads.{case}.{label}.d32", rel_l2(g32, g64)) <= 2.5e-4, label
    for label, g in zero64:
        assert float(g.abs().max()) <= 1e-10 * float(r64["grads"][_weight_of(label)].norm()), label
    if not cases.training(case):
        assert [label for label, _ in zero64] == [n + "[std]" for n in cases.SPLIT_IN_HALVES]
    if cases.opt_of(case).decode_diff_method == "dopri5":
        assert r64["solver_stats"]["n_accept"] == r32["solver_stats"]["n_accept"] >= 1
    record(f"vidode_grads.{case}.seconds_float64", r64["seconds"])
    record(f"vidode_grads.{case}.seconds_float32", r32["seconds"])


@pytest.mark.parametrize("case", ALL)
def test_forward_and_loss_match_the_float64_restatement(cuda, case):
    ref, dev = cases.reference(case, torch.float64), _device_step(case)
    n = cases.n_decoded(case)
    assert dev["pred_x"].shape == ref["pred_x"].shape and dev["pred_x"].shape[1] == n
    assert record(f"vidode_grads.{case}.forward.pred_x", rel_l2(dev["pred_x"], ref["pred_x"])) <= 5e-5
    assert record(f"vidode_grads.{case}.forward.pred_intermediates", rel_l2(dev["pred_intermediates"], ref["pred_intermediates"])) <= 5e-5
    want = float(ref["loss"])
    record(f"vidode_grads.{case}.forward.loss_rel", abs(dev["loss"] - want) / abs(want))
    assert abs(dev["loss"] - want) <= 1e-5 * abs(want) + 1e-7
    if dev["n_accept"] is not None:   # dopri5: as many accepted steps as the restatement, up to the 2 of test_hip_baseline_configs.py
        record(f"vidode_grads.{case}.n_accept", dev["n_accept"])
        assert abs(dev["n_accept"] - ref["solver_stats"]["n_accept"]) <= 2


@pytest.mark.parametrize("case", ALL)
def test_every_parameter_gradient_matches_float64_autograd(cuda, case):
    r64, r32, dev = cases.reference(case, torch.float64), cases.reference(case, torch.float32), _device_step(case)
    assert sorted(dev["grads"]) == sorted(r64["grads"])
    missing = [k for k, g in dev["grads"].items() if g is None]
    assert not missing, missing
    by_norm64, zero64 = cases.compared(case, r64["grads"])
    by_norm32, _ = cases.compared(case, r32["grads"])
    by_norm, zero = cases.compared(case, dev["grads"])
    assert len(by_norm) + len(zero) - len(cases.SPLIT_IN_HALVES) == len(dev["grads"])       # none skipped
    bad = {}
    for (label, g), (_, g64), (_, g32) in zip(by_norm, by_norm64, by_norm32):
        d32 = rel_l2(g32, g64)
        tol = max(4.0 * d32, 1e-3)
        err = rel_l2(g, g64)
        record(f"vidode_grads.{case}.{label}.d32", d32)
        record(f"vidode_grads.{case}.{label}.hip", err)
        record(f"vidode_grads.{case}.{label}.bound", tol)
        if not err <= tol:
            bad[label] = (err, tol)
    assert not bad, bad
    not_zero = [label for label, g in zero if float(g.abs().max()) != 0.0]
    assert not not_zero, not_zero


@pytest.mark.parametrize("case", TRAIN)
def test_batchnorm_buffers_after_the_step(cuda, case):
    """The encoder's BatchNorms saw two batches (all frames, then the last one), the decoder's one per decoded frame."""
    ref, dev, before = cases.reference(case, torch.float64), _device_step(case), cases.state(case)[1]
    assert sorted(dev["buffers"]) == sorted(ref["buffers"])
    for prefix in ENCODER_BN + DECODER_BN:
        assert record(f"vidode_grads.{case}.{prefix}running_mean", rel_l2(dev["buffers"][prefix + "running_mean"], ref["buffers"][prefix + "running_mean"])) <= 1e-5
        assert record(f"vidode_grads.{case}.{prefix}running_var", rel_l2(dev["buffers"][prefix + "running_var"], ref["buffers"][prefix + "running_var"])) <= 1e-4
        k = prefix + "num_batches_tracked"
        steps = 2 if prefix in ENCODER_BN else cases.n_decoded(case)
        assert int(dev["buffers"][k]) == int(ref["buffers"][k]) == int(before[k]) + steps, k


@pytest.mark.parametrize("case", [c for c in ALL if c not in TRAIN])
def test_eval_mode_leaves_the_buffers_alone(cuda, case):
    dev, before = _device_step(case), cases.state(case)[1]
    assert all(torch.equal(dev["buffers"][k].cpu(), before[k]) for k in before)
