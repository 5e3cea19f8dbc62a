"""Inputs and runs shared by tests/test_hip_sync_batchnorm.py (the full batch in one process) and tests/_syncbn_gpu_worker.py (one
shard per rank): both sides execute the same code on the same data, so they differ in the sharding alone."""
import argparse
import contextlib

import torch

import _vidode_upstream_ref as up
from conftest import procedural_tensor, vidode_state_dict

OP_SHAPE = (3, 32, 8, 8)                                             # two ranks: shards of 2 + 1 samples
OP_CASES = [(upsample, conv_bias) for upsample in (False, True) for conv_bias in (False, True)]
SHARDED = ("observed_data", "data_to_predict", "observed_mask", "mask_predicted_data")
BATCH, N_OBS, N_PRED = 4, 2, 2                                       # the models: shards of 2 + 2 (the loss is a batch mean)
RK4_OPT = argparse.Namespace(n_downs=2, resolution=64, in_channels=1, n_layers=2, decode_diff_method="rk4")
# convolution biases in front of a BatchNorm with batch statistics: their gradient is exactly zero in the fused pass
BN_FED_BIASES = {"encoder.cnn_encoder.0.bias", "encoder.cnn_encoder.3.bias", "encoder.cnn_encoder.6.bias", "decoder.model.1.bias",
                 "decoder.model.5.bias"}


def make_blob():
    from ode_rl_amd.models import conv_odegru
    from ode_rl_amd.models.VidODE import VidODE
    g = torch.Generator().manual_seed(11)
    n, c, h, w = OP_SHAPE
    x = torch.randn(OP_SHAPE, generator=g)
    x[2:] *= 3.0                                                     # the second shard's statistics differ
    blob = {"op.x": x, "op.conv_bias": torch.randn(c, generator=g) * 0.3,
            ("op.gout", False): torch.randn(n, c, h, w, generator=g), ("op.gout", True): torch.randn(n, c, 2 * h, 2 * w, generator=g),
            "op.bn": {"weight": torch.rand(c, generator=g) + 0.5, "bias": torch.randn(c, generator=g) * 0.5,
                      "running_mean": torch.randn(c, generator=g), "running_var": torch.rand(c, generator=g) + 0.5,
                      "num_batches_tracked": torch.tensor(3)}}
    blob["upstream.state"] = up.model_state_dict(conv_odegru.VidODE(up.model_opt(True), torch.device("cpu")).state_dict())
    observed = procedural_tensor((BATCH, N_OBS, 1, 64, 64), 4601, 0.0, 1.0)
    observed[BATCH // 2:] *= 3.0
    steps = up.TARGET_STEP * torch.arange(1, N_PRED + 1, dtype=torch.float32).view(1, N_PRED, 1, 1, 1)
    blob["upstream.batch"] = {"observed_data": observed, "data_to_predict": procedural_tensor((BATCH, N_PRED, 1, 64, 64), 4602, 0.0, 1.0) + steps,
                              "observed_tp": torch.tensor(up.MODEL_OBS_TP[:N_OBS], dtype=torch.float64),
                              "tp_to_predict": torch.tensor(up.MODEL_PRED_TP[:N_PRED], dtype=torch.float64),
                              "observed_mask": torch.ones(BATCH, N_OBS, 1), "mask_predicted_data": torch.ones(BATCH, N_PRED, 1)}
    blob["rk4.state"] = vidode_state_dict(VidODE(RK4_OPT, torch.device("cpu")).state_dict(), 14)
    blob["rk4.frames"] = observed.clone()
    return blob


def run_op(blob, case, lo, hi, dev, group):
    """bn_relu_up forward + backward on samples [lo, hi) of the op-level batch; everything the pass produces, on the host."""
    from ode_rl_amd.autograd import bn_relu_up
    upsample, with_bias = case
    bn = torch.nn.BatchNorm2d(OP_SHAPE[1])
    bn.load_state_dict(blob["op.bn"])
    bn = bn.to(dev).train()
    x = blob["op.x"][lo:hi].to(dev).requires_grad_(True)
    cb = blob["op.conv_bias"].to(dev).requires_grad_(True) if with_bias else None
    y = bn_relu_up(x, bn, upsample, conv_bias=cb, group=group)
    y.backward(blob["op.gout", upsample][lo:hi].to(dev))
    res = {"out": y.detach(), "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "num_batches_tracked": bn.num_batches_tracked}
    if with_bias:
        res["dconv_bias"] = cb.grad
    return {k: v.cpu() for k, v in res.items()}


@contextlib.contextmanager
def repeatable_library_convolutions():
    """The models' BatchNorm encoder and flow decoder convolve through the library, whose default choice among its algorithms is not the
    same in every call: the deterministic ones on every side of a comparison, as tests/test_hip_vidode_upstream.py does."""
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was


def _buffers(model):
    return {k: v.detach().cpu() for k, v in model.named_buffers() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def upstream_model(blob, dev, fused=True):
    from ode_rl_amd.models import conv_odegru
    model = conv_odegru.VidODE(up.model_opt(True), dev, fused=fused)
    model.load_state_dict(blob["upstream.state"])
    return model.train()


def upstream_step(model, batch, reduce_gradients):
    """compute_all_losses -> backward -> reduce_gradients(): prediction, every parameter gradient, every BatchNorm buffer."""
    res = model.compute_all_losses(dict(batch))
    res["loss"].backward()
    reduce_gradients()
    return {"pred_y": res["pred_y"].detach().cpu(), "grads": {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None},
            "buffers": _buffers(model)}


def rk4_model(blob, dev, fused=True):
    from ode_rl_amd.models.VidODE import VidODE
    model = VidODE(RK4_OPT, torch.device("cpu"))
    model.load_state_dict(blob["rk4.state"])
    model.conv_encoder.fused = model.conv_decoder.fused = fused
    return model.to(dev).train()


def rk4_forward(model, frames, dev):
    """One train() forward of models/VidODE.py's model, decoder solved with rk4."""
    b = frames.shape[0]
    ts = torch.arange(N_OBS + N_PRED, dtype=torch.float64) / (N_OBS + N_PRED)
    bd = {"observed_tp": ts[:N_OBS].to(dev), "tp_to_predict": ts[N_OBS:].to(dev), "observed_mask": torch.ones(b, N_OBS, 1, device=dev),
          "mask_predicted_data": torch.ones(b, N_PRED, 1, device=dev)}
    with torch.no_grad():
        pred, extra = model(frames.to(dev), bd)
    return {"pred_x": pred.cpu(), "optical_flow": extra["optical_flow"].cpu(), "buffers": _buffers(model)}
