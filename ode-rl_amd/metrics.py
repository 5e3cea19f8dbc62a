"""Evaluation metrics on the device: per-frame MSE, PSNR and SSIM of a predicted sequence, the quantities
the reference's `test()` forms on the host (train_test.py:104-117) -- `F.mse_loss(...).item()` and `math.log10` per predicted frame
and scikit-image's `structural_similarity` per sample and frame (helpers/utils.py:254-271).  Here they come from
`odehip_frame_metrics` (csrc/frame_metrics.hip): two launches for all frames, nothing copied to the host, nothing synchronised."""
import collections

import torch

from . import _lib, hip_ops

FrameMetrics = collections.namedtuple("FrameMetrics", ["mse", "psnr", "ssim", "sse", "ssim_per_sample"])
FrameMetrics.__doc__ = """mse, psnr, ssim: (T,) means over the batch per predicted frame; sse (sum of squared errors) and
ssim_per_sample: (B, T).  float32 device tensors; psnr is +inf where mse is 0 (the reference's math.log10(1 / 0) raises there)."""


def frame_metrics(pred, truth, data_range=1.0):
    """pred, truth: (B, T, C, 64, 64) float32 device tensors, C 1 or 3; data_range: the value range of the frames (a Python number:
    1 for frames in [0, 1], 255 for [0, 255]).  SSIM is scikit-image's structural_similarity(data_range=data_range,
    gaussian_weights=True, use_sample_covariance=False) per channel, averaged over the channels -- the reference's
    get_normalized_ssim before its mean over the batch.  A NaN in a frame makes that frame's values NaN and no others.  Inputs are
    made contiguous if they are not; the outputs never require grad (there is no backward)."""
    hip_ops.require_device_tensor(pred, "pred")
    hip_ops.require_device_tensor(truth, "truth")
    if pred.dim() != 5 or pred.shape != truth.shape:
        raise ValueError(f"frame_metrics: pred and truth must both be (B, T, C, H, W), got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"frame_metrics: pred is on {pred.device}, truth on {truth.device}")
    pred, truth = pred.detach().contiguous(), truth.detach().contiguous()
    b, t, c, h, w = pred.shape
    out = torch.empty(2 * b * t + 3 * t, dtype=torch.float32, device=pred.device)
    sse, ssim_bt = out[:b * t].view(b, t), out[b * t:2 * b * t].view(b, t)
    mse, psnr, ssim = (out[2 * b * t + k * t:2 * b * t + (k + 1) * t] for k in range(3))
    _lib.check(_lib.load().odehip_frame_metrics(hip_ops._ptr(pred), hip_ops._ptr(truth), b, t, c, h, w, float(data_range), hip_ops._ptr(sse),
                                                hip_ops._ptr(ssim_bt), hip_ops._ptr(mse), hip_ops._ptr(psnr), hip_ops._ptr(ssim),
                                                hip_ops._stream()))
    return FrameMetrics(mse, psnr, ssim, sse, ssim_bt)
