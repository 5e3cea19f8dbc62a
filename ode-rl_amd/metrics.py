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


# ---- upstream Vid-ODE's protocol: 8-bit RGB bytes, luma SSIM (csrc/png_metrics.hip) -----------------------------------------------------

PNG_SIZES = (32, 64, 128)   # 16 * 2**n_downs for the n_downs 1, 2, 3 that conv_odegru.VidODE accepts

PngMetrics = collections.namedtuple("PngMetrics", ["ssim", "mse", "sse", "pred_bytes", "truth_bytes"], defaults=(None, None))
PngMetrics.__doc__ = """ssim, mse: (B, T) float64; sse: (B, T) int64 (-1 for an image that holds a NaN); pred_bytes, truth_bytes:
(B, T, S, S, 3) uint8 in PNG pixel order, or None.  Device tensors."""


def _png_inputs(pred, truth):
    hip_ops.require_device_tensor(pred, "pred")
    hip_ops.require_device_tensor(truth, "truth")
    if pred.dim() != 5 or pred.shape != truth.shape:
        raise ValueError(f"png_metrics: pred and truth must both be (B, T, C, S, S), got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"png_metrics: pred is on {pred.device}, truth on {truth.device}")
    b, t, c, h, w = pred.shape
    if c not in (1, 3) or h != w or h not in PNG_SIZES:
        raise ValueError(f"png_metrics: unsupported frame shape (channels {c}, {h} x {w}): 1 or 3 channels of 32 x 32, 64 x 64 or 128 x 128 only")
    if b < 1 or t < 1:
        raise ValueError(f"png_metrics: empty batch {tuple(pred.shape)}")
    pred, truth = pred.detach().contiguous(), truth.detach().contiguous()
    if pred.data_ptr() % 16:      # a view into the middle of a buffer: the kernel loads 16 bytes at a time
        pred = pred.clone()
    if truth.data_ptr() % 16:
        truth = truth.clone()
    return pred, truth


def _png_launch(pred, truth, input_norm, return_bytes, accum):
    b, t, c, s, _ = pred.shape
    out = torch.empty(3, b, t, dtype=torch.int64, device=pred.device)      # one allocation: sse, then the bits of mse and ssim
    sse, mse, ssim = out[0], out[1].view(torch.float64), out[2].view(torch.float64)
    pb = tb = None
    if return_bytes:
        pb = torch.empty((b, t, s, s, 3), dtype=torch.uint8, device=pred.device)
        tb = torch.empty_like(pb)
    _lib.check(_lib.load().odehip_png_metrics(hip_ops._ptr(pred), hip_ops._ptr(truth), b, t, c, s, 1 if input_norm else 0, hip_ops._ptr(sse),
                                              hip_ops._ptr(mse), hip_ops._ptr(ssim), hip_ops._ptr(pb), hip_ops._ptr(tb), hip_ops._ptr(accum),
                                              hip_ops._stream()))
    return PngMetrics(ssim, mse, sse, pb, tb)


def png_metrics(pred, truth, input_norm=True, return_bytes=False):
    """Upstream Vid-ODE's per-image evaluation numbers (Vid-ODE/visualize.save_test_images + evaluate.Evaluation) without PNG files:
    pred, truth (B, T, C, S, S) float32 device tensors, C 1 or 3, S 32, 64 or 128.  Every frame is de-normalised (`input_norm`:
    upstream's opt.input_norm, utils.denorm), quantised to 8-bit RGB exactly as torchvision's save_image does (one channel replicated
    to three), and then: sse = the squared error of the bytes (exact), mse = sse / (255^2 * 3 S S), ssim = scikit-image's
    structural_similarity(data_range=255, gaussian_weights=True, use_sample_covariance=False) of the PIL 'L' luma of the two images,
    in float64.  `return_bytes` also returns the RGB bytes of both sequences, (B, T, S, S, 3): what upstream's PNG files hold.
    A NaN in either frame of an image makes its ssim and mse NaN (sse -1) and touches no other image.  Inputs are made contiguous if
    they are not; one launch, no host synchronisation."""
    pred, truth = _png_inputs(pred, truth)
    return _png_launch(pred, truth, bool(input_norm), bool(return_bytes), None)


class PngEvaluation:
    """Upstream's `evaluate.Evaluation` over a test set, accumulated on the device: `update` adds the images of a batch, `result`
    makes the single host transfer and returns upstream's (avg_ssim, avg_mse, avg_psnr), avg_psnr = 10 log10(1 / avg_mse) -- the PSNR of
    the MEAN MSE, not a mean of PSNRs -- or inf where avg_mse is 0.

    Upstream accumulates the MSE in a float32 device tensor (`avg_mse += F.mse_loss(...)`) and the SSIM in a Python float; here both
    sums are float64 on the device, added one image at a time in ascending order, so they do not depend on the batch split."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PngEvaluation on {self.device}: the HIP path needs a CUDA (ROCm) device and has no CPU fallback")
        self._acc = torch.zeros(3, dtype=torch.int64, device=self.device)   # the bits of two float64 sums, then the image count

    def update(self, pred, truth, input_norm=True):
        """Adds the B * T images of (pred, truth) -- shapes as `png_metrics`; batches may differ in B and T.  Two launches, no host
        read.  Returns the batch's PngMetrics."""
        pred, truth = _png_inputs(pred, truth)
        if pred.device != self._acc.device:
            raise ValueError(f"PngEvaluation: the accumulator is on {self._acc.device}, the frames on {pred.device}")
        return _png_launch(pred, truth, bool(input_norm), False, self._acc)

    def summary(self):
        """(avg_ssim, avg_mse, avg_psnr, number of images) from ONE host transfer."""
        import math
        host = self._acc.cpu()
        n = int(host[2])
        if n == 0:
            raise ValueError("PngEvaluation: no images yet")
        sums = host[:2].view(torch.float64)
        avg_ssim, avg_mse = float(sums[0]) / n, float(sums[1]) / n
        avg_psnr = math.inf if avg_mse == 0.0 else (10.0 * math.log10(1.0 / avg_mse) if avg_mse == avg_mse else math.nan)
        return avg_ssim, avg_mse, avg_psnr, n

    def result(self):
        """Upstream's `Evaluation` return values: (avg_ssim, avg_mse, avg_psnr)."""
        return self.summary()[:3]

    @property
    def n_images(self):
        """The image count so far (one host read)."""
        return int(self._acc[2])
