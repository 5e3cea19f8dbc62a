"""TEST INFRASTRUCTURE ONLY: CPU restatement of upstream Vid-ODE's evaluation protocol (Vid-ODE/tester.py:49-78,
visualize.save_test_images, evaluate.Evaluation): de-normalise, quantise to 8-bit RGB as torchvision's `save_image` does, PIL's
`convert('L')`, scikit-image's Gaussian SSIM at data_range 255 on the luma, the MSE of the bytes / 255, and the PSNR of the mean MSE.

Parity status.  The luma is pinned to Pillow's own output by tests/golden/png_metrics.npz (tests/test_png_metrics_cpu.py).  torchvision
and scikit-image are not installed offline: `save_image`'s quantisation line (`mul(255).add_(0.5).clamp_(0, 255).to(uint8)`,
torchvision/utils.py) and the SSIM (tests/_metrics_ref.py) are restated, "parity unpinned" (DESIGN.md section 2)."""
import math

import numpy as np
import torch

import _metrics_ref as mr


def quantise(x, input_norm):
    """float32 CPU tensor -> uint8 of the same shape, in torch float32 operations in upstream's order: utils.denorm ((x + 1) / 2,
    clamp_(0, 1)) when `input_norm`, then save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8).  A NaN gives 0 (the conversion
    of a NaN to uint8 is undefined; the kernel writes 0 and flags the image)."""
    assert x.dtype == torch.float32 and not x.is_cuda
    v = x.clone()
    if input_norm:
        v = (v + 1) / 2
        v = v.clamp_(0, 1)
    v = v.mul(255).add_(0.5).clamp_(0, 255)
    return torch.where(torch.isnan(x), torch.zeros_like(v), v).to(torch.uint8)


def rgb_bytes(x, input_norm):
    """(B, T, C, S, S) float32 -> (B, T, S, S, 3) uint8: the pixels of the PNG files save_image writes (one channel replicated)."""
    q = quantise(x, input_norm)
    if q.shape[2] == 1:
        q = q.expand(-1, -1, 3, -1, -1)
    return q.permute(0, 1, 3, 4, 2).contiguous()


def luma(rgb):
    """PIL's convert('L') of (..., 3) uint8: (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in integers."""
    v = np.asarray(rgb).astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def metrics_ref(pred, truth, input_norm):
    """float64 reference of `png_metrics`, from (B, T, C, S, S) float32 CPU tensors: dict of pred_bytes, truth_bytes (B, T, S, S, 3)
    uint8 tensors, sse (B, T) int64, mse and ssim (B, T) float64 arrays.  An image with a NaN: sse -1, mse and ssim NaN."""
    pb, tb = rgb_bytes(pred, input_norm), rgb_bytes(truth, input_norm)
    b, t, s = pb.shape[0], pb.shape[1], pb.shape[2]
    d = pb.numpy().astype(np.int64) - tb.numpy().astype(np.int64)
    sse = (d * d).sum(axis=(2, 3, 4))
    mse = sse.astype(np.float64) / (255.0 ** 2 * 3 * s * s)
    lp, lt = luma(pb.numpy()), luma(tb.numpy())
    ssim = np.empty((b, t))
    for i in range(b):
        for j in range(t):
            ssim[i, j] = mr.ssim_ref(lp[i, j], lt[i, j], 255.0, np.float64)
    bad = (torch.isnan(pred) | torch.isnan(truth)).flatten(2).any(dim=2).numpy()
    sse[bad], mse[bad], ssim[bad] = -1, np.nan, np.nan
    return {"pred_bytes": pb, "truth_bytes": tb, "sse": sse, "mse": mse, "ssim": ssim}


def evaluation_ref(per_image_ssim, per_image_mse):
    """Upstream's Evaluation: (mean ssim, mean mse, 10 log10(1 / mean mse)) over all images, float64."""
    ssim = float(np.mean(np.concatenate([np.ravel(v) for v in per_image_ssim])))
    mse = float(np.mean(np.concatenate([np.ravel(v) for v in per_image_mse])))
    return ssim, mse, (math.inf if mse == 0 else 10.0 * math.log10(1.0 / mse))


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------

def tie_values(input_norm):
    """float32 values around every rounding boundary of the quantisation, found by integer reasoning, not by running it: for each byte
    k the exact grid point (k / 255 in the space of v), the tie v * 255 + 0.5 == k + 1 and their neighbours one ulp either side, mapped
    back through the de-normalisation where it is on; plus values outside the range, signed zeros and infinities."""
    k = np.arange(0, 256, dtype=np.float64)
    centres = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(np.float32)
    v = np.concatenate([centres, np.nextafter(centres, np.float32(-np.inf)), np.nextafter(centres, np.float32(np.inf))])
    if input_norm:
        v = (v.astype(np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
        v = np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
    extra = np.array([-3.0, -1.0, -0.0, 0.0, 1.0, 1.0 + 2 ** -23, 2.5, 300.0, -1e30, 1e30, np.inf, -np.inf, 2 ** -149, -2 ** -149], dtype=np.float32)
    return torch.from_numpy(np.concatenate([v.astype(np.float32), extra]))


def byte_case(c, s, input_norm, seed, batch=2, n_frames=3):
    """(pred, truth) float32 (B, T, C, S, S): uniform values a little beyond the nominal range with the tie values scattered over both."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-1.2, 1.2) if input_norm else (-0.1, 1.1)
    out = []
    for _ in range(2):
        x = torch.rand((batch, n_frames, c, s, s), generator=g) * (hi - lo) + lo
        ties = tie_values(input_norm)
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:ties.numel()]
        flat[pos] = ties
        out.append(x)
    return out[0], out[1]


def smooth_bright_pair(s):
    """The cancellation case: a smooth bright pair (values 200 .. 255 of 255), where uxx - ux^2 is a small difference of numbers near
    65025.  (1, 1, 1, S, S) float32 in [0, 1] each."""
    y, x = np.mgrid[0:s, 0:s].astype(np.float64) / s
    a = (215.0 + 38.0 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y)) / 255.0
    b = (217.0 + 36.0 * np.sin(2.1 * x + 0.35) * np.cos(1.7 * y + 0.05)) / 255.0
    f = lambda v: torch.from_numpy(v.astype(np.float32)).view(1, 1, 1, s, s)     # noqa: E731
    return f(a), f(b)
