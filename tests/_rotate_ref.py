"""Upstream Vid-ODE's `RandomRotation` item transform restated in NumPy on the CPU, as DESIGN.md section 4.18 states it (scikit-image's
`rotate(frame, angle, preserve_range=True)`: bilinear, constant 0 outside the frame, values clipped from below to the frame's own
minimum), followed by upstream's `ToTensor(scale=True)`, `Normalize(0.5, 0.5)` and the mask multiply in torch's float32.  `dtype`
selects the precision of the coordinates and of the interpolation: float64 is the reference, float32 the same formula with every
operation rounded to float32, whose distance from the reference sizes the bound of the GPU tests.  tests/test_vidode_rotate_cpu.py
pins the float64 form to scipy.ndimage.map_coordinates.  Nothing here imports the code under test.
"""
import math

import numpy as np
import torch


def cos_sin(angle, dtype=np.float64):
    """cos and sin of an angle in degrees: deg2rad in float64 (x * (pi / 180)), then rounded to `dtype` before the functions."""
    a = math.radians(float(angle))
    if dtype == np.float64:
        return np.float64(math.cos(a)), np.float64(math.sin(a))
    a = dtype(a)
    return np.cos(a).astype(dtype), np.sin(a).astype(dtype)


def source_coordinates(height, width, angle, dtype=np.float64):
    """(sy, sx), each (H, W): where output pixel (y, x) reads the frame."""
    ca, sa = cos_sin(angle, dtype)
    cx, cy = dtype(width / 2 - 0.5), dtype(height / 2 - 0.5)
    ys, xs = np.mgrid[0:height, 0:width].astype(dtype)
    rx, ry = xs - cx, ys - cy
    return sa * rx + ca * ry + cy, ca * rx - sa * ry + cx


def rotate(frame, angle, dtype=np.float64):
    """frame (H, W, C) uint8 -> (H, W, C) `dtype` in byte units (0..255)."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    sy, sx = source_coordinates(h, w, angle, dtype)
    x0, x1, y0, y1 = np.floor(sx), np.ceil(sx), np.floor(sy), np.ceil(sy)
    dx, dy = (sx - x0)[..., None], (sy - y0)[..., None]

    def p(yy, xx):
        inside = (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        yi, xi = np.clip(yy, 0, h - 1).astype(np.int64), np.clip(xx, 0, w - 1).astype(np.int64)
        return np.where(inside[..., None], frame[yi, xi], 0).astype(dtype)

    one = dtype(1)
    top = (one - dx) * p(y0, x0) + dx * p(y0, x1)
    bottom = (one - dx) * p(y1, x0) + dx * p(y1, x1)
    v = (one - dy) * top + dy * bottom
    m = dtype(frame.min())
    if m > 0:
        v = np.where(v != 0, np.maximum(v, m), v)
    assert v.dtype == dtype
    return v


def to_tensor(values, input_norm):
    """(..., H, W, C) byte-unit values -> (..., C, H, W) float32: `.float().div(255)` and Normalize's `.sub_(mean).div_(std)`."""
    video = torch.from_numpy(np.ascontiguousarray(np.moveaxis(values, -1, -3))).float().div(255)
    if input_norm:
        video = video.sub_(torch.FloatTensor([0.5]).view(1, 1, 1)).div_(torch.FloatTensor([0.5]).view(1, 1, 1))
    return video


def batch(store, frames, factor, flip, angle, input_norm, dtype=np.float64):
    """What one output of the rotated launch holds: store (N, H, W, C) uint8; frames, factor (B, T); flip, angle (B,) -> (B, T, C, H, W)
    float32.  A frame index outside the store gives NaN."""
    n, h, w, c = store.shape
    out = torch.full((frames.shape[0], frames.shape[1], c, h, w), float("nan"))
    for b in range(frames.shape[0]):
        for t in range(frames.shape[1]):
            if 0 <= frames[b, t] < n:
                px = store[frames[b, t]]
                px = px[:, ::-1] if flip[b] else px
                out[b, t] = to_tensor(rotate(px, angle[b], dtype), input_norm) * torch.tensor(factor[b, t], dtype=torch.float32)
    return out
