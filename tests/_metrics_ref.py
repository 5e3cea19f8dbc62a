"""TEST INFRASTRUCTURE ONLY: CPU restatement of the reference's evaluation metrics (train_test.py:104-117,
helpers/utils.py:254-271) -- scikit-image's `structural_similarity(x, y, data_range=R, gaussian_weights=True,
use_sample_covariance=False)` for a 2-D float image, and the per-frame MSE / PSNR around it.

Parity status: scikit-image is not installed offline, so no fixture could be recorded from the reference's own
`get_normalized_ssim` -- "parity unpinned", restated faithfully.  `ssim_ref` makes exactly the scipy call
scikit-image makes (`gaussian_filter(sigma=1.5, truncate=3.5, mode='reflect')`); `ssim_direct` is an independent form without scipy
(an explicit 11 x 11 window per interior pixel) that pins the restatement on the CPU.  Also here: the frames the metric tests run
on (rendered Moving-MNIST truth, four degradations of it as predictions)."""
import numpy as np

SIGMA, TRUNCATE = 1.5, 3.5
RADIUS = int(TRUNCATE * SIGMA + 0.5)          # 5: scipy's gaussian_filter1d
CROP = (2 * RADIUS + 1 - 1) // 2              # 5: scikit-image crops (win_size - 1) // 2 before the mean
K1, K2 = 0.01, 0.03


def ssim_ref(x, y, R, dtype=np.float64):
    """SSIM of two (H, W) images as scikit-image computes it; the arithmetic runs in `dtype`, the final mean in float64."""
    from scipy import ndimage
    x = np.asarray(x).astype(dtype)
    y = np.asarray(y).astype(dtype)

    def filt(a):
        return ndimage.gaussian_filter(a, sigma=SIGMA, truncate=TRUNCATE, mode="reflect")

    ux, uy = filt(x), filt(y)
    uxx, uyy, uxy = filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
    a1, a2, b1, b2 = 2 * ux * uy + c1, 2 * vxy + c2, ux ** 2 + uy ** 2 + c1, vx + vy + c2
    s = (a1 * a2) / (b1 * b2)
    return float(s[CROP:-CROP, CROP:-CROP].mean(dtype=np.float64))


def ssim_direct(x, y, R):
    """The same quantity from the definition, float64, no scipy: for every interior pixel the 11 x 11 Gaussian-weighted moments of
    its window (which never leaves the image: no border case arises)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w1 = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    w1 /= w1.sum()
    w2 = np.outer(w1, w1)
    c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
    h, w = x.shape
    total, count = 0.0, 0
    for i in range(RADIUS, h - RADIUS):
        for j in range(RADIUS, w - RADIUS):
            px = x[i - RADIUS:i + RADIUS + 1, j - RADIUS:j + RADIUS + 1]
            py = y[i - RADIUS:i + RADIUS + 1, j - RADIUS:j + RADIUS + 1]
            ux, uy = float((w2 * px).sum()), float((w2 * py).sum())
            vx = float((w2 * px * px).sum()) - ux * ux
            vy = float((w2 * py * py).sum()) - uy * uy
            vxy = float((w2 * px * py).sum()) - ux * uy
            total += ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
            count += 1
    return total / count


def metrics_ref(pred, truth, R):
    """float64 reference of everything `frame_metrics` returns, from (B, T, C, H, W) arrays: dict of sse (B, T), ssim_per_sample
    (B, T; mean over the channels of ssim_ref), mse, psnr, ssim (T,).  psnr is +inf where mse is 0."""
    pred = np.asarray(pred, dtype=np.float64)
    truth = np.asarray(truth, dtype=np.float64)
    b, t, c, h, w = pred.shape
    sse = ((pred - truth) ** 2).sum(axis=(2, 3, 4))
    ssim = np.empty((b, t))
    for i in range(b):
        for j in range(t):
            ssim[i, j] = np.mean([ssim_ref(pred[i, j, k], truth[i, j, k], R) for k in range(c)])
    mse = sse.sum(axis=0) / (b * c * h * w)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(R * R / mse)
    return {"sse": sse, "ssim_per_sample": ssim, "mse": mse, "psnr": psnr, "ssim": ssim.mean(axis=0)}


DEGRADATIONS = ("noise", "blur", "constant", "shift_scale")


def degrade(x, kind, rng):
    """A prediction for the (H, W) truth frame x in [0, 1]: Gaussian noise (sigma 0.1, clipped to [0, 1]); blur (sigma 2); the
    constant frame at the truth's mean; shifted 3 px along the columns and scaled by 0.8.  float32."""
    from scipy import ndimage
    if kind == "noise":
        p = np.clip(x + rng.normal(0.0, 0.1, x.shape), 0.0, 1.0)
    elif kind == "blur":
        p = ndimage.gaussian_filter(x.astype(np.float64), 2.0)
    elif kind == "constant":
        p = np.full_like(x, x.mean())
    elif kind == "shift_scale":
        p = np.roll(x, 3, axis=1) * 0.8
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def make_frames(batch, n_frames, channels, seed=0):
    """(pred, truth): float32 (B, T, C, 64, 64) in [0, 1].  truth: frames of the oracle's Moving-MNIST renderer on the package's
    procedural glyphs (two digits per sample; the channels of a sample are independent walks); pred: the truth degraded, the kind
    cycling with b + t + c so that every frame mean over the batch mixes kinds."""
    from oracle import moving_mnist_ref as mm
    from ode_rl_amd import data
    glyphs = data.synthetic_digit_glyphs()
    rng = np.random.default_rng(seed)
    truth = np.empty((batch, n_frames, channels, 64, 64), dtype=np.float32)
    pred = np.empty_like(truth)
    for b in range(batch):
        for c in range(channels):
            ids = rng.integers(0, 10, size=2)
            _, frames = mm.render(glyphs, ids, rng.random(2), rng.random(2), rng.random(2) * 2 * np.pi, 0, n_frames)
            truth[b, :, c] = frames[:, 0] + np.float32(0.5)
            for t in range(n_frames):
                pred[b, t, c] = degrade(truth[b, t, c], DEGRADATIONS[(b + t + c) % 4], rng)
    return pred, truth
