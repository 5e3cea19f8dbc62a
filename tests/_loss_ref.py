"""NumPy float64 restatements of the two training losses of csrc/frame_loss.hip and of their gradients, from the definitions in
include/odecgru_hip.h -- no torch, no reuse of the package's code.  Inputs are the fp32 arrays the device sees; everything is formed
in float64, so the results are the exact values up to float64 rounding (1e-16 relative per operation, nothing next to the fp32
bounds of the tests)."""
import numpy as np


def mse_kl(pred, truth, kl=None, kl_weight=1.0, latent_elems=None, grad_out=1.0):
    """pred (K * B, ...) sample-major against truth (B, ...).  Returns a dict: loss, mse, kl_term, grad_pred, grad_kl (None without kl)."""
    p, t = np.asarray(pred, np.float64), np.asarray(truth, np.float64)
    b = t.shape[0]
    k = p.shape[0] // b
    assert p.shape[0] == k * b and p.shape[1:] == t.shape[1:]
    diff = p.reshape((k, b) + t.shape[1:]) - t[None]            # row k * B + b against row b
    n = float(diff.size)
    mse = float(np.sum(diff * diff) / n)
    out = {"mse": mse, "kl_term": 0.0, "loss": mse, "grad_kl": None,
           "grad_pred": (diff * (2.0 * float(grad_out) / n)).reshape(p.shape)}
    if kl is not None:
        scale = 1.0 / (b * int(latent_elems))
        kw = float(np.float32(kl_weight))
        out["kl_term"] = float(np.sum(np.asarray(kl, np.float64)) * scale)
        out["loss"] = mse + kw * out["kl_term"]
        out["grad_kl"] = np.full(b, float(grad_out) * kw * scale)
    return out


def selected_frames(mask, n):
    """s[b][j]: the j-th t with mask[b][t] != 0, or None where row b selects fewer than n frames."""
    m = np.asarray(mask)
    m = m.reshape(m.shape[0], m.shape[1])
    rows = []
    for b in range(m.shape[0]):
        on = [t for t in range(m.shape[1]) if m[b, t] != 0]
        rows.append(on[:n] if len(on) >= n else None)
    return rows


def sgn(x):
    """What the backward of torch.abs multiplies by: 0 at 0 and at NaN, +-1 elsewhere (the infinities included)."""
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def vidode_l1(pred, inter, truth, init, mask, grad_out=1.0):
    """pred, inter (B, n, ...), truth (B, T, ...), init (B, ...), mask (B, T[, 1]).  Returns a dict: loss, l1_pred, l1_diff,
    grad_pred, grad_inter.  A row with fewer than n selected frames: the three scalars are NaN."""
    p, x = np.asarray(pred, np.float64), np.asarray(inter, np.float64)
    t, i0 = np.asarray(truth, np.float64), np.asarray(init, np.float64)
    b, n = p.shape[0], p.shape[1]
    sel = selected_frames(mask, n)
    if any(r is None for r in sel):
        nan = float("nan")
        return {"loss": nan, "l1_pred": nan, "l1_diff": nan, "grad_pred": None, "grad_inter": None}
    prev = np.concatenate([i0[:, None], t[:, :-1]], axis=1)      # the frame before frame t; init before frame 0
    d = t - prev
    t_sel = np.stack([t[r, sel[r]] for r in range(b)])
    d_sel = np.stack([d[r, sel[r]] for r in range(b)])
    count = float(p.size)
    dp, dx = p - t_sel, x - d_sel
    with np.errstate(invalid="ignore"):
        l1_pred, l1_diff = float(np.sum(np.abs(dp)) / count), float(np.sum(np.abs(dx)) / count)
    return {"loss": l1_pred + l1_diff, "l1_pred": l1_pred, "l1_diff": l1_diff,
            "grad_pred": sgn(dp) * (float(grad_out) / count), "grad_inter": sgn(dx) * (float(grad_out) / count)}
