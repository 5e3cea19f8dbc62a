"""Upstream Vid-ODE's evaluation protocol on the device (csrc/png_metrics.hip through `ode_rl_amd.png_metrics`, `PngEvaluation` and
`train.evaluate_vidode`) against the CPU restatement of tests/_png_metrics_ref.py.  B = 2, T = 3 throughout.

Tolerances (fixed before the kernel ran on a GPU):
  bytes, sse   torch.equal: the quantisation is upstream's chain of single float32 operations, the squared error an integer.
  mse          1e-15 relative: one float64 division of an exact integer.
  ssim[b,t]    absolute 1e-9 against the float64 restatement.  float64 moments carry at most about 30 roundings of 2^-53 on magnitudes
               <= 65025, about 2e-10 absolute on a variance; the denominators are at least C2 = 58.5 and C1 = 6.5, so S is good to about
               1e-11; 1e-9 leaves two orders of margin and still rejects float32 moments (2.4e-6 in the image mean of the smooth bright
               pair).
  accumulator  1e-12 against float64 means of the same per-image values.
The worst observed SSIM error goes to conftest.record("png_ssim_abs_err", ...)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import _metrics_ref as mr
import _png_metrics_ref as ref
from conftest import record

pytestmark = pytest.mark.gpu

B, T = 2, 3
SSIM_ATOL = 1e-9
MSE_RTOL = 1e-15
ACC_TOL = 1e-12


def _call(cuda, pred, truth, **kw):
    import ode_rl_amd
    return ode_rl_amd.png_metrics(pred.to(cuda), truth.to(cuda), **kw)


def _check(m, r, what, with_bytes=True):
    """Every output of one call against the restatement; returns the worst SSIM error."""
    assert m.ssim.shape == m.mse.shape == m.sse.shape == r["sse"].shape
    assert m.ssim.dtype == torch.float64 and m.mse.dtype == torch.float64 and m.sse.dtype == torch.int64
    assert all(v is None or (v.is_cuda and not v.requires_grad) for v in m)
    if with_bytes:
        assert m.pred_bytes.dtype == torch.uint8 and m.pred_bytes.shape == r["pred_bytes"].shape
        assert torch.equal(m.pred_bytes.cpu(), r["pred_bytes"]), what
        assert torch.equal(m.truth_bytes.cpu(), r["truth_bytes"]), what
    assert torch.equal(m.sse.cpu(), torch.from_numpy(r["sse"])), what
    mse, ssim = m.mse.cpu().numpy(), m.ssim.cpu().numpy()
    mse_rel = np.abs(mse - r["mse"]) / np.maximum(r["mse"], 1e-300)
    err = np.abs(ssim - r["ssim"])
    print(f"{what}: ssim err {err.max():.3e} (ssim {r['ssim'].min():.4f} .. {r['ssim'].max():.4f})  mse rel {mse_rel.max():.3e}")
    record("png_ssim_abs_err", float(err.max()))
    assert np.isfinite(mse_rel).all() and mse_rel.max() <= MSE_RTOL, (what, mse_rel.max())
    assert np.isfinite(err).all() and err.max() <= SSIM_ATOL, (what, err.max())
    return float(err.max())


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("input_norm", [True, False])
@pytest.mark.parametrize("S", [32, 64, 128])
@pytest.mark.parametrize("C", [1, 3])
def test_bytes_and_squared_error_are_exact(cuda, C, S, input_norm):
    """Values beyond the range on both sides, every exact tie of v * 255 + 0.5 and the neighbours of the ties one ulp either side."""
    pred, truth = ref.byte_case(C, S, input_norm, seed=1000 + 10 * S + C + (5 if input_norm else 0), batch=B, n_frames=T)
    m = _call(cuda, pred, truth, input_norm=input_norm, return_bytes=True)
    r = ref.metrics_ref(pred, truth, input_norm)
    assert len(np.unique(r["pred_bytes"].numpy())) == 256
    _check(m, r, f"bytes C={C} S={S} input_norm={input_norm}")
    plain = _call(cuda, pred, truth, input_norm=input_norm)
    assert plain.pred_bytes is None and plain.truth_bytes is None
    for name in ("ssim", "mse", "sse"):      # the byte outputs change nothing else
        assert torch.equal(getattr(plain, name), getattr(m, name)), name


# ---- SSIM ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ssim_case(C, S):
    """(pred, truth, reference) in [0, 1], input_norm off: rendered frames with the four degradations of tests/_metrics_ref.py (cropped
    to 32 or tiled to 128), image (0, 0) replaced by the smooth bright pair, image (1, 2) by a flat 255 frame against a flat 254."""
    pred, truth = mr.make_frames(B, T, C, seed=300 + C + S)
    if S == 32:
        pred, truth = pred[..., 16:48, 16:48], truth[..., 16:48, 16:48]
    elif S == 128:
        pred, truth = np.tile(pred, (1, 1, 1, 2, 2)), np.tile(truth, (1, 1, 1, 2, 2))
    pred, truth = torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(truth))
    a, b = ref.smooth_bright_pair(S)
    for c in range(C):
        pred[0, 0, c], truth[0, 0, c] = torch.roll(a[0, 0, 0], 3 * c, 1), torch.roll(b[0, 0, 0], 3 * c, 1)
    pred[1, 2], truth[1, 2] = 1.0, float(np.float32(254.0 / 255.0))
    return pred, truth, ref.metrics_ref(pred, truth, False)


@pytest.mark.parametrize("S", [32, 64, 128])
@pytest.mark.parametrize("C", [1, 3])
def test_ssim_matches_the_float64_restatement(cuda, C, S):
    pred, truth, r = _ssim_case(C, S)
    assert r["sse"][1, 2] == 3 * S * S and 0.99 < r["ssim"][1, 2] < 1.0          # flat 255 against flat 254
    assert r["ssim"].min() < 0.5                                                  # and degraded frames far from 1
    worst = _check(_call(cuda, pred, truth, input_norm=False, return_bytes=True), r, f"ssim C={C} S={S}")
    record(f"png_ssim_abs_err_C{C}_S{S}", worst)


def test_ssim_through_the_denormalisation(cuda):
    pred, truth, r = _ssim_case(3, 64)
    p, x = pred * 2 - 1, truth * 2 - 1          # [-1, 1] frames: input_norm on (the bytes may differ by the rounding of the round trip)
    _check(_call(cuda, p, x, input_norm=True, return_bytes=True), ref.metrics_ref(p, x, True), "ssim C=3 S=64 input_norm")


# ---- identities -------------------------------------------------------------------------------------------------------------------------

def test_identical_inputs(cuda):
    import ode_rl_amd
    pred, _, _ = _ssim_case(3, 64)
    x = pred.to(cuda)
    m = ode_rl_amd.png_metrics(x, x.clone(), input_norm=False)
    assert torch.equal(m.ssim, torch.ones_like(m.ssim)) and torch.equal(m.mse, torch.zeros_like(m.mse)) and int(m.sse.abs().sum()) == 0
    ev = ode_rl_amd.PngEvaluation(cuda)
    ev.update(x, x.clone(), input_norm=False)
    assert ev.result() == (1.0, 0.0, math.inf)


@pytest.mark.parametrize("S", [32, 128])
def test_one_channel_is_the_replicated_three(cuda, S):
    pred, truth, _ = _ssim_case(1, S)
    one = _call(cuda, pred, truth, input_norm=False, return_bytes=True)
    three = _call(cuda, pred.expand(-1, -1, 3, -1, -1), truth.expand(-1, -1, 3, -1, -1), input_norm=False, return_bytes=True)
    for u, v in zip(one, three):
        assert torch.equal(u, v)


def test_deterministic_and_contiguity_independent(cuda):
    import ode_rl_amd
    pred, truth, _ = _ssim_case(3, 64)
    p, x = pred.to(cuda), truth.to(cuda)
    first = ode_rl_amd.png_metrics(p, x, input_norm=False, return_bytes=True)
    again = ode_rl_amd.png_metrics(p, x, input_norm=False, return_bytes=True)
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    p_perm = p.permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4)       # time-first storage
    wide = torch.zeros(B, T, 3, 64, 70, device=cuda)
    wide[..., 3:67] = x
    x_sliced = wide[..., 3:67]                                                   # a slice of a wider buffer, 4-byte aligned only
    assert not p_perm.is_contiguous() and not x_sliced.is_contiguous()
    for u, v in zip(first, ode_rl_amd.png_metrics(p_perm, x_sliced, input_norm=False, return_bytes=True)):
        assert torch.equal(u, v)
    flat = torch.zeros(p.numel() + 1, device=cuda)                               # contiguous, but not 16-byte aligned
    flat[1:] = p.reshape(-1)
    for u, v in zip(first, ode_rl_amd.png_metrics(flat[1:].view_as(p), x, input_norm=False, return_bytes=True)):
        assert torch.equal(u, v)
    out = ode_rl_amd.png_metrics(p.clone().requires_grad_(True), x, input_norm=False)
    assert not any(v is not None and v.requires_grad for v in out) and torch.equal(out.ssim, first.ssim)


# ---- NaN ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,S", [(1, 64), (3, 128)])
def test_nan_reaches_its_image_and_no_other(cuda, C, S):
    import ode_rl_amd
    pred, truth, _ = _ssim_case(C, S)
    p, x = pred.to(cuda), truth.to(cuda)
    clean = ode_rl_amd.png_metrics(p, x, input_norm=False, return_bytes=True)
    hit = torch.zeros(B, T, dtype=torch.bool, device=cuda)
    hit[1, 2] = True
    for which, pixel in (("pred", (0, 0)), ("pred", (S - 1, S - 1)), ("truth", (S // 2, 17))):
        q, y = p.clone(), x.clone()
        (q if which == "pred" else y)[1, 2, C - 1, pixel[0], pixel[1]] = float("nan")
        m = ode_rl_amd.png_metrics(q, y, input_norm=False, return_bytes=True)
        for name in ("ssim", "mse"):
            got, want = getattr(m, name), getattr(clean, name)
            assert torch.equal(torch.isnan(got), hit), (name, which, pixel)
            assert torch.equal(got[~hit], want[~hit]), (name, which, pixel)
        assert int(m.sse[1, 2]) == -1 and torch.equal(m.sse[~hit], clean.sse[~hit])
        nan_bytes = m.pred_bytes if which == "pred" else m.truth_bytes
        assert int(nan_bytes[1, 2, pixel[0], pixel[1], C - 1]) == 0
        assert torch.equal(m.pred_bytes[~hit], clean.pred_bytes[~hit]) and torch.equal(m.truth_bytes[~hit], clean.truth_bytes[~hit])
        ev = ode_rl_amd.PngEvaluation(cuda)      # not laundered by the accumulator either
        ev.update(q, y, input_norm=False)
        assert all(math.isnan(v) for v in ev.result())


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------

def test_accumulator_over_unequal_batches(cuda):
    """Batches of 2, 1 and 2 samples (the last with 2 frames instead of 3) under torch's synchronisation check: no update reads the
    device.  avg_psnr is the PSNR of the mean MSE, which on these frames is not the mean of the per-image PSNRs."""
    import ode_rl_amd
    pred, truth, r = _ssim_case(3, 64)
    parts = [(slice(0, 2), slice(0, 3)), (slice(1, 2), slice(0, 3)), (slice(0, 2), slice(1, 3))]
    p, x = pred.to(cuda), truth.to(cuda)
    batches = [(p[b, t].contiguous(), x[b, t].contiguous()) for b, t in parts]
    ev = ode_rl_amd.PngEvaluation(cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pb, xb in batches:
            m = ev.update(pb, xb, input_norm=False)
            assert m.ssim.shape == pb.shape[:2]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ev.result()
    ssim_parts, mse_parts = [r["ssim"][b, t] for b, t in parts], [r["mse"][b, t] for b, t in parts]
    want = ref.evaluation_ref(ssim_parts, mse_parts)
    n = sum(v.size for v in ssim_parts)
    assert ev.n_images == n == 6 + 3 + 4
    print("accumulator:", got, want)
    for g, w in zip(got, want):
        assert abs(g - w) <= ACC_TOL * max(1.0, abs(w)), (got, want)
    all_mse = np.concatenate([np.ravel(v) for v in mse_parts])
    mean_of_psnrs = float(np.mean(10.0 * np.log10(1.0 / all_mse)))
    assert abs(got[2] - mean_of_psnrs) > 0.1, (got[2], mean_of_psnrs)
    # the sums do not depend on the split: one update with everything in the same order gives the same bits
    one = ode_rl_amd.PngEvaluation(cuda)
    one.update(p, x, input_norm=False)
    two = ode_rl_amd.PngEvaluation(cuda)
    two.update(p[:1], x[:1], input_norm=False)
    two.update(p[1:], x[1:], input_norm=False)
    assert one.result() == two.result()


# ---- evaluate_vidode ------------------------------------------------------------------------------------------------------------------------

def _vidode_opt(extrap):
    import _vidode_upstream_ref as up
    opt = up.model_opt(extrap)
    # init_dim 16: the smallest the HIP convolutions take (the ODE functions' hidden width 2 * init_dim must be a multiple of 32)
    opt.init_dim, opt.input_norm, opt.dataset = 16, True, "kth"
    opt.window_size, opt.sample_size, opt.batch_size, opt.phase = 6, 6, 2, "test"
    return opt


def _clips():
    rng = np.random.default_rng(77)
    y, x = np.mgrid[0:64, 0:64]
    clips = []
    for n, length in enumerate((6, 8, 7)):
        frames = [np.clip(128 + 100 * np.sin(0.11 * (x + 3 * t + 5 * n)) * np.cos(0.09 * (y - 2 * t)) + rng.normal(0, 8, (64, 64)), 0, 255) for t in range(length)]
        clips.append(np.stack(frames).astype(np.uint8))
    return clips


@pytest.mark.parametrize("extrap", [True, False])
def test_evaluate_vidode_against_the_restatement(cuda, extrap):
    import ode_rl_amd
    from ode_rl_amd import train, vidode_data
    from ode_rl_amd.models import conv_odegru
    opt = _vidode_opt(extrap)
    torch.manual_seed(5)
    model = conv_odegru.VidODE(opt, cuda).train()
    store = vidode_data.ClipStore(_clips(), device=cuda)
    seen = []
    inner = model.get_reconstruction

    def recording(**kw):
        out = inner(**kw)
        seen.append(out[0].detach().cpu())
        return out

    model.get_reconstruction = recording
    res = train.evaluate_vidode(model, vidode_data.VidODEBatches(opt, store, train=False), opt, n_batches=2)
    assert model.training, "evaluate_vidode must put the model back into training mode"
    # the same batches again, scored by the restatement on the recorded reconstructions
    ssims, mses = [], []
    for preds, data_dict in zip(seen, vidode_data.VidODEBatches(opt, store, train=False)):
        bd = vidode_data.get_next_batch(data_dict, test_interp=not extrap)
        truth = bd["data_to_predict"].cpu()
        mask = bd["mask_predicted_data"]
        b, _, c, h, w = truth.shape
        truth = truth[mask.reshape(b, -1).bool()].view(b, int(mask[0].sum()), c, h, w)       # tester.py:65-67
        assert preds.shape == truth.shape and preds.shape[1] == (3 if extrap else 2)
        r = ref.metrics_ref(preds, truth, True)
        ssims.append(r["ssim"])
        mses.append(r["mse"])
    assert [s.shape[0] for s in ssims] == [2, 1]
    want = ref.evaluation_ref(ssims, mses)
    print("evaluate_vidode:", res, want)
    assert res["n_images"] == sum(s.size for s in ssims)
    for k, w in zip(("ssim", "mse", "psnr"), want):
        assert abs(res[k] - w) <= ACC_TOL * max(1.0, abs(w)), (k, res[k], w)
    assert 0.0 < res["mse"] < 1.0 and res["ssim"] < 1.0

    def broken():
        yield next(iter(vidode_data.VidODEBatches(opt, store, train=False)))
        yield {"mode": "test"}

    with pytest.raises(KeyError):
        train.evaluate_vidode(model, broken(), opt)
    assert model.training
    model.eval()
    train.evaluate_vidode(model, vidode_data.VidODEBatches(opt, store, train=False), opt, n_batches=1)
    assert not model.training


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_through_python(cuda):
    import ode_rl_amd
    z = lambda *s, **kw: torch.zeros(*s, device=cuda, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="48 x 48"):
        ode_rl_amd.png_metrics(z(B, T, 1, 48, 48), z(B, T, 1, 48, 48))
    with pytest.raises(ValueError, match="channels 2"):
        ode_rl_amd.png_metrics(z(B, T, 2, 64, 64), z(B, T, 2, 64, 64))
    with pytest.raises(ValueError, match="64 x 32"):
        ode_rl_amd.png_metrics(z(B, T, 1, 64, 32), z(B, T, 1, 64, 32))
    with pytest.raises(ValueError, match="must both be"):
        ode_rl_amd.png_metrics(z(B, T, 1, 64, 64), z(B, T + 1, 1, 64, 64))
    with pytest.raises(ValueError, match="must both be"):
        ode_rl_amd.png_metrics(z(T, 1, 64, 64), z(T, 1, 64, 64))
    with pytest.raises(TypeError, match="float32"):
        ode_rl_amd.png_metrics(z(B, T, 1, 64, 64, dtype=torch.float64), z(B, T, 1, 64, 64, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ode_rl_amd.png_metrics(torch.zeros(B, T, 1, 64, 64), z(B, T, 1, 64, 64))
    ev = ode_rl_amd.PngEvaluation(cuda)
    with pytest.raises(ValueError, match="48 x 48"):
        ev.update(z(B, T, 1, 48, 48), z(B, T, 1, 48, 48))
    with pytest.raises(ValueError, match="no images"):
        ev.result()
