"""z0 sampled on the device (csrc/latent_sample.hip through `hip_ops.latent_sample`, `ode_rl_amd.sample_z0`
and `opt.z_sample` of models/ODEConvGRU.py) against float64 restatements: the noise stream against tests/_philox_ref.py, z0 and the
KL term against float64 torch, the backward against float64 autograd, the model against the oracle pipeline of
tests/test_hip_train_end_to_end.py extended by the sampled z0 and the KL term.

Bounds.  NOISE_ABS_BOUND: the device evaluates the documented mapping with fp32 logf / sqrtf / sincospif, the restatement in
float64; the bound is 4 x the largest absolute difference observed over the three cases below on an MI355X (4.59e-7, i.e. about
one fp32 rounding, 2^-22 = 2.4e-7, of a normal in the tails, twice over; recorded as `noise_max_abs_err`).  z0: one fp32 rounding of
the result (the kernel uses one fma).  KL: 4 x the error of the fp32 torch composition against float64 on the same inputs (both
recorded).  Gradients: rel-L2 <= 1e-5, the level the elementwise kernel-versus-torch tests of this suite hold.  Model: the bounds
of tests/test_hip_train_end_to_end.py (pred 1e-4, loss 1e-5 relative, gradients 1e-3)."""
import argparse
import copy

import numpy as np
import pytest
import torch

import _philox_ref as pr
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 0
NOISE_ABS_BOUND = 4 * 4.59e-7


def _inputs(b, c, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(b, c, 16, 16, generator=g)
    std = torch.rand(b, c, 16, 16, generator=g) * 1.5 + 0.25
    return mean.to(cuda), std.to(cuda)


def _draw(mean, std, k=1, seed=SEED, offset=OFFSET, **kw):
    from ode_rl_amd import hip_ops
    return hip_ops.latent_sample(mean, std, k, seed, offset, want_eps=True, **kw)


# ---- 1. the noise stream ---------------------------------------------------------------------------------------------------------

def test_noise_agrees_with_the_restatement(cuda):
    worst = 0.0
    for b, c, k, boff, gb in ((2, 64, 1, 0, 2), (3, 128, 3, 0, 3), (2, 64, 2, 3, 7)):
        mean, std = _inputs(b, c, 1, cuda)
        _, _, eps = _draw(mean, std, k, offset=5, batch_offset=boff, global_batch=gb)
        ref = pr.noise(k, b, c, SEED, 5, batch_offset=boff, global_batch=gb)
        err = float(np.abs(eps.cpu().numpy().astype(np.float64) - ref).max())
        print(f"noise (B, C, K, batch_offset) = ({b}, {c}, {k}, {boff}): max abs error {err:.3e}")
        worst = max(worst, err)
    record("noise_max_abs_err", worst)
    assert worst <= NOISE_ABS_BOUND, worst


def test_device_stream_moments(cuda):
    mean, std = _inputs(64, 64, 2, cuda)
    _, _, eps = _draw(mean, std)                                  # seed 1234, offset 0: 2^20 normals
    r = pr.check_moments(eps.cpu().numpy())
    for key in ("mean_se", "var_se", "m4_se", "max_abs"):
        record("device_stream_" + key, r[key])


# ---- 2. shards, repeatability, the offset -----------------------------------------------------------------------------------------

def test_a_shard_draws_the_rows_of_the_full_draw(cuda):
    B, C, K, b0, b1 = 5, 64, 3, 1, 4
    mean, std = _inputs(B, C, 3, cuda)
    z, kl, eps = _draw(mean, std, K)
    zs, kls, epss = _draw(mean[b0:b1], std[b0:b1], K, batch_offset=b0, global_batch=B)
    for k in range(K):
        assert torch.equal(epss.view(K, b1 - b0, C, 16, 16)[k], eps.view(K, B, C, 16, 16)[k, b0:b1])
        assert torch.equal(zs.view(K, b1 - b0, C, 16, 16)[k], z.view(K, B, C, 16, 16)[k, b0:b1])
    assert torch.equal(kls, kl[b0:b1])
    z2, kl2, _ = _draw(mean, std, K)                              # same seed and offset
    assert torch.equal(z2, z) and torch.equal(kl2, kl)
    assert not torch.equal(_draw(mean, std, K, offset=OFFSET + 1)[0], z)
    assert not torch.equal(_draw(mean, std, K, seed=SEED + 1)[0], z)
    rows = eps.view(K * B, -1)                                    # no two rows share their noise
    assert len({float(r[0]) for r in rows}) == K * B


def test_sample_z0_sequence_follows_the_generator(cuda):
    import ode_rl_amd
    import ode_rl_amd.dist as od
    mean, std = _inputs(4, 64, 4, cuda)
    torch.manual_seed(77)
    a1, _ = ode_rl_amd.sample_z0(mean, std)
    n1 = ode_rl_amd.last_z0_noise()
    a2, _ = ode_rl_amd.sample_z0(mean, std)
    assert not torch.equal(a1, a2)                                # consecutive calls differ
    torch.manual_seed(77)
    b1, _ = ode_rl_amd.sample_z0(mean, std)
    b2, _ = ode_rl_amd.sample_z0(mean, std)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)            # the same seed twice: the same sequence twice
    torch.manual_seed(78)
    assert not torch.equal(ode_rl_amd.sample_z0(mean, std)[0], a1)
    # the generator's seed and first offset are the stream's, and last_z0_noise() regenerates exactly that draw
    z_direct, _, eps_direct = _draw(mean, std, 1, seed=77, offset=0)
    assert torch.equal(a1, z_direct) and torch.equal(n1, eps_direct)
    assert torch.equal(a2, _draw(mean, std, 1, seed=77, offset=1)[0])
    # an explicit seed counts its own calls and restarts when it changes
    c1, _ = ode_rl_amd.sample_z0(mean, std, seed=5)
    c2, _ = ode_rl_amd.sample_z0(mean, std, seed=5)
    ode_rl_amd.sample_z0(mean, std, seed=6)
    c3, _ = ode_rl_amd.sample_z0(mean, std, seed=5)
    assert not torch.equal(c1, c2) and torch.equal(c1, c3) and torch.equal(c1, _draw(mean, std, 1, seed=5, offset=0)[0])
    # the caller's own noise
    e = torch.randn(8, 64, 16, 16, device=cuda)
    d, _ = ode_rl_amd.sample_z0(mean, std, n_samples=2, eps=e)
    assert ode_rl_amd.last_z0_noise() is not None and torch.equal(ode_rl_amd.last_z0_noise(), e)
    want = torch.addcmul(mean.repeat(2, 1, 1, 1).double(), std.repeat(2, 1, 1, 1).double(), e.double())
    assert float(((d.double() - want).abs() - 2.0 ** -23 * want.abs()).max()) <= 0.0
    # under batch sharding a rank draws the rows the full batch would have drawn
    torch.manual_seed(77)
    full, klf = ode_rl_amd.sample_z0(mean, std, n_samples=2)
    try:
        lo, gb = od.set_noise_shard(4, rank=1, world=2)
        torch.manual_seed(77)
        part, klp = ode_rl_amd.sample_z0(mean[lo:], std[lo:], n_samples=2)
    finally:
        od.clear_noise_shard()
    assert (lo, gb) == (2, 4) and torch.equal(part.view(2, 2, -1), full.view(2, 4, -1)[:, 2:]) and torch.equal(klp, klf[2:])
    with pytest.raises(TypeError):
        ode_rl_amd.sample_z0(mean.double(), std.double())
    for bad in (mean[:, :, :8], mean[:, :6], mean[0]):
        with pytest.raises(ValueError):
            ode_rl_amd.sample_z0(bad, bad)
    with pytest.raises(ValueError):
        ode_rl_amd.sample_z0(mean, std[:2])


# ---- 3. forward --------------------------------------------------------------------------------------------------------------------

def _kl64(mean, std):
    n = torch.distributions.Normal
    return torch.distributions.kl_divergence(n(mean.double(), std.double()), n(torch.zeros_like(mean).double(), torch.ones_like(std).double())).sum((1, 2, 3))


@pytest.mark.parametrize("b,c,k", [(8, 64, 1), (3, 128, 3)])
def test_forward_against_float64(cuda, b, c, k):
    mean, std = _inputs(b, c, 5, cuda)
    z, kl, eps = _draw(mean, std, k)
    ref = mean.double().repeat(k, 1, 1, 1) + std.double().repeat(k, 1, 1, 1) * eps.double()
    excess = float(((z.double() - ref).abs() - (2.0 ** -23 * z.double().abs() + 1e-38)).max())
    assert excess <= 0.0, excess
    n = torch.distributions.Normal
    kl32 = torch.distributions.kl_divergence(n(mean, std), n(torch.zeros_like(mean), torch.ones_like(std))).sum((1, 2, 3))
    ref_kl = _kl64(mean, std)
    err_hip = record("kl_abs_err_hip", float((kl.double() - ref_kl).abs().max()))
    err_t32 = record("kl_abs_err_torch_fp32", float((kl32.double() - ref_kl).abs().max()))
    print(f"kl (B, C) = ({b}, {c}): |hip - f64| {err_hip:.3e}, |torch fp32 - f64| {err_t32:.3e}, kl ~ {float(ref_kl.mean()):.1f}")
    assert err_hip <= 4.0 * err_t32, (err_hip, err_t32)
    again = _draw(mean, std, k)[1]
    assert torch.equal(again, kl)                                 # fixed order, no atomics
    assert torch.equal(_draw(mean, std, 1, offset=9)[1], kl)      # and independent of K and of the noise
    assert _draw(mean, std, k, want_kl=False)[1] is None


# ---- 4. backward -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("with_kl", [False, True])
def test_backward_against_float64_autograd(cuda, k, with_kl):
    from ode_rl_amd import hip_ops
    b, c = 3, 64
    mean, std = _inputs(b, c, 6, cuda)
    _, _, eps = _draw(mean, std, k)
    g = torch.Generator().manual_seed(7)
    gz = torch.randn(k * b, c, 16, 16, generator=g).to(cuda)
    gkl = (torch.randn(b, generator=g) * 0.3).to(cuda) if with_kl else None
    m64, s64 = mean.double().requires_grad_(True), std.double().requires_grad_(True)
    z64 = m64.repeat(k, 1, 1, 1) + s64.repeat(k, 1, 1, 1) * eps.double()
    obj = (z64 * gz.double()).sum()
    if with_kl:
        obj = obj + (_kl64(m64, s64) * gkl.double()).sum()
    rm, rs = torch.autograd.grad(obj, [m64, s64])
    gm, gs = hip_ops.latent_sample_backward(gz, gkl, mean, std, k, SEED, OFFSET)
    em, es = record("grad_mean_rel_l2", rel_l2(gm, rm)), record("grad_std_rel_l2", rel_l2(gs, rs))
    assert em <= 1e-5 and es <= 1e-5, (em, es)
    gm2, gs2 = hip_ops.latent_sample_backward(gz, gkl, mean, std, k, eps_in=eps)
    assert torch.equal(gm2, gm) and torch.equal(gs2, gs)          # regenerated noise == stored noise, bit for bit


def test_sample_z0_under_autograd(cuda):
    import ode_rl_amd
    mean, std = _inputs(2, 64, 8, cuda)
    mean.requires_grad_(True)
    std.requires_grad_(True)
    g = torch.Generator().manual_seed(9)
    gz, gkl = torch.randn(6, 64, 16, 16, generator=g).to(cuda), torch.randn(2, generator=g).to(cuda)
    torch.manual_seed(3)
    z, kl = ode_rl_amd.sample_z0(mean, std, n_samples=3)
    eps = ode_rl_amd.last_z0_noise()
    ((z * gz).sum() + (kl * gkl).sum()).backward()
    m64, s64 = mean.detach().double().requires_grad_(True), std.detach().double().requires_grad_(True)
    obj = ((m64.repeat(3, 1, 1, 1) + s64.repeat(3, 1, 1, 1) * eps.double()) * gz.double()).sum() + (_kl64(m64, s64) * gkl.double()).sum()
    rm, rs = torch.autograd.grad(obj, [m64, s64])
    assert rel_l2(mean.grad, rm) <= 1e-5 and rel_l2(std.grad, rs) <= 1e-5
    # z0 alone (kl unused, then not even asked for): no KL term in the gradient
    for return_kl in (True, False):
        mean.grad = std.grad = None
        z, kl = ode_rl_amd.sample_z0(mean, std, seed=11, return_kl=return_kl)
        assert (kl is None) == (not return_kl)
        z.sum().backward()
        assert torch.equal(mean.grad, torch.ones_like(mean)) and torch.equal(std.grad, ode_rl_amd.last_z0_noise())
    # saved inputs are versioned
    z, _ = ode_rl_amd.sample_z0(mean, std)
    with torch.no_grad():
        std.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        z.sum().backward()


# ---- 5. non-finite values ----------------------------------------------------------------------------------------------------------

def test_zero_std_and_nan_are_not_laundered(cuda):
    b, c, k = 3, 64, 2
    mean, std = _inputs(b, c, 10, cuda)
    z_clean, kl_clean, _ = _draw(mean, std, k)
    std0 = std.clone()
    std0[0, 5, 3, 7] = 0.0
    z, kl, _ = _draw(mean, std0, k)
    assert float(kl[0]) == float("inf") and torch.isfinite(kl[1:]).all() and torch.equal(kl[1:], kl_clean[1:])
    assert torch.isfinite(z).all()
    for kk in range(k):
        assert float(z[kk * b, 5, 3, 7]) == float(mean[0, 5, 3, 7])
    mean_nan = mean.clone()
    mean_nan[1, 9, 0, 1] = float("nan")
    z, kl, _ = _draw(mean_nan, std, k)
    nan_rows = torch.isnan(z).view(k * b, -1).any(1).cpu().tolist()
    assert nan_rows == [r % b == 1 for r in range(k * b)]
    assert torch.isnan(kl).cpu().tolist() == [False, True, False] and torch.equal(kl[[0, 2]], kl_clean[[0, 2]])


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------

def _model(**opt_kw):
    """`_model('rk4')` of tests/test_hip_train_end_to_end.py with the z_sample switches in its opt, and one more step away from a kink:
    std_z0 = |second half of the head's output|, and the KL term carries 1 / std -- that half's weights times 0.25 and a bias of 1 keep
    std in about [0.3, 1.7], away from the kink of |.| at 0, where two correct fp32 implementations may disagree in sign (as that file
    keeps its ReLUs from theirs)."""
    from test_hip_train_end_to_end import _model as base
    m = base("rk4")
    for key, v in opt_kw.items():
        setattr(m.opt, key, v)
    with torch.no_grad():
        m.ode_convgru_cell.transform_z0[2].weight[64:].mul_(0.25)
        m.ode_convgru_cell.transform_z0[2].bias[64:].fill_(1.0)
    return m


def _oracle(m, frames, truth, t_obs, t_pred, eps, kl_weight):
    """_oracle_loss of tests/test_hip_train_end_to_end.py with z0 = mean + std * eps (eps (K * B, C, 16, 16), sample-major) and the KL
    term of the ODEConvGRU docstring."""
    from oracle import reference_modules as rm
    from oracle import torchdiffeq_ref
    sd = dict(m.named_parameters())
    pick = lambda prefix: {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}   # noqa: E731
    ws_e, bs_e = rm.split_convnet_state(pick("ode_encoder_func."), "gradient_net.")
    ws_d, bs_d = rm.split_convnet_state(pick("ode_decoder_func."), "gradient_net.")
    b, t, c, h, w = frames.shape
    enc = m.conv_encoder(frames.view(b * t, c, h, w))
    enc = enc.view(b, t, *enc.shape[1:]).permute(1, 0, 2, 3, 4)
    mean, std, _ = rm.ode_convgru_encode(enc, t_obs, rm.ode_func(ws_e, bs_e), pick("ode_convgru_cell.cgru_cell."), pick("ode_convgru_cell.transform_z0."))
    k = eps.shape[0] // b
    z0 = mean.repeat(k, 1, 1, 1) + std.repeat(k, 1, 1, 1) * eps
    sol = torchdiffeq_ref.odeint(rm.ode_func(ws_d, bs_d), z0, t_pred, method="rk4")
    t2, b2 = sol.shape[:2]
    pred = torch.sigmoid(m.conv_decoder(sol.reshape(t2 * b2, *sol.shape[2:])))
    pred = pred.view(t2, b2, *pred.shape[1:]).permute(1, 0, 2, 3, 4)
    n = torch.distributions.Normal
    kl = torch.distributions.kl_divergence(n(mean, std), n(torch.zeros_like(mean), torch.ones_like(std))).sum((1, 2, 3))
    mse = torch.nn.functional.mse_loss(pred, truth.repeat(k, 1, 1, 1, 1))
    kl_term = kl.mean() / mean[0].numel()
    return mse + kl_weight * kl_term, pred, mse, kl_term, std


def _data():
    g = torch.Generator().manual_seed(4)
    frames = torch.rand(2, 3, 1, 64, 64, generator=g)
    truth = torch.rand(2, 3, 1, 64, 64, generator=g)
    return frames, truth, torch.arange(6, dtype=torch.float64) / 6


def test_model_eval_is_the_deterministic_model_and_train_samples(cuda):
    frames, _, ts = _data()
    bd = {"observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)}
    on = _model(z_sample=True).to(cuda)
    off = copy.deepcopy(on)
    off.opt = argparse.Namespace(**{**vars(on.opt), "z_sample": False})
    x = frames.to(cuda)
    with torch.no_grad():
        on.eval(), off.eval()
        assert torch.equal(on(x, bd), off(x, bd))
        off.train()
        assert torch.equal(on(x, bd), off(x, bd))                 # z_sample=False: train() changes nothing either
        on.train()
        p1, p2 = on(x, bd), on(x, bd)
        assert p1.shape == (2, 3, 1, 64, 64) and not torch.equal(p1, p2)
        on.opt.z_n_samples = 3
        assert on(x, bd).shape == (6, 3, 1, 64, 64)


@pytest.mark.parametrize("k,kl_weight", [(1, None), (2, 0.5)])
def test_training_step_matches_the_oracle_pipeline(cuda, k, kl_weight):
    import ode_rl_amd
    kw = {"z_sample": True}
    if k != 1:
        kw["z_n_samples"] = k
    if kl_weight is not None:
        kw["kl_weight"] = kl_weight
    ref = _model(**kw)
    dev = copy.deepcopy(ref).to(cuda).train()
    frames, truth, ts = _data()
    torch.manual_seed(21)
    pred = dev(frames.to(cuda), {"observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)})
    eps = ode_rl_amd.last_z0_noise().cpu()
    loss = dev.get_loss(pred, truth.to(cuda))
    assert pred.shape == (2 * k, 3, 1, 64, 64) and eps.shape == (2 * k, 64, 16, 16)

    loss_ref, pred_ref, mse_ref, kl_ref, std_ref = _oracle(ref, frames, truth, ts[:3], ts[3:], eps, 1.0 if kl_weight is None else kl_weight)
    assert float(std_ref.detach().min()) > 0.05                        # the set-up holds: std_z0 is away from the kink of |.|
    loss_ref.backward()
    e_pred = record("sampled_model_pred_rel_l2", rel_l2(pred, pred_ref.detach()))
    assert e_pred <= 1e-4, e_pred
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref)) + 1e-7, (float(loss), float(loss_ref))
    terms = dev.last_loss_terms
    assert abs(float(terms["mse"]) - float(mse_ref)) <= 1e-5 * abs(float(mse_ref)) + 1e-7
    assert abs(float(terms["kl"]) - float(kl_ref)) <= 1e-5 * abs(float(kl_ref)) + 1e-7 and float(kl_ref) > 0
    loss.backward()
    refp = dict(ref.named_parameters())
    bad = {}
    for name, p in dev.named_parameters():
        assert p.grad is not None, name
        e = rel_l2(p.grad, refp[name].grad)
        if e > 1e-3:
            bad[name] = e
    assert not bad, bad
    # the std half of the head's second convolution: the ground a model without z_sample never trains
    for name in ("weight", "bias"):
        got = getattr(dev.ode_convgru_cell.transform_z0[2], name).grad[64:]
        want = getattr(ref.ode_convgru_cell.transform_z0[2], name).grad[64:]
        assert float(got.abs().max()) > 0 and float(want.abs().max()) > 0, name
        e = record("std_half_grad_rel_l2", rel_l2(got, want))
        assert e <= 1e-3, (name, e)
    plain = copy.deepcopy(ref).to(cuda).train()
    plain.opt = argparse.Namespace(**{**vars(ref.opt), "z_sample": False})
    plain.get_loss(plain(frames.to(cuda), {"observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)}), truth.to(cuda)).backward()
    assert float(plain.ode_convgru_cell.transform_z0[2].weight.grad[64:].abs().max()) == 0.0   # ... which is what this row shows


def test_train_batch_and_evaluate_run_with_z_sample(cuda):
    from ode_rl_amd import train
    model = _model(z_sample=True, z_n_samples=2).to(cuda).train()
    frames, truth, ts = _data()
    bd = {"observed_data": frames - 0.5, "data_to_predict": truth - 0.5, "observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses, terms = [], []
    for _ in range(3):
        pred, tru, loss, _ = train.train_batch(model, bd, opt)
        assert pred.shape == (4, 3, 1, 64, 64) and tru.shape == (2, 3, 1, 64, 64)
        losses.append(float(loss))
        terms.append({k: float(v) for k, v in model.last_loss_terms.items()})
    assert all(np.isfinite(losses)) and all(np.isfinite(list(t.values())).all() for t in terms), (losses, terms)
    assert all(abs(t["mse"] + t["kl"] - l) <= 1e-5 * abs(l) for t, l in zip(terms, losses))      # kl_weight defaults to 1.0
    assert terms[0] != terms[1]
    out = train.evaluate(model, [bd])
    assert model.training
    for key in ("mse", "psnr", "ssim"):
        assert out[key].shape == (3,) and torch.isfinite(out[key]).all(), key
    assert np.isfinite(out["loss"]) and np.isfinite(out["avg_ssim"])
