"""Upstream Vid-ODE's model on the GPU: the plain ConvGRU cell (csrc/convgru_plain.hip), the encoder around it in both directions and
ode_rl_amd.models.conv_odegru.VidODE, against the float64 restatement of tests/_vidode_upstream_ref.py.

Tolerance rule (every comparison of values): the fused result may err against the float64 yardstick by at most 4 x the error the fp32
torch composition (`fused=False` on the same GPU: cell, encoder, and for the whole model `VidODE(opt, device, fused=False)`) shows
against it on the same inputs, plus a floor of 4 * 2^-24 * max|yardstick|.  Errors are max-abs.  The observed ratios err / bound are
recorded through conftest.record (one run's summary is committed as profiles/vidode_upstream_parity_observed.json)."""
import contextlib

import pytest
import torch

import _vidode_upstream_ref as ref
from conftest import load_golden, record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _rule(name, fused, comp, yard):
    fused, comp, yard = fused.detach().double().cpu(), comp.detach().double().cpu(), yard.detach().double().cpu()
    assert fused.shape == yard.shape == comp.shape, (name, fused.shape, comp.shape, yard.shape)
    err_f, err_c = float((fused - yard).abs().max()), float((comp - yard).abs().max())
    bound = 4.0 * err_c + 4.0 * U * float(yard.abs().max())
    ratio = err_f / bound if bound > 0 else (0.0 if err_f == 0 else float("inf"))
    record(name + ".ratio", ratio)
    print(f"{name}: fused err {err_f:.3e}, composition err {err_c:.3e}, bound {bound:.3e}, ratio {ratio:.3f}, max|yardstick| {float(yard.abs().max()):.3e}")
    assert err_f <= bound, (name, err_f, err_c, bound)


def _weights(shape, seed):
    n = 1
    for d in shape:
        n *= d
    return torch.cos(torch.arange(n, dtype=torch.float64) * (0.37 + 0.01 * seed) + seed).view(shape)


# ---- one cell step ------------------------------------------------------------------------------------------------------------------

def _cell(sd, ch, fused, cuda):
    from ode_rl_amd.models import conv_odegru
    cell = conv_odegru.ConvGRUCell((16, 16), ch, ch, (3, 3), True, torch.FloatTensor, fused=fused)
    cell.load_state_dict(sd)
    return cell.to(cuda)


@pytest.mark.parametrize("ch", [64, 128])
def test_cell_forward_and_every_gradient(cuda, ch):
    sd, x, h = ref.cell_case(ch)
    gout = _weights((3, ch, 16, 16), 1)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64, h64 = x.double().requires_grad_(True), h.double().requires_grad_(True)
    y64 = ref.cell(sd64, x64, h64)
    (y64 * gout).sum().backward()
    res = {}
    for fused in (True, False):
        cell = _cell(sd, ch, fused, cuda)
        xd, hd = x.to(cuda).requires_grad_(True), h.to(cuda).requires_grad_(True)
        y = cell(xd, hd)
        (y * gout.float().to(cuda)).sum().backward()
        res[fused] = [y, xd.grad, hd.grad] + [p.grad for _, p in sorted(cell.named_parameters())]
    yard = [y64, x64.grad, h64.grad] + [sd64[k].grad for k in sorted(sd64)]
    for name, f, c, y in zip(["h_next", "grad_x", "grad_h"] + ["grad_" + k for k in sorted(sd64)], res[True], res[False], yard):
        _rule(f"cell[{ch}].{name}", f, c, y)


def test_masked_cell_forward_and_every_gradient(cuda):
    sd, x, h = ref.cell_case(64)
    mask, gout = torch.tensor(ref.CELL_MASK), _weights((3, 64, 16, 16), 5)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64, h64 = x.double().requires_grad_(True), h.double().requires_grad_(True)
    y64 = ref.cell(sd64, x64, h64, mask.double())
    (y64 * gout).sum().backward()
    res = {}
    for fused in (True, False):
        cell = _cell(sd, 64, fused, cuda)
        xd, hd = x.to(cuda).requires_grad_(True), h.to(cuda).requires_grad_(True)
        y = cell(xd, hd, mask.to(cuda))
        (y * gout.float().to(cuda)).sum().backward()
        res[fused] = [y, xd.grad, hd.grad] + [p.grad for _, p in sorted(cell.named_parameters())]
    yard = [y64, x64.grad, h64.grad] + [sd64[k].grad for k in sorted(sd64)]
    for name, f, c, y in zip(["h_next", "grad_x", "grad_h"] + ["grad_" + k for k in sorted(sd64)], res[True], res[False], yard):
        _rule(f"cell[64,masked].{name}", f, c, y)
    assert torch.count_nonzero(res[True][1][1]) == 0 and torch.equal(res[True][2][1].cpu(), gout[1].float())   # m == 0: x unused, h passes


def test_cell_with_mask_matches_fixture_case(cuda):
    gold = load_golden("vidode_upstream.npz")
    sd, x, h = ref.cell_case(64)
    mask = torch.tensor(ref.CELL_MASK)
    y64 = ref.cell({k: v.double() for k, v in sd.items()}, x.double(), h.double(), mask.double())
    with torch.no_grad():
        yf = _cell(sd, 64, True, cuda)(x.to(cuda), h.to(cuda), mask.to(cuda))
        yc = _cell(sd, 64, False, cuda)(x.to(cuda), h.to(cuda), mask.to(cuda))
    _rule("cell[64].masked_h_next", yf, yc, y64)
    _rule("cell[64].masked_h_next_vs_fixture", yf, yc, torch.from_numpy(gold["cell.h_next"]))
    assert torch.equal(yf[1].cpu(), h[1])


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------

ENC_MASKS = {"none": None, "ones": [[1.0] * 3] * 3, "mixed": [[1.0, 0.0, 0.5], [0.5, 1.0, 0.0], [0.0, 0.5, 1.0]]}


def _encoder(sd, rb, fused, cuda, ch=64):
    from ode_rl_amd.models import conv_odegru
    func = conv_odegru.ODEFunc(None, ch, ch, conv_odegru.create_convnet(ch, ch, n_layers=1, n_units=ch))
    solver = conv_odegru.DiffeqSolver(ch, func, "euler", ch, odeint_rtol=1e-3, odeint_atol=1e-4)
    enc = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), ch, ch, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                             return_all_layers=True, z0_diffeq_solver=solver, run_backwards=rb, fused=fused)
    enc.load_state_dict(sd)
    return enc.to(cuda)


def _run_encoder(enc, frames, mask, rb, weights, cuda):
    """(mean, std, latent_ys, grad_inputs, {parameter gradients}) with the gradient arriving through all three outputs."""
    x = frames.to(cuda).requires_grad_(True)
    m = None if mask is None else torch.tensor(mask, device=cuda).unsqueeze(-1)
    times = torch.tensor(ref.ENC_TIMES, dtype=torch.float64)
    if enc.fused:
        mean, std, latent = enc._encode(x, times, m, rb, True)      # one C call each way
    else:
        last, latent = enc.run_ode_conv_gru(x, m, times, rb)
        out = enc.transform_z0(last)
        mean, std = out[:, :enc.z0_dim], out[:, enc.z0_dim:].abs()
    gm, gs, gl = (w.float().to(cuda) for w in weights)
    ((mean * gm).sum() + (std * gs).sum() + (latent * gl).sum()).backward()
    return mean, std, latent, x.grad, {k: p.grad for k, p in enc.named_parameters()}


_enc_cache = {}


def _encoder_results(cuda, rb, mask_name):
    key = (rb, mask_name)
    if key not in _enc_cache:
        sd, frames = ref.encoder_case(64, 3)
        mask = ENC_MASKS[mask_name]
        weights = (_weights((3, 64, 16, 16), 2), _weights((3, 64, 16, 16), 3), _weights((3, 3, 64, 16, 16), 4) * 0.5)
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        x64 = frames.double().requires_grad_(True)
        m64, s64, l64 = ref.encoder(sd64, x64, ref.ENC_TIMES, None if mask is None else torch.tensor(mask).double(), rb)
        ((m64 * weights[0]).sum() + (s64 * weights[1]).sum() + (l64 * weights[2]).sum()).backward()
        yard = (m64, s64, l64, x64.grad, {k: v.grad for k, v in sd64.items()})
        fused = _run_encoder(_encoder(sd, rb, True, cuda), frames, mask, rb, weights, cuda)
        comp = _run_encoder(_encoder(sd, rb, False, cuda), frames, mask, rb, weights, cuda)
        _enc_cache[key] = (fused, comp, yard)
    return _enc_cache[key]


@pytest.mark.parametrize("mask_name", ["none", "ones", "mixed"])
@pytest.mark.parametrize("rb", [True, False])
def test_encoder_outputs_and_every_gradient(cuda, rb, mask_name):
    fused, comp, yard = _encoder_results(cuda, rb, mask_name)
    tag = f"encoder[rb={int(rb)},mask={mask_name}]"
    for i, name in enumerate(["mean", "std", "latent_ys", "grad_inputs"]):
        _rule(f"{tag}.{name}", fused[i], comp[i], yard[i])
    assert set(fused[4]) == set(yard[4])
    for k in sorted(yard[4]):
        _rule(f"{tag}.grad_{k}", fused[4][k], comp[4][k], yard[4][k])


@pytest.mark.parametrize("rb", [True, False])
def test_mask_of_ones_is_bitwise_the_unmasked_call(cuda, rb):
    a, b = _encoder_results(cuda, rb, "none")[0], _encoder_results(cuda, rb, "ones")[0]
    for i in range(4):
        assert torch.equal(a[i], b[i]), i
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k


@pytest.mark.parametrize("rb", [True, False])
def test_unobserved_frame_has_exactly_zero_input_gradient(cuda, rb):
    gin = _encoder_results(cuda, rb, "mixed")[0][3]
    for b, row in enumerate(ENC_MASKS["mixed"]):
        for i, m in enumerate(row):
            assert (torch.count_nonzero(gin[b, i]) == 0) == (m == 0.0), (b, i)


@pytest.mark.parametrize("rb", [True, False])
def test_nan_in_unobserved_frame_does_not_reach_mean(cuda, rb):
    sd, frames = ref.encoder_case(64, 3)
    enc = _encoder(sd, rb, True, cuda)
    mask = torch.tensor(ENC_MASKS["mixed"], device=cuda).unsqueeze(-1)
    times = torch.tensor(ref.ENC_TIMES, dtype=torch.float64)
    poisoned = frames.clone()
    poisoned[0, 1], poisoned[1, 2], poisoned[2, 0] = float("nan"), float("nan"), float("inf")
    with torch.no_grad():
        clean = enc(frames.to(cuda), times, mask=mask)
        got = enc(poisoned.to(cuda), times, mask=mask)
    assert torch.equal(clean[0], got[0]) and torch.equal(clean[1], got[1])


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def _model(extrap, cuda, fused=True):
    from ode_rl_amd.models import conv_odegru
    model = conv_odegru.VidODE(ref.model_opt(extrap), cuda, fused=fused)
    sd = ref.model_state_dict(model.state_dict())
    model.load_state_dict(sd)
    return model.train(), {k: v for k, v in sd.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


@contextlib.contextmanager
def _repeatable_library_convolutions():
    """The model's BatchNorm encoder and flow decoder convolve through the library, whose default choice among its algorithms is not
    the same in every call; the deterministic ones, for both sides of the comparison, as tests/test_hip_vidode_grads.py does."""
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was


@pytest.mark.parametrize("extrap", [True, False])
def test_compute_all_losses_and_every_parameter_gradient(cuda, extrap):
    """B = 2, three observed and three predicted frames, BatchNorm in train(), dec_diff = 'euler'.  The weights keep every ReLU
    pre-activation away from its kink (tests/_vidode_upstream_ref.py::model_state_dict), so the gradient is a smooth function of the
    rounding on both sides; the composition is the model's own fused=False form on the same GPU."""
    gold = load_golden("vidode_upstream.npz")
    batch = ref.model_batch()
    tag = "extrap" if extrap else "interp"
    got = {}
    with _repeatable_library_convolutions():
        for fused in (True, False):
            model, params = _model(extrap, cuda, fused)
            res = model.compute_all_losses(dict(batch))
            res["loss"].backward()
            got[fused] = (res, dict(model.named_parameters()))
    used = {k for k in params if not k.startswith("encoder_z0.cell_list.1.")}
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items() if k in used}
    yard = ref.losses(leaves, batch, 2, extrap)
    yard["loss"].backward()
    _rule(f"model[{tag}].loss", got[True][0]["loss"], got[False][0]["loss"], yard["loss"])
    _rule(f"model[{tag}].pred_y", got[True][0]["pred_y"], got[False][0]["pred_y"], yard["pred_y"])
    _rule(f"model[{tag}].pred_y_vs_fixture", got[True][0]["pred_y"], got[False][0]["pred_y"], torch.from_numpy(gold[f"{tag}.pred_y"]))
    for k in sorted(used):
        _rule(f"model[{tag}].grad_{k}", got[True][1][k].grad, got[False][1][k].grad, leaves[k].grad)
    for fused in (True, False):
        for k, p in got[fused][1].items():
            if k.startswith("encoder_z0.cell_list.1."):
                assert p.grad is None, k


def test_train_batch_gan_step_changes_the_used_parameters(cuda):
    import ode_rl_amd
    model, _ = _model(True, cuda)
    opt = ref.model_opt(True)
    netD_img, netD_seq, optD = ode_rl_amd.create_netD(opt, cuda)
    optG = ode_rl_amd.FusedAdamax([p for p in model.parameters()], lr=1e-3)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    batch = {k: (v - 0.5 if k in ("observed_data", "data_to_predict") else v) for k, v in ref.model_batch().items()}
    _, _, loss, loss_dict = ode_rl_amd.train_batch_gan(model, netD_img, netD_seq, batch, optG, optD)
    assert torch.isfinite(loss) and all(torch.isfinite(v) for v in loss_dict.values())
    # a convolution bias in front of a BatchNorm with batch statistics has a gradient of exactly zero: it moves nothing
    bn_fed = {"encoder.cnn_encoder.0.bias", "encoder.cnn_encoder.3.bias", "encoder.cnn_encoder.6.bias", "decoder.model.1.bias",
              "decoder.model.5.bias"}
    for k, p in model.named_parameters():
        if k.startswith("encoder_z0.cell_list.1."):
            assert p.grad is None and torch.equal(p, before[k]), k
        elif k not in bn_fed:
            assert not torch.equal(p, before[k]), k
