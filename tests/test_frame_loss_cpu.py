"""The training losses on the CPU: the float64 restatements of tests/_loss_ref.py against the torch compositions the models ran before
csrc/frame_loss.hip existed (written out below, word for word), the public functions, their torch path for CPU tensors, and the
argument errors -- all checked before a tensor reaches the device, so no GPU is needed."""
import argparse

import numpy as np
import pytest
import torch

import _loss_ref as lr


def _mse_composition(pred, truth, kl=None, kl_weight=1.0, per_row=None):
    """models/ODEConvGRU.py::get_loss as it stood: truth.repeat over the K draws, mse_loss, kl.mean() / per_row."""
    b, t, c, h, w = truth.size()
    if kl is None:
        return torch.nn.functional.mse_loss(pred.reshape(b * t, c, h, w), truth.reshape(b * t, c, h, w)), None, None
    n = pred.shape[0] // b
    if n > 1:
        truth = truth.repeat(n, 1, 1, 1, 1)
    mse = torch.nn.functional.mse_loss(pred.reshape(n * b * t, c, h, w), truth.reshape(n * b * t, c, h, w))
    kl_term = kl.mean() / per_row
    return mse + kl_weight * kl_term, mse, kl_term


def _vidode_composition(pred, inter, truth, init, mask):
    """models/VidODE.py::get_loss, get_mse and get_diff as they stood."""
    def get_mse(truth, pred_x, mask=None):
        b, _, c, h, w = truth.size()
        if mask is None:
            n, sel = truth.size(1), truth
        else:
            n = int(mask[0].sum())
            sel = truth[mask.squeeze(-1).bool()].view(b, n, c, h, w)
        return torch.sum(torch.abs(pred_x - sel)) / (b * n * c * h * w)

    def get_diff(data, mask):
        d = data[:, 1:, ...] - data[:, :-1, ...]
        b, _, c, h, w = d.size()
        n = int(mask[0].sum())
        return d[mask.squeeze(-1).bool()].view(b, n, c, h, w)

    data = torch.cat([init.unsqueeze(1), truth], dim=1)
    data_diff = get_diff(data, mask)
    l1_pred = torch.mean(get_mse(truth, pred, mask))
    l1_diff = torch.mean(get_mse(data_diff, inter, None))
    return torch.mean(l1_pred + l1_diff), l1_pred, l1_diff


def _mse_inputs(k, b, t, c, h, w, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(k * b, t, c, h, w, generator=g, dtype=dtype)
    truth = torch.rand(b, t, c, h, w, generator=g, dtype=dtype) - 0.5
    kl = torch.rand(b, generator=g, dtype=dtype) * 300.0 + 5.0
    return pred, truth, kl


HOLED = [[1, 0, 1, 1, 0], [0, 1, 1, 0, 1]]   # the positions differ per row; row 0 selects t = 0 (init is used), row 1 does not


def _l1_inputs(b, t, n, c, h, w, seed, mask_rows=None, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(b, n, c, h, w, generator=g, dtype=dtype) - 0.5
    outputs = torch.rand(b, n, c + 3, h, w, generator=g, dtype=dtype) - 0.5
    truth = torch.rand(b, t, c, h, w, generator=g, dtype=dtype) - 0.5
    observed = torch.rand(b, 3, c, h, w, generator=g, dtype=dtype) - 0.5
    mask = torch.ones(b, t, 1) if mask_rows is None else torch.tensor(mask_rows, dtype=torch.float32).view(b, t, 1)
    return pred, outputs[:, :, 2:2 + c], truth, observed[:, -1], mask


def test_the_mse_restatement_agrees_with_the_torch_composition():
    for k, with_kl, kw in ((1, False, 1.0), (3, True, 2.5), (2, True, 0.0)):
        pred, truth, kl = _mse_inputs(k, 2, 3, 1, 8, 12, 11 + k, torch.float64)
        pred.requires_grad_(True)
        kl.requires_grad_(True)
        loss, mse, kl_term = _mse_composition(pred, truth, kl if with_kl else None, kw, 64 * 256)
        (3.0 * loss).backward()
        ref = lr.mse_kl(pred.detach().numpy(), truth.numpy(), kl.detach().numpy() if with_kl else None, kw, 64 * 256, grad_out=3.0)
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-13 * abs(ref["loss"])
        assert np.allclose(pred.grad.numpy(), ref["grad_pred"], rtol=1e-12, atol=0.0)
        if with_kl:
            assert abs(float(mse.detach()) - ref["mse"]) <= 1e-13 * ref["mse"] and abs(float(kl_term.detach()) - ref["kl_term"]) <= 1e-13 * ref["kl_term"]
            assert np.allclose(kl.grad.numpy(), ref["grad_kl"], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("mask_rows", [None, HOLED], ids=["ones", "holed"])
def test_the_l1_restatement_agrees_with_the_torch_composition(mask_rows):
    b, t = (2, 5)
    n = 5 if mask_rows is None else 3
    pred, inter, truth, init, mask = _l1_inputs(b, t, n, 1, 8, 12, 5, mask_rows, torch.float64)
    pred.requires_grad_(True)
    inter = inter.clone().requires_grad_(True)
    loss, l1_pred, l1_diff = _vidode_composition(pred, inter, truth, init, mask)
    (3.0 * loss).backward()
    ref = lr.vidode_l1(pred.detach().numpy(), inter.detach().numpy(), truth.numpy(), init.numpy(), mask.numpy(), grad_out=3.0)
    for got, key in ((loss, "loss"), (l1_pred, "l1_pred"), (l1_diff, "l1_diff")):
        assert abs(float(got.detach()) - ref[key]) <= 1e-13 * ref[key], key
    assert np.allclose(pred.grad.numpy(), ref["grad_pred"], rtol=1e-12, atol=0.0)
    assert np.allclose(inter.grad.numpy(), ref["grad_inter"], rtol=1e-12, atol=0.0)
    if mask_rows is not None:
        assert lr.selected_frames(mask.numpy(), n) == [[0, 2, 3], [1, 2, 4]]
        assert lr.selected_frames(np.array([[1, 0, 0, 1, 0], [1, 1, 1, 0, 0]]), 3) == [None, [0, 1, 2]]
        short = lr.vidode_l1(pred.detach().numpy(), inter.detach().numpy(), truth.numpy(), init.numpy(), np.array([[1, 0, 0, 1, 0], [1, 1, 1, 0, 0]]))
        assert np.isnan(short["loss"]) and np.isnan(short["l1_pred"]) and np.isnan(short["l1_diff"])


def test_sgn_is_what_the_backward_of_torch_abs_uses():
    x = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf"), 2.0, -3.0], requires_grad=True)
    x.abs().sum().backward()
    assert np.array_equal(lr.sgn(x.detach().numpy().astype(np.float64)), x.grad.numpy().astype(np.float64))


def test_the_public_functions_exist():
    import ode_rl_amd
    for name in ("mse_kl_loss", "vidode_l1_loss"):
        assert name in ode_rl_amd.__all__ and callable(getattr(ode_rl_amd, name))
    from ode_rl_amd import hip_ops
    for name in ("loss_mse", "loss_mse_backward", "loss_vidode_l1", "loss_vidode_l1_backward"):
        assert callable(getattr(hip_ops, name))


def test_cpu_tensors_take_the_torch_composition():
    import ode_rl_amd
    pred, truth, kl = _mse_inputs(2, 2, 3, 1, 8, 12, 3)
    got = ode_rl_amd.mse_kl_loss(pred, truth, kl=kl, kl_weight=2.5, latent_elems=64 * 256)
    want = _mse_composition(pred, truth, kl, 2.5, 64 * 256)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    plain = ode_rl_amd.mse_kl_loss(pred[:2], truth)
    assert torch.equal(plain[0], torch.nn.functional.mse_loss(pred[:2], truth)) and torch.equal(plain[1], plain[0]) and plain[2] is None
    # the graph is the composition's
    p = pred.clone().requires_grad_(True)
    k = kl.clone().requires_grad_(True)
    ode_rl_amd.mse_kl_loss(p, truth, kl=k, kl_weight=2.5, latent_elems=64 * 256)[0].backward()
    p2, k2 = pred.clone().requires_grad_(True), kl.clone().requires_grad_(True)
    _mse_composition(p2, truth, k2, 2.5, 64 * 256)[0].backward()
    assert torch.equal(p.grad, p2.grad) and torch.equal(k.grad, k2.grad)
    for rows in (None, HOLED):
        a = _l1_inputs(2, 5, 5 if rows is None else 3, 1, 8, 12, 9, rows)
        got = ode_rl_amd.vidode_l1_loss(*a)
        want = _vidode_composition(*a)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        got2 = ode_rl_amd.vidode_l1_loss(*a[:4], a[4][:, :, 0].bool())      # (B, T) bool selects the same frames
        assert torch.equal(got2[0], want[0])


def test_the_models_go_through_the_public_functions_on_the_cpu():
    """VidODE.get_loss on CPU tensors is the composition's value (ODEConvGRU and ConvGRU: tests/test_latent_sample_cpu.py and
    tests/test_convgru_model_cpu.py compare get_loss with mse_loss bit for bit)."""
    from ode_rl_amd.models.VidODE import VidODE
    opt = argparse.Namespace(n_downs=2, resolution=64, in_channels=1, n_layers=2, decode_diff_method="rk4")
    model = VidODE(opt, torch.device("cpu"))
    pred, inter, truth, init, mask = _l1_inputs(2, 5, 3, 1, 8, 12, 21, HOLED)
    observed = torch.zeros(2, 2, 1, 8, 12)
    observed[:, -1] = init
    model.batch_dict = {"observed_data": observed, "data_to_predict": truth, "mask_predicted_data": mask}
    model.extra_info = {"pred_intermediates": inter}
    got = model.get_loss(pred, torch.zeros_like(truth))   # the reference's quirk: the truth is the batch dict's, not the argument
    assert torch.equal(got, _vidode_composition(pred, inter, truth, init, mask)[0])


def test_odeconvgru_get_loss_after_a_sampled_forward_on_the_cpu():
    """The KL branch of ODEConvGRU.get_loss (sample_z0 itself needs the device, so the forward's (kl, per_row) is set by hand): K = 2
    draws as a permuted view, as `forward` returns them, against kl (B,) -- the composition's value, terms and gradients bit for bit."""
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    opt = argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3, neural_ode_n_units=64,
                             neural_ode_decoder_out_ch=64, decode_diff_method="rk4", mem=False, z_sample=True, z_n_samples=2, kl_weight=0.5)
    model = ODEConvGRU(opt, torch.device("cpu"))
    pred, truth, kl = _mse_inputs(2, 2, 3, 1, 8, 12, 17)
    time_first = pred.permute(1, 0, 2, 3, 4).contiguous()
    p, k = time_first.clone().requires_grad_(True), kl.clone().requires_grad_(True)
    model._kl = (k, 64 * 256)
    got = model.get_loss(p.permute(1, 0, 2, 3, 4), truth)
    got.backward()
    p2, k2 = time_first.clone().requires_grad_(True), kl.clone().requires_grad_(True)
    want, mse, kl_term = _mse_composition(p2.permute(1, 0, 2, 3, 4), truth, k2, 0.5, 64 * 256)
    want.backward()
    assert torch.equal(got, want) and torch.equal(p.grad, p2.grad) and torch.equal(k.grad, k2.grad)
    assert torch.equal(model.last_loss_terms["mse"], mse) and torch.equal(model.last_loss_terms["kl"], kl_term)
    assert not model.last_loss_terms["mse"].requires_grad and not model.last_loss_terms["kl"].requires_grad and model._kl is None


def test_argument_errors():
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    pred, truth, kl = _mse_inputs(2, 2, 3, 1, 8, 12, 3)
    with pytest.raises(TypeError, match="pred"):
        ode_rl_amd.mse_kl_loss(pred.numpy(), truth)
    with pytest.raises(TypeError, match="kl"):
        ode_rl_amd.mse_kl_loss(pred, truth, kl=[1.0, 2.0], latent_elems=4)
    with pytest.raises(ValueError, match="pred"):
        ode_rl_amd.mse_kl_loss(pred[:3], truth)                       # 3 rows against 2
    with pytest.raises(ValueError, match="pred"):
        ode_rl_amd.mse_kl_loss(pred[..., :8], truth)
    with pytest.raises(ValueError, match="latent_elems"):
        ode_rl_amd.mse_kl_loss(pred, truth, kl=kl)
    with pytest.raises(ValueError, match="latent_elems"):
        ode_rl_amd.mse_kl_loss(pred, truth, kl=kl, latent_elems=0)
    with pytest.raises(ValueError, match="kl must be"):
        ode_rl_amd.mse_kl_loss(pred, truth, kl=kl[:1], latent_elems=4)
    with pytest.raises(NotImplementedError, match="truth"):
        ode_rl_amd.mse_kl_loss(pred, truth.clone().requires_grad_(True))
    a = _l1_inputs(2, 5, 3, 1, 8, 12, 9, HOLED)
    with pytest.raises(TypeError, match="mask"):
        ode_rl_amd.vidode_l1_loss(*a[:4], None)
    with pytest.raises(ValueError, match="inter"):
        ode_rl_amd.vidode_l1_loss(a[0], a[1][:, :2], *a[2:])
    with pytest.raises(ValueError, match="init"):
        ode_rl_amd.vidode_l1_loss(*a[:3], a[3][:1], a[4])
    with pytest.raises(ValueError, match="mask"):
        ode_rl_amd.vidode_l1_loss(*a[:4], a[4][:, :4])
    with pytest.raises(ValueError, match="truth"):
        ode_rl_amd.vidode_l1_loss(a[0], a[1], a[2][:, :2], a[3], a[4][:, :2])   # fewer truth frames than predictions
    for i, name in ((2, "truth"), (3, "init"), (4, "mask")):
        b = list(a)
        b[i] = b[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            ode_rl_amd.vidode_l1_loss(*b)
    # the device entry points have no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.loss_mse(pred, truth)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.loss_vidode_l1(*a)
    with pytest.raises(TypeError, match="torch.Tensor"):
        hip_ops.loss_mse(pred.numpy(), truth)


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    """Null pointers, counts below 1, misaligned pointers or strides: ODEHIP_EINVAL (-1), checked on the host."""
    import ctypes
    from ode_rl_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    a16, odd = P(4096), P(4100)
    assert lib.odehip_loss_mse_workspace_bytes(1, 1, 4096) == 8 and lib.odehip_loss_mse_workspace_bytes(1, 64, 40960) == 8 * 320
    assert lib.odehip_loss_mse_workspace_bytes(1, 1024, 40 * 4096) == 8 * 1024       # the partial count is capped
    assert lib.odehip_loss_vidode_l1_workspace_bytes(4, 10, 4096) == 16 * 40 and lib.odehip_loss_vidode_l1_workspace_bytes(2, 3, 12288) == 16 * 18
    assert lib.odehip_loss_mse(None, a16, 1, 1, 64, None, 0.0, 1.0, a16, a16, 8, None) == -1 and b"null" in lib.odehip_last_error()
    assert lib.odehip_loss_mse(a16, a16, 0, 1, 64, None, 0.0, 1.0, a16, a16, 8, None) == -1
    assert lib.odehip_loss_mse(a16, a16, 1, 0, 64, None, 0.0, 1.0, a16, a16, 8, None) == -1
    assert lib.odehip_loss_mse(a16, a16, 1, 1, 66, None, 0.0, 1.0, a16, a16, 8, None) == -1 and b"multiple of 4" in lib.odehip_last_error()
    assert lib.odehip_loss_mse(odd, a16, 1, 1, 64, None, 0.0, 1.0, a16, a16, 8, None) == -1 and b"aligned" in lib.odehip_last_error()
    assert lib.odehip_loss_mse(a16, a16, 1, 1, 64, None, 0.0, 1.0, a16, a16, 4, None) == -1 and b"workspace" in lib.odehip_last_error()
    assert lib.odehip_loss_mse_backward(a16, a16, a16, 1, 1, 64, 0.0, 1.0, None, None, None) == -1
    assert lib.odehip_loss_mse_backward(a16, a16, a16, 1, 1, 64, 0.0, 1.0, odd, None, None) == -1
    l1 = lambda **kw: lib.odehip_loss_vidode_l1(*[{**dict(pred=a16, inter=a16, ibs=3 * 4096, ifs=4096, truth=a16, init=a16, nbs=4096, mask=a16, byte=0,
                                                          batch=2, frames=5, sel=3, elems=4096, out=a16, ws=a16, wsb=1 << 20, stream=None), **kw}[k]
                                                  for k in ("pred", "inter", "ibs", "ifs", "truth", "init", "nbs", "mask", "byte", "batch", "frames", "sel",
                                                            "elems", "out", "ws", "wsb", "stream")])
    for bad in (dict(mask=None), dict(batch=0), dict(sel=0), dict(sel=6), dict(elems=4098), dict(inter=odd), dict(ifs=4098), dict(ifs=2048),
                dict(ibs=2 * 4096), dict(nbs=4094), dict(byte=2), dict(wsb=8), dict(mask=P(4097))):
        assert l1(**bad) == -1, bad
    assert lib.odehip_loss_vidode_l1_backward(a16, a16, a16, 3 * 4096, 4096, a16, a16, 4096, a16, 0, 2, 5, 3, 4096, a16, odd, None) == -1
    assert lib.odehip_loss_vidode_l1_backward(None, a16, a16, 3 * 4096, 4096, a16, a16, 4096, a16, 0, 2, 5, 3, 4096, a16, a16, None) == -1
