"""Upstream Vid-ODE's model (ode_rl_amd.models.conv_odegru), the parts a CPU can check: the float64-capable restatement
tests/_vidode_upstream_ref.py against the fixture upstream's own classes produced (tests/golden/vidode_upstream.npz), the new model's
keys, the fused=False encoder against fixture and restatement, the C argument checks of the plain cell, and the refusals.

Tolerances.  Restatement and fused=False encoder against the fixture: the same float32 torch kernels in the same order on the same
machine type, apart from where a float64 step size is rounded; a handful of ulps through three steps, bounded here by a rel-L2 of
1e-5 (a wrong gate order or init image is O(1)).  float32 autograd against the float64 restatement: eps32 = 6e-8, reductions of up to
1152 terms (sqrt -> 34) through about 24 convolutions each way: 6e-8 * 34 * 24 = 5e-5, bounded by 1e-4."""
import ctypes

import pytest
import torch

import _vidode_upstream_ref as ref
import ode_rl_amd
from conftest import load_golden, rel_l2
from ode_rl_amd import _lib
from ode_rl_amd.models import conv_odegru

FIXTURE_TOL, F32_TOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def gold():
    return load_golden("vidode_upstream.npz")


def test_restatement_cell_matches_fixture(gold):
    sd, x, h = ref.cell_case(64)
    got = ref.cell(sd, x, h, torch.tensor(ref.CELL_MASK))
    assert rel_l2(got, torch.from_numpy(gold["cell.h_next"])) <= FIXTURE_TOL
    assert torch.equal(got[1], h[1])                      # mask 0 keeps the state


@pytest.mark.parametrize("rb", [True, False])
def test_restatement_encoder_matches_fixture(gold, rb):
    sd, frames = ref.encoder_case(64, 2)
    mean, std, _ = ref.encoder(sd, frames, ref.ENC_TIMES, torch.tensor(ref.ENC_MASK), rb)
    assert rel_l2(mean, torch.from_numpy(gold[f"enc.rb{int(rb)}.mean"])) <= FIXTURE_TOL
    assert rel_l2(std, torch.from_numpy(gold[f"enc.rb{int(rb)}.std"])) <= FIXTURE_TOL


def _model_sd(extrap):
    model = conv_odegru.VidODE(ref.model_opt(extrap), "cpu", fused=False)
    return model, ref.model_state_dict(model.state_dict())


@pytest.mark.parametrize("extrap", [True, False])
def test_restatement_model_matches_fixture(gold, extrap):
    _, sd = _model_sd(extrap)
    with torch.no_grad():
        res = ref.losses(sd, ref.model_batch(), 2, extrap)
    tag = "extrap" if extrap else "interp"
    assert rel_l2(res["pred_y"], torch.from_numpy(gold[f"{tag}.pred_y"])) <= FIXTURE_TOL
    assert abs(float(res["loss"]) - float(gold[f"{tag}.loss"][0])) <= FIXTURE_TOL * float(gold[f"{tag}.loss"][0])
    assert not torch.equal(torch.from_numpy(gold["extrap.pred_y"]), torch.from_numpy(gold["interp.pred_y"]))


def test_model_has_upstreams_keys_and_parameter_count(gold):
    model, _ = _model_sd(True)
    assert sorted(model.state_dict().keys()) == [str(k) for k in gold["keys"]]
    assert sum(p.numel() for p in model.parameters()) == int(gold["n_params"][0])
    assert len(model.encoder_z0.cell_list) == 2
    for name in ("conv_odegru", "Encoder_z0_ODE_ConvGRU", "DiffeqSolver"):
        assert hasattr(ode_rl_amd, name) and hasattr(ode_rl_amd.models, name)


def _encoder_module(sd, rb, fused=False, device="cpu"):
    func = conv_odegru.ODEFunc(None, 64, 64, conv_odegru.create_convnet(64, 64, n_layers=1, n_units=64))
    solver = conv_odegru.DiffeqSolver(64, func, "euler", 64, odeint_rtol=1e-3, odeint_atol=1e-4)
    enc = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), 64, 64, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                             return_all_layers=True, z0_diffeq_solver=solver, run_backwards=rb, fused=fused)
    enc.load_state_dict(sd)
    return enc.to(device)


@pytest.mark.parametrize("rb", [True, False])
def test_composition_encoder_on_cpu_matches_fixture_and_restatement_gradients(gold, rb):
    sd, frames = ref.encoder_case(64, 2)
    mask = torch.tensor(ref.ENC_MASK)
    enc = _encoder_module(sd, rb)
    x = frames.clone().requires_grad_(True)
    mean, std = enc(x, torch.tensor(ref.ENC_TIMES, dtype=torch.float64), mask=mask.unsqueeze(-1))
    assert rel_l2(mean, torch.from_numpy(gold[f"enc.rb{int(rb)}.mean"])) <= FIXTURE_TOL
    assert rel_l2(std, torch.from_numpy(gold[f"enc.rb{int(rb)}.std"])) <= FIXTURE_TOL
    gm, gs = torch.cos(torch.arange(mean.numel()).view_as(mean) * 0.37), torch.sin(torch.arange(std.numel()).view_as(std) * 0.11)
    (mean * gm + std * gs).sum().backward()
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = frames.double().requires_grad_(True)
    m64, s64, _ = ref.encoder(sd64, x64, ref.ENC_TIMES, mask.double(), rb)
    (m64 * gm.double() + s64 * gs.double()).sum().backward()
    assert rel_l2(x.grad, x64.grad) <= F32_TOL
    assert torch.count_nonzero(x.grad[0, 1]) == 0 and torch.count_nonzero(x.grad[1, 2]) == 0     # unobserved (sample, frame)
    for k, p in enc.named_parameters():
        assert rel_l2(p.grad, sd64[k].grad) <= F32_TOL, k


def test_fused_cell_and_encoder_refuse_host_tensors():
    sd, x, h = ref.cell_case(64)
    cell = conv_odegru.ConvGRUCell((16, 16), 64, 64, (3, 3), True, torch.FloatTensor)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cell(x, h)


def _plain_desc(keep, n_null=4, ks=3, ch=64):
    """A cell descriptor over host memory (never dereferenced: the checks answer first); the first n_null of the four gn_* are NULL."""
    buf = ctypes.create_string_buffer(64)
    keep.append(buf)
    p = ctypes.addressof(buf)
    gn = [None] * n_null + [p] * (4 - n_null)
    return _lib.ConvGRUCellDesc(input=ch, hidden=ch, ks=ks, w_gates=p, b_gates=p, gn_gates_w=gn[0], gn_gates_b=gn[1], w_can=p, b_can=p,
                                gn_can_w=gn[2], gn_can_b=gn[3])


def test_plain_descriptor_argument_checks_answer_before_any_hip_call():
    lib, keep = _lib.load(), []
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    d = _plain_desc(keep)
    assert lib.odehip_convgru_cell_workspace_bytes(ctypes.byref(d), 2) > 0
    # all four NULL pass check_cell: the call gets as far as the workspace size
    assert lib.odehip_convgru_cell_forward(ctypes.byref(d), p, p, p, 2, p, 16, None) == -1
    assert b"workspace too small" in lib.odehip_last_error()
    bw = _lib.ConvGRUCellBwd(p.value, p.value, p.value, p.value)
    gr = _lib.ConvGRUCellGrads(p.value, p.value, None, None, p.value, p.value, None, None)
    assert lib.odehip_convgru_cell_backward(ctypes.byref(d), ctypes.byref(bw), p, p, p, p, p, ctypes.byref(gr), 2, p, 16, None) == -1
    assert b"workspace too small" in lib.odehip_last_error()
    # three of four NULL
    d3 = _plain_desc(keep, n_null=3)
    assert lib.odehip_convgru_cell_forward(ctypes.byref(d3), p, p, p, 2, p, 16, None) == -1
    assert b"null parameter pointer" in lib.odehip_last_error()
    # the sequence path keeps refusing plain cells with the message it has for a missing parameter: a 5x5 descriptor with every
    # weight image the path asks for (full Winograd forms, all four halves), so that the NULL gn_* pointers are the only thing wrong
    hv = _lib.ConvGRUCellHalves()
    for j in range(4):
        hv.wino[j] = p.value
    d5 = _plain_desc(keep, ks=5)
    d5.w_gates_wino = d5.w_can_wino = p.value
    assert lib.odehip_convgru_sequence_forward(ctypes.byref(d5), ctypes.byref(hv), p, p, 2, 2, p, p, 1 << 30, None) == -1
    assert b"null parameter pointer" in lib.odehip_last_error()
    g5 = _plain_desc(keep, n_null=0, ks=5)     # the same descriptor with GroupNorm pointers gets past the argument checks
    g5.w_gates_wino = g5.w_can_wino = p.value
    assert lib.odehip_convgru_sequence_forward(ctypes.byref(g5), ctypes.byref(hv), p, p, 2, 2, p, p, 16, None) == -1
    assert b"workspace too small" in lib.odehip_last_error()
    # upstream's 3x3 cell is refused for its kernel size, as any 3x3 cell is
    d3x3 = _plain_desc(keep, ks=3)
    assert lib.odehip_convgru_sequence_forward(ctypes.byref(d3x3), ctypes.byref(hv), p, p, 2, 2, p, p, 1 << 30, None) == -1
    assert b"serve ks = 5" in lib.odehip_last_error()


def test_plain_encoder_descriptor_reaches_the_workspace_check():
    lib, keep = _lib.load(), []
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    e = _lib.EncoderDesc()
    e.cell = _plain_desc(keep)
    e.f_enc.n_convs, e.f_enc.ks = 2, 3
    for i in range(3):
        e.f_enc.channels[i] = 64
    for i in range(2):
        e.f_enc.w_packed[i] = e.f_enc.bias[i] = p.value
    e.head_hidden, e.out_ch = 64, 64
    e.w_head0 = e.b_head0 = e.w_head1 = e.b_head1 = p.value
    t = (ctypes.c_double * 3)(0.0, 0.1, 0.2)
    assert lib.odehip_encoder_workspace_bytes(ctypes.byref(e), 3, 2) > 0 and lib.odehip_encoder_train_workspace_bytes(ctypes.byref(e), 3, 2) > 0
    for fn in (lib.odehip_odeconvgru_encode_masked, lib.odehip_odeconvgru_encode_train_masked):
        assert fn(ctypes.byref(e), p, t, 3, 2, 1, p, p, None, p, 16, None, None) == -1
        assert b"workspace too small" in lib.odehip_last_error()
    e.cell = _plain_desc(keep, n_null=3)
    assert lib.odehip_odeconvgru_encode_masked(ctypes.byref(e), p, t, 3, 2, 1, p, p, None, p, 16, None, None) == -1
    assert b"null parameter pointer" in lib.odehip_last_error()


def test_refusals():
    func = conv_odegru.ODEFunc(None, 64, 64, conv_odegru.create_convnet(64, 64, 1, 64))
    for kw in (dict(nru=True), dict(nru2=True)):
        with pytest.raises(NotImplementedError):
            conv_odegru.DiffeqSolver(64, func, "euler", 64, **kw)
    with pytest.raises(NotImplementedError):
        conv_odegru.create_convnet(64, 64, 1, 64, nonlinear="relu")
    opt = ref.model_opt(True)
    opt.slot_attention = True
    with pytest.raises(NotImplementedError):
        conv_odegru.VidODE(opt, "cpu")
    opt = ref.model_opt(True)
    opt.input_size = 128
    with pytest.raises(ValueError, match="input_size"):
        conv_odegru.VidODE(opt, "cpu")
    opt = ref.model_opt(True)
    opt.nru = True
    with pytest.raises(NotImplementedError):
        conv_odegru.VidODE(opt, "cpu")
