"""Gradient clipping by global norm on the device (csrc/optim_step.hip: grad_sqsum -> grad_norm_finish -> the clipping update / grad_scale) against
the float64 restatement of tests/_clip_ref.py and against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the same inputs.

Tensor set: 40 parameters, so two 24-tensor launch chunks: (1,), (7,3), (64,), (64,64,3,3) repeated, one tensor of 0 elements, one
parameter whose grad is None, and one of 300 000 elements (the sum of squares runs at most 32 workgroups of 256 threads per tensor
and the update 1024: both grid-stride loops wrap).

Bounds.  Norm: 2**-23 relative against the float64 norm of the same fp32 gradients (float64 accumulation, one fp32 rounding).
Scaled gradients and parameters: 4 x the error of torch's own fp32 composition against the same restatement on the same inputs;
both errors are recorded (conftest.record)."""
import argparse
import copy
import ctypes

import pytest
import torch

import _clip_ref
from conftest import record

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7, 3), (64,), (64, 64, 3, 3)] * 9 + [(1,)]
SHAPES = SHAPES[:5] + [(0,)] + SHAPES[5:30] + [(300000,)] + SHAPES[30:]     # 39 with a gradient; NO_GRAD_AT has none
NO_GRAD_AT = 11
assert len(SHAPES) == 39 and SHAPES.index((300000,)) >= 24      # two chunks, the large tensor in the second
HYPER = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _values(seed, scale=1.0):
    """one CPU tensor per parameter slot (40), from a generator: the same on every machine"""
    g = torch.Generator().manual_seed(seed)
    shapes = SHAPES[:NO_GRAD_AT] + [(5,)] + SHAPES[NO_GRAD_AT:]
    return [torch.randn(s, generator=g) * scale for s in shapes]


def _params(dev, seed=0):
    return [torch.nn.Parameter(v.to(dev)) for v in _values(seed)]


def _set_grads(ps, values):
    for i, (p, v) in enumerate(zip(ps, values)):
        p.grad = None if i == NO_GRAD_AT else v.to(p.device).clone()


def _with_grad(xs):
    return [x for i, x in enumerate(xs) if i != NO_GRAD_AT]


@pytest.fixture(scope="module")
def five_steps():
    """gradients of 5 steps (scale 1 + step), and their float64 restatements at a bound that bites (0.5) -- computed once, read only"""
    steps = [_values(100 + it, scale=1.0 + it) for it in range(5)]
    masked = [[None if i == NO_GRAD_AT else g for i, g in enumerate(s)] for s in steps]
    ref, scaled, norms = _clip_ref.clipped_adam64(_values(0), masked, 0.5, **HYPER)
    return steps, ref, scaled, norms


def test_total_norm_against_float64_and_bitwise_repeatable(cuda, five_steps):
    from ode_rl_amd.optim import clip_grad_norm_
    steps, _, _, norms = five_steps
    a, b = _params(cuda), _params(cuda)
    _set_grads(a, steps[0])
    _set_grads(b, steps[0])
    before = [p.grad.clone() for p in _with_grad(a)]
    ta, tb = clip_grad_norm_(a, 1e9), clip_grad_norm_(b, 1e9)      # far above the norm: the coefficient is exactly 1
    assert ta.is_cuda and ta.dim() == 0 and a[NO_GRAD_AT].grad is None
    err = record("clip_total_norm_rel_err", abs(float(ta) - norms[0]) / norms[0])
    assert err <= 2.0 ** -23, err
    assert torch.equal(ta, tb)
    for p, q, g in zip(_with_grad(a), _with_grad(b), before):
        assert torch.equal(p.grad, q.grad) and torch.equal(p.grad, g)


def test_clip_grad_norm_scales_like_the_restatement(cuda, five_steps):
    from ode_rl_amd.optim import clip_grad_norm_
    steps, _, _, norms = five_steps
    a, b = _params(cuda), _params(cuda)
    _set_grads(a, steps[0])
    _set_grads(b, steps[0])
    assert norms[0] > 0.5
    _, _, want = _clip_ref.clip64(_with_grad(steps[0]), 0.5)
    total = clip_grad_norm_(a, 0.5)
    torch.nn.utils.clip_grad_norm_(b, 0.5)
    ours = record("clip_scale_err_hip", _clip_ref.rel_l2_all([p.grad for p in _with_grad(a)], want))
    torchs = record("clip_scale_err_torch", _clip_ref.rel_l2_all([p.grad for p in _with_grad(b)], want))
    assert abs(float(total) - norms[0]) <= 2.0 ** -23 * norms[0]      # the norm BEFORE clipping
    assert ours <= 4 * torchs, (ours, torchs)
    after = _clip_ref.total_norm64([p.grad for p in _with_grad(a)])
    assert after <= 0.5 * (1 + 2.0 ** -22)


def test_fused_adam_clipped_steps_against_the_restatement(cuda, five_steps):
    from ode_rl_amd.optim import FusedAdam
    steps, ref, scaled, norms = five_steps
    a, b = _params(cuda), _params(cuda)
    oa, ob = FusedAdam(a, max_grad_norm=0.5, **HYPER), torch.optim.Adam(b, **HYPER)
    for it in range(5):
        _set_grads(a, steps[it])
        _set_grads(b, steps[it])
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, 0.5)
        ob.step()
        assert abs(float(oa.last_grad_norm) - norms[it]) <= 2.0 ** -23 * norms[it]
        assert float(oa.last_clipped_norm) <= 0.5 * (1 + 2.0 ** -22)
    g_ours = record("clip_adam_grad_err_hip", _clip_ref.rel_l2_all([p.grad for p in _with_grad(a)], _with_grad(scaled)))
    g_torch = record("clip_adam_grad_err_torch", _clip_ref.rel_l2_all([p.grad for p in _with_grad(b)], _with_grad(scaled)))
    p_ours = record("clip_adam_param_err_hip", _clip_ref.rel_l2_all(_with_grad(a), _with_grad(ref.p)))
    p_torch = record("clip_adam_param_err_torch", _clip_ref.rel_l2_all(_with_grad(b), _with_grad(ref.p)))
    assert g_ours <= 4 * g_torch, (g_ours, g_torch)
    assert p_ours <= 4 * p_torch, (p_ours, p_torch)
    assert torch.equal(a[NO_GRAD_AT].detach().cpu(), _values(0)[NO_GRAD_AT]) and a[NO_GRAD_AT] not in oa.state


def test_bound_above_the_norm_changes_no_bit(cuda, five_steps):
    """coefficient exactly 1: gradients, parameters and moments are those of an unclipped FusedAdam run"""
    from ode_rl_amd.optim import FusedAdam
    steps = five_steps[0]
    a, b = _params(cuda), _params(cuda)
    oa, ob = FusedAdam(a, max_grad_norm=1e6, **HYPER), FusedAdam(b, **HYPER)
    for it in range(3):
        _set_grads(a, steps[it])
        _set_grads(b, steps[it])
        oa.step()
        ob.step()
    assert float(oa.last_grad_norm) == float(oa.last_clipped_norm) > 0 and ob.last_grad_norm is None
    for p, q, g in zip(_with_grad(a), _with_grad(b), _with_grad(steps[2])):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad) and torch.equal(p.grad.cpu(), g)
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])


def test_a_nan_gradient_poisons_everything_as_in_torch(cuda, five_steps):
    from ode_rl_amd.optim import FusedAdam, clip_grad_norm_
    grads = [g.clone() for g in five_steps[0][0]]
    grads[20].view(-1)[3] = float("nan")
    a, b = _params(cuda), _params(cuda)
    _set_grads(a, grads)
    _set_grads(b, grads)
    assert torch.isnan(clip_grad_norm_(a, 0.5)) and torch.isnan(torch.nn.utils.clip_grad_norm_(b, 0.5))
    for p, q in zip(_with_grad(a), _with_grad(b)):
        assert bool(torch.isnan(p.grad).all()) and bool(torch.isnan(q.grad).all())
    _set_grads(a, grads)
    opt = FusedAdam(a, max_grad_norm=0.5, **HYPER)
    opt.step()
    assert torch.isnan(opt.last_grad_norm) and torch.isnan(opt.last_clipped_norm)
    for p in _with_grad(a):
        assert bool(torch.isnan(p).all()) and bool(torch.isnan(p.grad).all())
    assert not bool(torch.isnan(a[NO_GRAD_AT]).any())


def test_an_inf_gradient_gives_coefficient_zero_as_in_torch(cuda, five_steps):
    from ode_rl_amd.optim import FusedAdam, clip_grad_norm_
    grads = [g.clone() for g in five_steps[0][0]]
    grads[20].view(-1)[3] = float("inf")
    a, b, c = _params(cuda), _params(cuda), _params(cuda)
    for ps in (a, b, c):
        _set_grads(ps, grads)
    ta, tb = clip_grad_norm_(a, 0.5), torch.nn.utils.clip_grad_norm_(b, 0.5)
    assert float(ta) == float(tb) == float("inf")
    for i, (p, q) in enumerate(zip(a, b)):
        if i == NO_GRAD_AT:
            continue
        assert torch.equal(torch.isnan(p.grad), torch.isnan(q.grad)) and int(torch.isnan(p.grad).sum()) == (1 if i == 20 else 0)
        assert torch.equal(torch.nan_to_num(p.grad), torch.nan_to_num(q.grad)) and torch.equal(torch.signbit(p.grad), torch.signbit(q.grad))
        assert not bool(torch.nan_to_num(p.grad).any())
    # the fused step leaves the same gradients, and parameters equal to torch's clipping followed by the unclipped step
    oc, ob = FusedAdam(c, max_grad_norm=0.5, **HYPER), FusedAdam(b, **HYPER)
    oc.step()
    ob.step()
    assert float(oc.last_grad_norm) == float("inf") and torch.isnan(oc.last_clipped_norm)      # inf * 0
    for i, (p, q) in enumerate(zip(c, b)):
        if i == NO_GRAD_AT:
            continue
        assert torch.equal(torch.isnan(p.grad), torch.isnan(q.grad)) and torch.equal(torch.nan_to_num(p.grad), torch.nan_to_num(q.grad))
        assert torch.equal(torch.isnan(p), torch.isnan(q)) and int(torch.isnan(p).sum()) == (1 if i == 20 else 0)
        assert torch.equal(torch.nan_to_num(p.detach()), torch.nan_to_num(q.detach()))


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e-3, 795.0, 797.0, 1e9, 0.0])
def test_device_coefficient_is_torchs_expression_bit_for_bit(cuda, five_steps, max_norm):
    """the three floats of odehip_grad_norm against torch's own device arithmetic on the same fp32 norm (796.03 here: bounds on both
    sides of it and next to it)"""
    from ode_rl_amd.optim import _grad_norm
    grads = [g.to(cuda) for g in _with_grad(five_steps[0][0])]
    out3, _ = _grad_norm(grads, max_norm)
    total = out3[0].clone()
    want = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    assert torch.equal(out3[1], want), (float(out3[1]), float(want))
    assert torch.equal(out3[2], total * want)
    assert (float(want) == 1.0) == (max_norm > 796.1)


def test_unclipped_step_skips_a_tensor_without_elements(cuda):
    """torch.optim.Adam accepts a parameter of 0 elements (it has state and nothing to update); so does the unclipped FusedAdam"""
    from ode_rl_amd.optim import FusedAdam
    a = [torch.nn.Parameter(torch.zeros(0, device=cuda)), torch.nn.Parameter(torch.arange(3.0, device=cuda))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = FusedAdam(a, **HYPER), torch.optim.Adam(b, **HYPER)
    for ps in (a, b):
        ps[0].grad, ps[1].grad = torch.zeros(0, device=cuda), torch.tensor([1.0, -2.0, 0.5], device=cuda)
    oa.step()
    ob.step()
    assert sorted(oa.state[a[0]]) == ["exp_avg", "exp_avg_sq", "step"] and int(oa.state[a[0]]["step"]) == 1
    assert torch.allclose(a[1], b[1], rtol=1e-6, atol=0)
    # and a clipped step in which no parameter has a gradient reports a norm of zero, as torch's clip_grad_norm_ does
    for p in a:
        p.grad = None
    oa.step(max_grad_norm=1.0)
    assert float(oa.last_grad_norm) == 0.0 and float(oa.last_clipped_norm) == 0.0


def _plain_adam_step(ps, state, step, lr, betas, eps, weight_decay):
    """the unclipped C entry point called directly on the tensors that have elements: FusedAdam's step as it was before clipping"""
    from ode_rl_amd import _lib
    from ode_rl_amd.hip_ops import _stream
    live = [p for p in ps if p.grad is not None and p.numel() > 0]
    for p in live:
        state.setdefault(p, (torch.zeros_like(p), torch.zeros_like(p)))
    n = len(live)
    arr = lambda xs: (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    numel = (ctypes.c_longlong * n)(*[p.numel() for p in live])
    _lib.check(_lib.load().odehip_adam_step(arr(live), arr([p.grad for p in live]), arr([state[p][0] for p in live]),
                                            arr([state[p][1] for p in live]), numel, n, lr, betas[0], betas[1], eps, weight_decay, step,
                                            _stream()))


@pytest.mark.parametrize("off", [None, -1])
def test_clipping_off_is_the_step_as_it_was(cuda, five_steps, off):
    from ode_rl_amd.optim import FusedAdam
    steps = five_steps[0]
    a, b = _params(cuda), _params(cuda)
    oa, state = FusedAdam(a, max_grad_norm=off, **HYPER), {}
    for it in range(3):
        _set_grads(a, steps[it])
        _set_grads(b, steps[it])
        oa.step()
        with torch.no_grad():
            _plain_adam_step(b, state, it + 1, **HYPER)
    assert oa.last_grad_norm is None
    for p, q, g in zip(_with_grad(a), _with_grad(b), _with_grad(steps[2])):
        assert torch.equal(p, q) and torch.equal(p.grad.cpu(), g)      # gradients untouched
        if p.numel():
            assert torch.equal(oa.state[p]["exp_avg"], state[q][0]) and torch.equal(oa.state[p]["exp_avg_sq"], state[q][1])


def test_state_dict_round_trips_through_torch_adam(cuda, five_steps):
    from ode_rl_amd.optim import FusedAdam
    steps = five_steps[0]
    a = _params(cuda)
    oa = FusedAdam(a, max_grad_norm=0.5, **HYPER)
    _set_grads(a, steps[0])
    oa.step()
    sd = oa.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 0.5 and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = torch.optim.Adam(b, **HYPER)
    ob.load_state_dict(copy.deepcopy(sd))
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oc = FusedAdam(c, **HYPER)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert oc.param_groups[0]["max_grad_norm"] == 0.5      # torch carries unknown group keys along
    _set_grads(a, steps[1])
    _set_grads(c, steps[1])
    oa.step()
    oc.step()
    for p, q in zip(_with_grad(a), _with_grad(c)):
        assert torch.equal(p, q)


MODEL_OPT = argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3,
                               neural_ode_n_units=64, neural_ode_decoder_out_ch=64, decode_diff_method="dopri5", mem=False,
                               z_sample=False)


@pytest.fixture(scope="module")
def model_case(cuda):
    """weights and batch of the small ODEConvGRU model of test_hip_train_loop.py, the batch already on the device"""
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    torch.manual_seed(1)
    state = {k: v.clone() for k, v in ODEConvGRU(MODEL_OPT, torch.device("cpu")).state_dict().items()}
    g = torch.Generator().manual_seed(2)
    ts = torch.arange(6, dtype=torch.float64) / 6
    batch = {"observed_data": (torch.rand(2, 3, 1, 64, 64, generator=g) - 0.5).to(cuda),
             "data_to_predict": (torch.rand(2, 3, 1, 64, 64, generator=g) - 0.5).to(cuda),
             "observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)}
    return state, batch


def _model(state, cuda):
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    model = ODEConvGRU(MODEL_OPT, torch.device("cpu"))
    model.load_state_dict(state)
    return model.to(cuda)


def test_nothing_synchronises_with_the_host(cuda, five_steps, model_case):
    from ode_rl_amd import train
    from ode_rl_amd.optim import FusedAdam, clip_grad_norm_
    steps = five_steps[0]
    a = _params(cuda)
    oa = FusedAdam(a, max_grad_norm=0.5, **HYPER)
    model = _model(model_case[0], cuda)
    om = FusedAdam(model.parameters(), lr=1e-3)
    _set_grads(a, steps[0])
    clip_grad_norm_(a, 0.5)                 # first calls allocate workspaces and fill the host-side caches of the model's solver
    oa.step()
    train.train_batch(model, model_case[1], om, clip=1e-3)
    _set_grads(a, steps[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total = clip_grad_norm_(a, 0.5)
        oa.step()
        _, _, loss, ld = train.train_batch(model, model_case[1], om, clip=1e-3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert total.is_cuda and oa.last_grad_norm.is_cuda and oa.last_clipped_norm.is_cuda and ld["Gradient Norm"].is_cuda
    assert float(total) > 0.5 and float(ld["Gradient Norm"]) <= 1e-3 * (1 + 2.0 ** -22)


def test_train_batch_clips_like_torch_before_the_step(cuda, model_case):
    """clip = 1e-3 bites (asserted).  One step from the same weights: train_batch(clip=) against loss.backward(), torch's
    clip_grad_norm_, an unclipped FusedAdam.step(); both against the float64 restatement from the unclipped gradients."""
    from ode_rl_amd import train
    from ode_rl_amd.optim import FusedAdam
    state, batch = model_case
    ma, mb = _model(state, cuda), _model(state, cuda)
    oa, ob = FusedAdam(ma.parameters(), lr=1e-3), FusedAdam(mb.parameters(), lr=1e-3)
    start = [p.detach().clone() for p in mb.parameters()]
    _, _, _, ld = train.train_batch(ma, batch, oa, clip=1e-3)
    assert sorted(ld) == ["Gradient Norm", "Per Step Loss"] and ld["Gradient Norm"].is_cuda and ld["Gradient Norm"].dim() == 0
    assert float(oa.last_grad_norm) > 1e-3
    assert float(ld["Gradient Norm"]) <= 1e-3 * (1 + 2.0 ** -22)
    ob.zero_grad()
    mb.get_loss(mb.get_prediction(batch["observed_data"] + 0.5, batch_dict=batch), batch["data_to_predict"] + 0.5).backward()
    raw = [p.grad.detach().clone() for p in mb.parameters()]
    torch.nn.utils.clip_grad_norm_(mb.parameters(), 1e-3)
    ob.step()
    ref, scaled, _ = _clip_ref.clipped_adam64(start, [raw], 1e-3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    g_ours = record("clip_train_grad_err_hip", _clip_ref.rel_l2_all([p.grad for p in ma.parameters()], scaled))
    g_torch = record("clip_train_grad_err_torch", _clip_ref.rel_l2_all([p.grad for p in mb.parameters()], scaled))
    p_ours = record("clip_train_param_err_hip", _clip_ref.rel_l2_all(list(ma.parameters()), ref.p))
    p_torch = record("clip_train_param_err_torch", _clip_ref.rel_l2_all(list(mb.parameters()), ref.p))
    assert g_ours <= 4 * g_torch, (g_ours, g_torch)
    assert p_ours <= 4 * p_torch, (p_ours, p_torch)


def test_train_batch_without_clip_keeps_its_keys_and_other_optimizers_get_torchs_clip(cuda, model_case):
    from ode_rl_amd import train
    from ode_rl_amd.optim import FusedAdam
    state, batch = model_case
    m = _model(state, cuda)
    for clip in (None, -1):
        _, _, _, ld = train.train_batch(m, batch, FusedAdam(m.parameters(), lr=1e-3), clip=clip)
        assert list(ld) == ["Per Step Loss"]
    _, _, _, ld = train.train_batch(m, batch, torch.optim.Adam(m.parameters(), lr=1e-3), clip=1e-3)
    assert sorted(ld) == ["Gradient Norm", "Per Step Loss"] and float(ld["Gradient Norm"]) <= 1e-3 * (1 + 2.0 ** -22)
    after = _clip_ref.total_norm64([p.grad for p in m.parameters()])
    assert abs(after - float(ld["Gradient Norm"])) <= 1e-5 * after


def test_c_abi_argument_errors_surface_as_python_exceptions(cuda):
    from ode_rl_amd import _lib
    from ode_rl_amd.optim import clip_grad_norm_
    lib = _lib.load()
    p = torch.nn.Parameter(torch.ones(1000, device=cuda))
    p.grad = torch.ones(1000, device=cuda)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            clip_grad_norm_([p], bad)
    assert torch.equal(p.grad, torch.ones(1000, device=cuda))      # refused before anything ran
    grads = (ctypes.c_void_p * 1)(p.grad.data_ptr())
    numel = (ctypes.c_longlong * 1)(1000)
    need = lib.odehip_grad_norm_workspace_bytes(1, numel)
    assert need == 8 * 4       # ceil(1000 / 256) workgroups, one float64 each
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    out3 = torch.empty(3, device=cuda)
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(lib.odehip_grad_norm(grads, numel, 1, 1.0, ws.data_ptr(), need - 8, out3.data_ptr(), None))
    with pytest.raises(ValueError, match="null"):
        _lib.check(lib.odehip_grad_norm(None, numel, 1, 1.0, ws.data_ptr(), need, out3.data_ptr(), None))
    with pytest.raises(ValueError, match="null"):
        _lib.check(lib.odehip_grad_scale(None, numel, 1, out3.data_ptr(), None))
    with pytest.raises(ValueError, match="null"):
        _lib.check(lib.odehip_adam_step_clipped(grads, grads, grads, grads, numel, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None))
