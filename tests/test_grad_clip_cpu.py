"""Gradient clipping by global norm, the parts a CPU can check: the float64 restatement the GPU tests measure against
(tests/_clip_ref.py) agrees with torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on CPU tensors, and
ode_rl_amd.optim.clip_grad_norm_ hands anything that is not a CUDA float32 gradient to torch's function (the same call: equal bits)."""
import pytest
import torch

import _clip_ref

SHAPES = [(1,), (7, 3), (64,), (16, 16, 3, 3), (0,), (1000,)]
HYPER = dict(lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _params(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES + [(5,)]]
    for p in ps[:-1]:
        p.grad = torch.randn(p.shape, generator=g) * scale
    return ps   # the last one has no gradient


@pytest.mark.parametrize("max_norm", [0.5, 1e4])
def test_restatement_matches_torch_on_the_cpu(max_norm):
    """5 clipped Adam steps: fp32 torch against the float64 restatement.  fp32 against float64 arithmetic of a handful of operations
    per element and step: 1e-5 relative on the parameters leaves two orders of magnitude over the fp32 rounding of one update."""
    ps = _params(0)
    g = torch.Generator().manual_seed(1)
    steps = [[None if p.grad is None else torch.randn(p.shape, generator=g) * (1 + it) for p in ps] for it in range(5)]
    ref, scaled, norms = _clip_ref.clipped_adam64(ps, steps, max_norm, **HYPER)
    opt = torch.optim.Adam(ps, **HYPER)
    for it, grads in enumerate(steps):
        for p, gr in zip(ps, grads):
            p.grad = None if gr is None else gr.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(float(total) - norms[it]) <= 1e-6 * norms[it]
        opt.step()
    have = [i for i, gr in enumerate(steps[-1]) if gr is not None]
    assert _clip_ref.rel_l2_all([ps[i].grad for i in have], [scaled[i] for i in have]) <= 1e-6
    assert _clip_ref.rel_l2_all([ps[i] for i in have], [ref.p[i] for i in have]) <= 1e-5
    assert torch.equal(ps[-1].detach().double(), ref.p[-1])       # no gradient: untouched in both
    clipped = norms[-1] > max_norm
    assert float(_clip_ref.coef32(norms[-1], max_norm)) == (pytest.approx(max_norm / norms[-1], rel=1e-5) if clipped else 1.0)


def test_coefficient_is_torchs_expression_bit_for_bit():
    for total, max_norm in [(3.0, 1.0), (0.3, 1.0), (1e-3, 1e-3), (123.456, 0.7), (float("inf"), 1.0), (0.0, 2.0)]:
        t = torch.tensor(total, dtype=torch.float32)
        want = torch.clamp(max_norm / (t + 1e-6), max=1.0)
        assert torch.equal(_clip_ref.coef32(total, max_norm), want)
    assert torch.isnan(_clip_ref.coef32(float("nan"), 1.0))


def test_cpu_gradients_go_to_torch():
    from ode_rl_amd.optim import clip_grad_norm_
    a, b = _params(3, scale=4.0), _params(3, scale=4.0)
    got, want = clip_grad_norm_(a, 0.25), torch.nn.utils.clip_grad_norm_(b, 0.25)
    assert torch.equal(got, want) and float(got) > 0.25
    for p, q in zip(a[:-1], b[:-1]):
        assert torch.equal(p.grad, q.grad)
    assert a[-1].grad is None
    # float64 gradients are not the kernels' business either
    c = [torch.nn.Parameter(torch.ones(4, dtype=torch.float64))]
    c[0].grad = torch.full((4,), 2.0, dtype=torch.float64)
    assert float(clip_grad_norm_(c, 1.0)) == 4.0 and torch.allclose(c[0].grad, torch.full((4,), 0.5, dtype=torch.float64), rtol=1e-6)


def test_edge_cases_of_the_public_call():
    from ode_rl_amd.optim import clip_grad_norm_
    assert torch.equal(clip_grad_norm_([], 1.0), torch.tensor(0.0))
    assert torch.equal(clip_grad_norm_([torch.nn.Parameter(torch.ones(3))], 1.0), torch.tensor(0.0))   # no .grad anywhere
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    assert float(clip_grad_norm_(p, 10.0)) == pytest.approx(3 ** 0.5)       # a single tensor, as torch takes it
    for norm_type in (1, float("inf"), 2.5):
        with pytest.raises(ValueError, match="norm_type"):
            clip_grad_norm_([p], 1.0, norm_type=norm_type)


def test_fused_adam_carries_max_grad_norm_in_its_state_dict():
    from ode_rl_amd.optim import FusedAdam
    ps = _params(4)
    opt = FusedAdam(ps, lr=1e-3, max_grad_norm=0.5)
    assert opt.defaults["max_grad_norm"] == 0.5 and opt.param_groups[0]["max_grad_norm"] == 0.5
    assert opt.last_grad_norm is None and opt.last_clipped_norm is None
    fresh = FusedAdam(_params(4), lr=1e-3)
    assert fresh.param_groups[0]["max_grad_norm"] is None
    fresh.load_state_dict(opt.state_dict())
    assert fresh.param_groups[0]["max_grad_norm"] == 0.5
    # a torch.optim.Adam state dict has no such key: it loads, and clipping is off
    fresh.load_state_dict(torch.optim.Adam(_params(4), lr=1e-3).state_dict())
    assert fresh.param_groups[0]["max_grad_norm"] is None
    for bad in (-2.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdam(_params(4), max_grad_norm=bad)
    FusedAdam(_params(4), max_grad_norm=-1)   # the reference's "off"


def test_train_batch_takes_clip():
    import inspect
    from ode_rl_amd import train
    assert inspect.signature(train.train_batch).parameters["clip"].default is None
