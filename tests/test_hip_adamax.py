"""FusedAdamax (csrc/optim_step.hip) against torch.optim.Adamax(foreach=False) on the same device, fed bit-identical parameters and
gradients for 3 consecutive steps, and train_batch / decay_learning_rate around it (Vid-ODE's recipe, Vid-ODE/main.py:187,214).

Tensor sets: n tensors that reach the kernel, n = 23, 24, 25, 49 (the launches take 24 tensors each: one launch, one full, two, three),
of 1, 255, 256, 257 and 21 elements in turn, the last one of 1024 * 256 + 3 elements (the update runs at most 1024 workgroups of 256
threads per tensor: the smallest size at which its grid-stride loop wraps), one gradient non-contiguous; on top of the n, one tensor
of 0 elements and one parameter without a gradient.

Bounds.  exp_inf: torch.equal on every step -- each of its operations is a single fp32 rounding of bit-identical inputs.  Its inputs
are the gradient and, with weight decay, the parameter, so where wd != 0 the claim is checked with torch's parameters fed to ours
before every step as well (`_against_torch` says what holds free-running).  exp_avg and the parameters: the kernel computes
b1 m + (1 - b1) g with 1 - b1 formed in fp32 (0.10000002) where torch's lerp_ computes m + w (g - m) with w = fl32(1 - 0.9) = 0.1, so
the bound is measured, as max |a - b| over all tensors / max |b| over all tensors:
  * torch against itself, Adamax(foreach=True) against Adamax(foreach=False) on the 49-tensor set over the same 3 steps: measured 0
    for exp_avg and for the parameters (`bound` prints and records what it finds);
  * FusedAdam's own bound against torch.optim.Adam, tests/test_hip_train_loop.py: 1e-6.
BOUND = 4 x the larger of the two = 4e-6; the fixture takes the maximum at run time, so a torch that disagrees with itself by more
widens it and one that agrees with itself cannot narrow it below 4e-6.  Measured for FusedAdamax against torch on the MI355X after 3
steps at lr = 0.05: exp_avg 2.65e-7 (the weight's 2.4e-7), parameters 5.1e-8, exp_inf with weight decay free-running 3.3e-8; two
groups: 1.4e-7 and 9.7e-8; clipped at 0.5: exp_avg 3.4e-7, exp_inf 1.9e-7, parameters 1.0e-7 (wd = 0.01: 1.6e-6, 2.2e-6, 2.2e-6), the
total norm one ulp (1.2e-7) from torch's on the first step and equal on the other two, the scaled gradients 0 ulp apart
(`adamax_*` entries of conftest.record)."""
import argparse

import pytest
import torch

from conftest import record
from ode_rl_amd.optim import FusedAdamax, decay_learning_rate

pytestmark = pytest.mark.gpu

WRAP = 1024 * 256 + 3
FUSED_ADAM_BOUND = 1e-6      # tests/test_hip_train_loop.py::test_fused_adam_matches_torch_adam
HYPER = dict(lr=5e-2, betas=(0.9, 0.999), eps=1e-8)
SMALL = [(1,), (255,), (256,), (257,), (7, 3)]
NONCONTIG_AT = 4             # the first (7, 3) tensor gets its gradient as the transpose of a (3, 7) one


def _shapes(n):
    """n tensors for the kernel, then the two it must never see: one without elements, one without a gradient (the last)"""
    return [SMALL[i % len(SMALL)] for i in range(n - 1)] + [(WRAP,), (0,), (5,)]


def _values(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in shapes]


def _params(shapes, dev, seed=0):
    return [torch.nn.Parameter(v.to(dev)) for v in _values(shapes, seed)]


def _set_grads(ps, values):
    """the same bits into every optimizer's gradients; fresh tensors, so a clipped step of one never reaches another's"""
    for i, (p, v) in enumerate(zip(ps, values)):
        if i == len(ps) - 1:
            p.grad = None
        elif i == NONCONTIG_AT:
            p.grad = v.to(p.device).t().contiguous().t()
            assert not p.grad.is_contiguous() and p.grad.shape == p.shape
        else:
            p.grad = v.to(p.device).clone()


def _rel_max(xs, ys):
    """max |x - y| over all tensors / max |y| over all tensors; NaN if any difference is"""
    num = max(float((x.detach().double() - y.detach().double()).abs().max()) for x, y in zip(xs, ys) if y.numel())
    den = max(float(y.detach().double().abs().max()) for y in ys if y.numel())
    return num / den


def _ulps(a, b):
    """largest distance between two float32 tensors in units in the last place (finite values)"""
    def key(x):
        i = x.detach().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def _state(opt, ps, key):
    return [opt.state[p][key] for p in ps[:-1]]


@pytest.fixture(scope="module")
def bound(cuda):
    """4 x max(torch foreach=True against foreach=False, FusedAdam's bound), measured once on the 49-tensor set with weight decay"""
    shapes = _shapes(49)
    a, b = _params(shapes, cuda), _params(shapes, cuda)
    oa = torch.optim.Adamax(a, foreach=True, weight_decay=0.01, **HYPER)
    ob = torch.optim.Adamax(b, foreach=False, weight_decay=0.01, **HYPER)
    for it in range(3):
        grads = _values(shapes, 100 + it, scale=1.0 + it)
        _set_grads(a, grads)
        _set_grads(b, grads)
        oa.step()
        ob.step()
    own_p = record("adamax_torch_foreach_vs_single_param", _rel_max(a[:-1], b[:-1]))
    own_m = record("adamax_torch_foreach_vs_single_exp_avg", _rel_max(_state(oa, a, "exp_avg"), _state(ob, b, "exp_avg")))
    print(f"torch foreach=True vs foreach=False after 3 steps: parameters {own_p:.3e}, exp_avg {own_m:.3e}")
    return 4 * max(own_p, own_m, FUSED_ADAM_BOUND)


def _three_steps(cuda, shapes, groups, fused_kw=None, clip=None, bad=None, refeed=False):
    """3 steps of FusedAdamax and of torch.optim.Adamax(foreach=False) [after torch's clip_grad_norm_ when `clip`] from the same
    bits.  groups(ps) -> the params argument of both constructors.  refeed: torch's parameters are copied into ours before every
    step, so each step is fed bit-identical parameters.  Yields (step, ours, torchs, their optimizers, torch's norm) after every step."""
    a, b = _params(shapes, cuda), _params(shapes, cuda)
    oa = FusedAdamax(groups(a), **(fused_kw or {}))
    ob = torch.optim.Adamax(groups(b), foreach=False)
    for it in range(3):
        grads = _values(shapes, 100 + it, scale=1.0 + it)
        if bad is not None and it == 0:
            bad(grads)
        _set_grads(a, grads)
        _set_grads(b, grads)
        if refeed:
            with torch.no_grad():
                torch._foreach_copy_(a, [q.detach() for q in b])
        oa.step()
        total = torch.nn.utils.clip_grad_norm_(b, clip) if clip is not None else None
        ob.step()
        yield it, a, b, oa, ob, total


def _against_torch(cuda, bound, shapes, groups, decayed, tag):
    """The checks of the module docstring.  decayed(i): tensor i has weight decay.  exp_inf takes g + wd p in, so it can have torch's
    bits only while the parameters have: from the second step on they are within `bound` of torch's, not equal (exp_avg, above).  So:
    free-running, exp_inf is torch.equal on every step where wd == 0 and on the first step where not, and within `bound` after; and
    fed torch's parameters before every step -- bit-identical parameters and gradients, the premise of the bit-for-bit claim -- it is
    torch.equal on every step for every tensor, weight decay or not."""
    for it, a, b, oa, ob, _ in _three_steps(cuda, shapes, groups):
        for i, (p, q) in enumerate(zip(a[:-1], b[:-1])):
            if it == 0 or not decayed(i):
                assert torch.equal(oa.state[p]["exp_inf"], ob.state[q]["exp_inf"]), (it, i, tuple(p.shape))
            assert int(oa.state[p]["step"]) == int(ob.state[q]["step"]) == it + 1
    err_u = record(f"adamax_{tag}_exp_inf_err", _rel_max(_state(oa, a, "exp_inf"), _state(ob, b, "exp_inf")))
    err_m = record(f"adamax_{tag}_exp_avg_err", _rel_max(_state(oa, a, "exp_avg"), _state(ob, b, "exp_avg")))
    err_p = record(f"adamax_{tag}_param_err", _rel_max(a[:-1], b[:-1]))
    print(f"{tag}: exp_inf {err_u:.3e}, exp_avg {err_m:.3e}, parameters {err_p:.3e}, bound {bound:.3e}")
    assert err_u <= bound and err_m <= bound and err_p <= bound, (err_u, err_m, err_p, bound)
    if any(decayed(i) for i in range(len(shapes))):
        for it, c, d, oc, od, _ in _three_steps(cuda, shapes, groups, refeed=True):
            for i, (p, q) in enumerate(zip(c[:-1], d[:-1])):
                assert torch.equal(oc.state[p]["exp_inf"], od.state[q]["exp_inf"]), ("refed", it, i, tuple(p.shape))
        err_m = record(f"adamax_{tag}_refed_exp_avg_err", _rel_max(_state(oc, c, "exp_avg"), _state(od, d, "exp_avg")))
        err_p = record(f"adamax_{tag}_refed_param_err", _rel_max(c[:-1], d[:-1]))
        print(f"{tag}, parameters fed before every step: exp_avg {err_m:.3e}, parameters {err_p:.3e}")
        assert err_m <= bound and err_p <= bound, (err_m, err_p, bound)
    return a, oa


@pytest.mark.parametrize("n", [23, 24, 25, 49])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_three_steps_against_torch_adamax(cuda, bound, n, weight_decay):
    shapes = _shapes(n)
    groups = lambda ps: [{"params": ps, "weight_decay": weight_decay, **HYPER}]
    a, oa = _against_torch(cuda, bound, shapes, groups, lambda i: weight_decay != 0, f"n{n}_wd{weight_decay}")
    # the unclipped step leaves every gradient alone (the non-contiguous one too), the tensor without elements has torch's state and
    # the parameter without a gradient has none and has not moved
    last = _values(shapes, 102, scale=3.0)
    for p, g in zip(a[:-1], last):
        assert torch.equal(p.grad.cpu(), g)
    assert not a[NONCONTIG_AT].grad.is_contiguous()
    assert sorted(oa.state[a[-2]]) == ["exp_avg", "exp_inf", "step"] and a[-2].numel() == 0
    assert a[-1] not in oa.state and torch.equal(a[-1].detach().cpu(), _values(shapes, 0)[-1])


def test_two_groups_with_their_own_rates(cuda, bound):
    shapes = _shapes(25)
    groups = lambda ps: [{"params": ps[:9], "lr": 5e-2, "betas": (0.9, 0.999), "weight_decay": 0.01},
                         {"params": ps[9:], "lr": 2e-1, "betas": (0.8, 0.99)}]
    _against_torch(cuda, bound, shapes, groups, lambda i: i < 9, "groups")
    # the groups did move at their own rates: a first step is lr * sign(g) whatever the betas
    first = _params(shapes, cuda)
    o1 = FusedAdamax(groups(first))
    _set_grads(first, _values(shapes, 100))
    o1.step()
    start = _values(shapes, 0)
    assert float((first[1].detach().cpu() - start[1]).abs().max()) == pytest.approx(5e-2, rel=1e-4)      # 255 elements, group 0
    assert float((first[11].detach().cpu() - start[11]).abs().max()) == pytest.approx(2e-1, rel=1e-4)    # 255 elements, group 1


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_clipped_steps_against_torchs_clip_and_adamax(cuda, bound, weight_decay):
    """max_grad_norm = 0.5 clips every step (the norms are in the hundreds: asserted)"""
    shapes = _shapes(49)
    groups = lambda ps: [{"params": ps, "weight_decay": weight_decay, **HYPER}]
    for it, a, b, oa, ob, total in _three_steps(cuda, shapes, groups, fused_kw={"max_grad_norm": 0.5}, clip=0.5):
        assert float(total) > 0.5 and float(oa.last_clipped_norm) <= 0.5 * (1 + 2.0 ** -22)
        norm_err = record("adamax_clip_norm_err", abs(float(oa.last_grad_norm) - float(total)) / float(total))
        grad_ulps = record("adamax_clip_grad_ulps", max(_ulps(p.grad, q.grad) for p, q in zip(a[:-1], b[:-1])))
        print(f"wd={weight_decay} step {it}: total norm {float(oa.last_grad_norm)!r} vs torch {float(total)!r} ({norm_err:.2e}), "
              f"scaled gradients {grad_ulps} ulp apart")
        assert norm_err <= 1e-6
    assert grad_ulps <= 1, grad_ulps
    assert not a[NONCONTIG_AT].grad.is_contiguous()      # the kernel scaled a contiguous copy, which was copied back
    err_m = record("adamax_clip_exp_avg_err", _rel_max(_state(oa, a, "exp_avg"), _state(ob, b, "exp_avg")))
    err_u = record("adamax_clip_exp_inf_err", _rel_max(_state(oa, a, "exp_inf"), _state(ob, b, "exp_inf")))
    err_p = record("adamax_clip_param_err", _rel_max(a[:-1], b[:-1]))
    print(f"wd={weight_decay}: exp_avg {err_m:.3e}, exp_inf {err_u:.3e}, parameters {err_p:.3e}, bound {bound:.3e}")
    assert err_m <= bound and err_u <= bound and err_p <= bound, (err_m, err_u, err_p, bound)


def test_bound_above_the_norm_changes_no_bit(cuda):
    """coefficient exactly 1: gradients, parameters and both moments are those of the unclipped kernel"""
    shapes = _shapes(49)
    a, b = _params(shapes, cuda), _params(shapes, cuda)
    oa, ob = FusedAdamax(a, max_grad_norm=1e6, weight_decay=0.01, **HYPER), FusedAdamax(b, weight_decay=0.01, **HYPER)
    for it in range(3):
        grads = _values(shapes, 100 + it, scale=1.0 + it)
        _set_grads(a, grads)
        _set_grads(b, grads)
        oa.step()
        ob.step()
    assert float(oa.last_grad_norm) == float(oa.last_clipped_norm) > 0 and ob.last_grad_norm is None
    for p, q, g in zip(a[:-1], b[:-1], grads):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad) and torch.equal(p.grad.cpu(), g)
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_inf"], ob.state[q]["exp_inf"])


def test_non_finite_gradients_poison_what_torch_poisons_and_nothing_else(cuda, bound):
    """step 1 with a NaN in one gradient element and +inf in another, steps 2 and 3 clean: NaN wherever torch has NaN and inf wherever
    torch has inf, in every step (inf in exp_inf comes with inf in exp_avg: their quotient, and so the parameter, is NaN as in torch,
    and with weight decay on that parameter makes exp_inf NaN one step later), and every other element of those tensors and every other
    tensor has the clean run's bits"""
    shapes = _shapes(25)
    nan_at, inf_at = (3, 100), (24, 70000)      # (tensor, element): a 257-element tensor of the first launch, the large one of the second

    def bad(grads):
        grads[nan_at[0]].view(-1)[nan_at[1]] = float("nan")
        grads[inf_at[0]].view(-1)[inf_at[1]] = float("inf")

    groups = lambda ps: [{"params": ps, "weight_decay": 0.01, **HYPER}]
    clean = _three_steps(cuda, shapes, groups)
    for (it, a, b, oa, ob, _), (_, c, _, oc, _, _) in zip(_three_steps(cuda, shapes, groups, bad=bad), clean):
        for i, (p, q, r) in enumerate(zip(a[:-1], b[:-1], c[:-1])):
            hit = {nan_at[0]: nan_at[1], inf_at[0]: inf_at[1]}.get(i)
            for name, x, y, z in [("param", p.detach(), q.detach(), r.detach())] + \
                                 [(k, oa.state[p][k], ob.state[q][k], oc.state[r][k]) for k in ("exp_avg", "exp_inf")]:
                assert torch.equal(torch.isnan(x), torch.isnan(y)), (it, i, name)
                assert torch.equal(torch.isinf(x), torch.isinf(y)), (it, i, name)
                same = x.view(-1) == z.view(-1)
                if hit is None:
                    assert torch.equal(x, z), (it, i, name)
                else:
                    assert bool(same[:hit].all()) and bool(same[hit + 1:].all()) and not bool(same[hit]), (it, i, name)
        assert bool(torch.isnan(a[nan_at[0]].view(-1)[nan_at[1]])) and bool(torch.isnan(oa.state[a[nan_at[0]]]["exp_inf"].view(-1)[nan_at[1]]))
        u_inf = float(oa.state[a[inf_at[0]]]["exp_inf"].view(-1)[inf_at[1]])
        assert bool(torch.isnan(a[inf_at[0]].view(-1)[inf_at[1]]))
        assert u_inf == float("inf") if it == 0 else u_inf != u_inf      # the NaN parameter comes back through the weight decay


def test_two_runs_are_bitwise_equal(cuda):
    shapes = _shapes(49)
    runs = []
    for _ in range(2):
        a = _params(shapes, cuda)
        oa = FusedAdamax(a, max_grad_norm=0.5, weight_decay=0.01, **HYPER)
        for it in range(3):
            _set_grads(a, _values(shapes, 100 + it, scale=1.0 + it))
            oa.step()
        runs.append((a, oa))
    (a, oa), (b, ob) = runs
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)
    for p, q in zip(a[:-1], b[:-1]):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_inf"], ob.state[q]["exp_inf"])


def test_nothing_synchronises_with_the_host(cuda):
    shapes = _shapes(25)
    a = _params(shapes, cuda)
    oa = FusedAdamax(a, max_grad_norm=0.5, **HYPER)
    _set_grads(a, _values(shapes, 100))
    oa.step()      # the first call allocates the state and the norm's workspace
    _set_grads(a, _values(shapes, 101))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        oa.step()
        oa.step(max_grad_norm=None)
        decay_learning_rate(oa, 0.99, 1e-3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert oa.last_grad_norm.is_cuda and float(oa.last_grad_norm) > 0.5


def test_c_abi_takes_a_tensor_without_elements_only_in_the_clipped_call(cuda):
    """as the Adam pair: torch hands out no pointer for a tensor of 0 elements, and the clipped step gets the gradient list of the norm"""
    import ctypes
    from ode_rl_amd import _lib
    lib = _lib.load()
    x = [torch.ones(4, device=cuda), torch.ones(4, device=cuda), torch.zeros(4, device=cuda), torch.zeros(4, device=cuda)]
    coef = torch.ones(1, device=cuda)
    arrs = [(ctypes.c_void_p * 2)(None, t.data_ptr()) for t in x]
    numel = (ctypes.c_longlong * 2)(0, 4)
    hyper = (0.5, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(ValueError, match="tensor 0 has a null pointer"):
        _lib.check(lib.odehip_adamax_step(*arrs, numel, 2, *hyper, None))
    _lib.check(lib.odehip_adamax_step_clipped(*arrs, numel, 2, *hyper, coef.data_ptr(), None))
    assert torch.allclose(x[0], torch.full((4,), 0.5, device=cuda), rtol=1e-6, atol=0)      # first step: p - lr g / (|g| + eps), g = 1
    assert torch.equal(x[3], torch.full((4,), 1.0, device=cuda) + 1e-8)
    numel[0] = 1
    with pytest.raises(ValueError, match="tensor 0 has a null pointer"):
        _lib.check(lib.odehip_adamax_step_clipped(*arrs, numel, 2, *hyper, coef.data_ptr(), None))


def test_a_step_bumps_the_version_and_the_solver_sees_the_new_weights(cuda):
    """the kernels write through raw pointers: the packed-weight caches of the HIP solver are keyed on `_version`"""
    import ode_rl_amd
    torch.manual_seed(3)
    f = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False).to(cuda)
    z0 = torch.randn(2, 64, 16, 16, device=cuda) * 0.5
    t = torch.arange(3, dtype=torch.float64, device=cuda) / 4
    opt = FusedAdamax(f.parameters(), lr=1e-2)
    with torch.no_grad():
        before = ode_rl_amd.odeint(f, z0, t, method="rk4")
    for it in range(2):
        versions = [p._version for p in f.parameters()]
        for p in f.parameters():
            p.grad = torch.ones_like(p)
        opt.step() if it == 0 else opt.step(max_grad_norm=0.5)
        assert all(p._version > v for p, v in zip(f.parameters(), versions))
    with torch.no_grad():
        after = ode_rl_amd.odeint(f, z0, t, method="rk4")
    fresh = ode_rl_amd.ODEFunc(64, 64, 3, 64, False, "relu", final_act=False)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in f.state_dict().items()})
    with torch.no_grad():
        want = ode_rl_amd.odeint(fresh.to(cuda), z0, t, method="rk4")
    assert not torch.equal(after[1:], before[1:]) and torch.equal(after, want)


MODEL_OPT = argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3,
                               neural_ode_n_units=64, neural_ode_decoder_out_ch=64, decode_diff_method="rk4", mem=False,
                               z_sample=False)


def _model_and_batch(cuda, method="rk4", t_out=2):
    """the small ODEConvGRU model of tests/test_hip_train_loop.py and tests/test_hip_grad_clip.py with a fixed-grid decoder solver,
    and a batch of B = 2 with 3 observed and `t_out` predicted frames"""
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    opt = argparse.Namespace(**{**vars(MODEL_OPT), "decode_diff_method": method})
    torch.manual_seed(1)
    state = {k: v.clone() for k, v in ODEConvGRU(opt, torch.device("cpu")).state_dict().items()}
    g = torch.Generator().manual_seed(2)
    ts = torch.arange(3 + t_out, dtype=torch.float64) / (3 + t_out)
    batch = {"observed_data": (torch.rand(2, 3, 1, 64, 64, generator=g) - 0.5).to(cuda),
             "data_to_predict": (torch.rand(2, t_out, 1, 64, 64, generator=g) - 0.5).to(cuda),
             "observed_tp": ts[:3].to(cuda), "tp_to_predict": ts[3:].to(cuda)}

    def model():
        m = ODEConvGRU(opt, torch.device("cpu"))
        m.load_state_dict(state)
        return m.to(cuda)
    return model, batch


def test_train_batch_clips_inside_the_adamax_step_and_the_decay_scales_the_next_update(cuda, bound, tmp_path):
    """2 steps of train_batch(clip=1e-3; it bites: asserted) with FusedAdamax against the same 2 steps with torch.optim.Adamax, which
    train_batch gives torch's clip_grad_norm_ in front of its step().  ODEConvGRU at B = 2, 3 observed and 2 predicted frames, rk4.
    Bound: the 3-step bound of this file times 1 -- the existing Adam end-to-end test
    (tests/test_hip_train_loop.py::test_train_batch_and_checkpoint_round_trip) allows its two training runs 1e-6 relative, which is
    FusedAdam's single-step bound of the same file, so it allows no factor over it.  Measured: 9.6e-08.
    Why a fixed-grid solver: the two optimizers leave the first step an ulp or two apart (1.5e-8 of the largest parameter: torch's
    fp32 norm against the float64 one, lerp_ against b1 m + (1 - b1) g), and the step-size controller of dopri5, the solver of the
    model in the existing train tests, turns that into a difference at its tolerance in the second step's trajectory and gradients.
    Measured there: 5.385e-5 between FusedAdamax and torch.optim.Adamax after 2 steps -- and the same 5.385e-5 between
    torch.optim.Adamax and itself with ONE parameter element moved by one ulp after the first step.  That is the solver's
    sensitivity, not an optimizer's error, and it would hide one; the fixed grid does not have it.
    Then the checkpoint helpers round-trip the optimizer state through torch.optim.Adamax, and decay_learning_rate(opt, 0.99, lr / 10)
    makes the next update 0.99 of what it would have been, gradients held fixed: to the rounding of lr / (1 - b1^t) to fp32 (2^-23
    relative, on either side) and of each parameter (half an ulp, on either side)."""
    from ode_rl_amd import train
    model, batch = _model_and_batch(cuda)
    ma, mb = model(), model()
    lr = 2e-3
    oa, ob = FusedAdamax(ma.parameters(), lr=lr), torch.optim.Adamax(mb.parameters(), lr=lr, foreach=False)
    for _ in range(2):
        _, _, _, lda = train.train_batch(ma, batch, oa, clip=1e-3)
        _, _, _, ldb = train.train_batch(mb, batch, ob, clip=1e-3)
        assert sorted(lda) == ["Gradient Norm", "Per Step Loss"] and lda["Gradient Norm"].is_cuda
        assert float(oa.last_grad_norm) > 1e-3 and float(lda["Gradient Norm"]) <= 1e-3 * (1 + 2.0 ** -22)
        assert float(lda["Gradient Norm"]) == pytest.approx(float(ldb["Gradient Norm"]), rel=1e-5)
    err = record("adamax_train_batch_param_err", _rel_max(list(ma.parameters()), list(mb.parameters())))
    print(f"train_batch, 2 clipped steps: parameters {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    moved = _rel_max(list(ma.parameters()), list(model().parameters()))
    assert moved > 100 * bound, moved      # the comparison above is of two models that did train

    # checkpoint: FusedAdamax -> pickle -> torch.optim.Adamax -> pickle -> FusedAdamax, then both continue with the same bits
    path = train.save_model_params(ma, oa, epoch=0, step=2, logdir=str(tmp_path), ckpt_id="adamax")
    mt = model()
    ot = torch.optim.Adamax(mt.parameters(), lr=1.0)
    assert train.load_model_params(mt, path, ot) == (0, 2) and ot.param_groups[0]["lr"] == lr
    assert all(sorted(s) == ["exp_avg", "exp_inf", "step"] and int(s["step"]) == 2 for s in ot.state.values())
    path = train.save_model_params(mt, ot, epoch=0, step=3, logdir=str(tmp_path), ckpt_id="adamax")
    mc = model()
    oc = FusedAdamax(mc.parameters(), lr=1.0)
    train.load_model_params(mc, path, oc)
    for p, q in zip(ma.parameters(), mc.parameters()):
        assert torch.equal(p, q) and torch.equal(oa.state[p]["exp_avg"], oc.state[q]["exp_avg"])
        assert torch.equal(oa.state[p]["exp_inf"], oc.state[q]["exp_inf"]) and int(oc.state[q]["step"]) == 2
        q.grad = p.grad.clone()

    # the same third step from the same state and gradients, once at lr (ma) and once at the decayed lr (mc)
    assert decay_learning_rate(oc, 0.99, lr / 10) == [lr * 0.99]
    start = [p.detach().double().clone() for p in ma.parameters()]
    oa.step()
    oc.step()
    num = den = 0.0
    for p0, p, q in zip(start, ma.parameters(), mc.parameters()):
        full, decayed = p0 - p.detach().double(), p0 - q.detach().double()
        tol = 2.0 ** -23 * (p.detach().double().abs() + q.detach().double().abs()) / 2 + 2.0 ** -22 * full.abs()
        assert bool(((decayed - 0.99 * full).abs() <= tol).all())
        num, den = num + float(decayed.abs().sum()), den + float(full.abs().sum())
    assert den > 0 and num / den == pytest.approx(0.99, rel=1e-5)
    # and `lowest` holds: from 10 % above it one decay of 0.5 stops there
    oc.param_groups[0]["lr"] = 1.1 * lr / 10
    assert decay_learning_rate(oc, 0.5, lr / 10) == [lr / 10]
