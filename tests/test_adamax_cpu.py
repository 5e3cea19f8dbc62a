"""FusedAdamax and decay_learning_rate (Vid-ODE's optimizer and its per-epoch decay, Vid-ODE/main.py:187,214), the parts a CPU can
check: argument validation, the decay's arithmetic, state dicts going to torch.optim.Adamax and back, and the refusal of CPU tensors.
The arithmetic of the kernels is tests/test_hip_adamax.py's business."""
import copy
import ctypes

import pytest
import torch

from ode_rl_amd.optim import FusedAdamax, decay_learning_rate


def _params(n=3):
    g = torch.Generator().manual_seed(n)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(4, 3), (5,), (1,)][:n]]


def test_defaults_are_torchs():
    ours, torchs = FusedAdamax(_params()), torch.optim.Adamax(_params())
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert ours.defaults[k] == torchs.defaults[k], k
    assert ours.defaults["max_grad_norm"] is None and ours.last_grad_norm is None and ours.last_clipped_norm is None


@pytest.mark.parametrize("bad", [dict(lr=-1e-3), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(-0.1, 0.999)),
                                 dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1), dict(max_grad_norm=-2.0),
                                 dict(max_grad_norm=float("nan"))])
def test_invalid_hyper_parameters_raise(bad):
    with pytest.raises(ValueError):
        FusedAdamax(_params(), **bad)


@pytest.mark.parametrize("name", ["maximize", "foreach", "differentiable", "capturable"])
def test_torch_options_without_an_implementation_are_refused(name):
    for value in (True, False):      # refused by name: a False that is accepted today becomes a True that is ignored tomorrow
        with pytest.raises((TypeError, ValueError), match=name):
            FusedAdamax(_params(), **{name: value})


@pytest.mark.parametrize("name", ["maximize", "differentiable", "capturable"])
def test_a_state_dict_that_switches_such_an_option_on_does_not_load(name):
    sd = torch.optim.Adamax(_params()).state_dict()
    sd["param_groups"][0][name] = True
    opt = FusedAdamax(_params(), lr=0.5)
    with pytest.raises(ValueError, match=name):
        opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 0.5      # refused before anything was taken over


def test_decay_learning_rate_is_the_references_expression():
    ps = _params()
    opt = FusedAdamax([{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:2], "lr": 2e-3}, {"params": ps[2:]}], lr=1.5e-3)
    want = [1e-2, 2e-3, 1.5e-3]
    for _ in range(80):
        want = [max(lr * 0.99, 1e-3) for lr in want]
        got = decay_learning_rate(opt, 0.99, 1e-3)
        assert got == want == [g["lr"] for g in opt.param_groups]
    assert want[1] == want[2] == 1e-3 and 1e-3 < want[0] < 1e-2      # two groups have stopped at `lowest`, one is still on its way
    for _ in range(200):
        decay_learning_rate(opt, 0.99, 1e-3)
    assert [g["lr"] for g in opt.param_groups] == [1e-3] * 3
    # the reference's defaults, and any torch optimizer
    sgd = torch.optim.SGD(_params(), lr=0.1)
    assert decay_learning_rate(sgd) == [0.1 * 0.999] and sgd.param_groups[0]["lr"] == 0.1 * 0.999
    sgd.param_groups[0]["lr"] = 1.0005e-3
    assert decay_learning_rate(sgd) == [1e-3]


def _stepped_torch_adamax(ps):
    opt = torch.optim.Adamax(ps, lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    g = torch.Generator().manual_seed(9)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_state_dicts_go_to_torch_adamax_and_back():
    a = _params()
    torchs = _stepped_torch_adamax(a)
    sd = copy.deepcopy(torchs.state_dict())
    ours = FusedAdamax([torch.nn.Parameter(p.detach().clone()) for p in a])
    ours.load_state_dict(copy.deepcopy(sd))
    group = ours.param_groups[0]
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"]) == (3e-3, (0.8, 0.99), 1e-7, 0.01)
    assert group["max_grad_norm"] is None      # torch's state has no such key: clipping is off
    for p, q in zip(ours.param_groups[0]["params"], a):
        st = ours.state[p]
        assert sorted(st) == ["exp_avg", "exp_inf", "step"] and int(st["step"]) == 2
        assert torch.equal(st["exp_avg"], torchs.state[q]["exp_avg"]) and torch.equal(st["exp_inf"], torchs.state[q]["exp_inf"])
    # and back, with a clipping bound set on the way: torch carries the key along and steps on
    group["max_grad_norm"] = 0.5
    back = ours.state_dict()
    assert all(sorted(s) == ["exp_avg", "exp_inf", "step"] for s in back["state"].values())
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    again = torch.optim.Adamax(b)
    again.load_state_dict(copy.deepcopy(back))
    assert again.param_groups[0]["max_grad_norm"] == 0.5 and again.param_groups[0]["lr"] == 3e-3
    for p, q in zip(a, b):
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    torchs.step()
    again.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q) and int(again.state[q]["step"]) == 3
    # a FusedAdamax state dict loads into a fresh FusedAdamax with its bound
    fresh = FusedAdamax(_params())
    fresh.load_state_dict(copy.deepcopy(back))
    assert fresh.param_groups[0]["max_grad_norm"] == 0.5


def test_a_cpu_parameter_is_refused_not_updated():
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    opt = FusedAdamax(ps)
    for kw in ({}, {"max_grad_norm": 0.5}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step(**kw)
    for p, q in zip(ps, before):
        assert torch.equal(p, q)


def test_groups_must_share_their_bound():
    ps = _params()
    opt = FusedAdamax([{"params": ps[:1], "max_grad_norm": 0.5}, {"params": ps[1:]}])
    with pytest.raises(ValueError, match="FusedAdamax.*share max_grad_norm"):
        opt.step()


def test_the_package_exports_both_names():
    import ode_rl_amd
    assert ode_rl_amd.FusedAdamax is FusedAdamax and ode_rl_amd.decay_learning_rate is decay_learning_rate
    assert ode_rl_amd.optim.FusedAdam.__mro__[1] is FusedAdamax.__mro__[1]      # one step implementation for both


def test_c_abi_checks_its_arguments_before_any_launch():
    """null pointers and step < 1 are refused before any HIP call, so a machine without a GPU can ask"""
    from ode_rl_amd import _lib
    lib = _lib.load()
    some, none = (ctypes.c_void_p * 1)(16), (ctypes.c_void_p * 1)(None)
    numel = (ctypes.c_longlong * 1)(4)
    hyper = (2e-3, 0.9, 0.999, 1e-8, 0.0)
    for fn, tail in ((lib.odehip_adamax_step, (None,)), (lib.odehip_adamax_step_clipped, (ctypes.c_void_p(16), None))):
        for k in range(4):
            arrs = [None if i == k else some for i in range(4)]
            assert fn(*arrs, numel, 1, *hyper, 1, *tail) == -1 and b"null pointer" in lib.odehip_last_error()
            arrs = [none if i == k else some for i in range(4)]
            assert fn(*arrs, numel, 1, *hyper, 1, *tail) == -1 and b"tensor 0 has a null pointer" in lib.odehip_last_error()
        assert fn(some, some, some, some, None, 1, *hyper, 1, *tail) == -1 and b"null pointer" in lib.odehip_last_error()
        for step in (0, -3):
            assert fn(some, some, some, some, numel, 1, *hyper, step, *tail) == -1 and b"counts from 1" in lib.odehip_last_error()
    assert lib.odehip_adamax_step_clipped(some, some, some, some, numel, 1, *hyper, 1, None, None) == -1
    assert b"null pointer" in lib.odehip_last_error()
    with pytest.raises(ValueError, match="adamax_step_clipped"):
        _lib.check(-1)
