"""train_batch(async_solver=True) when the asynchronous pass fails (ode_rl_amd/train.py; host logic only: a stub model on the CPU,
no library call).  Whatever the pass raises -- a sealed solve (AsyncSolveTruncated), a failed one (AssertionError at the backward pass,
after NaN frames reached a BatchNorm), anything else -- the module buffers are restored to their values of before the pass and the
parameters and the optimiser are untouched.  A sealed pass is repeated on the synchronous path whatever the caller's setting; any other
error is re-raised, and an error from collecting the still-pending solves on the way out never replaces it."""
import pytest
import torch


class _Failing(torch.autograd.Function):
    """Identity whose backward raises `exc` -- what the backward pass of a failed asynchronous solve does at its collect."""

    @staticmethod
    def forward(ctx, v, exc):
        ctx.exc = exc
        return v.clone()

    @staticmethod
    def backward(ctx, g):
        raise ctx.exc


class _Stub(torch.nn.Module):
    """get_prediction fails the first `n_fail` calls the way a failed asynchronous solve does: NaN frames reach the BatchNorm in train
    mode (its running statistics fold them in) and the backward pass raises `exc()`."""

    def __init__(self, exc=None, n_fail=1):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.5, 3))
        self.bn = torch.nn.BatchNorm1d(3)
        self.exc, self.n_fail = exc, n_fail
        self.calls, self.async_seen = 0, []

    def get_prediction(self, inp, batch_dict=None):
        from ode_rl_amd import hip_ops
        self.calls += 1
        self.async_seen.append(hip_ops._async_dopri5)
        x = inp * self.w
        if self.exc is not None and self.calls <= self.n_fail:
            return _Failing.apply(self.bn(x * float("nan")), self.exc())
        return self.bn(x)

    def get_loss(self, pred, truth):
        return ((pred - truth) ** 2).mean()


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"observed_data": torch.randn(8, 3, generator=g), "data_to_predict": torch.randn(8, 3, generator=g)}


def _trained(exc, n_fail=1):
    """A stub model and an Adam that has taken one clean step (so that there is optimiser state to leave untouched)."""
    from ode_rl_amd.train import train_batch
    m = _Stub()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    train_batch(m, _batch(1), opt)
    m.exc, m.n_fail, m.calls, m.async_seen = exc, n_fail, 0, []
    return m, opt


def _snapshot(m, opt):
    st = opt.state[m.w]
    return ([b.detach().clone() for b in m.buffers()], m.w.detach().clone(),
            {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()})


def _assert_unchanged(m, opt, snap):
    bufs, w, st = snap
    assert [n for n, _ in m.named_buffers()] == ["bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    for b, kept in zip(m.buffers(), bufs):
        assert torch.equal(b, kept)
    assert torch.equal(m.w.detach(), w)
    now = opt.state[m.w]
    assert set(now) == set(st)
    for k, v in st.items():
        assert torch.equal(now[k], v) if torch.is_tensor(v) else now[k] == v


@pytest.mark.parametrize("caller_async", [False, True])
@pytest.mark.parametrize("exc", [lambda: AssertionError("non-finite state"), lambda: RuntimeError("anything else")],
                         ids=["solver_error", "other_error"])
def test_an_error_of_the_asynchronous_pass_restores_the_buffers_and_is_raised(monkeypatch, caller_async, exc):
    from ode_rl_amd import hip_ops
    from ode_rl_amd.train import train_batch
    monkeypatch.setattr(hip_ops, "_pending_solves", [])
    m, opt = _trained(exc)
    snap = _snapshot(m, opt)
    monkeypatch.setattr(hip_ops, "_async_dopri5", caller_async)   # True: what ODEHIP_DOPRI5_ASYNC=1 sets at import
    want = type(exc())
    with pytest.raises(want):
        train_batch(m, _batch(2), opt, async_solver=True)
    assert m.calls == 1 and m.async_seen == [True]                 # raised, not repeated
    assert hip_ops._async_dopri5 == caller_async
    _assert_unchanged(m, opt, snap)


@pytest.mark.parametrize("caller_async", [False, True])
def test_a_sealed_pass_is_repeated_synchronously_whatever_the_callers_setting(monkeypatch, caller_async):
    from ode_rl_amd import _lib, hip_ops
    from ode_rl_amd.train import train_batch
    monkeypatch.setattr(hip_ops, "_pending_solves", [])
    m, opt = _trained(lambda: _lib.AsyncSolveTruncated("sealed"))
    bufs, w, _ = _snapshot(m, opt)
    steps = int(opt.state[m.w]["step"])
    monkeypatch.setattr(hip_ops, "_async_dopri5", caller_async)
    _, _, loss, _ = train_batch(m, _batch(2), opt, async_solver=True)
    assert m.calls == 2 and m.async_seen == [True, False]
    assert hip_ops._async_dopri5 == caller_async
    assert torch.isfinite(loss)
    assert int(m.bn.num_batches_tracked) == int(bufs[2]) + 1       # one step's statistics on top of the clean ones, NaN-free
    assert torch.isfinite(m.bn.running_mean).all() and torch.isfinite(m.bn.running_var).all()
    assert int(opt.state[m.w]["step"]) == steps + 1 and not torch.equal(m.w.detach(), w)


def test_a_sealed_repeat_is_not_repeated_again(monkeypatch):
    """The repeat is synchronous, so an error there is final: it is raised, not repeated, and the caller's setting is restored."""
    from ode_rl_amd import _lib, hip_ops
    from ode_rl_amd.train import train_batch
    monkeypatch.setattr(hip_ops, "_pending_solves", [])
    m, opt = _trained(lambda: _lib.AsyncSolveTruncated("sealed"), n_fail=2)
    monkeypatch.setattr(hip_ops, "_async_dopri5", True)
    with pytest.raises(_lib.AsyncSolveTruncated):
        train_batch(m, _batch(2), opt, async_solver=True)
    assert m.calls == 2 and m.async_seen == [True, False] and hip_ops._async_dopri5 is True


@pytest.mark.parametrize("primary", [lambda: AssertionError("primary"), lambda: ValueError("primary")], ids=["assertion", "value"])
def test_an_error_from_collecting_pending_solves_does_not_replace_the_primary_one(monkeypatch, primary):
    from ode_rl_amd import hip_ops
    from ode_rl_amd.train import train_batch
    pending = []
    monkeypatch.setattr(hip_ops, "_pending_solves", pending)

    class Pending:   # a solve started in the failed pass and never collected by it: collecting it on the way out fails too
        collected = 0

        def collect(self):
            Pending.collected += 1
            pending.remove(self)
            raise RuntimeError("secondary")

    m, opt = _trained(primary)
    snap = _snapshot(m, opt)
    orig = m.get_prediction

    def get_prediction(inp, batch_dict=None):
        pending.append(Pending())
        return orig(inp, batch_dict)
    m.get_prediction = get_prediction
    monkeypatch.setattr(hip_ops, "_async_dopri5", False)
    with pytest.raises(type(primary()), match="primary"):
        train_batch(m, _batch(2), opt, async_solver=True)
    assert Pending.collected == 1 and not pending and hip_ops._async_dopri5 is False
    _assert_unchanged(m, opt, snap)
