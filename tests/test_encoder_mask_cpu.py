"""The observation mask of the ODE-ConvGRU encoder, host side (no GPU): the CPU restatement the GPU tests compare against
(tests/_mask_ref.py) at its two fixed points, and the refusals of the Python layer, which come before any library call."""
import pytest
import torch

import _mask_ref


def _case(ch=32, T=3, B=2, seed=5):
    enc = _mask_ref.build(ch)
    g = torch.Generator().manual_seed(seed)
    return enc, torch.randn(T, B, ch, 16, 16, generator=g) * 0.5, torch.arange(T, dtype=torch.float64) / 8


@pytest.mark.parametrize("run_backwards", [True, False])
def test_all_ones_mask_is_the_unmasked_oracle_exactly(run_backwards):
    from oracle import reference_modules as rm
    enc, x, t = _case()
    parts = _mask_ref.split_state({k: v.detach() for k, v in enc.state_dict().items()})
    with torch.no_grad():
        want = rm.ode_convgru_encode(x, t, *parts, run_backwards=run_backwards)
        got = _mask_ref.encode(x, t, *parts, torch.ones(2, 3), run_backwards)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("run_backwards", [True, False])
def test_all_zeros_mask_leaves_the_pure_euler_chain_from_the_zero_state(run_backwards):
    enc, x, t = _case()
    f_enc, cell, head = _mask_ref.split_state({k: v.detach() for k, v in enc.state_dict().items()})
    with torch.no_grad():
        _, _, latent = _mask_ref.encode(x, t, f_enc, cell, head, torch.zeros(2, 3), run_backwards)
        h = torch.zeros(2, 32, 16, 16)
        prev_t, t_i = t[-1] + 0.01, t[-1]
        for k, i in enumerate(reversed(range(3)) if run_backwards else range(3)):
            h = h + f_enc(prev_t, h) * (t_i - prev_t)
            prev_t, t_i = t[i], t[i - 1]
            assert torch.equal(latent[:, k], h)
    assert float(latent.abs().max()) > 0      # (the dynamics have biases: the chain leaves zero)


@pytest.fixture
def no_library(monkeypatch):
    """Any library call fails the test: the refusals below are the Python layer's own."""
    from ode_rl_amd import _lib

    def load():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("grad", [False, True], ids=["inference", "autograd"])
def test_bad_masks_are_refused_before_any_library_call(no_library, grad):
    enc, x, t = _case()            # T = 3, B = 2
    calls = [lambda m: enc(x, t, m), lambda m: enc.run_ode_conv_gru(x, t, run_backwards=False, mask=m)]
    with torch.set_grad_enabled(grad):
        for call in calls:
            for bad in (torch.ones(3, 2), torch.ones(2, 3, 2), torch.ones(2, 4), torch.ones(6), torch.ones(2, 3, 1, 1)):
                with pytest.raises(ValueError, match=r"mask must be \(B, T\) = \(2, 3\)"):
                    call(bad)
            with pytest.raises(TypeError, match="mask must be a torch.Tensor"):
                call([[1, 0, 1], [1, 1, 1]])
            with pytest.raises(TypeError, match="real or boolean"):
                call(torch.ones(2, 3, dtype=torch.complex64))
            with pytest.raises(NotImplementedError, match="mask is treated as a constant; a gradient with respect to it is not implemented"):
                call(torch.ones(2, 3, requires_grad=True))
            # a good mask of any accepted form gets past the mask checks: the next thing looked at is where the frames live
            for good in (torch.ones(2, 3), torch.ones(2, 3, 1, dtype=torch.bool), torch.ones(2, 3, dtype=torch.uint8), None):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call(good)


def test_the_library_image_of_a_mask():
    """(T, B) float32 contiguous; float32 values kept, every other dtype read as mask != 0; (B, T, 1) accepted."""
    from ode_rl_amd import hip_ops
    m = torch.tensor([[1.0, 0.25, 0.0], [0.0, 1.0, 1.0]])
    got = hip_ops.encoder_mask(m, 3, 2, torch.device("cpu"))
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, m.t())
    want = (m != 0).float().t()
    for other in (m != 0, (m * 4).to(torch.uint8), (m * 4).to(torch.int64), m.double(), m.half(), (m != 0).unsqueeze(-1)):
        assert torch.equal(hip_ops.encoder_mask(other, 3, 2, torch.device("cpu")), want)
    assert hip_ops.encoder_mask(None, 3, 2, torch.device("cpu")) is None
