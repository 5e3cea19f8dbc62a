"""The host step hint of the ODE-ConvGRU encoder, host side (no GPU): `hip_ops.observed_steps` reads off a HOST mask which frames any
sample observed (a frame nobody observed launches nothing of the cell, tests/test_hip_encoder_steps.py), `hip_ops.encoder_steps` is
the `steps=` keyword of the encoder calls.  Both are pure host code; the refusals come before any library call."""
import numpy as np
import pytest
import torch

import _mask_ref
from ode_rl_amd import hip_ops

M = [[1.0, 0.0, 0.0, 1.0, 0.0],      # column 1: observed by sample 1 only; column 2: by nobody; column 4: by nobody
     [0.0, 1.0, 0.0, 1.0, 0.0]]
COLUMNS = [1, 1, 0, 1, 0]


def _is_hint(h, want):
    assert isinstance(h, np.ndarray) and h.dtype == np.uint8 and h.shape == (len(want),) and h.flags["C_CONTIGUOUS"]
    assert h.tolist() == want
    return True


@pytest.mark.parametrize("dtype", [torch.float32, torch.bool, torch.uint8, torch.int64, torch.float64, torch.float16])
@pytest.mark.parametrize("trailing", [False, True], ids=["(B,T)", "(B,T,1)"])
def test_a_byte_is_one_iff_any_sample_observed_the_frame(dtype, trailing):
    m = torch.tensor(M).to(dtype)
    m = m.unsqueeze(-1) if trailing else m
    assert _is_hint(hip_ops.observed_steps(m, 5, 2), COLUMNS)
    # the hint is the column test of the image the library reads (encoder_mask), whatever the dtype
    image = hip_ops.encoder_mask(m, 5, 2, torch.device("cpu"))
    assert hip_ops.observed_steps(m, 5, 2).tolist() == (image != 0).any(dim=1).to(torch.uint8).tolist()


def test_fractional_values_count_and_negative_zero_does_not():
    m = torch.tensor([[1.0, 0.25, -0.0, 0.0], [0.5, 0.0, 0.0, -0.0]])
    assert _is_hint(hip_ops.observed_steps(m, 4, 2), [1, 1, 0, 0])
    assert _is_hint(hip_ops.observed_steps(torch.tensor([[1e-30, -1.0, 0.0]]), 3, 1), [1, 1, 0])
    assert _is_hint(hip_ops.observed_steps(torch.zeros(3, 2), 2, 3), [0, 0])
    assert _is_hint(hip_ops.observed_steps(torch.ones(3, 2, 1), 2, 3), [1, 1])


def test_no_mask_and_a_mask_that_is_not_on_the_host_give_no_hint():
    assert hip_ops.observed_steps(None, 3, 2) is None
    # a tensor without storage stands in for a device tensor: whatever is not on the host is not looked at, let alone read back
    assert hip_ops.observed_steps(torch.zeros(2, 3, device="meta"), 3, 2) is None
    assert hip_ops.encoder_steps(None, torch.zeros(2, 3, device="meta"), 3, 2) is None
    assert hip_ops.encoder_steps(None, None, 3, 2) is None


def test_a_mask_that_requires_grad_is_left_to_the_mask_check():
    assert _is_hint(hip_ops.observed_steps(torch.tensor([[1.0, 0.0]], requires_grad=True), 2, 1), [1, 0])


def test_bad_masks_are_refused_as_encoder_mask_refuses_them():
    for bad in (torch.ones(3, 2), torch.ones(2, 3, 2), torch.ones(2, 4), torch.ones(6), torch.ones(2, 3, 1, 1)):
        with pytest.raises(ValueError, match=r"mask must be \(B, T\) = \(2, 3\)"):
            hip_ops.observed_steps(bad, 3, 2)
    with pytest.raises(TypeError, match="mask must be a torch.Tensor"):
        hip_ops.observed_steps([[1, 0, 1], [1, 1, 1]], 3, 2)
    with pytest.raises(TypeError, match="real or boolean"):
        hip_ops.observed_steps(torch.ones(2, 3, dtype=torch.complex64), 3, 2)


def test_the_steps_keyword():
    m = torch.tensor(M)
    assert _is_hint(hip_ops.encoder_steps(None, m, 5, 2), COLUMNS)           # the default: derived from the host mask
    assert hip_ops.encoder_steps(False, m, 5, 2) is None                     # switched off: the derivation is not applied
    assert hip_ops.encoder_steps(False, None, 5, 2) is None
    # an explicit hint, in any host form, with a host mask, a mask elsewhere or none; it is taken as given, not combined with the mask
    for given in ([True, False, True, True, False], (1, 0, 1, 1, 0), np.array([1, 0, 2, 1, 0]), torch.tensor([1.0, 0.0, 0.5, 1.0, 0.0]),
                  torch.tensor([True, False, True, True, False])):
        for mask in (m, torch.zeros(2, 5, device="meta"), None):
            assert _is_hint(hip_ops.encoder_steps(given, mask, 5, 2), [1, 0, 1, 1, 0])


def test_bad_steps_are_refused():
    m = torch.tensor(M)
    for bad in ([1, 0, 1], [1] * 6, [], [[1, 0, 1, 1, 0]], np.ones((5, 1)), torch.ones(4)):
        with pytest.raises(ValueError, match=r"steps must be a sequence of T = 5 booleans"):
            hip_ops.encoder_steps(bad, m, 5, 2)
    with pytest.raises(TypeError, match="would have to be read back"):
        hip_ops.encoder_steps(torch.ones(5, device="meta"), m, 5, 2)


@pytest.fixture
def no_library(monkeypatch):
    """Any library call fails the test: the refusals below are the Python layer's own."""
    from ode_rl_amd import _lib

    def load():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("grad", [False, True], ids=["inference", "autograd"])
def test_the_modules_refuse_bad_steps_before_any_library_call(no_library, grad):
    enc = _mask_ref.build(32)
    x, t = torch.randn(3, 2, 32, 16, 16, generator=torch.Generator().manual_seed(5)) * 0.5, torch.arange(3, dtype=torch.float64) / 8
    mask = torch.tensor([[1.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    calls = [lambda s: enc(x, t, mask, steps=s), lambda s: enc.run_ode_conv_gru(x, t, run_backwards=False, mask=mask, steps=s),
             lambda s: enc(x, t, None, steps=s)]
    with torch.set_grad_enabled(grad):
        for call in calls:
            with pytest.raises(ValueError, match=r"steps must be a sequence of T = 3 booleans"):
                call([1, 0])
            with pytest.raises(TypeError, match="would have to be read back"):
                call(torch.ones(3, device="meta"))
            for good in (None, False, [1, 0, 1], torch.tensor([True, False, False])):   # past the checks: next, where the frames live
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call(good)


def test_the_upstream_encoder_takes_the_keyword_too(no_library):
    import inspect
    from ode_rl_amd.models import conv_odegru
    from ode_rl_amd import autograd
    for fn in (conv_odegru.Encoder_z0_ODE_ConvGRU.forward, conv_odegru.Encoder_z0_ODE_ConvGRU.run_ode_conv_gru, hip_ops.odeconvgru_encode,
               hip_ops.odeconvgru_encode_train, autograd.encode_with_grad):
        assert inspect.signature(fn).parameters["steps"].default is None, fn


def test_this_file_is_under_the_static_scan():
    import test_static
    assert __file__ in [p for p in test_static.python_files()]
    assert test_static.undefined_names(__file__) == []
