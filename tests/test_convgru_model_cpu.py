"""The ConvGRU baseline without a GPU: the harness has the reference's state_dict (fixture convgru_model.npz, written by
tests/golden/make_golden_convgru.py from the reference's own class), depth > 1 is refused, CPU tensors are refused, and the sequence
entry points of the C ABI check their arguments before any HIP call."""
import argparse
import ctypes

import pytest
import torch

from conftest import load_golden


def _opt(**kw):
    o = dict(convgru_out_ch=64, conv_encoder_out_ch=64, in_channels=1, phase="train", train_in_seq=10, train_out_seq=10, test_in_seq=10,
             test_out_seq=190, batch_size=2, depth=1, resolution=64)
    o.update(kw)
    return argparse.Namespace(**o)


def test_state_dict_is_the_reference_s():
    from ode_rl_amd.models import ConvGRU
    g = load_golden("convgru_model.npz")
    model = ConvGRU(_opt(), torch.device("cpu"))
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"][0]) == 1272705
    for prefix in ("encoder.conv_encoders.0.0.", "encoder.conv_encoders.0.2.", "encoder.conv_gru_cells.0.conv_gates.0.",
                   "encoder.conv_gru_cells.0.conv_gates.1.", "encoder.conv_gru_cells.0.conv_can.0.", "encoder.conv_gru_cells.0.conv_can.1.",
                   "decoder.conv_gru_cells.0.conv_gates.0.", "decoder.conv_decoders.0.0.", "decoder.conv_decoders.0.2."):
        assert prefix + "weight" in sd and prefix + "bias" in sd
    assert model.decODE is False and ConvGRU(_opt(), torch.device("cpu"), decODE=True).decODE is True   # stored, ignored
    assert ConvGRU(_opt(phase="test"), torch.device("cpu")).decoder.n_frames == 190


def test_depth_above_one_is_refused():
    from ode_rl_amd.models import ConvGRU
    with pytest.raises(NotImplementedError, match="depth"):
        ConvGRU(_opt(depth=2), torch.device("cpu"))


def test_no_cpu_fallback():
    import ode_rl_amd
    from ode_rl_amd.models import ConvGRU
    model = ConvGRU(_opt(), torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(2, 10, 1, 64, 64))
    cell = ode_rl_amd.ConvGRUCell((16, 16), 64, 64, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cell.rollout(None, torch.zeros(2, 64, 16, 16), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cell.rollout(torch.zeros(3, 2, 64, 16, 16), None, 3)
    with pytest.raises(ValueError, match="both None"):
        cell.rollout(None, None, 3)


def test_sequence_argument_errors_without_gpu():
    """Every check answers ODEHIP_EINVAL before any HIP call, so it is checkable here."""
    import ode_rl_amd
    L = ode_rl_amd._lib
    lib = L.load()
    p = ctypes.c_void_p(256)   # never dereferenced: the checks come first
    good = L.ConvGRUCellDesc(input=64, hidden=64, ks=5, b_gates=256, gn_gates_w=256, gn_gates_b=256, b_can=256, gn_can_w=256,
                             gn_can_b=256, w_gates_wino=256, w_can_wino=256)
    halves = L.ConvGRUCellHalves()
    for j in range(4):
        halves.wino[j] = 256
    hv = ctypes.byref(halves)
    bw, gr = L.ConvGRUCellBwd(), L.ConvGRUCellGrads()

    def calls(desc, x, h, t, b):
        d = ctypes.byref(desc) if desc is not None else None
        yield lib.odehip_convgru_sequence_forward(d, hv, x, h, t, b, p, p, 1 << 40, None)
        yield lib.odehip_convgru_sequence_train(d, hv, x, h, t, b, p, p, 1 << 40, None)
        yield lib.odehip_convgru_sequence_backward(d, hv, ctypes.byref(bw), int(x is not None), int(h is not None), t, b, p, p, p, ctypes.byref(gr),
                                                   p, 1 << 40, None)

    def expect(desc, x, h, t, b, word):
        for rc in calls(desc, x, h, t, b):
            assert rc == -1 and word in lib.odehip_last_error(), lib.odehip_last_error()

    expect(None, p, p, 4, 2, b"null cell")
    expect(good, p, p, 0, 2, b"n_steps")
    expect(good, p, p, 4, 0, b"batch")
    expect(good, None, None, 4, 2, b"both NULL")
    for field, value in (("ks", 3), ("input", 12), ("hidden", 48)):
        bad = L.ConvGRUCellDesc.from_buffer_copy(good)
        setattr(bad, field, value)
        expect(bad, p, p, 4, 2, b"F(2x2,5x5)")
    narrow = L.ConvGRUCellDesc.from_buffer_copy(good)   # the forward serves 32 / 32; the training path needs multiples of 64
    narrow.input = narrow.hidden = 32
    assert lib.odehip_convgru_sequence_train(ctypes.byref(narrow), hv, p, p, 4, 2, p, p, 1 << 40, None) == -1
    assert b"multiples of 64" in lib.odehip_last_error()
    assert lib.odehip_convgru_sequence_forward(ctypes.byref(good), None, p, p, 4, 2, p, p, 1 << 40, None) == -1
    assert b"null weight-halves" in lib.odehip_last_error()
    nohalf = L.ConvGRUCellHalves.from_buffer_copy(halves)
    nohalf.wino[1] = None
    assert lib.odehip_convgru_sequence_forward(ctypes.byref(good), ctypes.byref(nohalf), None, p, 4, 2, p, p, 1 << 40, None) == -1
    assert b"state-half" in lib.odehip_last_error()
    assert lib.odehip_convgru_sequence_workspace_bytes(None, 4, 2, 1, 0) == 0
    assert lib.odehip_convgru_sequence_workspace_bytes(ctypes.byref(good), 0, 2, 1, 0) == 0
    fwd = lib.odehip_convgru_sequence_workspace_bytes(ctypes.byref(good), 190, 4, 0, 0)
    assert fwd == 7 * 4 * 64 * 256 * 4            # two states + gates (2) + z + r*h + cand, whatever the number of steps
    per_step = (lib.odehip_convgru_sequence_workspace_bytes(ctypes.byref(good), 11, 64, 0, 1) -
                lib.odehip_convgru_sequence_workspace_bytes(ctypes.byref(good), 10, 64, 0, 1))
    assert 40 * (1 << 20) <= per_step <= 41 * (1 << 20)   # 10 state-sized tensors per step (+ partials and table entries)
    with pytest.raises(ValueError):
        L.check(-1)
