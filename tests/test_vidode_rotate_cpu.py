"""The host side of the rotation of ode_rl_amd.vidode_data (`VidODEBatches(rotate=)`) and the restatement the
GPU tests compare against (tests/_rotate_ref.py).  The restatement is pinned to scipy.ndimage.map_coordinates (bilinear, zeros outside)
where the clip rule is idle, the clip rule is checked on its own, angle 0 must be the pixel table and angle 90 `np.rot90`; the iterator
must make upstream's random calls in upstream's order (sampling, flip, angle).  No GPU: nothing is rendered."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch
from scipy import ndimage

import _rotate_ref as rot

ANGLES = [0.0, 90.0, 180.0, -10.0, 7.3, 45.0]
SHAPES = [(16, 16, 1), (12, 10, 3)]


def _frame(shape, seed, low=0):
    f = np.random.RandomState(seed).randint(low, 256, size=shape).astype(np.uint8)
    f[shape[0] // 2, shape[1] // 3, 0] = low          # the minimum is attained
    return f


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("angle", ANGLES)
def test_restatement_is_bilinear_sampling_with_zeros_outside(shape, angle):
    frame = _frame(shape, 11)
    assert frame.min() == 0                            # the clip rule is idle
    sy, sx = rot.source_coordinates(shape[0], shape[1], angle)
    want = np.stack([ndimage.map_coordinates(frame[..., c].astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0)
                     for c in range(shape[2])], axis=-1)
    got = rot.rotate(frame, angle)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-9


def test_clip_lifts_blended_values_to_the_frames_minimum_and_keeps_exact_zeros():
    frame = _frame((12, 10, 3), 12, low=7)
    assert frame.min() == 7
    sy, sx = rot.source_coordinates(12, 10, 30.0)
    plain = np.stack([ndimage.map_coordinates(frame[..., c].astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0)
                      for c in range(3)], axis=-1)
    got = rot.rotate(frame, 30.0)
    far = (sx <= -1) | (sx >= 10) | (sy <= -1) | (sy >= 12)      # all four sources outside the frame
    blended = (plain > 1e-9) & (plain < 7)
    assert far.any() and blended.any() and (plain >= 7).any()
    assert (got[far] == 0).all() and (got[~far] >= 7).all()
    assert (got[blended] == 7).all()
    assert np.abs(got - plain)[plain >= 7].max() <= 1e-9
    assert got.max() <= 255


@pytest.mark.parametrize("input_norm", [True, False])
@pytest.mark.parametrize("low", [0, 7])
def test_angle_zero_is_the_pixel_table(input_norm, low):
    from ode_rl_amd import vidode_data
    frame = _frame((12, 10, 3), 13, low=low)
    got = rot.to_tensor(rot.rotate(frame, 0.0), input_norm)
    want = vidode_data.pixel_table(input_norm)[torch.from_numpy(frame).long()].permute(2, 0, 1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("channels", [1, 3])
def test_angle_ninety_is_rot90(channels):
    frame = _frame((16, 16, channels), 14)
    assert np.abs(rot.rotate(frame, 90.0) - np.rot90(frame)).max() <= 1e-9


def test_float32_restatement_is_the_same_formula():
    frame = _frame((12, 10, 3), 15)
    v32, v64 = rot.rotate(frame, 7.3, np.float32), rot.rotate(frame, 7.3)
    assert v32.dtype == np.float32 and 0 < np.abs(v32 - v64).max() <= 1e-2


def _store_and_opt(irregular):
    from ode_rl_amd import vidode_data
    rng = np.random.RandomState(3)
    clips = [rng.randint(0, 256, size=(n, 6, 8, 1)).astype(np.uint8) for n in (12, 16, 20)]
    opt = types.SimpleNamespace(window_size=8, sample_size=6, irregular=irregular, extrap=not irregular, batch_size=3, input_norm=True)
    return vidode_data, vidode_data.ClipStore(clips, device="cpu"), opt


@pytest.mark.parametrize("irregular", [False, True])
def test_draw_makes_upstreams_random_calls_in_upstreams_order(irregular):
    """Per item: the sampling calls, then RandomHorizontalFlip's `random.random()`, then RandomRotation's `random.uniform(-10, 10)`."""
    vd, store, opt = _store_and_opt(irregular)
    it = vd.VidODEBatches(opt, store, train=True, hflip=True, rotate=10)
    clips = [2, 0, 1]
    random.seed(21)
    np.random.seed(22)
    plan = it.draw(clips=clips)
    after = (random.random(), np.random.rand())
    random.seed(21)
    np.random.seed(22)
    starts, flips, angles = [], [], []
    for c in clips:
        n = int(store.lengths[c])
        if irregular:       # Dataset_base.sampling, irregular interpolation: the window, then the picks between its ends
            start = random.randint(0, n - 9)
            np.random.choice(list(range(start + 1, start + 7)), size=4, replace=False)
        else:               # regular extrapolation
            start = random.randint(0, n - 6)
        starts.append(start)
        flips.append(random.random() < 0.5)
        angles.append(random.uniform(-10, 10))
    assert plan["rel"][:, 0].tolist() == starts and plan["flip"].tolist() == flips
    assert plan["angle"].dtype == np.float64 and plan["angle"].tolist() == angles
    assert after == (random.random(), np.random.rand())
    assert True in flips and False in flips and len(set(angles)) == 3 and all(-10 <= a <= 10 for a in angles)


def test_without_rotate_the_random_stream_is_untouched():
    vd, store, opt = _store_and_opt(False)
    random.seed(5)
    np.random.seed(5)
    plain = vd.VidODEBatches(opt, store, hflip=True).draw(clips=[0, 1, 2])
    after = random.random()
    random.seed(5)
    np.random.seed(5)
    by_hand = []
    for n in store.lengths:
        by_hand.append((random.randint(0, int(n) - 6), random.random() < 0.5))
    assert after == random.random()
    assert [(int(r), bool(f)) for r, f in zip(plain["rel"][:, 0], plain["flip"])] == by_hand
    assert plain["angle"].tolist() == [0.0, 0.0, 0.0]
    random.seed(5)
    np.random.seed(5)
    turned = vd.VidODEBatches(opt, store, hflip=True, rotate=(2.0, 3.0)).draw(clips=[0, 1, 2])
    assert all(2.0 <= a <= 3.0 for a in turned["angle"]) and not np.array_equal(turned["rel"], plain["rel"])


def test_rotate_argument():
    vd, store, opt = _store_and_opt(False)
    assert vd.VidODEBatches(opt, store).rotate is None
    assert vd.VidODEBatches(opt, store, rotate=10).rotate == (-10.0, 10.0)
    assert vd.VidODEBatches(opt, store, rotate=(-3, 5.5)).rotate == (-3.0, 5.5)
    with pytest.raises(ValueError, match="positive"):
        vd.VidODEBatches(opt, store, rotate=-1)
    with pytest.raises(ValueError, match="len 2"):
        vd.VidODEBatches(opt, store, rotate=(1, 2, 3))
    with pytest.raises(NotImplementedError, match=r"RandomRotation.*rotate="):
        vd.RandomRotation(10)
    it = vd.VidODEBatches(opt, store, rotate=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(it)


def test_the_store_keeps_each_frames_minimum():
    vd, store, _ = _store_and_opt(False)
    assert store.frame_min.dtype == torch.uint8 and store.frame_min.device == store.data.device
    assert torch.equal(store.frame_min, torch.from_numpy(store.data.numpy().reshape(store.n_frames, -1).min(axis=1)))
    rgb = vd.ClipStore([np.random.RandomState(1).randint(9, 256, size=(4, 5, 6, 3)).astype(np.uint8)], device="cpu")
    assert rgb.frame_min.shape == (4,) and int(rgb.frame_min.min()) >= 9


def test_c_abi_argument_errors_without_gpu():
    """`odehip_vidode_batch_rotated` checks its arguments before any HIP call."""
    from ode_rl_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    outs, nf = (ctypes.c_void_p * 1)(4096), (ctypes.c_int * 1)(2)

    def call(store=p, frames=10, h=8, w=8, c=1, fmin=p, norm=1, table=p, words=5 * 3 + 2 * 3 * 2, batch=3, n_out=1, outs=outs, nf=nf):
        return lib.odehip_vidode_batch_rotated(store, frames, h, w, c, fmin, norm, table, words, batch, n_out, outs, nf, None)

    for kwargs, text in [(dict(store=None), b"null"), (dict(fmin=None), b"null"), (dict(table=None), b"null"), (dict(c=2), b"1 or 3 channels"),
                         (dict(frames=0), b"frames"), (dict(w=0), b"frame size"), (dict(batch=0), b"batch"), (dict(n_out=4), b"outputs"),
                         (dict(words=26), b"the table has 26 words, these shapes need 27"),
                         (dict(words=15), b"the table has 15 words, these shapes need 27"),     # the unrotated launch's count
                         (dict(table=ctypes.c_void_p(4100)), b"8-byte aligned"), (dict(outs=(ctypes.c_void_p * 1)(4104)), b"16-byte aligned"),
                         (dict(nf=(ctypes.c_int * 1)(0)), b"no frames"), (dict(h=70000, w=1024), b"too large")]:
        assert call(**kwargs) == -1 and text in lib.odehip_last_error(), (kwargs, lib.odehip_last_error())
        assert b"vidode_batch_rotated" in lib.odehip_last_error()
