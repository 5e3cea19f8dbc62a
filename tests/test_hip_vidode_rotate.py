"""`odehip_vidode_batch_rotated` and `VidODEBatches(rotate=)` on the GPU against the float64 NumPy restatement of upstream's
RandomRotation -> ToTensor -> Normalize chain (tests/_rotate_ref.py, pinned to scipy by tests/test_vidode_rotate_cpu.py).

Bound, the project's rule for fused kernels: the device's distance from the float64 restatement is at most
4 x the distance of the float32 restatement of the same formula on the same inputs, plus 4 * 2^-24 * max|out|.  The kernel computes
coordinates and interpolation in float64 in the restatement's own operation order, so it sits far inside: observed on an MI355X, device
error 0 in every case (float32 restatement 6e-7 to 1.1e-5), as DESIGN.md section 4.18 records.

Shapes (H, W, C): (16, 16, 1) the 16-byte path, (12, 10, 3) a non-square frame whose width is no multiple of four (guarded path with a
partial last group), (64, 64, 3) more than one workgroup per frame.  B = 3, two outputs of 2 and 3 frames, flips on for some samples,
angles {0, 90, 180} and {-10, 7.3, 45}, input_norm on and off, a store with black pixels and one whose frames have a minimum above 0
(the clip rule binds)."""
import ctypes
import functools
import random
import types

import numpy as np
import pytest
import torch

import _rotate_ref as rot

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 1), (12, 10, 3), (64, 64, 3)]
ANGLE_SETS = {"right": (0.0, 90.0, 180.0), "oblique": (-10.0, 7.3, 45.0)}
FLIP = np.array([True, False, True])
N_FRAMES = 7
FRAMES = [np.array([[0, 3], [6, 1], [2, 2]], dtype=np.int32), np.array([[1, 4, 5], [0, 6, 3], [5, 2, 4]], dtype=np.int32)]
FACTOR = [np.array([[1, 1], [0, 1], [1, 1]], dtype=np.float32), np.array([[1, 0, 1], [1, 1, 1], [1, 1, 0]], dtype=np.float32)]


@functools.lru_cache(maxsize=None)
def _frames(shape, low):
    """(N_FRAMES, H, W, C) uint8; low 0: black pixels in every frame; low > 0: every frame's minimum is above 0 and differs per frame."""
    h, w, c = shape
    px = np.random.RandomState(100 * h + w + c + low).randint(low + N_FRAMES if low else 0, 256, size=(N_FRAMES, h, w, c)).astype(np.uint8)
    for i in range(N_FRAMES):
        px[i, (3 * i) % h, (5 * i) % w, i % c] = low + (i if low else 0)     # frame i's minimum: low + i, or 0
    return px


@functools.lru_cache(maxsize=None)
def _reference(shape, low, input_norm, angles, dtype):
    return [rot.batch(_frames(shape, low), f, k, FLIP, angles, input_norm, dtype) for f, k in zip(FRAMES, FACTOR)]


def _store(shape, low, cuda):
    from ode_rl_amd import vidode_data
    px = _frames(shape, low)
    return vidode_data.ClipStore([px[:3], px[3:]], device=cuda)


def _table(flip, parts, angles=None):
    words = [np.asarray(flip).astype(np.int32)]
    if angles is not None:
        words.insert(0, np.array([rot.cos_sin(a) for a in angles], dtype=np.float64).ravel().view(np.int32))
    for frames, factor in parts:
        words += [frames.ravel().astype(np.int32), factor.ravel().astype(np.float32).view(np.int32)]
    return torch.from_numpy(np.concatenate(words))


def _launch(store, flip, parts, angles, input_norm, fill=None):
    """The C entry itself; angles None: the unrotated `odehip_vidode_batch` with the pixel table of the same input_norm."""
    from ode_rl_amd import _lib, vidode_data
    dev = store.device
    table = _table(flip, parts, angles).to(dev)
    outs = [torch.empty((len(flip), f.shape[1], store.channels, store.height, store.width), device=dev) for f, _ in parts]
    if fill is not None:
        for o in outs:
            o.fill_(fill)
    ptrs = (ctypes.c_void_p * len(parts))(*[o.data_ptr() for o in outs])
    counts = (ctypes.c_int * len(parts))(*[f.shape[1] for f, _ in parts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    if angles is None:
        lut = vidode_data.pixel_table(input_norm).to(dev)
        _lib.check(lib.odehip_vidode_batch(store.data.data_ptr(), store.n_frames, store.height, store.width, store.channels, lut.data_ptr(),
                                           table.data_ptr(), table.numel(), len(flip), len(parts), ptrs, counts, stream))
    else:
        _lib.check(lib.odehip_vidode_batch_rotated(store.data.data_ptr(), store.n_frames, store.height, store.width, store.channels,
                                                   store.frame_min.data_ptr(), int(input_norm), table.data_ptr(), table.numel(), len(flip),
                                                   len(parts), ptrs, counts, stream))
    return [o.cpu() for o in outs]


PARTS = list(zip(FRAMES, FACTOR))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("low", [0, 9])
@pytest.mark.parametrize("input_norm", [True, False])
@pytest.mark.parametrize("name", sorted(ANGLE_SETS))
def test_rotated_batch_is_within_the_bound(cuda, shape, low, input_norm, name):
    angles = ANGLE_SETS[name]
    store = _store(shape, low, cuda)
    assert int(store.frame_min.min()) == low and (low == 0 or len(set(store.frame_min.tolist())) > 1)
    got = _launch(store, FLIP, PARTS, angles, input_norm, fill=7.0)
    again = _launch(store, FLIP, PARTS, angles, input_norm)
    ref64 = _reference(shape, low, input_norm, angles, np.float64)
    ref32 = _reference(shape, low, input_norm, angles, np.float32)
    for k, (g, g2, r64, r32) in enumerate(zip(got, again, ref64, ref32)):
        assert g.shape == r64.shape and torch.isfinite(g).all()
        assert torch.equal(g, g2)                                        # two launches are bitwise equal
        err = float((g.double() - r64.double()).abs().max())
        err32 = float((r32.double() - r64.double()).abs().max())
        bound = 4 * err32 + 4 * 2.0 ** -24 * float(r64.abs().max())
        print(f"{shape} low {low} norm {input_norm} {name} output {k}: device error {err:.3e}, float32 restatement {err32:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, err32, bound)
        zero = torch.from_numpy(FACTOR[k] == 0)
        assert zero.any() and (g[zero] == 0).all() and (g[~zero] != 0).any()   # a factor 0 slot is all zeros


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("low", [0, 9])
@pytest.mark.parametrize("input_norm", [True, False])
def test_angle_zero_equals_the_unrotated_launch(cuda, shape, low, input_norm):
    store = _store(shape, low, cuda)
    plain = _launch(store, FLIP, PARTS, None, input_norm)
    turned = _launch(store, FLIP, PARTS, (0.0, 0.0, 0.0), input_norm)
    assert all(torch.equal(a, b) for a, b in zip(plain, turned))
    # and in a batch with other angles, the sample at angle 0 alone
    mixed = _launch(store, FLIP, PARTS, ANGLE_SETS["right"], input_norm)
    assert all(torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) for a, b in zip(plain, mixed))


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_right_angles_move_whole_pixels(cuda, shape):
    """90 and 180 degrees on the byte values themselves: rot90 of a square frame, the point reflection of any frame -- to the float32
    rounding of a value that the float64 interpolation leaves within 1e-9 of a byte."""
    from ode_rl_amd import vidode_data
    store = _store(shape, 0, cuda)
    px, lut = _frames(shape, 0), vidode_data.pixel_table(False)
    frames = np.array([[0], [1], [2]], dtype=np.int32)
    got = _launch(store, [False] * 3, [(frames, np.ones((3, 1), np.float32))], ANGLE_SETS["right"], False)[0]
    want180 = lut[torch.from_numpy(px[2, ::-1, ::-1].copy()).long()].permute(2, 0, 1)
    assert (got[2, 0] - want180).abs().max() <= 2.0 ** -23
    if shape[0] == shape[1]:
        want90 = lut[torch.from_numpy(np.rot90(px[1]).copy()).long()].permute(2, 0, 1)
        assert (got[1, 0] - want90).abs().max() <= 2.0 ** -23


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_frame_outside_the_store_is_not_read(cuda, shape):
    store = _store(shape, 9, cuda)
    frames = np.array([[0, N_FRAMES, 5], [-1, N_FRAMES - 1, 6]], dtype=np.int32)
    factor = np.array([[1.0, 1.0, 0.5], [1.0, -2.0, 0.0]], dtype=np.float32)
    flip, angles = np.array([True, False]), (7.3, -10.0)
    got = _launch(store, flip, [(frames, factor)], angles, True, fill=7.0)[0]
    want = rot.batch(_frames(shape, 9), frames, factor, flip, angles, True)
    assert torch.isnan(got[0, 1]).all() and torch.isnan(got[1, 0]).all() and torch.isnan(want[0, 1]).all()
    known = ~torch.isnan(want)
    assert torch.isfinite(got[known]).all() and (got[known] - want[known]).abs().max() <= 4 * 2.0 ** -24 * 2    # |out| <= 2: factor -2
    assert (got[1, 2] == 0).all()


def _opt(irregular, extrap, **over):
    # irregular: 3 observed frames of a window of 6, so that test_interp has exactly half to compact
    return types.SimpleNamespace(**{**dict(window_size=6, sample_size=3 if irregular else 6, irregular=irregular, extrap=extrap, batch_size=3,
                                           phase="train", sample_from_beg=False, input_norm=True), **over})


def _loader(cuda, opt, shape=(12, 10, 3), low=9, rotate=10):
    from ode_rl_amd import vidode_data
    rng = np.random.RandomState(17)
    clips = [rng.randint(low, 256, size=(n,) + shape).astype(np.uint8) for n in (9, 7, 8)]
    return vidode_data.VidODEBatches(opt, vidode_data.ClipStore(clips, device=cuda), train=True, hflip=True, rotate=rotate, seed=1), clips


@pytest.mark.parametrize("test_interp", [None, False, True])
def test_loader_renders_the_rotated_batch(cuda, test_interp):
    """The iterator end to end (its own cos / sin, its table, all three routes): every float tensor against the restatement applied to
    the table `layout` describes, and `next_batch`'s outputs consistent with each other."""
    it, clips = _loader(cuda, _opt(True, False))
    random.seed(4)
    np.random.seed(4)
    plan = it.draw()
    assert plan["flip"].any() and not plan["flip"].all() and (np.abs(plan["angle"]) > 0.1).all()
    got = it.render(plan, test_interp)
    names, parts, host = it.layout(plan, test_interp)
    flat = np.concatenate(clips)
    for key, (frames, factor) in zip(names, parts):
        want = rot.batch(flat, frames, factor, plan["flip"], plan["angle"], True)
        want32 = rot.batch(flat, frames, factor, plan["flip"], plan["angle"], True, np.float32)
        err, err32 = float((got[key].cpu() - want).abs().max()), float((want32 - want).abs().max())
        assert got[key].device == cuda and err <= 4 * err32 + 4 * 2.0 ** -24 * float(want.abs().max()), (key, err, err32)
    assert not got["observed_mask"].is_cuda and torch.equal(got["observed_tp"], host["observed_tp"])
    if test_interp is False:
        mask = got["mask_predicted_data"].to(cuda).unsqueeze(-1).unsqueeze(-1)
        assert (got["mask_predicted_data"] == 0).any()
        assert torch.equal(got["data_to_predict"], got["orignal_data_to_predict"] * mask)
    plain, _ = _loader(cuda, _opt(True, False), rotate=None)
    assert not torch.equal(plain.render(plan, test_interp)["observed_data"], got["observed_data"])


def test_the_rotating_loader_does_not_synchronise(cuda):
    from ode_rl_amd import vidode_data
    it, _ = _loader(cuda, _opt(True, False))
    vidode_data.get_next_batch(next(it))
    it.next_batch(test_interp=True)
    torch.cuda.synchronize()
    was = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = next(it)
        b = it.next_batch()
        c = it.next_batch(test_interp=True)
    finally:
        torch.cuda.set_sync_debug_mode(was)
    assert all(torch.isfinite(x["observed_data"]).all() and torch.isfinite(x["data_to_predict"]).all() for x in (a, b, c))
    assert "orignal_data_to_predict" in b and c["observed_data"].shape[1] == 3
