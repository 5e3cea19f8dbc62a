"""Upstream Vid-ODE's training batches assembled on the GPU from clips that stay resident in device memory.

Stands in for upstream's `VideoDataset` + `DataLoader` + `video_collate_fn` + `utils.split_and_subsample_batch` + `utils.get_next_batch`
(Vid-ODE/dataloader.py, Vid-ODE/utils.py:73-209).  Upstream does per item a numpy gather, a flip copy, `ToTensor`, `Normalize` and
later a mask multiply on the host, then a collate and a host->device copy per step; here the clips are uploaded ONCE as uint8
(`ClipStore`), the host does only upstream's index arithmetic (`VidODEBatches.draw`: which frames, which mask, flipped or not) and
`odehip_vidode_batch` writes every float tensor of the batch in one launch.  With `rotate=` upstream's `RandomRotation` joins in:
the host draws one angle per item where upstream draws it and `odehip_vidode_batch_rotated` rotates inside the same single launch.

The host makes upstream's random calls in upstream's order per item (`random.randint` / `np.random.randint` for the window,
`np.random.choice` for the irregular picks, `random.random()` for the flip, `random.uniform` for the angle), so a run under seeded
`random` / `np.random` selects the frames, masks, flips and angles upstream selects for the same clips.  The clip order comes from the
iterator's own `torch.Generator`.

Where the pieces of a batch live: the frame tensors are on the device; the time grids (`observed_tp`, `tp_to_predict`) and the masks
(`observed_mask`, `mask_predicted_data`) are HOST tensors.  The models read frame counts and times on the host (`VidODE._selected`,
`hip_ops.host_times`), so a device mask would cost them a synchronisation per step; the only device copy of the mask values is the
factor column of the kernel's table.  Nothing here synchronises: the table travels in one small non-blocking copy from pinned memory.

Out of scope, refused by name: `Scale`, `CenterCrop`, `Pad`, mp4 decoding, `HurricaneVideoDataset`; `RandomRotation` as a transform
object too (the rotation is the `rotate=` argument of `VidODEBatches`).
"""
import ctypes
import math
import numbers
import os
import random

import numpy as np
import torch

from . import _lib


def _refuse(name, why):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not implemented: {why}")
    return type(name, (object,), {"__init__": __init__, "__doc__": f"Refused: {why}"})


Scale = _refuse("Scale", "clips are stored at the model's resolution, so resize them once before building the ClipStore.")
CenterCrop = _refuse("CenterCrop", "clips are stored at the model's resolution, so crop them once before building the ClipStore.")
Pad = _refuse("Pad", "clips are stored at the model's resolution, so pad them once before building the ClipStore.")
RandomRotation = _refuse("RandomRotation", "a host transform has no place in a device-resident loader; VidODEBatches(rotate=degrees) draws the "
                         "angle where upstream does and rotates inside the batch launch.")
HurricaneVideoDataset = _refuse("HurricaneVideoDataset", "the Hurricane set needs Pad and ToTensor(scale=False), neither of which this loader has.")


def pixel_table(input_norm):
    """(256,) float32: the value of a pixel byte after upstream's `ToTensor(scale=True)` (`.float().div(255)`) and, with `input_norm`,
    `Normalize(0.5, 0.5)` (`.sub_(mean).div_(std)` with one-element float32 tensors) -- the same torch operations in the same order on
    the 256 possible bytes, so the table holds upstream's float32 values bit for bit."""
    lut = torch.arange(256, dtype=torch.int16).to(torch.uint8).float().div(255)
    if input_norm:
        lut = lut.sub_(torch.FloatTensor([0.5])).div_(torch.FloatTensor([0.5]))
    return lut


def _upload(host, device):
    """Host tensor -> `device` without a synchronisation: through pinned memory, which the caching host allocator keeps until the copy
    has run."""
    if device.type != "cuda":
        return host
    return host.pin_memory().to(device, non_blocking=True)


class ClipStore:
    """uint8 clips (L_i, H, W, C) -- or (L_i, H, W) for one channel -- back to back in one device buffer, uploaded once.  Offsets
    and lengths stay on the host.  `frame_min` (n_frames,) uint8 on the same device holds each frame's smallest byte, which the rotated
    launch clips to.  A store on the CPU serves the host side (`VidODEBatches.draw`) only: rendering needs a GPU."""

    def __init__(self, clips, device=None, min_frames=None):
        clips = list(clips)
        if not clips:
            raise ValueError("ClipStore: no clips")
        shaped = []
        for i, c in enumerate(clips):
            c = np.asarray(c)
            if c.dtype != np.uint8:
                raise ValueError(f"ClipStore: clip {i} is {c.dtype}, the store holds uint8 frames")
            if c.ndim == 3:
                c = c[..., None]
            if c.ndim != 4 or c.shape[0] < 1:
                raise ValueError(f"ClipStore: clip {i} must be (L, H, W, C) or (L, H, W), got shape {c.shape}")
            if shaped and c.shape[1:] != shaped[0].shape[1:]:
                raise ValueError(f"ClipStore: clip {i} is {c.shape[1:]} (H, W, C), clip 0 is {shaped[0].shape[1:]}: one size per store")
            shaped.append(c)
        self.height, self.width, self.channels = (int(v) for v in shaped[0].shape[1:])
        if self.channels not in (1, 3):
            raise ValueError(f"ClipStore: 1 or 3 channels, got {self.channels}")
        self.lengths = np.array([c.shape[0] for c in shaped], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.n_frames = int(self.lengths.sum())
        if self.n_frames >= 2 ** 31:
            raise ValueError("ClipStore: the frame index of the kernel's table is int32")
        if min_frames is not None:
            self.require_min_frames(min_frames)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.data = torch.from_numpy(np.concatenate(shaped, axis=0)).to(self.device)
        self.frame_min = self.data.reshape(self.n_frames, -1).amin(dim=1)

    def __len__(self):
        return len(self.lengths)

    def require_min_frames(self, threshold):
        """Upstream's `remove_files_under_sample_size` threshold (window_size if irregular, else sample_size), as a refusal."""
        short = [int(i) for i in np.nonzero(self.lengths < threshold)[0]]
        if short:
            raise ValueError(f"ClipStore: clips {short[:8]} have fewer than the {threshold} frames this mode samples")

    @classmethod
    def from_directory(cls, path, device=None, min_frames=None):
        """The `.npy` clips of a directory in upstream's order (`sorted(os.listdir(path))`), without those shorter than `min_frames`
        (upstream drops them too)."""
        names = sorted(os.listdir(path))
        if any(n.endswith(".mp4") for n in names):
            raise NotImplementedError("ClipStore: mp4 decoding is not implemented (upstream reads those through cv2): convert the videos to "
                                      "uint8 .npy clips once.")
        clips = [np.load(os.path.join(path, n)) for n in names if n.endswith(".npy")]
        return cls([c for c in clips if min_frames is None or c.shape[0] >= min_frames], device)


class VidODEBatches:
    """Endless iterator over what upstream's `video_collate_fn` + `split_and_subsample_batch` yield: {"observed_data",
    "data_to_predict"} (B, T, C, H, W) float32 on the device, {"observed_tp", "tp_to_predict"} float32 and {"observed_mask",
    "mask_predicted_data"} (B, T, 1) float32 on the HOST (see the module docstring), "mode".  `next_batch(test_interp)` yields what
    `get_next_batch(next(it), test_interp)` would, with its mask multiplies and compaction folded into the one launch.

    opt: `window_size`, `sample_size`, `irregular`, `extrap`, `batch_size`; optional `phase` ('train'), `sample_from_beg` (False),
    `unequal` (False) with `input_sequence`, `input_norm` (False).  `train=False` fixes every window at frame 0, keeps the clips in
    order and names the mode "test".  `hflip` draws upstream's `RandomHorizontalFlip` per item (upstream adds it to training sets).
    `rotate` draws upstream's `RandomRotation` per item after the flip: a number d for angles in (-d, d) degrees (upstream's is 10) or
    a pair (lo, hi); None (the default) rotates nothing and makes no random call.
    An epoch ends with a smaller batch when the clips do not divide by the batch size (DataLoader's drop_last=False)."""

    def __init__(self, opt, store, train=True, hflip=False, rotate=None, seed=0):
        self.opt, self.store, self.train, self.hflip = opt, store, bool(train), bool(hflip)
        self.rotate = _degrees(rotate)
        if getattr(opt, "dataset", None) == "hurricane":
            HurricaneVideoDataset()
        self.window_size, self.sample_size = int(opt.window_size), int(opt.sample_size)
        self.irregular, self.extrap = bool(opt.irregular), bool(opt.extrap)
        self.phase = getattr(opt, "phase", "train")
        self.sample_from_beg = getattr(opt, "sample_from_beg", False)
        self.batch_size = int(opt.batch_size)
        if self.batch_size < 1:
            raise ValueError("VidODEBatches: batch_size must be positive")
        if self.sample_size > self.window_size:
            raise ValueError(f"VidODEBatches: sample_size {self.sample_size} > window_size {self.window_size}")
        if self.irregular and self.extrap and (self.window_size % 2 or self.sample_size % 2):
            raise ValueError("VidODEBatches: irregular extrapolation needs even window_size and sample_size")
        if self.irregular and self.sample_size < (4 if self.extrap else 2):
            raise ValueError("VidODEBatches: irregular sampling keeps the first and last frame of each part: sample_size is too small")
        if not self.irregular and not self.extrap and self.sample_size < 2:
            raise ValueError("VidODEBatches: regular interpolation needs sample_size >= 2")
        store.require_min_frames(self.window_size if self.irregular else self.sample_size)
        # parse_datasets' grid (dataloader.py:355-365): float64 arange / n, then float32
        if self.irregular:
            n_grid, self.n_data = self.window_size, self.window_size
        elif self.extrap:
            n_grid, self.n_data = self.sample_size, self.sample_size
        else:
            n_grid = self.sample_size // 2
            self.n_data = self.sample_size // 2 if self.phase == "train" else self.sample_size
        self.time_steps = torch.from_numpy(np.arange(0, n_grid) / n_grid).type(torch.FloatTensor)
        if self.extrap:
            self.n_observed = int(opt.input_sequence) if getattr(opt, "unequal", False) is True else self.n_data // 2
            if not 0 < self.n_observed < self.n_data:
                raise ValueError(f"VidODEBatches: input_sequence {self.n_observed} leaves no frame on one side of {self.n_data}")
        else:
            self.n_observed = self.n_data
        self.mode = "train" if self.train else "test"
        self.input_norm = bool(getattr(opt, "input_norm", False))
        self._lut_host = pixel_table(self.input_norm)
        self._lut = self._lut_host.to(store.device)
        self._gen = torch.Generator().manual_seed(seed)
        self._order, self._cursor = None, 0

    # ---- the host side: upstream's sampling -------------------------------------------------------------------------------------

    def _window_start(self, seq_len, span, np_rng):
        """Where the window starts.  Training draws it as the mode's sampler does: inclusive `random.randint(0, seq_len - span)`, or
        for regular interpolation `np.random.randint` with the exclusive bound one above it."""
        if self.sample_from_beg is not False or not self.train:
            return 0
        return int(np.random.randint(0, seq_len - span + 1)) if np_rng else random.randint(0, seq_len - span)

    def _sample(self, seq_len):
        """(frames of the clip that enter the batch, their mask) for one item: `Dataset_base.sampling` (dataloader.py:31-158)."""
        s, w = self.sample_size, self.window_size
        if not self.irregular:
            start = self._window_start(seq_len, s, np_rng=not self.extrap)
            if self.extrap or self.phase != "train":
                rel = np.arange(start, start + s)
                mask = np.ones(s, dtype=np.float32)
                if not self.extrap:   # every frame goes in, every other one is observed
                    mask[1::2] = 0.0
            else:
                rel = np.arange(start, start + s, 2)
                mask = np.ones(s // 2, dtype=np.float32)
            return rel, mask
        # irregular: the whole window goes in; the mask keeps its first and last frame and random ones between
        start = self._window_start(seq_len, w + 1, np_rng=False) if seq_len > w else 0
        if self.extrap:
            half = w // 2   # == seq_len // 2 where the clip is exactly one window long
            picks = sorted(np.random.choice(list(range(start + 1, start + half)), size=s // 2 - 1, replace=False))
            picks += sorted(np.random.choice(list(range(start + half, start + w - 1)), size=s // 2 - 1, replace=False))
        else:
            picks = sorted(np.random.choice(list(range(start + 1, start + w - 1)), size=s - 2, replace=False))
        mask = np.zeros(w, dtype=np.float32)
        mask[[0, w - 1] + [int(p) - start for p in picks]] = 1.0
        return np.arange(start, start + w), mask

    def _next_clips(self):
        n = len(self.store)
        if self._order is None or self._cursor >= n:
            self._order = (torch.randperm(n, generator=self._gen) if self.train else torch.arange(n)).numpy()
            self._cursor = 0
        idx = self._order[self._cursor:self._cursor + self.batch_size]
        self._cursor += self.batch_size
        return idx

    def draw(self, clips=None):
        """The random part of one batch, all on the host: {"clips" (B,), "rel" (B, T) frame numbers inside each clip, "frames" (B, T)
        int32 frame numbers in the store, "mask" (B, T) float32, "flip" (B,) bool, "angle" (B,) float64 degrees (zeros without
        `rotate`)}.  `clips` overrides the iterator's clip order."""
        clips = self._next_clips() if clips is None else np.asarray(clips, dtype=np.int64)
        rel, mask, flip, angle = [], [], [], []
        for c in clips:
            r, m = self._sample(int(self.store.lengths[c]))
            rel.append(r)
            mask.append(m)
            flip.append(self.hflip and random.random() < 0.5)
            angle.append(random.uniform(*self.rotate) if self.rotate is not None else 0.0)
        rel = np.stack(rel).astype(np.int64)
        frames = rel + self.store.offsets[clips][:, None]
        return {"clips": np.asarray(clips), "rel": rel, "frames": frames.astype(np.int32), "mask": np.stack(mask),
                "flip": np.array(flip, dtype=bool), "angle": np.array(angle, dtype=np.float64)}

    # ---- the device side ------------------------------------------------------------------------------------------------------------

    def _launch(self, flip, parts, angle=None):
        """One `odehip_vidode_batch` launch: parts = [(frames (B, T_k) int32, factors (B, T_k) float32)] -> the float tensors.  With
        `angle` (B,) degrees it is one `odehip_vidode_batch_rotated` launch, whose table starts with cos and sin per sample."""
        store, dev = self.store, self.store.device
        if dev.type != "cuda":
            raise RuntimeError("VidODEBatches assembles batches with the HIP library: the ClipStore must be on a GPU (no CPU fallback)")
        b = len(flip)
        words = [flip.astype(np.int32)]
        if angle is not None:
            rad = [math.radians(float(a)) for a in angle]
            words.insert(0, np.array([[math.cos(a), math.sin(a)] for a in rad], dtype=np.float64).ravel().view(np.int32))
        for frames, factor in parts:
            if int(frames.min()) < 0 or int(frames.max()) >= store.n_frames:
                raise ValueError("VidODEBatches: frame index outside the store")
            words += [np.ascontiguousarray(frames, dtype=np.int32).ravel(), np.ascontiguousarray(factor, dtype=np.float32).ravel().view(np.int32)]
        table = _upload(torch.from_numpy(np.concatenate(words)), dev)
        outs = [torch.empty((b, f.shape[1], store.channels, store.height, store.width), device=dev) for f, _ in parts]
        out_ptrs = (ctypes.c_void_p * len(parts))(*[o.data_ptr() for o in outs])
        counts = (ctypes.c_int * len(parts))(*[f.shape[1] for f, _ in parts])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream()
            if angle is None:
                _lib.check(_lib.load().odehip_vidode_batch(
                    store.data.data_ptr(), store.n_frames, store.height, store.width, store.channels, self._lut.data_ptr(),
                    table.data_ptr(), table.numel(), b, len(parts), out_ptrs, counts, ctypes.c_void_p(stream.cuda_stream)))
            else:
                _lib.check(_lib.load().odehip_vidode_batch_rotated(
                    store.data.data_ptr(), store.n_frames, store.height, store.width, store.channels, store.frame_min.data_ptr(),
                    int(self.input_norm), table.data_ptr(), table.numel(), b, len(parts), out_ptrs, counts,
                    ctypes.c_void_p(stream.cuda_stream)))
        table.record_stream(stream)   # the launch is asynchronous: keep the table alive until the stream has consumed it
        return outs

    def layout(self, plan, test_interp=None):
        """The host half of `render`: (names, parts, host entries).  parts[k] = (frames, factors), both (B, T_k): the table of the
        float tensor names[k]; the host entries are the times, masks and mode of the dictionary.  Touches no device."""
        frames, mask, n_obs = plan["frames"], plan["mask"], self.n_observed
        lo = n_obs if self.extrap else 0    # interpolation: both halves of the split are the whole sequence
        obs_f, obs_m, pred_f, pred_m = frames[:, :n_obs], mask[:, :n_obs], frames[:, lo:], mask[:, lo:]
        ones = np.ones_like

        def host_mask(m):
            return torch.from_numpy(np.ascontiguousarray(m)).unsqueeze(-1)

        host = {"observed_tp": self.time_steps[:n_obs].clone(), "tp_to_predict": self.time_steps[lo:].clone(),
                "observed_mask": host_mask(obs_m), "mask_predicted_data": host_mask(pred_m), "mode": self.mode}
        if test_interp is None:     # the collated and split batch: nothing masked yet
            return ["observed_data", "data_to_predict"], [(obs_f, ones(obs_m)), (pred_f, ones(pred_m))], host
        if not test_interp:         # the mask is the factor; the unmasked target is a third output
            return (["observed_data", "data_to_predict", "orignal_data_to_predict"],
                    [(obs_f, obs_m), (pred_f, pred_m), (pred_f, ones(pred_m))], host)
        obs_f = np.take_along_axis(obs_f, _selected_columns(obs_m), axis=1)
        t = pred_f.shape[1]
        host.update({"tp_to_predict": torch.from_numpy(np.arange(0, t) / t).type(torch.FloatTensor),
                     "observed_mask": torch.ones(obs_f.shape[0], obs_f.shape[1], 1), "mask_predicted_data": _unobserved(host_mask(pred_m))})
        return ["observed_data", "data_to_predict"], [(obs_f, np.ones(obs_f.shape, np.float32)), (pred_f, ones(pred_m))], host

    def render(self, plan, test_interp=None):
        """The batch of a `draw()`.  test_interp None: the collated and split dictionary (what `__next__` yields); False / True: the
        dictionary `get_next_batch(that, test_interp)` returns, from the same single launch."""
        names, parts, host = self.layout(plan, test_interp)
        angle = plan["angle"] if self.rotate is not None else None
        return {**dict(zip(names, self._launch(plan["flip"], parts, angle))), **host}

    def __iter__(self):
        return self

    def __next__(self):
        return self.render(self.draw())

    def next_batch(self, test_interp=False):
        return self.render(self.draw(), test_interp=bool(test_interp))


def _degrees(rotate):
    """`RandomRotation.__init__` (video_transforms.py): a number d means (-d, d) and must not be negative, anything else is (lo, hi)."""
    if rotate is None:
        return None
    if isinstance(rotate, numbers.Number):
        if rotate < 0:
            raise ValueError("VidODEBatches: if rotate is a single number, it must be positive")
        return (-float(rotate), float(rotate))
    if len(rotate) != 2:
        raise ValueError("VidODEBatches: if rotate is a sequence, it must be of len 2 (lo, hi)")
    return (float(rotate[0]), float(rotate[1]))


def _selected_columns(mask):
    """(B, T // 2) positions of the observed frames per row, in order: the compaction of upstream's `data[mask.byte()].view(b, t // 2,
    ...)`, which needs exactly T // 2 observed frames in every row."""
    mask = np.asarray(mask)
    t = mask.shape[1]
    if not (mask.sum(axis=1) == t // 2).all() or not np.isin(mask, (0.0, 1.0)).all():
        raise ValueError(f"test_interp keeps exactly {t // 2} of {t} observed frames per sample (interpolation modes with sample_size == half "
                         f"the frames of a batch); this mask keeps {mask.sum(axis=1).tolist()}")
    return np.stack([np.nonzero(row)[0] for row in mask]) if t // 2 else np.zeros((mask.shape[0], 0), dtype=np.int64)


def _unobserved(mask_pred):
    """utils.py:112-115: the frames to score when testing interpolation -- those NOT observed, the last frame excluded; (B, T) uint8."""
    sel = torch.ones_like(mask_pred) - mask_pred
    sel[:, -1, :] = 0.
    return sel.squeeze(-1).byte()


def get_next_batch(data_dict, test_interp=False):
    """Upstream's `utils.get_next_batch` (Vid-ODE/utils.py:73-117), both branches, in torch ops on the device the frames are on.  Masks
    and times stay where the loader put them (the host); the mask reaches the device through pinned memory, so this call does not
    synchronise either.
      test_interp False: observed_data and data_to_predict are multiplied by their masks; the unmasked target is kept as
                         "orignal_data_to_predict" (sic)
      test_interp True:  observed_data is compacted to the observed half of its frames (observed_mask becomes ones), tp_to_predict
                         becomes arange(T) / T and mask_predicted_data the uint8 (B, T) selection of the unobserved frames but the last"""
    obs = data_dict["observed_data"]
    dev = obs.device
    out = {"observed_data": obs, "observed_tp": data_dict["observed_tp"], "data_to_predict": data_dict["data_to_predict"],
           "tp_to_predict": data_dict["tp_to_predict"], "observed_mask": None, "mask_predicted_data": None, "mode": data_dict["mode"]}
    mask = data_dict.get("observed_mask")
    if mask is not None:
        out["observed_mask"] = mask
        if not test_interp:
            out["observed_data"] = _upload(mask.cpu(), dev).unsqueeze(-1).unsqueeze(-1) * obs
        else:
            keep = torch.from_numpy(_selected_columns(mask.cpu().squeeze(-1).numpy()))
            rows = torch.arange(obs.size(0)).unsqueeze(-1).expand_as(keep).contiguous()
            out["observed_data"] = obs[_upload(rows, dev), _upload(keep, dev)]
            out["observed_mask"] = torch.ones(obs.size(0), obs.size(1) // 2, 1)
    mask = data_dict.get("mask_predicted_data")
    if mask is not None:
        out["mask_predicted_data"] = mask
        if not test_interp:
            out["orignal_data_to_predict"] = out["data_to_predict"].clone()
            out["data_to_predict"] = _upload(mask.cpu(), dev).unsqueeze(-1).unsqueeze(-1) * out["data_to_predict"]
        else:
            t = out["data_to_predict"].size(1)
            out["tp_to_predict"] = torch.from_numpy(np.arange(0, t) / t).type(torch.FloatTensor)
            out["mask_predicted_data"] = _unobserved(mask.cpu())
    return out
