"""Upstream Vid-ODE's item transform, collate, split and `get_next_batch` restated in torch ops on the CPU (Vid-ODE/dataloader.py:
289-353, video_transforms.py:32-70 and :251-258, utils.py:73-209), for the tests of ode_rl_amd.vidode_data.  It takes the sampling as
given -- which frames of which clip, which mask, flipped or not -- and does the arithmetic and the bookkeeping after it; the sampling
itself is pinned to tests/golden/vidode_data.npz directly.  tests/test_vidode_data_cpu.py pins every function here to that fixture
(produced by upstream's own classes) with torch.equal.  Nothing here imports the code under test.
"""
import json

import numpy as np
import torch


def cases(gold):
    """{name: meta} of the fixture's cases; meta = the options, the clip set, the clips of the batch, the seed, train, hflip and the
    test_interp values that apply."""
    return {str(n): json.loads(str(gold[f"case.{n}.meta"])) for n in gold["cases"]}


def clip_set(gold, name):
    n = int(gold[f"clips.{name}.n"])
    return [gold[f"clips.{name}.{i}"] for i in range(n)]


def opt_of(meta):
    import types
    return types.SimpleNamespace(**meta["opt"])


def golden_dict(gold, name, tag):
    """The dictionary the fixture recorded for a case: tag 'raw' (collate + split), 'b0' / 'b1' (get_next_batch, test_interp off / on)."""
    prefix = f"case.{name}.{tag}."
    out = {k[len(prefix):]: torch.from_numpy(gold[k]) for k in gold if k.startswith(prefix)}
    out["mode"] = "train" if cases(gold)[name]["train"] else "test"
    return out


def item(clip, rel, flip, input_norm):
    """(T, C, H, W) float32 of one item: gather, RandomHorizontalFlip's mirror, ToTensor(scale=True), Normalize(0.5, 0.5)."""
    frames = np.asarray(clip)[np.asarray(rel)]
    if frames.ndim == 3:
        frames = frames[..., None]
    if flip:
        frames = frames[..., ::-1, :].copy()
    video = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 3, 1, 2).float().div(255)
    if input_norm:
        video = video.sub_(torch.FloatTensor([0.5]).view(1, 1, 1)).div_(torch.FloatTensor([0.5]).view(1, 1, 1))
    return video


def time_grid(opt):
    if opt.irregular:
        n = opt.window_size
    elif opt.extrap:
        n = opt.sample_size
    else:
        n = opt.sample_size // 2
    return torch.from_numpy(np.arange(0, n) / n).type(torch.FloatTensor)


def collate(clips, clip_ids, rel, mask, flip, opt, train):
    """The dictionary of `video_collate_fn`: the items stacked, the (B, T, 1) mask, the grid, split by the task."""
    data = torch.stack([item(clips[int(c)], r, bool(f), bool(getattr(opt, "input_norm", False))) for c, r, f in zip(clip_ids, rel, flip)])
    mask = torch.from_numpy(np.asarray(mask, dtype=np.float32)).unsqueeze(-1)
    ts = time_grid(opt)
    if opt.extrap:
        n = opt.input_sequence if getattr(opt, "unequal", False) is True else data.size(1) // 2
        out = {"observed_data": data[:, :n].clone(), "observed_tp": ts[:n].clone(), "data_to_predict": data[:, n:].clone(),
               "tp_to_predict": ts[n:].clone(), "observed_mask": mask[:, :n].clone(), "mask_predicted_data": mask[:, n:].clone()}
    else:
        out = {"observed_data": data.clone(), "observed_tp": ts.clone(), "data_to_predict": data.clone(), "tp_to_predict": ts.clone(),
               "observed_mask": mask.clone(), "mask_predicted_data": mask.clone()}
    out["mode"] = "train" if train else "test"
    return out


def get_next_batch(data_dict, test_interp=False):
    out = dict(data_dict)
    obs_mask, pred_mask = data_dict["observed_mask"], data_dict["mask_predicted_data"]
    if not test_interp:
        out["observed_data"] = obs_mask.unsqueeze(-1).unsqueeze(-1) * data_dict["observed_data"]
        out["orignal_data_to_predict"] = data_dict["data_to_predict"].clone()
        out["data_to_predict"] = pred_mask.unsqueeze(-1).unsqueeze(-1) * data_dict["data_to_predict"]
        return out
    b, t, c, h, w = data_dict["observed_data"].shape
    out["observed_data"] = data_dict["observed_data"][obs_mask.squeeze(-1).bool()].view(b, t // 2, c, h, w)
    out["observed_mask"] = torch.ones(b, t // 2, 1)
    t = data_dict["data_to_predict"].size(1)
    out["tp_to_predict"] = torch.from_numpy(np.arange(0, t) / t).type(torch.FloatTensor)
    sel = torch.ones_like(pred_mask) - pred_mask
    sel[:, -1, :] = 0.
    out["mask_predicted_data"] = sel.squeeze(-1).byte()
    return out


def same(got, want):
    """None, or what differs between two batch dictionaries: keys, shapes, dtypes, values (torch.equal) -- devices aside."""
    if set(got) != set(want):
        return f"keys {sorted(got)} != {sorted(want)}"
    for k, w in want.items():
        g = got[k]
        if not isinstance(w, torch.Tensor):
            if g != w:
                return f"{k}: {g!r} != {w!r}"
            continue
        g = g.cpu()
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{k}: {tuple(g.shape)} {g.dtype} != {tuple(w.shape)} {w.dtype}"
        if not torch.equal(g, w):
            return f"{k}: values differ in {int((g != w).sum())} of {w.numel()} elements"
    return None
