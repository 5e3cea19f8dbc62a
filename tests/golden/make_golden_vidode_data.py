"""Generate tests/golden/vidode_data.npz (dev container only; never runs on the GPU box).

Drives upstream Vid-ODE's own loader code from the REFERENCE checkout (read-only, never copied): `dataloader.Dataset_base.sampling`
(its four `sample_*`), `video_transforms.RandomHorizontalFlip`, `ToTensor(scale=True)`, `Normalize(0.5, 0.5)`,
`utils.split_and_subsample_batch` and `utils.get_next_batch`, on small synthetic clips under fixed seeds.  `cv2`, `torchvision` and
`skimage` are absent here and not exercised: they are stubbed before the import.  `VideoDataset.__getitem__` and `video_collate_fn`
cannot be called (the first needs upstream's directories, the second is a closure of `parse_datasets`, which builds them): their few
lines of glue -- sample, transform; stack, split, set the mode; the time grid -- are walked here in upstream's order.  `Tensor.cuda`
is made the identity for the run (get_next_batch's test_interp branch calls it).

Every clip carries its frame number in pixel (0, 0, 0), so the frames upstream picked are read off its result.  The file holds data
only: the clips, per case the options / seed / clip numbers as JSON, the frames, masks and flips upstream drew and the dictionaries
it produced ('raw': collate + split; 'b0' / 'b1': get_next_batch with test_interp off / on), and ToTensor / Normalize on all 256 bytes.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vidode_data.py REFERENCE_ROOT
"""
import copy
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# name: (lengths, H, W, C)
CLIP_SETS = {"A": ([12, 16, 20], 8, 8, 1), "B": ([13, 14, 17], 6, 12, 3), "D": ([12, 15], 7, 10, 1), "E": ([12, 15], 5, 10, 3)}

BASE = dict(window_size=8, sample_size=6, irregular=False, extrap=False, phase="train", sample_from_beg=False, unequal=False,
            input_sequence=3, input_norm=True, batch_size=3, dataset="kth")


def case(clip_set, clips, train=True, hflip=False, tis=(False,), seed=None, last_start=False, **opt):
    return dict(clip_set=clip_set, clips=list(clips), train=train, hflip=hflip, tis=list(tis), seed=seed, last_start=last_start,
                opt={**BASE, **opt, "batch_size": len(clips)})


CASES = {
    "reg_interp_train": case("A", [2, 0, 1], hflip=True, seed=3),
    "reg_interp_last_start": case("A", [1, 2, 0], last_start=True),
    "reg_interp_testphase": case("A", [0, 1, 2], train=False, tis=(False, True), phase="test_met", seed=5),
    "reg_interp_testphase_random": case("D", [1], tis=(False, True), phase="test_met", seed=7),
    "reg_interp_rgb_plain": case("B", [2, 1, 0], hflip=True, input_norm=False, seed=8),
    "reg_extrap_train": case("A", [1, 2, 0], hflip=True, extrap=True, seed=11),
    "reg_extrap_last_start": case("E", [0, 1], extrap=True, last_start=True),
    "reg_extrap_unequal": case("B", [0, 2, 1], extrap=True, unequal=True, input_sequence=2, input_norm=False, seed=13),
    "reg_extrap_test": case("E", [1], train=False, hflip=True, extrap=True, seed=17),
    "reg_extrap_from_beg": case("D", [0, 1], hflip=True, extrap=True, sample_from_beg=True, seed=21),
    "irr_interp_train": case("A", [2, 1, 0], hflip=True, tis=(False, True), irregular=True, sample_size=4, seed=23),
    "irr_interp_test": case("B", [0, 1, 2], train=False, tis=(False, True), irregular=True, sample_size=4, input_norm=False, seed=29),
    "irr_interp_whole_clip": case("D", [0], tis=(False, True), irregular=True, window_size=12, sample_size=6, seed=31),
    "irr_interp_sparse": case("E", [1, 0], hflip=True, irregular=True, window_size=10, sample_size=3, seed=37),
    "irr_extrap_train": case("A", [0, 2, 1], hflip=True, irregular=True, extrap=True, sample_size=4, seed=41),
    "irr_extrap_unequal": case("E", [1, 0], irregular=True, extrap=True, sample_size=4, unequal=True, input_sequence=3, seed=43),
    "irr_extrap_whole_clip": case("A", [0], irregular=True, extrap=True, window_size=12, sample_size=6, seed=47),
    "irr_extrap_test": case("D", [0, 1], train=False, irregular=True, extrap=True, sample_size=6, seed=53),
}


def make_clips(name):
    lengths, h, w, c = CLIP_SETS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    clips = []
    for n in lengths:
        clip = rng.randint(0, 256, size=(n, h, w, c)).astype(np.uint8)
        clip[:, 0, 0, 0] = np.arange(n)   # the frame number, readable from the result
        clips.append(clip)
    return clips


def stub_modules():
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "skimage"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]


def run_case(cfg, clips, dataloader, vtransforms, utils, seed):
    opt = types.SimpleNamespace(**cfg["opt"])
    ds = dataloader.Dataset_base(opt, train=cfg["train"])
    random.seed(seed)
    np.random.seed(seed)
    flipper, to_tensor, normalize = vtransforms.RandomHorizontalFlip(), vtransforms.ToTensor(scale=True), vtransforms.Normalize(0.5, 0.5)
    items, rel, flips = [], [], []
    for c in cfg["clips"]:
        images, mask = ds.sampling(images=clips[c], sample_from_beg=opt.sample_from_beg)
        rel.append(np.asarray(images)[:, 0, 0, 0].astype(np.int64))
        flipped = flipper(images) if cfg["hflip"] else images
        flips.append(flipped is not images)
        video = to_tensor(flipped)
        if opt.input_norm:
            video = normalize(video)
        items.append((video, mask))
    if opt.irregular:
        time_steps = np.arange(0, opt.window_size) / opt.window_size
    elif opt.extrap:
        time_steps = np.arange(0, opt.sample_size) / opt.sample_size
    else:
        time_steps = np.arange(0, opt.sample_size // 2) / (opt.sample_size // 2)
    time_steps = torch.from_numpy(time_steps).type(torch.FloatTensor)
    data_type = "train" if cfg["train"] else "test"
    data_dict = {"data": torch.stack([b[0] for b in items]), "time_steps": time_steps, "mask": torch.stack([b[1] for b in items])}
    data_dict = utils.split_and_subsample_batch(data_dict, opt, data_type=data_type)
    data_dict["mode"] = data_type
    dicts = {"raw": data_dict}
    for ti in cfg["tis"]:
        dicts[f"b{int(ti)}"] = utils.get_next_batch(copy.deepcopy(data_dict), test_interp=ti)
    return np.stack(rel), np.array(flips), dicts


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_vidode_data.py REFERENCE_ROOT")
    stub_modules()
    sys.path.insert(0, os.path.join(sys.argv[1], "Vid-ODE"))
    import dataloader
    import utils
    import video_transforms as vtransforms
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {"cases": np.array(sorted(CASES))}
    sets = {}
    for name in CLIP_SETS:
        sets[name] = make_clips(name)
        out[f"clips.{name}.n"] = np.array(len(sets[name]))
        for i, c in enumerate(sets[name]):
            out[f"clips.{name}.{i}"] = c
    every_byte = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    out["lut.plain"] = vtransforms.ToTensor(scale=True)(every_byte).reshape(256).numpy()
    out["lut.norm"] = vtransforms.Normalize(0.5, 0.5)(vtransforms.ToTensor(scale=True)(every_byte)).reshape(256).numpy()
    for name, cfg in sorted(CASES.items()):
        clips = sets[cfg["clip_set"]]
        span = cfg["opt"]["sample_size"]
        for seed in ([cfg["seed"]] if not cfg["last_start"] else range(1000)):
            rel, flips, dicts = run_case(cfg, clips, dataloader, vtransforms, utils, seed)
            # last_start: the first seed under which some window starts in the last frame it can (regular modes)
            if not cfg["last_start"] or any(r[0] == len(clips[c]) - span for r, c in zip(rel, cfg["clips"])):
                break
        else:
            raise SystemExit(f"{name}: no seed puts a window at its last start")
        meta = {k: v for k, v in cfg.items() if k != "last_start"}
        meta["seed"] = int(seed)
        out[f"case.{name}.meta"] = np.array(json.dumps(meta))
        out[f"case.{name}.rel"], out[f"case.{name}.flip"] = rel, flips
        for tag, d in dicts.items():
            for k, v in d.items():
                if isinstance(v, torch.Tensor):
                    out[f"case.{name}.{tag}.{k}"] = v.numpy()
                else:
                    assert k == "mode" and v == ("train" if cfg["train"] else "test"), (k, v)
        print(name, "seed", seed, "rel", rel.tolist(), "flip", flips.tolist())
    path = os.path.join(HERE, "vidode_data.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
