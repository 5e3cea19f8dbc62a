"""The host side of ode_rl_amd.vidode_data against tests/golden/vidode_data.npz, which upstream Vid-ODE's own loader classes produced
(tests/golden/make_golden_vidode_data.py): under the fixture's seeds the iterator draws the frames, masks and flips upstream drew, in
every sampling mode; its pixel table holds upstream's ToTensor / Normalize values; its time grids, masks and index tables describe the
dictionaries upstream built.  Every comparison is exact.  The restatement the GPU tests compare against (tests/_vidode_data_ref.py) is
pinned to the same fixture here.  No GPU: nothing is rendered."""
import random
import types

import numpy as np
import pytest
import torch

import _vidode_data_ref as ref
from conftest import load_golden

GOLD = load_golden("vidode_data.npz")
CASES = ref.cases(GOLD)
TAGS = [(n, tag) for n, m in sorted(CASES.items()) for tag in ["raw"] + [f"b{int(t)}" for t in m["tis"]]]
TI = {"raw": None, "b0": False, "b1": True}


def _iterator(name):
    from ode_rl_amd import vidode_data
    meta = CASES[name]
    store = vidode_data.ClipStore(ref.clip_set(GOLD, meta["clip_set"]), device="cpu")
    return vidode_data.VidODEBatches(ref.opt_of(meta), store, train=meta["train"], hflip=meta["hflip"]), store


def _draw(name):
    it, store = _iterator(name)
    random.seed(CASES[name]["seed"])
    np.random.seed(CASES[name]["seed"])
    return it, store, it.draw(clips=CASES[name]["clips"])


def test_the_fixture_covers_every_mode():
    seen = {(m["opt"]["irregular"], m["opt"]["extrap"]) for m in CASES.values()}
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert any(m["opt"]["phase"] != "train" and not m["opt"]["irregular"] and not m["opt"]["extrap"] for m in CASES.values())
    assert any(not m["train"] for m in CASES.values()) and any(m["opt"]["sample_from_beg"] for m in CASES.values())
    assert any(m["opt"]["unequal"] for m in CASES.values()) and any(True in m["tis"] for m in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_sampling_draws_what_upstream_draws(name):
    it, store, plan = _draw(name)
    meta = CASES[name]
    assert np.array_equal(plan["rel"], GOLD[f"case.{name}.rel"])
    assert np.array_equal(plan["flip"], GOLD[f"case.{name}.flip"])
    assert np.array_equal(plan["frames"], GOLD[f"case.{name}.rel"] + store.offsets[meta["clips"]][:, None]) and plan["frames"].dtype == np.int32
    if meta["opt"]["extrap"]:
        want = np.concatenate([GOLD[f"case.{name}.raw.observed_mask"], GOLD[f"case.{name}.raw.mask_predicted_data"]], axis=1)
    else:
        want = GOLD[f"case.{name}.raw.observed_mask"]
    assert np.array_equal(plan["mask"], want[..., 0]) and plan["mask"].dtype == np.float32


def test_a_window_starts_in_the_last_admissible_frame():
    for name in ("reg_interp_last_start", "reg_extrap_last_start"):
        meta, rel = CASES[name], GOLD[f"case.{name}.rel"]
        lengths = [len(c) for c in ref.clip_set(GOLD, meta["clip_set"])]
        assert any(r[0] == lengths[c] - meta["opt"]["sample_size"] for r, c in zip(rel, meta["clips"])), name


@pytest.mark.parametrize("input_norm", [True, False])
def test_pixel_table_is_upstreams_totensor_and_normalize(input_norm):
    from ode_rl_amd import vidode_data
    lut = vidode_data.pixel_table(input_norm)
    assert lut.dtype == torch.float32 and torch.equal(lut, torch.from_numpy(GOLD["lut.norm" if input_norm else "lut.plain"]))


def _emulate(store, lut, flip, frames, factor):
    """What the kernel's contract says one output holds, in torch ops on the host (include/odecgru_hip.h: odehip_vidode_batch)."""
    px = store.data[torch.from_numpy(frames.astype(np.int64))]                       # (B, T, H, W, C)
    px = torch.where(torch.from_numpy(flip).view(-1, 1, 1, 1, 1), px.flip(3), px)
    return lut[px.long()].permute(0, 1, 4, 2, 3) * torch.from_numpy(factor).view(*factor.shape, 1, 1, 1)


@pytest.mark.parametrize("name,tag", TAGS)
def test_layout_describes_upstreams_dictionary(name, tag):
    """Times, masks and mode equal the fixture's, and the index / factor tables, applied as the kernel's contract states, give its
    float tensors."""
    it, store, plan = _draw(name)
    names, parts, host = it.layout(plan, TI[tag])
    got = dict(host)
    for key, (frames, factor) in zip(names, parts):
        assert frames.dtype == np.int32 and factor.dtype == np.float32 and frames.shape == factor.shape
        got[key] = _emulate(store, it._lut_host, plan["flip"], frames, factor)
    assert ref.same(got, ref.golden_dict(GOLD, name, tag)) is None


@pytest.mark.parametrize("name,tag", TAGS)
def test_restatement_is_pinned_to_the_fixture(name, tag):
    meta = CASES[name]
    if meta["opt"]["extrap"]:
        mask = np.concatenate([GOLD[f"case.{name}.raw.observed_mask"], GOLD[f"case.{name}.raw.mask_predicted_data"]], axis=1)[..., 0]
    else:
        mask = GOLD[f"case.{name}.raw.observed_mask"][..., 0]
    raw = ref.collate(ref.clip_set(GOLD, meta["clip_set"]), meta["clips"], GOLD[f"case.{name}.rel"], mask, GOLD[f"case.{name}.flip"],
                      ref.opt_of(meta), meta["train"])
    got = raw if tag == "raw" else ref.get_next_batch(raw, TI[tag])
    assert ref.same(got, ref.golden_dict(GOLD, name, tag)) is None


@pytest.mark.parametrize("name,tag", [t for t in TAGS if t[1] != "raw"])
def test_module_get_next_batch_follows_upstream(name, tag):
    """`vidode_data.get_next_batch` is plain torch ops on whatever device the frames are on: on the fixture's own collated batch."""
    from ode_rl_amd import vidode_data
    got = vidode_data.get_next_batch(ref.golden_dict(GOLD, name, "raw"), test_interp=TI[tag])
    assert ref.same(got, ref.golden_dict(GOLD, name, tag)) is None


def test_clip_order_and_epochs():
    from ode_rl_amd import vidode_data
    clips = ref.clip_set(GOLD, "A")
    opt = types.SimpleNamespace(**{**CASES["reg_extrap_train"]["opt"], "batch_size": 2})
    a, b = (vidode_data.VidODEBatches(opt, vidode_data.ClipStore(clips, "cpu"), seed=5) for _ in range(2))
    seen = [a.draw()["clips"].tolist() for _ in range(4)]
    assert [len(s) for s in seen] == [2, 1, 2, 1] and sorted(seen[0] + seen[1]) == sorted(seen[2] + seen[3]) == [0, 1, 2]
    assert seen == [b.draw()["clips"].tolist() for _ in range(4)]
    t = vidode_data.VidODEBatches(opt, vidode_data.ClipStore(clips, "cpu"), train=False)
    assert [t.draw()["clips"].tolist() for _ in range(3)] == [[0, 1], [2], [0, 1]] and t.mode == "test"
    assert (t.draw()["rel"][:, 0] == 0).all()


def test_argument_errors():
    from ode_rl_amd import vidode_data as vd
    clips = ref.clip_set(GOLD, "A")
    base = CASES["reg_extrap_train"]["opt"]
    with pytest.raises(ValueError, match="uint8"):
        vd.ClipStore([clips[0].astype(np.float32)], "cpu")
    with pytest.raises(ValueError, match="one size per store"):
        vd.ClipStore([clips[0], clips[1][:, :, :4]], "cpu")
    with pytest.raises(ValueError, match="one size per store"):
        vd.ClipStore([clips[0], np.repeat(clips[1], 3, axis=3)], "cpu")
    with pytest.raises(ValueError, match="1 or 3 channels"):
        vd.ClipStore([np.repeat(clips[0], 2, axis=3)], "cpu")
    with pytest.raises(ValueError, match="no clips"):
        vd.ClipStore([], "cpu")
    with pytest.raises(ValueError, match=r"\(L, H, W, C\)"):
        vd.ClipStore([clips[0][0, 0]], "cpu")
    assert vd.ClipStore([c[..., 0] for c in clips], "cpu").channels == 1     # (L, H, W) is one channel
    store = vd.ClipStore(clips, "cpu")   # 12, 16 and 20 frames
    with pytest.raises(ValueError, match="fewer than the 13 frames"):         # regular: sample_size is the threshold
        vd.VidODEBatches(types.SimpleNamespace(**{**base, "window_size": 14, "sample_size": 13}), store)
    vd.VidODEBatches(types.SimpleNamespace(**{**base, "window_size": 14, "sample_size": 12}), store)
    with pytest.raises(ValueError, match="fewer than the 14 frames"):         # irregular: window_size is
        vd.VidODEBatches(types.SimpleNamespace(**{**base, "irregular": True, "window_size": 14, "sample_size": 6}), store)
    with pytest.raises(ValueError, match="fewer than the 13 frames"):
        vd.ClipStore(clips, "cpu", min_frames=13)
    with pytest.raises(ValueError, match="sample_size 9 > window_size 8"):
        vd.VidODEBatches(types.SimpleNamespace(**{**base, "sample_size": 9}), store)
    with pytest.raises(ValueError, match="even"):
        vd.VidODEBatches(types.SimpleNamespace(**{**base, "irregular": True, "sample_size": 5}), store)
    with pytest.raises(ValueError, match="input_sequence"):
        vd.VidODEBatches(types.SimpleNamespace(**{**base, "unequal": True, "input_sequence": 6}), store)
    it = vd.VidODEBatches(types.SimpleNamespace(**base), store)
    with pytest.raises(ValueError, match="test_interp keeps exactly"):        # extrapolation has no observed half to compact
        it.layout(it.draw(), test_interp=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(it)


def test_c_abi_argument_errors_without_gpu():
    """`odehip_vidode_batch` checks its arguments before any HIP call."""
    import ctypes
    from ode_rl_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    outs, nf = (ctypes.c_void_p * 1)(4096), (ctypes.c_int * 1)(2)

    def call(store=p, frames=10, h=8, w=8, c=1, lut=p, table=p, words=3 + 2 * 3 * 2, batch=3, n_out=1, outs=outs, nf=nf):
        return lib.odehip_vidode_batch(store, frames, h, w, c, lut, table, words, batch, n_out, outs, nf, None)

    for kwargs, text in [(dict(store=None), b"null"), (dict(c=2), b"1 or 3 channels"), (dict(frames=0), b"frames"), (dict(w=0), b"frame size"),
                         (dict(batch=0), b"batch"), (dict(n_out=4), b"outputs"), (dict(words=14), b"the table has 14 words, these shapes need 15"),
                         (dict(outs=(ctypes.c_void_p * 1)(4100)), b"16-byte aligned"), (dict(store=ctypes.c_void_p(4097)), b"4-byte aligned"),
                         (dict(nf=(ctypes.c_int * 1)(0)), b"no frames")]:
        assert call(**kwargs) == -1 and text in lib.odehip_last_error(), (kwargs, lib.odehip_last_error())


def test_out_of_scope_is_refused_by_name():
    from ode_rl_amd import vidode_data as vd
    for cls in (vd.Scale, vd.CenterCrop, vd.Pad, vd.RandomRotation, vd.HurricaneVideoDataset):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(64)
    store = vd.ClipStore(ref.clip_set(GOLD, "A"), "cpu")
    with pytest.raises(NotImplementedError, match="HurricaneVideoDataset"):
        vd.VidODEBatches(types.SimpleNamespace(**{**CASES["reg_extrap_train"]["opt"], "dataset": "hurricane"}), store)


def test_mp4_directories_are_refused(tmp_path):
    from ode_rl_amd import vidode_data as vd
    np.save(tmp_path / "b.npy", ref.clip_set(GOLD, "A")[1])
    np.save(tmp_path / "a.npy", ref.clip_set(GOLD, "A")[0])
    np.save(tmp_path / "c.npy", ref.clip_set(GOLD, "A")[2])
    store = vd.ClipStore.from_directory(str(tmp_path), "cpu", min_frames=13)   # sorted names; the 12-frame clip is dropped
    assert store.lengths.tolist() == [16, 20]
    (tmp_path / "video_1.mp4").write_bytes(b"")
    with pytest.raises(NotImplementedError, match="mp4"):
        vd.ClipStore.from_directory(str(tmp_path), "cpu")
