"""Sampled z0, the part that needs no GPU: the NumPy restatement of the noise stream (tests/_philox_ref.py)
reproduces the published Philox4x32-10 known answers and has the moments of N(0, 1); the two new C-ABI exports are in step with the
header and the ctypes table and refuse bad arguments before any HIP call; `sample_z0` has no CPU fallback and checks its arguments
before its tensors; a model built without `z_sample` is the model it was."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _philox_ref as pr
from conftest import ROOT

SEED, OFFSET = 1234, 0   # the stream the GPU test draws (tests/test_hip_latent_sample.py)


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: zeros, all ones, the digits of pi."""
    ones = (0xFFFFFFFF,) * 4
    assert _hex(pr.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(pr.philox4x32_10(ones, ones[:2])) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(pr.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays go through the same arithmetic as scalars
    c = [np.array([0, 0xFFFFFFFF], dtype=np.uint64)] * 4
    got = pr.philox4x32_10(c, (0, 0))
    assert _hex(w[0] for w in got) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_uniform_mapping_is_exact_in_fp32_and_open():
    w = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    u = pr.word_uniform(w)
    assert (u.astype(np.float32).astype(np.float64) == u).all()          # 24 significant bits
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24         # never 0 (ln) and never 1
    assert np.sqrt(-2.0 * np.log(u.min())) < 5.78                        # the largest radius: |eps| < 6 by construction


def test_stream_moments():
    x = pr.noise(1, 64, 64, SEED, OFFSET)                                # 2^20 normals
    assert x.size == 1 << 20
    r = pr.check_moments(x)
    assert r["max_abs"] > 4.0                                            # and the tails are there
    # the two Box-Muller outputs of a pair, and the two pairs of a quad, are uncorrelated
    q = x.reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs((q[:, i] * q[:, j]).mean()) <= 5.0 / np.sqrt(q.shape[0]), (i, j)


def test_stream_is_indexed_by_the_global_sample():
    full = pr.noise(3, 5, 8, SEED, 7)
    part = pr.noise(3, 2, 8, SEED, 7, batch_offset=2, global_batch=5)
    assert np.array_equal(full.reshape(3, 5, 8, 16, 16)[:, 2:4], part.reshape(3, 2, 8, 16, 16))
    assert not np.array_equal(pr.noise(1, 2, 8, SEED, 0), pr.noise(1, 2, 8, SEED, 1))       # the offset separates draws
    assert not np.array_equal(pr.noise(1, 2, 8, SEED, 0), pr.noise(1, 2, 8, SEED + 1, 0))   # and so does the seed
    hi = pr.noise(1, 1, 4, (1 << 63) + 5, (1 << 40) + 3)                 # the high words of both are used
    assert not np.array_equal(hi, pr.noise(1, 1, 4, 5, (1 << 40) + 3)) and not np.array_equal(hi, pr.noise(1, 1, 4, (1 << 63) + 5, 3))


def _kinds_of_header(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "odecgru_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, f"{name} is not declared in the header"
    params = [p.strip() for p in decl.group(1).split(",")]
    return src, ["p" if "*" in p else ("u" if p.startswith("uint64_t") else "i") for p in params]


def test_header_and_ctypes_table_declare_both_symbols():
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    for name in ("odehip_latent_sample", "odehip_latent_sample_backward"):
        src, kinds = _kinds_of_header(name)
        res, args = ode_rl_amd._lib.SIGNATURES[name]
        table = ["p" if a is ctypes.c_void_p else ("u" if a is ctypes.c_uint64 else "i") for a in args]
        assert res is ctypes.c_int and kinds == table, (name, kinds, table)
        assert hasattr(lib, name)
    assert lib.odehip_version() == 13 == ode_rl_amd._lib.ABI_VERSION
    assert int(re.search(r"#define\s+ODEHIP_ABI_VERSION\s+(\d+)", src).group(1)) == 13


def test_argument_errors_without_gpu():
    """Checked before any HIP call: -1 and a message that names the problem."""
    import ode_rl_amd
    L = ode_rl_amd._lib
    lib = L.load()
    p = ctypes.c_void_p(64)

    def fwd(mean=p, std=p, b=2, c=64, h=16, w=16, k=1, boff=0, gb=2, z0=p):
        rc = lib.odehip_latent_sample(mean, std, b, c, h, w, k, 1, 0, boff, gb, None, z0, None, None, None)
        return rc, lib.odehip_last_error().decode()

    def bwd(g=p, mean=p, std=p, b=2, c=64, h=16, w=16, k=1, boff=0, gb=2, gm=p, gs=p):
        rc = lib.odehip_latent_sample_backward(g, None, mean, std, b, c, h, w, k, 1, 0, boff, gb, None, gm, gs, None)
        return rc, lib.odehip_last_error().decode()

    for call, nulls in ((fwd, ({"mean": None}, {"std": None}, {"z0": None})),
                        (bwd, ({"g": None}, {"mean": None}, {"std": None}, {"gm": None}, {"gs": None}))):
        for kw in nulls:
            rc, msg = call(**kw)
            assert rc == -1 and "null" in msg, (kw, msg)
        rc, msg = call(h=8, w=8)
        assert rc == -1 and "8 x 8" in msg and "shape" in msg, msg
        rc, msg = call(c=6)
        assert rc == -1 and "channels 6" in msg, msg
        rc, msg = call(b=0)
        assert rc == -1 and "batch (0)" in msg, msg
        rc, msg = call(k=0)
        assert rc == -1 and "n_samples (0)" in msg, msg
        rc, msg = call(boff=1, gb=2)
        assert rc == -1 and "global batch" in msg, msg
        rc, msg = call(boff=-1)
        assert rc == -1 and "global batch" in msg, msg
    with pytest.raises(ValueError, match="global batch"):
        L.check(rc)


def test_sample_z0_has_no_cpu_fallback_and_checks_arguments_first():
    import ode_rl_amd
    x = torch.ones(2, 64, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ode_rl_amd.sample_z0(x, x)
    with pytest.raises(TypeError):
        ode_rl_amd.sample_z0(x.numpy(), x)
    # arguments before tensors: these would hit the CPU refusal otherwise
    for kw in ({"n_samples": 0}, {"n_samples": 2.0}, {"n_samples": True}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ode_rl_amd.sample_z0(x, x, **kw)
    with pytest.raises(ValueError, match="eps"):
        ode_rl_amd.sample_z0(x, x, eps=x, seed=3)
    assert ode_rl_amd.sample_z0 is ode_rl_amd.autograd.sample_z0 and "sample_z0" in ode_rl_amd.__all__ and "last_z0_noise" in ode_rl_amd.__all__


def test_noise_shard_bookkeeping():
    import ode_rl_amd.dist as od
    from ode_rl_amd import autograd
    try:
        assert od.set_noise_shard(10, rank=1, world=4) == (3, 10) and autograd._noise_shard == (3, 10)   # shard_bounds(10, 1, 4) = [3, 6)
        assert od.set_noise_shard(8, rank=0, world=2) == (0, 8)
        with pytest.raises(ValueError):
            autograd.set_noise_shard(4, 4)
    finally:
        od.clear_noise_shard()
    assert autograd._noise_shard is None


def _opt(**kw):
    return argparse.Namespace(resolution=64, n_downs=2, conv_encoder_out_ch=64, in_channels=1, n_ode_layers=3, neural_ode_n_units=64,
                              neural_ode_decoder_out_ch=64, decode_diff_method="rk4", mem=False, **kw)


def test_model_without_z_sample_in_opt_is_the_model_it_was():
    from ode_rl_amd.models.ODEConvGRU import ODEConvGRU
    absent, off, on = (ODEConvGRU(_opt(**kw), torch.device("cpu")) for kw in ({}, {"z_sample": False}, {"z_sample": True, "z_n_samples": 2}))
    keys = sorted(off.state_dict().keys())
    assert sorted(absent.state_dict().keys()) == keys == sorted(on.state_dict().keys())   # the switch adds no parameter and no buffer
    assert len(keys) > 20 and absent.last_loss_terms is None
    # get_loss without a sampled forward before it is the plain MSE, whatever the switch says
    pred, truth = torch.rand(2, 3, 1, 64, 64), torch.rand(2, 3, 1, 64, 64)
    for m in (absent, on):
        assert torch.equal(m.get_loss(pred, truth), torch.nn.functional.mse_loss(pred, truth))
        assert m.last_loss_terms is None
