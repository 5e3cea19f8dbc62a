"""Upstream Vid-ODE's evaluation protocol, the parts that need no GPU: the CPU restatement (tests/_png_metrics_ref.py) against
Pillow's recorded luma and against integer reasoning, the declaration of `odehip_png_metrics`, its argument checks (made before any HIP
call) and the refusals of the Python surface."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _metrics_ref as mr
import _png_metrics_ref as ref
from conftest import ROOT, load_golden

GOLD = load_golden("png_metrics.npz")
NAMES = sorted({k.split(".")[0] for k in GOLD})


@pytest.mark.parametrize("name", NAMES)
def test_luma_restatement_reproduces_pillow(name):
    rgb = GOLD[f"{name}.rgb"]
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    assert np.array_equal(ref.luma(rgb), GOLD[f"{name}.luma"])
    assert np.array_equal(ref.luma(rgb), GOLD[f"{name}.luma_png"])      # the PNG round trip changes nothing
    if name.startswith("grey"):
        assert np.array_equal(ref.luma(rgb), rgb[..., 0])


def test_fixture_covers_both_sizes_and_is_small():
    assert {GOLD[f"{n}.rgb"].shape[0] for n in NAMES} == {64, 128}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "png_metrics.npz")) < 256 * 1024


def test_float64_ssim_restatement_agrees_with_the_direct_form_on_luma():
    a = GOLD["ramps64.luma"][:32, :32]
    b = GOLD["random64.luma"][:32, :32] // 4 + (a // 4) * 3
    got, want = mr.ssim_ref(a, b, 255.0, np.float64), mr.ssim_direct(a, b, 255.0)
    assert abs(got - want) <= 1e-12, (got, want)
    assert mr.ssim_ref(a, a, 255.0, np.float64) == 1.0


@pytest.mark.parametrize("input_norm", [False, True])
def test_quantisation_restatement_matches_integer_reasoning(input_norm):
    """The byte by reasoning that does not run the chain in float32: the value u the chain sees (after the de-normalisation: x + 1
    rounds once to float32, / 2 and the clamp are exact) times 255 is EXACT in float64 (24 + 8 significant bits), so one rounding to
    float32 gives the chain's product p; p + 0.5 is again exact in float64 and rounds once to float32; the byte is its floor after the
    clamp.  Inputs: k / 255, the float32 nearest to every tie (k + 0.5) / 255, and the neighbours of both one ulp either side."""
    k = np.arange(256, dtype=np.float64)
    centres = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(np.float32)
    v = np.concatenate([centres, np.nextafter(centres, np.float32(-np.inf)), np.nextafter(centres, np.float32(np.inf))])
    x = (v * np.float32(2) - np.float32(1)).astype(np.float32) if input_norm else v
    # integer / float64 reasoning for the value the chain sees
    u = x.astype(np.float64)
    if input_norm:
        u = np.clip(((u + 1.0).astype(np.float32).astype(np.float64)) / 2.0, 0.0, 1.0)      # x + 1 rounds once; / 2 is exact
    p = (u * 255.0).astype(np.float32).astype(np.float64)        # u * 255 is exact in float64; one rounding to float32
    q = (p + 0.5).astype(np.float32).astype(np.float64)          # p + 0.5: one rounding (exact below 128, half-ulp steps above)
    want = np.floor(np.clip(q, 0.0, 255.0)).astype(np.uint8)
    got = ref.quantise(torch.from_numpy(x), input_norm).numpy()
    assert np.array_equal(got, want)
    if not input_norm:      # the grid points themselves: k / 255 -> k
        assert np.array_equal(got[:256], np.arange(256, dtype=np.uint8))
        # one ulp below a tie stays at k, the tie or above goes to k + 1 wherever the float32 product is exact enough to tell
        assert (got[256:512].astype(int) - np.arange(256) >= 0).all() and (got[256:512].astype(int) - np.arange(256) <= 1).all()
    assert ref.quantise(torch.tensor([float("nan"), -5.0, 7.0, float("inf"), float("-inf")]), input_norm).tolist() == [0, 0, 255, 255, 0]


def test_rgb_bytes_layout_and_metrics_ref_identities():
    x = torch.rand(2, 3, 1, 32, 32)
    rgb = ref.rgb_bytes(x, False)
    assert rgb.shape == (2, 3, 32, 32, 3) and torch.equal(rgb[..., 0], rgb[..., 1]) and torch.equal(rgb[..., 0], rgb[..., 2])
    assert torch.equal(rgb[..., 0], ref.quantise(x, False)[:, :, 0])
    r = ref.metrics_ref(x, x.clone(), False)
    assert (r["sse"] == 0).all() and (r["mse"] == 0).all() and (r["ssim"] == 1.0).all()
    assert ref.evaluation_ref([r["ssim"]], [r["mse"]]) == (1.0, 0.0, math.inf)


# ---- the C entry point and the Python surface -----------------------------------------------------------------------------------------

def test_header_and_ctypes_table_declare_png_metrics():
    import ode_rl_amd
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "odecgru_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+odehip_png_metrics\s*\(([^)]*)\)\s*;", src)
    assert decl, "odehip_png_metrics is not declared in the header"
    params = [p.strip() for p in decl.group(1).split(",")]
    res, args = ode_rl_amd._lib.SIGNATURES["odehip_png_metrics"]
    assert res is ctypes.c_int and len(args) == len(params) == 14
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == ("*" in p), (p, a)
        assert (a is ctypes.c_int) == p.startswith("int "), (p, a)
    assert hasattr(ode_rl_amd._lib.load(), "odehip_png_metrics")
    assert "png_metrics.hip" in open(os.path.join(ROOT, "ode-rl_amd", "csrc", "Makefile")).read()


def test_argument_errors_without_gpu():
    import ode_rl_amd
    lib = ode_rl_amd._lib.load()
    p = ctypes.c_void_p(4096)

    def call(pred=p, truth=p, b=2, t=3, c=1, s=64, outs=(p, p, p), pb=None, tb=None, acc=None):
        return lib.odehip_png_metrics(pred, truth, b, t, c, s, 1, *outs, pb, tb, acc, None), lib.odehip_last_error().decode()

    for kw, text in (({"pred": None}, "null"), ({"outs": (p, None, p)}, "null"), ({"b": 0}, "at least 1"), ({"t": 0}, "at least 1"),
                     ({"b": 70000, "t": 70000}, "grid limit"), ({"c": 2}, "channels 2"), ({"s": 48}, "48 x 48"), ({"s": 16}, "16 x 16"),
                     ({"s": 256}, "256 x 256"), ({"pb": p}, "go together"), ({"tb": p}, "go together"),
                     ({"pred": ctypes.c_void_p(4100)}, "16-byte aligned"), ({"acc": ctypes.c_void_p(4100)}, "8-byte aligned"),
                     ({"pb": ctypes.c_void_p(4098), "tb": p}, "4-byte aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)


def test_python_surface_refuses_before_any_launch():
    import ode_rl_amd
    x = torch.zeros(2, 3, 1, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ode_rl_amd.png_metrics(x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ode_rl_amd.png_metrics(x.numpy(), x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ode_rl_amd.PngEvaluation("cpu")
    assert ode_rl_amd.png_metrics is ode_rl_amd.metrics.png_metrics
    assert ode_rl_amd.PngMetrics._fields == ("ssim", "mse", "sse", "pred_bytes", "truth_bytes")


def test_select_frames_follows_upstream_indexing():
    """train._select_frames against upstream's `data[mask.squeeze(-1).byte()].view(b, n, c, h, w)` on the host."""
    from ode_rl_amd import train
    data = torch.arange(2 * 5 * 1 * 2 * 2, dtype=torch.float32).view(2, 5, 1, 2, 2)
    for mask in (torch.tensor([[1, 0, 1, 1, 0], [0, 1, 1, 0, 1]], dtype=torch.uint8),
                 torch.tensor([[1., 0., 1., 1., 0.], [0., 1., 1., 0., 1.]]).unsqueeze(-1)):
        want = data[mask.reshape(2, 5).bool()].view(2, 3, 1, 2, 2)
        assert torch.equal(train._select_frames(data, mask), want)
    assert train._select_frames(data, None) is data and train._select_frames(data, torch.ones(2, 5, 1)) is data
    with pytest.raises(ValueError, match="same number"):
        train._select_frames(data, torch.tensor([[1, 0, 1, 1, 0], [0, 1, 0, 0, 1]], dtype=torch.uint8))


def test_evaluate_vidode_refuses_hurricane_and_restores_the_mode():
    import types
    from ode_rl_amd import train
    model = torch.nn.Linear(1, 1).train()
    with pytest.raises(NotImplementedError, match="Hurricane"):
        train.evaluate_vidode(model, [], types.SimpleNamespace(dataset="hurricane", extrap=True, input_norm=True))
    with pytest.raises(ValueError, match="no batches"):
        train.evaluate_vidode(model, [], types.SimpleNamespace(dataset="kth", extrap=True, input_norm=True))
    assert model.training
