"""Plain references, in any dtype, for the three kernels behind VidODE's flow / mask / warp decoder (csrc/warp.hip, csrc/bn_relu_up.hip,
csrc/upsample.hip), and the cases at which tests/test_hip_flow_tail_shapes.py runs them (test infrastructure only).  The references are
torch's own operators on the CPU: run in float64 they are the yardstick, run in float32 they say how far two correct float32
implementations may sit apart (`bound`).  tests/test_flow_tail_ref_cpu.py checks, without a GPU, that every case below is one at which
that comparison means something: no source coordinate of the warp on an integer or on the border clamp, no BatchNorm pre-activation on
the ReLU kink, and a float32 restatement that stays below the floor of every compared tensor."""
import copy
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conftest import procedural_tensor, rel_l2

# floors of tests/test_hip_vidode.py (test_warp_chain_kernel_forward_and_backward, test_bn_relu_up_matches_torch, test_upsample2x_matches_torch)
WARP_FLOORS = {"pred_x": 1e-6, "warped": 1e-6, "masks": 1e-6, "g_flow": 1e-5, "g_inter": 1e-6, "g_logit": 1e-6, "g_start": 2e-6}
BN_FLOORS = {"out": 2e-6, "gx": 2e-5, "gw": 2e-5, "gb": 2e-5, "gcb": 2e-5, "running_mean": 1e-6, "running_var": 1e-6}
UP_FLOORS = {"out": 1e-6, "gx": 1e-6}

INTEGER_MARGIN = 1e-3   # pixels: floor() picks the corners and the flow gradient jumps across an integer coordinate
BORDER_MARGIN = 1e-3    # pixels: the clamp flag and the zero gradient switch at 0 and at W-1 / H-1
KINK_MARGIN = 1e-4      # BatchNorm pre-activation: the ReLU mask switches at 0
FLOW_NUDGE = 0.01       # pixels
BN_NUDGE = 0.01


def bound(r32, r64, floor):
    """(bound, d32): tests/_convgru_ref.py::bound -- the HIP result may sit 4 x as far from the float64 result as the float32
    restatement does, never asked below `floor`."""
    d32 = rel_l2(r32, r64)
    return max(4.0 * d32, floor), d32


# ---- warp chain + mask compositing ----------------------------------------------------------------------------------------------
def source_coordinates(flows, grid_x, grid_y):
    """Un-normalised source coordinates (ix, iy), each (B, T, H, W), BEFORE the border clamp: flows (B,T,2,H,W) in pixels, in the dtype
    to compute in; ATen's grid_sampler_unnormalize with align_corners=False on grid + flow / ((size - 1) / 2)."""
    h, w = flows.shape[-2:]
    gx = grid_x.view(1, 1, 1, w) + flows[:, :, 0] / ((w - 1.0) / 2.0)
    gy = grid_y.view(1, 1, h, 1) + flows[:, :, 1] / ((h - 1.0) / 2.0)
    return ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2


def leaf(t, dtype, requires_grad=True):
    """A fresh leaf holding t's values in `dtype` (never t itself: the cases' inputs are shared and stay as they are)."""
    return t.detach().to(dtype, copy=True).requires_grad_(requires_grad)


def warp_composite_ref(pred_outputs, start, grid_x, grid_y, dtype):
    """oracle/vidode_ref.py::warp_composite restated in `dtype`, on the grid values the kernel is given (grid_x (W,), grid_y (H,): the
    caller's float32 arrays cast to `dtype`, so both sides sample the same coordinates).  pred_outputs (B,T,c+3,H,W): flow (2),
    intermediate frame (c), mask logit (1); start (B,c,H,W).  Returns pred_x, warped (B,T,c,H,W), masks (B,T,1,H,W) and the
    un-normalised, unclamped source coordinates ix, iy (B,T,H,W), which depend on the flows alone."""
    pred_outputs, start = pred_outputs.to(dtype), start.to(dtype)
    grid_x, grid_y = grid_x.to(dtype), grid_y.to(dtype)
    b, t, cc, h, w = pred_outputs.shape
    c = cc - 3
    flows, inter, masks = pred_outputs[:, :, :2], pred_outputs[:, :, 2:2 + c], torch.sigmoid(pred_outputs[:, :, 2 + c:])
    gx = grid_x.view(1, 1, w, 1).expand(b, h, -1, -1)
    gy = grid_y.view(1, h, 1, 1).expand(b, -1, w, -1)
    grid = torch.cat([gx, gy], 3)
    last, warped = start, []
    for i in range(t):
        fl = flows[:, i]
        fl = torch.cat([fl[:, 0:1] / ((w - 1.0) / 2.0), fl[:, 1:2] / ((h - 1.0) / 2.0)], dim=1).permute(0, 2, 3, 1)
        last = F.grid_sample(last, grid + fl, mode="bilinear", padding_mode="border", align_corners=False)
        warped.append(last.unsqueeze(1))
    warped = torch.cat(warped, dim=1)
    with torch.no_grad():
        ix, iy = source_coordinates(flows, grid_x, grid_y)
    return masks * warped + (1 - masks) * inter, warped, masks, ix, iy


# (B, T, c, H, W, flow rms in pixels)
WARP_SHAPES = {
    "6x10": (2, 3, 1, 6, 10, 1.5),          # non-square both ways, H*W = 60 < the 256 threads of a workgroup
    "10x6": (2, 3, 2, 10, 6, 1.5),
    "20x36": (3, 2, 3, 20, 36, 4.0),        # H*W = 720: a ragged tail of the strided pixel loop
    "2x2": (1, 1, 1, 2, 2, 0.4),            # the smallest image the entry point admits, one step
    "c4_48x40": (2, 4, 4, 48, 40, 3.0),     # four channels, both passes inside the LDS budget (2 and 3 x 4 x 1920 x 4 B)
    "clamped": (2, 2, 2, 12, 20, 1e4),      # every coordinate far outside: the flow sign varies per quadrant
    "c4_64x64": (1, 2, 4, 64, 64, 3.0),     # the forward fits in LDS (128 KiB), the backward does not (192 KiB): forward only
}
WARP_SKEWED = ("6x10", "10x6", "20x36", "c4_48x40")   # also run with grid_y = linspace(-0.9, 0.9, H): the two grid arrays then differ in value
WARP_KEYS = tuple(WARP_SHAPES) + tuple(k + ".skew" for k in WARP_SKEWED)
WARP_SEEDS = {"2x2": 7054}   # of four pixels, one samples the interior on both axes
WARP_FORWARD_ONLY = ("c4_64x64",)
WARP_ALL_CLAMPED = ("clamped",)
WARP_SUBSET_CASE = "20x36"
# operand subsets of the backward: which output gradients exist, which inputs require grad
WARP_SUBSETS = {
    "from_pred_x": dict(use=(True, False, False), po_grad=True, start_grad=True),
    "from_masks": dict(use=(False, False, True), po_grad=True, start_grad=True),
    "start_frozen": dict(use=(True, True, True), po_grad=True, start_grad=False),
    "po_frozen": dict(use=(True, True, True), po_grad=False, start_grad=True),
}


def coordinate_margins(ix, iy, h, w):
    """(smallest distance of any coordinate from an integer, smallest distance from 0 and from size - 1), in pixels."""
    d_int = min(float((v - v.round()).abs().min()) for v in (ix, iy))
    d_border = min(float(torch.minimum(v.abs(), (v - (n - 1)).abs()).min()) for v, n in ((ix, w), (iy, h)))
    return d_int, d_border


def _offending(v, n):
    return ((v - v.round()).abs() < INTEGER_MARGIN) | (v.abs() < BORDER_MARGIN) | ((v - (n - 1)).abs() < BORDER_MARGIN)


@functools.lru_cache(maxsize=None)
def warp_inputs(key):
    """The float32 inputs of a warp case, from conftest.procedural_tensor: po, start, grid_x, grid_y and the output gradients gp, gw, gm.
    Flow components whose float64 source coordinate lies within the margins of an integer or of the border are moved by FLOW_NUDGE."""
    name, _, variant = key.partition(".")
    b, t, c, h, w, rms = WARP_SHAPES[name]
    seed = WARP_SEEDS.get(name, 7000 + 16 * list(WARP_SHAPES).index(name))
    po = procedural_tensor((b, t, c + 3, h, w), seed, -1.0, 1.0)
    po[:, :, 2:2 + c] = 0.5 * po[:, :, 2:2 + c] + 0.5     # intermediate frames in [0, 1)
    po[:, :, 2 + c:] *= 2.0                               # mask logits in [-2, 2)
    grid_x = torch.linspace(-1.0, 1.0, w)
    grid_y = torch.linspace(-0.9, 0.9, h) if variant == "skew" else torch.linspace(-1.0, 1.0, h)
    if name in WARP_ALL_CLAMPED:
        # |flow| in [0.5, 1.5) x rms / 1.04 (rms of the magnitude = rms); quadrant (y < H/2, x < W/2) decides the signs of (flow_x, flow_y)
        sx = torch.where(torch.arange(w) < w // 2, 1.0, -1.0).view(1, 1, 1, w)
        sy = torch.where(torch.arange(h) < h // 2, -1.0, 1.0).view(1, 1, h, 1)
        mag = (1.0 + 0.5 * po[:, :, :2]) * (rms / math.sqrt(1.0 + 1.0 / 12.0))
        po[:, :, 0] = mag[:, :, 0] * sx * sy              # x: + - on the upper half, - + on the lower
        po[:, :, 1] = mag[:, :, 1] * sy
    else:
        po[:, :, :2] *= rms * math.sqrt(3.0)              # uniform in [-a, a) has rms a / sqrt(3)
        for _ in range(8):
            ix, iy = source_coordinates(po[:, :, :2].double(), grid_x.double(), grid_y.double())
            bad = torch.stack([_offending(ix, w), _offending(iy, h)], dim=2)
            if not bool(bad.any()):
                break
            po[:, :, :2] += bad.float() * FLOW_NUDGE
        else:
            raise AssertionError(f"warp case {key}: nudging did not clear the margins")
    # start image of amplitude 0.5 and output gradients of non-zero mean: float32 rounds a source coordinate of a 48 x 40 image to ~1e-6
    # pixel, which white-noise images and zero-mean gradients (sums that cancel) turn into a relative error above the floors of g_logit
    # and g_start in the float32 RESTATEMENT (1.2e-6, 2.9e-6); with these values it stays below every floor at every case
    return SimpleNamespace(key=key, name=name, b=b, t=t, c=c, h=h, w=w, po=po, start=procedural_tensor((b, c, h, w), seed + 1, 0.25, 0.75),
                           grid_x=grid_x, grid_y=grid_y, gp=procedural_tensor((b, t, c, h, w), seed + 2, -0.5, 1.0),
                           gw=procedural_tensor((b, t, c, h, w), seed + 3, -0.15, 0.3), gm=procedural_tensor((b, t, 1, h, w), seed + 4, -0.15, 0.3))


def warp_run_ref(inp, dtype, use=(True, True, True), po_grad=True, start_grad=True, backward=True):
    """Forward and autograd backward of the reference in `dtype`.  use: which of (pred_x, warped, masks) receive their gradient
    (gp, gw, gm).  Returns a dict of the compared tensors; a gradient nothing flows into is zeros, one not asked for is absent."""
    po = leaf(inp.po, dtype, po_grad and backward)
    st = leaf(inp.start, dtype, start_grad and backward)
    pred_x, warped, masks, ix, iy = warp_composite_ref(po, st, inp.grid_x, inp.grid_y, dtype)
    r = {"pred_x": pred_x.detach(), "warped": warped.detach(), "masks": masks.detach(), "ix": ix, "iy": iy}
    if not backward:
        return r
    picked = [(o, g.to(dtype)) for o, g, u in zip((pred_x, warped, masks), (inp.gp, inp.gw, inp.gm), use) if u and o.requires_grad]
    outs, gouts = [o for o, _ in picked], [g for _, g in picked]
    wrt = [v for v, u in ((po, po_grad), (st, start_grad)) if u]
    grads = list(torch.autograd.grad(outs, wrt, gouts, allow_unused=True))
    if po_grad:
        g_po = grads.pop(0)
        g_po = torch.zeros_like(po) if g_po is None else g_po
        r.update(g_flow=g_po[:, :, :2], g_inter=g_po[:, :, 2:2 + inp.c], g_logit=g_po[:, :, 2 + inp.c:])
    if start_grad:
        g_st = grads.pop(0)
        r["g_start"] = torch.zeros_like(st) if g_st is None else g_st
    return r


@functools.lru_cache(maxsize=None)
def warp_refs(key, subset=None):
    """(inputs, float32 result, float64 result) of a case, computed once per process and left unchanged."""
    inp = warp_inputs(key)
    kw = dict(WARP_SUBSETS[subset]) if subset else {}
    kw["backward"] = inp.name not in WARP_FORWARD_ONLY
    return inp, warp_run_ref(inp, torch.float32, **kw), warp_run_ref(inp, torch.float64, **kw)


def compared(r, floors):
    """The (name, floor) pairs of the tensors that a result dict holds."""
    return [(k, f) for k, f in floors.items() if r.get(k) is not None]


# ---- BatchNorm2d -> ReLU (-> bilinear x2 upsampling) --------------------------------------------------------------------------------
def bn_relu_up_ref(x, bn, upsample, conv_bias, dtype):
    """relu(bn(x + conv_bias)) [upsampled x2] by a deep copy of `bn` cast to `dtype` (torch's own BatchNorm: a two-pass variance).
    Returns the output, the pre-activation and the module copy, for its buffers and gradients."""
    mod = copy.deepcopy(bn).to(dtype)
    x = x.to(dtype)
    if conv_bias is not None:
        x = x + conv_bias.to(dtype).view(1, -1, 1, 1)
    pre = mod(x)
    out = torch.relu(pre)
    if upsample:
        out = F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
    return out, pre, mod


def _bn_case(name, shape, training, upsample, **kw):
    d = dict(name=name, shape=shape, training=training, upsample=upsample, affine=True, track=True, momentum=0.1, conv_bias=False,
             frozen=False, layout="contiguous", offset=None)
    d.update(kw)
    return SimpleNamespace(**d)


def _bn_cases():
    cases = []
    # a batch above kBnSplit = 64 (a workgroup of the two reductions takes a second image; C = 3, H = 1 and the smallest width);
    # C off the 64-thread blocks of the finalize kernels, odd H, batch 1; odd H with upsampling at a W that is no power of two
    for shape in ((70, 8, 2, 4), (130, 3, 1, 4), (2, 65, 3, 4), (1, 200, 5, 8), (3, 16, 7, 12)):
        for training in (True, False):
            for upsample in (True, False):
                tag = "x".join(map(str, shape))
                cases.append(_bn_case(f"{tag}.{'train' if training else 'eval'}.{'up' if upsample else 'flat'}", shape, training, upsample))
    v = (4, 16, 6, 8)
    cases += [
        _bn_case("noaffine.train.up", v, True, True, affine=False),
        _bn_case("noaffine.train.flat.cb", v, True, False, affine=False, conv_bias=True),
        _bn_case("noaffine.eval.up.cb", v, False, True, affine=False, conv_bias=True),
        _bn_case("noaffine.eval.flat.cb", v, False, False, affine=False, conv_bias=True),
        _bn_case("notrack.train.up", v, True, True, track=False),
        _bn_case("notrack.eval.up", v, False, True, track=False),
        _bn_case("notrack.eval.flat.cb", v, False, False, track=False, conv_bias=True),
        _bn_case("momentum1.train.up", v, True, True, momentum=1.0),
        _bn_case("momentum001.train.flat", v, True, False, momentum=0.01),
        _bn_case("frozen.train.up", v, True, True, frozen=True),
        _bn_case("frozen.eval.flat", v, False, False, frozen=True),
        _bn_case("channels_last.train.up", v, True, True, layout="channels_last"),
        _bn_case("channels_last.eval.flat", v, False, False, layout="channels_last"),
        _bn_case("slice.train.up", v, True, True, layout="slice"),
        _bn_case("slice.eval.flat", v, False, False, layout="slice"),
        _bn_case("offset.train.up", v, True, True, offset=BN_OFFSET),
        _bn_case("offset.train.flat", v, True, False, offset=BN_OFFSET),
    ]
    return {c.name: c for c in cases}


# x = offset + amplitude * noise, noise uniform in [-1, 1): a common offset of 35 standard deviations.  In float32, sums of x and x * x
# would leave the variance 1200 * 6e-8 = 7e-5 off (the output floor is 2e-6); the float64 sums of the kernel lose nothing.  No larger
# ratio can be asked of a float32 implementation at these floors: the batch mean itself is rounded to float32 (ulp(300) / sqrt(12) =
# 9e-6, over a standard deviation of 8.7: 1e-6 of the normalised value).  At 300 + 0.05 * noise torch's own float32 BatchNorm is 4e-4
# from its float64 (and flips ReLU masks).
BN_OFFSET = (300.0, 15.0)
BN_CASES = _bn_cases()
BN_KEYS = tuple(BN_CASES)


def bn_module(case):
    """The nn.BatchNorm2d of a case on the CPU in float32, parameters and running statistics from conftest.procedural_tensor."""
    c = case.shape[1]
    seed = 9000 + 16 * BN_KEYS.index(case.name)
    bn = torch.nn.BatchNorm2d(c, momentum=case.momentum, affine=case.affine, track_running_stats=case.track)
    with torch.no_grad():
        if case.affine:
            bn.weight.copy_(procedural_tensor((c,), seed + 1, 0.5, 1.5))
            bn.bias.copy_(procedural_tensor((c,), seed + 2, -0.5, 0.5))
        if case.track:
            bn.running_mean.copy_(procedural_tensor((c,), seed + 3, -0.3, 0.3))
            bn.running_var.copy_(procedural_tensor((c,), seed + 4, 0.5, 1.5))
    if case.frozen:
        bn.weight.requires_grad_(False)
        bn.bias.requires_grad_(False)
    return bn.train(case.training)


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """The float32 inputs of a BatchNorm case: module, x (contiguous; `in_layout` gives it the case's memory layout), conv_bias, gout.
    Inputs whose float64 pre-activation lies within KINK_MARGIN of 0 are moved by BN_NUDGE, as test_bn_relu_up_matches_torch does."""
    case = BN_CASES[name]
    n, c, h, w = case.shape
    seed = 9000 + 16 * BN_KEYS.index(name)
    bn = bn_module(case)
    if case.offset is None:
        x = procedural_tensor(case.shape, seed, -2.3, 2.9)       # mean 0.3, standard deviation 1.5
    else:
        x = case.offset[0] + case.offset[1] * procedural_tensor(case.shape, seed, -1.0, 1.0)
    cb = procedural_tensor((c,), seed + 5, -0.7, 0.7) if case.conv_bias else None
    for _ in range(16):
        with torch.no_grad():
            near = bn_relu_up_ref(x, bn, False, cb, torch.float64)[1].abs() < KINK_MARGIN
        if not bool(near.any()):
            break
        x = x + near.float() * BN_NUDGE
    else:
        raise AssertionError(f"BatchNorm case {name}: nudging did not clear the ReLU kink")
    gout = procedural_tensor((n, c, 2 * h, 2 * w) if case.upsample else case.shape, seed + 6, -1.0, 1.0)
    return SimpleNamespace(case=case, bn=bn, x=x, cb=cb, gout=gout, filler=procedural_tensor(case.shape, seed + 7, -1.0, 1.0))


def in_layout(inp, x):
    """`x` (the case's input on any device) as the view the case hands to the op: contiguous, channels-last, or every other channel of
    a tensor of twice the channels."""
    layout = inp.case.layout
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    elif layout == "slice":
        full = torch.stack([x, inp.filler.to(x.device)], dim=2).flatten(1, 2)   # channels x0, f0, x1, f1, ...
        x = full[:, ::2]
        assert not x.is_contiguous()
    return x


def bn_run_ref(inp, dtype):
    case = inp.case
    x = leaf(inp.x, dtype)
    cb = leaf(inp.cb, dtype) if inp.cb is not None else None
    out, pre, mod = bn_relu_up_ref(x, inp.bn, case.upsample, cb, dtype)
    out.backward(inp.gout.to(dtype))
    learns = case.affine and not case.frozen
    return {"out": out.detach(), "pre": pre.detach(), "gx": x.grad, "gw": mod.weight.grad if learns else None,
            "gb": mod.bias.grad if learns else None, "gcb": cb.grad if cb is not None else None,
            "running_mean": mod.running_mean, "running_var": mod.running_var,
            "num_batches_tracked": None if mod.num_batches_tracked is None else int(mod.num_batches_tracked)}


def bn_uses_batch_statistics(case):
    return case.training or not case.track


def bn_compared(case, r):
    """The (name, floor) pairs of a BatchNorm case.  Under batch statistics a constant in front of BatchNorm has no gradient: the
    reference's conv_bias gradient is round-off there, and is not compared by a relative error."""
    return [(k, f) for k, f in compared(r, BN_FLOORS) if not (k == "gcb" and bn_uses_batch_statistics(case))]


@functools.lru_cache(maxsize=None)
def bn_refs(name):
    inp = bn_inputs(name)
    return inp, bn_run_ref(inp, torch.float32), bn_run_ref(inp, torch.float64)


# ---- bilinear x2 upsampling of (..., H, W) -----------------------------------------------------------------------------------------------
UP_SHAPES = {"5d": (2, 3, 4, 6, 8), "3d": (5, 3, 2)}
UP_KEYS = tuple(UP_SHAPES)


def up_run_ref(x, gout, dtype):
    """F.interpolate(scale_factor=2, bilinear, align_corners=False) on the flattened planes of x (..., H, W), and its autograd backward."""
    h, w = x.shape[-2:]
    xr = leaf(x, dtype)
    out = F.interpolate(xr.reshape(1, -1, h, w), scale_factor=2, mode="bilinear", align_corners=False).reshape(gout.shape)
    out.backward(gout.to(dtype))
    return {"out": out.detach(), "gx": xr.grad}


@functools.lru_cache(maxsize=None)
def up_refs(key):
    shape = UP_SHAPES[key]
    seed = 11000 + 4 * UP_KEYS.index(key)
    x = procedural_tensor(shape, seed, -1.0, 1.0)
    gout = procedural_tensor(shape[:-2] + (2 * shape[-2], 2 * shape[-1]), seed + 1, -1.0, 1.0)
    return SimpleNamespace(x=x, gout=gout), up_run_ref(x, gout, torch.float32), up_run_ref(x, gout, torch.float64)
