"""The three hand-written kernels behind VidODE's flow / mask / warp decoder (csrc/warp.hip, csrc/bn_relu_up.hip, csrc/upsample.hip) at
the shapes their entry points accept and the model never runs: non-square and tiny images, H*W off the 256 threads, 2 and 4 image
channels, one step, every coordinate clamped, two grid arrays of different values, null operands of the warp backward; batches above
the 64 partial sums of the BatchNorm reductions, channel counts off the 64-thread finalize blocks, H = 1 and odd H under upsampling,
BatchNorm without affine parameters / without running statistics / with another momentum / with frozen parameters, non-contiguous
input, a common offset of 35 standard deviations; 3-D and 5-D input of the upsampling; and the refusals.

Yardstick: tests/_flow_tail_ref.py in float64 on the CPU.  A HIP tensor may sit max(4 x d32, floor) from it (`bound`), d32 being the
distance of the same reference run in float32; the floors are those of tests/test_hip_vidode.py, and tests/test_flow_tail_ref_cpu.py
shows d32 <= floor for every tensor of every case here, so the bound in force is at most 4 x the floor.  Every figure is recorded as
flowtail.<op>.<case>.<tensor>."""
import copy

import pytest
import torch

import _flow_tail_ref as ref
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu


def _compare(op, case, got, r32, r64, pairs):
    """Every tensor of `pairs` against the float64 reference: all figures are printed and recorded before the first assertion."""
    assert pairs
    lines, failed = [], []
    for name, floor in pairs:
        assert got[name].shape == r64[name].shape, (name, got[name].shape, r64[name].shape)
        bnd, d32 = ref.bound(r32[name], r64[name], floor)
        err = record(f"flowtail.{op}.{case}.{name}", rel_l2(got[name], r64[name]))
        lines.append(f"flowtail.{op}.{case}.{name}: hip {err:.3e}  d32 {d32:.3e}  bound {bnd:.3e}")
        if not err <= bnd:
            failed.append(lines[-1])
    print("\n".join(lines))
    assert not failed, "\n".join(failed)


# ---- warp chain ------------------------------------------------------------------------------------------------------------------------
def _warp_hip(inp, cuda, use=(True, True, True), po_grad=True, start_grad=True, backward=True):
    """autograd.warp_composite and its backward on the GPU; also: the inference path without a graph returns the same bits."""
    from ode_rl_amd.autograd import warp_composite
    po = inp.po.to(cuda).requires_grad_(po_grad and backward)
    st = inp.start.to(cuda).requires_grad_(start_grad and backward)
    gx, gy = inp.grid_x.to(cuda), inp.grid_y.to(cuda)
    outs = warp_composite(po, st, gx, gy)
    got = {k: o.detach() for k, o in zip(("pred_x", "warped", "masks"), outs)}
    if backward:
        assert all(o.requires_grad for o in outs)
        picked = [(o, g.to(cuda)) for o, g, u in zip(outs, (inp.gp, inp.gw, inp.gm), use) if u]
        torch.autograd.backward([o for o, _ in picked], [g for _, g in picked])
        if po_grad:
            got.update(_split_g_po(po.grad, inp.c))
        if start_grad:
            got["g_start"] = st.grad
    with torch.no_grad():
        plain = warp_composite(inp.po.to(cuda), inp.start.to(cuda), gx, gy)
    assert not any(o.requires_grad for o in plain)
    for k, o in zip(("pred_x", "warped", "masks"), plain):
        assert torch.equal(o, got[k]), k
    return got, po, st


def _split_g_po(g_po, c):
    return {"g_flow": g_po[:, :, :2], "g_inter": g_po[:, :, 2:2 + c], "g_logit": g_po[:, :, 2 + c:]}


@pytest.mark.parametrize("key", [k for k in ref.WARP_KEYS if k.partition(".")[0] not in ref.WARP_FORWARD_ONLY])
def test_warp_chain_against_float64_autograd(cuda, key):
    inp, r32, r64 = ref.warp_refs(key)
    got, _, _ = _warp_hip(inp, cuda)
    pairs = ref.compared(r64, ref.WARP_FLOORS)
    assert len(pairs) == 7
    _compare("warp", key, got, r32, r64, pairs)
    if inp.name not in ref.WARP_ALL_CLAMPED:
        return
    ix, iy = r64["ix"], r64["iy"]
    assert bool(((ix <= 0) | (ix >= inp.w - 1)).all()) and bool(((iy <= 0) | (iy >= inp.h - 1)).all())
    bi = torch.arange(inp.b).view(inp.b, 1, 1)
    for side, start in ((r64, inp.start.double()), ({k: v.cpu() for k, v in got.items()}, inp.start)):
        # every sample is the border pixel of the image before it that its quadrant points at, replicated exactly
        for t in range(inp.t):
            prev = start if t == 0 else side["warped"][:, t - 1]
            cx = torch.where(ix[:, t] <= 0, 0, inp.w - 1)
            cy = torch.where(iy[:, t] <= 0, 0, inp.h - 1)
            assert len({int(v) for v in (cx + inp.w * cy).unique()}) == 4   # all four corners are used
            assert torch.equal(side["warped"][:, t], prev[bi, :, cy, cx].permute(0, 3, 1, 2))
        assert float(side["g_flow"].abs().max()) == 0.0   # a clamped coordinate has no gradient: exactly
        assert float(side["g_start"].abs().max()) > 0.0


@pytest.mark.parametrize("subset", sorted(ref.WARP_SUBSETS))
def test_warp_backward_operand_subsets(cuda, subset):
    """The backward with operands missing, through autograd (which hands the Function zeros for an output nothing flowed into) and
    through hip_ops.warp_composite_backward with the null operands themselves."""
    from ode_rl_amd import hip_ops
    key, kw = ref.WARP_SUBSET_CASE, ref.WARP_SUBSETS[subset]
    inp, r32, r64 = ref.warp_refs(key, subset)
    got, po, st = _warp_hip(inp, cuda, **kw)
    pairs = ref.compared(r64, ref.WARP_FLOORS)
    assert len(pairs) == 3 + (3 if kw["po_grad"] else 0) + (1 if kw["start_grad"] else 0)
    _compare("warp", f"{key}.{subset}", got, r32, r64, pairs)
    if not kw["start_grad"]:
        assert st.grad is None and "g_start" not in got
    if not kw["po_grad"]:
        assert po.grad is None
    if subset == "po_frozen":   # (the entry point always writes the gradient of pred_outputs: nothing of it is null here)
        return
    # the entry point itself, null where the subset has no operand
    gp, gw, gm = (g.to(cuda) if u else None for g, u in zip((inp.gp, inp.gw, inp.gm), kw["use"]))
    g_po, g_start = hip_ops.warp_composite_backward(po.detach(), st.detach(), got["warped"], inp.grid_x.to(cuda), inp.grid_y.to(cuda),
                                                    gp, gw, gm, kw["start_grad"])
    direct = dict(got, **_split_g_po(g_po, inp.c))
    assert (g_start is None) == (not kw["start_grad"])
    if g_start is not None:
        direct["g_start"] = g_start
    _compare("warp", f"{key}.{subset}.direct", direct, r32, r64, pairs)
    if subset == "from_masks":   # nothing reaches the frames: exactly zero, on both sides and by both routes
        for side in (r64, got, direct):
            assert float(side["g_inter"].abs().max()) == 0.0 and float(side["g_flow"].abs().max()) == 0.0 and float(side["g_start"].abs().max()) == 0.0
        assert float(got["g_logit"].abs().max()) > 0.0


def test_warp_backward_that_does_not_fit_in_lds_is_refused_at_the_call(cuda):
    """c = 4 at 64 x 64: the forward's two images fit in LDS (128 KiB), the backward's three do not (192 KiB).  Inputs that require grad
    are refused by autograd.warp_composite itself, not from inside loss.backward(); without a graph the forward runs."""
    from ode_rl_amd import hip_ops
    from ode_rl_amd.autograd import warp_composite
    inp, r32, r64 = ref.warp_refs("c4_64x64")
    assert (inp.c, inp.h, inp.w) == (4, 64, 64)
    gx, gy = inp.grid_x.to(cuda), inp.grid_y.to(cuda)
    for po_grad, start_grad in ((True, True), (True, False), (False, True)):
        po, st = inp.po.to(cuda).requires_grad_(po_grad), inp.start.to(cuda).requires_grad_(start_grad)
        with pytest.raises(ValueError, match=r"backward of a 4x64x64 image needs 192 KiB of LDS"):
            warp_composite(po, st, gx, gy)
    assert not hip_ops.warp_composite_backward_supported(4, 64, 64)
    assert hip_ops.warp_composite_backward_supported(4, 48, 40) and hip_ops.warp_composite_backward_supported(3, 64, 64)
    got, _, _ = _warp_hip(inp, cuda, backward=False)
    pairs = ref.compared(r64, ref.WARP_FLOORS)
    assert [k for k, _ in pairs] == ["pred_x", "warped", "masks"]
    _compare("warp", "c4_64x64", got, r32, r64, pairs)
    # the backward entry point still refuses it
    with pytest.raises(ValueError, match="does not fit in LDS"):
        hip_ops.warp_composite_backward(inp.po.to(cuda), inp.start.to(cuda), got["warped"], gx, gy, inp.gp.to(cuda), None, None, True)


# ---- BatchNorm2d -> ReLU (-> upsampling) ---------------------------------------------------------------------------------------------
def _bn_hip(inp, cuda, training=None):
    from ode_rl_amd.autograd import bn_relu_up
    case = inp.case
    bnd = copy.deepcopy(inp.bn).to(cuda)
    if training is not None:
        bnd.train(training)
    xd = ref.in_layout(inp, inp.x.to(cuda)).detach().requires_grad_(True)
    assert xd.is_contiguous() == (case.layout == "contiguous")
    cbd = inp.cb.to(cuda).requires_grad_(True) if inp.cb is not None else None
    out = bn_relu_up(xd, bnd, case.upsample, conv_bias=cbd)
    out.backward(inp.gout.to(cuda))
    return {"out": out.detach(), "gx": xd.grad, "gw": bnd.weight.grad if case.affine else None, "gb": bnd.bias.grad if case.affine else None,
            "gcb": cbd.grad if cbd is not None else None, "running_mean": bnd.running_mean, "running_var": bnd.running_var,
            "num_batches_tracked": None if bnd.num_batches_tracked is None else int(bnd.num_batches_tracked)}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", ref.BN_KEYS)
def test_bn_relu_up_against_float64(cuda, name):
    inp, r32, r64 = ref.bn_refs(name)
    case = inp.case
    got = _bn_hip(inp, cuda)
    pairs = ref.bn_compared(case, r64)
    _compare("bn", name, got, r32, r64, pairs)
    assert got["num_batches_tracked"] == r64["num_batches_tracked"]
    for k in ("gw", "gb", "gcb", "running_mean", "running_var"):   # what the reference does not have, the op does not invent
        if r64[k] is None:
            assert got[k] is None, k
    if case.conv_bias and ref.bn_uses_batch_statistics(case):   # a constant in front of batch statistics: no gradient, exactly
        assert float(got["gcb"].abs().max()) == 0.0
    _same_bits(got, _bn_hip(inp, cuda))
    if not case.track and not case.training:   # eval() without running statistics IS the train() computation
        again = _bn_hip(inp, cuda, training=True)
        assert got["running_mean"] is None and got["num_batches_tracked"] is None
        _same_bits(got, again)


def test_bn_relu_up_refusals_come_before_any_launch(cuda):
    from ode_rl_amd import hip_ops
    from ode_rl_amd.autograd import bn_relu_up
    bn = torch.nn.BatchNorm2d(4).to(cuda)
    before = copy.deepcopy(bn.state_dict())

    def untouched(mod):
        return all(torch.equal(v, before[k]) for k, v in mod.state_dict().items())

    for x in (torch.ones(2, 4, 3, 6, device=cuda), torch.ones(2, 4, 3, 6, device=cuda, requires_grad=True), torch.ones(2, 4, 8, 2, device=cuda)):
        with pytest.raises(ValueError, match="W % 4 == 0"):
            bn_relu_up(x, bn, False)
        with pytest.raises(ValueError, match="W % 4 == 0"):
            hip_ops.bn_relu_up_forward(x.detach(), bn, True)
    assert untouched(bn)
    cumulative = torch.nn.BatchNorm2d(4, momentum=None).to(cuda)
    for x in (torch.ones(2, 4, 3, 8, device=cuda), torch.ones(2, 4, 3, 8, device=cuda, requires_grad=True)):
        with pytest.raises(ValueError, match="momentum=None"):
            bn_relu_up(x, cumulative, True)
    assert untouched(cumulative) and int(cumulative.num_batches_tracked) == 0
    x = torch.ones(2, 4, 3, 8, device=cuda)
    for upsample, bad in ((True, (2, 4, 3, 8)), (False, (2, 4, 6, 16)), (True, (2, 4, 6, 15)), (False, (2, 3, 3, 8))):
        _, saved = hip_ops.bn_relu_up_forward(x, bn, upsample)
        with pytest.raises(ValueError, match="gradient of shape"):
            hip_ops.bn_relu_up_backward(torch.ones(bad, device=cuda), x, saved, upsample)


# ---- upsampling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ref.UP_KEYS)
def test_upsample2x_takes_any_number_of_leading_dimensions(cuda, key):
    from ode_rl_amd.autograd import upsample2x
    inp, r32, r64 = ref.up_refs(key)
    xd = inp.x.to(cuda).requires_grad_(True)
    out = upsample2x(xd)
    out.backward(inp.gout.to(cuda))
    got = {"out": out.detach(), "gx": xd.grad}
    _compare("up", key, got, r32, r64, ref.compared(r64, ref.UP_FLOORS))
    with torch.no_grad():
        assert torch.equal(upsample2x(inp.x.to(cuda)), got["out"])


def test_upsample2x_refuses_an_odd_width(cuda):
    from ode_rl_amd import hip_ops
    from ode_rl_amd.autograd import upsample2x
    for shape in ((2, 3, 4, 5), (4, 1), (2, 2, 2, 6, 7)):
        for grad in (False, True):
            with pytest.raises(ValueError, match="even W"):
                upsample2x(torch.ones(shape, device=cuda, requires_grad=grad))
    for shape in ((2, 3, 8, 7), (2, 3, 7, 8), (6, 1)):
        with pytest.raises(ValueError, match=r"needs \(\.\.\., 2H, 2W\)"):
            hip_ops.upsample2x_backward(torch.ones(shape, device=cuda))
