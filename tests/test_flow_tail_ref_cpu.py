"""The references and cases of tests/_flow_tail_ref.py, checked without a GPU: (i) the float32 restatement of the warp chain IS
oracle/vidode_ref.py::warp_composite, bit for bit; (ii) every case that tests/test_hip_flow_tail_shapes.py runs meets the conditions
under which a relative bound means something -- no float64 source coordinate within 1e-3 pixel of an integer or of the border clamp,
no BatchNorm pre-activation within 1e-4 of the ReLU kink; (iii) for every compared tensor of every case the float32 restatement sits
no further from the float64 one than that tensor's floor, so the bound in force on the GPU is the floor and not an inflated one."""
import pytest
import torch

import _flow_tail_ref as ref
from conftest import rel_l2


def test_float32_restatement_is_the_oracle_bit_for_bit():
    """At the first case of test_hip_vidode.py::test_warp_chain_kernel_forward_and_backward (B=3, T=4, c=1, 64x64, flows of 6 pixels)."""
    from oracle import vidode_ref
    b, t, c, gain = 3, 4, 1, 6.0
    gen = torch.Generator().manual_seed(b * 100 + t)
    po = torch.randn(b, t, c + 3, 64, 64, generator=gen)
    po[:, :, :2] *= gain
    start = torch.rand(b, c, 64, 64, generator=gen)
    gouts = [torch.randn(b, t, c, 64, 64, generator=gen), torch.randn(b, t, c, 64, 64, generator=gen) * 0.3,
             torch.randn(b, t, 1, 64, 64, generator=gen) * 0.3]
    po_o, st_o = po.clone().requires_grad_(True), start.clone().requires_grad_(True)
    want = vidode_ref.warp_composite(po_o, st_o)
    want_g = torch.autograd.grad(list(want), [po_o, st_o], gouts)
    po_r, st_r = po.clone().requires_grad_(True), start.clone().requires_grad_(True)
    grid = torch.linspace(-1.0, 1.0, 64)
    got = warp = ref.warp_composite_ref(po_r, st_r, grid, grid, torch.float32)
    got_g = torch.autograd.grad(list(got[:3]), [po_r, st_r], gouts)
    for a, e in zip(got[:3] + got_g, want + want_g):
        assert a.dtype == torch.float32 and torch.equal(a, e)
    # the coordinates it reports are those grid_sample was given
    ix, iy = warp[3], warp[4]
    assert ix.shape == iy.shape == (b, t, 64, 64)
    x = torch.arange(64.0).view(1, 1, 1, 64)
    y = torch.arange(64.0).view(1, 1, 64, 1)
    # (g + 1) W / 2 - 1/2 with g = (x + flow) / ((W - 1) / 2) - 1
    assert float((ix - ((x + po[:, :, 0]) * 64 / 63 - 0.5)).abs().max()) <= 1e-4 and float((iy - ((y + po[:, :, 1]) * 64 / 63 - 0.5)).abs().max()) <= 1e-4


@pytest.mark.parametrize("key", ref.WARP_KEYS)
def test_warp_cases_stay_off_integers_and_borders(key):
    inp, _, r64 = ref.warp_refs(key)
    ix, iy = r64["ix"], r64["iy"]
    assert ix.dtype == torch.float64 and ix.shape == iy.shape == (inp.b, inp.t, inp.h, inp.w)
    if inp.name in ref.WARP_ALL_CLAMPED:   # exempt by construction: every coordinate is thousands of pixels outside
        assert bool(((ix < -1000) | (ix > inp.w + 1000)).all()) and bool(((iy < -1000) | (iy > inp.h + 1000)).all())
        return
    d_int, d_border = ref.coordinate_margins(ix, iy, inp.h, inp.w)
    assert d_int >= ref.INTEGER_MARGIN and d_border >= ref.BORDER_MARGIN, (d_int, d_border)
    # the case still has both kinds of sample: clamped ones and interior ones
    inside = (ix > 0) & (ix < inp.w - 1) & (iy > 0) & (iy < inp.h - 1)
    assert 0 < int(inside.sum()) < inside.numel()


def _assert_floors(r32, r64, pairs, what):
    worst = {}
    for name, floor in pairs:
        worst[name] = d32 = rel_l2(r32[name], r64[name])
        assert d32 <= floor, f"{what}.{name}: d32 = {d32:.3e} above the floor {floor:.0e}"
    return worst


@pytest.mark.parametrize("key", ref.WARP_KEYS)
def test_warp_float32_restatement_is_within_every_floor(key):
    inp, r32, r64 = ref.warp_refs(key)
    pairs = ref.compared(r64, ref.WARP_FLOORS)
    assert len(pairs) == (3 if inp.name in ref.WARP_FORWARD_ONLY else 7)
    _assert_floors(r32, r64, pairs, f"warp.{key}")


@pytest.mark.parametrize("subset", sorted(ref.WARP_SUBSETS))
def test_warp_operand_subsets_are_within_every_floor(subset):
    _, r32, r64 = ref.warp_refs(ref.WARP_SUBSET_CASE, subset)
    kw = ref.WARP_SUBSETS[subset]
    pairs = ref.compared(r64, ref.WARP_FLOORS)
    assert len(pairs) == 3 + (3 if kw["po_grad"] else 0) + (1 if kw["start_grad"] else 0)
    _assert_floors(r32, r64, pairs, f"warp.{ref.WARP_SUBSET_CASE}.{subset}")


@pytest.mark.parametrize("name", ref.BN_KEYS)
def test_bn_cases_stay_off_the_relu_kink(name):
    inp, _, r64 = ref.bn_refs(name)
    assert r64["pre"].dtype == torch.float64 and tuple(r64["pre"].shape) == inp.case.shape
    assert float(r64["pre"].abs().min()) >= ref.KINK_MARGIN
    frac = float((r64["pre"] > 0).double().mean())
    assert 0.05 < frac < 0.95, frac   # both ReLU branches are taken


@pytest.mark.parametrize("name", ref.BN_KEYS)
def test_bn_float32_restatement_is_within_every_floor(name):
    inp, r32, r64 = ref.bn_refs(name)
    case = inp.case
    pairs = ref.bn_compared(case, r64)
    want = {"out", "gx"} | ({"gw", "gb"} if case.affine and not case.frozen else set()) | ({"running_mean", "running_var"} if case.track else set())
    if case.conv_bias and not ref.bn_uses_batch_statistics(case):
        want.add("gcb")
    assert {k for k, _ in pairs} == want
    _assert_floors(r32, r64, pairs, f"bn.{name}")
    assert r32["num_batches_tracked"] == r64["num_batches_tracked"] == ((1 if case.training else 0) if case.track else None)
    if case.conv_bias and ref.bn_uses_batch_statistics(case):   # what is not compared by a relative error is round-off
        assert float(r64["gcb"].abs().max()) <= 1e-9 * float(inp.gout.abs().sum())


def test_bn_layouts_hand_over_the_same_values():
    for name in ref.BN_KEYS:
        inp = ref.bn_inputs(name)
        v = ref.in_layout(inp, inp.x)
        assert torch.equal(v, inp.x) and v.is_contiguous() == (inp.case.layout == "contiguous")


@pytest.mark.parametrize("key", ref.UP_KEYS)
def test_upsample_float32_restatement_is_within_every_floor(key):
    inp, r32, r64 = ref.up_refs(key)
    assert r64["out"].shape == inp.gout.shape and r64["gx"].shape == inp.x.shape
    _assert_floors(r32, r64, ref.compared(r64, ref.UP_FLOORS), f"up.{key}")


def test_bound_is_the_projects_rule():
    import _convgru_ref
    a, b = torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0 + 1e-3])
    assert ref.bound(a, b, 1e-6) == _convgru_ref.bound(a, b, 1e-6) == (4.0 * rel_l2(a, b), rel_l2(a, b))
    assert ref.bound(a, a, 1e-6) == (1e-6, 0.0)
