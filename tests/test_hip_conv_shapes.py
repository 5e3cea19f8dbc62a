"""The forward convolutions at the channel shapes their argument checks accept but no other test runs: every instantiation
`launch_conv` (csrc/conv_q4.hip) can pick -- resident / ring / Winograd F(2x2,3x3) / F(2x2,5x5) unsplit and split / bf16 3x3 / bf16 5x5
ring -- at chunk counts below, at and past the depth of its ring, with a source boundary on and inside a chunk, with 96 / 160 output
channels, and every "decline" of a front kernel to the one behind it; then the ConvGRU cell and the dynamics stacks at such widths.

Reference: F.conv2d in float64 on the CPU (tests/_conv_cases.py).  Bounds: the per-family rel-L2 bounds of test_hip_conv.py and
test_hip_bf16.py (direct 2e-6, Winograd 3x3 5e-6, Winograd 5x5 1e-5, bf16 against the bf16-rounded reference 1e-5); the CPU test below
shows that the float32 CPU conv sits at most a quarter of the bound from the reference for every case.  A front kernel that runs must
not reproduce the direct kernel's bits; one that declines must.  Every call is repeated and must be bitwise reproducible."""
import ctypes
import os

import pytest
import torch

import _conv_cases as cc
import _convgru_ref
from conftest import record, rel_l2


# ---------------------------------------------------------------------------------------------------- the references alone (CPU)
def _all_layer_cases():
    """(family, case, bf16 reference?) of every layer case: a declined case is held to the bound of the direct kernel it falls to."""
    out = [("direct", c, False) for c in cc.DIRECT]
    out += [("wino3", c, False) for c in cc.WINO3_RUN] + [("direct", c, False) for c in cc.WINO3_DECLINE]
    out += [("wino5", k + (5, False, True), False) for k in cc.WINO5]
    out += [("bf16", c, True) for c in cc.BF16_3X3_RUN + cc.BF16_5X5_RUN]
    out += [("direct", c, False) for c in cc.BF16_3X3_DECLINE + [cc.BF16_5X5_OVER_LDS, cc.BF16_5X5_PACK_REFUSES]]
    return out


def test_references_leave_three_quarters_of_every_bound():
    """4 * d32 <= the family bound for every layer and input-gradient case (d32: float32 CPU conv against the float64 one), and the
    split labels of the F(2x2,5x5) table are what launch_wino5's rule gives."""
    worst = {}
    for fam, case, bf16 in _all_layer_cases():
        d32 = cc.layer_reference(case, bf16)[1]
        assert 4.0 * d32 <= cc.BOUND[fam], (fam, case, d32)
        worst[fam] = max(worst.get(fam, 0.0), d32)
    for b, cin, cout, fam in cc.WINO3_DGRAD:
        assert 4.0 * cc.dgrad_reference(b, cin, cout, 3)[3] <= cc.BOUND[fam], (cin, cout)
    b, c1, c2, cout = cc.WINO5_DGRAD
    assert 4.0 * cc.dgrad_reference(b, c1 + c2, cout, 5)[3] <= cc.BOUND["wino5"]
    for (b, c1, c2, cout), label in cc.WINO5.items():
        assert cc.wino5_split(b, c1 + c2, cout) == label, (b, c1, c2, cout)
    assert {s for s, _ in cc.WINO5.values()} == {1, 2, 4, 8}
    b, c1, c2, cout = cc.WINO5_DGRAD
    assert cc.wino5_split(b, cout, c1 + c2) == (4, 3)      # the input-gradient conv: 96 -> 64
    print("worst d32 per family:", worst)


# -------------------------------------------------------------------------------------------------------------------- GPU side
def _pack(kind, w, transpose_flip=False):
    from ode_rl_amd import hip_ops
    fn = {"direct": hip_ops.pack_conv_weight, "wino3": hip_ops.pack_conv_weight_winograd, "wino5": hip_ops.pack_conv_weight_winograd5,
          "bf16_3": hip_ops.pack_conv_weight_bf16, "bf16_5": hip_ops.pack_conv_weight_bf16_ks}[kind]
    return fn(w, transpose_flip=transpose_flip)


def _run(dev, case, front=None):
    """The layer through hip_ops.conv_q4 with the direct image and, if named, one front image ("wino3", "wino5", "bf16_3", "bf16_5")."""
    from ode_rl_amd import hip_ops
    b, cin1, cin2, cout, ks, relu, with_bias = case
    x, w, bias = cc.layer_values(b, cin1 + cin2, cout, ks, with_bias)
    xd, wd = x.to(dev), w.to(dev)
    src1 = hip_ops.nchw_to_q4(xd[:, :cin1].contiguous())
    src2 = hip_ops.nchw_to_q4(xd[:, cin1:].contiguous()) if cin2 else None
    kw = {}
    if front is not None:
        kw["w_bf16" if front.startswith("bf16") else "w_wino"] = _pack(front, wd)
    out = hip_ops.q4_to_nchw(hip_ops.conv_q4(src1, _pack("direct", wd), None if bias is None else bias.to(dev), cout, ks, src2=src2,
                                             relu=relu, **kw))
    assert out.shape == (b, cout, 16, 16)
    return out.cpu()


def _check(dev, fam, case, front, runs, bf16_ref=False, repeats=2, label=None):
    """The case against its reference under the family bound; a front kernel that runs differs from the direct kernel's bits, one that
    declines reproduces them; `repeats` launches are bitwise equal."""
    ref, _ = cc.layer_reference(case, bf16_ref)
    out = _run(dev, case, front)
    label = label or fam
    err = record(f"conv_shapes.{label}.{cc.case_id(case)}", rel_l2(out, ref))
    print(f"{label} {cc.case_id(case)}: rel-L2 {err:.3e} (bound {cc.BOUND[fam]:.0e})")
    for _ in range(repeats - 1):
        assert torch.equal(_run(dev, case, front), out), "not reproducible"
    if front is not None:
        direct = _run(dev, case)
        assert torch.equal(out, direct) == (not runs), "the front kernel ran" if not runs else "the front kernel did not run"
    assert bool(torch.isfinite(out).all())
    assert err <= cc.BOUND[fam], err


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.DIRECT, ids=cc.case_id)
def test_direct_fp32(cuda, case):
    _check(cuda, "direct", case, None, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.WINO3_RUN, ids=cc.case_id)
def test_winograd3_runs(cuda, case):
    _check(cuda, "wino3", case, "wino3", True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.WINO3_DECLINE, ids=cc.case_id)
def test_winograd3_declines_to_the_direct_kernels(cuda, case):
    """5, 6 and 16 chunks have no F(2x2,3x3) instantiation (pack_conv_weight_winograd packs them all the same), two sources none either:
    with the Winograd image the call gives the bits of the call without it."""
    _check(cuda, "direct", case, "wino3", False, label="wino3_declined")


@pytest.mark.gpu
@pytest.mark.parametrize("b,cin,cout,fam", cc.WINO3_DGRAD, ids=lambda v: str(v))
def test_winograd3_input_gradient_of_a_non_square_layer(cuda, b, cin, cout, fam):
    """The input gradient of a cin -> cout layer is a cout -> cin conv over the transposed + flipped weights, both images given:
    32 -> 96 gives a 96 -> 32 conv without a Winograd instantiation (ring kernel, bits of the call without the image); 64 -> 32 gives
    a 32 -> 64 conv on conv3x3_wino_kernel<2>."""
    from ode_rl_amd import hip_ops
    w, gy, ref, _ = cc.dgrad_reference(b, cin, cout, 3)
    wd, g = w.to(cuda), hip_ops.nchw_to_q4(gy.to(cuda))
    wp = hip_ops.pack_conv_weight(wd, transpose_flip=True)
    run = lambda **kw: hip_ops.q4_to_nchw(hip_ops.conv_q4(g, wp, None, cin, 3, **kw)).cpu()
    out = run(w_wino=hip_ops.pack_conv_weight_winograd(wd, transpose_flip=True))
    assert out.shape == ref.shape
    err = record(f"conv_shapes.{fam}.dgrad.{b}-{cin}-{cout}", rel_l2(out, ref))
    print(f"dgrad {cin}->{cout}: rel-L2 {err:.3e}")
    assert torch.equal(run(w_wino=hip_ops.pack_conv_weight_winograd(wd, transpose_flip=True)), out)
    assert torch.equal(out, run()) == (fam == "direct")
    assert err <= cc.BOUND[fam], err


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(cc.WINO5), ids=lambda k: cc.case_id(k) + "-S%d-share%d" % cc.WINO5[k])
def test_winograd5_runs(cuda, key):
    """Unsplit and split over S = 2 / 4 / 8 workgroups per tile (the id carries what launch_wino5's rule gives), odd shares, a source
    boundary inside a share; three launches for the split launches' last-arriver reduction."""
    assert "ODEHIP_WINO5_SPLIT" not in os.environ, "the split counts of this table hold for the library's default only"
    _check(cuda, "wino5", key + (5, False, True), "wino5", True, repeats=3)


@pytest.mark.gpu
def test_winograd5_declines_an_odd_first_source(cuda):
    """q1 = 3 quads: launch_wino5 declines and the direct ring kernel runs (bits of the call without the image)."""
    _check(cuda, "direct", cc.WINO5_DECLINE + (5, True, True), "wino5", False, label="wino5_declined")


@pytest.mark.gpu
def test_winograd5_input_gradient_of_a_two_source_layer(cuda):
    """(32 + 32) -> 96: the input gradient is a 96 -> 64 conv, 12 chunks split over S = 4 workgroups per tile."""
    from ode_rl_amd import hip_ops
    b, c1, c2, cout = cc.WINO5_DGRAD
    cin = c1 + c2
    w, gy, ref, _ = cc.dgrad_reference(b, cin, cout, 5)
    wd, g = w.to(cuda), hip_ops.nchw_to_q4(gy.to(cuda))
    wp = hip_ops.pack_conv_weight(wd, transpose_flip=True)
    run = lambda **kw: hip_ops.q4_to_nchw(hip_ops.conv_q4(g, wp, None, cin, 5, **kw)).cpu()
    out = run(w_wino=hip_ops.pack_conv_weight_winograd5(wd, transpose_flip=True))
    err = record(f"conv_shapes.wino5.dgrad.{b}-{cin}-{cout}", rel_l2(out, ref))
    print(f"dgrad {cin}->{cout} 5x5: rel-L2 {err:.3e}")
    for _ in range(2):
        assert torch.equal(run(w_wino=hip_ops.pack_conv_weight_winograd5(wd, transpose_flip=True)), out)
    direct = run()
    assert not torch.equal(out, direct)
    assert rel_l2(direct, ref) <= cc.BOUND["direct"]
    assert err <= cc.BOUND["wino5"], err


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.BF16_3X3_RUN + cc.BF16_5X5_RUN, ids=cc.case_id)
def test_bf16_runs(cuda, case):
    """bf16 operands, fp32 accumulation, against the conv of the bf16-rounded operands (the bias stays fp32)."""
    _check(cuda, "bf16", case, "bf16_3" if case[4] == 3 else "bf16_5", True, bf16_ref=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.BF16_3X3_DECLINE + [cc.BF16_5X5_OVER_LDS], ids=cc.case_id)
def test_bf16_declines_to_the_fp32_kernels(cuda, case):
    """3x3: pack_conv_weight_bf16 packs any cin % 16 == 0, launch_bf16 declines 3 and 6 blocks and two sources.  5x5: cin 176 packs, its
    tile is the first past the 160 KiB of LDS and launch_bf16_5x5 declines.  Each gives the bits of the fp32 call."""
    _check(cuda, "direct", case, "bf16_3" if case[4] == 3 else "bf16_5", False, label="bf16_declined")


@pytest.mark.gpu
def test_bf16_5x5_pack_refuses_cin_24(cuda):
    """cin % 16 != 0 never reaches launch_bf16_5x5's own `qin % 4` decline through the library: pack_conv_weight_bf16_ks refuses the
    weight (ValueError), and the layer runs fp32."""
    case = cc.BF16_5X5_PACK_REFUSES
    with pytest.raises(ValueError, match="cin % 16"):
        _run(cuda, case, "bf16_5")
    _check(cuda, "direct", case, None, True)


def _cell(dev, i, h, ks):
    import ode_rl_amd
    sd, x, h0 = cc.cell_values(i, h, ks)
    cell = ode_rl_amd.ConvGRUCell((16, 16), i, h, ks)
    cell.load_state_dict(sd)
    return cell.to(dev), x.to(dev), h0.to(dev)


def _check_cell_blocks(name, out, ref32, ref64, floor):
    """Whole state and every GroupNorm group of 32 channels on its own, each under _convgru_ref.bound of its own slice."""
    hid = ref64.shape[1]
    for lo, hi in [(0, hid)] + [(g, g + 32) for g in range(0, hid, 32)]:
        bound, d32 = _convgru_ref.bound(ref32[:, lo:hi], ref64[:, lo:hi], floor)
        err = rel_l2(out[:, lo:hi], ref64[:, lo:hi])
        if (lo, hi) == (0, hid):
            record(name, err)
            print(f"{name}: rel-L2 {err:.3e}, d32 {d32:.3e}, bound {bound:.3e}")
        assert err <= bound, (lo, hi, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("i,h,ks", cc.CELLS)
def test_convgru_cell_forward_values(cuda, i, h, ks):
    """One ConvGRU step at input != hidden, hidden = 96 (3 and 6 GroupNorm groups) and kernel sizes 5 / 3 / 1 against the float64 cell."""
    cell, x, h0 = _cell(cuda, i, h, ks)
    ref32, ref64 = cc.cell_reference(i, h, ks)
    with torch.no_grad():
        seq, out = cell(input_tensor=x[None], h_cur=h0, seq_len=1)
        _, again = cell(input_tensor=x[None], h_cur=h0, seq_len=1)
    assert seq.shape == (1, 2, h, 16, 16) and torch.equal(seq[0], out) and torch.equal(again, out)
    _check_cell_blocks(f"conv_shapes.cell.I{i}.H{h}.k{ks}", out.cpu(), ref32, ref64, 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("i,h,ks", cc.CELLS_BF16)
def test_convgru_cell_forward_values_bf16(cuda, i, h, ks):
    """bf16 compute mode against the cell emulated on bf16-rounded conv operands, under test_convgru_cell_and_encoder_bf16's bound for
    one step (1e-3: two chained bf16 convs + GroupNorm), whole and per GroupNorm group; and really bf16 (>= 1e-4 from the exact cell)."""
    import ode_rl_amd
    from oracle import reference_modules as rm
    cell, x, h0 = _cell(cuda, i, h, ks)
    sd, xc, hc = cc.cell_values(i, h, ks)
    with torch.no_grad():
        emu = rm.convgru_cell(xc, hc, sd, compute_dtype="bf16")
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        with torch.no_grad():
            _, out = cell(input_tensor=x[None], h_cur=h0, seq_len=1)
            _, again = cell(input_tensor=x[None], h_cur=h0, seq_len=1)
    finally:
        ode_rl_amd.set_compute_dtype(None)
    assert torch.equal(again, out)
    out = out.cpu()
    for lo, hi in [(0, h)] + [(g, g + 32) for g in range(0, h, 32)]:
        assert rel_l2(out[:, lo:hi], emu[:, lo:hi]) <= 1e-3, (lo, hi)
    record(f"conv_shapes.cell_bf16.I{i}.H{h}.k{ks}", rel_l2(out, emu))
    e = rel_l2(out, cc.cell_reference(i, h, ks)[1])
    assert 1e-4 <= e <= 3e-2, e


@pytest.mark.gpu
@pytest.mark.parametrize("i,h,ks", cc.CELLS_REFUSED)
def test_convgru_cell_refuses_cin_40_for_3x3_and_1x1(cuda, i, h, ks):
    """input 8 + hidden 32 = 40 channels: fine for 5x5 (cin % 8), not for 3x3 / 1x1 (cin % 16).  The library's own check raises before
    any kernel writes: the output buffer keeps its bytes and no workspace guard is touched."""
    from ode_rl_amd import _lib, hip_ops
    cell, x, h0 = _cell(cuda, i, h, ks)
    with torch.no_grad(), pytest.raises(ValueError, match=r"needs cin % 16 == 0 \(got 40\)"):
        cell(input_tensor=x[None], h_cur=h0, seq_len=1)
    # the call of hip_ops.convgru_cell_forward restated (same workspace key, same arguments) with an output buffer this test can see
    d = cell._packed().refresh()
    lib = _lib.load()
    nbytes = lib.odehip_convgru_cell_workspace_bytes(ctypes.byref(d), 2)
    ws = hip_ops.workspace(("cgru", 2, d.input, d.hidden), nbytes, cuda)
    out = torch.full_like(h0, -7.25)
    rc = lib.odehip_convgru_cell_forward(ctypes.byref(d), x.data_ptr(), h0.data_ptr(), out.data_ptr(), 2, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError, match=r"needs cin % 16 == 0 \(got 40\)"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    hip_ops.check_canaries()


@pytest.mark.gpu
@pytest.mark.parametrize("ch,n_layers,units", cc.STACKS)
def test_dynamics_stacks_of_other_widths(cuda, ch, n_layers, units):
    """hip_ops.convstack_forward on stacks that enqueue_f's one-launch evaluation does not take (csrc/persist.hip: a width other than
    64 / 128, or a 128 -> 128 adjacency), so every layer is its own launch_conv: the Winograd kernel where an instantiation exists
    (32, 64 and 128 -> ..), the ring kernel behind a declined Winograd image elsewhere (96 and 256 -> ..)."""
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    from ode_rl_amd.odeint import conv_stack_of
    sd, y = cc.stack_values(ch, n_layers, units)
    f = ode_rl_amd.ODEFunc(ch, ch, n_layers, units, False, "relu", final_act=False)
    f.load_state_dict(sd)
    f = f.to(cuda)
    ref32, ref64 = cc.stack_reference(ch, n_layers, units)
    bound, d32 = _convgru_ref.bound(ref32, ref64, 1e-5)
    out = hip_ops.convstack_forward(conv_stack_of(f), y.to(cuda))
    assert torch.equal(hip_ops.convstack_forward(conv_stack_of(f), y.to(cuda)), out)
    err = record(f"conv_shapes.stack.{ch}.{n_layers}.{units}", rel_l2(out, ref64))
    print(f"stack {ch}/{n_layers}/{units}: rel-L2 {err:.3e}, d32 {d32:.3e}, bound {bound:.3e}")
    assert out.shape == ref64.shape and err <= bound, (err, bound)
