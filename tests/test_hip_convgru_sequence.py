"""Whole-sequence ConvGRU rollouts (csrc/convgru_sequence.hip, ConvGRUCell.rollout) on the GPU.

Yardstick: oracle.reference_modules.convgru_cell looped over the sequence on the CPU (tests/_convgru_ref.py), fed explicit zeros where
the sequence path has no operand.  A T-step rollout compounds rounding, so the bound is built from the reference's own error: the
float32 restatement's rel-L2 distance d32 from the float64 restatement on the same inputs; the HIP result must be within 4 x d32 of the
float64 result (the factor covers Winograd F(2x2,5x5) against a direct float32 convolution), never asked below the one-step bound
2e-5.  Gradients: the same construction against float64 autograd, floor 1e-4 (the project's gradient bound)."""
import pytest
import torch

import _convgru_ref as ref
from conftest import procedural_tensor, record, rel_l2

pytestmark = pytest.mark.gpu

NAMES = ["conv_gates.0.weight", "conv_gates.0.bias", "conv_gates.1.weight", "conv_gates.1.bias",
         "conv_can.0.weight", "conv_can.0.bias", "conv_can.1.weight", "conv_can.1.bias"]


def _cell(cuda, width, seed):
    import ode_rl_amd
    cell = ode_rl_amd.ConvGRUCell((16, 16), width, width, 5)
    sd = ref.cell_state_dict(width, width, seed)
    cell.load_state_dict(sd)
    return cell.to(cuda), sd


def _inputs(T, B, width, driven, state, seed):
    x = procedural_tensor((T, B, width, 16, 16), seed, -1.0, 1.0) if driven else None
    h = procedural_tensor((B, width, 16, 16), seed + 1, -0.8, 0.8) if state else None
    return x, h


def _dev(t, cuda):
    return None if t is None else t.to(cuda)


def _reference_forward(sd, x, h, T, width):
    with torch.no_grad():
        r64 = ref.rollout(ref.cast(sd, torch.float64), None if x is None else x.double(), None if h is None else h.double(), T, width)
        r32 = ref.rollout(sd, x, h, T, width)
    return r32, r64


FORWARD_CASES = [  # (driven, state, T, B, width)
    (True, False, 10, 4, 64), (True, False, 10, 64, 64),
    (False, True, 10, 4, 64), (False, True, 190, 4, 64), (False, True, 10, 64, 64),
    (True, True, 10, 4, 64),
    (False, True, 10, 4, 32), (True, False, 10, 4, 32),
]


@pytest.mark.parametrize("driven,state,T,B,width", FORWARD_CASES)
def test_rollout_forward_against_the_float64_restatement(cuda, driven, state, T, B, width):
    cell, sd = _cell(cuda, width, 31)
    x, h = _inputs(T, B, width, driven, state, 500 + T + B)
    r32, r64 = _reference_forward(sd, x, h, T, width)
    with torch.no_grad():
        hs, last = cell.rollout(_dev(x, cuda), _dev(h, cuda), T)
    assert hs.shape == (T, B, width, 16, 16) and last.data_ptr() == hs[T - 1].data_ptr()   # the last state is a view, not a copy
    tol, d32 = ref.bound(r32, r64, 2e-5)
    err = rel_l2(hs, r64)
    tag = f"{'x' if driven else '0'}{'h' if state else '0'}_T{T}_B{B}_w{width}"
    record(f"seq_fwd_d32_{tag}", d32)
    record(f"seq_fwd_hip_{tag}", err)
    print(f"forward {tag}: float32 restatement {d32:.3e}, HIP {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, d32, tol)
    first = rel_l2(hs[0], r64[0])          # one step: the project's ConvGRU bound
    record(f"seq_fwd_step0_{tag}", first)
    assert first <= 2e-5, first


def _loss_weights(T, B, width, seed):
    return procedural_tensor((T, B, width, 16, 16), seed, -1.0, 1.0), procedural_tensor((B, width, 16, 16), seed + 1, -1.0, 1.0)


def _reference_grads(sd, x, h, T, width, gw, gl, dtype):
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = None if x is None else x.detach().clone().to(dtype).requires_grad_(True)
    hr = None if h is None else h.detach().clone().to(dtype).requires_grad_(True)
    hs = ref.rollout(p, xr, hr, T, width)
    loss = (hs * gw.to(dtype)).sum() + (hs[-1] * gl.to(dtype)).sum()
    leaves = [t for t in (xr, hr) if t is not None] + [p[k] for k in NAMES]
    grads = list(torch.autograd.grad(loss, leaves))
    gx = grads.pop(0) if xr is not None else None
    gh = grads.pop(0) if hr is not None else None
    return gx, gh, grads


def _hip_grads(cell, cuda, x, h, T, gw, gl):
    cell.zero_grad()
    xd = None if x is None else x.to(cuda).requires_grad_(True)
    hd = None if h is None else h.to(cuda).requires_grad_(True)
    hs, last = cell.rollout(xd, hd, T)
    ((hs * gw.to(cuda)).sum() + (last * gl.to(cuda)).sum()).backward()
    ps = dict(cell.named_parameters())
    return hs.detach(), (None if xd is None else xd.grad), (None if hd is None else hd.grad), [ps[k].grad.clone() for k in NAMES]


BPTT_CASES = [(True, False, 10, 4), (True, False, 10, 64), (False, True, 10, 4), (False, True, 10, 64), (True, True, 10, 4)]


@pytest.mark.parametrize("driven,state,T,B", BPTT_CASES)
def test_bptt_against_float64_autograd(cuda, driven, state, T, B):
    width = 64
    cell, sd = _cell(cuda, width, 32)
    x, h = _inputs(T, B, width, driven, state, 700 + B)
    gw, gl = _loss_weights(T, B, width, 800 + B)
    gx64, gh64, gp64 = _reference_grads(sd, x, h, T, width, gw, gl, torch.float64)
    gx32, gh32, gp32 = _reference_grads(sd, x, h, T, width, gw, gl, torch.float32)
    _, gx, gh, gp = _hip_grads(cell, cuda, x, h, T, gw, gl)
    tag = f"{'x' if driven else '0'}{'h' if state else '0'}_B{B}"
    checks = [("x", gx, gx32, gx64), ("h0", gh, gh32, gh64)] + [(n, a, b, c) for n, a, b, c in zip(NAMES, gp, gp32, gp64)]
    worst = 0.0
    for name, got, r32, r64 in checks:
        if r64 is None:
            assert got is None
            continue
        tol, d32 = ref.bound(r32, r64, 1e-4)
        err = rel_l2(got, r64)
        record(f"seq_bptt_d32_{tag}_{name}", d32)
        record(f"seq_bptt_hip_{tag}_{name}", err)
        print(f"bptt {tag} {name}: float32 restatement {d32:.3e}, HIP {err:.3e}, bound {tol:.3e}")
        worst = max(worst, err / tol)
        assert err <= tol, (name, err, d32, tol)
    if not driven:   # no gradient is formed for the zero frame: the frame half is exact zeros, as autograd gives for a zero input
        assert gx is None
        for k in (0, 4):
            assert bool((gp[k][:, :width] == 0).all()) and float(gp[k][:, width:].abs().max()) > 0
            assert float(gp64[k][:, :width].abs().max()) == 0.0


@pytest.mark.parametrize("driven,state,T,B", [(False, True, 10, 4), (True, False, 10, 4), (False, True, 190, 4)])
def test_rollout_agrees_with_the_step_by_step_forward(cuda, driven, state, T, B):
    """A/B against the route that exists: ConvGRUCell.forward in its Python loop, which feeds explicit zeros."""
    cell, _ = _cell(cuda, 64, 33)
    x, h = _inputs(T, B, 64, driven, state, 900 + T)
    with torch.no_grad():
        a, a_last = cell.rollout(_dev(x, cuda), _dev(h, cuda), T)
        b, b_last = cell(_dev(x, cuda), _dev(h, cuda), T)
    worst = max(rel_l2(a[t], b[t]) for t in range(T))
    tag = f"{'x' if driven else '0'}{'h' if state else '0'}_T{T}"
    record(f"seq_ab_worst_step_{tag}", worst)
    record(f"seq_ab_bitwise_{tag}", float(torch.equal(a, b)))
    print(f"A/B {tag}: worst step {worst:.3e}, bitwise {torch.equal(a, b)}")
    assert worst <= 1e-5, worst
    assert rel_l2(a_last, b_last) <= 1e-5
    moved, _ = cell.rollout(_dev(x, cuda), _dev(h, cuda), T, dim=1)   # the stack over another dim, as forward's torch.stack(dim=)
    assert torch.equal(moved, a.movedim(0, 1))


def test_bitwise_repeatable_and_independent_of_the_batch_position(cuda):
    T, B, width = 10, 4, 64
    cell, _ = _cell(cuda, width, 34)
    gw, gl = _loss_weights(T, B, width, 1100)
    for driven, state in ((False, True), (True, False), (True, True)):
        x, h = _inputs(T, B, width, driven, state, 1000)
        one = _hip_grads(cell, cuda, x, h, T, gw, gl)
        two = _hip_grads(cell, cuda, x, h, T, gw, gl)
        for a, b in zip([one[0], one[1], one[2]] + one[3], [two[0], two[1], two[2]] + two[3]):
            assert (a is None and b is None) or torch.equal(a, b)
        perm = torch.tensor([2, 0, 3, 1])
        xp = None if x is None else x[:, perm].contiguous()
        hp = None if h is None else h[perm].contiguous()
        moved = _hip_grads(cell, cuda, xp, hp, T, gw[:, perm].contiguous(), gl[perm].contiguous())
        assert torch.equal(moved[0], one[0][:, perm.to(cuda)])
        if driven:
            assert torch.equal(moved[1], one[1][:, perm.to(cuda)])
        if state:
            assert torch.equal(moved[2], one[2][perm.to(cuda)])


def test_nan_stays_in_its_sample_and_reaches_all_of_its_steps(cuda):
    T, B = 10, 4
    cell, _ = _cell(cuda, 64, 35)
    for driven in (False, True):
        x, h = _inputs(T, B, 64, driven, True, 1200)
        with torch.no_grad():
            clean, _ = cell.rollout(_dev(x, cuda), h.to(cuda), T)
            bad = h.clone()
            bad[1, 5, 3, 7] = float("nan")
            got, _ = cell.rollout(_dev(x, cuda), bad.to(cuda), T)
        for t in range(T):
            assert bool(torch.isnan(got[t, 1]).any()), t
        keep = torch.tensor([0, 2, 3], device=cuda)
        assert bool(torch.isfinite(got[:, keep]).all()) and torch.equal(got[:, keep], clean[:, keep])


def test_a_zero_state_reads_nothing_of_the_state_buffers(cuda):
    """h_cur=None: the first step must not read h0 (there is none) nor anything uninitialised -- every cached workspace is filled with
    NaN bit patterns first, in the forward-only and in the training call."""
    from ode_rl_amd import hip_ops
    T, B = 4, 4
    cell, sd = _cell(cuda, 64, 36)
    x, _ = _inputs(T, B, 64, True, False, 1300)
    r32, r64 = _reference_forward(sd, x, None, T, 64)
    tol, _ = ref.bound(r32, r64, 2e-5)
    with torch.no_grad():
        cell.rollout(x.to(cuda), None, T)       # the workspaces exist now
        for buf in hip_ops._workspaces.values():
            buf.fill_(0xFF)
        got, _ = cell.rollout(x.to(cuda), None, T)
    assert bool(torch.isfinite(got).all()) and rel_l2(got, r64) <= tol
    xd = x.to(cuda).requires_grad_(True)
    hs, _ = cell.rollout(xd, None, T)
    hs.sum().backward()
    assert bool(torch.isfinite(xd.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in cell.parameters())


def test_bf16_mode_runs_the_ring_kernel_or_raises(cuda):
    """bf16 compute: the sequence uses the bf16 5x5 ring kernel where the cell's bf16 condition holds (64 + 64 <= 128 channels), against the
    step-by-step forward in the same mode; a cell outside that condition raises."""
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    cell, _ = _cell(cuda, 64, 37)
    _, h = _inputs(6, 4, 64, False, True, 1400)
    with torch.no_grad(), hip_ops.compute_mode("bf16"):
        a, _ = cell.rollout(None, h.to(cuda), 6)
        b, _ = cell(None, h.to(cuda), 6)
    err = max(rel_l2(a[t], b[t]) for t in range(6))
    record("seq_bf16_ab_worst_step", err)
    # both routes round the same operands to bf16 and accumulate in fp32; they differ in summation order only, which can flip the bf16
    # rounding of a state element by one ulp (2^-8 = 3.9e-3 relative) in the next step: a few ulps at the very most
    assert err <= 1e-2, err
    wide = ode_rl_amd.ConvGRUCell((16, 16), 128, 128, 5).to(cuda)
    with torch.no_grad(), hip_ops.compute_mode("bf16"), pytest.raises(ValueError, match="bf16"):
        wide.rollout(None, torch.zeros(2, 128, 16, 16, device=cuda), 2)
