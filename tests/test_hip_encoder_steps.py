"""Encoder steps that NO sample observed launch nothing of the ConvGRU cell, in either pass (odehip_odeconvgru_encode*_steps, the host
step hint; csrc/convgru.hip, csrc/convgru_backward.hip).  The oracle is the code without the hint: the SAME call with the SAME mask
on the device cannot skip (a device mask is never read back), and everything the two runs produce must be the same bits -- except
the cell's own parameter gradients, whose weight-gradient tables list fewer steps and are therefore summed in another order; those
are held to the bounds of tests/test_hip_encoder_mask.py against the CPU restatement (tests/_mask_ref.py; the norm-free cell against
tests/_vidode_upstream_ref.py in float64): rel-L2 <= 5e-5 forward, <= 2e-4 per gradient tensor.  Inputs: the recipe of
tests/test_hip_encoder_mask.py.  Shapes: 64 channels, the smallest the training path takes; one forward-only case at 32."""
import copy
import functools

import pytest
import torch

import _mask_ref
import _vidode_upstream_ref as up
from conftest import procedural_tensor, rel_l2

pytestmark = pytest.mark.gpu

MASKS = {"alt": [[1, 0, 1, 0]] * 2,            # the last-visited frame is skipped under one order, the first-visited under the other
         "runs": [[1, 0, 0, 1, 0]] * 3,        # a run of two skipped steps
         "none": [[0, 0, 0]] * 2,              # no step runs the cell
         "partial": [[1, 0, 1], [1, 1, 1]],    # nothing may be skipped
         "frac": [[1, 0.25, 0], [0.5, 0, 0]]}  # one column all zero beside fractional ones
OBSERVED = {"alt": 2, "runs": 2, "none": 0, "partial": 3, "frac": 2}
ORDERS_AND_PATHS = [(rb, through) for rb in (True, False) for through in ("head", "latent")]


@functools.lru_cache(maxsize=None)
def _inputs(name, ch=64):
    mask = torch.tensor(MASKS[name], dtype=torch.float32)
    B, T = mask.shape
    g = torch.Generator().manual_seed(11 + T * 10 + B)
    return {"enc": _mask_ref.build(ch), "x": torch.randn(T, B, ch, 16, 16, generator=g) * 0.5, "t": torch.arange(T, dtype=torch.float64) / 8,
            "mask": mask, "gmean": torch.randn(B, ch, 16, 16, generator=g), "gstd": torch.randn(B, ch, 16, 16, generator=g),
            "glat": torch.randn(B, T, ch, 16, 16, generator=g), "glast": torch.randn(B, ch, 16, 16, generator=g), "T": T, "B": B}


@functools.lru_cache(maxsize=None)
def _reference(name, run_backwards, through):
    """The restatement's values and autograd gradients, computed once per (mask, order, path) and shared (never modified)."""
    c = _inputs(name)
    outs, gouts = (("mean", "std"), [c["gmean"], c["gstd"]]) if through == "head" else (("latent", "last"), [c["glat"], c["glast"]])
    return _mask_ref.oracle(c["enc"], c["x"], c["t"], c["mask"], outs, gouts, run_backwards)


def _device_encoder(name, cuda, ch=64):
    return copy.deepcopy(_inputs(name, ch)["enc"]).to(cuda)


def _run(enc, c, cuda, through, run_backwards, mask, steps=None, x=None):
    """One forward + backward of the module's packed encoder: ({output: value}, grad_inputs, {parameter: gradient}, (steps for which
    the forward launched the cell, the same of the backward))."""
    from ode_rl_amd.autograd import encode_with_grad
    enc.zero_grad(set_to_none=True)
    packed = enc._packed()
    packed.last_cell_steps = packed.last_cell_steps_backward = None
    x = (c["x"] if x is None else x).to(cuda).requires_grad_(True)
    out = encode_with_grad(packed, x, c["t"].to(cuda), want_latent=through == "latent", run_backwards=run_backwards, mask=mask, steps=steps)
    if through == "head":
        vals = {"mean": out[0], "std": out[1]}
        torch.autograd.backward([out[0], out[1]], [c["gmean"].to(cuda), c["gstd"].to(cuda)])
    else:
        vals = {"latent": out[2], "last": out[2][:, -1]}
        torch.autograd.backward([vals["latent"], vals["last"]], [c["glat"].to(cuda), c["glast"].to(cuda)])
    return ({k: v.detach() for k, v in vals.items()}, x.grad, {n: p.grad for n, p in enc.named_parameters()},
            (packed.last_cell_steps, packed.last_cell_steps_backward))


def _is_cell(name):
    return name.startswith(("cgru_cell.", "cell_list."))


def _differences(a, b, cell=True):
    """Names of everything that is not the same bits in two runs; cell=False leaves the cell's own parameter gradients out."""
    (va, gxa, gpa, _), (vb, gxb, gpb, _) = a, b
    diff = [k for k in va if not torch.equal(va[k], vb[k])]
    diff += ["grad_inputs"] if not torch.equal(gxa, gxb) else []
    for k in gpa:
        if not cell and _is_cell(k):
            continue
        if (gpa[k] is None) != (gpb[k] is None) or (gpa[k] is not None and not torch.equal(gpa[k], gpb[k])):
            diff.append(k)
    return diff


def _cell_gradient_errors(run, ref_gp):
    errs = {}
    for name, r in ref_gp.items():
        if _is_cell(name):
            assert r is not None and bool(r.any()), f"the reference gradient of {name} is zero: the ratio is not defined"
            assert run[2][name] is not None, name
            errs[name] = rel_l2(run[2][name], r)
    return errs


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
@pytest.mark.parametrize("name", ["alt", "runs", "partial", "frac"])
def test_host_mask_run_against_device_mask_run(cuda, name, run_backwards, through):
    c = _inputs(name)
    ref, ref_gx, ref_gp = _reference(name, run_backwards, through)
    enc = _device_encoder(name, cuda)
    host = _run(enc, c, cuda, through, run_backwards, c["mask"])
    dev = _run(enc, c, cuda, through, run_backwards, c["mask"].to(cuda))
    off = _run(enc, c, cuda, through, run_backwards, c["mask"], steps=False)
    # against the reference first: forward, then the cell's gradients of BOTH runs
    fwd = {k: rel_l2(v, ref[k]) for k, v in host[0].items()}
    errs_host, errs_dev = _cell_gradient_errors(host, ref_gp), _cell_gradient_errors(dev, ref_gp)
    same_cell = _differences(host, dev) == []
    print(name, run_backwards, through, "steps", host[3], dev[3], fwd, "cell gradients: host", errs_host, "device", errs_dev,
          "host == device bit for bit:", same_cell)
    assert all(e <= 5e-5 for e in fwd.values()), fwd
    assert rel_l2(host[1], ref_gx) <= 2e-4
    assert not {k: v for k, v in errs_host.items() if v > 2e-4}, errs_host
    assert not {k: v for k, v in errs_dev.items() if v > 2e-4}, errs_dev
    # the oracle: the code that cannot skip.  Everything but the cell's own gradients is the same bits
    assert _differences(host, dev, cell=False) == []
    assert _differences(off, dev) == []          # steps=False: today's launches, the cell's gradients included
    if OBSERVED[name] == c["T"]:                 # nothing skipped: the same launches, so the cell's gradients are the same bits too
        assert same_cell
    # step counts: the assertions that fail without the feature
    assert host[3] == (OBSERVED[name], OBSERVED[name])
    assert dev[3] == (c["T"], c["T"]) and off[3] == (c["T"], c["T"])


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
def test_no_frame_observed(cuda, run_backwards, through):
    c = _inputs("none")
    ref, ref_gx, ref_gp = _reference("none", run_backwards, through)
    enc = _device_encoder("none", cuda)
    host = _run(enc, c, cuda, through, run_backwards, c["mask"])
    dev = _run(enc, c, cuda, through, run_backwards, c["mask"].to(cuda))
    assert host[3] == (0, 0) and dev[3] == (c["T"], c["T"])
    assert all(rel_l2(v, ref[k]) <= 5e-5 for k, v in host[0].items())
    assert all(torch.equal(host[0][k], dev[0][k]) for k in host[0])
    cell = [k for k in host[2] if _is_cell(k)]
    assert len(cell) == 8
    for k in cell:      # present and exactly zero: not uninitialised memory
        assert host[2][k] is not None and not bool(host[2][k].any()), k
        assert not bool(ref_gp[k].any())
    assert not bool(host[1].any()) and not bool(ref_gx.any())
    assert _differences(host, dev, cell=False) == []
    assert any(bool(host[2][k].any()) for k in host[2] if k.startswith("ode_func."))     # (the dynamics do get a gradient)


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
def test_unobserved_content_cannot_matter(cuda, run_backwards, through):
    """NaN in the frames nobody observed: forward outputs AND every gradient finite and the same bits as the clean run.  Stronger than
    what the unskipped path promises (forward only): nothing multiplies those frames any more."""
    c = _inputs("alt")
    enc = _device_encoder("alt", cuda)
    poisoned = c["x"].clone()
    poisoned[1], poisoned[3] = float("nan"), float("nan")
    clean = _run(enc, c, cuda, through, run_backwards, c["mask"])
    got = _run(enc, c, cuda, through, run_backwards, c["mask"], x=poisoned)
    assert _differences(got, clean) == []
    assert all(bool(torch.isfinite(v).all()) for v in got[0].values()) and bool(torch.isfinite(got[1]).all())
    assert all(bool(torch.isfinite(g).all()) for g in got[2].values() if g is not None)
    assert got[3] == (2, 2)


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
def test_an_explicit_hint_overrides_the_rows_of_a_device_mask(cuda, run_backwards, through):
    """steps= with a device mask whose hinted-off row is NOT zero equals, bit for bit, the run with that row zeroed and no hint."""
    c = _inputs("alt")
    enc = _device_encoder("alt", cuda)
    full = torch.tensor([[1.0, 0.5, 1.0, 1.0], [1.0, 1.0, 0.25, 1.0]])
    zeroed = full.clone()
    zeroed[:, 1] = 0.0
    zeroed[:, 3] = 0.0
    hinted = _run(enc, c, cuda, through, run_backwards, full.to(cuda), steps=[True, False, True, False])
    plain = _run(enc, c, cuda, through, run_backwards, zeroed)          # on the host: derives the same hint
    unskipped = _run(enc, c, cuda, through, run_backwards, zeroed.to(cuda))
    assert _differences(hinted, plain) == []
    assert _differences(hinted, unskipped, cell=False) == []
    assert hinted[3] == (2, 2) and plain[3] == (2, 2) and unskipped[3] == (4, 4)


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
def test_a_hint_without_a_mask(cuda, run_backwards, through):
    c = _inputs("runs")
    enc = _device_encoder("runs", cuda)
    keep = [1, 0, 0, 1, 0]
    hinted = _run(enc, c, cuda, through, run_backwards, None, steps=keep)
    masked = _run(enc, c, cuda, through, run_backwards, torch.tensor([keep] * c["B"], dtype=torch.float32, device=cuda))
    assert _differences(hinted, masked, cell=False) == []
    assert hinted[3] == (2, 2) and masked[3] == (5, 5)
    same = _run(enc, c, cuda, through, run_backwards, torch.tensor([keep] * c["B"], dtype=torch.float32))
    assert _differences(hinted, same) == []
    assert _run(enc, c, cuda, through, run_backwards, None)[3] == (5, 5)      # no mask, no hint: every step, as before


def test_forward_only_at_32_channels(cuda):
    """The inference entry point (no training path at 32 channels): outputs and latent states, both orders, both module calls."""
    from ode_rl_amd import hip_ops
    c = _inputs("runs", 32)
    enc = _device_encoder("runs", cuda, 32)
    x, t = c["x"].to(cuda), c["t"].to(cuda)
    with torch.no_grad():
        for rb in (True, False):
            host = hip_ops.odeconvgru_encode(enc._packed(), x, t, want_latent=True, run_backwards=rb, mask=c["mask"])
            assert enc._packed().last_cell_steps == 2
            dev = hip_ops.odeconvgru_encode(enc._packed(), x, t, want_latent=True, run_backwards=rb, mask=c["mask"].to(cuda))
            assert enc._packed().last_cell_steps == 5
            assert all(torch.equal(a, b) for a, b in zip(host, dev))
            nolat = hip_ops.odeconvgru_encode(enc._packed(), x, t, run_backwards=rb, mask=c["mask"])
            assert torch.equal(nolat[0], dev[0]) and torch.equal(nolat[1], dev[1]) and nolat[2] is None
            last, lat = enc.run_ode_conv_gru(x, t, run_backwards=rb, mask=c["mask"])
            assert torch.equal(lat, dev[2]) and torch.equal(last, dev[2][:, -1])
        m, s = enc(x, t, c["mask"])
        assert enc._packed().last_cell_steps == 2
        m2, s2 = enc(x, t, c["mask"], steps=False)
        assert enc._packed().last_cell_steps == 5 and torch.equal(m, m2) and torch.equal(s, s2)


@pytest.fixture
def bf16_mode():
    import ode_rl_amd
    ode_rl_amd.set_compute_dtype("bf16")
    yield
    ode_rl_amd.set_compute_dtype(None)


@pytest.mark.parametrize("run_backwards,through", ORDERS_AND_PATHS)
def test_bf16_compute_mode(cuda, bf16_mode, run_backwards, through):
    """Host against device mask, both in bf16 compute mode: the equalities of the fp32 comparison."""
    c = _inputs("alt")
    enc = _device_encoder("alt", cuda)
    host = _run(enc, c, cuda, through, run_backwards, c["mask"])
    dev = _run(enc, c, cuda, through, run_backwards, c["mask"].to(cuda))
    assert _differences(host, dev, cell=False) == []
    assert host[3] == (2, 2) and dev[3] == (4, 4)
    for k in host[2]:
        if _is_cell(k):     # the same sums in another order: bf16 operands, fp32 accumulation
            assert rel_l2(host[2][k], dev[2][k]) <= 2e-4, k


# ---- the norm-free 3x3 cell of upstream Vid-ODE (csrc/convgru_plain.hip) ----------------------------------------------------------------

PLAIN_MASKS = {"alt": MASKS["alt"], "none": MASKS["none"]}


@functools.lru_cache(maxsize=None)
def _plain_inputs(name):
    mask = torch.tensor(PLAIN_MASKS[name], dtype=torch.float32)
    B, T = mask.shape
    sd, _ = up.encoder_case(64, B)
    return {"sd": sd, "frames": procedural_tensor((B, T, 64, 16, 16), 4490 + T, -1.0, 1.0), "mask": mask, "T": T, "B": B,
            "t": torch.arange(T, dtype=torch.float64) / 8, "gm": procedural_tensor((B, 64, 16, 16), 4481, -1.0, 1.0),
            "gs": procedural_tensor((B, 64, 16, 16), 4482, -1.0, 1.0), "gl": procedural_tensor((B, T, 64, 16, 16), 4483, -0.5, 0.5)}


@functools.lru_cache(maxsize=None)
def _plain_reference(name, rb):
    """float64 restatement with autograd, the gradient arriving through all three outputs; computed once and shared."""
    c = _plain_inputs(name)
    sd64 = {k: v.double().requires_grad_(True) for k, v in c["sd"].items()}
    x64 = c["frames"].double().requires_grad_(True)
    m, s, l = up.encoder(sd64, x64, c["t"], c["mask"].double(), rb)
    ((m * c["gm"]).sum() + (s * c["gs"]).sum() + (l * c["gl"]).sum()).backward()
    return {"mean": m.detach(), "std": s.detach(), "latent": l.detach()}, x64.grad, {k: v.grad for k, v in sd64.items()}


def _plain_encoder(c, rb, cuda):
    from ode_rl_amd.models import conv_odegru
    func = conv_odegru.ODEFunc(None, 64, 64, conv_odegru.create_convnet(64, 64, n_layers=1, n_units=64))
    solver = conv_odegru.DiffeqSolver(64, func, "euler", 64, odeint_rtol=1e-3, odeint_atol=1e-4)
    enc = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), 64, 64, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                             return_all_layers=True, z0_diffeq_solver=solver, run_backwards=rb, fused=True)
    enc.load_state_dict(c["sd"])
    return enc.to(cuda)


def _plain_run(enc, c, rb, mask, cuda, steps=None):
    enc.zero_grad(set_to_none=True)
    packed = enc._packed()
    packed.last_cell_steps = packed.last_cell_steps_backward = None
    x = c["frames"].to(cuda).requires_grad_(True)
    mean, std, latent = enc._encode(x, c["t"], mask, rb, True, steps)
    ((mean * c["gm"].to(cuda)).sum() + (std * c["gs"].to(cuda)).sum() + (latent * c["gl"].to(cuda)).sum()).backward()
    return ({"mean": mean.detach(), "std": std.detach(), "latent": latent.detach()}, x.grad, {k: p.grad for k, p in enc.named_parameters()},
            (packed.last_cell_steps, packed.last_cell_steps_backward))


@pytest.mark.parametrize("rb", [True, False])
@pytest.mark.parametrize("name", ["alt", "none"])
def test_the_norm_free_cell(cuda, name, rb):
    c = _plain_inputs(name)
    ref, ref_gx, ref_gp = _plain_reference(name, rb)
    enc = _plain_encoder(c, rb, cuda)
    host = _plain_run(enc, c, rb, c["mask"], cuda)
    dev = _plain_run(enc, c, rb, c["mask"].to(cuda), cuda)
    off = _plain_run(enc, c, rb, c["mask"], cuda, steps=False)
    n = int(c["mask"].any(dim=0).sum())
    assert host[3] == (n, n) and dev[3] == (c["T"], c["T"]) and off[3] == (c["T"], c["T"])
    fwd = {k: rel_l2(v, ref[k]) for k, v in host[0].items()}
    assert all(e <= 5e-5 for e in fwd.values()), fwd
    assert _differences(host, dev, cell=False) == [] and _differences(off, dev) == []
    cell = [k for k in host[2] if k.startswith("cell_list.0.")]
    assert len(cell) == 4
    if name == "none":
        for k in cell:
            assert host[2][k] is not None and not bool(host[2][k].any()) and not bool(ref_gp[k].any()), k
        assert not bool(host[1].any())
    else:
        errs = {}
        for k in cell:
            assert bool(ref_gp[k].any())
            errs[k] = (rel_l2(host[2][k], ref_gp[k]), rel_l2(dev[2][k], ref_gp[k]))
        print(name, rb, fwd, errs, "host == device bit for bit:", _differences(host, dev) == [])
        assert all(max(e) <= 2e-4 for e in errs.values()), errs
        assert rel_l2(host[1], ref_gx) <= 2e-4


# ---- end to end: upstream's model on an interpolation batch whose mask the loader left on the host ------------------------------------------

@pytest.fixture
def reproducible_library_convolutions():
    """The recipe of tests/test_hip_encoder_mask.py, re-stated: the model's BatchNorm encoder and flow decoder are the library's
    convolutions, whose default algorithms are not reproducible bit for bit; the comparison below is bitwise."""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_vidode_interpolation_batch_skips_without_any_change_by_the_user(cuda, reproducible_library_convolutions):
    from ode_rl_amd.models import conv_odegru
    model = conv_odegru.VidODE(up.model_opt(False), cuda, fused=True)      # resolution 64, n_downs 2, interpolation
    model.load_state_dict(up.model_state_dict(model.state_dict()))
    model.train()
    batch = up.model_batch(2)
    batch["observed_mask"] = torch.tensor([[1.0, 0.0, 1.0]] * 2).unsqueeze(-1)     # on the host, as VidODEBatches leaves it
    packed = model.encoder_z0._packed()
    results = []
    for where in ("host", "device"):
        model.zero_grad(set_to_none=True)
        b = dict(batch)
        if where == "device":
            b["observed_mask"] = batch["observed_mask"].to(cuda)
        loss = model.compute_all_losses(b)["loss"]
        loss.backward()
        results.append((loss.detach().clone(), packed.last_cell_steps, packed.last_cell_steps_backward,
                        {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (lh, fh, bh, gh), (ld, fd, bd, gd) = results
    assert bool(torch.isfinite(lh)) and torch.equal(lh, ld)
    assert (fh, bh) == (2, 2) and (fd, bd) == (3, 3)
    assert set(gh) == set(gd)
    assert all(bool(torch.isfinite(g).all()) for g in gh.values()) and any(bool(g.any()) for g in gh.values())
