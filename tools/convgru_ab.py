"""Bit identity of the ConvGRU family between two builds of the library (csrc/convgru.hip, convgru_plain.hip, convgru_backward.hip,
convgru_sequence.hip, convgru_cell.h).

  ODEHIP_LIB=<lib.so> python tools/convgru_ab.py run <out.pt>     every case from fixed seeds, in this (fresh) process
  python tools/convgru_ab.py compare <a.pt> <b.pt>                torch.equal on every tensor; exit status 1 on a difference

Cases (forward, every input gradient, every parameter gradient unless stated):
  GN cell         hidden 64 and 128 at B = 1 and 3; hidden 96 (three groups per gate: the odd boundary) forward only -- the cell's
                  backward takes multiples of 64
  norm-free cell  hidden 64, B = 3, unmasked and with the mask (1, 0, 0.5)
  encoder         64 channels at (T, B) = (1, 2) and (3, 2), 128 channels at (2, 1); both visiting orders; masks none / ones / mixed 0-1 /
                  fractional; step hints none / alternating / none observed; with and without a gradient through latent_ys
  variants        the norm-free encoder (masked, both orders); the 32-channel encoder, forward only
  sequence        width 64, B = 2, T = 1 and 3, {x + h, x only, h only}, forward-only and train + backward
  bf16 mode       one cell, one encoder, one sequence
The arithmetic is deterministic, so there is no tolerance."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _grads(module):
    return [p.grad for _, p in sorted(module.named_parameters())]


def _gn_cell(dev, hidden, B, backward, seed):
    import torch
    import ode_rl_amd
    torch.manual_seed(seed)
    cell = ode_rl_amd.ConvGRUCell((16, 16), hidden, hidden, 5).to(dev)
    with torch.no_grad():   # GroupNorm affine parameters away from (1, 0)
        for gn in (cell.conv_gates[1], cell.conv_can[1]):
            gn.weight.add_(0.3 * torch.randn_like(gn.weight))
            gn.bias.add_(0.3 * torch.randn_like(gn.bias))
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(1, B, hidden, 16, 16, generator=g) * 0.7).to(dev)
    h = (torch.randn(B, hidden, 16, 16, generator=g) * 0.7).to(dev)
    gout = torch.randn(B, hidden, 16, 16, generator=g).to(dev)
    if not backward:
        with torch.no_grad():
            return [cell(x, h, seq_len=1)[1]]
    x.requires_grad_(True)
    h.requires_grad_(True)
    out = cell(x, h, seq_len=1)[1]
    out.backward(gout)
    return [out.detach(), x.grad, h.grad] + _grads(cell)


def _plain_cell(dev, mask, seed):
    import torch
    from ode_rl_amd.models import conv_odegru
    torch.manual_seed(seed)
    cell = conv_odegru.ConvGRUCell((16, 16), 64, 64, (3, 3), True, torch.FloatTensor, fused=True).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(3, 64, 16, 16, generator=g) * 0.7).to(dev).requires_grad_(True)
    h = (torch.randn(3, 64, 16, 16, generator=g) * 0.7).to(dev).requires_grad_(True)
    gout = torch.randn(3, 64, 16, 16, generator=g).to(dev)
    out = cell(x, h, None if mask is None else torch.tensor(mask).to(dev))
    out.backward(gout)
    return [out.detach(), x.grad, h.grad] + _grads(cell)


MASKS = {"none": None, "ones": lambda B, T: [[1.0] * T] * B,
         "mixed": lambda B, T: [[float((b + i) % 2) for i in range(T)] for b in range(B)],
         "fractional": lambda B, T: [[(0.25, 1.0, 0.0, 0.6)[(2 * b + i) % 4] for i in range(T)] for b in range(B)]}
STEPS = {"none": lambda T: False, "alternating": lambda T: [i % 2 == 0 for i in range(T)], "none_observed": lambda T: [False] * T}


def _encoder(dev, ch, T, B, rb, mask, steps, through_latent, seed):
    import torch
    import ode_rl_amd
    from ode_rl_amd.autograd import encode_with_grad
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(n_inputs=ch, n_outputs=ch, n_layers=3, n_units=ch, downsize=False, nonlinear="relu", final_act=False)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), ch).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(T, B, ch, 16, 16, generator=g) * 0.5).to(dev).requires_grad_(True)
    t = (torch.arange(T, dtype=torch.float64) / 8).to(dev)
    out_ch = enc.transform_z0[-1].out_channels // 2
    gm, gs = torch.randn(B, out_ch, 16, 16, generator=g).to(dev), torch.randn(B, out_ch, 16, 16, generator=g).to(dev)
    gl = torch.randn(B, T, ch, 16, 16, generator=g).to(dev)
    m = None if MASKS[mask] is None else torch.tensor(MASKS[mask](B, T), dtype=torch.float32).to(dev)
    out = encode_with_grad(enc._packed(), x, t, want_latent=through_latent, run_backwards=rb, mask=m, steps=STEPS[steps](T))
    torch.autograd.backward(list(out), [gm, gs, gl][:len(out)])
    return [o.detach() for o in out] + [x.grad] + _grads(enc)


def _encoder_32_forward(dev, seed):
    import torch
    import ode_rl_amd
    from ode_rl_amd import hip_ops
    torch.manual_seed(seed)
    f = ode_rl_amd.ODEFunc(n_inputs=32, n_outputs=32, n_layers=3, n_units=32, downsize=False, nonlinear="relu", final_act=False)
    enc = ode_rl_amd.ODEConvGRUCell(f, None, (16, 16), 32).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(3, 2, 32, 16, 16, generator=g) * 0.5).to(dev)
    t = (torch.arange(3, dtype=torch.float64) / 8).to(dev)
    m = torch.tensor(MASKS["fractional"](2, 3), dtype=torch.float32).to(dev)
    with torch.no_grad():
        return list(hip_ops.odeconvgru_encode(enc._packed(), x, t, want_latent=True, run_backwards=True, mask=m, steps=False))


def _plain_encoder(dev, rb, seed):
    import torch
    from ode_rl_amd.models import conv_odegru
    torch.manual_seed(seed)
    func = conv_odegru.ODEFunc(None, 64, 64, conv_odegru.create_convnet(64, 64, n_layers=1, n_units=64))
    solver = conv_odegru.DiffeqSolver(64, func, "euler", 64, odeint_rtol=1e-3, odeint_atol=1e-4)
    enc = conv_odegru.Encoder_z0_ODE_ConvGRU((16, 16), 64, 64, (3, 3), 1, torch.FloatTensor, batch_first=True, bias=True,
                                             return_all_layers=True, z0_diffeq_solver=solver, run_backwards=rb, fused=True).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(3, 3, 64, 16, 16, generator=g) * 0.5).to(dev).requires_grad_(True)   # batch-first (B, T, ...)
    m = torch.tensor([[1.0, 0.0, 0.5], [0.5, 1.0, 0.0], [0.0, 0.5, 1.0]]).to(dev).unsqueeze(-1)
    mean, std, latent = enc._encode(x, torch.tensor([0.0, 0.13, 0.41], dtype=torch.float64), m, rb, True)
    w = [torch.randn(o.shape, generator=g).to(dev) for o in (mean, std, latent)]
    ((mean * w[0]).sum() + (std * w[1]).sum() + (latent * w[2]).sum()).backward()
    return [mean.detach(), std.detach(), latent.detach(), x.grad] + _grads(enc)


def _sequence(dev, T, driven, state, train, seed):
    import torch
    import ode_rl_amd
    torch.manual_seed(seed)
    cell = ode_rl_amd.ConvGRUCell((16, 16), 64, 64, 5).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(T, 2, 64, 16, 16, generator=g) * 0.7).to(dev) if driven else None
    h = (torch.randn(2, 64, 16, 16, generator=g) * 0.7).to(dev) if state else None
    gout = torch.randn(T, 2, 64, 16, 16, generator=g).to(dev)
    if not train:
        with torch.no_grad():
            return [cell.rollout(x, h, T)[0]]
    leaves = [v.requires_grad_(True) for v in (x, h) if v is not None]
    hs = cell.rollout(x, h, T)[0]
    hs.backward(gout)
    return [hs.detach()] + [v.grad for v in leaves] + _grads(cell)


def run(out_path):
    import torch
    import ode_rl_amd
    dev = torch.device("cuda:0")
    res = {}
    seed = 100

    def add(name, fn, *args):
        nonlocal seed
        seed += 2
        res[name] = fn(dev, *args, seed)

    for hidden in (64, 128):
        for B in (1, 3):
            add(f"cell.gn.h{hidden}.B{B}", _gn_cell, hidden, B, True)
    for B in (1, 3):
        add(f"cell.gn.h96.B{B}.forward", _gn_cell, 96, B, False)
    add("cell.plain.unmasked", _plain_cell, None)
    add("cell.plain.masked", _plain_cell, [1.0, 0.0, 0.5])
    for ch, T, B in ((64, 1, 2), (64, 3, 2), (128, 2, 1)):
        for rb in (True, False):
            for lat in (False, True):
                add(f"enc.c{ch}.T{T}.B{B}.rb{int(rb)}.latent{int(lat)}", _encoder, ch, T, B, rb, "none", "none", lat)
    for mask in ("ones", "mixed", "fractional"):
        for rb in (True, False):
            add(f"enc.c64.T3.B2.rb{int(rb)}.mask_{mask}", _encoder, 64, 3, 2, rb, mask, "none", True)
    for steps in ("alternating", "none_observed"):
        for mask in ("none", "mixed"):
            add(f"enc.c64.T3.B2.steps_{steps}.mask_{mask}", _encoder, 64, 3, 2, True, mask, steps, True)
    add("enc.plain.rb1", _plain_encoder, True)
    add("enc.plain.rb0", _plain_encoder, False)
    add("enc.c32.forward", _encoder_32_forward)
    for T in (1, 3):
        for driven, state in ((True, True), (True, False), (False, True)):
            for train in (False, True):
                add(f"seq.T{T}.{'x' if driven else '0'}{'h' if state else '0'}.{'train' if train else 'forward'}", _sequence, T, driven, state, train)
    ode_rl_amd.set_compute_dtype("bf16")
    try:
        add("bf16.cell.gn.h64.B3", _gn_cell, 64, 3, True)
        add("bf16.enc.c64.T3.B2", _encoder, 64, 3, 2, True, "fractional", "none", True)
        add("bf16.seq.T3.xh.train", _sequence, 3, True, True, True)
    finally:
        ode_rl_amd.set_compute_dtype(None)
    torch.cuda.synchronize()
    saved = {k: [x.detach().cpu() for x in v if x is not None] for k, v in res.items()}
    for k, v in saved.items():
        assert all(bool(torch.isfinite(x).all()) for x in v), k
    torch.save(saved, out_path)
    print(f"{ode_rl_amd._lib.LIB_PATH}: {len(saved)} cases, {sum(len(v) for v in saved.values())} tensors -> {out_path}")


def compare(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = 0
    for k in a:
        assert len(a[k]) == len(b[k]), k
        same = [torch.equal(x, y) for x, y in zip(a[k], b[k])]
        bad += same.count(False)
        print(f"{k}: {len(same)} tensors, {same.count(True)} bitwise equal" + ("" if all(same) else f"  DIFFER at {[i for i, s in enumerate(same) if not s]}"))
    print(f"{len(a)} cases, {bad} tensors differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
