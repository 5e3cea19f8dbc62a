"""Tableau-generic CPU restatement of torchdiffeq 0.2.1's adaptive Runge-Kutta solver (`_impl/rk_common.py`: _adaptive_step,
_runge_kutta_step, _interp_fit; `_impl/misc.py`: _optimal_step_size) -- test infrastructure, written against the conventions of
oracle/torchdiffeq_ref.py (float64 time, state arithmetic in y0.dtype, one RMS norm over the whole tensor, FSAL, per-output
max_num_steps, stats dict) and reusing what is already tableau-free there (_select_initial_step, _error_ratio, _interp_evaluate).

With DOPRI5 it is the oracle's own arithmetic, operation for operation (tests/test_adaptive_ref_cpu.py pins that bit for bit); BOSH3 is
`_impl/bosh3.py` (Bogacki-Shampine 3(2), order 3), pinned there by scipy's RK23 and by the order conditions.  PARITY UNPINNED like the
oracle's: torchdiffeq itself cannot be run here.

odeint_adjoint restates `_impl/adjoint.py` as the oracle does (interval by interval, the flat augmented state, the mixed norm or the
seminorm) on top of the generic odeint above."""
import collections

import torch

from oracle import torchdiffeq_ref as ref

Tableau = collections.namedtuple("Tableau", "name alpha beta c_sol c_error c_mid order")

DOPRI5 = Tableau("dopri5", ref.DP_ALPHA, ref.DP_BETA, ref.DP_C_SOL, ref.DP_C_ERROR, ref.DP_C_MID, 5)
BOSH3 = Tableau(
    "bosh3",
    [1 / 2, 3 / 4, 1.0],
    [[1 / 2], [0.0, 3 / 4], [2 / 9, 1 / 3, 4 / 9]],
    [2 / 9, 1 / 3, 4 / 9, 0.0],
    [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8],
    [0.0, 1 / 2, 0.0, 0.0],
    3)
TABLEAUS = {"dopri5": DOPRI5, "bosh3": BOSH3}


def rk_step(tb, func, y0, f0, t0, dt, t1):
    """_runge_kutta_step: y1, f1 (= the last stage: FSAL), y1_error and the stage derivatives as a list."""
    dtype = y0.dtype
    t0s, dts, t1s = t0.to(dtype), dt.to(dtype), t1.to(dtype)
    k = [f0]
    yi = y0
    for alpha_i, beta_i in zip(tb.alpha, tb.beta):
        ti = t1s if alpha_i == 1.0 else t0s + alpha_i * dts
        acc = torch.zeros_like(y0)
        for kj, bij in zip(k, beta_i):
            acc = acc + kj * (torch.tensor(bij, dtype=dtype) * dts)
        yi = y0 + acc
        k.append(func(ti, yi))
    y1 = yi  # c_sol == last beta row
    f1 = k[-1]
    err = torch.zeros_like(y0)
    for kj, cj in zip(k, tb.c_error):
        err = err + kj * (dts * torch.tensor(cj, dtype=dtype))
    return y1, f1, err, k


def optimal_step_size(last_step, error_ratio, order):
    """_optimal_step_size with the method's order (safety 0.9, ifactor 10, dfactor 0.2; under no_grad in torchdiffeq)."""
    last_step = last_step.detach()
    if error_ratio == 0:
        return last_step * ref.IFACTOR
    dfactor = 1.0 if error_ratio < 1 else ref.DFACTOR
    er = error_ratio.to(last_step.dtype)
    exponent = 1.0 / order
    factor = min(ref.IFACTOR, max(ref.SAFETY / float(er ** exponent), dfactor))
    return last_step * factor


def interp_fit(tb, y0, y1, k, dt):
    """_interp_fit through y0, y1, y_mid = y0 + dt sum c_mid[s] k_s, f0 = k[0], f1 = k[-1]."""
    dts = dt.to(y0.dtype)
    y_mid = y0.clone()
    for kj, cj in zip(k, tb.c_mid):
        y_mid = y_mid + kj * (dts * torch.tensor(cj, dtype=y0.dtype))
    f0, f1 = k[0], k[-1]
    a = 2 * dts * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dts * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dts * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    d = dts * f0
    e = y0
    return [e, d, c, b, a]


def dense_weight(tb, s, x):
    """Weight of stage s in value(x) = y0 + h sum_s W_s(x) k_s, the quartic above as a linear form in the stages (float64 Python
    arithmetic): what csrc/dopri5_control.h's dense_weight computes."""
    last = len(tb.c_sol) - 1
    d1, d7 = (1.0 if s == 0 else 0.0), (1.0 if s == last else 0.0)
    b, m = tb.c_sol[s], tb.c_mid[s]
    a4 = 2.0 * (d7 - d1) - 8.0 * b + 16.0 * m
    b3 = 5.0 * d1 - 3.0 * d7 + 14.0 * b - 32.0 * m
    c2 = d7 - 4.0 * d1 - 5.0 * b + 16.0 * m
    return x * d1 + x * x * c2 + x * x * x * b3 + x * x * x * x * a4


def _integrate(tb, func, y0, t, rtol, atol, stats, norm, options=None):
    solution = torch.empty(len(t), *y0.shape, dtype=y0.dtype)
    solution[0] = y0
    t = t.to(torch.float64)
    f0 = func(t[0].to(y0.dtype), y0)
    options = options or {}
    max_num_steps = options.get("max_num_steps", ref.MAX_NUM_STEPS)
    if options.get("first_step") is None:
        dt = ref._select_initial_step(func, t[0], y0, tb.order - 1, rtol, atol, f0, norm)
        stats["nfe"] = stats.get("nfe", 0) + 2
    else:
        dt = torch.as_tensor(options["first_step"], dtype=torch.float64)
        stats["nfe"] = stats.get("nfe", 0) + 1
    y, f, t0, t1 = y0, f0, t[0], t[0]
    interp = [y0] * 5
    for i in range(1, len(t)):
        next_t = t[i]
        n_steps = 0
        while next_t > t1:
            assert n_steps < max_num_steps, "max_num_steps exceeded ({}>={})".format(n_steps, max_num_steps)
            ta = t1
            tb_ = ta + dt
            assert tb_ > ta, "underflow in dt {}".format(dt.item())
            assert torch.isfinite(y).all(), "non-finite values in state `y`"
            y1, f1, err, k = rk_step(tb, func, y, f, ta, dt, tb_)
            ratio = ref._error_ratio(err, rtol, atol, y, y1, norm)
            accept = bool(ratio <= 1)
            stats["nfe"] += len(tb.beta)
            stats.setdefault("dts", []).append(float(dt))
            stats.setdefault("ratios", []).append(float(ratio))
            if accept:
                interp = interp_fit(tb, y, y1, k, dt)
                t0, t1 = ta, tb_
                y, f = y1, f1
                stats["n_accept"] = stats.get("n_accept", 0) + 1
                stats.setdefault("accepted", []).append((float(ta), float(dt)))
            else:
                stats["n_reject"] = stats.get("n_reject", 0) + 1
            dt = optimal_step_size(dt, ratio, tb.order)
            n_steps += 1
        stats.setdefault("steps_per_output", []).append(n_steps)
        solution[i] = ref._interp_evaluate(interp, t0, t1, next_t)
    return solution


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method="dopri5", options=None, stats=None, norm=None):
    """oracle.torchdiffeq_ref.odeint for the adaptive methods of TABLEAUS (a decreasing t integrates -f on -t)."""
    tb = TABLEAUS[method]
    if stats is None:
        stats = {}
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    ref._check_t(t)
    if len(t) > 1 and bool(t[0] > t[1]):
        t = -t
        fwd = func
        func = lambda tt, yy: -fwd(-tt, yy)  # noqa: E731
    stats.setdefault("n_accept", 0)
    stats.setdefault("n_reject", 0)
    return _integrate(tb, func, y0, t, rtol, atol, stats, norm or ref.rms_norm, options)


def odeint_adjoint(func, y0, t, params, grad_out, rtol=1e-7, atol=1e-9, method="dopri5", stats=None, adjoint_norm="mixed"):
    """oracle.torchdiffeq_ref.odeint_adjoint for the adaptive methods of TABLEAUS: (ys, grad_y0, [grad_theta...]); `stats` receives the
    counts of the BACKWARD solves."""
    params = list(params)
    with torch.no_grad():
        ys = odeint(func, y0, t, rtol=rtol, atol=atol, method=method)
    n_y = y0.numel()
    shapes = [p.shape for p in params]
    sizes = [p.numel() for p in params]

    def aug_dynamics(tt, state):
        y = state[:n_y].view_as(y0)
        a_y = state[n_y:2 * n_y].view_as(y0)
        with torch.enable_grad():
            yr = y.detach().requires_grad_(True)
            fy = func(tt, yr)
            grads = torch.autograd.grad(fy, [yr] + params, -a_y, allow_unused=True)
        vjp_y = grads[0] if grads[0] is not None else torch.zeros_like(y)
        vjp_p = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads[1:], params)]
        return torch.cat([fy.detach().reshape(-1), vjp_y.reshape(-1)] + [g.reshape(-1) for g in vjp_p])

    a_y = grad_out[-1].clone()
    a_p = torch.zeros(sum(sizes), dtype=y0.dtype)
    if adjoint_norm not in ("mixed", "seminorm"):
        raise ValueError("adjoint_norm must be 'mixed' or 'seminorm'")
    norm_chunks = [n_y, n_y] + (sizes if adjoint_norm == "mixed" else [])

    def mixed_norm(x):
        out, off = None, 0
        for n in norm_chunks:
            v = ref.rms_norm(x[off:off + n])
            out = v if out is None else torch.max(out, v)
            off += n
        return out

    with torch.no_grad():
        for i in range(len(t) - 1, 0, -1):
            state = torch.cat([ys[i].reshape(-1), a_y.reshape(-1), a_p])
            tt = torch.stack([t[i], t[i - 1]])
            sol = odeint(aug_dynamics, state, tt, rtol=rtol, atol=atol, method=method, stats=stats, norm=mixed_norm)
            end = sol[1]
            a_y = end[n_y:2 * n_y].view_as(y0) + grad_out[i - 1]
            a_p = end[2 * n_y:]
    grads_p, off = [], 0
    for s, n in zip(shapes, sizes):
        grads_p.append(a_p[off:off + n].view(s).clone())
        off += n
    return ys, a_y, grads_p
