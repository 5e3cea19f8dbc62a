"""Autograd glue: `odeint` participates in autograd w.r.t. y0 and every parameter of the dynamics, as the reference's
does (ownership).  Fixed-grid methods: the exact gradient of the discrete solver (what the
reference's loss.backward() computes through torchdiffeq's ops), by the explicit reverse sweep of
csrc/fixed_grid.hip + csrc/wgrad.hip."""
import torch

from . import hip_ops


def _pinned(fn):
    """backward runs with the compute dtype its forward ran with (autocast is not active on the autograd thread)."""
    def wrapper(ctx, *grads):
        with hip_ops.compute_mode(ctx.mode):
            return fn(ctx, *grads)
    return wrapper


def _stack_params(stack):
    """The parameters of the dynamics in the order the solver Functions take them and return their gradients: w0, b0, w1, b1, ..."""
    params = []
    for c in stack.convs:
        params += [c.weight, c.bias]
    return params


def _solver_backward_result(gz0, gws, gbs, n_const=3):
    """What the backward of a solver Function(y0, t_host, method or cfg, stack, *_stack_params(stack)) returns; n_const: the constants
    between y0 and the parameters (a Function that also takes `negate` or a grid has more than the three)."""
    grads = []
    for gw, gb in zip(gws, gbs):
        grads += [gw, gb]
    return (gz0,) + (None,) * n_const + tuple(grads)


def _accepted_steps(stats):
    """The accepted-step log of a finished dopri5 forward, all of it or an error: the backward pass walks these steps."""
    if stats["n_accept"] > len(stats["accepted"]):
        raise RuntimeError(f"odeint(HIP, dopri5): {stats['n_accept']} accepted steps exceed the {hip_ops.LOG_CAP} "
                           "the backward pass can re-integrate")
    return stats["accepted"]


class _FixedGridOdeint(torch.autograd.Function):
    """negate (here and in the Functions below): t was strictly decreasing, t_host is -t and the solve is that of the negated dynamics
    (set_reverse_time_grads); the backward pass is told, and carries the sign on its step sizes (csrc/fixed_grid.hip)."""

    @staticmethod
    def forward(ctx, y0, t_host, method, stack, negate, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        out, ws = hip_ops.odeint_fixed(stack, method, y0.detach(), t_host, save=True, negate=negate)
        ctx.stack, ctx.method, ctx.t_host, ctx.batch, ctx.ws, ctx.negate = stack, method, t_host, y0.shape[0], ws, negate
        hip_ops.record_versions(ctx, params)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        grads = hip_ops.odeint_fixed_backward(ctx.stack, ctx.method, ctx.t_host, ctx.batch, grad_out, ctx.ws, negate=ctx.negate)
        ctx.ws = None
        return _solver_backward_result(*grads, n_const=4)


class _GriddedOdeint(torch.autograd.Function):
    """A fixed-grid method on an internal grid (options={"grid_constructor": fn}) under autograd: the saving forward walks the grid and
    one launch interpolates the outputs; the backward turns grad_out into a gradient over the grid points with one launch
    (csrc/grid_interp.hip) and runs the reverse sweep of _FixedGridOdeint on the grid."""

    @staticmethod
    def forward(ctx, y0, t_host, method, stack, grid, negate, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        out, ws = hip_ops.odeint_fixed_on_grid(stack, method, y0.detach(), t_host, grid, save=True, negate=negate)
        ctx.stack, ctx.method, ctx.t_host, ctx.grid, ctx.batch, ctx.ws, ctx.negate = stack, method, t_host, grid, y0.shape[0], ws, negate
        hip_ops.record_versions(ctx, params)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        grads = hip_ops.odeint_fixed_on_grid_backward(ctx.stack, ctx.method, ctx.t_host, ctx.grid, ctx.batch, grad_out, ctx.ws,
                                                      negate=ctx.negate)
        ctx.ws = None
        return _solver_backward_result(*grads, n_const=5)


class _Dopri5Odeint(torch.autograd.Function):
    """odeint(method="dopri5" / "bosh3") under autograd: the gradient of the accepted steps (csrc/dopri5_backward.hip)."""

    @staticmethod
    def forward(ctx, y0, t_host, cfg, stack, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        y0d = y0.detach()
        # the forward keeps the activations of the accepted steps when it can (64-channel fp32 stacks on the adaptive walk): the
        # backward is then the reverse sweep alone; otherwise ctx.saved is None and the backward re-integrates the logged steps
        from .odeint import run_dopri5
        ctx.negate = bool(cfg.get("negate", False))   # a decreasing t: the negated dynamics on t_host = -t, solved synchronously
        out, ctx.pending, stats, ctx.saved = run_dopri5(stack, y0d, t_host, cfg, save=True, negate=ctx.negate)
        ctx.stack, ctx.t_host, ctx.method = stack, t_host, cfg.get("method", "dopri5")
        hip_ops.record_versions(ctx, params)
        # asynchronous solve (ctx.pending): nothing is known yet -- the backward pass collects it
        ctx.accepted = _accepted_steps(stats) if ctx.pending is None else None
        ctx.save_for_backward(y0d)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        (y0,) = ctx.saved_tensors
        if ctx.pending is not None:
            stats, ctx.saved = ctx.pending.collect()
            ctx.pending = None
            ctx.accepted = _accepted_steps(stats)
        if ctx.saved is not None and len(ctx.accepted) >= 1:
            grads = hip_ops.odeint_dopri5_backward_saved(ctx.stack, ctx.t_host, ctx.accepted, grad_out, ctx.saved, method=ctx.method,
                                                         negate=ctx.negate)
            ctx.saved = None
        else:
            grads = hip_ops.odeint_dopri5_backward(ctx.stack, ctx.t_host, ctx.accepted, y0, grad_out, method=ctx.method, negate=ctx.negate)
        return _solver_backward_result(*grads)


class _CellFn(torch.autograd.Function):
    """One ConvGRU step under autograd (csrc/convgru_backward.hip: odehip_convgru_cell_backward)."""

    @staticmethod
    def forward(ctx, x, h, packed, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        out = hip_ops.convgru_cell_forward(packed, x.detach(), h.detach())
        ctx.packed = packed
        hip_ops.record_versions(ctx, params)
        ctx.save_for_backward(x.detach(), h.detach())
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a ConvGRUCell parameter")
        x, h = ctx.saved_tensors
        gx, gh, grads = hip_ops.convgru_cell_backward(ctx.packed, x, h, grad_out)
        return (gx, gh, None) + tuple(grads)


def cell_with_grad(packed, x, h):
    return _CellFn.apply(x, h, packed, *packed._params())


class _SequenceFn(torch.autograd.Function):
    """A whole ConvGRU sequence under autograd (csrc/convgru_sequence.hip): the saving forward, back-propagation through time in one
    call.  x_seq / h0 may be None (zero input / zero state); the gradient of the last state arrives through the view h_seq[-1]."""

    @staticmethod
    def forward(ctx, x_seq, h0, n_steps, packed, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        h_seq, ctx.saved = hip_ops.convgru_sequence(packed, x_seq, h0, n_steps, save=True)
        ctx.packed = packed
        ctx.n_in = None if x_seq is None else x_seq.shape[0]
        hip_ops.record_versions(ctx, params)
        return h_seq

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_pinned
    def backward(ctx, grad_h_seq):
        hip_ops.check_versions(ctx, "a ConvGRUCell parameter")
        if ctx.saved is None:
            raise RuntimeError("the sequence's saved activations were already consumed (backward called twice)")
        gx, gh0, grads = hip_ops.convgru_sequence_backward(ctx.packed, ctx.saved, grad_h_seq)
        ctx.saved = None
        if gx is not None and ctx.n_in > gx.shape[0]:   # frames behind seq_len were never read
            gx = torch.cat([gx, gx.new_zeros((ctx.n_in - gx.shape[0],) + tuple(gx.shape[1:]))])
        return (gx, gh0, None, None) + tuple(grads)


def sequence_with_grad(packed, x_seq, h0, n_steps):
    return _SequenceFn.apply(x_seq, h0, n_steps, packed, *packed._params())


class _EncodeFn(torch.autograd.Function):
    """ODEConvGRUCell.forward / run_ode_conv_gru under autograd: csrc/convgru_backward.hip keeps the per-frame conv outputs and
    sweeps back; the gradient may arrive through (mean, std) and, when latent_ys was asked for, through latent_ys.  mask: the
    observation mask (hip_ops.encoder_mask), a constant; its device image lives in ctx.saved until the backward pass, and so does the
    host step hint (steps: hip_ops.encoder_steps), so the backward skips the steps the forward skipped."""

    @staticmethod
    def forward(ctx, inputs, timesteps, enc, want_latent, run_backwards, mask, steps, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        mean, std, latent, saved = hip_ops.odeconvgru_encode_train(enc, inputs.detach(), timesteps, want_latent, run_backwards, mask, steps)
        ctx.enc, ctx.saved, ctx.want_latent = enc, saved, want_latent
        hip_ops.record_versions(ctx, params)
        return (mean, std, latent) if want_latent else (mean, std)

    @staticmethod
    @_pinned
    def backward(ctx, grad_mean, grad_std, grad_latent=None):
        hip_ops.check_versions(ctx, "an encoder parameter")
        if ctx.saved is None:
            raise RuntimeError("the encoder's saved activations were already consumed (backward called twice)")
        gin, grads = hip_ops.odeconvgru_encode_backward(ctx.enc, ctx.saved, grad_mean, grad_std, grad_latent if ctx.want_latent else None)
        ctx.saved = None
        return (gin, None, None, None, None, None, None) + tuple(grads)


def encode_with_grad(enc, inputs, timesteps, want_latent=False, run_backwards=True, mask=None, steps=None):
    return _EncodeFn.apply(inputs, timesteps, enc, bool(want_latent), bool(run_backwards), mask, steps, *hip_ops.encoder_params(enc))


class _WarpCompositeFn(torch.autograd.Function):
    """VidODE's warp chain + mask compositing (csrc/warp.hip): one launch forward, one backward."""

    @staticmethod
    def forward(ctx, pred_outputs, start_image, grid_x, grid_y):
        if pred_outputs.dim() == 5:   # refuse up front what the backward does not implement, not from inside loss.backward()
            c, h, w = pred_outputs.shape[2] - 3, pred_outputs.shape[3], pred_outputs.shape[4]
            if not hip_ops.warp_composite_backward_supported(c, h, w):
                raise ValueError(f"warp_composite: the backward of a {c}x{h}x{w} image needs {hip_ops.warp_backward_lds_bytes(c, h, w) // 1024} KiB "
                                 f"of LDS ({hip_ops.WARP_LDS_BYTES // 1024} KiB available); run it under torch.no_grad() or on detached inputs")
        po, st = pred_outputs.detach().contiguous(), start_image.detach().contiguous()
        gx, gy = grid_x.detach().contiguous(), grid_y.detach().contiguous()
        pred_x, warped, masks = hip_ops.warp_composite(po, st, gx, gy)
        ctx.save_for_backward(po, st, warped, gx, gy)
        return pred_x, warped, masks

    @staticmethod
    def backward(ctx, g_pred_x, g_warped, g_masks):
        po, st, warped, gx, gy = ctx.saved_tensors
        g_po, g_start = hip_ops.warp_composite_backward(po, st, warped, gx, gy, g_pred_x, g_warped, g_masks, ctx.needs_input_grad[1])
        return g_po, g_start, None, None


def warp_composite(pred_outputs, start_image, grid_x, grid_y):
    """(pred_x, warped_pred_x, pred_masks) of models/VidODE.py:119-138 from the flow decoder's output and the last observed frame."""
    if torch.is_grad_enabled() and (pred_outputs.requires_grad or start_image.requires_grad):
        return _WarpCompositeFn.apply(pred_outputs, start_image, grid_x, grid_y)
    return hip_ops.warp_composite(pred_outputs, start_image, grid_x, grid_y)


class _Upsample2xFn(torch.autograd.Function):
    """Bilinear x2 upsampling (csrc/upsample.hip): linear, so the backward needs nothing saved."""

    @staticmethod
    def forward(ctx, x):
        return hip_ops.upsample2x(x.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return hip_ops.upsample2x_backward(g)


def upsample2x(x):
    if torch.is_grad_enabled() and x.requires_grad:
        return _Upsample2xFn.apply(x)
    return hip_ops.upsample2x(x)


class _BnReluUpFn(torch.autograd.Function):
    """BatchNorm2d -> ReLU (-> bilinear x2 upsampling) in one pass (csrc/bn_relu_up.hip): VidODE's flow decoder, models/VidODE.py:34-36."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv_bias, bn, upsample, group):
        out, saved = hip_ops.bn_relu_up_forward(x.detach(), bn, upsample, conv_bias=conv_bias, group=group)
        ctx.saved_stats, ctx.upsample, ctx.group = saved, upsample, group
        ctx.affine, ctx.has_conv_bias = weight is not None, conv_bias is not None
        ctx.save_for_backward(x.detach())
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx, gw, gb = hip_ops.bn_relu_up_backward(g, x, ctx.saved_stats, ctx.upsample, group=ctx.group)
        gcb = None
        if ctx.has_conv_bias:
            # a constant in front of batch statistics has no gradient; in eval() mode d/db = sum of dx = scale * sum g_pre = scale * d beta
            stats, training = ctx.saved_stats[:2]
            gcb = torch.zeros_like(gb) if training else stats[2] * gb
        return gx, (gw if ctx.affine else None), (gb if ctx.affine else None), gcb, None, None, None


def bn_relu_up(x, bn, upsample, conv_bias=None, group=None):
    """relu(bn(x)), upsampled x2 if `upsample`; bn: nn.BatchNorm2d (train() or eval() as the module says; running statistics and
    num_batches_tracked updated as the module itself would).  conv_bias: the bias of the convolution that produced x if the caller
    left it out of the convolution (hip_ops.bn_relu_up_forward).  group: the process group a sharded batch is spread over -- train()
    statistics are the global batch's, one all-reduce each way (hip_ops.bn_relu_up_forward; ode_rl_amd.dist.sync_batchnorm)."""
    if torch.is_grad_enabled() and (x.requires_grad or (bn.weight is not None and bn.weight.requires_grad) or
                                    (conv_bias is not None and conv_bias.requires_grad)):
        return _BnReluUpFn.apply(x, bn.weight, bn.bias, conv_bias, bn, bool(upsample), group)
    return hip_ops.bn_relu_up_forward(x, bn, upsample, conv_bias=conv_bias, group=group)[0]


class _AdjointOdeint(torch.autograd.Function):
    """torchdiffeq.odeint_adjoint: forward without a graph, backward by integrating the adjoint ODE backwards."""

    @staticmethod
    def forward(ctx, y0, t_host, method, stack, negate, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        out = hip_ops.odeint_fixed(stack, method, y0.detach(), t_host, negate=negate)
        ctx.stack, ctx.method, ctx.t_host, ctx.negate = stack, method, t_host, negate
        hip_ops.record_versions(ctx, params)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        (y_traj,) = ctx.saved_tensors
        grads = hip_ops.odeint_adjoint_backward(ctx.stack, ctx.method, ctx.t_host, y_traj, grad_out, negate=ctx.negate)
        return _solver_backward_result(*grads, n_const=4)


class _GriddedAdjointOdeint(torch.autograd.Function):
    """_AdjointOdeint under options={"grid_constructor": fn}: the forward is odeint's own gridded solve and keeps the trajectory alone;
    the backward hands the options on to every backward interval (hip_ops.adjoint_backward_grid)."""

    @staticmethod
    def forward(ctx, y0, t_host, method, stack, func, options, *params):
        from .odeint import internal_grid
        ctx.mode = hip_ops.current_compute_dtype()
        out = hip_ops.odeint_fixed_on_grid(stack, method, y0.detach(), t_host, internal_grid(func, y0, t_host, options))
        ctx.stack, ctx.method, ctx.t_host, ctx.func, ctx.options = stack, method, t_host, func, options
        hip_ops.record_versions(ctx, params)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        (y_traj,) = ctx.saved_tensors
        grads = hip_ops.odeint_adjoint_on_grid_backward(ctx.stack, ctx.method, ctx.t_host, y_traj, grad_out, ctx.func, ctx.options)
        res = _solver_backward_result(*grads)
        return res[:4] + (None, None) + res[4:]


class _AdjointDopri5(torch.autograd.Function):
    """odeint_adjoint with method="dopri5" / "bosh3": adaptive forward (csrc/dopri5.hip), adaptive augmented backward
    (csrc/adjoint_dopri5.hip) under either norm."""

    @staticmethod
    def forward(ctx, y0, t_host, cfg, stack, *params):
        ctx.mode = hip_ops.current_compute_dtype()
        from .odeint import run_dopri5
        out, ctx.pending, _, _ = run_dopri5(stack, y0.detach(), t_host, cfg)
        ctx.stack, ctx.t_host, ctx.cfg = stack, t_host, cfg
        hip_ops.record_versions(ctx, params)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @_pinned
    def backward(ctx, grad_out):
        hip_ops.check_versions(ctx, "a parameter of the ODE dynamics")
        (y_traj,) = ctx.saved_tensors
        if ctx.pending is not None:   # the forward solve's outcome: an error (or a sealed, unfinished solve) must stop the adjoint here
            ctx.pending.collect()
            ctx.pending = None
        cfg = ctx.cfg
        stats = {}
        grads = hip_ops.odeint_adjoint_dopri5_backward(ctx.stack, ctx.t_host, y_traj, grad_out, cfg["adjoint_rtol"], cfg["adjoint_atol"],
                                                       max_accept=cfg["max_accept"], stats=stats, mixed_norm=cfg["mixed_norm"],
                                                       method=cfg.get("method", "dopri5"))
        last_adjoint_stats.clear()
        last_adjoint_stats.update(stats)
        return _solver_backward_result(*grads)


last_adjoint_stats = {}


def odeint_adjoint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint_rtol=None, adjoint_atol=None,
                   adjoint_method=None, adjoint_options=None, adjoint_params=None):
    """`torchdiffeq.odeint_adjoint(func, y0, t, rtol=, atol=, method=, adjoint_options=)`.

    Fixed-grid methods: one backward step of the same method per interval, or -- after ode_rl_amd.set_adjoint_grids(True); the options
    are refused as before without it -- with options={"grid_constructor": fn} (`interp: "linear"` next to it;
    ode_rl_amd.step_size_grid(h) for a step size), on internal grids as torchdiffeq builds them: the forward is
    `odeint`'s gridded solve, and every backward interval (t[i], t[i-1]) is an `odeint` call of its own on the flipped pair (-t[i],
    -t[i-1]), so fn is called once per interval, i = T-1 .. 1, and the sub-steps of a step size are anchored at t[i], not at t[i-1]
    -- they differ from the forward grid's wherever h does not divide the interval.  Inside an interval the solver carries y itself;
    at an output time y is reset to the stored trajectory and a_y takes grad_out.  Between forward and backward only the (T,B,C,16,16)
    trajectory is kept, where autograd through `odeint` keeps every activation of the whole grid; the backward's scratch holds the
    activations of the backward grid.  Not in bf16 mode (TypeError); `adjoint_options` stay refused.  dopri5: adaptive backward solve with
    torchdiffeq's default mixed norm (every parameter tensor's error ratio steers the steps too) or, with
    `adjoint_options={"norm": "seminorm"}`, with the cheaper seminorm; `max_accept` in adjoint_options bounds the accepted
    backward steps whose activations are kept.

    A strictly decreasing t raises NotImplementedError, as it always did, until ode_rl_amd.set_reverse_time_grads(True).  Then the
    fixed-grid methods without an internal grid take it as torchdiffeq does: the forward is the solve of the negated dynamics on -t, and
    every backward interval runs from -t[i] back to -t[i-1] on the negation of the negated dynamics, plain f (fp32 mode; TypeError in
    bf16 mode).  dopri5 / bosh3 and `grid_constructor` on a decreasing t stay refused, each by a NotImplementedError of its own."""
    from .odeint import ADAPTIVE, FIXED_GRID, _check_monotone, _host_times, check_options, conv_stack_of, dopri5_cfg, odeint
    if method is None:
        method = "dopri5"
    if method not in FIXED_GRID + ADAPTIVE:
        raise ValueError('Invalid method "{}". Must be one of euler, midpoint, rk4, dopri5, bosh3'.format(method))
    if adjoint_method is not None and adjoint_method != method:
        raise NotImplementedError("odeint_adjoint(HIP): adjoint_method must equal method")
    check_options(method, options, "odeint_adjoint")
    gridded = method in FIXED_GRID and (options or {}).get("grid_constructor") is not None
    if gridded and hip_ops.current_compute_dtype() == "bf16":
        raise TypeError("odeint_adjoint(HIP): internal grids (grid_constructor) are not implemented in bf16 compute mode (fp32 only); "
                        'use set_compute_dtype("f32") or drop the grid')
    if adjoint_params is not None and ({id(p) for p in adjoint_params} != {id(p) for p in func.parameters()}):
        # torchdiffeq integrates a_theta for exactly these tensors; this path always does so for every parameter of `func`
        raise NotImplementedError("odeint_adjoint(HIP): adjoint_params must be omitted or be all of func.parameters()")
    if method in FIXED_GRID and adjoint_options:
        raise ValueError(f"odeint_adjoint(HIP): unsupported {method} adjoint_options {sorted(adjoint_options)}")
    if not torch.is_grad_enabled() or not (y0.requires_grad or any(p.requires_grad for p in func.parameters())):
        return odeint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options)
    hip_ops.require_device_tensor(y0, "y0")
    th = _host_times(t)
    _check_monotone(th)
    negate = len(th) > 1 and bool(th[0] > th[1])
    if negate:
        if not hip_ops.reverse_time_grads_enabled():
            raise NotImplementedError("odeint_adjoint(HIP): decreasing time grids are not supported" + hip_ops.REVERSE_TIME_HINT)
        if method not in FIXED_GRID:
            raise NotImplementedError(f"odeint_adjoint(HIP): a strictly decreasing t under method {method!r} is not implemented (the adaptive "
                                      "adjoint of the negated dynamics, under either norm); use euler / midpoint / rk4, or odeint, "
                                      "which differentiates dopri5 and bosh3 on a decreasing t")
        if gridded:
            raise NotImplementedError("odeint_adjoint(HIP): a strictly decreasing t with options['grid_constructor'] is not implemented "
                                      "(internal grids of the backward intervals of a negated solve); drop the grid, or use odeint")
        if hip_ops.current_compute_dtype() == "bf16":
            raise TypeError("odeint_adjoint(HIP): gradients through a strictly decreasing t are not implemented in bf16 compute mode "
                            '(fp32 only); use set_compute_dtype("f32")')
        th = -th   # torchdiffeq: the negated dynamics on -t
    stack = conv_stack_of(func)
    params = _stack_params(stack)
    if gridded:
        return _GriddedAdjointOdeint.apply(y0, th, method, stack, func, options, *params)
    if method in FIXED_GRID:
        return _AdjointOdeint.apply(y0, th, method, stack, negate, *params)
    adjoint_options = dict(adjoint_options or {})
    norm = adjoint_options.get("norm")
    if norm not in (None, "mixed", "seminorm"):
        raise ValueError(f'odeint_adjoint(HIP): adjoint_options["norm"] must be "seminorm" or omitted (torchdiffeq\'s mixed norm); got {norm!r}')
    unknown = set(adjoint_options) - {"norm", "max_accept"}
    if unknown:
        raise ValueError(f"odeint_adjoint(HIP): unsupported adjoint_options {sorted(unknown)}")
    cfg = dopri5_cfg(rtol, atol, options, method)
    cfg.update(adjoint_rtol=float(rtol if adjoint_rtol is None else adjoint_rtol),
               adjoint_atol=float(atol if adjoint_atol is None else adjoint_atol), max_accept=adjoint_options.get("max_accept"),
               mixed_norm=norm != "seminorm")
    return _AdjointDopri5.apply(y0, th, cfg, stack, *params)


def odeint_with_grad(func, y0, t, rtol, atol, method, options=None):
    from .odeint import FIXED_GRID, _check_monotone, _host_times, check_options, conv_stack_of, dopri5_cfg, internal_grid
    check_options(method, options)
    th = _host_times(t)
    _check_monotone(th)
    negate = len(th) > 1 and bool(th[0] > th[1])
    if negate:
        if not hip_ops.reverse_time_grads_enabled():
            raise NotImplementedError("odeint(HIP): reversed-time integration is not implemented yet" + hip_ops.REVERSE_TIME_HINT)
        if hip_ops.current_compute_dtype() == "bf16":
            raise TypeError("odeint(HIP): gradients through a strictly decreasing t are not implemented in bf16 compute mode (fp32 only); "
                            'use set_compute_dtype("f32")')
        th = -th   # torchdiffeq: the negated dynamics on -t, as in odeint_forward
    stack = conv_stack_of(func)
    params = _stack_params(stack)
    if method in FIXED_GRID:
        grid = internal_grid(func, y0, th, options)   # of -t for a decreasing t, as in the forward
        if grid is not None:
            return _GriddedOdeint.apply(y0, th, method, stack, grid, negate, *params)
        return _FixedGridOdeint.apply(y0, th, method, stack, negate, *params)
    cfg = dopri5_cfg(rtol, atol, options, method)
    if negate:
        cfg["negate"] = True
    return _Dopri5Odeint.apply(y0, th, cfg, stack, *params)


class _SampleZ0Fn(torch.autograd.Function):
    """z0 ~ N(mean, std) by the reparameterisation trick, and KL(N(mean, std) || N(0, 1)) per batch row (csrc/latent_sample.hip).  Keeps
    mean, std and either the caller's eps or the four integers of the counter-based draw: the backward regenerates the noise."""

    @staticmethod
    def forward(ctx, mean, std, n_samples, eps, noise, want_kl):
        seed, offset, batch_offset, global_batch = noise
        z0, kl, _ = hip_ops.latent_sample(mean, std, n_samples, seed, offset, batch_offset, global_batch, eps_in=eps, want_kl=want_kl)
        ctx.n_samples, ctx.noise, ctx.has_eps = n_samples, noise, eps is not None
        ctx.set_materialize_grads(False)   # an unused kl arrives as None, not as zeros: no KL term in the backward then
        ctx.save_for_backward(mean, std, *([eps] if eps is not None else []))   # unpacking them checks their versions
        return z0, kl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_z0, grad_kl):
        mean, std = ctx.saved_tensors[:2]
        eps = ctx.saved_tensors[2] if ctx.has_eps else None
        if grad_z0 is None:   # only the KL term was used
            grad_z0 = torch.zeros((ctx.n_samples * mean.shape[0],) + tuple(mean.shape[1:]), dtype=mean.dtype, device=mean.device)
        seed, offset, batch_offset, global_batch = ctx.noise
        gm, gs = hip_ops.latent_sample_backward(grad_z0, grad_kl, mean, std, ctx.n_samples, seed, offset, batch_offset, global_batch, eps_in=eps)
        return gm, gs, None, None, None, None


_explicit_seed = [None, 0]   # the last seed a caller passed to sample_z0 and the offset its next call takes
_noise_shard = None          # (batch_offset, global_batch) under batch sharding (dist.set_noise_shard), None on one device
_last_draw = None            # what last_z0_noise() regenerates from


def set_noise_shard(batch_offset=None, global_batch=None):
    """Place this process's batch rows in a global batch for the noise of sample_z0 (dist.set_noise_shard calls this with the
    shard's bounds); no arguments: back to one device.  Returns the previous setting."""
    global _noise_shard
    was = _noise_shard
    if batch_offset is None and global_batch is None:
        _noise_shard = None
        return was
    batch_offset, global_batch = int(batch_offset), int(global_batch)
    if not 0 <= batch_offset < global_batch:
        raise ValueError(f"set_noise_shard: batch_offset {batch_offset} does not lie in a global batch of {global_batch}")
    _noise_shard = (batch_offset, global_batch)
    return was


def _next_noise_position(seed, device):
    """(seed, offset) of this call.  seed None: the default CUDA generator's initial_seed(), and the offset lives IN that generator
    (its Philox offset in units of 4, advanced by one unit here): torch.manual_seed(s) restarts the sequence, torch.cuda.get_rng_state
    checkpoints the position.  An explicit seed: the library counts the calls and restarts when the seed changes."""
    if seed is None:
        gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        at = gen.get_offset()
        gen.set_offset(at + 4)
        return gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, at // 4
    if _explicit_seed[0] != seed:
        _explicit_seed[:] = [seed, 0]
    offset = _explicit_seed[1]
    _explicit_seed[1] = offset + 1
    return seed, offset


def sample_z0(mean, std, n_samples=1, eps=None, seed=None, return_kl=True):
    """z0 ~ N(mean, std) and its KL term, on the device in one launch each way (csrc/latent_sample.hip).

    mean, std: (B, C, 16, 16) float32 device tensors, C % 4 == 0 (the encoder head's mean_z0, std_z0).  Returns (z0, kl):
      z0 (n_samples * B, C, 16, 16), sample-major -- row k * B + b is mean[b] + std[b] * eps[k, b] -- ready for the solver;
      kl (B,) = sum over (C, 16, 16) of KL(N(mean, std) || N(0, 1)), or None with return_kl=False.  No clamp: std == 0 gives +inf.
    Differentiable with respect to mean and std (once).  Noise: `eps` (z0's shape), the caller's own, or the counter-based stream of
    include/odecgru_hip.h with (seed, offset): seed=None takes the default CUDA generator's seed, so torch.manual_seed(s) makes a run
    reproducible; every call advances the offset by one (see _next_noise_position).  Under batch sharding (dist.set_noise_shard) a
    rank draws the rows the full batch would have drawn.  Arguments are checked before tensors; there is no CPU fallback."""
    global _last_draw
    if isinstance(n_samples, bool) or not isinstance(n_samples, int) or not 1 <= n_samples <= 65535:
        raise ValueError(f"sample_z0: n_samples must be an int in [1, 65535], got {n_samples!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"sample_z0: seed must be None or an int in [0, 2**64), got {seed!r}")
    if eps is not None and seed is not None:
        raise ValueError("sample_z0: eps brings its own noise; a seed with it would be ignored")
    b, c = hip_ops._check_latent_pair(mean, std, "sample_z0")
    if eps is not None:
        eps = hip_ops._check_noise_rows(eps, "eps", n_samples * b, c, mean, "sample_z0")
        noise = (0, 0, 0, b)
    else:
        batch_offset, global_batch = _noise_shard if _noise_shard is not None else (0, b)
        if batch_offset + b > global_batch:
            raise ValueError(f"sample_z0: rows [{batch_offset}, {batch_offset + b}) exceed the global batch of {global_batch} (set_noise_shard)")
        noise = _next_noise_position(seed, mean.device) + (batch_offset, global_batch)
    _last_draw = (eps, noise, n_samples, b, c, mean.device)
    want_kl = bool(return_kl)
    if torch.is_grad_enabled() and (mean.requires_grad or std.requires_grad):
        return _SampleZ0Fn.apply(mean, std, n_samples, eps, noise, want_kl)
    z0, kl, _ = hip_ops.latent_sample(mean, std, n_samples, *noise, eps_in=eps, want_kl=want_kl)
    return z0, kl


def last_z0_noise():
    """The noise of the most recent sample_z0 call, (n_samples * B, C, 16, 16): the caller's eps, or the stream regenerated from
    the call's (seed, offset, batch_offset, global_batch) through `eps_out` -- nothing was stored."""
    if _last_draw is None:
        raise RuntimeError("last_z0_noise: sample_z0 has not been called")
    eps, noise, n_samples, b, c, device = _last_draw
    if eps is not None:
        return eps
    zero = torch.zeros((b, c, 16, 16), dtype=torch.float32, device=device)
    return hip_ops.latent_sample(zero, zero, n_samples, *noise, want_kl=False, want_eps=True)[2]


class _MseKlLossFn(torch.autograd.Function):
    """mean (pred - truth)^2 + kl_weight * kl_scale * sum(kl) (csrc/frame_loss.hip): two launches forward, one backward.  Returns
    (loss, mse, kl_term), three views of one device buffer; only `loss` is differentiable.  The backward reads pred, truth live."""

    @staticmethod
    def forward(ctx, pred, truth, kl, kl_weight, kl_scale):
        hip_ops.record_versions(ctx, tuple(x for x in (pred, truth, kl) if x is not None))
        ctx.pred, ctx.truth = pred.detach().contiguous(), truth.detach().contiguous()
        ctx.kl_weight, ctx.kl_scale, ctx.has_kl = kl_weight, kl_scale, kl is not None
        ctx.set_materialize_grads(False)
        loss, mse, kl_term = hip_ops.loss_mse(ctx.pred, ctx.truth, kl, kl_weight, kl_scale).unbind(0)
        ctx.mark_non_differentiable(mse, kl_term)
        return loss, mse, kl_term

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_mse, _grad_kl_term):
        if grad_loss is None:
            return None, None, None, None, None
        hip_ops.check_versions(ctx, "an input of mse_kl_loss")
        grad_pred, grad_kl = hip_ops.loss_mse_backward(grad_loss, ctx.pred, ctx.truth, ctx.kl_weight, ctx.kl_scale, want_kl=ctx.has_kl)
        ctx.pred = ctx.truth = None
        return grad_pred, None, grad_kl, None, None


class _VidodeL1LossFn(torch.autograd.Function):
    """The L1 pair of models/VidODE.py's get_loss (csrc/frame_loss.hip): two launches forward, one backward, no host synchronisation.
    Returns (loss, l1_pred, l1_diff); only `loss` is differentiable, with respect to pred and inter."""

    @staticmethod
    def forward(ctx, pred, inter, truth, init, mask):
        hip_ops.record_versions(ctx, (pred, inter, truth, init, mask))
        ctx.args = (pred.detach(), inter.detach(), truth.detach(), init.detach(), mask.detach())
        ctx.set_materialize_grads(False)
        loss, l1_pred, l1_diff = hip_ops.loss_vidode_l1(*ctx.args).unbind(0)
        ctx.mark_non_differentiable(l1_pred, l1_diff)
        return loss, l1_pred, l1_diff

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_l1_pred, _grad_l1_diff):
        if grad_loss is None:
            return None, None, None, None, None
        hip_ops.check_versions(ctx, "an input of vidode_l1_loss")
        grad_pred, grad_inter = hip_ops.loss_vidode_l1_backward(grad_loss, *ctx.args)
        ctx.args = None
        return grad_pred, grad_inter, None, None, None


def _constants(who, **tensors):
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"{who}: {name} is treated as a constant; a gradient with respect to it is not implemented")


def _fused_loss_ok(row_elems, *tensors):
    """The fused path of csrc/frame_loss.hip: CUDA float32 tensors, rows of a multiple of 4 elements, ODEHIP_FUSED_LOSS not 0."""
    return (hip_ops.fused_loss_enabled() and row_elems >= 4 and row_elems % 4 == 0 and
            all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors))


def mse_kl_loss(pred, truth, kl=None, kl_weight=1.0, latent_elems=None):
    """The training loss of ODEConvGRU / ConvGRU: (loss, mse, kl_term) with
        mse = mean (pred - truth)^2,  kl_term = mean_b kl[b] / latent_elems,  loss = mse + kl_weight * kl_term.
    pred (K * B, ...) holds K draws per truth row, sample-major: row k * B + b pairs with truth row b (B, ...); the truth is not
    repeated in memory.  kl (B,): the KL term per batch row (`sample_z0`), latent_elems the latent elements per row; kl=None: loss =
    mse and kl_term is None.  `loss` carries the graph (to pred and kl); mse and kl_term are detached scalars.  truth is a constant.
    CUDA float32 tensors with a row size that is a multiple of 4: one C ABI call each way (csrc/frame_loss.hip: float64 sums in a
    fixed order, two launches forward, one backward).  Anything else, or ODEHIP_FUSED_LOSS=0: the torch composition."""
    if not isinstance(pred, torch.Tensor) or not isinstance(truth, torch.Tensor):
        raise TypeError("mse_kl_loss: pred and truth must be torch.Tensors")
    if kl is not None and not isinstance(kl, torch.Tensor):
        raise TypeError("mse_kl_loss: kl must be a torch.Tensor or None")
    _constants("mse_kl_loss", truth=truth)
    if truth.dim() < 1 or pred.dim() != truth.dim() or truth.shape[0] < 1 or pred.shape[0] < 1 or pred.shape[0] % truth.shape[0] or \
            pred.shape[1:] != truth.shape[1:]:
        raise ValueError(f"mse_kl_loss: pred must be (K * B, ...) with truth's (B, ...) trailing shape, got {tuple(pred.shape)} for "
                         f"{tuple(truth.shape)}")
    b = truth.shape[0]
    n = pred.shape[0] // b
    if kl is not None:
        if isinstance(latent_elems, bool) or not isinstance(latent_elems, int) or latent_elems < 1:
            raise ValueError(f"mse_kl_loss: with kl, latent_elems must be a positive int (the latent elements per batch row), got {latent_elems!r}")
        if tuple(kl.shape) != (b,):
            raise ValueError(f"mse_kl_loss: kl must be ({b},), got {tuple(kl.shape)}")
    kl_weight = float(kl_weight)
    if _fused_loss_ok(truth[0].numel(), pred, truth, *([kl] if kl is not None else [])):
        kl_scale = 1.0 / (b * latent_elems) if kl is not None else 0.0
        if torch.is_grad_enabled() and (pred.requires_grad or (kl is not None and kl.requires_grad)):
            loss, mse, kl_term = _MseKlLossFn.apply(pred, truth, kl, kl_weight, kl_scale)
        else:
            loss, mse, kl_term = hip_ops.loss_mse(pred, truth, kl, kl_weight, kl_scale).unbind(0)
        return loss, mse, (kl_term if kl is not None else None)
    if n > 1:
        truth = truth.repeat(n, *([1] * (truth.dim() - 1)))
    mse = torch.nn.functional.mse_loss(pred, truth)
    if kl is None:
        return mse, mse.detach(), None
    kl_term = kl.mean() / latent_elems
    return mse + kl_weight * kl_term, mse.detach(), kl_term.detach()


def vidode_l1_loss(pred, inter, truth, init, mask):
    """The training loss of VidODE (reference models/VidODE.py:211-226): (loss, l1_pred, l1_diff) with
        l1_pred = mean |pred - truth[selected]|,  l1_diff = mean |inter - d[selected]|,  loss = l1_pred + l1_diff,
    d[:, t] = truth[:, t] - truth[:, t - 1] and truth[:, -1] = init, the last observed frame.  pred, inter (B, n, c, H, W) -- inter
    may be a channel slice --, truth (B, T, c, H, W), init (B, c, H, W), mask (B, T) or (B, T, 1): non-zero selects a frame, the first
    n selected frames of every row count; a row with fewer makes the result NaN on the fused path (the torch composition raises).
    `loss` carries the graph (to pred and inter); the two terms are detached scalars.  truth, init and mask are constants.
    CUDA float32 tensors with a frame size that is a multiple of 4: one C ABI call each way, no host synchronisation
    (csrc/frame_loss.hip).  Anything else, or ODEHIP_FUSED_LOSS=0: the torch composition (its boolean indexing synchronises)."""
    for name, t in (("pred", pred), ("inter", inter), ("truth", truth), ("init", init), ("mask", mask)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"vidode_l1_loss: {name} must be a torch.Tensor")
    _constants("vidode_l1_loss", truth=truth, init=init, mask=mask)
    if pred.dim() < 3 or truth.dim() != pred.dim() or truth.shape[0] != pred.shape[0] or truth.shape[2:] != pred.shape[2:] or \
            not 1 <= pred.shape[1] <= truth.shape[1]:
        raise ValueError(f"vidode_l1_loss: pred must be (B, n, ...) and truth (B, T >= n, ...) with the same frames, got {tuple(pred.shape)} "
                         f"and {tuple(truth.shape)}")
    if inter.shape != pred.shape:
        raise ValueError(f"vidode_l1_loss: inter must have pred's shape {tuple(pred.shape)}, got {tuple(inter.shape)}")
    if tuple(init.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
        raise ValueError(f"vidode_l1_loss: init must be {(pred.shape[0],) + tuple(pred.shape[2:])}, got {tuple(init.shape)}")
    if tuple(mask.shape) not in (tuple(truth.shape[:2]), tuple(truth.shape[:2]) + (1,)):
        raise ValueError(f"vidode_l1_loss: mask must be {tuple(truth.shape[:2])} (or with a trailing 1), got {tuple(mask.shape)}")
    if _fused_loss_ok(pred[0, 0].numel(), pred, inter, truth, init) and mask.is_cuda:
        if torch.is_grad_enabled() and (pred.requires_grad or inter.requires_grad):
            return _VidodeL1LossFn.apply(pred, inter, truth, init, mask)
        return tuple(hip_ops.loss_vidode_l1(pred, inter, truth, init, mask).unbind(0))
    b, n = pred.shape[0], pred.shape[1]
    sel = (mask.squeeze(-1) if mask.dim() == 3 else mask).bool()
    data = torch.cat([init.unsqueeze(1), truth], dim=1)
    d = data[:, 1:, ...] - data[:, :-1, ...]
    count = pred[0].numel() * b
    data_diff = d[sel].view((b, n) + tuple(pred.shape[2:]))
    l1_pred = torch.mean(torch.sum(torch.abs(pred - truth[sel].view((b, n) + tuple(pred.shape[2:])))) / count)
    l1_diff = torch.mean(torch.sum(torch.abs(inter - data_diff)) / count)
    return torch.mean(l1_pred + l1_diff), l1_pred.detach(), l1_diff.detach()


class _InstNormLReluFn(torch.autograd.Function):
    """InstanceNorm (no affine) + LeakyReLU(slope) over the planes of x (csrc/instnorm_act.hip): one launch each way."""

    @staticmethod
    def forward(ctx, x, eps, slope):
        y, mean, rstd = hip_ops.instnorm_lrelu(x, eps, slope)
        ctx.save_for_backward(x, mean, rstd)
        ctx.slope = slope
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd = ctx.saved_tensors
        return hip_ops.instnorm_lrelu_backward(grad_y, x, mean, rstd, ctx.slope), None, None


def instnorm_lrelu(x, eps=1e-5, slope=0.2):
    """F.leaky_relu(F.instance_norm(x, eps=eps), slope) for x (N, C, ...) float32 on the device, in one launch forward and one backward
    (csrc/instnorm_act.hip): a plane of up to 1024 elements is read once and written once.  slope=0 is InstanceNorm + ReLU.  Statistics
    in float64, never E[x^2] - mean^2; a NaN or Inf stays in its plane.  There is no CPU path."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("instnorm_lrelu: x must be a torch.Tensor")
    eps, slope = float(eps), float(slope)
    if torch.is_grad_enabled() and x.requires_grad:
        return _InstNormLReluFn.apply(x, eps, slope)
    return hip_ops.instnorm_lrelu(x, eps, slope)[0]


class _GanSeqFn(torch.autograd.Function):
    """The rows of the sequence discriminator (csrc/gan.hip): one gather launch each way; differentiable in `frames` alone."""

    @staticmethod
    def forward(ctx, input_real, frames, interp):
        ctx.shape, ctx.t_in, ctx.interp = tuple(frames.shape), input_real.shape[1], interp
        return hip_ops.gan_seq_assemble(input_real, frames, interp)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return None, hip_ops.gan_seq_assemble_backward(grad_out, ctx.shape, ctx.t_in, ctx.interp), None


def gan_sequences(input_real, frames, interp=False):
    """What Vid-ODE's sequence discriminator judges (reference Vid-ODE/models/gan.py, get_real_fake_seqs / rearrange_seq_interp), built
    in one launch instead of a loop of torch.cat: input_real (b, t_in, c, h, w), frames (b, t, c, h, w) -> (t * b, L * c, h, w).
        extrapolation   row i * b + n = [zeros x (L - l_i)] ++ input_real[n, i:] ++ frames[n, :i+1],  L = max(t, t_in + 1)
        interp=True     row i * b + n = input_real[n] with frame i replaced by frames[n, i]  (needs t_in == t; L = t)
    The graph reaches `frames` (one gather launch backward); input_real is a constant, as upstream uses it."""
    for name, x in (("input_real", input_real), ("frames", frames)):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"gan_sequences: {name} must be a torch.Tensor")
    _constants("gan_sequences", input_real=input_real)
    if torch.is_grad_enabled() and frames.requires_grad:
        return _GanSeqFn.apply(input_real, frames, bool(interp))
    return hip_ops.gan_seq_assemble(input_real, frames, bool(interp))


class _LsganLossFn(torch.autograd.Function):
    """mean (pred - target)^2 (csrc/gan.hip): two launches forward, one backward."""

    @staticmethod
    def forward(ctx, pred, target):
        ctx.save_for_backward(pred)
        ctx.target = target
        return hip_ops.loss_lsgan(pred, target)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        pred, = ctx.saved_tensors
        return hip_ops.loss_lsgan_backward(grad_loss, pred, ctx.target).view(pred.shape), None


def lsgan_loss(pred, target):
    """The LSGAN term mean (pred - target)^2 against a constant label (0: fake, 1: real) as a device scalar, without the label tensor:
    float64 sums in a fixed order, two launches forward, one backward (csrc/gan.hip).  There is no CPU path."""
    if not isinstance(pred, torch.Tensor):
        raise TypeError("lsgan_loss: pred must be a torch.Tensor")
    target = float(target)
    if torch.is_grad_enabled() and pred.requires_grad:
        return _LsganLossFn.apply(pred, target)
    return hip_ops.loss_lsgan(pred, target)
