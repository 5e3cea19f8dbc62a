"""Upstream Vid-ODE's own model (Vid-ODE/models/conv_odegru.py, base_conv_gru.py, ode_func.py, layers.py; built at main.py:164) around
the HIP hot path: constructor signatures, attribute names and state_dict keys are upstream's, so its checkpoints load key for key.
`models/VidODE.py` is the ODE-RL repository's re-typing of it and a different network (5x5 GroupNorm cell, ReLU dynamics).

What runs where
  * `ConvGRUCell`: 3x3 convolutions, no normalisation, gates split RESET first, UPDATE second, h' = (1-u) h + u c
    (base_conv_gru.py:47-72): one C call each way (csrc/convgru_plain.hip between the convolutions of csrc/conv_q4.hip);
  * `Encoder_z0_ODE_ConvGRU`: the whole reverse-time Euler + ConvGRU loop and `transform_z0` in ONE C call each way, observation mask
    included (odehip_odeconvgru_encode*_masked with a plain cell descriptor).  Only `cell_list[0]` is ever called (upstream :186); the
    other cells exist for the keys and keep `grad is None`;
  * `DiffeqSolver`: `ode_rl_amd.odeint`, result permuted to batch-first as upstream (:72);
  * `Encoder` / `Decoder`: the fused BatchNorm / ReLU / upsampling passes of `models/VidODE.py` under upstream's keys (and, with
    them, its cross-rank statistics under batch sharding: `ode_rl_amd.dist.sync_batchnorm`);
  * warp chain + compositing and the L1 loss: `warp_composite`, `vidode_l1_loss`.

`fused=False` (cell, encoder, solver, and through `VidODE(opt, device, fused=False)` every part of the model: BatchNorm / ReLU /
upsampling module by module, the warp chain by `grid_sample`, the loss by `get_mse` / `get_diff`) runs upstream's computation in plain
torch ops on the same parameters, the dynamics through the `nn.Sequential` itself; it also runs on the CPU and is what the tests and
tools compare against.  One difference to upstream's arithmetic in both flavours: the Euler step sizes are differences of the float64
host times, rounded to float32 once (upstream subtracts float32 tensors).

Not reproduced: the tracker's per-step `.cpu()` copies, the NaN asserts and the "first point" check (:168-180), `nru` / `nru2` (both
call `odeint` on a one-point grid, which returns its input) and slot attention (upstream leaves it at `pass`)."""
import torch
import torch.nn as nn

from .. import hip_ops
from ..autograd import warp_composite, vidode_l1_loss
from ..odeint import odeint, conv_stack_of
from . import VidODE as _flow


def create_convnet(n_inputs, n_outputs, n_layers=1, n_units=128, nonlinear='tanh'):
    """Upstream layers.py:15-32: Conv3x3, (Tanh, Conv3x3) x n_layers, Tanh, Conv3x3 -- no final activation."""
    if nonlinear != 'tanh':
        raise NotImplementedError('There is no named')
    layers = [nn.Conv2d(n_inputs, n_units, 3, 1, 1, dilation=1)]
    for _ in range(n_layers):
        layers += [nn.Tanh(), nn.Conv2d(n_units, n_units, 3, 1, 1, dilation=1)]
    layers += [nn.Tanh(), nn.Conv2d(n_units, n_outputs, 3, 1, 1, dilation=1)]
    return nn.Sequential(*layers)


class ODEFunc(nn.Module):
    def __init__(self, opt, input_dim, latent_dim, ode_func_net, device=torch.device("cpu")):
        super().__init__()
        self.input_dim, self.device, self.opt = input_dim, device, opt
        self.gradient_net = ode_func_net

    def forward(self, t_local, y, backwards=False):
        """dy/dt at y (autonomous).  Device tensors go through the HIP stack; host tensors through the Sequential itself."""
        if not y.is_cuda:
            grad = self.gradient_net(y)
            return -grad if backwards else grad
        return hip_ops.convstack_forward(conv_stack_of(self), y, negate=backwards)

    def get_ode_gradient_nn(self, t_local, y):
        return self.forward(t_local, y)

    def sample_next_point_from_prior(self, t_local, y):
        return self.get_ode_gradient_nn(t_local, y)


class DiffeqSolver(nn.Module):
    def __init__(self, input_dim, ode_func, method, latents, odeint_rtol=1e-4, odeint_atol=1e-5, device=torch.device("cpu"), nru=False,
                 nru2=False, fused=True):
        super().__init__()
        self.fused = fused
        if nru is True or nru2 is True:
            raise NotImplementedError("DiffeqSolver: nru / nru2 call odeint on a one-point grid upstream (it returns its input); not implemented")
        self.ode_method, self.latents, self.device, self.ode_func = method, latents, device, ode_func
        self.nru, self.nru2 = nru, nru2
        self.odeint_rtol, self.odeint_atol = odeint_rtol, odeint_atol

    def forward(self, first_point, time_steps_to_predict, backwards=False):
        """(B, T, C, h, w) batch-first (upstream ode_func.py:70-72).  An unknown method ('adams') raises as `odeint` does.
        fused=False: explicit Euler on the requested times in torch ops, the only method the composition restates."""
        if not self.fused:
            if self.ode_method != "euler":
                raise NotImplementedError(f"DiffeqSolver(fused=False) restates 'euler' only, got {self.ode_method!r}")
            times = [float(v) for v in hip_ops.host_times(time_steps_to_predict)]
            ys = [first_point]
            for k in range(1, len(times)):
                ys.append(ys[-1] + self.ode_func.gradient_net(ys[-1]) * (times[k] - times[k - 1]))
            return torch.stack(ys, 1)
        pred_y = odeint(self.ode_func, first_point, time_steps_to_predict, rtol=self.odeint_rtol, atol=self.odeint_atol,
                        method=self.ode_method)
        return pred_y.permute(1, 0, 2, 3, 4)


class ConvGRUCell(nn.Module):
    def __init__(self, input_size, input_dim, hidden_dim, kernel_size, bias, dtype, fused=True):
        super().__init__()
        self.height, self.width = input_size
        self.padding = kernel_size[0] // 2, kernel_size[1] // 2
        self.hidden_dim, self.bias, self.dtype, self.fused = hidden_dim, bias, dtype, fused
        self.conv_gates = nn.Conv2d(input_dim + hidden_dim, 2 * hidden_dim, kernel_size, padding=self.padding, bias=bias)
        self.conv_can = nn.Conv2d(input_dim + hidden_dim, hidden_dim, kernel_size, padding=self.padding, bias=bias)

    def init_hidden(self, batch_size):
        return torch.zeros(batch_size, self.hidden_dim, self.height, self.width, device=self.conv_can.weight.device)

    def _packed(self):
        p = getattr(self, "_hip_cell", None)
        if p is None:
            p = hip_ops.PackedCell(self)
            object.__setattr__(self, "_hip_cell", p)
        return p

    def compose(self, input_tensor, h_cur, mask=None):
        """Upstream's forward in torch ops (base_conv_gru.py:54-72)."""
        gates = self.conv_gates(torch.cat([input_tensor, h_cur], dim=1))
        reset_gate, update_gate = torch.split(gates, self.hidden_dim, dim=1)
        reset_gate, update_gate = torch.sigmoid(reset_gate), torch.sigmoid(update_gate)
        cand = torch.tanh(self.conv_can(torch.cat([input_tensor, reset_gate * h_cur], dim=1)))
        h_next = (1 - update_gate) * h_cur + update_gate * cand
        if mask is None:
            return h_next
        mask = mask.view(-1, 1, 1, 1).expand_as(h_cur)
        return mask * h_next + (1 - mask) * h_cur

    def forward(self, input_tensor, h_cur, mask=None):
        """(b, input_dim, h, w), (b, hidden_dim, h, w) -> h_next; mask (b,) or (b, 1) blends m h_next + (1 - m) h_cur.  fused: one C call
        each way for the cell (the blend of a lone step is two torch ops around it; inside the encoder it is part of the update kernel)."""
        if not self.fused:
            return self.compose(input_tensor, h_cur, mask)
        if torch.is_grad_enabled() and (input_tensor.requires_grad or h_cur.requires_grad or any(p.requires_grad for p in self.parameters())):
            from ..autograd import cell_with_grad
            h_next = cell_with_grad(self._packed(), input_tensor, h_cur)
        else:
            h_next = hip_ops.convgru_cell_forward(self._packed(), input_tensor, h_cur)
        if mask is None:
            return h_next
        mask = mask.view(-1, 1, 1, 1).to(h_next.dtype)
        return mask * h_next + (1 - mask) * h_cur


class Encoder_z0_ODE_ConvGRU(nn.Module):
    def __init__(self, input_size, input_dim, hidden_dim, kernel_size, num_layers, dtype, batch_first=False, bias=True,
                 return_all_layers=False, z0_diffeq_solver=None, run_backwards=None, opt=None, fused=True):
        super().__init__()
        kernel_size = self._extend_for_multilayer(kernel_size, num_layers)
        hidden_dim = self._extend_for_multilayer(hidden_dim, num_layers)
        if not len(kernel_size) == len(hidden_dim) == num_layers:
            raise ValueError('Inconsistent list length.')
        self.height, self.width = input_size
        self.input_dim, self.hidden_dim, self.kernel_size, self.dtype = input_dim, hidden_dim, kernel_size, dtype
        self.num_layers, self.batch_first, self.bias, self.return_all_layers = num_layers, batch_first, bias, return_all_layers
        self.z0_diffeq_solver, self.run_backwards, self.opt, self.fused = z0_diffeq_solver, run_backwards, opt, fused
        self.by_product = {}
        self.cell_list = nn.ModuleList([
            ConvGRUCell(input_size=(self.height, self.width), input_dim=input_dim if i == 0 else hidden_dim[i - 1],
                        hidden_dim=hidden_dim[i], kernel_size=kernel_size[i], bias=bias, dtype=dtype, fused=fused)
            for i in range(num_layers)])
        self.z0_dim = z = hidden_dim[0]
        self.transform_z0 = nn.Sequential(nn.Conv2d(z, z, 1, 1, 0), nn.ReLU(), nn.Conv2d(z, z * 2, 1, 1, 0))

    @staticmethod
    def _extend_for_multilayer(param, num_layers):
        return param if isinstance(param, list) else [param] * num_layers

    def _packed(self):
        p = getattr(self, "_hip_enc", None)
        if p is None:
            p = hip_ops.PackedEncoder(conv_stack_of(self.z0_diffeq_solver.ode_func), self.cell_list[0]._packed(), self.transform_z0)
            object.__setattr__(self, "_hip_enc", p)
        return p

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in hip_ops.encoder_params(self._packed())))

    def _encode(self, input_tensor, time_steps, mask, run_backwards, want_latent, steps=None):
        """The fused call on batch-first frames: (mean, std, latent_ys or None).  steps: hip_ops.encoder_steps -- by default a frame no
        sample of a HOST mask observed launches nothing of the cell."""
        hip_ops.require_device_tensor(input_tensor, "input_tensor")
        frames = input_tensor.permute(1, 0, 2, 3, 4)   # the library reads time-first frames
        if self._wants_grad(input_tensor):
            from ..autograd import encode_with_grad
            out = encode_with_grad(self._packed(), frames, time_steps, want_latent=want_latent, run_backwards=run_backwards, mask=mask,
                                   steps=steps)
            return out if want_latent else out + (None,)
        return hip_ops.odeconvgru_encode(self._packed(), frames, time_steps, want_latent=want_latent, run_backwards=run_backwards, mask=mask,
                                         steps=steps)

    def forward(self, input_tensor, time_steps, mask=None, tracker=None, steps=None):
        """-> (mean_z0, |std_z0|), each (b, z0_dim, h, w).  mask (b, t) or (b, t, 1), indexed by frame; None = every frame observed.
        `tracker` is accepted and ignored.  steps (fused only): see `_encode`."""
        if not self.batch_first:
            input_tensor = input_tensor.permute(1, 0, 2, 3, 4)
        assert input_tensor.size(1) == len(time_steps), "Sequence length should be same as time_steps"
        if self.fused:
            mean, std, _ = self._encode(input_tensor, time_steps, mask, self.run_backwards, False, steps)
            return mean, std
        last_yi, _ = self.run_ode_conv_gru(input_tensor=input_tensor, mask=mask, time_steps=time_steps, run_backwards=self.run_backwards)
        mean_z0, std_z0 = torch.split(self.transform_z0(last_yi), self.z0_dim, dim=1)
        return mean_z0, std_z0.abs()

    def run_ode_conv_gru(self, input_tensor, mask, time_steps, run_backwards=True, tracker=None, steps=None):
        """(last yi, latent_ys (b, t, c, h, w)) from batch-first frames (upstream :146-199); slot k of latent_ys is the state after the
        k-th visited frame."""
        if self.fused:
            _, _, latent = self._encode(input_tensor, time_steps, mask, run_backwards, True, steps)
            return latent[:, -1], latent
        b, t, c, h, w = input_tensor.size()
        times = [float(v) for v in hip_ops.host_times(time_steps)]
        net = self.z0_diffeq_solver.ode_func.gradient_net
        prev = torch.zeros((b, c, h, w), dtype=input_tensor.dtype, device=input_tensor.device)
        prev_t, t_i = times[-1] + 0.01, times[-1]
        latent_ys = []
        order = range(t - 1, -1, -1) if run_backwards else range(t)
        for i in order:
            yi_ode = prev + net(prev) * (t_i - prev_t)
            m = None if mask is None else mask[:, i].to(device=prev.device, dtype=prev.dtype)
            prev = self.cell_list[0].compose(input_tensor[:, i], yi_ode, m)
            prev_t, t_i = times[i], times[i - 1]
            latent_ys.append(prev)
        return prev, torch.stack(latent_ys, 1)


class Encoder(_flow.Encoder):
    """Upstream base_conv_gru.py:263-344 (`cnn_encoder.*`): the fused BatchNorm + ReLU passes of models/VidODE.py."""

    def __init__(self, input_dim=3, ch=64, n_downs=2, opt=None, device=None, fused=True):
        super().__init__(input_dim=input_dim, ch=ch, n_downs=n_downs, device=device)
        self.opt, self.device, self.resize, self.fused = opt, device, 2 ** n_downs, fused


class Decoder(_flow.Decoder):
    """Upstream base_conv_gru.py:347-377 (`model.*`): the fused passes of models/VidODE.py under upstream's attribute name."""
    SEQ_NAME = "model"

    def __init__(self, input_dim=256, output_dim=3, n_ups=2, opt=None, fused=True):
        super().__init__(input_dim=input_dim, output_dim=output_dim, n_ups=n_ups, device=None)
        self.fused = fused


class VidODE(nn.Module):
    def __init__(self, opt, device, fused=True):
        super().__init__()
        self.opt, self.device, self.fused = opt, device, fused
        if getattr(opt, "slot_attention", False) is True:
            raise NotImplementedError("VidODE: slot attention is not implemented (upstream leaves it at `pass`)")
        if opt.input_size != 16 * 2 ** opt.n_downs:
            raise ValueError(f"VidODE: input_size must be 16 * 2**n_downs = {16 * 2 ** opt.n_downs} (the HIP path works on 16 x 16 latents), "
                             f"got {opt.input_size}")
        self.build_model()
        self._grid = None

    def build_model(self):
        opt, dev = self.opt, self.device
        resize = 2 ** opt.n_downs
        base_dim = opt.init_dim * resize
        input_size = (opt.input_size // resize, opt.input_size // resize)
        nru, nru2 = getattr(opt, "nru", False), getattr(opt, "nru2", False)
        self.encoder = Encoder(input_dim=opt.input_dim, ch=opt.init_dim, n_downs=opt.n_downs, opt=opt, device=dev, fused=self.fused).to(dev)
        net_e, net_d = self.set_ode_func_netED()
        rec_ode_func = ODEFunc(opt=opt, input_dim=base_dim, latent_dim=base_dim, ode_func_net=net_e, device=dev).to(dev)
        z0_diffeq_solver = DiffeqSolver(base_dim, ode_func=rec_ode_func, method="euler", latents=base_dim, odeint_rtol=1e-3, odeint_atol=1e-4,
                                        device=dev, nru=nru, nru2=nru2, fused=self.fused)
        self.encoder_z0 = Encoder_z0_ODE_ConvGRU(input_size=input_size, input_dim=base_dim, hidden_dim=base_dim, kernel_size=(3, 3),
                                                 num_layers=opt.n_layers, dtype=torch.FloatTensor, batch_first=True, bias=True,
                                                 return_all_layers=True, z0_diffeq_solver=z0_diffeq_solver,
                                                 run_backwards=opt.run_backwards, opt=opt, fused=self.fused).to(dev)
        gen_ode_func = ODEFunc(opt=opt, input_dim=base_dim, latent_dim=base_dim, ode_func_net=net_d, device=dev).to(dev)
        self.diffeq_solver = DiffeqSolver(base_dim, gen_ode_func, opt.dec_diff, base_dim, odeint_rtol=1e-3, odeint_atol=1e-4, device=dev,
                                          nru=nru, nru2=nru2, fused=self.fused)
        self.decoder = Decoder(input_dim=base_dim * 2, output_dim=opt.input_dim + 3, n_ups=opt.n_downs, opt=opt, fused=self.fused).to(dev)

    def set_ode_func_netED(self):
        base_dim = self.opt.init_dim * 2 ** self.opt.n_downs
        return tuple(create_convnet(n_inputs=base_dim, n_outputs=base_dim, n_layers=self.opt.n_layers, n_units=base_dim // 2).to(self.device)
                     for _ in range(2))

    def _grids(self, h, w, device):
        key = (h, w, str(device))
        if self._grid is None or self._grid[0] != key:
            self._grid = (key, torch.linspace(-1.0, 1.0, w).float().to(device), torch.linspace(-1.0, 1.0, h).float().to(device))
        return self._grid[1], self._grid[2]

    def _init_image(self, observed):
        """The skip image, the warp start and the loss's init image: the last observed frame when extrapolating, the FIRST when
        interpolating (upstream :193, :317, :435-438)."""
        return observed[:, -1, ...] if self.opt.extrap else observed[:, 0, ...]

    @staticmethod
    def _selected(mask, n_frames):
        """(frames selected per row, the mask or None when it selects every frame) without reading a device tensor where that can be
        avoided: the count comes from the mask where the loader left it (the host), and a mask that selects all `n_frames` needs no
        indexing at all.  A mask that already lives on the device costs one host read, as upstream's `int(mask[0].sum())` does."""
        if mask is None:
            return n_frames, None
        n = int(mask[0].sum())
        return n, (None if n == n_frames == mask.size(1) else mask)

    def _warp(self, pred_outputs, start):
        """(pred_x, warped, masks): `warp_composite`, or with fused=False upstream's chain of `grid_sample` calls (:388-412, :321)."""
        b, _, _, h, w = pred_outputs.shape
        if self.fused:
            gx, gy = self._grids(h, w, pred_outputs.device)
            return warp_composite(pred_outputs, start, gx, gy)
        nc = self.opt.input_dim
        masks = torch.sigmoid(pred_outputs[:, :, 2 + nc:, ...])
        grid_x = torch.linspace(-1.0, 1.0, w).view(1, 1, w, 1).expand(b, h, -1, -1)
        grid_y = torch.linspace(-1.0, 1.0, h).view(1, h, 1, 1).expand(b, -1, w, -1)
        grid = torch.cat([grid_x, grid_y], 3).float().to(pred_outputs.device)
        last, warped = start, []
        for t in range(pred_outputs.size(1)):
            fl = pred_outputs[:, t, :2, ...]
            fl = torch.cat([fl[:, 0:1] / ((w - 1.0) / 2.0), fl[:, 1:2] / ((h - 1.0) / 2.0)], dim=1).permute(0, 2, 3, 1)
            last = nn.functional.grid_sample(last, grid + fl, mode="bilinear", padding_mode="border", align_corners=False)
            warped.append(last.unsqueeze(1))
        warped = torch.cat(warped, dim=1)
        return masks * warped + (1 - masks) * pred_outputs[:, :, 2:2 + nc, ...], warped, masks

    def get_reconstruction(self, time_steps_to_predict, truth, truth_time_steps, mask=None, out_mask=None):
        dev = self.device
        truth = truth.to(dev)
        n_pred, out_sel = self._selected(out_mask, len(time_steps_to_predict))
        b, t, c, h, w = truth.shape   # (the mask stays where the loader left it: on the host it also tells which encoder steps to skip)
        resize = 2 ** self.opt.n_downs
        start = self._init_image(truth)
        skip_conn_embed = self.encoder(start).view(b, -1, h // resize, w // resize)
        e_truth = self.encoder(truth.reshape(b * t, c, h, w)).view(b, t, -1, h // resize, w // resize)
        first_point_mu, _ = self.encoder_z0(input_tensor=e_truth, time_steps=truth_time_steps, mask=mask)
        sol_y = self.diffeq_solver(first_point_mu, time_steps_to_predict).contiguous()
        if out_sel is not None and out_sel.size(1) == sol_y.size(1):
            sol_y = sol_y[out_sel.to(dev).squeeze(-1).bool()].view(b, n_pred, *sol_y.shape[2:])
        pred_outputs = torch.cat(self.get_flowmaps(sol_out=sol_y[:, :n_pred], first_prev_embed=skip_conn_embed, mask=None), dim=1)
        pred_outputs = pred_outputs.float()   # under autocast the decoder's library convs hand over bf16; the warp and the loss take fp32
        pred_x, warped, masks = self._warp(pred_outputs, start)
        nc = self.opt.input_dim
        extra_info = {"optical_flow": pred_outputs[:, :, :2, ...], "warped_pred_x": warped,
                      "pred_intermediates": pred_outputs[:, :, 2:2 + nc, ...], "pred_masks": masks}
        return pred_x.view(b, -1, c, h, w), extra_info

    def get_flowmaps(self, sol_out, first_prev_embed, mask):
        """decoder(cat(z_t, z_{t-1})) per predicted frame (upstream :361-386); one decoder call per frame, as BatchNorm's batch
        statistics are per call.  mask None: every frame of sol_out."""
        b, _, c, h, w = sol_out.size()
        n, sel = self._selected(mask, sol_out.size(1))
        if sel is not None and sel.size(1) == sol_out.size(1):
            sol_out = sol_out[sel.to(sol_out.device).squeeze(-1).bool()].view(b, n, c, h, w)
        flows, prev = [], first_prev_embed
        for t in range(n):
            flows.append(self.decoder(torch.cat([sol_out[:, t, ...], prev], dim=1)).unsqueeze(1))
            prev = sol_out[:, t, ...]
        return flows

    def get_mse(self, truth, pred_x, mask=None):
        b, _, c, h, w = truth.size()
        n, sel = self._selected(mask, truth.size(1))
        picked = truth if sel is None else truth[sel.to(truth.device).squeeze(-1).bool()].view(b, n, c, h, w)
        return torch.sum(torch.abs(pred_x - picked[:, :n])) / (b * n * c * h * w)

    def get_diff(self, data, mask=None):
        d = data[:, 1:, ...] - data[:, :-1, ...]
        b, _, c, h, w = d.size()
        n, sel = self._selected(mask, d.size(1))
        return d[:, :n] if sel is None else d[sel.to(d.device).squeeze(-1).bool()].view(b, n, c, h, w)

    def _loss(self, pred_x, inter, truth, init, out_mask):
        if not self.fused:   # upstream :431-443 in torch ops
            data = torch.cat([init.unsqueeze(1), truth], dim=1)
            return torch.mean(self.get_mse(truth=truth, pred_x=pred_x, mask=out_mask) +
                              self.get_mse(truth=self.get_diff(data=data, mask=out_mask), pred_x=inter, mask=None))
        if out_mask is None:
            out_mask = torch.ones(truth.shape[:2], dtype=torch.float32, device=truth.device)
        return vidode_l1_loss(pred_x, inter, truth, init, out_mask.to(truth.device))[0]

    def compute_all_losses(self, batch_dict):
        """{'loss', 'pred_y'} (upstream :414-449): L1 of the prediction + L1 of the intermediates against the frame differences, the
        differences starting from the mode's init image, through `vidode_l1_loss`."""
        dev = self.device
        observed, target = batch_dict["observed_data"].to(dev), batch_dict["data_to_predict"].to(dev)
        out_mask = batch_dict["mask_predicted_data"]   # left where the loader put it: its frame count is read there
        pred_x, extra_info = self.get_reconstruction(time_steps_to_predict=batch_dict["tp_to_predict"], truth=observed,
                                                     truth_time_steps=batch_dict["observed_tp"], mask=batch_dict["observed_mask"],
                                                     out_mask=out_mask)
        loss = self._loss(pred_x, extra_info["pred_intermediates"], target, self._init_image(observed), out_mask)
        return {"loss": loss, "pred_y": pred_x}

    def get_prediction(self, input_frames, batch_dict=None):
        """Adaptor for `train_batch`, `train_batch_gan`, `test_batch` and `evaluate`: the reconstruction from `input_frames` (the observed
        frames in the space the caller works in) with the times and masks of `batch_dict`."""
        pred_x, extra_info = self.get_reconstruction(time_steps_to_predict=batch_dict["tp_to_predict"], truth=input_frames,
                                                     truth_time_steps=batch_dict["observed_tp"], mask=batch_dict.get("observed_mask"),
                                                     out_mask=batch_dict.get("mask_predicted_data"))
        self.extra_info, self.batch_dict, self._observed = extra_info, batch_dict, input_frames
        return pred_x

    def get_loss(self, pred_frames, truth, loss='MSE'):
        """The loss of `compute_all_losses` for the prediction `get_prediction` returned last, against `truth` in the same space."""
        out_mask = self.batch_dict.get("mask_predicted_data")
        return self._loss(pred_frames, self.extra_info["pred_intermediates"], truth, self._init_image(self._observed), out_mask)
