"""CPU restatement of VidODE's training forward and loss (test infrastructure only), in the dtype asked for: the BatchNorm encoder and
the flow decoder from torch.nn.functional on the state_dict entries, `oracle.reference_modules.ode_convgru_encode` (tests/_mask_ref.py
when an observation mask is given), `oracle.torchdiffeq_ref.odeint`, `oracle.vidode_ref.warp_composite` and the L1 pair of
tests/_loss_ref.py, wired as the reference's models/VidODE.py wires them (forward :96-140, get_flowmaps :143-158, get_loss :211-226)
with its two layout slips repaired unless `as_written`.  torch.autograd gives the gradients.  It imports neither the package's model nor
its autograd Functions; tests/test_vidode_ref_cpu.py pins it to tests/golden/vidode.npz, which the reference's own model produced."""
import torch
import torch.nn.functional as F

import _loss_ref
import _mask_ref
from oracle import reference_modules as rm
from oracle import torchdiffeq_ref, vidode_ref

BN_MOMENTUM, BN_EPS = 0.1, 1e-5          # nn.BatchNorm2d's defaults, which the reference's Encoder / Decoder keep
SOLVER_RTOL, SOLVER_ATOL = 1e-4, 1e-5    # DiffEqSolver's defaults (modules/DiffEqSolver.py:13), which VidODE keeps
# state_dict prefixes under which load_state_dict reaches the two shared ODE functions a second time; the later entry is the one that stays
ALIASES = {"encoder_z0.ode_func.": "ode_encoder_func.", "diffeq_solver.ode_func.": "ode_decoder_func."}


def split_state_dict(state_dict):
    """(parameters, buffers) of a VidODE state_dict as `load_state_dict` leaves them in the module: BatchNorm's running statistics and
    counters are the buffers; the ODE functions are registered twice, the value loaded last (the nested name) stays, under the name
    `named_parameters()` reports (the top-level one)."""
    params, buffers = {}, {}
    for k, v in state_dict.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            buffers[k] = v.detach().clone()
            continue
        for nested, top in ALIASES.items():
            if k.startswith(nested):
                k = top + k[len(nested):]
        params[k] = v.detach().clone()
    return params, buffers


class _L1Pair(torch.autograd.Function):
    """tests/_loss_ref.py::vidode_l1 (NumPy float64) as a node of the graph: its loss forward, its two gradients backward."""

    @staticmethod
    def forward(ctx, pred, inter, truth, init, mask):
        r = _loss_ref.vidode_l1(pred.detach().numpy(), inter.detach().numpy(), truth.numpy(), init.numpy(), mask.numpy())
        ctx.grads = (torch.from_numpy(r["grad_pred"]).to(pred.dtype), torch.from_numpy(r["grad_inter"]).to(inter.dtype))
        return torch.tensor(r["loss"], dtype=pred.dtype)

    @staticmethod
    def backward(ctx, g):
        return ctx.grads[0] * g, ctx.grads[1] * g, None, None, None


class _BatchNorms:
    """F.batch_norm on copies of the buffers: running statistics move in train() as nn.BatchNorm2d moves them, the counter with them."""

    def __init__(self, params, buffers, training, dtype):
        self.p, self.training = params, training
        self.buffers = {k: (v.clone().to(dtype) if torch.is_floating_point(v) else v.clone()) for k, v in buffers.items()}

    def __call__(self, x, prefix):
        if self.training:
            self.buffers[prefix + "num_batches_tracked"] += 1
        return F.batch_norm(x, self.buffers[prefix + "running_mean"], self.buffers[prefix + "running_var"], self.p[prefix + "weight"],
                            self.p[prefix + "bias"], self.training, BN_MOMENTUM, BN_EPS)


def _encoder(x, p, bn, n_downs):
    """[Conv, BatchNorm, ReLU] x (1 + n_downs): 3x3 stride 1, then 4x4 stride 2 (reference :12-26)."""
    for k in range(1 + n_downs):
        pre = f"conv_encoder.cnn_encoder.{3 * k}."
        x = F.conv2d(x, p[pre + "weight"], p[pre + "bias"], stride=1 if k == 0 else 2, padding=1)
        x = torch.relu(bn(x, f"conv_encoder.cnn_encoder.{3 * k + 1}."))
    return x


def _decoder(x, p, bn, n_ups):
    """[Upsample x2, Conv3x3, BatchNorm, ReLU] x n_ups + Conv3x3 (reference :28-45)."""
    for k in range(n_ups):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        pre = f"conv_decoder.cnn_decoder.{4 * k + 1}."
        x = F.conv2d(x, p[pre + "weight"], p[pre + "bias"], padding=1)
        x = torch.relu(bn(x, f"conv_decoder.cnn_decoder.{4 * k + 2}."))
    pre = f"conv_decoder.cnn_decoder.{4 * n_ups}."
    return F.conv2d(x, p[pre + "weight"], p[pre + "bias"], padding=1)


def _under(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def forward(state_dict, buffers, batch_dict, opt, training, as_written=False, dtype=torch.float64, solver_options=None):
    """state_dict: the parameters by their `named_parameters()` names (split_state_dict); buffers: BatchNorm's; batch_dict: the loader's
    keys on the CPU -- observed_data (B,Tin,c,H,W), observed_tp, tp_to_predict, optionally observed_mask, mask_predicted_data and, for
    the loss, data_to_predict.  Returns a dict: loss (None without data_to_predict), pred_x, optical_flow, pred_intermediates, pred_masks,
    warped_pred_x, z0, sol (T,B,C,h,w), buffers (after the forward), params (the leaves: .grad after loss.backward()), solver_stats."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state_dict.items()}
    bn = _BatchNorms(p, buffers, training, dtype)
    inputs = batch_dict["observed_data"].to(dtype)
    t_obs, t_pred = batch_dict["observed_tp"].double(), batch_dict["tp_to_predict"].double()
    mask, out_mask = batch_dict.get("observed_mask"), batch_dict.get("mask_predicted_data")
    b, t, c, h, w = inputs.shape
    n_downs = opt.n_downs

    enc = _encoder(inputs.reshape(b * t, c, h, w), p, bn, n_downs)
    enc = enc.view(b, t, *enc.shape[1:])
    if not as_written:
        enc = enc.permute(1, 0, 2, 3, 4)                       # time first into the cell; as written it gets the batch-first tensor
    f_enc = rm.ode_func(*rm.split_convnet_state(p, "ode_encoder_func.gradient_net."))
    cell, head = _under(p, "encoder_z0.cgru_cell."), _under(p, "encoder_z0.transform_z0.")
    if mask is not None and not as_written:
        z0, _, _ = _mask_ref.encode(enc, t_obs, f_enc, cell, head, mask.reshape(b, t).float())
    else:
        z0, _, _ = rm.ode_convgru_encode(enc, t_obs, f_enc, cell, head)

    stats = {}
    f_dec = rm.ode_func(*rm.split_convnet_state(p, "ode_decoder_func.gradient_net."))
    sol = torchdiffeq_ref.odeint(f_dec, z0, t_pred, rtol=SOLVER_RTOL, atol=SOLVER_ATOL, method=opt.decode_diff_method,
                                 options=solver_options, stats=stats)
    if as_written:
        sol_b = sol.contiguous().view(b, len(t_pred), -1, h // 2 ** n_downs, w // 2 ** n_downs)   # the reference's reinterpretation
    else:
        sol_b = sol.permute(1, 0, 2, 3, 4)

    skip = _encoder(inputs[:, -1], p, bn, n_downs)
    n = sol_b.shape[1]
    if out_mask is not None:
        n = int(out_mask[0].sum())
        if out_mask.shape[1] == sol_b.shape[1]:
            sol_b = sol_b[out_mask.reshape(b, -1).bool()].view(b, n, *sol_b.shape[2:])
    flows, prev = [], skip
    for i in range(n):                                          # one decoder call per frame: train() statistics are per frame
        flows.append(_decoder(torch.cat([sol_b[:, i], prev], dim=1), p, bn, n_downs).unsqueeze(1))
        prev = sol_b[:, i]
    pred_outputs = torch.cat(flows, dim=1)
    pred_x, warped, masks = vidode_ref.warp_composite(pred_outputs, inputs[:, -1])
    inter = pred_outputs[:, :, 2:2 + c]

    loss = None
    if "data_to_predict" in batch_dict:
        loss_mask = out_mask if out_mask is not None else torch.ones(b, batch_dict["data_to_predict"].shape[1], 1)
        loss = _L1Pair.apply(pred_x, inter, batch_dict["data_to_predict"].float(), batch_dict["observed_data"][:, -1].float(), loss_mask)
    return {"loss": loss, "pred_x": pred_x, "optical_flow": pred_outputs[:, :, :2], "pred_intermediates": inter, "pred_masks": masks,
            "warped_pred_x": warped, "z0": z0, "sol": sol, "buffers": bn.buffers, "params": p, "solver_stats": stats}


def kink_free(params):
    """Both ODE functions and the hidden layer of transform_z0 away from their ReLU kinks, in place, as
    tests/test_hip_train_end_to_end.py::_model does it: hidden weights x 0.15 with biases of alternating +-2.5, the last layer x 4,
    transform_z0's first convolution x 0.3 with the same biases."""
    def alt(n):
        return torch.where(torch.arange(n) % 2 == 0, 2.5, -2.5)
    with torch.no_grad():
        for f in ("ode_encoder_func.gradient_net.", "ode_decoder_func.gradient_net."):
            idx = sorted(int(k[len(f):].split(".")[0]) for k in params if k.startswith(f) and k.endswith(".weight"))
            for i in idx[:-1]:
                params[f"{f}{i}.weight"].mul_(0.15)
                params[f"{f}{i}.bias"].copy_(alt(params[f"{f}{i}.bias"].numel()))
            params[f"{f}{idx[-1]}.weight"].mul_(4.0)
        params["encoder_z0.transform_z0.0.weight"].mul_(0.3)
        params["encoder_z0.transform_z0.0.bias"].copy_(alt(params["encoder_z0.transform_z0.0.bias"].numel()))
    return params
