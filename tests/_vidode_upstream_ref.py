"""A dtype-generic restatement of upstream Vid-ODE's model (reference Vid-ODE/models/conv_odegru.py, base_conv_gru.py, ode_func.py,
layers.py), written from a reading of what it computes: functions of a state_dict with upstream's keys, so float64 runs are a
`.double()` away and torch.autograd gives the gradients.  The yardstick of tests/test_hip_vidode_upstream.py and, in float32,
checked against upstream's own classes through tests/golden/vidode_upstream.npz (tests/test_vidode_upstream_cpu.py).  It imports
neither the package's model nor its autograd Functions.

    dynamics   conv3x3, (tanh, conv3x3) x n, tanh, conv3x3 -- every Conv2d of `gradient_net.*` in order, tanh between them, none behind
    cell       (r, u) = sigmoid(conv_gates(cat(x, h))), RESET first;  c = tanh(conv_can(cat(x, r h)));  h' = (1-u) h + u c;
               with a mask m per sample: m h' + (1-m) h
    encoder    state 0; before visiting frame i an Euler step  h_ode = h + f(h) dt,  dt = t[-1] - (t[-1] + 0.01) first, then
               t[j-1] - t[j] after visiting frame j (Python indexing: j = 0 wraps);  frames visited T-1 .. 0 (run_backwards) or 0 .. T-1;
               head conv1x1, relu, conv1x1, split into mean and |std|.  Times are float64 Python numbers.
    model      BatchNorm conv encoder / flow decoder with batch statistics (train()), explicit Euler on the predicted times, one decoder
               call per frame on cat(z_t, z_{t-1}) with z_{-1} the encoding of the init image, warp chain + compositing from the init
               image, L1 of the prediction + L1 of the intermediates against the frame differences that start at the init image.  The
               init image is the LAST observed frame when extrapolating and the FIRST otherwise."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def under(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def dynamics(sd, y):
    """`sd`: the entries under `...gradient_net.`"""
    idx = sorted(int(k.split(".")[0]) for k in sd if k.endswith(".weight"))
    for n, i in enumerate(idx):
        y = F.conv2d(y, sd[f"{i}.weight"], sd[f"{i}.bias"], padding=1)
        if n + 1 < len(idx):
            y = torch.tanh(y)
    return y


def cell(sd, x, h, mask=None):
    """`sd`: conv_gates.{weight,bias}, conv_can.{weight,bias}; mask (B,) or None."""
    hid = h.shape[1]
    pad = sd["conv_gates.weight"].shape[-1] // 2
    gates = torch.sigmoid(F.conv2d(torch.cat([x, h], 1), sd["conv_gates.weight"], sd["conv_gates.bias"], padding=pad))
    r, u = gates[:, :hid], gates[:, hid:]
    c = torch.tanh(F.conv2d(torch.cat([x, r * h], 1), sd["conv_can.weight"], sd["conv_can.bias"], padding=pad))
    h_next = (1 - u) * h + u * c
    if mask is None:
        return h_next
    m = mask.reshape(-1, 1, 1, 1).to(h.dtype)
    return m * h_next + (1 - m) * h


def encoder(sd, frames, times, mask=None, run_backwards=True):
    """`sd`: the entries under `encoder_z0.`; frames (B,T,C,h,w) batch-first; mask (B,T) or None -> (mean, std, latent_ys (B,T,C,h,w))."""
    b, t = frames.shape[:2]
    times = [float(v) for v in times]
    f, c0, head = under(sd, "z0_diffeq_solver.ode_func.gradient_net."), under(sd, "cell_list.0."), under(sd, "transform_z0.")
    h = frames.new_zeros((b,) + tuple(frames.shape[2:]))
    prev_t, t_i = times[-1] + 0.01, times[-1]
    latent = []
    for i in (range(t - 1, -1, -1) if run_backwards else range(t)):
        h_ode = h + dynamics(f, h) * (t_i - prev_t)
        h = cell(c0, frames[:, i], h_ode, None if mask is None else mask[:, i])
        prev_t, t_i = times[i], times[i - 1]
        latent.append(h)
    out = F.conv2d(torch.relu(F.conv2d(h, head["0.weight"], head["0.bias"])), head["2.weight"], head["2.bias"])
    z = out.shape[1] // 2
    return out[:, :z], out[:, z:].abs(), torch.stack(latent, 1)


def _bn_relu(x, sd, prefix):
    return torch.relu(F.batch_norm(x, None, None, sd[prefix + "weight"], sd[prefix + "bias"], True, 0.1, BN_EPS))


def conv_encoder(sd, x, n_downs):
    for k in range(1 + n_downs):
        pre = f"encoder.cnn_encoder.{3 * k}."
        x = F.conv2d(x, sd[pre + "weight"], sd[pre + "bias"], stride=1 if k == 0 else 2, padding=1)
        x = _bn_relu(x, sd, f"encoder.cnn_encoder.{3 * k + 1}.")
    return x


def flow_decoder(sd, x, n_ups):
    for k in range(n_ups):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        pre = f"decoder.model.{4 * k + 1}."
        x = _bn_relu(F.conv2d(x, sd[pre + "weight"], sd[pre + "bias"], padding=1), sd, f"decoder.model.{4 * k + 2}.")
    pre = f"decoder.model.{4 * n_ups}."
    return F.conv2d(x, sd[pre + "weight"], sd[pre + "bias"], padding=1)


def losses(sd, batch, n_downs, extrap, run_backwards=True):
    """compute_all_losses in train() mode with dec_diff = 'euler' and every predicted frame selected: {'loss', 'pred_y'}.  `sd`: the
    parameters in the dtype wanted (leaves with requires_grad for gradients); batch: observed_data (B,T,c,H,W), data_to_predict,
    observed_tp, tp_to_predict, observed_mask (B,T) or (B,T,1)."""
    obs, target = batch["observed_data"], batch["data_to_predict"]
    dtype = sd["encoder.cnn_encoder.0.weight"].dtype
    obs, target = obs.to(dtype), target.to(dtype)
    b, t, c, h, w = obs.shape
    init = obs[:, -1] if extrap else obs[:, 0]
    skip = conv_encoder(sd, init, n_downs)
    e = conv_encoder(sd, obs.reshape(b * t, c, h, w), n_downs)
    e = e.view(b, t, *e.shape[1:])
    mask = batch.get("observed_mask")
    z, _, _ = encoder(under(sd, "encoder_z0."), e, batch["observed_tp"], None if mask is None else mask.reshape(b, t), run_backwards)
    f = under(sd, "diffeq_solver.ode_func.gradient_net.")
    tp = [float(v) for v in batch["tp_to_predict"]]
    sol = [z]
    for k in range(1, len(tp)):
        sol.append(sol[-1] + dynamics(f, sol[-1]) * (tp[k] - tp[k - 1]))
    flows, prev = [], skip
    for zt in sol:
        flows.append(flow_decoder(sd, torch.cat([zt, prev], 1), n_downs).unsqueeze(1))
        prev = zt
    pred_outputs = torch.cat(flows, 1)
    inter, masks = pred_outputs[:, :, 2:2 + c], torch.sigmoid(pred_outputs[:, :, 2 + c:])
    gx = torch.linspace(-1.0, 1.0, w, dtype=torch.float32, device=obs.device).view(1, 1, w, 1).expand(b, h, -1, -1)
    gy = torch.linspace(-1.0, 1.0, h, dtype=torch.float32, device=obs.device).view(1, h, 1, 1).expand(b, -1, w, -1)
    grid = torch.cat([gx, gy], 3).to(dtype)       # upstream's float32 linspace, then the state's dtype
    last, warped = init, []
    for i in range(pred_outputs.shape[1]):        # each frame warps the previous warped frame
        fl = pred_outputs[:, i, :2]
        fl = torch.cat([fl[:, 0:1] / ((w - 1.0) / 2.0), fl[:, 1:2] / ((h - 1.0) / 2.0)], 1).permute(0, 2, 3, 1)
        last = F.grid_sample(last, grid + fl, mode="bilinear", padding_mode="border", align_corners=False)
        warped.append(last.unsqueeze(1))
    warped = torch.cat(warped, 1)
    pred_x = masks * warped + (1 - masks) * inter
    data = torch.cat([init.unsqueeze(1), target], 1)
    diff = data[:, 1:] - data[:, :-1]
    loss = (pred_x - target).abs().mean() + (inter - diff).abs().mean()
    return {"loss": loss, "pred_y": pred_x}


# ---- the cases of tests/golden/vidode_upstream.npz: procedural inputs and weights, rebuilt by the tests (conftest.procedural_tensor) ----
CELL_MASK = [1.0, 0.0, 0.5]
ENC_TIMES = [0.0, 0.13, 0.41]                     # irregular
ENC_MASK = [[1.0, 0.0, 0.5], [0.5, 1.0, 0.0]]     # (B, T) of the fixture's encoder case
MODEL_OBS_TP = [0.0, 0.1, 0.25]
MODEL_PRED_TP = [0.3, 0.42, 0.5]
FLOW_GAIN = 10.0                                  # the flow decoder's last conv is scaled so that flows reach several pixels


def model_opt(extrap):
    import types
    return types.SimpleNamespace(init_dim=32, n_downs=2, n_layers=2, input_size=64, input_dim=1, extrap=extrap, run_backwards=True,
                                 dec_diff="euler", slot_attention=False, nru=False, nru2=False, dim=64, num_slots=1, pos=2,
                                 irregular=False, unequal=False, output_sequence=3, sample_size=6, lr=1e-3)


def cell_case(ch, batch=3):
    from conftest import procedural_tensor
    shapes = {"conv_gates.weight": (2 * ch, 2 * ch, 3, 3), "conv_gates.bias": (2 * ch,), "conv_can.weight": (ch, 2 * ch, 3, 3),
              "conv_can.bias": (ch,)}
    bound = 1.0 / (2 * ch * 9) ** 0.5
    sd = {k: procedural_tensor(s, 4100 + n + ch, -bound, bound) * (3.0 if k.endswith("weight") else 1.0) for n, (k, s) in enumerate(shapes.items())}
    x = procedural_tensor((batch, ch, 16, 16), 4200 + ch, -1.0, 1.0)
    h = procedural_tensor((batch, ch, 16, 16), 4300 + ch, -1.0, 1.0)
    return sd, x, h


def encoder_shapes(ch, n_units, n_hidden):
    shapes = {}
    widths = [ch] + [n_units] * (n_hidden + 1) + [ch]
    for n in range(len(widths) - 1):
        shapes[f"z0_diffeq_solver.ode_func.gradient_net.{2 * n}.weight"] = (widths[n + 1], widths[n], 3, 3)
        shapes[f"z0_diffeq_solver.ode_func.gradient_net.{2 * n}.bias"] = (widths[n + 1],)
    shapes.update({"cell_list.0.conv_gates.weight": (2 * ch, 2 * ch, 3, 3), "cell_list.0.conv_gates.bias": (2 * ch,),
                   "cell_list.0.conv_can.weight": (ch, 2 * ch, 3, 3), "cell_list.0.conv_can.bias": (ch,),
                   "transform_z0.0.weight": (ch, ch, 1, 1), "transform_z0.0.bias": (ch,),
                   "transform_z0.2.weight": (2 * ch, ch, 1, 1), "transform_z0.2.bias": (2 * ch,)})
    return shapes


def encoder_case(ch, batch, n_units=None, n_hidden=1, seed=4400):
    """(state_dict under `encoder_z0.` of an encoder with ONE cell, frames (B,3,ch,16,16))."""
    from conftest import procedural_tensor
    sd = {}
    for n, (k, s) in enumerate(encoder_shapes(ch, n_units or ch, n_hidden).items()):
        fan = 1
        for d in s[1:]:
            fan *= d
        bound = 1.0 / fan ** 0.5 if len(s) > 1 else 0.05
        sd[k] = procedural_tensor(s, seed + n + ch, -bound, bound) * (2.0 if len(s) > 1 else 1.0)
    frames = procedural_tensor((batch, 3, ch, 16, 16), seed + 90 + ch, -1.0, 1.0)
    return sd, frames


def model_state_dict(reference_sd, seed=41):
    """Procedural weights that keep every ReLU pre-activation of the model away from its kink, so that two correct float32 evaluations
    cannot disagree about a mask element (the device the other gradient suites use, tests/_vidode_ref.py::kink_free): BatchNorm weights
    in +-[0.14, 0.26] with biases of alternating +-2.5 -- a normalised activation would have to lie 9.6 standard deviations out to cross
    zero --, and transform_z0's first convolution x 0.3 with the same biases.  Half of those channels are switched off, half pass
    linearly."""
    from conftest import procedural_state_dict
    sd = procedural_state_dict(reference_sd, seed)
    for k in ("decoder.model.8.weight", "decoder.model.8.bias"):
        sd[k] = sd[k] * FLOW_GAIN
    for k in list(sd):
        if k.endswith("running_var") :
            pre = k[:-len("running_var")]
            n = sd[pre + "weight"].numel()
            sd[pre + "weight"] = sd[pre + "weight"] * 0.2
            sd[pre + "bias"] = torch.where(torch.arange(n) % 2 == 0, 2.5, -2.5)
    n = sd["encoder_z0.transform_z0.0.bias"].numel()
    sd["encoder_z0.transform_z0.0.weight"] = sd["encoder_z0.transform_z0.0.weight"] * 0.3
    sd["encoder_z0.transform_z0.0.bias"] = torch.where(torch.arange(n) % 2 == 0, 2.5, -2.5)
    return sd


TARGET_STEP = -20.0   # frame t of data_to_predict lies in [TARGET_STEP (t + 1), TARGET_STEP (t + 1) + 1)


def model_batch(batch=2):
    """The targets step down by 20 per frame, far below anything the model predicts here (|pred|, |intermediates| < 10): both L1
    terms of the loss then keep one sign in every element, so no |.| kink lies within rounding of an operand either (what the L1
    kernels do at the kink is tests/test_hip_frame_loss.py's subject)."""
    from conftest import procedural_tensor
    steps = TARGET_STEP * torch.arange(1, 4, dtype=torch.float32).view(1, 3, 1, 1, 1)
    return {"observed_data": procedural_tensor((batch, 3, 1, 64, 64), 4501, 0.0, 1.0),
            "data_to_predict": procedural_tensor((batch, 3, 1, 64, 64), 4502, 0.0, 1.0) + steps,
            "observed_tp": torch.tensor(MODEL_OBS_TP, dtype=torch.float64), "tp_to_predict": torch.tensor(MODEL_PRED_TP, dtype=torch.float64),
            "observed_mask": torch.ones(batch, 3, 1), "mask_predicted_data": torch.ones(batch, 3, 1)}
