"""CPU yardstick of the ConvGRU sequence / model tests: oracle.reference_modules.convgru_cell looped over the sequence, in float64
or float32, and the bound the issue's construction gives (4 x the float32 restatement's own distance from the float64 one, with a
floor)."""
import torch
import torch.nn.functional as F

from conftest import procedural_state_dict, rel_l2
from oracle import reference_modules as rm


def cell_state_dict(input_dim, hidden, seed, ks=5):
    shapes = {"conv_gates.0.weight": (2 * hidden, input_dim + hidden, ks, ks), "conv_gates.0.bias": (2 * hidden,),
              "conv_gates.1.weight": (2 * hidden,), "conv_gates.1.bias": (2 * hidden,),
              "conv_can.0.weight": (hidden, input_dim + hidden, ks, ks), "conv_can.0.bias": (hidden,),
              "conv_can.1.weight": (hidden,), "conv_can.1.bias": (hidden,)}
    return procedural_state_dict({k: torch.zeros(s) for k, s in shapes.items()}, seed)


def rollout(p, x_seq, h0, n_steps, input_dim):
    """(T,B,H,16,16): the restatement fed explicit zeros where the sequence path has no operand at all."""
    any_t = x_seq if x_seq is not None else h0
    hidden = p["conv_can.0.weight"].shape[0]
    b = x_seq.shape[1] if x_seq is not None else h0.shape[0]
    h = h0 if h0 is not None else torch.zeros(b, hidden, 16, 16, dtype=any_t.dtype)
    outs = []
    for t in range(n_steps):
        x = x_seq[t] if x_seq is not None else torch.zeros(b, input_dim, 16, 16, dtype=any_t.dtype)
        h = rm.convgru_cell(x, h, p)
        outs.append(h)
    return torch.stack(outs)


def cast(p, dtype):
    return {k: v.detach().to(dtype) for k, v in p.items()}


def bound(ref32, ref64, floor):
    """(bound, d32): the HIP result may sit 4 x as far from the float64 result as the float32 restatement does, never asked below `floor`."""
    d32 = rel_l2(ref32, ref64)
    return max(4.0 * d32, floor), d32


def model_forward(sd, inputs, n_in, n_out):
    """The reference ConvGRU (depth 1, leaky_relu) restated: conv encoder, driven cell from a zero state, autonomous cell, transposed-conv
    decoder, sigmoid.  sd: its state_dict in the dtype to compute in; inputs (B,T,1,64,64)."""
    b, t, c, hh, ww = inputs.shape
    x = inputs.reshape(b * t, c, hh, ww)
    x = F.leaky_relu(F.conv2d(x, sd["encoder.conv_encoders.0.0.weight"], sd["encoder.conv_encoders.0.0.bias"], stride=2, padding=1), 0.2)
    x = F.leaky_relu(F.conv2d(x, sd["encoder.conv_encoders.0.2.weight"], sd["encoder.conv_encoders.0.2.bias"], stride=2, padding=1), 0.2)
    x = x.view(b, t, -1, 16, 16).permute(1, 0, 2, 3, 4)
    enc = {k[len("encoder.conv_gru_cells.0."):]: v for k, v in sd.items() if k.startswith("encoder.conv_gru_cells.0.")}
    dec = {k[len("decoder.conv_gru_cells.0."):]: v for k, v in sd.items() if k.startswith("decoder.conv_gru_cells.0.")}
    h = rollout(enc, x, None, n_in, x.shape[2])[-1]
    hs = rollout(dec, None, h, n_out, h.shape[1])
    y = hs.reshape(n_out * b, -1, 16, 16)
    y = F.leaky_relu(F.conv_transpose2d(y, sd["decoder.conv_decoders.0.0.weight"], sd["decoder.conv_decoders.0.0.bias"], stride=2, padding=1), 0.2)
    y = F.conv_transpose2d(y, sd["decoder.conv_decoders.0.2.weight"], sd["decoder.conv_decoders.0.2.bias"], stride=2, padding=1)
    return torch.sigmoid(y).view(n_out, b, -1, 64, 64).permute(1, 0, 2, 3, 4)
