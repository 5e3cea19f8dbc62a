"""A dtype-generic restatement of Vid-ODE's discriminators (reference Vid-ODE/models/gan.py), written from a reading of what they
compute, for the GAN tests: functions of a state_dict, so float64 runs are a `.double()` away.  The yardstick of tests/test_hip_gan.py
and, in float32, checked against the reference's own classes through tests/golden/gan.npz (tests/test_gan_ref_cpu.py).

    discriminator   conv4x4/s2 (no bias) -> lrelu;  3 x [conv4x4 (bias) -> instance norm (no affine, biased variance, eps 1e-5) -> lrelu]
                    with strides 2, 2, 1 and paddings 1, 1, 2;  conv4x4/s1/p2 (no bias).  lrelu = LeakyReLU(0.2)
    sequences       extrapolation: row i b + n = [zeros] ++ input_real[n, i:] ++ frames[n, :i+1], right-aligned in L = max(t, t_in + 1)
                    frames; interpolation: input_real[n] with frame i replaced by frames[n, i]
    losses          D: ((D(real) - 1)^2).mean() / 2 + (D(fake.detach())^2).mean() / 2;   G: ((D(fake) - 1)^2).mean()"""
import torch
import torch.nn.functional as F

KEYS = ["layer_1.0.weight", "layer_2.main.0.weight", "layer_2.main.0.bias", "layer_3.main.0.weight", "layer_3.main.0.bias",
        "layer_4.main.0.weight", "layer_4.main.0.bias", "last_conv.weight"]
EPS = 1e-5
SLOPE = 0.2


def shapes(in_ch):
    return {"layer_1.0.weight": (64, in_ch, 4, 4), "layer_2.main.0.weight": (128, 64, 4, 4), "layer_2.main.0.bias": (128,),
            "layer_3.main.0.weight": (256, 128, 4, 4), "layer_3.main.0.bias": (256,), "layer_4.main.0.weight": (512, 256, 4, 4),
            "layer_4.main.0.bias": (512,), "last_conv.weight": (64, 512, 4, 4)}


def norm_act(x, slope=SLOPE, eps=EPS):
    """Instance norm over the trailing dimensions of (N, C, ...) + leaky ReLU, spelled out: two-pass, biased variance."""
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    mean = flat.mean(dim=2, keepdim=True)
    d = flat - mean
    var = (d * d).mean(dim=2, keepdim=True)
    xhat = (d / torch.sqrt(var + eps)).reshape(x.shape)
    return torch.where(xhat > 0, xhat, slope * xhat)


def discriminator(sd, x):
    h = F.conv2d(x, sd["layer_1.0.weight"], None, stride=2, padding=1)
    h = torch.where(h > 0, h, SLOPE * h)
    for name, stride, pad in (("layer_2", 2, 1), ("layer_3", 2, 1), ("layer_4", 1, 2)):
        h = norm_act(F.conv2d(h, sd[name + ".main.0.weight"], sd[name + ".main.0.bias"], stride=stride, padding=pad))
    return F.conv2d(h, sd["last_conv.weight"], None, stride=1, padding=2)


def seq_len(t_in, t):
    """L of the extrapolation form, from the rows themselves: every row must come out at one length."""
    lengths = set()
    for i in range(t):
        own = max(0, t_in - i) + i + 1
        lengths.add(max(own, t))        # a row shorter than t is padded with zero frames up to t
    if len(lengths) != 1:
        raise ValueError(f"rows of different lengths {sorted(lengths)} for t_in = {t_in}, t = {t}")
    return lengths.pop()


def sequences(input_real, frames):
    """(t b, L c, h, w): the extrapolation rows."""
    b, t, c, h, w = frames.shape
    t_in = input_real.shape[1]
    length = seq_len(t_in, t)
    out = frames.new_zeros((t, b, length, c, h, w))
    for i in range(t):
        keep = max(0, t_in - i)
        start = length - (keep + i + 1)
        if keep:
            out[i, :, start:start + keep] = input_real[:, i:]
        out[i, :, start + keep:] = frames[:, :i + 1]
    return out.reshape(t * b, length * c, h, w)


def sequences_interp(input_real, frames):
    """(t b, t c, h, w): input_real with frame i replaced, for every i."""
    b, t, c, h, w = frames.shape
    if input_real.shape[1] != t:
        raise ValueError(f"the interpolation form needs t_in == t, got {input_real.shape[1]} and {t}")
    out = input_real.unsqueeze(0).repeat(t, 1, 1, 1, 1, 1)
    for i in range(t):
        out[i, :, i] = frames[:, i]
    return out.reshape(t * b, t * c, h, w)


def _rows(x, input_real, seq, extrap):
    if not seq:
        return x.reshape((-1,) + tuple(x.shape[2:]))
    return sequences(input_real, x) if extrap else sequences_interp(input_real, x)


def d_loss(sd, real, fake, input_real=None, seq=False, extrap=True):
    pred_fake = discriminator(sd, _rows(fake.detach(), input_real, seq, extrap))
    pred_real = discriminator(sd, _rows(real, input_real, seq, extrap))
    return (((pred_real - 1) ** 2).mean() + (pred_fake ** 2).mean()) * 0.5


def g_loss(sd, fake, input_real=None, seq=False, extrap=True):
    return ((discriminator(sd, _rows(fake, input_real, seq, extrap)) - 1) ** 2).mean()


def weight_like(shape, seed):
    """Procedural discriminator weights: an index formula (no generator state), +-1 / sqrt(fan_in) for a convolution, +-0.04 for a bias."""
    from conftest import procedural_tensor
    if len(shape) == 1:
        return procedural_tensor(shape, seed, -0.04, 0.04)
    bound = 1.0 / float(shape[1] * shape[2] * shape[3]) ** 0.5
    return procedural_tensor(shape, seed, -bound, bound)


def state_dict(in_ch, seed):
    return {k: weight_like(s, seed + 17 * n) for n, (k, s) in enumerate(shapes(in_ch).items())}
