"""Vid-ODE's two LSGAN discriminators (reference Vid-ODE/models/gan.py; built at main.py:204, trained at main.py:239-254): `netD_img`
judges single frames, `netD_seq` judges, for each predicted frame i, the sequence "observed frames from i on, then predictions up to
i".  Constructor arguments, attribute names and state_dict keys are the reference's (five convolutions: layer_1.0.weight,
layer_2..4.main.0.{weight,bias}, last_conv.weight; InstanceNorm carries none), so its checkpoints load key for key.

The 4x4 convolutions are dense library work (F.conv2d, with their bias as upstream).  With fused=True everything around them is one
launch each way: InstanceNorm + LeakyReLU (`instnorm_lrelu`, csrc/instnorm_act.hip), the sequence assembly (`gan_sequences`) and the
LSGAN terms (`lsgan_loss`, both csrc/gan.hip); these have no CPU path.  fused=False is the plain torch composition -- what the tests
and tools/gan_bench.py compare against -- and runs anywhere.  There is no environment switch.

Not reproduced: the reference's device quirks (`.cuda()` in rearrange_seq_interp, `input_real.get_device()` for the zero padding,
`.to(self.device)` on the labels).  Tensors follow their inputs; `device` is stored as the reference stores it and otherwise unused."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..optim import FusedAdamax


class ConvNormAct(nn.Module):
    """Conv2d + InstanceNorm2d + ReLU / LeakyReLU(0.2) (reference gan.py:5-24).  `main` is the reference's Sequential, so the keys are
    main.0.weight / main.0.bias; the fused forward reads the convolution from it and runs norm + activation as one launch."""

    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, act_type='relu', fused=True):
        super().__init__()
        layers = [nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding), nn.InstanceNorm2d(out_ch)]
        if act_type == 'relu':
            layers += [nn.ReLU(inplace=True)]
            self.slope = 0.0
        elif act_type == 'lrelu':
            layers += [nn.LeakyReLU(0.2)]
            self.slope = 0.2
        else:
            raise NotImplementedError(f"ConvNormAct: act_type must be 'relu' or 'lrelu', got {act_type!r}")
        self.main = nn.Sequential(*layers)
        self.fused = fused

    def forward(self, x):
        if not self.fused:
            return self.main(x)
        from ..autograd import instnorm_lrelu
        conv, norm = self.main[0], self.main[1]
        return instnorm_lrelu(F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding), norm.eps, self.slope)


class Discriminator(nn.Module):
    def __init__(self, in_ch, device, seq=False, is_extrap=True, fused=True):
        super().__init__()
        self.device, self.seq, self.is_extrap, self.fused, self.in_ch = device, seq, is_extrap, fused, in_ch
        self.layer_1 = nn.Sequential(nn.Conv2d(in_ch, 64, kernel_size=4, stride=2, padding=1, bias=False), nn.LeakyReLU(0.2))
        self.layer_2 = ConvNormAct(64, 128, kernel_size=4, stride=2, padding=1, act_type='lrelu', fused=fused)
        self.layer_3 = ConvNormAct(128, 256, kernel_size=4, stride=2, padding=1, act_type='lrelu', fused=fused)
        self.layer_4 = ConvNormAct(256, 512, kernel_size=4, stride=1, padding=2, act_type='lrelu', fused=fused)
        self.last_conv = nn.Conv2d(512, 64, kernel_size=4, stride=1, padding=2, bias=False)

    def forward(self, x):
        h = self.layer_1(x)
        h = self.layer_2(h)
        h = self.layer_3(h)
        h = self.layer_4(h)
        return self.last_conv(h)

    def _lsgan(self, pred, target):
        if self.fused:
            from ..autograd import lsgan_loss
            return lsgan_loss(pred, target)
        return torch.mean((pred - target) ** 2) if target else torch.mean(pred ** 2)

    def _frames(self, x):
        b, t, c, h, w = x.size()
        return x.contiguous().view(-1, c, h, w)

    def netD_adv_loss(self, real, fake, input_real, unequal=False):
        """0.5 * (mean (D(real) - 1)^2 + mean D(fake.detach())^2) (reference gan.py:51-73): `fake` gets no gradient."""
        fake = fake.detach()
        if self.seq:
            if self.is_extrap:
                real, fake = self.rearrange_seq(real, fake, input_real, only_fake=False, unequal=unequal)
            else:
                real, fake = self.rearrange_seq_interp(real, fake, input_real, only_fake=False)
        else:
            real, fake = self._frames(real), self._frames(fake)
        pred_fake = self.forward(fake)
        pred_real = self.forward(real)
        return (self._lsgan(pred_real, 1.0) + self._lsgan(pred_fake, 0.0)) * 0.5

    def netG_adv_loss(self, real, fake, input_real, unequal=False):
        """mean (D(fake) - 1)^2 (reference gan.py:75-91); `real` is unused, as there."""
        if self.seq:
            if self.is_extrap:
                fake = self.rearrange_seq(real, fake, input_real, only_fake=True, unequal=unequal)
            else:
                fake = self.rearrange_seq_interp(None, fake, input_real, only_fake=True)
        else:
            fake = self._frames(fake)
        return self._lsgan(self.forward(fake), 1.0)

    def _check_in_ch(self, input_real, frames, interp):
        from ..hip_ops import gan_seq_len
        seq, c = gan_seq_len(input_real.size(1), frames.size(1), interp), frames.size(2)
        if self.in_ch != seq * c:
            raise ValueError(f"Discriminator: built for in_ch = {self.in_ch}, but sequences of {input_real.size(1)} observed and "
                             f"{frames.size(1)} predicted frames of {c} channels have {seq} x {c} = {seq * c} channels")

    def _assemble(self, input_real, frames, interp):
        """One set of rows: (t * b, L * c, h, w) from input_real (b, t_in, c, h, w) and frames (b, t, c, h, w)."""
        if self.fused:
            from ..autograd import gan_sequences
            return gan_sequences(input_real, frames, interp)
        b, t, c, h, w = frames.size()
        rows = []
        if interp:
            if input_real.size(1) != t:
                raise ValueError(f"rearrange_seq_interp needs as many observed frames as predictions, got {input_real.size(1)} and {t}")
            mask = torch.eye(t, dtype=frames.dtype, device=frames.device)
            for i in range(t):
                m = mask[i].view(1, -1, 1, 1, 1)
                rows.append((1 - m) * input_real + m * frames)
        else:
            for i in range(t):
                parts = [input_real[:, i:, ...], frames[:, :i + 1, ...]]
                length = parts[0].size(1) + parts[1].size(1)
                if length < t:
                    parts.insert(0, torch.zeros((b, t - length, c, h, w), dtype=frames.dtype, device=frames.device))
                rows.append(torch.cat(parts, dim=1))
            if len({r.size(1) for r in rows}) != 1:
                raise ValueError(f"get_real_fake_seqs: rows of different lengths {[r.size(1) for r in rows]}")
        return torch.cat(rows, dim=0).view(b * t, -1, h, w)

    def get_real_fake_seqs(self, real, fake, input_real, only_fake):
        """Reference gan.py:93-128: (real_seqs or None, fake_seqs), each (t * b, L * c, h, w)."""
        self._check_in_ch(input_real, fake, False)
        fake_seqs = self._assemble(input_real, fake, False)
        if only_fake:
            return None, fake_seqs
        return self._assemble(input_real, real, False), fake_seqs

    def rearrange_seq(self, real, fake, input_real, only_fake=True, unequal=False):
        real_seqs, fake_seqs = self.get_real_fake_seqs(real, fake, input_real, only_fake)
        if only_fake is True:
            return fake_seqs
        return real_seqs, fake_seqs

    def rearrange_seq_interp(self, real, fake, input_real, only_fake=True):
        """Reference gan.py:138-159: row i * b + n is input_real[n] with frame i replaced by the fake (real) frame i."""
        self._check_in_ch(input_real, fake, True)
        fake_seqs = self._assemble(input_real, fake, True)
        if only_fake:
            return fake_seqs
        return self._assemble(input_real, real, True), fake_seqs


def create_netD(opt, device, fused=True):
    """(netD_img, netD_seq, optimizer over both) with the reference's seq_len rules (gan.py:162-181): opt.unequal -> output_sequence, else
    sample_size // 2; irregular interpolation -> sample_size; extrapolation adds the one predicted frame.  The optimizer is
    FusedAdamax(lr=opt.lr) where the reference has optim.Adamax."""
    if opt.unequal is True:
        seq_len = opt.output_sequence
    else:
        seq_len = opt.sample_size // 2
    if opt.irregular and not opt.extrap:
        seq_len = opt.sample_size
    if opt.extrap:
        seq_len += 1
    netD_img = Discriminator(in_ch=opt.input_dim, device=device, seq=False, is_extrap=opt.extrap, fused=fused).to(device)
    netD_seq = Discriminator(in_ch=opt.input_dim * seq_len, device=device, seq=True, is_extrap=opt.extrap, fused=fused).to(device)
    optimizer_netD = FusedAdamax(list(netD_img.parameters()) + list(netD_seq.parameters()), lr=opt.lr)
    return netD_img, netD_seq, optimizer_netD
