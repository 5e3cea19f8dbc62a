"""Float64 restatement of gradient clipping by global norm followed by torch.optim.Adam's update (amsgrad off, L2 weight decay):
what torch.nn.utils.clip_grad_norm_ + torch.optim.Adam compute, with every sum, product and square root in float64.  Only the
clipping coefficient is fp32, formed exactly as torch forms it from an fp32 norm:
    total_norm = fl32(sqrt(sum g^2));  coef = clamp(fl32(fl32(1 / fl32(total_norm + 1e-6)) * max_norm), max = 1)
(`max_norm / tensor` is `tensor.reciprocal() * max_norm` in torch; clamp keeps a NaN).  Everything here runs on the CPU."""
import math

import torch


def total_norm64(grads):
    """sqrt of the float64 sum of squares of every element of every tensor (tensors of any dtype / device), as a Python float"""
    s = 0.0
    for g in grads:
        s += float((g.detach().double().cpu() ** 2).sum())
    return math.sqrt(s)


def coef32(total_norm, max_norm):
    """torch's clip coefficient from the norm rounded to fp32, in fp32 arithmetic; a (,) float32 tensor"""
    t = torch.tensor(total_norm, dtype=torch.float64).to(torch.float32)
    c = (t + 1e-6).reciprocal() * float(max_norm)
    return torch.clamp(c, max=1.0)


def clip64(grads, max_norm):
    """(total_norm as a float, coef as a (,) float32 tensor, the scaled gradients in float64 on the CPU)"""
    total = total_norm64(grads)
    coef = coef32(total, max_norm)
    return total, coef, [g.detach().double().cpu() * coef.double() for g in grads]


class Adam64:
    """torch.optim.Adam's single-tensor update in float64 on CPU copies of the parameters; `step(grads)` takes one gradient (or
    None: skipped, as a parameter without .grad) per parameter, already clipped."""

    def __init__(self, params, lr, betas, eps, weight_decay):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, betas[0], betas[1], eps, weight_decay

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.t[i] += 1
            g = g.double() + self.wd * self.p[i]
            self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * g * g
            bc1, bc2 = 1 - self.b1 ** self.t[i], 1 - self.b2 ** self.t[i]
            self.p[i] = self.p[i] - (self.lr / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + self.eps)


def clipped_adam64(params, grads_per_step, max_norm, **hyper):
    """Run len(grads_per_step) clipped steps from `params`.  grads_per_step: per step one list with a gradient or None per parameter.
    Returns (Adam64 after the last step, the scaled gradients of the last step (None kept), [total_norm per step])."""
    opt = Adam64(params, **hyper)
    norms, scaled = [], None
    for grads in grads_per_step:
        have = [g for g in grads if g is not None]
        total, _, clipped = clip64(have, max_norm)
        it = iter(clipped)
        scaled = [None if g is None else next(it) for g in grads]
        opt.step(scaled)
        norms.append(total)
    return opt, scaled, norms


def rel_l2_all(got, ref):
    """relative L2 error of a list of tensors against a list of float64 references, over all elements together"""
    num = sum(float(((a.detach().double().cpu() - b) ** 2).sum()) for a, b in zip(got, ref))
    den = sum(float((b ** 2).sum()) for b in ref)
    return math.sqrt(num / den)
