"""Cross-rank BatchNorm restated in torch, any dtype (the tests use float64): every rank reduces its shard to per-channel partial sums,
the sums are added over the ranks, and every rank normalises / differentiates with the reduced sums -- the split that
csrc/bn_relu_up.hip makes around its one collective each way (ode_rl_amd.dist.sync_batchnorm).  No ReLU, no upsampling: they are
per-element and sit outside the statistics."""
import torch


def forward_sums(x):
    """[sum x (C) | sum x^2 (C) | count] of one shard (N, C, H, W)."""
    count = x.new_tensor([x.shape[0] * x.shape[2] * x.shape[3]])
    return torch.cat([x.sum((0, 2, 3)), (x * x).sum((0, 2, 3)), count])


def statistics(sums):
    """(mean, biased variance, count) from reduced forward sums."""
    c = (sums.numel() - 1) // 2
    count = sums[2 * c]
    mean = sums[:c] / count
    return mean, (sums[c:2 * c] / count - mean * mean).clamp_min(0), count


def normalise(x, sums, weight, bias, eps):
    """(y, xhat) of one shard from the REDUCED sums."""
    mean, var, _ = statistics(sums)
    xhat = (x - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + eps).view(1, -1, 1, 1)
    return xhat * weight.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1), xhat


def running_update(running_mean, running_var, sums, momentum):
    """nn.BatchNorm2d's update with the global count: unbiased variance n / (n - 1)."""
    mean, var, n = statistics(sums)
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * n / (n - 1)


def backward_sums(g, xhat):
    """[sum g (C) | sum g * xhat (C)] of one shard: also this rank's d beta and d gamma."""
    return torch.cat([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))])


def input_gradient(g, xhat, bsums, fsums, weight, eps):
    """dx of one shard from the REDUCED backward sums and the reduced forward sums."""
    c = weight.numel()
    _, var, count = statistics(fsums)
    m1, m2 = (bsums[:c] / count).view(1, -1, 1, 1), (bsums[c:] / count).view(1, -1, 1, 1)
    return (weight * torch.rsqrt(var + eps)).view(1, -1, 1, 1) * (g - m1 - xhat * m2)


def sharded_batch_norm(shards, grads, weight, bias, eps, running_mean, running_var, momentum):
    """The whole exchange for a list of shards and the gradients of their outputs.  Returns a dict: per-shard `y` and `dx`, per-rank
    local `dgamma` / `dbeta`, and the running statistics every rank ends with."""
    fsums = sum(forward_sums(x) for x in shards)                       # the forward's all-reduce
    ys, xhats = zip(*(normalise(x, fsums, weight, bias, eps) for x in shards))
    local = [backward_sums(g, xh) for g, xh in zip(grads, xhats)]
    bsums = sum(local)                                                 # the backward's all-reduce
    c = weight.numel()
    rm, rv = running_update(running_mean, running_var, fsums, momentum)
    return {"y": list(ys), "dx": [input_gradient(g, xh, bsums, fsums, weight, eps) for g, xh in zip(grads, xhats)],
            "dbeta": [s[:c] for s in local], "dgamma": [s[c:] for s in local], "running_mean": rm, "running_var": rv}
