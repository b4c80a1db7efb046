"""Chains of matrix-core conv units for tests/test_conv2d_mfma_grad_gpu.py and tests/test_conv2d_mfma_grad_cpu.py, and
their reference with IMPOSED ReLU masks.  CPU only.

A chain is an nn.Sequential of eval-mode ``Unit``s (conv -> frozen BatchNorm -> optional ReLU).  With 81 channels on
64 x 64 pixels a chain has about a million pre-activations, and some of them lie closer to zero than the forward kernels'
error: a free float64 run takes another ReLU branch there than the GPU run, and the gradients of the two then differ by
whole terms, not by rounding.  So the reference takes the masks as data: unit i computes y = pre * mask_i, in forward and
backward, where mask_i is the GPU run's own [y_i > 0].  ``masks=None`` is the free run (y = relu(pre)), which also
returns the masks it took."""
import torch
import torch.nn.functional as F

import _model_cases as MC

CHAIN_HW = (64, 64)                 # the floor of the "mfma" route: 4096 pixels


def chain_case(name):
    """-> (chain (float32, CPU, eval), parts: the tensors whose channel concatenation is the input, r: the weights of the
    loss (out * r).sum())."""
    from decnet_amd.model import DynamicUpsampling, UpBlock
    H, W = CHAIN_HW
    g = torch.Generator().manual_seed({"upsampling": 411, "upblock": 412}[name])
    if name == "upsampling":
        seq = MC.seeded(lambda: DynamicUpsampling(8, 3), 511).weight_learning
        parts = [torch.randn(1, 73, H, W, generator=g)]
    else:
        seq = MC.seeded(lambda: UpBlock(72, 24), 512).conv
        parts = [torch.randn(1, 24, H, W, generator=g), torch.randn(1, 24, H, W, generator=g)]
    return seq, parts, torch.randn(1, seq[-1].conv.out_channels, H, W, generator=g)


def unit_pre(u, x):
    """The pre-activation of a Unit in eval mode, in torch: conv -> BatchNorm on the running statistics."""
    c = u.conv
    pre = F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation)
    if u.bn is not None:
        pre = F.batch_norm(pre, u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias, False, 0.0, u.bn.eps)
    return pre


def chain_grads(seq, parts, r, dtype, masks=None):
    """One run of (chain(cat(parts)) * r).sum() on a copy of the chain in `dtype` on the CPU -> ({name: gradient} over every
    parameter and "part<i>", [mask of every unit: bool, None without ReLU]).  masks: impose these instead of pre > 0."""
    import copy
    seq = copy.deepcopy(seq).to(dtype).eval()
    xs = [t.detach().clone().to(dtype).requires_grad_() for t in parts]
    x, took = torch.cat(xs, 1), []
    for i, u in enumerate(seq):
        pre = unit_pre(u, x)
        if not u.relu:
            took.append(None)
            x = pre
        elif masks is None:
            took.append(pre.detach() > 0)
            x = torch.relu(pre)
        else:
            took.append(masks[i])
            x = pre * masks[i].to(dtype)
    (x * r.to(dtype)).sum().backward()
    grads = {n: p.grad.detach() for n, p in seq.named_parameters()}
    grads.update({"part%d" % i: t.grad.detach() for i, t in enumerate(xs)})
    return grads, took
