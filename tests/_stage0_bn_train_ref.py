"""Float64 references of training-mode BatchNorm3d in stage 0 (decnet_amd/csrc/batchnorm.hip, the Columns layout,
stage0_grad.BatchNorm3dActFunction, CostRegNetNoDown in .train() mode under hip_grad()) for
tests/test_stage0_bn_train_cpu.py and tests/test_stage0_bn_train_gpu.py.  CPU only.

1. The entries.  A channels-last matrix z [rows, C] is the NCHW tensor [1, C, 1, rows] transposed, so the reference of the
   entries IS tests/_bn_train_ref.forward / .backward (float64, the pivot z[0, c] = z4[0, c, 0, 0]) on that view, and the
   data sets are its `entry_data`: the channels-last kernels are held to what the 2-D kernels are held to.
2. The module.  `_stage0_grad_ref.regnet` / `stage0_grads` restated for .train() mode: F.batch_norm(training=True) per unit
   whose bn is in train mode (a bn in eval mode keeps `unit_pre`), IMPOSED ReLU masks (y = pre * mask), and the running
   statistics after k steps."""
import copy

import torch
import torch.nn.functional as F

import _bn_train_ref as BR
import _stage0_grad_ref as SG

F64 = torch.float64
ROWS = 32                                   # DECNET_BN_CL_ROWS of include/decnet_hip.h: rows of a segment
FIN_J = 16                                  # csrc/batchnorm.hip, Columns: the finish kernel's threads per channel (of 16)
FIN_THREADS = 256                           # ... and of its workgroup


def entry_cases(R=ROWS):
    """The (rows, C) of the entry tests: the smallest, odd sizes, a segment less / exact / plus a row, one segment at the
    model's width, more channels than a workgroup has threads, and more partials per channel than the finish kernel has
    threads (so also more than the 16 that share a channel: the stride wraps either way)."""
    m = FIN_THREADS + 1
    return [(2, 1), (7, 3), (R - 1, 4), (R, 4), (R + 1, 5), (3, 216), (R + 1, 260), (m * R + 3, 1), (m * R + 3, 4)]


def shape4(rows, C):
    return (1, C, 1, rows)


def to_cl(t4):
    """[1, C, 1, rows] -> the channels-last matrix [rows, C]."""
    return t4[0, :, 0, :].t().contiguous()


def from_cl(t):
    """[rows, C] -> [1, C, 1, rows]."""
    return t.t().reshape(1, t.shape[1], 1, t.shape[0])


def entry_data(rows, C, first_kind=0, relu=False):
    """`_bn_train_ref.entry_data` on [1, C, 1, rows] -> its dict (z and gy in the NCHW view; `to_cl` gives the matrices)."""
    return BR.entry_data(shape4(rows, C), first_kind, relu)


def forward(z_cl, gamma, beta, eps, momentum=None, running_mean=None, running_var=None, relu=True):
    return BR.forward(from_cl(z_cl), gamma, beta, eps, momentum, running_mean, running_var, relu)


def backward(fwd, gy_cl, gamma, relu=True, mask_cl=None):
    return BR.backward(fwd, from_cl(gy_cl), gamma, relu, None if mask_cl is None else from_cl(mask_cl))


# ---- the module in .train() mode -----------------------------------------------------------------------------------------------
def unit_pre_train(u, x):
    """The pre-activation of a Conv3dUnit on NCDHW x: conv -> BatchNorm3d on the statistics of the batch when u.bn is in
    train mode (the running statistics and num_batches_tracked updated in place, as torch.nn.BatchNorm3d does), on the
    running statistics otherwise."""
    if not u.bn.training:
        return SG.unit_pre(u, x)
    z = F.conv3d(x, u.conv.weight, None, stride=1, padding=1)
    pre = F.batch_norm(z, u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias, True, u.bn.momentum, u.bn.eps)
    u.bn.num_batches_tracked += 1
    return pre


def regnet_train(mod, cv, masks=None):
    """`_stage0_grad_ref.regnet` with `unit_pre_train`: -> (reg [B,D,H,W], [pre-activation of every unit], [mask taken])."""
    x, keep, pres, took = cv, None, [], []
    for i, u in enumerate(mod.units()):
        pre = unit_pre_train(u, x)
        pres.append(pre.detach())
        if not u.relu:
            took.append(None)
            y = pre
        elif masks is None:
            took.append(pre.detach() > 0)
            y = torch.relu(pre)
        else:
            took.append(masks[i])
            y = pre * masks[i].to(pre.dtype)
        x = y + keep if i == 4 else y
        if i == 1:
            keep = y
    return x[:, 0], pres, took


def train_copy(mod, dtype, frozen=()):
    """A copy of `mod` in `dtype` on the CPU in .train() mode, the units `frozen` (indices) with their bn in eval mode."""
    mod = copy.deepcopy(mod).to("cpu", dtype).train()
    for i in frozen:
        mod.units()[i].bn.eval()
    return mod


def stage0_grads_train(mod, L, R, D, r, r2, dtype, masks=None, steps=1, frozen=()):
    """`steps` train-mode steps of (pred r).sum() + (reg r2).sum() on a `train_copy` of `mod`, the gradients cleared before
    each (nothing updates the parameters, so every step sees the same batch and the same masks) -> dict(grads of the last
    step: {name: gradient} over every parameter and "L", "R"; pred; reg; pre; took; buffers: {name: value after the steps};
    history: the buffers after every step)."""
    mod = train_copy(mod, dtype, frozen)
    history = []
    for _ in range(steps):
        mod.zero_grad(set_to_none=True)
        Lc, Rc = (t.detach().to("cpu", dtype).clone().requires_grad_() for t in (L, R))
        cv = SG.costvol(Lc, Rc, D, mod.cost_func).permute(0, 4, 1, 2, 3)
        reg, pres, took = regnet_train(mod, cv, masks)
        pred = (torch.softmax(reg, 1) * torch.arange(D, dtype=dtype).view(1, D, 1, 1)).sum(1)
        ((pred * r.to("cpu", dtype)).sum() + (reg * r2.to("cpu", dtype)).sum()).backward()
        history.append({n: b.detach().clone() for n, b in mod.named_buffers()})
    grads = {n: p.grad.detach() for n, p in mod.named_parameters()}
    grads.update(L=Lc.grad.detach(), R=Rc.grad.detach())
    return dict(grads=grads, pred=pred.detach(), reg=reg.detach(), pre=pres, took=took, buffers=history[-1], history=history)


def torch_modules_train(mod, L, R, D, r, r2, steps=1):
    """The same steps in float64 through torch's OWN modules: u.bn(u.conv(x)) with torch.nn.BatchNorm3d in train mode
    (which keeps its buffers itself), torch.relu, the residual -> the same dict (without pre / took)."""
    mod = train_copy(mod, F64)
    for _ in range(steps):
        mod.zero_grad(set_to_none=True)
        Lc, Rc = (t.detach().to("cpu", F64).clone().requires_grad_() for t in (L, R))
        x, keep = SG.costvol(Lc, Rc, D, mod.cost_func).permute(0, 4, 1, 2, 3), None
        for i, u in enumerate(mod.units()):
            y = u.bn(u.conv(x))
            y = torch.relu(y) if u.relu else y
            x = y + keep if i == 4 else y
            if i == 1:
                keep = y
        reg = x[:, 0]
        pred = (torch.softmax(reg, 1) * torch.arange(D, dtype=F64).view(1, D, 1, 1)).sum(1)
        ((pred * r.double()).sum() + (reg * r2.double()).sum()).backward()
    grads = {n: p.grad.detach() for n, p in mod.named_parameters()}
    grads.update(L=Lc.grad.detach(), R=Rc.grad.detach())
    return dict(grads=grads, pred=pred.detach(), reg=reg.detach(),
                buffers={n: b.detach().clone() for n, b in mod.named_buffers()})
