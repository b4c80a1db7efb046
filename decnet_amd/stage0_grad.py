"""Backward of stage 0 -- the cost volume and the Conv3dUnit layers of CostRegNetNoDown -- with frozen BatchNorm, under
``hip_grad()`` (conv2d_grad.py holds the switch and the 2-D Functions this follows).

One unit is y = act(conv(x, w) * scale[co] + shift[co]) on channels-last volumes [B,D,H,W,C], Conv3d k 3, s 1, p 1, with the
eval-mode BatchNorm3d folded into (scale, shift).  With the upstream gradient gy and gm = gy * [y > 0] (gm = gy without
ReLU):

    G[co,ci,kd,kh,kw] = sum gm[b,d,h,w,co] * x[b,d+kd-1,h+kh-1,w+kw-1,ci]       decnet_conv3d_wgrad (csrc/conv3d_grad.hip)
    gsum[co]          = sum gm[b,d,h,w,co]
    dW = scale[co] * G[co],  dscale[co] = <w[co], G[co]>,  dshift = gsum         (torch: conv2d_grad._param_grads)
    dx = conv(gm, W'),  W'[ci][co][kd][kh][kw] = w[co][ci][2-kd][2-kh][2-kw] * scale[co]: the forward entry, packed per
         backward (nothing is cached: the weights change every step)

``scale`` and ``shift`` enter ``Conv3dFunction`` as differentiable torch expressions of the BatchNorm parameters, so
autograd carries dscale / dshift on to ``bn.weight`` and ``bn.bias``; nothing flows to the running statistics.  The
forward is the per-layer inference entry -- decnet_conv3d_wino_bn_act, decnet_conv3d_bn_act, or for the one-channel last
unit decnet_conv3d_cout1_softargmax -- so y has the bits of the ``no_grad`` per-layer forward.  The fused Winograd stack
and decnet_stage0_forward_cf keep the activations on chip and are never taken under grad.

A unit whose ``bn`` is in ``.train()`` mode runs as ``Conv3dFunction`` with scale 1, shift 0 and no ReLU (z = conv(x, w):
no y saved, the weight gradient launched for dW alone, dx on the flipped weights), then ``BatchNorm3dActFunction``:
BatchNorm on the statistics of the batch (+ ReLU) on the channels-last volume, forward and backward on
decnet_bn_train_cl_forward / _backward (csrc/batchnorm.hip, the Columns layout), which also update the running statistics.

``CostVolumeFunction`` is decnet_costvol_forward_cf forward; its backward differentiates a torch restatement of the
header's formula.  Out of scope: cost_func "cat", a bf16x3 weight gradient, double backward, statistics synchronised across
GPUs, ``momentum=None``.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops2d
from .conv2d_grad import _param_grads, bn_act_backward, bn_act_forward, identity_epilogue


def flipped_weight3d(w, scale):
    """W'[ci][co][kd][kh][kw] = w[co][ci][2-kd][2-kh][2-kw] * scale[co] as a Conv3d weight [Ci,Co,3,3,3]: the convolution
    gm -> dx."""
    return (w * scale.view(-1, 1, 1, 1, 1)).flip(2, 3, 4).transpose(0, 1).contiguous()


def unit_operands(w, variant, last=False):
    """The forward operands of one unit from its weight w [Co,Ci,3,3,3] (fp32, on the GPU): dict(kind, w, variant).
    kind "wino" (decnet_conv3d_wino_bn_act, Winograd `variant`; output channels in fours), "direct" (decnet_conv3d_bn_act)
    or, with last=True and one output channel, "cout1" (decnet_conv3d_cout1_softargmax: the module's last unit)."""
    Co = int(w.shape[0])
    if last and Co == 1:
        return dict(kind="cout1", w=w.contiguous(), variant=None)
    if variant is not None and Co % 4 == 0:
        return dict(kind="wino", w=ops2d.conv3d_wino_pack_weight(w, variant), variant=variant)
    return dict(kind="direct", w=ops2d.conv3d_pack_weight(w), variant=None)


def _fma_exact(a, s, h):
    """fmaf(a, s, h) element by element, bit for bit, in torch ops (no host value is read): the product of two floats is
    exact in float64; its sum with h is rounded to odd there (two-sum: the error decides the sticky bit), and 53 bits
    rounded to odd round to the nearest float like the exact sum does."""
    p = a.double() * s.double()
    c = h.double().expand_as(p)
    r = p + c
    bb = r - p
    err = (p - (r - bb)) + (c - bb)                          # exact: p + c = r + err
    bits = r.view(torch.int64)
    away = (err > 0) == (r > 0)                              # |p + c| > |r|: r is the truncation already
    trunc = torch.where((err != 0) & ~away, bits - 1, bits)
    return torch.where(err != 0, trunc | 1, bits).view(torch.float64).float()


def _run_entry(ops, x, scale, shift, dims, Ci, Co, relu, ws=None):
    """One forward entry on a channels-last volume x [B,D,H,W,Ci] -> y [B,D,H,W,Co]; scale, shift [Co] on the GPU."""
    B, D, H, W = dims
    y = torch.empty(tuple(dims) + (Co,), dtype=torch.float32, device=x.device)
    if ops["kind"] == "cout1":
        # the entry takes scale and shift as host values: it runs with (1, 0), which leaves the sum as it is, and the fma
        # it would have done follows in torch, bit for bit
        raw = torch.empty(dims, dtype=torch.float32, device=x.device)
        t = None
        if Ci <= 256 and D <= 256:
            t = torch.empty(ops2d.size("conv3d_cout1_workspace_floats", B, D, H, W), dtype=torch.float32, device=x.device)
        ops2d.conv3d_cout1_softargmax(x, ops["w"], 1.0, 0.0, dims, Ci, reg=raw, ws=t)
        y = _fma_exact(raw, scale, shift).view(tuple(dims) + (1,))
        return torch.relu_(y) if relu else y
    if ops["kind"] == "wino":
        n = ops2d.size("conv3d_wino_workspace_floats", *dims, Ci, Co, ops["variant"])
        if ws is None or ws.numel() < n:
            ws = torch.empty(n, dtype=torch.float32, device=x.device)
        ops2d.conv3d_bn_act(x, ops["w"], scale, shift, None, y, dims, Ci, Co, 1 if relu else 0, ws, ops["variant"])
    else:
        ops2d.conv3d_bn_act(x, ops["w"], scale, shift, None, y, dims, Ci, Co, 1 if relu else 0)
    return y


class Conv3dFunction(Function):
    """apply(packed, relu, w, scale, shift, x) -> y [B,D,H,W,Co] for one Conv3dUnit on a channels-last volume x
    [B,D,H,W,Ci].  packed: ``unit_operands`` of the same weight (optionally with "ws": a Winograd workspace to share); w
    [Co,Ci,3,3,3], scale and shift [Co]: the differentiable ones.  The residual of CostRegNetNoDown is added by the caller
    in torch, after this, so that y > 0 stays the ReLU mask."""

    @staticmethod
    def forward(ctx, packed, relu, w, scale, shift, x):
        x = x.contiguous()
        dims, Ci, Co = tuple(int(d) for d in x.shape[:4]), int(x.shape[4]), int(w.shape[0])
        if int(w.shape[1]) != Ci:
            raise ValueError("the volume has %d channels, the layer takes %d" % (Ci, int(w.shape[1])))
        y = _run_entry(packed, x, scale.detach().float().contiguous(), shift.detach().float().contiguous(), dims, Ci, Co,
                       relu, packed.get("ws"))
        need_g = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        ctx.relu, ctx.dims, ctx.ci, ctx.co = bool(relu), dims, Ci, Co
        ctx.variant, ctx.ws = (packed["variant"] if packed["kind"] == "wino" else None), packed.get("ws")
        ctx.save_for_backward(w, scale, y if relu else None, x if need_g else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        dims, Ci, Co = ctx.dims, ctx.ci, ctx.co
        dw, dscale, dshift, gm, w32, s32 = _param_grads(
            ctx, gy.contiguous(), lambda xs, g, y: ops2d.conv3d_wgrad(xs[0], g, y, dims, Ci, Co), first=2, gm_co=-1)
        dx = None
        if ctx.needs_input_grad[5]:             # the forward entry on gm: Co -> Ci channels, scale 1, shift 0, no ReLU
            wt, cin = flipped_weight3d(w32, s32), Co
            if Co % 4:                          # (the last unit: one channel) the entries take channels in fours
                pad = 4 - Co % 4
                gm = torch.nn.functional.pad(gm, (0, pad))
                wt = torch.nn.functional.pad(wt, (0, 0, 0, 0, 0, 0, 0, pad))
                cin = Co + pad
            ops = unit_operands(wt, ctx.variant)
            dx = _run_entry(ops, gm, *identity_epilogue(Ci, gm.device), dims, cin, Ci, False, ctx.ws)
        return (None, None, dw, dscale, dshift, dx)


class BatchNorm3dActFunction(Function):
    """apply(z, weight, bias, running_mean, running_var, eps, momentum, relu) -> y = act(batch_norm(z)) on the statistics
    of the batch, z a channels-last volume [B,D,H,W,C] (decnet_bn_train_cl_forward): conv2d_grad.BatchNormActFunction on
    the other layout, one body (conv2d_grad.bn_act_forward / bn_act_backward)."""

    @staticmethod
    def forward(ctx, *args):
        return bn_act_forward(ops2d.bn_train_cl_forward, ctx, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return bn_act_backward(ops2d.bn_train_cl_backward, ctx, gy)


def bn_train_refusal(bn):
    """Why a BatchNorm in ``.train()`` mode cannot run on the statistics of the batch under ``hip_grad()`` (the condition of
    model.Unit._grad_route_train), or None."""
    if not bn.affine:
        return "affine=False"
    if not bn.track_running_stats:
        return "track_running_stats=False"
    if not isinstance(bn.momentum, float):
        return "momentum=%r (a cumulative average)" % (bn.momentum,)
    return None


_REFUSED = ("the gradient of stage 0 covers cost_func 'cor' and 'ssd'; '%s' (the 2C-channel volume behind conv_pre) is "
            "refused under grad")


# ---- the cost volume ---------------------------------------------------------------------------------------------------------
def _warp_matrices(H, W, D, device):
    """The bilinear warp of decnet_costvol_forward_cf -- xs = (x - d) W / (W - 1) - 0.5, ys = y H / (H - 1) - 0.5, zeros
    outside -- as interpolation matrices: My [H,H] (row y: its two source rows), Mx [D,W,W] (row (d, x): its two source
    columns).  Both coordinates are functions of the position alone, so the warp is linear in `right` with fixed weights."""
    f = dict(dtype=torch.float32, device=device)

    def interp(pos, n):                                      # pos [...]: source coordinates -> [..., n]
        p0 = torch.floor(pos)
        w1 = (pos - p0).unsqueeze(-1)
        col = torch.arange(n, **f)
        p0 = p0.unsqueeze(-1)
        return (col == p0).to(torch.float32) * (1 - w1) + (col == p0 + 1).to(torch.float32) * w1

    ys = torch.arange(H, **f) * H / (H - 1) - 0.5
    xs = (torch.arange(W, **f).view(1, W) - torch.arange(D, **f).view(D, 1)) * W / (W - 1) - 0.5
    return interp(ys, H), interp(xs, W)


def costvol_torch(left, right, D, cost_func):
    """The header's formula of decnet_costvol_forward_cf in torch ops, differentiable: l = (x >= d ? left : 0), r = the
    bilinear warp of right with zero padding; "cor" l r, "ssd" (l^2 + r^2) / 2 - ((l + r) / 2)^2.  [B,C,H,W] x2 ->
    [B,D,H,W,C].  The warp is two products with fixed interpolation matrices, so its gradient is a fixed-order sum."""
    B, C, H, W = left.shape
    My, Mx = _warp_matrices(H, W, D, left.device)
    My, Mx = My.to(left.dtype), Mx.to(left.dtype)
    r = torch.einsum("bcyq,dxq->bdyxc", torch.matmul(My, right), Mx)
    keep = (torch.arange(W, device=left.device).view(1, W) >= torch.arange(D, device=left.device).view(D, 1)).to(left.dtype)
    l = left.permute(0, 2, 3, 1).unsqueeze(1) * keep.view(1, D, 1, W, 1)
    if cost_func == "cor":
        return l * r
    if cost_func == "ssd":
        return (l * l + r * r) / 2 - ((l + r) / 2) ** 2
    raise NotImplementedError(_REFUSED % cost_func)


class CostVolumeFunction(Function):
    """apply(left, right, D, cost_func) -> the channels-last cost volume [B,D,H,W,C]: decnet_costvol_forward_cf forward
    (the bits of GetCostVolume); the backward recomputes ``costvol_torch`` under autograd and differentiates that."""

    @staticmethod
    def forward(ctx, left, right, D, cost_func):
        if cost_func not in ("cor", "ssd"):
            raise NotImplementedError(_REFUSED % cost_func)
        left, right = left.contiguous(), right.contiguous()
        ctx.D, ctx.cost_func = int(D), cost_func
        ctx.save_for_backward(left, right)
        return ops2d.costvol_forward_cf(left, right, int(D), cost_func)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        left, right = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(n) for t, n in zip((left, right), need)]
            cv = costvol_torch(leaves[0], leaves[1], ctx.D, ctx.cost_func)
            wanted = [t for t, n in zip(leaves, need) if n]
            got = list(torch.autograd.grad(cv, wanted, g.contiguous())) if wanted else []
        return tuple(got.pop(0) if n else None for n in need) + (None, None)


def unit_library(x, w, scale, shift, relu):
    """The library arm of one unit: torch's conv3d on the permuted (channels-last-3d) view of x [B,D,H,W,Ci], then
    * scale + shift and ReLU, under autograd -> [B,D,H,W,Co]."""
    y = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w, None, stride=1, padding=1).permute(0, 2, 3, 4, 1)
    y = y * scale + shift
    return torch.relu(y) if relu else y


def unit_library_train(x, w, bn, relu):
    """The library arm of one unit in ``.train()`` mode: torch's conv3d, then torch's batch_norm on the statistics of the
    batch (it updates bn's running statistics; ``num_batches_tracked`` is the caller's) and ReLU -> [B,D,H,W,Co]."""
    z = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w, None, stride=1, padding=1)
    y = torch.nn.functional.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)
    y = y.permute(0, 2, 3, 4, 1)
    return torch.relu(y) if relu else y
