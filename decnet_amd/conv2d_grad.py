"""Backward of the stride-1 Conv2dUnit layers (csrc/conv2d_small.hip, csrc/conv2d_mfma.hip) with frozen BatchNorm, opt-in.

For one unit, y = act(conv(x, w) * scale[co] + shift[co]) with the eval-mode BatchNorm folded into (scale, shift) -- or
(1, bias) without BatchNorm -- and x possibly the never-materialised concatenation of up to 6 tensors.  With the upstream
gradient gy and gm = gy * [y > 0] (gm = gy without ReLU):

    G[co,ci,ky,kx] = sum gm[b,co,y,x] * x[b,ci,y+(ky-k/2)d,x+(kx-k/2)d]      decnet_conv2d_wgrad (csrc/conv2d_grad.hip)
    gsum[co]       = sum gm[b,co,y,x]
    dW = scale[co] * G[co],  dscale[co] = <w[co], G[co]>,  dshift = gsum     (a few hundred floats: torch)
    dx = conv(gm, W'),  W'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] * scale[co], same dilation: the forward kernel

``scale`` and ``shift`` enter the Function as differentiable torch expressions of the BatchNorm parameters, so autograd
carries dscale / dshift on to ``bn.weight``, ``bn.bias`` and ``conv.bias``; nothing flows to the running statistics.

``hip_grad()`` switches the path on for the calling thread (default: off -- ``model.Unit`` then behaves as before).  The
same switch puts the warp, the dynamic upsampling and SoftAttention's blend on their HIP Functions (tail_grad.py).
The many-channel stride-1 units of the matrix-core route (``Unit._route`` "mfma") take ``Conv2dMfmaFunction``: the same
backward on decnet_conv2d_mfma_cat_bn_act and decnet_conv2d_mfma_wgrad (csrc/conv2d_mfma_grad.hip).
The layers between the pyramid levels -- Conv2d k 3, stride 3, padding 1 and ConvTranspose2d k 3, stride 3 (``Unit._route``
"conv_s3", "mfma_s3", "deconv", "mfma_deconv") -- take ``Conv2dS3Function`` / ``Deconv2dS3Function``:

    conv        G[co,ci,ky,kx] = sum gm[b,co,yo,xo] * x[b,ci,3yo-1+ky,3xo-1+kx]             decnet_conv2d_k3s3_wgrad
                dx = d2s3_pad1(conv1x1(gm, (w * scale) read as [Cout, 9 Cin], transposed))   (every input pixel: one window)
    transposed  G[ci,co,a,c] = sum x[b,ci,i,j] * gm[b,co,3i+a,3j+c]                          decnet_deconv2d_k3s3_wgrad
                dx = conv1x1(s2d3_pad0(gm), (w * scale[co]) read as [Cin, 9 Cout])           (w [Cin,Cout,3,3], no flip)

with the 1 x 1 convolutions on decnet_conv2d_mfma_cat_bn_act.

A unit in ``.train()`` mode (``Unit._forward_grad_train``) runs the same conv Function with scale 1, shift 0 and no ReLU,
then ``BatchNormActFunction``: BatchNorm2d on the statistics of the batch (+ ReLU), forward and backward on
csrc/batchnorm.hip, the running statistics updated in place by the forward kernel.
Stage 0 (Conv3d units, BatchNorm3d frozen or on the statistics of the batch) has its own Functions in stage0_grad.py, on
the parameter side (``_param_grads``) and the identity epilogue (``identity_epilogue``) of this file.
Out of scope: statistics synchronised across GPUs, ``momentum=None``, the ASPP tap-conv block, the
20 x 36 stride-1 layers, double backward.
"""
import contextlib
import threading

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops2d

_STATE = threading.local()


def hip_grad_enabled():
    """Whether the calling thread is inside ``hip_grad()`` (thread-local, off by default)."""
    return getattr(_STATE, "on", False)


@contextlib.contextmanager
def hip_grad(enabled=True):
    """While active (in this thread), an eval-mode ``Unit`` that ``Unit._grad_route`` covers records its backward on the
    HIP kernels instead of going to the library, and one in ``.train()`` mode that ``Unit._grad_route_train`` covers runs
    its BatchNorm on the statistics of the batch as ``BatchNormActFunction``.  Nests; ``hip_grad(False)`` switches it off
    inside an enabled region."""
    old = hip_grad_enabled()
    _STATE.on = bool(enabled)
    try:
        yield
    finally:
        _STATE.on = old


def flipped_weight(w, scale, rows=None):
    """W'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] * scale[co] as a Conv2d weight [Cin,Cout,k,k] (the convolution
    gm -> dx); rows: the (start, stop) channel ranges of ci to keep, in order."""
    wt = (w * scale.view(-1, 1, 1, 1)).flip(2, 3).transpose(0, 1)
    if rows is not None:
        wt = torch.cat([wt[a:b] for a, b in rows], 0)
    return wt.contiguous()


def _param_grads(ctx, gy, wgrad, co_dim=0, first=4, gm_co=1):
    """The parameter side of one unit's backward, shared by every Function here and by stage0_grad.Conv3dFunction: ->
    (dw, dscale, dshift, gm, w32, s32).  wgrad(xs, gy, y) -> (G, gsum, gm): the weight-gradient entry, launched only when
    the weight or the scale wants a gradient; co_dim: the output-channel axis of the weight (1 for a transposed layer),
    whose rank is the weight's own (4, or 5 for a Conv3d); first: the position of w among the Function's arguments (scale
    and shift follow it); gm_co: the channel axis of gm (1: NCHW planes, -1: channels-last volumes)."""
    w, scale, y = ctx.saved_tensors[:3]
    need_w, need_scale, need_shift = ctx.needs_input_grad[first:first + 3]
    w32, s32 = w.detach().float().contiguous(), scale.detach().float()
    dw = dscale = dshift = None
    if need_w or need_scale:
        G, gsum, gm = wgrad(ctx.saved_tensors[3:], gy, y)
        if need_w:
            dw = G * s32.view([-1 if d == co_dim else 1 for d in range(w.dim())])
        if need_scale:
            dscale = (w32.double() * G.double()).sum([d for d in range(w.dim()) if d != co_dim]).float()
        if need_shift:
            dshift = gsum
    else:                                   # no weight gradient wanted: the mask and the sum alone
        gm = gy if y is None else torch.ops.aten.threshold_backward(gy, y, 0)
        if need_shift:
            dshift = gm.sum([d for d in range(gm.dim()) if d != gm_co % gm.dim()], dtype=torch.float64).float()
    return dw, dscale, dshift, gm, w32, s32


def _unit_backward(ctx, gy, wgrad, dx_conv):
    """The backward of one stride-1 unit, shared by the few-channel and the matrix-core Function.  wgrad(xs, gy, y, k,
    dil) -> (G, gsum, gm): the weight-gradient entry; dx_conv(gm, wt, k, dil) -> conv(gm, wt) for wt [n, Cout, k, k]: the
    forward entry on the flipped weights."""
    need_parts = ctx.needs_input_grad[7:]
    dw, dscale, dshift, gm, w32, s32 = _param_grads(ctx, gy.contiguous(), lambda xs, g, y: wgrad(xs, g, y, ctx.k, ctx.dil))
    grads = [None] * len(need_parts)
    if any(need_parts):
        rows, at, c0 = [], {}, 0
        for i, c in enumerate(ctx.cins):
            if need_parts[i]:
                at[i] = sum(b - a for a, b in rows)
                rows.append((c0, c0 + c))
            c0 += c
        dx = dx_conv(gm, flipped_weight(w32, s32, rows), ctx.k, ctx.dil)   # wt: [channels wanted, Cout, k, k]
        for i, a in at.items():
            grads[i] = dx[:, a:a + ctx.cins[i]]
    return (None, None, None, None, dw, dscale, dshift) + tuple(grads)


def _save(ctx, k, dil, relu, w, scale, y, xs, first=4):
    need_g = ctx.needs_input_grad[first] or ctx.needs_input_grad[first + 1]
    ctx.k, ctx.dil, ctx.relu, ctx.cins = k, dil, relu, [int(t.shape[1]) for t in xs]
    ctx.save_for_backward(w, scale, y if relu else None, *(xs if need_g else ()))


def identity_epilogue(n, device):
    """(scale, shift) = (ones, zeros) [n]: a forward entry as the plain convolution gm -> dx."""
    return torch.ones(n, device=device), torch.zeros(n, device=device)


def _dx_small(gm, wt, k, dil):
    n, co = wt.shape[0], wt.shape[1]
    return ops2d.conv2d_bn_act(gm, ops2d.conv2d_pack_weight(wt, False), *identity_epilogue(n, gm.device), co, k, dil, 0)


def _dx_mfma(gm, wt, k, dil):
    n, co = wt.shape[0], wt.shape[1]
    return ops2d.conv2d_mfma_cat_bn_act([gm], ops2d.conv2d_mfma_pack_weight(wt, co, k), *identity_epilogue(n, gm.device),
                                        co, k, dil, 0)


class Conv2dSmallFunction(Function):
    """apply(packed, k, dil, relu, w, scale, shift, *parts) -> y [B,Cout,H,W].  packed: the forward kernels' operands
    (``Unit._folded()``: packed weight, scale, shift -- detached copies of the same values); w [Cout,Cin,k,k], scale and
    shift [Cout]: the differentiable ones; parts: the tensors [B,c_i,H,W] whose channel concatenation is the input."""

    @staticmethod
    def forward(ctx, packed, k, dil, relu, w, scale, shift, *parts):
        xs = [t.contiguous() for t in parts]
        cin = int(w.shape[1])
        if len(xs) == 1:
            y = ops2d.conv2d_bn_act(xs[0], *packed, cin, k, dil, 1 if relu else 0)
        else:
            y = ops2d.conv2d_cat_bn_act(xs, *packed, cin, k, dil, 1 if relu else 0)
        _save(ctx, k, dil, relu, w, scale, y, xs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _unit_backward(ctx, gy, ops2d.conv2d_wgrad, _dx_small)


class Conv2dMfmaFunction(Function):
    """The same for a unit of the matrix-core route (``Unit._route`` "mfma"): packed is ``Unit._folded_mfma()``, the
    forward is decnet_conv2d_mfma_cat_bn_act -- the entry and the bits of the ``no_grad`` forward --, the weight gradient
    decnet_conv2d_mfma_wgrad, dx the forward entry on the flipped weights (packed per backward: nothing is cached, the
    weights change every step)."""

    @staticmethod
    def forward(ctx, packed, k, dil, relu, w, scale, shift, *parts):
        xs = [t.contiguous() for t in parts]
        y = ops2d.conv2d_mfma_cat_bn_act(xs, *packed, int(w.shape[1]), k, dil, 1 if relu else 0)
        _save(ctx, k, dil, relu, w, scale, y, xs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _unit_backward(ctx, gy, ops2d.conv2d_mfma_wgrad, _dx_mfma)


def _conv1x1_mfma(x, wt):
    """conv1x1(x, wt) for wt [n, C] on the matrix-core forward entry (scale 1, shift 0, no ReLU), packed per backward."""
    n, c = wt.shape
    return ops2d.conv2d_mfma_cat_bn_act([x], ops2d.conv2d_mfma_pack_weight(wt.contiguous(), c, 1),
                                        *identity_epilogue(n, x.device), c, 1, 1, 0)


class Conv2dS3Function(Function):
    """apply(route, packed, relu, w, scale, shift, x) -> y [B,Cout,ceil(H/3),ceil(W/3)] for a Conv2d k 3, stride 3, padding 1
    unit.  route: the unit's forward route, "conv_s3" (packed: ``Unit._folded()``) or "mfma_s3" (``Unit._folded_mfma()``):
    the forward is that route's inference entry, so its bits are the ``no_grad`` forward's."""

    @staticmethod
    def forward(ctx, route, packed, relu, w, scale, shift, x):
        x = x.contiguous()
        ci = int(w.shape[1])
        if route == "mfma_s3":
            y = ops2d.conv2d_mfma_cat_bn_act([ops2d.s2d3_pad1(x)], *packed, 9 * ci, 1, 1, 1 if relu else 0)
        else:
            y = ops2d.conv2d_k3s3_bn_act(x, *packed, ci, 1 if relu else 0)
        ctx.hw = (int(x.shape[2]), int(x.shape[3]))
        _save(ctx, 3, 1, relu, w, scale, y, [x], first=3)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        dw, dscale, dshift, gm, w32, s32 = _param_grads(ctx, gy.contiguous(),
                                                        lambda xs, g, y: ops2d.conv2d_k3s3_wgrad(xs[0], g, y), first=3)
        dx = None
        if ctx.needs_input_grad[6]:         # the 1 x 1 convolution Cout -> 9 Cin of gm, then the adjoint of s2d3_pad1
            wt = (w32 * s32.view(-1, 1, 1, 1)).reshape(w32.shape[0], -1).t()
            dx = ops2d.d2s3_pad1(_conv1x1_mfma(gm, wt), *ctx.hw)
        return (None, None, None, dw, dscale, dshift, dx)


class Deconv2dS3Function(Function):
    """The same for a ConvTranspose2d k 3, stride 3 unit (w [Cin,Cout,3,3]; route "deconv" or "mfma_deconv") -> y
    [B,Cout,3H,3W]."""

    @staticmethod
    def forward(ctx, route, packed, relu, w, scale, shift, x):
        x = x.contiguous()
        entry = ops2d.deconv2d_mfma_k3s3_bn_act if route == "mfma_deconv" else ops2d.deconv2d_k3s3_bn_act
        y = entry(x, *packed, int(w.shape[0]), 1 if relu else 0)
        _save(ctx, 3, 1, relu, w, scale, y, [x], first=3)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        dw, dscale, dshift, gm, w32, s32 = _param_grads(ctx, gy.contiguous(),
                                                        lambda xs, g, y: ops2d.deconv2d_k3s3_wgrad(xs[0], g, y), co_dim=1,
                                                        first=3)
        dx = None
        if ctx.needs_input_grad[6]:         # the space-to-depth of gm, then the 1 x 1 convolution 9 Cout -> Cin
            wt = (w32 * s32.view(1, -1, 1, 1)).reshape(w32.shape[0], -1)
            dx = _conv1x1_mfma(ops2d.s2d3_pad0(gm), wt)
        return (None, None, None, dw, dscale, dshift, dx)


def bn_act_forward(bn_forward, ctx, z, weight, bias, running_mean, running_var, eps, momentum, relu):
    """The forward of BatchNormActFunction and stage0_grad.BatchNorm3dActFunction on their ops2d entry `bn_forward`.  The
    kernel writes running_mean / running_var in place, which autograd does not see: their versions are bumped here."""
    z = z.contiguous()
    y, stats = bn_forward(z, weight, bias, eps, momentum, running_mean, running_var, relu)
    if running_mean is not None:
        torch.autograd.graph.increment_version(running_mean)
        torch.autograd.graph.increment_version(running_var)
    ctx.relu = bool(relu)
    ctx.save_for_backward(z, weight, bias, stats)
    return y


def bn_act_backward(bn_backward, ctx, gy):
    """Their backward: the gradients of z, weight, bias, each only when wanted."""
    z, weight, bias, stats = ctx.saved_tensors
    need_z, need_w, need_b = ctx.needs_input_grad[:3]
    gz = dw = db = None
    if need_z or need_w or need_b:
        gz, dw, db = bn_backward(z, gy.contiguous(), weight, bias, stats, ctx.relu, want_gz=need_z)
    return (gz, dw if need_w else None, db if need_b else None, None, None, None, None, None)


class BatchNormActFunction(Function):
    """apply(z, weight, bias, running_mean, running_var, eps, momentum, relu) -> y = act(batch_norm(z)) on the statistics
    of the batch z [B,C,H,W] (decnet_bn_train_forward).  running_mean / running_var (both None, or both [C]) are written in
    place by the kernel, which autograd does not see: their versions are bumped, so the caches that fold the running
    statistics (stage0.source_key) rebuild on the next eval forward.  ``num_batches_tracked`` is the caller's.  Gradients:
    z, weight, bias, each only when wanted; the ReLU decision is recomputed from z, y is not saved."""

    @staticmethod
    def forward(ctx, *args):
        return bn_act_forward(ops2d.bn_train_forward, ctx, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return bn_act_backward(ops2d.bn_train_backward, ctx, gy)
