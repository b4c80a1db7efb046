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
Out of scope: training-mode BatchNorm, the stride-3 and transposed layers, stage 0, double backward.
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
    HIP kernels instead of going to the library.  Nests; ``hip_grad(False)`` switches it off inside an enabled region."""
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


def _unit_backward(ctx, gy, wgrad, dx_conv):
    """The backward of one unit, shared by the few-channel and the matrix-core Function.  wgrad(xs, gy, y, k, dil) ->
    (G, gsum, gm): the weight-gradient entry; dx_conv(gm, wt, k, dil) -> conv(gm, wt) for wt [n, Cout, k, k]: the
    forward entry on the flipped weights."""
    w, scale, y = ctx.saved_tensors[:3]
    xs = ctx.saved_tensors[3:]
    need_w, need_scale, need_shift = ctx.needs_input_grad[4:7]
    need_parts = ctx.needs_input_grad[7:]
    gy = gy.contiguous()
    w32, s32 = w.detach().float().contiguous(), scale.detach().float()
    dw = dscale = dshift = None
    if need_w or need_scale:
        G, gsum, gm = wgrad(xs, gy, y, ctx.k, ctx.dil)
        if need_w:
            dw = G * s32.view(-1, 1, 1, 1)
        if need_scale:
            dscale = (w32.double() * G.double()).sum((1, 2, 3)).float()
        if need_shift:
            dshift = gsum
    else:                                   # no weight gradient wanted: the mask and the sum alone
        gm = gy if y is None else torch.ops.aten.threshold_backward(gy, y, 0)
        if need_shift:
            dshift = gm.sum((0, 2, 3), dtype=torch.float64).float()
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


def _save(ctx, k, dil, relu, w, scale, y, xs):
    need_g = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
    ctx.k, ctx.dil, ctx.relu, ctx.cins = k, dil, relu, [int(t.shape[1]) for t in xs]
    ctx.save_for_backward(w, scale, y if relu else None, *(xs if need_g else ()))


def _dx_small(gm, wt, k, dil):
    n, co = wt.shape[0], wt.shape[1]
    return ops2d.conv2d_bn_act(gm, ops2d.conv2d_pack_weight(wt, False), torch.ones(n, device=gm.device),
                               torch.zeros(n, device=gm.device), co, k, dil, 0)


def _dx_mfma(gm, wt, k, dil):
    n, co = wt.shape[0], wt.shape[1]
    return ops2d.conv2d_mfma_cat_bn_act([gm], ops2d.conv2d_mfma_pack_weight(wt, co, k), torch.ones(n, device=gm.device),
                                        torch.zeros(n, device=gm.device), co, k, dil, 0)


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
