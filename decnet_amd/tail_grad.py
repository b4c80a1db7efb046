"""Forward and backward of the full-resolution tail on HIP under ``hip_grad()``: the warp of Refinement and the head and
tail of DynamicUpsampling (gathers, csrc/tail_grad.hip); SoftAttention's sigmoid + blend, with or without its soft mask, and
the squared difference and sigmoid / threshold tail of GenerateSparseMask's detail map (passes of csrc/detail_grad.hip).

Each Function runs the entry that inference runs (``decnet_warp_disparity``, ``decnet_unfold3_cat``,
``decnet_dynamic_upsample3``; the blend is the statement sequence of ``decnet_conv2d_cat_epilogue``'s epilogue 1), so a
module under ``hip_grad()`` computes the bits of its ``torch.no_grad()`` forward.  Every backward is a gather in a fixed
order -- no atomics, the gradient of ``right`` included -- launches only what ``ctx.needs_input_grad`` asks for, and can be
captured into a ``GraphedStep``.  model.py decides where they are taken (``model.tail_grad_route`` and its callers).
Out of scope: double backward.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops2d
from ._lib import DecnetHipError, UNSUPPORTED


def _grid_sample_grad_right(right, disp, gout):
    """g_right on torch's route (a width the HIP gather does not cover): the warp as model.warp_by_disparity builds it."""
    B, C, H, W = right.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=right.dtype, device=right.device),
                            torch.arange(W, dtype=right.dtype, device=right.device), indexing="ij")
    cx = (xs.unsqueeze(0) - disp) / ((W - 1.0) / 2.0) - 1.0
    cy = (ys / ((H - 1.0) / 2.0) - 1.0).unsqueeze(0).expand_as(cx)
    with torch.enable_grad():
        r = right.detach().requires_grad_()
        out = F.grid_sample(r, torch.stack((cx, cy), 3), mode="bilinear", padding_mode="zeros", align_corners=False)
        return torch.autograd.grad(out, r, gout)[0]


class WarpDisparityFunction(Function):
    """apply(right [B,C,H,W], disp [B,H,W]) -> the warp of model.warp_by_disparity (decnet_warp_disparity)."""

    @staticmethod
    def forward(ctx, right, disp):
        right, disp = right.contiguous(), disp.contiguous()
        out = ops2d.warp_disparity(right, disp)
        ctx.save_for_backward(right, disp)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        right, disp = ctx.saved_tensors
        want_r, want_d = ctx.needs_input_grad
        if not (want_r or want_d):
            return None, None
        gout = gout.contiguous()
        try:
            return ops2d.warp_disparity_backward(right, disp, gout, want_r, want_d)
        except DecnetHipError as e:                     # wider than the g_right gather's LDS plan: torch for that one
            if e.code != UNSUPPORTED or not want_r:
                raise
        gd = ops2d.warp_disparity_backward(right, disp, gout, False, True)[1] if want_d else None
        return _grid_sample_grad_right(right, disp, gout), gd


class Unfold3CatFunction(Function):
    """apply(fea [B,C,3h,3w], disp [B,h,w]) -> cat(disp, unfold(fea, 3, stride 3)) [B,9C+1,h,w] (decnet_unfold3_cat)."""

    @staticmethod
    def forward(ctx, fea, disp):
        return ops2d.unfold3_cat(fea.contiguous(), disp.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        want_f, want_d = ctx.needs_input_grad
        g = g.contiguous() if want_f else g
        return (ops2d.fold3(g) if want_f else None), (g[:, 0] if want_d else None)


class DynamicUpsample3Function(Function):
    """apply(logits [B,81,h,w], disp [B,h,w]) -> [B,3h,3w] (decnet_dynamic_upsample3)."""

    @staticmethod
    def forward(ctx, logits, disp):
        logits, disp = logits.contiguous(), disp.contiguous()
        ctx.save_for_backward(logits, disp)
        return ops2d.dynamic_upsample3(logits, disp)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        logits, disp = ctx.saved_tensors
        want_l, want_d = ctx.needs_input_grad
        if not (want_l or want_d):
            return None, None
        gl, gd = ops2d.dynamic_upsample3_backward(logits, disp, gout.contiguous(), want_d)
        return (gl if want_l else None), gd


def _blend_backward(ctx, backward, *grads):
    """Both blend Functions' backward; `backward`: the ops2d wrapper of the Function's own entry (a grad may be None)."""
    o, a, b = ctx.saved_tensors
    want_o, want_a, want_b = ctx.needs_input_grad
    if all(g is None for g in grads) or not (want_o or want_a or want_b):
        return None, None, None
    want_a, want_b = want_a and grads[0] is not None, want_b and grads[0] is not None   # (the soft mask does not read them)
    go, ga, gb = backward(o, a, b, *[None if g is None else g.contiguous() for g in grads], want_a, want_b)
    return (go if want_o else None), ga, gb


class SigmoidBlendFunction(Function):
    """apply(o, a, b) -> a * (1 - sigmoid(o)) + sigmoid(o) * b, planes of one shape (decnet_sigmoid_blend)."""

    @staticmethod
    def forward(ctx, o, a, b):
        o, a, b = o.contiguous(), a.contiguous(), b.contiguous()
        ctx.save_for_backward(o, a, b)
        return ops2d.sigmoid_blend(o, a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        return _blend_backward(ctx, ops2d.sigmoid_blend_backward, gout)


class SquaredDiffFunction(Function):
    """apply(a, b) -> (a - b) * (a - b), tensors of one shape (decnet_sqdiff): torch's bits, forward and backward."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return ops2d.sqdiff(a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        want_a, want_b = ctx.needs_input_grad
        if not (want_a or want_b):
            return None, None
        return ops2d.sqdiff_backward(a, b, gout.contiguous(), want_a, want_b)


class DetailTailFunction(Function):
    """apply(logits [B,H,W], thold, want_bits) -> (prob = sigmoid(logits), mask = prob > thold as float 0/1, bits: the mask
    as 64 pixels per int64 word, or None) (decnet_detail_tail).  Only ``prob`` carries a gradient."""

    @staticmethod
    def forward(ctx, logits, thold, want_bits):
        logits = logits.contiguous()
        ctx.save_for_backward(logits)
        prob, mask, bits = ops2d.detail_tail(logits, thold, True, True, bool(want_bits))
        ctx.mark_non_differentiable(*((mask,) if bits is None else (mask, bits)))
        return prob, mask, bits

    @staticmethod
    @once_differentiable
    def backward(ctx, g_prob, g_mask, g_bits):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        logits, = ctx.saved_tensors
        return ops2d.detail_tail_backward(logits, g_prob.contiguous()), None, None


class SigmoidBlendSoftFunction(Function):
    """apply(o, a, b) -> (a * (1 - s) + s * b, s), s = sigmoid(o) (decnet_sigmoid_blend_soft): SigmoidBlendFunction's blend,
    bit for bit, and the soft mask beside it.  An output that nobody differentiates costs no gradient tensor."""

    @staticmethod
    def forward(ctx, o, a, b):
        o, a, b = o.contiguous(), a.contiguous(), b.contiguous()
        ctx.save_for_backward(o, a, b)
        ctx.set_materialize_grads(False)
        return ops2d.sigmoid_blend_soft(o, a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, gsoft):
        return _blend_backward(ctx, ops2d.sigmoid_blend_soft_backward, gout, gsoft)
