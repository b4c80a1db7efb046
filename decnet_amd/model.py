"""Inference graph around the hot path: this repo's counterpart of
``modules/SparseDenseNetRefinementMask.py:102-236`` and ``modules/__init__.py:7-19``.

Only the per-stage loop matters here: it is what calls the MI355X kernels (stage 0:
``Stage0`` = cost volume + Conv3d aggregation + soft-argmax; stages 1..3: the fused
SpaMat/SpaVar launch).  The 2-D convolution blocks either side of the path (feature extractor,
mask generator, dynamic upsampling, soft attention, refinement -- ``modules/submodule.py:245-372,
566-604, 666-762``) are stock convolutions and run as PyTorch-ROCm (MIOpen) ops; they are declared
from small spec tables below with the reference's attribute names, so a reference checkpoint
(``--resume``, demo.py:124-133) loads key-for-key.

Inference only (``model.eval()``, ``torch.no_grad()``): the reference's training entry point is
not runnable as shipped.
"""
import math
import os
import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops2d
from .conv2d_grad import (BatchNormActFunction, Conv2dMfmaFunction, Conv2dS3Function, Conv2dSmallFunction, Deconv2dS3Function,
                          hip_grad_enabled)
from .tail_grad import (DetailTailFunction, DynamicUpsample3Function, SigmoidBlendFunction, SigmoidBlendSoftFunction,
                        SquaredDiffFunction, Unfold3CatFunction, WarpDisparityFunction)
from ._lib import DecnetHipError, UNSUPPORTED
from .ops import spamatvar_forward, spamatvar_forward_bits
from .stage0 import (CachesWeights, CostRegNetNoDown, Stage0, cache_attrs, drop_weight_caches, fold_bn, fold_none,  # noqa: F401
                     source_hold, source_key)
from .stage0_grad import bn_train_refusal


# bench.py's end-to-end accounting: a list that every Unit launch appends (kernel family, algorithmic flops, algorithmic
# bytes) to while it is set; None (the default) costs one comparison per layer.
TALLY = None


def _tally(unit, kind, x):
    """Algorithmic work of one Conv2dUnit / Deconv2dUnit launch: flops = 2 * outputs * Cin * taps per output, bytes = the
    input and output tensors once (fp32); the concatenated inputs count as what they are, never as a copy."""
    xs = x if isinstance(x, (tuple, list)) else (x,)
    B, _, H, W = xs[0].shape
    cin = sum(t.shape[1] for t in xs)
    c = unit.conv
    k, st, co = c.kernel_size[0], c.stride[0], c.out_channels
    if isinstance(c, nn.ConvTranspose2d):
        Ho, Wo = (H - 1) * st - 2 * c.padding[0] + k, (W - 1) * st - 2 * c.padding[0] + k
        taps = (k * k) / float(st * st)                  # k 3, stride 3: every output pixel has exactly one tap
    else:
        Ho = (H + 2 * c.padding[0] - c.dilation[0] * (k - 1) - 1) // st + 1
        Wo = (W + 2 * c.padding[1] - c.dilation[1] * (k - 1) - 1) // st + 1
        taps = k * k
    TALLY.append({"family": kind, "flops": 2.0 * B * Ho * Wo * cin * co * taps,
                  "bytes": 4.0 * B * (cin * H * W + co * Ho * Wo)})


# ---- which launches the HIP trunk takes: the switches (read per call), the gate, the layer shapes ----------------------------
def conv2d_switch():
    """DECNET_CONV2D: "hip" (the default) or anything else for the library route everywhere."""
    return os.environ.get("DECNET_CONV2D", "hip") == "hip"


def mfma_switch():
    """DECNET_CONV2D_MFMA=0 keeps the matrix-core kernels out of the trunk."""
    return os.environ.get("DECNET_CONV2D_MFMA", "1") == "1"


def spamat_bits_switch():
    return os.environ.get("DECNET_SPAMAT_BITS", "1") == "1"


def hip_gate(t, training=False, fp32=True, switch=True):
    """The HIP trunk may take this tensor: on the GPU, no autograd, not `training` (the module's flag, where the site has
    one), and -- terms a site can leave out or check elsewhere -- float32 and DECNET_CONV2D=hip."""
    return (not training and t.is_cuda and not torch.is_grad_enabled() and (not fp32 or t.dtype == torch.float32) and
            (not switch or conv2d_switch()))


def tail_grad_gate(*ts):
    """The tail Functions of tail_grad.py may take these tensors: inside ``hip_grad()`` with autograd on, all on the GPU
    in float32.  (CPU tensors: False before any library lookup.)"""
    return (hip_grad_enabled() and torch.is_grad_enabled() and
            all(t.is_cuda and t.dtype == torch.float32 for t in ts))


def _tail_shape(op, B, C, H, W, s=3, fea_hw=None):
    """The shapes the "warp", "unfold" and "upsample" entries take (arguments as tail_grad_route's): one answer for the
    inference branch of the op and for its route under ``hip_grad()``."""
    if op == "warp":
        return H > 1 and W > 1 and H <= 65535
    if op == "unfold":
        return s == 3 and H <= 65535 and B * (C + 1) <= 65535 and tuple(fea_hw) == (3 * H, 3 * W)
    if op == "upsample":
        return s == 3 and H <= 65535
    raise ValueError("no such op: %s" % op)


def tail_grad_route(op, B, C, H, W, s=3, fea_hw=None):
    """Whether `op` ("warp", "unfold", "upsample", "sqdiff", "detail") runs as its tail_grad Function under ``hip_grad()``:
    the shape limits of the inference route of the same op, decided with the switches at their defaults (as
    Unit._grad_route).  A function of sizes alone: no tensor, no GPU.  warp: right [B,C,H,W]; unfold: fea [B,C,*fea_hw],
    disp [B,H,W], down-scale s; upsample: disp [B,H,W] (C is not looked at); sqdiff: two tensors [B,C,H,W] (the flat
    entry's 2^40 floats); detail: logits [B,H,W] (C is not looked at; the limits of decnet_detail_mask) -- both less the
    sizes measured slower than the torch ops they replace (_detail_slower)."""
    if op == "sqdiff":
        return 1 <= B * C * H * W <= 1 << 40 and not _detail_slower(B * H * W)
    if op == "detail":
        return (1 <= B <= 65535 and 1 <= H <= 65535 and 1 <= W <= 1 << 28 and
                float(B) * H * ((W + 1023) // 1024) < 2.0e9 and not _detail_slower(B * H * W))
    return _tail_shape(op, B, C, H, W, s, fea_hw)


def _detail_slower(n):
    """The sizes (n = B H W, the pixels of the detail map over the batch) at which GenerateSparseMask.detail keeps its tail
    in torch ops under ``hip_grad()``: those where forward + backward through SquaredDiffFunction and DetailTailFunction was
    measured slower than the same module with `d * d`, sigmoid, clone and two masked fills -- eager, B = 4, one run
    (tools/bench_detail_grad.py, profiles/detail_grad.json; torch's time over ours, in brackets as GraphedStep replays).
      * n = 4 x 60 x 108 = 25920: train mode 0.95 (1.04), eval mode 1.03 (1.02); n = 4 x 180 x 324 = 233280: 0.98 (1.01) and
        0.98 (1.03).  An eager step of the generator is bound by the host there (0.92 - 1.44 ms whatever the size: dozens
        of small launches), and two Function calls through ctypes cost the host more than the ten torch ops they replace; the kernels
        themselves win (every replay is faster).  The eager verdict decides, as for _bn_train_slower, and is carried up to the
        next measured size.
      * n = 4 x 540 x 972 = 2099520: 1.00 (1.02) and 1.01 (1.02): from there on the Functions.
    Below 25920 pixels nothing is excluded (nothing was measured there): the tests run there."""
    return 25920 <= n < 2099520


def _mfma_grad_slower(cin, cout, hw):
    """The "mfma" shapes that stay on the library under ``hip_grad()``: those whose forward + backward was measured slower
    than (or level with) the library's under autograd -- eager, B = 4, one run (tools/bench_conv2d_mfma_grad.py,
    profiles/conv2d_mfma_grad.json).  Only two sizes were measured, the model's levels 60 x 108 (6480 pixels) and
    180 x 324 (58320 pixels); the rule looks at channels and pixels, not at B.
      * At 6480 pixels every unit was slower (72 -> 72, 144 -> 72, 217 -> 81, 81 -> 81, 76 -> 8: 0.52 - 0.98 of the
        library's speed eager, 0.65 - 1.00 as GraphedStep replays).  That verdict is carried up to the next measured size,
        58320 pixels, where units were first measured faster; nothing between the two was measured.
      * At 58320 pixels the units with at most 24 inputs and 24 outputs were slower eager (24 -> 24: 0.74 with k 3, 0.63
        with k 1) although faster as replays (1.42, 1.90): an eager step of one unit is some 25 small launches and is bound
        by the host.  They stay on the library from 6480 pixels on; the wider units there are 1.30 - 1.32 x the library.
    Below 6480 pixels nothing is excluded: the route's floor is the forward's (4096 pixels), where the tests of the Function
    run.  No layer of the model has such a shape at config 5; measured at 1 x 64 x 64, 24 -> 24 and 73 -> 81 are 0.54 and
    0.56 of the library's speed (0.51 and 0.43 as replays), so a caller with images that small gains nothing there."""
    return hw >= 6480 and (hw < 58320 or (cin <= 24 and cout <= 24))


def _s3_grad_slower(route, cin, cout, n):
    """The stride-3 shapes ("s3" / "deconv"; n = B H W, the pixels of the unit's INPUT over the batch) that stay on the
    library under ``hip_grad()``: those whose forward + backward was measured slower than (or level with) the library's
    under autograd -- eager, one run (tools/bench_conv2d_s3_grad.py, profiles/conv2d_s3_grad.json: the nine stride-3 units
    of the model at config 5, B = 8 in the extractor, B = 4 in the mask generators; speed relative to the library eager,
    in brackets as GraphedStep replays).
      * "s3": conv1[0] (8 -> 24, n = 8 x 540 x 972, the few-channel forward) is 2.51 x the library (2.70) and stays.  The
        units with more than 24 outputs (forward route "mfma_s3") were slower at both measured sizes -- conv3_1 72 -> 216 at
        n = 8 x 6480 = 51840: 0.57 (0.79); conv2[0] 24 -> 72 at n = 8 x 58320: 0.61 (1.16) -- and go back to the library from
        51840 pixels on.
      * "deconv": with 72 or more inputs, slower from the smallest measured size up to the first one measured faster --
        GenerateSparseMask(72).deconv[0] 216 -> 8 at n = 4 x 720 = 2880: 0.75 (0.70); deconv3.deconv 216 -> 72 at 5760: 0.64
        (0.88); GenerateSparseMask(24).deconv[0] 72 -> 8 at 25920: 0.90 (0.89); then deconv2.deconv 72 -> 24 at 51840: 1.53
        (1.56).  The 24-input units stay: deconv1.deconv 24 -> 8 at 8 x 58320: 6.57 (6.74), GenerateSparseMask(8).deconv[0]
        at 4 x 58320: 1.57 (1.60).
    Below the smallest measured n nothing is excluded (nothing was measured there): the routes' floors are the forwards',
    where the tests of the Functions run.  An eager step of one unit is some 20 small launches and is bound by the host
    at the small sizes, so a caller with one small image gains nothing there."""
    if route == "s3":
        return cout > 24 and n >= 51840
    return cin >= 72 and 2880 <= n < 51840


def _bn_train_slower(route, cin, cout, dil, n):
    """The units (route: the eval-mode decision of Unit._grad_route_train; dil: the dilation; n = B H W, the pixels of the
    unit's INPUT over the batch) that stay on the library in ``.train()`` mode under ``hip_grad()``: those whose forward +
    backward was measured slower than the library's conv -> batch norm -> ReLU under autograd -- eager, one run
    (tools/bench_bn_train.py, profiles/bn_train.json: every Unit of the model at config 5's sizes, B = 8 in the extractor,
    B = 4 elsewhere; speed relative to the library eager, in brackets as GraphedStep replays).
      * "conv" without dilation: all eleven units measured at the two smaller sizes were slower eager -- at n = 4 x 60 x 108
        = 25920 (8 -> 3, 3 -> 3, 3 -> 1 of the mask generator, 8 -> 8, 8 -> 1 of the attention): 0.44 - 0.54 (0.42 - 0.71);
        at n = 4 x 180 x 324 = 233280 (the same five and 12 -> 12 of the refinement): 0.54 - 0.88 (1.12 - 1.94): an eager
        step of one unit is bound by the host at 0.31 - 0.43 ms whatever the size (some 14 small launches, the route's own
        fills and repacks among them), against the library's 0.14 - 0.27 ms.  That verdict is carried up to the next
        measured size, 4 x 540 x 972 = 2099520 pixels, where the fifteen units measured (there and at 8 x 540 x 972) are
        2.68 - 7.22 x the library (3.13 - 7.26): a ninefold span in which nothing was measured.  The one dilated unit at
        those sizes, 12 -> 12 with dilation 6 at 233280, was 1.06 (1.32) -- the library's dilated convolution is slower --
        and stays.
      * "mfma" (48 -> 24 at 8 x 180 x 324, 49 -> 24, 73 -> 81, 81 -> 81 at 4 x 180 x 324): 1.25 - 1.94 (1.25 - 1.94);
        "s3" (8 -> 24 at 8 x 540 x 972): 2.57 (2.59); "deconv" (72 -> 24 at 8 x 60 x 108, 24 -> 8 at 8 x 180 x 324): 1.36, 6.43
        (1.56, 6.52): none goes back.  The units the eval-mode exclusions (_mfma_grad_slower, _s3_grad_slower) keep on the
        library were not measured in train mode and stay there.
    Below 25920 pixels nothing is excluded (nothing was measured there): the floor is the forward route's, where the tests
    run; a caller with one small image is bound by the host there and gains nothing."""
    return route == "conv" and dil == 1 and 25920 <= n < 2099520


_GRAD_FAMILY = {"conv": "conv_grad", "mfma": "mfma_grad", "s3": "s3_grad", "deconv": "deconv_grad"}


def _same_padded(c):
    """Conv2d k 1 or 3, stride 1, zero padding that keeps the size at its (square) dilation."""
    return (isinstance(c, nn.Conv2d) and c.kernel_size in ((1, 1), (3, 3)) and c.stride == (1, 1) and
            c.dilation[0] == c.dilation[1] and c.padding == (c.dilation[0] * (c.kernel_size[0] // 2),) * 2 and
            c.groups == 1 and c.padding_mode == "zeros")


def _k3s3p1(c):
    return (isinstance(c, nn.Conv2d) and c.kernel_size == (3, 3) and c.stride == (3, 3) and c.padding == (1, 1) and
            c.dilation == (1, 1) and c.groups == 1 and c.padding_mode == "zeros")


def _deconv_k3s3(c):
    return (isinstance(c, nn.ConvTranspose2d) and c.kernel_size == (3, 3) and c.stride == (3, 3) and c.padding == (0, 0) and
            c.output_padding == (0, 0) and c.dilation == (1, 1) and c.groups == 1)


class Unit(CachesWeights, nn.Module):
    """conv / transposed conv -> optional BatchNorm2d -> optional ReLU; attributes ``conv`` and
    ``bn`` as in the reference's Conv2dUnit / Deconv2dUnit (submodule.py:15-87)."""
    _CACHE_ATTRS = cache_attrs("_fold", "_mfold", "_tfold")

    def __init__(self, cin, cout, k, stride=1, pad=0, dil=1, relu=True, bn=True, momentum=0.1,
                 transposed=False):
        super().__init__()
        if transposed:
            self.conv = nn.ConvTranspose2d(cin, cout, k, stride=stride, padding=pad, bias=not bn)
        else:
            self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=not bn)
        self.bn = nn.BatchNorm2d(cout, momentum=momentum) if bn else None
        self.relu = relu

    # ---- fused HIP path for the full-resolution few-channel layers (csrc/conv2d_small.hip) ----
    def _hip_kind(self, x):
        """"conv" / "deconv" / "conv_s3" / "mfma" / "mfma_s3" / "mfma_deconv" when this unit, in eval mode on the GPU, is one
        the HIP kernels cover; else None.  x: a tensor, or a tuple of tensors standing for their channel concatenation."""
        parts = None
        if isinstance(x, (tuple, list)):
            parts, x0 = len(x), x[0]
            if any(t.shape[0] != x0.shape[0] or t.shape[2:] != x0.shape[2:] or t.dtype != x0.dtype or
                   t.device != x0.device for t in x):
                return None
            x = x0
        if not hip_gate(x, self.training, switch=False):
            return None
        return self._route(x.shape[0], x.shape[-2], x.shape[-1], parts)

    def _route(self, B, H, W, parts=None, switches=None):
        """The table behind _hip_kind, a function of the layer, the input size, the number of concatenated parts (None:
        one tensor) and the two switches alone: no tensor, no GPU.  (No threshold depends on B today.)
        switches: (conv2d_switch(), mfma_switch()) to decide with, None: as the environment has them."""
        c, hw = self.conv, H * W
        ci, co, tr = c.in_channels, c.out_channels, isinstance(c, nn.ConvTranspose2d)
        conv_on, mfma_on = (conv2d_switch(), mfma_switch()) if switches is None else switches
        if not conv_on or (parts is not None and (parts > 6 or not _same_padded(c))):          # (the `cat` entries are
            return None                                                                        # "conv"'s and "mfma"'s)
        if mfma_on:
            # many channels: the bf16x3 matrix-core kernel (csrc/conv2d_mfma.hip) where the image gives it enough
            # workgroups (>= 4096 pixels, e.g. the 60 x 108 level; at 20 x 36 the library's kernels win)
            # (round 3: also 9..23 outputs from >= 16 inputs.  The 20 x 36 level stays on the library: measured with the
            # pixel threshold at 512, 649 -> 81 takes 0.265 ms here against 0.107 ms, the 864 / 432 -> 216 1 x 1 layers
            # 0.131 / 0.081 against 0.053 / 0.042 -- 144 workgroups of a K = 5841 reduction each do not fill 256 CUs)
            if (co >= 9 or ci >= 48) and ci >= 16 and hw >= 4096 and c.dilation[0] <= 4 and _same_padded(c):
                return "mfma"
            # Conv2d k 3, stride 3, padding 1 with more than 24 outputs: space-to-depth + the same kernel as a 1 x 1 convolution
            if co > 24 and ci >= 8 and hw >= 4608 and _k3s3p1(c):
                return "mfma_s3"
            # transposed convolution k = 3, stride 3 with more than 8 output channels: the same kernel, as a 1 x 1
            # convolution to 9 Cout channels with a pixel-shuffle store
            if tr and (co > 8 or ci >= 64) and ci >= 16 and hw >= 512 and _deconv_k3s3(c):
                return "mfma_deconv"
        # the few-channel kernels at every size (at 60 x 108 and 20 x 36 they do not fill the chip, but one launch
        # replaces the library's convolution + layout transposes + bias / ReLU passes)
        if hw * (9 if tr else 1) < 256:
            return None
        if co <= 24 and c.stride == (3, 3) and _k3s3p1(c):
            return "conv_s3"
        # 9..24 output channels: only where the library is slow (dilated taps) or the input is thin
        if co > (8 if tr else 24) or (co > 8 and c.dilation[0] == 1 and ci > 12):
            return None
        if tr:
            return "deconv" if _deconv_k3s3(c) else None
        return "conv" if _same_padded(c) else None

    def _grad_route(self, B, H, W, parts=None):
        """"conv" when the unit's backward runs on the HIP kernels under ``hip_grad()`` (conv2d_grad.Conv2dSmallFunction),
        else None: the layers _route sends to "conv" with the switches at their defaults, up to 24 input channels (dx is
        the same kernel with the channel roles swapped), from 256 pixels.  Pure, like _route."""
        if self.conv.in_channels > 24 or H * W < 256:
            return None
        return "conv" if self._route(B, H, W, parts, switches=(True, True)) == "conv" else None

    def _grad_route_mfma(self, B, H, W, parts=None):
        """"mfma" when the unit's backward runs on the HIP kernels under ``hip_grad()`` as conv2d_grad.Conv2dMfmaFunction,
        else None: the layers _route sends to "mfma" with the switches at their defaults, within the channel limits of
        decnet_conv2d_mfma_wgrad (224 inputs, 224 outputs), less the shapes measured slower than the library
        (_mfma_grad_slower; tools/bench_conv2d_mfma_grad.py, profiles/conv2d_mfma_grad.json).  Pure, like _route."""
        c = self.conv
        if c.in_channels > 224 or c.out_channels > 224:
            return None
        if self._route(B, H, W, parts, switches=(True, True)) != "mfma":
            return None
        return None if _mfma_grad_slower(c.in_channels, c.out_channels, H * W) else "mfma"

    def _grad_route_s3(self, B, H, W):
        """"s3" / "deconv" when the unit's backward runs on the HIP kernels under ``hip_grad()`` as
        conv2d_grad.Conv2dS3Function / Deconv2dS3Function, else None: the layers _route sends to "conv_s3" or "mfma_s3" /
        to "deconv" or "mfma_deconv" with the switches at their defaults (so from those routes' floors on), within the
        channel limits of the weight-gradient entries (224 inputs, 224 outputs), less the shapes measured slower than the
        library (_s3_grad_slower: the one threshold of the routing that looks at B, as B H W).  Pure, like _route."""
        c = self.conv
        if c.in_channels > 224 or c.out_channels > 224:
            return None
        route = {"conv_s3": "s3", "mfma_s3": "s3", "deconv": "deconv", "mfma_deconv": "deconv"}.get(
            self._route(B, H, W, None, switches=(True, True)))
        if route is None or _s3_grad_slower(route, c.in_channels, c.out_channels, B * H * W):
            return None
        return route

    def _grad_route_train(self, B, H, W, parts=None):
        """The route ("conv" / "mfma" / "s3" / "deconv") of a unit in ``.train()`` mode under ``hip_grad()``
        (_forward_grad_train: the conv Function of that route with scale 1, shift 0 and no ReLU, then
        conv2d_grad.BatchNormActFunction), else None.  Only a unit whose ``bn`` is affine, tracks its running statistics
        and has a float momentum; the route is the eval-mode decision -- _grad_route, then _grad_route_mfma, then
        _grad_route_s3, with their measured exclusions -- less the units measured slower than the library in train mode
        (_bn_train_slower).  Pure, like _route."""
        bn = self.bn
        if bn is None or bn_train_refusal(bn) is not None:
            return None
        route = self._grad_route_any(B, H, W, parts)
        c = self.conv
        if route is None or _bn_train_slower(route, c.in_channels, c.out_channels, c.dilation[0], B * H * W):
            return None
        return route

    def _grad_route_any(self, B, H, W, parts=None):
        """The eval-mode decision under ``hip_grad()``: _grad_route, then _grad_route_mfma, then (one tensor) _grad_route_s3."""
        route = self._grad_route(B, H, W, parts)
        if route is None:
            route = self._grad_route_mfma(B, H, W, parts)
        if route is None and parts is None:
            route = self._grad_route_s3(B, H, W)
        return route

    def _grad_inputs(self, x):
        """-> (the parts of x as a tuple, their number or None for a single tensor) when the HIP Functions take them: float32
        tensors [B,c_i,H,W] of one batch, size and GPU, the weights float32; else None."""
        xs = tuple(x) if isinstance(x, (tuple, list)) else (x,)
        x0 = xs[0]
        if not (x0.is_cuda and self.conv.weight.dtype == torch.float32) or any(
                t.dim() != 4 or t.dtype != torch.float32 or t.device != x0.device or t.shape[0] != x0.shape[0] or
                t.shape[2:] != x0.shape[2:] for t in xs):
            return None
        return xs, (len(xs) if isinstance(x, (tuple, list)) else None)

    def _apply_grad_route(self, route, xs, relu, scale, shift, unfolded=False):
        """The conv Function of `route` on the parts xs.  scale, shift: what the Function differentiates; unfolded: they are
        also what the forward kernel applies (constants), in place of the cache's folded BatchNorm."""
        x0, c = xs[0], self.conv
        fold = (lambda p: (p[0], scale, shift)) if unfolded else (lambda p: p)
        if route in ("s3", "deconv"):
            fwd = self._route(x0.shape[0], x0.shape[-2], x0.shape[-1], None, switches=(True, True))
            packed = fold(self._folded_mfma() if fwd.startswith("mfma") else self._folded())
            fn = Conv2dS3Function if route == "s3" else Deconv2dS3Function
            return fn.apply(fwd, packed, relu, c.weight, scale, shift, x0)
        if route == "mfma":
            return Conv2dMfmaFunction.apply(fold(self._folded_mfma()), c.kernel_size[0], c.dilation[0], relu, c.weight,
                                            scale, shift, *xs)
        return Conv2dSmallFunction.apply(fold(self._folded()), c.kernel_size[0], c.dilation[0], relu, c.weight, scale,
                                         shift, *xs)

    def _forward_grad(self, x):
        """The forward under ``hip_grad()`` with autograd on: the same kernels, the backward recorded on ours.  None
        where the unit, the input or the shape is not covered (the caller then goes on as it always did)."""
        ins = self._grad_inputs(x)
        if ins is None:
            return None
        xs, parts = ins
        x0, c = xs[0], self.conv
        route = self._grad_route_any(x0.shape[0], x0.shape[-2], x0.shape[-1], parts)
        if route is None:
            return None
        if self.bn is not None:                                         # differentiable (fold_bn's arithmetic)
            scale, shift = fold_bn(self.bn)
        else:
            scale, shift = fold_none(c)
        n_tally = None if TALLY is None else len(TALLY)
        if TALLY is not None:
            _tally(self, _GRAD_FAMILY[route], x)
        try:
            return self._apply_grad_route(route, xs, bool(self.relu), scale, shift)
        except DecnetHipError as e:                     # the grid limits of the forward kernel: the library takes it
            if e.code != UNSUPPORTED:
                raise
            if n_tally is not None:
                del TALLY[n_tally:]
            return None

    def _forward_grad_train(self, x):
        """The forward of a unit in ``.train()`` mode under ``hip_grad()`` with autograd on: the convolution as the conv
        Function of _grad_route_train (scale 1, shift 0 as constants, no ReLU: its backward launches the weight gradient
        for dW alone), then BatchNormActFunction on the statistics of the batch, which also updates the running statistics;
        ``num_batches_tracked`` is counted here.  None where the unit, the input or the shape is not covered, or ``bn``
        itself is in eval mode (the caller then goes on as it always did; nothing has been updated)."""
        ins = self._grad_inputs(x)
        if ins is None or self.bn is None or not self.bn.training or self.bn.weight.dtype != torch.float32:
            return None
        xs, parts = ins
        x0, c, bn = xs[0], self.conv, self.bn
        route = self._grad_route_train(x0.shape[0], x0.shape[-2], x0.shape[-1], parts)
        if route is None:
            return None
        ones = torch.ones(c.out_channels, device=x0.device)
        zeros = torch.zeros(c.out_channels, device=x0.device)
        n_tally = None if TALLY is None else len(TALLY)
        if TALLY is not None:
            _tally(self, _GRAD_FAMILY[route], x)
        try:
            z = self._apply_grad_route(route, xs, False, ones, zeros, unfolded=True)
        except DecnetHipError as e:                     # the grid limits of the forward kernel: the library takes it
            if e.code != UNSUPPORTED:
                raise
            if n_tally is not None:
                del TALLY[n_tally:]
            return None
        if TALLY is not None:                           # z read twice and y written once; two sums and one fma per element
            TALLY.append({"family": "bn_train", "flops": 8.0 * z.numel(), "bytes": 12.0 * z.numel()})
        y = BatchNormActFunction.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                                       bool(self.relu))
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
        return y

    def _sources(self):
        c, bn = self.conv, self.bn
        return [c.weight] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else
                             ([c.bias] if c.bias is not None else []))

    def _scale_shift(self):
        scale, shift = fold_bn(self.bn) if self.bn is not None else fold_none(self.conv)
        return scale.contiguous(), shift.contiguous()

    def _folded(self, neg_last=False):
        """Per-channel scale / shift of the eval-mode BatchNorm (or 1 / bias), cached per weight version (stage0.source_key:
        a write through ``.data`` after the first forward needs ``drop_weight_caches``).
        neg_last: the weights of the last input channel negated (a caller that feeds -x passes x instead)."""
        def build():
            w = self.conv.weight.detach().float().contiguous()
            if neg_last:
                w = w.clone()
                w[:, -1] = -w[:, -1]
            return (ops2d.conv2d_pack_weight(w, isinstance(self.conv, nn.ConvTranspose2d)),) + self._scale_shift()
        return self._cached("_fold", self._sources(), (self.bn.eps if self.bn is not None else None, bool(neg_last)), build)

    def _folded_mfma(self):
        """Weights split into bf16 terms in the operand layout of csrc/conv2d_mfma.hip + folded BN, cached per version
        (stage0.source_key: a write through ``.data`` after the first forward needs ``drop_weight_caches``)."""
        def build():
            c = self.conv
            w = c.weight.detach().float().contiguous()
            if isinstance(c, nn.ConvTranspose2d):
                return (ops2d.deconv2d_mfma_pack_weight(w),) + self._scale_shift()
            s3 = c.stride == (3, 3)                                 # stride-3: [Cout, Cin, 3, 3] read as [Cout, 9 Cin]
            return (ops2d.conv2d_mfma_pack_weight(w, 9 * c.in_channels, 1) if s3 else
                    ops2d.conv2d_mfma_pack_weight(w, c.in_channels, c.kernel_size[0]),) + self._scale_shift()
        return self._cached("_mfold", self._sources(), (self.bn.eps if self.bn is not None else None,), build)

    def _folded_torch(self):
        """Eval-mode BatchNorm folded into the convolution itself (w * scale per output channel, bias =
        shift) for the layers that stay on MIOpen: one kernel instead of conv + batch-norm.  Cached per version
        (stage0.source_key: a write through ``.data`` after the first forward needs ``drop_weight_caches``)."""
        def build():
            scale, shift = fold_bn(self.bn, fp32=False)
            shape = (1, -1, 1, 1) if isinstance(self.conv, nn.ConvTranspose2d) else (-1, 1, 1, 1)
            return (self.conv.weight * scale.view(shape)).contiguous(), shift.contiguous()
        return self._cached("_tfold", self._sources(), (self.bn.eps,), build)

    def _forward_mfma(self, x):
        c, xs = self.conv, [t.contiguous() for t in (x if isinstance(x, (tuple, list)) else (x,))]
        return ops2d.conv2d_mfma_cat_bn_act(xs, *self._folded_mfma(), c.in_channels, c.kernel_size[0], c.dilation[0],
                                            1 if self.relu else 0)

    def _forward_hip(self, x, kind, out=None, epi=0, ea=None, eb=None, neg_last=False):
        """out: write into this [B,Cout,H,W] buffer (kind "conv"); epi / ea / eb: decnet_conv2d_cat_epilogue's fused tail
        of a single-output layer; neg_last: see _folded."""
        if TALLY is None:
            return self._forward_hip_kind(x, kind, out, epi, ea, eb, neg_last)
        n_tally = len(TALLY)
        _tally(self, kind, x)
        try:
            return self._forward_hip_kind(x, kind, out, epi, ea, eb, neg_last)
        except DecnetHipError:                           # forward() falls back to the library path and tallies THAT
            del TALLY[n_tally:]
            raise

    def _forward_hip_kind(self, x, kind, out, epi, ea, eb, neg_last):
        c, relu = self.conv, 1 if self.relu else 0
        ci, k, dil = c.in_channels, c.kernel_size[0], c.dilation[0]
        if kind == "mfma":
            return self._forward_mfma(x)
        if kind == "mfma_deconv":
            return ops2d.deconv2d_mfma_k3s3_bn_act(x.contiguous(), *self._folded_mfma(), ci, relu)
        if kind == "mfma_s3":       # Conv2d k 3, stride 3, padding 1: decnet_s2d3_pad1 + the matrix-core kernel as a 1 x 1 conv
            return ops2d.conv2d_mfma_cat_bn_act([ops2d.s2d3_pad1(x.contiguous())], *self._folded_mfma(), 9 * ci, 1, 1, relu)
        wss = self._folded(neg_last)
        if isinstance(x, (tuple, list)) or epi:         # concatenated input, never materialised
            xs = [t.contiguous() for t in (x if isinstance(x, (tuple, list)) else (x,))]
            if epi:
                return ops2d.conv2d_cat_epilogue(xs, *wss, ci, k, dil, relu, epi, ea, eb, out=out)
            return ops2d.conv2d_cat_bn_act(xs, *wss, ci, k, dil, relu, out=out)
        if kind == "conv_s3":
            return ops2d.conv2d_k3s3_bn_act(x.contiguous(), *wss, ci, relu)
        if kind == "deconv":
            return ops2d.deconv2d_k3s3_bn_act(x.contiguous(), *wss, ci, relu)
        return ops2d.conv2d_bn_act(x.contiguous(), *wss, ci, k, dil, relu, out=out)

    def forward(self, x):
        if hip_grad_enabled() and torch.is_grad_enabled():
            # (without bn the training flag changes nothing: the eval route, and its bits.  A training unit whose bn was put
            # into eval mode -- frozen statistics inside model.train() -- goes on as it always did: the library's
            # convolution and bn(x) on the running statistics, nothing written)
            if not self.training or self.bn is None:
                y = self._forward_grad(x)
            else:
                y = self._forward_grad_train(x) if self.bn.training else None
            if y is not None:
                return y
        kind = self._hip_kind(x)
        if kind is not None:
            try:
                return self._forward_hip(x, kind)
            except DecnetHipError as e:                 # e.g. LDS budget / grid limits of the matrix-core kernel
                if e.code != UNSUPPORTED:
                    raise
        if TALLY is not None:
            _tally(self, "library", x)
        if isinstance(x, (tuple, list)):
            x = torch.cat(tuple(x), 1)
        if self.bn is not None and hip_gate(x, self.training, fp32=False, switch=False):
            w, b = self._folded_torch()
            c = self.conv
            if isinstance(c, nn.ConvTranspose2d):
                x = F.conv_transpose2d(x, w, None, c.stride, c.padding, c.output_padding, c.groups, c.dilation)
            else:
                x = F.conv2d(x, w, None, c.stride, c.padding, c.dilation, c.groups)
            # bias + ReLU in one in-place pass (the library would add the bias in a kernel of its own)
            if x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] * x.shape[1] <= 65535:
                return ops2d.bias_act_inplace(x, b, 1 if self.relu else 0)
            x = x + b.view(1, -1, 1, 1)
            return torch.relu_(x) if self.relu else x
        if self.bn is not None and not self.training and x.is_cuda and hip_grad_enabled() and torch.is_grad_enabled():
            # a unit that stays on the library under hip_grad(): the arithmetic of the no_grad route above (BatchNorm folded
            # into the weights, then bias and ReLU), as differentiable torch ops -- the forward keeps the inference
            # forward's bits, like the units on the HIP Functions beside it
            scale, shift = fold_bn(self.bn, fp32=False)
            c = self.conv
            if isinstance(c, nn.ConvTranspose2d):
                x = F.conv_transpose2d(x, (c.weight * scale.view(1, -1, 1, 1)).contiguous(), None, c.stride, c.padding,
                                       c.output_padding, c.groups, c.dilation)
            else:
                x = F.conv2d(x, (c.weight * scale.view(-1, 1, 1, 1)).contiguous(), None, c.stride, c.padding, c.dilation,
                             c.groups)
            x = x + shift.view(1, -1, 1, 1)
            return torch.relu(x) if self.relu else x
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return F.relu(x) if self.relu else x


# masks_of(): both views' mask generators as one batch up to this many bytes of level features (see there)
TWO_VIEW_MASK_BYTES = 96 << 20

_SIDE = threading.local()


def _side_stream(device):
    """One extra HIP stream per (host thread, device): DataParallel drives replicas from worker threads."""
    d = getattr(_SIDE, "streams", None)
    if d is None:
        d = _SIDE.streams = {}
    key = torch.device(device).index
    if key not in d:
        d[key] = torch.cuda.Stream(device=device)
    return d[key]


def _seq(*units):
    return nn.Sequential(*units)


def _c3(cin, cout, **kw):
    return Unit(cin, cout, 3, pad=kw.pop("pad", 1), **kw)


class UpBlock(nn.Module):
    """Deconv2dBlock (submodule.py:162-178): x3 transposed conv, concat with the skip, two 3x3."""

    def __init__(self, cin, cout):
        super().__init__()
        self.deconv = Unit(cin, cout, 3, stride=3, transposed=True)
        self.conv = _seq(_c3(2 * cout, cout), _c3(cout, cout))

    def forward(self, skip, x):
        up = self.deconv(x)
        return self.conv((up, skip)), up                # Unit takes the concatenation as a tuple


class ASPP(CachesWeights, nn.Module):
    """submodule.py:225-241: a 1x1 branch and three dilated 3x3 branches, concatenated."""
    _CACHE_ATTRS = cache_attrs("_pk")

    def __init__(self, cin, cout, rates):
        super().__init__()
        self.stages = nn.Module()
        self.stages.add_module("c0", Unit(cin, cout, 1))
        for i, r in enumerate(rates):
            self.stages.add_module("c%d" % (i + 1), Unit(cin, cout, 3, pad=r, dil=r))

    # ---- fused path (csrc/tapconv.hip): one V, one batched per-tap GEMM, one gather for all branches ----
    def _hip_ok(self, x):
        return hip_gate(x, self.training, switch=False) and self._fusable(x.shape[-2], x.shape[-1])

    def _fusable(self, H, W):
        """The block's shape is one the tap-conv kernels take (a function of the layers, the image size and DECNET_CONV2D
        alone): up to four same-padded BN + ReLU branches of one Cin -> Cout, Cin % 4 == 0, Cout <= 224, <= 16384 pixels."""
        units = list(self.stages.children())
        c0 = units[0].conv
        if not conv2d_switch() or len(units) > 4 or c0.in_channels % 4 or c0.out_channels > 224 or H * W > 16384:
            return False
        return all(_same_padded(u.conv) and u.bn is not None and u.relu and u.conv.out_channels == c0.out_channels and
                   u.conv.in_channels == c0.in_channels for u in units)

    def _packed(self):
        """All branches' weights in the per-tap GEMM's layout + folded BN, cached per version (stage0.source_key: a
        write through ``.data`` after the first forward needs ``drop_weight_caches``)."""
        units = list(self.stages.children())
        ts = [t for u in units for t in (u.conv.weight, u.bn.weight, u.bn.bias, u.bn.running_mean, u.bn.running_var)]

        def build():
            ci, co = units[0].conv.in_channels, units[0].conv.out_channels
            ks = [u.conv.kernel_size[0] for u in units]
            tap0 = [sum(k * k for k in ks[:i]) for i in range(len(ks))]
            ntaps = sum(k * k for k in ks)
            u_all = torch.empty(ops2d.size("tapconv_weight_floats", ci, ntaps), dtype=torch.float32,
                                device=units[0].conv.weight.device)
            for u, t0 in zip(units, tap0):
                ops2d.tapconv_pack_weight(u.conv.weight.detach().float().contiguous(), u_all, t0)
            ops2d.tapconv_split_weight(u_all, ci, ntaps)
            torch.cuda.current_stream(u_all.device).synchronize()      # the weights' fp32 temporaries may go now
            scale, shift = zip(*[fold_bn(u.bn) for u in units])
            return dict(u=u_all, scale=torch.cat(scale).contiguous(), shift=torch.cat(shift).contiguous(), ks=ks, tap0=tap0,
                        ntaps=ntaps, dil=[u.conv.dilation[0] for u in units], co=co)
        return self._cached("_pk", ts, [u.bn.eps for u in units], build)

    def _forward_hip(self, x):
        pk = self._packed()
        x = x.contiguous()
        B, Ci, H, W = x.shape
        T = ops2d.tap_gemm(ops2d.tapconv_to_chunks(x), pk["u"], B * H * W, Ci, pk["co"], pk["ntaps"], 1)
        return ops2d.tapconv_gather(T, pk["scale"], pk["shift"], B, pk["co"], H, W, pk["tap0"], pk["ks"], pk["dil"], 1)

    def forward(self, x):
        if self._hip_ok(x):
            return self._forward_hip(x)
        return torch.cat([s(x) for s in self.stages.children()], 1)


class FeatExtNetChannelPlus(nn.Module):
    """submodule.py:245-343 for num_stage=4, down_scale in {3}: 1, 1/3, 1/9, 1/27 resolution with
    C, 3C, 9C, 27C channels; ``out_channels`` is coarse-to-fine like the reference's."""

    def __init__(self, base_channels, num_stage=4, down_scale=3):
        super().__init__()
        assert num_stage == 4 and down_scale == 3, "the shipped configuration (demo.sh / eval.sh)"
        c, s = base_channels, down_scale
        c1, c2, c3 = c * s, c * s * s, c * s ** 3
        self.conv0 = _seq(_c3(3, c), _c3(c, c))
        self.addition_trans0 = Unit(c, c, 1)
        self.conv1 = _seq(_c3(c, c1, stride=s), _c3(c1, c1), _c3(c1, c1))
        self.addition_trans1 = Unit(c1, c1, 1)
        self.deconv1 = UpBlock(c1, c)
        self.conv2 = _seq(_c3(c1, c2, stride=s), _c3(c2, c2), _c3(c2, c2))
        self.addition_trans2 = Unit(c2, c2, 1)
        self.deconv2 = UpBlock(c2, c1)
        self.conv3_1 = _c3(c2, c3, stride=s)
        self.conv3_2 = _seq(_c3(c3, c3), _c3(c3, c3))
        self.addition_ctx_collection = _seq(ASPP(c3, c3, [4, 8, 12]), Unit(4 * c3, c3, 1))
        self.addition_fusion = Unit(2 * c3, c3, 1)
        self.deconv3 = UpBlock(c3, c2)
        self.out_channels = [c3, c2, c1, c]

    def forward(self, x, x2=None):
        """x2: a second image batch (the right views); the result is that of forward(cat(x, x2)) -- every op is
        per-sample in eval mode -- without materialising the concatenation: the first convolution writes the two
        halves of one output buffer."""
        if x2 is not None:
            u0 = self.conv0[0]
            kind = u0._hip_kind(x)
            if kind == "conv" and x.shape == x2.shape:
                nb = x.shape[0]
                y = torch.empty((2 * nb, u0.conv.out_channels) + tuple(x.shape[-2:]), dtype=torch.float32, device=x.device)
                u0._forward_hip(x, kind, out=y[:nb])
                u0._forward_hip(x2, kind, out=y[nb:])
                f0 = self.conv0[1](y)
            else:
                f0 = self.conv0(torch.cat([x, x2]))
        else:
            f0 = self.conv0(x)
        f1 = self.conv1(f0)
        f2 = self.conv2(f1)
        f3a = self.conv3_1(f2)
        f3 = self.addition_fusion((self.conv3_2(f3a), self.addition_ctx_collection(f3a)))    # (the concatenation is the unit's)
        s1, _ = self.deconv3(self.addition_trans2(f2), f3)
        s2, _ = self.deconv2(self.addition_trans1(f1), s1)
        s3, _ = self.deconv1(self.addition_trans0(f0), s2)
        return {"stage0": f3, "stage1": s1, "stage2": s2, "stage3": s3}


class GenerateSparseMask(CachesWeights, nn.Module):
    """submodule.py:347-372: squared difference between the level's features and the upsampled
    previous level's, reduced to one logit per pixel."""
    _CACHE_ATTRS = cache_attrs("_hp")

    def __init__(self, in_channels, down_scale):
        super().__init__()
        self.deconv = _seq(Unit(in_channels * down_scale, 8, 3, stride=3, bn=False, transposed=True),
                           _c3(8, 3, relu=False))
        self.conv_sub = _seq(_c3(in_channels, 8, bn=False), _c3(8, 3, relu=False))
        self.conv = _seq(_c3(3, 3, relu=False), Unit(3, 1, 1, relu=False))

    def forward(self, cur, pre):
        d = self.conv_sub(cur) - self.deconv(pre)
        return self.conv(d * d).squeeze(1)

    def _host_params(self):
        """The 3x3 and 1x1 units of ``conv`` with BatchNorm folded, as host arrays (92 floats; one device ->
        host copy per weight version; stage0.source_key: a write through ``.data`` after the first forward needs
        ``drop_weight_caches``)."""
        u3, u1 = self.conv[0], self.conv[1]
        ts = [t for u in (u3, u1) for t in (u.conv.weight, u.bn.weight, u.bn.bias, u.bn.running_mean, u.bn.running_var)]

        def build():
            flat = [v for u in (u3, u1) for v in (u.conv.weight.float().reshape(-1),) + fold_bn(u.bn)]
            return ops2d.detail_mask_params(torch.cat(flat).cpu().tolist())
        return self._cached("_hp", ts, (u3.bn.eps, u1.bn.eps), build)

    def mask(self, cur, pre, thold, want_bits=False):
        """``(sigmoid(self(cur, pre)) > thold)`` as a float 0/1 plane [B,H,W] (SparseDenseNetRefinementMask.py:
        148-170).  On the GPU in eval mode the squared difference, both convolutions of ``conv``, the sigmoid
        and the threshold are one kernel (csrc/maskgen.hip).  want_bits: also the bit-packed copy the SpaMat kernels
        read."""
        if not hip_gate(cur, self.training) or cur.shape[-2] > 65535:
            m = (torch.sigmoid(self(cur, pre)) > thold).to(cur.dtype)
            return (m, None) if want_bits else m
        out, bits = ops2d.detail_mask(self.conv_sub(cur).contiguous(), self.deconv(pre).contiguous(), self._host_params(),
                                      thold, want_bits)
        return (out, bits) if want_bits else out

    def detail(self, cur, pre, thold, want_bits=False):
        """What the training forward keeps of a mask generator (SparseDenseNetRefinementMask.py:148-170) ->
        (prob, mask, bits): prob [B,H,W] = sigmoid(self(cur, pre)), with its autograd graph where autograd is on; mask =
        (prob > thold) as a float 0/1 plane without a graph (the reference thresholds under no_grad); bits: the mask as the
        bit-packed copy the SpaMat kernels read where want_bits is set and a HIP route ran, else None.

        Under ``hip_grad()`` with autograd on, in either BatchNorm mode: the units take their own routes, the squared
        difference is SquaredDiffFunction and sigmoid, threshold and bit plane are DetailTailFunction
        (csrc/detail_grad.hip).  Under ``no_grad`` in eval mode on the GPU: the one launch of mask() with its logits kept,
        and decnet_detail_tail for prob -- mask and bits are exactly mask()'s.  Otherwise torch ops.

        The composed ``hip_grad()`` route and the fused inference kernel order their arithmetic differently (separate
        convolutions with BatchNorm applied per layer against one fma chain with BatchNorm folded), so their masks may
        disagree on pixels whose probability is within rounding of thold."""
        if tail_grad_gate(cur, pre):
            c3, p3 = self.conv_sub(cur), self.deconv(pre)
            if c3.shape == p3.shape and tail_grad_gate(c3, p3) and tail_grad_route("sqdiff", *c3.shape):
                d2 = SquaredDiffFunction.apply(c3, p3)
            else:
                d = c3 - p3
                d2 = d * d
            logits = self.conv(d2).squeeze(1)
            if tail_grad_gate(logits) and tail_grad_route("detail", logits.shape[0], 1, *logits.shape[-2:]):
                return DetailTailFunction.apply(logits, thold, want_bits)
            prob = torch.sigmoid(logits)
            return prob, (prob.detach() > thold).to(prob.dtype), None
        if hip_gate(cur, self.training) and cur.shape[-2] <= 65535:
            mask, bits, logits = ops2d.detail_mask(self.conv_sub(cur).contiguous(), self.deconv(pre).contiguous(),
                                                   self._host_params(), thold, want_bits, want_logits=True)
            return ops2d.detail_tail(logits, thold, True, False, False)[0], mask, bits
        prob = torch.sigmoid(self(cur, pre))
        return prob, (prob.detach() > thold).to(prob.dtype), None


class DynamicUpsampling(nn.Module):
    """submodule.py:566-589: x3 upsampling of a disparity map with per-pixel softmax weights over
    the 3x3 neighbourhood, predicted from the finer level's features."""

    def __init__(self, in_channels, down_scale):
        super().__init__()
        self.s = down_scale
        k = down_scale ** 2 * 9
        self.pad = nn.ReplicationPad2d(1)
        self.weight_learning = _seq(_c3(in_channels * down_scale ** 2 + 1, k), _c3(k, k),
                                    _c3(k, k, relu=False))

    def forward(self, disp, fea):
        B, h, w = disp.shape
        s2 = self.s ** 2
        grad = tail_grad_gate(disp, fea)                # under hip_grad(): the same entries, the backward on ours
        if grad and tail_grad_route("unfold", B, fea.shape[1], h, w, self.s, fea.shape[-2:]):
            wts = Unfold3CatFunction.apply(fea, disp)
        elif hip_gate(fea) and _tail_shape("unfold", B, fea.shape[1], h, w, self.s, fea.shape[-2:]):
            # cat(disp, unfold(fea)) as one pass (csrc/unfold.hip)
            wts = ops2d.unfold3_cat(fea.contiguous(), disp.contiguous())
        else:
            wts = torch.cat((disp.unsqueeze(1), F.unfold(fea, self.s, stride=self.s).view(B, -1, h, w)), 1)
        logits = self.weight_learning(wts)
        if grad and tail_grad_gate(logits) and tail_grad_route("upsample", B, 81, h, w, self.s):
            return DynamicUpsample3Function.apply(logits, disp)
        if hip_gate(logits) and _tail_shape("upsample", B, 81, h, w, self.s):
            return ops2d.dynamic_upsample3(logits.contiguous(), disp.contiguous())
        wts = F.softmax(logits.view(B, s2, 9, h * w), 2)
        nb = F.unfold(self.pad(disp.unsqueeze(1)), 3).unsqueeze(1)
        up = (nb * wts).sum(2).view(B, s2, h, w)
        return (F.pixel_shuffle(up, self.s) * self.s).squeeze(1)


class SoftAttention(nn.Module):
    """submodule.py:593-604"""

    def __init__(self, in_channels, base_channels):
        super().__init__()
        self.conv = _seq(_c3(in_channels, base_channels), _c3(base_channels, base_channels),
                         _c3(base_channels, 1, relu=False))

    def forward(self, x):
        return torch.sigmoid(self.conv(x))

    def fuse(self, fea, dense, sparse, mask, var, want_soft=False):
        """The attention and the fusion of the stage loop (SparseDenseNetRefinementMask.py:195-202) in one go:
        soft = self(cat(fea, dense, sparse, mask, -var)); dense * (1 - soft) + soft * sparse.  On the GPU the
        concatenation, the negation (folded into the first layer's weights), the sigmoid and the blend are part
        of the three convolution launches.
        want_soft: -> (fused, soft), the soft mask the training loss reads; fused keeps the bits of the call without it
        (on the HIP routes the last unit then runs without its epilogue, and one pass writes both planes)."""
        parts = (fea, dense.unsqueeze(1), sparse.unsqueeze(1), mask.unsqueeze(1), var.unsqueeze(1))
        u0, u1, u2 = self.conv[0], self.conv[1], self.conv[2]
        if u2.conv.out_channels == 1 and not u2.relu and tail_grad_gate(*parts):
            y = self._fuse_grad(parts, dense, sparse, want_soft)
            if y is not None:
                return y
        k0 = u0._hip_kind(parts)
        if k0 in ("conv", "mfma") and u2.conv.out_channels == 1 and not u2.relu:
            if k0 == "conv":
                t = u0._forward_hip(parts, "conv", neg_last=True)
            else:                                       # many input channels (1/9, 1/3 resolution): matrix-core kernel
                t = u0._forward_hip(parts[:4] + (-var.unsqueeze(1),), "mfma")
            t = u1(t)
            if u2._hip_kind(t) == "conv":
                if want_soft:                           # the convolution of the epilogue entry, then the epilogue's statements
                    o = u2._forward_hip((t,), "conv").squeeze(1)
                    return ops2d.sigmoid_blend_soft(o, dense.contiguous(), sparse.contiguous())
                return u2._forward_hip(t, "conv", epi=1, ea=dense.contiguous(), eb=sparse.contiguous()).squeeze(1)
            soft = torch.sigmoid(u2(t)).squeeze(1)
            fused = dense * (1 - soft) + soft * sparse
            return (fused, soft) if want_soft else fused
        soft = self(parts[:4] + (-var.unsqueeze(1),)).squeeze(1)
        fused = dense * (1 - soft) + soft * sparse
        return (fused, soft) if want_soft else fused

    def _fuse_grad_route(self, B, H, W):
        """Whether fuse() under ``hip_grad()`` runs its three units as Conv2dSmallFunctions (the variance negated as a
        tensor: fma(-v, w, acc) and fma(v, -w, acc) are the same bits) and the blend as SigmoidBlendFunction.  Pure."""
        u0, u1, u2 = self.conv[0], self.conv[1], self.conv[2]
        return (u2.conv.out_channels == 1 and not u2.relu and u0._grad_route(B, H, W, 5) == "conv" and
                u1._grad_route(B, H, W) == "conv" and u2._grad_route(B, H, W) == "conv")

    def _fuse_grad_route_train(self, B, H, W):
        """The same in ``.train()`` mode: every unit with BatchNorm on Unit._grad_route_train's "conv" (batch statistics), one
        without as in eval mode.  Pure."""
        u0, u1, u2 = self.conv[0], self.conv[1], self.conv[2]
        route = lambda u, parts=None: (u._grad_route_train if u.bn is not None else u._grad_route)(B, H, W, parts)  # noqa: E731
        return (u2.conv.out_channels == 1 and not u2.relu and route(u0, 5) == "conv" and route(u1) == "conv" and
                route(u2) == "conv")

    def _fuse_grad(self, parts, dense, sparse, want_soft=False):
        """fuse() on the route of _fuse_grad_route (_fuse_grad_route_train in ``.train()`` mode); None where it does not
        hold (the caller goes on as it always did).  want_soft: (fused, soft) from SigmoidBlendSoftFunction."""
        B, _, H, W = parts[0].shape
        train = self.training
        if any(u.training != train or (train and u.bn is not None and not u.bn.training) for u in self.conv):
            return None                                 # (e.g. frozen BatchNorms inside a training module: the usual route)
        if not (self._fuse_grad_route_train(B, H, W) if train else self._fuse_grad_route(B, H, W)):
            return None
        n_tally = None if TALLY is None else len(TALLY)
        t = parts[:4] + (-parts[4],)
        for u in self.conv:
            y = u._forward_grad_train(t) if train and u.bn is not None else u._forward_grad(t)
            if y is None and train:                     # a grid limit of the forward kernel: this unit alone goes the usual
                y = u(t)                                # way -- the units before it have updated their running statistics
            elif y is None:                             # ... in eval mode: the usual route, from the start
                if n_tally is not None:
                    del TALLY[n_tally:]
                return None
            t = y
        if want_soft:
            return SigmoidBlendSoftFunction.apply(t.squeeze(1), dense, sparse)
        return SigmoidBlendFunction.apply(t.squeeze(1), dense, sparse)


def warp_by_disparity(right, disp):
    """Refinement.get_warped_feats_by_homgrp (submodule.py:719-745): the same stretched,
    half-pixel-shifted bilinear warp as stage 0, one disparity per pixel."""
    B, C, H, W = right.shape
    if tail_grad_gate(right, disp) and tail_grad_route("warp", B, C, H, W):
        return WarpDisparityFunction.apply(right, disp)
    if hip_gate(right) and _tail_shape("warp", B, C, H, W):
        return ops2d.warp_disparity(right.contiguous(), disp.contiguous())
    ys, xs = torch.meshgrid(torch.arange(H, dtype=right.dtype, device=right.device),
                            torch.arange(W, dtype=right.dtype, device=right.device), indexing="ij")
    cx = (xs.unsqueeze(0) - disp) / ((W - 1.0) / 2.0) - 1.0
    cy = (ys / ((H - 1.0) / 2.0) - 1.0).unsqueeze(0).expand_as(cx)
    return F.grid_sample(right, torch.stack((cx, cy), 3), mode="bilinear", padding_mode="zeros",
                         align_corners=False)


class Refinement(nn.Module):
    """submodule.py:666-762: residual disparity from (left, warped right, disparity)."""
    _DIL = {0: (1, 1, 1), 1: (1, 1, 1), 2: (2, 4, 6), 3: (3, 6, 9)}

    def __init__(self, in_channels, base_channels, stage_id=-1, down_scale=3):
        super().__init__()
        c, h = in_channels, in_channels // 2
        d0, d2, d4 = self._DIL[stage_id]
        self.conv = _seq(_c3(2 * c + 1, c, pad=d0, dil=d0), _c3(c, c), _c3(c, c, pad=d2, dil=d2),
                         _c3(c, h), _c3(h, h, pad=d4, dil=d4), _c3(h, h),
                         _c3(h, 1, relu=False, bn=False))

    def forward(self, left, right, disp):
        x = (left, warp_by_disparity(right, disp), disp.unsqueeze(1))
        last = self.conv[-1]
        if last.conv.out_channels == 1:
            t = x
            for u in list(self.conv)[:-1]:
                t = u(t)
            if last._hip_kind(t) == "conv":             # disp + res as the last layer's epilogue (reference :716)
                return last._forward_hip(t, "conv", epi=2, ea=disp.contiguous()).squeeze(1), None
            res = last(t).squeeze(1)
            return disp + res, res
        res = self.conv(x).squeeze(1)
        return disp + res, res


class SparseDenseNetRefinementMask(nn.Module):
    """Same constructor arguments and ``forward`` signature as the reference class
    (SparseDenseNetRefinementMask.py:17-99, 102); inference returns ``[pred]`` (:236)."""

    def __init__(self, max_disp=192, base_channels=8, num_stage=3, down_scale=3, step=(1, 2, 3),
                 samp_num=8, sample_spa_size_list=(-1, 3, 3, 3), down_func_name="bilinear",
                 weights=(0.2, 0.6, 1.8), grad_method="detach", cost_func="cat", if_overmask=False,
                 skip_stage_id=3, use_detail=False, thold=0.5, alpha=0.1):
        super().__init__()
        assert max_disp % down_scale ** (num_stage - 1) == 0, \
            "the max_disp({}) should be divisible by down_scale({})^num_stage({})".format(
                max_disp, down_scale, num_stage)                      # reference :42
        assert cost_func in ("ssd", "cor", "cat"), "no such cost_func: {}".format(cost_func)     # submodule.py:447
        self.max_disp, self.num_stage, self.down_scale = max_disp, num_stage, down_scale
        self.skip_stage_id, self.use_detail, self.thold = skip_stage_id, use_detail, thold
        self.feature_extractor = FeatExtNetChannelPlus(base_channels, num_stage, down_scale)
        ch = self.feature_extractor.out_channels
        self.cost_regularizer = CostRegNetNoDown(ch[0], ch[0] * 2, cost_func, down_scale)
        n = num_stage - 1
        self.detail_detection = nn.ModuleList(GenerateSparseMask(ch[i + 1], down_scale) for i in range(n))
        self.dynamic_upsampling = nn.ModuleList(DynamicUpsampling(ch[i + 1], down_scale) for i in range(n))
        self.soft_attention = nn.ModuleList(SoftAttention(ch[i + 1] + 4, base_channels) for i in range(n))
        self.refinement = nn.ModuleList(Refinement(ch[i + 1], base_channels // 2 ** i, i + 1, down_scale)
                                        for i in range(n))
        self._initialize_weights()

    def _initialize_weights(self):
        """SparseDenseNetRefinementMask.py:239-257: He-normal Conv2d / Conv3d weights (fan-out), zero conv
        biases, unit BatchNorm.  ConvTranspose2d is not a Conv2d: transposed convolutions keep PyTorch's
        default init, as in the reference.  The sub-nets above are built in the reference's order with
        the reference's layer shapes, so after ``torch.manual_seed(17)`` (demo.py:70) this yields the
        reference's from-scratch tensors bit for bit (tests/test_init_cpu.py)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.Conv3d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.kernel_size[2] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        drop_weight_caches(self)                        # the writes above go through .data: no cache key sees them

    def forward(self, left, right, disparity=None, left_mask_list=None, right_mask_list=None,
                is_check=False, is_eval=False):
        if self.training:
            raise NotImplementedError("inference only: call .eval() (SURVEY.md S11)")
        f2 = None
        if left.is_cuda and left.shape == right.shape:
            # both views in one pass (per-sample ops, eval BN: same result; the 1/9 and 1/27 layers
            # are too small at B pairs to fill 256 CUs)
            f2 = self.feature_extractor(left, right)
            nb = left.shape[0]
            lf = {k: v[:nb] for k, v in f2.items()}
            rf = {k: v[nb:] for k, v in f2.items()}
        else:
            lf = self.feature_extractor(left)
            rf = self.feature_extractor(right)
        nstage = self.num_stage

        def max_disp_of(stage):
            return self.max_disp // self.down_scale ** (nstage - stage - 1)

        def masks_of(stage):
            """reference :148-170 -> (lmask, rmask, lbits, rbits)"""
            L, R = lf["stage%d" % stage], rf["stage%d" % stage]
            if not self.use_detail:
                return left_mask_list[stage - 1], right_mask_list[stage - 1], None, None
            gen = self.detail_detection[stage - 1]
            # both views as one batch of 2 B samples where the levels are launch-bound (1/9, 1/3 resolution); at full
            # resolution a [16,8,540,972] tensor is 268 MB -- more than the 256 MiB Infinity Cache that keeps a
            # view's 134 MB intermediates on chip between producer and consumer (measured: 656 vs 608 us)
            if f2 is not None and 2 * L.numel() * 4 <= TWO_VIEW_MASK_BYTES:
                m2, b2 = gen.mask(f2["stage%d" % stage], f2["stage%d" % (stage - 1)], self.thold, want_bits=True)
                nb = L.shape[0]
                return m2[:nb], m2[nb:], (b2[:nb] if b2 is not None else None), (b2[nb:] if b2 is not None else None)
            lmask, lbits = gen.mask(L, lf["stage%d" % (stage - 1)], self.thold, want_bits=True)
            rmask, rbits = gen.mask(R, rf["stage%d" % (stage - 1)], self.thold, want_bits=True)
            return lmask, rmask, lbits, rbits

        def sparse_of(stage, masks, out=None):
            """SpaMat + (no_grad) SpaVar around its output, reference :183-192, one launch; the masks as the bit-packed
            copies the mask kernel wrote where there are any (the float planes stay what SoftAttention reads)."""
            L, R = lf["stage%d" % stage], rf["stage%d" % stage]
            lmask, rmask, lbits, rbits = masks
            D = max_disp_of(stage)
            res = None
            if lbits is not None and rbits is not None and spamat_bits_switch():
                try:
                    res = spamatvar_forward_bits(L.contiguous(), R.contiguous(), lbits, rbits, D, out=out)
                except DecnetHipError as e:             # shapes only the float-mask entry's fallback kernels cover
                    if e.code != UNSUPPORTED:
                        raise
            if res is None:
                res = spamatvar_forward(L.contiguous(), R.contiguous(), lmask.contiguous(), rmask.contiguous(), D, out=out)
            return res[0], res[1]

        # The masks and the SpaMat / SpaVar pass of EVERY level depend on the feature maps only -- not on the coarser
        # level's prediction (reference :148-192).  On the GPU they run ahead on a second HIP stream, beside the stage-0
        # Conv3d stack and the DynamicUpsampling convolutions (fp32-issue- and HBM-bound kernels beside bf16 matrix-core
        # GEMMs); the main stream picks a level's results up behind an event.
        stages = [st for st in range(1, nstage) if st < self.skip_stage_id]
        ahead = {}
        overlap = left.is_cuda and stages
        if overlap:
            cur = torch.cuda.current_stream(left.device)
            side = _side_stream(left.device)
            side.wait_stream(cur)                          # the feature maps are ready
            with torch.cuda.stream(side):
                for st in stages:
                    masks = masks_of(st)
                    sp = sparse_of(st, masks)
                    ev = torch.cuda.Event()
                    ev.record(side)
                    for t in masks + sp:                    # allocated on the side stream, consumed on the main one
                        if t is not None:
                            t.record_stream(cur)
                    ahead[st] = (masks, sp, ev)

        pred = None
        for stage in range(nstage):
            L, R = lf["stage%d" % stage], rf["stage%d" % stage]
            if stage == 0:
                # get_disp_samples -> GetCostVolume -> CostRegNetNoDown -> disparity_regression
                # (reference :127-137) as one channels-last pipeline on the matrix cores
                pred = self.cost_regularizer.stage0(L, R, max_disp_of(0))
                continue
            if stage >= self.skip_stage_id:                               # reference :143-144
                pred = F.interpolate(pred.unsqueeze(1) * self.down_scale, L.shape[-2:],
                                     mode="bicubic").squeeze(1)
                continue
            dense = self.dynamic_upsampling[stage - 1](pred, L)           # reference :178
            if overlap:
                masks, (sparse, var), ev = ahead.pop(stage)
                cur.wait_event(ev)
            else:
                masks = masks_of(stage)
                sparse, var = sparse_of(stage, masks)
            lmask = masks[0]
            fused = self.soft_attention[stage - 1].fuse(L, dense, sparse, lmask, var)     # reference :195-202
            pred, _ = self.refinement[stage - 1](L, R, fused)             # reference :207
        return [pred]


def get_model(**params):
    """modules/__init__.py:7-19"""
    if params["name"].lower() != "sparsedensenetrefinementmask":
        raise Exception("No such model: {}".format(params["name"]))
    keys = ("max_disp", "base_channels", "cost_func", "num_stage", "down_scale", "step", "samp_num",
            "sample_spa_size_list", "down_func_name", "weights", "grad_method", "if_overmask",
            "skip_stage_id", "use_detail", "thold")
    return SparseDenseNetRefinementMask(**{k: params[k] for k in keys})


def load_reference_checkpoint(model, state, strict=True):
    """demo.py:124-133: strip DataParallel's ``module.`` prefix and load.  The reference merges the checkpoint
    into the model's own state_dict, so a checkpoint with foreign key names silently loads nothing and the net
    runs on its random init; here (``strict=True``) every parameter and BatchNorm statistic of the model must
    come from the checkpoint and every checkpoint key must be consumed, else RuntimeError names the keys.
    Allowed: a missing ``num_batches_tracked`` (checkpoints of older PyTorch), and keys of the reference's
    parameter-free loss modules (``train_loss_func.*``, ``test_mask_loss_func.*``)."""
    own = model.state_dict()
    ckpt = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    missing = [k for k in own if k not in ckpt and not k.endswith("num_batches_tracked")]
    extra = [k for k in ckpt if k not in own and not k.startswith(("train_loss_func.", "test_mask_loss_func."))]
    if strict and (missing or extra):
        raise RuntimeError("checkpoint does not match the network: %d model keys missing (e.g. %s), %d checkpoint "
                           "keys unused (e.g. %s)" % (len(missing), missing[:3], len(extra), extra[:3]))
    own.update({k: v for k, v in ckpt.items() if k in own})
    model.load_state_dict(own)
    return model
