"""The image boundary on the device: wrappers of decnet_preprocess_u8 / decnet_disparity_to_u16 /
decnet_disparity_metrics (include/decnet_hip.h, csrc/imageio.hip) on the current stream, the normalisation table the
first one reads, and the float64 reduction of the third one's per-row sums.

The h x w image sits at the bottom right of the padded H x W plane (loader.pad_top_left pads on the top and left).
"""
import math

import numpy as np
import torch

from . import _lib
from .ops import _call  # noqa: F401  (tests/test_imageio_gpu.py calls imageio._call)

_U16 = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())     # two-byte integers: the bits are uint16


def padded_size(h, w, multiple=27):
    """The size loader.pad_top_left pads h x w to."""
    return int(math.ceil(h / multiple) * multiple), int(math.ceil(w / multiple) * multiple)


def normalise_table():
    """[256,3] float32: what the host path (loader._Base._item: ``pad_top_left(u8.astype(float32)) / 255`` through
    ``loader.normalise``) makes of pixel value v in channel c -- computed with those very numpy expressions, so that a
    lookup is bit-equal to the host path (a multiply by the reciprocal of 255 or of STD is not)."""
    from .loader import normalise
    v = np.repeat(np.arange(256, dtype=np.float32)[:, None, None], 3, axis=2)          # [256,1,3]: a 256 x 1 grey ramp
    return normalise(v / 255)[:, :, 0].t().contiguous()


def _chk(name, t, dtypes, shape):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.DecnetHipError("%s is on %s: decnet_amd runs on the MI355X HIP path only (no CPU fallback)"
                                  % (name, t.device))
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if not t.is_contiguous():
        raise AssertionError("%s must be contiguous" % name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def preprocess_u8(img, table, out):
    """img [B,h,w,3] uint8 -> out [B,3,H,W] float32 (H >= h, W >= w): padded on the top / left, scaled and normalised
    through ``table`` ([256,3] float32 on the device, normalise_table())."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or not isinstance(out, torch.Tensor) or out.dim() != 4:
        raise ValueError("img must be [B,h,w,3] and out [B,3,H,W]")
    B, h, w, _ = img.shape
    H, W = out.shape[-2:]
    _chk("img", img, (torch.uint8,), (B, h, w, 3))
    _chk("table", table, (torch.float32,), (256, 3))
    _chk("out", out, (torch.float32,), (B, 3, H, W))
    _call("decnet_preprocess_u8", out, img.data_ptr(), table.data_ptr(), out.data_ptr(), B, h, w, H, W)
    return out


def disparity_to_u16(pred, out):
    """pred [B,H,W] float32 -> out [B,h,w] (a two-byte integer tensor holding uint16 bits): demo.disparity_to_uint16 of
    every sample, the bottom-right h x w window."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or not isinstance(out, torch.Tensor) or out.dim() != 3:
        raise ValueError("pred must be [B,H,W] and out [B,h,w]")
    B, H, W = pred.shape
    h, w = out.shape[-2:]
    _chk("pred", pred, (torch.float32,), (B, H, W))
    _chk("out", out, _U16, (B, h, w))
    _call("decnet_disparity_to_u16", pred, pred.data_ptr(), out.data_ptr(), B, H, W, h, w)
    return out


def disparity_metrics(pred, gt, max_disp, partials):
    """pred [B,H,W], gt [B,h,w] (unpadded: compared with the bottom-right window of pred) -> partials [B,h,3]: per row
    the valid count (0 < gt < max_disp), sum |pred - gt| and the 3-px / 5 % count of eval.test_loss_func."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or not isinstance(gt, torch.Tensor) or gt.dim() != 3:
        raise ValueError("pred must be [B,H,W] and gt [B,h,w]")
    B, H, W = pred.shape
    h, w = gt.shape[-2:]
    _chk("pred", pred, (torch.float32,), (B, H, W))
    _chk("gt", gt, (torch.float32,), (B, h, w))
    _chk("partials", partials, (torch.float32,), (B, h, 3))
    _call("decnet_disparity_metrics", pred, pred.data_ptr(), gt.data_ptr(), float(max_disp), partials.data_ptr(),
          B, H, W, h, w)
    return partials


def sums_from_partials(partials):
    """[...,3] per-row sums -> their float64 totals [3] (count, sum of errors, good count), on partials' device and
    without a read-back."""
    p = torch.as_tensor(partials)
    return p.reshape(-1, 3).to(torch.float64).sum(0)


def metrics_from_sums(sums):
    """(epe, loss_3) of eval.test_loss_func from the totals (count, sum of errors, good count), in float64; no valid
    pixel gives NaN, as the reference's 0 / 0 does."""
    n, s, g = (float(v) for v in sums)
    if n == 0:
        return float("nan"), float("nan")
    return s / n, 100.0 - g / n * 100.0


def metrics_from_partials(partials):
    """(epe, loss_3) in float64 from the [B,h,3] per-row sums of disparity_metrics (reads them back)."""
    return metrics_from_sums(sums_from_partials(partials).cpu().numpy())
