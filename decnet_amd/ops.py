"""Tensor-level wrappers over the C ABI (include/decnet_hip.h).

PyTorch is used only for device memory and the current HIP stream; every wrapper checks
device / dtype / contiguity / shape (the reference checks none of them and would read out of
bounds -- SM_kernel.cu:369-376 takes raw data_ptr<float>()) and then passes raw pointers.
"""
import torch

from . import _lib


_F32 = torch.float32
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


# the current HIP stream of device `index` as a raw handle (what the C ABI takes as void*)
_stream_of = _raw_stream or (lambda index: torch.cuda.current_stream(index).cuda_stream)


def _stream(t):
    return _stream_of(t.device.index)


def _chk(name, t, shape=None):
    # fast path first: this runs for every tensor of every call (SpaMatFunction's host time is what is
    # left of a training step at stages 1-2, bench.py `train`)
    if (type(t) is torch.Tensor or isinstance(t, torch.Tensor)) and t.is_cuda and t.dtype is _F32 and \
            t.is_contiguous() and (shape is None or t.shape == shape):
        return t
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.DecnetHipError(
            "%s is on %s: decnet_amd runs on the MI355X HIP path only (no CPU fallback)"
            % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if not t.is_contiguous():
        raise AssertionError("%s must be contiguous" % name)      # functions/SpaMat.py:21-22
    raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


_FN = {}


def _fn(name):
    """ctypes entry point, looked up once."""
    f = _FN.get(name)
    if f is None:
        f = _FN[name] = getattr(_lib.lib(), name)
    return f


def _call(name, like, *args, returns_rc=False):
    """THE way to make a C call: entry `name` on like's device (as torch.cuda.device_of, functions/SpaMat.py:24), the
    current stream of that device appended as the last argument, the result checked under the entry's own name.  returns_rc: DECNET_ERR_UNSUPPORTED is an answer, not an
    error, and is returned (0 otherwise) -- for the entries whose caller has another route."""
    fn = _FN.get(name) or _fn(name)
    idx = like.device.index
    if idx == torch.cuda.current_device():          # (this runs for every launch: no context object on the usual path)
        rc = fn(*args, _stream_of(idx))
    else:
        with torch.cuda.device(idx):
            rc = fn(*args, _stream_of(idx))
    if rc and not (returns_rc and rc == _lib.UNSUPPORTED):
        _lib.check(rc, name)
    return rc


def _same_device(*ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t is not None and t.device != dev:
            raise ValueError("all tensors must be on %s" % dev)
    return dev


def _feat_args(ref, tar, rmask, tmask, max_disp):
    _chk("ref_feas", ref)
    if ref.dim() != 4:
        raise ValueError("ref_feas must be [B,C,H,W]")
    B, C, H, W = ref.shape
    _chk("tar_feas", tar, (B, C, H, W))
    _chk("ref_mask", rmask, (B, H, W))
    _chk("tar_mask", tmask, (B, H, W))
    _same_device(ref, tar, rmask, tmask)
    D = int(max_disp)                       # numpy.int64 arrives here
    if D < 1:
        raise ValueError("max_disp must be >= 1")
    return B, C, H, W, D


# ---- disparity ranges wider than one band of the matrix-core kernels (max_disp > 273) ------------------------------------
# Above that the library sweeps the range band by band and needs scratch.  The wrappers below allocate it with torch.empty
# and call the `_ws` entry (include/decnet_hip.h): the library then owns no memory, and an allocation made by torch is what
# makes the call capturable (under torch.cuda.graph it comes from the graph's private pool).  Up to 273 the query is 0 and
# the original entry is called as before, with no query at all (one ctypes call matters at the host-bound small stages).
ONE_BAND = 273                      # decnet_spamat_workspace_floats is 0 up to here, whatever the other dims
WS_SPAMAT_FWD, WS_SPAVAR_FWD, WS_FUSED_FWD, WS_FUSED_BITS_FWD, WS_SPAMAT_BWD, WS_SPAVAR_BWD = range(6)
_WS_FLOATS = {}


def workspace_floats(B, C, H, W, D, which):
    """decnet_spamat_workspace_floats, cached per shape (a pure host function of its arguments)."""
    if D <= ONE_BAND:
        return 0
    key = (B, C, H, W, D, which)
    n = _WS_FLOATS.get(key)
    if n is None:
        n = _WS_FLOATS[key] = int(_fn("decnet_spamat_workspace_floats")(B, C, H, W, D, which))
    return n


def _call_banded(name, which, like, dims, *ptrs):
    """Entry `name` where one band takes the call, else its `_ws` twin on a workspace allocated here."""
    n = workspace_floats(*dims, which)
    if n == 0:
        return _call(name, like, *ptrs, *dims)
    ws = torch.empty(n, dtype=_F32, device=like.device)                # torch allocations are 16-byte aligned
    _call(name + "_ws", like, *ptrs, *dims, ws.data_ptr(), n)


def spamat_forward(ref, tar, rmask, tmask, output, sum_sim, max_cost, max_disp):
    B, C, H, W, D = _feat_args(ref, tar, rmask, tmask, max_disp)
    for n, t in (("output", output), ("sum_similarities", sum_sim), ("max_cost", max_cost)):
        _chk(n, t, (B, H, W))
    _call_banded("decnet_spamat_forward", WS_SPAMAT_FWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rmask.data_ptr(), tmask.data_ptr(), output.data_ptr(),
          sum_sim.data_ptr(), max_cost.data_ptr())


def spamat_backward(ref, tar, rmask, tmask, output, sum_sim, max_cost, grad_out, grad_ref, grad_tar,
                    max_disp):
    B, C, H, W, D = _feat_args(ref, tar, rmask, tmask, max_disp)
    for n, t in (("output", output), ("sum_similarities", sum_sim), ("max_cost", max_cost),
                 ("grad_output", grad_out)):
        _chk(n, t, (B, H, W))
    _chk("grad_ref_feas", grad_ref, (B, C, H, W))
    _chk("grad_tar_feas", grad_tar, (B, C, H, W))
    _call_banded("decnet_spamat_backward", WS_SPAMAT_BWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rmask.data_ptr(), tmask.data_ptr(), output.data_ptr(),
          sum_sim.data_ptr(), max_cost.data_ptr(), grad_out.data_ptr(), grad_ref.data_ptr(),
          grad_tar.data_ptr())


def spavar_forward(ref, tar, rmask, tmask, disparity, output, sum_sim, max_cost, max_disp):
    B, C, H, W, D = _feat_args(ref, tar, rmask, tmask, max_disp)
    for n, t in (("disparity", disparity), ("output", output), ("sum_similarities", sum_sim),
                 ("max_cost", max_cost)):
        _chk(n, t, (B, H, W))
    _call_banded("decnet_spavar_forward", WS_SPAVAR_FWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rmask.data_ptr(), tmask.data_ptr(),
          disparity.data_ptr(), output.data_ptr(), sum_sim.data_ptr(), max_cost.data_ptr())


def spavar_backward(ref, tar, rmask, tmask, disparity, output, sum_sim, max_cost, grad_out,
                    grad_ref, grad_tar, grad_disp, max_disp):
    B, C, H, W, D = _feat_args(ref, tar, rmask, tmask, max_disp)
    for n, t in (("disparity", disparity), ("output", output), ("sum_similarities", sum_sim),
                 ("max_cost", max_cost), ("grad_output", grad_out), ("grad_disparity", grad_disp)):
        _chk(n, t, (B, H, W))
    _chk("grad_ref_feas", grad_ref, (B, C, H, W))
    _chk("grad_tar_feas", grad_tar, (B, C, H, W))
    _call_banded("decnet_spavar_backward", WS_SPAVAR_BWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rmask.data_ptr(), tmask.data_ptr(),
          disparity.data_ptr(), output.data_ptr(), sum_sim.data_ptr(), max_cost.data_ptr(),
          grad_out.data_ptr(), grad_ref.data_ptr(), grad_tar.data_ptr(), grad_disp.data_ptr())


def spamatvar_forward_bits(ref, tar, rbits, tbits, max_disp, out=None):
    """spamatvar_forward with bit-packed masks: rbits / tbits int64 [B,H,ceil(W/64)], bit i of word w of a row = pixel
    64 w + i (what ``decnet_detail_mask`` writes beside the float plane).  Same results as the float-mask call."""
    _chk("ref_feas", ref)
    if ref.dim() != 4:
        raise ValueError("ref_feas must be [B,C,H,W]")
    B, C, H, W = ref.shape
    _chk("tar_feas", tar, (B, C, H, W))
    for n, t in (("ref_bits", rbits), ("tar_bits", tbits)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous() or
                tuple(t.shape) != (B, H, (W + 63) // 64)):
            raise ValueError("%s must be a contiguous int64 tensor [B,H,ceil(W/64)]" % n)
    _same_device(ref, tar, rbits, tbits)
    D = int(max_disp)
    if D < 1:
        raise ValueError("max_disp must be >= 1")
    if out is None:
        out = tuple(torch.empty((B, H, W), dtype=torch.float32, device=ref.device) for _ in range(4))
    o, v, s, m = out
    for n, t in (("output", o), ("variance", v), ("sum_similarities", s), ("max_cost", m)):
        _chk(n, t, (B, H, W))
    _call_banded("decnet_spamatvar_forward_bits", WS_FUSED_BITS_FWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rbits.data_ptr(), tbits.data_ptr(), o.data_ptr(),
          v.data_ptr(), s.data_ptr(), m.data_ptr())
    return o, v, s, m


def spamatvar_forward(ref, tar, rmask, tmask, max_disp, out=None):
    """Fused SpaMat + SpaVar forward (the model's only use of SpaVar,
    SparseDenseNetRefinementMask.py:183-192).  Returns (disparity, variance, sum_sim, max_cost),
    each [B,H,W].  Inference only (no autograd graph is recorded)."""
    B, C, H, W, D = _feat_args(ref, tar, rmask, tmask, max_disp)
    if out is None:
        out = tuple(torch.empty((B, H, W), dtype=torch.float32, device=ref.device) for _ in range(4))
    o, v, s, m = out
    for n, t in (("output", o), ("variance", v), ("sum_similarities", s), ("max_cost", m)):
        _chk(n, t, (B, H, W))
    _call_banded("decnet_spamatvar_forward", WS_FUSED_FWD, ref, (B, C, H, W, D),
          ref.data_ptr(), tar.data_ptr(), rmask.data_ptr(), tmask.data_ptr(), o.data_ptr(),
          v.data_ptr(), s.data_ptr(), m.data_ptr())
    return o, v, s, m


# ---- one level of the multi-stage training loss (csrc/loss.hip) ------------------------------------------------------
_F64 = torch.float64


def _chk64(name, t, shape):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.DecnetHipError("%s is on %s: decnet_amd runs on the MI355X HIP path only (no CPU fallback)"
                                  % (name, t.device))
    if t.dtype != _F64:
        raise TypeError("%s must be float64, got %s" % (name, t.dtype))
    if not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a contiguous float64 tensor of shape %s" % (name, tuple(shape)))
    return t


def _loss_planes(pred, dense, sparse, fusion, soft_mask, left_mask, gt):
    _chk("pred", pred)
    if pred.dim() != 3:
        raise ValueError("pred must be [B,H,W]")
    shape = pred.shape
    _chk("gt", gt, shape)
    opt = (("dense", dense), ("sparse", sparse), ("fusion", fusion), ("soft_mask", soft_mask), ("left_mask", left_mask))
    given = [t is not None for _, t in opt]
    if any(given) and not all(given):
        raise ValueError("dense, sparse, fusion, soft_mask and left_mask are given together (the composite form) or not "
                         "at all (the simple form)")
    for n, t in opt:
        if t is not None:
            _chk(n, t, shape)
    _same_device(pred, gt, *(t for _, t in opt))
    return tuple(shape), [0 if t is None else t.data_ptr() for _, t in opt]


def stage_loss_forward(pred, dense, sparse, fusion, soft_mask, left_mask, gt, gt_max, down_size, skip_rows, row_sums,
                       sums, terms):
    """decnet_stage_loss_forward: planes [B,H,W] float32 (dense ... left_mask all None: the simple form) ->
    row_sums [B*H,8] float64 (scratch), sums [8] float64, terms [5] float32 (dense, sparse, soft-mask mean, fusion,
    pred)."""
    (B, H, W), opt = _loss_planes(pred, dense, sparse, fusion, soft_mask, left_mask, gt)
    _chk64("row_sums", row_sums, (B * H, 8))
    _chk64("sums", sums, (8,))
    _chk("terms", terms, (5,))
    _call("decnet_stage_loss_forward", pred, pred.data_ptr(), *opt, gt.data_ptr(), float(gt_max), float(down_size),
          int(skip_rows), row_sums.data_ptr(), sums.data_ptr(), terms.data_ptr(), B, H, W)
    return terms


def stage_loss_backward(pred, dense, sparse, fusion, soft_mask, left_mask, gt, gt_max, down_size, skip_rows, sums,
                        grad_terms, g_pred=None, g_dense=None, g_sparse=None, g_fusion=None, g_soft=None):
    """decnet_stage_loss_backward: every gradient plane that is not None is written in full."""
    (B, H, W), opt = _loss_planes(pred, dense, sparse, fusion, soft_mask, left_mask, gt)
    _chk64("sums", sums, (8,))
    _chk("grad_terms", grad_terms, (5,))
    outs = []
    for n, t in (("g_pred", g_pred), ("g_dense", g_dense), ("g_sparse", g_sparse), ("g_fusion", g_fusion),
                 ("g_soft", g_soft)):
        outs.append(0 if t is None else _chk(n, t, (B, H, W)).data_ptr())
    _call("decnet_stage_loss_backward", pred, pred.data_ptr(), *opt, gt.data_ptr(), float(gt_max), float(down_size),
          int(skip_rows), sums.data_ptr(), grad_terms.data_ptr(), *outs, B, H, W)
