"""Tensor-level wrappers of the 2-D trunk and stage-0 entries of the C ABI (include/decnet_hip.h): one function per
entry that model.py and stage0.py call.  Like ops.py for SpaMat / SpaVar: a wrapper takes tensors, checks them with
``ops._chk`` (on the GPU, fp32, contiguous, the shapes that follow from the others -- the C side takes raw pointers), goes
through ``ops._call`` (device, current stream, checked return code) and allocates its output unless ``out`` is given.
Every check comes before the first library lookup.  ``.contiguous()`` is the caller's business.
"""
import ctypes
from functools import partial

import torch

from . import _lib
from .ops import _F32, _call, _chk, _fn

_U8 = torch.uint8


def _run(name, ins, out, shape, *ints):
    """Entry `name`(inputs..., y, ints...) with y = out, or a new fp32 tensor of `shape` beside the first input; -> y."""
    y = torch.empty(shape, dtype=_F32, device=ins[0].device) if out is None else _chk("out", out, shape)
    _call(name, y, *[t.data_ptr() for t in ins], y.data_ptr(), *ints)
    return y


def _flat(name, t, n):
    """A buffer of at least n floats (workspaces grow only, so they may be longer) -> its address."""
    if _chk(name, t).numel() < n:
        raise ValueError("%s holds %d floats, the call needs %d" % (name, t.numel(), n))
    return t.data_ptr()


def _opt(name, t, shape=None):
    return None if t is None else _chk(name, t, shape).data_ptr()


def _new(want, like):
    """An optional output -> (a new tensor like `like`, its address), or (None, None) when it is not wanted."""
    t = torch.empty_like(like) if want else None
    return t, (t.data_ptr() if want else None)


def _mask_words(want, B, H, W, device):
    """The optional bit plane of a [B,H,W] mask, 64 pixels of a row per int64 word -> (tensor, address) or (None, None)."""
    t = torch.empty((B, H, (W + 63) // 64), dtype=torch.int64, device=device) if want else None
    return t, (t.data_ptr() if want else None)


def _wss(w, scale, shift, wtype=_F32):
    """Packed weight (a flat library-format buffer), folded scale and shift [Cout] -> (w, scale, shift), Cout."""
    if not (w.is_cuda and w.dtype is wtype and w.is_contiguous()):
        raise TypeError("the packed weight must be a contiguous %s tensor on the GPU" % wtype)
    _chk("shift", shift, _chk("scale", scale).shape)
    return (w, scale, shift), scale.shape[0]


def size(query, *dims):
    """A size query of the library (decnet_`query`: a pure host function of its arguments)."""
    return _fn("decnet_" + query)(*dims)


# ---- the few-channel fp32 kernels (csrc/conv2d_small.hip) and the bf16x3 matrix-core kernels (csrc/conv2d_mfma.hip) ---------
def conv2d_pack_weight(w, transposed):
    """Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k] weight -> the few-channel kernels' layout."""
    ci, co = _chk("weight", w).shape[:2] if transposed else (w.shape[1], w.shape[0])
    dims = (ci, co, w.shape[2], int(transposed))
    return _run("decnet_conv2d_pack_weight", (w,), None, (size("conv2d_packed_floats", *dims),), *dims)


def conv2d_mfma_pack_weight(w, cin, k):
    """[Cout, cin k k] fp32 -> bf16 terms in the operand layout (a stride-3 [Cout,Ci,3,3] goes in as cin = 9 Ci, k = 1)."""
    wp = torch.empty(size("conv2d_mfma_packed_bytes", cin, _chk("weight", w).shape[0], k), dtype=_U8, device=w.device)
    _call("decnet_conv2d_mfma_pack_weight", w, w.data_ptr(), wp.data_ptr(), cin, w.shape[0], k)
    return wp


def deconv2d_mfma_pack_weight(w):
    ci, co = _chk("weight", w).shape[:2]
    wp = torch.empty(size("deconv2d_mfma_packed_bytes", ci, co), dtype=_U8, device=w.device)
    _call("decnet_deconv2d_mfma_pack_weight", w, w.data_ptr(), wp.data_ptr(), ci, co)
    return wp


def _conv2d(name, up, wtype, x, w, scale, shift, cin, *ints, out=None):
    """A single-input entry: x [B,cin,H,W] -> [B,Cout,H,W] (up None), [B,Cout,3H,3W] (True), [B,Cout,ceil(H/3),ceil(W/3)]
    (False); ints: (k, dil, relu) or (relu)."""
    B, C, H, W = _chk("x", x).shape
    if C != cin:
        raise ValueError("the input has %d channels, the layer takes %d" % (C, cin))
    wss, Co = _wss(w, scale, shift, wtype)
    hw = (H, W) if up is None else (3 * H, 3 * W) if up else ((H - 1) // 3 + 1, (W - 1) // 3 + 1)
    return _run(name, (x,) + wss, out, (B, Co) + hw, B, cin, Co, H, W, *ints)


def _conv2d_cat(name, wtype, xs, w, scale, shift, cin, k, dil, relu, out=None, epi=None, ea=None, eb=None):
    """A `cat` entry: the parts xs [B,c_i,H,W] of a channel concatenation that is never materialised -> [B,Cout,H,W]."""
    B, _, H, W = _chk("input part", xs[0]).shape
    for t in xs[1:]:
        _chk("input part", t, (B, t.shape[1], H, W))
    cins, n = [int(t.shape[1]) for t in xs], len(xs)
    if sum(cins) != cin:
        raise ValueError("the parts have %d channels together, the layer takes %d" % (sum(cins), cin))
    wss, Co = _wss(w, scale, shift, wtype)
    y = torch.empty((B, Co, H, W), dtype=_F32, device=xs[0].device) if out is None else _chk("out", out, (B, Co, H, W))
    args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in xs]), (ctypes.c_int * n)(*cins), n, *[t.data_ptr() for t in wss],
            y.data_ptr(), B)
    if epi is None:
        _call(name, y, *args, Co, H, W, k, dil, relu)
    elif Co != 1:
        raise ValueError("the fused tail is a single-output layer's, this one has %d outputs" % Co)
    else:
        _call(name, y, *args, H, W, k, dil, relu, int(epi), _chk("ea", ea, (B, H, W)).data_ptr(), _opt("eb", eb, (B, H, W)))
    return y


# (x, w, scale, shift, cin, k, dil, relu, out=None) / (x, w, scale, shift, cin, relu, out=None); relu: 0 or 1
conv2d_bn_act = partial(_conv2d, "decnet_conv2d_bn_act", None, _F32)
conv2d_k3s3_bn_act = partial(_conv2d, "decnet_conv2d_k3s3_bn_act", False, _F32)
deconv2d_k3s3_bn_act = partial(_conv2d, "decnet_deconv2d_k3s3_bn_act", True, _F32)
deconv2d_mfma_k3s3_bn_act = partial(_conv2d, "decnet_deconv2d_mfma_k3s3_bn_act", True, _U8)
# (xs, w, scale, shift, cin, k, dil, relu, out=None)
conv2d_cat_bn_act = partial(_conv2d_cat, "decnet_conv2d_cat_bn_act", _F32)
conv2d_mfma_cat_bn_act = partial(_conv2d_cat, "decnet_conv2d_mfma_cat_bn_act", _U8)


def conv2d_cat_epilogue(xs, w, scale, shift, cin, k, dil, relu, epi, ea, eb=None, out=None):
    """The single-output layer with its fused tail: epi 1 = ea * (1 - sigmoid(v)) + sigmoid(v) * eb, 2 = ea + v."""
    return _conv2d_cat("decnet_conv2d_cat_epilogue", _F32, xs, w, scale, shift, cin, k, dil, relu, out, int(epi), ea, eb)


_WORKSPACE_FLOATS = {}


def _workspace_floats(name, dims, what):
    """The floats of workspace that entry decnet_`name` takes at `dims`: the library's size query, cached per entry and
    shape.  0 -- a shape the entry does not cover -- raises; what: the format of dims in that message."""
    n = _WORKSPACE_FLOATS.get((name,) + dims)
    if n is None:
        n = _WORKSPACE_FLOATS[(name,) + dims] = int(size(name + "_workspace_floats", *dims))
    if n == 0:
        raise _lib.DecnetHipError(("decnet_%s does not cover " + what) % ((name,) + dims))
    return n


def _wgrad_call(name, lead, gy, y, Co, G_shape, dims, what, tail):
    """The common end of the weight-gradient wrappers: decnet_`name`(lead..., gy, y, gm, G, gsum, workspace, its floats,
    tail...) -> (G, gsum, gm; gy itself without y).  The workspace comes from torch.empty, its size from
    _workspace_floats(name, dims, what)."""
    nws = _workspace_floats(name, dims, what)
    dev = gy.device
    G = torch.empty(G_shape, dtype=_F32, device=dev)
    gsum = torch.empty((Co,), dtype=_F32, device=dev)
    gm = gy if y is None else torch.empty_like(gy)
    ws = torch.empty(nws, dtype=_F32, device=dev)                      # torch allocations are 16-byte aligned
    _call("decnet_" + name, gy, *lead, gy.data_ptr(), None if y is None else y.data_ptr(),
          None if y is None else gm.data_ptr(), G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws, *tail)
    return G, gsum, gm


def _wgrad(name, xs, gy, y, k, dil):
    """One stride-1 weight-gradient entry `name` (conv2d_wgrad / conv2d_mfma_wgrad: one argument list)."""
    B, Co, H, W = _chk("gy", gy).shape
    if y is not None:
        _chk("y", y, (B, Co, H, W))
    for t in xs:
        _chk("input part", t, (B, t.shape[1], H, W))
    cins, n = [int(t.shape[1]) for t in xs], len(xs)
    cin, k, dil = sum(cins), int(k), int(dil)
    lead = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in xs]), (ctypes.c_int * n)(*cins), n)
    return _wgrad_call(name, lead, gy, y, Co, (Co, cin, k, k), (B, cin, Co, H, W, k),
                       "B %d, Cin %d, Cout %d, %d x %d, k %d", (B, Co, H, W, k, dil))


def conv2d_wgrad(xs, gy, y, k, dil):
    """Weight-gradient reduction of a few-channel stride-1 unit (decnet_conv2d_wgrad, csrc/conv2d_grad.hip): xs the parts
    [B,c_i,H,W] of the input, gy [B,Cout,H,W], y the unit's output (the ReLU mask y > 0) or None -> (G [Cout,Cin,k,k],
    gsum [Cout], gm = gy * [y > 0] [B,Cout,H,W]; gy itself without y)."""
    return _wgrad("conv2d_wgrad", xs, gy, y, k, dil)


def conv2d_mfma_wgrad(xs, gy, y, k, dil):
    """The same reduction for a many-channel unit (decnet_conv2d_mfma_wgrad, csrc/conv2d_mfma_grad.hip: Cin, Cout <= 224)."""
    return _wgrad("conv2d_mfma_wgrad", xs, gy, y, k, dil)


def _wgrad_s3(name, tr, x, gy, y):
    """One stride-3 weight-gradient entry (csrc/conv2d_mfma_grad.hip): x [B,Cin,H,W], gy (and y or None) the layer's output
    side -> (G in the layer's weight layout, gsum [Cout], gm)."""
    B, Ci, H, W = _chk("x", x).shape
    Co = _chk("gy", gy).shape[1]
    _chk("gy", gy, (B, Co, 3 * H, 3 * W) if tr else (B, Co, (H - 1) // 3 + 1, (W - 1) // 3 + 1))
    if y is not None:
        _chk("y", y, gy.shape)
    dims = (B, Ci, Co, H, W)
    return _wgrad_call(name, (x.data_ptr(),), gy, y, Co, (Ci, Co, 3, 3) if tr else (Co, Ci, 3, 3), dims,
                       "B %d, Cin %d, Cout %d, %d x %d", dims)


def conv2d_k3s3_wgrad(x, gy, y):
    """Conv2d k 3, stride 3, padding 1: gy [B,Cout,ceil(H/3),ceil(W/3)] -> (G [Cout,Cin,3,3], gsum, gm)."""
    return _wgrad_s3("conv2d_k3s3_wgrad", False, x, gy, y)


def deconv2d_k3s3_wgrad(x, gy, y):
    """ConvTranspose2d k 3, stride 3: gy [B,Cout,3H,3W] -> (G [Cin,Cout,3,3], gsum, gm)."""
    return _wgrad_s3("deconv2d_k3s3_wgrad", True, x, gy, y)


# ---- training-mode BatchNorm + ReLU under hip_grad() (csrc/batchnorm.hip) on its two layouts: NCHW planes (the Function
# is in conv2d_grad.py) and channels-last volumes, the Conv3d units of stage 0 (the Function is in stage0_grad.py) --------
BN_SEGMENT = 4096                  # DECNET_BN_SEGMENT of include/decnet_hip.h: floats of a plane one wave sums
BN_CL_ROWS = 32                    # DECNET_BN_CL_ROWS of include/decnet_hip.h: rows of a segment, one thread's partial sum


def _planes_dims(z):
    B, C, H, W = _chk("z", z).shape
    return B, C, H, W


def _columns_dims(z):
    """z [..., C] (contiguous: a matrix [rows, C]) -> (rows, C)."""
    if _chk("z", z).dim() < 2:
        raise ValueError("z must be channels-last [..., C] with two dimensions or more, got %s" % (tuple(z.shape),))
    C = int(z.shape[-1])
    return z.numel() // C if C else 0, C


# a layout: (z -> the entry's dims, C second; the stem of the public names, of the entries and of the size query)
_PLANES = (_planes_dims, "bn_train")
_COLUMNS = (_columns_dims, "bn_train_cl")


def _bn_train_args(layout, z, weight, bias):
    dims = layout[0](z)
    _chk("weight", weight, (dims[1],))
    _chk("bias", bias, (dims[1],))
    nws = int(size(layout[1] + "_workspace_floats", *dims))              # 0: a shape the entry refuses (it says which)
    ws = torch.empty(max(nws, 2), dtype=_F32, device=z.device)           # torch allocations are 16-byte aligned
    return dims, ws, nws


def _bn_train_forward(layout, z, weight, bias, eps, momentum, running_mean, running_var, relu):
    """Batch-statistics BatchNorm (+ ReLU) of z -> (y, stats [2C] float64: {mean, invstd} per channel, what the backward
    reads).  running_mean / running_var: both None, or both [C], updated in place.  The workspace comes from torch.empty
    per call, its size from the library's query."""
    dims, ws, nws = _bn_train_args(layout, z, weight, bias)
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var go together")
    stats = torch.empty(2 * dims[1], dtype=torch.float64, device=z.device)
    y = torch.empty_like(z)
    _call("decnet_%s_forward" % layout[1], z, z.data_ptr(), weight.data_ptr(), bias.data_ptr(), float(eps), float(momentum),
          _opt("running_mean", running_mean, (dims[1],)), _opt("running_var", running_var, (dims[1],)), stats.data_ptr(),
          y.data_ptr(), 1 if relu else 0, ws.data_ptr(), nws, *dims)
    return y, stats


def _bn_train_backward(layout, z, gy, weight, bias, stats, relu, want_gz=True):
    """-> (gz like z or None, dweight [C], dbias [C]); the ReLU decision is recomputed from z, as the forward made it."""
    dims, ws, nws = _bn_train_args(layout, z, weight, bias)
    _chk("gy", gy, z.shape)
    if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype is torch.float64 and stats.is_contiguous() and
            stats.shape == (2 * dims[1],)):
        raise TypeError("stats must be the contiguous float64 [2 C] tensor of %s_forward, on the GPU" % layout[1])
    gz, pz = _new(want_gz, z)
    dw, db = torch.empty_like(weight), torch.empty_like(bias)
    _call("decnet_%s_backward" % layout[1], z, z.data_ptr(), gy.data_ptr(), weight.data_ptr(), bias.data_ptr(),
          stats.data_ptr(), pz, dw.data_ptr(), db.data_ptr(), 1 if relu else 0, ws.data_ptr(), nws, *dims)
    return gz, dw, db


# (z, weight, bias, eps, momentum, running_mean, running_var, relu) / (z, gy, weight, bias, stats, relu, want_gz=True);
# z [B,C,H,W], or with _cl a channels-last [..., C]
bn_train_forward = partial(_bn_train_forward, _PLANES)
bn_train_backward = partial(_bn_train_backward, _PLANES)
bn_train_cl_forward = partial(_bn_train_forward, _COLUMNS)
bn_train_cl_backward = partial(_bn_train_backward, _COLUMNS)


def bias_act_inplace(x, b, relu):
    B, Co, H, W = _chk("x", x).shape
    _call("decnet_bias_act_inplace", x, x.data_ptr(), _chk("bias", b, (Co,)).data_ptr(), B, Co, H, W, relu)
    return x


def s2d3_pad1(x, out=None):
    """Space to depth of a k 3, stride 3, padding 1 convolution: [B,C,H,W] -> [B,9C,ceil(H/3),ceil(W/3)]."""
    B, C, H, W = _chk("x", x).shape
    return _run("decnet_s2d3_pad1", (x,), out, (B, 9 * C, (H - 1) // 3 + 1, (W - 1) // 3 + 1), B, C, H, W)


def d2s3_pad1(t, H, W, out=None):
    """The adjoint of s2d3_pad1: t [B,9C,ceil(H/3),ceil(W/3)] -> [B,C,H,W], written in full."""
    B, K, Ho, Wo = _chk("t", t).shape
    if K % 9 or (Ho, Wo) != ((H - 1) // 3 + 1, (W - 1) // 3 + 1):
        raise ValueError("t %s is not the space-to-depth of a %d x %d image" % (tuple(t.shape), H, W))
    return _run("decnet_d2s3_pad1", (t,), out, (B, K // 9, H, W), B, K // 9, H, W)


def s2d3_pad0(g, out=None):
    """Space to depth of a k 3, stride 3 transposed convolution's output: [B,C,3H,3W] -> [B,9C,H,W]."""
    B, C, H3, W3 = _chk("g", g).shape
    if H3 % 3 or W3 % 3:
        raise ValueError("g is %d x %d, not 3H x 3W" % (H3, W3))
    return _run("decnet_s2d3_pad0", (g,), out, (B, 9 * C, H3 // 3, W3 // 3), B, C, H3 // 3, W3 // 3)


# ---- the ASPP block as a per-tap GEMM (csrc/tapconv.hip) -------------------------------------------------------------
def tapconv_pack_weight(w, u, tap0):
    co, ci, k, _ = _chk("weight", w).shape
    _call("decnet_tapconv_pack_weight", w, w.data_ptr(), _chk("u", u).data_ptr(), co, ci, k, tap0)


def tapconv_split_weight(u, ci, ntaps):
    _call("decnet_tapconv_split_weight", u, _flat("u", u, size("tapconv_weight_floats", ci, ntaps)), ci, ntaps)


def tapconv_to_chunks(x):
    B, Ci, H, W = _chk("x", x).shape
    return _run("decnet_tapconv_to_chunks", (x,), None, (size("tapconv_chunk_floats", B, Ci, H, W),), B, Ci, H, W)


def tap_gemm(V, u, P, Ci, Co, ntaps, split):
    _chk("u", u)
    return _run("decnet_tap_gemm", (_chk("V", V), u), None, (ntaps * ((Co + 15) // 16) * 16 * P,), P, Ci, Co, ntaps, split)


def tapconv_gather(T, scale, shift, B, Co, H, W, tap0, ks, dil, relu, out=None):
    nb, ints = len(ks), lambda v: (ctypes.c_int * len(v))(*v)
    _chk("shift", shift, _chk("scale", scale, (nb * Co,)).shape)
    _flat("T", T, sum(k * k for k in ks) * ((Co + 15) // 16) * 16 * B * H * W)
    return _run("decnet_tapconv_gather", (T, scale, shift), out, (B, nb * Co, H, W), B, Co, H, W, nb, ints(tap0), ints(ks),
                ints(dil), relu)


# ---- the element-wise passes of the trunk ----------------------------------------------------------------------------
def unfold3_cat(fea, disp, out=None):
    """cat(disp, unfold(fea, 3, stride 3)): fea [B,C,3h,3w], disp [B,h,w] -> [B,9C+1,h,w]."""
    B, h, w = _chk("disp", disp).shape
    C = _chk("fea", fea).shape[1]
    _chk("fea", fea, (B, C, 3 * h, 3 * w))
    return _run("decnet_unfold3_cat", (fea, disp), out, (B, 9 * C + 1, h, w), B, C, h, w)


def dynamic_upsample3(logits, disp, out=None):
    B, h, w = _chk("disp", disp).shape
    _chk("logits", logits, (B, 81, h, w))
    return _run("decnet_dynamic_upsample3", (logits, disp), out, (B, 3 * h, 3 * w), B, h, w)


def warp_disparity(right, disp, out=None):
    B, C, H, W = _chk("right", right).shape
    _chk("disp", disp, (B, H, W))
    return _run("decnet_warp_disparity", (right, disp), out, (B, C, H, W), B, C, H, W)


# ---- the gathers of the full-resolution tail under hip_grad() (csrc/tail_grad.hip; the Functions are in tail_grad.py) ----
def warp_disparity_backward(right, disp, gout, want_right=True, want_disp=True):
    """-> (g_right [B,C,H,W] or None, g_disp [B,H,W] or None).  A width beyond the g_right kernel's LDS plan raises
    DecnetHipError with code UNSUPPORTED (nothing launched): ask for g_disp alone then."""
    B, C, H, W = _chk("right", right).shape
    _chk("disp", disp, (B, H, W))
    _chk("gout", gout, (B, C, H, W))
    if not (want_right or want_disp):
        return None, None
    (gr, pr), (gd, pd) = _new(want_right, right), _new(want_disp, disp)
    _call("decnet_warp_disparity_backward", right, right.data_ptr(), disp.data_ptr(), gout.data_ptr(), pr, pd, B, C, H, W)
    return gr, gd


def dynamic_upsample3_backward(logits, disp, gout, want_disp=True):
    """-> (g_logits [B,81,h,w], g_disp [B,h,w] or None).  The workspace comes from torch.empty, its size from the library's
    query, cached per shape."""
    B, h, w = _chk("disp", disp).shape
    _chk("logits", logits, (B, 81, h, w))
    _chk("gout", gout, (B, 3 * h, 3 * w))
    gl = torch.empty_like(logits)
    gd, pd = _new(want_disp, disp)
    nws = _workspace_floats("dynamic_upsample3_backward", (B, h, w), "B %d, %d x %d") if want_disp else 0
    ws = torch.empty(nws, dtype=_F32, device=disp.device) if want_disp else None      # (torch allocates 16-byte aligned)
    _call("decnet_dynamic_upsample3_backward", logits, logits.data_ptr(), disp.data_ptr(), gout.data_ptr(), gl.data_ptr(),
          pd, ws.data_ptr() if want_disp else None, nws, B, h, w)
    return gl, gd


def fold3(g, out=None):
    """Inverse of unfold3_cat's feature part: g [B,9C+1,h,w] -> [B,C,3h,3w] (channel 0 is not read)."""
    B, K, h, w = _chk("g", g).shape
    if K < 10 or (K - 1) % 9:
        raise ValueError("g has %d channels, not 9 C + 1" % K)
    C = (K - 1) // 9
    return _run("decnet_fold3", (g,), out, (B, C, 3 * h, 3 * w), B, C, h, w)


# ---- the elementwise passes under hip_grad() (csrc/detail_grad.hip; the Functions are in tail_grad.py) -------------------
def sigmoid_blend(o, a, b, out=None):
    """a * (1 - sigmoid(o)) + sigmoid(o) * b over planes of one shape: conv2d_cat_epilogue's epilogue 1 on its own."""
    _chk("b", b, _chk("a", a, _chk("o", o).shape).shape)
    return _run("decnet_sigmoid_blend", (o, a, b), out, o.shape, o.numel())


def _blend_backward(entry, o, a, b, grads, optional, want_a, want_b):
    """Both blend backwards.  grads: ((name, gradient of an output of `entry`), ...); optional: all but one may be None."""
    shape = _chk("b", b, _chk("a", a, _chk("o", o).shape).shape).shape
    ptrs = [None if optional and t is None else _chk(n, t, shape).data_ptr() for n, t in grads]
    if ptrs.count(None) == len(ptrs):
        raise ValueError("%s are both None" % " and ".join(n for n, _ in grads))
    go = torch.empty_like(o)
    ga = torch.empty_like(o) if want_a else None                      # (written out, not _new(): two more Python calls
    gb = torch.empty_like(o) if want_b else None                      # per backward showed in the eager timing)
    _call(entry, o, o.data_ptr(), a.data_ptr(), b.data_ptr(), *ptrs, go.data_ptr(), ga.data_ptr() if want_a else None,
          gb.data_ptr() if want_b else None, o.numel())
    return go, ga, gb


def sigmoid_blend_backward(o, a, b, gout, want_a=True, want_b=True):
    """-> (g_o, g_a or None, g_b or None)."""
    return _blend_backward("decnet_sigmoid_blend_backward", o, a, b, (("gout", gout),), False, want_a, want_b)


def sqdiff(a, b, out=None):
    """(a - b) * (a - b) over tensors of one shape, torch's bits."""
    _chk("b", b, _chk("a", a).shape)
    return _run("decnet_sqdiff", (a, b), out, a.shape, a.numel())


def sqdiff_backward(a, b, gout, want_a=True, want_b=True):
    """-> (g_a or None, g_b or None): 2 gout (a - b) and its negative."""
    _chk("gout", gout, _chk("b", b, _chk("a", a).shape).shape)
    if not (want_a or want_b):
        return None, None
    (ga, pa), (gb, pb) = _new(want_a, a), _new(want_b, a)
    _call("decnet_sqdiff_backward", a, a.data_ptr(), b.data_ptr(), gout.data_ptr(), pa, pb, a.numel())
    return ga, gb


def detail_tail(logits, thold, want_prob=True, want_mask=True, want_bits=False):
    """logits [B,H,W] -> (prob = sigmoid(logits), mask = prob > thold as float 0/1, bits: the mask as 64 pixels per int64
    word), each None unless asked for."""
    B, H, W = _chk("logits", logits).shape
    if not (want_prob or want_mask or want_bits):
        return None, None, None
    prob = torch.empty_like(logits) if want_prob else None            # (written out, not _new(): as _blend_backward)
    mask = torch.empty_like(logits) if want_mask else None
    bits, pb = _mask_words(want_bits, B, H, W, logits.device)
    _call("decnet_detail_tail", logits, logits.data_ptr(), float(thold), prob.data_ptr() if want_prob else None,
          mask.data_ptr() if want_mask else None, pb, B, H, W)
    return prob, mask, bits


def detail_tail_backward(logits, g_prob):
    """-> g_logits = g_prob * s * (1 - s), s = sigmoid(logits) as detail_tail computes it."""
    _chk("g_prob", g_prob, _chk("logits", logits).shape)
    gl = torch.empty_like(logits)
    _call("decnet_detail_tail_backward", logits, logits.data_ptr(), g_prob.data_ptr(), gl.data_ptr(), logits.numel())
    return gl


def sigmoid_blend_soft(o, a, b):
    """-> (sigmoid_blend(o, a, b), sigmoid(o)): the blend's bits, and the soft mask it was made with."""
    _chk("b", b, _chk("a", a, _chk("o", o).shape).shape)
    out, soft = torch.empty_like(o), torch.empty_like(o)
    _call("decnet_sigmoid_blend_soft", o, o.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), soft.data_ptr(),
          o.numel())
    return out, soft


def sigmoid_blend_soft_backward(o, a, b, gout, gsoft, want_a=True, want_b=True):
    """gout, gsoft: the gradients of the two outputs, one of them may be None -> (g_o, g_a or None, g_b or None)."""
    grads = (("gout", gout), ("gsoft", gsoft))
    return _blend_backward("decnet_sigmoid_blend_soft_backward", o, a, b, grads, True, want_a, want_b)


def detail_mask_params(flat):
    """The 92 folded host values of GenerateSparseMask.conv as the entry takes them: w3x3, scale3, shift3, w1x1, s1, b1."""
    arr = lambda v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    return arr(flat[0:81]), arr(flat[81:84]), arr(flat[84:87]), arr(flat[87:90]), flat[90], flat[91]


def detail_mask(cur3, pre3, params, thold, want_bits=False, out=None, want_logits=False):
    """-> (mask [B,H,W] float 0/1, bits: None or the bit-packed copy the SpaMat kernels read, 64 pixels per int64 word);
    with want_logits -> (mask, bits, logits [B,H,W]: `detail` before the sigmoid)."""
    B, C, H, W = _chk("cur3", cur3).shape
    _chk("pre3", pre3, (B, 3, H, W))
    if C != 3:
        raise ValueError("cur3 has %d channels, the layer takes 3" % C)
    y = torch.empty((B, H, W), dtype=_F32, device=cur3.device) if out is None else _chk("out", out, (B, H, W))
    bits, pb = _mask_words(want_bits, B, H, W, cur3.device)
    logits, pl = _new(want_logits, y)
    _call("decnet_detail_mask", cur3, cur3.data_ptr(), pre3.data_ptr(), *params, float(thold), y.data_ptr(), pl, pb, B, H, W)
    return (y, bits, logits) if want_logits else (y, bits)


# ---- stage 0 (channels-last [B,D,H,W,C] volumes; the activation buffers are flat, grow-only workspaces) ------------------
def ncdhw_to_ndhwc(x, out=None):
    B, C, D, H, W = _chk("x", x).shape
    return _run("decnet_ncdhw_to_ndhwc", (x,), out, (B, D, H, W, C), B, C, D, H, W)


def costvol_forward_cf(left, right, D, cost_func, out=None):
    """[B,C,H,W] x2 -> channels-last cost volume [B,D,H,W,C] ([B,D,H,W,2C] for cost_func "cat")."""
    B, C, H, W = _chk("left_feature_map", left).shape
    _chk("right_feature_map", right, (B, C, H, W))
    return _run("decnet_costvol_forward_cf", (left, right), out, (B, D, H, W, 2 * C if cost_func == "cat" else C),
                B, C, H, W, D, _lib.COST_FUNC[cost_func])


def conv3d_pointwise(x, w, out=None):
    """Conv3d k 1 without bias on a channels-last volume: x [B,D,H,W,Ci], w [Co,Ci] -> [B,D,H,W,Co]."""
    B, D, H, W, Ci = _chk("x", x).shape
    Co = _chk("w", w).shape[0]
    _chk("w", w, (Co, Ci))
    return _run("decnet_conv3d_pointwise", (x, w), out, (B, D, H, W, Co), B, Ci, Co, D * H * W, Ci, 1)


def conv3d_pack_weight(w):
    """[Co,Ci,3,3,3] -> [27,Ci,CoP]."""
    Co, Ci = _chk("weight", w).shape[:2]
    CoP = size("conv3d_packed_cout", Co)
    if CoP < 0:
        raise _lib.DecnetHipError("Conv3d with %d output channels is not supported (<= 224)" % Co)
    return _run("decnet_conv3d_pack_weight", (w,), None, (27, Ci, CoP), Co, Ci)


def conv3d_wino_pack_weight(w, variant):
    Co, Ci = _chk("weight", w).shape[:2]
    n = size("conv3d_wino_weight_floats", Ci, variant)
    return _run("decnet_conv3d_wino_pack_weight", (w,), None, (n,), Co, Ci, variant)


def conv3d_bn_act(src, w, scale, shift, res, dst, dims, Ci, Co, relu, ws=None, variant=None):
    """One Conv3dUnit on flat buffers, dims = (B, D, H, W): dst = act(bn(conv(src))) (+ res).  decnet_conv3d_bn_act (27-tap
    implicit GEMM, w from conv3d_pack_weight), or with ws (size conv3d_wino_workspace_floats) decnet_conv3d_wino_bn_act
    (Winograd `variant`, w from conv3d_wino_pack_weight)."""
    n = dims[0] * dims[1] * dims[2] * dims[3]
    _chk("shift", shift, _chk("scale", scale, (Co,)).shape)
    p = (_flat("src", src, n * Ci), _chk("weight", w).data_ptr(), scale.data_ptr(), shift.data_ptr(),
         None if res is None else _flat("res", res, n * Co), _flat("dst", dst, n * Co))
    if ws is None:
        _call("decnet_conv3d_bn_act", src, *p, *dims, Ci, Co, relu)
    else:
        _call("decnet_conv3d_wino_bn_act", src, *p, _chk("ws", ws).data_ptr(), *dims, Ci, Co, relu, variant)


def conv3d_wgrad(x, gy, y, dims, Ci, Co):
    """Weight-gradient reduction of one Conv3dUnit (decnet_conv3d_wgrad, csrc/conv3d_grad.hip) on channels-last volumes,
    dims = (B, D, H, W): x [B,D,H,W,Ci], gy [B,D,H,W,Co], y the unit's output (the ReLU mask y > 0) or None -> (G
    [Co,Ci,3,3,3], gsum [Co], gm = gy * [y > 0]; gy itself without y).  The workspace comes from torch.empty, its size from
    the library's query, cached per shape."""
    dims = tuple(int(d) for d in dims)
    _chk("x", x, dims + (Ci,))
    _chk("gy", gy, dims + (Co,))
    if y is not None:
        _chk("y", y, dims + (Co,))
    dims += (int(Ci), int(Co))
    return _wgrad_call("conv3d_wgrad", (x.data_ptr(),), gy, y, Co, (Co, Ci, 3, 3, 3), dims,
                       "B %d, D %d, %d x %d, Ci %d, Co %d", dims)


def conv3d_wino_stack_bn_act(x, layers, res_src, res_dst, out, ws, dims, C, variant):
    """The C -> C units `layers` (dicts of u, scale, shift) as ONE fused stack; False: "unsupported", nothing launched."""
    n = dims[0] * dims[1] * dims[2] * dims[3] * C
    for p in layers:
        _chk("u", p["u"])
        _chk("shift", p["shift"], _chk("scale", p["scale"], (C,)).shape)
    u, sc, sh = ((ctypes.c_void_p * len(layers))(*[p[k].data_ptr() for p in layers]) for k in ("u", "scale", "shift"))
    return 0 == _call("decnet_conv3d_wino_stack_bn_act", x, _flat("x", x, n), u, sc, sh, len(layers), res_src, res_dst,
                      _flat("out", out, n), _chk("ws", ws).data_ptr(), *dims, C, variant, returns_rc=True)


def conv3d_cout1_softargmax(x, w, scale, shift, dims, Ci, reg=None, pred=None, ws=None):
    """The last unit (one output channel; scale, shift: host floats) + softmax over D + expectation: x -> (reg [B,D,H,W]
    if given, pred [B,H,W]).  ws (size conv3d_cout1_workspace_floats): the tap-GEMM form, decnet_conv3d_cout1_softargmax_ws."""
    B, D, H, W = dims
    _chk("weight", w, (1, Ci, 3, 3, 3))
    y = torch.empty((B, H, W), dtype=_F32, device=x.device) if pred is None else _chk("pred", pred, (B, H, W))
    p = (_flat("x", x, B * D * H * W * Ci), w.data_ptr(), scale, shift, _opt("reg", reg, dims), y.data_ptr())
    if ws is None:
        _call("decnet_conv3d_cout1_softargmax", x, *p, *dims, Ci)
    else:
        _call("decnet_conv3d_cout1_softargmax_ws", x, *p, _chk("ws", ws).data_ptr(), *dims, Ci)
    return y


def stage0_forward_cf(left, right, params, w_pre, ws, D, variant, cost_func, reg=None, pred=None):
    """The whole stage-0 branch in one entry: [B,C,H,W] x2 -> pred [B,H,W] (and reg [B,D,H,W] where given); params: a
    _lib.Stage0Params, ws: size stage0_cf_workspace_floats."""
    B, C, H, W = _chk("left_feature_map", left).shape
    _chk("right_feature_map", right, (B, C, H, W))
    y = torch.empty((B, H, W), dtype=_F32, device=left.device) if pred is None else _chk("pred", pred, (B, H, W))
    _call("decnet_stage0_forward_cf", left, left.data_ptr(), right.data_ptr(), ctypes.byref(params), _opt("w_pre", w_pre),
          _chk("ws", ws).data_ptr(), _opt("reg", reg, (B, D, H, W)), y.data_ptr(), B, C, H, W, D, variant,
          _lib.COST_FUNC[cost_func])
    return y


def disparity_regression(cost_vol, disp_samples, out=None):
    """softmax over dim 1, expectation of disp_samples: [B,S,H,W] x2 -> [B,H,W]."""
    B, S, H, W = _chk("cost_vol", cost_vol).shape
    _chk("disp_samples", disp_samples, (B, S, H, W))
    return _run("decnet_disparity_regression", (cost_vol, disp_samples), out, (B, H, W), B, S, H, W)
