"""The stage-0 entries of include/decnet_hip.h (csrc/stage0.hip, conv3d_winograd.hip, stage0_entry.hip) through the C ABI
at edge shapes, against the float64 references of tests/_stage0_ref.py.  As in tests/test_trunk_edges_gpu.py every case
runs twice, with every non-library buffer (feature maps, activations, residuals, scale / shift, w_pre, samples, outputs) a
window of a sentinel-guarded buffer, 16-byte aligned and at an odd float offset.  Each run checks the margins, that the
inputs are bit-unchanged, that every output element is written (NaN pre-fill) and rc == 0; the two placements must be
bit-identical and the aligned one must match float64 (bounds: TOL_* below).  Library-format buffers (packed weights,
Winograd / stack / cout1 workspaces, the V / M of the GEMM) are 16-byte aligned by the header's rule; that misaligned ones
are rejected with DECNET_ERR_MISALIGNED and nothing launched is tested separately.  The stage-0 workspace is taken at any
alignment, so it follows the placement like the other buffers (margins checked, contents scratch).
The knob legs at the end re-run the cases in child processes under the switches the kernels read once per process.
-m gpu."""
import ctypes
import os
import subprocess
import sys
import zlib

import pytest
import torch

import _stage0_ref as R
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _assert_close, _both, _L, _st

pytestmark = pytest.mark.gpu

ERR_BAD_SHAPE = -2
COR, SSD, CAT, SUM = 0, 1, 2, 3
LDS = 160 * 1024                   # the fused stack's LDS limit (conv3d_winograd.hip: stack_ok, head_lds_bytes)

# Bounds against float64, relative to max(1, max|ref|) (pred: pixels, (max, mean)).  The existing tests' bounds were cost
# volume / pointwise 2e-5, layers 1e-4, reg 2e-4, pred (1e-3, 1e-4); these are tightened from the worst case measured on
# the MI355X over all cases here, at both GEMM kernels and chunkings (the knob legs), with ~3x headroom:
#   measured: cost volume 1.8e-6, pointwise 5.1e-7, direct conv 1.9e-6, Winograd conv 4.1e-6 (fp32 GEMM, chunked: the
#   same), Winograd GEMM alone 4.6e-7, stack (2 - 7 layers) 6.2e-6, cout1 reg 2.5e-7 / pred (8.1e-5, 4.2e-5) px (D = 256,
#   flat softmax), disparity_regression (3.3e-6, 7.6e-7) px, stage 0 reg 2.8e-6 / pred (3.1e-6, 6.3e-7) px.
TOL_COSTVOL = 5e-6
TOL_POINTWISE = 2e-6
TOL_DIRECT = 1e-5
TOL_WINO = 1.5e-5
TOL_GEMM = 2e-6
TOL_STACK = 2e-5
TOL_COUT1_REG = 2e-6
TOL_COUT1_PRED = (3e-4, 1e-4)
TOL_REGRESSION_PRED = (1e-5, 2.5e-6)
TOL_STAGE0_REG = 1e-5
TOL_STAGE0_PRED = (1e-5, 2e-6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _dev():
    return torch.device("cuda:0")


def _lib_buf(n, fill=float("nan")):
    """A library-format buffer: a fresh (16-byte aligned) torch allocation of n floats."""
    t = torch.full((max(int(n), 1),), fill, dtype=torch.float32, device=_dev())
    assert t.data_ptr() % 16 == 0
    return t


def _g(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _w(co, ci, g, pos=False):
    w = torch.randn(co, ci, 3, 3, 3, generator=g)
    return (w.abs() if pos else w) / (27 * ci) ** 0.5


def _bn(c, g):
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1


def _pred_ok(pred, ref, tol, what=""):
    """tol = (max, mean) in pixels."""
    err = (pred.double() - ref).abs()
    assert float(err.max()) <= tol[0] and float(err.mean()) <= tol[1], (what, float(err.max()), float(err.mean()))


def _pack_wino(w, variant):
    L = _L()
    Co, Ci = w.shape[:2]
    u = _lib_buf(L.decnet_conv3d_wino_weight_floats(Ci, variant))
    assert L.decnet_conv3d_wino_pack_weight(w.to(_dev()).data_ptr(), u.data_ptr(), Co, Ci, variant, _st()) == 0
    return u


def _pack_direct(w):
    L = _L()
    Co, Ci = w.shape[:2]
    wp = _lib_buf(27 * Ci * L.decnet_conv3d_packed_cout(Co))
    assert L.decnet_conv3d_pack_weight(w.to(_dev()).data_ptr(), wp.data_ptr(), Co, Ci, _st()) == 0
    return wp


# the LDS budgets of the fused stack, as conv3d_winograd.hip computes them
def stack_lds_bytes(D, H, W):
    return D * H * 4 * (W | 1) * 4


def head_lds_bytes(D, H, W):
    pitch = ((W + D - 1 + 23) & ~31) + 8
    return stack_lds_bytes(D, H, W) + (8 * H * W + 3 * (W + D) + 3 * H + 4 * H * pitch) * 4


def stack_ws_floats(B, D, H, W, C):
    """What the fused stack touches (V / M of one chunk + the residual plane), also where it declines the shape."""
    w = (_L().decnet_conv3d_wino_workspace_floats(B, D, H, W, C, C, 2) + 63) & ~63
    return w + B * ((C + 3) // 4) * D * H * 4 * (W | 1)


# ------------------------------------------------------------------------------------------------------------------
# decnet_costvol_forward_cf (stage0.hip: channel groups of <= 128, dchunk disparities per workgroup)
COSTVOL = [  # (B, C, H, W, D)
    (1, 1, 2, 2, 1), (2, 4, 3, 2, 5), (1, 4, 2, 3, 3), (1, 128, 2, 3, 3), (1, 129, 3, 2, 4), (2, 216, 2, 3, 7),
    (1, 257, 3, 3, 3), (1, 4, 64, 5, 33), (3, 5, 3, 4, 6),
]


def _run_costvol(case, cf, aligned):
    B, C, H, W, D = case
    g = _g("cv", case, cf)
    left, right = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    P = Place(_dev(), aligned)
    ld, rd = P.inp(left), P.inp(right)
    out = P.out((B, D, H, W, 2 * C if cf == CAT else C))
    assert _L().decnet_costvol_forward_cf(ld.data_ptr(), rd.data_ptr(), out.data_ptr(), B, C, H, W, D, cf, _st()) == 0
    P.check("costvol %s cf %d" % (case, cf))
    return {"y": out.cpu(), "ref": R.costvol(left, right, D, cf)}


@pytest.mark.parametrize("case", COSTVOL, ids=[str(i) for i in range(len(COSTVOL))])
@pytest.mark.parametrize("cf", [COR, SSD, CAT, SUM])
def test_costvol_edges(dev, case, cf):
    r = _both(_run_costvol, case, cf)
    _assert_close(r["y"], r["ref"], TOL_COSTVOL, (case, cf))


def test_costvol_rejects_one_row_or_column(dev):
    """H = 1 or W = 1: the warp divides by H - 1 / W - 1; -2, nothing written."""
    x = torch.randn(2 * 4 * 3, device=dev)
    out = torch.full((64,), float("nan"), device=dev)
    for H, W in ((1, 3), (3, 1), (1, 1)):
        for cf in (COR, SSD, CAT, SUM):
            assert _L().decnet_costvol_forward_cf(x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 2, H, W, 2, cf,
                                                  _st()) == ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# decnet_conv3d_pointwise (its values are tested in tests/test_stage0_gpu.py; here: the odd placement)
@pytest.mark.parametrize("B,Ci,Co,P,ldw,cl", [(2, 5, 3, 7, 5, 0), (1, 12, 7, 33, 24, 1), (2, 216, 216, 37, 432, 0),
                                              (1, 3, 1, 1, 4, 1)])
def test_pointwise_edges(dev, B, Ci, Co, P, ldw, cl):
    def run(aligned):
        g = _g("pw", B, Ci, Co, P)
        x = torch.randn(*((B, P, Ci) if cl else (B, Ci, P)), generator=g)
        w = torch.randn((Co - 1) * ldw + Ci, generator=g) / Ci ** 0.5
        Pl = Place(dev, aligned)
        xd, wd = Pl.inp(x), Pl.inp(w)
        y = Pl.out((B, P, Co) if cl else (B, Co, P))
        assert _L().decnet_conv3d_pointwise(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), B, Ci, Co, P, ldw, cl,
                                            _st()) == 0
        Pl.check("pointwise")
        return {"y": y.cpu(), "ref": R.pointwise(x, w, ldw, cl)}
    r = _both(run)
    _assert_close(r["y"], r["ref"], TOL_POINTWISE)


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv3d_bn_act (direct 27-tap implicit GEMM; BK 36 when Ci % 36 == 0, else 24) and decnet_conv3d_wino_bn_act
CONV = [  # (B, D, H, W, Ci, Co, relu, residual)
    (1, 1, 1, 1, 4, 1, 1, 0), (2, 2, 3, 5, 12, 5, 0, 1), (3, 3, 2, 1, 36, 16, 1, 1), (1, 5, 1, 3, 72, 17, 1, 0),
    (1, 2, 5, 2, 216, 216, 1, 1), (2, 3, 3, 3, 216, 224, 0, 0), (1, 5, 5, 5, 4, 224, 1, 1), (2, 1, 2, 3, 36, 1, 0, 1),
    (1, 3, 5, 1, 12, 17, 1, 1), (2, 5, 2, 5, 72, 216, 1, 0),
]


def _run_conv(case, algo, aligned):
    B, D, H, W, Ci, Co, relu, res = case
    L = _L()
    g = _g("conv", case)
    x = torch.randn(B, D, H, W, Ci, generator=g)
    w = _w(Co, Ci, g)
    scale, shift = _bn(Co, g)
    resid = torch.randn(B, D, H, W, Co, generator=g) if res else None
    wp = _pack_direct(w) if algo == "direct" else _pack_wino(w, algo)
    P = Place(_dev(), aligned)
    xd, sd, hd = P.inp(x), P.inp(scale), P.inp(shift)
    rd = P.inp(resid) if res else None
    y = P.out((B, D, H, W, Co))
    rp = rd.data_ptr() if res else None
    if algo == "direct":
        rc = L.decnet_conv3d_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), rp, y.data_ptr(),
                                    B, D, H, W, Ci, Co, relu, _st())
    else:
        ws = _lib_buf(L.decnet_conv3d_wino_workspace_floats(B, D, H, W, Ci, Co, algo))
        rc = L.decnet_conv3d_wino_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), rp, y.data_ptr(),
                                         ws.data_ptr(), B, D, H, W, Ci, Co, relu, algo, _st())
    assert rc == 0, rc
    P.check("conv3d %s %s" % (algo, case))
    return {"y": y.cpu(), "ref": R.conv3d_unit(x, w, scale, shift, resid, relu)}


@pytest.mark.parametrize("case", CONV, ids=[str(i) for i in range(len(CONV))])
def test_conv3d_direct_edges(dev, case):
    r = _both(_run_conv, case, "direct")
    _assert_close(r["y"], r["ref"], TOL_DIRECT, case)


WINO = CONV + [  # tile edges of 2 and 4 on every axis
    (1, 9, 4, 5, 12, 16, 1, 1), (1, 4, 9, 3, 36, 17, 1, 0), (2, 3, 5, 9, 216, 216, 1, 1), (1, 1, 9, 4, 216, 5, 0, 0),
    (1, 5, 3, 4, 4, 224, 1, 0), (3, 9, 17, 18, 4, 17, 1, 1),      # the last: > 192 tiles, chunked under the knob leg
]


@pytest.mark.parametrize("case", WINO, ids=[str(i) for i in range(len(WINO))])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_conv3d_wino_edges(dev, case, variant):
    r = _both(_run_conv, case, variant)
    _assert_close(r["y"], r["ref"], TOL_WINO, (case, variant))


def test_conv3d_rejects_what_the_header_excludes(dev):
    """Co = 225 (> 224): DECNET_ERR_UNSUPPORTED from both packers and both convolutions, nothing written."""
    L, st = _L(), _st()
    Ci, Co = 4, 225
    w = torch.randn(Co, Ci, 3, 3, 3, device=dev)
    x, s = torch.randn(1, 2, 2, 2, Ci, device=dev), torch.ones(Co, device=dev)
    wp = _lib_buf(27 * Ci * 256)
    y = _lib_buf(8 * Co)
    ws = _lib_buf(L.decnet_conv3d_wino_workspace_floats(1, 2, 2, 2, Ci, Co, 2))
    assert L.decnet_conv3d_packed_cout(Co) == -1
    assert L.decnet_conv3d_pack_weight(w.data_ptr(), wp.data_ptr(), Co, Ci, st) == ERR_UNSUPPORTED
    assert L.decnet_conv3d_bn_act(x.data_ptr(), wp.data_ptr(), s.data_ptr(), s.data_ptr(), None, y.data_ptr(), 1, 2, 2, 2,
                                  Ci, Co, 1, st) == ERR_UNSUPPORTED
    assert L.decnet_conv3d_wino_pack_weight(w.data_ptr(), wp.data_ptr(), Co, Ci, 2, st) == ERR_UNSUPPORTED
    assert L.decnet_conv3d_wino_bn_act(x.data_ptr(), wp.data_ptr(), s.data_ptr(), s.data_ptr(), None, y.data_ptr(),
                                       ws.data_ptr(), 1, 2, 2, 2, Ci, Co, 1, 2, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(wp).all())


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv3d_wino_gemm alone: V [points][ceil(Ci/16)][nt][16], U^T [points][ceil(Ci/16)][224][16] (the fp32 part of
# decnet_conv3d_wino_pack_weight's output), M [points][ceil(Co/16)][nt][16]
@pytest.mark.parametrize("nt", [1, 47, 96, 97])
@pytest.mark.parametrize("Ci,Co,variant", [(216, 216, 2), (20, 17, 2), (4, 1, 0), (36, 224, 1), (216, 5, 1)])
def test_wino_gemm_edges(dev, nt, Ci, Co, variant):
    L = _L()
    np_ = {0: 64, 1: 144, 2: 216}[variant]
    kc, kco = (Ci + 15) // 16, (Co + 15) // 16
    g = _g("gemm", nt, Ci, Co, variant)
    u = _pack_wino(_w(Co, Ci, g), variant)
    V = torch.randn(np_, kc * 16, nt, generator=g)
    V[:, Ci:] = 0                                                   # channels past Ci: zero, as the input transform writes
    Vd = _lib_buf(V.numel())
    Vd.copy_(V.view(np_, kc, 16, nt).permute(0, 1, 3, 2).reshape(-1))
    M = _lib_buf(np_ * kco * nt * 16)
    assert L.decnet_conv3d_wino_gemm(Vd.data_ptr(), u.data_ptr(), M.data_ptr(), nt, Ci, Co, variant, _st()) == 0
    torch.cuda.synchronize()
    U = u[:np_ * kc * 224 * 16].cpu().view(np_, kc, 224, 16).permute(0, 1, 3, 2).reshape(np_, kc * 16, 224)
    # (U^T rows past Ci are padding the packer leaves unwritten: the GEMM must not read them, M must not depend on them)
    ref = torch.einsum("xct,xco->xot", V[:, :Ci].double(), U[:, :Ci, :Co].double())   # [points][Co][nt]
    got = M.cpu().view(np_, kco, nt, 16).permute(0, 1, 3, 2).reshape(np_, kco * 16, nt)[:, :Co]
    assert not bool(torch.isnan(got).any()), "M not fully written"
    _assert_close(got, ref, TOL_GEMM, (nt, Ci, Co, variant))


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv3d_wino_stack_bn_act / decnet_costvol_wino_stack_bn_act_cf (F(4,3)^3, C = 216, bf16x3 GEMM)
STACK = [  # (B, D, H, W, n_layers, res_src, res_dst)
    (1, 1, 2, 2, 2, -1, -1), (1, 2, 3, 3, 3, 0, 1), (1, 3, 2, 2, 7, 1, 4), (2, 2, 3, 2, 3, -1, -1),
    (1, 5, 3, 2, 7, 1, 4), (2, 3, 2, 3, 2, -1, -1),
]


def _layers(C, n, g):
    out = []
    for _ in range(n):
        w = _w(C, C, g)
        s, h = _bn(C, g)
        out.append((w, s, h))
    return out


def _run_stack(case, cf, aligned, C=216):
    """cf None: decnet_conv3d_wino_stack_bn_act on a volume x; else decnet_costvol_wino_stack_bn_act_cf on (left, right)."""
    B, D, H, W, n, rs, rd_ = case
    L = _L()
    g = _g("stack", case, cf)
    layers = _layers(C, n, g)
    us = [_pack_wino(w, 2) for w, _, _ in layers]
    P = Place(_dev(), aligned)
    sds = [P.inp(s) for _, s, _ in layers]
    hds = [P.inp(h) for _, _, h in layers]
    y = P.out((B, D, H, W, C))
    ws = _lib_buf(stack_ws_floats(B, D, H, W, C))
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ua, sa, ha = arr(us), arr(sds), arr(hds)
    if cf is None:
        x = torch.relu(torch.randn(B, D, H, W, C, generator=g))
        xd = P.inp(x)
        rc = L.decnet_conv3d_wino_stack_bn_act(xd.data_ptr(), ua, sa, ha, n, rs, rd_, y.data_ptr(), ws.data_ptr(), B, D,
                                               H, W, C, 2, _st())
    else:
        left, right = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        ld, rgt = P.inp(left), P.inp(right)
        x = R.costvol(left, right, D, cf)
        rc = L.decnet_costvol_wino_stack_bn_act_cf(ld.data_ptr(), rgt.data_ptr(), ua, sa, ha, n, rs, rd_, y.data_ptr(),
                                                   ws.data_ptr(), B, C, H, W, D, 2, cf, _st())
    assert rc == 0, rc
    P.check("stack %s %s" % (case, cf))
    return {"y": y.cpu(), "ref": R.stack(x, layers, n, rs, rd_)}


@pytest.mark.parametrize("case", STACK, ids=[str(i) for i in range(len(STACK))])
@pytest.mark.parametrize("cf", [None, COR, SSD, SUM], ids=["volume", "cor", "ssd", "sum"])
def test_wino_stack_edges(dev, case, cf):
    r = _both(_run_stack, case, cf)
    _assert_close(r["y"], r["ref"], TOL_STACK, (case, cf))


# shapes on either side of the LDS budgets (D, H, W): the return code tells which route a caller takes
STACK_IN, STACK_OUT = (16, 58, 10), (16, 59, 10)       # stack_lds_bytes 163328 / 166144
HEAD_IN, HEAD_OUT = (1, 51, 42), (1, 51, 43)           # head_lds_bytes 163512 / 165156


def test_lds_boundary_shapes():
    assert stack_lds_bytes(*STACK_IN) <= LDS < stack_lds_bytes(*STACK_OUT)
    assert head_lds_bytes(*STACK_IN) > LDS
    assert head_lds_bytes(*HEAD_IN) <= LDS < head_lds_bytes(*HEAD_OUT)


@pytest.mark.parametrize("shape,entry,want", [(STACK_IN, "volume", 0), (STACK_OUT, "volume", ERR_UNSUPPORTED),
                                              (STACK_IN, "head", ERR_UNSUPPORTED), (HEAD_IN, "head", 0),
                                              (HEAD_OUT, "head", ERR_UNSUPPORTED)],
                         ids=["stack_in", "stack_out", "stack_in_head_out", "head_in", "head_out"])
def test_wino_stack_lds_boundary(dev, shape, entry, want):
    """Two layers just inside / just outside the LDS budget: 0 and float64 parity, or -3 with nothing written."""
    D, H, W = shape
    case = (1, D, H, W, 2, -1, -1)
    if want == 0:
        r = _run_stack(case, None if entry == "volume" else COR, aligned=True)
        _assert_close(r["y"], r["ref"], TOL_STACK, shape)
        return
    L, C, n = _L(), 216, 2
    g = _g("lds", shape)
    us = [_pack_wino(_w(C, C, g), 2) for _ in range(n)]
    s = torch.ones(C, device=dev)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    x = torch.randn(1, D, H, W, C, device=dev)
    y = _lib_buf(D * H * W * C)
    ws = _lib_buf(stack_ws_floats(1, D, H, W, C))
    if entry == "volume":
        assert L.decnet_conv3d_wino_stack_workspace_floats(1, D, H, W, C, 2) == 0
        rc = L.decnet_conv3d_wino_stack_bn_act(x.data_ptr(), arr(us), arr([s, s]), arr([s, s]), n, -1, -1, y.data_ptr(),
                                               ws.data_ptr(), 1, D, H, W, C, 2, _st())
    else:
        lr = torch.randn(C * H * W, device=dev)
        rc = L.decnet_costvol_wino_stack_bn_act_cf(lr.data_ptr(), lr.data_ptr(), arr(us), arr([s, s]), arr([s, s]), n,
                                                   -1, -1, y.data_ptr(), ws.data_ptr(), 1, C, H, W, D, 2, COR, _st())
    assert rc == want, rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a declined stack wrote its output"


def test_wino_stack_rejects(dev):
    """CAT -2; H or W = 1 on the head -3; C != 216 -3; res_dst = n_layers - 1 -3; nothing written."""
    L, C = _L(), 216
    g = _g("rej")
    us = [_pack_wino(_w(C, C, g), 2) for _ in range(3)]
    s = torch.ones(C, device=dev)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    B, D, H, W = 1, 2, 3, 3
    lr = torch.randn(C * H * W * 2, device=dev)
    y = _lib_buf(D * H * W * C * 2)
    ws = _lib_buf(stack_ws_floats(B, D, H, W, C) * 2)
    ua, sa = arr(us), arr([s, s, s])
    f = L.decnet_costvol_wino_stack_bn_act_cf
    assert f(lr.data_ptr(), lr.data_ptr(), ua, sa, sa, 3, -1, -1, y.data_ptr(), ws.data_ptr(), B, C, H, W, D, 2, CAT,
             _st()) == ERR_BAD_SHAPE
    for hh, ww in ((1, 3), (3, 1)):
        assert f(lr.data_ptr(), lr.data_ptr(), ua, sa, sa, 3, -1, -1, y.data_ptr(), ws.data_ptr(), B, C, hh, ww, D, 2, COR,
                 _st()) == ERR_UNSUPPORTED
    assert f(lr.data_ptr(), lr.data_ptr(), ua, sa, sa, 3, 0, 2, y.data_ptr(), ws.data_ptr(), B, C, H, W, D, 2, COR,
             _st()) == ERR_UNSUPPORTED
    assert L.decnet_conv3d_wino_stack_bn_act(lr.data_ptr(), ua, sa, sa, 3, 0, 2, y.data_ptr(), ws.data_ptr(), B, D, H, W,
                                             C, 2, _st()) == ERR_UNSUPPORTED
    assert L.decnet_conv3d_wino_stack_bn_act(lr.data_ptr(), ua, sa, sa, 3, -1, -1, y.data_ptr(), ws.data_ptr(), B, D, H,
                                             W, 212, 2, _st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv3d_cout1_softargmax (one kernel) and _ws (tap GEMM KC 8 / 14 / 16 + gather, PB = 256 / D pixels per block)
COUT1 = [  # (B, D, H, W, Ci, saturate: None, "first" or "last")
    (1, 1, 2, 3, 4, None), (2, 2, 3, 2, 128, None), (1, 127, 2, 2, 132, None), (1, 128, 3, 2, 224, "first"),
    (1, 129, 2, 3, 228, "last"), (1, 256, 2, 2, 256, None), (2, 3, 5, 7, 4, "last"), (1, 256, 1, 3, 128, "first"),
    (3, 5, 1, 1, 256, None), (1, 2, 4, 5, 132, "last"),
]


def _cout1_inputs(case, g):
    B, D, H, W, Ci, sat = case
    if sat is None:
        return torch.randn(B, D, H, W, Ci, generator=g), _w(1, Ci, g), 1.3, -0.2
    # only the centre depth tap: plane d's cost sees x plane d alone, so the peak plane is unique by ~|cost| ~ 5e2
    x = torch.randn(B, D, H, W, Ci, generator=g) * 0.01
    x[:, 0 if sat == "first" else D - 1] += 1.0
    w = _w(1, Ci, g, pos=True)
    w[:, :, 0], w[:, :, 2] = 0, 0
    return x, w, 500.0 / float(w.sum()), 3.0


def _run_cout1(case, entry, with_reg, aligned):
    B, D, H, W, Ci, _ = case
    L = _L()
    x, w, scale, shift = _cout1_inputs(case, _g("cout1", case))
    P = Place(_dev(), aligned)
    xd, wd = P.inp(x), P.inp(w)
    reg = P.out((B, D, H, W)) if with_reg else None
    pred = P.out((B, H, W))
    rp = reg.data_ptr() if with_reg else None
    if entry == "one":
        rc = L.decnet_conv3d_cout1_softargmax(xd.data_ptr(), wd.data_ptr(), scale, shift, rp, pred.data_ptr(), B, D, H,
                                              W, Ci, _st())
    else:
        ws = _lib_buf(L.decnet_conv3d_cout1_workspace_floats(B, D, H, W))
        rc = L.decnet_conv3d_cout1_softargmax_ws(xd.data_ptr(), wd.data_ptr(), scale, shift, rp, pred.data_ptr(),
                                                 ws.data_ptr(), B, D, H, W, Ci, _st())
    assert rc == 0, rc
    P.check("cout1 %s %s" % (entry, case))
    out = {"pred": pred.cpu()}
    if with_reg:
        out["reg"] = reg.cpu()
    return out


@pytest.mark.parametrize("case", COUT1, ids=[str(i) for i in range(len(COUT1))])
@pytest.mark.parametrize("entry", ["one", "ws"])
@pytest.mark.parametrize("with_reg", [1, 0], ids=["reg", "noreg"])
def test_cout1_softargmax_edges(dev, case, entry, with_reg):
    r = _both(_run_cout1, case, entry, with_reg)
    x, w, scale, shift = _cout1_inputs(case, _g("cout1", case))
    reg_ref, pred_ref = R.cout1_softargmax(x, w, scale, shift)
    if with_reg:
        _assert_close(r["reg"], reg_ref, TOL_COUT1_REG, case)
    _pred_ok(r["pred"], pred_ref, TOL_COUT1_PRED, case)
    if case[-1] is not None:                                       # saturated: the soft-argmax is the peak plane
        assert float(reg_ref.abs().max()) > 100
        assert torch.equal(r["pred"].round(), pred_ref.round().float())


@pytest.mark.parametrize("D,Ci", [(2, 260), (257, 4)])
def test_cout1_beyond_the_ws_limits(dev, D, Ci):
    """Ci = 260 or D = 257: the one-kernel entry computes it, _ws returns -3 with nothing written."""
    case = (1, D, 2, 3, Ci, None)
    r = _both(_run_cout1, case, "one", 1)
    x, w, scale, shift = _cout1_inputs(case, _g("cout1", case))
    reg_ref, pred_ref = R.cout1_softargmax(x, w, scale, shift)
    _assert_close(r["reg"], reg_ref, TOL_COUT1_REG)
    _pred_ok(r["pred"], pred_ref, TOL_COUT1_PRED)
    L = _L()
    xd, wd = x.to(dev), w.to(dev)
    pred = _lib_buf(6)
    ws = _lib_buf(L.decnet_conv3d_cout1_workspace_floats(1, D, 2, 3))
    assert L.decnet_conv3d_cout1_softargmax_ws(xd.data_ptr(), wd.data_ptr(), 1.0, 0.0, None, pred.data_ptr(),
                                               ws.data_ptr(), 1, D, 2, 3, Ci, _st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(ws).all())


# ------------------------------------------------------------------------------------------------------------------
# decnet_disparity_regression (arbitrary samples)
REGR = [  # (B, S, H, W, samples kind, saturate: None, "first", "last")
    (1, 1, 2, 3, "arange", None), (3, 5, 7, 37, "nonmono", None), (2, 4, 16, 16, "negative", None),
    (1, 6, 3, 257, "repeated", None), (2, 9, 5, 5, "arange", "first"), (3, 9, 1, 300, "nonmono", "last"),
    (1, 1, 1, 1, "negative", "first"),
]


def _regr_inputs(case):
    B, S, H, W, kind, sat = case
    g = _g("regr", case)
    cost = torch.randn(B, S, H, W, generator=g) * 3
    if sat:
        cost = torch.randn(B, S, H, W, generator=g) * 50
        cost[:, 0 if sat == "first" else S - 1] = 900.0
    base = {"arange": torch.arange(S, dtype=torch.float32),
            "nonmono": torch.randperm(S, generator=g).float() * 1.5 - 2,
            "negative": -torch.rand(S, generator=g) * 40,
            "repeated": torch.tensor([3.0, 3.0, -1.0, 3.0, 7.5, -1.0][:S])}[kind]
    samples = (base.view(1, S, 1, 1) + torch.randn(B, S, H, W, generator=g) * 0.25).contiguous()
    return cost, samples


@pytest.mark.parametrize("case", REGR, ids=[str(i) for i in range(len(REGR))])
def test_disparity_regression_edges(dev, case):
    B, S, H, W, _, sat = case
    cost, samples = _regr_inputs(case)

    def run(aligned):
        P = Place(dev, aligned)
        cd, sd = P.inp(cost), P.inp(samples)
        pred = P.out((B, H, W))
        assert _L().decnet_disparity_regression(cd.data_ptr(), sd.data_ptr(), pred.data_ptr(), B, S, H, W, _st()) == 0
        P.check("disparity_regression")
        return {"pred": pred.cpu()}
    r = _both(run)
    ref = R.disparity_regression(cost, samples)
    _pred_ok(r["pred"], ref, TOL_REGRESSION_PRED, case)
    if sat:                                                         # e^-(900 - |50 x|) underflows: exactly the sample
        assert torch.equal(r["pred"], samples[:, 0 if sat == "first" else S - 1])


# ------------------------------------------------------------------------------------------------------------------
# decnet_stage0_forward / decnet_stage0_forward_cf
def auto_variant(D):
    return 2 if 216 * ((D + 3) // 4) <= 0.92 * 144 * ((D + 1) // 2) else 1


STAGE0 = [  # (B, C, H, W, D, variant, cost_func), route
    ((1, 4, 3, 5, 4, 0, COR), "layers"), ((2, 8, 2, 3, 5, 1, SSD), "layers"), ((1, 4, 2, 2, 7, 3, CAT), "layers"),
    ((1, 8, 4, 3, 6, -1, COR), "layers"), ((1, 216, 4, 7, 8, 2, COR), "head + stack"),
    ((1, 216, 3, 2, 5, -1, SSD), "layers"), ((2, 216, 2, 3, 3, -1, CAT), "head + stack"),
    ((1, 216) + STACK_IN[1:] + (STACK_IN[0], 2, COR), "volume + stack"), ((1, 216, 2, 3, 4, 3, COR), "layers"),
]


def _stage0_params(C, g):
    layers = _layers(C, 7, g)
    wl = _w(1, C, g)
    return layers + [(wl, torch.tensor(1.7), torch.tensor(0.3))]


def _run_stage0(case, with_reg, aligned):
    B, C, H, W, D, variant, cf = case
    L = _L()
    g = _g("stage0", case)
    params = _stage0_params(C, g)
    left, right = torch.relu(torch.randn(B, C, H, W, generator=g)), torch.relu(torch.randn(B, C, H, W, generator=g))
    w_pre = torch.randn(C, 2 * C, 1, 1, 1, generator=g) * (2.0 / C) ** 0.5 if cf == CAT else None
    v = auto_variant(D) if variant < 0 else variant
    ws_w = [_pack_direct(w) if v == 3 else _pack_wino(w, v) for w, _, _ in params[:7]]
    P = Place(_dev(), aligned)
    ld, rd = P.inp(left), P.inp(right)
    sds = [P.inp(s) for _, s, _ in params[:7]]
    hds = [P.inp(h) for _, _, h in params[:7]]
    wl = P.inp(params[7][0])
    wpd = P.inp(w_pre) if cf == CAT else None
    reg = P.out((B, D, H, W)) if with_reg else None
    pred = P.out((B, H, W))
    from decnet_amd import _lib
    prm = _lib.Stage0Params()
    for i in range(7):
        prm.w[i], prm.scale[i], prm.shift[i] = ws_w[i].data_ptr(), sds[i].data_ptr(), hds[i].data_ptr()
    prm.w_last, prm.scale_last, prm.shift_last = wl.data_ptr(), float(params[7][1]), float(params[7][2])
    # the stage-0 workspace is taken at any alignment (the entry moves its buffers to the first 16-byte boundary inside
    # it): it follows the placement, margins checked, contents scratch
    ws = P.inplace(torch.full((L.decnet_stage0_cf_workspace_floats(B, C, H, W, D, variant, cf),), float("nan")))
    rp = reg.data_ptr() if with_reg else None
    if cf == COR and not with_reg:
        rc = L.decnet_stage0_forward(ld.data_ptr(), rd.data_ptr(), ctypes.byref(prm), ws.data_ptr(), rp,
                                     pred.data_ptr(), B, C, H, W, D, variant, _st())
    else:
        rc = L.decnet_stage0_forward_cf(ld.data_ptr(), rd.data_ptr(), ctypes.byref(prm),
                                        wpd.data_ptr() if cf == CAT else None, ws.data_ptr(), rp, pred.data_ptr(), B, C,
                                        H, W, D, variant, cf, _st())
    assert rc == 0, rc
    P.check("stage0 %s" % (case,))
    out = {"pred": pred.cpu()}
    if with_reg:
        out["reg"] = reg.cpu()
    return out


@pytest.mark.parametrize("case,route", STAGE0, ids=[str(i) for i in range(len(STAGE0))])
@pytest.mark.parametrize("with_reg", [1, 0], ids=["reg", "noreg"])
def test_stage0_forward_edges(dev, case, route, with_reg):
    B, C, H, W, D, variant, cf = case
    v = auto_variant(D) if variant < 0 else variant
    fused = v == 2 and C == 216
    assert route == ("layers" if not fused else "head + stack" if head_lds_bytes(D, H, W) <= LDS else "volume + stack")
    r = _both(_run_stage0, case, with_reg)
    g = _g("stage0", case)
    params = _stage0_params(C, g)
    left, right = torch.relu(torch.randn(B, C, H, W, generator=g)), torch.relu(torch.randn(B, C, H, W, generator=g))
    w_pre = torch.randn(C, 2 * C, 1, 1, 1, generator=g) * (2.0 / C) ** 0.5 if cf == CAT else None
    reg_ref, pred_ref = R.stage0(left, right, params, D, cf, w_pre)
    if with_reg:
        _assert_close(r["reg"], reg_ref, TOL_STAGE0_REG, case)
    _pred_ok(r["pred"], pred_ref, TOL_STAGE0_PRED, case)


def test_stage0_forward_rejects_c_not_a_multiple_of_4(dev):
    L, B, C, H, W, D = _L(), 1, 6, 3, 4, 3
    from decnet_amd import _lib
    g = _g("c6")
    u = [_pack_wino(_w(C, C, g), 1) for _ in range(7)]
    s = torch.ones(C, device=dev)
    wl = torch.randn(1, C, 3, 3, 3, device=dev)
    prm = _lib.Stage0Params()
    for i in range(7):
        prm.w[i], prm.scale[i], prm.shift[i] = u[i].data_ptr(), s.data_ptr(), s.data_ptr()
    prm.w_last, prm.scale_last, prm.shift_last = wl.data_ptr(), 1.0, 0.0
    x = torch.randn(B, C, H, W, device=dev)
    ws = _lib_buf(max(L.decnet_stage0_workspace_floats(B, C, H, W, D, 1), 1 << 16))
    pred, reg = _lib_buf(B * H * W), _lib_buf(B * D * H * W)
    assert L.decnet_stage0_forward(x.data_ptr(), x.data_ptr(), ctypes.byref(prm), ws.data_ptr(), reg.data_ptr(),
                                   pred.data_ptr(), B, C, H, W, D, 1, _st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(reg).all())


# ------------------------------------------------------------------------------------------------------------------
# decnet_ncdhw_to_ndhwc / decnet_ndhwc_to_ncdhw: exact
@pytest.mark.parametrize("B,C,D,H,W", [(1, 1, 1, 1, 1), (2, 33, 1, 5, 7), (1, 31, 3, 2, 11), (3, 216, 2, 3, 6),
                                       (1, 65, 1, 1, 33)])
def test_transposes_edges(dev, B, C, D, H, W):
    x = torch.randn(B, C, D, H, W, generator=_g("tr", C, W))

    def run(aligned):
        P = Place(dev, aligned)
        xd = P.inp(x)
        y = P.out((B, D, H, W, C))
        assert _L().decnet_ncdhw_to_ndhwc(xd.data_ptr(), y.data_ptr(), B, C, D, H, W, _st()) == 0
        yd = P.inp(y.cpu())
        z = P.out((B, C, D, H, W))
        assert _L().decnet_ndhwc_to_ncdhw(yd.data_ptr(), z.data_ptr(), B, C, D, H, W, _st()) == 0
        P.check("transposes")
        return {"y": y.cpu(), "z": z.cpu()}
    r = _both(run)
    assert torch.equal(r["y"], R.ncdhw_to_ndhwc(x).float()) and torch.equal(r["z"], x)


# ------------------------------------------------------------------------------------------------------------------
# DECNET_ERR_MISALIGNED: the library-format buffers of the 3-D entries off a 16-byte boundary
def test_misaligned_library_buffers_are_rejected(dev):
    """Every packed weight and every workspace but the stage-0 one at an odd float offset: -5, nothing launched (the NaN-filled outputs and the
    sentinel-filled packed buffers keep their contents)."""
    L, st = _L(), _st()
    B, D, H, W, C = 1, 2, 3, 3, 216
    g = _g("mis")
    w = _w(C, C, g).to(dev)
    x = torch.randn(B, D, H, W, C, device=dev)
    lr = torch.randn(B, C, H, W, device=dev)
    s = torch.ones(C, device=dev)
    y = _lib_buf(B * D * H * W * C)
    pred = _lib_buf(B * H * W)
    nu = L.decnet_conv3d_wino_weight_floats(C, 2)
    u_ok = _pack_wino(w.cpu(), 2)
    u = _lib_buf(nu + 4, 7.0)
    wp = _lib_buf(27 * C * 224 + 4, 7.0)
    wp_ok = _pack_direct(w.cpu())
    ws = _lib_buf(max(L.decnet_stage0_workspace_floats(B, C, H, W, D, 2), stack_ws_floats(B, D, H, W, C)) + 4, 7.0)
    torch.cuda.synchronize()
    for off in (1, 2, 3):
        o = 4 * off
        assert L.decnet_conv3d_pack_weight(w.data_ptr(), wp.data_ptr() + o, C, C, st) == ERR_MISALIGNED
        assert L.decnet_conv3d_bn_act(x.data_ptr(), wp.data_ptr() + o, s.data_ptr(), s.data_ptr(), None, y.data_ptr(),
                                      B, D, H, W, C, C, 1, st) == ERR_MISALIGNED
        assert L.decnet_conv3d_wino_pack_weight(w.data_ptr(), u.data_ptr() + o, C, C, 2, st) == ERR_MISALIGNED
        for uo, wo in ((o, 0), (0, o)):
            up = (u_ok.data_ptr() if uo == 0 else u.data_ptr() + uo)
            assert L.decnet_conv3d_wino_bn_act(x.data_ptr(), up, s.data_ptr(), s.data_ptr(), None, y.data_ptr(),
                                               ws.data_ptr() + wo, B, D, H, W, C, C, 1, 2, st) == ERR_MISALIGNED
            n = 3
            ua = (ctypes.c_void_p * n)(u_ok.data_ptr(), up, u_ok.data_ptr())
            sa = (ctypes.c_void_p * n)(*([s.data_ptr()] * n))
            assert L.decnet_conv3d_wino_stack_bn_act(x.data_ptr(), ua, sa, sa, n, -1, -1, y.data_ptr(),
                                                     ws.data_ptr() + wo, B, D, H, W, C, 2, st) == ERR_MISALIGNED
            assert L.decnet_costvol_wino_stack_bn_act_cf(lr.data_ptr(), lr.data_ptr(), ua, sa, sa, n, -1, -1,
                                                         y.data_ptr(), ws.data_ptr() + wo, B, C, H, W, D, 2, COR,
                                                         st) == ERR_MISALIGNED
        for vo, uo, mo in ((o, 0, 0), (0, o, 0), (0, 0, o)):
            assert L.decnet_conv3d_wino_gemm(ws.data_ptr() + vo, u_ok.data_ptr() if uo == 0 else u.data_ptr() + uo,
                                             y.data_ptr() + mo, 1, C, C, 2, st) == ERR_MISALIGNED
        assert L.decnet_conv3d_cout1_softargmax_ws(x.data_ptr(), w.data_ptr(), 1.0, 0.0, None, pred.data_ptr(),
                                                   ws.data_ptr() + o, B, D, H, W, C, st) == ERR_MISALIGNED
        from decnet_amd import _lib
        for which in ("w", "w_direct"):            # (the stage-0 workspace may sit anywhere: test_stage0_forward_edges)
            prm = _lib.Stage0Params()
            for i in range(7):
                bad = i == 4
                src = (wp if which == "w_direct" else u) if bad else (wp_ok if which == "w_direct" else u_ok)
                prm.w[i] = src.data_ptr() + (o if bad else 0)
                prm.scale[i], prm.shift[i] = s.data_ptr(), s.data_ptr()
            prm.w_last, prm.scale_last, prm.shift_last = w.data_ptr(), 1.0, 0.0
            variant = 3 if which == "w_direct" else 2
            assert L.decnet_stage0_forward(lr.data_ptr(), lr.data_ptr(), ctypes.byref(prm), ws.data_ptr(), None,
                                           pred.data_ptr(), B, C, H, W, D, variant, st) == ERR_MISALIGNED
            assert L.decnet_stage0_forward_cf(lr.data_ptr(), lr.data_ptr(), ctypes.byref(prm), w.data_ptr(),
                                              ws.data_ptr(), None, pred.data_ptr(), B, C, H, W, D, variant, CAT,
                                              st) == ERR_MISALIGNED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(pred).all()), "a rejected call wrote its output"
    assert bool((u == 7.0).all()) and bool((wp == 7.0).all()) and bool((ws == 7.0).all()), "a rejected call wrote"


# ------------------------------------------------------------------------------------------------------------------
KNOBS = [  # environment switches read once per process, and the cases they change
    ({"DECNET_WINO_GEMM": "fp32"}, "conv3d_wino or wino_gemm or stage0_forward"),     # no fused stack: -3
    ({"DECNET_WINO_STACK": "0"}, "stage0_forward"),
    ({"DECNET_WINO_HEAD": "0"}, "stage0_forward"),
    ({"DECNET_WINO_CHUNK_MB": "0.05"}, "conv3d_wino or stage0_forward"),
]


@pytest.mark.parametrize("env,sel", KNOBS, ids=["gemm_fp32", "stack0", "head0", "chunk"])
def test_knob_leg(env, sel):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "(%s) and not knob_leg and not lds and not rejects" % sel],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
