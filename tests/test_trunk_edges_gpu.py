"""The 2-D trunk entries of include/decnet_hip.h (csrc/conv2d_small.hip, conv2d_mfma.hip, conv2d_mfma_acc2.hip,
tapconv.hip, maskgen.hip, unfold.hip) through the C ABI at edge shapes, against the float64 references of
tests/_trunk_ref.py.  Every case runs twice, with every buffer a window of a larger one:
  aligned    the windows start 16-byte aligned;
  unaligned  the windows start at an odd float offset (4 bytes past a 16-byte boundary; bit words: 8 bytes past).
Each run checks that the margins (G elements on each side, a sentinel) are intact, that every output element is written
(outputs are pre-filled with NaN), that the input windows are bit-identical to their host copies afterwards, and that the
call returns 0.  The two placements must give bit-identical results (no entry takes a different arithmetic path by
alignment: vector and scalar stores write the same values), and the aligned one must match float64 within the
tolerance of the kernel's existing test:
  small fp32 kernels 2e-5 * max(1, max|ref|); bf16x3 matrix-core kernels 4e-6; tap-conv 3e-5; unfold3_cat / s2d3_pad1
  exact; mask bits equal wherever |sigmoid - thold| > 1e-4.
Library-format buffers (the packed weights of the matrix-core kernels, the tap-conv V / u / T) are 16-byte aligned by
the header's rule; that misaligned ones are rejected with nothing launched is tested separately.
The knob legs at the end re-run the cases in child processes under the environment switches the kernels read once.
-m gpu."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import _trunk_ref as R
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _L, _assert_close, _bn, _both, _ints, _ptrs, _st, _vp

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv2d_bn_act / decnet_conv2d_cat_bn_act / decnet_conv2d_cat_epilogue (csrc/conv2d_small.hip)
SMALL = [  # (segments, Cout, k, dilation, (B, H, W), relu, epilogue)
    ((8,), 8, 3, 1, (2, 1, 1), 1, 0), ((8,), 8, 3, 1, (2, 2, 3), 1, 0), ((5,), 4, 3, 1, (1, 3, 2), 0, 0),
    ((8,), 8, 3, 1, (2, 5, 5), 1, 0), ((3,), 3, 3, 2, (1, 2, 5), 1, 0), ((8,), 8, 1, 1, (2, 3, 1), 1, 0),
    ((8,), 8, 3, 1, (1, 3, 255), 1, 0), ((4,), 24, 3, 2, (1, 2, 256), 1, 0), ((16,), 8, 3, 1, (2, 3, 257), 1, 0),
    ((8, 4), 12, 3, 1, (1, 2, 1025), 1, 0), ((3,), 1, 3, 1, (2, 3, 257), 0, 0), ((8,), 1, 1, 1, (1, 1, 1025), 0, 0),
    ((8,), 4, 3, 6, (2, 3, 5), 1, 0), ((4,), 8, 3, 9, (2, 2, 7), 0, 0), ((8,), 12, 3, 5, (1, 5, 5), 1, 0),
    ((12,), 24, 3, 4, (2, 3, 4), 1, 0), ((1, 1, 1, 1, 1, 1), 12, 3, 1, (2, 5, 33), 1, 0),
    ((1, 1, 1, 1, 1, 1), 3, 3, 2, (1, 3, 257), 0, 0), ((17,), 3, 3, 3, (1, 4, 64), 1, 0),
    ((8, 8, 1), 1, 3, 1, (2, 5, 257), 0, 1), ((4,), 1, 3, 2, (1, 1, 3), 0, 1), ((6, 1, 1), 1, 3, 1, (2, 3, 256), 1, 2),
    ((8,), 1, 1, 1, (1, 2, 5), 0, 2), ((2,), 1, 3, 7, (2, 2, 2), 0, 1),
]


def _run_small(case, aligned):
    segs, cout, k, dil, (B, H, W), relu, epi = case
    L, dev = _L(), torch.device("cuda:0")
    cin = sum(segs)
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + W)
    xs = [torch.randn(B, c, H, W, generator=g) for c in segs]
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale, shift = _bn(cout, g, 100.0 if epi == 1 else 1.0)        # epilogue 1: |conv| ~ 100, sigmoid saturates
    ea, eb = torch.randn(B, H, W, generator=g) * 30, torch.randn(B, H, W, generator=g) * 30
    P = Place(dev, aligned)
    xd = [P.inp(x) for x in xs]
    wd, sd, hd, ead, ebd = P.inp(w), P.inp(scale), P.inp(shift), P.inp(ea), P.inp(eb)
    wp = P.out((L.decnet_conv2d_packed_floats(cin, cout, k, 0),))
    st = _st()
    assert L.decnet_conv2d_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, k, 0, st) == 0
    y = P.out((B, cout, H, W))
    xa, ca = _ptrs(xd), _ints(segs)                                # kept alive across the calls
    if epi:
        rc = L.decnet_conv2d_cat_epilogue(_vp(xa), _vp(ca), len(segs), wp.data_ptr(),
                                          sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, H, W, k, dil, relu, epi,
                                          ead.data_ptr(), ebd.data_ptr() if epi == 1 else None, st)
    elif len(segs) == 1:
        rc = L.decnet_conv2d_bn_act(xd[0].data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, cin,
                                    cout, H, W, k, dil, relu, st)
    else:
        rc = L.decnet_conv2d_cat_bn_act(_vp(xa), _vp(ca), len(segs), wp.data_ptr(),
                                        sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, cout, H, W, k, dil, relu, st)
    assert rc == 0, rc
    P.check("small conv %s" % (case,))
    ref = R.conv_bn_act(xs, w, scale, shift, dil, relu)
    if epi:
        ref = R.epilogue(ref, epi, ea, eb)
    return {"y": y.cpu(), "ref": ref}


@pytest.mark.parametrize("case", SMALL, ids=[str(i) for i in range(len(SMALL))])
def test_small_conv_edges(dev, case):
    r = _both(_run_small, case)
    _assert_close(r["y"], r["ref"], 2e-5, case)


# decnet_deconv2d_k3s3_bn_act (Cout <= 8) and decnet_conv2d_k3s3_bn_act (Cout <= 24), csrc/conv2d_small.hip
S3 = [(1, 1, 4, 3), (2, 2, 8, 8), (4, 5, 3, 1), (5, 4, 9, 24), (2, 5, 24, 12), (1, 2, 1, 4)]   # (H, W, Cin, Cout)


def _run_stride3(H, W, cin, cout, transposed, aligned):
    L, dev, B = _L(), torch.device("cuda:0"), 2
    g = torch.Generator().manual_seed(H * 100 + W * 10 + cout + transposed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(*((cin, cout) if transposed else (cout, cin)), 3, 3, generator=g) / (cin * 9) ** 0.5
    scale, shift = _bn(cout, g)
    P = Place(dev, aligned)
    xd, wd, sd, hd = P.inp(x), P.inp(w), P.inp(scale), P.inp(shift)
    wp = P.out((L.decnet_conv2d_packed_floats(cin, cout, 3, transposed),))
    st = _st()
    assert L.decnet_conv2d_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, 3, transposed, st) == 0
    if transposed:
        y = P.out((B, cout, 3 * H, 3 * W))
        rc = L.decnet_deconv2d_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                           cin, cout, H, W, 1, st)
        ref = R.deconv_s3_bn_act(x, w, scale, shift, True)
    else:
        y = P.out((B, cout, (H - 1) // 3 + 1, (W - 1) // 3 + 1))
        rc = L.decnet_conv2d_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                         cin, cout, H, W, 1, st)
        ref = R.conv_s3_bn_act(x, w, scale, shift, True)
    assert rc == 0, rc
    P.check("stride 3")
    return {"y": y.cpu(), "ref": ref}


@pytest.mark.parametrize("H,W,cin,cout", S3)
@pytest.mark.parametrize("transposed", [0, 1])
def test_small_stride3_edges(dev, H, W, cin, cout, transposed):
    if transposed and cout > 8:
        cout = 8
    r = _both(_run_stride3, H, W, cin, cout, transposed)
    _assert_close(r["y"], r["ref"], 2e-5)


# ------------------------------------------------------------------------------------------------------------------
# decnet_conv2d_mfma_cat_bn_act / decnet_deconv2d_mfma_k3s3_bn_act (csrc/conv2d_mfma.hip, DECNET_CONV2D_ACC=2:
# conv2d_mfma_acc2.hip)
MFMA = [  # (segments, Cout, k, dilation, (B, H, W), relu)
    ((16,), 24, 3, 1, (1, 1, 1), 1), ((24,), 17, 3, 1, (2, 3, 5), 1), ((7,), 33, 3, 2, (1, 2, 15), 0),
    ((24,), 24, 3, 5, (1, 3, 5), 1), ((16,), 64, 3, 6, (2, 2, 2), 1), ((40,), 49, 3, 4, (1, 4, 4), 0),
    ((1,), 130, 3, 1, (1, 5, 17), 1), ((130,), 1, 3, 1, (1, 6, 20), 0), ((65, 7), 17, 3, 2, (3, 5, 9), 1),
    ((3, 1, 17, 40), 81, 3, 1, (2, 9, 23), 1), ((3, 1, 17, 40), 24, 1, 1, (3, 4, 7), 1),
    ((24,), 24, 3, 1, (1, 5, 16), 1), ((24,), 40, 3, 1, (2, 9, 64), 1), ((33,), 72, 3, 1, (1, 5, 260), 1),
    ((48,), 17, 1, 1, (1, 3, 260), 0), ((1, 1, 1, 1, 1, 1), 97, 3, 3, (2, 7, 12), 1),
]


def _run_mfma(case, aligned):
    segs, cout, k, dil, (B, H, W), relu = case
    L, dev = _L(), torch.device("cuda:0")
    cin = sum(segs)
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + W + dil)
    xs = [torch.randn(B, c, H, W, generator=g) for c in segs]
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale, shift = _bn(cout, g)
    P = Place(dev, aligned)
    xd = [P.inp(x) for x in xs]
    wd, sd, hd = P.inp(w), P.inp(scale), P.inp(shift)
    wp = torch.empty(L.decnet_conv2d_mfma_packed_bytes(cin, cout, k), dtype=torch.uint8, device=dev)   # library format
    st = _st()
    assert L.decnet_conv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, k, st) == 0
    y = P.out((B, cout, H, W))
    xa, ca = _ptrs(xd), _ints(segs)
    rc = L.decnet_conv2d_mfma_cat_bn_act(_vp(xa), _vp(ca), len(segs), wp.data_ptr(),
                                         sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, cout, H, W, k, dil, relu, st)
    assert rc == 0, rc
    P.check("mfma conv %s" % (case,))
    return {"y": y.cpu(), "ref": R.conv_bn_act(xs, w, scale, shift, dil, relu)}


@pytest.mark.parametrize("case", MFMA, ids=[str(i) for i in range(len(MFMA))])
def test_mfma_conv_edges(dev, case):
    r = _both(_run_mfma, case)
    _assert_close(r["y"], r["ref"], 4e-6, case)


def _run_mfma_deconv(B, H, W, cin, cout, aligned):
    L, dev = _L(), torch.device("cuda:0")
    g = torch.Generator().manual_seed(H * 100 + W * 10 + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cin, cout, 3, 3, generator=g) / cin ** 0.5
    scale, shift = _bn(cout, g)
    P = Place(dev, aligned)
    xd, wd, sd, hd = P.inp(x), P.inp(w), P.inp(scale), P.inp(shift)
    wp = torch.empty(L.decnet_deconv2d_mfma_packed_bytes(cin, cout), dtype=torch.uint8, device=dev)
    st = _st()
    assert L.decnet_deconv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, st) == 0
    y = P.out((B, cout, 3 * H, 3 * W))
    rc = L.decnet_deconv2d_mfma_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                            cin, cout, H, W, 1, st)
    assert rc == 0, rc
    P.check("mfma deconv")
    return {"y": y.cpu(), "ref": R.deconv_s3_bn_act(x, w, scale, shift, True)}


@pytest.mark.parametrize("H,W,cin,cout", [(1, 1, 16, 9), (2, 2, 72, 24), (4, 5, 9, 30), (5, 4, 40, 8), (1, 5, 1, 3)])
def test_mfma_deconv_edges(dev, H, W, cin, cout):
    r = _both(_run_mfma_deconv, 2, H, W, cin, cout)
    _assert_close(r["y"], r["ref"], 4e-6)


def test_mfma_rejects_what_the_header_excludes(dev):
    """Dilation 7 (k = 3) and a packed-weight buffer that is not 16-byte aligned: the documented error, no launch."""
    L, st = _L(), _st()
    cin, cout, B, H, W = 16, 24, 1, 9, 20
    x = torch.randn(B, cin, H, W, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev)
    s, h = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    nb = L.decnet_conv2d_mfma_packed_bytes(cin, cout, 3)
    wbuf = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
    assert L.decnet_conv2d_mfma_pack_weight(w.data_ptr(), wbuf.data_ptr(), cin, cout, 3, st) == 0
    y = torch.full((B, cout, H, W), float("nan"), device=dev)
    xa, ca = _ptrs([x]), _ints([cin])
    xs, segs = _vp(xa), _vp(ca)
    assert L.decnet_conv2d_mfma_cat_bn_act(xs, segs, 1, wbuf.data_ptr(), s.data_ptr(), h.data_ptr(), y.data_ptr(),
                                           B, cout, H, W, 3, 7, 1, st) == ERR_UNSUPPORTED
    for off in (4, 8):
        assert L.decnet_conv2d_mfma_pack_weight(w.data_ptr(), wbuf.data_ptr() + off, cin, cout, 3, st) == ERR_MISALIGNED
        assert L.decnet_conv2d_mfma_cat_bn_act(xs, segs, 1, wbuf.data_ptr() + off, s.data_ptr(), h.data_ptr(),
                                               y.data_ptr(), B, cout, H, W, 3, 1, 1, st) == ERR_MISALIGNED
        assert L.decnet_deconv2d_mfma_pack_weight(w.data_ptr(), wbuf.data_ptr() + off, cin, 2, st) == ERR_MISALIGNED
        assert L.decnet_deconv2d_mfma_k3s3_bn_act(x.data_ptr(), wbuf.data_ptr() + off, s.data_ptr(), h.data_ptr(),
                                                  y.data_ptr(), B, cin, 2, 3, 3, 1, st) == ERR_MISALIGNED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a rejected call wrote its output"


# ------------------------------------------------------------------------------------------------------------------
# decnet_s2d3_pad1, decnet_unfold3_cat (csrc/unfold.hip): exact
@pytest.mark.parametrize("B,C,H,W", [(2, 1, 1, 1), (2, 1, 2, 4), (2, 3, 4, 5), (2, 2, 5, 2), (1, 1, 7, 771),
                                     (2, 2, 3, 768), (1, 1, 2, 772)])
def test_s2d3_edges(dev, B, C, H, W):
    def run(aligned):
        g = torch.Generator().manual_seed(H * 1000 + W)
        x = torch.randn(B, C, H, W, generator=g)
        P = Place(dev, aligned)
        xd = P.inp(x)
        out = P.out((B, 9 * C, (H - 1) // 3 + 1, (W - 1) // 3 + 1))
        assert _L().decnet_s2d3_pad1(xd.data_ptr(), out.data_ptr(), B, C, H, W, _st()) == 0
        P.check("s2d3")
        return {"y": out.cpu(), "ref": R.s2d3_pad1(x).float()}
    r = _both(lambda aligned: run(aligned))
    assert torch.equal(r["y"], r["ref"])


@pytest.mark.parametrize("B,C,h,w", [(2, 1, 1, 1), (1, 3, 1, 257), (2, 1, 2, 255), (3, 2, 3, 256), (1, 5, 4, 1)])
def test_unfold3_edges(dev, B, C, h, w):
    def run(aligned):
        g = torch.Generator().manual_seed(h * 1000 + w + C)
        fea, disp = torch.randn(B, C, 3 * h, 3 * w, generator=g), torch.randn(B, h, w, generator=g)
        P = Place(dev, aligned)
        fd, dd = P.inp(fea), P.inp(disp)
        out = P.out((B, 9 * C + 1, h, w))
        assert _L().decnet_unfold3_cat(fd.data_ptr(), dd.data_ptr(), out.data_ptr(), B, C, h, w, _st()) == 0
        P.check("unfold3_cat")
        return {"y": out.cpu(), "ref": R.unfold3_cat(fea, disp).float()}
    r = _both(lambda aligned: run(aligned))
    assert torch.equal(r["y"], r["ref"])


# ------------------------------------------------------------------------------------------------------------------
# decnet_warp_disparity, decnet_dynamic_upsample3 (csrc/conv2d_small.hip)
@pytest.mark.parametrize("B,C,H,W", [(1, 1, 2, 2), (2, 7, 2, 2), (3, 9, 3, 257), (1, 17, 4, 255), (2, 8, 2, 300)])
def test_warp_edges(dev, B, C, H, W):
    """Reference: float64 bilinear interpolation at the sample position computed with the float32 rounding of the
    reference's own grid (warp_coords, dtype float32): with a float64 position the float32 rounding of ix ~ W alone
    moves wide rows by ~1e-4 (tests/test_trunk_ref_cpu.py), a property of the reference, not of the kernel."""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + W)
    right = torch.randn(B, C, H, W, generator=g)
    for i, disp in enumerate(R.warp_disparities(B, H, W, g)):
        disp = disp.float()

        def run(aligned):
            P = Place(dev, aligned)
            rd, dd = P.inp(right), P.inp(disp)
            out = P.out((B, C, H, W))
            assert _L().decnet_warp_disparity(rd.data_ptr(), dd.data_ptr(), out.data_ptr(), B, C, H, W, _st()) == 0
            P.check("warp")
            return {"y": out.cpu()}
        r = _both(run)
        _assert_close(r["y"], R.warp(right, disp, coord_dtype=torch.float32), 2e-5, ("disparity kind", i))


@pytest.mark.parametrize("B,h,w,spread", [(1, 1, 1, 80.0), (3, 1, 1, 0.0), (3, 2, 255, 80.0), (1, 3, 256, 0.0),
                                          (2, 2, 257, 80.0), (3, 4, 5, 3.0)])
def test_upsample3_edges(dev, B, h, w, spread):
    """Logits spread over +-80 (softmax weights from 1 down to e^-160) or all equal (spread 0: weights 1/9)."""
    def run(aligned):
        g = torch.Generator().manual_seed(B * 1000 + h * 10 + w)
        logits = (torch.rand(B, 81, h, w, generator=g) * 2 - 1) * spread
        disp = torch.rand(B, h, w, generator=g) * 50 - 10
        P = Place(dev, aligned)
        ld, dd = P.inp(logits), P.inp(disp)
        out = P.out((B, 3 * h, 3 * w))
        assert _L().decnet_dynamic_upsample3(ld.data_ptr(), dd.data_ptr(), out.data_ptr(), B, h, w, _st()) == 0
        P.check("dynamic_upsample3")
        return {"y": out.cpu(), "ref": R.dynamic_upsample3(logits, disp)}
    r = _both(run)
    _assert_close(r["y"], r["ref"], 2e-5)


# ------------------------------------------------------------------------------------------------------------------
# tap-conv chain decnet_tapconv_to_chunks -> decnet_tap_gemm -> decnet_tapconv_gather (csrc/tapconv.hip)
TAP = [  # (Ci, Co, (B, H, W), branches as (k, dilation))
    (4, 1, (2, 3, 4), ((1, 1), (3, 3), (3, 4), (3, 9))),
    (20, 17, (2, 2, 5), ((1, 1), (3, 2), (3, 5), (3, 6))),
    (216, 224, (2, 3, 4), ((1, 1), (3, 1), (3, 4), (3, 5))),
    (216, 17, (2, 5, 7), ((1, 1), (3, 2), (3, 7), (3, 8))),
    (20, 224, (1, 1, 1), ((3, 1),)),
    (4, 17, (2, 1, 70), ((3, 1), (1, 1))),
]


def _run_tap(case, split, aligned):
    Ci, Co, (B, H, W), brs = case
    L, dev, st = _L(), torch.device("cuda:0"), _st()
    g = torch.Generator().manual_seed(Ci * 1000 + Co + H)
    x = torch.randn(B, Ci, H, W, generator=g)
    ws = [torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5 for k, _ in brs]
    nb = len(brs)
    scale, shift = _bn(nb * Co, g)
    ks, dils = [k for k, _ in brs], [d for _, d in brs]
    tap0 = [sum(k * k for k in ks[:i]) for i in range(nb)]
    ntaps = sum(k * k for k in ks)
    P = Place(dev, aligned)
    xd, sd, hd = P.inp(x), P.inp(scale), P.inp(shift)
    wds = [P.inp(w) for w in ws]
    # library-format buffers: 16-byte aligned (the header's rule)
    u = torch.full((L.decnet_tapconv_weight_floats(Ci, ntaps),), float("nan"), device=dev)
    for wd, t0, k in zip(wds, tap0, ks):
        assert L.decnet_tapconv_pack_weight(wd.data_ptr(), u.data_ptr(), Co, Ci, k, t0, st) == 0
    if split:
        assert L.decnet_tapconv_split_weight(u.data_ptr(), Ci, ntaps, st) == 0
    Pn = B * H * W
    V = torch.full((L.decnet_tapconv_chunk_floats(B, Ci, H, W),), float("nan"), device=dev)
    T = torch.full((ntaps * ((Co + 15) // 16) * 16 * Pn,), float("nan"), device=dev)
    y = P.out((B, nb * Co, H, W))
    assert L.decnet_tapconv_to_chunks(xd.data_ptr(), V.data_ptr(), B, Ci, H, W, st) == 0
    assert L.decnet_tap_gemm(V.data_ptr(), u.data_ptr(), T.data_ptr(), Pn, Ci, Co, ntaps, split, st) == 0
    assert L.decnet_tapconv_gather(T.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, Co, H, W, nb,
                                   _ints(tap0), _ints(ks), _ints(dils), 1, st) == 0
    P.check("tap-conv %s" % ((Ci, Co, B, H, W),))
    return {"y": y.cpu(), "ref": R.tap_gather(R.tap_gemm(x, ws), ks, dils, scale, shift, True)}


@pytest.mark.parametrize("case", TAP, ids=[str(i) for i in range(len(TAP))])
@pytest.mark.parametrize("split", [0, 1])
def test_tapconv_edges(dev, case, split):
    """B = 2 with dilations >= H and >= W: a tap that would cross into the neighbouring image (P = B H W positions in
    one row of T) must be skipped, which the float64 gather does by construction."""
    r = _both(_run_tap, case, split)
    _assert_close(r["y"], r["ref"], 3e-5, case)


def test_tapconv_rejects_misaligned_workspaces(dev):
    """V, u and T off a 16-byte boundary: DECNET_ERR_MISALIGNED and nothing launched (the buffers keep their NaN)."""
    L, st = _L(), _st()
    B, Ci, Co, H, W = 1, 16, 16, 3, 4
    x = torch.randn(B, Ci, H, W, device=dev)
    w = torch.randn(Co, Ci, 3, 3, device=dev)
    nu, nv, nt = L.decnet_tapconv_weight_floats(Ci, 9), L.decnet_tapconv_chunk_floats(B, Ci, H, W), 9 * 16 * B * H * W
    u = torch.full((nu + 4,), float("nan"), device=dev)
    V = torch.full((nv + 4,), float("nan"), device=dev)
    T = torch.full((nt + 4,), float("nan"), device=dev)
    assert L.decnet_tapconv_pack_weight(w.data_ptr(), u.data_ptr(), Co, Ci, 3, 0, st) == 0
    assert L.decnet_tapconv_to_chunks(x.data_ptr(), V.data_ptr(), B, Ci, H, W, st) == 0
    torch.cuda.synchronize()
    u_before, V_before = u.clone(), V.clone()
    for off in (1, 2, 3):
        assert L.decnet_tapconv_to_chunks(x.data_ptr(), V[off:].data_ptr(), B, Ci, H, W, st) == ERR_MISALIGNED
        assert L.decnet_tapconv_pack_weight(w.data_ptr(), u[off:].data_ptr(), Co, Ci, 3, 0, st) == ERR_MISALIGNED
        assert L.decnet_tapconv_split_weight(u[off:].data_ptr(), Ci, 9, st) == ERR_MISALIGNED
        for vo, uo, to in ((off, 0, 0), (0, off, 0), (0, 0, off)):
            assert L.decnet_tap_gemm(V[vo:].data_ptr(), u[uo:].data_ptr(), T[to:].data_ptr(), B * H * W, Ci, Co, 9, 0,
                                     st) == ERR_MISALIGNED
    torch.cuda.synchronize()
    assert bool(torch.isnan(T).all()), "a rejected decnet_tap_gemm wrote T"
    assert torch.equal(u.nan_to_num(7.0), u_before.nan_to_num(7.0)) and torch.equal(V.nan_to_num(7.0),
                                                                                    V_before.nan_to_num(7.0))


# ------------------------------------------------------------------------------------------------------------------
# decnet_detail_mask (csrc/maskgen.hip)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (3, 64), (2, 65), (1, 129), (4, 8)])
@pytest.mark.parametrize("want", ["mask", "logits", "bits", "all"])
def test_detail_mask_edges(dev, H, W, want):
    B = 2
    g = torch.Generator().manual_seed(H * 1000 + W)
    cur, pre = torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)
    w3 = torch.randn(3, 3, 3, 3, generator=g) * 0.3
    s3, b3 = _bn(3, g)
    w1 = torch.randn(3, generator=g)
    s1, b1 = 1.3, -0.2
    z = R.detail_logits(cur, pre, w3, s3, b3, w1, s1, b1)
    sig = torch.sigmoid(z)
    thold = float(sig.flatten().float().median()) if sig.numel() > 2 else float(sig.mean())
    fl = lambda t: (ctypes.c_float * t.numel())(*t.reshape(-1).tolist())
    nw = (W + 63) // 64

    def run(aligned):
        P = Place(dev, aligned)
        cd, pd = P.inp(cur), P.inp(pre)
        mask = P.out((B, H, W))
        logits = P.out((B, H, W)) if want in ("logits", "all") else None
        bits = P.out((B, H, nw), torch.int64, -1) if want in ("bits", "all") else None
        rc = _L().decnet_detail_mask(cd.data_ptr(), pd.data_ptr(), fl(w3), fl(s3), fl(b3), fl(w1), s1, b1, thold,
                                     mask.data_ptr(), logits.data_ptr() if logits is not None else None,
                                     bits.data_ptr() if bits is not None else None, B, H, W, _st())
        assert rc == 0, rc
        P.check("detail_mask")
        r = {"mask": mask.cpu()}
        if logits is not None:
            r["logits"] = logits.cpu()
        if bits is not None:
            r["bits"] = bits.cpu()
        return r
    r = _both(run)
    sure = (sig - thold).abs() > 1e-4
    ref = sig > thold
    assert bool((r["mask"] == ref.float())[sure].all()), "mask differs away from the threshold"
    assert set(r["mask"].unique().tolist()) <= {0.0, 1.0}
    if "logits" in r:
        _assert_close(r["logits"], z, 2e-5)
    if "bits" in r:
        words = r["bits"]
        unpacked = ((words.unsqueeze(-1) >> torch.arange(64)) & 1).reshape(B, H, nw * 64).bool()
        assert not bool(unpacked[:, :, W:].any()), "bits past W must be zero"
        assert torch.equal(unpacked[:, :, :W], r["mask"].bool()), "bits and float mask disagree"
        assert torch.equal(words[sure.all(-1)], R.pack_bits(ref)[sure.all(-1)])


# ------------------------------------------------------------------------------------------------------------------
# decnet_bias_act_inplace (csrc/conv2d_small.hip)
@pytest.mark.parametrize("B,C,H,W", [(1, 2, 1, 5), (2, 3, 2, 3), (2, 1, 3, 5), (1, 3, 4, 4), (2, 2, 7, 37)])
@pytest.mark.parametrize("relu", [0, 1])
def test_bias_act_edges(dev, B, C, H, W, relu):
    """H W % 4 = 1, 2, 3 and 0; in place, so the planes of one call sit at every alignment.  Exact: one float32 add
    (the float64 sum of two floats rounded once) and a max."""
    g = torch.Generator().manual_seed(H * W + C)
    y, shift = torch.randn(B, C, H, W, generator=g), torch.randn(C, generator=g)

    def run(aligned):
        P = Place(dev, aligned)
        yd, sd = P.inplace(y), P.inp(shift)
        assert _L().decnet_bias_act_inplace(yd.data_ptr(), sd.data_ptr(), B, C, H, W, relu, _st()) == 0
        P.check("bias_act_inplace")
        return {"y": yd.cpu()}
    r = _both(run)
    assert torch.equal(r["y"], R.bias_act(y, shift, relu).float())


# ------------------------------------------------------------------------------------------------------------------
KNOBS = [  # environment switches read once per process, and the cases they change
    ({"DECNET_CONV2D_SMALL": "mfma", "DECNET_NT_MB": "0"}, "small_conv"),
    ({"DECNET_CONV2D_SMALL": "valu", "DECNET_NT_MB": "0"}, "small_conv"),
    ({"DECNET_CONV2D_ACC": "2"}, "mfma"),
    ({"DECNET_CONV2D_MFMA_TM": "2"}, "mfma_conv"),
    ({"DECNET_CONV2D_MFMA_PC": "0"}, "mfma"),
]


@pytest.mark.parametrize("env,sel", KNOBS, ids=["small_mfma", "small_valu", "acc2", "tm2", "pc0"])
def test_knob_leg(env, sel):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "%s and not knob_leg" % sel], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
