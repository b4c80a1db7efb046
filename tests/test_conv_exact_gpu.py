"""The forward convolution entries of include/decnet_hip.h through the C ABI on exact data, bit for bit against the float64
references of tests/_trunk_ref.py and tests/_stage0_ref.py.  There is no tolerance in this module: the data
(tests/_exact.py) are chosen so that the float64 result is representable in fp32 and every partial sum is exact in any
order, so a correct kernel must return it bit for bit.
  dense    small integers at the shapes of the edge tables (test_trunk_edges_gpu.py, test_stage0_edges_gpu.py): indexing,
           halos, K tails, segment boundaries and the accumulation, on every fp32 and matrix-core kernel;
  select   one nonzero weight per output channel on one-, two- and three-term bf16 data: every one of the six term
           products of the bf16x3 kernels, on every input channel and tap (tests/test_exact_cpu.py proves on the host
           which pairing pins which product, and that the tables cover every channel, tap, chunk edge and segment edge).
One aligned guarded placement per case (margins, NaN pre-fill, inputs unmodified); the edge modules prove the two
placements and the LDS poison bit-identical at these shapes.  The knob legs re-run the module in child processes under
the switches the kernels read once per process: exact data stay exact under every one of them.  -m gpu."""
import os
import subprocess
import sys

import pytest
import torch

import _exact as E
import _stage0_ref as R0
import _trunk_ref as R
from _placement import Place, _L, _bits_equal, _ints, _ptrs, _st, _vp

pytestmark = pytest.mark.gpu
TAB = E.tables()
PAIR_IDS = ["T3xT1", "T1xT3", "T2xT2"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _dev():
    return torch.device("cuda:0")


def _lib_buf(n, dtype=torch.float32):
    """A library-format buffer: a fresh (16-byte aligned) allocation, NaN (bytes: 0xff) inside."""
    t = torch.full((max(int(n), 1),), float("nan") if dtype == torch.float32 else 255, dtype=dtype, device=_dev())
    assert t.data_ptr() % 16 == 0
    return t


def _same(got, ref64, what, unit=None):
    want = E.exact_or_fail(ref64, unit)
    if not _bits_equal(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ from float64, first at %s: %r != %r" % (
            what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------------------------------
# the entries, on given data
def _small(xs, w, scale, shift, k, dil, relu):
    L, st = _L(), _st()
    segs, cout = [x.shape[1] for x in xs], w.shape[0]
    cin, (B, _, H, W) = sum(segs), xs[0].shape
    P = Place(_dev(), True)
    xd, wd, sd, hd = [P.inp(x) for x in xs], P.inp(w), P.inp(scale), P.inp(shift)
    wp = P.out((L.decnet_conv2d_packed_floats(cin, cout, k, 0),))
    assert L.decnet_conv2d_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, k, 0, st) == 0
    y = P.out((B, cout, H, W))
    xa, ca = _ptrs(xd), _ints(segs)
    if len(segs) == 1:
        rc = L.decnet_conv2d_bn_act(xd[0].data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, cin,
                                    cout, H, W, k, dil, relu, st)
    else:
        rc = L.decnet_conv2d_cat_bn_act(_vp(xa), _vp(ca), len(segs), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                        y.data_ptr(), B, cout, H, W, k, dil, relu, st)
    assert rc == 0, rc
    P.check("small conv")
    return y.cpu()


def _stride3(x, w, scale, shift, transposed):
    L, st = _L(), _st()
    B, cin, H, W = x.shape
    cout = w.shape[1] if transposed else w.shape[0]
    P = Place(_dev(), True)
    xd, wd, sd, hd = P.inp(x), P.inp(w), P.inp(scale), P.inp(shift)
    wp = P.out((L.decnet_conv2d_packed_floats(cin, cout, 3, transposed),))
    assert L.decnet_conv2d_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, 3, transposed, st) == 0
    if transposed:
        y = P.out((B, cout, 3 * H, 3 * W))
        rc = L.decnet_deconv2d_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                           cin, cout, H, W, 1, st)
    else:
        y = P.out((B, cout, (H - 1) // 3 + 1, (W - 1) // 3 + 1))
        rc = L.decnet_conv2d_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                         cin, cout, H, W, 1, st)
    assert rc == 0, rc
    P.check("stride 3")
    return y.cpu()


def _mfma(xs, w, scale, shift, k, dil, relu):
    L, st = _L(), _st()
    segs, cout = [x.shape[1] for x in xs], w.shape[0]
    cin, (B, _, H, W) = sum(segs), xs[0].shape
    P = Place(_dev(), True)
    xd, wd, sd, hd = [P.inp(x) for x in xs], P.inp(w), P.inp(scale), P.inp(shift)
    wp = _lib_buf(L.decnet_conv2d_mfma_packed_bytes(cin, cout, k), torch.uint8)
    assert L.decnet_conv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, k, st) == 0
    y = P.out((B, cout, H, W))
    xa, ca = _ptrs(xd), _ints(segs)
    rc = L.decnet_conv2d_mfma_cat_bn_act(_vp(xa), _vp(ca), len(segs), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                         y.data_ptr(), B, cout, H, W, k, dil, relu, st)
    assert rc == 0, rc
    P.check("mfma conv")
    return y.cpu()


def _mfma_deconv(x, w, scale, shift, relu=1):
    L, st = _L(), _st()
    (B, cin, H, W), cout = x.shape, w.shape[1]
    P = Place(_dev(), True)
    xd, wd, sd, hd = P.inp(x), P.inp(w), P.inp(scale), P.inp(shift)
    wp = _lib_buf(L.decnet_deconv2d_mfma_packed_bytes(cin, cout), torch.uint8)
    assert L.decnet_deconv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, st) == 0
    y = P.out((B, cout, 3 * H, 3 * W))
    rc = L.decnet_deconv2d_mfma_k3s3_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B,
                                            cin, cout, H, W, relu, st)
    assert rc == 0, rc
    P.check("mfma deconv")
    return y.cpu()


def _tap(x, ws, brs, split, scale=None, shift=None):
    """to_chunks -> tap_gemm (-> gather when scale is given).  Returns y, or T as [ntaps][Co][P]."""
    L, st = _L(), _st()
    (B, Ci, H, W), Co, nb = x.shape, ws[0].shape[0], len(brs)
    ks, dils = [k for k, _ in brs], [d for _, d in brs]
    tap0 = [sum(k * k for k in ks[:i]) for i in range(nb)]
    ntaps, Pn, kco = sum(k * k for k in ks), B * H * W, (Co + 15) // 16
    P = Place(_dev(), True)
    xd, wds = P.inp(x), [P.inp(w) for w in ws]
    u = _lib_buf(L.decnet_tapconv_weight_floats(Ci, ntaps))
    for wd, t0, k in zip(wds, tap0, ks):
        assert L.decnet_tapconv_pack_weight(wd.data_ptr(), u.data_ptr(), Co, Ci, k, t0, st) == 0
    if split:
        assert L.decnet_tapconv_split_weight(u.data_ptr(), Ci, ntaps, st) == 0
    V = _lib_buf(L.decnet_tapconv_chunk_floats(B, Ci, H, W))
    T = _lib_buf(ntaps * kco * 16 * Pn)
    assert L.decnet_tapconv_to_chunks(xd.data_ptr(), V.data_ptr(), B, Ci, H, W, st) == 0
    assert L.decnet_tap_gemm(V.data_ptr(), u.data_ptr(), T.data_ptr(), Pn, Ci, Co, ntaps, split, st) == 0
    if scale is None:
        P.check("tap gemm")
        return T.cpu().view(ntaps, kco, Pn, 16).permute(0, 1, 3, 2).reshape(ntaps, kco * 16, Pn)[:, :Co]
    sd, hd = P.inp(scale), P.inp(shift)
    y = P.out((B, nb * Co, H, W))
    assert L.decnet_tapconv_gather(T.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, Co, H, W, nb,
                                   _ints(tap0), _ints(ks), _ints(dils), 1, st) == 0
    P.check("tap-conv")
    return y.cpu()


def _pack_wino(w, variant):
    L = _L()
    Co, Ci = w.shape[:2]
    u = _lib_buf(L.decnet_conv3d_wino_weight_floats(Ci, variant))
    assert L.decnet_conv3d_wino_pack_weight(w.to(_dev()).data_ptr(), u.data_ptr(), Co, Ci, variant, _st()) == 0
    return u


def _conv3d(x, w, scale, shift, resid, relu, algo):
    L, st = _L(), _st()
    (B, D, H, W, Ci), Co = x.shape, w.shape[0]
    if algo == "direct":
        wp = _lib_buf(27 * Ci * L.decnet_conv3d_packed_cout(Co))
        assert L.decnet_conv3d_pack_weight(w.to(_dev()).data_ptr(), wp.data_ptr(), Co, Ci, st) == 0
    else:
        wp = _pack_wino(w, algo)
    P = Place(_dev(), True)
    xd, sd, hd = P.inp(x), P.inp(scale), P.inp(shift)
    rp = P.inp(resid).data_ptr() if resid is not None else None
    y = P.out((B, D, H, W, Co))
    if algo == "direct":
        rc = L.decnet_conv3d_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), rp, y.data_ptr(),
                                    B, D, H, W, Ci, Co, relu, st)
    else:
        ws = _lib_buf(L.decnet_conv3d_wino_workspace_floats(B, D, H, W, Ci, Co, algo))
        rc = L.decnet_conv3d_wino_bn_act(xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), rp, y.data_ptr(),
                                         ws.data_ptr(), B, D, H, W, Ci, Co, relu, algo, st)
    assert rc == 0, rc
    P.check("conv3d %s" % algo)
    return y.cpu()


# ------------------------------------------------------------------------------------------------------------------
# dense small integers
@pytest.mark.parametrize("case", TAB["small"], ids=[str(i) for i in range(len(TAB["small"]))])
def test_dense_small_conv(dev, case):
    segs, cout, k, dil, (B, H, W), relu, _ = case
    xs, w, scale, shift = E.dense2d(case, segs, cout, k, B, H, W)
    _same(_small(xs, w, scale, shift, k, dil, relu), R.conv_bn_act(xs, w, scale, shift, dil, relu), case, 0.5)


@pytest.mark.parametrize("row,transposed", TAB["s3"], ids=["%s%d" % (("conv", "deconv")[tr], i % 6) for i, (_, tr) in enumerate(TAB["s3"])])
def test_dense_small_stride3(dev, row, transposed):
    H, W, cin, cout = row
    (x,), w, scale, shift = E.dense2d(("s3", H, W, cin, cout, transposed), (cin,), cout, 3, 2, H, W, transposed)
    ref = (R.deconv_s3_bn_act if transposed else R.conv_s3_bn_act)(x, w, scale, shift, True)
    _same(_stride3(x, w, scale, shift, transposed), ref, (row, transposed), 0.5)


@pytest.mark.parametrize("case", TAB["mfma"], ids=[str(i) for i in range(len(TAB["mfma"]))])
def test_dense_mfma_conv(dev, case):
    segs, cout, k, dil, (B, H, W), relu = case
    xs, w, scale, shift = E.dense2d(case, segs, cout, k, B, H, W)
    _same(_mfma(xs, w, scale, shift, k, dil, relu), R.conv_bn_act(xs, w, scale, shift, dil, relu), case, 0.5)


@pytest.mark.parametrize("H,W,cin,cout", TAB["deconv"])
def test_dense_mfma_deconv(dev, H, W, cin, cout):
    (x,), w, scale, shift = E.dense2d(("deconv", H, W, cin, cout), (cin,), cout, 3, 2, H, W, True)
    _same(_mfma_deconv(x, w, scale, shift), R.deconv_s3_bn_act(x, w, scale, shift, True), (H, W, cin, cout), 0.5)


@pytest.mark.parametrize("case", TAB["tap"], ids=[str(i) for i in range(len(TAB["tap"]))])
@pytest.mark.parametrize("split", [0, 1])
def test_dense_tapconv(dev, case, split):
    brs = case[3]
    x, ws, scale, shift = E.dense_tap(case)
    ref = R.tap_gather(R.tap_gemm(x, ws), [k for k, _ in brs], [d for _, d in brs], scale, shift, True)
    _same(_tap(x, ws, brs, split, scale, shift), ref, (case, split), 0.5)


@pytest.mark.parametrize("case", TAB["conv"], ids=[str(i) for i in range(len(TAB["conv"]))])
def test_dense_conv3d_direct(dev, case):
    x, w, scale, shift, resid = E.dense3d(case)
    _same(_conv3d(x, w, scale, shift, resid, case[6], "direct"), R0.conv3d_unit(x, w, scale, shift, resid, case[6]),
          case, 0.5)


@pytest.mark.parametrize("case", TAB["wino"], ids=[str(i) for i in range(len(TAB["wino"]))])
def test_dense_conv3d_wino_f23(dev, case):
    """F(2,3)^3: constants 0, +-1 and +-1/2, U a multiple of 1/8; at Ci = 216 the bf16x3 GEMM, elsewhere the fp32 one."""
    E.wino0_bound(case[4])
    x, w, scale, shift, resid = E.dense3d(case)
    _same(_conv3d(x, w, scale, shift, resid, case[6], 0), R0.conv3d_unit(x, w, scale, shift, resid, case[6]), case, 0.5)


@pytest.mark.parametrize("row", TAB["pointwise"], ids=[str(i) for i in range(len(TAB["pointwise"]))])
def test_dense_pointwise(dev, row):
    B, Ci, Co, Pn, ldw, cl = row
    x, w = E.dense_pointwise(row)
    P = Place(dev, True)
    xd, wd = P.inp(x), P.inp(w)
    y = P.out((B, Pn, Co) if cl else (B, Co, Pn))
    assert _L().decnet_conv3d_pointwise(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), B, Ci, Co, Pn, ldw, cl, _st()) == 0
    P.check("pointwise")
    _same(y.cpu(), R0.pointwise(x, w, ldw, cl), row, 1.0)


@pytest.mark.parametrize("case", TAB["cout1"], ids=[str(i) for i in range(len(TAB["cout1"]))])
@pytest.mark.parametrize("entry", ["one", "ws"])
def test_dense_cout1_reg(dev, case, entry):
    """reg only: pred goes through exp."""
    B, D, H, W, Ci, _ = case
    L = _L()
    x, w, scale, shift = E.dense_cout1(case)
    P = Place(dev, True)
    xd, wd = P.inp(x), P.inp(w)
    reg, pred = P.out((B, D, H, W)), P.out((B, H, W))
    if entry == "one":
        rc = L.decnet_conv3d_cout1_softargmax(xd.data_ptr(), wd.data_ptr(), scale, shift, reg.data_ptr(),
                                              pred.data_ptr(), B, D, H, W, Ci, _st())
    else:
        ws = _lib_buf(L.decnet_conv3d_cout1_workspace_floats(B, D, H, W))
        rc = L.decnet_conv3d_cout1_softargmax_ws(xd.data_ptr(), wd.data_ptr(), scale, shift, reg.data_ptr(),
                                                 pred.data_ptr(), ws.data_ptr(), B, D, H, W, Ci, _st())
    assert rc == 0, rc
    P.check("cout1 %s" % entry)
    _same(reg.cpu(), R0.cout1_softargmax(x, w, scale, shift)[0], (case, entry), 0.5)


@pytest.mark.parametrize("nt", E.GEMM0_NT)
@pytest.mark.parametrize("Ci,Co", E.GEMM0_CICO)
def test_dense_wino_gemm_f23(dev, nt, Ci, Co):
    """decnet_conv3d_wino_gemm alone, variant 0: integer V, integer U^T (read back from the packed weights)."""
    L, np_ = _L(), 64
    kc, kco = (Ci + 15) // 16, (Co + 15) // 16
    V, w = E.dense_gemm0(nt, Ci, Co)
    u = _pack_wino(w, 0)
    Vd = _lib_buf(V.numel())
    Vd.copy_(V.view(np_, kc, 16, nt).permute(0, 1, 3, 2).reshape(-1))
    M = _lib_buf(np_ * kco * nt * 16)
    assert L.decnet_conv3d_wino_gemm(Vd.data_ptr(), u.data_ptr(), M.data_ptr(), nt, Ci, Co, 0, _st()) == 0
    torch.cuda.synchronize()
    U = u[:np_ * kc * 224 * 16].cpu().view(np_, kc, 224, 16).permute(0, 1, 3, 2).reshape(np_, kc * 16, 224)[:, :Ci, :Co]
    assert bool((U == U.round()).all()) and float(U.abs().max()) <= 27 and bool((U != 0).any())
    got = M.cpu().view(np_, kco, nt, 16).permute(0, 1, 3, 2).reshape(np_, kco * 16, nt)[:, :Co]
    _same(got.contiguous(), torch.einsum("xct,xco->xot", V[:, :Ci].double(), U.double()), (nt, Ci, Co), 1.0)


# ------------------------------------------------------------------------------------------------------------------
# term selectors on the bf16x3 kernels
@pytest.mark.parametrize("pairing", E.PAIRINGS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", E.SEL_CONV, ids=[str(i) for i in range(len(E.SEL_CONV))])
def test_select_mfma_conv(dev, case, pairing):
    segs, cout, k, dil, (B, H, W) = case
    ran = []
    for r in range(E.rotations(sum(segs), cout, k * k)):
        xs, w, scale, shift, relu = E.selector_case(case, pairing, r, segs, cout, k * k, lambda c: (B, c, H, W))
        w4 = w.view(cout, -1, k, k)
        _same(_mfma(xs, w4, scale, shift, k, dil, relu), R.conv_bn_act(xs, w4, scale, shift, dil, relu),
              (case, pairing, "rotation", r))
        ran.append(w)
    E.assert_coverage(ran, segs)


@pytest.mark.parametrize("pairing", E.PAIRINGS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", E.SEL_DECONV, ids=[str(i) for i in range(len(E.SEL_DECONV))])
def test_select_mfma_deconv(dev, case, pairing):
    H, W, cin, cout = case
    ran = []
    for r in range(E.rotations(cin, cout, 9)):
        (x,), w, scale, shift, relu = E.selector_case(case, pairing, r, (cin,), cout, 9, lambda c: (2, c, H, W))
        w4 = w.permute(1, 0, 2).reshape(cin, cout, 3, 3).contiguous()
        _same(_mfma_deconv(x, w4, scale, shift, relu), R.deconv_s3_bn_act(x, w4, scale, shift, bool(relu)),
              (case, pairing, "rotation", r))
        ran.append(w)
    E.assert_coverage(ran, (cin,))


@pytest.mark.parametrize("pairing", E.PAIRINGS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", E.SEL_TAP, ids=["%dx%d" % (co, P) for _, co, P in E.SEL_TAP])
def test_select_tap_gemm(dev, case, pairing):
    """decnet_tap_gemm at Ci = 216 with split = 1 (wino_gemm_bf16x3<2, 7>, which the Winograd stack also runs); T itself."""
    Ci, Co, Pn = case
    ran = []
    for r in range(E.rotations(Ci, Co, 9)):
        (x,), w, _, _, _ = E.selector_case(case, pairing, r, (Ci,), Co, 9, lambda c: (1, c, 1, Pn))
        w4 = w.view(Co, Ci, 3, 3)
        ref = torch.stack(R.tap_gemm(x, [w4])).reshape(9, Co, Pn)
        _same(_tap(x, [w4], ((3, 1),), 1).contiguous(), ref, (case, pairing, "rotation", r))
        ran.append(w)
    E.assert_coverage(ran, (Ci,))


# ------------------------------------------------------------------------------------------------------------------
KNOBS = [  # environment switches read once per process; the whole module under each
    {"DECNET_CONV2D_ACC": "2"}, {"DECNET_CONV2D_MFMA_TM": "2"}, {"DECNET_CONV2D_MFMA_PC": "0"},
    {"DECNET_CONV2D_SMALL": "mfma", "DECNET_NT_MB": "0"}, {"DECNET_CONV2D_SMALL": "valu", "DECNET_NT_MB": "0"},
    {"DECNET_WINO_GEMM": "fp32"},
]


@pytest.mark.parametrize("env", KNOBS, ids=["acc2", "tm2", "pc0", "small_mfma", "small_valu", "gemm_fp32"])
def test_knob_leg(env):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "not knob_leg"], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
