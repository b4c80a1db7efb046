"""The backward of the stride-3 conv and transposed-conv units with frozen BatchNorm on the GPU (csrc/conv2d_mfma_grad.hip,
csrc/unfold.hip, decnet_amd/conv2d_grad.Conv2dS3Function / Deconv2dS3Function), against the float64 restatement of
tests/_conv2d_s3_grad_ref.py:
  1. decnet_d2s3_pad1 and decnet_s2d3_pad0 bit for bit against torch indexing, outputs pre-filled with NaN, at both placements
     and under both LDS poison words (tests/_placement._both);
  2. decnet_conv2d_k3s3_wgrad and decnet_deconv2d_k3s3_wgrad through the C ABI on integer data: bit for bit; on random data
     |G - G64| <= 4096 u S with S = sum |gm| |x| per element (u = 2^-24; 4096 terms: the kernel's longest fp32 chain), gsum
     likewise with S = sum |gm|, gm bit-equal;
  3. two calls bit-identical; rejected calls launch nothing;
  4. the Functions under hip_grad() on single Units at their forward routes' floors, with the GPU forward's own y as the
     reference's mask;
  5. the chain f0 -> conv1 = (8 -> 24 stride 3, 24 -> 24, 24 -> 24) -> UpBlock(24, 8)(f0, .): forward bits of the no_grad forward,
     gradients against float64 with the GPU run's masks imposed;
  6. eager twice and a GraphedStep replayed twice: every gradient bit-identical.
-m gpu."""
import copy
import itertools

import pytest
import torch

import _conv2d_grad_ref as GR
import _conv2d_s3_grad_ref as S3
import _model_cases as MC
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _L, _assert_close, _bits_equal, _both, _st

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
BOUND = GR.CHAIN * GR.U32                 # 4096 terms: the chain csrc/conv2d_mfma_grad.hip states
DX_TOL = MC.MFMA_TOL                      # dx runs on the matrix-core forward: its own gate


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- 1. the layout kernels ---------------------------------------------------------------------------------------------------
LAYOUT = [(2, 3, H, W) for H, W in itertools.product((4, 5, 6), (7, 8, 9))] + [(1, 1, 1, 1), (1, 2, 1, 130), (1, 2, 130, 1)]


def _run_d2s3(shape, aligned):
    B, C, H, W = shape
    Ho, Wo = S3.out_hw(False, H, W)
    t = torch.randn(B, 9 * C, Ho, Wo, generator=torch.Generator().manual_seed(H * 131 + W))
    P = Place(torch.device("cuda:0"), aligned)
    td, dx = P.inp(t), P.out((B, C, H, W))
    assert _L().decnet_d2s3_pad1(td.data_ptr(), dx.data_ptr(), B, C, H, W, _st()) == 0
    P.check("d2s3_pad1 %s" % (shape,))
    return {"dx": dx.cpu(), "ref": S3.d2s3_pad1(t, H, W).float()}


def _run_s2d0(shape, aligned):
    B, C, H, W = shape
    g = torch.randn(B, C, 3 * H, 3 * W, generator=torch.Generator().manual_seed(H * 137 + W))
    P = Place(torch.device("cuda:0"), aligned)
    gd, out = P.inp(g), P.out((B, 9 * C, H, W))
    assert _L().decnet_s2d3_pad0(gd.data_ptr(), out.data_ptr(), B, C, H, W, _st()) == 0
    P.check("s2d3_pad0 %s" % (shape,))
    return {"out": out.cpu(), "ref": S3.s2d3_pad0(g).float()}


def _run_round_trip(shape, aligned):
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * 139 + W))
    P = Place(torch.device("cuda:0"), aligned)
    Ho, Wo = S3.out_hw(False, H, W)
    xd, t, back = P.inp(x), P.out((B, 9 * C, Ho, Wo)), P.out((B, C, H, W))
    assert _L().decnet_s2d3_pad1(xd.data_ptr(), t.data_ptr(), B, C, H, W, _st()) == 0
    assert _L().decnet_d2s3_pad1(t.data_ptr(), back.data_ptr(), B, C, H, W, _st()) == 0
    P.check("round trip %s" % (shape,))
    return {"back": back.cpu(), "x": x}


@pytest.mark.parametrize("shape", LAYOUT, ids=lambda s: "x".join(map(str, s)))
def test_layout_kernels_exact(dev, shape):
    r = _both(_run_d2s3, shape)
    assert _bits_equal(r["dx"], r["ref"]), "d2s3_pad1 %s" % (shape,)
    r = _both(_run_s2d0, shape)
    assert _bits_equal(r["out"], r["ref"]), "s2d3_pad0 %s" % (shape,)
    r = _both(_run_round_trip, shape)
    B, C, H, W = shape
    want = r["x"].clone()                   # the last row / column of a multiple of 3 lies in no window: zero
    if H % 3 == 0:
        want[:, :, H - 1] = 0
    if W % 3 == 0:
        want[:, :, :, W - 1] = 0
    assert _bits_equal(r["back"], want), "d2s3_pad1(s2d3_pad1(x)) %s" % (shape,)


# ---- 2. the weight-gradient entries ---------------------------------------------------------------------------------------------
C, T = False, True                        # conv / transposed
CASES = [  # (transposed, Cin, Cout, B, H, W of the layer's input, relu)
    # residues and edges
    (C, 8, 24, 2, 7, 10, 1), (C, 8, 24, 1, 8, 11, 1), (C, 8, 24, 1, 9, 12, 0), (C, 16, 16, 1, 1, 1, 1), (C, 16, 16, 2, 1, 5, 1),
    (C, 16, 16, 1, 2, 2, 1),
    # the coarse plane at 63 | 64 | 65 and 130 pixels (a chunk: 64 consecutive coarse pixels)
    (C, 16, 16, 1, 7, 61, 1), (C, 16, 16, 1, 12, 48, 1), (C, 16, 16, 1, 15, 39, 1), (C, 16, 16, 1, 6, 193, 0),
    (T, 16, 16, 1, 3, 21, 1), (T, 16, 16, 1, 4, 16, 1), (T, 16, 16, 1, 5, 13, 1), (T, 16, 16, 1, 2, 65, 0),
    # slices of 7 | 8 | 9 chunks (8 chunks: the shortest slice)
    (C, 16, 9, 2, 84, 48, 1), (C, 16, 9, 2, 96, 48, 1), (C, 16, 9, 2, 108, 48, 1),
    (T, 9, 16, 2, 28, 16, 1), (T, 9, 16, 2, 32, 16, 1), (T, 9, 16, 2, 36, 16, 1),
    # slices of 16, 32 and 64 chunks (the longest chain: 4096 terms), each with one chunk over: one column block, so 256
    # images keep the launch at its 512 workgroups at that slice (PARTITION below holds plan()'s answer)
    (C, 1, 3, 256, 51, 183, 1), (T, 3, 1, 256, 33, 63, 1), (C, 1, 2, 256, 150, 246, 0),
    # column blocks: 64 GEMM columns up to 9 Cq + 1 = 64, 128 above -- 64 | 73 and 127 | 136 columns on the fine side
    (C, 7, 16, 1, 6, 15, 1), (C, 8, 16, 1, 6, 15, 1), (C, 14, 16, 1, 6, 15, 1), (C, 15, 16, 1, 6, 15, 1),
    (T, 16, 7, 1, 2, 5, 1), (T, 16, 8, 1, 2, 5, 1), (T, 16, 14, 1, 2, 5, 1), (T, 16, 15, 1, 2, 5, 1),
    # the model's pairs
    (C, 8, 24, 1, 5, 7, 1), (C, 24, 72, 1, 5, 7, 1), (C, 72, 216, 1, 5, 7, 1),
    (T, 216, 72, 1, 2, 3, 1), (T, 72, 24, 1, 2, 3, 1), (T, 24, 8, 1, 2, 3, 1), (T, 72, 8, 1, 2, 3, 0),
]
# row tiles: 16 channels on the fine side at a 2 x 5 coarse plane, the coarse side on both sides of the tile counts
# 1 | 2, 3 | 5, 5 | 6, 6 | 9, 9 | 14 the kernel is built for, and at the entry's limit
for _c in (15, 17, 48, 49, 80, 96, 97, 144, 145, 216, 224):
    CASES += [(C, 16, _c, 1, 6, 15, 1), (T, _c, 16, 1, 2, 5, 1)]
IDS = ["%s%dto%d_%dx%dx%d" % (("t" if c[0] else "c",) + c[1:6]) for c in CASES]
# (transposed, B, H, W) of the slice cases -> (sl: chunks of a slice, nsl: slices of one image), as plan() of
# csrc/conv2d_mfma_grad.hip partitions the coarse plane; _ws() holds the library's workspace query against it
PARTITION = {(C, 2, 84, 48): (8, 1), (C, 2, 96, 48): (8, 1), (C, 2, 108, 48): (8, 2),
             (T, 2, 28, 16): (8, 1), (T, 2, 32, 16): (8, 1), (T, 2, 36, 16): (8, 2),
             (C, 256, 51, 183): (16, 2), (T, 256, 33, 63): (32, 2), (C, 256, 150, 246): (64, 2)}


def _shapes(case):
    tr, ci, co, B, H, W, relu = case
    return (B, ci, H, W), (B, co) + S3.out_hw(tr, H, W), (ci, co, 3, 3) if tr else (co, ci, 3, 3)


def _data(case, exact):
    tr, ci, co, B, H, W, relu = case
    xs, gs, _ = _shapes(case)
    g = torch.Generator().manual_seed(ci * 1000 + co * 10 + W + (0 if exact else 1) + (5000 if tr else 0))
    if exact:
        ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=g).float()   # noqa: E731
        x, gy, y = ri(-2, 2, xs), ri(-2, 2, gs), ri(-1, 1, gs)
    else:
        x, gy, y = torch.randn(xs, generator=g), torch.randn(gs, generator=g), torch.randn(gs, generator=g)
    return x, gy, (y if relu else None)


_REFS = {}


def _ref(case, exact):
    """The float64 reference of a case, computed once."""
    key = (case, exact)
    if key not in _REFS:
        x, gy, y = _data(case, exact)
        G, gsum, gm = S3.wgrad(case[0], x, gy, y)
        SG, Ss, _ = S3.wgrad(case[0], x, gy, y, absolute=True)
        _REFS[key] = {"G": G, "gsum": gsum, "gm": gm, "SG": SG, "Ss": Ss}
    return _REFS[key]


def _entry(L, tr):
    return (L.decnet_deconv2d_k3s3_wgrad, L.decnet_deconv2d_k3s3_wgrad_workspace_floats) if tr else \
        (L.decnet_conv2d_k3s3_wgrad, L.decnet_conv2d_k3s3_wgrad_workspace_floats)


def _ws(L, dev, case):
    tr, ci, co, B, H, W, relu = case
    n = _entry(L, tr)[1](B, ci, co, H, W)
    assert n > 0 and n % 4 == 0, n
    if (tr, B, H, W) in PARTITION:          # partial sets [B nsl][Cp][9 Cq + 1] over the coarse plane
        sl, nsl = PARTITION[(tr, B, H, W)]
        hc, wc = (H, W) if tr else S3.out_hw(False, H, W)
        chunks = -(-hc * wc // 64)
        assert nsl == -(-chunks // sl) and (sl == 8 or chunks == sl + 1), (case, chunks)
        cp, cq = (ci, co) if tr else (co, ci)
        want = -(-B * nsl * cp * (9 * cq + 1) // 4) * 4
        if tr:                              # + sum x [Cin], + the float64 partial sums of gsum (65536 pixels of a plane each)
            want += -(-ci // 4) * 4 + -(-2 * co * B * -(-9 * H * W // 65536) // 4) * 4
        assert n == want, (case, n, want)
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n


def _run_wgrad(case, exact, aligned):
    tr, ci, co, B, H, W, relu = case
    L, dev = _L(), torch.device("cuda:0")
    x, gy, y = _data(case, exact)
    P = Place(dev, aligned)
    xd, gyd = P.inp(x), P.inp(gy)
    yd = P.inp(y) if relu else None
    gm = P.out(gy.shape) if relu else None                     # without ReLU: y NULL, gm NULL (gm == gy)
    G, gsum = P.out(_shapes(case)[2]), P.out((co,))
    ws, nws = _ws(L, dev, case)                                # the workspace: 16-byte aligned at either placement
    rc = _entry(L, tr)[0](xd.data_ptr(), gyd.data_ptr(), yd.data_ptr() if relu else None, gm.data_ptr() if relu else None,
                          G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws, B, ci, co, H, W, _st())
    assert rc == 0, rc
    P.check("stride-3 wgrad %s" % (case,))
    out = {"G": G.cpu(), "gsum": gsum.cpu()}
    if relu:
        out["gm"] = gm.cpu()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_exact(dev, case):
    """Integer data: every partial sum is an integer below 2^24, so the results equal float64 bit for bit in any order."""
    ref = _ref(case, True)
    for k in ("G", "gsum", "gm", "SG", "Ss"):
        assert float(ref[k].abs().max()) < 2 ** 24
    r = _both(_run_wgrad, case, True)
    for k in r:
        # (+ 0.0: a float64 sum whose terms are all -0 is +0 on the chip)
        assert _bits_equal(r[k], (ref[k] + 0.0).float()), "%s of %s differs from the float64 reference" % (k, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_float(dev, case):
    r, ref = _both(_run_wgrad, case, False), _ref(case, False)
    eg = (r["G"].double() - ref["G"]).abs()
    es = (r["gsum"].double() - ref["gsum"]).abs()
    print(case, "G: worst error / (4096 u S) = %.3g, gsum: %.3g" % (
        float((eg / (BOUND * ref["SG"]).clamp_min(1e-300)).max()), float((es / (BOUND * ref["Ss"]).clamp_min(1e-300)).max())))
    assert bool((eg <= BOUND * ref["SG"]).all()), case
    assert bool((es <= BOUND * ref["Ss"]).all()), case
    if "gm" in r:
        assert _bits_equal(r["gm"], ref["gm"].float())


# ---- 3. determinism and refusals at the entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(C, 16, 9, 2, 108, 48, 1), (T, 9, 16, 2, 36, 16, 1)], ids=["conv", "transposed"])
def test_two_calls_are_bit_identical(dev, case):
    a, b = _run_wgrad(case, False, True), _run_wgrad(case, False, True)
    for k in a:
        assert _bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("tr", [C, T], ids=["conv", "transposed"])
def test_rejections_launch_nothing(dev, tr):
    case = (tr, 16, 12, 2, 7, 11, 1)
    _, ci, co, B, H, W, relu = case
    L = _L()
    x, gy, y = _data(case, False)
    P = Place(dev, True)
    xd, gyd, yd = P.inp(x), P.inp(gy), P.inp(y)
    gm, G, gsum = P.out(gy.shape), P.out(_shapes(case)[2]), P.out((co,))
    ws, nws = _ws(L, dev, case)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
    entry, query = _entry(L, tr)

    def call(x_=xd.data_ptr(), gy_=gyd.data_ptr(), y_=yd.data_ptr(), gm_=gm.data_ptr(), G_=G.data_ptr(), gs_=gsum.data_ptr(),
             ws_=ws.data_ptr(), n_=nws, B_=B, ci_=ci, co_=co, H_=H, W_=W):
        return entry(x_, gy_, y_, gm_, G_, gs_, ws_, n_, B_, ci_, co_, H_, W_, _st())

    assert call(x_=None) == ERR_NULL and call(gy_=None) == ERR_NULL and call(G_=None) == ERR_NULL
    assert call(gs_=None) == ERR_NULL and call(ws_=None) == ERR_NULL
    assert call(gm_=None) == ERR_NULL                                   # y given, gm missing
    assert call(B_=0) == ERR_SHAPE and call(ci_=0) == ERR_SHAPE and call(co_=0) == ERR_SHAPE
    assert call(H_=0) == ERR_SHAPE and call(W_=-1) == ERR_SHAPE
    assert call(ci_=225) == ERR_UNSUPPORTED and call(co_=225) == ERR_UNSUPPORTED
    assert call(n_=nws - 1) == ERR_SHAPE                                # one float short
    assert call(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED   # an odd float offset
    assert query(B, 225, co, H, W) == 0 and query(B, ci, 225, H, W) == 0 and query(B, ci, co, 0, W) == 0
    P.check_untouched("rejected stride-3 wgrad")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all())
    assert call() == 0                                                  # and the very same arguments, complete, run
    P.check("accepted stride-3 wgrad")


# ---- 4. Function level, at the floors of the forward routes ------------------------------------------------------------------------
UNITS = {  # name: (transposed, Cin, Cout, (H, W), relu, bn, forward route)
    "s3_8to24": (C, 8, 24, (16, 18), True, True, "conv_s3"),
    "s3_8to24_norelu": (C, 8, 24, (16, 18), False, True, "conv_s3"),
    "s3_24to72": (C, 24, 72, (64, 72), True, True, "mfma_s3"),
    "s3_72to216": (C, 72, 216, (64, 72), True, True, "mfma_s3"),
    "dc_216to72": (T, 216, 72, (20, 36), True, True, "mfma_deconv"),
    "dc_72to24": (T, 72, 24, (16, 32), True, True, "mfma_deconv"),
    "dc_24to8": (T, 24, 8, (6, 6), True, True, "deconv"),
    "dc_72to8_bias": (T, 72, 8, (16, 32), True, False, "mfma_deconv"),
}


def _make(name):
    tr, ci, co, hw, relu, bn, route = UNITS[name]
    return MC.make_unit(ci, co, 3, stride=3, relu=relu, bn=bn, transposed=tr, seed=ci + co)


@pytest.mark.parametrize("name", sorted(UNITS))
def test_function_on_units(dev, name):
    import decnet_amd
    from decnet_amd import model
    tr, ci, co, (H, W), relu, bn, route = UNITS[name]
    u = _make(name).to(dev)
    assert u._route(1, H, W) == route and u._grad_route_s3(1, H, W) == ("deconv" if tr else "s3")
    g = torch.Generator().manual_seed(ci * 7 + co)
    x = torch.randn(1, ci, H, W, generator=g).to(dev).requires_grad_()
    gy = torch.randn((1, co) + S3.out_hw(tr, H, W), generator=g).to(dev)
    with torch.no_grad():
        y_plain = u(x)
    model.TALLY = []
    try:
        with decnet_amd.hip_grad():
            y = u(x)
        tally_on = [t["family"] for t in model.TALLY]
        del model.TALLY[:]
        y_lib = u(x)
        tally_off = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
    assert tally_on == ["deconv_grad" if tr else "s3_grad"] and tally_off == ["library"], (tally_on, tally_off)
    assert _bits_equal(y.detach(), y_plain), "the forward under hip_grad() is not the no_grad forward"
    assert MC.close(y_lib.detach(), y.detach().cpu(), MC.FP32_TOL) <= 1.0
    y.backward(gy)
    # the float64 CPU unit, fed the GPU forward's own y as the mask
    xc = x.detach().cpu()
    w = u.conv.weight.detach().cpu().double()
    ymask = y.detach().cpu() if relu else None
    G, gsum, gm = S3.wgrad(tr, xc, gy.cpu(), ymask)
    SG, Ss, _ = S3.wgrad(tr, xc, gy.cpu(), ymask, absolute=True)
    per_co = (0, 2, 3) if tr else (1, 2, 3)
    u64 = _make(name).double()
    if bn:
        scale, shift = GR.bn_fold(u64.bn)
        sd = scale.detach()
        dgamma, dbeta = torch.autograd.grad((scale, shift), (u64.bn.weight, u64.bn.bias), ((w * G).sum(per_co), gsum))
        sigma = torch.sqrt(u64.bn.running_var + u64.bn.eps)
        checks = [("bn.weight", u.bn.weight.grad, dgamma,
                   BOUND * ((w.abs() * SG).sum(per_co) + u64.bn.running_mean.abs() * Ss) / sigma),
                  ("bn.bias", u.bn.bias.grad, dbeta, BOUND * Ss)]
        assert u.bn.running_mean.grad is None and u.bn.running_var.grad is None
    else:
        sd = torch.ones(co, dtype=torch.float64)
        checks = [("conv.bias", u.conv.bias.grad, gsum, BOUND * Ss)]
    sv = sd.view((1, -1, 1, 1) if tr else (-1, 1, 1, 1))
    checks.append(("conv.weight", u.conv.weight.grad, sv * G, BOUND * sv.abs() * SG))
    for what, got, ref, bound in checks:
        err = (got.detach().cpu().double() - ref).abs()
        print(name, what, "worst error / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (name, what)
    _assert_close(x.grad.cpu(), S3.dx(tr, gm, w, sd, H, W), DX_TOL, (name, "x.grad"))


@pytest.mark.parametrize("name", ["s3_24to72", "dc_72to24"])
def test_function_skips_what_nobody_wants(dev, name):
    """No parameter wants a gradient: no wgrad launch; the input does not: no dx convolution and no layout kernel."""
    import decnet_amd
    from spy_util import entry_spy
    tr, ci, co, (H, W), relu, bn, route = UNITS[name]
    u = _make(name).to(dev)
    x = torch.randn(1, ci, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    fwd = ["decnet_deconv2d_mfma_k3s3_bn_act"] if tr else ["decnet_s2d3_pad1", "decnet_conv2d_mfma_cat_bn_act"]
    with entry_spy() as calls:
        with decnet_amd.hip_grad():
            u(x).sum().backward()                                       # parameters only
        assert calls == fwd + ["decnet_deconv2d_k3s3_wgrad" if tr else "decnet_conv2d_k3s3_wgrad"], calls
    with entry_spy() as calls:
        for p in u.parameters():
            p.requires_grad_(False)
        xg = x.clone().requires_grad_()
        with decnet_amd.hip_grad():
            u(xg).sum().backward()                                      # the input only
        assert calls == fwd + (["decnet_s2d3_pad0", "decnet_conv2d_mfma_cat_bn_act"] if tr else
                               ["decnet_conv2d_mfma_cat_bn_act", "decnet_d2s3_pad1"]), calls
    assert xg.grad is not None and u.conv.weight.grad is not None


# ---- 5. The chain ------------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def _chain_forward(conv1, up, f0):
    return up(f0, conv1(f0))[0]


def _gpu_chain(dev):
    import decnet_amd
    from decnet_amd import model
    conv1, up, f0, r = S3.chain_case()
    conv1, up = copy.deepcopy(conv1).to(dev).eval(), copy.deepcopy(up).to(dev).eval()
    x0 = f0.detach().clone().to(dev).requires_grad_()
    masks, hooks = [], []
    for _, u in S3.chain_units(conv1, up):
        hooks.append(u.register_forward_hook(lambda mod, i, o: masks.append((o.detach() > 0).cpu())))
    model.TALLY = []
    try:
        with decnet_amd.hip_grad():
            out = _chain_forward(conv1, up, x0)
        tally = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
        for h in hooks:
            h.remove()
    (out * r.to(dev)).sum().backward()
    with torch.no_grad():
        plain = _chain_forward(conv1, up, x0)
    grads = {"conv1." + n: p.grad.detach().cpu() for n, p in conv1.named_parameters()}
    grads.update({"up." + n: p.grad.detach().cpu() for n, p in up.named_parameters()})
    grads["f0"] = x0.grad.detach().cpu()
    return grads, out.detach(), plain, masks, tally


def chain_runs(dev=None):
    """HIP under hip_grad(), then torch CPU float64 and float32 with the HIP run's masks imposed -- once."""
    if not _CHAIN:
        conv1, up, f0, r = S3.chain_case()
        ghip, out, plain, masks, tally = _gpu_chain(dev or torch.device("cuda:0"))
        g64, _ = S3.chain_grads(conv1, up, f0, r, torch.float64, masks)
        g32, _ = S3.chain_grads(conv1, up, f0, r, torch.float32, masks)
        _CHAIN["runs"] = (g64, g32, ghip, out, plain, tally)
    return _CHAIN["runs"]


def chain_parity():
    """Per tensor: max|g_hip - g64|, max|g32 - g64| and the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|))."""
    g64, g32, ghip = chain_runs()[:3]
    rows = {}
    for k, ref in g64.items():
        e_hip = float((ghip[k].double() - ref).abs().max())
        e_32 = float((g32[k].double() - ref).abs().max())
        gate = max(4.0 * e_32, 2e-5 * max(1.0, float(ref.abs().max())))
        rows[k] = {"hip_vs_f64": e_hip, "f32_vs_f64": e_32, "gate": gate, "hip_over_f32": e_hip / e_32 if e_32 else None}
    return rows


def _expected_tally():
    """What the three route functions give for the chain's shapes."""
    conv1, up, f0, _ = S3.chain_case()
    H, W = S3.CHAIN_HW
    shapes = [(H, W, None), (H // 3, W // 3, None), (H // 3, W // 3, None), (H // 3, W // 3, None), (H, W, 2), (H, W, None)]
    fam = []
    for (_, u), (h, w, parts) in zip(S3.chain_units(conv1, up), shapes):
        route = u._grad_route(1, h, w, parts) or u._grad_route_mfma(1, h, w, parts) or (parts is None and u._grad_route_s3(1, h, w))
        fam.append({"conv": "conv_grad", "mfma": "mfma_grad", "s3": "s3_grad", "deconv": "deconv_grad"}.get(route, "library"))
    return fam


def test_chain_against_float64(dev):
    g64, g32, ghip, out, plain, tally = chain_runs(dev)
    want = _expected_tally()
    assert want[0] == "s3_grad" and want[3] == "deconv_grad" and tally == want, (tally, want)
    assert _bits_equal(out, plain), "the chain under hip_grad() differs from its no_grad forward"
    assert g64.keys() == ghip.keys() == g32.keys()
    rows = chain_parity()
    for k, row in rows.items():
        print(k, "hip %.3g  f32 %.3g  gate %.3g" % (row["hip_vs_f64"], row["f32_vs_f64"], row["gate"]))
    for k, row in rows.items():
        assert ghip[k].shape == g64[k].shape and row["hip_vs_f64"] <= row["gate"], (k, row)


# ---- 6. Determinism and capture --------------------------------------------------------------------------------------
def test_eager_and_graph_replays_are_bit_identical(dev):
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    conv1, up, f0, r = S3.chain_case()
    conv1, up = copy.deepcopy(conv1).to(dev).eval(), copy.deepcopy(up).to(dev).eval()
    x0, r = f0.to(dev).requires_grad_(), r.to(dev)
    leaves = [x0] + list(conv1.parameters()) + list(up.parameters())

    def step():
        with decnet_amd.hip_grad():
            out = _chain_forward(conv1, up, x0)
        (out * r).sum().backward()

    def snapshot():
        torch.cuda.synchronize()
        return [p.grad.detach().clone() for p in leaves]

    runs = []
    for _ in range(2):
        for p in leaves:
            p.grad = None
        step()
        runs.append(snapshot())
    graphed = GraphedStep(step, grads_of=leaves)
    for _ in range(2):
        for p in leaves:
            p.grad.fill_(float("nan"))
        graphed()
        runs.append(snapshot())
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert _bits_equal(a, b)
