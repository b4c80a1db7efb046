"""The backward of the matrix-core stride-1 conv units with frozen BatchNorm on the GPU (csrc/conv2d_mfma_grad.hip,
decnet_amd/conv2d_grad.Conv2dMfmaFunction), against the float64 restatement of tests/_conv2d_grad_ref.py:
  1. decnet_conv2d_mfma_wgrad + the dx convolution (decnet_conv2d_mfma_cat_bn_act on the flipped weights) through the C ABI
     on integer data: bit for bit, at both placements and under both LDS poison words (tests/_placement._both);
  2. the same shapes on random data: |G - G64| <= 4096 u S with S = sum |gm| |x| per element (u = 2^-24: the worst case of
     an fp32 chain of 4096 terms, the kernel's longest, with the product and the final rounding), gsum likewise with
     S = sum |gm|, gm bit-equal, dx within the matrix-core forward's own 4e-6 max(1, max|ref|);
  3. two calls bit-identical; rejected calls launch nothing;
  4. Conv2dMfmaFunction under hip_grad() on single Units at 64 x 64, with the GPU forward's own y as the reference's mask;
  5. the chains DynamicUpsampling(8, 3).weight_learning and UpBlock(72, 24).conv: forward bits of the no_grad forward,
     gradients against the float64 reference with the GPU run's masks imposed (tests/_conv2d_mfma_grad_ref.py);
  6. eager twice and a GraphedStep replayed twice: every gradient bit-identical.
-m gpu."""
import copy

import pytest
import torch

import _conv2d_grad_ref as GR
import _conv2d_mfma_grad_ref as MG
import _model_cases as MC
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _L, _assert_close, _bits_equal, _both, _ints, _ptrs, _st, _vp

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
BOUND = GR.CHAIN * GR.U32
DX_TOL = MC.MFMA_TOL                      # 4e-6: the gate of the matrix-core forward


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


CASES = [  # (segments, Cout, k, dilation, (B, H, W), relu)
    ((16,), 12, 3, 1, (2, 2, 3), 1), ((25,), 25, 3, 1, (1, 3, 17), 1), ((217,), 81, 3, 1, (1, 2, 5), 0),
    ((24,), 217, 1, 1, (2, 3, 1), 1), ((224,), 224, 1, 1, (1, 1, 2), 0), ((81,), 81, 3, 2, (1, 3, 65), 0),
    ((8, 8, 8, 8, 8, 8), 24, 3, 4, (2, 5, 33), 1), ((31, 1, 16), 33, 3, 3, (1, 2, 255), 1),
    ((73,), 81, 3, 1, (1, 2, 257), 1), ((72, 72), 72, 3, 1, (2, 9, 20), 1),
    ((48,), 9, 3, 1, (3, 33, 130), 1),              # many pixel slices, more than 16 partial sets
    ((20,), 16, 3, 6, (2, 3, 5), 1),                # every tap of some rows outside the image
    ((24,), 24, 3, 1, (1, 2, 1025), 1),
    # the kernel's own sizes.  Chunk: 64 consecutive pixels of the plane, rows run on -- H W = 63 | 64 | 65 and 126 | 128 | 130
    ((16,), 16, 3, 1, (1, 3, 21), 1), ((16,), 16, 3, 1, (1, 4, 16), 1), ((16,), 16, 3, 1, (1, 5, 13), 1),
    ((16,), 16, 3, 1, (1, 2, 63), 1), ((16,), 16, 3, 1, (1, 2, 64), 1),       # (2 x 65: the 81 -> 81 case above)
    # slice: 8 chunks at these sizes (the smallest) -- 7 | 8 | 9 chunks of one image, and 8 chunks and one pixel
    ((16,), 9, 3, 1, (2, 28, 16), 1), ((16,), 9, 3, 1, (2, 32, 16), 1), ((16,), 9, 3, 1, (2, 36, 16), 1),
    ((16,), 9, 3, 1, (2, 27, 19), 1),
    # slices of 16, 32 and 64 chunks (the longest chain: 4096 terms), each with one chunk over: 16 column blocks, and
    # enough images that the launch keeps its 512 workgroups at that slice (PARTITION below holds plan()'s answer)
    ((224,), 1, 3, 1, (16, 64, 17), 1), ((224,), 1, 3, 1, (16, 64, 33), 1), ((224,), 1, 3, 1, (32, 64, 65), 0),
    # column block: 64 GEMM columns up to Cin k k + 1 = 64, 128 above -- 63 | 64 | 65 and 127 | 128 | 129 columns
    ((62,), 16, 1, 1, (1, 2, 5), 1), ((63,), 16, 1, 1, (1, 2, 5), 1), ((64,), 16, 1, 1, (1, 2, 5), 1),
    ((14,), 16, 3, 1, (1, 2, 5), 1), ((126,), 16, 1, 1, (1, 2, 5), 1), ((127,), 16, 1, 1, (1, 2, 5), 1),
    ((128,), 16, 1, 1, (1, 2, 5), 1),
    # row tile: 16 channels, and the tile counts 3 | 5 | 6 | 9 | 14 the kernel is built for -- Cout 15 | 17, 48 | 49,
    # 80 (81 above), 96 | 97, 144 | 145 (128 columns below, 64 above)
    ((16,), 15, 3, 1, (1, 2, 5), 1), ((16,), 17, 3, 1, (1, 2, 5), 1), ((16,), 48, 3, 1, (1, 2, 5), 1),
    ((16,), 49, 3, 1, (1, 2, 5), 1), ((16,), 80, 3, 1, (1, 2, 5), 1), ((16,), 96, 3, 1, (1, 2, 5), 1),
    ((16,), 97, 3, 1, (1, 2, 5), 1), ((16,), 144, 3, 1, (1, 2, 5), 1), ((16,), 145, 3, 1, (1, 2, 5), 1),
]
IDS = [str(i) for i in range(len(CASES))]
# (B, H, W) of the slice cases -> (sl: chunks of a slice, nsl: slices of one image), as csrc/conv2d_mfma_grad.hip's plan()
# partitions them; _ws() holds the library's workspace query against it, so that a case cannot go stale silently
PARTITION = {(2, 28, 16): (8, 1), (2, 32, 16): (8, 1), (2, 36, 16): (8, 2), (2, 27, 19): (8, 2),
             (16, 64, 17): (16, 2), (16, 64, 33): (32, 2), (32, 64, 65): (64, 2)}


def _data(case, exact):
    segs, cout, k, dil, (B, H, W), relu = case
    cin = sum(segs)
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + W + (0 if exact else 1))
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()   # noqa: E731
        xs = [ri(-2, 2, B, c, H, W) for c in segs]
        gy, y, w = ri(-2, 2, B, cout, H, W), ri(-1, 1, B, cout, H, W), ri(-1, 1, cout, cin, k, k)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
    else:
        xs = [torch.randn(B, c, H, W, generator=g) for c in segs]
        gy, y = torch.randn(B, cout, H, W, generator=g), torch.randn(B, cout, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        scale = torch.rand(cout, generator=g) + 0.5
    return xs, gy, (y if relu else None), w, scale


_REFS = {}


def _ref(case, exact):
    """The float64 reference of a case, computed once."""
    key = (case, exact)
    if key not in _REFS:
        segs, cout, k, dil, _, relu = case
        xs, gy, y, w, scale = _data(case, exact)
        G, gsum, gm = GR.wgrad(xs, gy, y, k, dil)
        SG, Ss = GR.wgrad_abs(xs, gy, y, k, dil)
        _REFS[key] = {"G": G, "gsum": gsum, "gm": gm, "dx": GR.dx(gm, w, scale, dil), "SG": SG, "Ss": Ss}
    return _REFS[key]


def _ws(L, dev, case):
    segs, cout, k, dil, (B, H, W), relu = case
    n = L.decnet_conv2d_mfma_wgrad_workspace_floats(B, sum(segs), cout, H, W, k)
    assert n > 0 and n % 4 == 0, n
    if (B, H, W) in PARTITION:                                 # partial sets [B nsl][Cout][Cin k k + 1]
        sl, nsl = PARTITION[(B, H, W)]
        chunks = -(-H * W // 64)
        assert nsl == -(-chunks // sl), (case, chunks)
        assert n == -(-B * nsl * cout * (sum(segs) * k * k + 1) // 4) * 4, (case, n)
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n


def _run_backward(case, exact, aligned):
    """decnet_conv2d_mfma_wgrad, then dx = decnet_conv2d_mfma_cat_bn_act([gm], pack(W'), 1, 0, no ReLU) with the roles of the
    channels swapped."""
    segs, cout, k, dil, (B, H, W), relu = case
    L, dev, cin = _L(), torch.device("cuda:0"), sum(segs)
    xs, gy, y, w, scale = _data(case, exact)
    P = Place(dev, aligned)
    xd, gyd = [P.inp(x) for x in xs], P.inp(gy)
    yd = P.inp(y) if relu else None
    gm = P.out((B, cout, H, W)) if relu else None              # without ReLU: y NULL, gm NULL (gm == gy)
    G, gsum = P.out((cout, cin, k, k)), P.out((cout,))
    ws, nws = _ws(L, dev, case)                                # the workspace: 16-byte aligned at either placement
    xa, ca, st = _ptrs(xd), _ints(segs), _st()
    rc = L.decnet_conv2d_mfma_wgrad(_vp(xa), _vp(ca), len(segs), gyd.data_ptr(), yd.data_ptr() if relu else None,
                                    gm.data_ptr() if relu else None, G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws,
                                    B, cout, H, W, k, dil, st)
    assert rc == 0, rc
    wt = P.inp(GR.flipped(w, scale).float())                   # exact data: products of integers and powers of two
    one, zero = P.inp(torch.ones(cin)), P.inp(torch.zeros(cin))
    wp = torch.zeros(L.decnet_conv2d_mfma_packed_bytes(cout, cin, k), dtype=torch.uint8, device=dev)   # library format
    assert L.decnet_conv2d_mfma_pack_weight(wt.data_ptr(), wp.data_ptr(), cout, cin, k, st) == 0
    dx = P.out((B, cin, H, W))
    ga, gc = _ptrs([gm if relu else gyd]), _ints((cout,))
    rc = L.decnet_conv2d_mfma_cat_bn_act(_vp(ga), _vp(gc), 1, wp.data_ptr(), one.data_ptr(), zero.data_ptr(), dx.data_ptr(),
                                         B, cin, H, W, k, dil, 0, st)
    assert rc == 0, rc
    P.check("conv2d mfma backward %s" % (case,))
    out = {"G": G.cpu(), "gsum": gsum.cpu(), "dx": dx.cpu()}
    if relu:
        out["gm"] = gm.cpu()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_and_dx_exact(dev, case):
    """Integer data: every partial sum is an integer below 2^24, so the results equal float64 bit for bit in any order."""
    ref = _ref(case, True)
    for k in ("G", "gsum", "gm", "dx"):
        assert float(ref[k].abs().max()) < 2 ** 24
    r = _both(_run_backward, case, True)
    for k in r:
        # (+ 0.0: a float64 sum whose terms are all -0, e.g. a tap wholly outside under negative gm, is +0 on the chip)
        assert _bits_equal(r[k], (ref[k] + 0.0).float()), "%s of %s differs from the float64 reference" % (k, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_and_dx_float(dev, case):
    r, ref = _both(_run_backward, case, False), _ref(case, False)
    eg = (r["G"].double() - ref["G"]).abs()
    es = (r["gsum"].double() - ref["gsum"]).abs()
    edx = float((r["dx"].double() - ref["dx"]).abs().max()) / (DX_TOL * max(1.0, float(ref["dx"].abs().max())))
    print(case, "G: worst error / (4096 u S) = %.3g, gsum: %.3g, dx: worst error / gate = %.3g" % (
        float((eg / (BOUND * ref["SG"]).clamp_min(1e-300)).max()), float((es / (BOUND * ref["Ss"]).clamp_min(1e-300)).max()),
        edx))
    assert bool((eg <= BOUND * ref["SG"]).all()), case
    assert bool((es <= BOUND * ref["Ss"]).all()), case
    if "gm" in r:
        assert _bits_equal(r["gm"], ref["gm"].float())
    _assert_close(r["dx"], ref["dx"], DX_TOL, case)


def test_two_calls_are_bit_identical(dev):
    case = CASES[CASES.index(((48,), 9, 3, 1, (3, 33, 130), 1))]
    a, b = _run_backward(case, False, True), _run_backward(case, False, True)
    for k in a:
        assert _bits_equal(a[k], b[k]), k


def test_rejections_launch_nothing(dev):
    case = ((16,), 12, 3, 1, (2, 5, 33), 1)
    segs, cout, k, dil, (B, H, W), relu = case
    L, cin = _L(), 16
    xs, gy, y, w, scale = _data(case, False)
    P = Place(dev, True)
    xd, gyd, yd = [P.inp(x) for x in xs], P.inp(gy), P.inp(y)
    gm, G, gsum = P.out((B, cout, H, W)), P.out((cout, cin, k, k)), P.out((cout,))
    ws, nws = _ws(L, dev, case)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
    xa, ca, st = _ptrs(xd), _ints(segs), _st()
    xa7, ca7 = _ptrs(xd * 7), _ints((16,) * 7)
    xa2, ca2 = _ptrs(xd * 2), _ints((16, 209))                            # Cin 225
    null_x = (type(xa))(None)
    query = L.decnet_conv2d_mfma_wgrad_workspace_floats

    def call(xs_=xa, cins_=ca, nseg=1, gy_=gyd.data_ptr(), y_=yd.data_ptr(), gm_=gm.data_ptr(), G_=G.data_ptr(),
             gs_=gsum.data_ptr(), ws_=ws.data_ptr(), n_=nws, Co=cout, k_=k):
        return L.decnet_conv2d_mfma_wgrad(None if xs_ is None else _vp(xs_), None if cins_ is None else _vp(cins_), nseg,
                                          gy_, y_, gm_, G_, gs_, ws_, n_, B, Co, H, W, k_, dil, st)

    assert call(xs_=None) == ERR_NULL and call(cins_=None) == ERR_NULL and call(xs_=null_x) == ERR_NULL
    assert call(gy_=None) == ERR_NULL and call(G_=None) == ERR_NULL and call(gs_=None) == ERR_NULL
    assert call(ws_=None) == ERR_NULL
    assert call(gm_=None) == ERR_NULL                                   # y given, gm missing
    assert call(Co=225) == ERR_UNSUPPORTED and call(k_=2) == ERR_UNSUPPORTED
    assert call(xs_=xa2, cins_=ca2, nseg=2) == ERR_UNSUPPORTED          # Cin 225
    assert call(xs_=xa7, cins_=ca7, nseg=7) == ERR_UNSUPPORTED
    assert call(n_=nws - 1) == ERR_SHAPE                                # one float short
    assert call(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED   # an odd float offset
    assert query(B, 225, cout, H, W, k) == 0 and query(B, cin, 225, H, W, k) == 0 and query(B, cin, cout, H, W, 2) == 0
    P.check_untouched("rejected decnet_conv2d_mfma_wgrad")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all())
    assert call() == 0                                                  # and the very same arguments, complete, run
    P.check("accepted decnet_conv2d_mfma_wgrad")


# ---- 4. Function level at 64 x 64, the floor of the route ---------------------------------------------------------------------
UNITS = {  # name: (segments, Cout, k, dil, relu, bn, parts that require grad)
    "24to24": ((24,), 24, 3, 1, True, True, (0,)),
    "24to10_k1_norelu": ((24,), 10, 1, 1, False, True, (0,)),
    "48to8": ((48,), 8, 3, 1, True, True, (0,)),
    "24to24_six_parts": ((4,) * 6, 24, 3, 1, True, True, (1, 4, 5)),
    "73to81": ((73,), 81, 3, 1, True, True, (0,)),
    "24to24_dil4_bias": ((24,), 24, 3, 4, True, False, (0,)),
}


@pytest.mark.parametrize("name", sorted(UNITS))
def test_function_on_units(dev, name):
    import decnet_amd
    from decnet_amd import model
    segs, cout, k, dil, relu, bn, wanted = UNITS[name]
    cin, (B, H, W) = sum(segs), (1, 64, 64)
    u = MC.make_unit(cin, cout, k, dil=dil, relu=relu, bn=bn, seed=cin + cout).to(dev)
    g = torch.Generator().manual_seed(cin * 7 + cout)
    xs = [torch.randn(B, c, H, W, generator=g).to(dev).requires_grad_(i in wanted) for i, c in enumerate(segs)]
    gy = torch.randn(B, cout, H, W, generator=g).to(dev)
    arg = xs[0] if len(xs) == 1 else tuple(xs)
    with torch.no_grad():
        y_plain = u(arg)
    model.TALLY = []
    try:
        with decnet_amd.hip_grad():
            y = u(arg)
        tally_on = [t["family"] for t in model.TALLY]
        del model.TALLY[:]
        y_lib = u(arg)
        tally_off = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
    assert tally_on == ["mfma_grad"] and tally_off == ["library"], (tally_on, tally_off)
    assert _bits_equal(y.detach(), y_plain), "the forward under hip_grad() is not the no_grad forward"
    y.backward(gy)
    ref_y = MC.close(y.detach(), GR.R.conv_bn_act([t.detach().cpu() for t in xs], u.conv.weight.detach().cpu(),
                                                  *[t.detach().cpu() for t in u._scale_shift()], dil, relu), MC.MFMA_TOL)
    assert ref_y <= 1.0, ref_y
    assert MC.close(y_lib.detach(), y.detach().cpu(), MC.FP32_TOL) <= 1.0
    # the float64 CPU unit, fed the GPU forward's own y as the mask
    cpu = [t.detach().cpu() for t in xs]
    w = u.conv.weight.detach().cpu().double()
    ymask = y.detach().cpu() if relu else None
    G, gsum, gm = GR.wgrad(cpu, gy.cpu(), ymask, k, dil)
    SG, Ss = GR.wgrad_abs(cpu, gy.cpu(), ymask, k, dil)
    u64 = MC.make_unit(cin, cout, k, dil=dil, relu=relu, bn=bn, seed=cin + cout).double()
    if bn:
        scale, shift = GR.bn_fold(u64.bn)
        sd = scale.detach()
        dgamma, dbeta = torch.autograd.grad((scale, shift), (u64.bn.weight, u64.bn.bias), ((w * G).sum((1, 2, 3)), gsum))
        sigma = torch.sqrt(u64.bn.running_var + u64.bn.eps)
        checks = [("bn.weight", u.bn.weight.grad, dgamma,
                   BOUND * ((w.abs() * SG).sum((1, 2, 3)) + u64.bn.running_mean.abs() * Ss) / sigma),
                  ("bn.bias", u.bn.bias.grad, dbeta, BOUND * Ss)]
        assert u.bn.running_mean.grad is None and u.bn.running_var.grad is None
    else:
        sd = torch.ones(cout, dtype=torch.float64)
        checks = [("conv.bias", u.conv.bias.grad, gsum, BOUND * Ss)]
    checks.append(("conv.weight", u.conv.weight.grad, sd.view(-1, 1, 1, 1) * G, BOUND * sd.abs().view(-1, 1, 1, 1) * SG))
    for what, got, ref, bound in checks:
        err = (got.detach().cpu().double() - ref).abs()
        print(name, what, "worst error / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (name, what)
    dxs, c0 = GR.dx(gm, w, sd, dil), 0
    for i, c in enumerate(segs):
        if i in wanted:
            _assert_close(xs[i].grad.cpu(), dxs[:, c0:c0 + c], DX_TOL, (name, "x.grad", i))
        else:
            assert xs[i].grad is None
        c0 += c


def test_function_skips_what_nobody_wants(dev):
    """No parameter wants a gradient: no wgrad launch; no part does: no dx convolution (spied library entries)."""
    import decnet_amd
    from spy_util import entry_spy
    u = MC.make_unit(24, 24, 3, seed=5).to(dev)
    x = torch.randn(1, 24, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    with entry_spy() as calls:
        with decnet_amd.hip_grad():
            u(x).sum().backward()                                       # parameters only
        assert calls == ["decnet_conv2d_mfma_cat_bn_act", "decnet_conv2d_mfma_wgrad"], calls
    with entry_spy(plumbing=True) as calls:
        for p in u.parameters():
            p.requires_grad_(False)
        xg = x.clone().requires_grad_()
        with decnet_amd.hip_grad():
            u(xg).sum().backward()                                      # the input only
        got = [c for c in calls if not c.endswith(("_floats", "_bytes"))]
        assert got == ["decnet_conv2d_mfma_cat_bn_act", "decnet_conv2d_mfma_pack_weight",
                       "decnet_conv2d_mfma_cat_bn_act"], calls
    assert xg.grad is not None and u.conv.weight.grad is not None


# ---- 5. Chains --------------------------------------------------------------------------------------------------------------
_CHAIN_RUNS = {}


def _gpu_chain(seq, parts, r, dev):
    """(chain(parts) * r).sum().backward() under hip_grad() -> ({name: gradient on the CPU}, out, [y_i > 0 per unit])."""
    import decnet_amd
    from decnet_amd import model
    seq = copy.deepcopy(seq).to(dev).eval()
    xs = [t.detach().clone().to(dev).requires_grad_() for t in parts]
    arg = xs[0] if len(xs) == 1 else tuple(xs)
    masks, hooks = [], []
    for u in seq:
        hooks.append(u.register_forward_hook(
            lambda mod, i, o: masks.append((o.detach() > 0).cpu() if mod.relu else None)))
    model.TALLY = []
    try:
        with decnet_amd.hip_grad():
            out = seq(arg)
        tally = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
        for h in hooks:
            h.remove()
    (out * r.to(dev)).sum().backward()
    with torch.no_grad():
        plain = seq(arg)
    grads = {n: p.grad.detach().cpu() for n, p in seq.named_parameters()}
    grads.update({"part%d" % i: t.grad.detach().cpu() for i, t in enumerate(xs)})
    return grads, out.detach(), plain, masks, tally


def chain_runs(name, dev=None):
    """HIP under hip_grad(), then torch CPU float64 and float32 with the HIP run's masks imposed -- once per chain."""
    if name not in _CHAIN_RUNS:
        seq, parts, r = MG.chain_case(name)
        ghip, out, plain, masks, tally = _gpu_chain(seq, parts, r, dev or torch.device("cuda:0"))
        g64, _ = MG.chain_grads(seq, parts, r, torch.float64, masks)
        g32, _ = MG.chain_grads(seq, parts, r, torch.float32, masks)
        _CHAIN_RUNS[name] = (g64, g32, ghip, out, plain, tally)
    return _CHAIN_RUNS[name]


def chain_parity(name):
    """Per tensor: max|g_hip - g64|, max|g32 - g64| and the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|))."""
    g64, g32, ghip = chain_runs(name)[:3]
    rows = {}
    for k, ref in g64.items():
        e_hip = float((ghip[k].double() - ref).abs().max())
        e_32 = float((g32[k].double() - ref).abs().max())
        gate = max(4.0 * e_32, 2e-5 * max(1.0, float(ref.abs().max())))
        rows[k] = {"hip_vs_f64": e_hip, "f32_vs_f64": e_32, "gate": gate, "hip_over_f32": e_hip / e_32 if e_32 else None}
    return rows


@pytest.mark.parametrize("name", ["upblock", "upsampling"])
def test_chains_against_float64(dev, name):
    """The float64 (and float32) reference takes the GPU run's per-layer masks y > 0 as data, in forward and backward
    (tests/_conv2d_mfma_grad_ref.py): with about a million pre-activations per chain some lie closer to zero than the
    forward kernels' error, so a free float64 run takes other ReLU branches than the GPU and no seed keeps every
    pre-activation at a margin -- the margin-seed method of tests/test_conv2d_grad_gpu.py does not scale to these sizes."""
    g64, g32, ghip, out, plain, tally = chain_runs(name, dev)
    assert tally == ["mfma_grad"] * (3 if name == "upsampling" else 2), tally
    assert _bits_equal(out, plain), "%s under hip_grad() differs from its no_grad forward" % name
    assert g64.keys() == ghip.keys() == g32.keys()
    rows = chain_parity(name)
    for k, row in rows.items():
        print(name, k, "hip %.3g  f32 %.3g  gate %.3g" % (row["hip_vs_f64"], row["f32_vs_f64"], row["gate"]))
    for k, row in rows.items():
        assert ghip[k].shape == g64[k].shape and row["hip_vs_f64"] <= row["gate"], (name, k, row)


# ---- 6. Determinism and capture --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["upblock", "upsampling"])
def test_eager_and_graph_replays_are_bit_identical(dev, name):
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    seq, parts, r = MG.chain_case(name)
    seq = copy.deepcopy(seq).to(dev).eval()
    xs = [t.to(dev).requires_grad_() for t in parts]
    arg = xs[0] if len(xs) == 1 else tuple(xs)
    r = r.to(dev)
    leaves = xs + list(seq.parameters())

    def step():
        with decnet_amd.hip_grad():
            out = seq(arg)
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
