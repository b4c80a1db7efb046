"""The backward of the few-channel stride-1 conv units with frozen BatchNorm on the GPU (csrc/conv2d_grad.hip,
decnet_amd/conv2d_grad.py), against the float64 restatement of tests/_conv2d_grad_ref.py:
  1. decnet_conv2d_wgrad + the dx convolution through the C ABI on integer data: bit for bit, at both placements and under
     both LDS poison words (tests/_placement._both);
  2. the same shapes on random data: |G - G64| <= 4096 u S with S = sum |gm| |x| per element (u = 2^-24, the unit roundoff:
     the worst case of an fp32 chain of 4096 terms -- the kernel's are 512 -- with the product and the final rounding),
     gsum likewise with S = sum |gm|, dx within the small kernels' 2e-5 max(1, max|ref|);
  3. rejected calls launch nothing;
  4. Conv2dSmallFunction under hip_grad() on single Units, with the GPU forward's own y as the reference's mask;
  5. Refinement and SoftAttention.fuse against the float64 CPU module, gated by the float32 CPU module's own distance;
  6. eager twice and a GraphedStep replayed twice: every gradient bit-identical.
-m gpu."""
import pytest
import torch

import _conv2d_grad_ref as GR
import _model_cases as MC
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _L, _assert_close, _bits_equal, _both, _ints, _ptrs, _st, _vp

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
BOUND = GR.CHAIN * GR.U32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


CASES = [  # (segments, Cout, k, dilation, (B, H, W), relu)
    ((8,), 8, 3, 1, (2, 1, 1), 1), ((8,), 8, 3, 1, (2, 2, 3), 1), ((5,), 4, 3, 1, (1, 3, 2), 0),
    ((3,), 3, 3, 2, (1, 2, 5), 1), ((8,), 8, 1, 1, (2, 3, 1), 1), ((8,), 8, 3, 1, (1, 3, 255), 1),
    ((4,), 24, 3, 2, (1, 2, 256), 1), ((16,), 8, 3, 1, (2, 3, 257), 1), ((8, 4), 12, 3, 1, (1, 2, 1025), 1),
    ((3,), 1, 3, 1, (2, 3, 257), 0), ((8,), 4, 3, 6, (2, 3, 5), 1), ((4,), 8, 3, 9, (2, 2, 7), 0),
    ((12,), 24, 3, 4, (2, 3, 4), 1), ((1, 1, 1, 1, 1, 1), 13, 3, 1, (2, 5, 33), 1), ((8, 8, 1), 8, 3, 3, (2, 5, 257), 1),
    ((24,), 9, 3, 1, (2, 5, 64), 1),
]
IDS = [str(i) for i in range(len(CASES))]


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
    n = L.decnet_conv2d_wgrad_workspace_floats(B, sum(segs), cout, H, W, k)
    assert n > 0 and n % 4 == 0, n
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n


def _run_backward(case, exact, aligned):
    """decnet_conv2d_wgrad, then dx = decnet_conv2d_bn_act(gm, pack(W'), 1, 0, no ReLU) with the roles of the channels swapped."""
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
    rc = L.decnet_conv2d_wgrad(_vp(xa), _vp(ca), len(segs), gyd.data_ptr(), yd.data_ptr() if relu else None,
                               gm.data_ptr() if relu else None, G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws,
                               B, cout, H, W, k, dil, st)
    assert rc == 0, rc
    wt = P.inp(GR.flipped(w, scale).float())                   # exact data: products of integers and powers of two
    one, zero = P.inp(torch.ones(cin)), P.inp(torch.zeros(cin))
    wp = P.out((L.decnet_conv2d_packed_floats(cout, cin, k, 0),))
    assert L.decnet_conv2d_pack_weight(wt.data_ptr(), wp.data_ptr(), cout, cin, k, 0, st) == 0
    dx = P.out((B, cin, H, W))
    rc = L.decnet_conv2d_bn_act((gm if relu else gyd).data_ptr(), wp.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                dx.data_ptr(), B, cout, cin, H, W, k, dil, 0, st)
    assert rc == 0, rc
    P.check("conv2d backward %s" % (case,))
    out = {"G": G.cpu(), "gsum": gsum.cpu(), "dx": dx.cpu()}
    if relu:
        out["gm"] = gm.cpu()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_and_dx_exact(dev, case):
    """Integer data: every partial sum is an integer below 2^24, so the results equal float64 bit for bit in any order."""
    r, ref = _both(_run_backward, case, True), _ref(case, True)
    for k in r:
        assert float(ref[k].abs().max()) < 2 ** 24
        # (+ 0.0: a float64 sum whose terms are all -0, e.g. a tap wholly outside under negative gm, is +0 on the chip)
        assert _bits_equal(r[k], (ref[k] + 0.0).float()), "%s of %s differs from the float64 reference" % (k, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_and_dx_float(dev, case):
    r, ref = _both(_run_backward, case, False), _ref(case, False)
    eg = (r["G"].double() - ref["G"]).abs()
    es = (r["gsum"].double() - ref["gsum"]).abs()
    print(case, "G: worst error / (4096 u S) = %.3g, gsum: %.3g" % (
        float((eg / (BOUND * ref["SG"]).clamp_min(1e-300)).max()), float((es / (BOUND * ref["Ss"]).clamp_min(1e-300)).max())))
    assert bool((eg <= BOUND * ref["SG"]).all()), case
    assert bool((es <= BOUND * ref["Ss"]).all()), case
    if "gm" in r:
        assert _bits_equal(r["gm"], ref["gm"].float())
    _assert_close(r["dx"], ref["dx"], 2e-5, case)


def test_two_calls_are_bit_identical(dev):
    case = CASES[14]
    a, b = _run_backward(case, False, True), _run_backward(case, False, True)
    for k in a:
        assert _bits_equal(a[k], b[k]), k


def test_rejections_launch_nothing(dev):
    case = ((8,), 8, 3, 1, (2, 5, 33), 1)
    segs, cout, k, dil, (B, H, W), relu = case
    L, cin = _L(), 8
    xs, gy, y, w, scale = _data(case, False)
    P = Place(dev, True)
    xd, gyd, yd = [P.inp(x) for x in xs], P.inp(gy), P.inp(y)
    gm, G, gsum = P.out((B, cout, H, W)), P.out((cout, cin, k, k)), P.out((cout,))
    ws, nws = _ws(L, dev, case)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
    xa, ca, st = _ptrs(xd), _ints(segs), _st()
    xa7, ca7 = _ptrs(xd * 7), _ints((8,) * 7)
    null_x = (type(xa))(None)

    def call(xs_=xa, cins_=ca, nseg=1, gy_=gyd.data_ptr(), y_=yd.data_ptr(), gm_=gm.data_ptr(), G_=G.data_ptr(),
             gs_=gsum.data_ptr(), ws_=ws.data_ptr(), n_=nws, Co=cout, k_=k):
        return L.decnet_conv2d_wgrad(None if xs_ is None else _vp(xs_), None if cins_ is None else _vp(cins_), nseg, gy_,
                                     y_, gm_, G_, gs_, ws_, n_, B, Co, H, W, k_, dil, st)

    assert call(xs_=None) == ERR_NULL and call(cins_=None) == ERR_NULL and call(xs_=null_x) == ERR_NULL
    assert call(gy_=None) == ERR_NULL and call(G_=None) == ERR_NULL and call(gs_=None) == ERR_NULL
    assert call(ws_=None) == ERR_NULL
    assert call(gm_=None) == ERR_NULL                                   # y given, gm missing
    assert call(Co=25) == ERR_UNSUPPORTED and call(k_=2) == ERR_UNSUPPORTED
    assert call(xs_=xa7, cins_=ca7, nseg=7) == ERR_UNSUPPORTED
    assert call(n_=nws - 1) == ERR_SHAPE                                # one float short
    assert call(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED   # an odd float offset
    assert L.decnet_conv2d_wgrad_workspace_floats(B, 25, cout, H, W, k) == 0
    assert L.decnet_conv2d_wgrad_workspace_floats(B, cin, 25, H, W, k) == 0
    assert L.decnet_conv2d_wgrad_workspace_floats(B, cin, cout, H, W, 2) == 0
    P.check_untouched("rejected decnet_conv2d_wgrad")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all())
    assert call() == 0                                                  # and the very same arguments, complete, run
    P.check("accepted decnet_conv2d_wgrad")


# ---- 4. Function level ----------------------------------------------------------------------------------------------
UNITS = {  # name: (segments, Cout, k, dil, relu, bn, parts that require grad)
    "8to8": ((8,), 8, 3, 1, True, True, (0,)),
    "12to8_four_parts": ((3, 3, 3, 3), 8, 3, 1, True, True, (0, 1, 2, 3)),
    "17to8_dil3_last_part": ((8, 8, 1), 8, 3, 3, True, True, (2,)),
    "4to1_bias_norelu": ((4,), 1, 3, 1, False, False, (0,)),
}


@pytest.mark.parametrize("name", sorted(UNITS))
def test_function_on_units(dev, name):
    import decnet_amd
    from decnet_amd import model
    segs, cout, k, dil, relu, bn, wanted = UNITS[name]
    cin, (B, H, W) = sum(segs), (2, 17, 19)
    u = MC.make_unit(cin, cout, k, dil=dil, relu=relu, bn=bn, seed=cin + cout).to(dev)
    g = torch.Generator().manual_seed(cin * 7 + cout)
    xs = [torch.randn(B, c, H, W, generator=g).to(dev).requires_grad_(i in wanted) for i, c in enumerate(segs)]
    gy = torch.randn(B, cout, H, W, generator=g).to(dev)
    arg = xs[0] if len(xs) == 1 else tuple(xs)
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
    assert tally_on == ["conv_grad"] and tally_off == ["library"]
    y.backward(gy)
    ref_y = MC.close(y.detach(), GR.R.conv_bn_act([t.detach().cpu() for t in xs], u.conv.weight.detach().cpu(),
                                                  *[t.detach().cpu() for t in u._scale_shift()], dil, relu), MC.FP32_TOL)
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
            _assert_close(xs[i].grad.cpu(), dxs[:, c0:c0 + c], 2e-5, (name, "x.grad", i))
        else:
            assert xs[i].grad is None
        c0 += c


def test_function_skips_what_nobody_wants(dev):
    """No parameter wants a gradient: no wgrad launch; no part does: no dx convolution (spied library entries)."""
    import decnet_amd
    from spy_util import entry_spy
    u = MC.make_unit(8, 8, 3, seed=5).to(dev)
    x = torch.randn(1, 8, 16, 18, generator=torch.Generator().manual_seed(1)).to(dev)
    with entry_spy() as calls:
        with decnet_amd.hip_grad():
            u(x).sum().backward()                                       # parameters only
        assert calls == ["decnet_conv2d_bn_act", "decnet_conv2d_wgrad"], calls
        del calls[:]
        for p in u.parameters():
            p.requires_grad_(False)
        xg = x.clone().requires_grad_()
        with decnet_amd.hip_grad():
            u(xg).sum().backward()                                      # the input only
        assert calls == ["decnet_conv2d_bn_act", "decnet_conv2d_bn_act"], calls
    assert xg.grad is not None and u.conv.weight.grad is not None


# ---- 5. Module level ------------------------------------------------------------------------------------------------
_MODULE_RUNS = {}


def module_runs(name):
    """HIP under hip_grad(), torch CPU float64, torch CPU float32 -- computed once per module."""
    import decnet_amd
    from decnet_amd import model
    if name not in _MODULE_RUNS:
        m, ins, wrt, r = GR.module_case(name)
        margins = []
        g64, _, _ = GR.module_grads(name, m, ins, wrt, r, torch.float64, margins=margins)
        g32, _, _ = GR.module_grads(name, m, ins, wrt, r, torch.float32)
        model.TALLY = []
        try:
            ghip, _, _ = GR.module_grads(name, m, ins, wrt, r, torch.float32, "cuda:0", ctx=decnet_amd.hip_grad)
            tally = [t["family"] for t in model.TALLY]
        finally:
            model.TALLY = None
        _MODULE_RUNS[name] = (g64, g32, ghip, margins, tally)
    return _MODULE_RUNS[name]


def parity_ratios(name):
    """Per tensor: max|g_hip - g64|, max|g32 - g64| and the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|))."""
    g64, g32, ghip, _, _ = module_runs(name)
    rows = {}
    for k, ref in g64.items():
        e_hip = float((ghip[k].double() - ref).abs().max())
        e_32 = float((g32[k].double() - ref).abs().max())
        gate = max(4.0 * e_32, 2e-5 * max(1.0, float(ref.abs().max())))
        rows[k] = {"hip_vs_f64": e_hip, "f32_vs_f64": e_32, "gate": gate, "hip_over_f32": e_hip / e_32 if e_32 else None}
    return rows


@pytest.mark.parametrize("name", sorted(GR.MODULE_SEEDS))
def test_modules_against_float64(dev, name):
    g64, g32, ghip, margins, tally = module_runs(name)
    assert GR.margins_hold(margins), margins                            # all three runs take the same ReLU branches
    assert tally == ["conv_grad"] * (7 if name == "refinement" else 3), tally
    assert g64.keys() == ghip.keys() == g32.keys()
    rows = parity_ratios(name)
    for k, row in rows.items():
        print(name, k, "hip %.3g  f32 %.3g  gate %.3g" % (row["hip_vs_f64"], row["f32_vs_f64"], row["gate"]))
    for k, row in rows.items():
        assert ghip[k].shape == g64[k].shape and row["hip_vs_f64"] <= row["gate"], (name, k, row)


def test_all_ten_units_take_the_function(dev):
    assert sum(len(module_runs(n)[4]) for n in GR.MODULE_SEEDS) == 10
    assert all(f == "conv_grad" for n in GR.MODULE_SEEDS for f in module_runs(n)[4])


# ---- 6. Determinism and capture --------------------------------------------------------------------------------------
def test_eager_and_graph_replays_are_bit_identical(dev):
    import copy
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    m, ins, wrt, r = GR.module_case("refinement")
    m = copy.deepcopy(m).to(dev)
    t = {k: v.to(dev) for k, v in ins.items()}
    t["disp"].requires_grad_()
    r = r.to(dev)
    leaves = [t["disp"]] + list(m.parameters())

    def step():
        with decnet_amd.hip_grad():
            out = m(t["left"], t["right"], t["disp"])[0]
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
