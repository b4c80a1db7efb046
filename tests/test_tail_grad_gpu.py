"""The tail gradients on the GPU (csrc/tail_grad.hip, decnet_amd/tail_grad.py) against the float64 restatements of
tests/_tail_grad_ref.py.  Every C-ABI case goes through tests/_placement._both: aligned and unaligned windows, NaN-prefilled
outputs, both LDS poison words, all bit-identical to the unpoisoned aligned run.
  1. decnet_warp_disparity_backward at the forward's edge table, all six kinds of disparity planes: per element
     |got - ref| <= (n + 8) 2^-24 A, n the number of summed terms (4 C for g_disp, the contributor count for g_right), A
     the sum of absolute terms -- the forward bound of an fp32 sum in any order, 8 for the roundings of one term's factors;
     each output alone gives the bits of the joint call;
  2. decnet_dynamic_upsample3_backward at the forward's table, the project's module gate per tensor; rejections launch nothing;
  3. decnet_fold3: the permutation, bit for bit, and the inverse of decnet_unfold3_cat;
  4. decnet_sigmoid_blend: the bits of decnet_conv2d_cat_epilogue's epilogue 1; its backward within the module gate;
  5. the Functions: autograd sees what the entries wrote, launches only what is asked for;
  6. Refinement, SoftAttention.fuse and DynamicUpsampling under hip_grad(): the no_grad forward's bits, gradients within the
     module gate of float64, eager and graph replay bit-identical (right.grad included), TALLY untouched.
-m gpu."""
import copy

import pytest
import torch

import _conv2d_grad_ref as GR
import _model_cases as MC
import _tail_grad_ref as TR
import _trunk_ref as R
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, Place, _L, _bits_equal, _both, _ints, _ptrs, _st, _vp

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
U = TR.U32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


# ---- 1. warp ---------------------------------------------------------------------------------------------------------------
WARP = [(1, 1, 2, 2), (2, 7, 2, 2), (3, 9, 3, 257), (1, 17, 4, 255), (2, 8, 2, 300)]


def _run_warp(right, disp, gout, aligned):
    dev = torch.device("cuda:0")
    B, C, H, W = right.shape
    L, st = _L(), _st()
    P = Place(dev, aligned)
    rd, dd, gd = P.inp(right), P.inp(disp), P.inp(gout)
    g_right, g_disp = P.out((B, C, H, W)), P.out((B, H, W))
    assert L.decnet_warp_disparity_backward(_p(rd), _p(dd), _p(gd), _p(g_right), _p(g_disp), B, C, H, W, st) == 0
    P.check("warp backward")
    Pr, Pd, Ps = Place(dev, aligned), Place(dev, aligned), Place(dev, aligned)    # each output alone; spares stay NaN
    r1, d1 = Pr.out((B, C, H, W)), Pd.out((B, H, W))
    Ps.out((B, C, H, W)), Ps.out((B, H, W))
    assert L.decnet_warp_disparity_backward(_p(rd), _p(dd), _p(gd), _p(r1), None, B, C, H, W, st) == 0
    Pr.check("warp backward, g_right alone")
    Pd.check_untouched("warp backward, g_right alone")
    assert L.decnet_warp_disparity_backward(_p(rd), _p(dd), _p(gd), None, _p(d1), B, C, H, W, st) == 0
    Pd.check("warp backward, g_disp alone")
    Ps.check_untouched("warp backward, one output at a time")
    P.check("warp backward")
    return {"g_right": g_right.cpu(), "g_disp": g_disp.cpu(), "g_right_alone": r1.cpu(), "g_disp_alone": d1.cpu()}


@pytest.mark.parametrize("B,C,H,W", WARP)
def test_warp_backward_edges(dev, B, C, H, W):
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + W)
    right, gout = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    for i, disp in enumerate(R.warp_disparities(B, H, W, g)):
        disp = disp.float()
        r = _both(_run_warp, right, disp, gout)
        ref = TR.warp_backward(right, disp, gout)
        assert _bits_equal(r["g_right"], r["g_right_alone"]) and _bits_equal(r["g_disp"], r["g_disp_alone"]), i
        er = (r["g_right"].double() - ref["g_right"]).abs()
        br = (ref["n_right"] + 8) * U * ref["A_right"]
        ed = (r["g_disp"].double() - ref["g_disp"]).abs()
        bd = (4 * C + 8) * U * ref["A_disp"]
        print((B, C, H, W), "kind", i, "g_right: worst error / bound = %.3g, g_disp: %.3g, contributors <= %d" % (
            float((er / br.clamp_min(1e-300)).max()), float((ed / bd.clamp_min(1e-300)).max()), int(ref["n_right"].max())))
        assert bool((er <= br).all()), ("g_right", (B, C, H, W), i)
        assert bool((ed <= bd).all()), ("g_disp", (B, C, H, W), i)
        if i == 4:                                                        # 1e6: every tap off the image
            assert float(r["g_right"].abs().max()) == 0.0 and float(r["g_disp"].abs().max()) == 0.0


def test_warp_backward_rejections(dev):
    B, C, H, W = 1, 2, 3, 5
    L, st = _L(), _st()
    P = Place(dev, True)
    rd, dd, gd = (P.inp(torch.zeros(s)) for s in ((B, C, H, W), (B, H, W), (B, C, H, W)))
    gr, gdp = P.out((B, C, H, W)), P.out((B, H, W))

    def call(r=rd, d=dd, g=gd, o1=gr, o2=gdp, H_=H, W_=W):
        return L.decnet_warp_disparity_backward(_p(r), _p(d), _p(g), _p(o1), _p(o2), B, C, H_, W_, st)
    assert call(r=None) == ERR_NULL and call(d=None) == ERR_NULL and call(g=None) == ERR_NULL
    assert call(o1=None, o2=None) == ERR_NULL
    assert call(H_=1) == ERR_SHAPE and call(W_=1) == ERR_SHAPE
    assert call(W_=1820) == ERR_UNSUPPORTED                             # g_right: beyond the LDS plan (nothing is read)
    assert call(H_=65536) == ERR_UNSUPPORTED
    P.check_untouched("rejected decnet_warp_disparity_backward")
    assert call() == 0
    P.check("accepted decnet_warp_disparity_backward")


# ---- 2. dynamic upsampling ---------------------------------------------------------------------------------------------------
UPS = [(1, 1, 1, 80.0), (3, 1, 1, 0.0), (3, 2, 255, 80.0), (1, 3, 256, 0.0), (2, 2, 257, 80.0), (3, 4, 5, 3.0)]


def _ups_data(B, h, w, spread):
    g = torch.Generator().manual_seed(B * 1000 + h * 10 + w)
    logits = (torch.rand(B, 81, h, w, generator=g) * 2 - 1) * spread
    return logits, torch.rand(B, h, w, generator=g) * 50 - 10, torch.randn(B, 3 * h, 3 * w, generator=g)


def _run_ups(B, h, w, spread, aligned):
    dev = torch.device("cuda:0")
    L, st = _L(), _st()
    logits, disp, gout = _ups_data(B, h, w, spread)
    P = Place(dev, aligned)
    ld, dd, gd = P.inp(logits), P.inp(disp), P.inp(gout)
    gl, gdp = P.out((B, 81, h, w)), P.out((B, h, w))
    n = L.decnet_dynamic_upsample3_backward_workspace_floats(B, h, w)
    assert n >= 9 * B * h * w and n % 4 == 0, n
    ws = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)        # 16-byte aligned at either placement
    assert L.decnet_dynamic_upsample3_backward(_p(ld), _p(dd), _p(gd), _p(gl), _p(gdp), _p(ws), n, B, h, w, st) == 0
    P.check("upsample backward")
    P1 = Place(dev, aligned)                                            # without g_disp: no workspace either
    gl1 = P1.out((B, 81, h, w))
    assert L.decnet_dynamic_upsample3_backward(_p(ld), _p(dd), _p(gd), _p(gl1), None, None, 0, B, h, w, st) == 0
    P1.check("upsample backward, g_logits alone")
    return {"g_logits": gl.cpu(), "g_disp": gdp.cpu(), "g_logits_alone": gl1.cpu()}


@pytest.mark.parametrize("B,h,w,spread", UPS)
def test_upsample_backward_edges(dev, B, h, w, spread):
    r = _both(_run_ups, B, h, w, spread)
    assert _bits_equal(r["g_logits"], r["g_logits_alone"])
    data = _ups_data(B, h, w, spread)
    g64, g32 = TR.upsample3_backward(*data), TR.upsample3_backward(*data, dtype=torch.float32)
    for k in ("g_logits", "g_disp"):
        e, gate = TR.gate(r[k], g64[k], g32[k])
        print((B, h, w, spread), k, "hip %.3g  gate %.3g" % (e, gate))
        assert r[k].shape == g64[k].shape and e <= gate, (k, e, gate)


def test_upsample_backward_rejections(dev):
    B, h, w = 2, 3, 5
    L, st = _L(), _st()
    logits, disp, gout = _ups_data(B, h, w, 3.0)
    P = Place(dev, True)
    ld, dd, gd = P.inp(logits), P.inp(disp), P.inp(gout)
    gl, gdp = P.out((B, 81, h, w)), P.out((B, h, w))
    n = L.decnet_dynamic_upsample3_backward_workspace_floats(B, h, w)
    big = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=dev)

    def call(l=ld, d=dd, g=gd, o1=gl, o2=gdp, ws=big.data_ptr(), n_=n, h_=h):
        return L.decnet_dynamic_upsample3_backward(_p(l), _p(d), _p(g), _p(o1), _p(o2), ws, n_, B, h_, w, st)
    assert call(l=None) == ERR_NULL and call(d=None) == ERR_NULL and call(g=None) == ERR_NULL and call(o1=None) == ERR_NULL
    assert call(ws=None) == ERR_NULL
    assert call(n_=n - 1) == ERR_SHAPE                                  # one float short
    assert call(ws=big.data_ptr() + 4, n_=n + 4) == ERR_MISALIGNED      # an odd float offset
    assert call(h_=0) == ERR_SHAPE and call(h_=65536) == ERR_UNSUPPORTED
    assert L.decnet_dynamic_upsample3_backward_workspace_floats(B, 65536, w) == 0
    P.check_untouched("rejected decnet_dynamic_upsample3_backward")
    assert bool(torch.isnan(big).all())
    assert call() == 0
    P.check("accepted decnet_dynamic_upsample3_backward")


# ---- 3. fold3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,h,w", [(2, 2, 5, 7), (1, 3, 1, 257), (2, 1, 3, 1)])
def test_fold3_edges(dev, B, C, h, w):
    g = torch.Generator().manual_seed(C * 1000 + h * 10 + w)
    grad = torch.randn(B, 9 * C + 1, h, w, generator=g)
    fea, disp = torch.randn(B, C, 3 * h, 3 * w, generator=g), torch.randn(B, h, w, generator=g)

    def run(aligned):
        L, st = _L(), _st()
        P = Place(dev, aligned)
        gd, fd, dd = P.inp(grad), P.inp(fea), P.inp(disp)
        out, unf, back = P.out((B, C, 3 * h, 3 * w)), P.out((B, 9 * C + 1, h, w)), P.out((B, C, 3 * h, 3 * w))
        assert L.decnet_fold3(_p(gd), _p(out), B, C, h, w, st) == 0
        assert L.decnet_unfold3_cat(_p(fd), _p(dd), _p(unf), B, C, h, w, st) == 0
        assert L.decnet_fold3(_p(unf), _p(back), B, C, h, w, st) == 0
        P.check("fold3")
        return {"y": out.cpu(), "back": back.cpu()}
    r = _both(run)
    assert _bits_equal(r["y"], TR.fold3(grad)) and _bits_equal(r["back"], fea)


def test_fold3_rejections(dev):
    L, st = _L(), _st()
    P = Place(dev, True)
    gd, out = P.inp(torch.zeros(1, 10, 2, 2)), P.out((1, 1, 6, 6))
    assert L.decnet_fold3(None, _p(out), 1, 1, 2, 2, st) == ERR_NULL and L.decnet_fold3(_p(gd), None, 1, 1, 2, 2, st) == ERR_NULL
    assert L.decnet_fold3(_p(gd), _p(out), 1, 1, 0, 2, st) == ERR_SHAPE
    assert L.decnet_fold3(_p(gd), _p(out), 1, 1, 65536, 2, st) == ERR_SHAPE          # as decnet_unfold3_cat
    assert L.decnet_fold3(_p(gd), _p(out), 7, 9362, 2, 2, st) == ERR_SHAPE
    P.check_untouched("rejected decnet_fold3")


# ---- 4. sigmoid + blend ---------------------------------------------------------------------------------------------------------
def _blend_data(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(1, 4, 1, n, generator=g)
    x[0, 0, 0] = torch.rand(n, generator=g) * 60 - 30                   # the layer's centre tap of channel 0 has weight 1
    x[0, 0, 0, ::5] = 100.0
    x[0, 0, 0, 2::7] = -100.0
    w = torch.randn(1, 4, 3, 3, generator=g) * 0.01
    w[0, 0, 1, 1] = 1.0
    return x, w, torch.rand(1, 1, n, generator=g) * 4, torch.rand(1, 1, n, generator=g) * 4, torch.randn(1, 1, n, generator=g)


def _run_blend(n, aligned):
    dev = torch.device("cuda:0")
    L, st = _L(), _st()
    x, w, a, b, gout = _blend_data(n)
    P = Place(dev, aligned)
    xd, wd, ad, bd, gd = P.inp(x), P.inp(w), P.inp(a), P.inp(b), P.inp(gout)
    one, zero = P.inp(torch.ones(1)), P.inp(torch.zeros(1))
    wp = P.out((L.decnet_conv2d_packed_floats(4, 1, 3, 0),))
    assert L.decnet_conv2d_pack_weight(_p(wd), _p(wp), 4, 1, 3, 0, st) == 0
    xa, ca = _ptrs([xd]), _ints((4,))
    fused, o, out = P.out((1, 1, 1, n)), P.out((1, 1, 1, n)), P.out((1, 1, n))
    assert L.decnet_conv2d_cat_epilogue(_vp(xa), _vp(ca), 1, _p(wp), _p(one), _p(zero), _p(fused), 1, 1, n, 3, 1, 0, 1,
                                        _p(ad), _p(bd), st) == 0
    assert L.decnet_conv2d_cat_bn_act(_vp(xa), _vp(ca), 1, _p(wp), _p(one), _p(zero), _p(o), 1, 1, 1, n, 3, 1, 0, st) == 0
    assert L.decnet_sigmoid_blend(_p(o), _p(ad), _p(bd), _p(out), n, st) == 0
    go, ga, gb = P.out((1, 1, n)), P.out((1, 1, n)), P.out((1, 1, n))
    assert L.decnet_sigmoid_blend_backward(_p(o), _p(ad), _p(bd), _p(gd), _p(go), _p(ga), _p(gb), n, st) == 0
    P.check("sigmoid blend")
    Po, Pn = Place(dev, aligned), Place(dev, aligned)                   # g_o alone: g_a, g_b NULL
    go1, spare = Po.out((1, 1, n)), Pn.out((1, 1, n))
    assert L.decnet_sigmoid_blend_backward(_p(o), _p(ad), _p(bd), _p(gd), _p(go1), None, None, n, st) == 0
    Po.check("sigmoid blend backward, g_o alone")
    Pn.check_untouched("sigmoid blend backward, g_o alone")
    return {"fused": fused.cpu().view(1, 1, n), "o": o.cpu().view(1, 1, n), "out": out.cpu(), "g_o": go.cpu(), "g_a": ga.cpu(),
            "g_b": gb.cpu(), "g_o_alone": go1.cpu()}


@pytest.mark.parametrize("n", [1, 3, 255, 1027])
def test_blend_is_the_fused_epilogue_and_its_backward(dev, n):
    r = _both(_run_blend, n)
    _, _, a, b, gout = _blend_data(n)
    assert float(r["o"].max()) > 90 and (n < 3 or float(r["o"].min()) < -90)
    assert _bits_equal(r["out"], r["fused"]), "decnet_sigmoid_blend differs from the fused epilogue"
    assert _bits_equal(r["g_o"], r["g_o_alone"])
    assert not bool(torch.isnan(r["g_o"]).any()) and float(r["g_o"][0, 0, 0].abs()) == 0.0      # o = 100: saturated
    g64, g32 = TR.blend_backward(r["o"], a, b, gout), TR.blend_backward(r["o"], a, b, gout, dtype=torch.float32)
    for k in ("g_o", "g_a", "g_b"):
        e, gate = TR.gate(r[k], g64[k], g32[k])
        print(n, k, "hip %.3g  gate %.3g" % (e, gate))
        assert e <= gate, (k, e, gate)


def test_blend_rejections(dev):
    L, st = _L(), _st()
    P = Place(dev, True)
    o, out = P.inp(torch.zeros(5)), P.out((5,))
    assert L.decnet_sigmoid_blend(None, _p(o), _p(o), _p(out), 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend(_p(o), _p(o), _p(o), None, 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend(_p(o), _p(o), _p(o), _p(out), 0, st) == ERR_SHAPE
    assert L.decnet_sigmoid_blend_backward(_p(o), _p(o), _p(o), _p(o), None, _p(out), None, 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend_backward(_p(o), _p(o), _p(o), None, _p(out), None, None, 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend_backward(_p(o), _p(o), _p(o), _p(o), _p(out), None, None, 0, st) == ERR_SHAPE
    P.check_untouched("rejected decnet_sigmoid_blend")


# ---- 5. Functions -----------------------------------------------------------------------------------------------------------------
def test_warp_by_disparity_takes_the_hip_entry_under_hip_grad(dev):
    """Fails without the feature: autograd on used to send the warp to torch's grid_sample (no entry recorded)."""
    import decnet_amd
    from decnet_amd import model
    from spy_util import entry_spy
    g = torch.Generator().manual_seed(2)
    right, disp = torch.randn(1, 3, 9, 40, generator=g).to(dev), (torch.rand(1, 9, 40, generator=g) * 6).to(dev)
    with entry_spy() as calls:
        with decnet_amd.hip_grad():
            assert torch.is_grad_enabled()
            out = model.warp_by_disparity(right, disp)
        assert calls == ["decnet_warp_disparity"], calls
        del calls[:]
        plain = model.warp_by_disparity(right, disp)                    # hip_grad() off: torch's route, as ever
        assert calls == [], calls
    with torch.no_grad():
        assert _bits_equal(out, model.warp_by_disparity(right, disp))
    assert MC.close(plain, out.cpu(), MC.FP32_TOL) <= 1.0


def test_functions_hand_autograd_what_the_entries_wrote(dev):
    import decnet_amd
    from decnet_amd import ops2d
    g = torch.Generator().manual_seed(4)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)                 # noqa: E731
    right, disp, gout = rn(2, 9, 5, 40).requires_grad_(), (rn(2, 5, 40) * 3).requires_grad_(), rn(2, 9, 5, 40)
    decnet_amd.WarpDisparityFunction.apply(right, disp).backward(gout)
    gr, gd = ops2d.warp_disparity_backward(right.detach(), disp.detach(), gout)
    assert _bits_equal(right.grad, gr) and _bits_equal(disp.grad, gd)
    logits, d2, go2 = rn(2, 81, 4, 5).requires_grad_(), rn(2, 4, 5).requires_grad_(), rn(2, 12, 15)
    decnet_amd.DynamicUpsample3Function.apply(logits, d2).backward(go2)
    gl, gd = ops2d.dynamic_upsample3_backward(logits.detach(), d2.detach(), go2)
    assert _bits_equal(logits.grad, gl) and _bits_equal(d2.grad, gd)
    fea, d3, go3 = rn(2, 2, 12, 15).requires_grad_(), rn(2, 4, 5).requires_grad_(), rn(2, 19, 4, 5)
    decnet_amd.Unfold3CatFunction.apply(fea, d3).backward(go3)
    assert _bits_equal(fea.grad, TR.fold3(go3)) and _bits_equal(d3.grad, go3[:, 0])
    o, a, b, go4 = rn(3, 7, 9).requires_grad_(), rn(3, 7, 9).requires_grad_(), rn(3, 7, 9).requires_grad_(), rn(3, 7, 9)
    decnet_amd.SigmoidBlendFunction.apply(o, a, b).backward(go4)
    want = ops2d.sigmoid_blend_backward(o.detach(), a.detach(), b.detach(), go4)
    assert all(_bits_equal(t.grad, w) for t, w in zip((o, a, b), want))


def test_functions_launch_only_what_is_asked_for(dev):
    import decnet_amd
    from spy_util import entry_spy
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)                 # noqa: E731
    seen = {}

    def spied(name):                                                    # the g_right / g_disp pointers of every backward call
        from decnet_amd import _lib
        real = getattr(_lib.lib(), name)

        def call(*a):
            seen.setdefault(name, []).append((a[3], a[4]))
            return real(*a)
        return call
    right, disp = rn(1, 3, 9, 40), rn(1, 9, 40).requires_grad_()
    with entry_spy() as calls:
        out = decnet_amd.WarpDisparityFunction.apply(right, disp)       # `right` frozen
        del calls[:]
        out.sum().backward()
        assert calls == ["decnet_warp_disparity_backward"], calls
        assert right.grad is None and disp.grad is not None
        del calls[:]
        with torch.enable_grad():                                       # nothing requires grad: no backward launches
            for fn, args in ((decnet_amd.WarpDisparityFunction, (right, disp.detach())),
                             (decnet_amd.DynamicUpsample3Function, (rn(1, 81, 3, 4), rn(1, 3, 4))),
                             (decnet_amd.Unfold3CatFunction, (rn(1, 2, 9, 12), rn(1, 3, 4))),
                             (decnet_amd.SigmoidBlendFunction, (rn(7), rn(7), rn(7)))):
                leaf = torch.zeros((), device=dev, requires_grad=True)
                (fn.apply(*args).sum() * 0 + leaf).backward()
        assert [c for c in calls if c.endswith("_backward") or c == "decnet_fold3"] == [], calls
        del calls[:]
        o, a, b = rn(7).requires_grad_(), rn(7), rn(7).requires_grad_()
        decnet_amd.SigmoidBlendFunction.apply(o, a, b).sum().backward()
        assert calls == ["decnet_sigmoid_blend", "decnet_sigmoid_blend_backward"] and a.grad is None and b.grad is not None
    # the frozen `right`: the entry is handed a NULL g_right (no scan is launched for it)
    from decnet_amd import _lib, ops
    real, saved = _lib.lib(), dict(ops._FN)
    ops._FN.clear()
    ops._FN["decnet_warp_disparity_backward"] = spied("decnet_warp_disparity_backward")
    try:
        d = disp.detach().clone().requires_grad_()
        decnet_amd.WarpDisparityFunction.apply(right, d).sum().backward()
    finally:
        ops._FN.clear()
        ops._FN.update(saved)
    assert real is _lib.lib() and len(seen["decnet_warp_disparity_backward"]) == 1
    g_right_ptr, g_disp_ptr = seen["decnet_warp_disparity_backward"][0]
    assert g_right_ptr is None and g_disp_ptr


# ---- 6. modules ---------------------------------------------------------------------------------------------------------------------
WRT = {"refinement": ("disp", "right", "left"), "attention": ("dense", "sparse")}
_RUNS = {}


def _upsampling_case():
    from decnet_amd.model import DynamicUpsampling
    g = torch.Generator().manual_seed(77)
    m = MC.seeded(lambda: DynamicUpsampling(2, 3), 301)
    ins = {"disp": torch.rand(1, 5, 7, generator=g) * 20, "fea": torch.randn(1, 2, 15, 21, generator=g)}
    return m, ins, ("disp", "fea"), torch.randn(1, 15, 21, generator=g)


def _case(name):
    if name == "upsampling":
        return _upsampling_case()
    m, ins, _, r = GR.module_case(name)
    return m, ins, WRT[name], r


def _out(name, m, t):
    return m(t["disp"], t["fea"]) if name == "upsampling" else GR.module_out(name, m, t)


def _grads(name, m, ins, wrt, r, dtype, device="cpu", hip=False):
    import contextlib
    import decnet_amd
    m = copy.deepcopy(m).to(device=device, dtype=dtype).eval()
    t = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(k in wrt) for k, v in ins.items()}
    with (decnet_amd.hip_grad() if hip else contextlib.nullcontext()):
        out = _out(name, m, t)
    (out * r.to(device=device, dtype=dtype)).sum().backward()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    grads.update({k: t[k].grad.detach().cpu() for k in wrt})
    return grads, out.detach(), m, t


def _runs(name):
    """float64 CPU, float32 CPU, HIP under hip_grad() (with the TALLY it left), the no_grad forward -- once per module."""
    from decnet_amd import model
    if name not in _RUNS:
        m, ins, wrt, r = _case(name)
        g64 = _grads(name, m, ins, wrt, r, torch.float64)[0]
        g32 = _grads(name, m, ins, wrt, r, torch.float32)[0]
        model.TALLY = []
        try:
            ghip, out, mh, th = _grads(name, m, ins, wrt, r, torch.float32, "cuda:0", hip=True)
            tally = [e["family"] for e in model.TALLY]
        finally:
            model.TALLY = None
        with torch.no_grad():
            plain = _out(name, mh, th)
        _RUNS[name] = (g64, g32, ghip, tally, out, plain)
    return _RUNS[name]


@pytest.mark.parametrize("name", ["attention", "refinement"])
def test_module_forward_is_the_inference_forward(dev, name):
    _, _, _, tally, out, plain = _runs(name)
    assert _bits_equal(out, plain), "%s under hip_grad() differs from its no_grad forward" % name
    assert tally == ["conv_grad"] * (7 if name == "refinement" else 3), tally


@pytest.mark.parametrize("name", ["attention", "refinement", "upsampling"])
def test_module_gradients_against_float64(dev, name):
    g64, g32, ghip, _, _, _ = _runs(name)
    assert g64.keys() == ghip.keys() == g32.keys()
    rows = {k: TR.gate(ghip[k], g64[k], g32[k]) for k in g64}
    for k, (e, gate) in rows.items():
        print(name, k, "hip %.3g  gate %.3g" % (e, gate))
    for k, (e, gate) in rows.items():
        assert ghip[k].shape == g64[k].shape and e <= gate, (name, k, e, gate)


def test_module_entries(dev):
    """The tail of each module under hip_grad() is the inference entries plus ours: no torch route in between."""
    import decnet_amd
    from spy_util import entry_spy
    for name, want in (("refinement", ["decnet_warp_disparity", "decnet_warp_disparity_backward"]),
                       ("attention", ["decnet_sigmoid_blend", "decnet_sigmoid_blend_backward"]),
                       ("upsampling", ["decnet_unfold3_cat", "decnet_dynamic_upsample3", "decnet_dynamic_upsample3_backward",
                                       "decnet_fold3"])):
        m, ins, wrt, r = _case(name)
        with entry_spy() as calls:
            _grads(name, m, ins, wrt, r, torch.float32, "cuda:0", hip=True)
        assert [c for c in calls if "conv2d" not in c and "bias_act" not in c] == want, (name, calls)


@pytest.mark.parametrize("name", ["attention", "refinement", "upsampling"])
def test_eager_and_graph_replays_are_bit_identical(dev, name):
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    m, ins, wrt, r = _case(name)
    m = copy.deepcopy(m).to(dev)
    t = {k: v.to(dev).requires_grad_(k in wrt) for k, v in ins.items()}
    r = r.to(dev)
    leaves = [t[k] for k in wrt] + list(m.parameters())

    def step():
        with decnet_amd.hip_grad():
            out = _out(name, m, t)
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
