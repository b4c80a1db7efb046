"""Detail maps and soft masks under hip_grad() on the GPU (csrc/detail_grad.hip, decnet_amd/tail_grad.py,
GenerateSparseMask.detail, SoftAttention.fuse(want_soft=True)).  Every C-ABI case goes through tests/_placement._both: aligned
and unaligned windows, NaN-prefilled outputs, guard bands, both LDS poison words, all bit-identical.
  1. the flat entries at n = 1, 3, 4, 5, 1023, 1025: decnet_sqdiff and its backward give torch's bits on the device;
     decnet_sigmoid_blend_soft gives decnet_sigmoid_blend's; its backward without gsoft decnet_sigmoid_blend_backward's; with
     both gradients |g_o - ref64| <= 8 * 2^-24 (|gout (b - a)| + |gsoft|) (the sigmoid to 4 * 2^-24 relative, which s (1 - s)
     <= 1/4 inherits absolutely, and four roundings);
  2. decnet_detail_tail: |prob - sigmoid64(z)| <= 4 * 2^-24 sigmoid64(z) (expf to one ulp, the sum, the quotient), the mask
     from the kernel's own prob exactly, the bit plane, every subset of outputs, the logits of decnet_detail_mask; its
     backward within 8 * 2^-24 |g|;
  3. the Functions: the entries' bits, only the launches that are needed, twice in a row;
  4. detail(): routes, values and gradients at tests/_detail_ref.py's cases, eval and train mode;
  5. fuse(want_soft=True): the bits of fuse(), soft and the gradients against float64;
  6. one GraphedStep over both: the eager bits, no host synchronisation.
-m gpu."""
import itertools

import pytest
import torch

import _bn_train_ref as BR
import _detail_ref as DR
import _model_cases as MC
from _placement import Place, _L, _bits_equal, _both, _st

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
U = 2.0 ** -24
D = torch.float64
FLAT_N = [1, 3, 4, 5, 1023, 1025]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


def _sigmoid_ok(got, z):
    """|got - sigmoid64(z)| <= 4 * 2^-24 sigmoid64(z): expf to one ulp, the sum, the quotient.  The bound counts roundings,
    so it speaks of results float32 can hold: where sigmoid64(z) is below the smallest normal float32 (z < -87.3; the planted
    -200 is 1.4e-87) the kernel must give exactly 0.  -> (all within, worst error / bound over the representable ones)."""
    s64 = torch.sigmoid(z.double())
    err, tiny = (got.double() - s64).abs(), s64 < 2.0 ** -126
    ok = torch.where(tiny, got == 0, err <= 4 * U * s64)
    return bool(ok.all()), float((err / (4 * U * s64))[~tiny].max()) if bool((~tiny).any()) else 0.0


def _hip():
    import decnet_amd
    return decnet_amd.hip_grad()


# ---- 1. the flat entries ---------------------------------------------------------------------------------------------------------
def _sq_data(n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)


def _run_sqdiff(n, aligned):
    dev = torch.device("cuda:0")
    L, st = _L(), _st()
    a, b, gout = _sq_data(n)
    P = Place(dev, aligned)
    ad, bd, gd = P.inp(a), P.inp(b), P.inp(gout)
    out, ga, gb = P.out((n,)), P.out((n,)), P.out((n,))
    assert L.decnet_sqdiff(_p(ad), _p(bd), _p(out), n, st) == 0
    assert L.decnet_sqdiff_backward(_p(ad), _p(bd), _p(gd), _p(ga), _p(gb), n, st) == 0
    P.check("sqdiff")
    Pa, Pb, Ps = Place(dev, aligned), Place(dev, aligned), Place(dev, aligned)      # each gradient alone; the spare stays NaN
    ga1, gb1, spare = Pa.out((n,)), Pb.out((n,)), Ps.out((n,))
    assert L.decnet_sqdiff_backward(_p(ad), _p(bd), _p(gd), _p(ga1), None, n, st) == 0
    Pa.check("sqdiff backward, g_a alone")
    Pb.check_untouched("sqdiff backward, g_a alone")
    assert L.decnet_sqdiff_backward(_p(ad), _p(bd), _p(gd), None, _p(gb1), n, st) == 0
    Pb.check("sqdiff backward, g_b alone")
    Ps.check_untouched("sqdiff backward, one gradient at a time")
    ta, tb = ad.clone().requires_grad_(), bd.clone().requires_grad_()              # torch on the same device
    y = (ta - tb) * (ta - tb)
    tga, tgb = torch.autograd.grad(y, (ta, tb), gd.clone())
    return {"out": out.cpu(), "g_a": ga.cpu(), "g_b": gb.cpu(), "g_a_alone": ga1.cpu(), "g_b_alone": gb1.cpu(),
            "torch_out": y.detach().cpu(), "torch_g_a": tga.cpu(), "torch_g_b": tgb.cpu()}


@pytest.mark.parametrize("n", FLAT_N)
def test_sqdiff_is_torch_bit_for_bit(dev, n):
    r = _both(_run_sqdiff, n)
    a, b, gout = _sq_data(n)
    for k in ("out", "g_a", "g_b"):
        assert _bits_equal(r[k], r["torch_" + k]), "%s differs from torch on the device" % k
    assert _bits_equal(r["g_a"], r["g_a_alone"]) and _bits_equal(r["g_b"], r["g_b_alone"])
    d = a - b
    assert _bits_equal(r["out"], d * d) and _bits_equal(r["g_a"], gout * d + gout * d) and _bits_equal(r["g_b"], -r["g_a"])


def _blend_data(n):
    g = torch.Generator().manual_seed(100 + n)
    o = torch.rand(n, generator=g) * 60 - 30
    o[::5] = 200.0
    o[2::7] = -200.0
    return (o, torch.rand(n, generator=g) * 4, torch.rand(n, generator=g) * 4, torch.randn(n, generator=g),
            torch.randn(n, generator=g))


def _run_blend_soft(n, aligned):
    dev = torch.device("cuda:0")
    L, st = _L(), _st()
    o, a, b, gout, gsoft = _blend_data(n)
    P = Place(dev, aligned)
    od, ad, bd, gd, sd = P.inp(o), P.inp(a), P.inp(b), P.inp(gout), P.inp(gsoft)
    names = ("out", "soft", "plain", "go", "ga", "gb", "go_plain", "ga_plain", "gb_plain", "go_nosoft", "ga_nosoft",
             "gb_nosoft", "go_noout", "ga_noout", "gb_noout")
    t = {k: P.out((n,)) for k in names}
    assert L.decnet_sigmoid_blend_soft(_p(od), _p(ad), _p(bd), _p(t["out"]), _p(t["soft"]), n, st) == 0
    assert L.decnet_sigmoid_blend(_p(od), _p(ad), _p(bd), _p(t["plain"]), n, st) == 0
    bwd = L.decnet_sigmoid_blend_soft_backward
    assert bwd(_p(od), _p(ad), _p(bd), _p(gd), _p(sd), _p(t["go"]), _p(t["ga"]), _p(t["gb"]), n, st) == 0
    assert L.decnet_sigmoid_blend_backward(_p(od), _p(ad), _p(bd), _p(gd), _p(t["go_plain"]), _p(t["ga_plain"]),
                                           _p(t["gb_plain"]), n, st) == 0
    assert bwd(_p(od), _p(ad), _p(bd), _p(gd), None, _p(t["go_nosoft"]), _p(t["ga_nosoft"]), _p(t["gb_nosoft"]), n, st) == 0
    assert bwd(_p(od), _p(ad), _p(bd), None, _p(sd), _p(t["go_noout"]), _p(t["ga_noout"]), _p(t["gb_noout"]), n, st) == 0
    P.check("sigmoid blend soft")
    Po, Pn = Place(dev, aligned), Place(dev, aligned)                   # g_o alone: g_a, g_b NULL
    go1, spare = Po.out((n,)), Pn.out((n,))
    assert bwd(_p(od), _p(ad), _p(bd), _p(gd), _p(sd), _p(go1), None, None, n, st) == 0
    Po.check("sigmoid blend soft backward, g_o alone")
    Pn.check_untouched("sigmoid blend soft backward, g_o alone")
    r = {k: v.cpu() for k, v in t.items()}
    r["go_alone"] = go1.cpu()
    return r


@pytest.mark.parametrize("n", FLAT_N)
def test_blend_soft_is_the_blend_and_its_backward(dev, n):
    r = _both(_run_blend_soft, n)
    o, a, b, gout, gsoft = (t.double() for t in _blend_data(n))
    assert _bits_equal(r["out"], r["plain"]), "decnet_sigmoid_blend_soft differs from decnet_sigmoid_blend"
    s64 = torch.sigmoid(o)
    assert _sigmoid_ok(r["soft"], o)[0]
    assert float(r["soft"][0]) == 1.0 and (n < 3 or float(r["soft"][2]) == 0.0)            # o = 200, -200: saturated
    for k in ("go", "ga", "gb"):
        assert _bits_equal(r[k + "_nosoft"], r[k + "_plain"]), "%s without gsoft differs from decnet_sigmoid_blend_backward" % k
    assert _bits_equal(r["ga"], r["ga_plain"]) and _bits_equal(r["gb"], r["gb_plain"]) and _bits_equal(r["go"], r["go_alone"])
    d = s64 * (1 - s64)
    for k, ref, scale in (("go", (gout * (b - a) + gsoft) * d, (gout * (b - a)).abs() + gsoft.abs()),
                          ("go_noout", gsoft * d, gsoft.abs())):
        err = (r[k].double() - ref).abs()
        print(n, k, "worst error / bound = %.3g" % float((err / (8 * U * scale).clamp_min(1e-300)).max()))
        assert bool((err <= 8 * U * scale).all()), k
        assert not bool(torch.isnan(r[k]).any()) and float(r[k][0]) == 0.0                  # saturation: exactly 0
    assert float(r["ga_noout"].abs().max()) == 0.0 and float(r["gb_noout"].abs().max()) == 0.0


def test_flat_refusals_write_nothing(dev):
    L, st = _L(), _st()
    P = Place(dev, True)
    x = P.inp(torch.zeros(5))
    o1, o2, o3 = P.out((5,)), P.out((5,)), P.out((5,))
    big = (1 << 40) + 1
    assert L.decnet_sqdiff(None, _p(x), _p(o1), 5, st) == ERR_NULL and L.decnet_sqdiff(_p(x), _p(x), None, 5, st) == ERR_NULL
    assert L.decnet_sqdiff(_p(x), _p(x), _p(o1), 0, st) == ERR_SHAPE
    assert L.decnet_sqdiff(_p(x), _p(x), _p(o1), big, st) == ERR_UNSUPPORTED
    assert L.decnet_sqdiff_backward(_p(x), _p(x), None, _p(o1), _p(o2), 5, st) == ERR_NULL
    assert L.decnet_sqdiff_backward(_p(x), _p(x), _p(x), None, None, 5, st) == ERR_NULL
    assert L.decnet_sqdiff_backward(_p(x), _p(x), _p(x), _p(o1), _p(o2), 0, st) == ERR_SHAPE
    assert L.decnet_sqdiff_backward(_p(x), _p(x), _p(x), _p(o1), _p(o2), big, st) == ERR_UNSUPPORTED
    assert L.decnet_detail_tail_backward(_p(x), None, _p(o1), 5, st) == ERR_NULL
    assert L.decnet_detail_tail_backward(_p(x), _p(x), None, 5, st) == ERR_NULL
    assert L.decnet_detail_tail_backward(_p(x), _p(x), _p(o1), 0, st) == ERR_SHAPE
    assert L.decnet_detail_tail_backward(_p(x), _p(x), _p(o1), big, st) == ERR_UNSUPPORTED
    assert L.decnet_sigmoid_blend_soft(_p(x), _p(x), _p(x), _p(o1), None, 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend_soft(_p(x), _p(x), _p(x), None, _p(o2), 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend_soft(None, _p(x), _p(x), _p(o1), _p(o2), 5, st) == ERR_NULL
    assert L.decnet_sigmoid_blend_soft(_p(x), _p(x), _p(x), _p(o1), _p(o2), 0, st) == ERR_SHAPE
    assert L.decnet_sigmoid_blend_soft(_p(x), _p(x), _p(x), _p(o1), _p(o2), big, st) == ERR_UNSUPPORTED
    bwd = L.decnet_sigmoid_blend_soft_backward
    assert bwd(_p(x), _p(x), _p(x), None, None, _p(o1), _p(o2), _p(o3), 5, st) == ERR_NULL
    assert bwd(_p(x), _p(x), _p(x), _p(x), _p(x), None, _p(o2), _p(o3), 5, st) == ERR_NULL
    assert bwd(_p(x), None, _p(x), _p(x), _p(x), _p(o1), _p(o2), _p(o3), 5, st) == ERR_NULL
    assert bwd(_p(x), _p(x), _p(x), _p(x), _p(x), _p(o1), _p(o2), _p(o3), 0, st) == ERR_SHAPE
    assert bwd(_p(x), _p(x), _p(x), _p(x), _p(x), _p(o1), _p(o2), _p(o3), big, st) == ERR_UNSUPPORTED
    P.check_untouched("rejected flat entries")
    assert bwd(_p(x), _p(x), _p(x), _p(x), _p(x), _p(o1), _p(o2), _p(o3), 5, st) == 0
    P.check("accepted decnet_sigmoid_blend_soft_backward")


# ---- 2. decnet_detail_tail ---------------------------------------------------------------------------------------------------------
TAIL = [(1, 1, 1), (2, 3, 63), (1, 2, 64), (1, 2, 65), (2, 3, 129), (1, 1, 1023), (1, 2, 1026)]
THOLD = 0.37
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(("prob", "mask", "bits"), k)]


def _tail_data(B, H, W):
    g = torch.Generator().manual_seed(B * 100000 + H * 10000 + W)
    z = torch.rand(B, H, W, generator=g) * 60 - 30
    flat = z.view(-1)
    flat[0] = 200.0
    if flat.numel() > 1:
        flat[-1] = -200.0
    if flat.numel() > 70:
        flat[61], flat[64] = -200.0, 200.0
    return z, torch.randn(B, H, W, generator=g)


def _tail_call(L, z, thold, P, want, B, H, W):
    """One decnet_detail_tail call with the outputs in `want`; the others are passed as NULL."""
    nw = (W + 63) // 64
    prob = P.out((B, H, W)) if "prob" in want else None
    mask = P.out((B, H, W)) if "mask" in want else None
    bits = torch.full((B, H, nw), -1, dtype=torch.int64, device=z.device) if "bits" in want else None
    assert L.decnet_detail_tail(_p(z), thold, _p(prob), _p(mask), _p(bits), B, H, W, _st()) == 0
    return prob, mask, bits


def _run_tail(B, H, W, aligned):
    dev = torch.device("cuda:0")
    L, st = _L(), _st()
    z, g = _tail_data(B, H, W)
    P = Place(dev, aligned)
    zd, gd = P.inp(z), P.inp(g)
    r = {}
    for want in SUBSETS:
        Pw, Pn = Place(dev, aligned), Place(dev, aligned)
        spare = Pn.out((B, H, W))
        for k, t in zip(("prob", "mask", "bits"), _tail_call(L, zd, THOLD, Pw, want, B, H, W)):
            if t is not None:
                r["%s of %s" % (k, "+".join(want))] = t.cpu()
        Pw.check("detail_tail %s" % (want,))
        Pn.check_untouched("detail_tail %s" % (want,))
    gz = P.out((B, H, W))
    assert L.decnet_detail_tail_backward(_p(zd), _p(gd), _p(gz), B * H * W, st) == 0
    P.check("detail_tail")
    r["g_logits"] = gz.cpu()
    return r


@pytest.mark.parametrize("B,H,W", TAIL)
def test_detail_tail_edges(dev, B, H, W):
    from spy_util import unpack_mask_bits
    r = _both(_run_tail, B, H, W)
    z, g = _tail_data(B, H, W)
    full = "prob+mask+bits"
    prob, mask, bits = r["prob of " + full], r["mask of " + full], r["bits of " + full]
    for want in SUBSETS:                                                  # every subset writes what the full call writes
        for k in want:
            assert _bits_equal(r["%s of %s" % (k, "+".join(want))], r["%s of %s" % (k, full)]), (k, want)
    s64 = torch.sigmoid(z.double())
    ok, worst = _sigmoid_ok(prob, z)
    print((B, H, W), "prob: worst error / bound = %.3g" % worst)
    assert ok
    assert float(prob.view(-1)[0]) == 1.0 and (z.numel() < 2 or float(prob.view(-1)[-1]) == 0.0)   # +-200: exactly 1 and 0
    assert torch.equal(mask, (prob > torch.tensor(THOLD, dtype=torch.float32)).float())
    assert 0.0 < float(mask.mean()) < 1.0 or z.numel() < 3
    nw = (W + 63) // 64
    assert bits.shape == (B, H, nw)
    assert torch.equal(unpack_mask_bits(bits, W), mask)
    assert torch.equal(unpack_mask_bits(bits, nw * 64)[:, :, W:], torch.zeros(B, H, nw * 64 - W)), "bits past W must be zero"
    ref = g.double() * (s64 * (1 - s64))
    eg = (r["g_logits"].double() - ref).abs()
    print((B, H, W), "g_logits: worst error / bound = %.3g" % float((eg / (8 * U * g.double().abs()).clamp_min(1e-300)).max()))
    assert bool((eg <= 8 * U * g.double().abs()).all())
    assert not bool(torch.isnan(r["g_logits"]).any()) and float(r["g_logits"].view(-1)[0]) == 0.0


def test_detail_tail_refusals_write_nothing(dev):
    L, st = _L(), _st()
    B, H, W = 1, 2, 5
    P = Place(dev, True)
    z = P.inp(torch.zeros(B, H, W))
    prob, mask = P.out((B, H, W)), P.out((B, H, W))
    bits = torch.full((B, H, 1), -1, dtype=torch.int64, device=dev)

    def call(z_=z, p=prob, m=mask, b=bits, B_=B, H_=H, W_=W):
        return L.decnet_detail_tail(_p(z_), 0.5, _p(p), _p(m), _p(b), B_, H_, W_, st)
    assert call(z_=None) == ERR_NULL and call(p=None, m=None, b=None) == ERR_NULL
    assert call(B_=0) == ERR_SHAPE and call(H_=0) == ERR_SHAPE and call(W_=0) == ERR_SHAPE
    assert call(B_=65536) == ERR_SHAPE and call(H_=65536) == ERR_SHAPE          # as decnet_detail_mask
    assert call(W_=(1 << 28) + 1) == ERR_UNSUPPORTED and call(B_=65535, H_=65535, W_=1024) == ERR_UNSUPPORTED
    P.check_untouched("rejected decnet_detail_tail")
    assert bool((bits == -1).all())
    assert call() == 0
    P.check("accepted decnet_detail_tail")
    assert not bool((bits == -1).any())


@pytest.mark.parametrize("H,W", [(6, 66), (3, 1026)])
def test_detail_tail_reproduces_detail_mask_from_its_logits(dev, H, W):
    from decnet_amd import ops2d
    gen, cur, pre, thold = MC.mask_case(H, W)
    gen = gen.to(dev)
    with torch.no_grad():
        c3, p3 = gen.conv_sub(cur.to(dev)).contiguous(), gen.deconv(pre.to(dev)).contiguous()
        mask, bits, logits = ops2d.detail_mask(c3, p3, gen._host_params(), thold, True, want_logits=True)
        m0, b0 = ops2d.detail_mask(c3, p3, gen._host_params(), thold, True)
        prob, m1, b1 = ops2d.detail_tail(logits, thold, True, True, True)
    assert _bits_equal(m0, mask) and torch.equal(b0, bits)                  # want_logits changes neither
    assert _bits_equal(m1, mask) and torch.equal(b1, bits), "decnet_detail_tail differs from decnet_detail_mask on its logits"
    assert torch.equal(mask, (prob > torch.tensor(thold, dtype=torch.float32, device=dev)).float())
    assert 0.3 < float(mask.mean()) < 0.7


# ---- 3. the Functions ------------------------------------------------------------------------------------------------------------
def test_functions_hand_autograd_what_the_entries_wrote(dev):
    import decnet_amd
    from decnet_amd import ops2d
    g = torch.Generator().manual_seed(14)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)                 # noqa: E731
    for _ in range(2):                                                    # double apply: nothing is left behind
        a, b, go = rn(2, 3, 5, 7).requires_grad_(), rn(2, 3, 5, 7).requires_grad_(), rn(2, 3, 5, 7)
        out = decnet_amd.SquaredDiffFunction.apply(a, b)
        out.backward(go)
        assert _bits_equal(out.detach(), ops2d.sqdiff(a.detach(), b.detach()))
        assert all(_bits_equal(t.grad, w) for t, w in zip((a, b), ops2d.sqdiff_backward(a.detach(), b.detach(), go)))
        z, gp = (rn(2, 5, 70) * 4).requires_grad_(), rn(2, 5, 70)
        prob, mask, bits = decnet_amd.DetailTailFunction.apply(z, 0.4, True)
        assert prob.requires_grad and not mask.requires_grad and not bits.requires_grad and bits.dtype == torch.int64
        want = ops2d.detail_tail(z.detach(), 0.4, True, True, True)
        assert _bits_equal(prob.detach(), want[0]) and _bits_equal(mask, want[1]) and torch.equal(bits, want[2])
        prob.backward(gp)
        assert _bits_equal(z.grad, ops2d.detail_tail_backward(z.detach(), gp))
        assert decnet_amd.DetailTailFunction.apply(z, 0.4, False)[2] is None
        o, x, y = rn(3, 7, 9).requires_grad_(), rn(3, 7, 9).requires_grad_(), rn(3, 7, 9).requires_grad_()
        g1, g2 = rn(3, 7, 9), rn(3, 7, 9)
        fused, soft = decnet_amd.SigmoidBlendSoftFunction.apply(o, x, y)
        assert _bits_equal(fused.detach(), decnet_amd.SigmoidBlendFunction.apply(o.detach(), x.detach(), y.detach()))
        torch.autograd.backward((fused, soft), (g1, g2))
        want = ops2d.sigmoid_blend_soft_backward(o.detach(), x.detach(), y.detach(), g1, g2)
        assert all(_bits_equal(t.grad, w) for t, w in zip((o, x, y), want))


def test_functions_launch_only_what_is_asked_for(dev):
    import decnet_amd
    from decnet_amd import _lib, ops
    from spy_util import entry_spy
    g = torch.Generator().manual_seed(15)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)                 # noqa: E731
    with entry_spy() as calls:
        for fn, args in ((decnet_amd.SquaredDiffFunction, (rn(7), rn(7))),          # nothing requires grad: no backward launches
                         (decnet_amd.SigmoidBlendSoftFunction, (rn(7), rn(7), rn(7)))):
            leaf = torch.zeros((), device=dev, requires_grad=True)
            out = fn.apply(*args)
            ((out[0] if isinstance(out, tuple) else out).sum() * 0 + leaf).backward()
        leaf = torch.zeros((), device=dev, requires_grad=True)
        (decnet_amd.DetailTailFunction.apply(rn(1, 2, 7), 0.5, False)[0].sum() * 0 + leaf).backward()
        z = rn(1, 2, 7).requires_grad_()
        (decnet_amd.DetailTailFunction.apply(z, 0.5, True)[1].sum() * 0 + leaf).backward()      # the mask alone: no graph to z
        assert z.grad is None
        assert [c for c in calls if c.endswith("_backward")] == [], calls
        del calls[:]
        a, b = rn(7).requires_grad_(), rn(7)
        decnet_amd.SquaredDiffFunction.apply(a, b).sum().backward()
        assert calls == ["decnet_sqdiff", "decnet_sqdiff_backward"] and a.grad is not None and b.grad is None
    seen = []

    def spied(name):                                                    # the pointer arguments of every backward call
        real = getattr(_lib.lib(), name)

        def call(*a):
            seen.append((name, a))
            return real(*a)
        return call
    saved = dict(ops._FN)
    ops._FN.clear()
    for n in ("decnet_sqdiff_backward", "decnet_sigmoid_blend_soft_backward"):
        ops._FN[n] = spied(n)
    try:
        a, b = rn(7), rn(7).requires_grad_()                                # g_a is not asked for: a NULL pointer
        decnet_amd.SquaredDiffFunction.apply(a, b).sum().backward()
        o, x, y = rn(7).requires_grad_(), rn(7), rn(7).requires_grad_()
        fused, soft = decnet_amd.SigmoidBlendSoftFunction.apply(o, x, y)
        fused.sum().backward()                                              # soft unused: no gsoft tensor, g_a skipped
        o2, x2, y2 = rn(7).requires_grad_(), rn(7).requires_grad_(), rn(7).requires_grad_()
        fused2, soft2 = decnet_amd.SigmoidBlendSoftFunction.apply(o2, x2, y2)
        soft2.sum().backward()                                              # fused unused: no gout tensor, no g_a / g_b
    finally:
        ops._FN.clear()
        ops._FN.update(saved)
    assert [n for n, _ in seen] == ["decnet_sqdiff_backward"] + ["decnet_sigmoid_blend_soft_backward"] * 2
    assert seen[0][1][3] is None and seen[0][1][4] and a.grad is None and b.grad is not None
    _, (_, _, _, gout, gsoft, g_o, g_a, g_b, _, _) = seen[1]
    assert gout and gsoft is None and g_o and g_a is None and g_b
    assert x.grad is None and _bits_equal(y.grad, ops2d_blend_backward(o, x, y)[2])
    _, (_, _, _, gout, gsoft, g_o, g_a, g_b, _, _) = seen[2]
    assert gout is None and gsoft and g_o and g_a is None and g_b is None
    assert o2.grad is not None and x2.grad is None and y2.grad is None


def ops2d_blend_backward(o, a, b):
    from decnet_amd import ops2d
    return ops2d.sigmoid_blend_backward(o.detach(), a.detach(), b.detach(), torch.ones_like(o))


# ---- 4. detail() -------------------------------------------------------------------------------------------------------------------
LIBRARY_NODES = ("ConvolutionBackward0", "NativeBatchNormBackward0", "CudnnBatchNormBackward0", "MiopenBatchNormBackward0",
                 "SigmoidBackward0")
_VALUES = {}


def _value_run(H, W, mode):
    """detail() under hip_grad() on the value case, with the entries it made and the autograd nodes behind prob."""
    from spy_util import entry_spy
    key = (H, W, mode)
    if key not in _VALUES:
        c = DR.value_case(H, W, mode)
        dev = torch.device("cuda:0")
        gen = DR.copy_of(c["gen"], mode, torch.float32, dev)
        cur, pre = c["cur"].to(dev).requires_grad_(), c["pre"].to(dev).requires_grad_()
        with entry_spy() as calls:
            with _hip():
                prob, mask, bits = gen.detail(cur, pre, c["thold"], want_bits=True)
            fwd = list(calls)
            del calls[:]
            prob.sum().backward()
            bwd = list(calls)
        _VALUES[key] = dict(prob=prob, mask=mask, bits=bits, fwd=fwd, bwd=bwd, names=DR.node_names(prob), gen=gen)
    return _VALUES[key]


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_detail_routes_under_hip_grad(dev, H, W, mode):
    r = _value_run(H, W, mode)
    mine = [c for c in r["fwd"] + r["bwd"] if c in ("decnet_sqdiff", "decnet_detail_tail", "decnet_sqdiff_backward",
                                                     "decnet_detail_tail_backward", "decnet_detail_mask")]
    assert mine == ["decnet_sqdiff", "decnet_detail_tail", "decnet_detail_tail_backward", "decnet_sqdiff_backward"], mine
    names = r["names"]
    assert names.count("DetailTailFunctionBackward") == 1 and names.count("SquaredDiffFunctionBackward") == 1, names
    assert not [n for n in names if n in LIBRARY_NODES], names              # from 256 pixels every unit is a Function
    assert names.count("Conv2dSmallFunctionBackward") == 5 and names.count("Deconv2dS3FunctionBackward") == 1, names
    assert names.count("BatchNormActFunctionBackward") == (4 if mode == "train" else 0), names
    assert r["prob"].grad_fn is not None and not r["mask"].requires_grad and r["mask"].grad_fn is None
    assert r["bits"].dtype == torch.int64 and r["bits"].shape == (2, H, (W + 63) // 64)


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_detail_values_against_float64(dev, H, W, mode):
    from spy_util import unpack_mask_bits
    c, r = DR.value_case(H, W, mode), _value_run(H, W, mode)
    prob, mask = r["prob"].detach().cpu(), r["mask"].cpu()
    p64 = torch.sigmoid(c["logit64"])
    err = float((prob.double() - p64).abs().max())
    print((H, W), mode, "prob: hip %.3g  bound %.3g" % (err, c["bound"] / 4))
    assert err <= c["bound"] / 4
    assert torch.equal(mask, (prob > torch.tensor(c["thold"], dtype=torch.float32)).float())
    assert torch.equal(unpack_mask_bits(r["bits"], W).cpu(), mask)
    unsure = DR.unsure(c)
    assert int(unsure.sum()) <= DR.CAP * unsure.numel()
    ref = (p64 > c["thold"]).float()
    assert torch.equal(mask[~unsure], ref[~unsure]), "the mask differs from the float64 decision away from thold"


@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_detail_no_grad_route_is_mask_plus_prob(dev, H, W):
    from spy_util import entry_spy, unpack_mask_bits
    c = DR.value_case(H, W, "eval")
    gen = DR.copy_of(c["gen"], "eval", torch.float32, dev)
    cur, pre = c["cur"].to(dev), c["pre"].to(dev)
    with torch.no_grad():
        m0, b0 = gen.mask(cur, pre, c["thold"], want_bits=True)
        with entry_spy() as calls:
            prob, mask, bits = gen.detail(cur, pre, c["thold"], want_bits=True)
            p1, m1, none = gen.detail(cur, pre, c["thold"])
    mine = [n for n in calls if "detail" in n or "sqdiff" in n]
    assert mine == ["decnet_detail_mask", "decnet_detail_tail"] * 2, calls
    assert _bits_equal(mask, m0) and torch.equal(bits, b0) and none is None and _bits_equal(m1, m0) and _bits_equal(p1, prob)
    assert prob.grad_fn is None and torch.equal(mask, (prob > torch.tensor(c["thold"], device=dev)).float())
    assert torch.equal(unpack_mask_bits(bits, W), mask)
    err = float((prob.cpu().double() - torch.sigmoid(c["logit64"])).abs().max())
    assert err <= c["bound"] / 4, (err, c["bound"] / 4)
    with torch.no_grad():                                                   # train mode without autograd: torch ops, no bits
        gt = DR.copy_of(c["gen"], "train", torch.float32, dev)
        with entry_spy() as calls:
            pt, mt, bt = gt.detail(cur, pre, c["thold"], want_bits=True)
    assert bt is None and not [n for n in calls if "detail" in n or "sqdiff" in n], calls
    assert torch.equal(mt, (pt > c["thold"]).float())


def test_detail_on_the_cpu_is_torch(dev):
    from spy_util import entry_spy
    c = DR.value_case(6, 66, "eval")
    gen = DR.copy_of(c["gen"], "eval", torch.float32)
    with entry_spy() as calls:
        with _hip():
            prob, mask, bits = gen.detail(c["cur"], c["pre"], c["thold"], want_bits=True)
    assert calls == [] and bits is None and "SigmoidBackward0" in DR.node_names(prob)
    assert torch.equal(mask, (prob.detach() > c["thold"]).float())


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_detail_gradients_against_float64(dev, H, W, mode):
    c = DR.grad_case(H, W, mode)
    ghip, bufs, prob, mask = DR.detail_grads(c["gen"], c["cur"], c["pre"], c["thold"], c["r"], mode, torch.float32, dev, _hip)
    assert ghip.keys() == c["g64"].keys()
    rows = {k: (float((ghip[k].double() - c["g64"][k]).abs().max()), BR.gate(c["g64"][k], c["g32"][k])) for k in ghip}
    for k, (e, gate) in rows.items():
        print((H, W), mode, k, "hip %.3g  gate %.3g" % (e, gate))
    for k, (e, gate) in rows.items():
        assert ghip[k].shape == c["g64"][k].shape and e <= gate, (k, e, gate)
    before = dict(c["gen"].named_buffers())
    for k, ref in c["buf64"].items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(ref) == (1 if mode == "train" else 0), k
        elif mode == "train":
            assert MC.close(bufs[k], ref, MC.FP32_TOL) <= 1.0, k
        else:
            assert torch.equal(bufs[k], before[k]), k


# ---- 5. fuse(want_soft=True) ----------------------------------------------------------------------------------------------------------
def _fuse_args(ins, dev, wrt=()):
    return [ins[k].to(dev).requires_grad_(k in wrt) for k in ("fea", "dense", "sparse", "mask", "var")]


@pytest.mark.parametrize("mode", DR.MODES)
def test_fuse_with_soft_keeps_the_bits_of_fuse(dev, mode):
    from spy_util import entry_spy
    m, ins, wrt, r1, r2, k = DR.fuse_case(mode)
    assert k is not None
    a, b = DR.copy_of(m, mode, torch.float32, dev), DR.copy_of(m, mode, torch.float32, dev)
    with entry_spy() as calls:
        with _hip():
            fused, soft = a.fuse(*_fuse_args(ins, dev, wrt), want_soft=True)
        with_soft = list(calls)
        del calls[:]
        with _hip():
            alone = b.fuse(*_fuse_args(ins, dev, wrt))
        plain = list(calls)
    assert _bits_equal(fused, alone), "fuse(want_soft=True) changes the fused plane under hip_grad()"
    assert [c for c in with_soft if "blend" in c] == ["decnet_sigmoid_blend_soft"]
    assert [c for c in plain if "blend" in c] == ["decnet_sigmoid_blend"]           # the default: today's entries
    assert [c for c in with_soft if "blend" not in c] == [c for c in plain if "blend" not in c]
    ref = DR.copy_of(m, mode)
    x = torch.cat([ins["fea"]] + [ins[n].unsqueeze(1) for n in ("dense", "sparse", "mask")] + [-ins["var"].unsqueeze(1)], 1)
    with torch.no_grad():
        s64 = ref(x.double()).squeeze(1)
        s32 = DR.copy_of(m, mode, torch.float32)(x).squeeze(1)
    bound = MC.composite_bound(s64, s32, 1.5)
    err = float((soft.detach().cpu().double() - s64).abs().max())
    print(mode, "soft: hip %.3g  bound %.3g" % (err, bound))
    assert err <= bound


def test_fuse_with_soft_without_autograd(dev):
    """The no_grad leg: the last unit without its epilogue, then decnet_sigmoid_blend_soft -- the epilogue route's bits."""
    from spy_util import entry_spy
    m, ins, wrt, r1, r2, _ = DR.fuse_case("eval")
    m = DR.copy_of(m, "eval", torch.float32, dev)
    args = _fuse_args(ins, dev)
    with torch.no_grad(), entry_spy() as calls:
        alone = m.fuse(*args)
        plain = list(calls)
        del calls[:]
        fused, soft = m.fuse(*args, want_soft=True)
    assert plain == ["decnet_conv2d_cat_bn_act", "decnet_conv2d_bn_act", "decnet_conv2d_cat_epilogue"], plain
    assert calls == ["decnet_conv2d_cat_bn_act", "decnet_conv2d_bn_act", "decnet_conv2d_cat_bn_act",
                     "decnet_sigmoid_blend_soft"], calls
    assert _bits_equal(fused, alone), "fuse(want_soft=True) differs from the epilogue route"
    with _hip():
        f2, s2 = m.fuse(*_fuse_args(ins, dev, wrt), want_soft=True)
    assert _bits_equal(f2.detach(), fused) and _bits_equal(s2.detach(), soft)       # hip_grad(): the no_grad forward's bits
    cpu = DR.copy_of(m, "eval", torch.float32, "cpu")
    with torch.no_grad():
        fc, sc = cpu.fuse(*_fuse_args(ins, "cpu"), want_soft=True)
    assert MC.close(soft, sc, MC.FP32_TOL) <= 1.0 and MC.close(fused, fc, MC.FP32_TOL) <= 1.0


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("mode", DR.MODES)
def test_fuse_gradients_against_float64(dev, mode, both):
    m, ins, wrt, r1, r2, _ = DR.fuse_case(mode)
    r1 = r1 if both else None                                               # None: the soft mask alone
    g64 = DR.fuse_grads(m, ins, wrt, r1, r2, mode, D)[0]
    g32 = DR.fuse_grads(m, ins, wrt, r1, r2, mode, torch.float32)[0]
    ghip, _, _, names = DR.fuse_grads(m, ins, wrt, r1, r2, mode, torch.float32, dev, _hip)
    assert names.count("SigmoidBlendSoftFunctionBackward") == 1 and "SigmoidBlendFunctionBackward" not in names, names
    assert g64.keys() == ghip.keys() == g32.keys()
    rows = {k: (float((ghip[k].double() - g64[k]).abs().max()), BR.gate(g64[k], g32[k])) for k in g64}
    for k, (e, gate) in rows.items():
        print(mode, "both" if both else "soft alone", k, "hip %.3g  gate %.3g" % (e, gate))
    for k, (e, gate) in rows.items():
        assert ghip[k].shape == g64[k].shape and e <= gate, (k, e, gate)


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_never_synchronises(dev):
    from decnet_amd.graphs import GraphedStep
    c = DR.grad_case(6, 66, "eval")
    gen = DR.copy_of(c["gen"], "eval", torch.float32, dev)
    m, ins, wrt, r1, r2, _ = DR.fuse_case("eval")
    att = DR.copy_of(m, "eval", torch.float32, dev)
    cur, pre = c["cur"].to(dev).requires_grad_(), c["pre"].to(dev).requires_grad_()
    args = _fuse_args(ins, dev, wrt)
    r, r1, r2, thold = c["r"].to(dev), r1.to(dev), r2.to(dev), c["thold"]
    leaves = [cur, pre] + [t for t in args if t.requires_grad] + list(gen.parameters()) + list(att.parameters())

    def step():
        with _hip():
            prob, mask, bits = gen.detail(cur, pre, thold, want_bits=True)
            fused, soft = att.fuse(*args, want_soft=True)
        ((prob * r).sum() + (fused * r1 + soft * r2).sum()).backward()
        return prob.detach(), mask, bits, fused.detach(), soft.detach()

    def snapshot(outs):
        torch.cuda.synchronize()
        return [t.clone().contiguous() for t in outs] + [p.grad.clone().contiguous() for p in leaves]

    def reset():
        for p in leaves:
            p.grad = None
    reset()
    eager = snapshot(step())                                                # first call: library load, allocator growth
    reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    again = snapshot(outs)
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    graphed = GraphedStep(step, grads_of=leaves)
    for _ in range(2):
        for p in leaves:
            p.grad.fill_(float("nan"))
        replay = snapshot(graphed())
        for i, (a, b) in enumerate(zip(eager, replay)):
            assert a.shape == b.shape and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8)), i
