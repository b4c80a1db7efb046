"""Host proof that tests/test_conv_exact_gpu.py has teeth (tests/_exact.py): the value classes meet their predicates, the
bf16x3 model with all six term products reproduces float64 bit for bit on the selector cases while the model without any
one product does not (each product is pinned by a named pairing), the dense-integer cases are independent of the
summation order in fp32, and the committed selector tables meet their coverage conditions.  No GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _exact as E
import _stage0_ref as R0
import _trunk_ref as R
from _placement import _bits_equal


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,pred", [("T1", E.is_t1), ("T2", E.is_t2), ("T3", E.is_t3)])
def test_classes_meet_their_predicates(cls, pred):
    x = E.draw(cls, (10000,), E.gen("classes", cls))
    assert bool(pred(x).all()) and bool(torch.isfinite(x).all())
    h, m, l = (t.double() for t in E.split3(x))
    assert bool((h + m + l == x.double()).all())
    assert x.unique().numel() >= (15 if cls == "T1" else 42 if cls == "T2" else 9000)
    if cls == "T1":
        assert bool((x == 0).any()) and not bool((E.t1((1000,), E.gen("nz"), zero=False) == 0).any())
        i = E.ints((10000,), E.gen("ints"))
        assert bool(E.is_t1(i).all()) and sorted(i.unique().tolist()) == [-2, -1, 0, 1, 2]


def test_t3_rejection_is_cheap():
    ok = E.is_t3(E._raw_t3(100000, E.gen("raw")))
    assert 0.9 < float(ok.float().mean()) < 1.0              # the predicate does reject, and rarely


def test_subset_sums_of_the_term_products_are_fp32():
    """Whatever order (and grouping into accumulators) a kernel adds the kept products in, no partial sum rounds."""
    g = E.gen("subsets")
    for cx, cw in E.PAIRINGS:
        x, w = E.draw(cx, (10000,), g, zero=False), E.draw(cw, (10000,), g, zero=False)
        prods = [a.double() * b.double() for a in E.split3(x) for b in E.split3(w)]
        kept = [p for p, name in zip(prods, ("hh", "hm", "hl", "mh", "mm", "ml", "lh", "lm", "ll")) if name in E.SIX]
        assert bool((sum(kept) == x.double() * w.double()).all()), "the six kept products are the whole product"
        for n in range(1, 7):
            for sub in itertools.combinations(kept, n):
                assert bool(E._f32(sum(sub)).all()), (cx, cw, n)


# ------------------------------------------------------------------------------------------------------------------
# 3b on the host: coverage of the tables, the model with six products, the model without one
def _sel_rotations(key, pairing, segs, cout, kt, shape_of):
    return [E.selector_case(key, pairing, r, segs, cout, kt, shape_of)
            for r in range(E.rotations(sum(segs), cout, kt))]


@pytest.mark.parametrize("pairing", E.PAIRINGS, ids=["T3xT1", "T1xT3", "T2xT2"])
def test_selector_tables_meet_the_coverage_conditions(pairing):
    for case in E.SEL_CONV:
        segs, cout, k, _, (B, H, W) = case
        assert len(segs) <= 6
        E.assert_coverage([c[1] for c in _sel_rotations(case, pairing, segs, cout, k * k, lambda c: (B, c, H, W))], segs)
    for case in E.SEL_DECONV:
        H, W, cin, cout = case
        E.assert_coverage([c[1] for c in _sel_rotations(case, pairing, (cin,), cout, 9, lambda c: (2, c, H, W))], (cin,))
    for case in E.SEL_TAP:
        Ci, Co, P = case
        assert Ci == 216 and Co <= 224
        E.assert_coverage([c[1] for c in _sel_rotations(case, pairing, (Ci,), Co, 9, lambda c: (1, c, 1, P))], (Ci,))


def test_coverage_assertion_sees_a_gap():
    ws = [E.selector_weight(torch.ones(17), r, 24, 9) for r in range(2)]
    E.assert_coverage(ws, (24,))
    with pytest.raises(AssertionError):
        E.assert_coverage(ws[:1], (24,))                             # 17 of 24 channels
    with pytest.raises(AssertionError):
        E.assert_coverage([ws[0], ws[1] * 0], (24,))                 # an output channel without a weight
    with pytest.raises(AssertionError):
        E.rotations(216, 17, 9)                                      # 13 > MAX_ROT: why SEL_TAP has Co = 18


def test_pins_name_every_product():
    assert set(sum(E.PINS.values(), ())) == set(E.SIX)
    assert all("hh" in v for v in E.PINS.values())


@pytest.mark.parametrize("pairing", E.PAIRINGS, ids=["T3xT1", "T1xT3", "T2xT2"])
def test_model_is_exact_and_each_product_is_pinned(pairing):
    """emulate(SIX) is the float64 convolution bit for bit (and representable in fp32); without any one of the products
    this pairing pins, at least one output of every case differs."""
    for case in E.SEL_CONV:
        segs, cout, k, dil, (B, H, W) = case
        for xs, w, scale, shift, relu in _sel_rotations(case, pairing, segs, cout, k * k, lambda c: (B, c, H, W)):
            x, w4 = torch.cat(xs, 1), w.view(cout, -1, k, k)
            op = lambda a, b: R.conv(a, b, dil)
            want = R.conv(x, w4, dil)
            assert torch.equal(E.emulate(x, w4, E.SIX, op), want)
            assert _bits_equal(E.exact_or_fail(R.bn_act(want, scale, shift, relu)),
                               R.bn_act(want, scale, shift, relu).float())
            for p in E.PINS[pairing]:
                assert not torch.equal(E.emulate(x, w4, [q for q in E.SIX if q != p], op), want), (case, p)
            for p in set(E.SIX) - set(E.PINS[pairing]) - {"hm", "mh"}:       # (T2 x T2 has hm and mh as well)
                assert torch.equal(E.emulate(x, w4, [q for q in E.SIX if q != p], op), want), (case, p)


def test_dropped_product_is_invisible_to_the_max_norm_gate():
    """Why these tests exist: on the suite's random data a layer without one term product passes the 4e-6 gate."""
    g = E.gen("gate")
    x, w = torch.randn(1, 24, 5, 16, generator=g), torch.randn(24, 24, 3, 3, generator=g) / 216 ** 0.5
    want = R.conv(x, w)
    gate = 4e-6 * max(1.0, float(want.abs().max()))
    assert float((E.emulate(x, w) - want).abs().max()) < 1e-6
    for p in ("hl", "lh"):                                           # (mm: 0.7 - 0.97 of the gate, too close to assert)
        err = float((E.emulate(x, w, [q for q in E.SIX if q != p]) - want).abs().max())
        assert 0.1 * gate < err < gate, (p, err, gate)


# ------------------------------------------------------------------------------------------------------------------
# 3a on the host: fp32 in two channel orders equals float64 bit for bit
def _two_orders(run, cin, ref):
    want = E.exact_or_fail(ref, 1 / 16)
    for perm in (torch.arange(cin), torch.arange(cin).flip(0), torch.randperm(cin, generator=E.gen("perm", cin))):
        assert _bits_equal(run(perm) + 0.0, want)


def _bn32(y, scale, shift, relu):
    y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def test_dense_2d_cases_are_order_independent():
    T = E.tables()
    for case in T["small"] + T["mfma"]:
        segs, cout, k, dil, (B, H, W), relu = case[:6]
        xs, w, scale, shift = E.dense2d(case, segs, cout, k, B, H, W)
        x = torch.cat(xs, 1)
        assert sum(segs) * k * k * 2 * 2 + 3 < 2 ** 20                # every partial sum, in any order
        _two_orders(lambda p: _bn32(F.conv2d(x[:, p], w[:, p], padding=dil * (k // 2), dilation=dil), scale, shift, relu),
                    sum(segs), R.conv_bn_act(xs, w, scale, shift, dil, relu))
    for (H, W, cin, cout), tr in T["s3"]:
        (x,), w, scale, shift = E.dense2d(("s3", H, W, cin, cout, tr), (cin,), cout, 3, 2, H, W, tr)
        if tr:
            _two_orders(lambda p: _bn32(F.conv_transpose2d(x[:, p], w[p], stride=3), scale, shift, True), cin,
                        R.deconv_s3_bn_act(x, w, scale, shift, True))
        else:
            _two_orders(lambda p: _bn32(F.conv2d(x[:, p], w[:, p], stride=3, padding=1), scale, shift, True), cin,
                        R.conv_s3_bn_act(x, w, scale, shift, True))
    for H, W, cin, cout in T["deconv"]:
        (x,), w, scale, shift = E.dense2d(("deconv", H, W, cin, cout), (cin,), cout, 3, 2, H, W, True)
        _two_orders(lambda p: _bn32(F.conv_transpose2d(x[:, p], w[p], stride=3), scale, shift, True), cin,
                    R.deconv_s3_bn_act(x, w, scale, shift, True))
    for case in T["tap"]:
        Ci, Co, _, brs = case
        x, ws, scale, shift = E.dense_tap(case)
        ks, dils = [k for k, _ in brs], [d for _, d in brs]
        _two_orders(lambda p: _bn32(torch.cat([F.conv2d(x[:, p], w[:, p], padding=d * (k // 2), dilation=d)
                                               for w, k, d in zip(ws, ks, dils)], 1), scale, shift, True), Ci,
                    R.tap_gather(R.tap_gemm(x, ws), ks, dils, scale, shift, True))


def test_dense_3d_cases_are_order_independent():
    T = E.tables()
    assert set(T["conv"]) <= set(T["wino"]) and max(c[4] for c in T["wino"]) == 216
    for case in T["wino"]:
        B, Dd, H, W, Ci, Co, relu, res = case
        E.wino0_bound(Ci)
        x, w, scale, shift, resid = E.dense3d(case)

        def run(p):
            y = F.conv3d(x.permute(0, 4, 1, 2, 3)[:, p], w[:, p], padding=1).permute(0, 2, 3, 4, 1) * scale + shift
            y = torch.relu(y) if relu else y
            return y + resid if res else y
        _two_orders(run, Ci, R0.conv3d_unit(x, w, scale, shift, resid, relu))
    for row in T["pointwise"]:
        B, Ci, Co, P, ldw, cl = row
        x, w = E.dense_pointwise(row)
        wm = torch.stack([w[co * ldw:co * ldw + Ci] for co in range(Co)])
        _two_orders(lambda p: x[:, :, p] @ wm[:, p].t() if cl else torch.einsum("oc,bcp->bop", wm[:, p], x[:, p]), Ci,
                    R0.pointwise(x, w, ldw, cl))
    for case in T["cout1"]:
        assert case[5] is None
        x, w, scale, shift = E.dense_cout1(case)
        _two_orders(lambda p: F.conv3d(x.permute(0, 4, 1, 2, 3)[:, p], w[:, p], padding=1)[:, 0] * scale + shift,
                    case[4], R0.cout1_softargmax(x, w, scale, shift)[0])


def test_gemm0_weights_transform_to_integers():
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    for Ci, Co in E.GEMM0_CICO:
        V, w = E.dense_gemm0(97, Ci, Co)
        U = torch.einsum("xi,yj,zk,ocijk->ocxyz", G, G, G, w.double())
        assert bool((U == U.round()).all()) and float(U.abs().max()) <= 27 and float(V.abs().max()) <= 2
        assert Ci * 27 * 2 < 2 ** 24 and not bool(V[:, Ci:].any())
