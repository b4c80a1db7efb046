"""Host proof that tests/test_spamat_exact_gpu.py has teeth (tests/_spamat_exact.py): the truncation classes meet their
predicates, every subset sum of the kept term products is an fp32 number, the flat cases are exact from their magnitudes,
the host model of spamat_bwd_rowb reproduces the float64 reference bit for bit on the selector cases while the model without
any one pinned product -- everywhere, or only in one K group, one channel block or one band tile -- does not, and the
selector tables reach every role of every rowb instantiation (the coverage table is printed: pytest -s).  No GPU."""
import itertools

import pytest
import torch

import _spamat_exact as X


def _f32(v):
    return v.float().double() == v


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["K1", "K2", "K3"])
def test_classes_meet_their_predicates(cls):
    x = X.draw_view(cls, (10000,), X.gen("spamat-classes", cls))
    assert bool(X.PRED[cls](x).all()) and bool(torch.isfinite(x).all()) and not bool((x == 0).any())
    h, m, l = (t.double() for t in X.split3(x))
    assert bool((h + m + l == x.double()).all())
    assert bool((h.abs() >= m.abs()).all()) and bool((h * m >= 0).all()) and bool((h * l >= 0).all())   # truncation
    assert x.unique().numel() >= (14 if cls == "K1" else 42 if cls == "K2" else 9000)
    d = torch.arange(0, 225).repeat(40)
    out = X.draw_out(cls, d, X.gen("spamat-out", cls))
    w = (d.double() - out.double()).float()
    assert bool(X.PRED[cls](w).all()) and float(out.min()) >= 0 and float(out.max()) < 256
    assert bool((out.double() * 2 ** 14 == (out.double() * 2 ** 14).round()).all())


def test_split_is_the_kernels():
    """rb_split3 on a few hand values: truncation toward zero, exact residuals."""
    x = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -23, -255.0, -(1.0 + 2.0 ** -8)])
    h, m, l = X.split3(x)
    assert h.tolist() == [1.0 + 2.0 ** -7, -255.0, -1.0]
    assert m.tolist() == [2.0 ** -8, 0.0, -(2.0 ** -8)]
    assert l.tolist() == [2.0 ** -23, 0.0, 0.0]


def test_subset_sums_of_the_kept_products_are_fp32():
    """Whatever order (MFMA, K group, N half, wave) the kept products are added in, no partial sum rounds; g/S = +-2^k."""
    g = X.gen("spamat-subsets")
    names = [a + b for a in "hml" for b in "hml"]
    for wcls, vcls in X.PAIRINGS:
        d = torch.randint(0, 225, (10000,), generator=g)
        w = (d.double() - X.draw_out(wcls, d, g).double()).float()
        v = X.draw_view(vcls, (10000,), g)
        prods = {n: a.double() * b.double() for n, (a, b) in zip(names, itertools.product(X.split3(w), X.split3(v)))}
        kept = [prods[n] for n in X.KEPT]
        assert bool((sum(kept) == w.double() * v.double()).all()), "the kept products are the whole product"
        assert bool(_f32(w.double() * v.double()).all())
        for p in X.PINS[(wcls, vcls)]:
            assert bool((prods[p] != 0).all()), (wcls, vcls, p)
        for n in range(1, 8):
            for sub in itertools.combinations(kept, n):
                assert bool(_f32(sum(sub)).all()), (wcls, vcls, n)


def test_pins_name_every_product_but_lm():
    assert set(sum(X.PINS.values(), ())) == set(X.KEPT) - {"lm"}
    assert all(v == ("lm",) for v in X.NOT_PINNED.values())


# ------------------------------------------------------------------------------------------------------------------
# family 1
def test_flat_table_reaches_every_route():
    rowb = {X.rowb_of(*c[1:2], c[3], c[4]) for c in X.FLAT if c[7] == "rowb" and not c[6]}
    assert rowb == set(X.ROWB), sorted(set(X.ROWB) - rowb)
    for c in X.FLAT:
        if c[7] != "rowb":
            assert c[5] != "dense" or c[6] or X.rowb_of(c[1], c[3], c[4]) is None, c
    assert {c[7] for c in X.FLAT} == {"rowb", "sparse", "band", "rowtile", "wide"}
    assert {c[3] for c in X.FLAT} >= {641, 700, 701, 1024, 1025, 257, 300, 320}
    assert {c[4] for c in X.FLAT} >= {16, 33, 34, 81, 82, 161, 225, 162, 226, 274}
    assert {c[1] for c in X.FLAT} >= {5, 13, 20, 25, 72, 73}
    assert max(c[0] * c[1] * c[2] * c[3] for c in X.FLAT) == 2 * 24 * 2 * 1025


@pytest.mark.parametrize("row", X.FLAT, ids=X.FLAT_IDS)
def test_flat_cases_are_exact_from_their_magnitudes(row):
    """Every term of either gradient is a multiple of 1/16 and the sum of their magnitudes stays below 2^24 units: every
    partial sum is an fp32 number in any order.  Every cost is 0."""
    B, C, H, W, D, _, var, _ = row
    case = X.flat_case(row)
    assert X.flat_bound(D, var) < 2 ** 24
    assert not bool((case["L"] * case["R"]).any()) and float(case["L"].abs().max()) == 2 == float(case["R"].abs().max())
    assert bool(((case["L"] != 0).any(1) & (case["R"] != 0).any(1)).any())
    gs = case["g"] / case["S"]
    assert bool((gs * 4 == (gs * 4).round()).all()) and float(gs.abs().max()) <= 2
    if var:
        w = (torch.arange(D).view(-1, 1, 1, 1) - case["mu"]) ** 2 - case["out"]
        assert bool((w == w.round()).all()) and float(w.abs().max()) <= D * D + 2 * D
        assert bool((case["mu"] == case["mu"].round()).all())
    else:
        assert bool((case["out"] * 4 == (case["out"] * 4).round()).all())
        assert 0 <= float(case["out"].min()) and float(case["out"].max()) < D
    for k, t in X.reference(case).items():
        want = X.exact_or_fail(t, X.FLAT_UNIT)
        assert float(t.abs().max()) <= X.flat_bound(D, var) * X.FLAT_UNIT
        assert bool(want.any()), k


@pytest.mark.parametrize("i", [0, 3, 8, 14], ids=[X.FLAT_IDS[i] for i in (0, 3, 8, 14)])
def test_model_is_exact_on_flat_cases(i):
    case = X.flat_case(X.FLAT[i])
    ref = X.reference(case)
    gl, gr = X.emulate(case)
    assert torch.equal(gl, ref["gl"]) and torch.equal(gr, ref["gr"])
    gl, gr = X.emulate(case, X.Drop("gl", "hh", q=3, m=1))
    assert not torch.equal(gl, ref["gl"]) and torch.equal(gr, ref["gr"])
    if X.FLAT[i][4] > 64:                                             # |d - out| >= 64 in quarters: more than 8 bits
        _, gr = X.emulate(case, X.Drop("gr", "mh"))
        assert not torch.equal(gr, ref["gr"])


# ------------------------------------------------------------------------------------------------------------------
# family 2
SEL_PARAMS = [(row, p, run) for row in X.SEL for p in X.PAIRINGS for run in X.RUNS]
SEL_PARAM_IDS = ["%s-%sx%s-%s" % (X.SEL_IDS[X.SEL.index(r)], p[0], p[1], run) for r, p, run in SEL_PARAMS]


def _pinned(case):
    return "gl" if case["run"] == "left" else "gr"


def _restrictions(row, mat, prod):
    """Everywhere, and each K group that holds the product, each band tile and each channel block on its own."""
    nt, cb = X.rowb_of(row[0], row[2], row[3])
    return [{}] + [{"q": q} for q in X.groups(mat, prod)] + [{"m": m} for m in range(nt)] + [{"cb": b} for b in range(cb)]


@pytest.mark.parametrize("row,pairing,run", SEL_PARAMS, ids=SEL_PARAM_IDS)
def test_selector_model_is_exact_and_each_product_is_pinned(row, pairing, run):
    """The whole model equals the float64 reference (an fp32 number up to the e^-256 tail of the dead candidates) in the
    pinned gradient; without any one pinned product -- everywhere or in one K group, channel block or band tile -- at
    least one element differs after rounding to fp32; without a product this pairing does not pin, nothing changes."""
    case = X.selector_case(row, pairing, run)
    ref = X.reference(case)
    key = _pinned(case)
    want = {k: X.expect32(ref[k], X.TAIL) for k in X.exact_keys(run)}
    full = dict(zip(("gl", "gr"), X.emulate(case)))
    assert torch.equal(full[key].float() + 0.0, want[key])
    assert bool(_f32(full[key]).all())
    if run == "right":                                                # grad_ref is one product as well there
        assert torch.equal(full["gl"].float() + 0.0, want["gl"])
    # every expected element is one product: nonzero exactly at the live pixels' channels
    nz = want[key] != 0
    C, H, W, D, sel = row
    if run == "left":
        assert torch.equal(nz, case["live"][:, None].expand_as(nz))
    else:
        hit = torch.zeros_like(case["live"])
        b, y, xl = case["live"].nonzero(as_tuple=True)
        hit[b, y, xl - case["d"][b, y, xl]] = True
        assert torch.equal(nz, hit[:, None].expand_as(nz)) and int(hit.sum()) == int(case["live"].sum())
    drops = [X.Drop(key, prod, **rs) for prod in X.PINS[pairing] for rs in _restrictions(row, key, prod)]
    blind = [X.Drop(key, prod) for prod in sorted(set(X.KEPT) - set(X.PINS[pairing]))]
    res = X.emulate_many(case, drops + blind)
    for dr, got in zip(drops, res):
        assert not torch.equal(dict(zip(("gl", "gr"), got))[key].float() + 0.0, want[key]), dr
    for dr, got in zip(blind, res[len(drops):]):
        assert torch.equal(dict(zip(("gl", "gr"), got))[key].float() + 0.0, want[key]), dr


@pytest.mark.parametrize("row", X.SEL, ids=X.SEL_IDS)
def test_selector_cost_products(row):
    """The selector's cost is 1 x 1 or -255 x 1: hi x hi alone.  Without it every e is 2^(-log2 e) instead of 1 / 0 and
    the gradients change; the other cost products see zeros here (docs/rounds/spamat_exact.md: not pinned)."""
    case = X.selector_case(row, X.PAIRINGS[0], "left")
    want = X.expect32(X.reference(case)["gl"], X.TAIL)
    gl, _ = X.emulate(case, X.Drop("cost", "hh"))
    assert not torch.equal(gl.float() + 0.0, want)
    nt, cb = X.rowb_of(row[0], row[2], row[3])
    gl, _ = X.emulate(case, X.Drop("cost", "hh", cb=row[4] // 8, m=nt - 1))
    assert not torch.equal(gl.float() + 0.0, want)


def test_coverage_table(capsys):
    """Every role of every rowb instantiation receives a nonzero product in each run of each pairing (each role on its
    own: the marginals, not their joint tuples).  The channel roles come from the channels whose product is nonzero."""
    lines = ["instantiation case run      q r  j  i  m wave slot cb ch   d"]
    for row in X.SEL:
        need = X.required_roles(row)
        nt, cb = X.rowb_of(row[0], row[2], row[3])
        for pairing in X.PAIRINGS:
            for run in X.RUNS:
                got = X.selector_roles(row, X.selector_case(row, pairing, run))
                for k, v in need.items():
                    assert got[k] >= v, ("%s %s %s: role %s misses %s" % (row, pairing, run, k, sorted(v - got[k])))
                if run == "left" or row[3] <= 33:             # (wider bands: fewer selected pixels than disparities)
                    assert got["d"] == set(range(row[3])), (row, run, sorted(set(range(row[3])) - got["d"]))
                if pairing == X.PAIRINGS[0]:
                    lines.append("NT %2d CB %d   %-14s %-5s %2d %d %2d %2d %2d %4d %4d %2d %2d %3d" % (
                        nt, cb, X.SEL_IDS[X.SEL.index(row)], run, *(len(got[k]) for k in
                                                                     ("q", "r", "j", "i", "m", "wave", "slot", "cb", "ch", "d"))))
    assert {X.rowb_of(r[0], r[2], r[3]) for r in X.SEL} == set(X.ROWB)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_coverage_assertion_sees_a_gap():
    row = X.SEL[4]                                                    # C 16: two channel blocks
    case = X.selector_case(row, X.PAIRINGS[0], "left")
    case["live"] = case["live"] & (torch.arange(row[2]) % 16 != 5)
    assert 5 not in X.selector_roles(row, case)["j"]
    case["R"][:, 8:] = 0                                              # no product lands in the second channel block
    got = X.selector_roles(row, case)
    assert got["cb"] == {0} and got["ch"] == set(range(8))
    case["R"][:, 3] = 0
    assert 3 not in X.selector_roles(row, case)["ch"]


# ------------------------------------------------------------------------------------------------------------------
# family 3
COST_PARAMS = [(row, p) for row in X.COST for p in X.COST_PAIRINGS]
COST_PARAM_IDS = ["%s-%sx%s" % (X.COST_IDS[X.COST.index(r)], p[0], p[1]) for r, p in COST_PARAMS]


@pytest.mark.parametrize("row,pairing", COST_PARAMS, ids=COST_PARAM_IDS)
def test_cost_case_is_exact_and_each_cost_product_exceeds_the_bound(row, pairing):
    """The live cost 1 + R L is an fp32 number and no power of two, max_cost is imposed to it, the data channel reaches
    every channel block; the model is within the bound of the float64 reference, and without any one pinned cost product
    -- everywhere, in its K group, or in any one channel block -- some element is off by at least four bounds.  In another
    K group the drop is no drop; `lm` meets zeros (not pinned)."""
    C, H, W, D, sel = row
    nt, cb = X.rowb_of(C, W, D)
    case = X.cost_case(row, pairing)
    lv = case["live"]
    cost64 = (case["L"].double() * torch.gather(
        case["R"].double(), 3, (torch.arange(W) - case["d"]).clamp_min(0)[:, None].expand(1, C, H, W))).sum(1)
    mc = case["max_cost"]
    assert torch.equal(mc.double()[lv], cost64[lv]), "1 + R L is not an fp32 number"
    man, _ = torch.frexp(mc[lv])
    assert bool((man != 0.5).all()) and 0.25 <= float(mc[lv].min()) and float(mc[lv].max()) <= 2.75
    assert {c // 8 for c in case["dc"]} == set(range(cb)) and sel not in case["dc"]
    assert bool(X.PRED[pairing[0]](case["R"][0, case["dc"], range(H)]).all())
    for y in range(H):
        assert bool(X.PRED[pairing[1]](case["L"][0, case["dc"][y], y][lv[0, y]]).all())
    assert mc[lv].unique().numel() >= 8                              # (K2 x K2 has few pairs inside the cost window)
    ref = X.reference(case)["gl"][:, sel]
    assert X.cost_dev(X.cost_model(case), ref, case) <= 1.0
    worst = {}
    for prod in X.PINS[pairing]:
        q = X.COST_Q[prod]
        for rs in [{}, {"q": q}] + [{"cb": b} for b in range(cb)] + [{"q": q, "cb": b} for b in range(cb)]:
            dr = X.Drop("cost", prod, **rs)
            worst[dr] = X.cost_dev(X.cost_model(case, dr), ref, case)
            assert worst[dr] >= 4.0, (dr, worst[dr])
        assert torch.equal(X.cost_model(case, X.Drop("cost", prod, q=(q + 1) % 4)), X.cost_model(case))
    for prod in sorted(set(X.KEPT) - set(X.PINS[pairing])):
        assert torch.equal(X.cost_model(case, X.Drop("cost", prod)), X.cost_model(case)), prod
    assert set(sum((X.PINS[p] for p in X.COST_PAIRINGS), ())) == set(X.KEPT) - set(X.NOT_PINNED["cost"])


@pytest.mark.parametrize("i", [0, 4, 7])
def test_cost_model_is_the_whole_model(i):
    """cost_model (the live candidate alone) against emulate (every candidate), with and without a cost product."""
    row = X.COST[i]
    for pairing in X.COST_PAIRINGS:
        case = X.cost_case(row, pairing)
        for dr in (None, X.Drop("cost", X.PINS[pairing][-1]), X.Drop("cost", X.PINS[pairing][1], cb=case["dc"][1] // 8)):
            gl, _ = X.emulate(case, dr)
            assert torch.equal(gl[:, case["sel"]], X.cost_model(case, dr)), (row, pairing, dr)


def test_cost_bound_terms():
    """The bound is made of what the issue names and nothing else; the fma residual of the cases is far inside its term."""
    case = X.cost_case(X.COST[0], X.COST_PAIRINGS[0])
    b = X.cost_bound(case)
    assert torch.equal(b, (case["max_cost"].double() + 1) * 2.0 ** -24 + X.EXP_ACC)
    assert 0 <= X.EXP_ACC <= 2.0 ** -21


# ------------------------------------------------------------------------------------------------------------------
def test_dropped_product_is_invisible_to_the_gates():
    """Why these tests exist: on the suite's random data the backward without one term product passes both gates."""
    gate, full, errs = X.table_row(8, 700, 40, "relu")
    assert full < 0.05 * gate
    for e in errs[:3]:                                                # the contraction products
        assert 0.05 * gate < e < gate, (e, gate)
