"""The SpaMat / SpaVar backward on exact data (tests/_spamat_exact.py), bit for bit against the float64 reference of
tests/_spamat_ref.py: no tolerance.  The backward takes out, sum_similarities and max_cost as inputs, so they are imposed.
  family 1, flat dense: integer features with disjoint channel supports (every cost 0, every e 1), out a multiple of 1/4,
    g/S a multiple of 1/4: every partial sum of either gradient is an fp32 number in any order -- all ten instantiations of
    spamat_bwd_rowb, the sparse / mid rows, the band launch, the row-tile fallback, a wide case, and SpaVar (integer
    disparity and variance, grad_disparity included);
  family 2, selectors: one live candidate per left pixel, every gradient element ONE product g/S w view with (w, view)
    from the one-, two- and three-term classes of the kernel's truncating split: a term product of spamat_bwd_rowb that is
    dropped, doubled or read from the wrong term plane -- in one K group, channel block, band tile or ring slot -- changes
    a bit (tests/test_spamat_exact_cpu.py proves that on the host model).
  family 3, cost terms: the selector plus one data channel with a class pair on (R, L): the live cost is 1 + R L, exact but
    no power of two, and max_cost is imposed to it.  grad_ref's selector channel is g/S e (d - out): per element within
    X.cost_bound (fma residual, one product rounding, the accuracy of v_exp_f32) of the float64 reference; a dropped cost
    product -- everywhere, in its K group or in one channel block -- exceeds that bound fourfold (the CPU tests).  The same
    inputs through decnet_spamat_forward (C = 8: the bf16x3 dense route): max_cost is the exact cost bit for bit and the
    sum of similarities fl(1 + 1e-6f).
Every case goes through the C ABI with every buffer a guarded window, at both placements (bit-identical), and again under
both LDS poison words.  A -0 of the chip (0 x g/S carries the sign of g) counts as the reference's +0.  -m gpu."""
import types

import pytest
import torch

import _lds_poison
import _spamat_exact as X
from _placement import Place, _bits_equal, _L, _st

pytestmark = pytest.mark.gpu

WS_SPAMAT_BWD = 4                                                     # decnet_spamat_workspace_floats: `which`


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _dev():
    return torch.device("cuda:0")


def run_bwd(case, aligned, ws=False):
    """decnet_spamat_backward (decnet_spavar_backward where the case has a disparity; ws: the `_ws` entry on a guarded
    workspace of exactly the queried size) on guarded windows -> host gradients {"gl", "gr"[, "gd"]}."""
    dev = _dev()
    L = _L()
    P, pw = Place(dev, aligned), Place(dev, True)
    B, C, H, W = case["L"].shape
    dims = (B, C, H, W, case["D"])
    t = {k: P.inp(case[k]) for k in ("L", "R", "rm", "tm", "out", "S", "max_cost", "g")}
    o = {"gl": P.out((B, C, H, W)), "gr": P.out((B, C, H, W))}
    head = [t[k].data_ptr() for k in ("L", "R", "rm", "tm")]
    tail = [t[k].data_ptr() for k in ("out", "S", "max_cost", "g")] + [o["gl"].data_ptr(), o["gr"].data_ptr()]
    if "mu" in case:
        assert not ws
        o["gd"] = P.out((B, H, W))
        rc = L.decnet_spavar_backward(*head, P.inp(case["mu"]).data_ptr(), *tail, o["gd"].data_ptr(), *dims, _st())
    elif ws:
        n = int(L.decnet_spamat_workspace_floats(*dims, WS_SPAMAT_BWD))
        assert n > 0, "the case needs no workspace: it does not reach the banded sweep"
        win = pw.inplace(torch.full((n,), 12345.0))
        rc = L.decnet_spamat_backward_ws(*head, *tail, *dims, win.data_ptr(), n, _st())
    else:
        rc = L.decnet_spamat_backward(*head, *tail, *dims, _st())
    assert rc == 0, (dims, rc)
    P.check("%s aligned=%s" % (dims, aligned))
    pw.check("%s workspace" % (dims,))
    return {k: v.cpu() for k, v in o.items()}


def both(case, **kw):
    """Both placements (bit-identical), then both again under each LDS poison word -> the aligned results."""
    a = run_bwd(case, True, **kw)
    u = run_bwd(case, False, **kw)
    for k in a:
        assert _bits_equal(a[k], u[k]), "%s differs between aligned and unaligned placement" % k
    _lds_poison.hooks()
    _lds_poison.sweep(lambda aligned: run_bwd(case, aligned, **kw), a)
    return a


def assert_exact(got, want, what):
    """Bit for bit (the chip's -0 as +0); the message names the first differing element."""
    got = X.canon(got)
    if not _bits_equal(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ from float64; first at %s: got %r, want %r" % (
            what, bad.shape[0], want.numel(), i, float(got[i]), float(want[i])))


_FLAT = {}


def flat(i):
    """Case i of X.FLAT and its fp32 expectations (cached per process)."""
    if i not in _FLAT:
        case = X.flat_case(X.FLAT[i])
        _FLAT[i] = case, {k: X.exact_or_fail(t, X.FLAT_UNIT) for k, t in X.reference(case).items()}
    return _FLAT[i]


def via_function(case):
    """SpaMatFunction.backward on the imposed forward results (what autograd would have saved)."""
    from decnet_amd.modules.SparseMatching.functions.SpaMat import SpaMatFunction
    dev = _dev()
    ctx = types.SimpleNamespace(max_disp=case["D"], saved_tensors=tuple(
        case[k].to(dev) for k in ("L", "R", "rm", "tm", "out", "S", "max_cost")))
    gl, gr = SpaMatFunction.backward(ctx, case["g"].to(dev))[:2]
    return {"gl": gl.cpu(), "gr": gr.cpu()}


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(X.FLAT)), ids=X.FLAT_IDS)
def test_flat_dense_is_bit_exact(dev, i):
    case, want = flat(i)
    got = both(case)
    assert set(got) == set(want)
    for k in want:
        assert_exact(got[k], want[k], "%s %s" % (X.FLAT_IDS[i], k))


def test_flat_dense_through_the_ws_entry(dev):
    (i,) = [i for i, c in enumerate(X.FLAT) if c[7] == "wide"]
    case, want = flat(i)
    got = both(case, ws=True)
    for k in want:
        assert_exact(got[k], want[k], "%s %s (_ws)" % (X.FLAT_IDS[i], k))


def test_flat_dense_through_the_function(dev):
    i = max(range(len(X.FLAT)), key=lambda i: X.FLAT[i][0] * X.FLAT[i][1] * X.FLAT[i][3])      # B 2, H 2, C 24, W 1025
    case, want = flat(i)
    got = via_function(case)
    for k in want:
        assert_exact(got[k], want[k], "%s %s (SpaMatFunction.backward)" % (X.FLAT_IDS[i], k))


# ------------------------------------------------------------------------------------------------------------------
SEL_PARAMS = [(row, p, run) for row in X.SEL for p in X.PAIRINGS for run in X.RUNS]
SEL_PARAM_IDS = ["%s-%sx%s-%s" % (X.SEL_IDS[X.SEL.index(r)], p[0], p[1], run) for r, p, run in SEL_PARAMS]


def selector(row, pairing, run):
    case = X.selector_case(row, pairing, run)
    ref = X.reference(case)
    return case, {k: X.expect32(ref[k], X.TAIL) for k in X.exact_keys(run)}


@pytest.mark.parametrize("row,pairing,run", SEL_PARAMS, ids=SEL_PARAM_IDS)
def test_selector_products_are_bit_exact(dev, row, pairing, run):
    """left run: every grad_ref element is one product g/S w R; right run: every grad_tar element one product g/S w L (and
    grad_ref's selector channel g/S w).  The left run's grad_tar is a sum of D three-term numbers: not judged here."""
    case, want = selector(row, pairing, run)
    got = both(case)
    for k in want:
        assert_exact(got[k], want[k], "%s %s x %s %s run %s" % (row, *pairing, run, k))


@pytest.mark.parametrize("run", X.RUNS)
def test_selector_products_through_the_function(dev, run):
    row, pairing = X.SEL[6], X.PAIRINGS[2]                           # NT 11, CB 2; (K2, K2)
    case, want = selector(row, pairing, run)
    got = via_function(case)
    for k in want:
        assert_exact(got[k], want[k], "%s %s (SpaMatFunction.backward)" % (row, k))


# ------------------------------------------------------------------------------------------------------------------
COST_PARAMS = [(row, p) for row in X.COST for p in X.COST_PAIRINGS]
COST_PARAM_IDS = ["%s-%sx%s" % (X.COST_IDS[X.COST.index(r)], p[0], p[1]) for r, p in COST_PARAMS]
_COST = {}


def cost(row, pairing):
    """The case and the float64 reference of grad_ref's selector channel (cached per process)."""
    if (row, pairing) not in _COST:
        case = X.cost_case(row, pairing)
        _COST[row, pairing] = case, X.reference(case)["gl"][:, case["sel"]]
    return _COST[row, pairing]


@pytest.mark.parametrize("row,pairing", COST_PARAMS, ids=COST_PARAM_IDS)
def test_cost_products_within_the_per_element_bound(dev, row, pairing):
    """Worst |got - float64| / |float64| over the live pixels, in units of X.cost_bound (and absolute, for
    docs/rounds/spamat_exact.md), printed before it is judged."""
    case, ref = cost(row, pairing)
    got = both(case)["gl"][:, case["sel"]]
    lv = case["live"]
    rel = float(((got.double() - ref)[lv].abs() / ref[lv].abs()).max())
    dev_ = X.cost_dev(got, ref, case)
    print("\ncost %s %s x %s: worst relative deviation %.3e = %.3f of the bound" % (row, *pairing, rel, dev_))
    assert bool(torch.isfinite(got).all())
    assert dev_ <= 1.0, (row, pairing, rel, dev_)
    assert not bool(got[~lv].any()), "a pixel without a live candidate got a gradient in the selector channel"


def run_fwd(case, aligned):
    """decnet_spamat_forward on guarded windows -> host {"out", "S", "max_cost"}."""
    dev = _dev()
    L = _L()
    P = Place(dev, aligned)
    B, C, H, W = case["L"].shape
    t = [P.inp(case[k]).data_ptr() for k in ("L", "R", "rm", "tm")]
    o = {k: P.out((B, H, W)) for k in ("out", "S", "max_cost")}
    rc = L.decnet_spamat_forward(*t, *(o[k].data_ptr() for k in ("out", "S", "max_cost")), B, C, H, W, case["D"], _st())
    assert rc == 0, rc
    P.check("forward %s aligned=%s" % ((B, C, H, W, case["D"]), aligned))
    return {k: v.cpu() for k, v in o.items()}


FWD_PARAMS = [(r, p) for r, p in COST_PARAMS if r[0] == 8]
FWD_PARAM_IDS = [i for i, (r, p) in zip(COST_PARAM_IDS, COST_PARAMS) if r[0] == 8]


@pytest.mark.parametrize("row,pairing", FWD_PARAMS, ids=FWD_PARAM_IDS)
def test_cost_products_through_the_forward(dev, row, pairing):
    """The forward's dense rows at C = 8 form the cost as bf16x3 without lo x lo: at every left pixel with a live candidate
    max_cost is the exact cost 1 + R L bit for bit, and the sum of similarities is fl(1 + 1e-6f): one e of exactly 1."""
    case, _ = cost(row, pairing)
    a = run_fwd(case, True)
    u = run_fwd(case, False)
    for k in a:
        assert _bits_equal(a[k], u[k]), "%s differs between aligned and unaligned placement" % k
    _lds_poison.hooks()
    _lds_poison.sweep(lambda aligned: run_fwd(case, aligned), a)
    lv = case["live"]
    assert_exact(a["max_cost"][lv], case["max_cost"][lv], "%s %s x %s max_cost" % (row, *pairing))
    one = (torch.tensor(1.0) + torch.tensor(1e-6)).expand(int(lv.sum())).contiguous()
    assert_exact(a["S"][lv], one, "%s %s x %s sum_similarities" % (row, *pairing))
