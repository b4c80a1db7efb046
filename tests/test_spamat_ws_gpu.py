"""The caller-workspace SpaMat / SpaVar entries (`decnet_*_ws`, include/decnet_hip.h) on the GPU, for disparity ranges
wider than one band of the matrix-core kernels (max_disp > 273: csrc/spamat_wide.hip).

The yardstick is bit-identity: a `_ws` entry called eagerly returns exactly what the legacy entry returns eagerly (same band
kernels, band split and merge order, no floating-point atomics), and a HIP-graph replay of a `_ws` entry returns exactly
what the eager `_ws` call returns -- the legacy entries decline under capture (the bit-mask entry with -3, the float-mask
entries by running the row-tile kernels).  On top of that the same cases are held against the float64 references of
tests/_spamat_ref.py under the bounds of tests/test_spamat_edges_gpu.py (imported, not restated).

Every workspace is a window of exactly the queried size inside a sentinel-filled buffer (tests/_placement.py); rejected
calls must leave the outputs' NaN pre-fill alone.  The surface tests go through decnet_amd.ops (which allocates the
workspace with torch.empty), the autograd Functions under decnet_amd.graphs.GraphedStep, the model's captured forward and
the compiled drop-in modules.  -m gpu."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, "golden"), HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _lds_poison                                                      # noqa: E402
import test_spamat_edges_gpu as E                                        # noqa: E402
from _placement import ERR_MISALIGNED, ERR_UNSUPPORTED, SENT, Place, _bits_equal, _L, _st   # noqa: E402

pytestmark = pytest.mark.gpu

WHICH = {"m": 0, "v": 1, "f": 2, "b": 3, "mb": 4, "vb": 5}             # entry -> `which` of decnet_spamat_workspace_floats
OUT_KEYS = {"m": ("m_out", "m_S", "m_max"), "v": ("v_var", "v_S", "v_max"), "f": ("f_out", "f_var", "f_S", "f_max"),
            "b": ("b_out", "b_var", "b_S", "b_max"), "mb": ("m_gl", "m_gr"), "vb": ("v_gl", "v_gr", "v_gd")}
FEAT_KEYS = ("m_gl", "m_gr", "v_gl", "v_gr")
ALL_KEYS = E.FWD_KEYS + E.BITS_KEYS + E.GRAD_KEYS

# (B, C, H, W, D, masks, feats, disparity, P) as in tests/test_spamat_edges_gpu.py: D in {274, 405, 621} (2, 2 and 3
# bands), mask densities 1.0 / 0.5 / 0.1, C in {8, 24}, W < D, B = 2; row lengths of every residue mod 4, so that the
# staging kernels' 16-byte middle, scalar head and tail and every source alignment are exercised
CASES = [
    (1, 8, 2, 460, 274, "dense", "relu", "near", 0),
    (1, 8, 2, 461, 405, ("p", 0.5, 0.5), "relu", "near", 0),
    (2, 8, 2, 702, 621, ("p", 0.5, 0.5), "relu", "near", 0),
    (1, 24, 3, 303, 405, ("p", 0.1, 0.1), "relu", "near", 0),            # W < D: bands of (partly) empty candidates
    (1, 24, 1, 645, 621, "dense", "signed", "above", 0),
    (2, 8, 3, 333, 274, ("p", 0.1, 0.1), "relu", "neg", 0),
    (1, 8, 1, 3, 405, "dense", "relu", "near", 0),                       # a row shorter than one 16-byte vector
]
IDS = ["%d-B%dC%dH%dW%dD%d" % ((i,) + c[:5]) for i, c in enumerate(CASES)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _dev():
    return torch.device("cuda:0")


def query(dims):
    """{entry: decnet_spamat_workspace_floats} -- the symbol is looked up, so a library without it fails here."""
    q = _L().decnet_spamat_workspace_floats
    return {k: int(q(*dims, w)) for k, w in WHICH.items()}


def calls(t, fw, o, dims, st, ws=None, only=None):
    """The six entries on inputs t, forward results fw and outputs o (dicts of device tensors) -> {entry: rc}.
    ws None: the legacy entries; else {entry: (workspace pointer or None, workspace_floats)}: the `_ws` entries."""
    L = _L()
    p = lambda k: o[k].data_ptr()                                         # noqa: E731
    lr = (t["L"].data_ptr(), t["R"].data_ptr())
    mk = (t["rm"].data_ptr(), t["tm"].data_ptr())
    args = {
        "m": ("decnet_spamat_forward", (*lr, *mk, p("m_out"), p("m_S"), p("m_max"))),
        "v": ("decnet_spavar_forward", (*lr, *mk, t["mu"].data_ptr(), p("v_var"), p("v_S"), p("v_max"))),
        "f": ("decnet_spamatvar_forward", (*lr, *mk, p("f_out"), p("f_var"), p("f_S"), p("f_max"))),
        "b": ("decnet_spamatvar_forward_bits", (*lr, t["rbits"].data_ptr(), t["tbits"].data_ptr(), p("b_out"), p("b_var"),
                                                p("b_S"), p("b_max"))),
        "mb": ("decnet_spamat_backward", (*lr, *mk, fw["out"].data_ptr(), fw["S"].data_ptr(), fw["max_cost"].data_ptr(),
                                          t["g"].data_ptr(), p("m_gl"), p("m_gr"))),
        "vb": ("decnet_spavar_backward", (*lr, *mk, t["mu"].data_ptr(), fw["var"].data_ptr(), fw["S"].data_ptr(),
                                          fw["max_cost"].data_ptr(), t["g"].data_ptr(), p("v_gl"), p("v_gr"), p("v_gd"))),
    }
    rc = {}
    for k, (name, a) in args.items():
        if only is not None and k not in only:
            continue
        if ws is None:
            rc[k] = getattr(L, name)(*a, *dims, st)
        else:
            rc[k] = getattr(L, name + "_ws")(*a, *dims, ws[k][0], ws[k][1], st)
    return rc


def want_rc(C):
    return {"m": 0, "v": 0, "f": 0, "b": E.expect_bits_rc(), "mb": E.expect_bwd_rc(C), "vb": E.expect_bwd_rc(C)}


def run_ws(case, aligned=True):
    """All six `_ws` entries on one case, every buffer a guarded window (tensors at `aligned` placement, the workspaces --
    exactly the queried size -- always 16-byte aligned) -> (host results, {entry: workspace window})."""
    B, C, H, W, D = case[:5]
    x = E.inputs_of(case)
    dev = _dev()
    P, rej, pb, pw = Place(dev, aligned), Place(dev, True), Place(dev, False), Place(dev, True)
    t = {k: P.inp(x[k]) for k in ("L", "R", "rm", "tm", "g", "mu")}
    t["rbits"], t["tbits"] = pb.inp(x["rbits"]), pb.inp(x["tbits"])
    fw = {k: P.inp(x["m32"][k]) for k in ("out", "S", "max_cost", "var")}
    want = want_rc(C)
    o = {}
    for e, keys in OUT_KEYS.items():
        for k in keys:
            o[k] = (P if want[e] == 0 else rej).out((B, C, H, W) if k in FEAT_KEYS else (B, H, W))
    dims = (B, C, H, W, D)
    n = query(dims)
    assert all(v > 0 for v in n.values()) if D > 273 else not any(n.values()), n
    win = {k: pw.inplace(torch.full((v,), SENT)) for k, v in n.items() if v}
    ws = {k: (win[k].data_ptr() if v else None, v) for k, v in n.items()}
    rc = calls(t, fw, o, dims, _st(), ws)
    assert rc == want, (case[:5], rc)
    what = "%s _ws aligned=%s" % (case[:5], aligned)
    P.check(what)
    pb.check(what + " bits")
    pw.check(what + " workspace")                                          # nothing outside workspace[0 .. query)
    rej.check_untouched(what + " rejected call")
    skip = sum((OUT_KEYS[e] for e in want if want[e]), ())
    return {k: v.cpu() for k, v in o.items() if k not in skip}, win


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ws_entries_equal_the_legacy_entries_bit_for_bit(dev, case):
    """Eager: each `_ws` entry == its legacy entry as int32 bit patterns (outputs pre-filled with NaN, guarded
    workspaces), at both placements of the tensors; and the float64 bounds of the edge tests hold."""
    legacy = E.run(case, None)
    got, _ = run_ws(case, True)
    assert set(got) == set(legacy)
    for k in legacy:
        assert _bits_equal(got[k], legacy[k]), "%s: %s of the _ws entry differs from the legacy entry" % (case[:5], k)
    un, _ = run_ws(case, False)
    for k in legacy:
        assert _bits_equal(un[k], legacy[k]), "%s: %s differs with the tensors at an odd float offset" % (case[:5], k)
    E.check_values(case, got)


# one wide case per route: dense rows in 2 bands; half-dense rows (the compacted kernels) in 3 bands, B = 2; sparse rows
# with C = 24 and W < D (bands of empty candidates)
@pytest.mark.parametrize("i", [0, 2, 3], ids=[IDS[0], IDS[2], IDS[3]])
def test_ws_entries_do_not_depend_on_what_lds_held(dev, i):
    """The forward and backward `_ws` entries with LDS poisoned before each (tests/_lds_poison.py), at both placements and
    under each pattern: bit-identical to the unpoisoned aligned run."""
    base, _ = run_ws(CASES[i], True)
    _lds_poison.sweep(lambda aligned: run_ws(CASES[i], aligned)[0], base)


def test_query_zero_means_the_existing_entry(dev):
    """max_disp 273 (still one band): the query is 0, the `_ws` entries take workspace == NULL and are the legacy entries."""
    case = (1, 8, 2, 460, 273, ("p", 0.8, 0.8), "relu", "near", 0)
    legacy = E.run(case, None)
    got, win = run_ws(case, True)
    assert not win
    for k in legacy:
        assert _bits_equal(got[k], legacy[k]), k


@pytest.mark.parametrize("D", [274, 405])
def test_rejected_workspace_launches_nothing(dev, D):
    """query > 0: no workspace -> -1, a short one -> -2, a misaligned one -> -5; the outputs keep their NaN pre-fill and
    the workspace its sentinel."""
    B, C, H, W = 1, 8, 2, 460
    case = (B, C, H, W, D, ("p", 0.8, 0.8), "relu", "near", 0)
    x = E.inputs_of(case)
    P, rej, pw, pu = Place(dev, True), Place(dev, True), Place(dev, True), Place(dev, False)
    t = {k: P.inp(x[k]) for k in ("L", "R", "rm", "tm", "g", "mu", "rbits", "tbits")}
    fw = {k: P.inp(x["m32"][k]) for k in ("out", "S", "max_cost", "var")}
    o = {k: rej.out((B, C, H, W) if k in FEAT_KEYS else (B, H, W)) for k in ALL_KEYS}
    dims = (B, C, H, W, D)
    n = query(dims)
    assert all(v > 0 for v in n.values()), n
    good = {k: pw.inplace(torch.full((v,), SENT)) for k, v in n.items()}
    odd = {k: pu.inplace(torch.full((v,), SENT)) for k, v in n.items()}
    st = _st()
    assert calls(t, fw, o, dims, st, {k: (None, n[k]) for k in n}) == dict.fromkeys(n, -1)
    assert calls(t, fw, o, dims, st, {k: (good[k].data_ptr(), n[k] - 1) for k in n}) == dict.fromkeys(n, -2)
    assert calls(t, fw, o, dims, st, {k: (good[k].data_ptr(), 0) for k in n}) == dict.fromkeys(n, -2)
    assert calls(t, fw, o, dims, st, {k: (odd[k].data_ptr(), n[k]) for k in n}) == dict.fromkeys(n, ERR_MISALIGNED)
    rej.check_untouched("rejected _ws calls")
    P.check("rejected _ws calls: inputs")
    for k in n:
        assert bool((good[k] == SENT).all()) and bool((odd[k] == SENT).all()), "a rejected call wrote its workspace"
    pw.check("workspace margins")
    pu.check("workspace margins")


# ------------------------------------------------------------------------------------------------------------------
def _device_inputs(case, dev):
    x = E.inputs_of(case)
    t = {k: x[k].to(dev) for k in ("L", "R", "rm", "tm", "g", "mu", "rbits", "tbits")}
    fw = {k: x["m32"][k].to(dev) for k in ("out", "S", "max_cost", "var")}
    return t, fw


def _nan_outs(dims, dev):
    B, C, H, W = dims[:4]
    return {k: torch.full((B, C, H, W) if k in FEAT_KEYS else (B, H, W), float("nan"), device=dev) for k in ALL_KEYS}


def capture_ws(D, dev, pinned_ok=True):
    """The six `_ws` calls at max_disp D: eager, captured into one graph on one stream, replayed; then the inputs are
    changed in place and the graph is replayed again.  Returns nothing; asserts bit-identity throughout."""
    B, C, H, W = 1, 8, 2, 460 if D < 600 else 702
    case = (B, C, H, W, D, ("p", 0.8, 0.8), "relu", "near", 0)
    other = (B, C, H, W, D, ("p", 0.6, 0.7), "signed", "near", 0)       # same shape, other values
    dims = (B, C, H, W, D)
    t, fw = _device_inputs(case, dev)
    n = query(dims)
    assert all(v > 0 for v in n.values()), n
    pw = Place(dev, True)
    win = {k: pw.inplace(torch.full((v,), SENT)) for k, v in n.items()}
    ws = {k: (win[k].data_ptr(), n[k]) for k in n}
    want = want_rc(C)
    assert want["b"] == 0 or E.PINNED == "rowtile"

    def eager():
        o = _nan_outs(dims, dev)
        rc = calls(t, fw, o, dims, _st(), ws)
        assert rc == want, rc
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in o.items()}
    first = eager()                                      # (also loads every code object before the capture)
    o = _nan_outs(dims, dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = calls(t, fw, o, dims, _st(), ws)
    assert rc == want, "under capture: %s" % rc            # the bit-mask entry included
    graph.replay()
    torch.cuda.synchronize()
    skip = sum((OUT_KEYS[e] for e in want if want[e]), ())
    for k in ALL_KEYS:
        if k not in skip:
            assert _bits_equal(o[k], first[k]), "D=%d: replayed %s differs from the eager _ws call" % (D, k)
    E.check_values(case, {k: v.cpu() for k, v in o.items() if k not in skip})
    # new values in the same storage
    t2, fw2 = _device_inputs(other, dev)
    for k in t:
        t[k].copy_(t2[k])
    for k in fw:
        fw[k].copy_(fw2[k])
    for v in o.values():
        v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    for k in ALL_KEYS:
        if k not in skip:
            assert _bits_equal(o[k], second[k]), "D=%d: %s of the replay on new inputs differs from an eager call" % (D, k)
            assert not _bits_equal(o[k], first[k]), "D=%d: %s did not follow the new inputs" % (D, k)
    pw.check("capture workspaces")


@pytest.mark.parametrize("D", [274, 405, 621])
def test_ws_entries_capture_and_replay_bit_identical(dev, D):
    capture_ws(D, dev)


# ------------------------------------------------------------------------------------------------------------------
# the Python surface
def _step_inputs(dev, D, seed):
    B, C, H, W = 1, 8, 3, 461
    g = torch.Generator().manual_seed(seed)
    L = torch.relu(torch.randn(B, C, H, W, generator=g)).to(dev)
    R = torch.relu(torch.randn(B, C, H, W, generator=g)).to(dev)
    rm = (torch.rand(B, H, W, generator=g) < 0.6).float().to(dev)
    tm = (torch.rand(B, H, W, generator=g) < 0.6).float().to(dev)
    go = torch.randn(B, H, W, generator=g).to(dev)
    mu = (D * torch.rand(B, H, W, generator=g)).to(dev)
    return L, R, rm, tm, go, mu


@pytest.mark.parametrize("which", ["SpaMat", "SpaVar"])
def test_graphed_step_at_wide_disparity_equals_an_eager_step(dev, which):
    """decnet_amd.graphs.GraphedStep around the autograd Function, forward + backward at max_disp 405: the replayed .grad
    tensors equal an eager step's bit for bit (under capture the legacy entries ran the row-tile kernels instead)."""
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    D = 405
    L, R, rm, tm, go, mu = _step_inputs(dev, D, 11)
    L.requires_grad_()
    R.requires_grad_()
    mu.requires_grad_(which == "SpaVar")
    leaves = [L, R] + ([mu] if which == "SpaVar" else [])

    def fn(a, b, c):
        if which == "SpaMat":
            return decnet_amd.SpaMatFunction.apply(a, b, rm, tm, D)
        return decnet_amd.SpaVarFunction.apply(a, b, rm, tm, c, D)

    step = GraphedStep(lambda: fn(L, R, mu).backward(go), grads_of=leaves)
    with torch.no_grad():                                 # new values, same storage
        L.mul_(0.75)
        R.add_(0.1)
    step()
    torch.cuda.synchronize()
    got = [t.grad.clone() for t in leaves]
    fresh = [t.detach().clone().requires_grad_() for t in leaves] + ([] if which == "SpaVar" else [mu])
    fn(*fresh).backward(go)
    torch.cuda.synchronize()
    for a, b in zip(got, fresh):
        assert b.grad is not None and _bits_equal(a, b.grad), "%s: a replayed gradient differs from the eager step's" % which
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


def test_spamatvar_forward_bits_runs_inside_a_capture(dev):
    """decnet_amd.spamatvar_forward_bits at max_disp 405 while the stream is being captured: no DecnetHipError, and the
    replay equals the eager call and the float-mask call bit for bit."""
    import decnet_amd
    D = 405
    L, R, rm, tm, _, _ = _step_inputs(dev, D, 12)
    rb, tb = E.pack_bits(rm.cpu()).to(dev), E.pack_bits(tm.cpu()).to(dev)
    want = [v.clone() for v in decnet_amd.spamatvar_forward_bits(L, R, rb, tb, D)]
    flt = decnet_amd.spamatvar_forward(L, R, rm, tm, D)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = decnet_amd.spamatvar_forward_bits(L, R, rb, tb, D)
    graph.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(out, want, flt):
        assert _bits_equal(a, b) and _bits_equal(a, c)


def _ops_all(t, fw, dims, dev):
    """The six wrappers of decnet_amd.ops on NaN-filled outputs -> dict of outputs."""
    from decnet_amd import ops
    D = dims[4]
    o = _nan_outs(dims, dev)
    ops.spamat_forward(t["L"], t["R"], t["rm"], t["tm"], o["m_out"], o["m_S"], o["m_max"], D)
    ops.spavar_forward(t["L"], t["R"], t["rm"], t["tm"], t["mu"], o["v_var"], o["v_S"], o["v_max"], D)
    ops.spamatvar_forward(t["L"], t["R"], t["rm"], t["tm"], D, out=(o["f_out"], o["f_var"], o["f_S"], o["f_max"]))
    ops.spamatvar_forward_bits(t["L"], t["R"], t["rbits"], t["tbits"], D, out=(o["b_out"], o["b_var"], o["b_S"], o["b_max"]))
    ops.spamat_backward(t["L"], t["R"], t["rm"], t["tm"], fw["out"], fw["S"], fw["max_cost"], t["g"], o["m_gl"], o["m_gr"], D)
    ops.spavar_backward(t["L"], t["R"], t["rm"], t["tm"], t["mu"], fw["var"], fw["S"], fw["max_cost"], t["g"], o["v_gl"],
                        o["v_gr"], o["v_gd"], D)
    return o


def child_mfma():
    """DECNET_SPAMAT_KERNEL=mfma (no row-tile fallback): through decnet_amd.ops the six calls at max_disp 405 and 621 are
    captured and replay bit-identical to the eager calls; through the legacy entries the capture is UNSUPPORTED."""
    assert os.environ.get("DECNET_SPAMAT_KERNEL") == "mfma"
    dev = _dev()
    for D in (405, 621):
        B, C, H, W = 1, 8, 2, 460 if D < 600 else 702
        dims = (B, C, H, W, D)
        t, fw = _device_inputs((B, C, H, W, D, ("p", 0.8, 0.8), "relu", "near", 0), dev)
        eager = _ops_all(t, fw, dims, dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o = _ops_all(t, fw, dims, dev)
            legacy_rc = calls(t, fw, _nan_outs(dims, dev), dims, _st())
        assert legacy_rc == dict.fromkeys(WHICH, ERR_UNSUPPORTED), legacy_rc
        graph.replay()
        torch.cuda.synchronize()
        for k in ALL_KEYS:
            assert not bool(torch.isnan(o[k]).any()), k
            assert _bits_equal(o[k], eager[k]), "D=%d %s" % (D, k)
    print("CHILD-OK")


def child_rowtile():
    """DECNET_SPAMAT_KERNEL=rowtile: the `_ws` entries check the workspace and then do not use it -- the row-tile
    results of the legacy entries, bit for bit, and every workspace window still holds its sentinel."""
    assert os.environ.get("DECNET_SPAMAT_KERNEL") == "rowtile" and E.PINNED == "rowtile"
    case = (1, 8, 2, 460, 405, ("p", 0.8, 0.8), "relu", "near", 0)
    legacy = E.run(case, None)
    got, win = run_ws(case, True)
    assert "b_out" not in got and set(got) == set(legacy)              # the bit-mask entry: -3, as the legacy one
    for k in legacy:
        assert _bits_equal(got[k], legacy[k]), k
    assert len(win) == 6
    for k, w in win.items():
        assert bool((w == SENT).all()), "the %s entry wrote its workspace under rowtile" % k
    E.check_values(case, got)
    print("CHILD-OK")


@pytest.mark.parametrize("pin", ["mfma", "rowtile"])
def test_pinned_kernels_in_a_child_process(pin):
    code = "import sys; sys.path[:0] = %r\nimport test_spamat_ws_gpu as T\nT.child_%s()\n" % (
        [HERE, os.path.dirname(HERE)], pin)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DECNET_SPAMAT_KERNEL=pin),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------------------
def test_model_forward_captured_at_stage3_max_disp_405(dev):
    """SparseDenseNetRefinementMask with max_disp 405 (stage 3 at 405, above one band), forward captured the way bench.py
    captures its `e2e` leg: the bit-mask entry serves stage 3 inside the capture (no UNSUPPORTED, no float-mask fallback),
    and stage 3's disparity and variance planes after a replay equal those of an eager forward bit for bit."""
    from make_golden import E2E_KW
    import decnet_amd.model as M
    torch.manual_seed(5)
    model = M.get_model(**dict(E2E_KW, max_disp=405)).to(dev).eval()
    g = torch.Generator().manual_seed(99)
    left, right = torch.randn(1, 3, 54, 486, generator=g).to(dev), torch.randn(1, 3, 54, 486, generator=g).to(dev)
    seen = []                                              # (entry, D, outcome, (disparity, variance))
    orig_b, orig_f = M.spamatvar_forward_bits, M.spamatvar_forward

    def count_b(L, R, lb, rb, D, out=None):
        try:
            res = orig_b(L, R, lb, rb, D, out=out)
        except M.DecnetHipError as e:
            seen.append(("bits", int(D), e.code, None))
            raise
        seen.append(("bits", int(D), 0, (res[0], res[1])))
        return res

    def count_f(L, R, lm, rm, D, out=None):
        res = orig_f(L, R, lm, rm, D, out=out)
        seen.append(("float", int(D), 0, (res[0], res[1])))
        return res

    def stage3():
        hit = [s for s in seen if s[1] == 405]
        assert [s[:3] for s in hit] == [("bits", 405, 0)], [s[:3] for s in seen]
        return hit[0][3]
    M.spamatvar_forward_bits, M.spamatvar_forward = count_b, count_f
    try:
        with torch.no_grad():
            want_out = model(left, right)[-1].clone()
            torch.cuda.synchronize()
            want = [v.clone() for v in stage3()]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model(left, right)
            torch.cuda.current_stream().wait_stream(side)
            del seen[:]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model(left, right)[-1]
            got = stage3()                                   # the bit-mask entry, once, rc 0, inside the capture
            assert sorted(s[1] for s in seen) == [45, 135, 405] and all(s[0] == "bits" and s[2] == 0 for s in seen), \
                [s[:3] for s in seen]
            for _ in range(2):
                graph.replay()
            torch.cuda.synchronize()
            assert _bits_equal(got[0], want[0]), "stage-3 disparity of the replay differs from the eager forward"
            assert _bits_equal(got[1], want[1]), "stage-3 variance of the replay differs from the eager forward"
            assert torch.equal(out, want_out)
            assert float(want[0].abs().max()) > 0
    finally:
        M.spamatvar_forward_bits, M.spamatvar_forward = orig_b, orig_f


# ------------------------------------------------------------------------------------------------------------------
def test_compiled_modules_equal_ops_at_wide_disparity(dev):
    """The compiled drop-in modules (csrc/pybind) at max_disp 405, eager == decnet_amd.ops bit for bit, and capturable."""
    from test_pybind_ext import load
    from decnet_amd import ops
    sm, sv = load("SpaMat"), load("SpaVar")
    D = 405
    L, R, rm, tm, go, mu = _step_inputs(dev, D, 13)

    def through(fwd, bwd, vfwd, vbwd):
        o, s, m = (torch.full_like(rm, float("nan")) for _ in range(3))
        fwd(L, R, rm, tm, o, s, m, D)
        gl, gr = torch.full_like(L, float("nan")), torch.full_like(R, float("nan"))
        bwd(L, R, rm, tm, o, s, m, go, gl, gr, D)
        v, vs, vm = (torch.full_like(rm, float("nan")) for _ in range(3))
        vfwd(L, R, rm, tm, mu, v, vs, vm, D)
        vgl, vgr, vgd = torch.full_like(L, float("nan")), torch.full_like(R, float("nan")), torch.full_like(rm, float("nan"))
        vbwd(L, R, rm, tm, mu, v, vs, vm, go, vgl, vgr, vgd, D)
        return [o, s, m, gl, gr, v, vs, vm, vgl, vgr, vgd]
    compiled = (sm.sparse_matching_cuda_forward, sm.sparse_matching_cuda_backward, sv.sparse_var_cuda_forward,
                sv.sparse_var_cuda_backward)
    a = through(*compiled)
    b = through(ops.spamat_forward, ops.spamat_backward, ops.spavar_forward, ops.spavar_backward)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert not bool(torch.isnan(x).any()) and _bits_equal(x, y)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = through(*compiled)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(c, b):
        assert _bits_equal(x, y)
