"""Training-mode BatchNorm under hip_grad() on the GPU (csrc/batchnorm.hip, conv2d_grad.BatchNormActFunction,
Unit._forward_grad_train) against the float64 restatement of tests/_bn_train_ref.py:
  1. decnet_bn_train_forward / _backward through the C ABI at the edge shapes, at both placements and under both LDS poison
     words (tests/_placement._both), every bound counted from roundings (u = 2^-24; see _bn_train_ref.check_entry);
  2. the recomputed ReLU decision, bit-identical repeats and graph replays, refusals that launch nothing;
  3. single Units in .train() mode, one per route: autograd graph, tally, forward, gradients, running statistics, caches;
  4. Refinement and SoftAttention.fuse in .train() mode: gradients and buffers against the float64 CPU run, a second
     backward, and the refinement step as a GraphedStep replayed on new inputs.
-m gpu."""
import copy

import pytest
import torch

import _bn_train_ref as BR
import _model_cases as MC
from _placement import ERR_MISALIGNED, Place, _L, _bits_equal, _both, _st

pytestmark = pytest.mark.gpu
ERR_NULL, ERR_SHAPE = -1, -2
U = BR.U32
SEG = 4096
EPS, MOM = 1e-5, 0.1
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 7), (1, 8, 16, 18), (1, 2, 1, SEG), (3, 5, 1, SEG + 1), (5, 1, 1, 60 * SEG + 3)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from decnet_amd import ops2d
    assert ops2d.BN_SEGMENT == SEG
    return torch.device("cuda:0")


# ---- 1. the entries -----------------------------------------------------------------------------------------------------------
def _ws(L, dev, shape):
    n = L.decnet_bn_train_workspace_floats(*shape)
    B, C, H, W = shape
    assert n == 2 * (2 * C * B * -(-H * W // SEG) + 2 * C), (shape, n)
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n        # torch allocations: 16-byte aligned


def _run_entry(shape, first_kind, relu, ones=False, want_gz=True, aligned=True):
    """Forward, then backward on the forward's stats, through the C ABI -> the results on the CPU."""
    L, dev = _L(), torch.device("cuda:0")
    d = BR.entry_data(shape, first_kind, relu)
    gy = torch.ones(shape) if ones else d["gy"]
    C = shape[1]
    P = Place(dev, aligned)
    z, gyd, gamma, beta = P.inp(d["z"]), P.inp(gy), P.inp(d["gamma"]), P.inp(d["beta"])
    rm, rv = P.inplace(d["running_mean"]), P.inplace(d["running_var"])
    stats, y = P.out((2 * C,), torch.float64), P.out(shape)
    gz = P.out(shape) if want_gz else None
    dg, db = P.out((C,)), P.out((C,))
    ws, nws = _ws(L, dev, shape)
    rc = L.decnet_bn_train_forward(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOM, rm.data_ptr(), rv.data_ptr(),
                                   stats.data_ptr(), y.data_ptr(), int(relu), ws.data_ptr(), nws, *shape, _st())
    assert rc == 0, rc
    ws2, _ = _ws(L, dev, shape)                                 # (a fresh one: the backward reads nothing the forward left)
    rc = L.decnet_bn_train_backward(z.data_ptr(), gyd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                    gz.data_ptr() if want_gz else None, dg.data_ptr(), db.data_ptr(), int(relu),
                                    ws2.data_ptr(), nws, *shape, _st())
    assert rc == 0, rc
    P.check("bn_train %s" % (shape,))
    assert not bool(torch.isnan(stats).any())
    out = {"y": y.cpu(), "stats": stats.cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu(), "dgamma": dg.cpu(),
           "dbeta": db.cpu()}
    if want_gz:
        out["gz"] = gz.cpu()
    return out


_REFS = {}


def _ref(shape, first_kind, relu):
    """The float64 forward of a case, computed once."""
    key = (shape, first_kind, relu)
    if key not in _REFS:
        d = BR.entry_data(shape, first_kind, relu)
        _REFS[key] = (d, BR.forward(d["z"], d["gamma"], d["beta"], EPS, MOM, d["running_mean"], d["running_var"], relu))
    return _REFS[key]


def _pc(v):
    return v.view(1, -1, 1, 1)


def _check_entry(r, shape, first_kind, relu):
    """The bounds of _bn_train_ref.check_entry, each from counting roundings; and the channel put below zero."""
    d, f = _ref(shape, first_kind, relu)
    BR.check_entry(r, f, d["gamma"], d["beta"], d["gy"], relu, EPS, (shape, first_kind, relu))
    if relu and shape[1] > 1:                                   # the channel with every pre-activation below zero
        c = shape[1] - 1
        assert not bool(r["y"][:, c].any()) and not bool(r["gz"][:, c].any())
        assert float(r["dgamma"][c]) == 0.0 and float(r["dbeta"][c]) == 0.0


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("first_kind", [0, 1, 2], ids=BR.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entries_against_float64(dev, shape, first_kind, relu):
    _check_entry(_both(_run_entry, shape, first_kind, relu), shape, first_kind, relu)


# ---- 2. decisions, determinism, refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_backward_recomputes_the_forward_relu_decision(dev, shape):
    """gy = 1: dbeta[c] is the number of elements the backward let through, and equals the count of y[:, c] > 0 exactly."""
    for first_kind in (0, 1):
        for aligned in (True, False):
            r = _run_entry(shape, first_kind, True, ones=True, aligned=aligned)
            assert torch.equal(r["dbeta"], (r["y"] > 0).sum((0, 2, 3)).float()), (shape, first_kind, aligned)


def test_parameter_gradients_alone(dev):
    """gz NULL: two launches, the same dgamma and dbeta."""
    shape = SHAPES[4]
    a, b = _run_entry(shape, 0, True), _run_entry(shape, 0, True, want_gz=False)
    assert "gz" not in b and all(_bits_equal(a[k], b[k]) for k in b)


def test_two_calls_and_graph_replays_are_bit_identical(dev):
    from decnet_amd import ops2d
    shape = SHAPES[4]
    first = _run_entry(shape, 1, True)
    again = _run_entry(shape, 1, True)
    for k in first:
        assert _bits_equal(first[k], again[k]), k
    d = BR.entry_data(shape, 1, True)
    t = {k: v.to(dev) for k, v in d.items()}
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()

    def run():
        y, stats = ops2d.bn_train_forward(t["z"], t["gamma"], t["beta"], EPS, MOM, rm, rv, True)
        gz, dg, db = ops2d.bn_train_backward(t["z"], t["gy"], t["gamma"], t["beta"], stats, True)
        return {"y": y, "stats": stats, "gz": gz, "dgamma": dg, "dbeta": db}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        rm.copy_(t["running_mean"])
        rv.copy_(t["running_var"])
        for v in out.values():
            v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = dict({k: v.cpu() for k, v in out.items()}, running_mean=rm.cpu(), running_var=rv.cpu())
        for k in first:
            assert _bits_equal(first[k], got[k]), "%s differs between the eager call and a graph replay" % k


def test_rejections_launch_nothing(dev):
    L = _L()
    shape = (2, 3, 5, 7)
    d = BR.entry_data(shape, 0, True)
    P = Place(dev, True)
    z, gy, gamma, beta = P.inp(d["z"]), P.inp(d["gy"]), P.inp(d["gamma"]), P.inp(d["beta"])
    rm, rv = P.inp(d["running_mean"]), P.inp(d["running_var"])
    stats, y, gz, dg, db = P.out((6,), torch.float64), P.out(shape), P.out(shape), P.out((3,)), P.out((3,))
    ws, nws = _ws(L, dev, shape)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)

    def fwd(rm_=rm.data_ptr(), rv_=rv.data_ptr(), ws_=ws.data_ptr(), n_=nws, dims=shape):
        return L.decnet_bn_train_forward(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOM, rm_, rv_, stats.data_ptr(),
                                         y.data_ptr(), 1, ws_, n_, *dims, _st())

    def bwd(ws_=ws.data_ptr(), n_=nws, dims=shape):
        return L.decnet_bn_train_backward(z.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                          gz.data_ptr(), dg.data_ptr(), db.data_ptr(), 1, ws_, n_, *dims, _st())

    assert fwd(dims=(1, 3, 1, 1)) == ERR_SHAPE and bwd(dims=(1, 3, 1, 1)) == ERR_SHAPE          # N = 1
    assert fwd(n_=nws - 1) == ERR_SHAPE and bwd(n_=nws - 1) == ERR_SHAPE                        # a short workspace
    assert fwd(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED                            # off by 4 bytes
    assert bwd(ws_=big.data_ptr() + 4, n_=nws + 4) == ERR_MISALIGNED
    assert fwd(rm_=None) == ERR_NULL and fwd(rv_=None) == ERR_NULL                              # one of the two alone
    assert fwd(ws_=None) == ERR_NULL and bwd(ws_=None) == ERR_NULL
    P.check_untouched("rejected bn_train")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all())
    assert fwd(rm_=None, rv_=None) == 0 and bwd() == 0          # without running statistics; and the complete backward
    P.check("accepted bn_train")


# ---- 3. Units in .train() mode ---------------------------------------------------------------------------------------------------
CONV_FN = {"conv": "Conv2dSmallFunction", "mfma": "Conv2dMfmaFunction", "s3": "Conv2dS3Function", "deconv": "Deconv2dS3Function"}
# the forward gates of the convolution kernels (tests/_model_cases.py), per forward route
Z_TOL = {"conv": MC.FP32_TOL, "conv_s3": MC.FP32_TOL, "deconv": MC.FP32_TOL, "mfma": MC.MFMA_TOL, "mfma_s3": MC.S3_TOL,
         "mfma_deconv": MC.MFMA_TOL}


def _graph_names(t):
    seen, names, todo = set(), [], [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _library_nodes(names):
    return [n for n in names if ("Convolution" in n or "BatchNorm" in n) and not n.startswith("BatchNormActFunction")]


def _unit_on(dev, name):
    u, xs, gy = BR.unit_case(name)
    ud = copy.deepcopy(u).to(dev).train()
    xd = [t.to(dev).requires_grad_() for t in xs]
    return u, xs, gy, ud, xd, (tuple(xd) if len(xd) > 1 else xd[0])


@pytest.mark.parametrize("name", [n for n in sorted(BR.UNIT_CASES) if n != "nobn"])
def test_unit_in_train_mode(dev, name):
    """One unit per route.  Forward bound: the convolution kernel's own gate dz = tol max(1, max|z64|) on z (Z_TOL) carried
    through the normalisation -- mean moves by at most dz, invstd by at most invstd^2 dz relative to itself, so xhat by at
    most invstd dz (2 + |xhat|) -- plus the entry's output bound 4 u (|xhat gamma| + |beta|).  The same bound says which
    ReLU decisions may differ from float64's.  Measured on an MI355X, worst error over this bound: conv 0.0053, conv_s3
    0.0030, deconv 0.0020, mfma 0.032, mfma_deconv 0.016, mfma_s3 0.011 -- the gates of the convolution kernels are that
    much wider than their errors at these sizes -- and no ReLU decision of any case differed from float64's (the test
    prints both figures)."""
    import decnet_amd
    from decnet_amd import model
    route = BR.UNIT_CASES[name][0]
    u, xs, gy, ud, xd, arg = _unit_on(dev, name)
    B, _, H, W = xs[0].shape
    parts = len(xs) if len(xs) > 1 else None
    assert ud._route(B, H, W, parts) == route and ud._grad_route_train(B, H, W, parts) == BR.GRAD_ROUTE[route]
    model.TALLY = []
    try:
        with decnet_amd.hip_grad():
            y = ud(arg)
        tally = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
    assert tally == [BR.GRAD_ROUTE[route] + "_grad", "bn_train"], tally
    assert ud._hip_kind(arg) is None
    names = _graph_names(y)
    assert "BatchNormActFunctionBackward" in names and CONV_FN[BR.GRAD_ROUTE[route]] + "Backward" in names, names
    assert not _library_nodes(names), names
    y.backward(gy.to(dev))
    # forward against float64 conv -> batch_norm(training) -> relu
    y64, pre64, _, _ = BR.unit_train(u, xs, BR.D)
    c64 = copy.deepcopy(u).double()
    with torch.no_grad():
        z64 = c64.conv(torch.cat([t.double() for t in xs], 1))
    f = BR.forward(z64, u.bn.weight, u.bn.bias, u.bn.eps)
    assert float((f["y"] - y64).abs().max()) <= 1e-9
    gam, bet = _pc(u.bn.weight.double().abs()), _pc(u.bn.bias.double().abs())
    dz = Z_TOL[route] * max(1.0, float(z64.abs().max()))
    b_y = gam * _pc(f["invstd"]) * dz * (2 + f["xhat"].abs()) + 4 * U * (f["xhat"].abs() * gam + bet)
    yc = y.detach().cpu()
    e_y = (yc.double() - y64).abs()
    print(name, "y: worst error / bound = %.3g" % float((e_y / b_y).max()))
    assert bool((e_y <= b_y).all())
    # gradients against float64 with the GPU run's ReLU decisions imposed; float32 on the CPU sets the gate
    mask = yc > 0
    flipped = mask != (pre64 > 0)
    print(name, "ReLU decisions that differ from float64's: %d of %d" % (int(flipped.sum()), flipped.numel()))
    assert bool((pre64.abs()[flipped] <= b_y[flipped]).all()), "a ReLU decision far from zero differs from float64's"
    _, _, g64, u64 = BR.unit_train(u, xs, BR.D, mask, gy)
    _, _, g32, _ = BR.unit_train(u, xs, torch.float32, mask, gy)
    got = {"x%d" % i: t.grad for i, t in enumerate(xd)}
    got.update({n: p.grad for n, p in ud.named_parameters()})
    assert got.keys() == g64.keys()
    for k, ref in g64.items():
        err, gate = float((got[k].cpu().double() - ref).abs().max()), BR.gate(ref, g32[k])
        print(name, k, "hip %.3g  gate %.3g" % (err, gate))
        assert got[k].shape == ref.shape and err <= gate, (name, k, err, gate)
    # running statistics after one and after three steps (the project's small-kernel yardstick on values of order 1)
    for steps in (1, 3):
        if steps == 3:
            for _ in range(2):
                with decnet_amd.hip_grad():
                    ud(arg)
                u64 = BR.unit_train(u64, xs, BR.D)[3]
        assert int(ud.bn.num_batches_tracked) == steps == int(u64.bn.num_batches_tracked)
        for k in ("running_mean", "running_var"):
            assert MC.close(getattr(ud.bn, k), getattr(u64.bn, k), MC.FP32_TOL) <= 1.0, (name, k, steps)
    # the folded caches saw the new statistics: the eval forward has the bits of a cold copy's
    cold = copy.deepcopy(ud).eval()
    with torch.no_grad():
        assert _bits_equal(ud.eval()(arg), cold(arg))
        assert ud._hip_kind(arg) == route


def test_unit_in_train_mode_without_hip_grad(dev):
    import decnet_amd
    u, xs, gy, ud, xd, arg = _unit_on(dev, "conv")
    names = _graph_names(ud(arg))
    with decnet_amd.hip_grad(), torch.no_grad():
        assert ud(arg).grad_fn is None
    assert not [n for n in names if "Function" in n] and _library_nodes(names), names
    assert int(ud.bn.num_batches_tracked) == 2


@pytest.mark.parametrize("name", ["conv", "mfma_deconv"])
def test_training_unit_with_frozen_bn_goes_on_as_before(dev, name):
    """model.train() with every BatchNorm put back into eval mode -- fine-tuning on frozen statistics: under hip_grad() the
    unit records none of the new Functions, writes no buffer and computes the bits it computes with hip_grad() off."""
    import decnet_amd
    u, xs, gy, ud, xd, arg = _unit_on(dev, name)
    ud.bn.eval()
    assert ud.training and not ud.bn.training
    before = {k: b.detach().clone() for k, b in ud.named_buffers()}
    with decnet_amd.hip_grad():
        y = ud(arg)
    names = _graph_names(y)
    assert not [n for n in names if "Function" in n] and _library_nodes(names), names
    y_off = ud(arg)
    assert _bits_equal(y.detach(), y_off.detach())
    ref = BR.forward(ud.conv(torch.cat(xd, 1)).detach().cpu(), u.bn.weight, u.bn.bias, u.bn.eps)     # batch statistics
    assert float((y.detach().cpu().double() - ref["y"]).abs().max()) > 1e-2, "the frozen statistics were not used"
    for k, b in ud.named_buffers():
        assert torch.equal(b, before[k]), k
    assert int(ud.bn.num_batches_tracked) == 0
    y.backward(gy.to(dev))
    assert all(p.grad is not None for p in ud.parameters())


def test_fuse_with_frozen_bn_goes_on_as_before(dev):
    import decnet_amd
    m, ins, wrt, r = BR.module_case("attention")
    m = copy.deepcopy(m).to(dev).train()
    for u in m.conv:
        u.bn.eval()
    t = {k: v.to(dev).requires_grad_(k in wrt) for k, v in ins.items()}
    before = {k: b.detach().clone() for k, b in m.named_buffers()}
    with decnet_amd.hip_grad():
        out = BR.module_out("attention", m, t)
    names = _graph_names(out)
    assert "BatchNormActFunctionBackward" not in names and "SigmoidBlendFunctionBackward" not in names, names
    assert _bits_equal(out.detach(), BR.module_out("attention", m, t).detach())
    for k, b in m.named_buffers():
        assert torch.equal(b, before[k]), k


def test_unit_without_bn_in_train_mode(dev):
    """Without BatchNorm the training flag changes nothing: the eval route's Function, and the bits of the eval forward."""
    import decnet_amd
    u, xs, gy, ud, xd, arg = _unit_on(dev, "nobn")
    with torch.no_grad():
        plain = copy.deepcopy(ud).eval()(arg)
    with decnet_amd.hip_grad():
        y = ud(arg)
    names = _graph_names(y)
    assert ud.training and "Conv2dSmallFunctionBackward" in names and not _library_nodes(names), names
    assert "BatchNormActFunctionBackward" not in names and _bits_equal(y.detach(), plain)


# ---- 4. Modules in .train() mode -------------------------------------------------------------------------------------------------
_RUNS = {}


def _module_runs(name, dev):
    """float64 and float32 on the CPU, HIP under hip_grad(): one step and three steps each -- once."""
    import decnet_amd
    if name not in _RUNS:
        case = BR.module_case(name)
        _RUNS[name] = {(tag, steps): BR.module_grads(name, *case, dtype, device=d, ctx=ctx, steps=steps)[:2]
                       for steps in (1, 3)
                       for tag, dtype, d, ctx in (("f64", torch.float64, "cpu", None), ("f32", torch.float32, "cpu", None),
                                                  ("hip", torch.float32, dev, decnet_amd.hip_grad))}
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(BR.MODULE_SEEDS))
def test_module_gradients_and_buffers(dev, name):
    runs = _module_runs(name, dev)
    for steps in (1, 3):
        for what in (0, 1):                                      # gradients (of the last step), buffers
            r64, r32, rhip = runs[("f64", steps)][what], runs[("f32", steps)][what], runs[("hip", steps)][what]
            assert r64.keys() == rhip.keys()
            for k, ref in r64.items():
                if k.endswith("num_batches_tracked"):
                    assert int(rhip[k]) == steps == int(ref), k
                    continue
                err, gate = float((rhip[k].double() - ref).abs().max()), BR.gate(ref, r32[k])
                print(name, steps, k, "hip %.3g  gate %.3g" % (err, gate))
                assert rhip[k].shape == ref.shape and err <= gate, (name, steps, k, err, gate)


@pytest.mark.parametrize("name", sorted(BR.MODULE_SEEDS))
def test_module_graph_and_second_backward(dev, name):
    import decnet_amd
    from decnet_amd import model
    m, ins, wrt, r = BR.module_case(name)
    m = copy.deepcopy(m).to(dev).train()
    t = {k: v.to(dev) for k, v in ins.items()}
    for k in wrt:
        t[k].requires_grad_()
    r = r.to(dev)
    leaves = list(m.parameters()) + [t[k] for k in wrt]
    model.TALLY = []
    try:
        out = BR.module_step(name, m, t, wrt, r, decnet_amd.hip_grad)
        tally = [x["family"] for x in model.TALLY]
    finally:
        model.TALLY = None
    names = _graph_names(out)
    units = [u for u in m.modules() if isinstance(u, model.Unit)]
    assert names.count("BatchNormActFunctionBackward") == sum(u.bn is not None for u in units), names
    assert not _library_nodes(names), names
    assert tally == [f for u in units for f in (["conv_grad", "bn_train"] if u.bn is not None else ["conv_grad"])], tally
    if name == "attention":
        assert "SigmoidBlendFunctionBackward" in names
    first = [p.grad.detach().clone() for p in leaves]
    BR.module_step(name, m, t, wrt, r, decnet_amd.hip_grad)     # the same batch: the same statistics, the same gradient
    for a, p in zip(first, leaves):
        assert _bits_equal(p.grad, a + a), "a second backward does not add exactly"


def test_refinement_graphed_step(dev):
    """The refinement step captured once and replayed three times on new inputs copied in place: every replay's gradients
    have the bits of an eager step on that data, the buffers those after three eager steps."""
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    name = "refinement"
    m0, ins, wrt, r = BR.module_case(name)
    r = r.to(dev)
    g = torch.Generator().manual_seed(5)
    data = [{k: (torch.randn(v.shape, generator=g) if k != "disp" else torch.rand(v.shape, generator=g) * 4)
             for k, v in ins.items()} for _ in range(3)]

    def setup():
        m = copy.deepcopy(m0).to(dev).train()
        t = {k: v.to(dev) for k, v in ins.items()}
        for k in wrt:
            t[k].requires_grad_()
        return m, t, list(m.parameters()) + [t[k] for k in wrt]

    me, te, le = setup()
    eager = []
    for d in data:
        with torch.no_grad():
            for k, v in d.items():
                te[k].copy_(v)
        for p in le:
            p.grad = None
        BR.module_step(name, me, te, wrt, r, decnet_amd.hip_grad)
        torch.cuda.synchronize()
        eager.append([p.grad.detach().clone() for p in le])
    mg, tg, lg = setup()
    start = {k: b.detach().clone() for k, b in mg.named_buffers()}
    graphed = GraphedStep(lambda: BR.module_step(name, mg, tg, wrt, r, decnet_amd.hip_grad), grads_of=lg)
    with torch.no_grad():                                       # the warm-up steps moved the buffers: back to the start
        for k, b in mg.named_buffers():
            b.copy_(start[k])
    for d, want in zip(data, eager):
        with torch.no_grad():
            for k, v in d.items():
                tg[k].copy_(v)
        for p in lg:
            p.grad.fill_(float("nan"))
        graphed()
        torch.cuda.synchronize()
        for p, w in zip(lg, want):
            assert _bits_equal(p.grad, w), "a replay's gradient differs from the eager step's"
    be = dict(me.named_buffers())
    for k, b in mg.named_buffers():
        assert torch.equal(b, be[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(b) == 3
