"""Training-mode BatchNorm under hip_grad() without a GPU: the float64 restatement of tests/_bn_train_ref.py against torch's
own float64 autograd of F.batch_norm(training=True) + ReLU, the pure routing of a unit in train mode
(Unit._grad_route_train, SoftAttention._fuse_grad_route_train), the C ABI's refusals and workspace query, and the margin
property of the seeded module cases the GPU test runs."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _bn_train_ref as BR
import _model_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 4096
# the shapes of the GPU test's entry cases, the three longest cut down to CPU size with the same structure (a full segment,
# a one-element tail, many segments)
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 7), (1, 8, 16, 18), (1, 2, 1, SEG), (3, 5, 1, SEG + 1), (5, 1, 1, 6 * SEG + 3)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _torch_float64(z, d, relu, eps, mom):
    """torch's own float64 autograd of F.batch_norm(training=True) (+ ReLU) on z -> dict of y, pre, the two buffers and the
    three gradients."""
    z = z.clone().requires_grad_()
    gamma, beta = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    rm, rv = d["running_mean"].double().clone(), d["running_var"].double().clone()
    pre = F.batch_norm(z, rm, rv, gamma, beta, True, mom, eps)
    y = torch.relu(pre) if relu else pre
    y.backward(d["gy"].double())
    return dict(y=y.detach(), pre=pre.detach(), running_mean=rm, running_var=rv, gz=z.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("first_kind", [0, 1, 2], ids=BR.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reference_against_torch_float64(shape, first_kind, relu):
    """Forward, running buffers and all three gradients to 1e-12 (of max(1, max|torch's value|) per tensor) of torch's
    float64 batch_norm + ReLU, on every data set.

    torch forms its float64 mean without a pivot, so on a channel of mean 1000 and spread 0.01 its OWN xhat is off by
    2^-53 |mean| / sigma = 1e-11 (measured: 5.6e-12 on y at shape 1x1x1x2), which no restatement can match to 1e-12.  Batch
    norm is invariant under a per-channel shift, and z - p is exact in float64, so the comparison at the full 1e-12 is
    made with torch run on z - p (its mean moved back by p); torch run on z itself is held to 1e-12 on the other
    channels and to 1e-12 x 1e5, the conditioning, on the channels of mean 1000."""
    d = BR.entry_data(shape, first_kind, relu)
    eps, mom = 1e-5, 0.1
    z64 = d["z"].double()
    p = z64[0, :, 0, 0].clone()
    fwd = BR.forward(d["z"], d["gamma"], d["beta"], eps, mom, d["running_mean"], d["running_var"], relu)
    shifted, direct = _torch_float64(z64 - p.view(1, -1, 1, 1), d, relu, eps, mom), _torch_float64(z64, d, relu, eps, mom)
    shifted["running_mean"] = shifted["running_mean"] + mom * p
    mask = shifted["pre"] > 0                                  # torch's decisions (they differ only within rounding of 0)
    own = mask == (fwd["pre"] > 0)
    assert bool((own | (fwd["pre"].abs() <= 1e-12 * fwd["pre"].abs().max().clamp_min(1.0))).all())
    bwd = BR.backward(fwd, d["gy"], d["gamma"], relu, mask if relu else None)
    got = dict(fwd, **bwd)
    offset = torch.tensor([BR.KINDS[(c + first_kind) % 3] == "offset" for c in range(shape[1])])
    cond = torch.where(offset, 1e5, 1.0).double()
    for what in ("y", "running_mean", "running_var", "gz", "dgamma", "dbeta"):
        ref = shifted[what]
        err = float((got[what] - ref).abs().max())
        tol = 1e-12 * max(1.0, float(ref.abs().max()))
        print(shape, first_kind, relu, what, "error %.3g, tolerance %.3g" % (err, tol))
        assert err <= tol, (what, err, tol)
        ref = direct[what]
        if relu and what in ("gz", "dgamma", "dbeta") and not bool(((direct["pre"] > 0) == mask).all()):
            continue                                           # (torch on z itself decided an element at 0 otherwise)
        ec = (got[what] - ref).abs()
        ec = ec.amax((0, 2, 3)) if ec.dim() == 4 else ec
        assert bool((ec <= tol * cond).all()), (what, "torch on z itself", ec, tol)
    assert not any(bool(torch.isnan(v).any()) for v in list(fwd.values()) + list(bwd.values()))
    for c in range(shape[1]):
        if BR.KINDS[(c + first_kind) % 3] == "constant":
            assert float(fwd["var"][c]) == 0.0 and float(fwd["mean"][c]) == float(d["z"][0, c, 0, 0])
    if relu and shape[1] > 1:                                  # the channel whose beta puts every pre-activation below zero
        c = shape[1] - 1
        assert bool((fwd["pre"][:, c] < 0).all())
        assert float(bwd["dgamma"][c]) == 0.0 and float(bwd["dbeta"][c]) == 0.0 and not bool(bwd["gz"][:, c].any())


def _unit(name):
    route, ci, co, k, kw, B, H, W, parts = BR.UNIT_CASES[name]
    return MC.make_unit(ci, co, k, seed=1, **kw), route, B, H, W, (len(parts) if parts else None)


@pytest.mark.parametrize("name", [n for n in sorted(BR.UNIT_CASES) if n != "nobn"])
def test_train_route_of_each_unit_case(name, monkeypatch):
    """Every unit case of the GPU test sits on the forward route its name says (Unit._route) and takes the train-mode
    route of that family; the routing looks at the layer and the sizes alone."""
    monkeypatch.delenv("DECNET_CONV2D", raising=False)
    monkeypatch.delenv("DECNET_CONV2D_MFMA", raising=False)
    u, route, B, H, W, parts = _unit(name)
    assert u._route(B, H, W, parts) == route
    assert u._grad_route_train(B, H, W, parts) == BR.GRAD_ROUTE[route]
    assert u.train()._grad_route_train(B, H, W, parts) == BR.GRAD_ROUTE[route]      # the flag is the caller's business
    big = MC.make_unit(32, 32, 3, seed=1)                       # a unit of the library at this size, in either mode
    assert big._route(1, 10, 10) is None and big._grad_route_train(1, 10, 10) is None


def test_train_route_refusals():
    u, route, B, H, W, parts = _unit("conv")
    assert u._grad_route_train(B, H, W, parts) == "conv"
    u.bn.momentum = None                                        # a cumulative average: not what the kernel computes
    assert u._grad_route_train(B, H, W, parts) is None
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        u.bn = torch.nn.BatchNorm2d(8, **kw)
        assert u._grad_route_train(B, H, W, parts) is None, kw
    u.bn = torch.nn.BatchNorm2d(8)
    assert u._grad_route_train(B, H, W, parts) == "conv"
    nobn, route, B, H, W, parts = _unit("nobn")
    assert nobn.bn is None and nobn._route(B, H, W) == "conv" and nobn._grad_route(B, H, W) == "conv"
    assert nobn._grad_route_train(B, H, W) is None
    assert u._grad_route_train(1, 15, 17, 3) is None            # 255 pixels: below the route's floor, as in eval mode


def test_fuse_route_in_train_mode():
    from decnet_amd.model import SoftAttention
    att = MC.seeded(lambda: SoftAttention(12, 8), 3)
    H, W = BR.MODULE_HW
    assert att._fuse_grad_route(BR.MODULE_B, H, W) and att._fuse_grad_route_train(BR.MODULE_B, H, W)
    att.conv[1].bn.momentum = None
    assert att._fuse_grad_route(BR.MODULE_B, H, W) and not att._fuse_grad_route_train(BR.MODULE_B, H, W)


def test_nothing_changes_on_the_cpu():
    """A train-mode unit on the CPU under hip_grad() is the library's conv -> batch_norm -> ReLU, bit for bit, and updates
    its buffers as ever."""
    import decnet_amd
    u, xs, gy = BR.unit_case("conv")
    a, b = MC.make_unit(17, 8, 3, dil=3, seed=17 + 24).train(), MC.make_unit(17, 8, 3, dil=3, seed=17 + 24).train()
    with decnet_amd.hip_grad():
        ya = a(tuple(xs))
    yb = b(tuple(xs))
    assert torch.equal(ya, yb) and torch.equal(a.bn.running_var, b.bn.running_var)
    assert int(a.bn.num_batches_tracked) == 1 and "BatchNormActFunction" not in type(ya.grad_fn).__name__


@pytest.fixture(scope="module")
def lib():
    from decnet_amd import _lib, build
    h = ctypes.CDLL(build.build())
    for name in ("decnet_bn_train_workspace_floats", "decnet_bn_train_forward", "decnet_bn_train_backward"):
        getattr(h, name).argtypes = _lib.SIGNATURES[name]
    h.decnet_bn_train_workspace_floats.restype = ctypes.c_size_t
    return h


def test_segment_constant_and_workspace_query(lib):
    from decnet_amd import ops2d
    src = open(os.path.join(ROOT, "include", "decnet_hip.h")).read()
    assert int(re.search(r"#define\s+DECNET_BN_SEGMENT\s+(\d+)", src).group(1)) == ops2d.BN_SEGMENT == SEG
    q = lib.decnet_bn_train_workspace_floats
    for (B, C, H, W) in SHAPES + [(5, 1, 1, 60 * SEG + 3), (8, 8, 540, 972)]:
        nseg = -(-H * W // SEG)
        assert q(B, C, H, W) == 2 * (2 * C * B * nseg + 2 * C), (B, C, H, W)
    assert q(1, 4, 1, 1) == 0 and q(0, 4, 5, 5) == 0 and q(1, 4, 5, -1) == 0         # N < 2, a dimension < 1
    assert q(2, 1, 32768, 32768) == 0 and q(1, 1, 32768, 65535) > 0                  # B C H W >= 2^31 | below


def test_refusals_before_any_launch(lib):
    """Argument validation comes before the first HIP call, so it runs without a GPU (the pointers are never read)."""
    NULL, SHAPE, MISALIGNED = -1, -2, -5
    one = 4096
    fwd, bwd, q = lib.decnet_bn_train_forward, lib.decnet_bn_train_backward, lib.decnet_bn_train_workspace_floats
    n = q(2, 3, 5, 7)

    def f(z=one, gamma=one, beta=one, rm=one, rv=one, stats=one, y=one, ws=one, nws=n, dims=(2, 3, 5, 7)):
        return fwd(z, gamma, beta, 1e-5, 0.1, rm, rv, stats, y, 1, ws, nws, *dims, None)

    def b(z=one, gy=one, gamma=one, beta=one, stats=one, dg=one, db=one, ws=one, nws=n, dims=(2, 3, 5, 7)):
        return bwd(z, gy, gamma, beta, stats, None, dg, db, 1, ws, nws, *dims, None)

    assert f(z=None) == NULL and f(gamma=None) == NULL and f(beta=None) == NULL and f(stats=None) == NULL
    assert f(y=None) == NULL and f(ws=None) == NULL
    assert f(rm=None) == NULL and f(rv=None) == NULL                                  # one of the two alone
    assert f(dims=(1, 3, 1, 1)) == SHAPE and f(dims=(2, 0, 5, 7)) == SHAPE            # N = 1; a dimension < 1
    assert f(dims=(2, 1, 32768, 32768), nws=1 << 40) == SHAPE                         # B C H W = 2^31
    assert f(nws=n - 1) == SHAPE                                                      # a short workspace
    assert f(ws=one + 4) == MISALIGNED and f(stats=one + 4) == MISALIGNED             # off by 4 bytes
    assert b(z=None) == NULL and b(gy=None) == NULL and b(stats=None) == NULL and b(dg=None) == NULL
    assert b(db=None) == NULL and b(ws=None) == NULL
    assert b(dims=(1, 3, 1, 1)) == SHAPE and b(nws=n - 1) == SHAPE and b(ws=one + 4) == MISALIGNED


@pytest.mark.parametrize("name", sorted(BR.MODULE_SEEDS))
def test_module_seeds_have_margins(name):
    """The seeds recorded in _bn_train_ref.MODULE_SEEDS: in the float64 train-mode run no BatchNorm output of a ReLU'd unit
    lies within MARGIN max(1, max|pre|) of zero, so a float32 run decides every ReLU as float64 does and the module's
    gradients can be compared without imposing masks.  (Chosen as the first seed from 1 up with that property.)"""
    m, ins, wrt, r = BR.module_case(name)
    assert m.training and all(u.training for u in m.modules())
    margins = []
    g64, bufs, m64, _ = BR.module_grads(name, m, ins, wrt, r, torch.float64, margins=margins)
    assert len(margins) == (6 if name == "refinement" else 2)
    print(name, [(un, "%.3g" % (lo / max(1.0, hi))) for un, lo, hi in margins])
    assert BR.margins_hold(margins)
    assert all(int(v) == 1 for k, v in bufs.items() if k.endswith("num_batches_tracked"))
    assert all(bool(torch.isfinite(v).all()) for v in g64.values())
