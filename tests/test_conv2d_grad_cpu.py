"""CPU side of the few-channel conv backward (decnet_amd/conv2d_grad.py, csrc/conv2d_grad.hip):
  * tests/_conv2d_grad_ref.py (G, gsum, gm, dx through the flipped-weight convolution) and the identities dW = scale G,
    dscale = <w, G>, dshift = gsum, chained to bn.weight / bn.bias / conv.bias, equal torch's own float64 autograd of
    conv -> eval BatchNorm -> ReLU to 1e-12 relative;
  * Unit._grad_route row by row over tests/_model_cases.py;
  * hip_grad(): off by default, nests, restores, thread-local; on the CPU a Unit is untouched by it (no library lookup);
  * the seeds of the GPU test's module cases keep every ReLU pre-activation of the float64 run away from zero."""
import threading

import pytest
import torch
import torch.nn.functional as F

import _conv2d_grad_ref as GR
import _model_cases as MC
from decnet_amd import hip_grad, hip_grad_enabled
from decnet_amd.conv2d_grad import flipped_weight

D = torch.float64
REL = 1e-12


def _rel(got, ref):
    return float((got - ref).abs().max()) / max(1e-300, float(ref.abs().max()))


# (segments, Cout, k, dil, (B, H, W), relu, bn)
UNIT64 = [((8,), 8, 3, 1, (2, 6, 7), True, True), ((5,), 4, 1, 1, (2, 5, 6), True, True),
          ((8, 8, 1), 8, 3, 3, (1, 7, 9), True, True), ((4,), 3, 3, 9, (2, 6, 11), False, True),
          ((3, 2, 4), 5, 3, 1, (2, 5, 5), False, True), ((4,), 1, 3, 1, (1, 6, 6), False, False),
          ((6,), 4, 3, 3, (1, 8, 5), True, False)]


@pytest.mark.parametrize("case", UNIT64, ids=[str(i) for i in range(len(UNIT64))])
def test_reference_equals_float64_autograd(case):
    segs, cout, k, dil, (B, H, W), relu, bn = case
    cin = sum(segs)
    u = MC.make_unit(cin, cout, k, dil=dil, relu=relu, bn=bn, seed=cin + 10 * cout).double()
    g = torch.Generator().manual_seed(cin * 100 + W)
    xs = [torch.randn(B, c, H, W, generator=g, dtype=D).requires_grad_() for c in segs]
    gy = torch.randn(B, cout, H, W, generator=g, dtype=D)
    # torch's own unit: conv -> eval BatchNorm -> ReLU (what Conv2dUnit executes)
    y = F.conv2d(torch.cat(xs, 1), u.conv.weight, u.conv.bias, 1, dil * (k // 2), dil)
    if bn:
        y = F.batch_norm(y, u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias, False, 0.0, u.bn.eps)
    y = torch.relu(y) if relu else y
    params = [u.conv.weight] + ([u.bn.weight, u.bn.bias] if bn else [u.conv.bias])
    want = torch.autograd.grad(y, params + xs, gy)
    # the restatement
    G, gsum, gm = GR.wgrad(xs, gy, y if relu else None, k, dil)
    if bn:
        scale, shift = GR.bn_fold(u.bn)
    else:
        scale, shift = torch.ones(cout, dtype=D), u.conv.bias
    w = u.conv.weight.detach()
    dW, dscale, dshift = scale.detach().view(-1, 1, 1, 1) * G, (w * G).sum((1, 2, 3)), gsum
    assert _rel(dW, want[0]) <= REL
    if bn:
        dgamma, dbeta = torch.autograd.grad((scale, shift), (u.bn.weight, u.bn.bias), (dscale, dshift))
        assert _rel(dgamma, want[1]) <= REL and _rel(dbeta, want[2]) <= REL
        assert u.bn.running_mean.grad is None and u.bn.running_var.grad is None
    else:
        assert _rel(dshift, want[1]) <= REL
    dxs = GR.dx(gm, w, scale.detach(), dil)
    c0 = 0
    for c, ref in zip(segs, want[len(params):]):
        assert _rel(dxs[:, c0:c0 + c], ref) <= REL
        c0 += c
    # the package's weight builder is the reference's, also restricted to the wanted parts
    wt = flipped_weight(w, scale.detach())
    assert torch.equal(wt, GR.flipped(w, scale.detach()))
    rows = [(0, segs[0])] + ([(cin - segs[-1], cin)] if len(segs) > 2 else [])
    assert torch.equal(flipped_weight(w, scale.detach(), rows), torch.cat([wt[a:b] for a, b in rows], 0))


def _expected_grad_route(c):
    return "conv" if c["route"] == "conv" and c["cin"] <= 24 and c["H"] * c["W"] >= 256 else None


@pytest.mark.parametrize("name", sorted(MC.UNIT_CASES))
@pytest.mark.parametrize("env", [None, "torch"])
def test_grad_route_rows(name, env, monkeypatch):
    """"conv" exactly where _route says "conv" under the DEFAULT switches (whatever the environment holds), Cin <= 24
    and H W >= 256."""
    c = MC.UNIT_CASES[name]
    monkeypatch.delenv("DECNET_CONV2D", raising=False)
    monkeypatch.delenv("DECNET_CONV2D_MFMA", raising=False)
    u = MC.make_unit(c["cin"], c["cout"], c["k"], **c["kw"])
    parts = None if c["parts"] is None else len(c["parts"])
    assert u._route(c["B"], c["H"], c["W"], parts) == c["route"]
    if env is not None:
        monkeypatch.setenv("DECNET_CONV2D", env)
        monkeypatch.setenv("DECNET_CONV2D_MFMA", "0")
    assert u._grad_route(c["B"], c["H"], c["W"], parts) == _expected_grad_route(c)


def test_grad_route_limits():
    assert MC.make_unit(24, 8, 3)._grad_route(1, 16, 16) == "conv"
    assert MC.make_unit(25, 8, 3)._grad_route(1, 16, 16) is None
    assert MC.make_unit(8, 8, 3)._grad_route(1, 15, 17) is None           # H W = 255
    assert MC.make_unit(8, 8, 3)._grad_route(1, 16, 16) == "conv"
    assert MC.make_unit(17, 8, 3, dil=3)._grad_route(1, 16, 18, 3) == "conv"
    assert MC.make_unit(8, 8, 3, stride=3)._grad_route(1, 64, 64) is None  # stride 3: out of scope
    assert MC.make_unit(8, 8, 3, stride=3, transposed=True)._grad_route(1, 64, 64) is None


def test_hip_grad_default_nesting_threads():
    assert hip_grad_enabled() is False
    with hip_grad():
        assert hip_grad_enabled()
        with hip_grad(False):
            assert not hip_grad_enabled()
            with hip_grad():
                assert hip_grad_enabled()
            assert not hip_grad_enabled()
        assert hip_grad_enabled()
        seen = []
        th = threading.Thread(target=lambda: seen.append(hip_grad_enabled()))
        th.start()
        th.join()
        assert seen == [False]                                           # thread-local
    assert not hip_grad_enabled()
    with pytest.raises(RuntimeError):
        with hip_grad():
            raise RuntimeError("x")
    assert not hip_grad_enabled()


def test_cpu_unit_is_untouched_by_hip_grad(monkeypatch):
    from decnet_amd import ops

    class Spy(dict):
        looked = []

        def get(self, name, *a):
            Spy.looked.append(name)
            return dict.get(self, name, *a)

        def __getitem__(self, name):
            Spy.looked.append(name)
            return dict.__getitem__(self, name)

    monkeypatch.setattr(ops, "_FN", Spy())
    u = MC.make_unit(8, 8, 3)
    x = torch.randn(1, 8, 16, 16, generator=torch.Generator().manual_seed(3), requires_grad=True)
    want = u(x)
    gw = torch.autograd.grad(want.sum(), [x, u.conv.weight])
    with hip_grad():
        got = u(x)
        parts = u((x[:, :4], x[:, 4:]))
    gg = torch.autograd.grad(got.sum(), [x, u.conv.weight])
    assert torch.equal(got, want) and torch.equal(parts, want)
    assert all(torch.equal(a, b) for a, b in zip(gg, gw))
    assert Spy.looked == []


@pytest.mark.parametrize("name", sorted(GR.MODULE_SEEDS))
def test_module_case_seeds_keep_relu_inputs_away_from_zero(name):
    """The property the GPU test's gate rests on, checked here on the CPU for the seeds it uses: in the float64 run no
    pre-activation of a ReLU'd unit lies within 1e-4 max(1, max|pre|) of zero."""
    m, ins, wrt, r = GR.module_case(name)
    margins = []
    grads, _, _ = GR.module_grads(name, m, ins, wrt, r, D, margins=margins)
    assert len(margins) == (6 if name == "refinement" else 2)
    assert GR.margins_hold(margins), margins
    assert set(wrt) <= set(grads) and all(float(g.abs().max()) > 0 for g in grads.values())
