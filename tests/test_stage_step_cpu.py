"""The float64 reference of one training stage (tests/_stage_step_ref.py), checked without a GPU, so that the gates of
tests/test_stage_step_gpu.py rest on something:
  1. composition: `reference` (formulas, free run) agrees with the modules' own torch routes in float64 around the reference
     SpaMat Function, and its forward with the formulas of tests/_model_ref.py;
  2. RefSpaMat: its backward is the derivative of its forward with max_cost held fixed (quirk S7), by central differences;
  3. every leaf and every parameter gets a non-zero float64 gradient and no ReLU'd unit is dead (else the GPU gates could
     pass vacuously);
  4. the float32 run, the yardstick of the module gate, stays close to the float64 run;
  5. routes: each case reaches what it is meant to reach (pure functions of sizes);
  6. imposed data: imposing the free run's own decisions changes nothing; an imposed flip is reported by the guards."""
import pytest
import torch

import _model_ref as MR
import _stage_step_ref as S

CASE_NAMES = sorted(S.CASES)
_RUNS = {}


def _runs(case):
    """(modules, data, float64 reference, float32 reference, the torch routes in float64) -- once per case."""
    if case not in _RUNS:
        D = S.CASES[case]["D"]
        mods, t = S.modules(case), S.data(case)
        _RUNS[case] = (mods, t, S.reference(mods, t, D), S.reference(mods, t, D, torch.float32), S.torch_step(mods, t, D))
    return _RUNS[case]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_reference_is_the_composition_of_the_torch_routes(case):
    mods, t, r64, _, (planes, grads) = _runs(case)
    for k, want in planes.items():
        got = r64["planes"][k]
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k
    assert grads.keys() == r64["grads"].keys()
    for k, want in grads.items():
        assert float((r64["grads"][k] - want).abs().max()) <= 1e-9 * float(want.abs().max()), k
    # the formulas are those of _model_ref: the same planes from its (detached) functions
    p = r64["planes"]
    dense = MR.dynamic_upsampling(t["pred0"], t["L"], MR.seq_params(mods["up"].weight_learning))
    fused = MR.fuse(t["L"], dense, p["sparse"], t["lmask"], p["var"], MR.seq_params(mods["att"].conv))
    pred = MR.refinement(t["L"], t["R"], fused, MR.seq_params(mods["ref"].conv))
    for k, want in (("dense", dense), ("fused", fused), ("pred", pred)):
        assert float((p[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k


def test_ref_spamat_backward_is_the_derivative_with_max_cost_fixed():
    B, C, H, W, D = 1, 3, 2, 7, 4
    g = torch.Generator().manual_seed(41)
    L, R = (torch.relu(torch.randn(B, C, H, W, generator=g, dtype=torch.float64)) for _ in range(2))
    lm, rm = ((torch.rand(B, H, W, generator=g) < 0.7).double() for _ in range(2))
    r = torch.randn(B, H, W, generator=g, dtype=torch.float64)
    La, Ra = L.clone().requires_grad_(), R.clone().requires_grad_()
    out = S.RefSpaMat.apply(La, Ra, lm, rm, D, None)
    mx = S.SR.forward(L, R, lm, rm, D)["max_cost"]
    assert torch.equal(out.detach(), S.spamat_out_fixed_max(L, R, lm, rm, D, mx))
    (out * r).sum().backward()
    assert float(La.grad.abs().max()) > 0 and float(Ra.grad.abs().max()) > 0
    eps = 1e-6
    for x, got, other, left in ((L, La.grad, R, True), (R, Ra.grad, L, False)):
        fd = torch.zeros_like(x)
        for i in range(x.numel()):
            vals = []
            for s in (1, -1):
                xp = x.clone()
                xp.view(-1)[i] += s * eps
                a, b = (xp, other) if left else (other, xp)
                vals.append(float((S.spamat_out_fixed_max(a, b, lm, rm, D, mx) * r).sum()))
            fd.view(-1)[i] = (vals[0] - vals[1]) / (2 * eps)
        # central differences in float64: truncation eps^2 f''' / 6 and cancellation 2^-53 |f| / eps, both ~ 1e-10
        assert float((got - fd).abs().max()) <= 1e-7 * max(1.0, float(fd.abs().max())), "L" if left else "R"


@pytest.mark.parametrize("case", CASE_NAMES)
def test_no_gradient_vanishes_and_no_unit_is_dead(case):
    _, _, r64, _, _ = _runs(case)
    assert set(S.LEAVES) <= r64["grads"].keys() and len(r64["grads"]) == 3 + 9 + 9 + 6 * 3 + 2
    for k, g in r64["grads"].items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    for k in ("L", "R"):
        assert float(r64["g_sp"][k].abs().max()) > 0, k
    active = {k: float(m.double().mean()) for k, m in r64["rec"]["free"].items()}
    assert len(active) == 2 + 2 + 6 and min(active.values()) >= 0.1, active


@pytest.mark.parametrize("case", CASE_NAMES)
def test_float32_yardstick_is_close_to_float64(case):
    """The module gate is max(4 e32, 2e-5 max(1, max|g64|)), e32 the distance of this float32 run: a sloppy yardstick
    would open the gate.  float32 carries 2^-24 per rounding; through some twenty layers and sums over up to 38016 pixels
    (relative growth ~ sqrt(38016) 2^-24 = 1.2e-5 per reduction) a float32 gradient keeps at least 2.5e-4 of its tensor's
    scale, so the gate's float32 term stays below 0.1 %."""
    _, _, r64, r32, _ = _runs(case)
    for k in ("dense", "fused", "pred", "tot"):
        a, b = r32["planes"][k].double(), r64["planes"][k]
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max())), k
    rel = {k: float((r32["grads"][k].double() - g).abs().max()) / float(g.abs().max()) for k, g in r64["grads"].items()}
    worst = max(rel, key=rel.get)
    print(case, "worst float32 distance: %.3g of max|g64| on %s" % (rel[worst], worst))
    assert rel[worst] <= 2.5e-4, (worst, rel[worst])


@pytest.mark.parametrize("case", CASE_NAMES)
def test_cases_reach_their_routes(case):
    from decnet_amd import model
    c = S.CASES[case]
    B, C, h, w = c["B"], c["C"], c["h"], c["w"]
    H, W = 3 * h, 3 * w
    mods = S.modules(case)
    att, ref, wl = mods["att"], mods["ref"], mods["up"].weight_learning
    few = [(att.conv[0], 5), (att.conv[1], None), (att.conv[2], None), (ref.conv[0], 3)] + [(u, None) for u in ref.conv[1:]]
    assert len(few) == 10
    for u, parts in few:
        assert u._grad_route(B, H, W, parts) == "conv", u
    assert att._fuse_grad_route(B, H, W)
    assert model.tail_grad_route("warp", B, C, H, W)
    assert model.tail_grad_route("unfold", B, C, h, w, 3, (H, W))
    assert model.tail_grad_route("upsample", B, 81, h, w, 3)
    for u in wl:
        assert u._grad_route(B, h, w) is None
        assert u._grad_route_mfma(B, h, w) == ("mfma" if case == "floor" else None), u
    assert [(u.conv.in_channels, u.conv.out_channels) for u in wl] == [(73, 81), (81, 81), (81, 81)]
    if case == "floor":
        assert 4096 <= h * w < 6480


def test_imposing_the_free_decisions_changes_nothing_and_a_flip_is_reported():
    mods, t, r64, r32, _ = _runs("small")
    D = S.CASES["small"]["D"]
    p = r64["planes"]
    S64 = S.SR.forward(t["L"], t["R"], t["lmask"], t["rmask"], D)
    imposed = dict(planes=(p["sparse"], S64["S"], S64["max_cost"]), var=p["var"], masks=dict(r64["rec"]["free"]),
                   cells=r64["rec"]["cells_free"])
    again = S.reference(mods, t, D, imposed=imposed)
    for k, g in r64["grads"].items():
        assert torch.equal(again["grads"][k], g), k
    tol_of = lambda name: S.MC.FP32_TOL                                                          # noqa: E731
    assert all(n == 0 for n, _, _ in S.mask_flips(again, r32, tol_of).values())
    assert S.cell_flips(again, r32)[0] == 0
    # flip the decision of the element farthest from zero (from its cell's edge): counted, and far outside the bound
    name = "ref.conv.2"
    pre = r64["rec"]["pre"][name]
    masks = {k: m.clone() for k, m in r64["rec"]["free"].items()}
    i = int(pre.abs().argmax())
    masks[name].view(-1)[i] = ~masks[name].view(-1)[i]
    cells = r64["rec"]["cells_free"].clone()
    frac = r64["rec"]["ix"] - cells
    j = int((frac - 0.5).abs().argmin())
    cells.view(-1)[j] += 1
    flipped = S.reference(mods, t, D, imposed=dict(imposed, masks=masks))
    n, worst, bound = S.mask_flips(flipped, r32, tol_of)[name]
    assert n == 1 and worst == float(pre.abs().max()) and worst > bound
    assert not torch.equal(flipped["grads"]["pred0"], r64["grads"]["pred0"])
    flipped = S.reference(mods, t, D, imposed=dict(imposed, cells=cells))       # (what follows the warp moves with it)
    n, worst, bound = S.cell_flips(flipped, r32)
    assert n == 1 and 0.4 < worst < 0.6 and worst > bound
    assert not torch.equal(flipped["grads"]["pred0"], r64["grads"]["pred0"])


@pytest.mark.parametrize("make", [lambda ps: torch.optim.SGD(ps, lr=0.01, momentum=0.9),
                                  lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True),
                                  lambda ps: torch.optim.Adam(ps, lr=1e-3, foreach=False),
                                  lambda ps: torch.optim.SGD(ps, lr=0.01, fused=True)],
                         ids=["sgd", "adam_fused", "adam_single", "sgd_fused"])
def test_an_optimizer_step_invalidates_the_weight_caches(make):
    """The fused optimizers write the parameters without bumping ``_version``; the cache key also counts optimizer steps
    (stage0.source_key), so a cache is rebuilt from the new weights after a step of any of them."""
    u = S.MC.make_unit(5, 4, 3)
    params = list(u.parameters())
    opt = make(params)
    built = []

    def get():
        return u._cached("_fold", u._sources(), (u.bn.eps,), lambda: built.append(u.conv.weight.detach().clone()) or len(built))
    assert get() == 1 and get() == 1
    for p in params:
        p.grad = torch.ones_like(p)
    before = u.conv.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, u.conv.weight.detach())
    assert get() == 2 and get() == 2 and torch.equal(built[-1], u.conv.weight.detach())
