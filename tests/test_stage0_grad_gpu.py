"""The backward of stage 0 on the GPU (csrc/conv3d_grad.hip, decnet_amd/stage0_grad.py, CostRegNetNoDown under
hip_grad()), against the float64 restatements of tests/_stage0_grad_ref.py:
  1. decnet_conv3d_wgrad through the C ABI on integer data: gm, G and gsum bit for bit, at both placements and under both
     LDS poison words (tests/_placement._both);
  2. the same shapes on random data, with and without y: |G - G64| <= (n + 1) u S with S = sum |gm| |x| per element, u = 2^-24
     and n the case's chain length (the slice of the partition, <= 4096: an fp32 fma chain of n terms, then one rounding of
     the float64 sum of the sets); gsum likewise with S = sum |gm|; gm bit-equal;
  3. a misaligned workspace is refused with nothing written;
  4. Conv3dFunction on single units, the GPU forward's own y as the reference's mask;
  5. CostRegNetNoDown.stage0 under hip_grad(): entries taken, forward bits, every gradient against the float64 reference with
     the run's masks imposed, the imposed decisions within the forward gate of zero, frozen running statistics;
  6. eager twice and a GraphedStep replay bit-identical, a second replay on new data equal to eager on it;
  7. two SGD steps: the second forward sees the updated weights;
  8. the library arm within the same gate.
-m gpu."""
import copy

import pytest
import torch

import _stage0_grad_ref as SG
from _placement import ERR_MISALIGNED, Place, _L, _assert_close, _bits_equal, _both, _st
from test_stage0_edges_gpu import TOL_DIRECT, TOL_STAGE0_PRED, TOL_STAGE0_REG, TOL_WINO, _pred_ok

pytestmark = pytest.mark.gpu
U = SG.U32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- 1 - 3. the entry ---------------------------------------------------------------------------------------------------------
_REFS = {}


def _ref(case, exact, with_y):
    """The float64 reference of a case, computed once."""
    key = (case, exact, with_y)
    if key not in _REFS:
        G, gsum, gm, SGa, Ss = SG.wgrad(*SG.wgrad_data(case, exact, with_y))
        _REFS[key] = {"G": G, "gsum": gsum, "gm": gm, "SG": SGa, "Ss": Ss}
    return _REFS[key]


def _ws(L, dev, case):
    n = L.decnet_conv3d_wgrad_workspace_floats(*case)
    assert n == SG.plan_sl(case)[1] * case[5] * (27 * case[4] + 1), (case, n)
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev), n


def _run_wgrad(case, exact, with_y, aligned):
    B, D, H, W, Ci, Co = case
    L, dev = _L(), torch.device("cuda:0")
    x, gy, y = SG.wgrad_data(case, exact, with_y)
    P = Place(dev, aligned)
    xd, gyd = P.inp(x), P.inp(gy)
    yd = P.inp(y) if with_y else None
    gm = P.out((B, D, H, W, Co)) if with_y else None           # without ReLU: y NULL, gm NULL (gm == gy)
    G, gsum = P.out((Co, Ci, 3, 3, 3)), P.out((Co,))
    ws, nws = _ws(L, dev, case)                                # the workspace: 16-byte aligned at either placement
    rc = L.decnet_conv3d_wgrad(xd.data_ptr(), gyd.data_ptr(), yd.data_ptr() if with_y else None,
                               gm.data_ptr() if with_y else None, G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws,
                               B, D, H, W, Ci, Co, _st())
    assert rc == 0, rc
    P.check("conv3d wgrad %s" % (case,))
    out = {"G": G.cpu(), "gsum": gsum.cpu()}
    if with_y:
        out["gm"] = gm.cpu()
    return out


@pytest.mark.parametrize("case", SG.WGRAD_CASES, ids=SG.WGRAD_IDS)
def test_wgrad_exact(dev, case):
    """Integers in [-3, 3]: every partial sum is an integer below 2^24, so the results equal float64 bit for bit in any
    order; one dropped tap, voxel or channel block shows."""
    ref = _ref(case, True, True)
    assert float(ref["SG"].max()) < 2 ** 24 and float(ref["Ss"].max()) < 2 ** 24
    r = _both(_run_wgrad, case, True, True)
    for k in r:
        # (+ 0.0: a float64 sum whose terms are all -0 is +0 on the chip)
        assert _bits_equal(r[k], (ref[k] + 0.0).float()), "%s of %s differs from the float64 reference" % (k, case)


@pytest.mark.parametrize("with_y", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("case", SG.WGRAD_CASES, ids=SG.WGRAD_IDS)
def test_wgrad_float(dev, case, with_y):
    r, ref = _both(_run_wgrad, case, False, with_y), _ref(case, False, with_y)
    n = SG.plan_sl(case)[0]
    bound = (n + 1) * U
    eg = (r["G"].double() - ref["G"]).abs()
    es = (r["gsum"].double() - ref["gsum"]).abs()
    print(case, "chain %d, G: worst error / ((n + 1) u S) = %.3g, gsum: %.3g" % (
        n, float((eg / (bound * ref["SG"]).clamp_min(1e-300)).max()), float((es / (bound * ref["Ss"]).clamp_min(1e-300)).max())))
    assert bool((eg <= bound * ref["SG"]).all()), case
    assert bool((es <= bound * ref["Ss"]).all()), case
    if with_y:
        assert _bits_equal(r["gm"], ref["gm"].float())


def test_misaligned_workspace_launches_nothing(dev):
    case = (2, 2, 3, 5, 12, 5)
    B, D, H, W, Ci, Co = case
    L = _L()
    x, gy, y = SG.wgrad_data(case, False)
    P = Place(dev, True)
    xd, gyd, yd = P.inp(x), P.inp(gy), P.inp(y)
    gm, G, gsum = P.out((B, D, H, W, Co)), P.out((Co, Ci, 3, 3, 3)), P.out((Co,))
    ws, nws = _ws(L, dev, case)
    big = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)

    def call(ws_, n_):
        return L.decnet_conv3d_wgrad(xd.data_ptr(), gyd.data_ptr(), yd.data_ptr(), gm.data_ptr(), G.data_ptr(),
                                     gsum.data_ptr(), ws_, n_, B, D, H, W, Ci, Co, _st())

    assert call(big.data_ptr() + 4, nws + 4) == ERR_MISALIGNED          # an odd float offset
    assert call(ws.data_ptr(), nws - 1) == -2                           # one float short
    P.check_untouched("rejected decnet_conv3d_wgrad")
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(big).all())
    assert call(ws.data_ptr(), nws) == 0                                # and the very same arguments, complete, run
    P.check("accepted decnet_conv3d_wgrad")


# ---- 4. Conv3dFunction on one unit ----------------------------------------------------------------------------------------------
UNITS = {  # name: (Ci, Co, relu, (B, D, H, W))
    "4to16": (4, 16, True, (2, 3, 4, 5)), "36to17": (36, 17, True, (2, 3, 4, 5)), "216to216": (216, 216, True, (2, 3, 4, 5)),
    "216to1_norelu": (216, 1, False, (2, 3, 4, 5)), "4to224": (4, 224, True, (2, 3, 4, 5)),
    "4to16_d9": (4, 16, True, (1, 9, 4, 5)),                   # the F(4,3) depth tiles: 9 = 2 tiles and one plane
}


@pytest.mark.parametrize("name", sorted(UNITS))
def test_function_on_units(dev, name):
    from decnet_amd import Conv3dFunction, ops2d, stage0, stage0_grad
    Ci, Co, relu, dims = UNITS[name]
    B, D, H, W = dims
    g = torch.Generator().manual_seed(Ci * 7 + Co + D)
    x = torch.randn(*dims, Ci, generator=g)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (27 * Ci) ** 0.5
    scale, shift = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
    gy = torch.randn(*dims, Co, generator=g)
    xd, wd, sd, hd = (t.to(dev).requires_grad_() for t in (x, w, scale, shift))
    variant = stage0.WINO_VARIANT.get(stage0.conv_algo(D))
    assert variant is not None
    packed = stage0_grad.unit_operands(wd.detach(), variant, last=(Co == 1))
    kind = packed["kind"]
    assert kind == ("cout1" if Co == 1 else "wino" if Co % 4 == 0 else "direct")
    y = Conv3dFunction.apply(packed, relu, wd, sd, hd, xd)
    # the bits of the no_grad entry call
    with torch.no_grad():
        if kind == "cout1":
            plain = torch.empty(dims, device=dev)
            t = torch.empty(ops2d.size("conv3d_cout1_workspace_floats", *dims), device=dev)
            ops2d.conv3d_cout1_softargmax(xd.detach(), wd.detach(), float(scale[0]), float(shift[0]), dims, Ci, reg=plain, ws=t)
            plain = plain.unsqueeze(-1)
        else:
            plain = torch.empty(dims + (Co,), device=dev)
            ws = None
            if kind == "wino":
                ws = torch.empty(ops2d.size("conv3d_wino_workspace_floats", *dims, Ci, Co, variant), device=dev)
            ops2d.conv3d_bn_act(xd.detach(), packed["w"], sd.detach(), hd.detach(), None, plain, dims, Ci, Co, int(relu), ws,
                                variant if kind == "wino" else None)
    assert _bits_equal(y.detach(), plain), "the forward under autograd is not the no_grad entry's"
    y.backward(gy.to(dev))
    tol = TOL_WINO if kind == "wino" else TOL_DIRECT
    y64 = SG.conv3d_cl(x.double(), w.double()) * scale.double() + shift.double()
    _assert_close(y.detach().cpu(), torch.relu(y64) if relu else y64, tol, (name, "y"))
    # the float64 unit, fed the GPU forward's own y as the mask
    ymask = y.detach().cpu() if relu else None
    G, gsum, gm, SGa, Ss = SG.wgrad(x, gy, ymask)
    n = SG.plan_sl(dims + (Ci, Co))[0]
    s64, w64 = scale.double(), w.double()
    # dW = fp32(s G32): the chain bound on G and one rounding of the product; dscale = fp32(sum w G32 in float64)
    checks = [("dW", wd.grad, s64.view(-1, 1, 1, 1, 1) * G, (n + 2) * U * s64.view(-1, 1, 1, 1, 1) * SGa),
              ("dscale", sd.grad, (w64 * G).sum((1, 2, 3, 4)), (n + 2) * U * (w64.abs() * SGa).sum((1, 2, 3, 4))),
              ("dshift", hd.grad, gsum, (n + 1) * U * Ss)]
    for what, got, ref, bound in checks:
        err = (got.detach().cpu().double() - ref).abs()
        print(name, what, "worst error / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
        assert got.shape == ref.shape and bool((err <= bound).all()), (name, what)
    dx64 = SG.dx(gm, w, scale)
    print(name, "dx (%s): worst error / gate = %.3g" % (
        "wino" if kind == "wino" else "direct",
        float((xd.grad.cpu().double() - dx64).abs().max()) / (tol * max(1.0, float(dx64.abs().max())))))
    _assert_close(xd.grad.cpu(), dx64, TOL_WINO if kind == "wino" else TOL_DIRECT, (name, "dx"))


# ---- 5 - 8. the module ------------------------------------------------------------------------------------------------------------
def _leaves(mod, L, R):
    return {"L": L, "R": R, **dict(mod.named_parameters())}


def _gpu_step(mod, L, R, D, r, r2):
    """(pred r).sum() + (reg r2).sum() through mod.stage0 under hip_grad() -> (pred, reg, [y_i of every unit], entries)."""
    import decnet_amd
    from spy_util import entry_spy
    rec, orig = {}, mod._units_grad

    def spy(x):
        rec["outs"] = orig(x)
        return rec["outs"]
    mod._units_grad = spy
    try:
        with entry_spy() as calls:
            with decnet_amd.hip_grad():
                pred, reg = mod.stage0(L, R, D, return_reg=True)
            ((pred * r).sum() + (reg * r2).sum()).backward()
            torch.cuda.synchronize()
    finally:
        del mod._units_grad
    return pred.detach(), reg.detach(), [o.detach() for o in rec["outs"]], list(calls)


def _on_gpu(name, dev):
    mod, L, R, D, r, r2 = SG.module_case(name)
    modg = copy.deepcopy(mod).to(dev).eval()
    Lg, Rg = (t.to(dev).requires_grad_() for t in (L, R))
    return mod, modg, (L, R, D, r, r2), (Lg, Rg, D, r.to(dev), r2.to(dev))


def _masks_of(outs, mod):
    return [(o > 0).permute(0, 4, 1, 2, 3).cpu() if u.relu else None for o, u in zip(outs, mod.units())]


def _check_grads(name, mod, cpu, masks, got):
    """Every gradient against the float64 run with `masks` imposed; the gate of tests/test_conv2d_mfma_grad_gpu.py:
    max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)), g32 the float32 CPU run under the same masks."""
    r64 = SG.stage0_grads(mod, *cpu, torch.float64, masks)
    r32 = SG.stage0_grads(mod, *cpu, torch.float32, masks)
    assert r64["grads"].keys() == got.keys() and len(got) == 2 + 8 * 3
    for k, ref in r64["grads"].items():
        e_hip = float((got[k].detach().cpu().double() - ref).abs().max())
        e_32 = float((r32["grads"][k].double() - ref).abs().max())
        gate = max(4.0 * e_32, 2e-5 * max(1.0, float(ref.abs().max())))
        print(name, k, "hip %.3g  f32 %.3g  gate %.3g  max|g64| %.3g" % (e_hip, e_32, gate, float(ref.abs().max())))
        assert got[k].shape == ref.shape and e_hip <= gate, (name, k, e_hip, gate)
    return r64, r32


@pytest.mark.parametrize("name", sorted(SG.MODULE_CASES))
def test_module_against_float64(dev, name, monkeypatch):
    import decnet_amd
    mod, modg, cpu, gpu = _on_gpu(name, dev)
    Lg, Rg, D = gpu[:3]
    stats = [(u.bn.running_mean, u.bn.running_var) for u in modg.units()]
    before = [(m.clone(), v.clone(), m._version, v._version) for m, v in stats]
    with torch.no_grad():
        pred_n, reg_n = modg.stage0(Lg, Rg, D, return_reg=True)
    pred, reg, outs, calls = _gpu_step(modg, *gpu)
    assert not [c for c in calls if "_stack_" in c or c.startswith("decnet_stage0_forward")], calls
    assert calls.count("decnet_conv3d_wgrad") == 8, calls
    _pred_ok(pred.cpu(), pred_n.cpu().double(), TOL_STAGE0_PRED, name)
    _assert_close(reg.cpu(), reg_n.cpu().double(), TOL_STAGE0_REG, name)
    monkeypatch.setenv("DECNET_WINO_STACK", "0")
    with torch.no_grad():
        reg_layers = modg(decnet_amd.GetCostVolume("homgrp", modg.cost_func)(Lg.detach(), Rg.detach(), max_disp=D))
    monkeypatch.delenv("DECNET_WINO_STACK")
    assert _bits_equal(reg, reg_layers), "reg under hip_grad() is not the per-layer no_grad forward's"
    got = {k: t.grad for k, t in _leaves(modg, Lg, Rg).items()}
    r64, r32 = _check_grads(name, mod, cpu, _masks_of(outs, modg), got)
    for i, (flips, worst, bound) in enumerate(SG.flips_within_gate(r64, r32, TOL_WINO)):
        print(name, "unit %d: %d imposed decisions differ, worst |pre64| %.3g, gate %.3g" % (i, flips, worst, bound))
        assert worst <= bound, (name, i, flips, worst, bound)
    for (m, v), (m0, v0, mv, vv) in zip(stats, before):
        assert torch.equal(m, m0) and torch.equal(v, v0) and (m._version, v._version) == (mv, vv)
        assert m.grad is None and v.grad is None


def test_eager_and_graph_replays_are_bit_identical(dev):
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    _, modg, _, (Lg, Rg, D, r, r2) = _on_gpu("c8_cor", dev)
    leaves = list(_leaves(modg, Lg, Rg).values())

    def step():
        with decnet_amd.hip_grad():
            pred, reg = modg.stage0(Lg, Rg, D, return_reg=True)
        ((pred * r).sum() + (reg * r2).sum()).backward()

    def eager():
        for p in leaves:
            p.grad = None
        step()
        torch.cuda.synchronize()
        return [p.grad.detach().clone() for p in leaves]

    runs = [eager(), eager()]
    L2 = torch.relu(torch.randn(Lg.shape, generator=torch.Generator().manual_seed(5))).to(dev)
    L1 = Lg.detach().clone()
    with torch.no_grad():
        Lg.copy_(L2)
    new = eager()
    with torch.no_grad():
        Lg.copy_(L1)
    graphed = GraphedStep(step, grads_of=leaves)
    for p in leaves:
        p.grad.fill_(float("nan"))
    graphed()
    torch.cuda.synchronize()
    runs.append([p.grad.detach().clone() for p in leaves])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert _bits_equal(a, b)
    with torch.no_grad():
        Lg.copy_(L2)                                            # the graph reads the tensors it was captured on
    graphed()
    torch.cuda.synchronize()
    assert not all(_bits_equal(a, b) for a, b in zip(runs[0], new)), "the new data changed nothing"
    for a, p in zip(new, leaves):
        assert _bits_equal(a, p.grad)


def test_second_step_sees_the_optimizer_update(dev):
    """Two SGD steps: the forward of the second runs on the updated conv weights AND the updated BatchNorm weights and
    biases (the differentiable scale and shift are formed per call, never read from prepare()'s cache)."""
    import decnet_amd
    mod, modg, _, (Lg, Rg, D, r, r2) = _on_gpu("c8_cor", dev)
    opt = torch.optim.SGD(modg.parameters(), lr=0.05)

    def step(m, L, R):
        with decnet_amd.hip_grad():
            pred, reg = m.stage0(L, R, D, return_reg=True)
        ((pred * r).sum() + (reg * r2).sum()).backward()
        return pred.detach().clone(), reg.detach().clone()

    first = step(modg, Lg, Rg)
    opt.step()
    opt.zero_grad(set_to_none=True)
    Lg.grad = Rg.grad = None
    state = copy.deepcopy(modg.state_dict())
    second = step(modg, Lg, Rg)
    fresh = copy.deepcopy(mod).to(dev).eval()
    fresh.load_state_dict(state)
    Lf, Rf = (t.detach().clone().requires_grad_() for t in (Lg, Rg))
    want = step(fresh, Lf, Rf)
    assert not _bits_equal(first[1], second[1]), "the step changed nothing"
    assert _bits_equal(second[0], want[0]) and _bits_equal(second[1], want[1])
    for (k, p), q in zip(modg.named_parameters(), fresh.parameters()):
        assert _bits_equal(p.grad, q.grad), k
    assert _bits_equal(Lg.grad, Lf.grad) and _bits_equal(Rg.grad, Rf.grad)
    opt.step()
    with torch.no_grad():                                       # and the inference path repacks too
        assert not _bits_equal(modg.stage0(Lg, Rg, D), second[0])


def test_library_arm(dev, monkeypatch):
    from decnet_amd import stage0
    monkeypatch.setattr(stage0, "_conv3d_grad_slower", lambda C, voxels: True)
    mod, modg, cpu, gpu = _on_gpu("c8_cor", dev)
    pred, reg, outs, calls = _gpu_step(modg, *gpu)
    assert "decnet_conv3d_wgrad" not in calls and "decnet_costvol_forward_cf" in calls, calls
    got = {k: t.grad for k, t in _leaves(modg, gpu[0], gpu[1]).items()}
    _check_grads("c8_cor library", mod, cpu, _masks_of(outs, modg), got)
