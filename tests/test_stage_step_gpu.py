"""One training stage end to end on the GPU (tests/_stage_step_ref.py has the step, the two cases and the float64 reference):
DynamicUpsampling -> SpaMatFunction (+ the no_grad SpaVar) -> SoftAttention.fuse -> Refinement -> Loss -> backward ->
optimizer, under hip_grad().  Each module has a test of its own; here the pieces meet.
  a. the step runs on the HIP Functions it is meant to (TALLY, the entries called, the autograd graph): nothing on a torch route;
  b. dense / fused / pred under hip_grad() have the bits of the same composition under no_grad;
  c. every gradient against float64 within the module gate max(4 e32, 2e-5 max(1, max|g64|)) (L and R with the SpaMat
     allowance 5e-5 max|g_sp|), the SpaMat planes held to `_spamat_ref.forward`, every imposed decision within its forward gate.
     Measured (profiles/stage_step_parity.json, tools/stage_step_parity.py): see `parity_ratios`;
  d. a second backward adds into the first one's .grad: exactly gA + gB;
  e. three optimizer steps (SGD momentum, fused Adam, single-tensor Adam behind clip_grad_norm_): the packed-weight caches
     follow the weights -- warm modules against a cold deep copy, forward and backward, bit for bit; on the SGD legs every
     step's gradients against float64 at the GPU's current weights;
  f. a GraphedStep replays the eager bits, and on new data (new masks whose density changes per row included) the bits of
     an eager step on that data.
-m gpu."""
import collections
import contextlib
import copy

import pytest
import torch

import _model_cases as MC
import _stage_step_ref as S
import _tail_grad_ref as TR
from _placement import _bits_equal

pytestmark = pytest.mark.gpu
F32 = torch.float32
U = 2.0 ** -24
K_MAX = 14.0                            # tests/test_spamat_edges_gpu.py: max_cost within K_MAX u max(k_max, |max_cost|)
SPAMAT_ALLOWANCE = 5e-5                 # the project's SpaMat gradient tolerance, x max|g|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- running the step -------------------------------------------------------------------------------------------------------
def _step(mods, t, D, grad=True):
    """The step as a trainer writes it -> the planes (tot included); backward done when grad."""
    import decnet_amd
    with (decnet_amd.hip_grad() if grad else torch.no_grad()):
        out = S.compose(mods, t, D, **S.gpu_slots())
    if grad:
        out["tot"].backward()
    return out


@contextlib.contextmanager
def _relu_masks(mods):
    """Record [y > 0] of every ReLU'd unit while active: units reached through Unit.forward by a hook, the units fuse()
    drives through _forward_grad by wrapping that method on the instance."""
    masks, undo = {}, []
    for name, u in S.relu_units(mods).items():
        def wrapped(x, name=name, real=u._forward_grad):
            y = real(x)
            if y is not None:
                masks[name] = y.detach() > 0
            return y
        u._forward_grad = wrapped
        undo.append((u, u.register_forward_hook(lambda m, i, o, name=name: masks.__setitem__(name, o.detach() > 0))))
    try:
        yield masks
    finally:
        for u, h in undo:
            h.remove()
            del u._forward_grad


def _set_data(t, new):
    with torch.no_grad():
        for k, v in new.items():
            t[k].copy_(v)


def _clear(mods, t):
    for p in list(S.named_parameters(mods).values()) + [t[k] for k in S.LEAVES]:
        p.grad = None


def _full_run(mods, t, D):
    """One step on the GPU modules and data as they are (gradients cleared first) -> everything the reference takes as
    given: the planes, the gradients, the ReLU masks, SpaMat's own three planes from the entry, all on the CPU."""
    from decnet_amd import ops
    _clear(mods, t)
    with _relu_masks(mods) as masks:
        out = _step(mods, t, D)
    o, s, m = (torch.empty_like(t["lmask"]) for _ in range(3))
    ops.spamat_forward(t["L"].detach(), t["R"].detach(), t["lmask"], t["rmask"], o, s, m, D)
    torch.cuda.synchronize()
    assert _bits_equal(o, out["sparse"].detach())
    assert set(masks) == set(S.relu_units(mods))
    return dict(planes={k: v.detach().cpu() for k, v in out.items()}, grads=S.grads_of(mods, t),
                masks={k: v.cpu() for k, v in masks.items()}, spamat=(o.cpu(), s.cpu(), m.cpu()))


def _references(mods, t, D, run):
    """float64 and float32 reference runs at the weights of `mods` (wherever they live) with the GPU run's data imposed."""
    W = t["L"].shape[-1]
    imposed = dict(planes=run["spamat"], var=run["planes"]["var"], masks=run["masks"], cells=S.cells_of(run["planes"]["fused"], W))
    return S.reference(mods, t, D, torch.float64, imposed), S.reference(mods, t, D, F32, imposed)


def _tol_of(case):
    return lambda name: MC.MFMA_TOL if case == "floor" and name.startswith("up.") else MC.FP32_TOL


def _gate_rows(case, run, r64, r32):
    """{tensor: dict(hip_vs_f64, f32_vs_f64, gate, ratio, rel)} and the guards of the imposed decisions."""
    rows = {}
    assert run["grads"].keys() == r64["grads"].keys() == r32["grads"].keys()
    for k, g64 in r64["grads"].items():
        assert run["grads"][k].shape == g64.shape, k
        e, gate = TR.gate(run["grads"][k], g64, r32["grads"][k])
        if k in r64["g_sp"]:
            gate += SPAMAT_ALLOWANCE * float(r64["g_sp"][k].abs().max())
        rows[k] = dict(hip_vs_f64=e, f32_vs_f64=float((r32["grads"][k].double() - g64).abs().max()), gate=gate,
                       ratio=e / gate, rel=e / float(g64.abs().max()))
    flips = S.mask_flips(r64, r32, _tol_of(case))
    cells = S.cell_flips(r64, r32)
    return rows, flips, cells


def _assert_rows(what, rows, flips, cells):
    for k, r in rows.items():
        print("%s %-34s |hip - f64| %.3g  gate %.3g  ratio %.3g  (%.2g of max|g64|)" % (what, k, r["hip_vs_f64"], r["gate"],
                                                                                     r["ratio"], r["rel"]))
    for k, (n, worst, bound) in flips.items():
        if n:
            print("%s %s: %d imposed ReLU decisions differ from float64's, |pre64| <= %.3g, forward gate %.3g" % (what, k, n, worst, bound))
    print("%s warp: %d imposed cells differ, distance to the edge <= %.3g, gate %.3g" % ((what,) + cells))
    for k, (n, worst, bound) in flips.items():
        assert worst <= bound, (what, k, n, worst, bound)
    assert cells[1] <= cells[2], (what, cells)
    for k, r in rows.items():
        assert r["hip_vs_f64"] <= r["gate"], (what, k, r)


_CASE = {}


def _case(case):
    """CPU modules and data, the GPU copies, one full GPU run and its two reference runs -- once per case."""
    if case not in _CASE:
        D = S.CASES[case]["D"]
        mods, t = S.modules(case), S.data(case)
        gm, gt = S.to(mods, t, "cuda:0", F32)
        run = _full_run(gm, gt, D)
        _CASE[case] = dict(D=D, mods=mods, t=t, gmods=gm, gt=gt, run=run, refs=_references(mods, t, D, run))
    return _CASE[case]


def parity_ratios(case):
    """The rows of test c for tools/stage_step_parity.py (profiles/stage_step_parity.json)."""
    c = _case(case)
    rows, flips, cells = _gate_rows(case, c["run"], *c["refs"])
    return dict(tensors=rows, relu_flips={k: dict(zip(("flips", "worst_pre64", "gate"), v)) for k, v in flips.items() if v[0]},
                warp_cell_flips=dict(zip(("flips", "worst_distance", "gate"), cells)))


# ---- a. the step ran where it should ----------------------------------------------------------------------------------------------
TAIL_ENTRIES = {"decnet_unfold3_cat": 1, "decnet_dynamic_upsample3": 1, "decnet_warp_disparity": 1, "decnet_sigmoid_blend": 1,
                "decnet_fold3": 1, "decnet_dynamic_upsample3_backward": 1, "decnet_warp_disparity_backward": 1,
                "decnet_sigmoid_blend_backward": 1, "decnet_spamat_forward": 1, "decnet_spamatvar_forward": 1,
                "decnet_spamat_backward": 1, "decnet_stage_loss_forward": 2, "decnet_stage_loss_backward": 2}
CONV_ENTRIES = {"small": {"decnet_conv2d_bn_act", "decnet_conv2d_cat_bn_act", "decnet_conv2d_wgrad"}}
CONV_ENTRIES["floor"] = CONV_ENTRIES["small"] | {"decnet_conv2d_mfma_cat_bn_act", "decnet_conv2d_mfma_wgrad"}
TORCH_NODES = ("Convolution", "GridSampler", "Softmax", "Sigmoid", "Im2Col", "Col2Im", "Unfold", "PixelShuffle", "ReplicationPad",
               "SmoothL1", "Index", "MaskedSelect")


def _node_names(fn):
    names, seen, todo = [], set(), [fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(n.name())
        todo.extend(f for f, _ in n.next_functions)
    return names


@pytest.mark.parametrize("case", ["small", "floor"])
def test_step_runs_on_the_hip_functions(dev, case):
    import decnet_amd
    from decnet_amd import model
    from spy_util import entry_spy
    c = _case(case)
    mods, t = S.to(c["mods"], c["t"], dev, F32)
    model.TALLY = []
    try:
        with entry_spy() as calls:
            with decnet_amd.hip_grad():
                out = S.compose(mods, t, c["D"], **S.gpu_slots())
            nodes = collections.Counter(_node_names(out["tot"].grad_fn))
            out["tot"].backward()
        tally = collections.Counter(e["family"] for e in model.TALLY)
    finally:
        model.TALLY = None
    torch.cuda.synchronize()
    assert tally == ({"conv_grad": 10, "mfma_grad": 3} if case == "floor" else {"conv_grad": 10, "library": 3}), tally
    calls = [n[:-3] if n.endswith("_ws") else n for n in calls]
    convs = {n for n in calls if "conv2d" in n or "bias_act" in n}
    assert collections.Counter(n for n in calls if n not in convs) == TAIL_ENTRIES, calls
    assert convs == CONV_ENTRIES[case], convs
    # the graph autograd recorded: our Functions, and torch's convolution only for the three library units of `small`
    want = {"Conv2dSmallFunctionBackward": 10, "Conv2dMfmaFunctionBackward": 3 if case == "floor" else 0,
            "Unfold3CatFunctionBackward": 1, "DynamicUpsample3FunctionBackward": 1, "SpaMatFunctionBackward": 1,
            "SigmoidBlendFunctionBackward": 1, "WarpDisparityFunctionBackward": 1, "StageLossFunctionBackward": 2}
    assert {k: nodes[k] for k in want} == want, nodes
    torch_nodes = {k: v for k, v in nodes.items() if k not in want and any(s in k for s in TORCH_NODES)}
    assert torch_nodes == ({} if case == "floor" else {"ConvolutionBackward0": 3}), torch_nodes


# ---- b. forward bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "floor"])
def test_forward_under_hip_grad_is_the_no_grad_forward(dev, case):
    c = _case(case)
    plain = _step(c["gmods"], c["gt"], c["D"], grad=False)
    torch.cuda.synchronize()
    for k in ("dense", "sparse", "var", "fused", "pred"):
        assert _bits_equal(c["run"]["planes"][k], plain[k].cpu()), "%s under hip_grad() differs from its no_grad forward" % k


# ---- c. gradients against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "floor"])
def test_spamat_planes_against_float64(dev, case):
    """What the reference takes as given is right: the project's SpaMat tolerances (tests/test_spamat_edges_gpu.py)."""
    c = _case(case)
    t, run = c["t"], c["run"]
    ref = S.SR.forward(t["L"], t["R"], t["lmask"], t["rmask"], c["D"])
    out, s, mx = (p.double() for p in run["spamat"])
    var = run["planes"]["var"].double()
    for what, got, want, tol in (("out", out, ref["out"], 2e-4 + 1e-5 * ref["out"].abs()), ("S", s, ref["S"], 2e-5 * ref["S"]),
                                 ("var", var, ref["var_self"], 2e-3 + 2e-4 * ref["var_self"].abs()),
                                 ("max_cost", mx, ref["max_cost"], K_MAX * U * torch.maximum(ref["k_max"], ref["max_cost"].abs()))):
        err = (got - want).abs()
        print(case, what, "worst error / tolerance %.3g" % float((err / tol.clamp_min(1e-300)).max()))
        assert bool((err <= tol).all()), what


@pytest.mark.parametrize("case", ["small", "floor"])
def test_gradients_against_float64(dev, case):
    """Measured on the MI355X (profiles/stage_step_parity.json): the worst |hip - f64| / gate is 0.0084 in `small` and 0.010
    in `floor`, both on the bias of Refinement's last unit; the gradients here are those of a mean over the image, so for
    most tensors the gate's floor 2e-5 is the active term -- the rows also print the error as a share of max|g64|, at most
    1.5e-6 (`small`) and 3.9e-6 (`floor`, pred0), and it is at most 7.2 x the float32 CPU run's own distance.  No ReLU
    decision and no warp cell of the GPU runs differed from float64's, so the imposed decisions changed nothing."""
    c = _case(case)
    rows, flips, cells = _gate_rows(case, c["run"], *c["refs"])
    tot64, tot32 = (r["planes"]["tot"] for r in c["refs"])
    assert float((c["run"]["planes"]["tot"].double() - tot64).abs()) <= MC.composite_bound(tot64, tot32, 1.5)
    _assert_rows(case, rows, flips, cells)


# ---- d. accumulation ----------------------------------------------------------------------------------------------------------------
def test_second_backward_adds_into_the_first(dev):
    c = _case("small")
    D = c["D"]
    mods, t = S.to(c["mods"], c["t"], dev, F32)
    A, B = S.data("small"), S.data("small", variant=1)
    alone = []
    for d in (A, B):
        _set_data(t, d)
        _clear(mods, t)
        _step(mods, t, D)
        torch.cuda.synchronize()
        alone.append(S.grads_of(mods, t))
    assert any(not _bits_equal(alone[0][k], alone[1][k]) for k in alone[0])
    _clear(mods, t)
    _set_data(t, A)
    _step(mods, t, D)
    _set_data(t, B)
    _step(mods, t, D)
    torch.cuda.synchronize()
    both = S.grads_of(mods, t)
    for k, g in both.items():
        assert _bits_equal(g, alone[0][k] + alone[1][k]), "%s: .grad after A then B is not gA + gB" % k
    # and the first step's gradients were not disturbed by anything the second one reused
    _clear(mods, t)
    _set_data(t, A)
    _step(mods, t, D)
    torch.cuda.synchronize()
    again = S.grads_of(mods, t)
    for k, g in again.items():
        assert _bits_equal(g, alone[0][k]), k


# ---- e. optimizer steps ---------------------------------------------------------------------------------------------------------------
def _sgd(ps):
    return torch.optim.SGD(ps, lr=0.01, momentum=0.9)


def _adam_fused(ps):
    return torch.optim.Adam(ps, lr=2e-3, fused=True)


def _adam_single(ps):
    return torch.optim.Adam(ps, lr=2e-3, foreach=False)


@pytest.mark.parametrize("case,make,clip,steps", [("small", _sgd, False, 3), ("small", _adam_fused, False, 3),
                                                  ("small", _adam_single, True, 3), ("floor", _sgd, False, 3)],
                         ids=["small-sgd", "small-adam_fused", "small-adam_single_clip", "floor-sgd"])
def test_optimizer_steps_keep_forward_and_backward_on_the_same_weights(dev, case, make, clip, steps):
    c = _case(case)
    D = c["D"]
    mods, t = S.to(c["mods"], c["t"], dev, F32)
    params = list(S.named_parameters(mods).values())
    opt = make(params)
    check64 = make is _sgd
    _clear(mods, t)
    _step(mods, t, D)                                                   # warms every cache at the initial weights
    for i in range(steps):
        before = [p.detach().clone() for p in params]
        if clip:
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params)), "a parameter did not move"
        cold = {k: copy.deepcopy(m) for k, m in mods.items()}           # its caches start cold: it repacks
        tc = {k: v.detach().clone().requires_grad_(k in S.LEAVES) for k, v in t.items()}
        run = _full_run(mods, t, D)                                     # warm: forward under hip_grad(), backward
        plain = _step(mods, t, D, grad=False)
        _clear(cold, tc)
        out_c = _step(cold, tc, D)
        torch.cuda.synchronize()
        g_cold = S.grads_of(cold, tc)
        for k in ("dense", "fused", "pred", "tot"):
            assert _bits_equal(run["planes"][k], out_c[k].detach().cpu()), "step %d: warm %s differs from a cold copy's" % (i, k)
        for k in ("dense", "fused", "pred"):
            assert _bits_equal(run["planes"][k], plain[k].cpu()), "step %d: %s under hip_grad() differs from no_grad" % (i, k)
        for k, g in run["grads"].items():
            assert _bits_equal(g, g_cold[k]), "step %d: gradient of %s differs between warm and cold modules" % (i, k)
        if check64:                                                     # an independent gradient check at these weights
            rows, flips, cells = _gate_rows(case, run, *_references(mods, c["t"], D, run))
            _assert_rows("%s step %d" % (case, i), rows, flips, cells)


# ---- f. one graph, new data -------------------------------------------------------------------------------------------------------------
def test_graph_replays_eager_bits_and_follows_new_data(dev):
    from decnet_amd.graphs import GraphedStep
    c = _case("small")
    D = c["D"]
    mods, t = S.to(c["mods"], c["t"], dev, F32)
    leaves = [t[k] for k in S.LEAVES] + list(S.named_parameters(mods).values())

    def step():
        return _step(mods, t, D)["tot"].detach()

    def eager():
        _clear(mods, t)
        tot = step()
        torch.cuda.synchronize()
        return tot.clone(), S.grads_of(mods, t)

    tot0, g0 = eager()
    new = S.data("small", variant=2, rows=True)
    rows = new["lmask"].mean(2)[0, :4].tolist()
    assert rows[0] == 1.0 and rows[1] == 0.0 and 0 < rows[2] < 0.35 and 0.25 < rows[3] < 0.75, rows
    old = {k: v.detach().clone() for k, v in t.items()}
    _set_data(t, new)
    tot1, g1 = eager()
    assert not _bits_equal(tot1, tot0)
    _set_data(t, old)
    _clear(mods, t)
    graphed = GraphedStep(step, grads_of=leaves)
    for _ in range(3):
        for p in leaves:
            p.grad.fill_(float("nan"))
        tot = graphed()
        torch.cuda.synchronize()
        assert _bits_equal(tot, tot0), "tot: replay differs from eager"
        for k, g in S.grads_of(mods, t).items():
            assert _bits_equal(g, g0[k]), "%s: replay differs from eager" % k
    _set_data(t, new)                                                  # in place: the graph reads the same tensors
    for p in leaves:
        p.grad.fill_(float("nan"))
    tot = graphed()
    torch.cuda.synchronize()
    assert _bits_equal(tot, tot1), "tot: replay on new data differs from an eager step on that data"
    for k, g in S.grads_of(mods, t).items():
        assert _bits_equal(g, g1[k]), "%s: replay on new data differs from an eager step on that data" % k
