"""The training loss on the GPU (csrc/loss.hip through decnet_amd.Loss and through the C ABI) against the recorded run of
the reference's Loss and the float64 torch restatement (tests/_loss_ref.py).  The gates are _loss_ref's: all accumulation
is float64, so only the per-element fp32 roundings remain.  -m gpu."""
import functools
import os

import numpy as np
import pytest
import torch

import _loss_ref as R
from _placement import Place, _L, _bits_equal, _both, _st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(R.GOLDEN_CASES)
FILL = -7777.0                          # pre-fill of outputs that may legitimately hold a NaN
PLANES = ("pred", "dense", "sparse", "fusion", "soft_mask", "left_mask")
GRADS = ("pred", "dense", "sparse", "fusion", "soft_mask")
GRAD_TERMS = (0.7, -1.3, 0.9, 0.4, 1.1)                  # upstream gradients of (dense, sparse, soft mean, fusion, pred)


@functools.lru_cache(maxsize=None)
def _res64(case):
    return R.restate(case, torch.float64)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "loss_uploss.npz"))


def _loss_step(case):
    """-> (leaf tensors on the GPU, a function that runs forward + backward of the objective and returns
    (tot_loss, loss_list stacked))."""
    import decnet_amd
    leaf, kwargs, ctor = R.case_setup(case, torch.float32, DEV)
    loss = decnet_amd.Loss(**ctor)
    n = kwargs["num_stage"]

    def step():
        kw = dict(kwargs, pred_list=list(kwargs["pred_list"][:n]))       # (the upsample loss grows the list it is given)
        _, _, tot, loss_list = loss(**kw)
        R.objective(tot, loss_list).backward()
        return tot.detach(), torch.stack([t.detach() for t in loss_list])
    return leaf, step


# ---- the recorded cases through decnet_amd.Loss ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_loss_matches_the_recorded_reference_run(case, golden):
    res64 = _res64(case)
    leaf, step = _loss_step(case)
    tot, loss_list = step()
    gates = R.term_gates(res64)
    assert loss_list.shape == golden[case + "/loss64"].shape
    print(case, "max term error / gate:", [
        "%.2g/%.2g" % (abs(float(a) - float(b)), g) for a, b, g in zip(loss_list.cpu(), golden[case + "/loss64"], gates)])
    R.assert_within(loss_list, golden[case + "/loss64"], torch.tensor(gates), "loss_list")
    R.assert_within(tot, golden[case + "/tot64"], R.tot_gate(res64, gates), "tot_loss")
    gg = R.grad_gates(res64) if R.GOLDEN_CASES[case][0].endswith("uploss") else R.upsample_grad_gates(res64)
    got = R.leaf_grads(leaf)
    assert set(gg) <= set(got)
    for key in got:
        # the recorded gradient is the float64 one rounded once to float32: 2^-25 |g|, inside the 4 eps |ref64| of the gate;
        # an input that feeds no term (a simple-form stage, the upsample loss) has no gate: its gradient is exactly zero
        R.assert_within(got[key], golden["%s/g_%s" % (case, key)].astype(np.float64), gg.get(key, 0.0), key)


# ---- one level through the C ABI, in guarded windows ---------------------------------------------------------------------------
def _stage_inputs(B, H, W, seed, s=3.0, gt_max=40.0, composite=True):
    """Host float32 planes: gt with 30 % zeros and values above gt_max, predictions around it with noise of sigma 0.3 and
    5 (in units of 1 / s: both smooth-L1 branches), a left mask of 40 % ones, a uniform soft mask."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, H, W, generator=g) * gt_max * 1.1
    gt[torch.rand(B, H, W, generator=g) < 0.3] = 0
    inp = dict(gt=gt)

    def noisy():
        sigma = torch.where(torch.rand(B, H, W, generator=g) < 0.5, 0.3, 5.0)
        return gt + sigma * torch.randn(B, H, W, generator=g) / s
    inp["pred"] = noisy()
    if composite:
        for n in ("dense", "sparse", "fusion"):
            inp[n] = noisy()
        inp["soft_mask"] = torch.rand(B, H, W, generator=g)
        inp["left_mask"] = (torch.rand(B, H, W, generator=g) < 0.4).float()
        if B * H * W < 8:                    # so few pixels: make the first one count for every term
            inp["left_mask"].view(-1)[0] = 1
    if B * H * W < 8:
        gt.view(-1)[0] = 0.5 * gt_max
    return inp


def _stage_abi(inp, gt_max, s, skip_rows, aligned):
    """decnet_stage_loss_forward + _backward on guarded windows -> the outputs on the host."""
    L, P = _L(), Place(DEV, aligned)
    B, H, W = inp["pred"].shape
    dev = [P.inp(inp[n]).data_ptr() if inp.get(n) is not None else None for n in PLANES]
    planes = dev + [P.inp(inp["gt"]).data_ptr()]
    # (a NaN is a legitimate value of every output here, so the pre-fill is FILL and "written" is checked below)
    row_sums = P.inplace(torch.full((B * H, 8), FILL, dtype=torch.float64))
    sums = P.inplace(torch.full((8,), FILL, dtype=torch.float64))
    terms = P.inplace(torch.full((5,), FILL))
    grad_terms = P.inp(torch.tensor(GRAD_TERMS))
    rc = L.decnet_stage_loss_forward(*planes, gt_max, s, skip_rows, row_sums.data_ptr(), sums.data_ptr(), terms.data_ptr(),
                                     B, H, W, _st())
    assert rc == 0, rc
    # every gradient plane, also those of the terms the simple form does not have (they are written as zeros)
    grads = {n: P.inplace(torch.full((B, H, W), FILL)) for n in GRADS}
    rc = L.decnet_stage_loss_backward(*planes, gt_max, s, skip_rows, sums.data_ptr(), grad_terms.data_ptr(),
                                      *[grads[n].data_ptr() for n in GRADS], B, H, W, _st())
    assert rc == 0, rc
    P.check("stage loss %s aligned=%s" % ((B, H, W), aligned))
    out = dict(terms=terms.cpu(), sums=sums.cpu(), row_sums=row_sums.cpu(), **{"g_" + n: grads[n].cpu() for n in GRADS})
    for k, v in out.items():
        assert bool((v != FILL).all()), "%s: output element not written" % k
    return out


def _stage_ref(inp, gt_max, s, skip_rows):
    """The float64 restatement of one level -> (terms64 [5], {g_name: plane}, term gates [5], {g_name: gate plane})."""
    x = {n: (v.double().requires_grad_(n in GRADS) if v is not None else None) for n, v in inp.items()}
    kw = dict(pred=x["pred"], gt=x["gt"], gt_max=gt_max, s=s, skip_rows=skip_rows)
    if inp.get("dense") is not None:
        kw.update({n: x[n] for n in PLANES[1:]})
    terms = R.stage_terms(**kw)
    scale = R.term_scale(**{k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    valid = R.valid_mask(x["gt"], gt_max, skip_rows)
    grads, ggates = {}, {}
    for k, n in enumerate(R.TERM_NAMES):
        if x.get(n) is None:
            grads["g_" + n] = torch.zeros_like(x["pred"]).detach()
            ggates["g_" + n] = torch.zeros_like(grads["g_" + n])
            continue
        g = GRAD_TERMS[k] * torch.autograd.grad(terms[k], x[n], retain_graph=True)[0]
        grads["g_" + n] = g
        if n == "soft_mask":
            ggates["g_" + n] = 4 * R.EPS * g.abs()
            continue
        cnt = int((valid & (x["left_mask"] == 1)).sum()) if n == "sparse" else int(valid.sum())
        coef = abs(GRAD_TERMS[k]) * s / cnt if cnt else 0.0
        ggates["g_" + n] = coef * 4 * R.EPS * scale[k] + 4 * R.EPS * g.abs()
    t64 = torch.stack([t.detach() for t in terms])
    tgates = torch.tensor([R.term_gate(scale[k], float(t64[k])) if float(t64[k]) == float(t64[k]) else 0.0
                           for k in range(5)])
    return t64, grads, tgates, ggates


def _check_stage(inp, gt_max, s, skip_rows):
    got = _both(lambda aligned: _stage_abi(inp, gt_max, s, skip_rows, aligned))
    t64, grads, tgates, ggates = _stage_ref(inp, gt_max, s, skip_rows)
    R.assert_within(got["terms"], t64, tgates, "terms")
    for k in grads:
        R.assert_within(got[k], grads[k], ggates[k], k)
    # the totals are those of the restatement's masks, exactly
    valid = R.valid_mask(inp["gt"], gt_max, skip_rows)
    assert float(got["sums"][0]) == float(valid.sum())
    if inp.get("left_mask") is not None:
        left = inp["left_mask"] == 1
        assert float(got["sums"][1]) == float((valid & left).sum()) and float(got["sums"][2]) == float(left.sum())
    return got, t64


# (1, 33001, 3): more rows than a launch has waves (8192 workgroups of 4): the grid-stride path
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 3), (2, 5, 63), (2, 5, 64), (2, 5, 65), (1, 7, 257), (3, 20, 36),
                                   (1, 33001, 3)])
def test_composite_level_at_edge_shapes(shape):
    B, H, W = shape
    inp = _stage_inputs(B, H, W, seed=B * 100000 + H * 1000 + W)
    _check_stage(inp, 40.0, 3.0, skip_rows=H // 3)


def test_simple_level():
    inp = _stage_inputs(2, 5, 65, seed=65, composite=False)
    got, t64 = _check_stage(inp, 40.0, 3.0, skip_rows=1)
    assert [float(v) for v in got["terms"][:4]] == [0.0] * 4 and float(got["terms"][4]) > 0
    for n in GRADS[1:]:
        assert not bool(got["g_" + n].any())


EMPTY = {"gt_all_zero": (R.TERM_NAMES.index("dense"), R.TERM_NAMES.index("sparse"), R.TERM_NAMES.index("fusion"),
                         R.TERM_NAMES.index("pred")),
         "skip_rows_past_H": (0, 1, 3, 4),
         "left_mask_all_zero": (R.TERM_NAMES.index("sparse"), R.TERM_NAMES.index("soft_mask"))}


@pytest.mark.parametrize("which", sorted(EMPTY))
def test_empty_sets_give_nan_terms_and_zero_gradients(which):
    inp = _stage_inputs(2, 5, 65, seed=7)
    skip = 0
    if which == "gt_all_zero":
        inp["gt"] = torch.zeros_like(inp["gt"])
    elif which == "skip_rows_past_H":
        skip = 5
    else:
        inp["left_mask"] = torch.zeros_like(inp["left_mask"])
    got, t64 = _check_stage(inp, 40.0, 3.0, skip)
    for k, n in enumerate(R.TERM_NAMES):
        if k in EMPTY[which]:
            assert bool(torch.isnan(got["terms"][k])), n
            assert not bool(got["g_" + n].any()), "g_%s of an empty term must be all zeros" % n
        else:
            assert bool(torch.isfinite(got["terms"][k])), n
            assert bool(got["g_" + n].any()), n
    _check_stage(inp, 40.0, 3.0, skip + 6)                       # skip_rows > H: the same as == H, no row is touched


def test_nan_outside_the_mask_changes_nothing_inside_it_reaches_the_term():
    inp = _stage_inputs(2, 5, 65, seed=11)
    flat_gt = inp["gt"].view(-1)
    off = int((flat_gt == 0).nonzero()[3])                        # a pixel without ground truth
    on = int(((flat_gt > 0) & (flat_gt < 40.0) & (inp["left_mask"].view(-1) == 0)).nonzero()[3])     # valid, not `whole`
    base = _both(lambda aligned: _stage_abi(inp, 40.0, 3.0, 0, aligned))
    poisoned = {k: v.clone() for k, v in inp.items()}
    for n in ("pred", "dense", "sparse", "fusion"):
        poisoned[n].view(-1)[off] = float("nan")
    poisoned["sparse"].view(-1)[on] = float("nan")                # valid, but outside the sparse term's own mask
    got = _both(lambda aligned: _stage_abi(poisoned, 40.0, 3.0, 0, aligned))
    for k in base:
        assert _bits_equal(base[k], got[k]), "%s changed with a NaN outside the masks" % k
    poisoned["pred"].view(-1)[on] = float("nan")
    got = _both(lambda aligned: _stage_abi(poisoned, 40.0, 3.0, 0, aligned))
    assert bool(torch.isnan(got["terms"][4])) and bool(torch.isfinite(got["terms"][:4]).all())
    for k in base:
        if k not in ("terms", "sums", "row_sums", "g_pred"):
            assert _bits_equal(base[k], got[k]), k


def test_rejected_calls_write_nothing():
    L = _L()
    inp = _stage_inputs(2, 5, 65, seed=3)
    for aligned in (True, False):
        P = Place(DEV, aligned)
        planes = [P.inp(inp[n]).data_ptr() for n in PLANES] + [P.inp(inp["gt"]).data_ptr()]
        row_sums, sums, terms = P.out((10, 8), torch.float64), P.out((8,), torch.float64), P.out((5,))
        grads = [P.out((2, 5, 65)).data_ptr() for _ in GRADS]
        fo = (row_sums.data_ptr(), sums.data_ptr(), terms.data_ptr())
        gin = (P.inp(torch.ones(8, dtype=torch.float64)).data_ptr(), P.inp(torch.tensor(GRAD_TERMS)).data_ptr())
        partial = planes[:2] + [None] + planes[3:]
        for pl, skip, dims, rc in ((planes, -1, (2, 5, 65), -2), (partial, 0, (2, 5, 65), -1), (planes, 0, (2, 0, 65), -2),
                                   (planes, 0, (2, 5, -65), -2), (planes, 0, (2, 32768, 32768), -2),
                                   ([None] + planes[1:], 0, (2, 5, 65), -1), (planes[:6] + [None], 0, (2, 5, 65), -1)):
            assert L.decnet_stage_loss_forward(*pl, 40.0, 3.0, skip, *fo, *dims, _st()) == rc
            assert L.decnet_stage_loss_backward(*pl, 40.0, 3.0, skip, *gin, *grads, *dims, _st()) == rc
        assert L.decnet_stage_loss_forward(*planes, 40.0, 3.0, 0, fo[0], None, fo[2], 2, 5, 65, _st()) == -1
        assert L.decnet_stage_loss_backward(*planes, 40.0, 3.0, 0, gin[0], None, *grads, 2, 5, 65, _st()) == -1
        P.check_untouched("rejected stage-loss calls")


# ---- determinism, capture, no host synchronisation ---------------------------------------------------------------------------
def _snapshot(leaf, result):
    out = {"tot": result[0].clone(), "loss_list": result[1].clone()}
    out.update({k: v.clone() for k, v in R.leaf_grads(leaf).items()})
    return out


def _reset(leaf):
    for ts in leaf.values():
        for t in ts:
            t.grad = None


def test_two_eager_calls_agree_bit_for_bit():
    leaf, step = _loss_step("up_bicubic_over")
    a = _snapshot(leaf, step())
    _reset(leaf)
    b = _snapshot(leaf, step())
    for k in a:
        assert _bits_equal(a[k], b[k]), k


def test_graph_replay_equals_eager_bit_for_bit():
    from decnet_amd.graphs import GraphedStep
    leaf, step = _loss_step("up_bicubic_plain")
    eager = _snapshot(leaf, step())
    torch.cuda.synchronize()
    graphed = GraphedStep(step, grads_of=[t for ts in leaf.values() for t in ts])
    for _ in range(3):
        for ts in leaf.values():
            for t in ts:
                t.grad.fill_(float("nan"))
        replay = _snapshot(leaf, graphed())
        torch.cuda.synchronize()
        for k in eager:
            assert _bits_equal(eager[k], replay[k]), "%s: replay differs from eager" % k


def test_eager_loss_never_synchronises_with_the_host():
    leaf, step = _loss_step("up_bicubic_over")
    step()                                           # first call: library load, allocator growth
    _reset(leaf)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaf["pred"])


# ---- a training step that ends at the loss, as one graph ---------------------------------------------------------------------
def test_spamat_into_loss_is_one_graph_and_matches_the_torch_loss():
    """SpaMatFunction -> a composite stage of Loss -> backward, captured whole: the test a torch-written loss cannot pass
    (its boolean gathers read back to the host).  The feature gradients agree with the same step under the torch
    restatement within the project's SpaMat gradient tolerance, 5e-5 max |g|."""
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    B, C, H, W, D, S = 1, 24, 18, 27, 24, 3
    g = torch.Generator().manual_seed(1827)
    L = torch.relu(torch.randn(B, C, H, W, generator=g)).to(DEV).requires_grad_()
    Rf = torch.relu(torch.randn(B, C, H, W, generator=g)).to(DEV).requires_grad_()
    rm = (torch.rand(B, H, W, generator=g) < 0.5).float().to(DEV)
    tm = (torch.rand(B, H, W, generator=g) < 0.5).float().to(DEV)
    gt = torch.rand(B, H, W, generator=g) * D * 1.1
    gt[torch.rand(B, H, W, generator=g) < 0.3] = 0
    coarse = gt[:, S // 2::S, S // 2::S] / S
    pred0 = (coarse + torch.randn(coarse.shape, generator=g)).to(DEV)
    full = [(gt + 2 * torch.randn(B, H, W, generator=g)).to(DEV) for _ in range(3)]            # pred, dense, fusion
    soft = torch.rand(B, H, W, generator=g).to(DEV)
    gt = gt.to(DEV)
    weights = [0.5, 1.0]
    loss = decnet_amd.Loss("multi_stage_regression_uploss")

    def kwargs(sparse):
        return dict(pred_list=[pred0, full[0]], fusion_list=[full[2]], dense_list=[full[1]], sparse_list=[sparse],
                    left_mask_list=[rm], gt=gt, weights=weights, num_stage=2, down_func_name="bicubic", down_scale=S,
                    max_disp=D, sparse_mask_list=[soft])

    def fused():
        tot = loss(**kwargs(decnet_amd.SpaMatFunction.apply(L, Rf, rm, tm, D)))[2]
        tot.backward()
        return tot.detach()

    def composed():
        kw = kwargs(decnet_amd.SpaMatFunction.apply(L, Rf, rm, tm, D))
        tot = R.uploss(kw["pred_list"], kw["fusion_list"], kw["dense_list"], kw["sparse_list"], kw["left_mask_list"], gt,
                       weights, 2, "bicubic", S, D, kw["sparse_mask_list"])[1]
        tot.backward()
        return tot.detach()

    def run(fn):
        L.grad = Rf.grad = None
        tot = fn()
        torch.cuda.synchronize()
        return tot.clone(), L.grad.clone(), Rf.grad.clone()
    want = run(composed)
    eager = run(fused)
    assert float(want[1].abs().max()) > 0 and float(want[2].abs().max()) > 0
    for got, ref, name in zip(eager[1:], want[1:], ("grad_ref_feas", "grad_tar_feas")):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(name, "max error %.3g, 5e-5 max|g| = %.3g" % (err, 5e-5 * scale))
        assert err <= 5e-5 * scale, name
    graphed = GraphedStep(fused, grads_of=[L, Rf])
    for _ in range(3):
        L.grad.fill_(float("nan"))
        Rf.grad.fill_(float("nan"))
        tot = graphed()
        torch.cuda.synchronize()
        for got, ref, name in zip((tot, L.grad, Rf.grad), eager, ("tot_loss", "grad_ref_feas", "grad_tar_feas")):
            assert _bits_equal(got, ref), "%s: replay differs from eager" % name
