"""tests/_model_ref.py (float64 references of the composite modules, written from the reference's formulas) against
(a) each module's own torch route on the CPU in float64 (``copy.deepcopy(module).double()``) and (b) the committed goldens
of the reference graph (tests/golden/e2e_bc2_54x243*.npz: its masks, per-stage sparse results and final disparity).
Also asserts, per mask case of tests/_model_cases.py, that the float64 reference alone leaves at most 1 % of the pixels
within the close-call margin of the threshold -- the cap the GPU tests may exclude.  No GPU."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import _model_cases as MC  # noqa: E402
import _model_ref as MR  # noqa: E402

TOL = 1e-11                # float64 against float64, different summation order


def _close(got, ref):
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= TOL * max(1.0, float(ref.abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("kw", [dict(cin=5, cout=7, k=3), dict(cin=5, cout=7, k=3, dil=3, relu=False),
                                dict(cin=4, cout=3, k=1, bn=False), dict(cin=4, cout=3, k=3, bn=False, bias=False),
                                dict(cin=6, cout=5, k=3, stride=3), dict(cin=6, cout=5, k=3, stride=3, transposed=True),
                                dict(cin=6, cout=5, k=3, stride=3, transposed=True, bn=False, relu=False)],
                         ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()))
def test_unit(kw):
    u = MC.make_unit(seed=3, **kw)
    xs = (torch.randn(2, kw["cin"] - 1, 10, 11, generator=_gen(1)), torch.randn(2, 1, 10, 11, generator=_gen(2)))
    with torch.no_grad():
        want = copy.deepcopy(u).double()(torch.cat(xs, 1).double())
    _close(MR.unit(xs, MR.unit_params(u)), want)
    _close(MR.unit(torch.cat(xs, 1), MR.unit_params(u)), want)


def test_upblock_and_aspp():
    from decnet_amd.model import ASPP, UpBlock
    m = MC.seeded(lambda: UpBlock(6, 4), 5)
    x, skip = torch.randn(2, 6, 4, 5, generator=_gen(3)), torch.randn(2, 4, 12, 15, generator=_gen(4))
    with torch.no_grad():
        want, want_up = copy.deepcopy(m).double()(skip.double(), x.double())
    got, up = MR.upblock(skip, x, MR.upblock_params(m))
    _close(got, want)
    _close(up, want_up)
    for rates, relu in (([4, 8, 12], True), ([1, 2, 3, 5], True), ([2, 3], False)):
        a = MC.seeded(lambda: ASPP(8, 6, rates), 6)
        list(a.stages.children())[1].relu = relu
        x = torch.randn(2, 8, 9, 14, generator=_gen(5))
        with torch.no_grad():
            want = copy.deepcopy(a).double()(x.double())
        assert want.shape[1] == 6 * (len(rates) + 1)
        _close(MR.aspp(x, MR.aspp_params(a)), want)


def test_feature_extractor():
    from decnet_amd.model import FeatExtNetChannelPlus
    m = MC.seeded(lambda: FeatExtNetChannelPlus(2), 7)
    x = torch.randn(2, 3, 27, 54, generator=_gen(6))
    with torch.no_grad():
        want = copy.deepcopy(m).double()(x.double())
    got = MR.featext(x, MR.featext_params(m))
    assert sorted(got) == sorted(want) == ["stage0", "stage1", "stage2", "stage3"]
    for k in want:
        _close(got[k], want[k])


@pytest.mark.parametrize("H,W", MC.MASK_CASES)
def test_mask_generator_and_its_close_call_cap(H, W):
    gen, cur, pre, thold = MC.mask_case(H, W)
    with torch.no_grad():
        g64 = copy.deepcopy(gen).double()
        want_logit = g64(cur.double(), pre.double())
        want = g64.mask(cur.double(), pre.double(), thold)
    m, logit = MR.mask(cur, pre, MR.maskgen_params(gen), thold)
    _close(logit, want_logit)
    assert torch.equal(m, want.bool())
    assert 0 < int(m.sum()) < m.numel()                     # the case really has both values
    # the cap: with the loosest bound any leg of the GPU test uses (factor 1.5) the reference leaves <= 1 % undecided
    unsure = MR.mask_unsure(logit, thold, MC.mask_margin(gen, cur, pre, logit, 1.5))
    print("mask %dx%d: thold %.4f, %d of %d pixels within the margin" % (H, W, thold, int(unsure.sum()), unsure.numel()))
    assert float(unsure.double().mean()) <= 0.01


def test_dynamic_upsampling_fuse_warp_refinement():
    from decnet_amd.model import DynamicUpsampling, Refinement, SoftAttention, warp_by_disparity
    g = _gen(8)
    du = MC.seeded(lambda: DynamicUpsampling(2, 3), 9)
    for h, w in ((5, 7), (1, 4), (4, 1)):
        disp, fea = torch.rand(2, h, w, generator=g) * 20, torch.randn(2, 2, 3 * h, 3 * w, generator=g)
        with torch.no_grad():
            want = copy.deepcopy(du).double()(disp.double(), fea.double())
        _close(MR.dynamic_upsampling(disp, fea, MR.seq_params(du.weight_learning)), want)

    sa = MC.seeded(lambda: SoftAttention(6 + 4, 4), 10)
    B, H, W = 2, 9, 12
    fea, dense, sparse = torch.randn(B, 6, H, W, generator=g), torch.rand(B, H, W, generator=g) * 30, \
        torch.rand(B, H, W, generator=g) * 30
    lmask, var = (torch.rand(B, H, W, generator=g) < 0.5).float(), torch.rand(B, H, W, generator=g)
    with torch.no_grad():
        want = copy.deepcopy(sa).double().fuse(fea.double(), dense.double(), sparse.double(), lmask.double(), var.double())
    _close(MR.fuse(fea, dense, sparse, lmask, var, MR.seq_params(sa.conv)), want)

    right = torch.randn(B, 5, H, W, generator=g)
    disps = [torch.rand(B, H, W, generator=g) * 3 * W - W, torch.randint(-3, W + 3, (B, H, W), generator=g).float()]
    for disp in disps:
        with torch.no_grad():
            want = warp_by_disparity(right.double(), disp.double())
        got = MR.warp(right, disp)
        assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))   # grid_sample's own chain

    for stage_id in (0, 1, 2, 3):
        for c in (6, 5):                                    # 5: an odd half
            rf = MC.seeded(lambda: Refinement(c, 4, stage_id), 11 + stage_id)
            rf.conv[-1].conv.bias.data.normal_(0, 0.3)
            left, right = torch.randn(B, c, 20, 21, generator=g), torch.randn(B, c, 20, 21, generator=g)
            disp = torch.rand(B, 20, 21, generator=g) * 10
            with torch.no_grad():
                want, res = copy.deepcopy(rf).double()(left.double(), right.double(), disp.double())
            got = MR.refinement(left, right, disp, MR.seq_params(rf.conv))
            assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("cost_func", ["cor", "ssd", "cat"])
def test_masks_of_the_reference_graph(cost_func):
    """The reference graph's own (float32) masks, recorded in the e2e goldens: the float64 feature extractor + mask
    references must reproduce every pixel whose float64 decision is not a close call for float32; the margin is the
    composite yardstick on this repo's float32 torch route (1.5 x its distance to float64), through the sigmoid's slope."""
    from make_golden import E2E_KW, e2e_inputs
    from netparams import fill_state_dict
    from decnet_amd.model import get_model, load_reference_checkpoint
    d = np.load(os.path.join(HERE, "golden", "e2e_bc2_54x243%s.npz" % ("" if cost_func == "cor" else "_" + cost_func)))
    model = get_model(**dict(E2E_KW, cost_func=cost_func))
    load_reference_checkpoint(model, fill_state_dict(model.state_dict())).eval()
    left, _ = e2e_inputs()
    f64 = MR.featext(left, MR.featext_params(model.feature_extractor))
    with torch.no_grad():
        f32 = model.feature_extractor(left)
    for st in (1, 2, 3):
        gen = model.detail_detection[st - 1]
        m, logit = MR.mask(f64["stage%d" % st], f64["stage%d" % (st - 1)], MR.maskgen_params(gen), model.thold)
        with torch.no_grad():
            l32 = gen(f32["stage%d" % st], f32["stage%d" % (st - 1)])
        unsure = MR.mask_unsure(logit, model.thold, MC.composite_bound(logit, l32, 1.5))
        gold = torch.from_numpy(d["lmask%d" % st]) != 0
        assert gold.shape == m.shape
        flips = (gold != m)
        print("stage %d: %d flips, %d close calls of %d" % (st, int(flips.sum()), int(unsure.sum()), m.numel()))
        assert not bool((flips & ~unsure).any())
        assert float(unsure.double().mean()) <= 0.01


@pytest.mark.parametrize("cost_func", ["cor", "ssd", "cat"])
def test_final_prediction_of_the_reference_graph(cost_func):
    """The references chained into the stage loop (SparseDenseNetRefinementMask.py:127-207) against the final disparity
    and the per-stage sparse results the reference graph recorded in the e2e goldens.  Stage 0 is oracle/stage0.py in
    float64; SpaMat / SpaVar are oracle/spamat_oracle.c on float32 copies, exactly what stood in for the compiled ops when
    the goldens were made (tests/golden/make_golden.py).  Gates: those of tests/test_model_gpu.py for the same goldens
    (mean |difference| below 1e-3 px); no mask bit differs here (test_masks_of_the_reference_graph), so every pixel counts."""
    import oracle
    from oracle import stage0 as o0
    from make_golden import E2E_KW, e2e_inputs
    from netparams import fill_state_dict
    from decnet_amd.model import get_model, load_reference_checkpoint
    oracle.build()
    d = np.load(os.path.join(HERE, "golden", "e2e_bc2_54x243%s.npz" % ("" if cost_func == "cor" else "_" + cost_func)))
    model = get_model(**dict(E2E_KW, cost_func=cost_func))
    load_reference_checkpoint(model, fill_state_dict(model.state_dict())).eval()
    left, right = e2e_inputs()
    fp = MR.featext_params(model.feature_extractor)
    lf, rf = MR.featext(left, fp), MR.featext(right, fp)
    reg = model.cost_regularizer
    params = [{"w": p["w"].double(), "bn": tuple(t.double() for t in p["bn"])} for p in o0.params_from_module(reg)]
    w_pre = reg.conv_pre.weight.detach().double() if cost_func == "cat" else None
    pred, _, _ = o0.stage0_forward(lf["stage0"], rf["stage0"], params, model.max_disp // 27, cost_func, w_pre)
    for st in (1, 2, 3):
        L, R = lf["stage%d" % st], rf["stage%d" % st]
        dense = MR.dynamic_upsampling(pred, L, MR.seq_params(model.dynamic_upsampling[st - 1].weight_learning))
        mp = MR.maskgen_params(model.detail_detection[st - 1])
        lm, _ = MR.mask(L, lf["stage%d" % (st - 1)], mp, model.thold)
        rm, _ = MR.mask(R, rf["stage%d" % (st - 1)], mp, model.thold)
        assert np.array_equal(lm.numpy(), d["lmask%d" % st] != 0)
        D = model.max_disp // 3 ** (3 - st)
        f = lambda t: t.float()
        sp, _, _ = oracle.spamat_forward(f(L), f(R), f(lm), f(rm), D)
        var, _, _ = oracle.spavar_forward(f(L), f(R), f(lm), f(rm), torch.from_numpy(sp), D)
        on = lm.numpy()
        assert np.abs(sp - d["sparse%d" % st])[on].mean() < 1e-3, st
        fused = MR.fuse(L, dense, torch.from_numpy(sp), lm.double(), torch.from_numpy(var),
                        MR.seq_params(model.soft_attention[st - 1].conv))
        pred = MR.refinement(L, R, fused, MR.seq_params(model.refinement[st - 1].conv))
    err = (pred - torch.from_numpy(d["pred"]).double()).abs()
    print("%s: final disparity mean |difference| %.2e px, max %.2e" % (cost_func, float(err.mean()), float(err.max())))
    assert pred.shape == d["pred"].shape
    assert float(err.mean()) < 1e-3
