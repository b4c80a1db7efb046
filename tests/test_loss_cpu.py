"""The training loss without a GPU: the torch restatement (tests/_loss_ref.py) against the recorded run of the reference's
own Loss (tests/golden/loss_uploss.npz, made by tests/golden/make_loss_golden.py), the argument checks of the two C entries
(nothing is launched for a rejected call, so they run without a device), and what decnet_amd.Loss refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _loss_ref as R

CASES = sorted(R.GOLDEN_CASES)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "loss_uploss.npz"))


def _same(a, b, rel):
    """a == b to `rel` relative, NaN where b is NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return bool((np.abs(a - b)[ok] <= rel * np.abs(b)[ok]).all())


@pytest.mark.parametrize("case", CASES)
def test_inputs_are_the_recorded_ones(case, golden):
    inp = R.golden_inputs(R.GOLDEN_CASES[case][1])
    assert R.inputs_crc(inp) == int(golden[case + "/inputs_crc"])
    gt = inp["gt"]
    assert 0.25 < float((gt == 0).mean()) < 0.35 and bool((gt > R.GOLDEN_MAX_DISP).any())
    assert all(0.15 < float(m.mean()) < 0.25 or m.size < 100 for m in inp["left_mask"])


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_float64_run(case, golden):
    res = R.restate(case, torch.float64)
    assert _same(res["loss_list"].numpy(), golden[case + "/loss64"], 1e-12)
    assert _same(res["tot"].numpy(), golden[case + "/tot64"], 1e-12)
    for key, g in res["grads"].items():
        # the gradients are stored rounded once to float32 (2^-25 relative)
        assert _same(g.numpy(), golden["%s/g_%s" % (case, key)].astype(np.float64), 2.0 ** -24), key
    # both smooth-L1 branches at every stage: some |d s| below 1 and some above (the predictions sit around the strided pick
    # of gt, which is what bilinear and bicubic give; the pooled ground truths are far from it: the linear branch)
    for kw, _ in res["stages"] if R.GOLDEN_CASES[case][2] in ("bilinear", "bicubic") else []:
        v = R.valid_mask(kw["gt"], kw["gt_max"], kw["skip_rows"])
        if bool(v.any()):
            d = ((kw["pred"].detach() - kw["gt"]) * kw["s"])[v].abs()
            assert bool((d < 1).any()) and bool((d > 1).any())


@pytest.mark.parametrize("case", CASES)
def test_float32_runs_are_within_the_gate(case, golden):
    """The reference's own float32 run and the float32 restatement, against the float64 run."""
    res64 = R.restate(case, torch.float64)
    res32 = R.restate(case, torch.float32)
    gates = R.term_gates(res64)
    for name, got in (("reference", golden[case + "/loss32"]), ("restatement", res32["loss_list"].numpy())):
        R.assert_within(got, res64["loss_list"], torch.tensor(gates), "%s loss_list" % name)
    tg = R.tot_gate(res64, gates)
    R.assert_within(golden[case + "/tot32"], res64["tot"], tg, "reference tot_loss")
    R.assert_within(res32["tot"], res64["tot"], tg, "restatement tot_loss")
    gg = R.grad_gates(res64) if R.GOLDEN_CASES[case][0].endswith("uploss") else R.upsample_grad_gates(res64)
    for key, gate in gg.items():
        R.assert_within(res32["grads"][key], res64["grads"][key], gate, "restatement " + key)
        assert float(golden["%s/g32_maxdiff_%s" % (case, key)]) <= float(gate.max()) or not bool(gate.any()), key


# ---- argument validation of the C entries ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from decnet_amd import _lib, build
    h = ctypes.CDLL(build.build())
    for name in ("decnet_stage_loss_forward", "decnet_stage_loss_backward"):
        getattr(h, name).argtypes = _lib.SIGNATURES[name]
        getattr(h, name).restype = ctypes.c_int
    return h


ONE = 64                                    # a non-NULL pointer value; nothing dereferences it before a rejection
NULL, BAD_SHAPE = -1, -2


def _fwd(lib, planes=(ONE,) * 7, scal=(8.0, 1.0, 0), outs=(ONE,) * 3, dims=(1, 1, 1)):
    return lib.decnet_stage_loss_forward(*planes, *scal, *outs, *dims, None)


def _bwd(lib, planes=(ONE,) * 7, scal=(8.0, 1.0, 0), ins=(ONE, ONE), outs=(ONE,) * 5, dims=(1, 1, 1)):
    return lib.decnet_stage_loss_backward(*planes, *scal, *ins, *outs, *dims, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_entries_reject_bad_arguments_before_any_launch(call, lib):
    for i in (0, 6):                                                 # pred, gt
        assert call(lib, planes=tuple(None if j == i else ONE for j in range(7))) == NULL
    for missing in ((1,), (5,), (1, 2, 3, 4), (2, 3, 4, 5)):         # some but not all of dense .. left_mask
        assert call(lib, planes=tuple(None if j in missing else ONE for j in range(7))) == NULL
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        assert call(lib, dims=dims) == BAD_SHAPE
        assert call(lib, planes=(ONE,) + (None,) * 5 + (ONE,), dims=dims) == BAD_SHAPE
    assert call(lib, dims=(2, 32768, 32768)) == BAD_SHAPE            # B H W = 2^31
    assert call(lib, dims=(1, 46341, 46341)) == BAD_SHAPE            # just above it
    assert call(lib, scal=(8.0, 1.0, -1)) == BAD_SHAPE               # negative skip_rows


def test_entries_reject_missing_outputs(lib):
    for i in range(3):                                               # row_sums, sums, terms
        assert _fwd(lib, outs=tuple(None if j == i else ONE for j in range(3))) == NULL
    for i in range(2):                                               # sums, grad_terms
        assert _bwd(lib, ins=tuple(None if j == i else ONE for j in range(2))) == NULL
    assert _bwd(lib, outs=(None,) * 5) == 0                          # no gradient asked for: nothing to launch


# ---- the module ----------------------------------------------------------------------------------------------------------
def test_loss_refuses_cpu_tensors():
    import decnet_amd
    _, kwargs, ctor = R.case_setup("up_bicubic_plain", torch.float32)
    with pytest.raises(decnet_amd.DecnetHipError):
        decnet_amd.Loss(**ctor)(**kwargs)
    _, kwargs, ctor = R.case_setup("upsample_bilinear", torch.float32)
    with pytest.raises(decnet_amd.DecnetHipError):
        decnet_amd.Loss(**ctor)(**kwargs)


@pytest.mark.parametrize("name", ["chamfer", "LR_consistency", "multi_stage_regression_UpMaskloss"])
def test_loss_names_the_types_it_does_not_implement(name):
    import decnet_amd
    _, kwargs, _ = R.case_setup("up_bicubic_plain", torch.float32)
    with pytest.raises(NotImplementedError, match=name.lower()):
        decnet_amd.Loss(name)(**kwargs)
    with pytest.raises(ValueError):
        decnet_amd.Loss("no_such_loss")


def test_loss_needs_the_soft_masks_for_composite_stages():
    import decnet_amd
    _, kwargs, ctor = R.case_setup("up_bicubic_plain", torch.float32)
    kwargs["sparse_mask_list"] = None
    with pytest.raises(ValueError, match="sparse_mask_list"):
        decnet_amd.Loss(**ctor)(**kwargs)
