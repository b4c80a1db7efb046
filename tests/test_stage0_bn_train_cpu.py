"""Training-mode BatchNorm3d of stage 0 under hip_grad() without a GPU: the train-mode restatement of
tests/_stage0_bn_train_ref.py against torch.nn.BatchNorm3d itself in float64, the channels-last view of the entry
reference, the new names of the C ABI and of ops2d with the host-side refusals and the workspace query, and the refusals
of CostRegNetNoDown in .train() mode on CPU tensors."""
import ctypes
import glob
import os
import re

import pytest
import torch

import _bn_train_ref as BR
import _stage0_bn_train_ref as SB
import _stage0_grad_ref as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("decnet_bn_train_cl_workspace_floats", "decnet_bn_train_cl_forward", "decnet_bn_train_cl_backward")


@pytest.mark.parametrize("name", sorted(SG.MODULE_CASES))
def test_restatement_against_torch_batchnorm3d(name):
    """Outputs, every gradient, running_mean, running_var (torch's: the unbiased variance) and num_batches_tracked after 1
    and after 3 steps, each to 1e-12 of max(1, max|torch's value|) per tensor, in float64."""
    mod, L, R, D, r, r2 = SG.module_case(name)
    for steps in (1, 3):
        mine = SB.stage0_grads_train(mod, L, R, D, r, r2, torch.float64, steps=steps)
        ref = SB.torch_modules_train(mod, L, R, D, r, r2, steps=steps)
        assert mine["grads"].keys() == ref["grads"].keys() and len(ref["grads"]) == 2 + 8 * 3
        assert mine["buffers"].keys() == ref["buffers"].keys() and len(ref["buffers"]) == 8 * 3
        pairs = [("pred", mine["pred"], ref["pred"]), ("reg", mine["reg"], ref["reg"])]
        pairs += [(k, mine["grads"][k], v) for k, v in ref["grads"].items()]
        pairs += [(k, mine["buffers"][k], v) for k, v in ref["buffers"].items()]
        for k, got, want in pairs:
            if k.endswith("num_batches_tracked"):
                assert int(got) == int(want) == steps, k
                continue
            err = float((got - want).abs().max())
            assert got.shape == want.shape and err <= 1e-12 * max(1.0, float(want.abs().max())), (name, steps, k, err)
    # the update is torch's: momentum 0.1 towards the batch mean and the UNBIASED batch variance of the unit's conv output
    one = SB.stage0_grads_train(mod, L, R, D, r, r2, torch.float64, steps=1)
    u0 = mod.units()[0]
    cv = SG.costvol(L.double(), R.double(), D, mod.cost_func).permute(0, 4, 1, 2, 3)
    z = torch.nn.functional.conv3d(cv, u0.conv.weight.detach().double(), None, stride=1, padding=1)
    n = z.numel() // z.shape[1]
    var = z.var((0, 2, 3, 4), unbiased=False)
    want_v = 0.9 * u0.bn.running_var.double() + 0.1 * var * n / (n - 1)
    want_m = 0.9 * u0.bn.running_mean.double() + 0.1 * z.mean((0, 2, 3, 4))
    assert float((one["buffers"]["conv0.0.bn.running_var"] - want_v).abs().max()) <= 1e-12 * float(want_v.abs().max())
    assert float((one["buffers"]["conv0.0.bn.running_mean"] - want_m).abs().max()) <= 1e-12 * max(1.0, float(want_m.abs().max()))


def test_frozen_units_keep_their_buffers_in_the_restatement():
    mod, L, R, D, r, r2 = SG.module_case("c8_cor")
    out = SB.stage0_grads_train(mod, L, R, D, r, r2, torch.float64, steps=2, frozen=(1, 6))
    start = dict(mod.named_buffers())
    names = ["conv0.0", "conv0.1", "conv1.0", "conv1.1", "conv1.2", "conv2.0", "conv2.1", "conv2.2"]
    for i, n in enumerate(names):
        moved = not torch.equal(out["buffers"][n + ".bn.running_mean"], start[n + ".bn.running_mean"].double())
        assert moved == (i not in (1, 6)), n
        assert int(out["buffers"][n + ".bn.num_batches_tracked"]) == (0 if i in (1, 6) else 2), n


def test_channels_last_view_of_the_entry_reference():
    """[rows, C] <-> [1, C, 1, rows]: the same elements, the pivot z[0, c]; the reference on the view is BatchNorm over the
    rows of every column."""
    rows, C = 37, 5
    d = SB.entry_data(rows, C, 1, True)
    z = SB.to_cl(d["z"])
    assert z.shape == (rows, C) and torch.equal(SB.from_cl(z), d["z"]) and torch.equal(z[0], d["z"][0, :, 0, 0])
    f = SB.forward(z, d["gamma"], d["beta"], 1e-5, 0.1, d["running_mean"], d["running_var"], True)
    z64 = z.double()
    assert float((f["mean"] - z64.mean(0)).abs().max()) <= 1e-9
    assert float((f["var"] - z64.var(0, unbiased=False)).abs().max()) <= 1e-9
    g = SB.backward(f, SB.to_cl(d["gy"]), d["gamma"], True)
    assert SB.to_cl(g["gz"]).shape == (rows, C)
    cases = SB.entry_cases()
    assert (SB.ROWS + 1, 260) in cases and max(-(-rows // SB.ROWS) for rows, _ in cases) > SB.FIN_THREADS > SB.FIN_J


def test_new_names_in_the_binding_and_in_ops2d():
    from decnet_amd import _lib, ops2d, stage0_grad
    import decnet_amd
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
    assert callable(ops2d.bn_train_cl_forward) and callable(ops2d.bn_train_cl_backward)
    src = open(os.path.join(ROOT, "include", "decnet_hip.h")).read()
    assert int(re.search(r"#define\s+DECNET_BN_CL_ROWS\s+(\d+)", src).group(1)) == ops2d.BN_CL_ROWS == SB.ROWS
    assert decnet_amd.BatchNorm3dActFunction is stage0_grad.BatchNorm3dActFunction
    # one copy of the pre-activation, in the one kernel file of both layouts, which is built without -fno-honor-nans
    csrc = os.path.join(ROOT, "decnet_amd", "csrc")
    sources = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))
    assert sum(len(re.findall(r"float\s+bn_pre\s*\(", open(f).read())) for f in sources) == 1
    from decnet_amd import build
    assert "batchnorm.hip" not in build.EXTRA_FLAGS
    assert not os.path.exists(os.path.join(csrc, "batchnorm_cl.hip")) and not os.path.exists(os.path.join(csrc, "bn_pre.h"))


@pytest.fixture(scope="module")
def lib():
    from decnet_amd import _lib, build
    h = ctypes.CDLL(build.build())
    for name in NAMES:
        getattr(h, name).argtypes = _lib.SIGNATURES[name]
    h.decnet_bn_train_cl_workspace_floats.restype = ctypes.c_size_t
    return h


def test_workspace_query(lib):
    q = lib.decnet_bn_train_cl_workspace_floats
    for rows, C in SB.entry_cases() + [(23040, 216), (46080, 216), (46080, 1)]:
        nseg = -(-rows // SB.ROWS)
        assert q(rows, C) == 2 * (2 * nseg * C + 2 * C), (rows, C)
    assert q(1, 4) == 0 and q(0, 4) == 0 and q(5, 0) == 0 and q(5, -1) == 0          # rows < 2, C < 1
    assert q(2 ** 31, 1) == 0 and q(2 ** 31 - 1, 1) > 0 and q(2 ** 30, 2) == 0       # rows C >= 2^31 | below
    assert q(2 ** 33, 1) == 0 and q(2 ** 40 + 2, 1) == 0                             # (rows is a size_t: nothing wraps)


def test_refusals_before_any_launch(lib):
    """Argument validation comes before the first HIP call, so it runs without a GPU (the pointers are never read)."""
    NULL, SHAPE, MISALIGNED = -1, -2, -5
    one = 4096
    fwd, bwd, q = lib.decnet_bn_train_cl_forward, lib.decnet_bn_train_cl_backward, lib.decnet_bn_train_cl_workspace_floats
    n = q(70, 3)

    def f(z=one, gamma=one, beta=one, rm=one, rv=one, stats=one, y=one, ws=one, nws=n, dims=(70, 3)):
        return fwd(z, gamma, beta, 1e-5, 0.1, rm, rv, stats, y, 1, ws, nws, *dims, None)

    def b(z=one, gy=one, gamma=one, beta=one, stats=one, dg=one, db=one, ws=one, nws=n, dims=(70, 3)):
        return bwd(z, gy, gamma, beta, stats, None, dg, db, 1, ws, nws, *dims, None)

    assert f(z=None) == NULL and f(gamma=None) == NULL and f(beta=None) == NULL and f(stats=None) == NULL
    assert f(y=None) == NULL and f(ws=None) == NULL
    assert f(rm=None) == NULL and f(rv=None) == NULL                                  # one of the two alone
    assert f(dims=(1, 3)) == SHAPE and f(dims=(70, 0)) == SHAPE                       # rows = 1; C = 0
    assert f(dims=(2 ** 30, 2), nws=1 << 40) == SHAPE                                 # rows C = 2^31
    assert f(nws=n - 1) == SHAPE                                                      # a short workspace
    assert f(ws=one + 4) == MISALIGNED and f(stats=one + 4) == MISALIGNED             # off by 4 bytes
    assert b(z=None) == NULL and b(gy=None) == NULL and b(stats=None) == NULL and b(dg=None) == NULL
    assert b(db=None) == NULL and b(ws=None) == NULL
    assert b(dims=(1, 3)) == SHAPE and b(dims=(70, 0)) == SHAPE and b(nws=n - 1) == SHAPE
    assert b(ws=one + 4) == MISALIGNED and b(stats=one + 4) == MISALIGNED


def test_train_mode_refusals_on_cpu_tensors():
    """The refusals CostRegNetNoDown keeps in .train() mode: CPU tensors with hip_grad() on or off, no_grad, and a module
    whose parameters take no gradient; nothing has touched a buffer.  (tests/test_stage0_grad_cpu.py pins the first.)"""
    import decnet_amd
    mod, L, R, D, _, _ = SG.module_case("c8_cor")
    mod.train()
    before = {k: b.clone() for k, b in mod.named_buffers()}
    Lg = L.clone().requires_grad_()
    for on in (True, False):
        with decnet_amd.hip_grad(on), pytest.raises(NotImplementedError, match="hip_grad"):
            mod.stage0(Lg, R, D)
        with decnet_amd.hip_grad(on), pytest.raises(NotImplementedError, match="hip_grad"):
            mod(torch.zeros(1, 8, 3, 4, 5))
        with decnet_amd.hip_grad(on), torch.no_grad(), pytest.raises(NotImplementedError):
            mod.stage0(L, R, D)
    for k, b in mod.named_buffers():
        assert torch.equal(b, before[k]), k
    assert mod.eval()._grad_mode(L) is False                    # eval mode outside grad: the inference path, as ever


def test_bn_train_refusal_names_the_condition():
    from decnet_amd import stage0_grad
    ok = torch.nn.BatchNorm3d(8)
    assert stage0_grad.bn_train_refusal(ok) is None
    assert "affine" in stage0_grad.bn_train_refusal(torch.nn.BatchNorm3d(8, affine=False))
    assert "track_running_stats" in stage0_grad.bn_train_refusal(torch.nn.BatchNorm3d(8, track_running_stats=False))
    assert "momentum" in stage0_grad.bn_train_refusal(torch.nn.BatchNorm3d(8, momentum=None))
    assert stage0_grad.bn_train_refusal(torch.nn.BatchNorm2d(8, momentum=None)) is not None      # Unit's condition too


def test_routing_sends_nothing_to_the_library_unmeasured():
    from decnet_amd import stage0
    for ci, co in ((8, 8), (216, 216), (216, 1)):
        for voxels in (1, 120, 10 ** 7):
            assert stage0._conv3d_bn_train_slower(ci, co, voxels) is False
