"""The stage-0 backward without a GPU: the float64 reference of tests/_stage0_grad_ref.py against free autograd, finite
differences and tests/_stage0_ref.py; the flipped weights of the dx convolution; the partition decnet_conv3d_wgrad states in
include/decnet_hip.h against its workspace query; its host-side refusals through ctypes (nothing can launch: there is no
device); and the refusals of CostRegNetNoDown outside ``hip_grad()``."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _stage0_grad_ref as SG
import _stage0_ref as S0

F64 = torch.float64
ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_MISALIGNED = -1, -2, -3, -5


@pytest.fixture(scope="module")
def lib():
    from decnet_amd import _lib
    return _lib.lib()


def test_costvol_restatements_agree():
    """The grid_sample form of the helper and the matrix form of decnet_amd.stage0_grad equal tests/_stage0_ref.costvol."""
    from decnet_amd.stage0_grad import costvol_torch
    g = torch.Generator().manual_seed(5)
    L, R = torch.randn(2, 3, 4, 7, generator=g, dtype=F64), torch.randn(2, 3, 4, 7, generator=g, dtype=F64)
    for cf in ("cor", "ssd"):
        ref = S0.costvol(L, R, 5, cf)
        assert float((SG.costvol(L, R, 5, cf) - ref).abs().max()) < 1e-12
        # (the interpolation weights of the package's form are built in float32, as the kernel builds its own)
        assert float((costvol_torch(L, R, 5, cf) - ref).abs().max()) < 2e-6 * float(ref.abs().max())
    with pytest.raises(NotImplementedError, match="cat"):
        costvol_torch(L, R, 5, "cat")


def test_masked_reference_equals_free_autograd():
    mod, L, R, D, r, r2 = SG.module_case("c8_cor")
    free = SG.stage0_grads(mod, L, R, D, r, r2, F64)
    again = SG.stage0_grads(mod, L, R, D, r, r2, F64, masks=free["took"])
    assert free["grads"].keys() == again["grads"].keys() and len(free["grads"]) == 2 + 8 * 3
    for k, g in free["grads"].items():
        assert torch.equal(g, again["grads"][k]), k
    assert float(max(g.abs().max() for g in free["grads"].values())) > 0
    # and the forward is tests/_stage0_ref.stage0 on the same parameters
    m64 = copy.deepcopy(mod).double()
    params = [(u.conv.weight.detach(),) + S0.fold_bn((u.bn.weight.detach(), u.bn.bias.detach(), u.bn.running_mean,
                                                      u.bn.running_var)) for u in m64.units()]
    reg, pred = S0.stage0(L, R, params, D, "cor")
    assert float((free["reg"] - reg).abs().max()) < 1e-10 and float((free["pred"] - pred).abs().max()) < 1e-10


def test_masked_reference_against_finite_differences():
    """C = 4: with the masks held fixed the loss is smooth, so central differences of the masked forward are its gradient."""
    from decnet_amd import CostRegNetNoDown
    import _model_cases as MC
    mod = MC.seeded(lambda: CostRegNetNoDown(4, 8, "ssd"), 77).double()
    g = torch.Generator().manual_seed(78)
    L, R = (torch.relu(torch.randn(1, 4, 3, 4, generator=g, dtype=F64)) for _ in range(2))
    D, r, r2 = 3, torch.randn(1, 3, 4, generator=g, dtype=F64), torch.randn(1, 3, 3, 4, generator=g, dtype=F64)
    free = SG.stage0_grads(mod, L, R, D, r, r2, F64)
    masks = free["took"]

    def loss(m, l, rr):
        with torch.no_grad():
            reg, _, _ = SG.regnet(m, SG.costvol(l, rr, D, "ssd").permute(0, 4, 1, 2, 3), masks)
            pred = (torch.softmax(reg, 1) * torch.arange(D, dtype=F64).view(1, D, 1, 1)).sum(1)
            return float((pred * r).sum() + (reg * r2).sum())

    h = 1e-6
    targets = [("L", L), ("R", R)] + [(n, p) for n, p in mod.named_parameters()
                                      if n.startswith(("conv0.0", "conv1.1", "conv2.2"))]
    for name, t in targets:
        flat = t.data.view(-1)
        for idx in torch.randperm(flat.numel(), generator=g)[:3].tolist():
            old = float(flat[idx])
            flat[idx] = old + h
            up = loss(mod, L, R)
            flat[idx] = old - h
            dn = loss(mod, L, R)
            flat[idx] = old
            fd, an = (up - dn) / (2 * h), float(free["grads"][name].view(-1)[idx])
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, idx, fd, an)


def test_flipped_weights_give_dx():
    from decnet_amd.stage0_grad import flipped_weight3d
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 4, 5, 6, generator=g, dtype=F64, requires_grad=True)         # [B,D,H,W,Ci]
    w, scale = torch.randn(7, 6, 3, 3, 3, generator=g, dtype=F64), torch.rand(7, generator=g, dtype=F64) + 0.5
    gm = torch.randn(2, 3, 4, 5, 7, generator=g, dtype=F64)
    (SG.conv3d_cl(x, w) * scale * gm).sum().backward()
    wt = flipped_weight3d(w, scale)
    assert wt.shape == (6, 7, 3, 3, 3) and wt.is_contiguous() and torch.equal(wt, SG.flipped(w, scale))
    assert float((SG.conv3d_cl(gm, wt) - x.grad).abs().max()) < 1e-12
    # and the reference's weight-gradient sums are F.conv3d's
    x2 = x.detach()
    wl = w.clone().requires_grad_()
    (SG.conv3d_cl(x2, wl) * gm).sum().backward()
    G, gsum, _, SGa, Ss = SG.wgrad(x2, gm, None)
    assert float((G - wl.grad).abs().max()) < 1e-12 and float((gsum - gm.sum((0, 1, 2, 3))).abs().max()) < 1e-12
    assert bool((SGa >= G.abs()).all()) and bool((Ss >= gsum.abs()).all())


@pytest.mark.parametrize("case", SG.WGRAD_CASES, ids=SG.WGRAD_IDS)
def test_workspace_query_is_the_stated_partition(lib, case):
    """nsets = ceil(V / sl) slices of sl voxels, sl a power of two in [256, 4096]: the query is exactly nsets Co (27 Ci + 1),
    and no slice -- so no fp32 chain -- is longer than 4096 voxels."""
    B, D, H, W, Ci, Co = case
    n = lib.decnet_conv3d_wgrad_workspace_floats(*case)
    per = Co * (27 * Ci + 1)
    assert n > 0 and n % per == 0, (case, n)
    nsets, V = n // per, B * D * H * W
    sl, want = SG.plan_sl(case)
    assert nsets == want and -(-V // nsets) <= sl <= 4096 and sl >= 256 and sl & (sl - 1) == 0, (case, nsets, sl)


def test_case_table_covers_the_chain_lengths():
    sls = {c: SG.plan_sl(c) for c in SG.WGRAD_CASES}
    assert {s for s, _ in sls.values()} >= {256, 1024, 4096}
    assert max(n for _, n in sls.values()) > 16 and sls[(1, 1, 17, 241, 4, 3)] == (256, 17)
    assert any(c[0] * c[1] * c[2] * c[3] >= 17 * 4096 + 1 for c in SG.WGRAD_CASES)


def test_host_refusals(lib):
    """Every refusal is decided on the host before the first launch: the pointers are never dereferenced, no GPU is needed."""
    case = (2, 2, 3, 5, 12, 5)
    n = lib.decnet_conv3d_wgrad_workspace_floats(*case)
    p = 0x10000                                                         # never dereferenced

    def call(x=p, gy=p, y=p, gm=p, G=p, gsum=p, ws=p, nws=n, dims=case):
        return lib.decnet_conv3d_wgrad(x, gy, y, gm, G, gsum, ws, nws, *dims, None)

    for k in ("x", "gy", "G", "gsum", "ws"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(gm=None) == ERR_NULL                                    # y given, gm missing
    for i in range(6):
        dims = list(case)
        dims[i] = 0
        assert call(dims=tuple(dims)) == ERR_SHAPE and lib.decnet_conv3d_wgrad_workspace_floats(*dims) == 0, i
    for dims in ((2, 2, 3, 5, 6, 5), (2, 2, 3, 5, 12, 225), (2, 2, 3, 5, 228, 5)):
        assert call(dims=dims, nws=1 << 40) == ERR_UNSUPPORTED and lib.decnet_conv3d_wgrad_workspace_floats(*dims) == 0, dims
    assert call(nws=n - 1) == ERR_SHAPE                                 # one float short
    assert call(ws=p + 4) == ERR_MISALIGNED
    # the size limit of the header: B D H W max(Ci, Co) < 2^31
    ok, over = (1, 64, 512, 292, 224, 8), (1, 64, 512, 293, 224, 8)     # 9 568 256 and 9 601 024 voxels x 224
    assert ok[1] * ok[2] * ok[3] * 224 < 2 ** 31 <= over[1] * over[2] * over[3] * 224
    assert lib.decnet_conv3d_wgrad_workspace_floats(*ok) > 0 and lib.decnet_conv3d_wgrad_workspace_floats(*over) == 0
    assert call(dims=over, nws=1 << 40) == ERR_UNSUPPORTED
    assert lib.decnet_conv3d_wgrad_workspace_floats(1, 64, 512, 293, 8, 224) == 0


def test_refused_outside_hip_grad_and_in_train_mode():
    import decnet_amd
    mod, L, R, D, _, _ = SG.module_case("c8_cor")
    Lg = L.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="hip_grad"):
        mod.stage0(Lg, R, D)
    with pytest.raises(NotImplementedError, match="hip_grad"):
        mod(torch.zeros(1, 8, 3, 4, 5, requires_grad=True))
    mod.train()
    for on in (True, False):
        with decnet_amd.hip_grad(on), pytest.raises(NotImplementedError):
            mod.stage0(Lg, R, D)
        with decnet_amd.hip_grad(on), pytest.raises(NotImplementedError):
            mod(torch.zeros(1, 8, 3, 4, 5))
    cat = decnet_amd.CostRegNetNoDown(8, 16, "cat").eval()
    with decnet_amd.hip_grad(), pytest.raises(NotImplementedError, match="cat"):
        cat.stage0(Lg, R, D)
    assert decnet_amd.Conv3dFunction is decnet_amd.stage0_grad.Conv3dFunction


def test_routing_sends_nothing_to_the_library_unmeasured():
    from decnet_amd import stage0
    for C in (4, 8, 216, 224):
        for voxels in (1, 120, 23040, 46080, 10 ** 7):
            assert stage0._conv3d_grad_slower(C, voxels) is False
