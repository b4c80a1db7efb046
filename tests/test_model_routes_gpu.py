"""Every route of the Python dispatch layer (decnet_amd/model.py) against the float64 references of tests/_model_ref.py.
-m gpu.

A case names the route it must take; the test asserts it twice -- by ``_hip_kind`` / ``_hip_ok`` and by the C entries
that were really called (tests/spy_util.entry_spy) -- and then compares values.  Every threshold of the dispatch has a
case on either side.  The whole file runs again in child processes under DECNET_CONV2D=torch, DECNET_CONV2D_MFMA=0 and
DECNET_CONV2D_ACC=2 (test_switch_leg); the expected route of a case depends on the switch, so the tables carry it per
switch: ``route`` (default and ACC=2, which changes the kernel behind the same entries), ``mfma0`` and, for every case,
the library under ``torch``.

Bounds (none is new): small fp32 kernels 2e-5 * max(1, max|ref|), bf16x3 matrix-core kernels 4e-6, stride 3 on the matrix
cores 1e-5, tap-conv 3e-5, the library route 1e-4 (tests/test_conv2d_gpu.py, tests/test_trunk_edges_gpu.py).  Composite
modules: the yardstick of tests/test_inputdata_gpu.py -- the distance to float64 at most 1.5 x (default) or 1.1 x (the
three switches) the distance of the module's own float32 torch route on the CPU, with the single-layer bound as floor.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import _model_cases as MC  # noqa: E402
import _model_ref as MR  # noqa: E402
import _trunk_ref as TR  # noqa: E402
from spy_util import entry_spy, spamat_spy  # noqa: E402

SWITCHES = {"torch": {"DECNET_CONV2D": "torch"}, "mfma0": {"DECNET_CONV2D_MFMA": "0"}, "acc2": {"DECNET_CONV2D_ACC": "2"}}


def _switch():
    for name, env in SWITCHES.items():
        if all(os.environ.get(k) == v for k, v in env.items()):
            return name
    return "default"


SW = _switch()
FACTOR = 1.5 if SW == "default" else 1.1
LIB_TOL = 1e-4
ENTRIES = {"mfma": ["decnet_conv2d_mfma_cat_bn_act"], "mfma_s3": ["decnet_s2d3_pad1", "decnet_conv2d_mfma_cat_bn_act"],
           "mfma_deconv": ["decnet_deconv2d_mfma_k3s3_bn_act"], "conv": ["decnet_conv2d_bn_act"],
           "cat": ["decnet_conv2d_cat_bn_act"], "conv_s3": ["decnet_conv2d_k3s3_bn_act"],
           "deconv": ["decnet_deconv2d_k3s3_bn_act"], "lib": ["decnet_bias_act_inplace"], "lib_nobn": []}
TOLS = {"mfma": MC.MFMA_TOL, "mfma_s3": MC.S3_TOL, "mfma_deconv": MC.MFMA_TOL, "conv": MC.FP32_TOL, "conv_s3": MC.FP32_TOL,
        "deconv": MC.FP32_TOL, None: LIB_TOL}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import decnet_amd  # noqa: F401
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _want(route, mfma0):
    return {"default": route, "acc2": route, "mfma0": mfma0, "torch": None}[SW]


# ---- Unit -----------------------------------------------------------------------------------------------------------------
T, UNIT_CASES, ASPP_CASES = MC.T, MC.UNIT_CASES, MC.ASPP_CASES          # (shared with tests/test_model_routes_cpu.py)


def _unit_case(name):
    c = UNIT_CASES[name]
    u = MC.make_unit(c["cin"], c["cout"], c["k"], seed=len(name) * 7 + c["cin"], **c["kw"])
    g = _gen(c["H"] * 131 + c["W"])
    xs = tuple(torch.randn(c["B"], n, c["H"], c["W"], generator=g) for n in (c["parts"] or (c["cin"],)))
    return c, u, xs


def _check_unit(dev, c, u, xs, want):
    ref = MR.unit(xs, MR.unit_params(u))
    ud = u.to(dev)
    xd = tuple(t.to(dev) for t in xs)
    xd = xd if c["parts"] else xd[0]
    with torch.no_grad():
        assert ud._hip_kind(xd) == want
        with entry_spy() as calls:
            got = ud(xd)
    key = want if want is not None else ("lib" if u.bn is not None else "lib_nobn")
    if key == "conv" and c["parts"]:
        key = "cat"
    assert calls == ENTRIES[key], (calls, key)
    assert got.shape == ref.shape
    r = MC.close(got, ref, TOLS[want])
    print("unit: route %s, error %.2f of the bound" % (want, r))
    assert r <= 1.0


@pytest.mark.parametrize("name", list(UNIT_CASES))
def test_unit_routes(dev, name):
    c, u, xs = _unit_case(name)
    _check_unit(dev, c, u, xs, _want(c["route"], c["mfma0"]))


def test_unit_tuple_parts_that_do_not_fit_together(dev):
    """Parts whose batch, size, dtype or device differ have no fused route (``_hip_kind`` is None; what torch.cat then
    makes of them is torch's business)."""
    u = MC.make_unit(24, 24, 3).to(dev)
    a = torch.zeros(2, 12, 64, 64, device=dev)
    with torch.no_grad():
        assert u._hip_kind((a, a)) == _want("mfma", None)
        for b in (a[:1], a[:, :, :63], a[..., :63], a.double(), a.cpu()):
            assert u._hip_kind((a, b)) is None
        assert u._hip_kind((a.double(), a.double())) is None
    with torch.enable_grad():
        assert u._hip_kind((a, a)) is None
    assert u.train()._hip_kind((a, a)) is None


@pytest.mark.parametrize("B,co,relu", [(1, 65535, True), (2, 32768, False), (3, 21845, False), (1, 65536, True)])
def test_library_route_bias_pass_at_its_grid_limit(dev, B, co, relu):
    """B Co 65535 | 65536: decnet_bias_act_inplace takes one block row per plane; above its limit the torch add +
    relu_ take over.  Tiny planes."""
    u = MC.make_unit(2, co, 1, relu=relu, seed=co)
    x = torch.randn(B, 2, 2, 3, generator=_gen(co))
    ref = MR.unit(x, MR.unit_params(u))
    ud = u.to(dev)
    with torch.no_grad(), entry_spy() as calls:
        assert ud._hip_kind(x.to(dev)) is None
        got = ud(x.to(dev))
    assert calls == (["decnet_bias_act_inplace"] if B * co <= 65535 else [])
    assert MC.close(got, ref, LIB_TOL) <= 1.0
    if relu:
        assert float(got.min()) == 0.0                      # (a missing ReLU would leave negatives)


def test_library_route_with_a_channels_last_input(dev):
    """A convolution result that is not contiguous skips the in-place pass (it indexes NCHW): same values either way."""
    u = MC.make_unit(32, 32, 3, seed=5)
    x = torch.randn(2, 32, 10, 11, generator=_gen(5))
    ref = MR.unit(x, MR.unit_params(u))
    ud = u.to(dev)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        raw = F.conv2d(xd, ud._folded_torch()[0], None, 1, 1)
        with entry_spy() as calls:
            got = ud(xd)
    assert calls == (["decnet_bias_act_inplace"] if raw.is_contiguous() else []), raw.stride()
    assert MC.close(got, ref, LIB_TOL) <= 1.0


def test_unsupported_entry_falls_back_to_the_library_and_tallies_that(dev):
    """A transposed convolution to 7282 channels is one the matrix-core entry declines by return code before any launch
    (csrc/conv2d_mfma.hip: 9 Cout must stay under 65536 column tiles, ``Cout > 7281 -> DECNET_ERR_UNSUPPORTED`` in
    decnet_deconv2d_mfma_packed_bytes / _pack_weight / _k3s3_bn_act), while ``_hip_kind`` has no such limit: forward()
    must catch it, run the library route and leave exactly one "library" record in TALLY."""
    import decnet_amd.model as M
    u = MC.make_unit(16, 7282, 3, seed=9, **T)
    x = torch.randn(1, 16, 16, 32, generator=_gen(9))
    ref = MR.unit(x, MR.unit_params(u))
    ud = u.to(dev)
    M.TALLY = []
    try:
        with torch.no_grad():
            assert ud._hip_kind(x.to(dev)) == _want("mfma_deconv", None)
            got = ud(x.to(dev))
        tally = M.TALLY
    finally:
        M.TALLY = None
    assert [t["family"] for t in tally] == ["library"]
    assert MC.close(got, ref, LIB_TOL) <= 1.0


# ---- composite modules: the yardstick -------------------------------------------------------------------------------------
def _yardstick(got, ref64, out32, what, tol=MC.FP32_TOL):
    bound = MC.composite_bound(ref64, out32, FACTOR, tol)
    err = float((got.double().cpu() - ref64).abs().max())
    print("%s: |gpu - f64| %.3e, bound %.3e (%.2f)" % (what, err, bound, err / bound))
    assert got.shape == ref64.shape
    assert err <= bound, what


def _on(route, mfma0="same"):
    return _want(route, route if mfma0 == "same" else mfma0)


@pytest.mark.parametrize("cin,cout,hw,k_dec,k_c0", [(18, 6, (16, 32), ("deconv", "deconv"), ("conv", "conv")),
                                                     (54, 18, (16, 32), ("mfma_deconv", None), ("mfma", None)),
                                                     (6, 2, (5, 7), ("deconv", "deconv"), ("conv", "conv"))])
def test_upblock(dev, cin, cout, hw, k_dec, k_c0):
    from decnet_amd.model import UpBlock
    m = MC.seeded(lambda: UpBlock(cin, cout), cin)
    g = _gen(cin)
    x, skip = torch.randn(2, cin, *hw, generator=g), torch.randn(2, cout, 3 * hw[0], 3 * hw[1], generator=g)
    ref, ref_up = MR.upblock(skip, x, MR.upblock_params(m))
    with torch.no_grad():
        o32, up32 = m(skip, x)
        md = m.to(dev)
        xd, sd = x.to(dev), skip.to(dev)
        assert md.deconv._hip_kind(xd) == _on(*k_dec)
        with entry_spy() as calls:
            got, up = md(sd, xd)
        assert md.conv[0]._hip_kind((up, sd)) == _on(*k_c0)
    want = ENTRIES[_on(*k_dec) or "lib"] + {"conv": ENTRIES["cat"], "mfma": ENTRIES["mfma"], None: ENTRIES["lib"]}[_on(*k_c0)]
    assert calls[:len(want)] == want, calls
    _yardstick(up, ref_up, up32, "UpBlock.up")
    _yardstick(got, ref, o32, "UpBlock")


@pytest.mark.parametrize("name", list(ASPP_CASES))
def test_aspp_routes(dev, name):
    from decnet_amd.model import ASPP
    cin, cout, rates, (H, W), relu1, fused = ASPP_CASES[name]
    m = MC.seeded(lambda: ASPP(cin, cout, rates), cin + cout)
    list(m.stages.children())[1].relu = relu1
    x = torch.randn(2, cin, H, W, generator=_gen(H))
    ref = MR.aspp(x, MR.aspp_params(m))
    fused = fused and SW != "torch"
    md = m.to(dev)
    with torch.no_grad(), entry_spy() as calls:
        assert md._hip_ok(x.to(dev)) == fused
        got = md(x.to(dev))
    if fused:
        assert calls == ["decnet_tapconv_to_chunks", "decnet_tap_gemm", "decnet_tapconv_gather"]
    else:                                                   # the branches as Units on routes of their own
        assert not [c for c in calls if "tap" in c] and len(calls) >= len(rates) + 1
    assert MC.close(got, ref, MC.ASPP_TOL if fused else LIB_TOL) <= 1.0


@pytest.mark.parametrize("B", [1, 2, 3])
def test_feature_extractor_two_views(dev, B):
    """forward(x, x2) against forward(cat(x, x2)): bit-identical -- the first layer runs per sample either way, the rest
    is the same call.  Also x.shape != x2.shape (other batch size: the concatenation route), and both against float64.
    (A first layer that is not "conv" needs a plane under 256 pixels, which the x27 pyramid cannot have; the
    DECNET_CONV2D=torch leg of this file takes that branch.)"""
    from decnet_amd.model import FeatExtNetChannelPlus
    m = MC.seeded(lambda: FeatExtNetChannelPlus(2), 21)
    g = _gen(B)
    x, x2, x3 = (torch.randn(n, 3, 27, 54, generator=g) for n in (B, B, B + 1))
    ref = MR.featext(torch.cat((x, x2)), MR.featext_params(m))
    with torch.no_grad():
        o32 = m(torch.cat((x, x2)))
        md = m.to(dev)
        xd, x2d, x3d = x.to(dev), x2.to(dev), x3.to(dev)
        assert md.conv0[0]._hip_kind(xd) == _on("conv")
        with entry_spy() as calls:
            two = md(xd, x2d)
        assert calls[:2] == (["decnet_conv2d_bn_act"] * 2 if SW != "torch" else ["decnet_bias_act_inplace"] * 2)
        one = md(torch.cat((xd, x2d)))
        odd = md(xd, x3d)
        odd_cat = md(torch.cat((xd, x3d)))
    for k in ref:
        assert torch.equal(two[k], one[k]), k
        assert torch.equal(odd[k], odd_cat[k]), k
        _yardstick(two[k], ref[k], o32[k], "FeatExt " + k)


# ---- GenerateSparseMask.mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", MC.MASK_CASES)
def test_mask_routes_bits_and_batches(dev, H, W):
    """want_bits both ways; bit i of word w == the float mask at pixel 64 w + i and the bits past W in the last word
    are zero -- the kernel clears them (``x0 + e < W``) and its consumer relies on it: csrc/spamat_mfma.hip's mask4_bits
    reads the four bits x .. x + 3 of a row with only x checked against W, so a set bit past W would be an active pixel;
    the two-view batch against two single-view calls, bit-identical; the torch route (under enable_grad) as a third
    opinion; all against the float64 reference away from its close calls (tests/test_model_ref_cpu.py caps those at 1 %)."""
    from spy_util import unpack_mask_bits
    gen, cur, pre, thold = MC.mask_case(H, W)
    ref, logit = MR.mask(cur, pre, MR.maskgen_params(gen), thold)
    unsure = MR.mask_unsure(logit, thold, MC.mask_margin(gen, cur, pre, logit, FACTOR))
    assert float(unsure.double().mean()) <= 0.01
    gd = gen.to(dev)
    cd, pd = cur.to(dev), pre.to(dev)
    with torch.no_grad():
        with entry_spy() as calls:
            m0 = gd.mask(cd, pd, thold)
        assert ("decnet_detail_mask" in calls) == (SW != "torch")
        m1, bits = gd.mask(cd, pd, thold, want_bits=True)
        halves = [gd.mask(cd[i:i + 1], pd[i:i + 1], thold, want_bits=True) for i in range(cd.shape[0])]
    with torch.enable_grad():
        m_torch = gd.mask(cd, pd, thold).detach()
    assert m0.shape == ref.shape and set(m0.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(m0, m1)
    assert torch.equal(torch.cat([h[0] for h in halves]), m1)
    if SW == "torch":
        assert bits is None
    else:
        assert bits.shape == (cd.shape[0], H, (W + 63) // 64) and bits.dtype == torch.int64
        assert torch.equal(torch.cat([h[1] for h in halves]), bits)
        assert torch.equal(unpack_mask_bits(bits, W), m1)
        assert torch.equal(unpack_mask_bits(bits, 64 * bits.shape[-1])[:, :, W:].sum(), torch.zeros((), device=dev))
    sure = ~unsure
    assert torch.equal(m0.cpu().bool()[sure], ref[sure]), "mask differs from float64 away from the threshold"
    assert torch.equal(m_torch.cpu().bool()[sure], ref[sure]), "torch route differs from float64 away from the threshold"


# ---- DynamicUpsampling, warp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,h,w,extra", [(2, 2, 5, 7, (0, 0)), (2, 2, 1, 9, (0, 0)), (2, 2, 9, 1, (0, 0)), (1, 2, 1, 1, (0, 0)),
                                           (2, 2, 5, 7, (1, 2)), (4369, 14, 1, 2, (0, 0)), (4096, 15, 1, 2, (0, 0))])
def test_dynamic_upsampling_routes(dev, B, C, h, w, extra):
    """``fea`` of exactly (3h, 3w) takes decnet_unfold3_cat, any other size F.unfold (which drops the remainder);
    B (C + 1) = 65535 | 65536 is that kernel's grid limit.  The softmax tail kernel runs either way."""
    from decnet_amd.model import DynamicUpsampling
    m = MC.seeded(lambda: DynamicUpsampling(C, 3), C)
    g = _gen(B + h)
    disp, fea = torch.rand(B, h, w, generator=g) * 20, torch.randn(B, C, 3 * h + extra[0], 3 * w + extra[1], generator=g)
    ref = MR.dynamic_upsampling(disp, fea[:, :, :3 * h, :3 * w], MR.seq_params(m.weight_learning))
    with torch.no_grad():
        o32 = m(disp, fea)
        md = m.to(dev)
        with entry_spy() as calls:
            got = md(disp.to(dev), fea.to(dev))
    unfold = SW != "torch" and extra == (0, 0) and B * (C + 1) <= 65535
    assert ("decnet_unfold3_cat" in calls) == unfold
    assert ("decnet_dynamic_upsample3" in calls) == (SW != "torch")
    _yardstick(got, ref, o32, "DynamicUpsampling")


@pytest.mark.parametrize("H,W", [(9, 40), (1, 40), (40, 1), (2, 2)])
def test_warp_routes(dev, H, W):
    """H = 1 or W = 1 takes the torch route (the stretch divides by H - 1 and W - 1; only the route is asserted there);
    disparities that push samples off
    both image sides, exactly integer ones and the rest of tests/_trunk_ref.warp_disparities.  Reference: the float64
    warp at the float32 coordinates the reference graph computes, as tests/test_trunk_edges_gpu.py."""
    from decnet_amd.model import warp_by_disparity
    g = _gen(H * 100 + W)
    right = torch.randn(2, 3, H, W, generator=g)
    for i, disp in enumerate(TR.warp_disparities(2, H, W, g)):
        disp = disp.float()
        with torch.no_grad(), entry_spy() as calls:
            got = warp_by_disparity(right.to(dev), disp.to(dev))
        assert calls == (["decnet_warp_disparity"] if H > 1 and W > 1 and SW != "torch" else [])
        if H > 1 and W > 1:
            assert MC.close(got, TR.warp(right, disp, coord_dtype=torch.float32), MC.FP32_TOL) <= 1.0, i
        else:                                               # (H - 1 = 0 or W - 1 = 0 in the stretch: the coordinates are
            assert got.shape == right.shape                 # 0 / 0 or x / 0, and what grid_sample makes of them is torch's own)


# ---- SoftAttention.fuse, Refinement -----------------------------------------------------------------------------------------
def _fuse_inputs(B, C, H, W, seed):
    g = _gen(seed)
    return (torch.randn(B, C, H, W, generator=g), torch.rand(B, H, W, generator=g) * 30, torch.rand(B, H, W, generator=g) * 30,
            (torch.rand(B, H, W, generator=g) < 0.5).float(), torch.rand(B, H, W, generator=g) * 4)


@pytest.mark.parametrize("C,base,hw,k0,plain_u2", [(6, 2, (18, 81), ("conv", "conv"), False), (6, 2, (18, 81), ("conv", "conv"), True),
                                                    (44, 2, (64, 64), ("mfma", "conv"), False), (18, 9, (64, 65), ("mfma", None), False),
                                                    (6, 2, (9, 27), (None, None), False)])
def test_soft_attention_fuse_routes(dev, C, base, hw, k0, plain_u2):
    """k0 == "conv" (the negated variance folded into the first layer's weights), "mfma" (negated by torch) and None (the
    module's own forward); the last layer's sigmoid + blend as its epilogue or, where it has no fused route, as torch ops
    (with the shipped constructor that branch needs a last layer under 256 pixels, where k0 is None already, so the test
    takes the route away from u2 by hand)."""
    from decnet_amd.model import SoftAttention
    m = MC.seeded(lambda: SoftAttention(C + 4, base), C + base)
    args = _fuse_inputs(2, C, hw[0], hw[1], C)
    ref = MR.fuse(*args, MR.seq_params(m.conv))
    with torch.no_grad():
        o32 = m.fuse(*args)
        md = m.to(dev)
        ad = tuple(t.to(dev) for t in args)
        if plain_u2:
            md.conv[2]._hip_kind = lambda t: None
        parts = (ad[0],) + tuple(t.unsqueeze(1) for t in ad[1:])
        assert md.conv[0]._hip_kind(parts) == _on(*k0)
        with entry_spy() as calls:
            got = md.fuse(*ad)
    k = _on(*k0)
    if k is not None:
        assert calls[0] == {"conv": "decnet_conv2d_cat_bn_act", "mfma": "decnet_conv2d_mfma_cat_bn_act"}[k]
        assert (calls[-1] == "decnet_conv2d_cat_epilogue") == (not plain_u2)
    else:
        assert "decnet_conv2d_cat_epilogue" not in calls
    _yardstick(got, ref, o32, "fuse")


def test_unit_alternating_neg_last(dev):
    """``_folded`` keeps one slot: the same unit called with neg_last=True, False, True, False must give, each time, what
    a fresh unit gives (bit for bit), and the float64 value of the negated / plain last channel."""
    u = MC.make_unit(10, 2, 3, seed=31)
    g = _gen(31)
    parts = (torch.randn(2, 6, 18, 81, generator=g), torch.randn(2, 4, 18, 81, generator=g))
    flip = (parts[0], torch.cat((parts[1][:, :3], -parts[1][:, 3:]), 1))
    refs = {True: MR.unit(flip, MR.unit_params(u)), False: MR.unit(parts, MR.unit_params(u))}
    import copy
    ud = copy.deepcopy(u).to(dev)
    pd = tuple(t.to(dev) for t in parts)
    with torch.no_grad():
        assert ud._hip_kind(pd) == _on("conv")
        if SW == "torch":
            return
        for neg in (True, False, True, False):
            got = ud._forward_hip(pd, "conv", neg_last=neg)
            fresh = copy.deepcopy(u).to(dev)._forward_hip(pd, "conv", neg_last=neg)
            assert torch.equal(got, fresh), neg
            assert MC.close(got, refs[neg], MC.FP32_TOL) <= 1.0, neg
    assert not torch.equal(refs[True], refs[False])


@pytest.mark.parametrize("stage_id", [0, 1, 2, 3])
@pytest.mark.parametrize("c,hw,epi", [(6, (18, 81), True), (6, (9, 27), False), (24, (64, 66), True)])
def test_refinement_routes(dev, stage_id, c, hw, epi):
    """disp + res as the last layer's epilogue (planes of 256 pixels and more) and as a torch add (below); each of the
    four _DIL rows; in_channels 6 gives an odd half (3); 24 channels puts the first layers on the matrix cores."""
    from decnet_amd.model import Refinement
    m = MC.seeded(lambda: Refinement(c, 4, stage_id), 41 + stage_id)
    m.conv[-1].conv.bias.data.normal_(0, 0.3)
    g = _gen(stage_id + c)
    left, right = torch.randn(2, c, *hw, generator=g), torch.randn(2, c, *hw, generator=g)
    disp = torch.rand(2, *hw, generator=g) * 12 - 2
    ref = MR.refinement(left, right, disp, MR.seq_params(m.conv))
    with torch.no_grad():
        o32, _ = m(left, right, disp)
        md = m.to(dev)
        with entry_spy() as calls:
            got, res = md(left.to(dev), right.to(dev), disp.to(dev))
    epi = epi and SW != "torch"
    assert (calls[-1] == "decnet_conv2d_cat_epilogue") == epi, calls
    assert (res is None) == epi
    if c == 24 and SW in ("default", "acc2"):
        assert "decnet_conv2d_mfma_cat_bn_act" in calls
    if res is not None:
        assert torch.equal(got, disp.to(dev) + res)
    _yardstick(got, ref, o32, "Refinement")


# ---- the stage loop -------------------------------------------------------------------------------------------------------
def _net(dev, seed=1, **kw):
    from make_golden import E2E_KW
    from netparams import fill_state_dict
    from decnet_amd.model import get_model
    m = get_model(**dict(E2E_KW, **kw))
    m.load_state_dict(fill_state_dict(m.state_dict(), seed=seed))
    return m.to(dev).eval()


def _views(dev, B=1, H=54, W=243, seed=3):
    g = _gen(seed)
    return torch.randn(B, 3, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)


def _fwd(m, *a, **kw):
    with torch.no_grad(), entry_spy() as calls:
        out = m(*a, **kw)[-1].clone()
    torch.cuda.synchronize()
    return out, calls


@pytest.mark.parametrize("skip", [1, 2, 3])
def test_stage_loop_skip_stage_id(dev, skip):
    """Stages from skip_stage_id on are bicubic x3 of the stage before (reference :143-144): the output must be exactly
    that interpolation of what the default model hands from stage skip - 1 to stage skip (same kernels up to there)."""
    l, r = _views(dev, B=2)
    full = _net(dev)
    seen = {}
    hooks = [full.refinement[i].register_forward_hook(lambda m, a, out, i=i: seen.__setitem__(i + 1, out[0].clone()))
             for i in range(3)]
    stage0 = full.cost_regularizer.stage0
    full.cost_regularizer.stage0 = lambda *a, **k: seen.setdefault(0, stage0(*a, **k))
    try:
        _fwd(full, l, r)
    finally:
        del full.cost_regularizer.stage0
        for h in hooks:
            h.remove()
    got, calls = _fwd(_net(dev, skip_stage_id=skip), l, r)
    assert sum(c.startswith("decnet_spamatvar") for c in calls) == skip - 1
    want = seen[skip - 1]
    for _ in range(skip, 4):
        want = F.interpolate(want.unsqueeze(1) * 3, scale_factor=3, mode="bicubic").squeeze(1)
    assert got.shape == (2, 54, 243)
    assert torch.equal(got, want)


def test_stage_loop_variants_against_the_default(dev, monkeypatch):
    """Each variant's output against the default variant's, bit for bit: caller masks (use_detail=False, fed with the
    masks the default run generated: the float-mask SpaMat entry instead of the bit-packed one, documented to give the
    same results), DECNET_SPAMAT_BITS=0 (the same), and the two views' masks generated per view instead of as one batch
    (the limit TWO_VIEW_MASK_BYTES lowered instead of 96 MB of features allocated)."""
    import decnet_amd.model as M
    l, r = _views(dev, B=2)
    monkeypatch.delenv("DECNET_SPAMAT_BITS", raising=False)
    masks = []
    with spamat_spy(lambda L, R, lm, rm, D, o: masks.append((lm.clone(), rm.clone()))):
        want, calls = _fwd(_net(dev), l, r)
    bits_entry = SW != "torch"                              # (the torch mask route writes no bit planes)
    assert ("decnet_spamatvar_forward_bits" in calls) == bits_entry
    assert [tuple(m[0].shape[-2:]) for m in masks] == [(6, 27), (18, 81), (54, 243)]

    m = _net(dev, use_detail=False)
    got, calls = _fwd(m, l, r, None, [a for a, _ in masks], [b for _, b in masks])
    assert calls.count("decnet_spamatvar_forward") == 3 and "decnet_detail_mask" not in calls
    assert torch.equal(got, want), "caller masks"

    monkeypatch.setenv("DECNET_SPAMAT_BITS", "0")
    got, calls = _fwd(_net(dev), l, r)
    assert calls.count("decnet_spamatvar_forward") == 3 and "decnet_spamatvar_forward_bits" not in calls
    assert torch.equal(got, want), "DECNET_SPAMAT_BITS=0"
    monkeypatch.delenv("DECNET_SPAMAT_BITS")

    n_default = calls.count("decnet_detail_mask")
    monkeypatch.setattr(M, "TWO_VIEW_MASK_BYTES", 0)
    got, calls = _fwd(_net(dev), l, r)
    if SW != "torch":
        assert (n_default, calls.count("decnet_detail_mask")) == (3, 6)
    assert torch.equal(got, want), "per-view masks"


def test_stage_loop_views_of_different_shapes_raise(dev):
    """left.shape != right.shape: the extractor runs per view, then stage 0 refuses the pair by its shape check
    (ValueError) before any kernel of the hot path is launched."""
    m = _net(dev)
    l, r = _views(dev, B=2)
    for bad in (r[:1], r[..., :216]):
        with torch.no_grad(), entry_spy() as calls, pytest.raises(ValueError):
            m(l, bad)
        assert not [c for c in calls if c.startswith(("decnet_stage0", "decnet_spamat"))]


def test_stage_loop_wider_than_one_band(dev):
    """max_disp 297: stage 3 runs at D = 297 > 273 (one band of the matrix-core SpaMat kernels), i.e. through the `_ws`
    entry on a torch workspace; eagerly and as a replay of a captured graph, bit-identical; and the same again with the
    float-mask entry."""
    l, r = _views(dev, B=1, H=54, W=324)
    m = _net(dev, max_disp=297)
    want, calls = _fwd(m, l, r)
    assert ("decnet_spamatvar_forward_bits_ws" if SW != "torch" else "decnet_spamatvar_forward_ws") in calls, calls
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(l, r)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(l, r)[-1]
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, want)
    del graph
    os.environ["DECNET_SPAMAT_BITS"] = "0"
    try:
        got, calls = _fwd(_net(dev, max_disp=297), l, r)
    finally:
        del os.environ["DECNET_SPAMAT_BITS"]
    assert "decnet_spamatvar_forward_ws" in calls
    assert torch.equal(got, want)


# ---- the whole file again under each switch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SWITCHES) + ["spamat_bits0"])
def test_switch_leg(name):
    """One child process per switch (read per call or once per process by the library), one at a time, each with its
    own timeout.  spamat_bits0: the stage-loop tests with DECNET_SPAMAT_BITS=0 from the start of the process."""
    if SW != "default" or os.environ.get("DECNET_ROUTES_CHILD"):
        return                                              # (a child does not start children)
    env = dict(os.environ, DECNET_ROUTES_CHILD="1", **SWITCHES.get(name, {"DECNET_SPAMAT_BITS": "0"}))
    sel = "stage_loop_skip or stage_loop_views" if name == "spamat_bits0" else "not switch_leg"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", sel], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
