"""CPU side of the stride-3 conv / transposed-conv backward (decnet_amd/conv2d_grad.Conv2dS3Function / Deconv2dS3Function,
csrc/conv2d_mfma_grad.hip, csrc/unfold.hip):
  * the closed forms of tests/_conv2d_s3_grad_ref.py (what the GPU test compares the kernels with) equal torch's own double
    autograd of F.conv2d(stride 3, padding 1) / F.conv_transpose2d(stride 3);
  * Unit._grad_route_s3 is pure, agrees with Unit._route, and is pinned over the model's stride-3 layers at config 5's sizes;
    Unit._grad_route and Unit._grad_route_mfma still answer None for these layers;
  * the new entries are declared in include/decnet_hip.h and bound in _lib.py with matching signatures, and refuse NULL and
    bad shapes before any launch."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import _conv2d_s3_grad_ref as S3
import _model_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


# ---- 1. the reference's closed forms ----------------------------------------------------------------------------------------------
SIZES = list(itertools.product((4, 5, 6), (7, 8, 9))) + [(1, 5), (5, 1), (1, 1)]      # all nine residue pairs mod 3; H = 1, W = 1


@pytest.mark.parametrize("tr", [False, True], ids=["conv", "transposed"])
@pytest.mark.parametrize("relu,bn", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_closed_forms_equal_double_autograd(tr, relu, bn, hw):
    H, W = hw
    B, ci, co = 2, 3, 4
    g = torch.Generator().manual_seed(17 * H + W + (100 if tr else 0))
    x = torch.randn(B, ci, H, W, generator=g, dtype=D)
    w = torch.randn((ci, co, 3, 3) if tr else (co, ci, 3, 3), generator=g, dtype=D)
    scale = torch.rand(co, generator=g, dtype=D) + 0.5 if bn else torch.ones(co, dtype=D)
    shift = torch.randn(co, generator=g, dtype=D)
    gy = torch.randn((B, co) + S3.out_hw(tr, H, W), generator=g, dtype=D)
    own, ours = S3.autograd(tr, x, w, scale, shift, relu, gy), S3.closed(tr, x, w, scale, shift, relu, gy)
    assert own.keys() == ours.keys()
    for k, ref in own.items():
        assert ours[k].shape == ref.shape, k
        assert float((ours[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k


def test_layout_references():
    """d2s3_pad1 is the adjoint of s2d3_pad1 (<s2d(x), t> = <x, d2s(t)>), and s2d3_pad0 is F.unfold(3, stride 3)."""
    import _trunk_ref as R
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    for H, W in SIZES:
        x = torch.randn(2, 3, H, W, generator=g, dtype=D)
        t = torch.randn(2, 27, *S3.out_hw(False, H, W), generator=g, dtype=D)
        assert abs(float((R.s2d3_pad1(x) * t).sum() - (x * S3.d2s3_pad1(t, H, W)).sum())) <= 1e-11
        gm = torch.randn(2, 3, 3 * H, 3 * W, generator=g, dtype=D)
        assert torch.equal(S3.s2d3_pad0(gm), F.unfold(gm, 3, stride=3).view(2, 27, H, W))


def test_imposed_mask_chain_equals_double_autograd_of_the_modules():
    """With its own masks imposed the chain reference gives the gradients of the free run."""
    conv1, up, f0, r = S3.chain_case()
    f0, r = f0[:, :, :24, :27], r[:, :, :24, :27]
    free, masks = S3.chain_grads(conv1, up, f0, r, D)
    imposed, took = S3.chain_grads(conv1, up, f0, r, D, masks)
    assert len(masks) == 6 and all(a is b for a, b in zip(took, masks))
    import copy
    c1, u = copy.deepcopy(conv1).double(), copy.deepcopy(up).double()
    x0 = f0.double().requires_grad_()
    (u(x0, c1(x0))[0] * r.double()).sum().backward()                    # torch's own modules: conv -> BatchNorm -> ReLU
    own = {"conv1." + n: p.grad for n, p in c1.named_parameters()}
    own.update({"up." + n: p.grad for n, p in u.named_parameters()})
    own["f0"] = x0.grad
    assert own.keys() == imposed.keys() == free.keys()
    for k, ref in own.items():
        scale = max(1e-300, float(ref.abs().max()))
        assert float((imposed[k] - ref).abs().max()) <= 1e-12 * scale, k
        assert float((free[k] - ref).abs().max()) <= 1e-12 * scale, k


# ---- 2. the route ----------------------------------------------------------------------------------------------------------------
FULL, L1, L2, L3 = (540, 972), (180, 324), (60, 108), (20, 36)        # config 5's levels
# where in the model: ((H, W) of the unit's input, B, forward route, Unit._grad_route_s3 at that B, and for one image).  At
# config 5's batch five of the nine were measured slower than the library and stay on it (model._s3_grad_slower,
# profiles/conv2d_s3_grad.json)
MODEL_TABLE = {
    "feat.conv1.0": (FULL, 8, "conv_s3", "s3", "s3"), "feat.conv2.0": (L1, 8, "mfma_s3", None, None),
    "feat.conv3_1": (L2, 8, "mfma_s3", None, "s3"),
    "feat.deconv3.deconv": (L3, 8, "mfma_deconv", None, "deconv"), "feat.deconv2.deconv": (L2, 8, "mfma_deconv", "deconv", None),
    "feat.deconv1.deconv": (L1, 8, "deconv", "deconv", "deconv"),
    "mask72.deconv.0": (L3, 4, "mfma_deconv", None, "deconv"), "mask24.deconv.0": (L2, 4, "mfma_deconv", None, None),
    "mask8.deconv.0": (L1, 4, "deconv", "deconv", "deconv"),
}


def _model_units():
    from decnet_amd.model import FeatExtNetChannelPlus, GenerateSparseMask
    mods = {"feat": FeatExtNetChannelPlus(8).eval()}
    mods.update({"mask%d" % c: GenerateSparseMask(c, 3).eval() for c in (72, 24, 8)})
    return {"%s.%s" % (k, n): u for k, m in mods.items() for n, u in m.named_modules() if n and hasattr(u, "_grad_route_s3")}


def test_grad_route_s3_over_the_model(monkeypatch):
    monkeypatch.delenv("DECNET_CONV2D", raising=False)
    monkeypatch.delenv("DECNET_CONV2D_MFMA", raising=False)
    units = _model_units()
    strided = {n for n, u in units.items() if u.conv.stride == (3, 3)}
    assert strided == set(MODEL_TABLE)
    for n, ((H, W), B, route, want, want1) in MODEL_TABLE.items():
        u = units[n]
        assert u._route(B, H, W) == route, n
        assert u._grad_route_s3(B, H, W) == want and u._grad_route_s3(1, H, W) == want1, n
        assert u._grad_route(B, H, W) is None and u._grad_route_mfma(B, H, W) is None, n
    for n, u in units.items():                                          # every stride-1 unit, at every level
        if n not in strided:
            assert all(u._grad_route_s3(4, H, W) is None for H, W in (FULL, L1, L2, L3)), n
    for env in ("torch", "hip"):                                        # decided at the default switches: pure
        monkeypatch.setenv("DECNET_CONV2D", env)
        monkeypatch.setenv("DECNET_CONV2D_MFMA", "0")
        for n, ((H, W), B, route, want, _) in MODEL_TABLE.items():
            assert units[n]._grad_route_s3(B, H, W) == want, (env, n)


@pytest.mark.parametrize("name", sorted(MC.UNIT_CASES))
def test_grad_route_s3_agrees_with_route(name, monkeypatch):
    """Over the rows of tests/_model_cases.py: "s3" / "deconv" exactly on the four stride-3 forward routes (so None below
    their floors, e.g. hw < 256 or "mfma_s3" below 4608 pixels, and on every stride-1 and library row)."""
    monkeypatch.delenv("DECNET_CONV2D", raising=False)
    monkeypatch.delenv("DECNET_CONV2D_MFMA", raising=False)
    c = MC.UNIT_CASES[name]
    u = MC.make_unit(c["cin"], c["cout"], c["k"], **c["kw"])
    want = {"conv_s3": "s3", "mfma_s3": "s3", "deconv": "deconv", "mfma_deconv": "deconv"}.get(c["route"])
    if c["parts"] is None:
        assert u._grad_route_s3(c["B"], c["H"], c["W"]) == want
    else:
        assert want is None
    if want is not None:
        assert u._grad_route(c["B"], c["H"], c["W"]) is None and u._grad_route_mfma(c["B"], c["H"], c["W"]) is None


def test_grad_route_s3_limits():
    s3 = lambda ci, co: MC.make_unit(ci, co, 3, stride=3)                                   # noqa: E731
    dc = lambda ci, co: MC.make_unit(ci, co, 3, stride=3, transposed=True)                  # noqa: E731
    assert s3(8, 24)._grad_route_s3(1, 16, 16) == "s3" and s3(8, 24)._grad_route_s3(1, 15, 17) is None     # 256 | 255 pixels
    assert s3(8, 25)._grad_route_s3(1, 72, 64) == "s3" and s3(8, 25)._grad_route_s3(1, 17, 271) is None    # 4608 | 4607
    assert s3(7, 25)._grad_route_s3(1, 72, 64) is None                                      # the forward's 8 inputs
    assert s3(16, 224)._grad_route_s3(1, 72, 64) == "s3" and s3(16, 225)._grad_route_s3(1, 72, 64) is None  # the entry's 224
    assert s3(224, 32)._grad_route_s3(1, 72, 64) == "s3" and s3(225, 32)._grad_route_s3(1, 72, 64) is None
    assert dc(16, 9)._grad_route_s3(1, 16, 32) == "deconv" and dc(16, 9)._grad_route_s3(1, 7, 73) is None  # 512 | 511
    assert dc(4, 4)._grad_route_s3(1, 1, 29) == "deconv" and dc(4, 4)._grad_route_s3(1, 1, 28) is None     # 9 hw >= 256
    assert dc(224, 224)._grad_route_s3(1, 16, 32) == "deconv" and dc(225, 16)._grad_route_s3(1, 16, 32) is None
    assert dc(16, 225)._grad_route_s3(1, 16, 32) is None
    assert MC.make_unit(24, 24, 3)._grad_route_s3(1, 64, 64) is None and MC.make_unit(4, 4, 3)._grad_route_s3(1, 16, 16) is None
    # the measured exclusions at their literal thresholds, in pixels over the batch: "s3" with more than 24 outputs from
    # 51840; "deconv" with 72 or more inputs from 2880 up to 51840
    assert s3(72, 216)._grad_route_s3(8, 60, 108) is None and s3(72, 216)._grad_route_s3(7, 60, 108) == "s3"
    assert s3(24, 25)._grad_route_s3(1, 240, 216) is None and s3(24, 25)._grad_route_s3(1, 239, 216) == "s3"
    assert s3(8, 24)._grad_route_s3(8, 540, 972) == "s3"
    assert dc(216, 8)._grad_route_s3(4, 20, 36) is None and dc(216, 8)._grad_route_s3(3, 20, 36) == "deconv"
    assert dc(72, 24)._grad_route_s3(8, 60, 108) == "deconv" and dc(72, 24)._grad_route_s3(1, 239, 216) is None
    assert dc(72, 8)._grad_route_s3(4, 60, 108) is None and dc(71, 8)._grad_route_s3(4, 60, 108) == "deconv"
    assert dc(24, 8)._grad_route_s3(4, 180, 324) == "deconv" and dc(24, 8)._grad_route_s3(1, 64, 64) == "deconv"


def test_cpu_unit_is_untouched_by_hip_grad(monkeypatch):
    from decnet_amd import _lib, hip_grad, model

    def no_lib():
        raise AssertionError("a CPU unit looked the library up")

    monkeypatch.setattr(_lib, "lib", no_lib)
    for u, shape in ((MC.make_unit(8, 24, 3, stride=3), (1, 8, 16, 18)), (MC.make_unit(24, 8, 3, stride=3, transposed=True), (1, 24, 6, 6))):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3), requires_grad=True)
        assert u._grad_route_s3(*shape[:1], *shape[2:]) is not None
        model.TALLY = []
        try:
            want = u(x)
            with hip_grad():
                got = u(x)
            tally = [t["family"] for t in model.TALLY]
        finally:
            model.TALLY = None
        assert torch.equal(got, want) and tally == ["library", "library"]


# ---- 3. the boundary ---------------------------------------------------------------------------------------------------------------
def _header_decl(name):
    src = open(os.path.join(ROOT, "include", "decnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/decnet_hip.h" % name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype(arg):
    if "*" in arg:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}[arg.split()[0]]


ENTRIES = (("decnet_conv2d_k3s3_wgrad_workspace_floats", "size_t"), ("decnet_conv2d_k3s3_wgrad", "int"),
           ("decnet_deconv2d_k3s3_wgrad_workspace_floats", "size_t"), ("decnet_deconv2d_k3s3_wgrad", "int"),
           ("decnet_d2s3_pad1", "int"), ("decnet_s2d3_pad0", "int"))


def test_entries_and_signatures():
    from decnet_amd import _lib, build, ops2d
    for name, ret in ENTRIES:
        got_ret, args = _header_decl(name)
        assert got_ret == ret
        assert [_ctype(a) for a in args] == _lib.SIGNATURES[name], name
    assert _header_decl("decnet_conv2d_k3s3_wgrad")[1] == _header_decl("decnet_deconv2d_k3s3_wgrad")[1]
    assert _header_decl("decnet_d2s3_pad1")[1][2:] == _header_decl("decnet_s2d3_pad1")[1][2:]
    for wrapper in ("conv2d_k3s3_wgrad", "deconv2d_k3s3_wgrad", "d2s3_pad1", "s2d3_pad0"):
        assert callable(getattr(ops2d, wrapper))
    L = ctypes.CDLL(build.build())                                      # hipcc cross-compiles for gfx950 without a GPU
    one = ctypes.c_void_p(64)
    for tr, name in ((False, "decnet_conv2d_k3s3_wgrad"), (True, "decnet_deconv2d_k3s3_wgrad")):
        q = getattr(L, name + "_workspace_floats")
        q.argtypes, q.restype = [ctypes.c_int] * 5, ctypes.c_size_t
        assert q(8, 225, 72, 60, 108) == 0 and q(8, 72, 225, 60, 108) == 0 and q(0, 72, 24, 60, 108) == 0
        assert q(8, 72, 24, 0, 108) == 0 and q(8, 72, 24, 60, -1) == 0
        n = q(8, 72, 216, 60, 108)
        assert n > 0 and n % 4 == 0
        if not tr:                                                      # whole partial sets [Cout][9 Cin + 1]
            assert n % (216 * (72 * 9 + 1)) == 0
        assert q(1, 16, 16, 1, 1) > 0
        f = getattr(L, name)
        f.argtypes = _lib.SIGNATURES[name]
        ok = (one, one, None, None, one, one, one, 1 << 20, 1, 16, 16, 2, 2, None)
        for i in (0, 1, 4, 5, 6):                                       # x, gy, G, gsum, workspace
            assert f(*[None if j == i else a for j, a in enumerate(ok)]) == -1, (name, i)
        assert f(one, one, one, None, one, one, one, 1 << 20, 1, 16, 16, 2, 2, None) == -1      # y without gm
        for i in range(8, 13):                                          # B, Cin, Cout, H, W
            assert f(*[0 if j == i else a for j, a in enumerate(ok)]) == -2, (name, i)
        assert f(*[225 if j == 9 else a for j, a in enumerate(ok)]) == -3
        assert f(*[225 if j == 10 else a for j, a in enumerate(ok)]) == -3
        assert f(*[4 if j == 7 else a for j, a in enumerate(ok)]) == -2                        # workspace too short
        assert f(*[ctypes.c_void_p(68) if j == 6 else a for j, a in enumerate(ok)]) == -5      # misaligned workspace
    for name in ("decnet_d2s3_pad1", "decnet_s2d3_pad0"):
        f = getattr(L, name)
        f.argtypes = _lib.SIGNATURES[name]
        assert f(None, one, 1, 1, 1, 1, None) == -1 and f(one, None, 1, 1, 1, 1, None) == -1
        for i in range(2, 6):
            assert f(*[0 if j == i else a for j, a in enumerate((one, one, 1, 1, 1, 1, None))]) == -2, (name, i)
        assert f(one, one, 256, 256, 1, 1, None) == -3                  # B C: a grid dimension
    assert L.decnet_d2s3_pad1(one, one, 1, 1, 65536, 1, None) == -3 and L.decnet_s2d3_pad0(one, one, 1, 1, 21846, 1, None) == -3
