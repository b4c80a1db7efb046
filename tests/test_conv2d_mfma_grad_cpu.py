"""CPU side of the matrix-core conv backward (decnet_amd/conv2d_grad.Conv2dMfmaFunction, csrc/conv2d_mfma_grad.hip):
  * Unit._grad_route_mfma row by row over tests/_model_cases.py, decided at the default switches; Unit._grad_route unchanged;
  * on the CPU a Unit of an "mfma" shape is untouched by hip_grad() (no library lookup, TALLY as without it);
  * the imposed-mask chain reference of tests/_conv2d_mfma_grad_ref.py equals plain float64 autograd where no ReLU branch
    is in doubt;
  * the query and the entry are declared in include/decnet_hip.h and bound in _lib.py with matching signatures, and the
    query's refusals and one size."""
import ctypes
import os
import re

import pytest
import torch

import _conv2d_mfma_grad_ref as MG
import _model_cases as MC
from decnet_amd import hip_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


def _expected_mfma(c):
    """"mfma" exactly where the route is "mfma" within the entry's 224 channels, less the measured exclusions
    (profiles/conv2d_mfma_grad.json): from 6480 pixels on, every unit below 58320 pixels (the two measured sizes) and the units
    with at most 24 inputs and 24 outputs at any size.  Nothing is excluded below 6480 pixels (nothing was measured there)."""
    if c["route"] != "mfma" or c["cin"] > 224 or c["cout"] > 224:
        return None
    hw = c["H"] * c["W"]
    return None if hw >= 6480 and (hw < 58320 or (c["cin"] <= 24 and c["cout"] <= 24)) else "mfma"


def _expected_conv(c):
    return "conv" if c["route"] == "conv" and c["cin"] <= 24 and c["H"] * c["W"] >= 256 else None


@pytest.mark.parametrize("name", sorted(MC.UNIT_CASES))
@pytest.mark.parametrize("env", [None, "torch"])
def test_grad_route_mfma_rows(name, env, monkeypatch):
    c = MC.UNIT_CASES[name]
    monkeypatch.delenv("DECNET_CONV2D", raising=False)
    monkeypatch.delenv("DECNET_CONV2D_MFMA", raising=False)
    u = MC.make_unit(c["cin"], c["cout"], c["k"], **c["kw"])
    parts = None if c["parts"] is None else len(c["parts"])
    assert u._route(c["B"], c["H"], c["W"], parts) == c["route"]
    if env is not None:
        monkeypatch.setenv("DECNET_CONV2D", env)
        monkeypatch.setenv("DECNET_CONV2D_MFMA", "0")
    want = _expected_mfma(c)
    assert u._grad_route_mfma(c["B"], c["H"], c["W"], parts) == want
    if c["route"] != "mfma":
        assert want is None                                             # every conv, s3, deconv and library row
    assert u._grad_route(c["B"], c["H"], c["W"], parts) == _expected_conv(c)       # unchanged


def test_grad_route_mfma_limits():
    assert MC.make_unit(73, 81, 3)._grad_route_mfma(4, 180, 324) == "mfma"
    assert MC.make_unit(48, 24, 3)._grad_route_mfma(4, 180, 324, 2) == "mfma"
    assert MC.make_unit(224, 224, 1)._grad_route_mfma(1, 64, 64) == "mfma"
    assert MC.make_unit(225, 24, 1)._grad_route_mfma(1, 64, 64) is None   # the entry's 224 channels
    assert MC.make_unit(24, 225, 1)._grad_route_mfma(1, 64, 64) is None
    assert MC.make_unit(24, 24, 3)._grad_route_mfma(1, 63, 65) is None    # 4095 pixels: the library's
    assert MC.make_unit(8, 25, 3, stride=3)._grad_route_mfma(1, 72, 64) is None            # "mfma_s3": out of scope
    assert MC.make_unit(16, 9, 3, stride=3, transposed=True)._grad_route_mfma(1, 16, 32) is None
    # the measured exclusions, at their literal thresholds: 6480 and 58320 pixels, 24 channels
    assert MC.make_unit(217, 81, 3)._grad_route_mfma(4, 60, 108) is None  # 6480 pixels
    assert MC.make_unit(81, 81, 3)._grad_route_mfma(4, 179, 325) is None  # 58175
    assert MC.make_unit(81, 81, 3)._grad_route_mfma(4, 243, 240) == "mfma"  # 58320
    assert MC.make_unit(81, 81, 3)._grad_route_mfma(1, 180, 324) == "mfma"  # (B plays no part)
    assert MC.make_unit(81, 81, 3)._grad_route_mfma(4, 79, 82) == "mfma"  # 6478: below everything measured
    assert MC.make_unit(81, 81, 3)._grad_route_mfma(4, 80, 81) is None    # 6480
    assert MC.make_unit(24, 24, 3)._grad_route_mfma(4, 180, 324) is None and MC.make_unit(24, 24, 1)._grad_route_mfma(4, 180, 324) is None
    assert MC.make_unit(25, 24, 3)._grad_route_mfma(4, 180, 324) == "mfma" and MC.make_unit(24, 25, 3)._grad_route_mfma(4, 180, 324) == "mfma"
    assert MC.make_unit(24, 24, 3)._grad_route_mfma(1, 64, 64) == "mfma"


def test_cpu_unit_is_untouched_by_hip_grad(monkeypatch):
    from decnet_amd import _lib, model

    def no_lib():
        raise AssertionError("a CPU unit looked the library up")

    monkeypatch.setattr(_lib, "lib", no_lib)
    u = MC.make_unit(24, 24, 3)
    assert u._grad_route_mfma(1, 64, 64) == "mfma"
    x = torch.randn(1, 24, 64, 64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    model.TALLY = []
    try:
        want = u(x)
        tally_off = [t["family"] for t in model.TALLY]
        del model.TALLY[:]
        with hip_grad():
            got = u(x)
            parts = u((x[:, :8], x[:, 8:]))
        tally_on = [t["family"] for t in model.TALLY]
    finally:
        model.TALLY = None
    gw = torch.autograd.grad(want.sum(), [x, u.conv.weight])
    gg = torch.autograd.grad(got.sum(), [x, u.conv.weight])
    assert torch.equal(got, want) and torch.equal(parts, want)
    assert all(torch.equal(a, b) for a, b in zip(gg, gw))
    assert tally_off == ["library"] and tally_on == ["library", "library"]


def test_imposed_mask_reference_equals_float64_autograd():
    """On a chain whose float64 pre-activations all keep a margin from zero, imposing the chain's own masks changes nothing:
    gradients equal plain autograd (relu) to 1e-12 relative, and the masks are the ones the free run took."""
    from decnet_amd.model import _c3, _seq
    g = torch.Generator().manual_seed(5)
    seq = MC.seeded(lambda: _seq(_c3(6, 5), _c3(5, 5), _c3(5, 4, relu=False)), 77)
    parts = [torch.randn(2, 4, 7, 9, generator=g), torch.randn(2, 2, 7, 9, generator=g)]
    r = torch.randn(2, 4, 7, 9, generator=g)
    free, masks = MG.chain_grads(seq, parts, r, D)
    assert [m is None for m in masks] == [False, False, True]
    x = torch.cat([t.to(D) for t in parts], 1)
    for u in seq[:2]:                                                   # no branch in doubt
        x = MG.unit_pre(u.double(), x)
        assert float(x.detach().abs().min()) > 1e-9
        x = torch.relu(x)
    imposed, took = MG.chain_grads(seq, parts, r, D, masks)
    assert all(a is b for a, b in zip(took, masks))
    # torch's own modules: Unit.forward on the CPU is conv -> BatchNorm -> ReLU
    import copy
    m = copy.deepcopy(seq).double()
    xs = [t.to(D).requires_grad_() for t in parts]
    (m(torch.cat(xs, 1)) * r.to(D)).sum().backward()
    own = {n: p.grad for n, p in m.named_parameters()}
    own.update({"part%d" % i: t.grad for i, t in enumerate(xs)})
    assert own.keys() == imposed.keys() == free.keys()
    for k, ref in own.items():
        scale = max(1e-300, float(ref.abs().max()))
        assert float((imposed[k] - ref).abs().max()) <= 1e-12 * scale, k
        assert float((free[k] - ref).abs().max()) <= 1e-12 * scale, k
    # and a flipped mask does change the gradients (the masks are used, in forward and backward)
    flipped = [~masks[0], masks[1], None]
    other, _ = MG.chain_grads(seq, parts, r, D, flipped)
    assert float((other["0.conv.weight"] - own["0.conv.weight"]).abs().max()) > 1e-6


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


def test_entries_and_signatures():
    from decnet_amd import _lib, build
    for name, ret in (("decnet_conv2d_mfma_wgrad_workspace_floats", "size_t"), ("decnet_conv2d_mfma_wgrad", "int")):
        got_ret, args = _header_decl(name)
        assert got_ret == ret
        assert [_ctype(a) for a in args] == _lib.SIGNATURES[name], name
    # the same argument list as the few-channel entry, argument for argument
    assert _header_decl("decnet_conv2d_mfma_wgrad")[1] == _header_decl("decnet_conv2d_wgrad")[1]
    assert _lib.SIGNATURES["decnet_conv2d_mfma_wgrad"] == _lib.SIGNATURES["decnet_conv2d_wgrad"]
    L = ctypes.CDLL(build.build())                                      # hipcc cross-compiles for gfx950 without a GPU
    q = L.decnet_conv2d_mfma_wgrad_workspace_floats
    q.argtypes, q.restype = [ctypes.c_int] * 6, ctypes.c_size_t
    assert q(4, 217, 81, 60, 108, 2) == 0 and q(4, 225, 81, 60, 108, 3) == 0 and q(4, 217, 225, 60, 108, 3) == 0
    n = q(4, 217, 81, 60, 108, 3)
    assert n > 0 and n % 4 == 0 and n % (81 * (217 * 9 + 1)) == 0       # whole partial sets [Cout][Cin k k + 1]
    assert q(1, 16, 12, 2, 3, 3) > 0                                    # fewer channels than the route ever sends
    # refusals before any launch (no GPU here): NULL, and y without gm
    f = L.decnet_conv2d_mfma_wgrad
    f.argtypes = _lib.SIGNATURES["decnet_conv2d_mfma_wgrad"]
    one = ctypes.c_void_p(64)
    assert f(None, one, 1, one, None, None, one, one, one, 4, 1, 1, 1, 1, 1, 1, None) == -1
    xs, cins = (ctypes.c_void_p * 1)(64), (ctypes.c_int * 1)(16)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)                      # noqa: E731
    assert f(vp(xs), vp(cins), 1, one, one, None, one, one, one, 4, 1, 1, 1, 1, 1, 1, None) == -1
    assert f(vp(xs), vp(cins), 1, one, None, None, one, one, one, 4, 1, 1, 1, 1, 2, 1, None) == -3
    assert f(vp(xs), vp(cins), 1, one, None, None, one, one, one, 4, 1, 225, 1, 1, 1, 1, None) == -3
    assert f(vp(xs), vp(cins), 1, one, None, None, one, one, one, 4, 1, 1, 1, 1, 1, 1, None) == -2      # workspace too short
