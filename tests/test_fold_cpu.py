"""The shared pieces of the Python dispatch layer, as far as they show without a GPU: ``fold_bn`` / ``fold_none``
(decnet_amd/stage0.py) against the float64 formula and, bit for bit, against the expressions they replaced;
``CachesWeights._cached``; and the argument checks of the tensor-level wrappers (decnet_amd/ops2d.py), which come before
any library lookup."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _model_cases as MC  # noqa: E402
import _model_ref as MR  # noqa: E402


# ---- the fold -------------------------------------------------------------------------------------------------------------
def _close64(got, ref):
    # one float32 rounding per operation of a three-operation chain on values of order 1
    assert got.dtype == torch.float32 and float((got.double() - ref).abs().max()) <= 4 * 2.0 ** -24 * max(1.0, float(ref.abs().max()))


def test_fold_bn_with_an_eps_that_matters():
    """eps = 0.3 against variances in 0.5 .. 1.5 (tests/_model_cases.randomise_bn)."""
    from decnet_amd.stage0 import fold_bn
    u = MC.make_unit(6, 5, 3, eps=0.3, seed=3)
    bn = u.bn
    assert 0.5 <= float(bn.running_var.min()) and float(bn.running_var.max()) <= 1.5
    with torch.no_grad():
        scale, shift = fold_bn(bn)
        # the expressions at the parent commit (Unit._folded, five sites in fp32; Unit._folded_torch in the parameters' dtype)
        s0 = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
        b0 = bn.bias.float() - bn.running_mean.float() * s0
        assert torch.equal(scale, s0) and torch.equal(shift, b0)
        p = MR.unit_params(u)["bn"]                             # the float64 values the reference module folds
        ref_s = p["g"] / torch.sqrt(p["v"] + p["eps"])
        _close64(scale, ref_s)
        _close64(shift, p["b"] - p["m"] * ref_s)
        d = u.double()
        s_own, b_own = fold_bn(d.bn, fp32=False)
        assert s_own.dtype == torch.float64
        s1 = d.bn.weight / torch.sqrt(d.bn.running_var + d.bn.eps)
        assert torch.equal(s_own, s1) and torch.equal(b_own, d.bn.bias - d.bn.running_mean * s1)
        assert fold_bn(d.bn)[0].dtype == torch.float32


@pytest.mark.parametrize("bias", [True, False])
def test_fold_none(bias):
    from decnet_amd.stage0 import fold_none
    u = MC.make_unit(4, 3, 3, bn=False, bias=bias, seed=5)
    c = u.conv
    with torch.no_grad():
        scale, shift = fold_none(c)
        # the expressions at the parent commit
        s0 = torch.ones(3, device=c.weight.device)
        b0 = c.bias.float() if c.bias is not None else torch.zeros(3, device=c.weight.device)
    assert torch.equal(scale, s0) and torch.equal(shift, b0) and scale.dtype == shift.dtype == torch.float32
    assert bias == bool(shift.abs().max() > 0)


def test_fold_against_the_reference_module():
    """scale * conv(x) + shift with the folded pair is the float64 reference's Unit (tests/_model_ref.unit)."""
    from decnet_amd.stage0 import fold_bn, fold_none
    for kw in (dict(eps=0.3), dict(bn=False), dict(bn=False, bias=False)):
        u = MC.make_unit(4, 3, 3, relu=False, seed=7, **kw)
        x = torch.randn(2, 4, 6, 7, generator=torch.Generator().manual_seed(1))
        ref = MR.unit(x, MR.unit_params(u))
        with torch.no_grad():
            scale, shift = fold_bn(u.bn) if u.bn is not None else fold_none(u.conv)
            got = torch.nn.functional.conv2d(x.double(), u.conv.weight.double(), None, 1, 1) * scale.double().view(1, -1, 1, 1) \
                + shift.double().view(1, -1, 1, 1)
        assert MC.close(got, ref, 1e-6) <= 1.0, kw


# ---- _cached ----------------------------------------------------------------------------------------------------------------
def test_cached_rebuilds_when_its_sources_change_and_only_then():
    from decnet_amd.model import Unit
    from decnet_amd.stage0 import cache_attrs
    torch.manual_seed(0)
    u = Unit(5, 4, 3, pad=1).eval()
    built = []

    def get(extra=(1,)):
        return u._cached("_fold", u._sources(), extra, lambda: built.append(torch.is_grad_enabled()) or len(built))
    assert get() == 1 and get() == 1 and built == [False]              # (built under no_grad)
    assert u._fold == 1 and u._fold_key[-1] == 1 and len(u._fold_key) == 6
    assert [t.data_ptr() for t in u._fold_src] == [t.data_ptr() for t in u._sources()]
    with torch.no_grad():
        u.conv.weight.mul_(2)                                          # an in-place write under no_grad
    assert get() == 2 and get() == 2
    u.bn.weight.data = torch.ones(4)                                   # a re-assigned .data
    assert get() == 3 and get() == 3
    assert get((2,)) == 4 and get((2,)) == 4                           # the plain values that go into the packing
    assert u._cached("_fold", u._sources(), (2,), lambda: 9, head=("a",)) == 9 and u._fold_key[0] == "a"
    assert Unit._CACHE_ATTRS == cache_attrs("_fold", "_mfold", "_tfold") and cache_attrs("_x") == ("_x", "_x_key", "_x_src")
    assert all(hasattr(u, a) for a in ("_fold", "_fold_key", "_fold_src"))
    u._drop_caches()
    assert not any(hasattr(u, a) for a in Unit._CACHE_ATTRS)
    assert get((2,)) == 5 and get((2,)) == 5


def test_cached_keeps_nothing_of_a_build_that_raised():
    u = MC.make_unit(5, 4, 3)
    with pytest.raises(ZeroDivisionError):
        u._cached("_fold", u._sources(), (), lambda: 1 // 0)
    assert not hasattr(u, "_fold") and not hasattr(u, "_fold_key")


# ---- the wrappers' argument checks ----------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """A host tensor that says it is on the GPU: what a wrapper's checks see of a device tensor.  They refuse the call
    before anything looks the library up or reads an address."""
    is_cuda = True


def _g(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnGpu)


def _wrapper_cases():
    from decnet_amd import ops2d
    x, w, s = _g(2, 4, 6, 7), _g(99), _g(5)
    parts = lambda x: [x, _g(2, 3, 6, 7)]                             # noqa: E731
    return {
        "conv2d_cat_bn_act": (lambda x=x, out=None, cin=7: ops2d.conv2d_cat_bn_act(parts(x), w, s, s, cin, 3, 1, True, out=out),
                              (2, 5, 6, 7)),
        "conv2d_mfma_cat_bn_act": (lambda x=x, out=None, cin=7: ops2d.conv2d_mfma_cat_bn_act(
            parts(x), _g(99, dtype=torch.uint8), s, s, cin, 3, 1, True, out=out), (2, 5, 6, 7)),
        "deconv2d_k3s3_bn_act": (lambda x=x, out=None, cin=4: ops2d.deconv2d_k3s3_bn_act(x, w, s, s, cin, True, out=out),
                                 (2, 5, 18, 21)),
        "detail_mask": (lambda x=_g(2, 3, 6, 7), out=None, cin=3: ops2d.detail_mask(
            x if cin == 3 else _g(2, cin, 6, 7), _g(2, 3, 6, 7), (None,) * 6, 0.5, out=out), (2, 6, 7)),
    }


@pytest.fixture()
def no_library(monkeypatch):
    from decnet_amd import ops

    def never(name):
        raise AssertionError("%s was looked up before the arguments were checked" % name)
    monkeypatch.setattr(ops, "_fn", never)
    import decnet_amd.ops2d as ops2d
    monkeypatch.setattr(ops2d, "_fn", never)


@pytest.mark.parametrize("name", ["conv2d_cat_bn_act", "conv2d_mfma_cat_bn_act", "deconv2d_k3s3_bn_act", "detail_mask"])
def test_wrapper_refuses_bad_arguments(no_library, name):
    from decnet_amd import DecnetHipError
    call, out_shape = _wrapper_cases()[name]
    x = _g(2, 3, 6, 7) if name == "detail_mask" else _g(2, 4, 6, 7)
    with pytest.raises(DecnetHipError):
        call(x=torch.zeros(x.shape))                                   # a CPU tensor
    with pytest.raises(TypeError):
        call(x=_g(*x.shape, dtype=torch.float64))
    with pytest.raises(AssertionError, match="contiguous"):
        call(x=_g(2, 7, 6, x.shape[1]).permute(0, 3, 2, 1))            # the right shape, strided
    with pytest.raises(ValueError):
        call(out=_g(*out_shape[:-1], out_shape[-1] + 1))
    with pytest.raises(ValueError):
        call(cin=8 if name != "detail_mask" else 4)                    # channels that are not the layer's Cin
