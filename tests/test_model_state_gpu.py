"""One model, many calls: what decnet_amd/model.py and stage0.py keep between calls (six packed-weight caches, five
workspace caches) must never change a result.  Every comparison is BIT FOR BIT against a fresh model that holds the same
weights and is called once -- both run the same kernels on the same values, so no tolerance applies.  -m gpu.

The whole net runs at base_channels 2 (tests/golden/make_golden.py's E2E_KW).  Its small planes (54 x 243 and the like)
stay on the few-channel kernels and the library; the 432 x 864 plane of test_shapes_* is the smallest on which the net's
own layers reach the three matrix-core routes (1/9 resolution = 48 x 96 >= 4608 pixels for the stride-3 18 -> 54 layer,
1/27 = 16 x 32 >= 512 for the 54 -> 18 transposed one), asserted there with the C-entry spy.  Every route is also
covered by a module of its own (MODULES).
"""
import copy
import io
import os
import pickle
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from make_golden import E2E_KW  # noqa: E402
from netparams import fill_state_dict  # noqa: E402
from spy_util import entry_spy  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import decnet_amd  # noqa: F401
    return torch.device("cuda:0")


def _pair(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)


# ---- subjects: (constructor, run(module, dev) -> tuple of tensors, C entry that proves the route) ---------------------
def _net(**kw):
    from decnet_amd.model import get_model
    return get_model(**dict(E2E_KW, **kw))


def _run_net(m, dev, shape=(1, 54, 243), seed=0):
    l, r = _pair(*shape, seed=seed)
    return (m(l.to(dev), r.to(dev))[-1],)


def _x(dev, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(dev)


def _unit(*a, **kw):
    from decnet_amd.model import Unit
    return lambda: Unit(*a, **kw)


def _aspp():
    from decnet_amd.model import ASPP
    return ASPP(16, 16, [1, 2, 3])


def _maskgen():
    from decnet_amd.model import GenerateSparseMask
    return GenerateSparseMask(4, 3)


def _run_mask(m, dev):
    cur, pre = _x(dev, 2, 4, 12, 66), _x(dev, 2, 12, 4, 22)
    return sum((m.mask(cur, pre, th, want_bits=True) for th in (0.4, 0.5, 0.6)), ())


def _reg(cost_func):
    from decnet_amd.stage0 import CostRegNetNoDown
    return lambda: CostRegNetNoDown(24, 48, cost_func)


def _run_reg(m, dev):
    L, R = torch.relu(_x(dev, 2, 24, 5, 9)), torch.relu(_x(dev, 2, 24, 5, 10)[..., 1:])
    # D 8 / 2 / 8: winograd444 / winograd4 / winograd444 through prepare()'s one slot; the next run starts with the
    # algorithm the last one ended with, so a Stage0Params of that algorithm is there to go stale
    return (m.stage0(L, R, 8), m.stage0(L, R, 2), m.stage0(L, R, 8))


MODULES = {
    "net": (_net, _run_net, "decnet_stage0_forward_cf"),
    "unit_conv": (_unit(8, 8, 3, pad=1), lambda m, d: (m(_x(d, 2, 8, 20, 30)),), "decnet_conv2d_bn_act"),
    "unit_conv_cat": (_unit(9, 4, 3, pad=1), lambda m, d: (m((_x(d, 2, 8, 20, 30), _x(d, 2, 1, 20, 30))),),
                      "decnet_conv2d_cat_bn_act"),
    "unit_mfma": (_unit(24, 24, 3, pad=1), lambda m, d: (m(_x(d, 1, 24, 64, 64)),), "decnet_conv2d_mfma_cat_bn_act"),
    "unit_mfma_s3": (_unit(8, 32, 3, stride=3, pad=1), lambda m, d: (m(_x(d, 1, 8, 72, 66)),), "decnet_s2d3_pad1"),
    "unit_mfma_deconv": (_unit(16, 12, 3, stride=3, transposed=True), lambda m, d: (m(_x(d, 1, 16, 16, 32)),),
                         "decnet_deconv2d_mfma_k3s3_bn_act"),
    "unit_deconv": (_unit(6, 4, 3, stride=3, transposed=True), lambda m, d: (m(_x(d, 1, 6, 8, 8)),),
                    "decnet_deconv2d_k3s3_bn_act"),
    "unit_conv_s3": (_unit(4, 8, 3, stride=3, pad=1), lambda m, d: (m(_x(d, 1, 4, 30, 30)),), "decnet_conv2d_k3s3_bn_act"),
    "unit_library": (_unit(32, 32, 3, pad=1), lambda m, d: (m(_x(d, 1, 32, 10, 10)),), "decnet_bias_act_inplace"),
    "unit_library_deconv": (_unit(32, 16, 3, stride=3, transposed=True), lambda m, d: (m(_x(d, 1, 32, 5, 5)),),
                            "decnet_bias_act_inplace"),
    "aspp": (_aspp, lambda m, d: (m(_x(d, 1, 16, 12, 12)),), "decnet_tap_gemm"),
    "maskgen": (_maskgen, _run_mask, "decnet_detail_mask"),
    "reg_cor": (_reg("cor"), _run_reg, "decnet_stage0_forward_cf"),
    "reg_cat": (_reg("cat"), _run_reg, "decnet_stage0_forward_cf"),
}


def _state(module, seed):
    return fill_state_dict(module.state_dict(), seed=seed)


def _build(name, sd, dev, tweak=None):
    """A fresh module that holds sd, on the GPU, never called."""
    m = MODULES[name][0]()
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    if tweak is not None:
        tweak(m)
    return m


def _run(name, m, dev, **kw):
    with torch.no_grad():
        out = MODULES[name][1](m, dev, **kw)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _tensors(m):
    return dict(list(m.named_parameters()) + list(m.named_buffers()))


# ---- ways to change the weights of a module that has run ------------------------------------------------------------------
def ch_load_state_dict(m, new, dev):
    m.load_state_dict(new)


def ch_load_reference_checkpoint(m, new, dev):
    from decnet_amd.model import load_reference_checkpoint
    load_reference_checkpoint(m, {"module." + k: v for k, v in new.items()})


def ch_copy_in_place(m, new, dev):
    with torch.no_grad():
        for k, t in _tensors(m).items():
            t.copy_(new[k])


def ch_add_in_place(m, new, dev):
    with torch.no_grad():
        for k, t in _tensors(m).items():
            if t.is_floating_point():
                t.add_(new[k].to(dev) - t)                  # (not exactly new: the comparison reads m's own state back)


def ch_data_copy_then_drop(m, new, dev):
    """The documented contract (stage0.source_key): a write through .data is invisible to the cache keys and
    needs drop_weight_caches.  What the caches hold without that call is not asserted."""
    from decnet_amd import drop_weight_caches
    for k, t in _tensors(m).items():
        t.data.copy_(new[k])
    drop_weight_caches(m)


def ch_data_assign(m, new, dev):
    for k, t in _tensors(m).items():
        t.data = new[k].to(dev)


def ch_data_assign_twice(m, new, dev):
    """A -> B -> A on the addresses: the first assignment frees the tensors the caches were built from, the second one's
    tensors are allocated right after and, with a caching allocator, land where those were -- same address, same
    ``_version`` (``.data =`` keeps it), other values.  No forward in between."""
    other = _state(m, 4321)
    for k, t in _tensors(m).items():
        t.data = other[k].to(dev)
    torch.cuda.synchronize()
    for k, t in _tensors(m).items():
        t.data = new[k].to(dev)


def ch_load_assign(m, new, dev):
    m.load_state_dict({k: v.to(dev) for k, v in new.items()}, assign=True)


def ch_cpu_load_cuda(m, new, dev):
    m.cpu()
    m.load_state_dict(new, assign=True)
    m.to(dev)


def ch_bn_stats_alone(m, new, dev):
    with torch.no_grad():
        for k, t in _tensors(m).items():
            if k.endswith(("running_mean", "running_var")):
                t.copy_(new[k])


def ch_bn_eps(m, new, dev):
    def tweak(x):
        for s in x.modules():
            if isinstance(s, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
                s.eps = 0.5
    tweak(m)
    return tweak


CHANGES = [ch_load_state_dict, ch_load_reference_checkpoint, ch_copy_in_place, ch_add_in_place, ch_data_copy_then_drop,
           ch_data_assign, ch_data_assign_twice, ch_load_assign, ch_cpu_load_cuda, ch_bn_stats_alone, ch_bn_eps]


# (load_reference_checkpoint is a loader of the whole net)
@pytest.mark.parametrize("name,change", [(n, c) for n in MODULES for c in CHANGES
                                         if n == "net" or c is not ch_load_reference_checkpoint],
                         ids=lambda v: v if isinstance(v, str) else v.__name__[3:])
def test_weights_changed_after_the_first_forward(dev, name, change):
    m = _build(name, _state(MODULES[name][0](), 1), dev)
    with entry_spy() as calls:
        before = _run(name, m, dev)
    assert MODULES[name][2] in calls, (name, calls)          # the route this subject stands for
    new = _state(m, 2)
    tweak = change(m, new, dev)
    got = _run(name, m, dev)
    want = _run(name, _build(name, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, dev, tweak), dev)
    assert not _same(before, want), "the change did not change the result: the case tests nothing"
    assert _same(got, want), "a module that ran before the change differs from a fresh one with the same weights"


def test_initialize_weights_after_a_forward(dev):
    """SparseDenseNetRefinementMask._initialize_weights writes through .data only (as the reference's does): forward,
    re-initialise under another seed, forward must give the new weights' result."""
    torch.manual_seed(3)
    m = _net().to(dev).eval()
    before = _run("net", m, dev)
    torch.manual_seed(4)
    m._initialize_weights()
    got = _run("net", m, dev)
    want = _run("net", _build("net", {k: v.cpu().clone() for k, v in m.state_dict().items()}, dev), dev)
    assert not _same(before, want)
    assert _same(got, want)


def test_settings_changed_after_the_first_forward(dev):
    """unit.relu and model.thold are read per call, not cached: flipping them after a forward takes effect."""
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    before = _run("net", m, dev)

    def relu_off(x):
        x.feature_extractor.conv0[1].relu = False
        x.feature_extractor.conv2[1].relu = False

    def thold(x):
        x.thold = 0.45
    for tweak in (relu_off, thold):
        tweak(m)
        got = _run("net", m, dev)
        want = _run("net", _build("net", sd, dev, lambda x: (relu_off(x), tweak(x))), dev)
        assert not _same(before, want)
        assert _same(got, want), tweak.__name__
        before = want
    sd_u = _state(MODULES["unit_mfma"][0](), 1)
    u = _build("unit_mfma", sd_u, dev)
    before = _run("unit_mfma", u, dev)
    u.relu = False
    want = _run("unit_mfma", _build("unit_mfma", sd_u, dev, lambda x: setattr(x, "relu", False)), dev)
    assert not _same(before, want) and _same(_run("unit_mfma", u, dev), want)


# ---- shapes ---------------------------------------------------------------------------------------------------------------
def _poison(module):
    """NaN into every cached scratch buffer (CostRegNetNoDown._ws): nothing may read what an earlier call left."""
    n = 0
    for m in module.modules():
        for v in getattr(m, "_ws", {}).values():
            for t in (v if isinstance(v, (list, tuple)) else (v,)):
                if isinstance(t, torch.Tensor) and t.is_floating_point():
                    t.fill_(float("nan"))
                    n += 1
    return n


def test_shapes_big_small_big_with_poisoned_workspaces(dev):
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    big, small = (1, 432, 864), (1, 54, 243)
    with entry_spy() as calls:
        got = [_run("net", m, dev, shape=big)]
    for entry in ("decnet_conv2d_mfma_cat_bn_act", "decnet_deconv2d_mfma_k3s3_bn_act", "decnet_s2d3_pad1",
                  "decnet_conv2d_cat_epilogue", "decnet_detail_mask", "decnet_spamatvar_forward_bits"):
        assert entry in calls, entry                        # the matrix-core routes (and the rest) are what ran
    for shape in (small, big, (1, 81, 108)):
        assert _poison(m) >= 1                              # the workspaces are now larger than this call needs
        got.append(_run("net", m, dev, shape=shape))
    for g, shape in zip(got, (big, small, big, (1, 81, 108))):
        assert all(bool(torch.isfinite(t).all()) for t in g)
        assert _same(g, _run("net", _build("net", sd, dev), dev, shape=shape)), shape


def test_batch_sizes_2_1_3(dev):
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    for B in (2, 1, 3):
        _poison(m)
        got = _run("net", m, dev, shape=(B, 54, 243), seed=B)
        assert _same(got, _run("net", _build("net", sd, dev), dev, shape=(B, 54, 243), seed=B)), B


def test_max_disp_54_216_54(dev):
    """Stage 0 runs at D = max_disp / 27: 2 -> 8 -> 2 moves conv_algo from winograd4 to winograd444 and back, so
    prepare()'s single slot repacks and a new Stage0Params is built each time."""
    from decnet_amd.stage0 import conv_algo
    assert (conv_algo(2), conv_algo(8)) == ("winograd4", "winograd444")
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    res = {}
    for md in (54, 216, 54):
        m.max_disp = md
        _poison(m)
        got = _run("net", m, dev, shape=(2, 54, 243))
        want = _run("net", _build("net", sd, dev, lambda x: setattr(x, "max_disp", md)), dev, shape=(2, 54, 243))
        assert _same(got, want), md
        res[md] = got
    assert not _same(res[54], res[216])


def test_prepare_repacks_for_the_algorithm(dev):
    """CostRegNetNoDown.prepare keeps ONE slot, keyed by the weights and by the Conv3d algorithm the depth picks: asked
    for D = 2, 8, 2 it must hand back Winograd weights of that algorithm's size each time (checked on the buffers, before
    anything is launched on them), and the same object while nothing changes."""
    from decnet_amd import _lib
    from decnet_amd.stage0 import WINO_VARIANT, conv_algo
    reg = _build("reg_cor", _state(MODULES["reg_cor"][0](), 1), dev)
    last = None
    for D in (2, 8, 2):
        P = reg.prepare(D)
        assert P is not last and reg.prepare(D) is P
        n = _lib.lib().decnet_conv3d_wino_weight_floats(P[0]["Ci"], WINO_VARIANT[conv_algo(D)])
        assert all(p["u"].numel() == n for p in P[:7]), D
        assert reg._packed_key[0] == conv_algo(D)
        last = P
    assert _lib.lib().decnet_conv3d_wino_weight_floats(24, 1) != _lib.lib().decnet_conv3d_wino_weight_floats(24, 2)


# ---- copies ---------------------------------------------------------------------------------------------------------------
def _copies(m):
    yield "deepcopy", copy.deepcopy(m)
    yield "pickle", pickle.loads(pickle.dumps(m))
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    yield "torch.save", torch.load(buf, weights_only=False)


@pytest.mark.parametrize("name", ["net", "unit_conv", "unit_mfma", "unit_library", "aspp", "maskgen", "reg_cat"])
def test_copies_of_a_module_that_has_run(dev, name):
    """A module that has run holds ctypes structures (Stage0Params, the mask generator's host arrays) and device buffers
    in its caches; none of that takes part in copying or pickling: a copy starts cold, repacks, and is independent."""
    sd = _state(MODULES[name][0](), 1)
    m = _build(name, sd, dev)
    want = _run(name, m, dev)
    new = _state(m, 2)
    want_new = _run(name, _build(name, new, dev), dev)
    assert not _same(want, want_new)
    for how, c in _copies(m):
        assert all(s.__dict__.get(a) in (None, {}) for s in c.modules() for a in getattr(s, "_CACHE_ATTRS", ())), \
            how + ": a copy must start cold"
        assert _same(_run(name, c, dev), want), how
        ch_copy_in_place(c, new, dev)                        # the copy's weights change: the original's result stays
        assert _same(_run(name, c, dev), want_new), how
        assert _same(_run(name, m, dev), want), how
    c = copy.deepcopy(m)
    ch_copy_in_place(m, new, dev)                            # and the reverse
    assert _same(_run(name, m, dev), want_new)
    assert _same(_run(name, c, dev), want)


def test_replicas_of_a_module_that_has_run(dev):
    from torch.nn.parallel import replicate
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    want = _run("net", m, dev)
    with torch.no_grad():
        reps = replicate(m, [0, 0])
    for r in reps:
        assert r.cost_regularizer._ws == {}
        assert _same(_run("net", r, dev), want)
    assert _same(_run("net", m, dev), want)


# ---- capture --------------------------------------------------------------------------------------------------------------
def _capture(fn):
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
    return g, out


@pytest.mark.parametrize("name", ["unit_conv", "unit_mfma", "unit_library"])
def test_a_captured_unit_keeps_the_packed_weights_of_its_time(dev, name):
    """A captured graph holds the ADDRESSES of the packed weights of its time.  After a write through .data (which no
    cache key sees, so nothing is repacked or freed) the old graph still replays the old packed weights: expected, and
    asserted here.  drop_weight_caches + a new capture sees the new weights.  (The old graph is not replayed after the
    drop: its buffers are gone.)  This holds per packed layer, not for the whole net: its layers without BatchNorm on the
    library route and the last Conv3d of stage 0 read the parameters' own memory, so an old graph of the whole net would
    replay a mixture -- DESIGN.md says to capture again after any weight change."""
    from decnet_amd import drop_weight_caches
    sd = _state(MODULES[name][0](), 1)
    m = _build(name, sd, dev)
    x = _x(dev, *{"unit_conv": (2, 8, 20, 30), "unit_mfma": (1, 24, 64, 64), "unit_library": (1, 32, 10, 10)}[name])
    with torch.no_grad():
        want = m(x).clone()
    g1, out1 = _capture(lambda: m(x))
    g1.replay()
    torch.cuda.synchronize()
    assert torch.equal(out1, want)
    new = _state(m, 2)
    for k, t in _tensors(m).items():
        t.data.copy_(new[k])
    g1.replay()
    torch.cuda.synchronize()
    assert torch.equal(out1, want), "the old graph replays the packed weights it was captured with"
    del g1, out1
    drop_weight_caches(m)
    with torch.no_grad():
        want_new = _build(name, new, dev)(x).clone()
    assert not torch.equal(want_new, want)
    g2, out2 = _capture(lambda: m(x))
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, want_new)


def test_capture_of_the_net_with_warm_caches_and_after_a_weight_change(dev):
    """A forward captured after the caches are warm replays bit-identically; after load_state_dict (which drops the
    caches; the old graph is discarded first) a new capture sees the new weights."""
    sd = _state(_net(), 1)
    m = _build("net", sd, dev)
    l, r = (t.to(dev) for t in _pair(1, 54, 243))
    want = _run("net", m, dev)[0]
    g1, out1 = _capture(lambda: m(l, r)[-1])
    for _ in range(3):
        g1.replay()
    torch.cuda.synchronize()
    assert torch.equal(out1, want)
    del g1, out1
    new = _state(m, 2)
    m.load_state_dict(new)
    want_new = _run("net", _build("net", new, dev), dev)[0]
    assert not torch.equal(want_new, want)
    g2, out2 = _capture(lambda: m(l, r)[-1])
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, want_new)
