"""The bookkeeping of the packed-weight caches of decnet_amd/model.py and stage0.py, as far as it shows without a GPU:
what the cache key sees, which of the project's own write paths drop the caches, and that caches take no part in copying
or pickling.  (Values after each kind of weight change: tests/test_model_state_gpu.py.)"""
import copy
import io
import os
import pickle
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from make_golden import E2E_KW  # noqa: E402
from netparams import fill_state_dict  # noqa: E402


def _unit():
    from decnet_amd.model import Unit
    torch.manual_seed(0)
    return Unit(5, 4, 3, pad=1).eval()


def test_what_the_cache_key_sees():
    from decnet_amd.stage0 import source_key
    u = _unit()
    ts = u._sources()
    assert len(ts) == 5
    k0 = source_key(ts, u.bn.eps)
    with torch.no_grad():
        u.conv.weight.mul_(2)
    k1 = source_key(ts, u.bn.eps)
    assert k1 != k0
    u.bn.running_var.detach().add_(1)
    k2 = source_key(ts, u.bn.eps)
    assert k2 != k1
    u.bn.eps = 1e-3
    k3 = source_key(u._sources(), u.bn.eps)
    assert k3 != k2
    u.bn.weight.data = torch.ones(4)                        # other memory while the old one is still owned
    assert source_key(u._sources(), u.bn.eps) != k3
    # the documented blind spot: a write THROUGH .data changes neither address nor version
    k4 = source_key(u._sources(), u.bn.eps)
    u.conv.weight.data.copy_(torch.zeros_like(u.conv.weight))
    u.bn.running_var.data.fill_(3.0)
    assert source_key(u._sources(), u.bn.eps) == k4


def test_a_cache_entry_owns_the_memory_it_was_built_from():
    """``p.data = other`` keeps ``_version`` and frees the old tensor, whose address the allocator may hand out again: the
    entry keeps aliases of its sources, so that address stays taken as long as the entry could match it."""
    u = _unit()
    w0, _ = u._folded_torch()
    ptr = u.conv.weight.data_ptr()
    u.conv.weight.data = torch.randn(4, 5, 3, 3)
    assert u._tfold_src[0].data_ptr() == ptr
    later = [torch.empty(4, 5, 3, 3) for _ in range(64)]
    assert all(t.data_ptr() != ptr for t in later)
    w1, _ = u._folded_torch()
    assert not torch.equal(w0, w1)
    assert u._tfold_src[0].data_ptr() == u.conv.weight.data_ptr()


def test_drop_weight_caches_and_the_write_through_data():
    from decnet_amd import drop_weight_caches
    u = _unit()
    u._folded_torch()
    u.conv.weight.data.copy_(torch.randn(4, 5, 3, 3))
    assert drop_weight_caches(u) is u
    assert not hasattr(u, "_tfold") and not hasattr(u, "_tfold_key")
    w, b = u._folded_torch()
    scale = u.bn.weight / torch.sqrt(u.bn.running_var + u.bn.eps)
    assert torch.equal(w, (u.conv.weight * scale.view(-1, 1, 1, 1)).detach())


def _warm(model):
    """Stand-ins for what a forward on the GPU leaves behind, ctypes objects included."""
    import ctypes
    from decnet_amd import _lib
    n = 0
    for m in model.modules():
        for a in getattr(m, "_CACHE_ATTRS", ()):
            if a != "_ws":
                setattr(m, a, (ctypes.c_float * 3)(1, 2, 3))
                n += 1
    reg = model.cost_regularizer
    reg._ws[("s0params", "dev")] = ([], 1, _lib.Stage0Params())
    reg._ws[("s0", "dev")] = torch.zeros(4)
    return n


def _cold(model):
    for m in model.modules():
        for a in getattr(m, "_CACHE_ATTRS", ()):
            v = m.__dict__.get(a)
            if v is not None and v != {}:
                return False
    return True


@pytest.fixture()
def net():
    from decnet_amd.model import get_model
    torch.manual_seed(1)
    return get_model(**E2E_KW).eval()


def test_own_write_paths_drop_the_caches(net):
    from decnet_amd.model import load_reference_checkpoint
    sd = fill_state_dict(net.state_dict())
    for write in (lambda: net._initialize_weights(), lambda: net.load_state_dict(sd),
                  lambda: net.load_state_dict({k: v.clone() for k, v in sd.items()}, assign=True),
                  lambda: load_reference_checkpoint(net, {"module." + k: v for k, v in sd.items()}),
                  lambda: net.to(torch.float64), lambda: net.float(), lambda: net.cpu()):
        assert _warm(net) > 100 and not _cold(net)
        write()
        assert _cold(net)


def test_a_warm_model_can_be_copied_and_pickled(net):
    _warm(net)
    with pytest.raises(ValueError):                         # what the caches hold cannot be pickled ...
        pickle.dumps(net.cost_regularizer._ws)
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    for c in (copy.deepcopy(net), pickle.loads(pickle.dumps(net)), torch.load(buf, weights_only=False)):
        assert _cold(c) and not _cold(net)                  # ... so they stay behind: a copy starts cold
        assert c.cost_regularizer._ws == {} and c.cost_regularizer._packed is None
        for (k, a), (_, b) in zip(net.state_dict().items(), c.state_dict().items()):
            assert torch.equal(a, b) and (a.data_ptr() != b.data_ptr() or a.numel() == 0), k
