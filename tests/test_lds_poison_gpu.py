"""The LDS poison itself (tests/_lds_poison.py, tests/support/lds_poison.hip): that a poison launch reaches nearly all of
the device's LDS and survives until the entry under test starts, that the sweep catches a planted read of unwritten LDS,
and the model layer end to end with LDS poisoned before every module.  -m gpu."""
import os
import sys

import pytest
import torch

import _lds_poison as P
from _placement import Place

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    P.hooks()
    return torch.device("cuda:0")


@pytest.mark.parametrize("pat", P.PATTERNS, ids=["nan", "one"])
def test_a_poison_launch_is_visible_to_the_next_kernel(dev, pat):
    """Poison, then probe: at least MIN_SHARE of all LDS words the probe's workgroups read hold the pattern.  (The other
    pattern is written first, so that words left from an earlier test cannot count.)"""
    P.poison(P.PATTERNS[1] if pat == P.PATTERNS[0] else P.PATTERNS[0])
    share = P.visible_share(pat)
    print("visible share of 0x%08X at ROUNDS=%d: %.4f" % (pat, P.ROUNDS, share))
    assert share >= P.MIN_SHARE, "the poison reached %.1f%% of the probed LDS words" % (100 * share)


@pytest.mark.parametrize("pat", P.PATTERNS, ids=["nan", "one"])
def test_place_traffic_between_poison_and_entry_leaves_lds_alone(dev, pat):
    """What a runner does between the poison and its entry in the worst case -- a `Place.inp` copy and a `Place.out` fill,
    torch's elementwise kernels -- must not disturb LDS."""
    P.poison(P.PATTERNS[1] if pat == P.PATTERNS[0] else P.PATTERNS[0])
    P.poison(pat)
    pl = Place(dev, False)
    pl.inp(torch.randn(3, 8, 20, 36))
    pl.out((3, 8, 20, 36))
    share = P.probe(pat)
    print("share of 0x%08X after Place traffic at ROUNDS=%d: %.4f" % (pat, P.ROUNDS, share))
    assert share >= P.MIN_SHARE, "after a Place copy and fill %.1f%% of the probed LDS words still hold the pattern" % (
        100 * share)


def _leaky_run(aligned):
    L = P.wrap(P.hooks())                                 # the poisoning proxy while a pattern is set, as `_placement._L()`
    out = torch.full((P.LEAKY_WORDS,), 7.0, dtype=torch.float32, device="cuda")
    assert L.decnet_test_lds_leaky(0.0, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return {"y": out.cpu()}


def test_the_planted_bug_is_caught(dev):
    """decnet_test_lds_leaky writes 1 + 0 * (LDS it never wrote): NaN under the first pattern, 1.0 under the second, and
    the sweep of `_placement._both` raises on it."""
    nan, one = P.PATTERNS
    with P.pattern(nan):
        assert bool(torch.isnan(_leaky_run(True)["y"]).all())
    with P.pattern(one):
        assert bool((_leaky_run(True)["y"] == 1.0).all())
    P.poison(0)
    base = _leaky_run(True)
    assert bool((base["y"] == 1.0).all())
    with pytest.raises(AssertionError, match="LDS pattern 0x7FC07FC0, aligned placement"):
        P.sweep(_leaky_run, base)


def test_model_forward_does_not_depend_on_what_lds_held(dev):
    """The small end-to-end configuration of tests/test_model_gpu.py, eager under no_grad, with a forward pre-hook that
    poisons LDS on every module (the units launch from their own forward and never call their leaves, so leaves alone
    would miss them): the final disparity and the three SpaMat results are bit-identical without hooks and under either
    pattern.  This reaches the launches that go through decnet_amd.ops and model.Unit."""
    from netparams import fill_state_dict
    from make_golden import E2E_KW, e2e_inputs
    from decnet_amd.model import get_model, load_reference_checkpoint
    from spy_util import spamat_spy
    model = get_model(**E2E_KW)
    sd = fill_state_dict(model.state_dict())
    load_reference_checkpoint(model, {"module." + k: v for k, v in sd.items()})
    model = model.to(dev).eval()
    left, right = (t.to(dev) for t in e2e_inputs())

    def forward():
        rec = {}

        def spy(L, R, lm, rm, D, o):
            i = len(rec) // 4
            for j, t in enumerate(o):
                rec["spamat%d_%d" % (i, j)] = t.cpu()
        with spamat_spy(spy), torch.no_grad():
            rec["pred"] = model(left, right)[-1].cpu()
        return rec

    forward()                                              # weight caches and workspaces filled
    base = forward()
    assert len(base) == 13 and not bool(torch.isnan(base["pred"]).any())
    P.assert_same(base, forward(), "no poison (a second plain run)")
    for pat in P.PATTERNS:
        handles = [m.register_forward_pre_hook(lambda mod, args, pat=pat: P.poison(pat)) for m in model.modules()]
        try:
            got = forward()
        finally:
            for h in handles:
                h.remove()
        P.assert_same(base, got, "%s before every module" % P.name(pat))
