"""The five weight-gradient entries (csrc/conv2d_grad.hip, csrc/conv2d_mfma_grad.hip, csrc/conv3d_grad.hip; the shared
mask, reduction and host path of csrc/wgrad_common.h) and the autograd Functions on top of them (decnet_amd/conv2d_grad.py,
decnet_amd/stage0_grad.py) bit for bit against tests/golden/wgrad_bits.json: SHA-256 digests of every result of every
case of tests/golden/make_wgrad_bits.py, recorded on an MI355X from the library of the commit the JSON names -- an older one
than the tree under test, in a checkout of its own --, so a changed order of addition in the reduction, another expression
in the mask or another torch expression in `_param_grads` shows here, where the 4096 u sum|terms| bounds of the entry tests
would let it through.  The unaligned placement is held to the same recorded digests.

The recorder reads its entry cases from the entry tests' own tables; `test_the_cases_are_the_tables` holds the recording
against them.  At the recording every Function case of the four UNITS tables reproduced its own digests across two runs
in the older commit ("unstable": [] in the JSON), so none is left out of the pin.  -m gpu."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_wgrad_bits as MW  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = {MW.case_id(c): c for c in MW.entry_cases()}
FUNCTION = {MW.case_id(c): c for c in MW.function_cases()}


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(os.path.join(GOLDEN, "wgrad_bits.json")) as f:
        doc = json.load(f)
    assert doc["library"], "the recording does not say which commit's library made it"
    return doc


def test_the_cases_are_the_tables(recorded):
    import _stage0_grad_ref as SG
    import test_conv2d_grad_gpu as T1
    import test_conv2d_mfma_grad_gpu as T2
    import test_conv2d_s3_grad_gpu as T3
    import test_stage0_grad_gpu as T4
    assert len(ENTRY) == len(T1.CASES) + len(T2.CASES) + len(T3.CASES) + 1 + 2 * len(SG.WGRAD_CASES)
    assert MW.S3_FINE not in T3.CASES and 3 * MW.S3_FINE[4] * 3 * MW.S3_FINE[5] > 65536       # two chan_sum_partial slices
    assert sorted(recorded["entries"]) == sorted(ENTRY), "the entry tests' tables are no longer the recorded ones"
    assert len(FUNCTION) == sum(len(T.UNITS) for T in (T1, T2, T3, T4))
    assert recorded["unstable"] == [] and sorted(recorded["functions"]) == sorted(FUNCTION), \
        "the UNITS tables are no longer the recorded ones"


def _compare(got, want, what):
    assert got["inputs"] == want["inputs"], "the inputs differ from the recording: torch's generator? %s" % what
    assert got["results"].keys() == want["results"].keys(), what
    differ = [k for k, h in got["results"].items() if h != want["results"][k]]
    assert not differ, "%s: %s differ from the recorded bits" % (what, differ)


@pytest.mark.parametrize("cid", sorted(ENTRY))
def test_every_entry_has_the_recorded_bits(recorded, cid):
    data = MW.entry_data(ENTRY[cid])
    for aligned in (True, False):
        _compare(MW.run_entry(ENTRY[cid], aligned, data), recorded["entries"][cid],
                 "%s %s" % (cid, "aligned" if aligned else "unaligned"))


@pytest.mark.parametrize("cid", sorted(FUNCTION))
def test_every_function_has_the_recorded_bits(recorded, cid):
    _compare(MW.run_function(FUNCTION[cid]), recorded["functions"][cid], cid)
