"""The elementwise passes of the training forward (csrc/detail_grad.hip, csrc/maskgen.hip over csrc/pointwise.h) bit for
bit against tests/golden/tail_bits.json: SHA-256 digests of every result of every case of tests/golden/make_tail_bits.py,
recorded on an MI355X from the library of the commit the JSON names -- an older one than the tree under test, in which
every kernel still carried its own copy of the access, the sigmoid, the blend and the bit packing.  A changed statement
order, a lost contraction pin or a mask pixel that moves at the threshold shows here.  The unaligned placement is held to
the same recorded digests.  -m gpu."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_tail_bits as MT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(os.path.join(GOLDEN, "tail_bits.json")) as f:
        doc = json.load(f)
    assert doc["library"], "the recording does not say which commit's library made it"
    return doc["cases"]


@pytest.fixture(scope="module")
def runs():
    """Every case at the aligned and at the unaligned placement, once."""
    return {aligned: {MT.case_id(c): MT.run(c, aligned) for c in MT.cases()} for aligned in (True, False)}


def test_the_inputs_are_the_recorded_ones(recorded, runs):
    import test_detail_grad_gpu as TD
    assert MT.FLAT_N == sorted(set(TD.FLAT_N) | {1024}) and MT.TAIL == TD.TAIL and MT.SUBSETS == TD.SUBSETS, \
        "the recorder's shapes are no longer the entry tests'"
    assert {4, 1023, 1024, 1025} <= set(MT.FLAT_N)
    assert sorted(recorded) == sorted(runs[True]), "the case list differs from the recording"
    differ = [k for k, v in runs[True].items() if v["inputs"] != recorded[k]["inputs"]]
    assert not differ, "the inputs differ from the recording: torch's generator? %s" % differ


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_every_result_has_the_recorded_bits(recorded, runs, aligned):
    assert sorted(recorded) == sorted(runs[aligned])
    differ = []
    for k, got in runs[aligned].items():
        assert got["inputs"] == recorded[k]["inputs"], "the inputs differ from the recording: torch's generator? %s" % k
        assert got["results"].keys() == recorded[k]["results"].keys(), k
        differ += ["%s %s" % (k, name) for name, h in got["results"].items() if h != recorded[k]["results"][name]]
    assert not differ, "%d results differ from the recorded bits: %s" % (len(differ), differ[:20])
