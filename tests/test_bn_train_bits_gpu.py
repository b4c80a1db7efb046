"""The six training-mode BatchNorm entries (csrc/batchnorm.hip, both layouts) bit for bit against
tests/golden/bn_train_bits.json: SHA-256 digests of every result of every case of tests/golden/make_bn_train_bits.py,
recorded on an MI355X from the library of the commit the JSON names -- an older one than the tree under test, so a changed
order of addition, a lost contraction pin or another per-element expression shows here, where the float64 bounds of
tests/test_bn_train_gpu.py and tests/test_stage0_bn_train_gpu.py would let it through.  The unaligned placement is held
to the same recorded digests.  -m gpu."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_bn_train_bits as MB  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(os.path.join(GOLDEN, "bn_train_bits.json")) as f:
        doc = json.load(f)
    assert doc["library"], "the recording does not say which commit's library made it"
    return doc["cases"]


@pytest.fixture(scope="module")
def runs():
    """Every case at the aligned and at the unaligned placement, once."""
    return {aligned: {MB.case_id(c): MB.run(c, aligned) for c in MB.cases()} for aligned in (True, False)}


def test_the_inputs_are_the_recorded_ones(recorded, runs):
    import test_bn_train_gpu as T2
    assert MB.PLANES[:-1] == T2.SHAPES[:-1] and MB.SEG == T2.SEG, "the recorder's shapes are no longer the entry tests'"
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
