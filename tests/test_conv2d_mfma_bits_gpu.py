"""The matrix-core Conv2dUnit entries (csrc/conv2d_mfma.hip, csrc/conv2d_mfma_acc2.hip and what they share in
csrc/conv2d_mfma_common.h: split, epilogue, refusals, launch path) bit for bit against tests/golden/conv2d_mfma_bits.json:
SHA-256 digests of the packed weights and of y of every case of tests/golden/make_conv2d_mfma_bits.py, recorded on an MI355X
from the library of the commit the JSON names -- an older one than the tree under test, in a checkout of its own --, so
another order of the MFMAs, another rounding in the split or another byte in the packed format shows here, where the
4e-6 bound of the edge tests would let it through.  Both placements are held to the one recording.

The cases are the edge tests' own tables (`test_the_cases_are_the_tables`).  The tile height and the kernel kind follow
the workgroup count, at these sizes always TM = 2 and the producer / consumer kernel, so `test_leg` reruns the cases in
child processes under the switches the files read once per process (LEGS of the recorder: DECNET_CONV2D_MFMA_PC=0,
DECNET_CONV2D_MFMA_TM = 4, 5, 6, 8, and each again with DECNET_CONV2D_ACC=2); the recording is keyed by leg, and the
process itself compares against the leg its own environment names.  -m gpu."""
import json
import os
import subprocess
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_conv2d_mfma_bits as MB  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {MB.case_id(c): c for c in MB.cases()}


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(os.path.join(GOLDEN, "conv2d_mfma_bits.json")) as f:
        doc = json.load(f)
    assert doc["library"], "the recording does not say which commit's library made it"
    return doc


def test_the_cases_are_the_tables(recorded):
    import test_trunk_edges_gpu as T
    assert len(T.MFMA) == 16 and len(CASES) == len(T.MFMA) + 5
    assert sorted(recorded["legs"]) == sorted(MB.LEGS) and len(MB.LEGS) == 12
    for leg, got in recorded["legs"].items():
        assert sorted(got) == sorted(CASES), "the edge tests' tables are no longer the recorded ones (leg %s)" % leg


@pytest.mark.parametrize("cid", sorted(CASES))
def test_every_case_has_the_recorded_bits(recorded, cid):
    leg = MB.leg_of()
    assert leg, ("%s in this process's environment are the switches of no recorded leg (%s): run this file with them "
                 "unset, test_leg sets them for its child processes" % (
                     {k: os.environ[k] for k in MB.SWITCHES if k in os.environ}, ", ".join(MB.LEGS)))
    want, data = recorded["legs"][leg][cid], MB.case_data(CASES[cid])
    for aligned in (True, False):
        got = MB.run_case(CASES[cid], aligned, data)
        what = "%s %s, leg %s" % (cid, "aligned" if aligned else "unaligned", leg)
        assert got["inputs"] == want["inputs"], "the inputs differ from the recording: torch's generator? %s" % what
        differ = [k for k in ("packed", "y") if got[k] != want[k]]
        assert not differ, "%s: %s differ from the recorded bits" % (what, differ)


@pytest.mark.parametrize("leg", [leg for leg in MB.LEGS if leg != "unset"])
def test_leg(leg):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "recorded_bits"], env=MB.leg_env(leg), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
