"""The dispatch table of decnet_amd/model.py without a GPU: ``Unit._route`` and ``ASPP._fusable`` are functions of the
layer, the input size, the number of concatenated parts and the two switches alone, so every row of the tables that
tests/test_model_routes_gpu.py runs on real tensors (tests/_model_cases.py) is asserted here too, under each of the four
switch settings -- every dispatch threshold is under test on any machine."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _model_cases as MC  # noqa: E402

SWITCHES = {"default": {}, "torch": {"DECNET_CONV2D": "torch"}, "mfma0": {"DECNET_CONV2D_MFMA": "0"},
            "acc2": {"DECNET_CONV2D_ACC": "2"}}


@pytest.fixture(params=list(SWITCHES))
def sw(request, monkeypatch):
    for k in ("DECNET_CONV2D", "DECNET_CONV2D_MFMA", "DECNET_CONV2D_ACC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SWITCHES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.mark.parametrize("name", list(MC.UNIT_CASES))
def test_unit_route_table(sw, name):
    c = MC.UNIT_CASES[name]
    u = MC.make_unit(c["cin"], c["cout"], c["k"], **c["kw"])
    want = {"default": c["route"], "acc2": c["route"], "mfma0": c["mfma0"], "torch": None}[sw]
    assert u._route(c["B"], c["H"], c["W"], len(c["parts"]) if c["parts"] else None) == want


def test_unit_route_of_a_tuple_is_a_cat_route(sw):
    """A tuple, even of one part, has the routes of the `cat` entries only; the same layer on a tensor keeps its own."""
    for name, kinds in (("dc_cout8", ("deconv",)), ("s3_hw256", ("conv_s3",)), ("conv_hw256", ("conv",))):
        c = MC.UNIT_CASES[name]
        u = MC.make_unit(c["cin"], c["cout"], c["k"], **c["kw"])
        one = u._route(1, c["H"], c["W"], None)
        assert one == (None if sw == "torch" else c["route"])
        assert u._route(1, c["H"], c["W"], 1) == (one if one == "conv" else None)


@pytest.mark.parametrize("name", list(MC.ASPP_CASES))
def test_aspp_route_table(sw, name):
    from decnet_amd.model import ASPP
    cin, cout, rates, (H, W), relu1, fused = MC.ASPP_CASES[name]
    m = MC.seeded(lambda: ASPP(cin, cout, rates), cin + cout)
    list(m.stages.children())[1].relu = relu1
    assert m._fusable(H, W) == (fused and sw != "torch")
