#!/usr/bin/env python
"""Record tests/golden/conv2d_mfma_bits.json: SHA-256 digests of what the matrix-core Conv2dUnit entries
(decnet_conv2d_mfma_pack_weight + decnet_conv2d_mfma_cat_bn_act, decnet_deconv2d_mfma_pack_weight +
decnet_deconv2d_mfma_k3s3_bn_act; csrc/conv2d_mfma.hip, conv2d_mfma_acc2.hip) compute, bit for bit, on an MI355X.

    python tests/golden/make_conv2d_mfma_bits.py OUT.json [LABEL]

The entries are driven through the C ABI alone (decnet_amd._lib, ctypes, tests/_placement.Place), so this file runs
unchanged in a checkout of an older commit: copy it there, build that commit's library, run it there and commit the JSON
here.  LABEL (the commit the library was built from) is stored beside the device's name and architecture.  The pin is only
worth something when the library is NOT the one under test; tests/test_conv2d_mfma_bits_gpu.py reruns the cases on the tree
under test and compares.

Cases (`cases()`): the MFMA table and the shapes of test_mfma_deconv_edges of tests/test_trunk_edges_gpu.py, read from that
module and fed as its _run_mfma / _run_mfma_deconv feed them, so the lists cannot drift apart.  Per case three digests: the
raw bytes of the inputs; the whole packed-weight buffer, the zeroed prefetch padding included (pre-filled with 0xA5: a
byte the pack leaves unwritten shows); y.
Legs (`LEGS`): at these sizes the entries choose TM = 2 and the producer / consumer kernel, so the other instantiations are
reached through the switches the files read -- once per process, hence `main` records every leg in a child process of its
own (`--leg`: the cases under the environment as it is, as JSON on stdout)."""
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_trunk_edges_gpu as T                                  # noqa: E402
from _placement import Place, _bn, _ints, _ptrs, _st, _vp        # noqa: E402

SWITCHES = ("DECNET_CONV2D_ACC", "DECNET_CONV2D_MFMA_PC", "DECNET_CONV2D_MFMA_TM")
_ONE = {"unset": {}, "pc0": {"DECNET_CONV2D_MFMA_PC": "0"}}
_ONE.update({"tm%d" % tm: {"DECNET_CONV2D_MFMA_TM": str(tm)} for tm in (4, 5, 6, 8)})
LEGS = dict(_ONE)
LEGS.update({"acc2_" + name: dict(env, DECNET_CONV2D_ACC="2") for name, env in _ONE.items()})
DECONV_B = 2                                                      # test_mfma_deconv_edges runs its shapes at B = 2


def cases():
    """-> [("conv", a row of T.MFMA) | ("deconv", (H, W, Cin, Cout))]"""
    shapes = [m for m in T.test_mfma_deconv_edges.pytestmark if m.name == "parametrize"][0].args[1]
    return [("conv", c) for c in T.MFMA] + [("deconv", tuple(s)) for s in shapes]


def case_id(case):
    return "%s-%s" % (case[0], repr(case[1]).replace(" ", ""))


def leg_env(leg, environ=os.environ):
    """The environment of a child process that runs `leg`: the three switches cleared, then the leg's set."""
    env = {k: v for k, v in environ.items() if k not in SWITCHES}
    env.update(LEGS[leg])
    return env


def leg_of(environ=os.environ):
    """The leg whose switches are exactly those set in `environ`, or None: an environment no leg was recorded under
    (DECNET_CONV2D_MFMA_TM=2, say) runs other instantiations, and there are no bits to hold it to."""
    have = {k: environ[k] for k in SWITCHES if k in environ}
    match = [leg for leg, env in LEGS.items() if env == have]
    return match[0] if match else None


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def case_data(case):
    """-> (the parts of x, w, scale, shift) on the host, with the seeds of the edge tests."""
    kind, c = case
    if kind == "conv":
        segs, cout, k, dil, (B, H, W), _ = c
        cin = sum(segs)
        g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + W + dil)
        xs = [torch.randn(B, s, H, W, generator=g) for s in segs]
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    else:
        H, W, cin, cout = c
        g = torch.Generator().manual_seed(H * 100 + W * 10 + cout)
        xs = [torch.randn(DECONV_B, cin, H, W, generator=g)]
        w = torch.randn(cin, cout, 3, 3, generator=g) / cin ** 0.5
    return (xs, w) + _bn(cout, g)


def run_case(case, aligned=True, data=None):
    """Pack and run one case -> {"inputs": digest, "packed": digest, "y": digest}."""
    from decnet_amd import _lib
    L, dev, st = _lib.lib(), torch.device("cuda:0"), _st()
    kind, c = case
    xs, w, scale, shift = data or case_data(case)
    P = Place(dev, aligned)
    xd = [P.inp(x) for x in xs]
    wd, sd, hd = P.inp(w), P.inp(scale), P.inp(shift)
    if kind == "conv":
        segs, cout, k, dil, (B, H, W), relu = c
        cin = sum(segs)
        nbytes = L.decnet_conv2d_mfma_packed_bytes(cin, cout, k)
    else:
        H, W, cin, cout = c
        nbytes = L.decnet_deconv2d_mfma_packed_bytes(cin, cout)
    assert nbytes > 0, case
    wp = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)           # library format: 16-byte aligned
    if kind == "conv":
        assert L.decnet_conv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, k, st) == 0
        y = P.out((B, cout, H, W))
        xa, ca = _ptrs(xd), _ints(segs)
        rc = L.decnet_conv2d_mfma_cat_bn_act(_vp(xa), _vp(ca), len(segs), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                             y.data_ptr(), B, cout, H, W, k, dil, relu, st)
    else:
        assert L.decnet_deconv2d_mfma_pack_weight(wd.data_ptr(), wp.data_ptr(), cin, cout, st) == 0
        y = P.out((DECONV_B, cout, 3 * H, 3 * W))
        rc = L.decnet_deconv2d_mfma_k3s3_bn_act(xd[0].data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(),
                                                DECONV_B, cin, cout, H, W, 1, st)
    assert rc == 0, (case, rc)
    P.check(case_id(case))
    return {"inputs": digest(*xs, w, scale, shift), "packed": digest(wp), "y": digest(y)}


def run_leg():
    return {case_id(c): run_case(c) for c in cases()}


def main(out, label=""):
    assert torch.cuda.is_available(), "the recording needs the MI355X"
    doc = {"library": label, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__, "legs": {}}
    for leg in LEGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg"], env=leg_env(leg), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, (leg, r.stdout[-2000:], r.stderr[-2000:])
        doc["legs"][leg] = json.loads(r.stdout.strip().split("\n")[-1])
        assert len(doc["legs"][leg]) == len(cases()), leg
        print("recorded", leg, flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(LEGS), "legs of", len(cases()), "cases")


if __name__ == "__main__":
    if sys.argv[1] == "--leg":
        print(json.dumps(run_leg(), sort_keys=True))
    else:
        main(*sys.argv[1:3])
