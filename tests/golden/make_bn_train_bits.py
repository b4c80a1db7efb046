#!/usr/bin/env python
"""Record tests/golden/bn_train_bits.json: SHA-256 digests of what the six training-mode BatchNorm entries
(decnet_bn_train_* / decnet_bn_train_cl_*) compute, bit for bit, on an MI355X.

    python tests/golden/make_bn_train_bits.py OUT.json [LABEL]

The entries are driven through the C ABI alone (decnet_amd._lib, ctypes, tests/_placement.Place at the aligned placement),
so this file runs unchanged in a checkout of an older commit: copy it there, build that commit's library, run it there and
commit the JSON here.  LABEL (the commit the library was built from) is stored beside the device's name and architecture.
The pin is only worth something when the library is NOT the one under test; tests/test_bn_train_bits_gpu.py reruns
`cases()` on the tree under test and compares.

Cases (`cases()`): the NCHW shapes of test_bn_train_gpu.SHAPES but the last, (5, 1, 1, 6 SEG + 3) in its place, and the
(rows, C) of _stage0_bn_train_ref.entry_cases(), each with first_kind 0, 1, 2 and relu off and on, on the data of
`entry_data`; and once per layout -- (3, 5, 1, SEG + 1) and (ROWS + 1, 5), first_kind 0, relu on -- with gz = NULL and with
running_mean = running_var = NULL.  Per case: one digest over the raw bytes of the inputs (z, gy, gamma, beta,
running_mean, running_var as they go in), one per result (y, stats, running_mean, running_var, gz, dgamma, dbeta).
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _bn_train_ref as BR              # noqa: E402
import _stage0_bn_train_ref as SB       # noqa: E402
from _placement import Place            # noqa: E402

from decnet_amd.ops2d import BN_SEGMENT as SEG      # noqa: E402

ROWS = SB.ROWS
EPS, MOM = 1e-5, 0.1
# test_bn_train_gpu.SHAPES but the last (tests/test_bn_train_bits_gpu.py holds the lists together), and 6 segments + 3
PLANES = [(1, 1, 1, 2), (2, 3, 5, 7), (1, 8, 16, 18), (1, 2, 1, SEG), (3, 5, 1, SEG + 1), (5, 1, 1, 6 * SEG + 3)]
INPUTS = ("z", "gy", "gamma", "beta", "running_mean", "running_var")
RESULTS = ("y", "stats", "running_mean", "running_var", "gz", "dgamma", "dbeta")


def cases():
    """-> [(layout, dims, first_kind, relu, variant)]; variant "full", "no_gz" (gz NULL) or "no_running" (both NULL)."""
    out = [(layout, dims, first_kind, relu, "full")
           for layout, all_dims in (("planes", PLANES), ("columns", SB.entry_cases()))
           for dims in all_dims for first_kind in (0, 1, 2) for relu in (False, True)]
    for layout, dims in (("planes", PLANES[4]), ("columns", (ROWS + 1, 5))):
        out += [(layout, dims, 0, True, "no_gz"), (layout, dims, 0, True, "no_running")]
    return out


def case_id(case):
    layout, dims, first_kind, relu, variant = case
    return "%s-%s-%s-%s-%s" % (layout, "x".join(map(str, dims)), BR.KINDS[first_kind], "relu" if relu else "id", variant)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(case, aligned=True):
    """Forward, then backward on the forward's stats -> {"inputs": digest, "results": {name: digest}}."""
    from decnet_amd import _lib
    layout, dims, first_kind, relu, variant = case
    L, dev = _lib.lib(), torch.device("cuda:0")
    if layout == "planes":
        d = BR.entry_data(dims, first_kind, relu)
        C, entry = dims[1], "decnet_bn_train"
    else:
        d = SB.entry_data(*dims, first_kind, relu)
        d = dict(d, z=SB.to_cl(d["z"]), gy=SB.to_cl(d["gy"]))
        C, entry = dims[1], "decnet_bn_train_cl"
    P = Place(dev, aligned)
    z, gy, gamma, beta = (P.inp(d[k]) for k in INPUTS[:4])
    running = variant != "no_running"
    rm, rv = (P.inplace(d["running_mean"]), P.inplace(d["running_var"])) if running else (None, None)
    stats, y = P.out((2 * C,), torch.float64), P.out(z.shape)
    gz = P.out(z.shape) if variant != "no_gz" else None
    dg, db = P.out((C,)), P.out((C,))
    nws = getattr(L, entry + "_workspace_floats")(*dims)
    assert nws > 0, case

    def ws():                                                   # NaN-filled, a fresh one per call; 16-byte aligned
        return torch.full((nws,), float("nan"), dtype=torch.float32, device=dev)

    def ptr(t):
        return None if t is None else t.data_ptr()

    st = torch.cuda.current_stream().cuda_stream
    w = ws()
    rc = getattr(L, entry + "_forward")(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, MOM, ptr(rm), ptr(rv),
                                        stats.data_ptr(), y.data_ptr(), int(relu), w.data_ptr(), nws, *dims, st)
    assert rc == 0, (case, rc)
    w = ws()
    rc = getattr(L, entry + "_backward")(z.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                         ptr(gz), dg.data_ptr(), db.data_ptr(), int(relu), w.data_ptr(), nws, *dims, st)
    assert rc == 0, (case, rc)
    P.check(case_id(case))
    got = dict(y=y, stats=stats, running_mean=rm, running_var=rv, gz=gz, dgamma=dg, dbeta=db)
    return {"inputs": digest(*[d[k] for k in INPUTS]),
            "results": {k: digest(got[k]) for k in RESULTS if got[k] is not None}}


def main(out, label=""):
    assert torch.cuda.is_available(), "the recording needs the MI355X"
    doc = {"library": label, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
           "cases": {case_id(c): run(c) for c in cases()}}
    assert len(doc["cases"]) == len(cases())
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main(*sys.argv[1:3])
