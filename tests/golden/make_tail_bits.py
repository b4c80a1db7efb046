#!/usr/bin/env python
"""Record tests/golden/tail_bits.json: SHA-256 digests of what the elementwise passes of the training forward compute, bit
for bit, on an MI355X -- the seven flat entries (decnet_sigmoid_blend, _backward, _soft, _soft_backward, decnet_sqdiff,
_backward, decnet_detail_tail_backward) and the two row entries (decnet_detail_tail, decnet_detail_mask).

    python tests/golden/make_tail_bits.py OUT.json [LABEL]

The entries are driven through the C ABI alone (decnet_amd._lib, ctypes, tests/_placement.Place at the aligned placement),
so this file runs unchanged in a checkout of an older commit: copy it there, build that commit's library, run it there and
commit the JSON here.  LABEL (the commit the library was built from) is stored beside the device's name and architecture.
The pin is only worth something when the library is NOT the one under test; tests/test_tail_bits_gpu.py reruns `cases()`
on the tree under test, at both placements, and compares.

Cases (`cases()`):
  * ("flat", n) for n in FLAT_N -- test_detail_grad_gpu.FLAT_N and 1024: with 4, 1023, 1024 and 1025 the last full quad,
    the last thread of a workgroup and the first thread of the next.  Data: o = +-200 planted among uniform [-30, 30).
    Every entry, and every NULL combination one accepts: g_o alone for both blend backwards; gout only, gsoft only and
    both for the soft one; g_a and g_b alone for decnet_sqdiff_backward;
  * ("tail", B, H, W) for the shapes of test_detail_grad_gpu.TAIL: decnet_detail_tail with every subset of (prob, mask, bits);
  * ("mask", B, H, W), B in {1, 2}, H in {1, 3}, W in {1, 63, 64, 65, 1023, 1026}: decnet_detail_mask with and without
    logits and bits, on data that puts both mask values into every 64-pixel word of more than one pixel (checked).
Per case: one digest over the raw bytes of the inputs, one per result.
"""
import ctypes
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _placement import Place            # noqa: E402

FLAT_N = [1, 3, 4, 5, 1023, 1024, 1025]
TAIL = [(1, 1, 1), (2, 3, 63), (1, 2, 64), (1, 2, 65), (2, 3, 129), (1, 1, 1023), (1, 2, 1026)]
MASK = [(B, H, W) for B in (1, 2) for H in (1, 3) for W in (1, 63, 64, 65, 1023, 1026)]
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(("prob", "mask", "bits"), k)]
THOLD = 0.37


def cases():
    return [("flat", n) for n in FLAT_N] + [("tail",) + s for s in TAIL] + [("mask",) + s for s in MASK]


def case_id(case):
    return "%s-%s" % (case[0], "x".join(map(str, case[1:])))


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def flat_data(n):
    """-> o (saturated at every fifth and seventh element, ordinary elsewhere), a, b, two gradients."""
    g = torch.Generator().manual_seed(7000 + n)
    o = torch.rand(n, generator=g) * 60 - 30
    o[::5] = 200.0
    o[2::7] = -200.0
    return [o, torch.rand(n, generator=g) * 4, torch.rand(n, generator=g) * 4, torch.randn(n, generator=g),
            torch.randn(n, generator=g)]


def tail_data(B, H, W):
    g = torch.Generator().manual_seed(B * 100000 + H * 10000 + W + 7)
    z = torch.rand(B, H, W, generator=g) * 60 - 30
    z.view(-1)[::11] = 200.0
    z.view(-1)[3::13] = -200.0
    return [z]


def mask_data(B, H, W):
    """-> cur3, pre3 [B,3,H,W] and the 92 folded values of the layer (w3x3, scale3, shift3, w1x1, scale1, shift1): the 3x3
    unit is the identity plus noise and the 1x1 unit the channels' mean less 1, so that the logit of a pixel follows its own
    squared difference -- |cur - pre| in [1.5, 2.5) (mask 1 at threshold 0.5) or below 0.5 (mask 0), at random, with pixels
    64 w and 64 w + 1 of every row planted as 1 and 0."""
    g = torch.Generator().manual_seed(B * 100000 + H * 10000 + W + 11)
    big = torch.rand(B, 1, H, W, generator=g) < 0.5
    big[..., 0::64] = True
    big[..., 1::64] = False
    mag = torch.where(big, torch.rand(B, 3, H, W, generator=g) + 1.5, torch.rand(B, 3, H, W, generator=g) * 0.5)
    sign = torch.where(torch.rand(B, 3, H, W, generator=g) < 0.5, -1.0, 1.0)
    pre = torch.randn(B, 3, H, W, generator=g)
    w3 = torch.randn(3, 3, 3, 3, generator=g) * 0.004
    for c in range(3):
        w3[c, c, 1, 1] += 1.0
    flat = torch.cat([w3.reshape(-1), torch.rand(3, generator=g) * 0.1 + 0.95, torch.randn(3, generator=g) * 0.01,
                      torch.rand(3, generator=g) * 0.02 + 1.0 / 3, torch.tensor([1.0, -1.0])])
    return [pre + sign * mag, pre, flat]


def _p(t):
    return None if t is None else t.data_ptr()


def _run_flat(L, P, st, n, d):
    o, a, b, g1, g2 = (P.inp(t) for t in d)
    names = ("blend", "blend_go", "blend_ga", "blend_gb", "blend_go_alone", "soft_out", "soft_soft", "soft_go", "soft_ga",
             "soft_gb", "soft_go_alone", "soft_gout_only_go", "soft_gout_only_ga", "soft_gout_only_gb", "soft_gsoft_only_go",
             "soft_gsoft_only_ga", "soft_gsoft_only_gb", "sqdiff", "sqdiff_ga", "sqdiff_gb", "sqdiff_ga_alone",
             "sqdiff_gb_alone", "tail_gz")
    r = {k: P.out((n,)) for k in names}
    q = {k: t.data_ptr() for k, t in r.items()}
    bwd, sbwd, qbwd = L.decnet_sigmoid_blend_backward, L.decnet_sigmoid_blend_soft_backward, L.decnet_sqdiff_backward
    rcs = [L.decnet_sigmoid_blend(_p(o), _p(a), _p(b), q["blend"], n, st),
           bwd(_p(o), _p(a), _p(b), _p(g1), q["blend_go"], q["blend_ga"], q["blend_gb"], n, st),
           bwd(_p(o), _p(a), _p(b), _p(g1), q["blend_go_alone"], None, None, n, st),
           L.decnet_sigmoid_blend_soft(_p(o), _p(a), _p(b), q["soft_out"], q["soft_soft"], n, st),
           sbwd(_p(o), _p(a), _p(b), _p(g1), _p(g2), q["soft_go"], q["soft_ga"], q["soft_gb"], n, st),
           sbwd(_p(o), _p(a), _p(b), _p(g1), _p(g2), q["soft_go_alone"], None, None, n, st),
           sbwd(_p(o), _p(a), _p(b), _p(g1), None, q["soft_gout_only_go"], q["soft_gout_only_ga"], q["soft_gout_only_gb"], n, st),
           sbwd(_p(o), _p(a), _p(b), None, _p(g2), q["soft_gsoft_only_go"], q["soft_gsoft_only_ga"], q["soft_gsoft_only_gb"], n,
                st),
           L.decnet_sqdiff(_p(a), _p(b), q["sqdiff"], n, st),
           qbwd(_p(a), _p(b), _p(g1), q["sqdiff_ga"], q["sqdiff_gb"], n, st),
           qbwd(_p(a), _p(b), _p(g1), q["sqdiff_ga_alone"], None, n, st),
           qbwd(_p(a), _p(b), _p(g1), None, q["sqdiff_gb_alone"], n, st),
           L.decnet_detail_tail_backward(_p(o), _p(g1), q["tail_gz"], n, st)]
    assert rcs == [0] * len(rcs), (n, rcs)
    return r


def _run_tail(L, P, st, B, H, W, d):
    z = P.inp(d[0])
    r = {}
    for want in SUBSETS:
        t = {"prob": P.out((B, H, W)) if "prob" in want else None, "mask": P.out((B, H, W)) if "mask" in want else None,
             "bits": P.out((B, H, (W + 63) // 64), torch.int64, -1) if "bits" in want else None}
        rc = L.decnet_detail_tail(_p(z), THOLD, _p(t["prob"]), _p(t["mask"]), _p(t["bits"]), B, H, W, st)
        assert rc == 0, (B, H, W, want, rc)
        r.update({"%s of %s" % (k, "+".join(want)): t[k] for k in want})
    return r


def _run_mask(L, P, st, B, H, W, d):
    cur, pre = P.inp(d[0]), P.inp(d[1])
    flat = d[2].tolist()
    arr = lambda v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    params = (arr(flat[0:81]), arr(flat[81:84]), arr(flat[84:87]), arr(flat[87:90]), flat[90], flat[91])
    r = {}
    for want_logits, want_bits in itertools.product((False, True), repeat=2):
        tag = "%s%s" % ("+logits" if want_logits else "", "+bits" if want_bits else "")
        mask = P.out((B, H, W))
        logits = P.out((B, H, W)) if want_logits else None
        bits = P.out((B, H, (W + 63) // 64), torch.int64, -1) if want_bits else None
        rc = L.decnet_detail_mask(_p(cur), _p(pre), *params, 0.5, _p(mask), _p(logits), _p(bits), B, H, W, st)
        assert rc == 0, (B, H, W, tag, rc)
        r["mask of mask" + tag] = mask
        if want_logits:
            r["logits of mask" + tag] = logits
        if want_bits:
            r["bits of mask" + tag] = bits
    return r


def run(case, aligned=True):
    """-> {"inputs": digest, "results": {name: digest}}"""
    from decnet_amd import _lib
    L, dev, st = _lib.lib(), torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
    kind, dims = case[0], case[1:]
    d = {"flat": flat_data, "tail": tail_data, "mask": mask_data}[kind](*dims)
    P = Place(dev, aligned)
    r = {"flat": _run_flat, "tail": _run_tail, "mask": _run_mask}[kind](L, P, st, *dims, d)
    P.check(case_id(case))
    if kind == "mask":                                          # both values in every word of more than one pixel
        m = r["mask of mask"].cpu()
        for w0 in range(0, dims[2] - 1, 64):
            word = m[..., w0:w0 + 64]
            assert bool((word.amin(-1) == 0).all()) and bool((word.amax(-1) == 1).all()), (case, w0)
    return {"inputs": digest(*d), "results": {k: digest(t) for k, t in r.items()}}


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
