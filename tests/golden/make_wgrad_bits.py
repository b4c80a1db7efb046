#!/usr/bin/env python
"""Record tests/golden/wgrad_bits.json: SHA-256 digests of what the five weight-gradient entries (decnet_conv2d_wgrad,
decnet_conv2d_mfma_wgrad, decnet_conv2d_k3s3_wgrad, decnet_deconv2d_k3s3_wgrad, decnet_conv3d_wgrad) and the autograd
Functions on top of them compute, bit for bit, on an MI355X.

    python tests/golden/make_wgrad_bits.py OUT.json [LABEL]

The entries are driven through the C ABI alone (decnet_amd._lib, ctypes, tests/_placement.Place, a NaN-filled workspace per
call), the Functions through the public modules, so this file runs unchanged in a checkout of an older commit: copy it
there, build that commit's library, run it there and commit the JSON here.  LABEL (the commit the library was built from)
is stored beside the device's name and architecture.  The pin is only worth something when the library is NOT the one
under test; tests/test_wgrad_bits_gpu.py reruns the cases on the tree under test and compares.

Entry cases (`entry_cases()`): the float (randn) data of the tables the entry tests hold -- CASES of test_conv2d_grad_gpu,
test_conv2d_mfma_grad_gpu and test_conv2d_s3_grad_gpu, _stage0_grad_ref.WGRAD_CASES with and without y -- read from
those modules, so the lists cannot drift apart; and S3_FINE, the one case no table has: the transposed stride-3 entry on a
258 x 258 fine plane, just over the 65536 pixels of one chan_sum_partial slice (two slices per plane).  Per case: one digest
over the raw bytes of the inputs, one each for G, gsum and (with y) gm.
Function cases (`function_cases()`): the UNITS tables of the same four test modules, built and fed as their
test_function_on_units does -- a change there shows in the input digest --, each 2-D unit required to tally its HIP
Function's family and not the library arm; per case one digest over the inputs (data and parameters) and one per gradient.  `main`
runs every Function case twice and lists under "unstable" those whose two runs differ; their digests are not stored.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _conv2d_s3_grad_ref as S3            # noqa: E402
import _model_cases as MC                   # noqa: E402
import _stage0_grad_ref as SG               # noqa: E402
import test_conv2d_grad_gpu as T1           # noqa: E402
import test_conv2d_mfma_grad_gpu as T2      # noqa: E402
import test_conv2d_s3_grad_gpu as T3        # noqa: E402
import test_stage0_grad_gpu as T4           # noqa: E402
from _placement import Place, _ints, _ptrs, _vp      # noqa: E402

S3_FINE = (True, 1, 2, 1, 86, 86, 1)        # (transposed, Cin, Cout, B, H, W, relu): gy, y, gm [1,2,258,258]
STRIDE1 = {"small": (T1, "decnet_conv2d_wgrad"), "mfma": (T2, "decnet_conv2d_mfma_wgrad")}


def entry_cases():
    """-> [(family, case)]; family "small", "mfma", "s3" (both stride-3 entries) or "conv3d" (case + (with_y,))."""
    out = [(fam, c) for fam, (T, _) in STRIDE1.items() for c in T.CASES]
    out += [("s3", c) for c in T3.CASES + [S3_FINE]]
    return out + [("conv3d", c + (with_y,)) for c in SG.WGRAD_CASES for with_y in (True, False)]


def function_cases():
    """-> [(family, name of the unit in that test module's UNITS)]."""
    return [(fam, name) for fam, T in (("small", T1), ("mfma", T2), ("s3", T3), ("conv3d", T4)) for name in sorted(T.UNITS)]


def case_id(case):
    fam, c = case
    return "%s-%s" % (fam, c if isinstance(c, str) else repr(c).replace(" ", ""))


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def entry_data(case):
    """-> (the parts of x, gy, y or None): float data, as the entry tests' _data(case, False) makes it."""
    fam, c = case
    if fam in STRIDE1:
        xs, gy, y = STRIDE1[fam][0]._data(c, False)[:3]
        return xs, gy, y
    x, gy, y = SG.wgrad_data(c[:6], False, c[6]) if fam == "conv3d" else T3._data(c, False)
    return [x], gy, y


def run_entry(case, aligned=True, data=None):
    """One call of the case's entry -> {"inputs": digest, "results": {"G", "gsum", "gm" with y: digest}}."""
    from decnet_amd import _lib
    fam, c = case
    L, dev = _lib.lib(), torch.device("cuda:0")
    xs, gy, y = data or entry_data(case)
    P = Place(dev, aligned)
    xd, gyd = [P.inp(x) for x in xs], P.inp(gy)
    yd = None if y is None else P.inp(y)
    gm = None if y is None else P.out(gy.shape)                # without ReLU: y NULL, gm NULL (gm == gy)
    st = torch.cuda.current_stream().cuda_stream
    if fam in STRIDE1:
        segs, co, k, dil, (B, H, W), _ = c
        entry, dims, gshape = STRIDE1[fam][1], (B, sum(segs), co, H, W, k), (co, sum(segs), k, k)
        xa, ca = _ptrs(xd), _ints(segs)
        lead, tail = (_vp(xa), _vp(ca), len(segs)), (B, co, H, W, k, dil)
    elif fam == "s3":
        tr, ci, co, B, H, W, _ = c
        entry = "decnet_deconv2d_k3s3_wgrad" if tr else "decnet_conv2d_k3s3_wgrad"
        dims, gshape = (B, ci, co, H, W), (ci, co, 3, 3) if tr else (co, ci, 3, 3)
        lead, tail = (xd[0].data_ptr(),), dims
    else:
        dims = c[:6]
        entry, co, gshape = "decnet_conv3d_wgrad", c[5], (c[5], c[4], 3, 3, 3)
        lead, tail = (xd[0].data_ptr(),), dims
    G, gsum = P.out(gshape), P.out((co,))
    nws = getattr(L, entry + "_workspace_floats")(*dims)
    assert nws > 0, case
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device=dev)     # 16-byte aligned at either placement
    rc = getattr(L, entry)(*lead, gyd.data_ptr(), None if y is None else yd.data_ptr(), None if y is None else gm.data_ptr(),
                           G.data_ptr(), gsum.data_ptr(), ws.data_ptr(), nws, *tail, st)
    assert rc == 0, (case, rc)
    P.check(case_id(case))
    got = {"G": G, "gsum": gsum, "gm": gm}
    return {"inputs": digest(*xs, gy, y), "results": {k: digest(t) for k, t in got.items() if t is not None}}


def _unit_case(fam, name):
    """-> (unit on the CPU, the parts of its input with requires_grad set, gy), as that module's test_function_on_units."""
    if fam == "s3":
        tr, ci, co, (H, W), relu, bn, route = T3.UNITS[name]
        g = torch.Generator().manual_seed(ci * 7 + co)
        xs = [torch.randn(1, ci, H, W, generator=g).requires_grad_()]
        return T3._make(name), xs, torch.randn((1, co) + S3.out_hw(tr, H, W), generator=g)
    segs, cout, k, dil, relu, bn, wanted = STRIDE1[fam][0].UNITS[name]
    cin, (B, H, W) = sum(segs), (2, 17, 19) if fam == "small" else (1, 64, 64)
    u = MC.make_unit(cin, cout, k, dil=dil, relu=relu, bn=bn, seed=cin + cout)
    g = torch.Generator().manual_seed(cin * 7 + cout)
    xs = [torch.randn(B, c, H, W, generator=g).requires_grad_(i in wanted) for i, c in enumerate(segs)]
    return u, xs, torch.randn(B, cout, H, W, generator=g)


def run_function(case):
    """Forward under hip_grad() and backward of one unit -> {"inputs": digest, "results": {gradient: digest}}."""
    import decnet_amd
    fam, name = case
    dev = torch.device("cuda:0")
    if fam == "conv3d":
        from decnet_amd import stage0, stage0_grad
        Ci, Co, relu, dims = T4.UNITS[name]
        g = torch.Generator().manual_seed(Ci * 7 + Co + dims[1])
        x = torch.randn(*dims, Ci, generator=g)
        w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (27 * Ci) ** 0.5
        scale, shift = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
        gy = torch.randn(*dims, Co, generator=g)
        ins = (x, w, scale, shift, gy)
        xd, wd, sd, hd = (t.to(dev).requires_grad_() for t in (x, w, scale, shift))
        packed = stage0_grad.unit_operands(wd.detach(), stage0.WINO_VARIANT.get(stage0.conv_algo(dims[1])), last=(Co == 1))
        decnet_amd.Conv3dFunction.apply(packed, relu, wd, sd, hd, xd).backward(gy.to(dev))
        got = {"dw": wd.grad, "dscale": sd.grad, "dshift": hd.grad, "dx": xd.grad}
    else:
        u, xs, gy = _unit_case(fam, name)
        ins = tuple(t.detach() for t in xs) + (gy,) + tuple(v for _, v in sorted(u.state_dict().items()))
        u = u.to(dev)
        xd = [t.detach().to(dev).requires_grad_(t.requires_grad) for t in xs]
        from decnet_amd import model
        model.TALLY = []
        try:
            with decnet_amd.hip_grad():
                y = u(xd[0] if len(xd) == 1 else tuple(xd))
            tally = [t["family"] for t in model.TALLY]
        finally:
            model.TALLY = None
        want = {"small": "conv_grad", "mfma": "mfma_grad"}.get(fam) or ("deconv_grad" if T3.UNITS[name][0] else "s3_grad")
        assert tally == [want], (case, tally)                   # the HIP Function, never the library arm
        y.backward(gy.to(dev))
        got = {n: p.grad for n, p in u.named_parameters()}
        got.update({"part%d" % i: t.grad for i, t in enumerate(xd) if t.requires_grad})
    torch.cuda.synchronize()
    assert all(t is not None for t in got.values()), (case, [k for k, t in got.items() if t is None])
    return {"inputs": digest(*ins), "results": {k: digest(t) for k, t in got.items()}}


def main(out, label=""):
    assert torch.cuda.is_available(), "the recording needs the MI355X"
    doc = {"library": label, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
           "entries": {case_id(c): run_entry(c) for c in entry_cases()}, "functions": {}, "unstable": []}
    assert len(doc["entries"]) == len(entry_cases())
    for c in function_cases():
        a, b = run_function(c), run_function(c)
        if a == b:
            doc["functions"][case_id(c)] = a
        else:
            doc["unstable"].append({"id": case_id(c), "differ": sorted(k for k in a["results"] if a["results"][k] != b["results"][k])})
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(doc["entries"]), "entry cases,", len(doc["functions"]), "function cases, unstable:", doc["unstable"])


if __name__ == "__main__":
    main(*sys.argv[1:3])
