#!/usr/bin/env python
"""Timing of the stride-3 conv / transposed-conv backward (decnet_amd.hip_grad / Conv2dS3Function, Deconv2dS3Function over
csrc/conv2d_mfma_grad.hip and csrc/unfold.hip) on the nine stride-3 units of the model at config 5's sizes: B = 8 for the
extractor's units (both views), B = 4 for the mask generators' transposed convolutions.

    python tools/bench_conv2d_s3_grad.py [--out profiles/conv2d_s3_grad.json] [--calls 50] [--repeats 3]
    python tools/bench_conv2d_s3_grad.py --parity profiles/conv2d_s3_grad_parity.json   (no timing: the GPU test's ratios)

Per unit, forward + backward with every parameter and the input taking a gradient:
    hip    under decnet_amd.hip_grad(): the unit's inference entry, the stride-3 wgrad entry, dx on the matrix-core forward
    lib    outside it: the library's convolution and backward with an unfused BatchNorm -- the parent's behaviour
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
Each leg is timed eager and as one GraphedStep replay (hip_graph, lib_graph).  The library's eager time in the same run is
the yardstick: a shape with lib_over_hip <= 1 belongs into model._s3_grad_slower (the rows are measured with that exclusion
lifted and say whether it holds for them).
The wgrad entry alone (`--calls` calls per graph replay): its operand bytes 4 (|x| + 2 |gy| + |gm|) (|gy| + |gm| without
ReLU) at 8 TB/s and its flops 2 Cp (9 Cq + 1) B (coarse pixels) at the 157.3 TFLOP/s fp32 matrix peak, each over its time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_conv2d_grad import alternate, stats, timed  # noqa: E402

HBM, FP32 = 8.0e12, 157.3e12
FULL, L1, L2, L3 = (540, 972), (180, 324), (60, 108), (20, 36)
UNITS = [  # (where in the model, transposed, Cin, Cout, bn, B, (H, W) of the input)
    ("conv1[0]", False, 8, 24, True, 8, FULL),
    ("conv2[0]", False, 24, 72, True, 8, L1),
    ("conv3_1", False, 72, 216, True, 8, L2),
    ("deconv3.deconv", True, 216, 72, True, 8, L3),
    ("deconv2.deconv", True, 72, 24, True, 8, L2),
    ("deconv1.deconv", True, 24, 8, True, 8, L1),
    ("GenerateSparseMask(72).deconv[0]", True, 216, 8, False, 4, L3),
    ("GenerateSparseMask(24).deconv[0]", True, 72, 8, False, 4, L2),
    ("GenerateSparseMask(8).deconv[0]", True, 24, 8, False, 4, L1),
]


def unit_rows(dev, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import model, ops2d
    from decnet_amd.graphs import GraphedStep
    import _model_cases as MC
    g = torch.Generator().manual_seed(11)
    rows = []
    slower, model._s3_grad_slower = model._s3_grad_slower, lambda *a: False         # measure the excluded shapes too
    a = torch.randn(4096, 4096, device=dev)                             # bring the clocks up before the first row
    for _ in range(100):
        a @ a
    torch.cuda.synchronize()
    for where, tr, cin, cout, bn, B, (H, W) in UNITS:
        u = MC.make_unit(cin, cout, 3, stride=3, bn=bn, transposed=tr, seed=cin + cout).to(dev)
        Ho, Wo = (3 * H, 3 * W) if tr else ((H - 1) // 3 + 1, (W - 1) // 3 + 1)
        x = torch.randn(B, cin, H, W, generator=g).to(dev).requires_grad_()
        gy = torch.randn(B, cout, Ho, Wo, generator=g).to(dev)
        leaves = [x] + list(u.parameters())

        def step(on, u=u, x=x, gy=gy, leaves=leaves):
            for t in leaves:
                t.grad = None
            with decnet_amd.hip_grad(on):
                y = u(x)
            y.backward(gy)

        def captured(on, u=u, x=x, gy=gy):
            with decnet_amd.hip_grad(on):
                y = u(x)
            y.backward(gy)
        legs = {"hip": lambda: step(True), "lib": lambda: step(False)}
        note = None
        try:                                                            # the same step as one graph replay: no host in it
            legs["hip_graph"] = GraphedStep(lambda: captured(True), grads_of=leaves)
            legs["lib_graph"] = GraphedStep(lambda: captured(False), grads_of=leaves)
        except RuntimeError as e:
            legs.pop("hip_graph", None)
            note = "the library's step was not captured: %s" % str(e).splitlines()[0]
            torch.cuda.synchronize()
        route = "deconv" if tr else "s3"
        row = {"where": where, "transposed": tr, "cin": cin, "cout": cout, "bn": bn, "shape": [B, H, W],
               "route": u._route(B, H, W, None, switches=(True, True)), "grad_route": u._grad_route_s3(B, H, W),
               "excluded_as_slower": bool(slower(route, cin, cout, B * H * W)),
               "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
        assert row["grad_route"] == route, row
        t = row["ms_forward_backward"]
        row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
        if note is None:
            row["lib_over_hip_graph"] = t["lib_graph"]["median"] / t["hip_graph"]["median"]
        else:
            row["graph_note"] = note
        legs.clear()
        wgrad = ops2d.deconv2d_k3s3_wgrad if tr else ops2d.conv2d_k3s3_wgrad
        with torch.no_grad():                                           # the wgrad entry alone
            xd, y = x.detach(), u(x).detach()
            wgrad(xd, gy, y)
            torch.cuda.synchronize()
            graph, per = torch.cuda.CUDAGraph(), calls
            with torch.cuda.graph(graph):
                for _ in range(per):
                    wgrad(xd, gy, y)
            graph.replay()
            us = stats([timed(graph.replay, 4) / per * 1e3 for _ in range(repeats)])
        cp, cq, coarse = (cin, cout, H * W) if tr else (cout, cin, Ho * Wo)
        flops = 2.0 * cp * (9 * cq + 1) * B * coarse
        nbytes = 4.0 * (x.numel() + 3 * gy.numel() + (gy.numel() if tr else 0))     # (transposed: gm once more, for gsum)
        sec = us["median"] * 1e-6
        row["wgrad"] = {"us_per_call": us, "flops": flops, "operand_bytes": nbytes,
                        "share_of_fp32_matrix_peak_at_median": flops / sec / FP32,
                        "share_of_8TBps_at_median": nbytes / sec / HBM,
                        "workspace_floats": int(ops2d.size(("deconv2d" if tr else "conv2d") + "_k3s3_wgrad_workspace_floats",
                                                           B, cin, cout, H, W))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, gy, leaves, xd, y, graph
        torch.cuda.empty_cache()
    model._s3_grad_slower = slower
    return rows


def parity(path):
    import test_conv2d_s3_grad_gpu as T
    rows = T.chain_parity()
    ratios = [r["hip_over_f32"] for r in rows.values() if r["hip_over_f32"] is not None]
    rep = {"what": "the chain f0 [1,8,192,192] -> conv1 -> UpBlock(24, 8): max|g_hip - g64|, max|g32 - g64| and the gate "
                   "max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)) per tensor; g64 and g32: the CPU chain with the GPU run's "
                   "ReLU masks imposed",
           "worst_hip_over_gate": max(r["hip_vs_f64"] / r["gate"] for r in rows.values()),
           "worst_hip_over_f32": max(ratios), "tensors": rows}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: rep[k] for k in ("worst_hip_over_gate", "worst_hip_over_f32")}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_s3_grad.json"))
    ap.add_argument("--parity", default=None, metavar="JSON")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_s3_grad.py measures on the GPU; there is none")
    if a.parity:
        return parity(a.parity)
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "calls": a.calls,
              "repeats": a.repeats, "warmup": a.warmup, "fp32_matrix_flop_per_s": FP32, "hbm_bytes_per_s": HBM,
              "units": unit_rows(dev, a.calls, a.repeats, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
