#!/usr/bin/env python
"""Timing of the matrix-core conv backward (decnet_amd.hip_grad / Conv2dMfmaFunction over csrc/conv2d_mfma_grad.hip) on the
units of the model that Unit._route sends to "mfma", at config 5's level shapes (B = 4: 180 x 324 and 60 x 108).

    python tools/bench_conv2d_mfma_grad.py [--out profiles/conv2d_mfma_grad.json] [--calls 50] [--repeats 3]
    python tools/bench_conv2d_mfma_grad.py --parity profiles/conv2d_mfma_grad_parity.json   (no timing: the GPU test's ratios)

Per unit (one row per distinct shape), forward + backward with every parameter and the input taking a gradient:
    hip    under decnet_amd.hip_grad(): decnet_conv2d_mfma_cat_bn_act, decnet_conv2d_mfma_wgrad, dx on the forward entry
    lib    outside it: torch.cat, the library's convolution and backward, an unfused BatchNorm -- the parent's behaviour
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
Each leg is timed eager and as one GraphedStep replay (hip_graph, lib_graph: the same kernels without the host between them).
Two rows at the route's floor (1 x 64 x 64) follow the model's.
The library's eager time in the same run is the yardstick: a shape with lib_over_hip <= 1 belongs into model._mfma_grad_slower
(the rows are measured with that exclusion lifted and say whether it holds for them; the modules run the real routing).
The wgrad entry alone (`--calls` calls per graph replay): its flops 2 Cout (Cin k^2 + 1) B H W over its time as a share of
the 157.3 TFLOP/s fp32 matrix peak.  Then DynamicUpsampling(8, 3) and UpBlock(72, 24).conv: eager with hip / lib, hip as one
GraphedStep replay, and hip with the previous routing (the "mfma" units on the library, everything else as now)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_conv2d_grad import alternate, stats, timed  # noqa: E402

FP32 = 157.3e12
FINE, COARSE = (180, 324), (60, 108)
UNITS = [  # (where in the model, parts, Cout, k, relu, (H, W))
    ("conv1[1..2], deconv2.conv[1]", (24,), 24, 3, True, FINE),
    ("addition_trans1", (24,), 24, 1, True, FINE),
    ("deconv2.conv[0]", (24, 24), 24, 3, True, FINE),
    ("conv2[1..2], deconv3.conv[1]", (72,), 72, 3, True, COARSE),
    ("addition_trans2", (72,), 72, 1, True, COARSE),
    ("deconv3.conv[0]", (72, 72), 72, 3, True, COARSE),
    ("DynamicUpsampling(24).weight_learning[0]", (217,), 81, 3, True, COARSE),
    ("DynamicUpsampling(24).weight_learning[1]", (81,), 81, 3, True, COARSE),
    ("DynamicUpsampling(24).weight_learning[2]", (81,), 81, 3, False, COARSE),
    ("DynamicUpsampling(8).weight_learning[0]", (73,), 81, 3, True, FINE),
    ("DynamicUpsampling(8).weight_learning[1]", (81,), 81, 3, True, FINE),
    ("DynamicUpsampling(8).weight_learning[2]", (81,), 81, 3, False, FINE),
    ("SoftAttention.conv[0] at 1/3", (24, 1, 1, 1, 1), 8, 3, True, FINE),
    ("SoftAttention.conv[0] at 1/9", (72, 1, 1, 1, 1), 8, 3, True, COARSE),
]
FLOOR_UNITS = [  # the route's floor, 4096 pixels, one image: no layer of the model at config 5, the shapes of the GPU tests
    ("route floor", (24,), 24, 3, True, (64, 64)),
    ("route floor", (73,), 81, 3, True, (64, 64)),
]


def unit_rows(dev, batch, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import ops2d
    from decnet_amd import model
    from decnet_amd.graphs import GraphedStep
    import _model_cases as MC
    g = torch.Generator().manual_seed(11)
    rows = []
    slower, model._mfma_grad_slower = model._mfma_grad_slower, lambda *a: False     # measure the excluded shapes too
    a = torch.randn(4096, 4096, device=dev)                             # bring the clocks up before the first row
    for _ in range(100):
        a @ a
    torch.cuda.synchronize()
    for where, segs, cout, k, relu, (H, W) in UNITS + FLOOR_UNITS:
        B = batch if where != "route floor" else 1
        cin = sum(segs)
        u = MC.make_unit(cin, cout, k, relu=relu, seed=cin + cout).to(dev)
        xs = [torch.randn(B, s, H, W, generator=g).to(dev).requires_grad_() for s in segs]
        gy = torch.randn(B, cout, H, W, generator=g).to(dev)
        arg = xs[0] if len(xs) == 1 else tuple(xs)
        leaves = xs + list(u.parameters())

        def step(on, u=u, arg=arg, gy=gy, leaves=leaves):
            for t in leaves:
                t.grad = None
            with decnet_amd.hip_grad(on):
                y = u(arg)
            y.backward(gy)
        parts = len(segs) if len(segs) > 1 else None

        def captured(on, u=u, arg=arg, gy=gy):
            with decnet_amd.hip_grad(on):
                y = u(arg)
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
        row = {"where": where, "cin": cin, "cout": cout, "k": k, "parts": list(segs), "relu": relu, "shape": [B, H, W],
               "route": u._route(B, H, W, parts, switches=(True, True)), "grad_route": u._grad_route_mfma(B, H, W, parts),
               "excluded_as_slower": bool(slower(cin, cout, H * W)),
               "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
        t = row["ms_forward_backward"]
        row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
        if note is None:
            row["lib_over_hip_graph"] = t["lib_graph"]["median"] / t["hip_graph"]["median"]
        else:
            row["graph_note"] = note
        legs.clear()
        with torch.no_grad():                                           # the wgrad entry alone
            xd = [x.detach() for x in xs]
            y = u(arg).detach() if relu else None
            ops2d.conv2d_mfma_wgrad(xd, gy, y, k, 1)
            torch.cuda.synchronize()
            graph, per = torch.cuda.CUDAGraph(), calls
            with torch.cuda.graph(graph):
                for _ in range(per):
                    ops2d.conv2d_mfma_wgrad(xd, gy, y, k, 1)
            graph.replay()
            us = stats([timed(graph.replay, 4) / per * 1e3 for _ in range(repeats)])
        flops = 2.0 * cout * (cin * k * k + 1) * B * H * W
        row["wgrad"] = {"us_per_call": us, "flops": flops, "share_of_fp32_matrix_peak_at_median": flops / (us["median"] * 1e-6) / FP32,
                        "workspace_floats": int(ops2d.size("conv2d_mfma_wgrad_workspace_floats", B, cin, cout, H, W, k))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del xs, gy, arg, leaves, xd, y, graph
        torch.cuda.empty_cache()
    model._mfma_grad_slower = slower
    return rows


def module_rows(dev, B, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import model
    from decnet_amd.graphs import GraphedStep
    import _model_cases as MC
    g = torch.Generator().manual_seed(12)
    out = {}
    for name in ("DynamicUpsampling(8, 3)", "UpBlock(72, 24).conv"):
        H, W = FINE
        if name.startswith("Dynamic"):
            m = MC.seeded(lambda: model.DynamicUpsampling(8, 3), 1).to(dev)
            disp = (torch.rand(B, H, W, generator=g) * 20).to(dev).requires_grad_()
            fea = torch.randn(B, 8, 3 * H, 3 * W, generator=g).to(dev).requires_grad_()
            run, wrt = (lambda m=m, disp=disp, fea=fea: m(disp, fea)), [disp, fea]
            r = torch.randn(B, 3 * H, 3 * W, generator=g).to(dev)
        else:
            m = MC.seeded(lambda: model.UpBlock(72, 24), 2).to(dev).conv
            up, skip = (torch.randn(B, 24, H, W, generator=g).to(dev).requires_grad_() for _ in range(2))
            run, wrt = (lambda m=m, up=up, skip=skip: m((up, skip))), [up, skip]
            r = torch.randn(B, 24, H, W, generator=g).to(dev)
        leaves = wrt + list(m.parameters())

        def step(on, run=run, r=r):
            with decnet_amd.hip_grad(on):
                o = run()
            (o * r).sum().backward()

        def eager(on, leaves=leaves, step=step):
            for t in leaves:
                t.grad = None
            step(on)

        def previous(eager=eager):                                      # the routing before Conv2dMfmaFunction
            keep = model.Unit._grad_route_mfma
            model.Unit._grad_route_mfma = lambda self, *a, **k: None
            try:
                eager(True)
            finally:
                model.Unit._grad_route_mfma = keep
        graphed = GraphedStep(lambda step=step: step(True), grads_of=leaves)
        out[name] = alternate({"hip_eager": lambda: eager(True), "lib_eager": lambda: eager(False), "hip_graph": graphed,
                               "hip_eager_previous_routing": previous}, calls, repeats, warmup)
        print(json.dumps({name: out[name]}), flush=True)
        del graphed
        torch.cuda.empty_cache()
    return out


def parity(path):
    import test_conv2d_mfma_grad_gpu as T
    rows = {name: T.chain_parity(name) for name in ("upblock", "upsampling")}
    worst = max(r["hip_vs_f64"] / r["gate"] for t in rows.values() for r in t.values())
    ratios = [r["hip_over_f32"] for t in rows.values() for r in t.values() if r["hip_over_f32"] is not None]
    rep = {"what": "max|g_hip - g64|, max|g32 - g64| and the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)) per tensor; "
                   "g64 and g32: the CPU chain with the GPU run's ReLU masks imposed",
           "worst_hip_over_gate": worst, "worst_hip_over_f32": max(ratios), "tensors": rows}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: rep[k] for k in ("worst_hip_over_gate", "worst_hip_over_f32")}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_mfma_grad.json"))
    ap.add_argument("--parity", default=None, metavar="JSON")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_mfma_grad.py measures on the GPU; there is none")
    if a.parity:
        return parity(a.parity)
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "batch": a.batch,
              "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup, "fp32_matrix_flop_per_s": FP32,
              "units": unit_rows(dev, a.batch, a.calls, a.repeats, a.warmup),
              "modules_ms_forward_backward": module_rows(dev, a.batch, a.calls, a.repeats, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
