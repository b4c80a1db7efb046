#!/usr/bin/env python
"""Timing of the few-channel conv backward (decnet_amd.hip_grad / Conv2dSmallFunction over csrc/conv2d_grad.hip) on the ten
stage-3 units of Refinement(8, 8, stage_id=3) and SoftAttention(12, 8) at config 5's per-GPU batch (B = 4, 540 x 972).

    python tools/bench_conv2d_grad.py [--out profiles/conv2d_grad.json] [--calls 50] [--repeats 3]
    python tools/bench_conv2d_grad.py --parity profiles/conv2d_grad_parity.json      (no timing: the ratios of the GPU test)

Per unit, forward + backward with every parameter and the input (for the two first layers: the disparity-like last part
alone, as with a frozen trunk) taking a gradient:
    hip    under decnet_amd.hip_grad(): our forward, decnet_conv2d_wgrad, dx on the forward kernel
    lib    outside it: the library under autograd -- the parent commit's behaviour and the yardstick
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
The wgrad entry alone (`--calls` calls per graph replay): its algorithmic bytes 4 B H W (Cin + 3 Cout) and flops
2 Cout Cin k^2 B H W over its time, as a share of the binding roof (8 TB/s, 157.3 TFLOP/s fp32).  Then the two whole
modules: eager with hip / lib, and hip as one GraphedStep replay."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM, FP32 = 8.0e12, 157.3e12


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def alternate(legs, calls, repeats, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            ms[name].append(timed(fn, calls))
    return {k: stats(v) for k, v in ms.items()}


def unit_rows(dev, B, H, W, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import ops2d
    import _model_cases as MC
    from decnet_amd.model import Refinement, SoftAttention
    g = torch.Generator().manual_seed(11)
    mods = {"refinement": (MC.seeded(lambda: Refinement(8, 8, stage_id=3), 1).to(dev), (8, 8, 1)),
            "attention": (MC.seeded(lambda: SoftAttention(12, 8), 2).to(dev), (8, 1, 1, 1, 1))}
    rows = []
    for mname, (m, first) in mods.items():
        for i, u in enumerate(m.conv):
            c = u.conv
            segs = first if i == 0 else (c.in_channels,)
            xs = [torch.randn(B, s, H, W, generator=g).to(dev) for s in segs]
            xs[-1].requires_grad_()
            gy = torch.randn(B, c.out_channels, H, W, generator=g).to(dev)
            arg = xs[0] if len(xs) == 1 else tuple(xs)
            leaves = [xs[-1]] + list(u.parameters())

            def step(on, u=u, arg=arg, gy=gy, leaves=leaves):
                for t in leaves:
                    t.grad = None
                with decnet_amd.hip_grad(on):
                    y = u(arg)
                y.backward(gy)
            row = {"module": mname, "unit": i, "cin": c.in_channels, "cout": c.out_channels, "k": c.kernel_size[0],
                   "dilation": c.dilation[0], "parts": list(segs), "relu": bool(u.relu),
                   "grad_route": u._grad_route(B, H, W, len(segs) if len(segs) > 1 else None),
                   "ms_forward_backward": alternate({"hip": lambda: step(True), "lib": lambda: step(False)}, calls, repeats,
                                                    warmup)}
            t = row["ms_forward_backward"]
            row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
            # the wgrad entry alone
            with torch.no_grad():
                xd = [x.detach() for x in xs]
                y = u(arg).detach() if u.relu else None
                k, d = c.kernel_size[0], c.dilation[0]
                ops2d.conv2d_wgrad(xd, gy, y, k, d)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(calls):
                        ops2d.conv2d_wgrad(xd, gy, y, k, d)
                graph.replay()
                us = stats([timed(graph.replay, 1) / calls * 1e3 for _ in range(repeats)])
            px = B * H * W
            nbytes, flops = 4.0 * px * (c.in_channels + 3 * c.out_channels), 2.0 * c.out_channels * c.in_channels * k * k * px
            floor_us = max(nbytes / HBM, flops / FP32) * 1e6
            row["wgrad"] = {"us_per_call": us, "bytes": nbytes, "flops": flops,
                            "binding_roof": "hbm" if nbytes / HBM >= flops / FP32 else "fp32",
                            "share_of_roof_at_median": floor_us / us["median"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs, gy, arg, leaves, xd, y, graph
            torch.cuda.empty_cache()
    return rows


def module_rows(dev, B, H, W, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    import _model_cases as MC
    from decnet_amd.model import Refinement, SoftAttention
    g = torch.Generator().manual_seed(12)
    out = {}
    for name in ("refinement", "attention"):
        if name == "refinement":
            m = MC.seeded(lambda: Refinement(8, 8, stage_id=3), 1).to(dev)
            left, right = (torch.randn(B, 8, H, W, generator=g).to(dev) for _ in range(2))
            disp = (torch.rand(B, H, W, generator=g) * 4).to(dev).requires_grad_()
            run, wrt = (lambda m=m, left=left, right=right, disp=disp: m(left, right, disp)[0]), [disp]
        else:
            m = MC.seeded(lambda: SoftAttention(12, 8), 2).to(dev)
            fea = torch.randn(B, 8, H, W, generator=g).to(dev)
            dense, sparse = ((torch.rand(B, H, W, generator=g) * 4).to(dev).requires_grad_() for _ in range(2))
            mask, var = (torch.rand(B, H, W, generator=g) < 0.5).float().to(dev), torch.rand(B, H, W, generator=g).to(dev)
            run = lambda m=m, fea=fea, dense=dense, sparse=sparse, mask=mask, var=var: m.fuse(fea, dense, sparse, mask, var)  # noqa: E731
            wrt = [dense, sparse]
        r = torch.randn(B, H, W, generator=g).to(dev)
        leaves = wrt + list(m.parameters())

        def step(on, run=run, r=r):
            with decnet_amd.hip_grad(on):
                o = run()
            (o * r).sum().backward()

        def eager(on, leaves=leaves, step=step):
            for t in leaves:
                t.grad = None
            step(on)
        graphed = GraphedStep(lambda step=step: step(True), grads_of=leaves)
        out[name] = alternate({"hip_eager": lambda: eager(True), "lib_eager": lambda: eager(False), "hip_graph": graphed},
                              calls, repeats, warmup)
        print(json.dumps({name: out[name]}), flush=True)
        del graphed
        torch.cuda.empty_cache()
    return out


def parity(path):
    import test_conv2d_grad_gpu as T
    rows = {name: T.parity_ratios(name) for name in sorted(T.GR.MODULE_SEEDS)}
    worst = max(r["hip_vs_f64"] / r["gate"] for t in rows.values() for r in t.values())
    ratios = [r["hip_over_f32"] for t in rows.values() for r in t.values() if r["hip_over_f32"] is not None]
    rep = {"what": "max|g_hip - g64|, max|g32 - g64| and the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)) per tensor",
           "worst_hip_over_gate": worst, "worst_hip_over_f32": max(ratios), "tensors": rows}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: rep[k] for k in ("worst_hip_over_gate", "worst_hip_over_f32")}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_grad.json"))
    ap.add_argument("--parity", default=None, metavar="JSON")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=(4, 540, 972), metavar=("B", "H", "W"))
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_grad.py measures on the GPU; there is none")
    if a.parity:
        return parity(a.parity)
    dev = torch.device("cuda:0")
    B, H, W = a.shape
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "shape": [B, H, W],
              "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup, "roofs": {"hbm_B_per_s": HBM, "fp32_flop_per_s": FP32},
              "units": unit_rows(dev, B, H, W, a.calls, a.repeats, a.warmup),
              "modules_ms_forward_backward": module_rows(dev, B, H, W, a.calls, a.repeats, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
