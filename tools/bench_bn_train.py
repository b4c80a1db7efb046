#!/usr/bin/env python
"""Timing of the conv units in ``.train()`` mode under decnet_amd.hip_grad() (Unit._forward_grad_train: the route's conv
Function with scale 1, shift 0 and no ReLU, then conv2d_grad.BatchNormActFunction over csrc/batchnorm.hip) on every Unit of
the model at config 5's sizes: B = 8 in the feature extractor (both views), B = 4 in the mask generators, the dynamic
upsampling, the attention and the refinement.

    python tools/bench_bn_train.py [--out profiles/bn_train.json] [--calls 50] [--repeats 3]

The units and their input shapes are found by running each sub-module once in eval mode under forward hooks; equal
(layer, shape) pairs are timed once.  Per unit, forward + backward with every parameter and the input taking a gradient:
    hip    under decnet_amd.hip_grad(): the conv Function of the unit's route, then the three BatchNorm launches each way
    lib    outside it: the library's convolution -> batch norm -> ReLU under autograd -- the parent's behaviour
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
Each leg is timed eager and as one GraphedStep replay (hip_graph, lib_graph).  The library's time in the same run is the
yardstick: a unit with lib_over_hip <= 1 belongs into model._bn_train_slower (the rows are measured with that exclusion
lifted and say whether it holds for them).  Units without a train-mode route
(Unit._grad_route_train is None) run the library either way and are listed, not timed.
The BatchNorm entries alone, per distinct output shape (`--calls` calls per graph replay): the forward entry (three launches:
z read twice, y written once, 12 B per element) and the backward entry (three launches: z and gy read twice, gz written
once, 20 B per element), each against its bytes at 8 TB/s.
`refinement[2]`, `soft_attention[2].fuse` and `DynamicUpsampling(8, 3)` are timed as modules in train mode the same way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_conv2d_grad import alternate, stats, timed  # noqa: E402

HBM = 8.0e12
FULL, L1, L2, L3 = (540, 972), (180, 324), (60, 108), (20, 36)
LEVELS = [L2, L1, FULL]                # stage 1, 2, 3: the level of detail_detection[i], dynamic_upsampling[i], ...


def _net():
    import torch
    from decnet_amd.model import SparseDenseNetRefinementMask
    torch.manual_seed(17)
    return SparseDenseNetRefinementMask(max_disp=216, base_channels=8, num_stage=4, down_scale=3, use_detail=True)


def _module_inputs(net, dev, B_ext=8, B=4):
    """(name, module call on random inputs) of every sub-module with Units, at config 5's sizes."""
    import torch
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                          # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g).to(dev)                           # noqa: E731
    ch = net.feature_extractor.out_channels                                       # [216, 72, 24, 8]
    calls = [("feature_extractor", lambda: net.feature_extractor(r(B_ext, 3, *FULL)))]
    for i, (H, W) in enumerate(LEVELS):
        c = ch[i + 1]
        calls += [
            ("detail_detection.%d" % i, lambda i=i, c=c, H=H, W=W: net.detail_detection[i](r(B, c, H, W), r(B, 3 * c, H // 3, W // 3))),
            ("dynamic_upsampling.%d" % i, lambda i=i, c=c, H=H, W=W: net.dynamic_upsampling[i](u(B, H // 3, W // 3) * 4, r(B, c, H, W))),
            # (unit by unit: fuse() enters its first and last unit below Module.__call__, where no hook sees them)
            ("soft_attention.%d" % i, lambda i=i, c=c, H=H, W=W: net.soft_attention[i].conv(
                (r(B, c, H, W), u(B, 1, H, W) * 4, u(B, 1, H, W) * 4, (u(B, 1, H, W) < 0.5).float(), -u(B, 1, H, W)))),
            ("refinement.%d" % i, lambda i=i, c=c, H=H, W=W: net.refinement[i](r(B, c, H, W), r(B, c, H, W), u(B, H, W) * 4)),
        ]
    return calls


def find_units(net, dev):
    """-> [(names, Unit, [shape of every input part])], equal (layer, shape) pairs merged."""
    import torch
    from decnet_amd.model import Unit
    seen, found = {}, []

    def hook(name):
        def pre(mod, args):
            x = args[0]
            shapes = [tuple(t.shape) for t in (x if isinstance(x, (tuple, list)) else (x,))]
            c = mod.conv
            key = (type(c).__name__, c.in_channels, c.out_channels, c.kernel_size, c.stride, c.dilation, bool(mod.relu),
                   mod.bn is not None, tuple(shapes))
            if key in seen:
                seen[key][0].append(name)
            else:
                seen[key] = ([name], mod, shapes)
                found.append(seen[key])
        return pre
    hooks = [m.register_forward_pre_hook(hook(n)) for n, m in net.named_modules() if isinstance(m, Unit)]
    net.eval()
    with torch.no_grad():
        for _, call in _module_inputs(net, dev):
            call()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    return found


def _legs(step, captured, leaves):
    import torch
    from decnet_amd.graphs import GraphedStep
    legs = {"hip": lambda: step(True), "lib": lambda: step(False)}
    note = None
    try:                                                                # the same step as one graph replay: no host in it
        legs["hip_graph"] = GraphedStep(lambda: captured(True), grads_of=leaves)
        legs["lib_graph"] = GraphedStep(lambda: captured(False), grads_of=leaves)
    except RuntimeError as e:
        legs.pop("hip_graph", None)
        note = "the library's step was not captured: %s" % str(e).splitlines()[0]
        torch.cuda.synchronize()
    return legs, note


def _ratios(row, note):
    t = row["ms_forward_backward"]
    row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
    if note is None:
        row["lib_over_hip_graph"] = t["lib_graph"]["median"] / t["hip_graph"]["median"]
    else:
        row["graph_note"] = note
    return row


def unit_rows(found, dev, calls, repeats, warmup, emit):
    import copy
    import torch
    import decnet_amd
    from decnet_amd import model
    g = torch.Generator().manual_seed(11)
    rows, bn_shapes = [], {}
    slower, model._bn_train_slower = model._bn_train_slower, lambda *a: False       # measure the excluded units too
    try:
        for names, unit, shapes in found:
            u = copy.deepcopy(unit).to(dev).train()
            c = u.conv
            B, _, H, W = shapes[0]
            parts = len(shapes) if len(shapes) > 1 else None
            row = {"where": names, "layer": type(c).__name__, "cin": c.in_channels, "cout": c.out_channels, "k": c.kernel_size[0],
                   "stride": c.stride[0], "dilation": c.dilation[0], "relu": bool(u.relu), "bn": u.bn is not None,
                   "parts": [s[1] for s in shapes], "shape": [B, H, W],
                   "route": u._route(B, H, W, parts, switches=(True, True)),
                   "grad_route_train": u._grad_route_train(B, H, W, parts)}
            if row["grad_route_train"] is not None:
                row["excluded_as_slower"] = bool(slower(row["grad_route_train"], c.in_channels, c.out_channels, c.dilation[0],
                                                        B * H * W))
            if row["grad_route_train"] is None:                             # the library in either leg: nothing to compare
                rows.append(emit(row))
                continue
            xs = [torch.randn(s, generator=g).to(dev).requires_grad_() for s in shapes]
            arg = tuple(xs) if parts else xs[0]
            with torch.no_grad():
                gy = torch.randn_like(u(arg))
            leaves = xs + list(u.parameters())

            def step(on, u=u, arg=arg, gy=gy, leaves=leaves):
                for t in leaves:
                    t.grad = None
                with decnet_amd.hip_grad(on):
                    y = u(arg)
                y.backward(gy)

            def captured(on, u=u, arg=arg, gy=gy):
                with decnet_amd.hip_grad(on):
                    y = u(arg)
                y.backward(gy)
            legs, note = _legs(step, captured, leaves)
            row["ms_forward_backward"] = alternate(legs, calls, repeats, warmup)
            rows.append(emit(_ratios(row, note)))
            bn_shapes.setdefault(tuple(gy.shape), bool(u.relu))
            legs.clear()
            del xs, arg, gy, leaves
            torch.cuda.empty_cache()
    finally:
        model._bn_train_slower = slower
    return rows, bn_shapes


def bn_rows(bn_shapes, dev, calls, repeats, emit):
    """The forward entry and the backward entry alone, `calls` calls per graph replay."""
    import torch
    from decnet_amd import ops2d
    g = torch.Generator().manual_seed(13)
    rows = []
    for shape, relu in sorted(bn_shapes.items()):
        C = shape[1]
        z, gy = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
        w, b = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        _, st = ops2d.bn_train_forward(z, w, b, 1e-5, 0.1, rm, rv, relu)
        row = {"shape": list(shape), "relu": relu, "elements": z.numel()}
        for name, fn, per_el in (("forward", lambda: ops2d.bn_train_forward(z, w, b, 1e-5, 0.1, rm, rv, relu), 12.0),
                                 ("backward", lambda: ops2d.bn_train_backward(z, gy, w, b, st, relu), 20.0)):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            us = stats([timed(graph.replay, 4) / calls * 1e3 for _ in range(repeats)])
            nbytes = per_el * z.numel()
            row[name] = {"launches": 3, "us_per_call": us, "bytes": nbytes,
                         "share_of_8TBps_at_median": nbytes / (us["median"] * 1e-6) / HBM}
            del graph
        rows.append(emit(row))
        del z, gy
        torch.cuda.empty_cache()
    return rows


def module_rows(net, dev, calls, repeats, warmup, emit, B=4):
    import copy
    import torch
    import decnet_amd
    from decnet_amd.model import DynamicUpsampling
    g = torch.Generator().manual_seed(19)
    H, W = FULL
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                          # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g).to(dev)                           # noqa: E731
    torch.manual_seed(23)
    cases = [
        ("refinement[2]", copy.deepcopy(net.refinement[2]), lambda m, t: m(t["left"], t["right"], t["disp"])[0],
         {"left": r(B, 8, H, W), "right": r(B, 8, H, W), "disp": u(B, H, W) * 4}, ("disp",)),
        ("soft_attention[2].fuse", copy.deepcopy(net.soft_attention[2]),
         lambda m, t: m.fuse(t["fea"], t["dense"], t["sparse"], t["mask"], t["var"]),
         {"fea": r(B, 8, H, W), "dense": u(B, H, W) * 4, "sparse": u(B, H, W) * 4, "mask": (u(B, H, W) < 0.5).float(),
          "var": u(B, H, W)}, ("dense", "sparse")),
        ("DynamicUpsampling(8, 3)", DynamicUpsampling(8, 3), lambda m, t: m(t["disp"], t["fea"]),
         {"disp": u(B, H // 3, W // 3) * 4, "fea": r(B, 8, H, W)}, ("disp", "fea")),
    ]
    rows = []
    for name, m, fwd, t, wrt in cases:
        m = m.to(dev).train()
        for k in wrt:
            t[k].requires_grad_()
        with torch.no_grad():
            gy = torch.randn_like(fwd(m, t))
        leaves = [t[k] for k in wrt] + list(m.parameters())

        def step(on, m=m, t=t, gy=gy, leaves=leaves, fwd=fwd):
            for p in leaves:
                p.grad = None
            with decnet_amd.hip_grad(on):
                y = fwd(m, t)
            y.backward(gy)

        def captured(on, m=m, t=t, gy=gy, fwd=fwd):
            with decnet_amd.hip_grad(on):
                y = fwd(m, t)
            y.backward(gy)
        legs, note = _legs(step, captured, leaves)
        row = {"module": name, "shape": [B, H, W], "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
        rows.append(emit(_ratios(row, note)))
        legs.clear()
        del t, gy, leaves
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_train.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_train.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")

    def emit(row):
        print(json.dumps(row), flush=True)
        return row
    net = _net().to(dev)
    found = find_units(net, dev)
    x = torch.randn(4096, 4096, device=dev)                             # bring the clocks up before the first row
    for _ in range(100):
        x @ x
    torch.cuda.synchronize()
    del x
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "calls": a.calls,
              "repeats": a.repeats, "warmup": a.warmup, "hbm_bytes_per_s": HBM}
    report["units"], bn_shapes = unit_rows(found, dev, a.calls, a.repeats, a.warmup, emit)
    report["bn_entries"] = bn_rows(bn_shapes, dev, a.calls, a.repeats, emit)
    report["modules"] = module_rows(net, dev, a.calls, a.repeats, a.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
