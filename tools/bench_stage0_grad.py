#!/usr/bin/env python
"""Timing of the stage-0 backward (decnet_amd.hip_grad / Conv3dFunction over csrc/conv3d_grad.hip) at the stage-0 volumes of
config 5 (B = 4, C = 216, 20 x 36, D = 8: 23 040 voxels) and config 2 (B = 8: 46 080 voxels).

    python tools/bench_stage0_grad.py [--out profiles/stage0_grad.json] [--calls 50] [--repeats 3]

Per size, forward + backward of one 216 -> 216 unit and of the 216 -> 1 unit, every parameter and the input taking a gradient:
    hip    Conv3dFunction: the per-layer inference entry, decnet_conv3d_wgrad, dx on the forward entry
    lib    stage0_grad.unit_library: torch's conv3d on the channels-last-3d view, * scale + shift, ReLU, under autograd
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
Each leg is timed eager and as one GraphedStep replay.  The library's eager time in the same run is the yardstick: a shape
with lib_over_hip <= 1 belongs into stage0._conv3d_grad_slower.
The wgrad entry alone: its flops 2 Co (27 Ci + 1) voxels over its time as a share of the 157.3 TFLOP/s fp32 matrix peak, and
its operand bytes (x, gm, G once) at 8 TB/s.  Then CostRegNetNoDown.stage0 forward + backward on both arms, with the head
(the cost volume, forward + backward) and the tail (soft-argmax in torch ops) timed on their own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_conv2d_grad import alternate, timed, stats  # noqa: E402

FP32, HBM = 157.3e12, 8.0e12
C, H, W, D = 216, 20, 36, 8
SIZES = {"config5": 4, "config2": 8}


def with_graphs(legs, captured, leaves):
    """Add `name`_graph legs (one GraphedStep replay each); -> a note when a capture failed."""
    import torch
    from decnet_amd.graphs import GraphedStep
    try:
        for name, fn in captured.items():
            legs[name + "_graph"] = GraphedStep(fn, grads_of=leaves)
    except RuntimeError as e:
        for name in captured:
            legs.pop(name + "_graph", None)
        torch.cuda.synchronize()
        return "not captured: %s" % str(e).splitlines()[0]
    return None


def unit_row(dev, B, co, relu, calls, repeats, warmup):
    import torch
    from decnet_amd import Conv3dFunction, ops2d, stage0, stage0_grad
    g = torch.Generator().manual_seed(11 + co)
    dims = (B, D, H, W)
    x = torch.randn(*dims, C, generator=g).to(dev).requires_grad_()
    w = (torch.randn(co, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(dev).requires_grad_()
    scale, shift = (torch.rand(co, generator=g) + 0.5).to(dev).requires_grad_(), torch.zeros(co, device=dev, requires_grad=True)
    gy = torch.randn(*dims, co, generator=g).to(dev)
    variant = stage0.WINO_VARIANT.get(stage0.conv_algo(D))
    packed = stage0_grad.unit_operands(w.detach(), variant, last=(co == 1))
    leaves = [x, w, scale, shift]

    def hip():
        Conv3dFunction.apply(packed, relu, w, scale, shift, x).backward(gy)

    def lib():
        stage0_grad.unit_library(x, w, scale, shift, relu).backward(gy)

    def eager(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn()
        return run
    legs = {"hip": eager(hip), "lib": eager(lib)}
    note = with_graphs(legs, {"hip": hip, "lib": lib}, leaves)
    row = {"unit": "%d -> %d" % (C, co), "relu": relu, "dims": list(dims), "voxels": B * D * H * W, "forward_entry": packed["kind"],
           "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
    t = row["ms_forward_backward"]
    row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
    if note is None:
        row["lib_over_hip_graph"] = t["lib_graph"]["median"] / t["hip_graph"]["median"]
    else:
        row["graph_note"] = note
    legs.clear()
    with torch.no_grad():                                               # the wgrad entry alone
        xd = x.detach()
        y = torch.randn(*dims, co, generator=g).to(dev) if relu else None
        ms = stats([timed(lambda: ops2d.conv3d_wgrad(xd, gy, y, dims, C, co), calls) for _ in range(repeats)])["median"]
    n = B * D * H * W
    flops, nbytes = 2.0 * co * (27 * C + 1) * n, 4.0 * (n * C + n * co * (3 if relu else 1) + co * (27 * C + 1))
    row["wgrad"] = {"ms": ms, "flop": flops, "share_of_fp32_matrix_peak": flops / (ms * 1e-3) / FP32,
                    "bound_ms_matrix": flops / FP32 * 1e3, "operand_bytes": nbytes, "bound_ms_hbm": nbytes / HBM * 1e3,
                    "workspace_floats": int(ops2d.size("conv3d_wgrad_workspace_floats", *dims, C, co))}
    return row


def stage0_row(dev, B, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import stage0, stage0_grad
    import _model_cases as MC
    mod = MC.seeded(lambda: decnet_amd.CostRegNetNoDown(C, 2 * C, "cor"), 5).to(dev).eval()
    g = torch.Generator().manual_seed(12)
    L, R = (torch.relu(torch.randn(B, C, H, W, generator=g)).to(dev).requires_grad_() for _ in range(2))
    r, r2 = torch.randn(B, H, W, generator=g).to(dev), torch.randn(B, D, H, W, generator=g).to(dev)
    leaves = [L, R] + list(mod.parameters())
    slower = stage0._conv3d_grad_slower

    def step(library):
        stage0._conv3d_grad_slower = (lambda c, v: True) if library else slower
        try:
            with decnet_amd.hip_grad():
                pred, reg = mod.stage0(L, R, D, return_reg=True)
            ((pred * r).sum() + (reg * r2).sum()).backward()
        finally:
            stage0._conv3d_grad_slower = slower

    def eager(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn()
        return run
    legs = {"hip": eager(lambda: step(False)), "lib": eager(lambda: step(True))}
    note = with_graphs(legs, {"hip": lambda: step(False), "lib": lambda: step(True)}, leaves)
    gcv = torch.randn(B, D, H, W, C, generator=g).to(dev)
    reg0 = torch.randn(B, D, H, W, generator=g).to(dev).requires_grad_()

    def head():
        L.grad = R.grad = None
        stage0_grad.CostVolumeFunction.apply(L, R, D, "cor").backward(gcv)

    def tail():
        reg0.grad = None
        (mod._softargmax(reg0) * r).sum().backward()
    legs.update(head=head, tail=tail)
    row = {"B": B, "voxels": B * D * H * W, "routed_to_library": bool(slower(C, B * D * H * W)),
           "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
    t = row["ms_forward_backward"]
    row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
    row["head_share_of_hip"] = t["head"]["median"] / t["hip"]["median"]
    row["tail_share_of_hip"] = t["tail"]["median"] / t["hip"]["median"]
    if note is not None:
        row["graph_note"] = note
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage0_grad.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import decnet_amd
    dev = torch.device("cuda:0")
    warm = torch.randn(4096, 4096, device=dev)                          # bring the clocks up before the first row
    for _ in range(100):
        warm @ warm
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "library": decnet_amd.version(), "calls": a.calls, "repeats": a.repeats,
           "fp32_matrix_flop_per_s": FP32, "hbm_bytes_per_s": HBM, "C": C, "plane": [H, W], "D": D, "sizes": {}}
    for name, B in SIZES.items():
        out["sizes"][name] = {
            "units": [unit_row(dev, B, C, True, a.calls, a.repeats, a.warmup),
                      unit_row(dev, B, 1, False, a.calls, a.repeats, a.warmup)],
            "stage0": stage0_row(dev, B, a.calls, a.repeats, a.warmup)}
        print(json.dumps({name: out["sizes"][name]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
