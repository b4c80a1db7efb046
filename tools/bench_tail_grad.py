#!/usr/bin/env python
"""Timing of the tail Functions of decnet_amd/tail_grad.py (csrc/tail_grad.hip) at config 5's per-GPU batch: B = 4,
540 x 972, C = 8 for the warp and fold3, 180 x 324 -> 540 x 972 for the upsampling.

    python tools/bench_tail_grad.py [--out profiles/tail_grad.json] [--calls 50] [--repeats 3]

Per op, forward + backward: the Function against today's torch route under autograd (the yardstick, measured in the same
run); for the warp with and without right.requires_grad.  Per module (Refinement(8, 8, stage_id=3), SoftAttention(12,
8).fuse, DynamicUpsampling(8, 3)): eager and as one GraphedStep under hip_grad(), against the same module on the parent's
routing (hip_grad() on, the tail Functions off).  Per kernel: `--calls` calls per graph replay, time against the
algorithmic bytes at 8 TB/s.  One process, alternating blocks, `--repeats` blocks of `--calls` calls after a warm-up; medians."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12

from bench_conv2d_grad import alternate, stats, timed  # noqa: E402


@contextlib.contextmanager
def parent_routing():
    """hip_grad() as before the tail Functions: model.tail_grad_gate answers no."""
    from decnet_amd import model
    real, model.tail_grad_gate = model.tail_grad_gate, lambda *ts: False
    try:
        yield
    finally:
        model.tail_grad_gate = real


def op_rows(dev, B, C, H, W, calls, repeats, warmup):
    import torch
    import torch.nn.functional as F
    import decnet_amd
    from decnet_amd import model, ops2d
    g = torch.Generator().manual_seed(21)
    h, w = H // 3, W // 3
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    rows = {}

    def legs(make, leaves, gout):
        def step(hip):
            for t in leaves:
                t.grad = None
            make(hip).backward(gout)
        return alternate({"hip": lambda: step(True), "torch": lambda: step(False)}, calls, repeats, warmup)

    def add(name, t):
        t["torch_over_hip"] = t["torch"]["median"] / t["hip"]["median"]
        rows[name] = t
        print(json.dumps({name: t}), flush=True)

    # warp
    right, disp = rn(B, C, H, W), (torch.rand(B, H, W, generator=g) * 64).to(dev).requires_grad_()
    gout = rn(B, C, H, W)

    def warp(hip):
        with decnet_amd.hip_grad(hip):
            return model.warp_by_disparity(right, disp)
    add("warp_right_frozen", legs(warp, [disp], gout))
    right.requires_grad_()
    add("warp_right_grad", legs(warp, [disp, right], gout))
    right.requires_grad_(False)
    # unfold3_cat / fold3
    fea, cd = rn(B, C, H, W).requires_grad_(), rn(B, h, w).requires_grad_()
    gu = rn(B, 9 * C + 1, h, w)
    add("unfold3_cat", legs(lambda hip: decnet_amd.Unfold3CatFunction.apply(fea, cd) if hip else
                            torch.cat((cd.unsqueeze(1), F.unfold(fea, 3, stride=3).view(B, -1, h, w)), 1), [fea, cd], gu))
    # dynamic_upsample3
    logits = rn(B, 81, h, w).requires_grad_()
    pad = torch.nn.ReplicationPad2d(1)

    def ups(hip):
        if hip:
            return decnet_amd.DynamicUpsample3Function.apply(logits, cd)
        wts = F.softmax(logits.view(B, 9, 9, h * w), 2)
        nb = F.unfold(pad(cd.unsqueeze(1)), 3).unsqueeze(1)
        return (F.pixel_shuffle((nb * wts).sum(2).view(B, 9, h, w), 3) * 3).squeeze(1)
    gup = rn(B, H, W)
    add("dynamic_upsample3", legs(ups, [logits, cd], gup))
    # sigmoid + blend
    o, a, b = rn(B, H, W).requires_grad_(), rn(B, H, W).requires_grad_(), rn(B, H, W).requires_grad_()

    def blend(hip):
        if hip:
            return decnet_amd.SigmoidBlendFunction.apply(o, a, b)
        s = torch.sigmoid(o)
        return a * (1 - s) + s * b
    add("sigmoid_blend", legs(blend, [o, a, b], gup))
    # the kernels alone
    kernels = {}
    with torch.no_grad():
        rd, dd, od, ad, bd, ld, cdd = (t.detach() for t in (right, disp, o, a, b, logits, cd))
        for name, fn, nbytes in (
                ("warp_backward", lambda: ops2d.warp_disparity_backward(rd, dd, gout), 4.0 * B * H * W * (3 * C + 2)),
                ("warp_backward_disp_only", lambda: ops2d.warp_disparity_backward(rd, dd, gout, False, True),
                 4.0 * B * H * W * (2 * C + 2)),
                ("dynamic_upsample3_backward", lambda: ops2d.dynamic_upsample3_backward(ld, cdd, gup),
                 4.0 * B * h * w * (2 * 81 + 9 + 2)),
                ("fold3", lambda: ops2d.fold3(gu), 8.0 * B * C * 9 * h * w),
                ("sigmoid_blend_backward", lambda: ops2d.sigmoid_blend_backward(od, ad, bd, gup), 28.0 * B * H * W)):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            us = stats([timed(graph.replay, 1) / calls * 1e3 for _ in range(repeats)])
            kernels[name] = {"us_per_call": us, "bytes": nbytes, "share_of_hbm_roof_at_median": nbytes / HBM * 1e6 / us["median"]}
            print(json.dumps({name: kernels[name]}), flush=True)
            del graph
    return rows, kernels


def module_rows(dev, B, H, W, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    import _model_cases as MC
    from decnet_amd.model import DynamicUpsampling, Refinement, SoftAttention
    g = torch.Generator().manual_seed(22)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g).to(dev)  # noqa: E731
    out = {}
    for name in ("refinement", "attention", "upsampling"):
        if name == "refinement":
            m = MC.seeded(lambda: Refinement(8, 8, stage_id=3), 1).to(dev)
            left, right, disp = rn(B, 8, H, W), rn(B, 8, H, W).requires_grad_(), (ru(B, H, W) * 4).requires_grad_()
            run, wrt = (lambda m=m, left=left, right=right, disp=disp: m(left, right, disp)[0]), [disp, right]
        elif name == "attention":
            m = MC.seeded(lambda: SoftAttention(12, 8), 2).to(dev)
            fea, dense, sparse = rn(B, 8, H, W), (ru(B, H, W) * 4).requires_grad_(), (ru(B, H, W) * 4).requires_grad_()
            mask, var = (ru(B, H, W) < 0.5).float(), ru(B, H, W)
            run = lambda m=m, fea=fea, dense=dense, sparse=sparse, mask=mask, var=var: m.fuse(fea, dense, sparse, mask, var)  # noqa: E731
            wrt = [dense, sparse]
        else:
            m = MC.seeded(lambda: DynamicUpsampling(8, 3), 3).to(dev)
            cd, fea = (ru(B, H // 3, W // 3) * 20).requires_grad_(), rn(B, 8, H, W).requires_grad_()
            run, wrt = (lambda m=m, cd=cd, fea=fea: m(cd, fea)), [cd, fea]
        r = rn(B, H, W)
        leaves = wrt + list(m.parameters())

        def step(run=run, r=r):
            with decnet_amd.hip_grad():
                o = run()
            (o * r).sum().backward()

        def eager(parent, leaves=leaves, step=step):
            for t in leaves:
                t.grad = None
            with (parent_routing() if parent else contextlib.nullcontext()):
                step()
        graphed = GraphedStep(step, grads_of=leaves)
        with parent_routing():
            graphed_parent = GraphedStep(step, grads_of=leaves)
        out[name] = alternate({"tail_eager": lambda: eager(False), "parent_eager": lambda: eager(True), "tail_graph": graphed,
                               "parent_graph": graphed_parent}, calls, repeats, warmup)
        print(json.dumps({name: out[name]}), flush=True)
        del graphed, graphed_parent
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_grad.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=4, default=(4, 8, 540, 972), metavar=("B", "C", "H", "W"))
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_grad.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, C, H, W = a.shape
    ops, kernels = op_rows(dev, B, C, H, W, a.calls, a.repeats, a.warmup)
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "shape": [B, C, H, W],
              "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup, "hbm_B_per_s": HBM,
              "ops_ms_forward_backward": ops, "kernels": kernels,
              "modules_ms_forward_backward": module_rows(dev, B, H, W, a.calls, a.repeats, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
