#!/usr/bin/env python
"""Timing of the multi-stage training loss (decnet_amd.Loss over csrc/loss.hip): forward + backward at config 5's four
levels, B = 4 (20 x 36, 60 x 108, 180 x 324, 540 x 972; max_disp 192, bicubic ground truth), against the same loss written
with torch ops on the GPU (tests/_loss_ref.py: boolean gathers, a host read-back each).

    python tools/bench_loss.py [--out profiles/loss_step.json] [--calls 200] [--repeats 3]

Legs, alternating, `--repeats` rounds of `--calls` calls each, device events around a round, medians reported:
    fused_eager     decnet_amd.Loss forward + tot_loss.backward(), issued call by call
    fused_graph     the same step as ONE HIP-graph replay (decnet_amd.graphs.GraphedStep)
    torch_eager     _loss_ref.uploss forward + backward under torch autograd, float32 (cannot be captured)
and, for the kernels alone, the forward entry (two launches) and the backward entry (one launch, five gradient planes) of
the 540 x 972 composite level as graph replays of `--calls` calls: microseconds per call and the rate of the bytes the
kernels move (forward 7 planes read = 28 B / pixel; backward 6 planes read, 5 written = 44 B / pixel).  The same buffers
are used by every call and fit the 256 MiB last-level cache, as in the image-boundary kernels' figures this is set beside."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B, H, W, SCALE, STAGES, MAX_DISP = 4, 540, 972, 3, 4, 192
WEIGHTS = [1.0, 1.0, 1.0, 1.0]


def make_inputs(dev, B=B, H=H, W=W):
    """gt with 30 % zeros and 1 % above max_disp; every prediction = the strided pick of gt at its level + noise of
    sigma 0.3 / 5 full-resolution pixels; left masks 20 % ones."""
    import torch
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(B, H, W, generator=g) * (MAX_DISP - 6) + 1
    high = torch.rand(B, H, W, generator=g) < 0.01
    gt[high] = MAX_DISP + 20.0
    gt[torch.rand(B, H, W, generator=g) < 0.3] = 0
    lists = dict(pred=[], dense=[], sparse=[], fusion=[], soft=[], left=[])
    for k in range(STAGES):
        ds = SCALE ** (STAGES - k - 1)
        base = gt[:, ds // 2::ds, ds // 2::ds] / ds

        def noisy():
            sigma = torch.where(torch.rand(base.shape, generator=g) < 0.5, 0.3, 5.0)
            return (base + sigma * torch.randn(base.shape, generator=g) / ds).to(dev).requires_grad_()
        lists["pred"].append(noisy())
        if k:
            for n in ("dense", "sparse", "fusion"):
                lists[n].append(noisy())
            lists["soft"].append(torch.rand(base.shape, generator=g).to(dev).requires_grad_())
            lists["left"].append((torch.rand(base.shape, generator=g) < 0.2).float().to(dev))
    return gt.to(dev), lists


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


def kernel_rates(gt, lists, calls, repeats):
    """The two C entries at the finest level, `calls` calls per graph replay."""
    import torch
    from decnet_amd import ops
    with torch.no_grad():
        planes = [lists[n][-1].detach() for n in ("pred", "dense", "sparse", "fusion", "soft", "left")]
        Bn, Hn, Wn = gt.shape
        row_sums = torch.empty(Bn * Hn, 8, dtype=torch.float64, device=gt.device)
        sums = torch.empty(8, dtype=torch.float64, device=gt.device)
        terms = torch.empty(5, device=gt.device)
        gterms = torch.ones(5, device=gt.device)
        grads = [torch.empty_like(gt) for _ in range(5)]

        def fwd():
            ops.stage_loss_forward(*planes, gt, float(MAX_DISP), 1.0, 0, row_sums, sums, terms)

        def bwd():
            ops.stage_loss_backward(*planes, gt, float(MAX_DISP), 1.0, 0, sums, gterms, *grads)
        out = {}
        pixels = Bn * Hn * Wn
        for name, fn, bpp in (("forward", fwd, 28), ("backward", bwd, 44)):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            us = stats([timed(graph.replay, 1) / calls * 1e3 for _ in range(repeats)])
            out[name] = {"us_per_call": us, "bytes_per_pixel": bpp, "bytes": pixels * bpp,
                         "TB_per_s_at_median": pixels * bpp / (us["median"] * 1e-6) / 1e12}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_step.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import decnet_amd
    from decnet_amd.graphs import GraphedStep
    import _loss_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    gt, lists = make_inputs(dev)
    leaves = [t for n in ("pred", "dense", "sparse", "fusion", "soft") for t in lists[n]]
    loss = decnet_amd.Loss("multi_stage_regression_uploss")
    kw = dict(pred_list=lists["pred"], fusion_list=lists["fusion"], dense_list=lists["dense"], sparse_list=lists["sparse"],
              left_mask_list=lists["left"], gt=gt, weights=WEIGHTS, num_stage=STAGES, down_func_name="bicubic",
              down_scale=SCALE, max_disp=MAX_DISP, sparse_mask_list=lists["soft"])

    def fused():
        tot = loss(**kw)[2]
        tot.backward()
        return tot.detach()

    def composed():
        tot = R.uploss(kw["pred_list"], kw["fusion_list"], kw["dense_list"], kw["sparse_list"], kw["left_mask_list"], gt,
                       WEIGHTS, STAGES, "bicubic", SCALE, MAX_DISP, kw["sparse_mask_list"])[1]
        tot.backward()
        return tot.detach()

    def eager(fn):
        def run():
            for t in leaves:
                t.grad = None
            return fn()
        return run
    # the two implementations agree before anything is timed
    t_torch = float(eager(composed)())
    g_torch = [t.grad.clone() for t in lists["pred"]]
    t_fused = float(eager(fused)())
    g_err = max(float((t.grad - g).abs().max() / g.abs().max()) for t, g in zip(lists["pred"], g_torch))
    graphed = GraphedStep(fused, grads_of=leaves)
    legs = {"fused_eager": eager(fused), "fused_graph": graphed, "torch_eager": eager(composed)}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            ms[name].append(timed(fn, a.calls))
    tab = {k: stats(v) for k, v in ms.items()}
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "unit": "ms per forward + backward",
              "shape": {"B": B, "levels": [[H // SCALE ** k, W // SCALE ** k] for k in range(STAGES - 1, -1, -1)],
                        "max_disp": MAX_DISP, "down_func_name": "bicubic"},
              "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup, "ms": tab, "runs": ms,
              "torch_eager_over_fused_eager": tab["torch_eager"]["median"] / tab["fused_eager"]["median"],
              "torch_eager_over_fused_graph": tab["torch_eager"]["median"] / tab["fused_graph"]["median"],
              "agreement": {"tot_loss_fused": t_fused, "tot_loss_torch": t_torch,
                            "max_relative_pred_gradient_difference": g_err},
              "kernels_540x972": kernel_rates(gt, lists, a.calls, a.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: report[k] for k in ("ms", "torch_eager_over_fused_eager", "torch_eager_over_fused_graph",
                                             "agreement", "kernels_540x972")}, indent=1))


if __name__ == "__main__":
    main()
