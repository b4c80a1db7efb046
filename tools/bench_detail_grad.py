#!/usr/bin/env python
"""Timing of the detail maps and soft masks under hip_grad() (csrc/detail_grad.hip, decnet_amd/tail_grad.py) at config 5's
per-GPU batch: B = 4 at the three levels 540 x 972 (C 8), 180 x 324 (C 24) and 60 x 108 (C 72).

    python tools/bench_detail_grad.py [--out profiles/detail_grad.json] [--calls 50] [--repeats 3]

Per level and BatchNorm mode, forward + backward of (prob * r).sum():
  hip    GenerateSparseMask(C, 3).detail(cur, pre, thold, want_bits=True) under hip_grad()
  torch  the same module under hip_grad() (the units on the same routes) with the tail in torch ops: sigmoid(gen(cur, pre))
         and the reference's threshold statements (clone, two masked fills, under no_grad) -- the yardstick
each eager and as one GraphedStep replay.  SoftAttention(C + 4, 8).fuse(want_soft=True) against the same units followed by
torch's sigmoid and blend, in the same way.  The entries of csrc/detail_grad.hip and decnet_detail_mask alone at the first
level (`kernels`; `--kernels-only` stops after them): `--calls` calls per graph replay, time against the algorithmic bytes
at 8 TB/s, and `alone_us_per_call`, the same calls eager -- the ops2d wrapper and the launch, bound by the host where the
kernel is shorter than they are.  One process, alternating blocks, `--repeats` blocks of `--calls` calls after
a warm-up; medians.  model._detail_slower, the exclusion these numbers decide, is switched off for the run: the hip leg is
the Functions at every level."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12
LEVELS = ((540, 972, 8), (180, 324, 24), (60, 108, 72))
THOLD = 0.5

from bench_conv2d_grad import alternate, stats, timed  # noqa: E402


def _ratios(t):
    t["torch_over_hip_eager"] = t["torch_eager"]["median"] / t["hip_eager"]["median"]
    t["torch_over_hip_graph"] = t["torch_graph"]["median"] / t["hip_graph"]["median"]
    return t


def _four_legs(hip_step, torch_step, leaves, calls, repeats, warmup):
    """Both steps eager and as GraphedStep replays, alternating."""
    import torch
    from decnet_amd.graphs import GraphedStep

    def eager(step):
        for t in leaves:
            t.grad = None
        step()
    g_hip = GraphedStep(hip_step, grads_of=leaves)
    g_torch = GraphedStep(torch_step, grads_of=leaves)
    out = _ratios(alternate({"hip_eager": lambda: eager(hip_step), "torch_eager": lambda: eager(torch_step),
                             "hip_graph": g_hip, "torch_graph": g_torch}, calls, repeats, warmup))
    del g_hip, g_torch
    torch.cuda.empty_cache()
    return out


def detail_rows(dev, B, calls, repeats, warmup):
    import torch
    import decnet_amd
    import _model_cases as MC
    from decnet_amd.model import GenerateSparseMask
    g = torch.Generator().manual_seed(31)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    rows = {}
    for H, W, C in LEVELS:
        cur, pre, r = rn(B, C, H, W).requires_grad_(), rn(B, 3 * C, H // 3, W // 3).requires_grad_(), rn(B, H, W)
        for mode in ("train", "eval"):
            gen = MC.seeded(lambda: GenerateSparseMask(C, 3), 5).to(dev)
            gen = gen.train() if mode == "train" else gen.eval()
            leaves = [cur, pre] + list(gen.parameters())

            def hip_step(gen=gen, cur=cur, pre=pre, r=r):
                with decnet_amd.hip_grad():
                    prob, mask, bits = gen.detail(cur, pre, THOLD, want_bits=True)
                (prob * r).sum().backward()

            def torch_step(gen=gen, cur=cur, pre=pre, r=r):
                with decnet_amd.hip_grad():
                    prob = torch.sigmoid(gen(cur, pre))
                with torch.no_grad():                       # SparseDenseNetRefinementMask.py:164-170
                    mask = torch.clone(prob)
                    mask[mask <= THOLD] = 0.
                    mask[mask > THOLD] = 1.
                (prob * r).sum().backward()
            key = "%dx%d_C%d_%s" % (H, W, C, mode)
            rows[key] = _four_legs(hip_step, torch_step, leaves, calls, repeats, warmup)
            print(json.dumps({key: rows[key]}), flush=True)
    return rows


def fuse_rows(dev, B, calls, repeats, warmup):
    import torch
    import decnet_amd
    import _model_cases as MC
    from decnet_amd.model import SoftAttention
    g = torch.Generator().manual_seed(32)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g).to(dev)  # noqa: E731
    rows = {}
    for H, W, C in LEVELS:
        fea, dense, sparse = rn(B, C, H, W), (ru(B, H, W) * 4).requires_grad_(), (ru(B, H, W) * 4).requires_grad_()
        mask, var, r1, r2 = (ru(B, H, W) < 0.5).float(), ru(B, H, W), rn(B, H, W), rn(B, H, W)
        for mode in ("train", "eval"):
            att = MC.seeded(lambda: SoftAttention(C + 4, 8), 6).to(dev)
            att = att.train() if mode == "train" else att.eval()
            leaves = [dense, sparse] + list(att.parameters())
            nodes = []

            def hip_step(att=att, nodes=nodes):
                with decnet_amd.hip_grad():
                    fused, soft = att.fuse(fea, dense, sparse, mask, var, want_soft=True)
                if not nodes:
                    nodes.append(type(fused.grad_fn).__name__)
                (fused * r1 + soft * r2).sum().backward()

            def torch_step(att=att):
                with decnet_amd.hip_grad():
                    t = (fea, dense.unsqueeze(1), sparse.unsqueeze(1), mask.unsqueeze(1), -var.unsqueeze(1))
                    for u in att.conv:                      # the same units on the same routes
                        t = u(t)
                    soft = torch.sigmoid(t).squeeze(1)
                    fused = dense * (1 - soft) + soft * sparse
                (fused * r1 + soft * r2).sum().backward()
            key = "%dx%d_C%d_%s" % (H, W, C, mode)
            rows[key] = _four_legs(hip_step, torch_step, leaves, calls, repeats, warmup)
            rows[key]["node_behind_fused"] = nodes[0]
            print(json.dumps({key: rows[key]}), flush=True)
    return rows


def kernel_rows(dev, B, calls, repeats):
    import torch
    from decnet_amd import ops2d
    H, W, _ = LEVELS[0]
    g = torch.Generator().manual_seed(33)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    a3, b3, g3 = rn(B, 3, H, W), rn(B, 3, H, W), rn(B, 3, H, W)
    z, o, a, b, g1, g2 = (rn(B, H, W) for _ in range(6))
    n3, n1 = float(a3.numel()), float(z.numel())
    params = ops2d.detail_mask_params([0.01 * ((i * 37) % 11 - 5) for i in range(81)] + [1.0] * 3 + [0.0] * 3 + [0.3] * 3 +
                                      [1.0, -0.5])
    kernels = {}
    with torch.no_grad():
        for name, fn, nbytes in (
                ("sqdiff", lambda: ops2d.sqdiff(a3, b3), 12.0 * n3),
                ("sqdiff_backward", lambda: ops2d.sqdiff_backward(a3, b3, g3), 20.0 * n3),
                ("detail_tail", lambda: ops2d.detail_tail(z, THOLD, True, True, True), (12.0 + 1.0 / 8) * n1),
                ("detail_tail_backward", lambda: ops2d.detail_tail_backward(z, g1), 12.0 * n1),
                ("sigmoid_blend_soft", lambda: ops2d.sigmoid_blend_soft(o, a, b), 20.0 * n1),
                ("sigmoid_blend_soft_backward", lambda: ops2d.sigmoid_blend_soft_backward(o, a, b, g1, g2), 32.0 * n1),
                ("sigmoid_blend_soft_backward_gsoft_only",
                 lambda: ops2d.sigmoid_blend_soft_backward(o, a, b, None, g2, False, False), 12.0 * n1),
                ("sigmoid_blend", lambda: ops2d.sigmoid_blend(o, a, b), 16.0 * n1),
                ("sigmoid_blend_backward", lambda: ops2d.sigmoid_blend_backward(o, a, b, g1), 28.0 * n1),
                ("detail_mask", lambda: ops2d.detail_mask(a3, b3, params, THOLD, True), (8.0 * n3 + (4.0 + 1.0 / 8) * n1))):
            for _ in range(10):
                fn()
            alone = stats([timed(fn, calls) * 1e3 for _ in range(repeats)])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            us = stats([timed(graph.replay, 1) / calls * 1e3 for _ in range(repeats)])
            kernels[name] = {"us_per_call": us, "alone_us_per_call": alone, "bytes": nbytes,
                             "share_of_hbm_roof_at_median": nbytes / HBM * 1e6 / us["median"]}
            print(json.dumps({name: kernels[name]}), flush=True)
            del graph
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detail_grad.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_detail_grad.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    from decnet_amd import model
    model._detail_slower = lambda n: False
    report = {"device": torch.cuda.get_device_name(0), "version": decnet_amd.version(), "batch": a.batch,
              "levels_H_W_C": [list(v) for v in LEVELS], "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup,
              "hbm_B_per_s": HBM, "kernels": kernel_rows(dev, a.batch, a.calls, a.repeats)}
    if not a.kernels_only:
        report["detail_ms_forward_backward"] = detail_rows(dev, a.batch, a.calls, a.repeats, a.warmup)
        report["fuse_ms_forward_backward"] = fuse_rows(dev, a.batch, a.calls, a.repeats, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
