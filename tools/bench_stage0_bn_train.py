#!/usr/bin/env python
"""Timing of stage 0 in .train() mode under decnet_amd.hip_grad() (Conv3dFunction, then BatchNorm3dActFunction over
the Columns layout of csrc/batchnorm.hip) at the stage-0 volumes of config 5 (B = 4, C = 216, 20 x 36, D = 8: 23 040
voxels) and config 2 (B = 8: 46 080 voxels).

    python tools/bench_stage0_bn_train.py [--out profiles/stage0_bn_train.json] [--calls 50] [--repeats 3]
    python tools/bench_stage0_bn_train.py --parity [--out profiles/stage0_bn_train_parity.json]

Per size, forward + backward of one 216 -> 216 unit and of the 216 -> 1 unit, every parameter and the input taking a gradient:
    hip    Conv3dFunction (scale 1, shift 0, no ReLU), then BatchNorm3dActFunction on the statistics of the batch
    lib    stage0_grad.unit_library_train: torch's conv3d -> batch_norm(training) -> ReLU under autograd
in alternating blocks in one process, `--repeats` blocks of `--calls` calls under device events after a warm-up; medians.
Each leg is timed eager and as one GraphedStep replay.  The library's eager time in the same run is the yardstick: a shape
with lib_over_hip <= 1 belongs into stage0._conv3d_bn_train_slower.
The two new entries alone, against their bytes at 8 TB/s: the forward reads z twice and writes y (12 B per element), the
backward reads z and gy twice and writes gz (20 B).  Then CostRegNetNoDown.stage0 forward + backward in .train() mode on
both arms.

--parity: no timing; the gradient parity of tests/test_stage0_bn_train_gpu.py (`parity_ratios`) as numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_conv2d_grad import alternate, timed, stats  # noqa: E402
from bench_stage0_grad import with_graphs  # noqa: E402

HBM = 8.0e12
C, H, W, D = 216, 20, 36, 8
SIZES = {"config5": 4, "config2": 8}
EPS, MOM = 1e-5, 0.1


def unit_row(dev, B, co, relu, calls, repeats, warmup):
    import torch
    from decnet_amd import BatchNorm3dActFunction, Conv3dFunction, ops2d, stage0, stage0_grad
    g = torch.Generator().manual_seed(11 + co)
    dims = (B, D, H, W)
    x = torch.randn(*dims, C, generator=g).to(dev).requires_grad_()
    w = (torch.randn(co, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(dev).requires_grad_()
    bn = torch.nn.BatchNorm3d(co, eps=EPS, momentum=MOM).to(dev).train()
    gy = torch.randn(*dims, co, generator=g).to(dev)
    variant = stage0.WINO_VARIANT.get(stage0.conv_algo(D))
    packed = stage0_grad.unit_operands(w.detach(), variant, last=(co == 1))
    ones, zeros = torch.ones(co, device=dev), torch.zeros(co, device=dev)
    leaves = [x, w, bn.weight, bn.bias]

    def hip():
        z = Conv3dFunction.apply(packed, False, w, ones, zeros, x)
        BatchNorm3dActFunction.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, EPS, MOM, relu).backward(gy)

    def lib():
        stage0_grad.unit_library_train(x, w, bn, relu).backward(gy)

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
    with torch.no_grad():                                               # the two entries alone
        z = torch.randn(*dims, co, generator=g).to(dev)
        gam, bet = bn.weight.detach(), bn.bias.detach()
        rm, rv = bn.running_mean, bn.running_var
        _, st = ops2d.bn_train_cl_forward(z, gam, bet, EPS, MOM, rm, rv, relu)
        fwd = stats([timed(lambda: ops2d.bn_train_cl_forward(z, gam, bet, EPS, MOM, rm, rv, relu), calls)
                     for _ in range(repeats)])["median"]
        bwd = stats([timed(lambda: ops2d.bn_train_cl_backward(z, gy, gam, bet, st, relu), calls) for _ in range(repeats)])["median"]
    n = float(z.numel())
    row["entries"] = {"elements": int(n), "workspace_floats": int(ops2d.size("bn_train_cl_workspace_floats", B * D * H * W, co)),
                      "forward": {"ms": fwd, "bytes": 12 * n, "bound_ms_hbm": 12 * n / HBM * 1e3,
                                  "share_of_hbm": 12 * n / HBM * 1e3 / fwd},
                      "backward": {"ms": bwd, "bytes": 20 * n, "bound_ms_hbm": 20 * n / HBM * 1e3,
                                   "share_of_hbm": 20 * n / HBM * 1e3 / bwd}}
    return row


def stage0_row(dev, B, calls, repeats, warmup):
    import torch
    import decnet_amd
    from decnet_amd import stage0
    import _model_cases as MC
    mod = MC.seeded(lambda: decnet_amd.CostRegNetNoDown(C, 2 * C, "cor"), 5).to(dev).train()
    g = torch.Generator().manual_seed(12)
    L, R = (torch.relu(torch.randn(B, C, H, W, generator=g)).to(dev).requires_grad_() for _ in range(2))
    r, r2 = torch.randn(B, H, W, generator=g).to(dev), torch.randn(B, D, H, W, generator=g).to(dev)
    leaves = [L, R] + list(mod.parameters())
    slower = stage0._conv3d_bn_train_slower

    def step(library):
        stage0._conv3d_bn_train_slower = (lambda ci, co, v: True) if library else slower
        try:
            with decnet_amd.hip_grad():
                pred, reg = mod.stage0(L, R, D, return_reg=True)
            ((pred * r).sum() + (reg * r2).sum()).backward()
        finally:
            stage0._conv3d_bn_train_slower = slower

    def eager(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn()
        return run
    legs = {"hip": eager(lambda: step(False)), "lib": eager(lambda: step(True))}
    note = with_graphs(legs, {"hip": lambda: step(False), "lib": lambda: step(True)}, leaves)
    row = {"B": B, "voxels": B * D * H * W, "mode": "train",
           "routed_to_library": [bool(slower(C, co, B * D * H * W)) for co in (C, 1)],
           "ms_forward_backward": alternate(legs, calls, repeats, warmup)}
    t = row["ms_forward_backward"]
    row["lib_over_hip"] = t["lib"]["median"] / t["hip"]["median"]
    if note is not None:
        row["graph_note"] = note
    return row


def parity(out):
    import torch
    import decnet_amd
    import test_stage0_bn_train_gpu as T
    cases = {}
    for name in sorted(T.SG.MODULE_CASES):
        p = T.parity_ratios(name)
        cases[name] = {"tensors": p["tensors"], "flips": p["flips"], "buffers": p["buffers"], "eval_forward": p["eval_forward"]}
    worst = {name: max(c["tensors"].items(), key=lambda kv: kv[1]["ratio"]) for name, c in cases.items()}
    rep = {"what": "max|g_hip - g64|, max|g32 - g64|, the gate max(4 max|g32 - g64|, 2e-5 max(1, max|g64|)), ratio = hip_vs_f64 / "
                   "gate, per tensor of one train-mode step of CostRegNetNoDown.stage0 (the GPU's ReLU masks imposed on both "
                   "CPU runs); the imposed decisions that differ from float64's own; the buffers after 1 and 3 steps",
           "device": torch.cuda.get_device_name(0), "version": decnet_amd.version(),
           "worst_hip_over_gate": {n: {"tensor": k, "ratio": r["ratio"]} for n, (k, r) in worst.items()}, "cases": cases}
    with open(out, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rep["worst_hip_over_gate"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    a = ap.parse_args()
    import torch
    import decnet_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage0_bn_train.py measures on the GPU; there is none")
    name = "stage0_bn_train_parity.json" if a.parity else "stage0_bn_train.json"
    path = a.out or os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if a.parity:
        return parity(path)
    dev = torch.device("cuda:0")
    warm = torch.randn(4096, 4096, device=dev)                          # bring the clocks up before the first row
    for _ in range(100):
        warm @ warm
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "library": decnet_amd.version(), "calls": a.calls, "repeats": a.repeats,
           "hbm_bytes_per_s": HBM, "C": C, "plane": [H, W], "D": D, "sizes": {}}
    for name, B in SIZES.items():
        out["sizes"][name] = {
            "units": [unit_row(dev, B, C, True, a.calls, a.repeats, a.warmup),
                      unit_row(dev, B, 1, False, a.calls, a.repeats, a.warmup)],
            "stage0": stage0_row(dev, B, a.calls, a.repeats, a.warmup)}
        print(json.dumps({name: out["sizes"][name]}), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
