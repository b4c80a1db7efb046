#!/usr/bin/env python
"""Image-in / disparity-out throughput: what a user of the package gets, against the benchmark's ceiling.

    python tools/bench_engine.py [--tiny] [--blocks 3] [--out profiles/engine_throughput.json]

On seeded in-memory uint8 pairs (BASELINE config 2: 8 x 960 x 540 per batch, max_disp 216, the network of bench.py's e2e
leg) three paths are timed in ONE process, alternating block by block (>= 3 blocks each, after a warm-up of each), every
block ending in a device synchronise:

  (a) eager    the calls of decnet_amd.eval.test per batch: pad_top_left / 255 and normalise of every view on the host,
               stack, .to(device), synchronize, the eager forward, synchronize, disparity_to_uint16 per sample
               (the loader's placeholder masks and padded ground truth are left out: they only add host time);
  (b) engine   decnet_amd.StereoEngine: submit / results per batch, one flush at the end of the block;
  (c) ceiling  replays of the captured forward on inputs that are already resident and normalised (bench.py's e2e leg).

Also: the three image-boundary kernels alone, timed between device events, with their bytes / time.  One JSON line on
stdout; the same object is written to --out (default profiles/engine_throughput.json; nothing with --tiny).
--tiny (base_channels 2, 2 x 54 x 108 per batch, 4 batches per block) runs in seconds: tests/test_engine_gpu.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decnet_amd import StereoEngine, imageio, loader  # noqa: E402
from decnet_amd.demo import disparity_to_uint16  # noqa: E402
from decnet_amd.model import get_model  # noqa: E402


def make_model(dev, base_channels, max_disp):
    torch.manual_seed(17)                     # bench.py's e2e_model: demo.sh hyper-parameters, thold 0.5 -> mixed masks
    return get_model(name="sparsedensenetrefinementmask", max_disp=max_disp, base_channels=base_channels,
                     cost_func="cor", grad_method="detach", num_stage=4, down_scale=3, step=[-1., 1., 1., 1.],
                     samp_num=[-1., 12., 10., 6.], sample_spa_size_list=[-1, 3, 5, 7], down_func_name="bicubic",
                     weights=[1., 1., 1., 1.], if_overmask=False, skip_stage_id=4, use_detail=True,
                     thold=0.5).to(dev).eval()


def host_batch(views):
    """_Base._item + eval.collate for one view of a batch: pad, / 255, normalise, stack."""
    return torch.stack([loader.normalise(loader.pad_top_left(v.astype(np.float32)) / 255) for v in views])


def eager_batch(model, lefts, rights, dev):
    h, w = lefts[0].shape[:2]
    left, right = host_batch(lefts), host_batch(rights)
    with torch.no_grad():
        left, right = left.to(dev), right.to(dev)
        torch.cuda.synchronize()
        pred = model(left, right)[-1]
        torch.cuda.synchronize()
        return [disparity_to_uint16(pred[j:j + 1], h, w) for j in range(len(lefts))]


def time_kernel(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def kernel_times(dev, B, h, w, iters):
    H, W = imageio.padded_size(h, w)
    rng = np.random.RandomState(3)
    img = torch.from_numpy(rng.randint(0, 256, (B, h, w, 3)).astype(np.uint8)).to(dev)
    table = imageio.normalise_table().to(dev)
    out = torch.empty((B, 3, H, W), device=dev)
    pred = torch.rand((B, H, W), device=dev) * 200
    gt = torch.rand((B, h, w), device=dev) * 250
    u16 = torch.empty((B, h, w), dtype=torch.int16, device=dev)
    part = torch.empty((B, h, 3), device=dev)
    res = {}
    for name, fn, nbytes in (
            ("preprocess_u8", lambda: imageio.preprocess_u8(img, table, out), B * h * w * 3 + B * 3 * H * W * 4),
            ("disparity_to_u16", lambda: imageio.disparity_to_u16(pred, u16), B * h * w * (4 + 2)),
            ("disparity_metrics", lambda: imageio.disparity_metrics(pred, gt, 216, part), B * h * w * 8 + B * h * 12)):
        t = time_kernel(fn, iters)
        res[name] = {"us": 1e6 * t, "bytes": nbytes, "GB_per_s": nbytes / t * 1e-9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--batches", type=int, default=0, help="batches per engine / ceiling block (default 24; --tiny 4)")
    ap.add_argument("--eager-batches", type=int, default=0, help="batches per eager block (default 3; --tiny 4)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be >= 3")
    dev = torch.device("cuda:0")
    if args.tiny:
        B, h, w, D, bc, nb, nb_eager = 2, 54, 108, 54, 2, 4, 4
    else:
        B, h, w, D, bc, nb, nb_eager = 8, 540, 960, 216, 8, 24, 3
    nb, nb_eager = args.batches or nb, args.eager_batches or nb_eager
    out_path = args.out or (None if args.tiny else os.path.join(ROOT, "profiles", "engine_throughput.json"))
    H, W = imageio.padded_size(h, w)
    rng = np.random.RandomState(17)
    pool = [([rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)],
             [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)]) for _ in range(4)]
    model = make_model(dev, bc, D)
    engine = StereoEngine(model, batch_size=B)

    # (c): the captured forward on resident, already normalised inputs
    with torch.no_grad():
        left, right = host_batch(pool[0][0]).to(dev), host_batch(pool[0][1]).to(dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(left, right)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            model(left, right)

    def block_eager():
        for i in range(nb_eager):
            eager_batch(model, *pool[i % len(pool)], dev)
        return nb_eager

    def block_engine():
        for i in range(nb):
            engine.submit(*pool[i % len(pool)])
            engine.results()
        engine.flush()
        return nb

    def block_ceiling():
        for _ in range(nb):
            graph.replay()
        return nb

    legs = (("eager", block_eager), ("engine", block_engine), ("ceiling", block_ceiling))
    # warm-up of every leg (first-call work: lazy init, the engine's capture), and the engine checked against (a) once
    want = eager_batch(model, *pool[1], dev)
    engine.submit(*pool[1])
    got = engine.flush()[0][1]
    equal = all(np.array_equal(a, b) for a, b in zip(want, got))
    for _, fn in legs:
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in legs}
    for _ in range(args.blocks):
        for name, fn in legs:                               # alternating: drift of the box hits every leg alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            rates[name].append(n * B / (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    res = {"config": "tiny: 2 x 54 x 108, max_disp 54, base_channels 2" if args.tiny else
           "config 2: 8 x 960 x 540 (padded %d x %d), max_disp 216, base_channels 8" % (W, H),
           "batch": B, "blocks": args.blocks, "batches_per_block": {"eager": nb_eager, "engine": nb, "ceiling": nb},
           "eager_pairs_per_s": med["eager"], "engine_pairs_per_s": med["engine"], "ceiling_pairs_per_s": med["ceiling"],
           "engine_over_eager": med["engine"] / med["eager"], "engine_over_ceiling": med["engine"] / med["ceiling"],
           "block_pairs_per_s": rates, "engine_equals_eager": bool(equal),
           "kernels": kernel_times(dev, B, h, w, 20 if args.tiny else 200)}
    line = json.dumps(res)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
