"""decnet_amd.StereoEngine on the GPU: its uint16 maps equal, exactly, what the eager forward on the same
host-preprocessed batch gives through demo.disparity_to_uint16 -- full and short batches, alternating shapes with and
without room for both buckets, after a weight change + reset(); `demo --pipeline 1` and `eval --pipeline 1` against the
default paths; tools/bench_engine.py --tiny.  Every model has base_channels 2.  -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w), max_disp: 40 x 100 pads to 54 x 108; 54 x 81 needs no padding
CASES = {"padded": ((40, 100), 54), "exact": ((54, 81), 216)}


@pytest.fixture(scope="module")
def model():
    from decnet_amd import demo
    torch.manual_seed(5)
    args = demo.build_parser().parse_args(["--base_channels", "2", "--thold", "0.5"])
    return demo.build_model(args, torch.device("cuda:0"))


def _pairs(case, n, seed):
    (h, w), _ = CASES[case]
    rng = np.random.RandomState(seed)
    return ([rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)],
            [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)])


def _eager(model, lefts, rights, max_disp, B=None):
    """The default path on the batch filled up to B with its last pair: host pad / normalise, eager forward, uint16."""
    from decnet_amd import loader
    from decnet_amd.demo import disparity_to_uint16
    n, (h, w) = len(lefts), lefts[0].shape[:2]
    idx = [min(i, n - 1) for i in range(B or n)]
    L, R = (torch.stack([loader.normalise(loader.pad_top_left(v[i].astype(np.float32)) / 255) for i in idx]).cuda()
            for v in (lefts, rights))
    saved = model.max_disp
    model.max_disp = max_disp
    try:
        with torch.no_grad():
            pred = model(L, R)[-1]
    finally:
        model.max_disp = saved
    return [disparity_to_uint16(pred[j:j + 1], h, w) for j in range(n)]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == np.uint16 and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_engine_equals_the_eager_forward_exactly(model, case, B):
    from decnet_amd import StereoEngine
    D = CASES[case][1]
    lefts, rights = _pairs(case, B, seed=B)
    want = _eager(model, lefts, rights, D)
    assert any(w.any() for w in want)
    torch.cuda.synchronize()
    eng = StereoEngine(model, batch_size=B)
    before = model.max_disp
    eng.submit(lefts, rights, max_disp=D, tag="t")
    assert model.max_disp == before                                   # set for the capture only
    (tag, got, metrics), = eng.flush()
    assert tag == "t" and metrics is None
    _same(got, want)
    eng.submit(lefts, rights, max_disp=D)                              # the same bucket again: a replay, the same maps
    _same(eng.flush()[0][1], want)
    assert len(eng._buckets) == 1


def test_a_short_batch_equals_the_eager_forward_on_the_filled_batch(model):
    from decnet_amd import StereoEngine
    lefts, rights = _pairs("padded", 2, seed=7)
    want = _eager(model, lefts, rights, 54, B=3)
    torch.cuda.synchronize()
    eng = StereoEngine(model, batch_size=3)
    eng.submit(lefts, rights, max_disp=54)
    _same(eng.flush()[0][1], want)


@pytest.mark.parametrize("max_buckets", [4, 1])
def test_alternating_shapes_come_back_in_order(model, max_buckets):
    """Five submissions alternating between two shapes; with max_buckets=1 every one of them captures again."""
    from decnet_amd import StereoEngine
    order = ["padded", "exact", "padded", "exact", "padded"]
    batches = [_pairs(c, 1, seed=20 + i) for i, c in enumerate(order)]
    want = [_eager(model, l, r, CASES[c][1]) for (l, r), c in zip(batches, order)]
    torch.cuda.synchronize()
    eng = StereoEngine(model, batch_size=1, max_buckets=max_buckets)
    got = []
    for i, ((l, r), c) in enumerate(zip(batches, order)):
        eng.submit(l, r, max_disp=CASES[c][1], tag=i)
        got += eng.results()
    got += eng.flush()
    assert [g[0] for g in got] == [0, 1, 2, 3, 4]
    for g, w in zip(got, want):
        _same(g[1], w)
    assert len(eng._buckets) == min(2, max_buckets)


def test_reset_after_a_weight_change(model):
    from decnet_amd import StereoEngine
    lefts, rights = _pairs("exact", 1, seed=31)
    eng = StereoEngine(model, batch_size=1)
    eng.submit(lefts, rights, max_disp=216)
    old = eng.flush()[0][1]
    p = next(model.feature_extractor.parameters())
    with torch.no_grad():
        p.add_(0.05 * torch.randn_like(p))
    try:
        eng.reset()
        assert not eng._buckets
        want = _eager(model, lefts, rights, 216)
        torch.cuda.synchronize()
        eng.submit(lefts, rights, max_disp=216)
        new = eng.flush()[0][1]
        _same(new, want)
        assert not np.array_equal(new[0], old[0])                     # the change is one the output sees
    finally:
        eng.reset()


def test_metrics_of_a_batch(model):
    """submit(gts=...): (epe, loss_3) over the real samples of a short batch, against test_loss_func on the same
    predictions; and the device-side record of sums_out."""
    from decnet_amd import StereoEngine, imageio, loader
    from decnet_amd.eval import test_loss_func
    (h, w), D = CASES["padded"]
    lefts, rights = _pairs("padded", 2, seed=41)
    rng = np.random.RandomState(42)
    gts = [(rng.rand(h, w).astype(np.float32) * 70 - 8) for _ in range(2)]
    eng = StereoEngine(model, batch_size=3)
    eng.submit(lefts, rights, max_disp=D, gts=gts)
    rec = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    eng.submit(lefts, rights, max_disp=D, gts=gts, sums_out=rec[1])
    (_, _, m0), (_, _, m1) = eng.flush()
    assert m1 is None and m0 is not None
    assert imageio.metrics_from_sums(rec[1].cpu().numpy()) == m0 and not rec[0].any()
    # the same predictions through the default formula: the eager forward on the filled batch, padded ground truth
    idx = [0, 1, 1]
    L, R = (torch.stack([loader.normalise(loader.pad_top_left(v[i].astype(np.float32)) / 255) for i in idx]).cuda()
            for v in (lefts, rights))
    saved, model.max_disp = model.max_disp, D
    try:
        with torch.no_grad():
            pred = model(L, R)[-1][:2]
    finally:
        model.max_disp = saved
    gt = torch.stack([torch.from_numpy(loader.pad_top_left(g)) for g in gts]).cuda()
    epe, l3 = test_loss_func(pred, gt, D)
    W = pred.shape[-1]
    print("engine epe %.9g loss_3 %.9g | test_loss_func epe %.9g loss_3 %.9g" % (m0[0], m0[1], float(epe), float(l3)))
    assert abs(m0[0] - float(epe)) <= 2 * (W - 1) * 2.0 ** -24 * m0[0]
    assert abs(m0[1] - float(l3)) <= 5e-5


def _demo_dir(tmp_path):
    """The two synthetic pairs of test_model_gpu.test_demo_counterpart_runs_on_a_directory."""
    from PIL import Image
    rng = np.random.RandomState(0)
    for name, (h, w) in (("a", (40, 100)), ("b", (54, 81))):
        d = tmp_path / "in" / name
        d.mkdir(parents=True)
        for f in ("im0.png", "im1.png"):
            Image.fromarray(rng.randint(0, 255, (h, w, 3)).astype(np.uint8)).save(str(d / f))
    (tmp_path / "in" / "b" / "calib.txt").write_text("ndisp=40\n")          # -> max_disp 54
    return str(tmp_path / "in")


def test_demo_pipeline_writes_the_same_pngs(tmp_path):
    from PIL import Image
    from decnet_amd import demo
    root = _demo_dir(tmp_path)
    out = {}
    for p in (0, 1):
        args = demo.build_parser().parse_args(["--root", root, "--save2where", str(tmp_path / ("out%d" % p)),
                                               "--base_channels", "2", "--max_disp", "216", "--thold", "0.5",
                                               "--pipeline", str(p)])
        demo.test(args)
        out[p] = {n: np.asarray(Image.open(str(tmp_path / ("out%d" % p) / (n + ".png")))) for n in ("a", "b")}
    for n, shape in (("a", (40, 100)), ("b", (54, 81))):
        assert out[1][n].shape == shape and out[1][n].dtype == np.uint16
        assert np.array_equal(out[0][n], out[1][n]), n
    assert out[0]["a"].any()


@pytest.mark.parametrize("batch_size", [3, 1])
def test_eval_pipeline_agrees_with_the_default_path(tmp_path, batch_size):
    """3 synthetic .npy samples, full batches (one of 3, three of 1: a batch of another size may run other library
    convolution algorithms, which is not what this compares).  loss_3 within 5e-5: the counts are exact, the default path
    rounds a ratio and a difference at magnitude 100 in fp32 (each <= 100 x 2^-24).  EPE within 2 (W - 1) 2^-24 relative:
    the kernel's per-row fp32 sums plus as much again for torch's own fp32 reduction."""
    from decnet_amd import eval as E
    rng = np.random.RandomState(11)
    h, w, D = 40, 100, 54
    (tmp_path / "test").mkdir()
    for i in range(3):
        img = rng.randint(0, 256, (h, w, 6)).astype(np.float32)
        gt = (rng.rand(h, w, 1) * 70 - 8).astype(np.float32)               # invalid on both sides of (0, 54)
        np.save(tmp_path / "test" / ("s%d.npy" % i), np.concatenate([img, gt], -1))
    flags = ["--dataset", "sceneflowmask", "--data_path", str(tmp_path), "--test_split", "test", "--base_channels", "2",
             "--thold", "0.5", "--max_disp", str(D), "--batch_size", str(batch_size), "--skip_stage_id", "4",
             "--is_eval", "1"]
    torch.manual_seed(5)
    model = E.build_model(E.build_parser().parse_args(flags), torch.device("cuda:0"))
    epe0, l30 = E.test(E.build_parser().parse_args(flags + ["--pipeline", "0"]), model=model)
    epe1, l31 = E.test(E.build_parser().parse_args(flags + ["--pipeline", "1"]), model=model)
    W = 108
    print("pipeline 0: epe %.9g loss_3 %.9g | pipeline 1: epe %.9g loss_3 %.9g | rel. epe diff %.3g (bound %.3g)"
          % (epe0, l30, epe1, l31, abs(epe0 - epe1) / epe1, 2 * (W - 1) * 2.0 ** -24))
    assert np.isfinite(epe1) and 0 < l31 <= 100
    assert abs(l30 - l31) <= 5e-5
    assert abs(epe0 - epe1) <= 2 * (W - 1) * 2.0 ** -24 * epe1


def test_eval_pipeline_submission_mode_writes_the_default_paths_pngs(tmp_path):
    from PIL import Image
    from decnet_amd import eval as E
    root = _demo_dir(tmp_path)
    out = {}
    torch.manual_seed(5)
    flags = ["--dataset", "pairs", "--data_path", root, "--base_channels", "2", "--thold", "0.5", "--batch_size", "1",
             "--skip_stage_id", "4", "--is_eval", "0"]
    model = E.build_model(E.build_parser().parse_args(flags), torch.device("cuda:0"))
    for p in (0, 1):
        d = tmp_path / ("out%d" % p)
        assert E.test(E.build_parser().parse_args(flags + ["--pipeline", str(p), "--save2where", str(d)]),
                      model=model) is None
        out[p] = {n: np.asarray(Image.open(str(d / (n + ".png")))) for n in ("a", "b")}
    for n in ("a", "b"):
        assert np.array_equal(out[0][n], out[1][n]), n


def test_bench_engine_tool_tiny():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_engine.py"), "--tiny"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("eager_pairs_per_s", "engine_pairs_per_s", "ceiling_pairs_per_s", "kernels"):
        assert k in res
    assert set(res["kernels"]) == {"preprocess_u8", "disparity_to_u16", "disparity_metrics"}
    assert all(res[k] > 0 for k in ("eager_pairs_per_s", "engine_pairs_per_s", "ceiling_pairs_per_s"))
    assert res["engine_equals_eager"] is True
