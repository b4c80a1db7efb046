"""Host logic of decnet_amd.StereoEngine with the device layer stubbed (bucket keys, LRU eviction, slot / order
bookkeeping, where the D2H of a batch goes on the copy stream, short-batch filling), the refusals, and the loaders' raw
mode.  No GPU."""
import pickle
import types

import numpy as np
import pytest
import torch


class FakeDevice:
    """Stands in for engine._HipBackend: logs every device call; a batch 'computes' / 'finishes' when the test says so."""

    def __init__(self):
        self.log, self.computed_tags, self.finished_tags = [], set(), set()

    def new_slot(self):
        from decnet_amd import engine
        s = engine._Slot()
        s.downloaded = False
        return s

    def new_bucket(self, key):
        self.log.append(("capture", key))
        return types.SimpleNamespace(key=key)

    def drop_bucket(self, bucket):
        self.log.append(("drop", bucket.key))

    def stage(self, slot, lefts, rights, gts, B, sums_out=None):
        slot.shape, slot.n = (B,) + lefts[0].shape[:2], len(lefts)
        slot.payload = [a[..., 0].astype(np.uint16) for a in lefts]
        slot.downloaded = False

    def upload(self, slot):
        self.log.append(("h2d", slot.tag))

    def compute_batch(self, slot, bucket):
        self.log.append(("compute", slot.tag, bucket.key))

    def download(self, slot):
        self.log.append(("d2h", slot.tag))
        slot.downloaded = True

    def computed(self, slot):
        return slot.tag in self.computed_tags

    def done(self, slot):
        return slot.downloaded and slot.tag in self.finished_tags

    def wait(self, slot):
        assert slot.downloaded, "waited for a batch whose D2H was never enqueued"
        self.log.append(("wait", slot.tag))
        self.finished_tags.add(slot.tag)

    def collect(self, slot):
        return slot.payload, None

    def finish(self, *tags):
        self.computed_tags.update(tags)
        self.finished_tags.update(tags)


def _model(**kw):
    return types.SimpleNamespace(**dict(dict(use_detail=True, max_disp=216), **kw))


def _engine(**kw):
    from decnet_amd import StereoEngine
    dev = FakeDevice()
    return StereoEngine(_model(), backend=dev, **kw), dev


def _pair(h, w, v=0, n=1):
    a = [np.full((h, w, 3), v + i, np.uint8) for i in range(n)]
    return a, [x.copy() for x in a]


def test_bucket_key_is_batch_padded_size_and_range():
    eng, _ = _engine(batch_size=3)
    assert eng.bucket_key(40, 100) == (3, 54, 108, 216)
    assert eng.bucket_key(54, 81, 54) == (3, 54, 81, 54)
    assert eng.bucket_key(1, 1, 27) == (3, 27, 27, 27)
    assert eng.bucket_key(375, 1242) == (3, 378, 1242, 216)
    eng.model.max_disp = 192                              # None follows the model as it is at submit time
    assert eng.bucket_key(40, 100) == (3, 54, 108, 192)


def test_buckets_are_kept_lru_and_evicted_at_max_buckets():
    eng, dev = _engine(batch_size=1, max_buckets=2, depth=1)
    shapes = {"a": (40, 100), "b": (54, 81), "c": (27, 27)}

    def go(name, **kw):
        eng.submit(*_pair(*shapes[name]), tag=name, **kw)
    ka, kb, kc = (1, 54, 108, 216), (1, 54, 81, 216), (1, 27, 27, 216)
    go("a"), go("b"), go("a"), go("c"), go("a"), go("b")
    eng.flush()
    events = [e for e in dev.log if e[0] in ("capture", "drop")]
    assert events == [("capture", ka), ("capture", kb),               # a again: a hit, and b becomes the oldest
                      ("drop", kb), ("capture", kc),                  # c evicts b, not a
                      ("drop", kc), ("capture", kb)]                  # a hit again; b evicts c
    assert list(eng._buckets) == [ka, kb]
    go("a", max_disp=54)                                              # another range is another bucket
    assert list(eng._buckets) == [kb, (1, 54, 108, 54)]
    eng.reset()
    assert not eng._buckets and [e for e in dev.log if e[0] == "drop"][-2:] == [("drop", kb), ("drop", (1, 54, 108, 54))]


def test_results_come_back_in_submission_order_and_d2h_goes_behind_the_next_h2d():
    eng, dev = _engine(batch_size=2, depth=2)
    eng.submit(*_pair(27, 27, 10, n=2), tag="A")
    eng.submit(*_pair(27, 27, 20, n=1), tag="B")
    k = (2, 27, 27, 216)
    assert dev.log == [("capture", k), ("h2d", "A"), ("compute", "A", k), ("h2d", "B"), ("d2h", "A"), ("compute", "B", k)]
    assert eng.results() == []                                        # nothing finished: no wait, and no D2H of B
    assert ("d2h", "B") not in dev.log and not any(e[0] == "wait" for e in dev.log)
    dev.finish("B")                                                   # B done before A: order is kept
    assert eng.results() == []
    dev.finish("A")
    got = eng.results()
    assert [g[0] for g in got] == ["A", "B"] and ("d2h", "B") in dev.log
    assert [int(a[0, 0]) for a in got[0][1]] == [10, 11] and [int(a[0, 0]) for a in got[1][1]] == [20]
    assert got[0][2] is None
    # every slot busy: submit waits for the oldest only
    eng.submit(*_pair(27, 27, 30), tag="C")
    eng.submit(*_pair(27, 27, 40), tag="D")
    assert not any(e[0] == "wait" for e in dev.log)
    eng.submit(*_pair(27, 27, 50), tag="E")
    assert [e for e in dev.log if e[0] == "wait"] == [("wait", "C")]
    rest = eng.flush()
    assert [g[0] for g in rest] == ["C", "D", "E"] and eng.flush() == [] and eng.results() == []
    assert [e[1] for e in dev.log if e[0] == "wait"] == ["C", "D", "E"]


def test_depth_one_downloads_before_it_waits():
    eng, dev = _engine(batch_size=1, depth=1)
    eng.submit(*_pair(27, 27, 1), tag=0)
    eng.submit(*_pair(27, 27, 2), tag=1)
    assert [e for e in dev.log if e[0] in ("d2h", "wait")] == [("d2h", 0), ("wait", 0)]
    assert [g[0] for g in eng.flush()] == [0, 1]


def test_reset_keeps_the_results_that_were_not_handed_out():
    """reset() waits for what is in flight and drops the buckets; the finished batches still come back from results()."""
    eng, dev = _engine(batch_size=1, depth=2)
    eng.submit(*_pair(27, 27, 10), tag="A")
    eng.submit(*_pair(27, 27, 20), tag="B")
    eng.reset()
    assert not eng._buckets and [e[1] for e in dev.log if e[0] == "wait"] == ["A", "B"]
    got = eng.results()
    assert [g[0] for g in got] == ["A", "B"] and [int(g[1][0][0, 0]) for g in got] == [10, 20]
    assert eng.flush() == []
    eng.submit(*_pair(27, 27, 30), tag="C")                           # and the engine goes on: a new capture
    eng.reset()
    assert [g[0] for g in eng.flush()] == ["C"] and [e[0] for e in dev.log].count("capture") == 2


def test_cache_tensors_lists_what_the_cache_attributes_hold():
    """What a bucket keeps alive: the tensors under a module's _CACHE_ATTRS, at any nesting, and nothing else."""
    from decnet_amd.engine import _cache_tensors
    from decnet_amd.stage0 import CachesWeights

    class M(CachesWeights, torch.nn.Module):
        _CACHE_ATTRS = ("_a", "_ws", "_unset")

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2))
            self.other = torch.ones(3)                                # not a cache
    m = M()
    assert m.cache_tensors() == []
    deep = torch.zeros(1)
    for _ in range(9):
        deep = [deep]
    ts = [torch.zeros(i + 1) for i in range(4)]
    m._a = (ts[0], ts[1], 3.5, None)
    m._ws = {("wino", "cpu"): dict(u=ts[2], keep=[ts[3], ts[0]]), "deep": deep}
    got = m.cache_tensors()
    assert sorted(t.numel() for t in got) == [1, 1, 2, 3, 4] and not any(t is m.other or t is m.w for t in got)
    assert len(_cache_tensors(torch.nn.Sequential(m, torch.nn.ReLU(), M()))) == 5
    m._drop_caches()
    assert m.cache_tensors() == []


def test_submit_refuses_bad_batches():
    eng, _ = _engine(batch_size=2)
    l, r = _pair(27, 27, n=3)
    with pytest.raises(ValueError):
        eng.submit(l, r)                                              # more than batch_size
    with pytest.raises(ValueError):
        eng.submit([], [])
    with pytest.raises(ValueError):
        eng.submit(l[:2], r[:1])
    with pytest.raises(ValueError):
        eng.submit([l[0], np.zeros((27, 28, 3), np.uint8)], r[:2])    # unequal sizes
    with pytest.raises(ValueError):
        eng.submit([l[0].astype(np.float32)], r[:1])                  # not uint8
    with pytest.raises(ValueError):
        eng.submit(l[:1], r[:1], gts=[np.zeros((5, 5), np.float32)])
    with pytest.raises(ValueError):
        eng.submit(l[:1], r[:1], sums_out=torch.zeros(3, dtype=torch.float64))     # needs gts


def test_short_batches_are_filled_with_their_last_item():
    from decnet_amd.engine import fill_batch
    items = [np.full((2, 3), i, np.uint8) for i in (7, 9)]
    dst = np.full((4, 2, 3), 255, np.uint8)
    fill_batch(dst, items)
    assert [int(d[0, 0]) for d in dst] == [7, 9, 9, 9] and all((d == d[0, 0]).all() for d in dst)
    gt = np.full((4, 2, 3), 5, np.float32)
    fill_batch(gt, [np.ones((2, 3), np.float32)] * 2, repeat_last=False)          # no valid pixel in the filled samples
    assert gt[:2].min() == 1 and not gt[2:].any()
    fill_batch(dst[:2], items)                                                     # a full batch: a plain copy
    assert [int(d[0, 0]) for d in dst[:2]] == [7, 9]


def test_use_detail_false_and_cpu_models_are_refused():
    from decnet_amd import StereoEngine
    from decnet_amd.model import get_model
    with pytest.raises(ValueError, match="use_detail"):
        StereoEngine(_model(use_detail=False), backend=FakeDevice())
    kw = dict(name="sparsedensenetrefinementmask", max_disp=54, base_channels=2, cost_func="cor", grad_method="detach",
              num_stage=4, down_scale=3, step=[-1, 1, 1, 1], samp_num=[-1, 12, 10, 6],
              sample_spa_size_list=[-1, 3, 5, 7], down_func_name="bicubic", weights=[1, 1, 1, 1], if_overmask=False,
              skip_stage_id=4, thold=0.5)
    with pytest.raises(ValueError, match="use_detail"):
        StereoEngine(get_model(use_detail=False, **kw).eval())
    with pytest.raises(ValueError, match="CPU"):
        StereoEngine(get_model(use_detail=True, **kw).eval())          # a use_detail model, but on the CPU
    with pytest.raises(ValueError):
        StereoEngine(_model(), batch_size=0, backend=FakeDevice())


# ---- the loaders' raw mode ----------------------------------------------------------------------------------------------
def test_npy_raw_mode_round_trips_exactly_and_refuses_fractions(tmp_path):
    from decnet_amd import loader
    rng = np.random.RandomState(0)
    (tmp_path / "test").mkdir()
    u8 = rng.randint(0, 256, (30, 50, 6)).astype(np.uint8)
    u8[0, 0, :] = [0, 255, 1, 254, 0, 255]
    disp = rng.rand(30, 50, 1).astype(np.float32) * 40
    np.save(tmp_path / "test" / "a.npy", np.concatenate([u8.astype(np.float32), disp], -1))
    left, right, d, name, nd = loader.NpyPairs(str(tmp_path), split="test", raw=True)[0]
    assert left.dtype == np.uint8 and left.shape == (30, 50, 3) and left.flags.c_contiguous
    assert np.array_equal(left, u8[..., :3]) and np.array_equal(right, u8[..., 3:])
    assert d.dtype == np.float32 and np.array_equal(d, disp[..., 0]) and (name, nd) == ("a", -1)
    # the default mode is what it was: the same pixels, padded and normalised on the host
    full = loader.NpyPairs(str(tmp_path), split="test")[0]
    assert len(full) == 14 and torch.equal(full[0], loader.normalise(loader.pad_top_left(u8[..., :3].astype(np.float32)) / 255))
    for bad in (0.5, 256.0, -1.0):
        arr = np.concatenate([u8.astype(np.float32), disp], -1)
        arr[3, 4, 1] = bad
        np.save(tmp_path / "test" / "b.npy", arr)
        ds = loader.NpyPairs(str(tmp_path), split="test", raw=True)
        with pytest.raises(ValueError, match="b.npy"):
            ds[1]
    with pytest.raises(ValueError, match="training"):                 # no raw training samples: refused, not ignored
        loader.NpyPairs(str(tmp_path), split="test", raw=True, is_training=True)


def test_middlebury_and_pair_directory_raw_mode(tmp_path):
    from PIL import Image
    from decnet_amd import loader
    rng = np.random.RandomState(2)
    d = tmp_path / "mb" / "MiddEval3H_processed" / "trainingH"
    d.mkdir(parents=True)
    im0, im1 = (rng.randint(0, 256, (20, 31, 3)).astype(np.uint8) for _ in range(2))
    gt = rng.rand(20, 31).astype(np.float32) * 50
    gt[3, 4] = np.inf
    with open(d / "Adirondack.pkl", "wb") as f:
        pickle.dump({"ndisp": 145, "im0": im0, "im1": im1, "disparity": gt.copy()}, f)
    left, right, disp, name, nd = loader.MiddleburyPickles(str(tmp_path / "mb"), split="eval_H", raw=True)[0]
    assert np.array_equal(left, im0) and np.array_equal(right, im1) and left.dtype == np.uint8
    assert disp[3, 4] == 0 and np.array_equal(np.delete(disp.ravel(), 3 * 31 + 4), np.delete(gt.ravel(), 3 * 31 + 4))
    assert (name, nd) == ("Adirondack", 145)
    p = tmp_path / "pairs" / "p0"
    p.mkdir(parents=True)
    Image.fromarray(im0).save(str(p / "im0.png"))
    Image.fromarray(im1).save(str(p / "im1.png"))
    (p / "calib.txt").write_text("ndisp=40\n")
    left, right, disp, name, nd = loader.PairDirectory(str(tmp_path / "pairs"), raw=True)[0]
    assert np.array_equal(left, im0) and np.array_equal(right, im1) and (name, nd) == ("p0", 54)
    assert disp.shape == (20, 31) and disp.dtype == np.float32 and not disp.any()


def test_demo_and_eval_flags_default_to_the_existing_path():
    from decnet_amd import demo
    from decnet_amd import eval as E
    a = demo.build_parser().parse_args([])
    assert (a.pipeline, a.batch_size, a.workers) == (0, 1, 4)
    e = E.build_parser().parse_args([])
    assert (e.pipeline, e.batch_size, e.workers) == (0, 8, 4)
    with pytest.raises(SystemExit):
        demo.build_parser().parse_args(["--pipeline", "2"])


def test_demo_batches_are_runs_of_one_size_and_range():
    from decnet_amd import demo
    a, b = np.zeros((4, 5, 3), np.uint8), np.zeros((4, 6, 3), np.uint8)
    items = [("0", a, a, 216), ("1", a, a, 216), ("2", a, a, 216), ("3", b, b, 216), ("4", b, b, 54), ("5", a, a, 54)]
    assert [[i[0] for i in g] for g in demo.pair_batches(items, 2)] == [["0", "1"], ["2"], ["3"], ["4"], ["5"]]
    assert [[i[0] for i in g] for g in demo.pair_batches(items, 1)] == [[str(i)] for i in range(6)]
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(2) as pool:
        assert list(demo.prefetched(pool, lambda x: x * x, range(7), ahead=3)) == [i * i for i in range(7)]
