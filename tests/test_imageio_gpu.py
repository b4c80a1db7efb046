"""The image-boundary kernels on the GPU (csrc/imageio.hip through decnet_amd/imageio.py) against the host path they
replace: loader.normalise(pad_top_left(...)/255), demo.disparity_to_uint16, eval.test_loss_func.  Every buffer is a window
of a larger sentinel-filled buffer, once 16-byte aligned and once at an odd element offset: margins intact, inputs
unmodified, outputs fully written, the two placements bit-identical.  -m gpu."""
import numpy as np
import pytest
import torch

import _lds_poison
from test_imageio_cpu import metrics_formula, u16_formula

pytestmark = pytest.mark.gpu

G = 61                                    # guard elements on each side; odd
SENT = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.float32: 12345.0}
# (h, w) -> (H, W): one pixel; no padding; both pads, W = 2 x 27; odd width (a 303-byte row pitch); no padding, odd W
SHAPES = [((1, 1), (27, 27)), ((27, 27), (27, 27)), ((26, 28), (27, 54)), ((40, 101), (54, 108)), ((54, 81), (54, 81))]


def _bits(t):
    """A 1-D tensor as its bytes: an input that holds NaN compares equal to itself."""
    return t.contiguous().view(torch.uint8)


class Guarded:
    """Windows of sentinel-filled device buffers of any dtype; the window starts 16-byte aligned or at an odd offset."""

    def __init__(self, dev, aligned):
        self.dev, self.aligned, self.items = dev, aligned, []

    def _win(self, n, dtype):
        item = torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((n + 2 * G + 16,), SENT[dtype], dtype=dtype, device=self.dev)
        off = next(o for o in range(G, G + 17)
                   if ((buf.data_ptr() + o * item) % 16 == 0) == self.aligned and (self.aligned or o % 2 == 1))
        return buf, off

    def inp(self, x):
        x = x.contiguous()
        buf, off = self._win(x.numel(), x.dtype)
        buf[off:off + x.numel()].copy_(x.reshape(-1))
        self.items.append((buf, off, x.numel(), _bits(x.cpu().clone().reshape(-1))))
        return buf[off:off + x.numel()].view(x.shape)

    def out(self, shape, dtype):
        n = int(np.prod(shape))
        buf, off = self._win(n, dtype)
        self.items.append((buf, off, n, None))
        return buf[off:off + n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, off, n, host in self.items:
            s = SENT[buf.dtype]
            assert bool((buf[:off] == s).all()) and bool((buf[off + n:] == s).all()), "write outside a window"
            if host is not None:
                assert torch.equal(_bits(buf[off:off + n].cpu()), host), "an input was modified"


def _poisoned(run, base):
    """run(aligned) -> host array, at both placements with LDS poisoned before the entry (tests/_lds_poison.py: the package's
    handle replaced by the poisoning proxy), under each pattern: the same bytes as `base`, the unpoisoned aligned result."""
    for aligned in (True, False):
        for pat in _lds_poison.PATTERNS:
            with _lds_poison.package(pat):
                got = run(aligned)
            assert np.array_equal(np.asarray(got).view(np.uint8), np.asarray(base).view(np.uint8)), \
                "result differs under %s, aligned=%s" % (_lds_poison.name(pat), aligned)


def _images(B, h, w, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (B, h, w, 3)).astype(np.uint8)
    if h * w >= 256:                       # the first image holds all 256 values in every channel
        flat = img[0].reshape(-1, 3)
        for c in range(3):
            flat[:256, c] = np.roll(np.arange(256, dtype=np.uint8), 85 * c)
    return img


@pytest.fixture(scope="module")
def table():
    from decnet_amd import imageio
    return imageio.normalise_table()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,HW", SHAPES)
def test_preprocess_is_the_host_path_bit_for_bit(hw, HW, B, table):
    from decnet_amd import imageio, loader
    dev = torch.device("cuda:0")
    (h, w), (H, W) = hw, HW
    assert imageio.padded_size(h, w) == (H, W)
    img = _images(B, h, w, seed=h * 1000 + w + B)
    if h * w >= 256:
        assert all(len(np.unique(img[0, ..., c])) == 256 for c in range(3))
    want = torch.stack([loader.normalise(loader.pad_top_left(a.astype(np.float32)) / 255) for a in img])
    got = {}
    for aligned in (True, False):
        g = Guarded(dev, aligned)
        out = g.out((B, 3, H, W), torch.float32)
        out.fill_(float("nan"))
        imageio.preprocess_u8(g.inp(torch.from_numpy(img).to(dev)), g.inp(table.to(dev)), out)
        g.check()
        got[aligned] = out.cpu()
        assert torch.equal(got[aligned].view(torch.int32), want.view(torch.int32)), "aligned=%s" % aligned
    assert torch.equal(got[True].view(torch.int32), got[False].view(torch.int32))

    def again(aligned):
        g = Guarded(dev, aligned)
        out = g.out((B, 3, H, W), torch.float32)
        out.fill_(float("nan"))
        imageio.preprocess_u8(g.inp(torch.from_numpy(img).to(dev)), g.inp(table.to(dev)), out)
        g.check()
        return out.cpu().numpy()
    _poisoned(again, got[True].numpy())


def _pred(B, H, W, seed):
    rng = np.random.RandomState(seed)
    p = (rng.rand(B, H, W).astype(np.float32) * 300 - 20)                  # negatives and values past 255.996
    p.reshape(-1)[:7] = [255.998, 255.99609375, 256.0, 1e9, -1e9, -0.001, 0.0039]
    p[:, -1, -1] = 255.998
    return p


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,HW", SHAPES + [((27, 54), (27, 54))])         # + a full-window crop with W = 8 k + 6
def test_u16_is_disparity_to_uint16(hw, HW, B):
    from decnet_amd import imageio
    from decnet_amd.demo import disparity_to_uint16
    dev = torch.device("cuda:0")
    (h, w), (H, W) = hw, HW
    pred = _pred(B, H, W, seed=H + W + B)
    want = np.stack([disparity_to_uint16(torch.from_numpy(pred[j:j + 1]), h, w) for j in range(B)])
    assert np.array_equal(want, u16_formula(pred, h, w))
    got = {}
    for aligned in (True, False):
        g = Guarded(dev, aligned)
        out = g.out((B, h, w), torch.int16)
        imageio.disparity_to_u16(g.inp(torch.from_numpy(pred).to(dev)), out)
        g.check()
        got[aligned] = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[aligned], want), "aligned=%s" % aligned
    assert np.array_equal(got[True], got[False])

    def again(aligned):
        g = Guarded(dev, aligned)
        out = g.out((B, h, w), torch.int16)
        imageio.disparity_to_u16(g.inp(torch.from_numpy(pred).to(dev)), out)
        g.check()
        return out.cpu().numpy()
    _poisoned(again, got[True])


@pytest.mark.parametrize("hw,HW", [((26, 28), (27, 54)), ((40, 101), (54, 108))])
def test_u16_output_at_an_odd_byte_address(hw, HW):
    """The header asks no alignment at all of the uint16 buffer: the window starts at an odd BYTE address of a guarded byte
    buffer (no two-byte tensor can sit there, so the entry is called with the raw pointer)."""
    from decnet_amd import imageio
    dev = torch.device("cuda:0")
    (h, w), (H, W), B = hw, HW, 3
    pred = _pred(B, H, W, seed=H + W)
    want = torch.from_numpy(np.ascontiguousarray(u16_formula(pred, h, w)).view(np.uint8).reshape(-1))
    n = want.numel()
    buf = torch.full((n + 2 * G + 16,), SENT[torch.uint8], dtype=torch.uint8, device=dev)
    off = G + (1 - (buf.data_ptr() + G) % 2)
    assert (buf.data_ptr() + off) % 2 == 1
    p = torch.from_numpy(pred).to(dev)
    imageio._call("decnet_disparity_to_u16", p, p.data_ptr(), buf.data_ptr() + off, B, H, W, h, w)
    torch.cuda.synchronize()
    s = SENT[torch.uint8]
    assert bool((buf[:off] == s).all()) and bool((buf[off + n:] == s).all()), "write outside the window"
    assert torch.equal(buf[off:off + n].cpu(), want)
    assert torch.equal(_bits(p.cpu().reshape(-1)), _bits(torch.from_numpy(pred).reshape(-1)))


def _metric_inputs(B, h, w, H, W, D, seed):
    rng = np.random.RandomState(seed)
    gt = (rng.rand(B, h, w).astype(np.float32) * (D * 1.5) - D * 0.1)      # invalid on both sides of (0, D)
    pred = rng.rand(B, H, W).astype(np.float32) * D
    win = pred[:, H - h:, W - w:]
    win[:, ::2] = gt[:, ::2] + (rng.randn(B, (h + 1) // 2, w) * 2).astype(np.float32)     # errors around both gates
    if h > 3:
        gt[0, 3] = 0                                                       # a row without a valid pixel
        win[0, 3] = np.nan                                                 # ... whose predictions must not count
    return pred, gt


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,HW", SHAPES)
def test_metrics_counts_exact_and_sums_within_fp32_summation(hw, HW, B):
    from decnet_amd import imageio
    dev = torch.device("cuda:0")
    (h, w), (H, W) = hw, HW
    D = 40
    pred, gt = _metric_inputs(B, h, w, H, W, D, seed=H * W + B)
    want = metrics_formula(pred, gt, D)                                    # float64 sums of the fp32 errors
    got = {}
    for aligned in (True, False):
        g = Guarded(dev, aligned)
        part = g.out((B, h, 3), torch.float32)
        part.fill_(float("nan"))
        imageio.disparity_metrics(g.inp(torch.from_numpy(pred).to(dev)), g.inp(torch.from_numpy(gt).to(dev)), D, part)
        g.check()
        got[aligned] = part.cpu().numpy()
        p = got[aligned].astype(np.float64)
        assert np.array_equal(p[..., 0], want[..., 0]) and np.array_equal(p[..., 2], want[..., 2])
        # any fp32 summation order over w non-negative terms: (w - 1) 2^-24 relative
        assert np.all(np.abs(p[..., 1] - want[..., 1]) <= (w - 1) * 2.0 ** -24 * want[..., 1])
        if h > 3:
            assert not p[0, 3].any()
    assert np.array_equal(got[True].view(np.int32), got[False].view(np.int32))

    def again(aligned):
        g = Guarded(dev, aligned)
        part = g.out((B, h, 3), torch.float32)
        part.fill_(float("nan"))
        imageio.disparity_metrics(g.inp(torch.from_numpy(pred).to(dev)), g.inp(torch.from_numpy(gt).to(dev)), D, part)
        g.check()
        return part.cpu().numpy()
    _poisoned(again, got[True])
    epe, l3 = imageio.metrics_from_partials(torch.from_numpy(got[True]))
    n = want[..., 0].sum()
    assert abs(epe - want[..., 1].sum() / n) <= (w - 1) * 2.0 ** -24 * epe
    assert l3 == 100.0 - want[..., 2].sum() / n * 100.0


def test_metrics_nan_prediction_gives_a_nan_sum_and_is_not_good():
    from decnet_amd import imageio
    dev = torch.device("cuda:0")
    h, w, H, W = 26, 28, 27, 54
    pred = np.full((1, H, W), 5.0, np.float32)
    gt = np.full((1, h, w), 5.0, np.float32)
    pred[0, H - h + 2, W - w + 7] = np.nan
    part = torch.empty((1, h, 3), device=dev)
    imageio.disparity_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), 192, part)
    p = part.cpu().numpy()
    assert np.isnan(p[0, 2, 1]) and p[0, 2, 0] == w and p[0, 2, 2] == w - 1
    rest = np.delete(p[0], 2, axis=0)
    assert np.array_equal(rest, np.tile(np.float32([w, 0, w]), (h - 1, 1)))
    epe, l3 = imageio.metrics_from_partials(part)
    assert np.isnan(epe) and l3 == 100.0 - (h * w - 1) / (h * w) * 100.0


def test_the_three_kernels_replay_inside_a_captured_graph(table):
    from decnet_amd import imageio
    dev = torch.device("cuda:0")
    B, (h, w), (H, W), D = 3, (40, 101), (54, 108), 40
    img = torch.from_numpy(_images(B, h, w, seed=9)).to(dev)
    pred_h, gt_h = _metric_inputs(B, h, w, H, W, D, seed=10)
    pred, gt, tab = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev), table.to(dev)

    def run(out, u16, part):
        imageio.preprocess_u8(img, tab, out)
        imageio.disparity_to_u16(pred, u16)
        imageio.disparity_metrics(pred, gt, D, part)

    def fresh():
        return (torch.zeros((B, 3, H, W), device=dev), torch.zeros((B, h, w), dtype=torch.int16, device=dev),
                torch.zeros((B, h, 3), device=dev))
    eager, static = fresh(), fresh()
    run(*eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(*static)
    for t in static:
        t.zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for e, s in zip(eager, static):
        assert torch.equal(e.view(torch.int32) if e.dtype == torch.float32 else e,
                           s.view(torch.int32) if s.dtype == torch.float32 else s)
