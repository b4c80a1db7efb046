"""CPU-side checks of the image boundary (csrc/imageio.hip, decnet_amd/imageio.py): the three entries reject bad
arguments before any HIP call, the normalisation table is the loader's own arithmetic bit for bit, and numpy restatements
of the two formulas the kernels implement agree with demo.disparity_to_uint16 / eval.test_loss_func on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
ONE = ctypes.c_void_p(64)                 # a non-null pointer that is never dereferenced: the checks come first


@pytest.fixture(scope="module")
def lib():
    from decnet_amd import build
    h = ctypes.CDLL(build.build())
    h.decnet_preprocess_u8.argtypes = [P] * 3 + [I] * 5 + [P]
    h.decnet_disparity_to_u16.argtypes = [P] * 2 + [I] * 5 + [P]
    h.decnet_disparity_metrics.argtypes = [P, P, F, P] + [I] * 5 + [P]
    return h


def _pre(lib, ptrs=(ONE, ONE, ONE), dims=(1, 4, 5, 27, 27)):
    return lib.decnet_preprocess_u8(*ptrs, *dims, None)


def _u16(lib, ptrs=(ONE, ONE), dims=(1, 27, 27, 4, 5)):
    return lib.decnet_disparity_to_u16(*ptrs, *dims, None)


def _met(lib, ptrs=(ONE, ONE, ONE), dims=(1, 27, 27, 4, 5)):
    return lib.decnet_disparity_metrics(ptrs[0], ptrs[1], 192.0, ptrs[2], *dims, None)


def test_null_pointers_are_rejected(lib):
    for k in range(3):
        assert _pre(lib, tuple(None if i == k else ONE for i in range(3))) == -1
        assert _met(lib, tuple(None if i == k else ONE for i in range(3))) == -1
    for k in range(2):
        assert _u16(lib, tuple(None if i == k else ONE for i in range(2))) == -1


def test_bad_shapes_are_rejected(lib):
    # decnet_preprocess_u8 takes (B, h, w, H, W), the other two (B, H, W, h, w)
    for k in range(5):
        for bad in (0, -3):
            d = [1, 4, 5, 27, 27]
            d[k] = bad
            assert _pre(lib, dims=tuple(d)) == -2, d
            d = [1, 27, 27, 4, 5]
            d[k] = bad
            assert _u16(lib, dims=tuple(d)) == -2, d
            assert _met(lib, dims=tuple(d)) == -2, d
    assert _pre(lib, dims=(1, 28, 5, 27, 27)) == -2            # H < h
    assert _pre(lib, dims=(1, 4, 28, 27, 27)) == -2            # W < w
    for f in (_u16, _met):
        assert f(lib, dims=(1, 27, 27, 28, 5)) == -2
        assert f(lib, dims=(1, 27, 27, 4, 28)) == -2


def test_index_spaces_of_2_to_the_31_are_rejected(lib):
    assert _u16(lib, dims=(2, 32768, 32768, 1, 1)) == -2       # B H W = 2^31
    assert _met(lib, dims=(2, 32768, 32768, 1, 1)) == -2
    assert _pre(lib, dims=(1, 1, 1, 32768, 32768)) == -2       # 3 B H W >= 2^31 although B H W is not
    assert _pre(lib, dims=(2, 1, 1, 32768, 32768)) == -2


def test_binding_knows_the_three_entries():
    from decnet_amd import _lib
    for name in ("decnet_preprocess_u8", "decnet_disparity_to_u16", "decnet_disparity_metrics"):
        assert name in _lib.SIGNATURES


def test_table_is_the_loaders_arithmetic_bit_for_bit():
    from decnet_amd import imageio, loader
    t = imageio.normalise_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (256, 3) and t.is_contiguous()
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)          # a 1 x 256 image, all values
    want = loader.normalise(ramp.astype(np.float32) / 255)                               # [3,1,256], _Base._item's calls
    assert np.array_equal(t.numpy().view(np.int32), want[:, 0, :].t().contiguous().numpy().view(np.int32))
    # the padding holds (0 - mean) / std: the reference pads before it normalises
    assert np.array_equal(t[0].numpy(), ((np.float32(0) - loader.MEAN) / loader.STD).astype(np.float32))


def test_padded_size_is_pad_top_lefts():
    from decnet_amd import imageio, loader
    for h, w in ((1, 1), (27, 27), (26, 28), (40, 101), (540, 960), (375, 1242)):
        assert imageio.padded_size(h, w) == loader.pad_top_left(np.zeros((h, w, 1), np.float32)).shape[:2]


def u16_formula(pred, h, w):
    """What decnet_disparity_to_u16 computes, in numpy: fp32 multiply, clamp, truncate, bottom-right window."""
    v = np.minimum(np.maximum(pred.astype(np.float32) * np.float32(256), np.float32(0)), np.float32(65535))
    return v.astype(np.uint16)[:, pred.shape[1] - h:, pred.shape[2] - w:]


def metrics_formula(pred, gt, max_disp):
    """What decnet_disparity_metrics computes, in numpy: per-row sums [B,h,3] over the bottom-right window (float64 sum)."""
    B, h, w = gt.shape
    p = pred[:, pred.shape[1] - h:, pred.shape[2] - w:].astype(np.float32)
    valid = (gt > 0) & (gt < np.float32(max_disp))
    err = np.abs(p - gt)                                                                # fp32
    good = valid & ((err < 3) | (err < np.float32(0.05) * gt))
    return np.stack([valid.sum(-1).astype(np.float64), np.where(valid, err, 0).astype(np.float64).sum(-1),
                     good.sum(-1).astype(np.float64)], axis=-1)


def test_u16_formula_is_disparity_to_uint16():
    """Anchors the restatement that tests/test_imageio_gpu.py holds the kernel to: u16_formula against the existing
    demo.disparity_to_uint16 at the clamp and truncation edges.  It runs none of the new library code by itself (the
    kernel sees the same edge values on the GPU, test_u16_is_disparity_to_uint16 there)."""
    from decnet_amd.demo import disparity_to_uint16
    rng = np.random.RandomState(3)
    pred = (rng.rand(2, 27, 54).astype(np.float32) * 300 - 20)                         # values < 0 and >= 256
    pred[0, -1, -5:] = [255.998, 255.99609375, 256.0, -0.001, 0.0039]
    pred[1, 0, :3] = [1e9, -1e9, 65535.0 / 256]
    for h, w in ((27, 54), (26, 50), (1, 1)):
        got = u16_formula(pred, h, w)
        for j in range(2):
            assert np.array_equal(got[j], disparity_to_uint16(torch.from_numpy(pred[j:j + 1]), h, w))
    assert u16_formula(np.full((1, 1, 1), 255.998, np.float32), 1, 1)[0, 0, 0] == 65535    # 65535.488 truncates
    assert u16_formula(np.full((1, 1, 1), 255.99, np.float32), 1, 1)[0, 0, 0] == 65533


def test_metrics_formula_is_test_loss_func():
    from decnet_amd import imageio, loader
    from decnet_amd.eval import test_loss_func
    rng = np.random.RandomState(4)
    B, h, w, D = 2, 26, 50, 40
    H, W = imageio.padded_size(h, w)
    gt = (rng.rand(B, h, w).astype(np.float32) * 60 - 5)                               # invalid on both sides of (0, D)
    gt[0, 3] = 0                                                                        # a row without a valid pixel
    pred = rng.rand(B, H, W).astype(np.float32) * 45
    pred[:, -h:, -w:][:, ::2] = gt[:, ::2] + rng.randn(B, (h + 1) // 2, w).astype(np.float32)   # errors around the 3-px gate
    part = metrics_formula(pred, gt, D)
    assert part.shape == (B, h, 3) and not part[0, 3].any()
    gt_padded = torch.stack([torch.from_numpy(loader.pad_top_left(g)) for g in gt])
    epe, loss_3 = test_loss_func(torch.from_numpy(pred), gt_padded, D)
    got_epe, got_l3 = imageio.metrics_from_partials(torch.from_numpy(part))
    n = part[..., 0].sum()
    assert n == int(((gt_padded < D) & (gt_padded > 0)).sum())
    assert abs(got_epe - float(epe)) <= 2 * n * 2.0 ** -24 * got_epe                    # torch's mean is an fp32 sum
    assert abs(got_l3 - float(loss_3)) <= 2 * 100 * 2.0 ** -24
    # the good count itself, exactly
    m = (gt_padded < D) & (gt_padded > 0)
    err = (torch.from_numpy(pred)[m] - gt_padded[m]).abs()
    assert part[..., 2].sum() == int(((err < 3) | (err < 0.05 * gt_padded[m])).sum())


def test_metrics_nan_and_empty():
    from decnet_amd import imageio
    pred = np.ones((1, 2, 3), np.float32)
    gt = np.full((1, 2, 3), 5, np.float32)
    pred[0, 0, 1] = np.nan
    part = metrics_formula(pred, gt, 10)
    assert np.isnan(part[0, 0, 1]) and part[0, 0, 0] == 3 and part[0, 0, 2] == 0 and part[0, 1, 2] == 0
    epe, l3 = imageio.metrics_from_partials(np.zeros((1, 4, 3), np.float32))
    assert np.isnan(epe) and np.isnan(l3)
    assert imageio.metrics_from_sums([4, 2.0, 3]) == (0.5, 25.0)


def test_wrappers_refuse_cpu_tensors():
    import decnet_amd
    from decnet_amd import imageio
    with pytest.raises(decnet_amd.DecnetHipError):
        imageio.preprocess_u8(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), imageio.normalise_table(),
                              torch.zeros(1, 3, 27, 27))
    with pytest.raises(decnet_amd.DecnetHipError):
        imageio.disparity_to_u16(torch.zeros(1, 27, 27), torch.zeros(1, 2, 2, dtype=torch.int16))
    with pytest.raises(decnet_amd.DecnetHipError):
        imageio.disparity_metrics(torch.zeros(1, 27, 27), torch.zeros(1, 2, 2), 192, torch.zeros(1, 2, 3))
