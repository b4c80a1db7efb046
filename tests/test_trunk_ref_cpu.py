"""The float64 references of tests/_trunk_ref.py against independent formulations (torch's own operators in float64,
explicit per-pixel loops at tiny shapes) and against the model's CPU paths (decnet_amd.model), so that the GPU edge
tests compare the HIP entries with something that is itself checked.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

import _trunk_ref as R

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("k,dil,shape", [(3, 1, (2, 5, 7)), (3, 4, (1, 3, 5)), (3, 2, (2, 1, 9)), (1, 1, (1, 4, 6))])
def test_conv_vs_torch_and_a_loop(k, dil, shape):
    g = _g(k * 10 + dil)
    B, H, W = shape
    xs = [torch.randn(B, c, H, W, generator=g, dtype=D) for c in (2, 1, 3)]
    w = torch.randn(4, 6, k, k, generator=g, dtype=D)
    scale, shift = torch.rand(4, generator=g, dtype=D) + 0.5, torch.randn(4, generator=g, dtype=D)
    got = R.conv_bn_act(xs, w, scale, shift, dil, relu=True)
    x = torch.cat(xs, 1)
    ref = torch.relu(F.conv2d(x, w, padding=dil * (k // 2), dilation=dil) * scale[:, None, None] + shift[:, None, None])
    _close(got, ref)
    p = dil * (k // 2)
    loop = torch.zeros(B, 4, H, W, dtype=D)
    for b in range(B):
        for co in range(4):
            for yy in range(H):
                for xx in range(W):
                    s = 0.0
                    for ci in range(6):
                        for ky in range(k):
                            for kx in range(k):
                                yi, xi = yy - p + ky * dil, xx - p + kx * dil
                                if 0 <= yi < H and 0 <= xi < W:
                                    s += float(x[b, ci, yi, xi]) * float(w[co, ci, ky, kx])
                    loop[b, co, yy, xx] = max(0.0, s * float(scale[co]) + float(shift[co]))
    _close(got, loop)


@pytest.mark.parametrize("epi", [1, 2])
def test_epilogue_formula(epi):
    g = _g(epi)
    v = torch.randn(2, 1, 3, 4, generator=g, dtype=D) * 100          # sigmoid saturates for most
    ea, eb = torch.randn(2, 3, 4, generator=g, dtype=D), torch.randn(2, 3, 4, generator=g, dtype=D)
    got = R.epilogue(v, epi, ea, eb)[:, 0]
    for i in range(v.numel()):
        b, yy, xx = i // 12, (i // 4) % 3, i % 4
        vv, a, e = float(v[b, 0, yy, xx]), float(ea[b, yy, xx]), float(eb[b, yy, xx])
        s = 1.0 / (1.0 + math.exp(-vv))
        want = a * (1 - s) + s * e if epi == 1 else a + vv
        assert abs(float(got[b, yy, xx]) - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (4, 4), (5, 2), (7, 10), (9, 9)])
def test_s2d3_vs_unfold_and_stride3_conv(H, W):
    g = _g(H * 16 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=D)
    Ho, Wo = (H - 1) // 3 + 1, (W - 1) // 3 + 1
    ref = F.unfold(x, 3, padding=1, stride=3).view(2, 27, Ho, Wo)
    assert torch.equal(R.s2d3_pad1(x), ref)
    w = torch.randn(5, 3, 3, 3, generator=g, dtype=D)
    scale, shift = torch.rand(5, generator=g, dtype=D) + 0.5, torch.randn(5, generator=g, dtype=D)
    conv = F.conv2d(x, w, stride=3, padding=1) * scale[:, None, None] + shift[:, None, None]
    _close(R.conv_s3_bn_act(x, w, scale, shift, relu=False), conv)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (4, 5)])
def test_deconv_vs_conv_transpose(H, W):
    g = _g(H + W)
    x = torch.randn(2, 4, H, W, generator=g, dtype=D)
    w = torch.randn(4, 6, 3, 3, generator=g, dtype=D)
    scale, shift = torch.rand(6, generator=g, dtype=D) + 0.5, torch.randn(6, generator=g, dtype=D)
    ref = torch.relu(F.conv_transpose2d(x, w, stride=3) * scale[:, None, None] + shift[:, None, None])
    _close(R.deconv_s3_bn_act(x, w, scale, shift, relu=True), ref)


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 2, 2), (1, 2, 4, 9), (2, 1, 3, 17)])
def test_warp_vs_grid_sample_and_a_loop(B, C, H, W):
    g = _g(B * 100 + W)
    right = torch.randn(B, C, H, W, generator=g, dtype=D)
    for disp in R.warp_disparities(B, H, W, g):
        got = R.warp(right, disp)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=D), torch.arange(W, dtype=D), indexing="ij")
        cx = (xs - disp) / ((W - 1.0) / 2.0) - 1.0
        cy = (ys / ((H - 1.0) / 2.0) - 1.0).expand_as(cx)
        ref = F.grid_sample(right, torch.stack((cx, cy), 3), mode="bilinear", padding_mode="zeros", align_corners=False)
        _close(got, ref, 1e-10)
    disp = R.warp_disparities(B, H, W, g)[-1]
    got = R.warp(right, disp)
    for b in range(B):                                            # per-pixel, from the header's formula
        for yy in range(H):
            for xx in range(W):
                ix = (xx - float(disp[b, yy, xx])) * W / (W - 1) - 0.5
                iy = yy * H / (H - 1) - 0.5
                x0, y0 = math.floor(ix), math.floor(iy)
                for c in range(C):
                    s = 0.0
                    for yi, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
                        for xi, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
                            if 0 <= yi < H and 0 <= xi < W:
                                s += float(right[b, c, yi, xi]) * wx * wy
                    assert abs(float(got[b, c, yy, xx]) - s) < 1e-10


def test_warp_vs_the_model_cpu_path():
    """decnet_amd.model.warp_by_disparity on CPU (float32 meshgrid + grid_sample).  With the coordinates rounded as
    float32 the reference is that path up to the rounding of torch's own unnormalisation order and of the interpolation
    (2e-5, the small-kernel tolerance); with float64 coordinates the sample position moves by the float32 rounding of
    ix ~ W (an ulp of 300 is 3e-5 pixels, times a gradient of a few units: 1e-4)."""
    from decnet_amd import model as M
    g = _g(5)
    B, C, H, W = 2, 3, 6, 300
    right = torch.randn(B, C, H, W, generator=g)
    for disp in R.warp_disparities(B, H, W, g):
        disp = disp.float()
        with torch.no_grad():
            ref = M.warp_by_disparity(right, disp).double()
        _close(R.warp(right, disp, coord_dtype=torch.float32), ref, 2e-5)
        _close(R.warp(right, disp), ref, 1e-4)


def test_dynamic_upsample3_vs_a_loop_and_the_model():
    from decnet_amd.model import DynamicUpsampling
    g = _g(9)
    B, h, w, C = 2, 3, 4, 2
    logits = torch.randn(B, 81, h, w, generator=g) * 20
    disp = torch.rand(B, h, w, generator=g) * 30
    got = R.dynamic_upsample3(logits, disp)
    for b in range(B):
        for yy in range(3 * h):
            for xx in range(3 * w):
                y, x, s = yy // 3, xx // 3, (yy % 3) * 3 + xx % 3
                z = [float(logits[b, 9 * s + k, y, x]) for k in range(9)]
                m = max(z)
                e = [math.exp(v - m) for v in z]
                nb = [float(disp[b, min(max(y + k // 3 - 1, 0), h - 1), min(max(x + k % 3 - 1, 0), w - 1)])
                      for k in range(9)]
                want = 3 * sum(ei * n for ei, n in zip(e, nb)) / sum(e)
                assert abs(float(got[b, yy, xx]) - want) < 1e-12 * max(1.0, abs(want))

    class Const(torch.nn.Module):                  # stands in for weight_learning: records its input, returns logits
        def forward(self, wts):
            self.wts = wts
            return logits

    m = DynamicUpsampling(C, 3).eval()
    m.weight_learning = Const()
    fea = torch.randn(B, C, 3 * h, 3 * w, generator=g)
    with torch.no_grad():
        out = m(disp, fea)                         # CPU: F.unfold + cat, softmax, replicate pad, pixel_shuffle
    _close(got, out.double(), 2e-6)
    assert torch.equal(R.unfold3_cat(fea, disp), m.weight_learning.wts.double())


def test_unfold3_cat_vs_unfold():
    g = _g(3)
    fea, disp = torch.randn(2, 3, 6, 9, generator=g, dtype=D), torch.randn(2, 2, 3, generator=g, dtype=D)
    ref = torch.cat((disp.unsqueeze(1), F.unfold(fea, 3, stride=3).view(2, 27, 2, 3)), 1)
    assert torch.equal(R.unfold3_cat(fea, disp), ref)


def test_bias_act():
    g = _g(4)
    y, sh = torch.randn(2, 3, 2, 5, generator=g, dtype=D), torch.randn(3, generator=g, dtype=D)
    for relu in (0, 1):
        got = R.bias_act(y, sh, relu)
        for b, c, i, j in ((0, 0, 0, 0), (1, 2, 1, 4), (0, 1, 1, 2)):
            v = float(y[b, c, i, j]) + float(sh[c])
            assert float(got[b, c, i, j]) == (max(v, 0.0) if relu else v)


def test_detail_logits_vs_the_model_units_and_bits():
    from decnet_amd.model import GenerateSparseMask
    torch.manual_seed(1)
    gen = GenerateSparseMask(8, 3).eval()
    for u in gen.conv:
        u.bn.weight.data.uniform_(0.5, 1.5); u.bn.bias.data.normal_(0, 0.3)
        u.bn.running_mean.data.normal_(0, 0.2); u.bn.running_var.data.uniform_(0.5, 1.5)
    g = _g(6)
    cur, pre = torch.randn(2, 3, 4, 70, generator=g), torch.randn(2, 3, 4, 70, generator=g)
    gen = gen.double()                                  # BatchNorm folded in float64 below, as the model's units run
    u3, u1 = gen.conv[0], gen.conv[1]
    fold = lambda u: (u.bn.weight / torch.sqrt(u.bn.running_var + u.bn.eps),
                      u.bn.bias - u.bn.running_mean * u.bn.weight / torch.sqrt(u.bn.running_var + u.bn.eps))
    (s3, b3), (s1, b1) = fold(u3), fold(u1)
    with torch.no_grad():
        got = R.detail_logits(cur, pre, u3.conv.weight, s3, b3, u1.conv.weight.reshape(3), float(s1), float(b1))
        d = cur.double() - pre.double()
        ref = gen.conv(d * d).squeeze(1)
    _close(got, ref, 1e-12)
    mask = torch.sigmoid(got) > 0.5
    words = R.pack_bits(mask)
    assert words.shape == (2, 4, 2)
    for b in range(2):
        for yy in range(4):
            for wi in range(2):
                want = 0
                for i in range(64):
                    if 64 * wi + i < 70 and bool(mask[b, yy, 64 * wi + i]):
                        want |= 1 << i
                assert int(words[b, yy, wi]) & (2 ** 64 - 1) == want


@pytest.mark.parametrize("B,H,W,dils", [(2, 3, 4, (1, 3, 4)), (2, 2, 2, (2, 5, 9)), (1, 5, 7, (1, 2, 3))])
def test_tap_chain_equals_the_dilated_convolutions(B, H, W, dils):
    """tap_gemm -> tap_gather == the four ASPP branches as convolutions: at B = 2 with dilation >= H and >= W the taps
    that would land in the other image must be the zero padding of a convolution."""
    g = _g(B * 31 + H)
    Ci, Co = 8, 5
    x = torch.randn(B, Ci, H, W, generator=g, dtype=D)
    ws = [torch.randn(Co, Ci, 1, 1, generator=g, dtype=D)] + [torch.randn(Co, Ci, 3, 3, generator=g, dtype=D)
                                                              for _ in dils]
    ks, ds = (1,) + (3,) * len(dils), (1,) + tuple(dils)
    scale, shift = torch.rand(4 * Co, generator=g, dtype=D) + 0.5, torch.randn(4 * Co, generator=g, dtype=D)
    got = R.tap_gather(R.tap_gemm(x, ws), ks, ds, scale, shift, relu=True)
    ref = torch.cat([F.conv2d(x, w, padding=d * (w.shape[-1] // 2), dilation=d) for w, d in zip(ws, ds)], 1)
    ref = torch.relu(ref * scale[:, None, None] + shift[:, None, None])
    _close(got, ref)
