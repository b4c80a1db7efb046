"""The float64 references of tests/_stage0_ref.py against independent formulations: oracle/stage0.py (torch's own
grid_sample / conv3d / batch_norm, run in float64, and its closed-form warp), explicit loops at tiny shapes, and the
committed goldens of the reference's own classes (tests/golden/stage0_*.npz, within their float32 noise), so that the GPU
edge tests compare the HIP entries with something that is itself checked.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stage0_ref as R
from oracle import stage0 as o0

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _params64(params):
    """oracle params (w, (gamma, beta, mean, var)) -> the references' (w, scale, shift) in float64."""
    out = []
    for p in params:
        s, h = R.fold_bn(p["bn"])
        out.append((p["w"].double(), s, h))
    w, s, h = out[7]
    out[7] = (w, s.reshape(()), h.reshape(()))
    return out


@pytest.mark.parametrize("B,C,H,W,D", [(1, 2, 2, 2, 1), (2, 3, 3, 5, 4), (1, 1, 2, 3, 7), (2, 2, 5, 9, 6)])
def test_warp_vs_grid_sample_and_closed_form(B, C, H, W, D):
    right = torch.randn(B, C, H, W, generator=_g(B * 100 + W * 10 + D), dtype=F64)
    got = R.warp(right, D)
    ref = o0.warp_right(right, o0.disp_samples(D, B, H, W, F64))                  # [B,C,D,H,W], float64 grid_sample
    _close(got, ref.permute(0, 2, 3, 4, 1))
    cf = o0.warp_right_closed_form(right.float(), D).double()                      # float32 numpy arithmetic
    _close(got, cf.permute(0, 2, 3, 4, 1), 1e-5)


@pytest.mark.parametrize("cf", ["cor", "ssd", "cat"])
@pytest.mark.parametrize("B,C,H,W,D", [(1, 2, 2, 2, 1), (2, 3, 3, 2, 5), (1, 4, 4, 7, 3)])
def test_costvol_vs_oracle(cf, B, C, H, W, D):
    g = _g(C * 100 + W * 10 + D)
    left, right = torch.randn(B, C, H, W, generator=g, dtype=F64), torch.randn(B, C, H, W, generator=g, dtype=F64)
    got = R.costvol(left, right, D, cf)
    _close(got, o0.cost_volume(left, right, D, cf).permute(0, 2, 3, 4, 1))


def test_costvol_sum_is_the_cat_halves_added():
    g = _g(5)
    left, right = torch.randn(2, 3, 3, 4, generator=g, dtype=F64), torch.randn(2, 3, 3, 4, generator=g, dtype=F64)
    cat = R.costvol(left, right, 6, "cat")
    _close(R.costvol(left, right, 6, "sum"), cat[..., :3] + cat[..., 3:])


def _bilinear_loop(r, yf, xf):
    H, W = r.shape
    y0, x0 = math.floor(yf), math.floor(xf)
    s = 0.0
    for yy, wy in ((y0, 1 - (yf - y0)), (y0 + 1, yf - y0)):
        for xx, wx in ((x0, 1 - (xf - x0)), (x0 + 1, xf - x0)):
            if 0 <= yy < H and 0 <= xx < W:
                s += float(r[yy, xx]) * wy * wx
    return s


def test_costvol_vs_a_loop():
    """The header's formula, one voxel at a time, including D > W (planes past the image are all zero on the left)."""
    B, C, H, W, D = 1, 2, 3, 2, 4
    g = _g(11)
    left, right = torch.randn(B, C, H, W, generator=g, dtype=F64), torch.randn(B, C, H, W, generator=g, dtype=F64)
    vols = {cf: R.costvol(left, right, D, cf) for cf in ("cor", "ssd", "cat", "sum")}
    for d in range(D):
        for y in range(H):
            for x in range(W):
                for c in range(C):
                    l = float(left[0, c, y, x]) if x >= d else 0.0
                    r = _bilinear_loop(right[0, c], y * H / (H - 1) - 0.5, (x - d) * W / (W - 1) - 0.5)
                    assert abs(float(vols["cor"][0, d, y, x, c]) - l * r) < 1e-12
                    assert abs(float(vols["ssd"][0, d, y, x, c]) - ((l * l + r * r) / 2 - ((l + r) / 2) ** 2)) < 1e-12
                    assert abs(float(vols["sum"][0, d, y, x, c]) - (l + r)) < 1e-12
                    assert float(vols["cat"][0, d, y, x, c]) == l
                    assert abs(float(vols["cat"][0, d, y, x, C + c]) - r) < 1e-12


@pytest.mark.parametrize("channels_last", [0, 1])
def test_pointwise_vs_a_loop(channels_last):
    g = _g(3 + channels_last)
    B, Ci, Co, P, ldw = 2, 3, 4, 5, 7
    x = torch.randn(B, P, Ci, generator=g, dtype=F64) if channels_last else torch.randn(B, Ci, P, generator=g, dtype=F64)
    w = torch.randn((Co - 1) * ldw + Ci, generator=g, dtype=F64)
    got = R.pointwise(x, w, ldw, channels_last)
    for b in range(B):
        for co in range(Co):
            for p in range(P):
                s = sum(float(w[co * ldw + ci]) * float(x[b, p, ci] if channels_last else x[b, ci, p]) for ci in range(Ci))
                assert abs(float(got[b, p, co] if channels_last else got[b, co, p]) - s) < 1e-12


@pytest.mark.parametrize("relu,res", [(1, 0), (0, 1), (1, 1)])
def test_conv3d_unit_vs_a_loop(relu, res):
    g = _g(relu * 2 + res)
    B, D, H, W, Ci, Co = 2, 2, 3, 2, 3, 2
    x = torch.randn(B, D, H, W, Ci, generator=g, dtype=F64)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=F64)
    s, h = torch.rand(Co, generator=g, dtype=F64) + 0.5, torch.randn(Co, generator=g, dtype=F64)
    r = torch.randn(B, D, H, W, Co, generator=g, dtype=F64) if res else None
    got = R.conv3d_unit(x, w, s, h, r, relu)
    for b in range(B):
        for d in range(D):
            for y in range(H):
                for xx in range(W):
                    for co in range(Co):
                        acc = 0.0
                        for kd in range(3):
                            for ky in range(3):
                                for kx in range(3):
                                    zd, zy, zx = d + kd - 1, y + ky - 1, xx + kx - 1
                                    if 0 <= zd < D and 0 <= zy < H and 0 <= zx < W:
                                        acc += float((x[b, zd, zy, zx] * w[co, :, kd, ky, kx]).sum())
                        v = acc * float(s[co]) + float(h[co])
                        v = max(v, 0.0) if relu else v
                        v += float(r[b, d, y, xx, co]) if res else 0.0
                        assert abs(float(got[b, d, y, xx, co]) - v) < 1e-12


def test_stack_wiring():
    """The residual of unit res_src lands on unit res_dst after its ReLU, as CostRegNetNoDown.forward adds o0."""
    g = _g(7)
    C = 3
    x = torch.randn(1, 3, 2, 4, C, generator=g, dtype=F64)
    layers = [(torch.randn(C, C, 3, 3, 3, generator=g, dtype=F64) * 0.3, torch.rand(C, generator=g, dtype=F64) + 0.5,
               torch.randn(C, generator=g, dtype=F64) * 0.1) for _ in range(7)]
    u = lambda i, t, res=None: torch.relu(R.conv3d_unit(t, *layers[i], None, False)) + (0 if res is None else res)
    o0_ = u(1, u(0, x))
    ref = u(6, u(5, u(4, u(3, u(2, o0_)), o0_)))
    _close(R.stack(x, layers, 7, 1, 4), ref)
    _close(R.stack(x, layers, 3), u(2, u(1, u(0, x))))
    o = u(0, x)
    _close(R.stack(x, layers, 3, 0, 1), u(2, u(1, o, o)))


def test_cout1_softargmax_and_regression_vs_a_loop():
    g = _g(9)
    B, D, H, W, Ci = 1, 3, 2, 2, 4
    x = torch.randn(B, D, H, W, Ci, generator=g, dtype=F64)
    w = torch.randn(1, Ci, 3, 3, 3, generator=g, dtype=F64)
    reg, pred = R.cout1_softargmax(x, w, 300.0, -2.0)                              # saturating scale
    ref = R.conv3d_unit(x, w, torch.tensor([300.0], dtype=F64), torch.tensor([-2.0], dtype=F64), None, False)[..., 0]
    _close(reg, ref)
    for y in range(H):
        for xx in range(W):
            c = [float(reg[0, d, y, xx]) for d in range(D)]
            m = max(c)
            e = [math.exp(v - m) for v in c]
            assert abs(float(pred[0, y, xx]) - sum(ei * d for d, ei in enumerate(e)) / sum(e)) < 1e-12
    samples = torch.tensor([3.0, -1.5, 3.0], dtype=F64).view(1, 3, 1, 1).expand(B, D, H, W)
    got = R.disparity_regression(reg, samples)
    _close(got, o0.disparity_regression(reg, samples))


def test_transposes_round_trip():
    x = torch.randn(2, 3, 4, 5, 6, generator=_g(1), dtype=F64)
    y = R.ncdhw_to_ndhwc(x)
    assert y.shape == (2, 4, 5, 6, 3) and float(y[1, 2, 3, 4, 0]) == float(x[1, 0, 2, 3, 4])
    assert torch.equal(R.ndhwc_to_ncdhw(y), x)


@pytest.mark.parametrize("cf", ["cor", "ssd", "cat"])
def test_stage0_vs_oracle(cf):
    """The whole branch against oracle/stage0.py's torch composition run in float64."""
    B, C, H, W, D = 1, 4, 3, 5, 7
    g = _g(21)
    left = torch.relu(torch.randn(B, C, H, W, generator=g, dtype=F64))
    right = torch.relu(torch.randn(B, C, H, W, generator=g, dtype=F64))
    params = o0.random_params(C, 3)
    p64 = [{"w": p["w"].double(), "bn": tuple(t.double() for t in p["bn"])} for p in params]
    w_pre = o0.random_w_pre(C, 3).double() if cf == "cat" else None
    pred_o, reg_o, _ = o0.stage0_forward(left, right, p64, D, cf, w_pre)
    reg, pred = R.stage0(left, right, _params64(params), D, cf, w_pre)
    _close(reg, reg_o, 1e-10)
    _close(pred, pred_o, 1e-10)


@pytest.mark.parametrize("name,cf", [("stage0_small.npz", "cor"), ("stage0_c216.npz", "cor"),
                                     ("stage0_ssd_small.npz", "ssd"), ("stage0_cat_small.npz", "cat")])
def test_goldens_of_the_reference_classes(golden_dir, name, cf):
    """The reference's own classes ran in float32: the volume within 1e-5, reg within 1e-4 * max|reg|, pred 1e-3 px."""
    d = np.load(os.path.join(golden_dir, name))
    left, right = torch.from_numpy(d["left"]), torch.from_numpy(d["right"])
    C, D = left.shape[1], int(d["max_disp"])
    if "w0" in d.files:                                                            # the weights the classes held
        params = [{"w": torch.from_numpy(d["w%d" % i]),
                   "bn": tuple(torch.from_numpy(d["bn%d_%s" % (i, k)]) for k in ("gamma", "beta", "mean", "var"))}
                  for i in range(8)]
    else:
        params = o0.random_params(C, int(d["param_seed"]))
    w_pre = torch.from_numpy(d["w_pre"]) if cf == "cat" else None
    cv = R.costvol(left, right, D, cf)
    _close(cv, torch.from_numpy(d["cost_vol"]).double().permute(0, 2, 3, 4, 1), 1e-5)
    reg, pred = R.stage0(left, right, _params64(params), D, cf, w_pre)
    _close(reg, torch.from_numpy(d["reg"]).double(), 1e-4)
    assert float((pred - torch.from_numpy(d["pred"]).double()).abs().max()) < 1e-3
