"""The float64 references of tests/_spamat_ref.py against independent formulations: explicit Python loops at tiny sizes,
the fp32 C restatement oracle/spamat_oracle.c (both FMA builds, within fp32 noise), the committed recordings of the
reference's own kernels (tests/golden/spamat_ref_*.npz), central finite differences of the forward, and the quirk answers
of the header.  So the GPU edge tests (tests/test_spamat_edges_gpu.py) compare the HIP entries with something that is
itself checked.  CPU only."""
import math

import numpy as np
import pytest
import torch

import _spamat_ref as R
import oracle
from test_spamat_ref import K, fixture, gd_tol, gscale, inputs

F64 = torch.float64


def _case(seed, B, C, H, W, pr=1.0, pt=1.0, relu=True, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    L = torch.randn(B, C, H, W, generator=g) * scale
    Rt = torch.randn(B, C, H, W, generator=g) * scale
    if relu:
        L, Rt = torch.relu(L), torch.relu(Rt)
    rm = (torch.rand(B, H, W, generator=g) < pr).float()
    tm = (torch.rand(B, H, W, generator=g) < pt).float()
    return L, Rt, rm, tm


def _loops(L, Rt, rm, tm, D, mu):
    """Plain per-pixel loops over the header's formulas (float64)."""
    B, C, H, W = L.shape
    L, Rt = L.double().numpy(), Rt.double().numpy()
    res = {k: np.zeros((B, H, W)) for k in ("out", "S", "max_cost", "var")}
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if rm[b, y, x] == 0:
                    continue
                cand = [(d, float(np.dot(L[b, :, y, x], Rt[b, :, y, x - d]))) for d in range(min(D, x + 1))
                        if tm[b, y, x - d] != 0]
                m = max([R.EPS] + [c for _, c in cand])
                S = R.EPS + sum(math.exp(c - m) for _, c in cand)
                res["out"][b, y, x] = (R.EPS + sum(math.exp(c - m) * d for d, c in cand)) / S
                res["var"][b, y, x] = (R.EPS + sum(math.exp(c - m) * (d - float(mu[b, y, x])) ** 2 for d, c in cand)) / S
                res["S"][b, y, x], res["max_cost"][b, y, x] = S, m
    return {k: torch.from_numpy(v) for k, v in res.items()}


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


@pytest.mark.parametrize("B,C,H,W,D,pr,pt,relu", [(1, 1, 1, 1, 1, 1.0, 1.0, True), (2, 3, 2, 7, 5, 1.0, 0.5, False),
                                                   (1, 4, 1, 9, 20, 0.7, 0.7, False), (3, 2, 1, 6, 2, 1.0, 1.0, True)])
def test_forward_matches_explicit_loops(B, C, H, W, D, pr, pt, relu):
    L, Rt, rm, tm = _case(B * 1000 + W * 10 + D, B, C, H, W, pr, pt, relu)
    mu = torch.randn(B, H, W, generator=torch.Generator().manual_seed(1)) * 3
    got = R.forward(L, Rt, rm, tm, D, disparity=mu)
    want = _loops(L, Rt, rm, tm, D, mu.double())
    for k in ("out", "S", "max_cost", "var"):
        _close(got[k], want[k])
    self_var = _loops(L, Rt, rm, tm, D, got["out"])["var"]
    _close(got["var_self"], self_var)


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("B,C,H,W,D,pr,pt,relu,scale", [(2, 8, 3, 300, 216, 0.6, 0.6, True, 1.0),
                                                         (1, 24, 2, 81, 72, 0.9, 0.9, False, 0.5),
                                                         (1, 72, 2, 27, 24, 0.5, 0.5, True, 1.0),
                                                         (1, 5, 2, 40, 60, 1.0, 1.0, False, 0.5)])
def test_matches_the_fp32_oracle(fma, B, C, H, W, D, pr, pt, relu, scale):
    L, Rt, rm, tm = _case(7 + C + W, B, C, H, W, pr, pt, relu, scale)
    g = torch.randn(B, H, W, generator=torch.Generator().manual_seed(2))
    o, s, m = oracle.spamat_forward(L, Rt, rm, tm, D, fma=fma)
    mu = torch.from_numpy(o) + torch.randn(B, H, W, generator=torch.Generator().manual_seed(3))
    v, _, _ = oracle.spavar_forward(L, Rt, rm, tm, mu, D, fma=fma)
    r = R.forward(L, Rt, rm, tm, D, disparity=mu)
    np.testing.assert_allclose(m, r["max_cost"].numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(s, r["S"].numpy(), rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(o, r["out"].numpy(), rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(v, r["var"].numpy(), rtol=2e-4, atol=2e-3)
    gl, gr = oracle.spamat_backward(L, Rt, rm, tm, o, s, m, g, D, fma=fma)
    rl, rr = R.backward(L, Rt, rm, tm, o, s, m, g, D)
    sc = gscale(rl.numpy(), rr.numpy())
    assert np.abs(gl - rl.numpy()).max() < 5e-5 * sc and np.abs(gr - rr.numpy()).max() < 5e-5 * sc
    vl, vr, vd = oracle.spavar_backward(L, Rt, rm, tm, mu, v, s, m, g, D, fma=fma)
    ql, qr, qd = R.backward(L, Rt, rm, tm, v, s, m, g, D, disparity=mu)
    sc = gscale(ql.numpy(), qr.numpy())
    assert np.abs(vl - ql.numpy()).max() < 5e-5 * sc and np.abs(vr - qr.numpy()).max() < 5e-5 * sc
    assert np.abs(vd - qd.numpy()).max() < 5e-5 * gscale(qd.numpy()) + 2.0 ** -22 * D * float(g.abs().max())


@pytest.mark.parametrize("name", K.all_names())
def test_matches_the_reference_kernels_recordings(name):
    fx = fixture(name)
    x = inputs(name, fx)
    D = x["max_disp"]
    r = R.forward(x["L"], x["R"], x["rm"], x["tm"], D)
    np.testing.assert_allclose(r["max_cost"].numpy(), fx["mx"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(r["S"].numpy(), fx["ssum"], rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(r["out"].numpy(), fx["out"], rtol=1e-5, atol=2e-4)
    gl, gr = R.backward(x["L"], x["R"], x["rm"], x["tm"], fx["out"], fx["ssum"], fx["mx"], x["g"], D)
    sc = gscale(fx["gl"], fx["gr"])
    assert np.abs(gl.numpy() - fx["gl"]).max() < 5e-5 * sc and np.abs(gr.numpy() - fx["gr"]).max() < 5e-5 * sc
    for tag, mu in (("v0", fx["out"]), ("v1", fx["out"] + x["mu_noise"])):
        r = R.forward(x["L"], x["R"], x["rm"], x["tm"], D, disparity=mu)
        v = r["var"]
        np.testing.assert_allclose(v.numpy(), fx[tag + "_var"], rtol=2e-4, atol=2e-3)
        ql, qr, qd = R.backward(x["L"], x["R"], x["rm"], x["tm"], fx[tag + "_var"], fx[tag + "_ssum"], fx[tag + "_mx"],
                                x["g"], D, disparity=mu)
        sc = gscale(fx[tag + "_gl"], fx[tag + "_gr"])
        assert np.abs(ql.numpy() - fx[tag + "_gl"]).max() < 5e-5 * sc
        assert np.abs(qr.numpy() - fx[tag + "_gr"]).max() < 5e-5 * sc
        # the recording's own fp32 noise: cost errors of ~eps A_d move sum_d e_d (d - mu) by ~eps k_out S
        noise = 2.0 ** -22 * 2 * float((np.abs(x["g"]) * r["k_out"].numpy()).max())
        assert np.abs(qd.numpy() - fx[tag + "_gd"]).max() < gd_tol(fx, tag, x) + noise


@pytest.mark.parametrize("var", [False, True])
def test_backward_matches_central_differences(var):
    """The backward with out / S / max_cost from the float64 forward equals the derivative of that forward with max_cost
    held constant (S7): central differences of the loss sum(g * out) at a fixed max_cost."""
    B, C, H, W, D = 1, 3, 2, 9, 6
    L, Rt, rm, tm = (t.double() for t in _case(11, B, C, H, W, 0.8, 0.8, relu=False, scale=0.7))
    g = torch.randn(B, H, W, generator=torch.Generator().manual_seed(4), dtype=F64)
    mu = torch.randn(B, H, W, generator=torch.Generator().manual_seed(5), dtype=F64) + 2
    f0 = R.forward(L, Rt, rm, tm, D, disparity=mu)
    m0 = f0["max_cost"]

    def loss(L_, R_, mu_):
        cost, _, valid = R._planes(L_, R_, rm, tm, D)
        e = torch.where(valid, torch.exp(cost - m0), torch.zeros_like(cost))
        d = R._dvec(cost.shape[0])
        S = R.EPS + e.sum(0)
        q = (R.EPS + (e * ((d - mu_) ** 2 if var else d)).sum(0)) / S
        return float((g * torch.where(R.mask_on(rm), q, torch.zeros_like(q))).sum())

    out = f0["var"] if var else f0["out"]
    grads = R.backward(L, Rt, rm, tm, out, f0["S"], m0, g, D, disparity=mu if var else None)
    h = 1e-6
    for which, (x0, gx) in enumerate(zip((L, Rt) + ((mu,) if var else ()), grads)):
        fd = torch.zeros_like(x0)
        for i in range(x0.numel()):
            xp, xm = x0.clone(), x0.clone()
            xp.view(-1)[i] += h
            xm.view(-1)[i] -= h
            args = [L, Rt, mu]
            args[which] = xp
            lp = loss(*args)
            args[which] = xm
            fd.view(-1)[i] = (lp - loss(*args)) / (2 * h)
        _close(gx, fd, 1e-7)
    assert float(grads[0].abs().max()) > 0.01 and float(grads[1].abs().max()) > 0.01


def test_quirk_answers():
    """ref-off -> 0 everywhere; no valid candidate -> out = var = 1.0, S = max_cost = EPS; every cost below the floor ->
    max_cost = EPS; -0.0 is off, a denormal (1e-45), -1, 0.5 and 3e38 are on."""
    B, C, H, W, D = 1, 2, 1, 8, 5
    L = torch.full((B, C, H, W), 0.5)
    Rt = torch.full((B, C, H, W), -0.5)                       # every cost -0.5 < EPS
    rm = torch.tensor([[[0.0, 1, 1, 1, 1, 1, 1, 1]]])
    tm = torch.tensor([[[1.0, -0.0, 1e-45, -1, 0.5, 3e38, 0, 0]]])
    assert float(tm[0, 0, 2]) != 0, "the denormal survived float32"
    r = R.forward(L, Rt, rm, tm, D, disparity=torch.zeros(B, H, W))
    assert float(r["out"][0, 0, 0]) == 0 and float(r["S"][0, 0, 0]) == 0 and float(r["max_cost"][0, 0, 0]) == 0
    assert bool((r["max_cost"][0, 0, 1:] == R.EPS).all())
    on = R.mask_on(tm)[0, 0].tolist()
    assert on == [True, False, True, True, True, True, False, False]
    cost, _, valid = R._planes(L, Rt, rm, tm, D)
    for x in range(1, W):
        n = sum(on[x - d] for d in range(min(D, x + 1)))
        assert int(valid[:, 0, 0, x].sum()) == n
    # x = 1: candidates d = 0 (tar x 1: -0.0, off) and d = 1 (tar x 0: on) -> one candidate at d = 1
    e = math.exp(-0.5 - R.EPS)
    assert abs(float(r["out"][0, 0, 1]) - (R.EPS + e) / (R.EPS + e)) < 1e-15
    # no valid candidate: x = 7 at D = 1 sees tar x 7 (off)
    r1 = R.forward(L, Rt, rm, tm, 1, disparity=torch.full((B, H, W), 3.0))
    assert float(r1["out"][0, 0, 7]) == 1.0 and float(r1["var"][0, 0, 7]) == 1.0 and float(r1["var_self"][0, 0, 7]) == 1.0
    assert float(r1["S"][0, 0, 7]) == R.EPS and float(r1["max_cost"][0, 0, 7]) == R.EPS
    assert float(r1["k_out"][0, 0, 7]) == 0 and float(r1["k_max"][0, 0, 7]) == 0
    # ref off: no gradient from a nonzero grad_output there, and no gradient into an off right pixel
    g = torch.ones(B, H, W)
    gl, gr = R.backward(L, Rt, rm, tm, r["out"], r["S"], r["max_cost"], g, D)
    assert float(gl[..., 0].abs().max()) == 0 and float(gr[..., 1].abs().max()) == 0 and float(gr[..., 6:].abs().max()) == 0
    assert float(gl.abs().max()) > 0


def test_all_zero_features_give_the_flat_softmax_in_closed_form():
    """cost 0 everywhere: max_cost = EPS, e_d = exp(-EPS), out = (EPS + e n (n - 1) / 2) / (EPS + e n), n = min(D, x + 1)."""
    B, C, H, W, D = 1, 3, 1, 40, 17
    z = torch.zeros(B, C, H, W)
    ones = torch.ones(B, H, W)
    r = R.forward(z, z, ones, ones, D)
    e = math.exp(-R.EPS)
    for x in range(W):
        n = min(D, x + 1)
        assert abs(float(r["out"][0, 0, x]) - (R.EPS + e * n * (n - 1) / 2) / (R.EPS + e * n)) < 1e-12
        assert float(r["k_out"][0, 0, x]) == 0
