"""CPU half of the tail gradients (decnet_amd/tail_grad.py, csrc/tail_grad.hip):
  1. the float64 restatements of tests/_tail_grad_ref.py equal torch's own float64 autograd of F.grid_sample (the warp as
     model.warp_by_disparity builds it), of _trunk_ref.dynamic_upsample3, of _trunk_ref.unfold3_cat and of
     dense (1 - sigmoid(o)) + sigmoid(o) sparse to 1e-12 relative -- formulas, sign and the W / (W - 1) factor;
  2. the route predicates of model.py, row by row;
  3. CPU tensors under hip_grad() never reach the library, and model.TALLY is what it was."""
import types

import pytest
import torch
import torch.nn.functional as F

import _tail_grad_ref as TR
import _trunk_ref as R

D = torch.float64
RTOL = 1e-12


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= RTOL * max(1.0, float(ref.abs().max())), (what, err)


def _away_from_integers(B, H, W, g):
    """Disparities over [-W/2, 3W/2) (taps off both sides) whose float64 ix is at least 1e-3 away from every integer."""
    disp = torch.rand(B, H, W, generator=g, dtype=D) * 2 * W - W / 2
    for _ in range(20):
        ix, _ = R.warp_coords(disp, H, W, D)
        bad = (ix - torch.round(ix)).abs() < 1e-3
        if not bool(bad.any()):
            return disp
        disp = torch.where(bad, disp + 0.01, disp)
    raise AssertionError("no disparity plane away from the integers")


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 2, 2), (2, 3, 2, 5), (2, 9, 3, 17), (1, 2, 5, 33)])
def test_warp_restatement_is_grid_sample_autograd(B, C, H, W):
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + W)
    right = torch.randn(B, C, H, W, generator=g, dtype=D).requires_grad_()
    disp = _away_from_integers(B, H, W, g).requires_grad_()
    gout = torch.randn(B, C, H, W, generator=g, dtype=D)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D), torch.arange(W, dtype=D), indexing="ij")
    cx = (xs.unsqueeze(0) - disp) / ((W - 1.0) / 2.0) - 1.0
    cy = (ys / ((H - 1.0) / 2.0) - 1.0).unsqueeze(0).expand_as(cx)
    out = F.grid_sample(right, torch.stack((cx, cy), 3), mode="bilinear", padding_mode="zeros", align_corners=False)
    gr, gd = torch.autograd.grad(out, (right, disp), gout)
    ref = TR.warp_backward(right, disp, gout, coord_dtype=D)
    _close(ref["g_right"], gr, "g_right")
    _close(ref["g_disp"], gd, "g_disp")
    assert bool((ref["A_right"] >= ref["g_right"].abs() * (1 - 1e-12)).all())
    assert bool((ref["A_disp"] >= ref["g_disp"].abs() * (1 - 1e-12)).all())
    assert float(ref["n_right"].max()) >= 1 and float(ref["n_right"].sum()) <= 4 * B * C * H * W
    assert float(gd.abs().max()) > 0 and float(gr.abs().max()) > 0


def test_all_outside_disparities_give_zero_gradients():
    g = torch.Generator().manual_seed(3)
    right, gout = torch.randn(1, 2, 3, 5, generator=g), torch.randn(1, 2, 3, 5, generator=g)
    ref = TR.warp_backward(right, torch.full((1, 3, 5), 1e6), gout)
    for k in ("g_right", "g_disp", "A_right", "A_disp", "n_right"):
        assert float(ref[k].abs().max()) == 0.0, k


@pytest.fixture
def differentiable_trunk_ref(monkeypatch):
    """_trunk_ref promotes its inputs with detach(); for autograd through its formulas, without."""
    monkeypatch.setattr(R, "_d", lambda t: t.to("cpu", D))


@pytest.mark.parametrize("B,h,w,spread", [(1, 1, 1, 3.0), (2, 1, 4, 3.0), (2, 3, 1, 0.0), (2, 4, 5, 8.0)])
def test_upsample_restatement_is_autograd(differentiable_trunk_ref, B, h, w, spread):
    g = torch.Generator().manual_seed(B * 100 + h * 10 + w)
    logits = ((torch.rand(B, 81, h, w, generator=g, dtype=D) * 2 - 1) * spread).requires_grad_()
    disp = (torch.rand(B, h, w, generator=g, dtype=D) * 50 - 10).requires_grad_()
    gout = torch.randn(B, 3 * h, 3 * w, generator=g, dtype=D)
    gl, gd = torch.autograd.grad(R.dynamic_upsample3(logits, disp), (logits, disp), gout)
    ref = TR.upsample3_backward(logits, disp, gout)
    _close(ref["g_logits"], gl, "g_logits")
    _close(ref["g_disp"], gd, "g_disp")
    assert bool((ref["A_logits"] >= ref["g_logits"].abs() * (1 - 1e-12)).all())
    assert bool((ref["A_disp"] >= ref["g_disp"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("B,C,h,w", [(2, 2, 5, 7), (1, 3, 1, 4), (2, 1, 3, 1)])
def test_fold3_restatement_is_autograd(differentiable_trunk_ref, B, C, h, w):
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w)
    fea = torch.randn(B, C, 3 * h, 3 * w, generator=g, dtype=D).requires_grad_()
    disp = torch.randn(B, h, w, generator=g, dtype=D).requires_grad_()
    gout = torch.randn(B, 9 * C + 1, h, w, generator=g, dtype=D)
    gf, gd = torch.autograd.grad(R.unfold3_cat(fea, disp), (fea, disp), gout)
    rf, rd = TR.unfold3_cat_backward(gout)
    assert torch.equal(rf, gf) and torch.equal(rd, gd)
    assert torch.equal(TR.fold3(R.unfold3_cat(fea, disp).detach()), fea.detach())


def test_blend_restatement_is_autograd():
    g = torch.Generator().manual_seed(11)
    o = torch.cat((torch.rand(200, generator=g, dtype=D) * 60 - 30, torch.tensor([100.0, -100.0], dtype=D))).requires_grad_()
    a = (torch.rand(202, generator=g, dtype=D) * 4).requires_grad_()
    b = (torch.rand(202, generator=g, dtype=D) * 4).requires_grad_()
    gout = torch.randn(202, generator=g, dtype=D)
    s = torch.sigmoid(o)
    go, ga, gb = torch.autograd.grad(a * (1 - s) + s * b, (o, a, b), gout)
    ref = TR.blend_backward(o, a, b, gout)
    _close(ref["g_o"], go, "g_o")
    _close(ref["g_a"], ga, "g_a")
    _close(ref["g_b"], gb, "g_b")
    assert float(ref["g_o"][-2:].abs().max()) < 1e-40 and not bool(torch.isnan(ref["g_o"]).any())


# ---- 2. routes -------------------------------------------------------------------------------------------------------------
def _fake(cuda=True, dtype=torch.float32):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype)


def test_gate_rows():
    import decnet_amd
    from decnet_amd import model
    gpu, cpu, half = _fake(), _fake(cuda=False), _fake(dtype=torch.float16)
    assert not model.tail_grad_gate(gpu)                                  # hip_grad() off
    with decnet_amd.hip_grad():
        assert model.tail_grad_gate(gpu) and model.tail_grad_gate(gpu, gpu)
        assert not model.tail_grad_gate(cpu) and not model.tail_grad_gate(gpu, cpu)
        assert not model.tail_grad_gate(half) and not model.tail_grad_gate(_fake(dtype=D))
        with torch.no_grad():
            assert not model.tail_grad_gate(gpu)                          # autograd off: the inference route
        with decnet_amd.hip_grad(False):
            assert not model.tail_grad_gate(gpu)
    assert not model.tail_grad_gate(gpu)


def test_shape_rows(monkeypatch):
    from decnet_amd import model
    r = model.tail_grad_route
    for env in ("hip", "library"):                                        # decided with the switches at their defaults
        monkeypatch.setenv("DECNET_CONV2D", env)
        assert r("warp", 1, 8, 2, 2) and r("warp", 4, 8, 540, 972) and r("warp", 1, 1, 65535, 2)
        assert not r("warp", 1, 8, 1, 9) and not r("warp", 1, 8, 9, 1) and not r("warp", 1, 1, 65536, 2)
        assert r("unfold", 4, 8, 180, 324, 3, (540, 972)) and r("unfold", 1, 1, 1, 1, 3, (3, 3))
        assert not r("unfold", 4, 8, 180, 324, 2, (360, 648))             # s == 3 only
        assert not r("unfold", 4, 8, 180, 324, 3, (541, 972)) and not r("unfold", 4, 8, 180, 324, 3, (540, 973))
        assert r("unfold", 1, 1, 65535, 1, 3, (196605, 3)) and not r("unfold", 1, 1, 65536, 1, 3, (196608, 3))
        assert r("unfold", 7, 9361, 2, 2, 3, (6, 6)) and not r("unfold", 7, 9362, 2, 2, 3, (6, 6))     # B (C + 1) <= 65535
        assert r("upsample", 4, 81, 180, 324) and r("upsample", 1, 81, 65535, 1)
        assert not r("upsample", 1, 81, 65536, 1) and not r("upsample", 4, 81, 180, 324, 2)
    with pytest.raises(ValueError):
        r("blend", 1, 1, 2, 2)


def test_fuse_route_rows():
    from decnet_amd.model import SoftAttention
    full = SoftAttention(12, 8)                                           # stage 3: 8 + 4 inputs, few-channel units
    assert full._fuse_grad_route(1, 16, 18) and full._fuse_grad_route(4, 540, 972)
    assert not full._fuse_grad_route(1, 15, 17)                           # below 256 pixels: Unit._grad_route's floor
    coarse = SoftAttention(76, 8)                                         # 72 + 4 inputs: the matrix-core first layer
    assert not coarse._fuse_grad_route(1, 64, 64) and not coarse._fuse_grad_route(1, 16, 18)


# ---- 3. CPU tensors under hip_grad() ------------------------------------------------------------------------------------------
def test_cpu_modules_under_hip_grad_never_reach_the_library(monkeypatch):
    import decnet_amd
    import _conv2d_grad_ref as GR
    from decnet_amd import _lib, model, ops

    def no_library(*a):
        raise AssertionError("a CPU tensor reached the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(ops, "_FN", {})
    monkeypatch.setattr(model, "TALLY", [])
    outs = {}
    for name in sorted(GR.MODULE_SEEDS):
        m, ins, wrt, r = GR.module_case(name)
        plain = GR.module_out(name, m, ins)
        t = {k: v.clone().requires_grad_(k in ("disp", "right", "dense", "sparse")) for k, v in ins.items()}
        del model.TALLY[:]
        with decnet_amd.hip_grad():
            out = GR.module_out(name, m, t)
        outs[name] = [e["family"] for e in model.TALLY]
        (out * r).sum().backward()
        assert torch.equal(out.detach(), plain.detach())
        assert all(t[k].grad is not None for k in t if t[k].requires_grad)
    assert outs == {"refinement": ["library"] * 7, "attention": ["library"] * 3}
    up = model.DynamicUpsampling(2, 3).eval()
    disp, fea = torch.rand(1, 5, 7).requires_grad_(), torch.randn(1, 2, 15, 21).requires_grad_()
    with decnet_amd.hip_grad():
        up(disp, fea).sum().backward()
    assert disp.grad is not None and fea.grad is not None


def test_functions_are_exported():
    import decnet_amd
    from decnet_amd import tail_grad
    for n in ("WarpDisparityFunction", "DynamicUpsample3Function", "Unfold3CatFunction", "SigmoidBlendFunction"):
        assert getattr(decnet_amd, n) is getattr(tail_grad, n) and n in decnet_amd.__all__
