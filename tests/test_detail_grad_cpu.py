"""CPU half of the detail maps and soft masks under hip_grad() (csrc/detail_grad.hip, decnet_amd/tail_grad.py,
GenerateSparseMask.detail, SoftAttention.fuse(want_soft=True)):
  1. the six entries are bound, refuse bad arguments before any launch, and their Functions are exported;
  2. the route predicates, row by row;
  3. CPU tensors never reach the library: the Functions refuse them, the modules take their torch routes;
  4. what tests/test_detail_grad_gpu.py relies on about its cases (tests/_detail_ref.py): the threshold rule, the 1 % cap
     of excused pixels on the float64 reference alone, the margin search, live gradients;
  5. the formulas the kernels restate are torch's."""
import ctypes

import pytest
import torch

import _detail_ref as DR
import _model_cases as MC

D = torch.float64
ENTRIES = ("decnet_sqdiff", "decnet_sqdiff_backward", "decnet_detail_tail", "decnet_detail_tail_backward",
           "decnet_sigmoid_blend_soft", "decnet_sigmoid_blend_soft_backward")
FUNCTIONS = ("SquaredDiffFunction", "DetailTailFunction", "SigmoidBlendSoftFunction")


# ---- 1. the boundary ---------------------------------------------------------------------------------------------------------
def test_entries_are_bound_and_functions_exported():
    import decnet_amd
    from decnet_amd import _lib, ops2d, tail_grad
    for e in ENTRIES:
        assert e in _lib.SIGNATURES and hasattr(ops2d, e[len("decnet_"):]), e
    for n in FUNCTIONS:
        assert getattr(decnet_amd, n) is getattr(tail_grad, n) and n in decnet_amd.__all__


def test_refusals_come_before_any_launch():
    """Every refusal without a GPU: fake addresses, so a launch (or a read of one of them) could not go unnoticed."""
    from decnet_amd import _lib, build
    h = ctypes.CDLL(build.build())
    for e in ENTRIES:
        getattr(h, e).argtypes = _lib.SIGNATURES[e]
    p, N, n = ctypes.c_void_p(64), None, 5
    NULL, SHAPE, UNSUP = -1, -2, -3
    big = (1 << 40) + 1
    assert h.decnet_sqdiff(N, p, p, n, N) == NULL and h.decnet_sqdiff(p, N, p, n, N) == NULL
    assert h.decnet_sqdiff(p, p, N, n, N) == NULL
    assert h.decnet_sqdiff(p, p, p, 0, N) == SHAPE and h.decnet_sqdiff(p, p, p, big, N) == UNSUP
    assert h.decnet_sqdiff_backward(N, p, p, p, p, n, N) == NULL and h.decnet_sqdiff_backward(p, p, N, p, p, n, N) == NULL
    assert h.decnet_sqdiff_backward(p, p, p, N, N, n, N) == NULL
    assert h.decnet_sqdiff_backward(p, p, p, p, N, 0, N) == SHAPE and h.decnet_sqdiff_backward(p, p, p, N, p, big, N) == UNSUP
    tail = h.decnet_detail_tail
    assert tail(N, 0.5, p, p, p, 1, 2, 3, N) == NULL and tail(p, 0.5, N, N, N, 1, 2, 3, N) == NULL
    assert tail(p, 0.5, p, p, p, 0, 2, 3, N) == SHAPE and tail(p, 0.5, p, p, p, 1, 0, 3, N) == SHAPE
    assert tail(p, 0.5, p, p, p, 1, 2, 0, N) == SHAPE
    assert tail(p, 0.5, p, p, p, 65536, 2, 3, N) == SHAPE and tail(p, 0.5, p, p, p, 1, 65536, 3, N) == SHAPE   # as decnet_detail_mask
    assert tail(p, 0.5, p, p, p, 1, 2, (1 << 28) + 1, N) == UNSUP
    assert tail(p, 0.5, p, p, p, 65535, 65535, 1024, N) == UNSUP            # 4.3e9 workgroups
    assert h.decnet_detail_tail_backward(N, p, p, n, N) == NULL and h.decnet_detail_tail_backward(p, N, p, n, N) == NULL
    assert h.decnet_detail_tail_backward(p, p, N, n, N) == NULL
    assert h.decnet_detail_tail_backward(p, p, p, 0, N) == SHAPE and h.decnet_detail_tail_backward(p, p, p, big, N) == UNSUP
    soft = h.decnet_sigmoid_blend_soft
    for i in range(5):
        assert soft(*[N if j == i else p for j in range(5)], n, N) == NULL, i
    assert soft(p, p, p, p, p, 0, N) == SHAPE and soft(p, p, p, p, p, big, N) == UNSUP
    bwd = h.decnet_sigmoid_blend_soft_backward
    for i in (0, 1, 2, 5):                                                  # o, a, b, g_o
        assert bwd(*[N if j == i else p for j in range(8)], n, N) == NULL, i
    assert bwd(p, p, p, N, N, p, p, p, n, N) == NULL                        # neither gradient
    assert bwd(p, p, p, p, N, p, N, N, 0, N) == SHAPE and bwd(p, p, p, N, p, p, N, N, big, N) == UNSUP


# ---- 2. routes -------------------------------------------------------------------------------------------------------------------
def test_route_rows(monkeypatch):
    from decnet_amd import model
    r = model.tail_grad_route
    for env in ("hip", "library"):                                          # pure functions of sizes
        monkeypatch.setenv("DECNET_CONV2D", env)
        assert r("sqdiff", 4, 3, 540, 972) and r("sqdiff", 1, 1, 1, 1) and r("sqdiff", 1, 1, 1 << 20, 1 << 20)
        for op, C in (("sqdiff", 3), ("detail", 1)):                        # measured slower eager: model._detail_slower
            assert not r(op, 4, C, 60, 108) and not r(op, 4, C, 180, 324) and not r(op, 1, C, 1, 2099519)
            assert r(op, 1, C, 1, 25919) and r(op, 1, C, 1, 2099520) and r(op, 2, C, 3, 1026)
        assert not r("sqdiff", 1, 2, 1 << 20, 1 << 20) and not r("sqdiff", 0, 3, 4, 4)
        assert r("detail", 4, 1, 540, 972) and r("detail", 1, 1, 1, 1) and r("detail", 65535, 1, 1, 33)
        assert r("detail", 1, 1, 65535, 1024) and r("detail", 1, 1, 1, 1 << 28)
        assert not r("detail", 65536, 1, 1, 33) and not r("detail", 1, 1, 65536, 33)
        assert not r("detail", 1, 1, 1, (1 << 28) + 1) and not r("detail", 0, 1, 2, 2)
        assert r("detail", 30518, 1, 65535, 1024) and not r("detail", 30519, 1, 65535, 1024)      # B H ceil(W/1024) < 2e9
        assert not r("detail", 30518, 1, 65535, 1025)


# ---- 3. CPU tensors ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from decnet_amd import _lib, ops

    def refuse(*a):
        raise AssertionError("a CPU tensor reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(ops, "_FN", {})


def test_functions_refuse_cpu_tensors_before_any_lookup(no_library):
    import decnet_amd
    x = torch.zeros(2, 3, 5, requires_grad=True)
    with pytest.raises(decnet_amd.DecnetHipError):
        decnet_amd.SquaredDiffFunction.apply(x, x)
    with pytest.raises(decnet_amd.DecnetHipError):
        decnet_amd.DetailTailFunction.apply(x, 0.5, True)
    with pytest.raises(decnet_amd.DecnetHipError):
        decnet_amd.SigmoidBlendSoftFunction.apply(x, x, x)


@pytest.mark.parametrize("mode", DR.MODES)
def test_cpu_modules_take_the_torch_route(no_library, mode):
    import decnet_amd
    c = DR.value_case(6, 66, mode)
    gen = DR.copy_of(c["gen"], mode, torch.float32)
    plain = DR.copy_of(c["gen"], mode, torch.float32)
    cur, pre = c["cur"].clone().requires_grad_(), c["pre"].clone().requires_grad_()
    with decnet_amd.hip_grad():
        prob, mask, bits = gen.detail(cur, pre, c["thold"], want_bits=True)
    ref = torch.sigmoid(plain(c["cur"], c["pre"]))
    assert torch.equal(prob.detach(), ref.detach()) and prob.grad_fn is not None
    assert torch.equal(mask, (ref.detach() > c["thold"]).float()) and not mask.requires_grad and bits is None
    assert torch.equal(mask, DR.copy_of(c["gen"], mode, torch.float32).mask(c["cur"], c["pre"], c["thold"]).detach())
    with torch.no_grad():
        p2, m2, b2 = DR.copy_of(c["gen"], mode, torch.float32).detail(c["cur"], c["pre"], c["thold"])
    assert torch.equal(p2, ref.detach()) and torch.equal(m2, mask) and b2 is None and not p2.requires_grad
    prob.sum().backward()
    assert cur.grad is not None and pre.grad is not None
    m, ins, wrt, r1, r2, _ = DR.fuse_case(mode)
    a, b = DR.copy_of(m, mode, torch.float32), DR.copy_of(m, mode, torch.float32)
    args = [ins[k] for k in ("fea", "dense", "sparse", "mask", "var")]
    with decnet_amd.hip_grad():
        fused, soft = a.fuse(*args, want_soft=True)
        alone = b.fuse(*args)
    assert torch.equal(fused, alone)
    s = DR.copy_of(m, mode, torch.float32)(torch.cat((ins["fea"], ins["dense"].unsqueeze(1), ins["sparse"].unsqueeze(1),
                                                      ins["mask"].unsqueeze(1), -ins["var"].unsqueeze(1)), 1)).squeeze(1)
    assert torch.equal(soft, s) and torch.equal(fused, ins["dense"] * (1 - s) + s * ins["sparse"])


# ---- 4. the cases of the GPU test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_threshold_rule_is_mask_cases(H, W):
    c = DR.value_case(H, W, "eval")
    assert MC.mask_case(H, W)[3] == c["thold"]
    assert abs(DR.thold_of(c["logit64"]) - c["thold"]) <= 1e-12             # (_model_ref's formulas against the module's route)
    t = DR.value_case(H, W, "train")
    assert 0.0 < t["thold"] < 1.0 and not torch.equal(t["logit64"], c["logit64"])     # batch statistics: another run


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_float64_reference_alone_stays_within_the_cap(H, W, mode):
    c = DR.value_case(H, W, mode)
    u = DR.unsure(c)
    print((H, W), mode, "thold %.6f  logit bound %.3g  excused %d of %d" % (c["thold"], c["bound"], int(u.sum()), u.numel()))
    assert int(u.sum()) <= DR.CAP * u.numel()
    on = torch.sigmoid(c["logit64"]) > c["thold"]
    assert 0.3 < float(on.double().mean()) < 0.7                            # the median rule: both decisions occur


@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_margin_search_succeeds(H, W):
    import _bn_train_ref as BR
    found = [(k, bad) for k, _, _, bad in DR.variants(H, W)]
    print((H, W), "offending pixels per variant:", found)
    gen, cur, pre, k = DR.grad_data(H, W)
    assert k is not None and k == min(v for v, bad in found if bad == 0)
    for p in DR.relu_pre(gen, cur, pre):
        assert float(p.abs().min()) > BR.MARGIN * max(1.0, float(p.abs().max()))
    raw = MC.mask_case(H, W)
    assert (k == 0) == (torch.equal(cur, raw[1]) and torch.equal(pre, raw[2]))
    changed = int((cur != raw[1]).any(1).sum()) + int((pre != raw[2]).any(1).sum())
    assert changed <= 0.01 * cur[:, 0].numel()                             # a repair, not another case


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W", DR.SHAPES)
def test_gradient_cases_are_live(H, W, mode):
    c = DR.grad_case(H, W, mode)
    names = {n for n, _ in c["gen"].named_parameters()} | {"cur", "pre"}
    assert set(c["g64"]) == names == set(c["g32"])
    for n, g in c["g64"].items():
        assert float(g.abs().max()) > 0.0, n
    if mode == "train":                                                     # one step moved every BatchNorm's statistics
        before = dict(c["gen"].named_buffers())
        for n, b in c["buf64"].items():
            assert not torch.equal(b, before[n].to(b.dtype)), n


@pytest.mark.parametrize("mode", DR.MODES)
def test_fuse_case_clears_the_margin(mode):
    import _bn_train_ref as BR
    found = [(k, bad) for k, _, bad in DR.fuse_variants(mode)]
    print(mode, "offending pixels per variant:", found)
    m, ins, wrt, r1, r2, k = DR.fuse_case(mode)
    assert k is not None and k == min(v for v, bad in found if bad == 0) and (mode != "train" or k == 0)
    pres = DR.fuse_pre(m, ins, mode)
    assert sorted(pres) == ["0", "1"]
    for p in pres.values():
        assert float(p.abs().min()) > BR.MARGIN * max(1.0, float(p.abs().max()))
    raw = BR.module_case("attention")[1]
    assert all(torch.equal(ins[n], raw[n]) for n in raw if n != "fea")
    assert int((ins["fea"] != raw["fea"]).any(1).sum()) <= 0.05 * raw["dense"].numel()      # a repair, not another case
    for r1_ in (r1, None):                                                  # both losses of the GPU test: live gradients
        g64 = DR.fuse_grads(m, ins, wrt, r1_, r2, mode, D)[0]
        assert set(g64) == {n for n, _ in m.named_parameters()} | set(wrt)
        assert all(float(g.abs().max()) > 0.0 for g in g64.values())


# ---- 5. the formulas ---------------------------------------------------------------------------------------------------------------
def test_sqdiff_backward_statements_are_torch_autograd_bits():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1025, generator=g).requires_grad_(), torch.randn(1025, generator=g).requires_grad_()
    gout = torch.randn(1025, generator=g)
    d = a - b
    ga, gb = torch.autograd.grad(d * d, (a, b), gout)
    t = gout * d.detach()
    assert torch.equal(ga, t + t) and torch.equal(gb, -(t + t))


def test_blend_soft_backward_formula_is_autograd():
    g = torch.Generator().manual_seed(6)
    o = torch.cat((torch.rand(200, generator=g, dtype=D) * 60 - 30, torch.tensor([200.0, -200.0], dtype=D))).requires_grad_()
    a = (torch.rand(202, generator=g, dtype=D) * 4).requires_grad_()
    b = (torch.rand(202, generator=g, dtype=D) * 4).requires_grad_()
    gout, gsoft = torch.randn(202, generator=g, dtype=D), torch.randn(202, generator=g, dtype=D)
    s = torch.sigmoid(o)
    go, ga, gb = torch.autograd.grad((a * (1 - s) + s * b, s), (o, a, b), (gout, gsoft))
    sd = s.detach()
    ref = (gout * (b - a) + gsoft) * (sd * (1 - sd))
    assert float((ref.detach() - go).abs().max()) <= 1e-12 * max(1.0, float(go.abs().max()))
    assert torch.allclose(ga, gout * (1 - sd), rtol=1e-12, atol=0) and torch.allclose(gb, gout * sd, rtol=1e-12, atol=0)
    gz, = torch.autograd.grad(torch.sigmoid(o), o, gsoft)
    assert float((gsoft * (sd * (1 - sd)) - gz).abs().max()) <= 1e-12
