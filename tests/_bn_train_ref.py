"""Float64 restatement of training-mode BatchNorm2d (+ ReLU), forward and backward (decnet_amd/csrc/batchnorm.hip,
conv2d_grad.BatchNormActFunction), the data sets of its tests, and the seeded unit and module cases of
tests/test_bn_train_gpu.py, and `check_entry`, the bounds both GPU files hold the entries to.  CPU only; a helper
module of tests/test_bn_train_cpu.py (which holds it against torch's own float64 autograd) and of the GPU tests.

For z [B,C,H,W], N = B H W values per channel, the pivot p_c = z[0,c,0,0]:
    mean = p + sum (z - p) / N,  var = sum (z - mean)^2 / N (biased),  invstd = 1 / sqrt(var + eps),  xhat = (z - mean) invstd
    pre = xhat gamma + beta,  y = act(pre)
    running_mean <- (1 - m) running_mean + m mean,  running_var <- (1 - m) running_var + m var N / (N - 1)
and with gm = gy [pre > 0] (gm = gy without ReLU; the mask may be imposed):
    dbeta = sum gm,  dgamma = sum gm xhat,  gz = gamma invstd (gm - dbeta / N - xhat dgamma / N)
"""
import copy

import torch
import torch.nn.functional as F

D = torch.float64
U32 = 2.0 ** -24


def _d(t):
    return t.detach().to(D)


def _pc(v):
    return v.view(1, -1, 1, 1)


def forward(z, gamma, beta, eps, momentum=None, running_mean=None, running_var=None, relu=True):
    """-> dict of float64 tensors: mean, var, invstd [C]; xhat, pre, y [B,C,H,W]; dev1 = mean |z - p|, dev2 = mean (z - p)^2
    [C] (the scales of the statistics' bounds); running_mean, running_var after the update where given."""
    z, gamma, beta = _d(z), _d(gamma), _d(beta)
    n = z.numel() // z.shape[1]
    p = z[0, :, 0, 0]
    dp = z - _pc(p)
    m1 = dp.sum((0, 2, 3)) / n
    mean = p + m1
    dm = dp - _pc(m1)                                   # z - mean without the rounding of mean at its own magnitude
    var = (dm * dm).sum((0, 2, 3)) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = dm * _pc(invstd)
    pre = xhat * _pc(gamma) + _pc(beta)
    out = dict(mean=mean, var=var, invstd=invstd, xhat=xhat, pre=pre, y=torch.relu(pre) if relu else pre,
               dev1=dp.abs().sum((0, 2, 3)) / n, dev2=(dp * dp).sum((0, 2, 3)) / n)
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * _d(running_mean) + momentum * mean
        out["running_var"] = (1 - momentum) * _d(running_var) + momentum * var * n / (n - 1)
    return out


def backward(fwd, gy, gamma, relu=True, mask=None):
    """The closed-form backward on forward()'s dict.  mask: a bool tensor imposed as [pre > 0] (None: the reference's own).
    -> dict: gm, gz [B,C,H,W]; dgamma, dbeta [C]; and the sums of absolute terms abs_dgamma = sum |gm xhat|, abs_dbeta = sum |gm|."""
    gy, gamma = _d(gy), _d(gamma)
    xhat = fwd["xhat"]
    n = gy.numel() // gy.shape[1]
    if relu:
        gm = torch.where(fwd["pre"] > 0 if mask is None else mask, gy, torch.zeros((), dtype=D))
    else:
        gm = gy
    dbeta = gm.sum((0, 2, 3))
    dgamma = (gm * xhat).sum((0, 2, 3))
    gz = _pc(gamma * fwd["invstd"]) * (gm - _pc(dbeta) / n - xhat * _pc(dgamma) / n)
    return dict(gm=gm, gz=gz, dgamma=dgamma, dbeta=dbeta, abs_dgamma=(gm * xhat).abs().sum((0, 2, 3)),
                abs_dbeta=gm.abs().sum((0, 2, 3)))


def check_entry(r, f, gamma, beta, gy, relu, eps, tag, buffers=True):
    """The bounds of the entries' results r (y and gz in the NCHW view) against f, the float64 forward of the same z, each
    from counting roundings with a margin of a small factor (u = 2^-24):
      statistics   |mean - mean64| <= 2^-40 mean|z - p|; |var - var64| <= 2^-40 mean (z - p)^2 + 16 x 2^-53 (var64 + eps), var taken
                   back out of the kernel's invstd as 1 / invstd^2 - eps -- the second term: eight float64 roundings of at
                   most 2^-53 (var + eps) each (the sum var + eps, the square root and the division in the kernel, the
                   last two twice in invstd^2; the square, the division and the subtraction here), margin 2; and through
                   invstd = (var + eps)^-1/2 itself, whose derivative carries
                   |var - var64| <= 2^-40 mean (z - p)^2 to |invstd - invstd64| <= invstd64 (2^-41 mean (z - p)^2 / (var64 + eps)
                   + 4 x 2^-53) -- the second term: the square root and the division in float64 -- so that a constant channel
                   (var = 0 exactly) is held to the roundings of 1 / sqrt(eps) alone;
      buffers      2 u relative;
      output       4 u (|xhat64 gamma| + |beta|) + |a| |mean - mean64|;
      dgamma       4 u sum |gm xhat|, dbeta 2 u sum |gm|, gz 8 u |a| (|gm| + |dbeta| / N + |xhat| |dgamma| / N), the mask [y_gpu > 0]
                   imposed, every imposed decision that is not float64's own within the output bound of zero."""
    U = U32
    n = f["xhat"].numel() // f["xhat"].shape[1]
    mean, invstd = r["stats"][0::2], r["stats"][1::2]
    e_mean = (mean - f["mean"]).abs()
    assert bool((e_mean <= 2.0 ** -40 * f["dev1"]).all()), ("mean", e_mean, f["dev1"])
    b_inv = f["invstd"] * (2.0 ** -41 * f["dev2"] / (f["var"] + eps) + 4 * 2.0 ** -53)
    assert bool(((invstd - f["invstd"]).abs() <= b_inv).all()), ("invstd", invstd - f["invstd"], b_inv)
    var = 1.0 / (invstd * invstd) - eps                       # the kernel's var back out of invstd, in float64
    b_var = 2.0 ** -40 * f["dev2"] + 16 * 2.0 ** -53 * (f["var"] + eps)
    assert bool(((var - f["var"]).abs() <= b_var).all()), ("var", var - f["var"], b_var)
    if buffers:
        for k in ("running_mean", "running_var"):
            assert bool(((r[k].double() - f[k]).abs() <= 2 * U * f[k].abs()).all()), k
    g64 = gamma.double()
    a = (g64 * f["invstd"]).abs()
    b_y = 4 * U * ((f["xhat"] * _pc(g64)).abs() + _pc(beta.double().abs())) + _pc(a * e_mean)
    e_y = (r["y"].double() - f["y"]).abs()
    print(tag, "y: worst error / bound = %.3g" % float((e_y / b_y.clamp_min(1e-300)).max()))
    assert bool((e_y <= b_y).all()), "y"
    mask = None
    if relu:
        mask = r["y"] > 0
        flipped = mask != (f["pre"] > 0)
        assert bool((f["pre"].abs()[flipped] <= b_y[flipped]).all()), "a ReLU decision far from zero differs from float64's"
    g = backward(f, gy, gamma, relu, mask)
    for k, factor in (("dgamma", 4), ("dbeta", 2)):
        err, bound = (r[k].double() - g[k]).abs(), factor * U * g["abs_" + k]
        print(tag, k, "worst error / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (k, err, bound)
    b_gz = 8 * U * _pc(a) * (g["gm"].abs() + _pc(g["dbeta"].abs()) / n + f["xhat"].abs() * _pc(g["dgamma"].abs()) / n)
    e_gz = (r["gz"].double() - g["gz"]).abs()
    print(tag, "gz: worst error / bound = %.3g" % float((e_gz / b_gz.clamp_min(1e-300)).max()))
    assert bool((e_gz <= b_gz).all()), "gz"
    assert not any(bool(torch.isnan(v).any()) for v in r.values())


# ---- the data sets of the entry tests ------------------------------------------------------------------------------------------
KINDS = ("normal", "offset", "constant")          # per channel, in turn: standard normal; mean 1000, spread 0.01; a constant


def entry_data(shape, first_kind=0, relu=False, seed=0):
    """z [B,C,H,W] float32 whose channel c is of kind KINDS[(c + first_kind) % 3], gy, gamma, beta, running_mean,
    running_var (float32).  Under ReLU, with two channels or more, the LAST channel's beta puts every pre-activation below
    zero (|xhat| <= sqrt(N))."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 131 * H * W + 7 * C + B + 17 * first_kind)
    z = torch.randn(shape, generator=g)
    for c in range(C):
        kind = KINDS[(c + first_kind) % 3]
        if kind == "offset":
            z[:, c] = 1000.0 + 0.01 * z[:, c]
        elif kind == "constant":
            z[:, c] = 0.7 + 0.1 * c
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::2] = -gamma[::2]                       # (both signs)
    beta = torch.randn(C, generator=g) * 0.3
    if relu and C > 1:
        beta[C - 1] = -(float(gamma[C - 1].abs()) * (B * H * W) ** 0.5 + 1.0)
    return dict(z=z, gy=torch.randn(shape, generator=g), gamma=gamma, beta=beta,
                running_mean=torch.randn(C, generator=g) * 0.2, running_var=torch.rand(C, generator=g) + 0.5)


# ---- one Unit in train mode as torch ops (any dtype), the ReLU mask imposed where given ---------------------------------------------
def unit_train(u, parts, dtype, mask=None, gy=None):
    """conv -> batch_norm(training) -> ReLU of a copy of Unit `u` in `dtype` on the CPU, on the channel concatenation of
    `parts`.  mask: [y > 0] to impose in place of the run's own.  With gy: also backward -> (y, pre, grads: dict over
    "x0".."xn", conv.weight, bn.weight, bn.bias, the copy); without: (y, pre, None, the copy)."""
    u = copy.deepcopy(u).cpu().to(dtype).train()
    xs = [t.detach().cpu().to(dtype).requires_grad_() for t in parts]
    c, bn = u.conv, u.bn
    x = torch.cat(xs, 1)
    if isinstance(c, torch.nn.ConvTranspose2d):
        z = F.conv_transpose2d(x, c.weight, c.bias, c.stride, c.padding)
    else:
        z = F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation)
    if bn is not None:
        pre = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)
        bn.num_batches_tracked += 1
    else:
        pre = z
    if not u.relu:
        y = pre
    elif mask is None:
        y = torch.relu(pre)
    else:
        y = pre * mask.to(dtype)
    grads = None
    if gy is not None:
        y.backward(gy.detach().cpu().to(dtype))
        grads = {"x%d" % i: t.grad.detach() for i, t in enumerate(xs)}
        grads.update({n: p.grad.detach() for n, p in u.named_parameters()})
    return y.detach(), pre.detach(), grads, u


# (route of Unit._route, cin, cout, k, kwargs of tests/_model_cases.make_unit, B, H, W, channels of the input parts or None)
UNIT_CASES = {
    "conv": ("conv", 17, 8, 3, dict(dil=3), 2, 16, 18, (8, 8, 1)),
    "mfma": ("mfma", 24, 24, 3, {}, 1, 64, 66, None),
    "conv_s3": ("conv_s3", 8, 24, 3, dict(stride=3), 2, 24, 36, None),
    "mfma_s3": ("mfma_s3", 24, 72, 3, dict(stride=3), 1, 72, 66, None),
    "deconv": ("deconv", 24, 8, 3, dict(stride=3, transposed=True), 2, 6, 8, None),
    "mfma_deconv": ("mfma_deconv", 72, 24, 3, dict(stride=3, transposed=True), 1, 16, 33, None),
    "nobn": ("conv", 8, 1, 3, dict(bn=False), 2, 16, 18, None),
}
GRAD_ROUTE = {"conv": "conv", "mfma": "mfma", "conv_s3": "s3", "mfma_s3": "s3", "deconv": "deconv", "mfma_deconv": "deconv"}


def unit_case(name):
    """-> (Unit in train mode (float32, CPU), the input parts, gy)."""
    import _model_cases as MC
    route, ci, co, k, kw, B, H, W, parts = UNIT_CASES[name]
    u = MC.make_unit(ci, co, k, seed=ci + 3 * co, **kw).train()
    g = torch.Generator().manual_seed(ci * 11 + co)
    xs = [torch.randn(B, c, H, W, generator=g) for c in (parts or (ci,))]
    if kw.get("transposed"):
        ho, wo = 3 * H, 3 * W
    elif kw.get("stride") == 3:
        ho, wo = (H - 1) // 3 + 1, (W - 1) // 3 + 1
    else:
        ho, wo = H, W
    return u, xs, torch.randn(B, co, ho, wo, generator=g)


# ---- the module cases of the GPU test: Refinement(8, 8, stage_id=3) and SoftAttention(12, 8).fuse at 2 x 16 x 18, train mode ------
MODULE_B, MODULE_HW = 2, (16, 18)
# chosen by tests/test_bn_train_cpu.py's margin property: the first seeds from 1 up that satisfy it (see there; with some
# 28000 BatchNorm outputs of ReLU'd units in the refinement case, about one seed in 3000 does)
MODULE_SEEDS = {"refinement": 3408, "attention": 49}
MARGIN = 1e-4                                           # as tests/_conv2d_grad_ref.py: 5 x the forward tolerance of the small kernels


def module_case(name, seed=None):
    """-> (module in train mode (float32, CPU), inputs: dict of float32 CPU tensors, names of the inputs that take a
    gradient, r: the weights of the loss (out * r).sum())."""
    import _model_cases as MC
    from decnet_amd.model import Refinement, SoftAttention
    seed = MODULE_SEEDS[name] if seed is None else seed
    B, (H, W) = MODULE_B, MODULE_HW
    g = torch.Generator().manual_seed(7919 * seed + 29)
    if name == "refinement":
        m = MC.seeded(lambda: Refinement(8, 8, stage_id=3), 300 + seed)
        m.conv[-1].conv.bias.data = torch.randn(1, generator=g) * 0.3
        ins = {"left": torch.randn(B, 8, H, W, generator=g), "right": torch.randn(B, 8, H, W, generator=g),
               "disp": torch.rand(B, H, W, generator=g) * 4}
        wrt = ("disp",)
    else:
        m = MC.seeded(lambda: SoftAttention(12, 8), 400 + seed)
        ins = {"fea": torch.randn(B, 8, H, W, generator=g), "dense": torch.rand(B, H, W, generator=g) * 4,
               "sparse": torch.rand(B, H, W, generator=g) * 4, "mask": (torch.rand(B, H, W, generator=g) < 0.5).float(),
               "var": torch.rand(B, H, W, generator=g)}
        wrt = ("dense", "sparse")
    return m.train(), ins, wrt, torch.randn(B, H, W, generator=g)


def module_out(name, m, t):
    if name == "refinement":
        return m(t["left"], t["right"], t["disp"])[0]
    return m.fuse(t["fea"], t["dense"], t["sparse"], t["mask"], t["var"])


def module_step(name, m, t, wrt, r, ctx=None):
    """One forward + backward of the loss (out * r).sum() on module `m` and the tensors `t` as they are (gradients
    accumulate).  ctx: a context manager factory around the forward (hip_grad)."""
    import contextlib
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        out = module_out(name, m, t)
    (out * r).sum().backward()
    return out


def module_grads(name, m, ins, wrt, r, dtype, device="cpu", ctx=None, margins=None, steps=1):
    """`steps` train-mode steps of module_step on a copy of `m` in `dtype` on `device`, the gradients cleared before each
    -> ({tensor name: gradient of the last step, on the CPU} over every parameter and the inputs `wrt`, {buffer name:
    value after the steps}, the copy, its input tensors).  margins: a list that receives (unit name, min |pre-activation|,
    max |pre-activation|) of every ReLU'd unit with BatchNorm (library route only: the hook is BatchNorm2d's)."""
    m = copy.deepcopy(m).to(device=device, dtype=dtype).train()
    t = {k: v.detach().clone().to(device=device, dtype=dtype) for k, v in ins.items()}
    for k in wrt:
        t[k].requires_grad_()
    r = r.to(device=device, dtype=dtype)
    hooks = []
    if margins is not None:
        from decnet_amd.model import Unit
        for un, u in m.named_modules():
            if isinstance(u, Unit) and u.relu and u.bn is not None:
                hooks.append(u.bn.register_forward_hook(
                    lambda mod, i, o, un=un: margins.append((un, float(o.detach().abs().min()), float(o.detach().abs().max())))))
    for _ in range(steps):
        for p in list(m.parameters()) + [t[k] for k in wrt]:
            p.grad = None
        module_step(name, m, t, wrt, r, ctx)
    for h in hooks:
        h.remove()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    grads.update({k: t[k].grad.detach().cpu() for k in wrt})
    return grads, {n: b.detach().cpu().clone() for n, b in m.named_buffers()}, m, t


def margins_hold(margins):
    """No BatchNorm output of a ReLU'd unit within MARGIN * max(1, max|pre|) of zero."""
    return bool(margins) and all(lo > MARGIN * max(1.0, hi) for _, lo, hi in margins)


def gate(g64, g32):
    """The module gate of a gradient tensor: max(4 e32, 2e-5 max(1, max|g64|)), e32 the float32 CPU run's own distance."""
    e32 = float((g32.double() - g64).abs().max())
    return max(4.0 * e32, 2e-5 * max(1.0, float(g64.abs().max())))
