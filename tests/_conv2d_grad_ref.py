"""Float64 restatement of the backward of one few-channel conv unit with frozen BatchNorm (decnet_amd/conv2d_grad.py,
csrc/conv2d_grad.hip), and the seeded module cases of tests/test_conv2d_grad_gpu.py.  CPU only; a helper module of
tests/test_conv2d_grad_cpu.py (which holds it against torch's own float64 autograd) and of the GPU test.

For y = act(conv(x, w) * scale[co] + shift[co]) (k 1 or 3, stride 1, padding d * (k // 2)), upstream gradient gy and
gm = gy * [y > 0] (gm = gy without ReLU):
    G[co,ci,ky,kx] = sum_{b,y,x} gm[b,co,y,x] * x[b,ci,y+(ky-k/2)d,x+(kx-k/2)d]   (zeros outside),  gsum[co] = sum gm
    dW = scale * G,  dscale = <w, G>,  dshift = gsum,  dx = conv(gm, W'),  W'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] scale[co]
"""
import copy

import torch

import _trunk_ref as R

D = torch.float64
U32 = 2.0 ** -24                   # unit roundoff of float32: the `eps` of the 4096-term chain bound
CHAIN = 4096


def _cat(xs):
    return torch.cat([R._d(t) for t in xs], 1) if isinstance(xs, (list, tuple)) else R._d(xs)


def mask(gy, y):
    """gm = gy * [y > 0]; y None: no ReLU."""
    gy = R._d(gy)
    return gy if y is None else torch.where(R._d(y) > 0, gy, torch.zeros((), dtype=D))


def _taps(gm, x, k, dil):
    B, C, H, W = x.shape
    p = dil * (k // 2)
    xp = torch.zeros(B, C, H + 2 * p, W + 2 * p, dtype=D)
    xp[:, :, p:p + H, p:p + W] = x
    G = torch.zeros(gm.shape[1], C, k, k, dtype=D)
    for ky in range(k):
        for kx in range(k):
            G[:, :, ky, kx] = torch.einsum("bohw,bchw->oc", gm, xp[:, :, ky * dil:ky * dil + H, kx * dil:kx * dil + W])
    return G


def wgrad(xs, gy, y, k, dil):
    """-> (G [Cout,Cin,k,k], gsum [Cout], gm [B,Cout,H,W]) in float64."""
    gm = mask(gy, y)
    return _taps(gm, _cat(xs), k, dil), gm.sum((0, 2, 3)), gm


def wgrad_abs(xs, gy, y, k, dil):
    """The sums of absolute terms behind G and gsum: S = sum |gm| |x| per element of G, sum |gm| per channel."""
    gm = mask(gy, y).abs()
    return _taps(gm, _cat(xs).abs(), k, dil), gm.sum((0, 2, 3))


def flipped(w, scale):
    w = R._d(w) * R._d(scale).view(-1, 1, 1, 1)
    return w.flip(2, 3).transpose(0, 1).contiguous()


def dx(gm, w, scale, dil):
    """The input gradient as the same-padded convolution of gm with the flipped, scaled weights."""
    return R.conv(R._d(gm), flipped(w, scale), dil)


def bn_fold(bn):
    """(scale, shift) of an eval-mode BatchNorm2d as float64 expressions of its (leaf) parameters."""
    scale = bn.weight.to(D) / torch.sqrt(bn.running_var.to(D) + bn.eps)
    return scale, bn.bias.to(D) - bn.running_mean.to(D) * scale


# ---- the module cases of the GPU test: Refinement(8, 8, stage_id=3) and SoftAttention(12, 8).fuse at 1 x 16 x 18 ----------
MODULE_HW = (16, 18)
MODULE_SEEDS = {"refinement": 9, "attention": 8}        # chosen by tests/test_conv2d_grad_cpu.py's margin property (see there)
MARGIN = 1e-4                                           # 5 x the forward tolerance of the small kernels (2e-5)


def module_case(name, seed=None):
    """-> (module in eval mode (float32, CPU), inputs: dict of float32 CPU tensors, names of the inputs that take a
    gradient, r: the weights of the loss (out * r).sum())."""
    import _model_cases as MC
    from decnet_amd.model import Refinement, SoftAttention
    seed = MODULE_SEEDS[name] if seed is None else seed
    H, W = MODULE_HW
    g = torch.Generator().manual_seed(7919 * seed + 13)
    if name == "refinement":
        m = MC.seeded(lambda: Refinement(8, 8, stage_id=3), 100 + seed)
        m.conv[-1].conv.bias.data = torch.randn(1, generator=g) * 0.3
        ins = {"left": torch.randn(1, 8, H, W, generator=g), "right": torch.randn(1, 8, H, W, generator=g),
               "disp": torch.rand(1, H, W, generator=g) * 4}
        wrt = ("disp",)
    else:
        m = MC.seeded(lambda: SoftAttention(12, 8), 200 + seed)
        ins = {"fea": torch.randn(1, 8, H, W, generator=g), "dense": torch.rand(1, H, W, generator=g) * 4,
               "sparse": torch.rand(1, H, W, generator=g) * 4, "mask": (torch.rand(1, H, W, generator=g) < 0.5).float(),
               "var": torch.rand(1, H, W, generator=g)}
        wrt = ("dense", "sparse")
    return m, ins, wrt, torch.randn(1, H, W, generator=g)


def module_out(name, m, t):
    if name == "refinement":
        return m(t["left"], t["right"], t["disp"])[0]
    return m.fuse(t["fea"], t["dense"], t["sparse"], t["mask"], t["var"])


def module_grads(name, m, ins, wrt, r, dtype, device="cpu", ctx=None, margins=None):
    """One run of the module's loss (out * r).sum() on a copy of `m` in `dtype` on `device`: -> {tensor name: gradient on
    the CPU} over every parameter and the inputs `wrt`.  ctx: a context manager factory around forward (hip_grad).
    margins: a list that receives (unit name, min |pre-activation|, max |pre-activation|) of every ReLU'd unit."""
    import contextlib
    from decnet_amd.model import Unit
    m = copy.deepcopy(m).to(device=device, dtype=dtype).eval()
    t = {k: v.detach().clone().to(device=device, dtype=dtype) for k, v in ins.items()}
    for k in wrt:
        t[k].requires_grad_()
    hooks = []
    if margins is not None:
        for un, u in m.named_modules():
            if isinstance(u, Unit) and u.relu and u.bn is not None:
                hooks.append(u.bn.register_forward_hook(
                    lambda mod, i, o, un=un: margins.append((un, float(o.detach().abs().min()), float(o.detach().abs().max())))))
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        out = module_out(name, m, t)
    (out * r.to(device=device, dtype=dtype)).sum().backward()
    for h in hooks:
        h.remove()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    grads.update({k: t[k].grad.detach().cpu() for k in wrt})
    return grads, m, t


def margins_hold(margins):
    """No pre-activation of a ReLU'd unit within MARGIN * max(1, max|pre|) of zero."""
    return all(lo > MARGIN * max(1.0, hi) for _, lo, hi in margins)
