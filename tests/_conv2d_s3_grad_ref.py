"""Float64 restatement of the backward of the stride-3 units with frozen BatchNorm (decnet_amd/conv2d_grad.Conv2dS3Function /
Deconv2dS3Function, csrc/conv2d_mfma_grad.hip, csrc/unfold.hip).  CPU only; a helper module of
tests/test_conv2d_s3_grad_cpu.py (which holds the closed forms against torch's own double autograd) and of
tests/test_conv2d_s3_grad_gpu.py.

With gm = gy * [y > 0] (gm = gy without ReLU), gsum[co] = sum gm, dW = scale * G, dscale = <w, G>, dshift = gsum:
  conv (Conv2d k 3, stride 3, padding 1; x [B,Ci,H,W], y [B,Co,Ho,Wo], w [Co,Ci,3,3])
    G[co,ci,ky,kx] = sum gm[b,co,yo,xo] x[b,ci,3yo-1+ky,3xo-1+kx]                         (0 outside)
    dx[b,ci,r,s]   = sum_co gm[b,co,(r+1)/3,(s+1)/3] w[co,ci,(r+1)%3,(s+1)%3] scale[co]   (0 where (r+1)/3 = Ho, (s+1)/3 = Wo)
  transposed (ConvTranspose2d k 3, stride 3; x [B,Ci,H,W], y [B,Co,3H,3W], w [Ci,Co,3,3])
    G[ci,co,a,c]   = sum x[b,ci,i,j] gm[b,co,3i+a,3j+c]
    dx[b,ci,i,j]   = sum_{co,a,c} gm[b,co,3i+a,3j+c] w[ci,co,a,c] scale[co]
"""
import torch
import torch.nn.functional as F

import _conv2d_grad_ref as GR
import _trunk_ref as R

D = torch.float64


def out_hw(tr, H, W):
    return (3 * H, 3 * W) if tr else ((H - 1) // 3 + 1, (W - 1) // 3 + 1)


def s2d3_pad0(g):
    """[B,C,3H,3W] -> [B,9C,H,W], channel c * 9 + 3a + c'."""
    g = R._d(g)
    B, C, H3, W3 = g.shape
    return g.reshape(B, C, H3 // 3, 3, W3 // 3, 3).permute(0, 1, 3, 5, 2, 4).reshape(B, 9 * C, H3 // 3, W3 // 3)


def d2s3_pad1(t, H, W):
    """The adjoint of _trunk_ref.s2d3_pad1: t [B,9C,Ho,Wo] -> [B,C,H,W], by indexing."""
    t = R._d(t)
    B, K, Ho, Wo = t.shape
    C = K // 9
    r, s = torch.arange(H) + 1, torch.arange(W) + 1
    tp = torch.zeros(B, C, 9, Ho + 1, Wo + 1, dtype=D)                  # a zero row / column behind
    tp[:, :, :, :Ho, :Wo] = t.reshape(B, C, 9, Ho, Wo)
    ch = (r % 3)[:, None] * 3 + (s % 3)[None, :]                        # [H,W]
    return tp[:, :, ch, (r // 3)[:, None].expand(H, W), (s // 3)[None, :].expand(H, W)]


def _corr(P, Q9):
    """R[cp][cq][3ky+kx] = sum_{b,i,j} P[b,cp,i,j] Q9[b,cq,3ky+kx,i,j]."""
    return torch.einsum("bpij,bqtij->pqt", P, Q9)


def wgrad(tr, x, gy, y, absolute=False):
    """-> (G in the layer's weight layout, gsum [Cout], gm) in float64; absolute: the sums of |gm| |x| and of |gm|."""
    gm, x = GR.mask(gy, y), R._d(x)
    if absolute:
        gm, x = gm.abs(), x.abs()
    B, Ci = x.shape[:2]
    Co = gm.shape[1]
    if tr:
        G = _corr(x, s2d3_pad0(gm).reshape(B, Co, 9, *x.shape[2:])).reshape(Ci, Co, 3, 3)
    else:
        G = _corr(gm, R.s2d3_pad1(x).reshape(B, Ci, 9, *gm.shape[2:])).reshape(Co, Ci, 3, 3)
    return G, gm.sum((0, 2, 3)), gm


def dx(tr, gm, w, scale, H, W):
    """The input gradient [B,Ci,H,W] of the closed forms above."""
    gm, w, scale = R._d(gm), R._d(w), R._d(scale)
    if tr:
        ws = (w * scale.view(1, -1, 1, 1)).reshape(w.shape[0], -1)               # [Ci, 9 Co]
        return torch.einsum("bkij,ck->bcij", s2d3_pad0(gm), ws)
    ws = (w * scale.view(-1, 1, 1, 1)).reshape(w.shape[0], -1)                   # [Co, 9 Ci]
    return d2s3_pad1(torch.einsum("boij,ok->bkij", gm, ws), H, W)


def forward(tr, x, w, scale, shift, relu):
    return (R.deconv_s3_bn_act if tr else R.conv_s3_bn_act)(x, w, scale, shift, relu)


def autograd(tr, x, w, scale, shift, relu, gy):
    """Double autograd of the torch layer y = act(conv(x, w) * scale + shift) -> dict of dx, dw, dscale, dshift, y."""
    x, w, scale, shift = (R._d(t).requires_grad_() for t in (x, w, scale, shift))
    pre = F.conv_transpose2d(x, w, stride=3) if tr else F.conv2d(x, w, stride=3, padding=1)
    pre = pre * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    y = torch.relu(pre) if relu else pre
    g = torch.autograd.grad(y, (x, w, scale, shift), R._d(gy))
    return dict(zip(("dx", "dw", "dscale", "dshift"), g), y=y.detach())


def closed(tr, x, w, scale, shift, relu, gy):
    """The same gradients from the closed forms."""
    y = forward(tr, x, w, scale, shift, relu)
    G, gsum, gm = wgrad(tr, x, gy, y if relu else None)
    sv = R._d(scale).view((1, -1, 1, 1) if tr else (-1, 1, 1, 1))
    return {"dx": dx(tr, gm, w, scale, *x.shape[2:]), "dw": G * sv,
            "dscale": (R._d(w) * G).sum((0, 2, 3) if tr else (1, 2, 3)), "dshift": gsum, "y": y}


# ---- the chain of tests/test_conv2d_s3_grad_gpu.py: f0 -> conv1 = (8 -> 24 s3, 24 -> 24, 24 -> 24) -> UpBlock(24, 8)(f0, .) ----
CHAIN_HW = (192, 192)


def chain_case():
    """-> (conv1: nn.Sequential of three Units, up: UpBlock(24, 8), f0 [1,8,192,192], r [1,8,192,192]) in float32, eval."""
    import _model_cases as MC
    from decnet_amd.model import Unit, UpBlock, _c3, _seq
    g = torch.Generator().manual_seed(431)
    conv1 = MC.seeded(lambda: _seq(Unit(8, 24, 3, stride=3, pad=1), _c3(24, 24), _c3(24, 24)), 531)
    up = MC.seeded(lambda: UpBlock(24, 8), 532)
    H, W = CHAIN_HW
    return conv1, up, torch.randn(1, 8, H, W, generator=g), torch.randn(1, 8, H, W, generator=g)


def chain_units(conv1, up):
    """The chain's units in forward order, with their names in the gradient dicts."""
    return [("conv1.%d" % i, u) for i, u in enumerate(conv1)] + [("up.deconv", up.deconv), ("up.conv.0", up.conv[0]),
                                                                 ("up.conv.1", up.conv[1])]


def chain_grads(conv1, up, f0, r, dtype, masks=None):
    """One run of (chain(f0) * r).sum() on copies in `dtype` on the CPU, in torch ops -> ({name: gradient} over every
    parameter and "f0", [mask of every unit]).  masks: impose these [y > 0] instead of the run's own (see
    tests/_conv2d_mfma_grad_ref.py for why)."""
    import copy
    import _conv2d_mfma_grad_ref as MG
    conv1, up = copy.deepcopy(conv1).to(dtype).eval(), copy.deepcopy(up).to(dtype).eval()
    x0 = f0.detach().clone().to(dtype).requires_grad_()
    took = []

    def run(u, x):
        c = u.conv
        if isinstance(c, torch.nn.ConvTranspose2d):
            pre = F.conv_transpose2d(x, c.weight, c.bias, c.stride, c.padding)
            pre = F.batch_norm(pre, u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias, False, 0.0, u.bn.eps)
        else:
            pre = MG.unit_pre(u, x)
        if masks is None:
            took.append(pre.detach() > 0)
            return torch.relu(pre)
        took.append(masks[len(took)])
        return pre * took[-1].to(dtype)

    x = x0
    for u in conv1:
        x = run(u, x)
    x = run(up.deconv, x)
    x = run(up.conv[0], torch.cat((x, x0), 1))
    x = run(up.conv[1], x)
    (x * r.to(dtype)).sum().backward()
    grads = {"conv1." + n: p.grad.detach() for n, p in conv1.named_parameters()}
    grads.update({"up." + n: p.grad.detach() for n, p in up.named_parameters()})
    grads["f0"] = x0.grad.detach()
    return grads, took
