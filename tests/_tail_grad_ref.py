"""Float64 restatements of the four backwards of csrc/tail_grad.hip (decnet_amd/tail_grad.py), written out as the formulas
of include/decnet_hip.h.  CPU only; a helper module of tests/test_tail_grad_cpu.py (which holds each against torch's own
float64 autograd) and tests/test_tail_grad_gpu.py.

Every function returns, beside each gradient, the same expression over the absolute values of every term (`A`: what an
fp32 summation error is proportional to), and for g_right the number of contributors per element.  The warp ones take
the sampling position from tests/_trunk_ref.warp_coords in float32 by default -- the reference's own grid, as the
forward's edge test does: with float64 coordinates the cell floor(ix) flips at integer ix, and the derivative of a
bilinear warp jumps there, a property of the reference's grid, not of the kernel.  `dtype` (float32) evaluates the
upsampling and blend formulas in that precision: the g32 of the project's module gate.
"""
import torch

import _trunk_ref as R

D = torch.float64
U32 = 2.0 ** -24


def _taps(right, ix, iy):
    """The four taps of every output pixel: [(name, value [B,C,H,W] (0 outside), ok [B,H,W], flat index [B,H*W],
    x weight, y weight)] in the order nw, ne, sw, se."""
    B, C, H, W = right.shape
    x0, y0 = torch.floor(ix), torch.floor(iy)
    flat = right.reshape(B, C, H * W)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, H * W)
            v = torch.gather(flat, 2, idx.unsqueeze(1).expand(B, C, H * W)).reshape(B, C, H, W)
            v = torch.where(ok.unsqueeze(1), v, torch.zeros((), dtype=D))
            out.append((v, ok, idx, 1 - (ix - xi).abs(), 1 - (iy - yi).abs()))
    return out


def warp_backward(right, disp, gout, coord_dtype=torch.float32):
    """-> dict: g_right, A_right, n_right [B,C,H,W]; g_disp, A_disp [B,H,W]."""
    r, g = R._d(right), R._d(gout)
    B, C, H, W = r.shape
    ix, iy = R.warp_coords(disp, H, W, coord_dtype)
    (nw, _, _, _, _), (ne, _, _, _, _), (sw, _, _, _, _), (se, _, _, _, _) = taps = _taps(r, ix, iy)
    ty = (iy - torch.floor(iy)).unsqueeze(1)
    f = W / (W - 1.0)
    g_disp = -f * (g * ((ne - nw) * (1 - ty) + (se - sw) * ty)).sum(1)
    A_disp = f * (g.abs() * ((ne.abs() + nw.abs()) * (1 - ty) + (se.abs() + sw.abs()) * ty)).sum(1)
    g_right, A_right, n_right = (torch.zeros(B, C, H * W, dtype=D) for _ in range(3))
    for _, ok, idx, wx, wy in taps:
        wgt = torch.where(ok, wx * wy, torch.zeros((), dtype=D)).reshape(B, 1, H * W)
        i3 = idx.unsqueeze(1).expand(B, C, H * W)
        g_right.scatter_add_(2, i3, g.reshape(B, C, H * W) * wgt)
        A_right.scatter_add_(2, i3, g.reshape(B, C, H * W).abs() * wgt)
        n_right.scatter_add_(2, i3, ok.to(D).reshape(B, 1, H * W).expand(B, C, H * W).contiguous())
    return {"g_right": g_right.view(B, C, H, W), "A_right": A_right.view(B, C, H, W), "n_right": n_right.view(B, C, H, W),
            "g_disp": g_disp, "A_disp": A_disp}


def _neighbours(d):
    """[B,h,w] -> (the replicate-padded 3 x 3 neighbours [B,9,h,w], their flat source index [9,h*w])."""
    B, h, w = d.shape
    ys, xs = torch.arange(h), torch.arange(w)
    nb, idx = [], []
    for ky in range(3):
        for kx in range(3):
            yy, xx = (ys + ky - 1).clamp(0, h - 1), (xs + kx - 1).clamp(0, w - 1)
            nb.append(d[:, yy][:, :, xx])
            idx.append((yy.view(h, 1) * w + xx.view(1, w)).reshape(-1))
    return torch.stack(nb, 1), torch.stack(idx, 0)


def upsample3_backward(logits, disp, gout, dtype=D):
    """-> dict: g_logits, A_logits [B,81,h,w]; g_disp, A_disp [B,h,w], evaluated in `dtype`, returned as float64."""
    lg, d, g = (t.detach().to("cpu", dtype) for t in (logits, disp, gout))
    B, h, w = d.shape
    nb, idx = _neighbours(d)                                              # [B,k,h,w]
    p = torch.softmax(lg.view(B, 9, 9, h, w), 2)                          # [B,s,k,h,w]
    gs = g.view(B, h, 3, w, 3).permute(0, 2, 4, 1, 3).reshape(B, 9, 1, h, w)     # gout_s
    m = (p * nb.unsqueeze(1)).sum(2, keepdim=True)
    g_logits = 3 * gs * p * (nb.unsqueeze(1) - m)
    A_logits = 3 * gs.abs() * p * (nb.abs().unsqueeze(1) + (p * nb.abs().unsqueeze(1)).sum(2, keepdim=True))
    q, qa = 3 * (gs * p).sum(1), 3 * (gs.abs() * p).sum(1)                # [B,k,h,w]
    g_disp, A_disp = torch.zeros(B, h * w, dtype=dtype), torch.zeros(B, h * w, dtype=dtype)
    for k in range(9):
        i2 = idx[k].view(1, -1).expand(B, h * w)
        g_disp.scatter_add_(1, i2, q[:, k].reshape(B, h * w))
        A_disp.scatter_add_(1, i2, qa[:, k].reshape(B, h * w))
    return {"g_logits": g_logits.reshape(B, 81, h, w).to(D), "A_logits": A_logits.reshape(B, 81, h, w).to(D),
            "g_disp": g_disp.view(B, h, w).to(D), "A_disp": A_disp.view(B, h, w).to(D)}


def fold3(g):
    """g [B,9C+1,h,w] -> g_fea[b,c,3y+i,3x+j] = g[b,1+9c+3i+j,y,x] (same dtype: a permutation)."""
    B, K, h, w = g.shape
    C = (K - 1) // 9
    return g[:, 1:].reshape(B, C, 3, 3, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, C, 3 * h, 3 * w)


def unfold3_cat_backward(g):
    """-> (g_fea [B,C,3h,3w], g_disp [B,h,w]) in float64."""
    g = R._d(g)
    return fold3(g), g[:, 0]


def blend_backward(o, a, b, gout, dtype=D):
    """out = a (1 - s) + s b, s = sigmoid(o) -> dict: g_o, g_a, g_b and A_o, A_a, A_b, evaluated in `dtype`."""
    o, a, b, g = (t.detach().to("cpu", dtype) for t in (o, a, b, gout))
    s = torch.sigmoid(o)
    ds = s * (1 - s)
    r = {"g_o": g * (b - a) * ds, "g_a": g * (1 - s), "g_b": g * s,
         "A_o": g.abs() * (b.abs() + a.abs()) * ds, "A_a": g.abs() * (1 - s), "A_b": g.abs() * s}
    return {k: v.to(D) for k, v in r.items()}


def gate(got, g64, g32):
    """The project's module gate (tests/test_conv2d_grad_gpu.parity_ratios) -> (max|got - g64|, the gate)."""
    e = float((got.double() - g64).abs().max())
    e32 = float((g32.double() - g64).abs().max())
    return e, max(4.0 * e32, 2e-5 * max(1.0, float(g64.abs().max())))
