"""Plain float64 torch-CPU references of the 2-D trunk entries of include/decnet_hip.h (the "2-D trunk" and tap-conv
sections), written from the formulas stated there.  A helper module of tests/test_trunk_ref_cpu.py (which checks each
one against an independent formulation) and tests/test_trunk_edges_gpu.py (which compares the HIP entries with them).

Every function takes and returns CPU tensors; inputs are promoted to float64.  Layouts are the ones of the header:
NCHW feature maps, [B,H,W] planes, weights in torch layout.
"""
import torch

D = torch.float64


def _d(t):
    return t.detach().to("cpu", D)


def conv(xs, w, dil=1):
    """Conv2d k = 1 or 3, stride 1, padding dil * (k // 2), no bias, on the channel concatenation of xs
    (a tensor or a sequence of [B,c_i,H,W]); w [Cout,Cin,k,k].  A sum of shifted planes, one per tap."""
    x = torch.cat([_d(t) for t in xs], 1) if isinstance(xs, (list, tuple)) else _d(xs)
    w = _d(w)
    B, C, H, Wd = x.shape
    k = w.shape[-1]
    p = dil * (k // 2)
    xp = torch.zeros(B, C, H + 2 * p, Wd + 2 * p, dtype=D)
    xp[:, :, p:p + H, p:p + Wd] = x
    y = torch.zeros(B, w.shape[0], H, Wd, dtype=D)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky * dil:ky * dil + H, kx * dil:kx * dil + Wd]
            y += torch.einsum("bchw,oc->bohw", win, w[:, :, ky, kx])
    return y


def bn_act(y, scale, shift, relu):
    """act(y * scale[c] + shift[c]) per channel of [B,C,H,W]."""
    y = _d(y) * _d(scale)[None, :, None, None] + _d(shift)[None, :, None, None]
    return torch.relu(y) if relu else y


def conv_bn_act(xs, w, scale, shift, dil=1, relu=True):
    """decnet_conv2d_bn_act / decnet_conv2d_cat_bn_act / decnet_conv2d_mfma_cat_bn_act."""
    return bn_act(conv(xs, w, dil), scale, shift, relu)


def epilogue(v, epi, ea, eb=None):
    """The fused tails of decnet_conv2d_cat_epilogue on the one-channel layer output v [B,1,H,W] (after BN / act):
    1: s = sigmoid(v), ea (1 - s) + s eb;  2: ea + v.  Returns [B,1,H,W]."""
    v, ea = _d(v)[:, 0], _d(ea)
    if epi == 1:
        s = torch.sigmoid(v)
        out = ea * (1 - s) + s * _d(eb)
    else:
        out = ea + v
    return out.unsqueeze(1)


def s2d3_pad1(x):
    """decnet_s2d3_pad1: out[b, 9c + 3ky + kx, yo, xo] = x[b, c, 3yo - 1 + ky, 3xo - 1 + kx], 0 outside."""
    x = _d(x)
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 3 + 1, (W - 1) // 3 + 1
    xp = torch.zeros(B, C, 3 * Ho + 2, 3 * Wo + 2, dtype=D)      # one zero row / column in front, enough behind
    xp[:, :, 1:1 + H, 1:1 + W] = x
    out = torch.empty(B, C, 9, Ho, Wo, dtype=D)
    for ky in range(3):
        for kx in range(3):
            out[:, :, 3 * ky + kx] = xp[:, :, ky:ky + 3 * Ho:3, kx:kx + 3 * Wo:3]
    return out.reshape(B, 9 * C, Ho, Wo)


def conv_s3_bn_act(x, w, scale, shift, relu=True):
    """decnet_conv2d_k3s3_bn_act: Conv2d k 3, stride 3, padding 1 (w [Cout,Cin,3,3]) + BN + act."""
    w = _d(w)
    y = torch.einsum("bkhw,ok->bohw", s2d3_pad1(x), w.reshape(w.shape[0], -1))
    return bn_act(y, scale, shift, relu)


def deconv_s3_bn_act(x, w, scale, shift, relu=True):
    """decnet_deconv2d_k3s3_bn_act / decnet_deconv2d_mfma_k3s3_bn_act: ConvTranspose2d k 3, stride 3, padding 0,
    w [Cin,Cout,3,3]: out[b, co, 3y + ky, 3x + kx] = sum_ci x[b, ci, y, x] w[ci, co, ky, kx]; then BN + act."""
    x, w = _d(x), _d(w)
    B, _, H, W = x.shape
    t = torch.einsum("bchw,coij->bohiwj", x, w)                   # [B,Cout,H,3,W,3]
    return bn_act(t.reshape(B, w.shape[1], 3 * H, 3 * W), scale, shift, relu)


def warp_coords(disp, H, W, dtype=D):
    """Sampling position of decnet_warp_disparity: ix = (x - d) W / (W - 1) - 0.5, iy = y H / (H - 1) - 0.5, through
    the normalised coordinate the reference builds (submodule.py:719-745: cx = (x - d) / ((W - 1) / 2) - 1, then
    grid_sample's unnormalisation ((cx + 1) W - 1) / 2).  dtype = float32 evaluates that chain with the float32 rounding
    of every step, as the reference does (its grid is a float32 tensor); the result is returned as float64."""
    disp = disp.detach().to("cpu", dtype)
    B = disp.shape[0]
    xs = torch.arange(W, dtype=dtype).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=dtype).view(1, H, 1).expand(B, H, W)
    cx = (xs - disp) / ((W - 1.0) / 2.0) - 1.0
    cy = ys / ((H - 1.0) / 2.0) - 1.0
    ix = ((cx + 1.0) * W - 1.0) / 2.0
    iy = ((cy + 1.0) * H - 1.0) / 2.0
    return ix.to(D), iy.to(D)


def warp_disparities(B, H, W, g):
    """Disparity planes [B,H,W] (float64) of every kind the warp is tested with: exact integers, negative, samples with
    ix in (-1, 0) and in (W-1, W) (one tap inside the image), beyond it, 1e6, and a spread over [-W/2, 3W/2)."""
    xs = torch.arange(W, dtype=D).view(1, 1, W)
    r = lambda: torch.rand(B, H, W, generator=g, dtype=D)
    return [torch.randint(-3, W + 3, (B, H, W), generator=g).to(D),
            -r() * 5,
            xs + (0.45 - 0.9 * r()) * (W - 1) / W,               # ix = (x - d) W / (W - 1) - 0.5 = -1 + u, u in (.05, .95)
            xs - (W - 0.45 + 0.9 * r()) * (W - 1) / W,           # ix = W - 1 + u
            torch.full((B, H, W), 1e6, dtype=D),
            r() * 2 * W - W / 2]


def warp(right, disp, coord_dtype=D):
    """decnet_warp_disparity: out[b,c,y,x] = bilinear(right[b,c]; ix, iy) with zero padding (warp_coords)."""
    r = _d(right)
    B, C, H, W = r.shape
    ix, iy = warp_coords(disp, H, W, coord_dtype)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros(B, C, H, W, dtype=D)
    flat = r.reshape(B, C, H * W)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (1 - (ix - xi).abs()) * (1 - (iy - yi).abs())
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, 1, H * W).expand(B, C, H * W)
            v = torch.gather(flat, 2, idx).reshape(B, C, H, W)
            out += torch.where(ok.unsqueeze(1), v * wgt.unsqueeze(1), torch.zeros((), dtype=D))
    return out


def dynamic_upsample3(logits, disp):
    """decnet_dynamic_upsample3: logits [B,81,h,w] (channel 9 s + k: sub-position s = 3 sy + sx, neighbour k = 3 ky +
    kx), disp [B,h,w] -> out[b, 3y + sy, 3x + sx] = 3 sum_k softmax_k(logits[b, 9 s + k, y, x]) n_k(y, x), n_k the
    replicate-padded neighbour disp[b, clamp(y + ky - 1), clamp(x + kx - 1)]."""
    lg, d = _d(logits), _d(disp)
    B, h, w = d.shape
    ys, xs = torch.arange(h), torch.arange(w)
    nb = torch.stack([d[:, (ys + ky - 1).clamp(0, h - 1)][:, :, (xs + kx - 1).clamp(0, w - 1)]
                      for ky in range(3) for kx in range(3)], 1)          # [B,9,h,w]
    wts = torch.softmax(lg.view(B, 9, 9, h, w), 2)                       # [B, s, k, h, w]
    up = (wts * nb.unsqueeze(1)).sum(2)                                  # [B, s, h, w]
    return 3 * up.view(B, 3, 3, h, w).permute(0, 3, 1, 4, 2).reshape(B, 3 * h, 3 * w)


def unfold3_cat(fea, disp):
    """decnet_unfold3_cat: out[b,0] = disp, out[b, 1 + 9c + 3i + j, y, x] = fea[b, c, 3y + i, 3x + j]."""
    f, d = _d(fea), _d(disp)
    B, C, H3, W3 = f.shape
    h, w = H3 // 3, W3 // 3
    t = f.view(B, C, h, 3, w, 3).permute(0, 1, 3, 5, 2, 4).reshape(B, 9 * C, h, w)
    return torch.cat((d.unsqueeze(1), t), 1)


def bias_act(y, shift, relu):
    """decnet_bias_act_inplace: act(y[b,c] + shift[c])."""
    y = _d(y) + _d(shift)[None, :, None, None]
    return torch.relu(y) if relu else y


def detail_logits(cur3, pre3, w3, scale3, shift3, w1, scale1, shift1):
    """`detail` of decnet_detail_mask: res = (cur - pre)^2 -> conv 3x3 (padding 1) * scale3 + shift3 -> the 1x1
    conv w1 [3] -> * scale1 + shift1.  Returns [B,H,W]."""
    res = (_d(cur3) - _d(pre3)) ** 2
    t = bn_act(conv(res, w3, 1), scale3, shift3, False)
    z = torch.einsum("bchw,c->bhw", t, _d(w1))
    return z * float(scale1) + float(shift1)


def pack_bits(mask):
    """[B,H,W] bool -> [B,H,ceil(W/64)] int64 words, bit i of word w = pixel 64 w + i, zero past W."""
    B, H, W = mask.shape
    nw = (W + 63) // 64
    m = torch.zeros(B, H, nw * 64, dtype=torch.bool)
    m[:, :, :W] = mask
    m = m.view(B, H, nw, 64).to(torch.int64)
    words = (m << torch.arange(64, dtype=torch.int64)).sum(-1)             # two's complement wrap gives bit 63
    return words


def tap_gemm(x, ws):
    """decnet_tap_gemm on the values of decnet_tapconv_to_chunks / _pack_weight: for every tap t (branches in order,
    taps ky-major) T[t][b, co, y, x] = sum_ci x[b, ci, y, x] w_br[co, ci, ky, kx].  ws: list of [Co,Ci,k,k]."""
    x = _d(x)
    T = []
    for w in ws:
        w = _d(w)
        k = w.shape[-1]
        for t in range(k * k):
            T.append(torch.einsum("bchw,oc->bohw", x, w[:, :, t // k, t % k]))
    return T


def tap_gather(T, ks, dils, scale, shift, relu):
    """decnet_tapconv_gather: y[b, br Co + co, y, x] = act(scale * sum_{t of br} T[t][b, co, y + dy_t, x + dx_t] + shift),
    taps whose position (y + dy, x + dx) is outside the image skipped; dy, dx = (ky - k // 2) dil, (kx - k // 2) dil."""
    outs, t0 = [], 0
    for k, dil in zip(ks, dils):
        B, Co, H, W = T[t0].shape
        acc = torch.zeros(B, Co, H, W, dtype=D)
        for t in range(k * k):
            dy, dx = (t // k - k // 2) * dil, (t % k - k // 2) * dil
            ys, ye = max(0, -dy), min(H, H - dy)                          # output rows whose tap row is inside
            xs, xe = max(0, -dx), min(W, W - dx)
            if ys < ye and xs < xe:
                acc[:, :, ys:ye, xs:xe] += T[t0 + t][:, :, ys + dy:ye + dy, xs + dx:xe + dx]
        outs.append(acc)
        t0 += k * k
    y = torch.cat(outs, 1)
    return bn_act(y, scale, shift, relu)
