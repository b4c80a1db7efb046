"""Plain float64 references of the stage-0 entries of include/decnet_hip.h (csrc/stage0.hip, conv3d_winograd.hip,
stage0_entry.hip), written from the header's formulas.  CPU only; every function takes and returns float64 tensors
(inputs of other types are converted).  Volumes are channels-last [B,D,H,W,C] as in the library; feature maps NCHW.
Checked against independent formulations by tests/test_stage0_ref_cpu.py."""
import torch
import torch.nn.functional as F

F64 = torch.float64
COST = {"cor": 0, "ssd": 1, "cat": 2, "sum": 3}
BN_EPS = 1e-5


def _d(t):
    return t.to(F64) if torch.is_tensor(t) else torch.tensor(t, dtype=F64)


def warp(right, D):
    """bilinear(right[b,c]; xs, ys) for every disparity d < D: xs = (x-d) W/(W-1) - 0.5, ys = y H/(H-1) - 0.5, zero
    padding.  right [B,C,H,W] -> [B,D,H,W,C]."""
    r = _d(right)
    B, C, H, W = r.shape
    assert H >= 2 and W >= 2, "the formula divides by H - 1 and W - 1"
    ys = torch.arange(H, dtype=F64) * H / (H - 1) - 0.5
    y0 = torch.floor(ys)
    wy1 = ys - y0
    y0 = y0.long()
    out = torch.zeros(B, D, H, W, C, dtype=F64)
    rc = r.permute(0, 2, 3, 1)                                                   # [B,H,W,C]
    for d in range(D):
        xs = (torch.arange(W, dtype=F64) - d) * W / (W - 1) - 0.5
        x0 = torch.floor(xs)
        wx1 = xs - x0
        x0 = x0.long()
        for dy, wy in ((0, 1 - wy1), (1, wy1)):
            yy = y0 + dy
            oky = (yy >= 0) & (yy < H)
            for dx, wx in ((0, 1 - wx1), (1, wx1)):
                xx = x0 + dx
                okx = (xx >= 0) & (xx < W)
                v = rc[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]         # [B,H,W,C]
                wgt = (wy * oky)[:, None] * (wx * okx)[None, :]                  # [H,W]
                out[:, d] += v * wgt[None, :, :, None]
    return out


def costvol(left, right, D, cost_func):
    """The cost volume of decnet_costvol_forward_cf: l = (x >= d ? left : 0), r = warp(right); COR l r, SSD
    (l^2 + r^2)/2 - ((l + r)/2)^2, CAT [l, r] (2C channels), SUM l + r.  -> [B,D,H,W,C] (2C for CAT)."""
    cf = COST.get(cost_func, cost_func)
    lf = _d(left)
    B, C, H, W = lf.shape
    r = warp(right, D)
    keep = (torch.arange(W)[None, :] >= torch.arange(D)[:, None]).to(F64)       # [D,W]
    l = lf.permute(0, 2, 3, 1)[:, None] * keep[None, :, None, :, None]          # [B,D,H,W,C]
    if cf == 0:
        return l * r
    if cf == 1:
        return (l * l + r * r) / 2 - ((l + r) / 2) ** 2
    if cf == 2:
        return torch.cat((l, r), dim=-1)
    if cf == 3:
        return l + r
    raise ValueError(cost_func)


def pointwise(x, w, ldw, channels_last):
    """decnet_conv3d_pointwise: y[b,co,p] = sum_ci w[co ldw + ci] x[b,ci,p]; x [B,Ci,P] or [B,P,Ci] (channels_last)."""
    x = _d(x)
    Ci = x.shape[2] if channels_last else x.shape[1]
    wf = _d(w).reshape(-1)
    Co = (wf.numel() - Ci) // ldw + 1
    wm = torch.stack([wf[co * ldw:co * ldw + Ci] for co in range(Co)])           # [Co,Ci]
    return x @ wm.t() if channels_last else torch.einsum("oc,bcp->bop", wm, x)


def conv3d_unit(x, w, scale, shift, residual=None, relu=True):
    """One Conv3dUnit channels-last: act(conv3d_k3_s1_p1(x) scale + shift) (+ residual after the activation).
    x [B,D,H,W,Ci], w [Co,Ci,3,3,3] -> [B,D,H,W,Co]."""
    y = F.conv3d(_d(x).permute(0, 4, 1, 2, 3), _d(w), None, stride=1, padding=1).permute(0, 2, 3, 4, 1)
    y = y * _d(scale) + _d(shift)
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + _d(residual)
    return y


def stack(x, layers, n, res_src=-1, res_dst=-1):
    """decnet_conv3d_wino_stack_bn_act: n units with ReLU, layers[i] = (w, scale, shift); the output of layer res_src is
    added to the output of layer res_dst after its ReLU."""
    cur, keep = _d(x), None
    for i in range(n):
        w, s, h = layers[i]
        cur = conv3d_unit(cur, w, s, h, keep if i == res_dst else None, True)
        if i == res_src:
            keep = cur
    return cur


def softargmax(cost, samples):
    """sum_s softmax_s(cost) samples along dim 1."""
    return (torch.softmax(_d(cost), dim=1) * _d(samples)).sum(1)


def cout1_softargmax(x, w, scale, shift):
    """decnet_conv3d_cout1_softargmax: reg = conv(x, w[1,Ci,3,3,3]) scale + shift [B,D,H,W]; pred = soft-argmax of reg
    over arange(D).  Returns (reg, pred)."""
    reg = conv3d_unit(x, _d(w).reshape(1, -1, 3, 3, 3), _d(scale).reshape(1), _d(shift).reshape(1), None, False)[..., 0]
    D = reg.shape[1]
    return reg, softargmax(reg, torch.arange(D, dtype=F64).view(1, D, 1, 1))


def disparity_regression(cost, samples):
    """decnet_disparity_regression: cost, samples [B,S,H,W] -> [B,H,W]."""
    return softargmax(cost, samples)


def ncdhw_to_ndhwc(x):
    return _d(x).permute(0, 2, 3, 4, 1).contiguous()


def ndhwc_to_ncdhw(x):
    return _d(x).permute(0, 4, 1, 2, 3).contiguous()


def fold_bn(bn):
    """(gamma, beta, running_mean, running_var) -> (scale, shift) of eval-mode BatchNorm3d."""
    g, b, m, v = (_d(t) for t in bn)
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale


def stage0(left, right, params, D, cost_func="cor", w_pre=None):
    """decnet_stage0_forward_cf the way CostRegNetNoDown.forward composes it: cost volume (CAT: the 2C-channel volume,
    then conv_pre w_pre [C,2C,1,1,1]), seven units with the residual from unit 1 onto unit 4, the last unit (no ReLU)
    and the soft-argmax over arange(D).  params: 8 tuples (w, scale, shift), the last with w [1,C,3,3,3] and scalar
    scale / shift.  Returns (reg [B,D,H,W], pred [B,H,W])."""
    cv = costvol(left, right, D, cost_func)
    if COST.get(cost_func, cost_func) == 2:
        wp = _d(w_pre).reshape(w_pre.shape[0], -1)
        cv = pointwise(cv.reshape(cv.shape[0], -1, cv.shape[-1]), wp, wp.shape[1], True).reshape(*cv.shape[:4], -1)
    y = stack(cv, params, 7, 1, 4)
    w, s, h = params[7]
    return cout1_softargmax(y, w, s, h)
