"""Float64 references of the stage-0 backward (csrc/conv3d_grad.hip, decnet_amd/stage0_grad.py) for
tests/test_stage0_grad_cpu.py and tests/test_stage0_grad_gpu.py: the case tables, the weight-gradient sums with their
absolute-value companions, and CostRegNetNoDown.stage0 under autograd with IMPOSED ReLU masks (y = pre * mask, as
tests/_conv2d_mfma_grad_ref.chain_grads).  CPU only; volumes are channels-last [B,D,H,W,C] as in the library."""
import copy

import torch
import torch.nn.functional as F

F64 = torch.float64
U32 = 2.0 ** -24
MAXSL, MINSL, NB = 4096, 256, 64            # csrc/conv3d_grad.hip: the slice (fp32 chain) bounds, the column block

# (B, D, H, W, Ci, Co) of decnet_conv3d_wgrad
WGRAD_CASES = [
    (1, 1, 1, 1, 4, 1), (2, 2, 3, 5, 12, 5), (1, 3, 1, 2, 36, 17), (1, 2, 2, 1, 216, 216), (1, 1, 2, 2, 224, 224),
    (1, 5, 7, 117, 4, 5),                   # 4095 voxels
    (1, 1, 17, 241, 4, 3),                  # 4097: 17 slices of 256, past the reduce's 16-way wrap
    (2, 3, 89, 131, 4, 5),                  # 69954 >= 17 * 4096 + 1
    # the kernel's own chain lengths (plan_sl below): slices of 256 at 255 | 257 voxels, of 1024 and of 4096 with a rest
    (1, 3, 5, 17, 4, 5), (1, 1, 1, 257, 4, 2), (1, 2, 75, 76, 216, 1), (1, 3, 128, 129, 216, 1),
]
WGRAD_IDS = ["%dx%dx%dx%d_%dto%d" % c for c in WGRAD_CASES]


def plan_sl(case):
    """-> (sl, nsets) as include/decnet_hip.h states the partition of decnet_conv3d_wgrad: slices of sl consecutive voxels,
    sl = 4096 halved down to 256 while ceil((27 Ci + 1) / 64) * ceil(V / sl) < 1024."""
    B, D, H, W, Ci, Co = case
    V, ncb, sl = B * D * H * W, -(-(27 * Ci + 1) // NB), MAXSL
    while sl > MINSL and ncb * -(-V // sl) < 1024:
        sl //= 2
    return sl, -(-V // sl)


def wgrad_data(case, exact, with_y=True):
    """-> x [B,D,H,W,Ci], gy, y [B,D,H,W,Co] (y None without ReLU), float32.  exact: integers in [-3, 3], y random-signed."""
    B, D, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(Ci * 1000 + Co * 10 + W + (0 if exact else 1))
    if exact:
        ri = lambda *s: torch.randint(-3, 4, s, generator=g).float()        # noqa: E731
        x, gy = ri(B, D, H, W, Ci), ri(B, D, H, W, Co)
    else:
        x, gy = torch.randn(B, D, H, W, Ci, generator=g), torch.randn(B, D, H, W, Co, generator=g)
    y = torch.randn(B, D, H, W, Co, generator=g)
    return x, gy, (y if with_y else None)


def _taps(x):
    """x [B,D,H,W,Ci] -> the 27 shifted volumes x[b,d+kd-1,h+kh-1,w+kw-1,ci] (zeros outside), tap = 9 kd + 3 kh + kw."""
    B, D, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                yield xp[:, kd:kd + D, kh:kh + H, kw:kw + W]


def wgrad(x, gy, y):
    """-> (G [Co,Ci,3,3,3], gsum [Co], gm [B,D,H,W,Co]) in float64, and the same sums over absolute values (SG, Ss)."""
    x, gy = x.to(F64), gy.to(F64)
    gm = gy if y is None else torch.where(y > 0, gy, torch.zeros((), dtype=F64))      # (a select: +0 where masked)
    Ci, Co = x.shape[-1], gy.shape[-1]
    a = gm.reshape(-1, Co)
    G = torch.stack([a.t() @ t.reshape(-1, Ci) for t in _taps(x)], -1).reshape(Co, Ci, 3, 3, 3)
    SG = torch.stack([a.abs().t() @ t.abs().reshape(-1, Ci) for t in _taps(x)], -1).reshape(Co, Ci, 3, 3, 3)
    return G, a.sum(0), gm, SG, a.abs().sum(0)


def flipped(w, scale):
    """w'[ci][co][kd][kh][kw] = w[co][ci][2-kd][2-kh][2-kw] scale[co], written out index by index."""
    Co, Ci = w.shape[:2]
    wt = torch.empty((Ci, Co, 3, 3, 3), dtype=w.dtype)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                wt[:, :, kd, kh, kw] = (w[:, :, 2 - kd, 2 - kh, 2 - kw] * scale.view(-1, 1)).t()
    return wt


def conv3d_cl(x, w):
    """Conv3d k 3, s 1, p 1 without bias on a channels-last volume."""
    return F.conv3d(x.permute(0, 4, 1, 2, 3), w, None, stride=1, padding=1).permute(0, 2, 3, 4, 1)


def dx(gm, w, scale):
    """dx of y = conv(x, w) scale for the gradient gm at y, float64: conv(gm, w')."""
    return conv3d_cl(gm.to(F64), flipped(w.to(F64), scale.to(F64)))


# ---- the module ---------------------------------------------------------------------------------------------------------------
# name: (C, cost_func, B, H, W, D, seed)
MODULE_CASES = {"c8_cor": (8, "cor", 2, 4, 5, 3, 4101), "c12_ssd": (12, "ssd", 2, 4, 5, 3, 4102),
                "c216_cor": (216, "cor", 1, 5, 6, 8, 4103)}


def module_case(name):
    """-> (CostRegNetNoDown(C, 2C, cost_func): float32, CPU, eval, seeded, BatchNorm statistics randomised; L, R [B,C,H,W]
    (ReLU'd features); D; r [B,H,W], r2 [B,D,H,W]: the weights of the loss (pred r).sum() + (reg r2).sum())."""
    import _model_cases as MC
    from decnet_amd import CostRegNetNoDown
    C, cf, B, H, W, D, seed = MODULE_CASES[name]
    mod = MC.seeded(lambda: CostRegNetNoDown(C, 2 * C, cf), seed)
    g = torch.Generator().manual_seed(seed + 7)
    L, R = (torch.relu(torch.randn(B, C, H, W, generator=g)) for _ in range(2))
    return mod, L, R, D, torch.randn(B, H, W, generator=g), torch.randn(B, D, H, W, generator=g)


def costvol(left, right, D, cost_func):
    """The cost volume of decnet_costvol_forward_cf in the dtype of its inputs, differentiable, with torch's grid_sample as
    the bilinear warp (zero padding): the sample of (d, y, x) lies at the pixel coordinates ((x - d) W / (W - 1) - 0.5,
    y H / (H - 1) - 0.5), in normalised ones (2 (x - d) / (W - 1) - 1, 2 y / (H - 1) - 1).  -> [B,D,H,W,C]."""
    B, C, H, W = left.shape
    dt = left.dtype
    gy, gx = torch.meshgrid(2 * torch.arange(H, dtype=dt) / (H - 1) - 1, torch.arange(W, dtype=dt), indexing="ij")
    out = []
    for d in range(D):
        grid = torch.stack((2 * (gx - d) / (W - 1) - 1, gy), -1).expand(B, H, W, 2)
        r = F.grid_sample(right, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        l = left * (torch.arange(W) >= d).to(dt)
        cost = l * r if cost_func == "cor" else (l * l + r * r) / 2 - ((l + r) / 2) ** 2
        out.append(cost.permute(0, 2, 3, 1))
    return torch.stack(out, 1)


def unit_pre(u, x):
    """The pre-activation of a Conv3dUnit in eval mode on NCDHW x: conv -> BatchNorm3d on the running statistics."""
    pre = F.conv3d(x, u.conv.weight, None, stride=1, padding=1)
    v = lambda p: p[None, :, None, None, None]                              # noqa: E731
    return (pre - v(u.bn.running_mean)) / torch.sqrt(v(u.bn.running_var) + u.bn.eps) * v(u.bn.weight) + v(u.bn.bias)


def regnet(mod, cv, masks=None):
    """CostRegNetNoDown.forward (submodule.py:650-662) on an NCDHW volume with the parameters of `mod` -> (reg [B,D,H,W],
    [pre-activation of every unit], [mask taken: bool NCDHW, None without ReLU]).  masks: impose these instead of pre > 0."""
    x, keep, pres, took = cv, None, [], []
    for i, u in enumerate(mod.units()):
        pre = unit_pre(u, x)
        pres.append(pre.detach())
        if not u.relu:
            took.append(None)
            y = pre
        elif masks is None:
            took.append(pre.detach() > 0)
            y = torch.relu(pre)
        else:
            took.append(masks[i])
            y = pre * masks[i].to(pre.dtype)
        x = y + keep if i == 4 else y
        if i == 1:
            keep = y
    return x[:, 0], pres, took


def stage0_grads(mod, L, R, D, r, r2, dtype, masks=None):
    """One run of (pred r).sum() + (reg r2).sum() through the cost volume, the eight units and the soft-argmax on a copy of
    `mod` in `dtype` on the CPU -> dict(grads: {name: gradient} over every parameter and "L", "R"; pred; reg; pre; took)."""
    mod = copy.deepcopy(mod).to("cpu", dtype).eval()
    Lc, Rc = (t.detach().to("cpu", dtype).clone().requires_grad_() for t in (L, R))
    cv = costvol(Lc, Rc, D, mod.cost_func).permute(0, 4, 1, 2, 3)
    reg, pres, took = regnet(mod, cv, masks)
    pred = (torch.softmax(reg, 1) * torch.arange(D, dtype=dtype).view(1, D, 1, 1)).sum(1)
    ((pred * r.to("cpu", dtype)).sum() + (reg * r2.to("cpu", dtype)).sum()).backward()
    grads = {n: p.grad.detach() for n, p in mod.named_parameters()}
    grads.update(L=Lc.grad.detach(), R=Rc.grad.detach())
    return dict(grads=grads, pred=pred.detach(), reg=reg.detach(), pre=pres, took=took)


def flips_within_gate(ref64, ref32, tol, factor=1.5):
    """Per ReLU'd unit of an imposed float64 run: the elements whose imposed mask differs from the free decision pre64 > 0
    of the same run (as `_stage_step_ref.mask_flips`), and whether every one of them has |pre64| within the forward gate
    of zero -- factor x the float32 run's distance to the
    float64 one, floor tol * max(1, max|pre64|) (`_model_cases.composite_bound`).  -> [(flips, worst |pre64| at a flip,
    bound)]; a unit passes when worst <= bound."""
    out = []
    for pre, pre32, took in zip(ref64["pre"], ref32["pre"], ref64["took"]):
        if took is None:
            continue
        diff = took != (pre > 0)
        bound = max(factor * float((pre32.double() - pre).abs().max()), tol * max(1.0, float(pre.abs().max())))
        out.append((int(diff.sum()), float(pre[diff].abs().max()) if bool(diff.any()) else 0.0, bound))
    return out
