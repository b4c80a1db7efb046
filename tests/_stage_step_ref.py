"""One training stage end to end -- DynamicUpsampling, SpaMat (+ the no_grad SpaVar), SoftAttention.fuse, Refinement, the
multi-stage loss, backward -- and its float64 reference.  A helper module of tests/test_stage_step_cpu.py (which holds the
reference against the modules' own torch routes, `_model_ref` and finite differences) and tests/test_stage_step_gpu.py.

The step is one composite stage of the reference's training forward (SparseDenseNetRefinementMask.py:148-236) into
multi_stage_regression_uploss (loss.py:168-242) with num_stage = 2, down_scale = 3 and the stage_id = 3 dilations:

    dense  = DynamicUpsampling(C, 3)(pred0, L)
    sparse = SpaMat(L, R, lmask, rmask, D)
    var    = SpaVar around sparse, no_grad (reference :183-192)
    fused  = SoftAttention(C + 4, 8).fuse(L, dense, sparse, lmask, var)
    pred   = Refinement(C, 8, stage_id=3)(L, R, fused)[0]
    tot    = uploss([pred0, pred], [fused], [dense], [sparse], [lmask], gt, [0.5, 1.0], 2, "bilinear", 3, D, [soft])

Leaves: L, R, pred0 and every parameter of the three modules.  `compose` is that sequence with the SpaMat, the SpaVar and
the loss as slots: `gpu_slots()` fills them with the package's public pieces (what a trainer writes), `cpu_slots()` with
the float64 restatements (`RefSpaMat`, `_spamat_ref.forward`, `_loss_ref.uploss`) around the modules' own torch routes.

`reference` is the same composition written out as formulas (those of tests/_model_ref.py, here in any dtype and with
autograd on), with two kinds of imposed data:
  * SpaMat planes: the forward may return the GPU run's sparse / S / max_cost / var; the backward is the closed form with
    those taken as given (`_spamat_ref.backward`'s own convention).  The GPU test holds the planes to `_spamat_ref.forward`
    separately, so a forward error cannot hide behind the imposition.
  * branch decisions: a unit's ReLU mask (the GPU run's own y > 0, as `_conv2d_mfma_grad_ref.chain_grads`) and the cell
    floor(ix) of the warp (from the GPU run's `fused`, the float32 grid of `_trunk_ref.warp_coords`).  Where an imposed
    decision differs from the free one the two runs differ by whole terms, not by rounding; the GPU test requires every
    such element to lie within the forward gate of zero (of the cell edge), `flips_within_gate`.
CPU only."""
import copy

import torch
import torch.nn.functional as F
from torch.autograd import Function

import _loss_ref as LR
import _model_cases as MC
import _spamat_ref as SR

D64 = torch.float64
WEIGHTS = [0.5, 1.0]
SCALE = 3
# small: the batch stride; every few-channel unit on "conv" (864 pixels), weight_learning (96 pixels) on the library.
# floor: 4224 coarse pixels, at the "mfma" floor (4096) and below the 6480 from which _mfma_grad_slower sends units back.
# The seeds are chosen for live networks: with four- and eight-channel units a random draw often leaves a whole unit of
# Refinement behind a dead ReLU, and its gradients then vanish (tests/test_stage_step_cpu.py holds every unit to >= 10 %
# active outputs).
CASES = {"small": dict(B=2, C=8, h=8, w=12, D=24, seed=3122), "floor": dict(B=1, C=8, h=64, w=66, D=48, seed=3128)}
MODULE_NAMES = ("up", "att", "ref")


# ---- the case: modules and data --------------------------------------------------------------------------------------------
def modules(case):
    """-> {"up": DynamicUpsampling(C, 3), "att": SoftAttention(C + 4, 8), "ref": Refinement(C, 8, stage_id=3)}: float32, CPU,
    eval mode, seeded, BatchNorm statistics randomised, a non-zero bias on the last unit of Refinement."""
    from decnet_amd.model import DynamicUpsampling, Refinement, SoftAttention
    c = CASES[case]
    C, seed = c["C"], c["seed"]
    mods = {"up": MC.seeded(lambda: DynamicUpsampling(C, SCALE), seed),
            "att": MC.seeded(lambda: SoftAttention(C + 4, 8), seed + 10),
            "ref": MC.seeded(lambda: Refinement(C, 8, stage_id=3), seed + 20)}
    mods["ref"].conv[-1].conv.bias.data = torch.randn(1, generator=torch.Generator().manual_seed(seed + 30)) * 0.3
    return mods


def row_density_masks(B, H, W, g):
    """Masks whose density changes per row, in turn all on, all off, 0.1 and 0.5: SpaMat's row routes."""
    dens = torch.tensor([1.0, 0.0, 0.1, 0.5])[torch.arange(H) % 4].view(1, H, 1)
    return (torch.rand(B, H, W, generator=g) < dens).float()


def data(case, variant=0, rows=False):
    """-> float32 CPU tensors L, R [B,C,H,W] (ReLU'd features, as the trunk hands them over), pred0 [B,h,w], gt, lmask,
    rmask, soft [B,H,W].  gt in [0, 0.9 D) with 30 % zeros; pred0 the downsampled gt plus unit noise, clamped at 0; masks
    Bernoulli(0.5), or with rows=True of a density that changes per row.  variant: another draw of everything."""
    c = CASES[case]
    B, C, h, w, D = c["B"], c["C"], c["h"], c["w"], c["D"]
    H, W = SCALE * h, SCALE * w
    g = torch.Generator().manual_seed(c["seed"] + 1000 * (variant + 1))
    t = {"L": torch.relu(torch.randn(B, C, H, W, generator=g)), "R": torch.relu(torch.randn(B, C, H, W, generator=g))}
    gt = torch.rand(B, H, W, generator=g) * 0.9 * D
    gt[torch.rand(B, H, W, generator=g) < 0.3] = 0
    t["gt"] = gt
    t["pred0"] = (LR.downsample_gt(gt, SCALE, "bilinear") + torch.randn(B, h, w, generator=g)).clamp_min(0).contiguous()
    if rows:
        t["lmask"], t["rmask"] = row_density_masks(B, H, W, g), row_density_masks(B, H, W, g).roll(1, 1)
    else:
        t["lmask"], t["rmask"] = ((torch.rand(B, H, W, generator=g) < 0.5).float() for _ in range(2))
    t["soft"] = torch.rand(B, H, W, generator=g)
    return t


LEAVES = ("L", "R", "pred0")


def named_parameters(mods):
    return {"%s.%s" % (k, n): p for k in MODULE_NAMES for n, p in mods[k].named_parameters()}


def relu_units(mods):
    """{name: Unit} of every unit with a ReLU, in forward order."""
    seqs = (("up.weight_learning", mods["up"].weight_learning), ("att.conv", mods["att"].conv), ("ref.conv", mods["ref"].conv))
    return {"%s.%d" % (n, i): u for n, s in seqs for i, u in enumerate(s) if u.relu}


# ---- the step with its slots ---------------------------------------------------------------------------------------------------
def compose(mods, t, D, spamat, spavar, loss):
    """-> dict(tot, dense, sparse, var, fused, pred): the sequence of the module docstring.  spamat(L, R, lmask, rmask, D) ->
    sparse; spavar(L, R, lmask, rmask, D, sparse) -> var (no gradient); loss(**the keywords of Loss.forward) -> tot."""
    dense = mods["up"](t["pred0"], t["L"])
    sparse = spamat(t["L"], t["R"], t["lmask"], t["rmask"], D)
    with torch.no_grad():
        var = spavar(t["L"], t["R"], t["lmask"], t["rmask"], D, sparse)
    fused = mods["att"].fuse(t["L"], dense, sparse, t["lmask"], var)
    pred = mods["ref"](t["L"], t["R"], fused)[0]
    tot = loss(pred_list=[t["pred0"], pred], fusion_list=[fused], dense_list=[dense], sparse_list=[sparse],
               left_mask_list=[t["lmask"]], gt=t["gt"], weights=WEIGHTS, num_stage=2, down_func_name="bilinear",
               down_scale=SCALE, max_disp=D, sparse_mask_list=[t["soft"]])
    return dict(tot=tot, dense=dense, sparse=sparse, var=var, fused=fused, pred=pred)


def gpu_slots():
    """The package's public pieces, as a trainer would write them."""
    import decnet_amd
    from decnet_amd import ops
    loss = decnet_amd.Loss("multi_stage_regression_uploss")
    return dict(spamat=decnet_amd.SpaMatFunction.apply,
                spavar=lambda L, R, lm, rm, D, sparse: ops.spamatvar_forward(L.detach(), R.detach(), lm, rm, D)[1],
                loss=lambda **kw: loss(**kw)[2])


class RefSpaMat(Function):
    """apply(L, R, lmask, rmask, D, planes) on the CPU in L's dtype: `_spamat_ref.forward` / `_spamat_ref.backward` (float64
    inside).  planes: None, or (out, S, max_cost) to return and differentiate around instead of the float64 forward's."""

    @staticmethod
    def forward(ctx, L, R, lmask, rmask, D, planes):
        if planes is None:
            r = SR.forward(L, R, lmask, rmask, D)
            planes = (r["out"], r["S"], r["max_cost"])
        out, S, mx = (p.detach().to("cpu", D64) for p in planes)
        ctx.save_for_backward(L, R, lmask, rmask, out, S, mx)
        ctx.D = int(D)
        return out.to(L.dtype)

    @staticmethod
    def backward(ctx, g):
        L, R, lmask, rmask, out, S, mx = ctx.saved_tensors
        gl, gr = SR.backward(L, R, lmask, rmask, out, S, mx, g, ctx.D)
        return gl.to(L.dtype), gr.to(R.dtype), None, None, None, None


def spamat_out_fixed_max(L, R, lmask, rmask, D, mx):
    """The disparity of `_spamat_ref.forward` with max_cost given instead of recomputed (quirk S7: a constant of the
    backward), in float64: what RefSpaMat.backward is the derivative of."""
    cost, _, valid = SR._planes(L, R, lmask, rmask, D)
    e = torch.where(valid, torch.exp(cost - mx.to(D64)), torch.zeros_like(cost))
    out = (SR.EPS + (e * SR._dvec(cost.shape[0])).sum(0)) / (SR.EPS + e.sum(0))
    return torch.where(SR.mask_on(lmask), out, torch.zeros_like(out))


def cpu_slots(planes=None, var=None):
    """The float64 restatements (any dtype outside): RefSpaMat, the fused entry's variance (around the disparity that
    `_spamat_ref.forward` computes itself), `_loss_ref.uploss`."""
    def spavar(L, R, lm, rm, D, sparse):
        v = SR.forward(L, R, lm, rm, D)["var_self"] if var is None else var
        return v.detach().to("cpu", L.dtype)

    def loss(**kw):
        return LR.uploss(kw["pred_list"], kw["fusion_list"], kw["dense_list"], kw["sparse_list"], kw["left_mask_list"],
                         kw["gt"], kw["weights"], kw["num_stage"], kw["down_func_name"], kw["down_scale"], kw["max_disp"],
                         kw["sparse_mask_list"])[1]
    return dict(spamat=lambda L, R, lm, rm, D: RefSpaMat.apply(L, R, lm, rm, D, planes), spavar=spavar, loss=loss)


def to(mods, t, device, dtype):
    """Copies of the modules and the data on `device` in `dtype`, the leaves requiring a gradient."""
    mods = {k: copy.deepcopy(m).to(device=device, dtype=dtype).eval() for k, m in mods.items()}
    t = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(k in LEAVES) for k, v in t.items()}
    return mods, t


def grads_of(mods, t):
    g = {n: p.grad.detach().cpu().clone() for n, p in named_parameters(mods).items()}
    g.update({k: t[k].grad.detach().cpu().clone() for k in LEAVES})
    return g


def torch_step(mods, t, D, dtype=D64):
    """The step on the modules' own torch routes on the CPU in `dtype` with cpu_slots() -> (planes, gradients)."""
    mods, t = to(mods, t, "cpu", dtype)
    out = compose(mods, t, D, **cpu_slots())
    out["tot"].backward()
    return {k: v.detach() for k, v in out.items()}, grads_of(mods, t)


# ---- the reference: the formulas of tests/_model_ref.py in any dtype, under autograd, with imposed decisions -----------------
def _unit(x, u, name, imposed, rec):
    """submodule.py:15-87, eval mode: conv -> (y - mean) / sqrt(var + eps) gamma + beta -> ReLU (or the imposed mask)."""
    c, bn = u.conv, u.bn
    pre = F.conv2d(x, c.weight, c.bias, stride=c.stride, padding=c.padding, dilation=c.dilation)
    if bn is not None:
        v = lambda p: p[None, :, None, None]                                                     # noqa: E731
        pre = (pre - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)
    if not u.relu:
        return pre
    free = pre.detach() > 0
    mask = imposed.get(name, free) if imposed is not None else free
    rec["pre"][name], rec["free"][name], rec["took"][name] = pre.detach(), free, mask
    return pre * mask.to(pre.dtype)


def _seq(x, seq, name, imposed, rec):
    for i, u in enumerate(seq):
        x = _unit(x, u, "%s.%d" % (name, i), imposed, rec)
    return x


def _dynamic_upsampling(disp, fea, m, imposed, rec):
    """_model_ref.dynamic_upsampling (submodule.py:566-589, down_scale 3)."""
    B, h, w = disp.shape
    C = fea.shape[1]
    s2d = fea.view(B, C, h, 3, w, 3).permute(0, 1, 3, 5, 2, 4).reshape(B, 9 * C, h, w)
    logits = _seq(torch.cat((disp.unsqueeze(1), s2d), 1), m.weight_learning, "up.weight_learning", imposed, rec)
    wts = torch.softmax(logits.view(B, 9, 9, h, w), 2)
    pad = F.pad(disp.unsqueeze(1), (1, 1, 1, 1), mode="replicate")[:, 0]
    nb = torch.stack([pad[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)
    up = (wts * nb.unsqueeze(1)).sum(2)
    return 3 * up.view(B, 3, 3, h, w).permute(0, 3, 1, 4, 2).reshape(B, 3 * h, 3 * w)


def _fuse(fea, dense, sparse, lmask, var, m, imposed, rec):
    """_model_ref.fuse (submodule.py:593-604, SparseDenseNetRefinementMask.py:195-202)."""
    x = torch.cat((fea, dense.unsqueeze(1), sparse.unsqueeze(1), lmask.unsqueeze(1), -var.unsqueeze(1)), 1)
    soft = torch.sigmoid(_seq(x, m.conv, "att.conv", imposed, rec)).squeeze(1)
    return dense * (1 - soft) + soft * sparse


def warp_ix(disp, W):
    """The x sampling position, through the normalised coordinate as `_trunk_ref.warp_coords` (and grid_sample) build it."""
    xs = torch.arange(W, dtype=disp.dtype).view(1, 1, W)
    cx = (xs - disp) / ((W - 1.0) / 2.0) - 1.0
    return ((cx + 1.0) * W - 1.0) / 2.0


def cells_of(fused32, W):
    """floor(ix) [B,H,W] (float64 integers) of the float32 grid of a float32 disparity plane: the cells the kernel reads."""
    return torch.floor(warp_ix(fused32.detach().to("cpu", torch.float32), W)).to(D64)


def _warp(right, disp, cells, rec):
    """_model_ref.warp (submodule.py:719-745): bilinear, zero padding, half-pixel-shifted; the weights as functions of disp
    (autograd carries g_disp), the cell x0 = floor(ix) or as imposed -- outside its own cell the same linear piece."""
    B, C, H, W = right.shape
    dt = right.dtype
    ix = warp_ix(disp, W)
    cy = torch.arange(H, dtype=dt) / ((H - 1.0) / 2.0) - 1.0
    iy = (((cy + 1.0) * H - 1.0) / 2.0).view(1, H, 1).expand(B, H, W)
    free = torch.floor(ix.detach())
    x0 = free if cells is None else cells.to(dt)
    rec["ix"], rec["cells_free"], rec["cells_took"] = ix.detach(), free, x0
    y0 = torch.floor(iy)
    flat = right.reshape(B, C, H * W)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wx = (ix - x0) if dx else (1 - (ix - x0))
            wy = (iy - y0) if dy else (1 - (iy - y0))
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, 1, H * W).expand(B, C, H * W)
            v = torch.gather(flat, 2, idx).reshape(B, C, H, W)
            out = out + torch.where(ok.unsqueeze(1), v * (wx * wy).unsqueeze(1), torch.zeros((), dtype=dt))
    return out


def _refinement(left, right, disp, m, imposed, cells, rec):
    """_model_ref.refinement (submodule.py:748-762)."""
    x = torch.cat((left, _warp(right, disp, cells, rec), disp.unsqueeze(1)), 1)
    return disp + _seq(x, m.conv, "ref.conv", imposed, rec).squeeze(1)


def reference(mods, t, D, dtype=D64, imposed=None):
    """The step as formulas on the CPU in `dtype`.  imposed: None (the free run), or a dict with any of
        planes: (sparse, S, max_cost) and var: the GPU run's SpaMat / SpaVar planes;
        masks: {unit name: bool [B,Cout,H,W]}; cells: floor(ix) of the warp [B,H,W].
    -> dict(planes: tot / dense / sparse / var / fused / pred; grads: {name: gradient} over every parameter and L, R, pred0;
    g_sp: the part of L's and R's gradient that arrives through the SpaMat node alone; rec: per ReLU'd unit the
    pre-activation, the free mask and the mask taken, and the warp's ix, free and taken cells)."""
    imposed = imposed or {}
    mods, t = to(mods, t, "cpu", dtype)
    rec = {"pre": {}, "free": {}, "took": {}}
    masks = imposed.get("masks")
    Lsp, Rsp = (t[k].detach().clone().requires_grad_() for k in ("L", "R"))      # SpaMat's own leaves: g_sp
    dense = _dynamic_upsampling(t["pred0"], t["L"], mods["up"], masks, rec)
    sparse = RefSpaMat.apply(Lsp, Rsp, t["lmask"], t["rmask"], D, imposed.get("planes"))
    var = cpu_slots(var=imposed.get("var"))["spavar"](Lsp.detach(), Rsp.detach(), t["lmask"], t["rmask"], D, sparse)
    fused = _fuse(t["L"], dense, sparse, t["lmask"], var, mods["att"], masks, rec)
    pred = _refinement(t["L"], t["R"], fused, mods["ref"], masks, imposed.get("cells"), rec)
    tot = LR.uploss([t["pred0"], pred], [fused], [dense], [sparse], [t["lmask"]], t["gt"], WEIGHTS, 2, "bilinear", SCALE, D,
                    [t["soft"]])[1]
    tot.backward()
    g_sp = {"L": Lsp.grad.detach().clone(), "R": Rsp.grad.detach().clone()}
    t["L"].grad += Lsp.grad
    t["R"].grad += Rsp.grad
    planes = dict(tot=tot, dense=dense, sparse=sparse, var=var, fused=fused, pred=pred)
    return dict(planes={k: v.detach() for k, v in planes.items()}, grads=grads_of(mods, t), g_sp=g_sp, rec=rec)


# ---- the guard of the imposed decisions -------------------------------------------------------------------------------------
def mask_flips(ref64, ref32, tol_of, factor=1.5):
    """Per ReLU'd unit of an imposed float64 run: the elements where the mask taken differs from the free one, and whether
    every one of them has |pre64| within the unit's forward gate, `_model_cases.composite_bound` of the pre-activation
    (factor x the float32 run's distance, floor tol_of(name) * max(1, max|pre64|)).  -> {name: (flips, worst |pre64| at
    a flip, the bound)}."""
    out = {}
    for name, pre in ref64["rec"]["pre"].items():
        diff = ref64["rec"]["took"][name] != ref64["rec"]["free"][name]
        bound = MC.composite_bound(pre, ref32["rec"]["pre"][name], factor, tol_of(name))
        out[name] = (int(diff.sum()), float(pre[diff].abs().max()) if bool(diff.any()) else 0.0, bound)
    return out


def cell_flips(ref64, ref32, factor=1.5):
    """The same for the warp's cells: a pixel whose imposed cell differs from floor(ix64) must have ix64 within the
    forward gate of `fused`, carried to ix (W / (W - 1)) plus four float32 roundings of a coordinate up to W, of the
    edge between the two cells.  -> (flips, worst distance to that edge, the bound)."""
    rec = ref64["rec"]
    ix, free, took = rec["ix"], rec["cells_free"], rec["cells_took"]
    W = ix.shape[-1]
    f64, f32 = ref64["planes"]["fused"], ref32["planes"]["fused"]
    bound = MC.composite_bound(f64, f32, factor) * W / (W - 1.0) + 4 * 2.0 ** -24 * W
    diff = took != free
    edge = torch.maximum(took, free)                                # neighbouring cells n - 1 | n meet at ix = n
    far = (took - free).abs() > 1
    dist = torch.where(far, torch.full_like(ix, float("inf")), (ix - edge).abs())
    return int(diff.sum()), float(dist[diff].max()) if bool(diff.any()) else 0.0, bound
