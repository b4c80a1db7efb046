"""Cases and float64 references of GenerateSparseMask.detail and SoftAttention.fuse(want_soft=True).  A helper module of
tests/test_detail_grad_cpu.py (which holds what is asserted here about the cases: the 1 % cap of excused pixels on the
float64 reference alone, the success of the margin search, live gradients) and tests/test_detail_grad_gpu.py.

References are the modules' own torch routes in float64 on the CPU (``detail`` / ``fuse`` outside ``hip_grad()``) and
tests/_model_ref.py.  CPU only.

Value cases: `MC.mask_case` as it is.  In eval mode its threshold is the case's own; in train mode `thold_of` restates
mask_case's widest-gap rule on the float64 train-mode run.

Gradient cases: the two ReLU'd units of the generator (``conv_sub[0]``, ``deconv[0]``; neither has BatchNorm, so the
margins do not depend on the mode) see 13 000 to 98 000 pre-activations per case, and a standard-normal draw leaves some as
close to zero as 3e-6 to 3e-5 -- below `BR.MARGIN`, where a float32 run may take the other branch and differ from float64 by
a whole term.  A fresh draw of everything cannot clear the margin at these counts (some 5 to 35 offenders are expected per
draw), so a data variant is a repair of the one before: variant 0 is mask_case's draw, variant k + 1 redraws, under its own
seed, the input pixels (all channels) behind variant k's offenders -- the centre pixel of a 3 x 3 window of ``cur``, the one
source pixel of a stride-3 transposed tap of ``pre``.  `grad_case` keeps the first of the variants 0..15 whose float64
pre-activations all clear ``BR.MARGIN * max(1, max|pre|)``."""
import copy

import torch

import _bn_train_ref as BR
import _model_cases as MC

D = torch.float64
SHAPES = [(6, 66), (6, 195), (3, 1026)]
MODES = ("eval", "train")
CAP = 0.01                                              # at most 1 % of the pixels may be excused
VARIANTS = 16
_CACHE = {}


def in_mode(m, mode):
    return m.train() if mode == "train" else m.eval()


def copy_of(gen, mode, dtype=D, device="cpu"):
    return in_mode(copy.deepcopy(gen).to(device=device, dtype=dtype), mode)


def thold_of(logit64, quant=0.5):
    """mask_case's rule: the middle of the widest gap between neighbouring sigmoid values around the `quant` quantile."""
    s = torch.sigmoid(logit64.detach()).flatten().sort().values
    i = int(quant * (s.numel() - 1))
    lo, hi = max(0, i - 8), min(s.numel() - 1, i + 8)
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    j = lo + int(gaps.argmax())
    return float((s[j] + s[j + 1]) / 2)


def logits_of(gen, cur, pre, mode, dtype):
    """The module's torch route on the CPU in `dtype`, on a copy (train mode updates running statistics)."""
    with torch.no_grad():
        return copy_of(gen, mode, dtype)(cur.to(dtype), pre.to(dtype))


def value_case(H, W, mode):
    """-> dict(gen, cur, pre, thold, logit64, logit32, bound): mask_case's module and data, the threshold of `mode`, the
    float64 / float32 logits of the torch route on the CPU and the composite bound of the logit (factor 1.5)."""
    key = ("value", H, W, mode)
    if key not in _CACHE:
        gen, cur, pre, thold = MC.mask_case(H, W)
        l64 = logits_of(gen, cur, pre, mode, D)
        if mode == "train":
            thold = thold_of(l64)
        l32 = logits_of(gen, cur, pre, mode, torch.float32)
        _CACHE[key] = dict(gen=gen, cur=cur, pre=pre, thold=thold, logit64=l64, logit32=l32,
                           bound=MC.composite_bound(l64, l32, 1.5))
    return _CACHE[key]


def unsure(case):
    import _model_ref as MR
    return MR.mask_unsure(case["logit64"], case["thold"], case["bound"])


# ---- the gradient cases: data whose ReLU decisions are not close calls ---------------------------------------------------------
def relu_pre(gen, cur, pre):
    """float64 pre-activations of the two ReLU'd units -> (conv_sub[0]: [B,8,H,W], deconv[0]: [B,8,H,W])."""
    g = copy.deepcopy(gen).double()
    with torch.no_grad():
        return g.conv_sub[0].conv(cur.double()), g.deconv[0].conv(pre.double())


def offenders(p):
    """[B,H,W] bool: pixels with a pre-activation (any channel) within the margin of zero."""
    return (p.abs() <= BR.MARGIN * max(1.0, float(p.abs().max()))).any(1)


def variants(H, W):
    """Yields (k, cur, pre, number of offending pixels) for k = 0..VARIANTS-1 (see the module docstring)."""
    gen, cur, pre, _ = MC.mask_case(H, W)
    cur, pre = cur.clone(), pre.clone()
    for k in range(VARIANTS):
        pc, pp = relu_pre(gen, cur, pre)
        oc, op = offenders(pc), offenders(pp)
        yield k, cur.clone(), pre.clone(), int(oc.sum()) + int(op.sum())
        g = torch.Generator().manual_seed(100000 * (k + 1) + 1000 * H + W)
        b, y, x = oc.nonzero(as_tuple=True)
        cur[b, :, y, x] = torch.randn(b.numel(), cur.shape[1], generator=g)
        B, h, w = pre.shape[0], pre.shape[2], pre.shape[3]
        b, y, x = op.view(B, h, 3, w, 3).any(4).any(2).nonzero(as_tuple=True)      # each source pixel once
        pre[b, :, y, x] = torch.randn(b.numel(), pre.shape[1], generator=g)


def grad_data(H, W):
    """-> (gen, cur, pre, variant) of the first variant without offenders; variant None: the search failed."""
    key = ("data", H, W)
    if key not in _CACHE:
        gen = MC.mask_case(H, W)[0]
        _CACHE[key] = (gen, None, None, None)
        for k, cur, pre, bad in variants(H, W):
            if bad == 0:
                _CACHE[key] = (gen, cur, pre, k)
                break
    return _CACHE[key]


def loss_weights(H, W, B=2):
    return torch.randn(B, H, W, generator=torch.Generator().manual_seed(31 * H + W))


def detail_step(gen, cur, pre, thold, r, ctx=None, want_bits=False):
    """One forward + backward of (prob * r).sum() through gen.detail on the tensors as they are -> (prob, mask, bits)."""
    import contextlib
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        prob, mask, bits = gen.detail(cur, pre, thold, want_bits)
    (prob * r).sum().backward()
    return prob, mask, bits


def detail_grads(gen, cur, pre, thold, r, mode, dtype, device="cpu", ctx=None):
    """One step on a copy of `gen` in `mode` -> ({name: gradient on the CPU} over "cur", "pre" and every parameter, {buffer
    name: value after the step}, prob, mask)."""
    m = copy_of(gen, mode, dtype, device)
    c = cur.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    p = pre.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    prob, mask, _ = detail_step(m, c, p, thold, r.to(device=device, dtype=dtype), ctx)
    grads = {n: q.grad.detach().cpu() for n, q in m.named_parameters()}
    grads.update(cur=c.grad.detach().cpu(), pre=p.grad.detach().cpu())
    return grads, {n: b.detach().cpu().clone() for n, b in m.named_buffers()}, prob.detach().cpu(), mask.detach().cpu()


def grad_case(H, W, mode):
    """-> dict(gen, cur, pre, variant, thold, r, g64, g32, buf64) of the gradient case, the float64 and float32 CPU runs of
    the torch route included (once per case)."""
    key = ("grad", H, W, mode)
    if key not in _CACHE:
        gen, cur, pre, k = grad_data(H, W)
        assert k is not None, "no data variant clears the ReLU margin at %s" % ((H, W),)
        thold = thold_of(logits_of(gen, cur, pre, mode, D))
        r = loss_weights(H, W)
        g64, buf64, _, _ = detail_grads(gen, cur, pre, thold, r, mode, D)
        g32, _, _, _ = detail_grads(gen, cur, pre, thold, r, mode, torch.float32)
        _CACHE[key] = dict(gen=gen, cur=cur, pre=pre, variant=k, thold=thold, r=r, g64=g64, g32=g32, buf64=buf64)
    return _CACHE[key]


# ---- SoftAttention.fuse(want_soft=True) ------------------------------------------------------------------------------------------
def fuse_pre(m, ins, mode):
    """float64 BatchNorm outputs of the ReLU'd units of SoftAttention `m` in `mode` on the torch route -> {unit: [B,C,H,W]}."""
    m = copy_of(m, mode)
    pres, hooks = {}, []
    for un, u in m.conv.named_children():
        if u.relu and u.bn is not None:
            hooks.append(u.bn.register_forward_hook(lambda mod, i, o, un=un: pres.__setitem__(un, o.detach())))
    t = {k: v.double() for k, v in ins.items()}
    with torch.no_grad():
        m.fuse(t["fea"], t["dense"], t["sparse"], t["mask"], t["var"])
    for h in hooks:
        h.remove()
    return pres


def fuse_variants(mode):
    """Yields (k, inputs, offending pixels) for k = 0..VARIANTS-1: variant 0 is `BR.module_case("attention")`'s data (chosen
    there for its train-mode margins; with the running statistics of eval mode one pre-activation of ``conv[1]`` sits at
    3e-6), variant k + 1 redraws ``fea`` at the pixels of variant k's offenders, as `variants` does."""
    m, ins, _, _ = BR.module_case("attention")
    ins = {k: v.clone() for k, v in ins.items()}
    for k in range(VARIANTS):
        bad = torch.stack([offenders(p) for p in fuse_pre(m, ins, mode).values()]).any(0)
        yield k, {n: v.clone() for n, v in ins.items()}, int(bad.sum())
        g = torch.Generator().manual_seed(200000 * (k + 1) + 17)
        b, y, x = bad.nonzero(as_tuple=True)
        ins["fea"][b, :, y, x] = torch.randn(b.numel(), ins["fea"].shape[1], generator=g)


def fuse_case(mode):
    """`BR.module_case("attention")`'s module (a copy in `mode`) and the first data variant whose float64 pre-activations
    clear the margin in `mode` -> (module, inputs, wrt, r1, r2, variant); variant None: the search failed."""
    key = ("fuse", mode)
    if key not in _CACHE:
        m, ins, wrt, r1 = BR.module_case("attention")
        r2 = torch.randn(r1.shape, generator=torch.Generator().manual_seed(4242))
        found = next(((k, v) for k, v, bad in fuse_variants(mode) if bad == 0), (None, ins))
        _CACHE[key] = (m, found[1], wrt, r1, r2, found[0])
    m, ins, wrt, r1, r2, k = _CACHE[key]
    return in_mode(copy.deepcopy(m), mode), ins, wrt, r1, r2, k


def fuse_grads(m, ins, wrt, r1, r2, mode, dtype, device="cpu", ctx=None):
    """One step of (fused * r1 + soft * r2).sum() (r1 None: soft alone) on a copy of `m` -> (gradients on the CPU over the
    parameters and `wrt`, fused, soft, the autograd node names reachable from the loss)."""
    import contextlib
    m = copy_of(m, mode, dtype, device)
    t = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(k in wrt) for k, v in ins.items()}
    with (ctx() if ctx is not None else contextlib.nullcontext()):
        fused, soft = m.fuse(t["fea"], t["dense"], t["sparse"], t["mask"], t["var"], want_soft=True)
    loss = (soft * r2.to(soft)).sum()
    if r1 is not None:
        loss = loss + (fused * r1.to(fused)).sum()
    names = node_names(loss)
    loss.backward()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}
    grads.update({k: t[k].grad.detach().cpu() for k in wrt if t[k].grad is not None})
    return grads, fused.detach().cpu(), soft.detach().cpu(), names


def node_names(t):
    """Names of the autograd nodes reachable from tensor t, with repetitions."""
    seen, names, stack = set(), [], [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        stack.extend(n for n, _ in f.next_functions)
    return names
