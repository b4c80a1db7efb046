"""The multi-stage loss restated with plain torch ops, generic in dtype and device: boolean gathers and torch's
smooth_l1_loss, as the formulas of include/decnet_hip.h (decnet_stage_loss_forward) state them.  The yardstick of
tests/test_loss_cpu.py (against the recorded reference run), tests/test_loss_gpu.py (in float64) and tools/bench_loss.py
(in float32 on the GPU: what a training script runs without the fused kernels)."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


def downsample_gt(gt, ds, name):
    x = gt.unsqueeze(1)
    if name in ("bilinear", "bicubic"):
        return F.interpolate(x / ds, scale_factor=1 / ds, mode=name).squeeze(1)
    if name == "max":
        return F.max_pool2d(x / ds, ds, ds, 0, 1, False, False).squeeze(1)
    if name == "min":
        filled = (gt * (gt > 0) + 1e6 * (gt == 0)).unsqueeze(1)
        return -F.max_pool2d(-filled / ds, ds, ds, 0, 1, False, False).squeeze(1)
    raise ValueError(name)


def valid_mask(gt, gt_max, skip_rows):
    m = (gt < gt_max) & (gt > 0)
    if skip_rows > 0:
        m = m.clone()
        m[:, :skip_rows, :] = False
    return m


def _sl1(a, gt, mask, s):
    return F.smooth_l1_loss(a[mask] * s, gt[mask] * s, reduction="mean")


def stage_terms(pred, gt, gt_max, s=1.0, skip_rows=0, dense=None, sparse=None, fusion=None, soft_mask=None,
                left_mask=None):
    """The five means of one level as a list in the kernel's order (dense, sparse, soft-mask mean, fusion, pred); the
    simple form (no dense ... left_mask) gives zeros for the first four."""
    valid = valid_mask(gt, gt_max, skip_rows)
    p = _sl1(pred, gt, valid, s)
    if dense is None:
        z = torch.zeros((), dtype=pred.dtype, device=pred.device)
        return [z, z, z, z, p]
    left = left_mask == 1
    return [_sl1(dense, gt, valid, s), _sl1(sparse, gt, left & valid, s), soft_mask[left].mean(),
            _sl1(fusion, gt, valid, s), p]


def term_scale(pred, gt, gt_max, s=1.0, skip_rows=0, dense=None, sparse=None, fusion=None, soft_mask=None,
               left_mask=None):
    """X of the tolerance per term (same order): the largest |a s| or |gt s| over the term's masked pixels (0 where the
    mask is empty); for the soft-mask mean the largest |soft_mask| over its pixels."""
    valid = valid_mask(gt, gt_max, skip_rows)

    def big(a, m):
        if not bool(m.any()):
            return 0.0
        return float(torch.maximum((a.detach()[m].double() * s).abs().max(), (gt[m].double() * s).abs().max()))
    if dense is None:
        return [0.0, 0.0, 0.0, 0.0, big(pred, valid)]
    left = left_mask == 1
    return [big(dense, valid), big(sparse, left & valid), float(soft_mask.detach()[left].abs().max()) if bool(left.any()) else 0.0,
            big(fusion, valid), big(pred, valid)]


TERM_NAMES = ("dense", "sparse", "soft_mask", "fusion", "pred")      # the order of stage_terms and of the kernel's terms


def uploss(pred_list, fusion_list, dense_list, sparse_list, left_mask_list, gt, weights, num_stage, down_func_name,
           down_scale, max_disp, sparse_mask_list, if_overmask=False, stop_stage_id=4):
    """-> gt_list, tot_loss, loss_list, stages: stages[k] = (the keyword arguments stage_terms got at stage k,
    {term name: its position in loss_list})."""
    tot, gt_list, loss_list, stages = 0., [], [], []
    for k in range(num_stage):
        ds = down_scale ** (num_stage - k - 1) if k + 1 < num_stage else 1.
        cur_gt = downsample_gt(gt, ds, down_func_name) if k + 1 < num_stage else gt
        gt_list.append(cur_gt)
        kw = dict(pred=pred_list[k], gt=cur_gt, gt_max=max_disp / ds, s=ds, skip_rows=int(108 // ds) if if_overmask else 0)
        if not (k == 0 or k >= stop_stage_id):
            kw.update(dense=dense_list[k - 1], sparse=sparse_list[k - 1], fusion=fusion_list[k - 1],
                      soft_mask=sparse_mask_list[k - 1], left_mask=left_mask_list[k - 1])
        d, sp, sm, f, p = stage_terms(**kw)
        if "dense" in kw:
            stages.append((kw, {n: len(loss_list) + i for i, n in enumerate(TERM_NAMES)}))
            loss_list += [d, sp, sm, f, p]
            tot = tot + (p * 0.5 + d * 0.1 + sp * 0.2 * 1 / (10 + k * 3.75) + f * 0.2) * weights[k]
        else:
            stages.append((kw, {"pred": len(loss_list)}))
            loss_list.append(p)
            tot = tot + p * weights[k]
    return gt_list, tot, loss_list, stages


def upsampleloss(pred_list, gt, weights, num_stage, down_func_name, down_scale, max_disp):
    """-> as uploss; the `pred` of a stage record is the prediction interpolated to full resolution (its .grad is kept)."""
    tot, loss_list, stages = 0., [], []
    for k in range(num_stage):
        p = pred_list[k]
        if k + 1 < num_stage:
            ds = down_scale ** (num_stage - k - 1)
            p = F.interpolate(p.unsqueeze(1) * ds, scale_factor=ds, mode=down_func_name).squeeze(1)
            if p.requires_grad:
                p.retain_grad()
        kw = dict(pred=p, gt=gt, gt_max=max_disp, s=1.0, skip_rows=0)
        loss = stage_terms(**kw)[4]
        stages.append((kw, {"pred": len(loss_list)}))
        loss_list.append(loss)
        tot = tot + loss * weights[k]
    return [gt] * num_stage, tot, loss_list, stages


def term_gate(x, ref64):
    """|ours - ref64| allowed for a term: all accumulation is float64, so only the per-element fp32 roundings remain."""
    return 4 * EPS * x + 4 * EPS * abs(ref64)


# ---- the inputs of the recorded cases (tests/golden/loss_uploss.npz stores only their CRC32) ---------------------------
GOLDEN_B, GOLDEN_H, GOLDEN_W, GOLDEN_SCALE, GOLDEN_MAX_DISP = 2, 135, 81, 3, 216
GOLDEN_WEIGHTS = (0.5, 0.7, 1.0, 1.3)
# name -> (loss type, num_stage, down_func_name, if_overmask, stop_stage_id)
GOLDEN_CASES = {"up_%s_%s" % (f, "over" if o else "plain"): ("multi_stage_regression_uploss", 4, f, o, 4)
                for f in ("bilinear", "bicubic", "max", "min") for o in (False, True)}
GOLDEN_CASES["up_s3_stop2"] = ("multi_stage_regression_uploss", 3, "bicubic", False, 2)
GOLDEN_CASES["upsample_bilinear"] = ("multi_stage_regression_upsampleloss", 4, "bilinear", False, 4)


def golden_inputs(num_stage, seed=2024):
    """float32 numpy inputs from numpy's frozen RandomState stream (the same on every host): gt [B,H,W] with 30 % zeros
    and 1 % values above max_disp; per level a prediction = the strided pick of gt at that level + noise of sigma 0.3 (35 %) or
    5 (65 %) full-resolution pixels (both smooth-L1 branches at every level); for the stages 1.. dense / sparse / fusion
    likewise, a uniform soft mask and a left mask of 20 % ones.  -> dict of lists, coarsest first."""
    import numpy as np
    rs = np.random.RandomState(seed + num_stage)
    B, H, W, S = GOLDEN_B, GOLDEN_H, GOLDEN_W, GOLDEN_SCALE
    f32 = np.float32
    gt = (rs.rand(B, H, W) * 210 + 1).astype(f32)
    high = rs.rand(B, H, W) < 0.01
    gt[high] = (GOLDEN_MAX_DISP + rs.rand(int(high.sum())) * 50).astype(f32)
    gt[rs.rand(B, H, W) < 0.3] = 0
    out = dict(gt=gt, pred=[], dense=[], sparse=[], fusion=[], soft_mask=[], left_mask=[])

    def noisy(base, ds):
        sigma = np.where(rs.rand(*base.shape) < 0.35, 0.3, 5.0)
        return (base + (sigma * rs.standard_normal(base.shape) / ds).astype(f32)).astype(f32)
    for k in range(num_stage):
        ds = S ** (num_stage - k - 1)
        base = (gt[:, ds // 2::ds, ds // 2::ds] / f32(ds)).astype(f32)
        out["pred"].append(noisy(base, ds))
        if k > 0:
            for n in ("dense", "sparse", "fusion"):
                out[n].append(noisy(base, ds))
            out["soft_mask"].append(rs.rand(*base.shape).astype(f32))
            out["left_mask"].append((rs.rand(*base.shape) < 0.2).astype(f32))
    return out


def inputs_crc(inp):
    import zlib
    crc = zlib.crc32(inp["gt"].tobytes())
    for n in ("pred", "dense", "sparse", "fusion", "soft_mask", "left_mask"):
        for a in inp[n]:
            crc = zlib.crc32(a.tobytes(), crc)
    return crc


def objective(tot_loss, loss_list):
    """What the recorded gradients are the gradients of: tot_loss plus every entry of loss_list with a weight of its own
    (tot_loss alone leaves the soft-mask mean without a gradient)."""
    return tot_loss + sum((0.1 + 0.01 * j) * t for j, t in enumerate(loss_list))


GRAD_INPUTS = ("pred", "dense", "sparse", "fusion", "soft_mask")


def case_setup(case, dtype, device="cpu"):
    """-> (leaf tensors {input name: list}, keyword arguments of Loss.forward, keyword arguments of Loss())."""
    loss_type, num_stage, func, over, stop = GOLDEN_CASES[case]
    inp = golden_inputs(num_stage)

    def t(a):
        return torch.from_numpy(a).to(device=device, dtype=dtype)
    leaf = {n: [t(a).requires_grad_() for a in inp[n]] for n in GRAD_INPUTS}
    kwargs = dict(pred_list=list(leaf["pred"]), fusion_list=leaf["fusion"], dense_list=leaf["dense"],
                  sparse_list=leaf["sparse"], left_mask_list=[t(a) for a in inp["left_mask"]], gt=t(inp["gt"]),
                  weights=list(GOLDEN_WEIGHTS[:num_stage]), num_stage=num_stage, down_func_name=func,
                  down_scale=GOLDEN_SCALE, max_disp=GOLDEN_MAX_DISP, sparse_mask_list=leaf["soft_mask"])
    return leaf, kwargs, dict(loss_type=loss_type, if_overmask=over, stop_stage_id=stop)


def leaf_grads(leaf):
    return {"%s_%d" % (n, i): (t.grad if t.grad is not None else torch.zeros_like(t)).detach()
            for n in GRAD_INPUTS for i, t in enumerate(leaf[n])}


def restate(case, dtype, device="cpu"):
    """The restatement on a recorded case, forward and backward of `objective` -> dict(tot, loss_list, grads, stages,
    grad_terms = d objective / d loss_list[j], tot_coefs = d tot_loss / d loss_list[j], num_stage)."""
    leaf, kw, ctor = case_setup(case, dtype, device)
    if ctor["loss_type"].endswith("uploss"):
        _, tot, loss_list, stages = uploss(kw["pred_list"], kw["fusion_list"], kw["dense_list"], kw["sparse_list"],
                                           kw["left_mask_list"], kw["gt"], kw["weights"], kw["num_stage"],
                                           kw["down_func_name"], kw["down_scale"], kw["max_disp"], kw["sparse_mask_list"],
                                           ctor["if_overmask"], ctor["stop_stage_id"])
    else:
        _, tot, loss_list, stages = upsampleloss(kw["pred_list"], kw["gt"], kw["weights"], kw["num_stage"],
                                                 kw["down_func_name"], kw["down_scale"], kw["max_disp"])
    obj = objective(tot, loss_list)
    grad_terms = [float(g) for g in torch.autograd.grad(obj, loss_list, retain_graph=True)]
    tot_coefs = [0.0 if g is None else float(g)
                 for g in torch.autograd.grad(tot, loss_list, retain_graph=True, allow_unused=True)]
    obj.backward()
    return dict(tot=tot.detach(), loss_list=torch.stack([v.detach() for v in loss_list]), grads=leaf_grads(leaf),
                stages=stages, grad_terms=grad_terms, tot_coefs=tot_coefs, num_stage=kw["num_stage"], leaf=leaf)


# ---- the gates (eps = 2^-24) ---------------------------------------------------------------------------------------------
# All accumulation of the kernels is float64, so only the per-element fp32 roundings remain (a s, gt s, their difference):
#   a term:              |ours - ref64| <= 4 eps X + 4 eps |ref64|,  X = the largest |a s| or |gt s| over the term's pixels
#   a gradient element:  <= (|grad_term| s / n) 4 eps X + 4 eps |ref64|
#   the soft-mask plane: one float64 quotient rounded to fp32: 4 eps |ref64|
def _count(kw, name):
    valid = valid_mask(kw["gt"], kw["gt_max"], kw["skip_rows"])
    if name == "sparse":
        valid = valid & (kw["left_mask"] == 1)
    return int(valid.sum())


def term_gates(res64):
    """Per entry of loss_list, from a float64 `restate` result."""
    gates = [0.0] * len(res64["loss_list"])
    for kw, idx in res64["stages"]:
        x = dict(zip(TERM_NAMES, term_scale(**kw)))
        for name, j in idx.items():
            ref = float(res64["loss_list"][j])
            gates[j] = term_gate(x[name], ref) if ref == ref else 0.0
    return gates


def tot_gate(res64, gates):
    """tot_loss is combined in fp32 from the terms: each term's own gate times its coefficient, plus the roundings of the
    combination -- a term passes through at most 4 products and 8 running sums, 12 roundings of eps / 2 -- 8 eps sum |c t|."""
    c, t = res64["tot_coefs"], [float(v) for v in res64["loss_list"]]
    return sum(abs(cj) * g for cj, g in zip(c, gates)) + 8 * EPS * sum(abs(cj * tj) for cj, tj in zip(c, t) if cj != 0)


def grad_gates(res64):
    """{input key: gate plane} for a float64 `restate` result of an uploss case (every input feeds exactly one term)."""
    out = {}
    for k, (kw, idx) in enumerate(res64["stages"]):
        x = dict(zip(TERM_NAMES, term_scale(**kw)))
        for name, j in idx.items():
            key = "%s_%d" % (name, k if name == "pred" else k - 1)
            ref = res64["grads"][key].abs()
            if name == "soft_mask":
                out[key] = 4 * EPS * ref
                continue
            n = _count(kw, name)
            coef = abs(res64["grad_terms"][j]) * kw["s"] / n if n else 0.0
            out[key] = coef * 4 * EPS * x[name] + 4 * EPS * ref
    return out


def upsample_grad_gates(res64, down_scale=GOLDEN_SCALE, mode="bilinear"):
    """The upsample loss: the kernel's gradient is that of the full-resolution interpolated prediction (gate as above);
    torch's fp32 backward of `interpolate(pred * ds)` then adds, per coarse element, K <= (2 ds)^2 weighted contributions
    (bilinear weights are >= 0) and scales by ds.  So the gate of a coarse element is the interpolation's transpose T of
    the full-resolution gate, plus the worst case of an fp32 sum of K terms in any order, (K + 2) eps T(|g|)."""
    out, S = {}, res64["num_stage"]
    for k, (kw, idx) in enumerate(res64["stages"]):
        n = _count(kw, "pred")
        x = term_scale(**kw)[4]
        g_full = (kw["pred"].grad if k + 1 < S else res64["grads"]["pred_%d" % k]).abs()
        gate_full = abs(res64["grad_terms"][idx["pred"]]) / n * 4 * EPS * x + 4 * EPS * g_full
        if k + 1 == S:
            out["pred_%d" % k] = gate_full
            continue
        ds = down_scale ** (S - k - 1)
        q = torch.zeros_like(res64["leaf"]["pred"][k]).requires_grad_()

        def transpose(plane):
            up = F.interpolate(q.unsqueeze(1) * ds, scale_factor=ds, mode=mode).squeeze(1)
            return torch.autograd.grad((up * plane).sum(), q)[0]
        t_gate, t_abs = transpose(gate_full), transpose(g_full)
        out["pred_%d" % k] = t_gate + ((2 * ds) ** 2 + 2) * EPS * t_abs
    return out


def assert_within(got, ref64, gate, what):
    """NaN exactly where the reference is NaN; elsewhere |got - ref64| <= gate (a number or a tensor)."""
    got, ref64 = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref64).double().cpu()
    gate = torch.as_tensor(gate, dtype=torch.float64).cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    nan = torch.isnan(ref64)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN pattern differs" % what
    excess = ((got - ref64).abs() - gate.expand_as(ref64))[~nan]
    if excess.numel():
        worst = int(excess.argmax())
        assert float(excess.max()) <= 0, "%s: error %.3g over a gate of %.3g" % (
            what, float((got - ref64).abs()[~nan][worst]), float(gate.expand_as(ref64)[~nan][worst]))
