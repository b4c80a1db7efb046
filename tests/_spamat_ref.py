"""Float64 references of the SpaMat / SpaVar entries of include/decnet_hip.h, written from the header's formulas and the
reference's quirks, for tests/test_spamat_edges_gpu.py:
  - candidates d in [0, min(max_disp, x + 1)); a candidate is valid iff both masks are on (a mask is on iff it is != 0:
    -0.0 is off, a denormal is on);
  - max_cost = max(EPS, max_d cost_d), a constant of the backward (S7);
  - sums start at EPS (the kernels' 1e-6f): S = EPS + sum_d e_d,  out = (EPS + sum_d e_d d) / S,
    var = (EPS + sum_d e_d (d - mu)^2) / S,  e_d = exp(cost_d - max_cost);
  - ref mask off: 0 in every output; no valid candidate: out = var = 1.0 (EPS / EPS), S = max_cost = EPS.
Beside every forward output a float64 condition estimate is returned for the error bounds, from A_d = sum_c |l_c r_c| (a
bound of the rounding error of cost_d in units of the fp32 epsilon) and p_d = e_d / S:
  k_out = sum_d p_d |d - out| A_d,  k_var = sum_d p_d |(d - mu)^2 - var| A_d,  k_sum = sum_d p_d A_d + max_d A_d,
  k_max = max_d A_d   (over the valid candidates; 0 where there is none),
and the mean deviation dev = sum_d p_d |d - mu| of the variance, which scales its error from rounding d - mu.
The backwards are the closed forms of the reference kernels (SM_kernel.cu:143-195, 300-355; SV_kernel.cu:142-325) with
out / sum / max_cost taken as given.  Everything loops over d and keeps [D', B, H, W] planes (D' = min(D, W)), so rows of
~2100 pixels at D ~ 550 stay cheap.  CPU only."""
import numpy as np
import torch

F64 = torch.float64
EPS = float(np.float32(1e-6))


def mask_on(m):
    """The header's rule: on iff != 0 (evaluated on the float32 values as given: -0.0 off, denormals on)."""
    return torch.as_tensor(m).float() != 0


def _planes(ref, tar, rmask, tmask, D):
    """-> cost, A, valid: [D', B, H, W] with D' = min(D, W) (candidates d >= W are never valid)."""
    ref, tar = torch.as_tensor(ref).to(F64), torch.as_tensor(tar).to(F64)
    rm, tm = mask_on(rmask), mask_on(tmask)
    B, C, H, W = ref.shape
    n = min(int(D), W)
    cost = torch.zeros(n, B, H, W, dtype=F64)
    A = torch.zeros(n, B, H, W, dtype=F64)
    valid = torch.zeros(n, B, H, W, dtype=torch.bool)
    for d in range(n):
        prod = ref[..., d:] * tar[..., :W - d]                  # pixel x pairs with right pixel x - d
        cost[d, ..., d:] = prod.sum(1)
        A[d, ..., d:] = prod.abs().sum(1)
        valid[d, ..., d:] = rm[..., d:] & tm[..., :W - d]
    return cost, A, valid


def _dvec(n):
    return torch.arange(n, dtype=F64).view(n, 1, 1, 1)


def _softmax(cost, valid):
    mx = torch.where(valid, cost, torch.full_like(cost, -float("inf"))).amax(0).clamp_min(EPS)
    e = torch.where(valid, torch.exp(cost - mx), torch.zeros_like(cost))
    return mx, e, EPS + e.sum(0)


def forward(ref, tar, rmask, tmask, max_disp, disparity=None):
    """-> dict of float64 [B,H,W] planes: out, var_self (variance around out: the fused entry), S, max_cost, and the
    condition estimates k_out, k_var_self, k_sum, k_max and the mean deviations dev_self = sum_d p_d |d - out|; with
    `disparity` also var (SpaVar's), k_var and dev."""
    cost, A, valid = _planes(ref, tar, rmask, tmask, max_disp)
    n = cost.shape[0]
    on = mask_on(rmask)
    mx, e, S = _softmax(cost, valid)
    d = _dvec(n)
    p = e / S
    out = (EPS + (e * d).sum(0)) / S
    Amax = torch.where(valid, A, torch.zeros_like(A)).amax(0)

    def var_of(mu):
        dd2 = (d - mu) ** 2
        v = (EPS + (e * dd2).sum(0)) / S
        return v, (p * (dd2 - v).abs() * A).sum(0), (p * (d - mu).abs()).sum(0)

    r = {"out": out, "S": S, "max_cost": mx, "k_out": (p * (d - out).abs() * A).sum(0),
         "k_sum": (p * A).sum(0) + Amax, "k_max": Amax}
    r["var_self"], r["k_var_self"], r["dev_self"] = var_of(out)
    if disparity is not None:
        r["var"], r["k_var"], r["dev"] = var_of(torch.as_tensor(disparity).to(F64))
    z = torch.zeros_like(out)
    return {k: torch.where(on, v, z) for k, v in r.items()}


def backward(ref, tar, rmask, tmask, out, S, max_cost, grad_output, max_disp, disparity=None):
    """The closed-form backward with out / S / max_cost as given (the forward's fp32 results).  SpaMat (disparity None):
    -> grad_ref, grad_tar;  SpaVar (`out` is its variance, `disparity` its input): -> grad_ref, grad_tar, grad_disparity."""
    tar64 = torch.as_tensor(tar).to(F64)
    ref64 = torch.as_tensor(ref).to(F64)
    cost, _, valid = _planes(ref, tar, rmask, tmask, max_disp)
    n = cost.shape[0]
    out, S, mx, g = (torch.as_tensor(t).to(F64) for t in (out, S, max_cost, grad_output))
    e = torch.where(valid, torch.exp(cost - mx), torch.zeros_like(cost))
    d = _dvec(n)
    if disparity is None:
        w = g * e * (d - out) / S                                   # SM_kernel.cu:191, 351
    else:
        mu = torch.as_tensor(disparity).to(F64)
        w = g * e * ((d - mu) ** 2 - out) / S                       # SV_kernel.cu:191, 267
    w = torch.where(valid, w, torch.zeros_like(w))                  # (S is 0 at ref-off pixels)
    B, C, H, W = ref64.shape
    gl = torch.zeros(B, C, H, W, dtype=F64)
    gr = torch.zeros(B, C, H, W, dtype=F64)
    for k in range(n):
        gl[..., k:] += w[k, :, None, :, k:] * tar64[..., :W - k]
        gr[..., :W - k] += w[k, :, None, :, k:] * ref64[..., k:]
    if disparity is None:
        return gl, gr
    gd = -2.0 * g * (e * (d - mu)).sum(0) / S                       # SV_kernel.cu:321
    gd = torch.where(mask_on(rmask) & (S > 0), gd, torch.zeros_like(gd))
    return gl, gr, gd
