"""Seeded modules and inputs shared by tests/test_model_ref_cpu.py (CPU) and tests/test_model_routes_gpu.py /
tests/test_model_state_gpu.py (GPU), so that what the CPU test asserts about a case (e.g. that the float64 reference
alone leaves at most 1 % of a mask case's pixels undecided) is asserted about the very case the GPU test runs."""
import torch

import _model_ref as MR

FP32_TOL = 2e-5            # small fp32 kernels: 2e-5 * max(1, max|ref|)   (tests/test_conv2d_gpu.py, test_trunk_edges_gpu.py)
MFMA_TOL = 4e-6            # bf16x3 matrix-core kernels
S3_TOL = 1e-5              # stride-3 convolution on the matrix cores (test_conv2d_gpu.py)
ASPP_TOL = 3e-5            # tap-conv


def randomise_bn(module, g):
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
            n = m.num_features
            m.weight.data = torch.rand(n, generator=g) + 0.5
            m.bias.data = torch.randn(n, generator=g) * 0.2
            m.running_mean.data = torch.randn(n, generator=g) * 0.2
            m.running_var.data = torch.rand(n, generator=g) + 0.5
    return module


def seeded(ctor, seed):
    """A module built under its own seed, BatchNorm statistics randomised, in eval mode."""
    torch.manual_seed(seed)
    return randomise_bn(ctor(), torch.Generator().manual_seed(seed + 1)).eval()


def make_unit(cin, cout, k, stride=1, dil=1, relu=True, bn=True, transposed=False, bias=True, eps=None, seed=0):
    from decnet_amd.model import Unit
    pad = 0 if transposed else (1 if stride == 3 else dil * (k // 2))
    u = seeded(lambda: Unit(cin, cout, k, stride=stride, pad=pad, dil=dil, relu=relu, bn=bn, transposed=transposed), seed)
    if eps is not None:
        u.bn.eps = eps
    if not bn:
        if bias:
            u.conv.bias.data = torch.randn(cout, generator=torch.Generator().manual_seed(seed + 2)) * 0.3
        else:
            u.conv.bias = None
    return u


def close(got, ref, tol):
    """|got - ref| <= tol * max(1, max|ref|) everywhere; returns the worst ratio to that bound."""
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max()) / (tol * max(1.0, float(ref.abs().max())))


def composite_bound(ref64, out32, factor, tol=FP32_TOL):
    """The project's yardstick for a composite module (tests/test_inputdata_gpu.py): factor x the distance of torch's own
    float32 run (the module's torch route on the CPU) to the float64 reference, with the single-layer bound as floor."""
    return max(factor * float((out32.double() - ref64).abs().max()), tol * max(1.0, float(ref64.abs().max())))


# ---- GenerateSparseMask ---------------------------------------------------------------------------------------------
# mask() runs on an exact x3 pair (cur [B,C,H,W], pre [B,3C,H/3,W/3]), so H and W are multiples of 3: the widths below
# sit on either side of one, four and sixteen 64-pixel words of the bit plane (63 | 66, 192 = 3 words exactly | 195,
# 255 | 258, 1023 | 1026) and at the smallest plane; the C entry itself is tested at W = 1, 63, 64, 65, 129 in
# tests/test_trunk_edges_gpu.py.
MASK_CASES = [(3, 3), (3, 63), (6, 66), (3, 192), (6, 195), (3, 255), (6, 258), (3, 1023), (3, 1026)]


def mask_case(H, W, B=2, C=4, quant=0.5):
    """-> (module, cur, pre, thold).  thold is chosen from the float64 reference alone: the middle of the widest gap
    between neighbouring sigmoid values around the `quant` quantile, so that few decisions are close calls."""
    from decnet_amd.model import GenerateSparseMask
    gen = seeded(lambda: GenerateSparseMask(C, 3), 1000 * H + W)
    for u in (gen.deconv[0], gen.conv_sub[0]):                 # bn=False units: a non-zero bias
        u.conv.bias.data.normal_(0, 0.3)
    g = torch.Generator().manual_seed(H + 7 * W)
    cur = torch.randn(B, C, H, W, generator=g)
    pre = torch.randn(B, 3 * C, H // 3, W // 3, generator=g)
    _, logit = MR.mask(cur, pre, MR.maskgen_params(gen), 0.5)
    s = torch.sigmoid(logit).flatten().sort().values
    i = int(quant * (s.numel() - 1))
    lo, hi = max(0, i - 8), min(s.numel() - 1, i + 8)
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    j = lo + int(gaps.argmax())
    return gen, cur, pre, float((s[j] + s[j + 1]) / 2)


def mask_margin(gen, cur, pre, logit64, factor=1.5):
    """Bound of the logit (the composite yardstick on the module's float32 torch route) for MR.mask_unsure."""
    with torch.no_grad():
        l32 = gen.float().cpu()(cur, pre)
    return composite_bound(logit64, l32, factor)
