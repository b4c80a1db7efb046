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


# ---- Unit / ASPP routes: the rows of tests/test_model_routes_gpu.py (real tensors, spied entries, values) and
# tests/test_model_routes_cpu.py (the pure routing table).  ``route``: the route under the default switches and under
# DECNET_CONV2D_ACC=2; ``mfma0``: under DECNET_CONV2D_MFMA=0; under DECNET_CONV2D=torch every case is the library's. ----
def U(cin, cout, k=3, H=64, W=64, B=1, parts=None, route=None, mfma0="same", **kw):
    return dict(cin=cin, cout=cout, k=k, H=H, W=W, B=B, parts=parts, route=route, mfma0=route if mfma0 == "same" else mfma0,
                kw=kw)


T = dict(stride=3, transposed=True)
S3 = dict(stride=3)
UNIT_CASES = {
    # -> "mfma": H W 4096 | 4095; Cout 9 | 8 with Cin < 48; Cin 48 | 47 with Cout <= 8; Cin 16 | 15; dilation 4 | 5; k 1 and 3;
    # a tuple of 6 | 7 parts
    "mfma_hw4096": U(24, 24, route="mfma", mfma0=None), "mfma_hw4095": U(24, 24, H=63, W=65, route=None),
    "mfma_cout9": U(24, 9, route="mfma", mfma0=None), "mfma_cout8": U(24, 8, route="conv"),
    "mfma_cin48": U(48, 8, route="mfma", mfma0="conv"), "mfma_cin47": U(47, 8, route="conv"),
    "mfma_cin16": U(16, 12, route="mfma", mfma0=None), "mfma_cin15": U(15, 12, route=None),
    "mfma_cin15_dil2": U(15, 12, dil=2, route="conv"),
    "mfma_dil4": U(24, 24, dil=4, route="mfma", mfma0="conv"), "mfma_dil5": U(24, 24, dil=5, route="conv"),
    "mfma_k1": U(24, 24, k=1, route="mfma", mfma0=None), "mfma_k1_norelu": U(24, 10, k=1, relu=False, route="mfma", mfma0=None),
    "mfma_6parts": U(24, 24, parts=(4,) * 6, route="mfma", mfma0=None),
    "mfma_7parts": U(24, 24, parts=(4, 4, 4, 4, 4, 2, 2), route=None),
    "mfma_B3": U(24, 24, B=3, H=64, W=67, route="mfma", mfma0=None),
    # -> "mfma_s3": H W 4608 | 4607; Cout 25 | 24; Cin 8 | 7; H and W that are not multiples of 3
    "s3_hw4608": U(8, 25, H=72, W=64, route="mfma_s3", mfma0=None, **S3), "s3_hw4607": U(8, 25, H=17, W=271, route=None, **S3),
    "s3_cout24": U(8, 24, H=72, W=64, route="conv_s3", **S3), "s3_cin7": U(7, 25, H=72, W=64, route=None, **S3),
    "s3_ragged": U(8, 25, H=70, W=67, B=2, route="mfma_s3", mfma0=None, **S3),
    # -> "mfma_deconv": H W 512 | 511; Cout 9 | 8; Cin 64 | 63 with few outputs; Cin 16 | 15
    "dc_hw512": U(16, 9, H=16, W=32, route="mfma_deconv", mfma0=None, **T), "dc_hw511": U(16, 9, H=7, W=73, route=None, **T),
    "dc_cout8": U(16, 8, H=16, W=32, route="deconv", **T),
    "dc_cin64": U(64, 4, H=16, W=32, route="mfma_deconv", mfma0="deconv", **T), "dc_cin63": U(63, 4, H=16, W=32, route="deconv", **T),
    "dc_cin15": U(15, 9, H=16, W=32, route=None, **T),
    # -> "conv" / "conv_s3" / "deconv" / library: H W up 256 | 255; the output tiers 8 | 9 and 24 | 25; the
    # `cout > 8 and dil == 1 and cin > 12` exclusion both ways; bn=False with and without a bias; relu both ways
    "conv_hw256": U(4, 4, H=16, W=16, route="conv"), "conv_hw255": U(4, 4, H=15, W=17, route=None),
    "deconv_hw29": U(4, 4, H=1, W=29, route="deconv", **T), "deconv_hw28": U(4, 4, H=1, W=28, route=None, **T),
    "s3_hw256": U(4, 8, H=16, W=16, route="conv_s3", **S3), "s3_hw255": U(4, 8, H=15, W=17, route=None, **S3),
    "conv_cout8": U(8, 8, H=20, W=21, route="conv"), "conv_cout9": U(8, 9, H=20, W=21, route="conv"),
    "conv_cout24": U(8, 24, H=20, W=21, route="conv"), "conv_cout25": U(8, 25, H=20, W=21, route=None),
    "deconv_cout8": U(8, 8, H=6, W=7, route="deconv", **T), "deconv_cout9": U(8, 9, H=6, W=7, route=None, **T),
    "excl_cin13": U(13, 9, H=20, W=21, route=None), "excl_cin12": U(12, 9, H=20, W=21, route="conv"),
    "excl_dil2": U(13, 9, H=20, W=21, dil=2, route="conv"), "excl_cout8": U(13, 8, H=20, W=21, route="conv"),
    "nobn_bias": U(4, 4, H=20, W=21, bn=False, route="conv"),
    "nobn_nobias_norelu": U(4, 1, H=20, W=21, bn=False, bias=False, relu=False, route="conv"),
    "conv_norelu_cat": U(9, 3, H=20, W=21, B=2, parts=(8, 1), relu=False, route="conv"),
    "lib_nobn_bias": U(4, 4, H=9, W=9, bn=False, route=None), "lib_nobn_nobias": U(4, 4, H=9, W=9, bn=False, bias=False, route=None),
    # a BatchNorm eps that matters (0.3 against variances of 0.5 .. 1.5) through each of the three folds, and a
    # transposed library unit with Cin == Cout (where a scale along the wrong weight axis would still broadcast)
    "eps_mfma": U(24, 24, eps=0.3, route="mfma", mfma0=None), "eps_conv": U(8, 8, H=20, W=21, eps=0.3, route="conv"),
    "eps_s3": U(8, 25, H=72, W=64, eps=0.3, route="mfma_s3", mfma0=None, **S3),
    "eps_dc": U(16, 9, H=16, W=32, eps=0.3, route="mfma_deconv", mfma0=None, **T), "eps_lib": U(32, 32, H=10, W=10, eps=0.3, route=None),
    "lib_deconv_square": U(16, 16, H=5, W=5, route=None, **T),
    "lib_norelu": U(32, 32, H=10, W=10, B=2, relu=False, route=None), "lib_deconv": U(32, 16, H=5, W=5, route=None, **T),
}

ASPP_CASES = {  # (cin, cout, rates, (H, W), relu of branch 1, fused?)
    "hw16384": (8, 8, [1, 2, 3], (128, 128), True, True), "hw16385": (8, 8, [1, 2, 3], (113, 145), True, False),
    "cin_mod4": (6, 8, [1, 2, 3], (12, 12), True, False), "cout224": (4, 224, [1, 2, 3], (6, 7), True, True),
    "cout225": (4, 225, [1, 2, 3], (6, 7), True, False), "five_branches": (8, 8, [1, 2, 3, 4], (12, 12), True, False),
    "four_branches_dil12": (8, 8, [4, 8, 12], (20, 36), True, True), "a_branch_without_relu": (8, 8, [1, 2, 3], (12, 12), False, False),
}


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
