// decnet_amd/csrc/unfold.hip -- head of DynamicUpsampling.forward (modules/submodule.py:578-580):
//     torch.cat((disp.unsqueeze(1), F.unfold(fea, 3, stride=3).view(B, 9C, h, w)), 1)
// a space-to-depth of the fine-level features (channel c*9 + i*3 + j = fea[c, 3y+i, 3x+j]) behind the coarse
// disparity plane, as one pass (the stock path is im2col + a view + a concatenation copy).
#include "common.h"

namespace {
__global__ __launch_bounds__(256) void unfold3_cat(const float *__restrict__ fea, const float *__restrict__ disp,
                                                   float *__restrict__ out, int C, int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int b = blockIdx.z / (C + 1), c = blockIdx.z - b * (C + 1);   // c == C: the disparity plane
    if (x >= w) return;
    const size_t cp = (size_t)h * w;                                    // coarse plane
    float *o = out + ((size_t)b * (9 * C + 1)) * cp + (size_t)y * w + x;
    if (c == C) {
        o[0] = disp[((size_t)b * h + y) * w + x];
        return;
    }
    const float *f = fea + (((size_t)b * C + c) * 3 * h + 3 * y) * (3 * (size_t)w) + 3 * x;
    float v[9];                                     // nine requests, then nine stores
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i * 3 + j] = f[(size_t)i * 3 * w + j];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) o[(size_t)(1 + c * 9 + t) * cp] = v[t];
}
// The stride-3 convolutions of FeatExtNetChannelPlus (Conv2d k 3, stride 3, padding 1: submodule.py:270-300) as a
// space-to-depth gather in front of a 1 x 1 convolution on the matrix cores (csrc/conv2d_mfma.hip):
//     out[b, c*9 + ky*3 + kx, yo, xo] = x[b, c, 3 yo - 1 + ky, 3 xo - 1 + kx]   (0 outside the image)
// -- every input pixel feeds exactly one output pixel, so this is a permutation with a zero border; the channel order
// is the row-major flattening of the weight [Cout, Cin, 3, 3].
__global__ __launch_bounds__(256) void s2d3_pad1(const float *__restrict__ x, float *__restrict__ out, int C, int H, int W,
                                                 int Ho, int Wo) {
    const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
    const int b = blockIdx.z / C, c = blockIdx.z - b * C;
    if (xo >= Wo) return;
    const size_t cp = (size_t)Ho * Wo;
    float *o = out + ((size_t)b * 9 * C + 9 * c) * cp + (size_t)yo * Wo + xo;
    const float *f = x + ((size_t)b * C + c) * H * (size_t)W;
    float v[9];                                     // nine requests, then nine stores (a store right behind its load
#pragma unroll                                      // is a memory round trip per tap: round 5, from the ISA)
    for (int ky = 0; ky < 3; ++ky) {
        const int yi = 3 * yo - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int xi = 3 * xo - 1 + kx;
            v[ky * 3 + kx] = (yi >= 0 && yi < H && xi >= 0 && xi < W) ? f[(size_t)yi * W + xi] : 0.f;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) o[(size_t)t * cp] = v[t];
}
// The two layout passes of the stride-3 layers' input gradients (decnet_amd/conv2d_grad.py).  A workgroup moves SEG = 768
// consecutive floats of one fine row through LDS: the fine side goes in 16-byte units where the tensor's address and the
// row length allow it (vec), the coarse side as three coalesced dword streams, one per kx.
constexpr int SEG = 768;

// dx[b,c,r,s] = t[b, 9c + 3 ((r+1) % 3) + (s+1) % 3, (r+1) / 3, (s+1) / 3], zero where (r+1) / 3 = Ho or (s+1) / 3 = Wo:
// the adjoint of s2d3_pad1.  Fine column s0 + 3 tx + j is (xo, kx) = (s0 / 3 + tx, j + 1) for j < 2, (s0 / 3 + tx + 1, 0) for j = 2.
__global__ __launch_bounds__(256) void d2s3_pad1(const float *__restrict__ t, float *__restrict__ dx, int C, int H, int W,
                                                 int Ho, int Wo, int vec) {
    __shared__ __attribute__((aligned(16))) float row[SEG];
    const int tx = threadIdx.x, r = blockIdx.y, s0 = blockIdx.x * SEG;
    const int b = blockIdx.z / C, c = blockIdx.z - b * C;
    const int yo = (r + 1) / 3, ky = r + 1 - 3 * yo, xo = s0 / 3 + tx;
    const size_t cp = (size_t)Ho * Wo;
    const float *tp = t + ((size_t)b * 9 * C + 9 * c + 3 * ky) * cp + (size_t)min(yo, Ho - 1) * Wo;
    const bool in0 = yo < Ho && xo < Wo, in1 = yo < Ho && xo + 1 < Wo;
    const float v0 = in0 ? tp[cp + xo] : 0.f, v1 = in0 ? tp[2 * cp + xo] : 0.f, v2 = in1 ? tp[xo + 1] : 0.f;
    row[3 * tx] = v0;
    row[3 * tx + 1] = v1;
    row[3 * tx + 2] = v2;
    __syncthreads();
    float *o = dx + (((size_t)b * C + c) * H + r) * W + s0;
    const int n = min(SEG, W - s0);
    if (vec) {
        int e = 4 * tx;
        if (e + 3 < n) *reinterpret_cast<float4 *>(o + e) = *reinterpret_cast<const float4 *>(row + e);
        else if (tx < SEG / 4)
            for (; e < n; ++e) o[e] = row[e];
    } else {
        for (int e = tx; e < n; e += 256) o[e] = row[e];
    }
}

// out[b, 9c + 3a + j, i, x] = g[b, c, 3i + a, 3x + j]: the space-to-depth of a ConvTranspose2d k 3, stride 3 (padding 0)
__global__ __launch_bounds__(256) void s2d3_pad0(const float *__restrict__ g, float *__restrict__ out, int C, int H, int W,
                                                 int vec) {
    __shared__ __attribute__((aligned(16))) float row[SEG];
    const int tx = threadIdx.x, rf = blockIdx.y, s0 = blockIdx.x * SEG, Wf = 3 * W;
    const int b = blockIdx.z / C, c = blockIdx.z - b * C;
    const int i = rf / 3, a = rf - 3 * i;
    const float *src = g + (((size_t)b * C + c) * 3 * H + rf) * Wf + s0;
    const int n = min(SEG, Wf - s0);                                    // (a multiple of 3)
    if (vec) {
        int e = 4 * tx;
        if (e + 3 < n) *reinterpret_cast<float4 *>(row + e) = *reinterpret_cast<const float4 *>(src + e);
        else if (tx < SEG / 4)
            for (; e < n; ++e) row[e] = src[e];
    } else {
        for (int e = tx; e < n; e += 256) row[e] = src[e];
    }
    __syncthreads();
    const int x = s0 / 3 + tx;
    if (x >= W) return;
    const size_t cp = (size_t)H * W;
    float *o = out + (((size_t)b * 9 * C + 9 * c + 3 * a) * H + i) * W + x;
    o[0] = row[3 * tx];
    o[cp] = row[3 * tx + 1];
    o[2 * cp] = row[3 * tx + 2];
}
}  // namespace

extern "C" int decnet_d2s3_pad1(const float *t, float *dx, int B, int C, int H, int W, void *stream) {
    if (!t || !dx) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    if (H > 65535 || (long)B * C > 65535) return DECNET_ERR_UNSUPPORTED;
    const int vec = !((uintptr_t)dx & 15) && !(W & 3);
    hipLaunchKernelGGL(d2s3_pad1, dim3((unsigned)ceil_div(W, SEG), (unsigned)H, (unsigned)(B * C)), dim3(256), 0,
                       (hipStream_t)stream, t, dx, C, H, W, (H - 1) / 3 + 1, (W - 1) / 3 + 1, vec);
    return decnet_launch_status();
}

extern "C" int decnet_s2d3_pad0(const float *g, float *out, int B, int C, int H, int W, void *stream) {
    if (!g || !out) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    if (H > 21845 || W > 715827882 || (long)B * C > 65535) return DECNET_ERR_UNSUPPORTED;    // (3 H rows: a grid dimension)
    const int vec = !((uintptr_t)g & 15) && !(W & 3);
    hipLaunchKernelGGL(s2d3_pad0, dim3((unsigned)ceil_div(3 * W, SEG), (unsigned)(3 * H), (unsigned)(B * C)), dim3(256), 0,
                       (hipStream_t)stream, g, out, C, H, W, vec);
    return decnet_launch_status();
}

extern "C" int decnet_s2d3_pad1(const float *x, float *out, int B, int C, int H, int W, void *stream) {
    if (!x || !out) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    const int Ho = (H - 1) / 3 + 1, Wo = (W - 1) / 3 + 1;            // floor((H + 2 - 3) / 3) + 1
    if (Ho > 65535 || (long)B * C > 65535) return DECNET_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(s2d3_pad1, dim3((unsigned)ceil_div(Wo, 256), (unsigned)Ho, (unsigned)(B * C)), dim3(256), 0,
                       (hipStream_t)stream, x, out, C, H, W, Ho, Wo);
    return decnet_launch_status();
}

extern "C" int decnet_unfold3_cat(const float *fea, const float *disp, float *out, int B, int C, int h, int w,
                                  void *stream) {
    if (!fea || !disp || !out) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || h < 1 || w < 1 || h > 65535 || (long)B * (C + 1) > 65535) return DECNET_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(unfold3_cat, dim3((unsigned)ceil_div(w, 256), (unsigned)h, (unsigned)(B * (C + 1))), dim3(256), 0,
                       (hipStream_t)stream, fea, disp, out, C, h, w);
    return decnet_launch_status();
}
