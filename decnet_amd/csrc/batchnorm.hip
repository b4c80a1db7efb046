// decnet_amd/csrc/batchnorm.hip -- training-mode BatchNorm2d (batch statistics) with an optional ReLU, forward and backward,
// for the conv units under hip_grad(): z [B,C,H,W] fp32 is the convolution's output, N = B H W values per channel.
//
//   bn_stats_partial     per segment of a plane (a wave each): S1 = sum (z - p_c), S2 = sum (z - p_c)^2 in float64;
//   bn_stats_finish      one workgroup per channel: the partials added in a fixed order, {mean, invstd} and the running
//                        statistics;
//   bn_apply             y = act(fma(z - mean, a, beta)), a = (float)(gamma invstd);
//   bn_grad_partial      per segment: sum gm and sum gm xhat in float64 (gm = gy [pre > 0], xhat = (z - mean) invstd);
//   bn_grad_finish       one workgroup per channel: dbeta, dgamma (each rounded once), the float64 totals kept;
//   bn_grad_input        gz = a (gm - dbeta / N - xhat dgamma / N), every element written.
//
// The idiom of loss.hip and conv2d_wgrad_reduce.h: a plane (b, c) is H W consecutive floats, cut into segments of
// DECNET_BN_SEGMENT floats; a wave owns a segment, lane l takes the elements l, l + 64, ... in order and accumulates in
// float64 from the first element on, the 64 lane sums are added in a fixed butterfly, and the finish kernel adds a
// channel's partials in a fixed order (thread t: t, t + 256, ...; then a fixed tree).  No atomics, no allocation, no host
// read-back: every entry runs under stream capture, and the bits depend neither on the launch shape nor on the alignment
// of a plane (all accesses are single floats) nor on eager versus replay.
//
// The pivot p_c = z[0,c,0,0] keeps a channel whose mean is far above its spread from cancelling in S2 / N - (S1 / N)^2.
// z - mean is formed in float64 (mean is never rounded to fp32); the pre-activation is ONE function (bn_pre.h), contraction
// pinned, that forward and backward both call, so the backward's ReLU decision is the forward's on every element and y is not
// read again.
//
// This file is built WITHOUT -fno-honor-nans: a NaN in a channel has to reach that channel's statistics and no other's.
#include "bn_pre.h"
#include "common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_WAVES = BN_THREADS / DECNET_WAVE;         // segments a workgroup works on at a time (one per wave)
constexpr int SEG = DECNET_BN_SEGMENT;

inline unsigned bn_grid(size_t segs) {
    const size_t b = (segs + BN_WAVES - 1) / BN_WAVES;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

inline int bn_nseg(int H, int W) { return (int)(((size_t)H * W + SEG - 1) / SEG); }

// segment g of the B C nseg segments: its channel, its first element, its length and its slot among the channel's partials
struct Segment {
    int c, n;
    size_t base, slot;
};

__device__ __forceinline__ Segment bn_segment(size_t g, int B, int C, int HW, int nseg) {
    const size_t plane = g / (size_t)nseg;                 // (two divisions per segment, none per element)
    const int s = (int)(g - plane * (size_t)nseg);
    const int b = (int)(plane / (size_t)C);
    Segment q;
    q.c = (int)(plane - (size_t)b * C);
    const size_t left = (size_t)HW - (size_t)s * SEG;      // elements of the plane from this segment on (>= 1)
    q.base = plane * (size_t)HW + (size_t)s * SEG;
    q.n = left < (size_t)SEG ? (int)left : SEG;
    q.slot = ((size_t)q.c * B + b) * (size_t)nseg + s;
    return q;
}

__device__ __forceinline__ void wave_sum2(double &s1, double &s2) {
    for (int k = DECNET_WAVE / 2; k > 0; k >>= 1) {
        s1 += __shfl_xor(s1, k);
        s2 += __shfl_xor(s2, k);
    }
}

// The n partial pairs of one channel, added by one workgroup: thread t takes t, t + 256, ... in rising order, the 256
// thread sums are added in a fixed tree.  Every thread returns with the totals.
__device__ __forceinline__ void channel_sum2(const double *__restrict__ part, size_t n, double &t1, double &t2) {
#pragma clang fp contract(off)
    __shared__ double acc[BN_THREADS][2];
    double a1 = 0., a2 = 0.;
    for (size_t r = threadIdx.x; r < n; r += BN_THREADS) {
        a1 += part[2 * r];
        a2 += part[2 * r + 1];
    }
    acc[threadIdx.x][0] = a1;
    acc[threadIdx.x][1] = a2;
    __syncthreads();
    for (int k = BN_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            acc[threadIdx.x][0] += acc[threadIdx.x + k][0];
            acc[threadIdx.x][1] += acc[threadIdx.x + k][1];
        }
        __syncthreads();
    }
    t1 = acc[0][0];
    t2 = acc[0][1];
}

__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial(const float *__restrict__ z, double *__restrict__ part,
                                                               size_t segs, int B, int C, int HW, int nseg) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t g = (size_t)blockIdx.x * BN_WAVES + wave; g < segs; g += (size_t)gridDim.x * BN_WAVES) {
        const Segment q = bn_segment(g, B, C, HW, nseg);
        const double pivot = (double)z[(size_t)q.c * HW];
        const float *__restrict__ p = z + q.base;
        double s1 = 0., s2 = 0.;
#pragma unroll 4
        for (int i = lane; i < q.n; i += DECNET_WAVE) {
            const double d = (double)p[i] - pivot;
            s1 += d;
            s2 = fma(d, d, s2);
        }
        wave_sum2(s1, s2);
        if (lane == 0) {
            part[2 * q.slot] = s1;
            part[2 * q.slot + 1] = s2;
        }
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_stats_finish(const float *__restrict__ z, const double *__restrict__ part,
                                                              double eps, double momentum, float *__restrict__ running_mean,
                                                              float *__restrict__ running_var, double *__restrict__ stats,
                                                              int B, int HW, int nseg) {
#pragma clang fp contract(off)
    const int c = blockIdx.x;
    const size_t n = (size_t)B * nseg;
    double s1, s2;
    channel_sum2(part + 2 * n * c, n, s1, s2);
    if (threadIdx.x == 0) {
        const double N = (double)B * (double)HW;
        const double m1 = s1 / N;
        const double mean = (double)z[(size_t)c * HW] + m1;
        double var = s2 / N - m1 * m1;
        if (var < 0.) var = 0.;                             // (a NaN is not below 0 and stays a NaN)
        stats[2 * c] = mean;
        stats[2 * c + 1] = 1. / sqrt(var + eps);
        if (running_mean) {
            running_mean[c] = (float)((1. - momentum) * (double)running_mean[c] + momentum * mean);
            running_var[c] = (float)((1. - momentum) * (double)running_var[c] + momentum * (var * N / (N - 1.)));
        }
    }
}

template <bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_apply(const float *__restrict__ z, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const double *__restrict__ stats,
                                                       float *__restrict__ y, size_t segs, int B, int C, int HW, int nseg) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t g = (size_t)blockIdx.x * BN_WAVES + wave; g < segs; g += (size_t)gridDim.x * BN_WAVES) {
        const Segment q = bn_segment(g, B, C, HW, nseg);
        const double mean = stats[2 * q.c];
        const float a = (float)((double)gamma[q.c] * stats[2 * q.c + 1]), bt = beta[q.c];
        const float *__restrict__ p = z + q.base;
        float *__restrict__ o = y + q.base;
#pragma unroll 4
        for (int i = lane; i < q.n; i += DECNET_WAVE) {
            const float pre = bn_pre(p[i], mean, a, bt);
            o[i] = RELU ? (pre < 0.f ? 0.f : pre) : pre;    // (a NaN stays a NaN)
        }
    }
}

template <bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_grad_partial(const float *__restrict__ z, const float *__restrict__ gy,
                                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                                              const double *__restrict__ stats, double *__restrict__ part,
                                                              size_t segs, int B, int C, int HW, int nseg) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t g = (size_t)blockIdx.x * BN_WAVES + wave; g < segs; g += (size_t)gridDim.x * BN_WAVES) {
        const Segment q = bn_segment(g, B, C, HW, nseg);
        const double mean = stats[2 * q.c], invstd = stats[2 * q.c + 1];
        const float a = (float)((double)gamma[q.c] * invstd), bt = beta[q.c];
        const float *__restrict__ p = z + q.base;
        const float *__restrict__ gp = gy + q.base;
        double s1 = 0., s2 = 0.;
#pragma unroll 4
        for (int i = lane; i < q.n; i += DECNET_WAVE) {
            const float zv = p[i], gv = gp[i];              // (both loads before the decision: they stay batched)
            const float gm = (!RELU || bn_pre(zv, mean, a, bt) > 0.f) ? gv : 0.f;
            const double xh = ((double)zv - mean) * invstd;
            s1 += (double)gm;
            s2 = fma((double)gm, xh, s2);
        }
        wave_sum2(s1, s2);
        if (lane == 0) {
            part[2 * q.slot] = s1;
            part[2 * q.slot + 1] = s2;
        }
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_grad_finish(const double *__restrict__ part, double *__restrict__ total,
                                                             float *__restrict__ dgamma, float *__restrict__ dbeta, int B,
                                                             int nseg) {
    const int c = blockIdx.x;
    const size_t n = (size_t)B * nseg;
    double s1, s2;
    channel_sum2(part + 2 * n * c, n, s1, s2);
    if (threadIdx.x == 0) {
        total[2 * c] = s1;
        total[2 * c + 1] = s2;
        dbeta[c] = (float)s1;
        dgamma[c] = (float)s2;
    }
}

// gz = a (gm - dbeta / N - xhat dgamma / N): the two per-channel constants in float64, an element in float64, rounded once
template <bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_grad_input(const float *__restrict__ z, const float *__restrict__ gy,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const double *__restrict__ stats, const double *__restrict__ total,
                                                            float *__restrict__ gz, size_t segs, int B, int C, int HW,
                                                            int nseg) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    const double N = (double)B * (double)HW;
    for (size_t g = (size_t)blockIdx.x * BN_WAVES + wave; g < segs; g += (size_t)gridDim.x * BN_WAVES) {
        const Segment q = bn_segment(g, B, C, HW, nseg);
        const double mean = stats[2 * q.c], invstd = stats[2 * q.c + 1];
        const float a = (float)((double)gamma[q.c] * invstd), bt = beta[q.c];
        const double c1 = total[2 * q.c] / N, c2 = total[2 * q.c + 1] / N, ad = (double)a;
        const float *__restrict__ p = z + q.base;
        const float *__restrict__ gp = gy + q.base;
        float *__restrict__ o = gz + q.base;
#pragma unroll 4
        for (int i = lane; i < q.n; i += DECNET_WAVE) {
            const float zv = p[i], gv = gp[i];
            const float gm = (!RELU || bn_pre(zv, mean, a, bt) > 0.f) ? gv : 0.f;
            const double xh = ((double)zv - mean) * invstd;
            o[i] = (float)(ad * (((double)gm - c1) - xh * c2));
        }
    }
}

// shared shape and workspace check of the two entries
inline int bn_args(const void *ws, size_t ws_floats, const void *stats, int B, int C, int H, int W) {
    if (B < 1 || C < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * H * W < 2.0 || (double)B * C * H * W >= 2147483648.0) return DECNET_ERR_BAD_SHAPE;
    if (ws_floats < decnet_bn_train_workspace_floats(B, C, H, W)) return DECNET_ERR_BAD_SHAPE;
    if (((uintptr_t)ws & 7) || ((uintptr_t)stats & 7)) return DECNET_ERR_MISALIGNED;
    return DECNET_OK;
}

}  // namespace

size_t decnet_bn_train_workspace_floats(int B, int C, int H, int W) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || (double)B * H * W < 2.0 || (double)B * C * H * W >= 2147483648.0) return 0;
    // [C][B nseg][2] partials + [C][2] totals, float64
    return 2 * (2 * (size_t)C * B * bn_nseg(H, W) + 2 * (size_t)C);
}

int decnet_bn_train_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                            float *running_mean, float *running_var, double *stats, float *y, int relu, void *ws,
                            size_t ws_floats, int B, int C, int H, int W, void *stream) {
    if (!z || !gamma || !beta || !stats || !y || !ws) return DECNET_ERR_NULL_POINTER;
    if ((running_mean == nullptr) != (running_var == nullptr)) return DECNET_ERR_NULL_POINTER;
    if (const int rc = bn_args(ws, ws_floats, stats, B, C, H, W)) return rc;
    const int HW = H * W, nseg = bn_nseg(H, W);
    const size_t segs = (size_t)B * C * nseg;
    double *part = (double *)ws;
    const dim3 grid(bn_grid(segs)), block(BN_THREADS);
    hipLaunchKernelGGL(bn_stats_partial, grid, block, 0, (hipStream_t)stream, z, part, segs, B, C, HW, nseg);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_stats_finish, dim3(C), block, 0, (hipStream_t)stream, z, (const double *)part, eps, momentum,
                       running_mean, running_var, stats, B, HW, nseg);
    if (const int rc = decnet_launch_status()) return rc;
    if (relu)
        hipLaunchKernelGGL(bn_apply<true>, grid, block, 0, (hipStream_t)stream, z, gamma, beta, (const double *)stats, y,
                           segs, B, C, HW, nseg);
    else
        hipLaunchKernelGGL(bn_apply<false>, grid, block, 0, (hipStream_t)stream, z, gamma, beta, (const double *)stats, y,
                           segs, B, C, HW, nseg);
    return decnet_launch_status();
}

int decnet_bn_train_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                             float *gz, float *dgamma, float *dbeta, int relu, void *ws, size_t ws_floats, int B, int C,
                             int H, int W, void *stream) {
    if (!z || !gy || !gamma || !beta || !stats || !dgamma || !dbeta || !ws) return DECNET_ERR_NULL_POINTER;
    if (const int rc = bn_args(ws, ws_floats, stats, B, C, H, W)) return rc;
    const int HW = H * W, nseg = bn_nseg(H, W);
    const size_t segs = (size_t)B * C * nseg;
    double *part = (double *)ws, *total = part + 2 * (size_t)C * B * nseg;
    const dim3 grid(bn_grid(segs)), block(BN_THREADS);
    if (relu)
        hipLaunchKernelGGL(bn_grad_partial<true>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats, part,
                           segs, B, C, HW, nseg);
    else
        hipLaunchKernelGGL(bn_grad_partial<false>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats, part,
                           segs, B, C, HW, nseg);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_grad_finish, dim3(C), block, 0, (hipStream_t)stream, (const double *)part, total, dgamma, dbeta,
                       B, nseg);
    if (const int rc = decnet_launch_status()) return rc;
    if (!gz) return DECNET_OK;
    if (relu)
        hipLaunchKernelGGL(bn_grad_input<true>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats,
                           (const double *)total, gz, segs, B, C, HW, nseg);
    else
        hipLaunchKernelGGL(bn_grad_input<false>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats,
                           (const double *)total, gz, segs, B, C, HW, nseg);
    return decnet_launch_status();
}
