// decnet_amd/csrc/batchnorm.hip -- training-mode BatchNorm (batch statistics) with an optional ReLU, forward and backward,
// under hip_grad(), on two layouts of the convolution's fp32 output z with N values per channel:
//
//   Planes    z [B,C,H,W], N = B H W: the conv units of the 2-D trunk (decnet_bn_train_*);
//   Columns   z [rows, C] channels-last, N = rows, channel c the column z[:, c]: the Conv3d units of stage 0, whose volumes
//             are [B,D,H,W,C] (decnet_bn_train_cl_*).
//
// Six kernels, each a template over the layout, the arithmetic written once:
//
//   bn_stats_partial     per work item: S1 = sum (z - p_c), S2 = sum (z - p_c)^2 in float64;
//   bn_stats_finish      per channel: the partials added in a fixed order, {mean, invstd} and the running statistics;
//   bn_apply             y = act(fma(z - mean, a, beta)), a = (float)(gamma invstd);
//   bn_grad_partial      per work item: sum gm and sum gm xhat in float64 (gm = gy [pre > 0], xhat = (z - mean) invstd);
//   bn_grad_finish       per channel: dbeta, dgamma (each rounded once), the float64 totals kept;
//   bn_grad_input        gz = a (gm - dbeta / N - xhat dgamma / N), every element written.
//
// A layout cuts a channel's values into work items and says which thread walks which elements; an item's elements are
// p[offset(k)], k = k0, k0 + STEP, ... < n, taken in rising order and accumulated in float64 from the first one on.
//
//   Planes    the idiom of loss.hip and wgrad_common.h: a plane (b, c) is H W consecutive floats, cut into
//             segments of DECNET_BN_SEGMENT floats.  A wave owns a segment, lane l takes l, l + 64, ..., the 64 lane sums are added in a
//             fixed butterfly and lane 0 writes the partial, part [C][B nseg][2].  One finish workgroup per channel
//             (thread t: t, t + 256, ...; then a fixed tree).
//   Columns   a column has no consecutive floats.  The rows are cut into segments of DECNET_BN_CL_ROWS rows; item
//             i = s C + c is channel c of segment s, and thread after thread takes item after item, so consecutive lanes take
//             consecutive channels and a wave reads 256 consecutive bytes of a row (and goes on into the next segment
//             where C is no multiple of 64: no lane idles at C = 216).  A partial is ONE thread's sequential sum, whatever
//             the grid, part [nseg][C][2].  One finish workgroup per 16 channels (16 threads per channel, thread j:
//             j, j + 16, ...; then a fixed tree over the 16).
//
// No atomics, no allocation, no host read-back: every entry runs under stream capture, and the bits depend neither on the
// launch shape nor on the alignment of a pointer (all accesses are single floats; there is no 16-byte path) nor on eager
// versus replay.
//
// The pivot p_c = z[0,c,0,0] (z[0, c]) keeps a channel whose mean is far above its spread from cancelling in
// S2 / N - (S1 / N)^2.  z - mean is formed in float64 (mean is never rounded to fp32); the pre-activation is ONE function,
// bn_pre, contraction pinned, that forward and backward of both layouts call, so the backward's ReLU decision is the
// forward's on every element and y is not read again.
//
// This file is built WITHOUT -fno-honor-nans: a NaN in a channel has to reach that channel's statistics and no other's.
#include "common.h"

namespace {

constexpr int BN_THREADS = 256;

// fma(z - mean, a, beta): z - mean in float64, rounded once; no contraction beyond the explicit fma
__device__ __forceinline__ float bn_pre(float z, double mean, float a, float beta) {
#pragma clang fp contract(off)
    const float d = (float)((double)z - mean);
    return fmaf(d, a, beta);
}

// a work item: its channel, its first element, its length and the slot of its partial pair
struct Item {
    int c, n;
    size_t first, slot;
};

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

constexpr int FIN_J = 16;                                   // threads that share a channel's partials in tile_sum2

// The nseg partial pairs of the 16 channels of one workgroup, part [nseg][C][2]: thread (j, cc) takes the segments
// j, j + 16, ... of channel c0 + cc in rising order (16 channels x 16 bytes: 256 consecutive bytes per segment), the 16
// sums of a channel are added in a fixed tree.  Every thread of a channel returns with the totals.
__device__ __forceinline__ void tile_sum2(const double *__restrict__ part, size_t nseg, int C, int c, bool live, double &t1,
                                          double &t2) {
#pragma clang fp contract(off)
    constexpr int FIN_CH = BN_THREADS / FIN_J;
    __shared__ double acc[FIN_J][FIN_CH][2];
    const int cc = threadIdx.x % FIN_CH, j = threadIdx.x / FIN_CH;
    double a1 = 0., a2 = 0.;
    if (live)
        for (size_t s = j; s < nseg; s += FIN_J) {
            const double *__restrict__ q = part + 2 * (s * (size_t)C + c);
            a1 += q[0];
            a2 += q[1];
        }
    acc[j][cc][0] = a1;
    acc[j][cc][1] = a2;
    __syncthreads();
    for (int k = FIN_J / 2; k > 0; k >>= 1) {
        if (j < k) {
            acc[j][cc][0] += acc[j + k][cc][0];
            acc[j][cc][1] += acc[j + k][cc][1];
        }
        __syncthreads();
    }
    t1 = acc[0][cc][0];
    t2 = acc[0][cc][1];
}

// ---- the two layouts ----------------------------------------------------------------------------------------------
// STEP threads share a work item (thread t of them takes the elements t, t + STEP, ...), so a workgroup works on
// BN_THREADS / STEP items at a time; FIN_CH channels share a finish workgroup.  items == 0: a shape the entries refuse.
struct Planes {
    static constexpr int STEP = DECNET_WAVE, UNROLL = 4, FIN_CH = 1, SEG = DECNET_BN_SEGMENT;
    int B, C, HW, nseg;
    size_t items;                                           // the B C nseg segments

    static Planes make(int B, int C, int H, int W) {
        if (B < 1 || C < 1 || H < 1 || W < 1 || (double)B * H * W < 2.0 || (double)B * C * H * W >= 2147483648.0)
            return Planes{B, C, 0, 0, 0};
        const int nseg = (int)(((size_t)H * W + SEG - 1) / SEG);
        return Planes{B, C, H * W, nseg, (size_t)B * C * nseg};
    }
    __device__ __forceinline__ Item item(size_t g) const {
        const size_t plane = g / (size_t)nseg;              // (two divisions per segment, none per element)
        const int s = (int)(g - plane * (size_t)nseg);
        const int b = (int)(plane / (size_t)C);
        Item q;
        q.c = (int)(plane - (size_t)b * C);
        const size_t left = (size_t)HW - (size_t)s * SEG;   // elements of the plane from this segment on (>= 1)
        q.first = plane * (size_t)HW + (size_t)s * SEG;
        q.n = left < (size_t)SEG ? (int)left : SEG;
        q.slot = ((size_t)q.c * B + b) * (size_t)nseg + s;  // part [C][B nseg][2]
        return q;
    }
    __device__ __forceinline__ size_t offset(int k) const { return (size_t)k; }
    __device__ __forceinline__ size_t pivot(int c) const { return (size_t)c * HW; }
    __device__ __forceinline__ double N() const { return (double)B * (double)HW; }
    // the 64 lane sums in a fixed butterfly; lane 0 writes
    __device__ __forceinline__ bool combine(double &s1, double &s2) const {
        for (int k = DECNET_WAVE / 2; k > 0; k >>= 1) {
            s1 += __shfl_xor(s1, k);
            s2 += __shfl_xor(s2, k);
        }
        return (threadIdx.x & (DECNET_WAVE - 1)) == 0;
    }
    __device__ __forceinline__ void sum2(const double *__restrict__ part, int c, bool, double &t1, double &t2) const {
        const size_t n = (size_t)B * nseg;
        channel_sum2(part + 2 * n * c, n, t1, t2);
    }
};

struct Columns {
    static constexpr int STEP = 1, UNROLL = 8, FIN_CH = BN_THREADS / FIN_J, ROWS = DECNET_BN_CL_ROWS;
    size_t rows;
    int C;
    size_t nseg, items;                                     // the nseg C (segment, channel) pairs; < rows C + C < 2^32

    static Columns make(size_t rows, int C) {
        if (!(rows >= 2 && C >= 1 && rows < ((size_t)1 << 31) && rows * (size_t)C < ((size_t)1 << 31)))
            return Columns{rows, C, 0, 0};
        const size_t nseg = (rows + ROWS - 1) / ROWS;
        return Columns{rows, C, nseg, nseg * (size_t)C};
    }
    __device__ __forceinline__ Item item(size_t i) const {
        const unsigned s = (unsigned)i / (unsigned)C;       // (one division per item, none per element)
        Item q;
        q.c = (int)((unsigned)i - s * (unsigned)C);
        const size_t row0 = (size_t)s * ROWS, left = rows - row0;          // rows from this segment on (>= 1)
        q.first = row0 * (size_t)C + q.c;
        q.n = left < (size_t)ROWS ? (int)left : ROWS;
        q.slot = i;                                         // part [nseg][C][2]
        return q;
    }
    __device__ __forceinline__ size_t offset(int k) const { return (size_t)k * C; }
    __device__ __forceinline__ size_t pivot(int c) const { return (size_t)c; }
    __device__ __forceinline__ double N() const { return (double)rows; }
    __device__ __forceinline__ bool combine(double &, double &) const { return true; }        // one thread's own sum
    __device__ __forceinline__ void sum2(const double *__restrict__ part, int c, bool live, double &t1, double &t2) const {
        tile_sum2(part, nseg, C, c, live, t1, t2);
    }
};

// The loops every element kernel runs, for a layout L:
//     for (size_t g = bn_first_item<L>(); g < lay.items; g += bn_item_stride<L>())      the items of this thread's group
//         for (int k = bn_k0<L>(); k < q.n; k += L::STEP)                               this thread's elements of item q
template <class L>
__device__ __forceinline__ size_t bn_first_item() {
    return (size_t)blockIdx.x * (BN_THREADS / L::STEP) + threadIdx.x / L::STEP;
}

template <class L>
__device__ __forceinline__ size_t bn_item_stride() {
    return (size_t)gridDim.x * (BN_THREADS / L::STEP);
}

template <class L>
__device__ __forceinline__ int bn_k0() {
    return threadIdx.x % L::STEP;
}

// the constants of channel c; c1, c2 (of the float64 sums `total` of bn_grad_finish) only with TOTALS
struct Channel {
    double mean, invstd, c1, c2, ad;
    float a, bt;
};

template <bool TOTALS = false>
__device__ __forceinline__ Channel bn_channel(const float *__restrict__ gamma, const float *__restrict__ beta,
                                              const double *__restrict__ stats, int c,
                                              const double *__restrict__ total = nullptr, double N = 0.) {
#pragma clang fp contract(off)
    Channel ch;
    ch.mean = stats[2 * c];
    ch.invstd = stats[2 * c + 1];
    ch.a = (float)((double)gamma[c] * ch.invstd);
    ch.bt = beta[c];
    ch.c1 = TOTALS ? total[2 * c] / N : 0.;
    ch.c2 = TOTALS ? total[2 * c + 1] / N : 0.;
    ch.ad = (double)ch.a;
    return ch;
}

// gm = gy [pre > 0] on the forward's own decision, xhat = (z - mean) invstd in float64
template <bool RELU>
__device__ __forceinline__ void bn_gm_xhat(float zv, float gv, const Channel &ch, float &gm, double &xh) {
#pragma clang fp contract(off)
    gm = (!RELU || bn_pre(zv, ch.mean, ch.a, ch.bt) > 0.f) ? gv : 0.f;
    xh = ((double)zv - ch.mean) * ch.invstd;
}

template <class L>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial(const float *__restrict__ z, double *__restrict__ part,
                                                               const L lay) {
#pragma clang fp contract(off)
    for (size_t g = bn_first_item<L>(); g < lay.items; g += bn_item_stride<L>()) {
        const Item q = lay.item(g);
        const double pivot = (double)z[lay.pivot(q.c)];
        const float *__restrict__ p = z + q.first;
        double s1 = 0., s2 = 0.;
#pragma unroll L::UNROLL
        for (int k = bn_k0<L>(); k < q.n; k += L::STEP) {
            const double d = (double)p[lay.offset(k)] - pivot;
            s1 += d;
            s2 = fma(d, d, s2);
        }
        if (lay.combine(s1, s2)) {
            part[2 * q.slot] = s1;
            part[2 * q.slot + 1] = s2;
        }
    }
}

template <class L>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_finish(const float *__restrict__ z, const double *__restrict__ part,
                                                              double eps, double momentum, float *__restrict__ running_mean,
                                                              float *__restrict__ running_var, double *__restrict__ stats,
                                                              const L lay) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * L::FIN_CH + threadIdx.x % L::FIN_CH;
    const bool live = c < lay.C;
    double s1, s2;
    lay.sum2(part, c, live, s1, s2);
    if (live && threadIdx.x < L::FIN_CH) {
        const double N = lay.N();
        const double m1 = s1 / N;
        const double mean = (double)z[lay.pivot(c)] + m1;
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

template <class L, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_apply(const float *__restrict__ z, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const double *__restrict__ stats,
                                                       float *__restrict__ y, const L lay) {
    for (size_t g = bn_first_item<L>(); g < lay.items; g += bn_item_stride<L>()) {
        const Item q = lay.item(g);
        const Channel ch = bn_channel(gamma, beta, stats, q.c);
        const float *__restrict__ p = z + q.first;
        float *__restrict__ o = y + q.first;
#pragma unroll L::UNROLL
        for (int k = bn_k0<L>(); k < q.n; k += L::STEP) {
            const float pre = bn_pre(p[lay.offset(k)], ch.mean, ch.a, ch.bt);
            o[lay.offset(k)] = RELU ? (pre < 0.f ? 0.f : pre) : pre;       // (a NaN stays a NaN)
        }
    }
}

template <class L, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_grad_partial(const float *__restrict__ z, const float *__restrict__ gy,
                                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                                              const double *__restrict__ stats, double *__restrict__ part,
                                                              const L lay) {
#pragma clang fp contract(off)
    for (size_t g = bn_first_item<L>(); g < lay.items; g += bn_item_stride<L>()) {
        const Item q = lay.item(g);
        const Channel ch = bn_channel(gamma, beta, stats, q.c);
        const float *__restrict__ p = z + q.first;
        const float *__restrict__ gp = gy + q.first;
        double s1 = 0., s2 = 0.;
#pragma unroll L::UNROLL
        for (int k = bn_k0<L>(); k < q.n; k += L::STEP) {
            const float zv = p[lay.offset(k)], gv = gp[lay.offset(k)]; // (both loads before the decision: they stay batched)
            float gm;
            double xh;
            bn_gm_xhat<RELU>(zv, gv, ch, gm, xh);
            s1 += (double)gm;
            s2 = fma((double)gm, xh, s2);
        }
        if (lay.combine(s1, s2)) {
            part[2 * q.slot] = s1;
            part[2 * q.slot + 1] = s2;
        }
    }
}

template <class L>
__global__ __launch_bounds__(BN_THREADS) void bn_grad_finish(const double *__restrict__ part, double *__restrict__ total,
                                                             float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                             const L lay) {
    const int c = blockIdx.x * L::FIN_CH + threadIdx.x % L::FIN_CH;
    const bool live = c < lay.C;
    double s1, s2;
    lay.sum2(part, c, live, s1, s2);
    if (live && threadIdx.x < L::FIN_CH) {
        total[2 * c] = s1;
        total[2 * c + 1] = s2;
        dbeta[c] = (float)s1;
        dgamma[c] = (float)s2;
    }
}

// gz = a (gm - dbeta / N - xhat dgamma / N): the two per-channel constants in float64, an element in float64, rounded once
template <class L, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_grad_input(const float *__restrict__ z, const float *__restrict__ gy,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const double *__restrict__ stats, const double *__restrict__ total,
                                                            float *__restrict__ gz, const L lay) {
#pragma clang fp contract(off)
    const double N = lay.N();
    for (size_t g = bn_first_item<L>(); g < lay.items; g += bn_item_stride<L>()) {
        const Item q = lay.item(g);
        const Channel ch = bn_channel<true>(gamma, beta, stats, q.c, total, N);
        const float *__restrict__ p = z + q.first;
        const float *__restrict__ gp = gy + q.first;
        float *__restrict__ o = gz + q.first;
#pragma unroll L::UNROLL
        for (int k = bn_k0<L>(); k < q.n; k += L::STEP) {
            const float zv = p[lay.offset(k)], gv = gp[lay.offset(k)];
            float gm;
            double xh;
            bn_gm_xhat<RELU>(zv, gv, ch, gm, xh);
            o[lay.offset(k)] = (float)(ch.ad * (((double)gm - ch.c1) - xh * ch.c2));
        }
    }
}

// ---- the entries, once per direction -------------------------------------------------------------------------------
// part [items][2] + total [C][2], float64
template <class L>
size_t bn_workspace_floats(const L &lay) {
    return lay.items ? 2 * (2 * lay.items + 2 * (size_t)lay.C) : 0;
}

// the refusals that follow the NULL checks: shape, workspace size, alignment
template <class L>
int bn_refusal(const L &lay, const void *ws, size_t ws_floats, const void *stats) {
    if (!lay.items) return DECNET_ERR_BAD_SHAPE;
    if (ws_floats < bn_workspace_floats(lay)) return DECNET_ERR_BAD_SHAPE;
    if (((uintptr_t)ws & 7) || ((uintptr_t)stats & 7)) return DECNET_ERR_MISALIGNED;
    return DECNET_OK;
}

template <class L>
dim3 bn_grid(const L &lay) {
    const size_t per = BN_THREADS / L::STEP, b = (lay.items + per - 1) / per;
    return dim3((unsigned)(b < 8192 ? b : 8192));
}

template <class L>
dim3 bn_finish_grid(const L &lay) {
    return dim3((lay.C + L::FIN_CH - 1) / L::FIN_CH);
}

template <class L>
int bn_forward(const L &lay, const float *z, const float *gamma, const float *beta, double eps, double momentum,
               float *running_mean, float *running_var, double *stats, float *y, int relu, void *ws, size_t ws_floats,
               hipStream_t stream) {
    if (!z || !gamma || !beta || !stats || !y || !ws) return DECNET_ERR_NULL_POINTER;
    if ((running_mean == nullptr) != (running_var == nullptr)) return DECNET_ERR_NULL_POINTER;
    if (const int rc = bn_refusal(lay, ws, ws_floats, stats)) return rc;
    double *part = (double *)ws;
    const dim3 grid = bn_grid(lay), block(BN_THREADS);
    const auto apply = relu ? bn_apply<L, true> : bn_apply<L, false>;
    hipLaunchKernelGGL(bn_stats_partial<L>, grid, block, 0, stream, z, part, lay);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_stats_finish<L>, bn_finish_grid(lay), block, 0, stream, z, (const double *)part, eps, momentum,
                       running_mean, running_var, stats, lay);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(apply, grid, block, 0, stream, z, gamma, beta, (const double *)stats, y, lay);
    return decnet_launch_status();
}

template <class L>
int bn_backward(const L &lay, const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                float *gz, float *dgamma, float *dbeta, int relu, void *ws, size_t ws_floats, hipStream_t stream) {
    if (!z || !gy || !gamma || !beta || !stats || !dgamma || !dbeta || !ws) return DECNET_ERR_NULL_POINTER;
    if (const int rc = bn_refusal(lay, ws, ws_floats, stats)) return rc;
    double *part = (double *)ws, *total = part + 2 * lay.items;
    const dim3 grid = bn_grid(lay), block(BN_THREADS);
    const auto partial = relu ? bn_grad_partial<L, true> : bn_grad_partial<L, false>;
    const auto input = relu ? bn_grad_input<L, true> : bn_grad_input<L, false>;
    hipLaunchKernelGGL(partial, grid, block, 0, stream, z, gy, gamma, beta, stats, part, lay);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_grad_finish<L>, bn_finish_grid(lay), block, 0, stream, (const double *)part, total, dgamma, dbeta,
                       lay);
    if (const int rc = decnet_launch_status()) return rc;
    if (!gz) return DECNET_OK;
    hipLaunchKernelGGL(input, grid, block, 0, stream, z, gy, gamma, beta, stats, (const double *)total, gz, lay);
    return decnet_launch_status();
}

}  // namespace

size_t decnet_bn_train_workspace_floats(int B, int C, int H, int W) {
    return bn_workspace_floats(Planes::make(B, C, H, W));
}

int decnet_bn_train_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                            float *running_mean, float *running_var, double *stats, float *y, int relu, void *ws,
                            size_t ws_floats, int B, int C, int H, int W, void *stream) {
    return bn_forward(Planes::make(B, C, H, W), z, gamma, beta, eps, momentum, running_mean, running_var, stats, y, relu, ws,
                      ws_floats, (hipStream_t)stream);
}

int decnet_bn_train_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                             float *gz, float *dgamma, float *dbeta, int relu, void *ws, size_t ws_floats, int B, int C,
                             int H, int W, void *stream) {
    return bn_backward(Planes::make(B, C, H, W), z, gy, gamma, beta, stats, gz, dgamma, dbeta, relu, ws, ws_floats,
                       (hipStream_t)stream);
}

size_t decnet_bn_train_cl_workspace_floats(size_t rows, int C) { return bn_workspace_floats(Columns::make(rows, C)); }

int decnet_bn_train_cl_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                               float *running_mean, float *running_var, double *stats, float *y, int relu, void *ws,
                               size_t ws_floats, size_t rows, int C, void *stream) {
    return bn_forward(Columns::make(rows, C), z, gamma, beta, eps, momentum, running_mean, running_var, stats, y, relu, ws,
                      ws_floats, (hipStream_t)stream);
}

int decnet_bn_train_cl_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                                float *gz, float *dgamma, float *dbeta, int relu, void *ws, size_t ws_floats, size_t rows,
                                int C, void *stream) {
    return bn_backward(Columns::make(rows, C), z, gy, gamma, beta, stats, gz, dgamma, dbeta, relu, ws, ws_floats,
                       (hipStream_t)stream);
}
