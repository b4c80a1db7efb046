// decnet_amd/csrc/batchnorm_cl.hip -- training-mode BatchNorm (batch statistics) with an optional ReLU, forward and
// backward, on a CHANNELS-LAST matrix z [rows, C] fp32: the Conv3d units of stage 0 under hip_grad(), whose volumes are
// [B,D,H,W,C] (rows = B D H W values per channel; channel c is the column z[:, c]).  batchnorm.hip is the same contract on
// NCHW planes; a column has no consecutive floats, so the reduction is laid out anew:
//
//   bn_cl_stats_partial  per (segment, channel) -- a thread each: S1 = sum (z - p_c), S2 = sum (z - p_c)^2 in float64;
//   bn_cl_stats_finish   one workgroup per 16 channels: the partials added in a fixed order, {mean, invstd} and the
//                        running statistics;
//   bn_cl_apply          y = act(fma(z - mean, a, beta)), a = (float)(gamma invstd);
//   bn_cl_grad_partial   per (segment, channel): sum gm and sum gm xhat in float64 (gm = gy [pre > 0],
//                        xhat = (z - mean) invstd);
//   bn_cl_grad_finish    one workgroup per 16 channels: dbeta, dgamma (each rounded once), the float64 totals kept;
//   bn_cl_grad_input     gz = a (gm - dbeta / N - xhat dgamma / N), every element written.
//
// The rows are cut into segments of DECNET_BN_CL_ROWS rows.  Work item i = s C + c is channel c of segment s; thread
// after thread takes item after item, so consecutive lanes take consecutive channels and a wave reads 256 consecutive
// bytes of a row (and goes on into the next segment where C is no multiple of 64: no lane idles at C = 216).  A thread
// walks its rows in rising order and accumulates in float64 from the first one on: a partial is ONE thread's sequential
// sum, whatever the grid.  The finish kernel adds a channel's partials in a fixed order (16 threads per channel, thread j:
// j, j + 16, ... in rising order; then a fixed tree over the 16).  No atomics, no allocation, no host read-back: every
// entry runs under stream capture, and the bits depend neither on the launch shape nor on the alignment of a pointer
// (all accesses are single floats; there is no 16-byte path) nor on eager versus replay.
//
// The pivot p_c = z[0, c] keeps a channel whose mean is far above its spread from cancelling in S2 / N - (S1 / N)^2.
// z - mean is formed in float64 (mean is never rounded to fp32); the pre-activation is the ONE function bn_pre (bn_pre.h),
// contraction pinned, of batchnorm.hip, that forward and backward both call, so the backward's ReLU decision is the
// forward's on every element and y is not read again.
//
// This file is built WITHOUT -fno-honor-nans: a NaN in a channel has to reach that channel's statistics and no other's.
#include "bn_pre.h"
#include "common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_ROWS = DECNET_BN_CL_ROWS;
constexpr int FIN_CH = 16;                                  // channels of a finish workgroup
constexpr int FIN_J = CL_THREADS / FIN_CH;                  // threads that share a channel's partials

inline size_t cl_nseg(size_t rows) { return (rows + CL_ROWS - 1) / CL_ROWS; }

inline unsigned cl_grid(size_t items) {
    const size_t b = (items + CL_THREADS - 1) / CL_THREADS;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

// item i of the nseg C items: its channel, its first element and its number of rows (one division per item, none per
// element; items < rows C + C < 2^32)
struct Item {
    int c, n;
    size_t first;
};

__device__ __forceinline__ Item cl_item(size_t i, size_t rows, int C) {
    const unsigned s = (unsigned)i / (unsigned)C;
    Item q;
    q.c = (int)((unsigned)i - s * (unsigned)C);
    const size_t row0 = (size_t)s * CL_ROWS, left = rows - row0;       // rows from this segment on (>= 1)
    q.first = row0 * (size_t)C + q.c;
    q.n = left < (size_t)CL_ROWS ? (int)left : CL_ROWS;
    return q;
}

// The nseg partial pairs of the 16 channels of one workgroup, part [nseg][C][2]: thread (j, cc) takes the segments
// j, j + 16, ... of channel c0 + cc in rising order (16 channels x 16 bytes: 256 consecutive bytes per segment), the 16
// sums of a channel are added in a fixed tree.  Every thread of a channel returns with the totals.
__device__ __forceinline__ void tile_sum2(const double *__restrict__ part, size_t nseg, int C, int c, bool live, double &t1,
                                          double &t2) {
#pragma clang fp contract(off)
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

__global__ __launch_bounds__(CL_THREADS) void bn_cl_stats_partial(const float *__restrict__ z, double *__restrict__ part,
                                                                  size_t items, size_t rows, int C) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; i < items; i += (size_t)gridDim.x * CL_THREADS) {
        const Item q = cl_item(i, rows, C);
        const double pivot = (double)z[q.c];
        const float *__restrict__ p = z + q.first;
        double s1 = 0., s2 = 0.;
#pragma unroll 8
        for (int r = 0; r < q.n; ++r) {
            const double d = (double)p[(size_t)r * C] - pivot;
            s1 += d;
            s2 = fma(d, d, s2);
        }
        part[2 * i] = s1;
        part[2 * i + 1] = s2;
    }
}

__global__ __launch_bounds__(CL_THREADS) void bn_cl_stats_finish(const float *__restrict__ z, const double *__restrict__ part,
                                                                 double eps, double momentum, float *__restrict__ running_mean,
                                                                 float *__restrict__ running_var, double *__restrict__ stats,
                                                                 size_t rows, int C, size_t nseg) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH;
    const bool live = c < C;
    double s1, s2;
    tile_sum2(part, nseg, C, c, live, s1, s2);
    if (live && threadIdx.x < FIN_CH) {
        const double N = (double)rows;
        const double m1 = s1 / N;
        const double mean = (double)z[c] + m1;
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
__global__ __launch_bounds__(CL_THREADS) void bn_cl_apply(const float *__restrict__ z, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const double *__restrict__ stats,
                                                          float *__restrict__ y, size_t items, size_t rows, int C) {
    for (size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; i < items; i += (size_t)gridDim.x * CL_THREADS) {
        const Item q = cl_item(i, rows, C);
        const double mean = stats[2 * q.c];
        const float a = (float)((double)gamma[q.c] * stats[2 * q.c + 1]), bt = beta[q.c];
        const float *__restrict__ p = z + q.first;
        float *__restrict__ o = y + q.first;
#pragma unroll 8
        for (int r = 0; r < q.n; ++r) {
            const float pre = bn_pre(p[(size_t)r * C], mean, a, bt);
            o[(size_t)r * C] = RELU ? (pre < 0.f ? 0.f : pre) : pre;    // (a NaN stays a NaN)
        }
    }
}

template <bool RELU>
__global__ __launch_bounds__(CL_THREADS) void bn_cl_grad_partial(const float *__restrict__ z, const float *__restrict__ gy,
                                                                 const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta,
                                                                 const double *__restrict__ stats, double *__restrict__ part,
                                                                 size_t items, size_t rows, int C) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; i < items; i += (size_t)gridDim.x * CL_THREADS) {
        const Item q = cl_item(i, rows, C);
        const double mean = stats[2 * q.c], invstd = stats[2 * q.c + 1];
        const float a = (float)((double)gamma[q.c] * invstd), bt = beta[q.c];
        const float *__restrict__ p = z + q.first;
        const float *__restrict__ gp = gy + q.first;
        double s1 = 0., s2 = 0.;
#pragma unroll 8
        for (int r = 0; r < q.n; ++r) {
            const float zv = p[(size_t)r * C], gv = gp[(size_t)r * C];  // (both loads before the decision: they stay batched)
            const float gm = (!RELU || bn_pre(zv, mean, a, bt) > 0.f) ? gv : 0.f;
            const double xh = ((double)zv - mean) * invstd;
            s1 += (double)gm;
            s2 = fma((double)gm, xh, s2);
        }
        part[2 * i] = s1;
        part[2 * i + 1] = s2;
    }
}

__global__ __launch_bounds__(CL_THREADS) void bn_cl_grad_finish(const double *__restrict__ part, double *__restrict__ total,
                                                                float *__restrict__ dgamma, float *__restrict__ dbeta, int C,
                                                                size_t nseg) {
    const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH;
    const bool live = c < C;
    double s1, s2;
    tile_sum2(part, nseg, C, c, live, s1, s2);
    if (live && threadIdx.x < FIN_CH) {
        total[2 * c] = s1;
        total[2 * c + 1] = s2;
        dbeta[c] = (float)s1;
        dgamma[c] = (float)s2;
    }
}

// gz = a (gm - dbeta / N - xhat dgamma / N): the two per-channel constants in float64, an element in float64, rounded once
template <bool RELU>
__global__ __launch_bounds__(CL_THREADS) void bn_cl_grad_input(const float *__restrict__ z, const float *__restrict__ gy,
                                                               const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               const double *__restrict__ stats,
                                                               const double *__restrict__ total, float *__restrict__ gz,
                                                               size_t items, size_t rows, int C) {
#pragma clang fp contract(off)
    const double N = (double)rows;
    for (size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x; i < items; i += (size_t)gridDim.x * CL_THREADS) {
        const Item q = cl_item(i, rows, C);
        const double mean = stats[2 * q.c], invstd = stats[2 * q.c + 1];
        const float a = (float)((double)gamma[q.c] * invstd), bt = beta[q.c];
        const double c1 = total[2 * q.c] / N, c2 = total[2 * q.c + 1] / N, ad = (double)a;
        const float *__restrict__ p = z + q.first;
        const float *__restrict__ gp = gy + q.first;
        float *__restrict__ o = gz + q.first;
#pragma unroll 8
        for (int r = 0; r < q.n; ++r) {
            const float zv = p[(size_t)r * C], gv = gp[(size_t)r * C];
            const float gm = (!RELU || bn_pre(zv, mean, a, bt) > 0.f) ? gv : 0.f;
            const double xh = ((double)zv - mean) * invstd;
            o[(size_t)r * C] = (float)(ad * (((double)gm - c1) - xh * c2));
        }
    }
}

inline bool cl_shape_ok(size_t rows, int C) {
    return rows >= 2 && C >= 1 && rows < ((size_t)1 << 31) && rows * (size_t)C < ((size_t)1 << 31);
}

// shared shape and workspace check of the two entries
inline int cl_args(const void *ws, size_t ws_floats, const void *stats, size_t rows, int C) {
    if (!cl_shape_ok(rows, C)) return DECNET_ERR_BAD_SHAPE;
    if (ws_floats < decnet_bn_train_cl_workspace_floats(rows, C)) return DECNET_ERR_BAD_SHAPE;
    if (((uintptr_t)ws & 7) || ((uintptr_t)stats & 7)) return DECNET_ERR_MISALIGNED;
    return DECNET_OK;
}

}  // namespace

size_t decnet_bn_train_cl_workspace_floats(size_t rows, int C) {
    if (!cl_shape_ok(rows, C)) return 0;
    // [nseg][C][2] partials + [C][2] totals, float64
    return 2 * (2 * cl_nseg(rows) * (size_t)C + 2 * (size_t)C);
}

int decnet_bn_train_cl_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                               float *running_mean, float *running_var, double *stats, float *y, int relu, void *ws,
                               size_t ws_floats, size_t rows, int C, void *stream) {
    if (!z || !gamma || !beta || !stats || !y || !ws) return DECNET_ERR_NULL_POINTER;
    if ((running_mean == nullptr) != (running_var == nullptr)) return DECNET_ERR_NULL_POINTER;
    if (const int rc = cl_args(ws, ws_floats, stats, rows, C)) return rc;
    const size_t nseg = cl_nseg(rows), items = nseg * (size_t)C;
    double *part = (double *)ws;
    const dim3 grid(cl_grid(items)), block(CL_THREADS), fin((C + FIN_CH - 1) / FIN_CH);
    hipLaunchKernelGGL(bn_cl_stats_partial, grid, block, 0, (hipStream_t)stream, z, part, items, rows, C);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_cl_stats_finish, fin, block, 0, (hipStream_t)stream, z, (const double *)part, eps, momentum,
                       running_mean, running_var, stats, rows, C, nseg);
    if (const int rc = decnet_launch_status()) return rc;
    if (relu)
        hipLaunchKernelGGL(bn_cl_apply<true>, grid, block, 0, (hipStream_t)stream, z, gamma, beta, (const double *)stats, y,
                           items, rows, C);
    else
        hipLaunchKernelGGL(bn_cl_apply<false>, grid, block, 0, (hipStream_t)stream, z, gamma, beta, (const double *)stats, y,
                           items, rows, C);
    return decnet_launch_status();
}

int decnet_bn_train_cl_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                                float *gz, float *dgamma, float *dbeta, int relu, void *ws, size_t ws_floats, size_t rows,
                                int C, void *stream) {
    if (!z || !gy || !gamma || !beta || !stats || !dgamma || !dbeta || !ws) return DECNET_ERR_NULL_POINTER;
    if (const int rc = cl_args(ws, ws_floats, stats, rows, C)) return rc;
    const size_t nseg = cl_nseg(rows), items = nseg * (size_t)C;
    double *part = (double *)ws, *total = part + 2 * items;
    const dim3 grid(cl_grid(items)), block(CL_THREADS), fin((C + FIN_CH - 1) / FIN_CH);
    if (relu)
        hipLaunchKernelGGL(bn_cl_grad_partial<true>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats, part,
                           items, rows, C);
    else
        hipLaunchKernelGGL(bn_cl_grad_partial<false>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats, part,
                           items, rows, C);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(bn_cl_grad_finish, fin, block, 0, (hipStream_t)stream, (const double *)part, total, dgamma, dbeta, C,
                       nseg);
    if (const int rc = decnet_launch_status()) return rc;
    if (!gz) return DECNET_OK;
    if (relu)
        hipLaunchKernelGGL(bn_cl_grad_input<true>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats,
                           (const double *)total, gz, items, rows, C);
    else
        hipLaunchKernelGGL(bn_cl_grad_input<false>, grid, block, 0, (hipStream_t)stream, z, gy, gamma, beta, stats,
                           (const double *)total, gz, items, rows, C);
    return decnet_launch_status();
}
