// decnet_amd/csrc/loss.hip -- one pyramid level of the multi-stage training loss (modules/loss.py:168-242) and its
// gradient: masked smooth-L1 means of up to four predictions against the ground truth of that level, plus the mean of
// the soft mask over the detail pixels.
//
//   stage_loss_rows      per row of the level: three counts (valid, whole, left) and five sums, 8 doubles;
//   stage_loss_finish    one workgroup: the rows added in a fixed order into sums[8], the five means into terms[5];
//   stage_loss_grad      the gradient planes of the means, every element written.
//
// The reference gathers x[mask] a dozen times per level (a nonzero with a host read-back each).  Here a pixel outside a
// mask is selected out where it is read, so nothing is compacted, nothing read back and nothing data-dependent in shape:
// all three kernels run under stream capture.  Row-structured like imageio.hip's disparity_metrics: a wave owns a row (no
// division per element), lane l takes the pixels l, l + 64, ... in order and accumulates in float64 from the first
// element on, the 64 lane sums are added in a fixed butterfly, and stage_loss_finish adds the rows in a fixed order: the
// same bits for every launch shape and every alignment of the planes (all accesses are single floats), no atomics.
//
// This file is built WITHOUT -fno-honor-nans: a NaN inside a mask has to reach the term, one outside must not.
#include "common.h"

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / DECNET_WAVE;     // rows a workgroup works on at a time (one per wave)
constexpr int NSUM = 8;                                    // per row: n_valid, n_whole, n_left, S_pred, S_dense, S_sparse,
enum { N_VALID, N_WHOLE, N_LEFT, S_PRED, S_DENSE, S_SPARSE, S_FUSION, S_SOFT };     // S_fusion, S_soft
// terms[] in the order the reference appends to loss_list (loss.py:233-237)
enum { T_DENSE, T_SPARSE, T_SOFT, T_FUSION, T_PRED };

inline unsigned loss_grid(size_t rows) {
    const size_t b = (rows + LOSS_WAVES - 1) / LOSS_WAVES;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

// d = a s - g s with each product and the difference rounded to fp32, as torch evaluates pred[mask] * s - gt[mask] * s
// (no contraction into an fma)
__device__ __forceinline__ float scaled_diff(float a, float g, float s) {
#pragma clang fp contract(off)
    const float x = a * s;
    const float y = g * s;
    return x - y;
}

// smooth-L1 with beta 1 of an fp32 difference, in float64
__device__ __forceinline__ double smooth_l1(float d) {
    const double a = fabs((double)d);
    return a < 1.0 ? 0.5 * a * a : a - 0.5;               // a NaN takes the second branch and stays a NaN
}

__device__ __forceinline__ float clamp1(float d) {         // d of the middle branch as it is: a NaN stays a NaN
    return d < -1.f ? -1.f : (d > 1.f ? 1.f : d);
}

template <bool COMPOSITE>
__global__ __launch_bounds__(LOSS_THREADS) void stage_loss_rows(
    const float *__restrict__ pred, const float *__restrict__ dense, const float *__restrict__ sparse,
    const float *__restrict__ fusion, const float *__restrict__ soft, const float *__restrict__ left,
    const float *__restrict__ gt, float gt_max, float s, int skip_rows, double *__restrict__ row_sums, size_t rows, int H,
    int W) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t r = (size_t)blockIdx.x * LOSS_WAVES + wave; r < rows; r += (size_t)gridDim.x * LOSS_WAVES) {
        const bool row_on = (int)(r % (size_t)H) >= skip_rows;                // one division per row
        const size_t o = r * (size_t)W;
        int nv = 0, nw = 0, nl = 0;
        double sp = 0., sd = 0., ss = 0., sf = 0., sm = 0.;
#pragma unroll 2
        for (int x = lane; x < W; x += DECNET_WAVE) {
            const float g = gt[o + x];
            const bool valid = row_on && g > 0.f && g < gt_max;
            if (valid) {
                ++nv;
                sp += smooth_l1(scaled_diff(pred[o + x], g, s));
            }
            if (COMPOSITE) {
                const bool lm = left[o + x] == 1.f;
                if (valid) {
                    sd += smooth_l1(scaled_diff(dense[o + x], g, s));
                    sf += smooth_l1(scaled_diff(fusion[o + x], g, s));
                }
                if (lm) {
                    ++nl;
                    sm += (double)soft[o + x];
                    if (valid) {
                        ++nw;
                        ss += smooth_l1(scaled_diff(sparse[o + x], g, s));
                    }
                }
            }
        }
        for (int k = DECNET_WAVE / 2; k > 0; k >>= 1) {
            nv += __shfl_xor(nv, k);
            sp += __shfl_xor(sp, k);
            if (COMPOSITE) {
                nw += __shfl_xor(nw, k);
                nl += __shfl_xor(nl, k);
                sd += __shfl_xor(sd, k);
                ss += __shfl_xor(ss, k);
                sf += __shfl_xor(sf, k);
                sm += __shfl_xor(sm, k);
            }
        }
        if (lane == 0) {
            double *q = row_sums + r * NSUM;
            q[N_VALID] = (double)nv;
            q[N_WHOLE] = (double)nw;
            q[N_LEFT] = (double)nl;
            q[S_PRED] = sp;
            q[S_DENSE] = sd;
            q[S_SPARSE] = ss;
            q[S_FUSION] = sf;
            q[S_SOFT] = sm;
        }
    }
}

// One workgroup.  Thread t adds the rows t, t + 256, ... in order; the 256 thread sums are added in a fixed tree.
__global__ __launch_bounds__(LOSS_THREADS) void stage_loss_finish(const double *__restrict__ row_sums, size_t rows,
                                                                  int composite, double *__restrict__ sums,
                                                                  float *__restrict__ terms) {
    __shared__ double acc[LOSS_THREADS][NSUM + 1];          // + 1: the eight columns of a thread start in different banks
    double a[NSUM];
    for (int k = 0; k < NSUM; ++k) a[k] = 0.;
    for (size_t r = threadIdx.x; r < rows; r += LOSS_THREADS)
        for (int k = 0; k < NSUM; ++k) a[k] += row_sums[r * NSUM + k];
    for (int k = 0; k < NSUM; ++k) acc[threadIdx.x][k] = a[k];
    __syncthreads();
    for (int n = LOSS_THREADS / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n)
            for (int k = 0; k < NSUM; ++k) acc[threadIdx.x][k] += acc[threadIdx.x + n][k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double *t = acc[0];
        for (int k = 0; k < NSUM; ++k) sums[k] = t[k];
        // a mean over no pixels is 0 / 0 = NaN, as the reference's mean of an empty tensor is
        terms[T_PRED] = (float)(t[S_PRED] / t[N_VALID]);
        terms[T_DENSE] = composite ? (float)(t[S_DENSE] / t[N_VALID]) : 0.f;
        terms[T_FUSION] = composite ? (float)(t[S_FUSION] / t[N_VALID]) : 0.f;
        terms[T_SPARSE] = composite ? (float)(t[S_SPARSE] / t[N_WHOLE]) : 0.f;
        terms[T_SOFT] = composite ? (float)(t[S_SOFT] / t[N_LEFT]) : 0.f;
    }
}

// Gradient of term k with respect to an element inside its mask: grad_terms[k] s clamp(d, -1, 1) / n; of the soft-mask
// mean: grad_terms[2] / n_left; 0 elsewhere, and everywhere when the term's count is 0 (torch's gradient of an empty
// gather).  The per-term factor is formed once per thread in float64; an element is one float64 product, rounded once.
template <bool COMPOSITE>
__global__ __launch_bounds__(LOSS_THREADS) void stage_loss_grad(
    const float *__restrict__ pred, const float *__restrict__ dense, const float *__restrict__ sparse,
    const float *__restrict__ fusion, const float *__restrict__ left, const float *__restrict__ gt, float gt_max, float s,
    int skip_rows, const double *__restrict__ sums, const float *__restrict__ grad_terms, float *__restrict__ g_pred,
    float *__restrict__ g_dense, float *__restrict__ g_sparse, float *__restrict__ g_fusion, float *__restrict__ g_soft,
    size_t rows, int H, int W) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    const double nv = sums[N_VALID], nw = sums[N_WHOLE], nl = sums[N_LEFT];
    const double cp = nv > 0. ? (double)grad_terms[T_PRED] * (double)s / nv : 0.;
    double cd = 0., cs = 0., cf = 0.;
    float cm = 0.f;
    if (COMPOSITE) {
        cd = nv > 0. ? (double)grad_terms[T_DENSE] * (double)s / nv : 0.;
        cf = nv > 0. ? (double)grad_terms[T_FUSION] * (double)s / nv : 0.;
        cs = nw > 0. ? (double)grad_terms[T_SPARSE] * (double)s / nw : 0.;
        cm = nl > 0. ? (float)((double)grad_terms[T_SOFT] / nl) : 0.f;
    }
    for (size_t r = (size_t)blockIdx.x * LOSS_WAVES + wave; r < rows; r += (size_t)gridDim.x * LOSS_WAVES) {
        const bool row_on = (int)(r % (size_t)H) >= skip_rows;
        const size_t o = r * (size_t)W;
#pragma unroll 2
        for (int x = lane; x < W; x += DECNET_WAVE) {
            const float g = gt[o + x];
            const bool valid = row_on && g > 0.f && g < gt_max;
            if (g_pred) g_pred[o + x] = valid ? (float)(cp * (double)clamp1(scaled_diff(pred[o + x], g, s))) : 0.f;
            if (COMPOSITE) {
                const bool lm = left[o + x] == 1.f;
                if (g_dense)
                    g_dense[o + x] = valid ? (float)(cd * (double)clamp1(scaled_diff(dense[o + x], g, s))) : 0.f;
                if (g_fusion)
                    g_fusion[o + x] = valid ? (float)(cf * (double)clamp1(scaled_diff(fusion[o + x], g, s))) : 0.f;
                if (g_sparse)
                    g_sparse[o + x] =
                        (valid && lm) ? (float)(cs * (double)clamp1(scaled_diff(sparse[o + x], g, s))) : 0.f;
                if (g_soft) g_soft[o + x] = lm ? cm : 0.f;
            } else {                                                          // the simple form has no such term
                if (g_dense) g_dense[o + x] = 0.f;
                if (g_fusion) g_fusion[o + x] = 0.f;
                if (g_sparse) g_sparse[o + x] = 0.f;
                if (g_soft) g_soft[o + x] = 0.f;
            }
        }
    }
}

// shared argument check; *composite: all five optional planes given (none: the simple form)
inline int loss_args(const float *pred, const float *dense, const float *sparse, const float *fusion, const float *soft,
                     const float *left, const float *gt, int skip_rows, int B, int H, int W, bool *composite) {
    if (!pred || !gt) return DECNET_ERR_NULL_POINTER;
    const int given = (dense != nullptr) + (sparse != nullptr) + (fusion != nullptr) + (soft != nullptr) + (left != nullptr);
    if (given != 0 && given != 5) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || H < 1 || W < 1 || skip_rows < 0) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * H * W >= 2147483648.0) return DECNET_ERR_BAD_SHAPE;
    *composite = given == 5;
    return DECNET_OK;
}

}  // namespace

int decnet_stage_loss_forward(const float *pred, const float *dense, const float *sparse, const float *fusion,
                              const float *soft_mask, const float *left_mask, const float *gt, float gt_max,
                              float down_size, int skip_rows, double *row_sums, double *sums, float *terms, int B, int H,
                              int W, void *stream) {
    bool composite = false;
    if (!row_sums || !sums || !terms) return DECNET_ERR_NULL_POINTER;
    if (const int rc = loss_args(pred, dense, sparse, fusion, soft_mask, left_mask, gt, skip_rows, B, H, W, &composite))
        return rc;
    const size_t rows = (size_t)B * H;
    const dim3 grid(loss_grid(rows)), block(LOSS_THREADS);
    if (composite)
        hipLaunchKernelGGL(stage_loss_rows<true>, grid, block, 0, (hipStream_t)stream, pred, dense, sparse, fusion,
                           soft_mask, left_mask, gt, gt_max, down_size, skip_rows, row_sums, rows, H, W);
    else
        hipLaunchKernelGGL(stage_loss_rows<false>, grid, block, 0, (hipStream_t)stream, pred, dense, sparse, fusion,
                           soft_mask, left_mask, gt, gt_max, down_size, skip_rows, row_sums, rows, H, W);
    if (const int rc = decnet_launch_status()) return rc;
    hipLaunchKernelGGL(stage_loss_finish, dim3(1), block, 0, (hipStream_t)stream, (const double *)row_sums, rows,
                       composite ? 1 : 0, sums, terms);
    return decnet_launch_status();
}

int decnet_stage_loss_backward(const float *pred, const float *dense, const float *sparse, const float *fusion,
                               const float *soft_mask, const float *left_mask, const float *gt, float gt_max,
                               float down_size, int skip_rows, const double *sums, const float *grad_terms, float *g_pred,
                               float *g_dense, float *g_sparse, float *g_fusion, float *g_soft, int B, int H, int W,
                               void *stream) {
    bool composite = false;
    if (!sums || !grad_terms) return DECNET_ERR_NULL_POINTER;
    if (const int rc = loss_args(pred, dense, sparse, fusion, soft_mask, left_mask, gt, skip_rows, B, H, W, &composite))
        return rc;
    if (!g_pred && !g_dense && !g_sparse && !g_fusion && !g_soft) return DECNET_OK;      // nothing asked for
    const size_t rows = (size_t)B * H;
    const dim3 grid(loss_grid(rows)), block(LOSS_THREADS);
    if (composite)
        hipLaunchKernelGGL(stage_loss_grad<true>, grid, block, 0, (hipStream_t)stream, pred, dense, sparse, fusion,
                           left_mask, gt, gt_max, down_size, skip_rows, sums, grad_terms, g_pred, g_dense, g_sparse,
                           g_fusion, g_soft, rows, H, W);
    else
        hipLaunchKernelGGL(stage_loss_grad<false>, grid, block, 0, (hipStream_t)stream, pred, dense, sparse, fusion,
                           left_mask, gt, gt_max, down_size, skip_rows, sums, grad_terms, g_pred, g_dense, g_sparse,
                           g_fusion, g_soft, rows, H, W);
    return decnet_launch_status();
}
