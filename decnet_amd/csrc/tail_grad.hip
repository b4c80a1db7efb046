// decnet_amd/csrc/tail_grad.hip -- the gathers of the full-resolution tail under hip_grad(): backward of
// decnet_warp_disparity and decnet_dynamic_upsample3 and the inverse permutation of decnet_unfold3_cat
// (decnet_amd/tail_grad.py; SoftAttention's sigmoid + blend is an elementwise pass, csrc/detail_grad.hip).  Every gradient
// is a gather in a fixed order: no atomics, no allocation, no synchronisation, the same bits on every run and under graph
// replay.  Planes are accepted at any float alignment.
#include "pointwise.h"                                                   // aligned16

namespace {

// ---- inverse of unfold3_cat's feature part: g_fea[b,c,3y+i,3x+j] = g[b,1+9c+3i+j,y,x] ----------------------------------------
__global__ __launch_bounds__(256) void fold3(const float *__restrict__ g, float *__restrict__ g_fea, int C, int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int b = blockIdx.z / C, c = blockIdx.z - b * C;
    if (x >= w) return;
    const size_t cp = (size_t)h * w;                                    // coarse plane
    const float *s = g + ((size_t)b * (9 * C + 1) + 1 + 9 * c) * cp + (size_t)y * w + x;
    float *f = g_fea + (((size_t)b * C + c) * 3 * h + 3 * y) * (3 * (size_t)w) + 3 * x;
    float v[9];                                     // nine requests, then nine stores
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = s[(size_t)t * cp];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) f[(size_t)i * 3 * w + j] = v[i * 3 + j];
}

// ---- backward of dynamic_upsample3 ---------------------------------------------------------------------------------------
// Per coarse pixel and sub-position s: p = softmax_k(logits[9 s + k]) (the forward's max-subtracted expf), m_s = sum_k p_k n_k,
// g_logits[9 s + k] = 3 gout_s p_k (n_k - m_s); q_k = 3 sum_s gout_s p_{s,k} (s rising) goes to the workspace [B,9,h,w]
// for the gather of g_disp (q: NULL when nobody wants g_disp).
__global__ __launch_bounds__(256) void dynamic_upsample3_bwd(const float *__restrict__ logits,
                                                             const float *__restrict__ disp,
                                                             const float *__restrict__ gout,
                                                             float *__restrict__ g_logits, float *__restrict__ q,
                                                             int h, int w) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= w) return;
    const size_t plane = (size_t)h * w;
    const float *dp = disp + (size_t)b * plane;
    float nb[9], qk[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = min(max(y + ky - 1, 0), h - 1), xx = min(max(x + kx - 1, 0), w - 1);   // ReplicationPad2d(1)
            nb[ky * 3 + kx] = dp[(size_t)yy * w + xx];
            qk[ky * 3 + kx] = 0.f;
        }
    const size_t pix = (size_t)y * w + x;
    const float *lp = logits + (size_t)b * 81 * plane + pix;
    float *gl = g_logits + (size_t)b * 81 * plane + pix;
    const float *gp = gout + ((size_t)b * 3 * h + 3 * y) * (3 * (size_t)w) + 3 * x;
#pragma unroll
    for (int sy = 0; sy < 3; ++sy)
#pragma unroll
        for (int sx = 0; sx < 3; ++sx) {
            float v[9], m = -INFINITY;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                v[k] = lp[(size_t)((sy * 3 + sx) * 9 + k) * plane];
                m = fmaxf(m, v[k]);
            }
            const float g3 = gp[(size_t)sy * 3 * w + sx] * 3.0f;
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                v[k] = expf(v[k] - m);
                sum += v[k];
            }
            float ms = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                v[k] = v[k] / sum;
                ms += v[k] * nb[k];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float gpk = g3 * v[k];
                qk[k] += gpk;
                gl[(size_t)((sy * 3 + sx) * 9 + k) * plane] = gpk * (nb[k] - ms);
            }
        }
    if (q) {
        float *qp = q + (size_t)b * 9 * plane + pix;
#pragma unroll
        for (int k = 0; k < 9; ++k) qp[(size_t)k * plane] = qk[k];
    }
}

// g_disp[Y,X] = sum of q_k(y,x) over every (y, x, k) whose replicate-clamped neighbour is (Y,X): y, then x, then k, rising.
__global__ __launch_bounds__(256) void dynamic_upsample3_gdisp(const float *__restrict__ q, float *__restrict__ g_disp,
                                                               int h, int w) {
#pragma clang fp contract(off)
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
    if (X >= w) return;
    const size_t plane = (size_t)h * w;
    const float *qb = q + (size_t)b * 9 * plane;
    float acc = 0.f;
    for (int y = max(Y - 1, 0); y <= min(Y + 1, h - 1); ++y)
        for (int x = max(X - 1, 0); x <= min(X + 1, w - 1); ++x)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = min(max(y + k / 3 - 1, 0), h - 1), xx = min(max(x + k % 3 - 1, 0), w - 1);
                if (yy == Y && xx == X) acc += qb[(size_t)k * plane + (size_t)y * w + x];
            }
    g_disp[(size_t)b * plane + (size_t)Y * w + X] = acc;
}

// ---- backward of warp_disparity -------------------------------------------------------------------------------------------
// The sampling position with the forward kernel's fp32 operation sequence (csrc/conv2d_small.hip, contraction off): the
// cell floor(ix), floor(iy) is the forward's cell.
__device__ __forceinline__ float warp_ix(int x, float d, int W) {
#pragma clang fp contract(off)
    const float cx = ((float)x - d) / ((float)(W - 1.0) / 2.0f) - 1.0f;
    return ((cx + 1.0f) * (float)W - 1.0f) / 2.0f;
}
__device__ __forceinline__ float warp_iy(int y, int H) {
#pragma clang fp contract(off)
    const float cy = (float)y / ((float)(H - 1.0) / 2.0f) - 1.0f;
    return ((cy + 1.0f) * (float)H - 1.0f) / 2.0f;
}

// g_disp[b,y,x] = -W/(W-1) sum_c gout[b,c,y,x] ((v_ne - v_nw)(1 - t_y) + (v_se - v_sw) t_y), taps outside the image zero:
// grid_sampler's within-cell derivative chained through cx and the un-normalisation.  A gather with the forward's
// structure: all loads of a channel block from clamped addresses, selected afterwards; channels summed in rising order.
__global__ __launch_bounds__(256) void warp_disparity_gdisp(const float *__restrict__ right,
                                                            const float *__restrict__ disp,
                                                            const float *__restrict__ gout, float *__restrict__ g_disp,
                                                            int C, int H, int W, int nrows) {
#pragma clang fp contract(off)
    int bx, row;
    if (!decnet_xcd_rows((W + 255) >> 8, nrows, bx, row)) return;
    const int x = bx * 256 + threadIdx.x, b = row / H, y = row - b * H;
    if (x >= W) return;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const float ix = warp_ix(x, disp[(size_t)b * plane + pix], W), iy = warp_iy(y, H);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float wn = fy + 1.0f - iy, ws = iy - fy;                       // the forward's row weights: 1 - t_y, t_y
    const bool vx0 = (unsigned)x0 < (unsigned)W, vx1 = (unsigned)x1 < (unsigned)W;
    const bool vy0 = (unsigned)y0 < (unsigned)H, vy1 = (unsigned)y1 < (unsigned)H;
    const float *rb = right + (size_t)b * C * plane;
    const float *gb = gout + (size_t)b * C * plane + pix;
    const size_t o00 = (size_t)(vy0 ? y0 : 0) * W + (vx0 ? x0 : 0), o01 = (size_t)(vy0 ? y0 : 0) * W + (vx1 ? x1 : 0);
    const size_t o10 = (size_t)(vy1 ? y1 : 0) * W + (vx0 ? x0 : 0), o11 = (size_t)(vy1 ? y1 : 0) * W + (vx1 ? x1 : 0);
    float acc = 0.f;
    for (int c0 = 0; c0 < C; c0 += 8) {
        float t[8][4], g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const size_t co = (size_t)(c0 + e < C ? c0 + e : c0) * plane;
            const float *rp = rb + co;
            t[e][0] = rp[o00]; t[e][1] = rp[o01]; t[e][2] = rp[o10]; t[e][3] = rp[o11];
            g[e] = gb[co];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (c0 + e >= C) break;
            const float nw = vy0 && vx0 ? t[e][0] : 0.f, ne = vy0 && vx1 ? t[e][1] : 0.f;
            const float sw = vy1 && vx0 ? t[e][2] : 0.f, se = vy1 && vx1 ? t[e][3] : 0.f;
            const float top = (ne - nw) * wn, bot = (se - sw) * ws;
            acc += g[e] * (top + bot);
        }
    }
    g_disp[(size_t)b * plane + pix] = -((float)W / (float)(W - 1)) * acc;
}

// g_right[b,c,y',x'] = sum over the output pixels (y, x) that sampled (y', x'), rows y rising, then x rising: the transpose
// of the forward as a gather.  iy = y H/(H-1) - 0.5 has slope > 1, so at most two output rows (y within y' +- 2) touch a
// source row; in x the map is data dependent, so a workgroup (one (b, y'), 256 columns x') stages the row's ix[W] in LDS,
// reduces the row's min / max of x - ix, stages gout of the columns that can reach its x' (8 channels at a time) and
// every thread scans the window that min / max allow.  Weights are the forward's: (fx + 1 - ix | ix - fx) * (row weight).
// LDS: 4 W (ix) + 32 W (gout block) + 8 words of the reduction.
__global__ __launch_bounds__(256) void warp_disparity_gright(const float *__restrict__ disp,
                                                             const float *__restrict__ gout,
                                                             float *__restrict__ g_right, int C, int H, int W) {
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    float *red = lds, *ixs = lds + 8, *gs = lds + 8 + W;                 // gs[e][window column]
    const int tid = threadIdx.x, X0 = blockIdx.x * 256, xp = X0 + tid, yp = blockIdx.y, b = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float lim = (float)(W + 2);
    for (int c0 = 0; c0 < C; c0 += 8) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int y = max(yp - 2, 0); y <= min(yp + 2, H - 1); ++y) {     // workgroup-uniform
            const float iy = warp_iy(y, H), fy = floorf(iy);
            const int y0 = (int)fy;
            float wy;
            if (y0 == yp) wy = fy + 1.0f - iy;
            else if (y0 + 1 == yp) wy = iy - fy;
            else continue;
            __syncthreads();                                             // the previous row's scans are done
            const float *dp = disp + (size_t)b * plane + (size_t)y * W;
            float lo = lim, hi = -lim;
            for (int x = tid; x < W; x += 256) {
                const float ix = warp_ix(x, dp[x], W);
                ixs[x] = ix;
                const float dl = fminf(fmaxf((float)x - ix, -lim), lim);
                lo = fminf(lo, dl);
                hi = fmaxf(hi, dl);
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                lo = fminf(lo, __shfl_xor(lo, s));
                hi = fmaxf(hi, __shfl_xor(hi, s));
            }
            if ((tid & 63) == 0) { red[tid >> 6] = lo; red[4 + (tid >> 6)] = hi; }
            __syncthreads();
            lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
            hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
            // x' = ix + t, |t| < 1 and x = ix + (x - ix): x in (x' - 1 + lo, x' + 1 + hi); one more column each side for
            // the rounding of x - ix
            const int dlo = (int)floorf(lo) - 2, dhi = (int)ceilf(hi) + 2;
            const int s0 = max(X0 + dlo, 0), s1 = min(X0 + 255 + dhi, W - 1), sw = s1 - s0 + 1;   // the block's window
            const float *gp = gout + ((size_t)b * C + c0) * plane + (size_t)y * W;
            for (int e = 0; e < 8; ++e) {
                if (c0 + e >= C) break;
                for (int i = tid; i < sw; i += 256) gs[e * W + i] = gp[(size_t)e * plane + s0 + i];
            }
            __syncthreads();
            if (xp < W) {
                const int a = max(xp + dlo, 0), z = min(xp + dhi, W - 1);
                for (int x = a; x <= z; ++x) {
                    const float ix = ixs[x], fx = floorf(ix);
                    float wx;
                    if (fx == (float)xp) wx = fx + 1.0f - ix;
                    else if (fx + 1.0f == (float)xp) wx = ix - fx;
                    else continue;
                    const float wgt = wx * wy;
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c0 + e < C) acc[e] += gs[e * W + (x - s0)] * wgt;
                }
            }
        }
        if (xp < W) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C) g_right[((size_t)b * C + c0 + e) * plane + (size_t)yp * W + xp] = acc[e];
        }
    }
}

constexpr int GRIGHT_MAX_W = (DECNET_LDS_BUDGET - 32) / 36;              // 1819: ix[W] + gout[8][W] in 64 KiB

}  // namespace

extern "C" {

int decnet_fold3(const float *g, float *g_fea, int B, int C, int h, int w, void *stream) {
    if (!g || !g_fea) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || h < 1 || w < 1 || h > 65535 || (long)B * (C + 1) > 65535) return DECNET_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(fold3, dim3((unsigned)ceil_div(w, 256), (unsigned)h, (unsigned)(B * C)), dim3(256), 0,
                       (hipStream_t)stream, g, g_fea, C, h, w);
    return decnet_launch_status();
}

size_t decnet_dynamic_upsample3_backward_workspace_floats(int B, int h, int w) {
    if (B < 1 || h < 1 || w < 1 || h > 65535 || B > 65535) return 0;
    return ((size_t)B * 9 * h * w + 3) / 4 * 4;
}

int decnet_dynamic_upsample3_backward(const float *logits, const float *disp, const float *gout, float *g_logits,
                                      float *g_disp, float *workspace, size_t workspace_floats, int B, int h, int w,
                                      void *stream) {
    if (!logits || !disp || !gout || !g_logits) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || h < 1 || w < 1) return DECNET_ERR_BAD_SHAPE;
    if (h > 65535 || B > 65535) return DECNET_ERR_UNSUPPORTED;
    if (g_disp) {
        if (!workspace) return DECNET_ERR_NULL_POINTER;
        if (workspace_floats < decnet_dynamic_upsample3_backward_workspace_floats(B, h, w)) return DECNET_ERR_BAD_SHAPE;
        if (!aligned16(workspace)) return DECNET_ERR_MISALIGNED;
    }
    const dim3 grid((unsigned)ceil_div(w, 256), (unsigned)h, (unsigned)B);
    hipLaunchKernelGGL(dynamic_upsample3_bwd, grid, dim3(256), 0, (hipStream_t)stream, logits, disp, gout, g_logits,
                       g_disp ? workspace : nullptr, h, w);
    int rc = decnet_launch_status();
    if (rc || !g_disp) return rc;
    hipLaunchKernelGGL(dynamic_upsample3_gdisp, grid, dim3(256), 0, (hipStream_t)stream, workspace, g_disp, h, w);
    return decnet_launch_status();
}

int decnet_warp_disparity_backward(const float *right, const float *disp, const float *gout, float *g_right,
                                   float *g_disp, int B, int C, int H, int W, void *stream) {
    if (!right || !disp || !gout || (!g_right && !g_disp)) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || H < 2 || W < 2) return DECNET_ERR_BAD_SHAPE;
    if (H > 65535 || B > 65535 || (double)B * H * ceil_div(W, 256) >= 2.0e9) return DECNET_ERR_UNSUPPORTED;
    if (g_right && W > GRIGHT_MAX_W) return DECNET_ERR_UNSUPPORTED;     // the row no longer fits the LDS plan
    if (g_disp) {
        hipLaunchKernelGGL(warp_disparity_gdisp, dim3(decnet_xcd_grid(ceil_div(W, 256), (long)H * B)), dim3(256), 0,
                           (hipStream_t)stream, right, disp, gout, g_disp, C, H, W, H * B);
        const int rc = decnet_launch_status();
        if (rc) return rc;
    }
    if (g_right) {
        hipLaunchKernelGGL(warp_disparity_gright, dim3((unsigned)ceil_div(W, 256), (unsigned)H, (unsigned)B), dim3(256),
                           (size_t)(8 + 9 * W) * 4, (hipStream_t)stream, disp, gout, g_right, C, H, W);
        return decnet_launch_status();
    }
    return DECNET_OK;
}

}  // extern "C"
