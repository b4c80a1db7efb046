// decnet_amd/csrc/wgrad_common.h -- what the five weight-gradient entries share (csrc/conv2d_grad.hip,
// csrc/conv2d_mfma_grad.hip, csrc/conv3d_grad.hip).  Every entry is the same sequence around its own GEMM kernel:
//   refusals, nothing launched: NULL pointers (also y without gm), the shape and its plan, then wgrad_workspace() -- fewer
//     workspace floats than the entry's query: BAD_SHAPE; a workspace off 16 bytes: MISALIGNED;
//   1. launch_relu_mask forms gm = gy * [y > 0] once (skipped when gm is NULL: no ReLU, the GEMM reads gy).
//      csrc/conv2d_grad.hip forms gm inside its GEMM instead;
//   2. the file's *_partial kernel writes partial sets [set][Cout][N1] of the GEMM [Cout x pixels] . [pixels x N1] to the
//      caller's workspace; column N1 - 1 is all ones and yields gsum.  Partition and order are functions of the shape alone;
//   3. launch_wgrad_reduce adds the sets in a fixed order in float64 -- thread (element, s) the sets s, s + 16, ... in
//      rising order, then the 16 sums in rising s --, rounds once and writes G in the layer's weight layout and gsum.
// All on the caller's stream, no atomics, decnet_launch_status() after each launch.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// ---- the parts [B, c_i, H, W] of a channel concatenation that is never materialised (the stride-1 entries) -------------------
constexpr int MAXSEG = 6;
struct Segs {
    const float *p[MAXSEG];
    int c[MAXSEG];
    int n;
};

// (xs, cins, nseg <= MAXSEG) -> *in and the channels together; a part of more than max_channels is refused
inline int make_segs(const float *const *xs, const int *cins, int nseg, int max_channels, Segs *in, int *cin) {
    *cin = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!xs[i]) return DECNET_ERR_NULL_POINTER;
        if (cins[i] < 1) return DECNET_ERR_BAD_SHAPE;
        if (cins[i] > max_channels) return DECNET_ERR_UNSUPPORTED;
        in->p[i] = xs[i]; in->c[i] = cins[i];
        *cin += cins[i];
    }
    in->n = nseg;
    return DECNET_OK;
}

// The refusals of a stride-1 entry (decnet_conv2d_wgrad, decnet_conv2d_mfma_wgrad: one argument list) that come before its
// plan, in their order; Cout and Cin are at most max_channels.
inline int wgrad_stride1_args(const float *const *xs, const int *cins, int nseg, const float *gy, const float *y,
                              const float *gm, const float *G, const float *gsum, const float *workspace, int B, int Cout,
                              int H, int W, int k, int dilation, int max_channels, Segs *in, int *cin) {
    if (!xs || !cins || !gy || !G || !gsum || !workspace || (y && !gm)) return DECNET_ERR_NULL_POINTER;
    if (nseg < 1 || nseg > MAXSEG) return DECNET_ERR_UNSUPPORTED;
    if (B < 1 || Cout < 1 || H < 1 || W < 1 || dilation < 1) return DECNET_ERR_BAD_SHAPE;
    if (int rc = make_segs(xs, cins, nseg, max_channels, in, cin)) return rc;
    if ((k != 1 && k != 3) || Cout > max_channels || *cin > max_channels) return DECNET_ERR_UNSUPPORTED;
    if ((double)B * (*cin > Cout ? *cin : Cout) * H * W >= 9.0e18) return DECNET_ERR_BAD_SHAPE;
    return DECNET_OK;
}

// the last two refusals of every entry, after its plan: `need` is the entry's own size query
inline int wgrad_workspace(const float *workspace, size_t workspace_floats, size_t need) {
    if (workspace_floats < need) return DECNET_ERR_BAD_SHAPE;
    if ((uintptr_t)workspace & 15) return DECNET_ERR_MISALIGNED;
    return DECNET_OK;
}

// ---- 1. gm = gy * [y > 0] (without y: a copy) ---------------------------------------------------------------------------------
// (csrc/conv2d_grad.hip, which forms gm in its GEMM, carries a copy of this small kernel that it never launches)
__global__ __launch_bounds__(256) void relu_mask(const float *__restrict__ gy, const float *__restrict__ y,
                                                 float *__restrict__ gm, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        gm[i] = !y || y[i] > 0.f ? gy[i] : 0.f;
}

// gm NULL: nothing to do
inline int launch_relu_mask(const float *gy, const float *y, float *gm, size_t n, hipStream_t s) {
    if (!gm) return DECNET_OK;
    const size_t blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(relu_mask, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, gy, y, gm, n);
    return decnet_launch_status();
}

// ---- 3. G and gsum[co] (GEMM column N1 - 1) = the float64 sum of the `nsets` partial sets, rounded once ------------------------
// TAPS 0: G[co][n], the GEMM columns are in the weight's own order (the NCHW entries).  TAPS 27: column n = tap Ci + ci goes
// to G[co][ci][tap], torch's [Co,Ci,3,3,3] (the channels-last entry).
template <int TAPS>
__global__ __launch_bounds__(256) void wgrad_reduce(const float *__restrict__ ws, float *__restrict__ G,
                                                    float *__restrict__ gsum, long nsets, int Cout, int N1) {
    __shared__ double part[16][17];
    const int e = threadIdx.x & 15, s = threadIdx.x >> 4;
    const long total = (long)Cout * N1, el = (long)blockIdx.x * 16 + e;
    double a = 0.0;
    if (el < total) {
        const float *p = ws + (size_t)s * total + el;                  // (a pointer walk: one 64-bit add per set)
        for (long set = s; set < nsets; set += 16, p += 16 * (size_t)total) a += (double)*p;
    }
    part[s][e] = a;
    __syncthreads();
    if (s == 0 && el < total) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += part[i][e];
        // (el < total: a 32-bit division wherever Cout N1 fits one, which is every shape the entries' plans cover today)
        const int co = total >> 31 ? (int)(el / N1) : (int)((unsigned)el / (unsigned)N1), n = (int)(el - (long)co * N1);
        if (n == N1 - 1) gsum[co] = (float)t;
        else if (TAPS == 0) G[(size_t)co * (N1 - 1) + n] = (float)t;
        else {
            const int Ci = (N1 - 1) / TAPS, tap = n / Ci, ci = n - tap * Ci;
            G[((size_t)co * Ci + ci) * TAPS + tap] = (float)t;
        }
    }
}

template <int TAPS = 0>
inline int launch_wgrad_reduce(const float *ws, float *G, float *gsum, long nsets, int Cout, int N1, hipStream_t s) {
    const long total = (long)Cout * N1;
    hipLaunchKernelGGL(wgrad_reduce<TAPS>, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, ws, G, gsum, nsets, Cout, N1);
    return decnet_launch_status();
}

}  // namespace
