// decnet_amd/csrc/conv2d_wgrad_reduce.h -- the second launch of the weight-gradient reductions (csrc/conv2d_grad.hip,
// csrc/conv2d_mfma_grad.hip): the partial sets [set][Cout][N1] of the caller's workspace are added in a fixed order in
// float64 -- thread (element, s) the sets s, s + 16, ... in rising order, then the 16 sums in rising s -- and rounded once.
#pragma once
#include "common.h"

namespace {

// G[co][n] (n < N) and gsum[co] (n = N) = the float64 sum of the `nsets` partial sets, rounded once.
__global__ __launch_bounds__(256) void conv2d_wgrad_reduce(const float *__restrict__ ws, float *__restrict__ G,
                                                           float *__restrict__ gsum, int nsets, int Cout, int N1) {
    __shared__ double part[16][17];
    const int e = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int total = Cout * N1, el = blockIdx.x * 16 + e;
    double a = 0.0;
    if (el < total)
        for (int set = s; set < nsets; set += 16) a += (double)ws[(size_t)set * total + el];
    part[s][e] = a;
    __syncthreads();
    if (s == 0 && el < total) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += part[i][e];
        const int co = el / N1, n = el - co * N1;
        if (n == N1 - 1) gsum[co] = (float)t;
        else G[(size_t)co * (N1 - 1) + n] = (float)t;
    }
}

}  // namespace
