// decnet_amd/csrc/bn_pre.h -- the pre-activation of training-mode BatchNorm, shared by batchnorm.hip (NCHW planes) and
// batchnorm_cl.hip (channels-last rows): ONE function, contraction pinned, that every forward and backward kernel calls,
// so a backward's ReLU decision is the forward's on every element.
#pragma once
#include <hip/hip_runtime.h>

// fma(z - mean, a, beta): z - mean in float64, rounded once; no contraction beyond the explicit fma
__device__ __forceinline__ float bn_pre(float z, double mean, float a, float beta) {
#pragma clang fp contract(off)
    const float d = (float)((double)z - mean);
    return fmaf(d, a, beta);
}
