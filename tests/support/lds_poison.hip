// Test hooks, not part of the product ABI: fill every CU's LDS with a chosen word before a kernel under test, count how
// much of such a fill a later kernel still finds, and one planted bug (a kernel that uses LDS it never wrote).
// Built into decnet_amd/lib/libdecnet_testhooks.so by decnet_amd.build.build_testhooks(); loaded by tests/_lds_poison.py.
//
// Geometry of poison and probe: 256-thread workgroups that each ask for the device's whole dynamic LDS, so that one
// workgroup owns one CU's LDS while it runs; rounds x multiProcessorCount of them.
// LDS is touched through pointers that keep the LDS address space: a volatile generic pointer made from the array would
// compile to flat loads and stores.
#include <hip/hip_runtime.h>

typedef volatile unsigned __attribute__((address_space(3))) *lds_words;
typedef volatile float __attribute__((address_space(3))) *lds_floats;

#define HOOK_THREADS 256
#define LEAKY_WORDS 1024

extern __shared__ unsigned hook_lds[];

__global__ __launch_bounds__(HOOK_THREADS) void lds_poison_kernel(unsigned pattern, int words) {
    lds_words p = (lds_words)hook_lds;
    for (int i = threadIdx.x; i < words; i += HOOK_THREADS) p[i] = pattern;
}

__global__ __launch_bounds__(HOOK_THREADS) void lds_probe_kernel(unsigned pattern, int words, unsigned *counts) {
    lds_words p = (lds_words)hook_lds;
    unsigned n = 0;
    for (int i = threadIdx.x; i < words; i += HOOK_THREADS) n += p[i] == pattern ? 1u : 0u;
    __syncthreads();                                   // every word has been read: the first words may now carry the sums
    p[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int i = 0; i < HOOK_THREADS; ++i) s += p[i];
        counts[blockIdx.x] = s;
    }
}

// The planted bug: out[i] = 1 + zero * (an LDS word this kernel never wrote), i < LEAKY_WORDS.
__global__ __launch_bounds__(HOOK_THREADS) void lds_leaky_kernel(float zero, float *out) {
    lds_floats p = (lds_floats)hook_lds;
    for (int i = threadIdx.x; i < LEAKY_WORDS; i += HOOK_THREADS) out[i] = 1.0f + zero * p[i];
}

static int geometry(const void *fn, int rounds, int *lds_bytes, int *blocks) {
    if (rounds < 1 || rounds > 64) return -2;
    int dev = 0, lds = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    if (lds < HOOK_THREADS * 4 || cus < 1) return -3;
    *lds_bytes = lds;
    *blocks = rounds * cus;
    return 0;
}

extern "C" {

__attribute__((visibility("default"))) int decnet_test_lds_poison(unsigned pattern, int rounds, void *stream) {
    int lds = 0, blocks = 0;
    int rc = geometry((const void *)lds_poison_kernel, rounds, &lds, &blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(lds_poison_kernel, dim3(blocks), dim3(HOOK_THREADS), lds, (hipStream_t)stream, pattern, lds / 4);
    return (int)hipGetLastError();
}

// counts: rounds x multiProcessorCount words.  Returns the number of LDS words each workgroup read (> 0), or -error.
__attribute__((visibility("default"))) int decnet_test_lds_probe(unsigned pattern, int rounds, unsigned *counts,
                                                                 void *stream) {
    if (!counts) return -1;
    int lds = 0, blocks = 0;
    int rc = geometry((const void *)lds_probe_kernel, rounds, &lds, &blocks);
    if (rc) return rc < 0 ? rc : -rc;
    hipLaunchKernelGGL(lds_probe_kernel, dim3(blocks), dim3(HOOK_THREADS), lds, (hipStream_t)stream, pattern, lds / 4,
                       counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? lds / 4 : -(int)e;
}

// out: LEAKY_WORDS (1024) floats.
__attribute__((visibility("default"))) int decnet_test_lds_leaky(float zero, float *out, void *stream) {
    if (!out) return -1;
    hipLaunchKernelGGL(lds_leaky_kernel, dim3(1), dim3(HOOK_THREADS), LEAKY_WORDS * 4, (hipStream_t)stream, zero, out);
    return (int)hipGetLastError();
}

}
