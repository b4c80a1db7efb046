// decnet_amd/csrc/pointwise.h -- what the elementwise fp32 passes share (csrc/detail_grad.hip, csrc/maskgen.hip; the
// alignment test also serves csrc/tail_grad.hip).  A pass gives every thread four consecutive floats of each of its planes:
//   * the quad access: 16 bytes per plane where the host found every plane of the call 16-byte aligned and all four
//     elements exist (`full`), otherwise clamped scalar reads and guarded scalar stores.  The values do not depend on it;
//   * flat passes (n floats, planes of one shape): thread t of the grid flat_grid(n) has the floats 4 t .. 4 t + 3
//     (flat_quad), and flat_pass() is the entry's tail: its refusals after the NULL test, the launch, the launch's status;
//   * row passes ([B,H,W], 1024 pixels of a row per workgroup): row_refusal(), and pack_mask_bits() for the bit plane;
//   * sigmoid_f and blend_f: the statements of SoftAttention's tail and of the detail map's, contraction off.  blend_f is the
//     statement sequence of the epi == 1 branch of conv2d_small (csrc/conv2d_small.hip): the same bits.
#pragma once
#include "common.h"

namespace {

// ---- device: the quad access -----------------------------------------------------------------------------------------------
// v[k][e] = p_k[i0 + e], e < 4, for the planes p_0, p_1, ... of n > i0 floats each: a read past n is the read of p_k[i0].
// ONE branch on `full` around all of a thread's loads (a branch per plane costs the blend's backward 90 instructions).
// The planes are __restrict__ parameters: without that detail_tail (csrc/detail_grad.hip) compiles to other code.
template <typename... P>
__device__ __forceinline__ void load_quads(size_t i0, size_t n, bool full, float (*v)[4], const P *__restrict__... p) {
    int k = 0;
    if (full) {
        const auto quad = [&](const float *q) {
            const float4 t = *reinterpret_cast<const float4 *>(q + i0);
            v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
            ++k;
        };
        (quad(p), ...);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t i = i0 + e < n ? i0 + e : i0;
            k = 0;
            ((v[k++][e] = p[i]), ...);
        }
    }
}

// p_k[i0 + e] = v[k][e] for i0 + e < n.  Bit k of OPTIONAL: plane k may be NULL and is skipped then.
template <unsigned OPTIONAL = 0, typename... P>
__device__ __forceinline__ void store_quads(size_t i0, size_t n, bool full, const float (*v)[4], P *__restrict__... p) {
    int k = 0;
    const auto given = [&](const float *q) { return !(OPTIONAL >> k & 1) || q; };
    if (full) {
        const auto quad = [&](float *q) {
            if (given(q)) *reinterpret_cast<float4 *>(q + i0) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
            ++k;
        };
        (quad(p), ...);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) {
                const auto one = [&](float *q) {
                    if (given(q)) q[i0 + e] = v[k][e];
                    ++k;
                };
                k = 0;
                (one(p), ...);
            }
    }
}

// A flat pass's thread: its quad starts at i0 (false: past n, nothing to do); full: see above.
__device__ __forceinline__ bool flat_quad(size_t n, int vec, size_t &i0, bool &full) {
    i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    full = vec && i0 + 3 < n;
    return i0 < n;
}

// torch.sigmoid
__device__ __forceinline__ float sigmoid_f(float z) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-z));
}

// a (1 - s) + s b
__device__ __forceinline__ float blend_f(float sft, float a, float b) {
#pragma clang fp contract(off)
    const float t1 = a * (1.f - sft), t2 = sft * b;
    return t1 + t2;
}

// bit i of a 16-bit value -> bit 4 i of a 64-bit word
__device__ __forceinline__ unsigned long long spread4(unsigned long long x) {
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

// The bit plane of a row pass, bit i of word w = pixel 64 w + i: on[e] is the thread's pixel x0 + e (false past W),
// x0 = 4 (256 bx + threadIdx.x).  Four ballots: lane l holds pixels 4 l .. 4 l + 3 of the wave's 256, word w of them =
// lanes 16 w .. 16 w + 15, written by lane 16 w.  Every lane of the wave calls this.
__device__ __forceinline__ void pack_mask_bits(const bool (&on)[4], int x0, size_t row, int words_per_row,
                                               unsigned long long *__restrict__ bits) {
    const unsigned long long b0 = __ballot(on[0]), b1 = __ballot(on[1]), b2 = __ballot(on[2]), b3 = __ballot(on[3]);
    const int lane = threadIdx.x & 63;
    if ((lane & 15) == 0) {
        const int sh = lane;
        const unsigned long long word = spread4(b0 >> sh) | (spread4(b1 >> sh) << 1) | (spread4(b2 >> sh) << 2) |
                                        (spread4(b3 >> sh) << 3);
        const int wi = x0 >> 6;
        if (wi < words_per_row) bits[row * (size_t)words_per_row + wi] = word;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// every pointer 16-byte aligned (NULL counts as aligned)
template <typename... P>
inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }

constexpr size_t FLAT_MAX = (size_t)1 << 40;
inline unsigned flat_grid(size_t n) { return (unsigned)((n + 1023) / 1024); }

// What a flat entry does after its NULL test: n < 1 is BAD_SHAPE, n > FLAT_MAX is UNSUPPORTED (nothing launched), else
// the kernel over flat_grid(n) on the caller's stream.
template <typename... K, typename... A>
inline int flat_pass(void (*kernel)(K...), size_t n, void *stream, A... args) {
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, args...);
    return decnet_launch_status();
}

// The limits of a row pass over [B,H,W] after its NULL test; its grid is B H ceil(W / 1024) workgroups.
inline int row_refusal(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * H * ceil_div(W, 1024) >= 2.0e9 || W > (1 << 28)) return DECNET_ERR_UNSUPPORTED;
    return DECNET_OK;
}

}  // namespace
