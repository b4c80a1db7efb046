// decnet_amd/csrc/detail_grad.hip -- the two outputs a training forward keeps beside the disparities: the detail maps of
// GenerateSparseMask (the squared difference and the sigmoid / threshold / bit-plane tail as passes of their own, each with
// its backward; the units in between have their own routes) and SoftAttention's soft mask next to its blend
// (decnet_amd/tail_grad.py).  Every kernel is elementwise fp32 with contraction off: no LDS, no atomics, no allocation, no
// synchronisation, the same bits on every run and under graph replay.  Planes are accepted at any float alignment (16-byte
// accesses only where every plane of the call is 16-byte aligned; the values do not depend on it).
#include "common.h"

namespace {

// four consecutive floats from i0 (clamped reads past n), as 16 bytes where `full`
__device__ __forceinline__ void load4(const float *__restrict__ p, size_t i0, size_t n, bool full, float v[4]) {
    if (full) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p[i0 + e < n ? i0 + e : i0];
    }
}

__device__ __forceinline__ void store4(float *__restrict__ p, size_t i0, size_t n, bool full, const float v[4]) {
    if (full) {
        *reinterpret_cast<float4 *>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) p[i0 + e] = v[e];
    }
}

// ---- res_info = (cur - pre)^2: d = a - b, out = d d, both rounded (torch's (a - b) * (a - b)) ------------------------------
__global__ __launch_bounds__(256) void sqdiff(const float *__restrict__ a, const float *__restrict__ b,
                                              float *__restrict__ out, size_t n, int vec) {
#pragma clang fp contract(off)
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float va[4], vb[4], r[4];
    load4(a, i0, n, full, va);
    load4(b, i0, n, full, vb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = va[e] - vb[e];
        r[e] = d * d;
    }
    store4(out, i0, n, full, r);
}

// t = gout d, g_a = t + t, g_b = -g_a: autograd through d * d (gout d twice, summed) and through a - b.  g_a, g_b: one
// may be NULL.
__global__ __launch_bounds__(256) void sqdiff_bwd(const float *__restrict__ a, const float *__restrict__ b,
                                                  const float *__restrict__ gout, float *__restrict__ g_a,
                                                  float *__restrict__ g_b, size_t n, int vec) {
#pragma clang fp contract(off)
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float va[4], vb[4], vg[4], ra[4], rb[4];
    load4(a, i0, n, full, va);
    load4(b, i0, n, full, vb);
    load4(gout, i0, n, full, vg);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = va[e] - vb[e];
        const float t = vg[e] * d;
        ra[e] = t + t;
        rb[e] = -ra[e];
    }
    if (g_a) store4(g_a, i0, n, full, ra);
    if (g_b) store4(g_b, i0, n, full, rb);
}

// ---- the tail of the detail map: prob = sigmoid(z), mask = prob > thold, the mask bit-packed -----------------------------------
// bit i of a 16-bit value -> bit 4 i of a 64-bit word (spread4 of csrc/maskgen.hip)
__device__ __forceinline__ unsigned long long spread4(unsigned long long x) {
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

// One row segment of 1024 pixels per workgroup, four consecutive pixels per thread (the layout of detail_mask,
// csrc/maskgen.hip, so that the bit plane is assembled the same way).  Every thread of a workgroup that has a pixel in the
// row stays for the ballots: a lane past W contributes zero bits.  prob, mask, bits: each may be NULL.
__global__ __launch_bounds__(256) void detail_tail(const float *__restrict__ logits, float thold,
                                                   float *__restrict__ prob, float *__restrict__ mask,
                                                   unsigned long long *__restrict__ bits, int W, int gx,
                                                   int words_per_row, int vec) {
#pragma clang fp contract(off)
    const size_t row = blockIdx.x / (unsigned)gx;
    const int bx = (int)(blockIdx.x - row * (unsigned)gx);
    const int x0 = (bx * 256 + threadIdx.x) * 4;
    const size_t pix = row * (size_t)W + (x0 < W ? x0 : 0);
    const size_t nrow = (size_t)(x0 < W ? W - x0 : 0);                       // pixels of the row from x0 on
    const bool full = vec && nrow >= 4;
    float z[4], s[4], m[4];
    bool on[4];
    if (nrow) {
        load4(logits + pix, 0, nrow, full, z);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s[e] = 1.f / (1.f + expf(-z[e]));                                      // the statement of csrc/maskgen.hip (torch.sigmoid)
        on[e] = (size_t)e < nrow && s[e] > thold;
        m[e] = on[e] ? 1.f : 0.f;
    }
    if (nrow) {
        if (prob) store4(prob + pix, 0, nrow, full, s);
        if (mask) store4(mask + pix, 0, nrow, full, m);
    }
    if (bits) {
        // the ballot packing of csrc/maskgen.hip: lane l holds pixels 4 l .. 4 l + 3 of the wave's 256, word w = lanes 16 w .. 16 w + 15
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
}

// g_z = g (s (1 - s)), s recomputed as the forward computes it: a saturated sigmoid gives s (1 - s) = 0 exactly.
__global__ __launch_bounds__(256) void detail_tail_bwd(const float *__restrict__ logits, const float *__restrict__ g_prob,
                                                       float *__restrict__ g_logits, size_t n, int vec) {
#pragma clang fp contract(off)
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float z[4], g[4], r[4];
    load4(logits, i0, n, full, z);
    load4(g_prob, i0, n, full, g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s = 1.f / (1.f + expf(-z[e]));
        r[e] = g[e] * (s * (1.f - s));
    }
    store4(g_logits, i0, n, full, r);
}

// ---- SoftAttention's tail with the soft mask kept: the statement sequence of sigmoid_blend (csrc/tail_grad.hip), which is
// that of the epi == 1 branch of conv2d_small (csrc/conv2d_small.hip): the same bits; soft = sft ------------------------------
__global__ __launch_bounds__(256) void sigmoid_blend_soft(const float *__restrict__ o, const float *__restrict__ a,
                                                          const float *__restrict__ b, float *__restrict__ out,
                                                          float *__restrict__ soft, size_t n, int vec) {
#pragma clang fp contract(off)
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float vo[4], va[4], vb[4], r[4], sf[4];
    load4(o, i0, n, full, vo);
    load4(a, i0, n, full, va);
    load4(b, i0, n, full, vb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float sft = 1.f / (1.f + expf(-vo[e]));
        const float t1 = va[e] * (1.f - sft), t2 = sft * vb[e];
        r[e] = t1 + t2;
        sf[e] = sft;
    }
    store4(out, i0, n, full, r);
    store4(soft, i0, n, full, sf);
}

// g_o = (gout (b - a) + gsoft) (s (1 - s)), g_a = gout (1 - s), g_b = gout s -- sigmoid_blend_bwd (csrc/tail_grad.hip) with
// the soft mask's gradient added before the sigmoid's derivative.  gout, gsoft: one may be NULL (wave-uniform): without
// gsoft the statements of sigmoid_blend_bwd, without gout g_o = gsoft (s (1 - s)) and zeros for g_a, g_b.  g_a, g_b: may be
// NULL.
__global__ __launch_bounds__(256) void sigmoid_blend_soft_bwd(const float *__restrict__ o, const float *__restrict__ a,
                                                              const float *__restrict__ b, const float *__restrict__ gout,
                                                              const float *__restrict__ gsoft, float *__restrict__ g_o,
                                                              float *__restrict__ g_a, float *__restrict__ g_b, size_t n,
                                                              int vec) {
#pragma clang fp contract(off)
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float vo[4], va[4], vb[4], vg[4], vs[4], ro[4], ra[4], rb[4];
    load4(o, i0, n, full, vo);
    if (gout) {
        load4(a, i0, n, full, va);
        load4(b, i0, n, full, vb);
        load4(gout, i0, n, full, vg);
    }
    if (gsoft) load4(gsoft, i0, n, full, vs);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float sft = 1.f / (1.f + expf(-vo[e]));
        const float om = 1.f - sft;
        if (gout) {
            float t = vg[e] * (vb[e] - va[e]);
            if (gsoft) t = t + vs[e];
            ro[e] = t * (sft * om);
            ra[e] = vg[e] * om;
            rb[e] = vg[e] * sft;
        } else {
            ro[e] = vs[e] * (sft * om);
            ra[e] = 0.f;
            rb[e] = 0.f;
        }
    }
    store4(g_o, i0, n, full, ro);
    if (g_a) store4(g_a, i0, n, full, ra);
    if (g_b) store4(g_b, i0, n, full, rb);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }    // (NULL counts as aligned)
inline unsigned flat_grid(size_t n) { return (unsigned)((n + 1023) / 1024); }
constexpr size_t FLAT_MAX = (size_t)1 << 40;                                 // as the flat entries of csrc/tail_grad.hip

}  // namespace

extern "C" {

int decnet_sqdiff(const float *a, const float *b, float *out, size_t n, void *stream) {
    if (!a || !b || !out) return DECNET_ERR_NULL_POINTER;
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    const int vec = aligned16(a) && aligned16(b) && aligned16(out);
    hipLaunchKernelGGL(sqdiff, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, out, n, vec);
    return decnet_launch_status();
}

int decnet_sqdiff_backward(const float *a, const float *b, const float *gout, float *g_a, float *g_b, size_t n,
                           void *stream) {
    if (!a || !b || !gout || (!g_a && !g_b)) return DECNET_ERR_NULL_POINTER;
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    const int vec = aligned16(a) && aligned16(b) && aligned16(gout) && aligned16(g_a) && aligned16(g_b);
    hipLaunchKernelGGL(sqdiff_bwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, gout, g_a, g_b, n, vec);
    return decnet_launch_status();
}

int decnet_detail_tail(const float *logits, float thold, float *prob, float *mask, unsigned long long *bits, int B, int H,
                       int W, void *stream) {
    if (!logits || (!prob && !mask && !bits)) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * H * ceil_div(W, 1024) >= 2.0e9 || W > (1 << 28)) return DECNET_ERR_UNSUPPORTED;   // as decnet_detail_mask
    const int gx = ceil_div(W, 1024);
    // rows start at multiples of W floats: 16-byte accesses need W % 4 == 0 as well
    const int vec = (W & 3) == 0 && aligned16(logits) && aligned16(prob) && aligned16(mask);
    hipLaunchKernelGGL(detail_tail, dim3((unsigned)((size_t)B * H * gx)), dim3(256), 0, (hipStream_t)stream, logits, thold,
                       prob, mask, bits, W, gx, (W + 63) / 64, vec);
    return decnet_launch_status();
}

int decnet_detail_tail_backward(const float *logits, const float *g_prob, float *g_logits, size_t n, void *stream) {
    if (!logits || !g_prob || !g_logits) return DECNET_ERR_NULL_POINTER;
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    const int vec = aligned16(logits) && aligned16(g_prob) && aligned16(g_logits);
    hipLaunchKernelGGL(detail_tail_bwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, logits, g_prob, g_logits, n,
                       vec);
    return decnet_launch_status();
}

int decnet_sigmoid_blend_soft(const float *o, const float *a, const float *b, float *out, float *soft, size_t n,
                              void *stream) {
    if (!o || !a || !b || !out || !soft) return DECNET_ERR_NULL_POINTER;
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    const int vec = aligned16(o) && aligned16(a) && aligned16(b) && aligned16(out) && aligned16(soft);
    hipLaunchKernelGGL(sigmoid_blend_soft, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, o, a, b, out, soft, n,
                       vec);
    return decnet_launch_status();
}

int decnet_sigmoid_blend_soft_backward(const float *o, const float *a, const float *b, const float *gout,
                                       const float *gsoft, float *g_o, float *g_a, float *g_b, size_t n, void *stream) {
    if (!o || !a || !b || (!gout && !gsoft) || !g_o) return DECNET_ERR_NULL_POINTER;
    if (n < 1) return DECNET_ERR_BAD_SHAPE;
    if (n > FLAT_MAX) return DECNET_ERR_UNSUPPORTED;
    const int vec = aligned16(o) && aligned16(a) && aligned16(b) && aligned16(gout) && aligned16(gsoft) &&
                    aligned16(g_o) && aligned16(g_a) && aligned16(g_b);
    hipLaunchKernelGGL(sigmoid_blend_soft_bwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, o, a, b, gout, gsoft,
                       g_o, g_a, g_b, n, vec);
    return decnet_launch_status();
}

}  // extern "C"
