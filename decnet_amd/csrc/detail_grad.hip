// decnet_amd/csrc/detail_grad.hip -- the elementwise passes of a training forward under hip_grad(), each with its
// backward (decnet_amd/tail_grad.py): SoftAttention's sigmoid + blend, with or without the soft mask beside it, and the
// detail maps of GenerateSparseMask (the squared difference and the sigmoid / threshold / bit-plane tail; the units in
// between have their own routes).  Every kernel is fp32 with contraction off: no LDS, no atomics, no allocation, no
// synchronisation, the same bits on every run and under graph replay.  Planes are accepted at any float alignment; the
// access, the sigmoid, the blend and the bit plane are those of csrc/pointwise.h.
#include "pointwise.h"

namespace {

// ---- SoftAttention's tail: s = sigmoid(o), out = a (1 - s) + s b ---------------------------------------------------------
// The plain forward keeps its own spelling of the quad access: through store_quads the compiler splits its one 16-byte store
// into 12 + 4 bytes, and the pass measured 9 % slower (profiles/README.md).
__global__ __launch_bounds__(256) void sigmoid_blend(const float *__restrict__ o, const float *__restrict__ a,
                                                     const float *__restrict__ b, float *__restrict__ out, size_t n,
                                                     int vec) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool full = vec && i0 + 3 < n;
    float vo[4], va[4], vb[4], r[4];
    if (full) {
        const float4 to = *reinterpret_cast<const float4 *>(o + i0), ta = *reinterpret_cast<const float4 *>(a + i0);
        const float4 tb = *reinterpret_cast<const float4 *>(b + i0);
        vo[0] = to.x; vo[1] = to.y; vo[2] = to.z; vo[3] = to.w;
        va[0] = ta.x; va[1] = ta.y; va[2] = ta.z; va[3] = ta.w;
        vb[0] = tb.x; vb[1] = tb.y; vb[2] = tb.z; vb[3] = tb.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t i = i0 + e < n ? i0 + e : i0;
            vo[e] = o[i]; va[e] = a[i]; vb[e] = b[i];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = blend_f(sigmoid_f(vo[e]), va[e], vb[e]);
    if (full) {
        *reinterpret_cast<float4 *>(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) out[i0 + e] = r[e];
    }
}

// The same with the soft mask kept: soft = s.
__global__ __launch_bounds__(256) void sigmoid_blend_soft(const float *__restrict__ o, const float *__restrict__ a,
                                                          const float *__restrict__ b, float *__restrict__ out,
                                                          float *__restrict__ soft, size_t n, int vec) {
    size_t i0;
    bool full;
    if (!flat_quad(n, vec, i0, full)) return;
    float v[3][4], r[2][4];                                                    // o, a, b -> out, soft
    load_quads(i0, n, full, v, o, a, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[1][e] = sigmoid_f(v[0][e]);
        r[0][e] = blend_f(r[1][e], v[1][e], v[2][e]);
    }
    store_quads(i0, n, full, r, out, soft);
}

// g_o = (gout (b - a) + gsoft) (s (1 - s)), g_a = gout (1 - s), g_b = gout s, with s recomputed from o as the forward
// computes it (a saturated sigmoid gives s (1 - s) = 0 exactly: g_o = 0, never NaN).  GOUT, GSOFT: which gradients came
// (the host picks; a plane that did not come is not read, nor are a and b without gout): without gsoft its term is not
// added, without gout g_o = gsoft (s (1 - s)) and g_a, g_b are zeros.  g_a, g_b: may be NULL.
template <bool GOUT, bool GSOFT>
__global__ __launch_bounds__(256) void blend_bwd(const float *__restrict__ o, const float *__restrict__ a,
                                                 const float *__restrict__ b, const float *__restrict__ gout,
                                                 const float *__restrict__ gsoft, float *__restrict__ g_o,
                                                 float *__restrict__ g_a, float *__restrict__ g_b, size_t n, int vec) {
#pragma clang fp contract(off)
    size_t i0;
    bool full;
    if (!flat_quad(n, vec, i0, full)) return;
    float v[5][4], r[3][4];                                                    // o, then a, b, gout (GOUT), then gsoft
    if constexpr (GOUT && GSOFT) load_quads(i0, n, full, v, o, a, b, gout, gsoft);
    else if constexpr (GOUT) load_quads(i0, n, full, v, o, a, b, gout);
    else load_quads(i0, n, full, v, o, gsoft);
    const float *vs = v[GOUT ? 4 : 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float sft = sigmoid_f(v[0][e]);
        const float om = 1.f - sft;
        if constexpr (GOUT) {
            float t = v[3][e] * (v[2][e] - v[1][e]);
            if constexpr (GSOFT) t = t + vs[e];
            r[0][e] = t * (sft * om);
            r[1][e] = v[3][e] * om;
            r[2][e] = v[3][e] * sft;
        } else {
            r[0][e] = vs[e] * (sft * om);
            r[1][e] = 0.f;
            r[2][e] = 0.f;
        }
    }
    store_quads<6>(i0, n, full, r, g_o, g_a, g_b);
}

// ---- res_info = (cur - pre)^2: d = a - b, out = d d, both rounded (torch's (a - b) * (a - b)) ------------------------------
__global__ __launch_bounds__(256) void sqdiff(const float *__restrict__ a, const float *__restrict__ b,
                                              float *__restrict__ out, size_t n, int vec) {
#pragma clang fp contract(off)
    size_t i0;
    bool full;
    if (!flat_quad(n, vec, i0, full)) return;
    float v[2][4], r[4];
    load_quads(i0, n, full, v, a, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = v[0][e] - v[1][e];
        r[e] = d * d;
    }
    store_quads(i0, n, full, &r, out);
}

// t = gout d, g_a = t + t, g_b = -g_a: autograd through d * d (gout d twice, summed) and through a - b.  g_a, g_b: one
// may be NULL.
__global__ __launch_bounds__(256) void sqdiff_bwd(const float *__restrict__ a, const float *__restrict__ b,
                                                  const float *__restrict__ gout, float *__restrict__ g_a,
                                                  float *__restrict__ g_b, size_t n, int vec) {
#pragma clang fp contract(off)
    size_t i0;
    bool full;
    if (!flat_quad(n, vec, i0, full)) return;
    float v[3][4], r[2][4];
    load_quads(i0, n, full, v, a, b, gout);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = v[0][e] - v[1][e];
        const float t = v[2][e] * d;
        r[0][e] = t + t;
        r[1][e] = -r[0][e];
    }
    store_quads<3>(i0, n, full, r, g_a, g_b);
}

// ---- the tail of the detail map: prob = sigmoid(z), mask = prob > thold, the mask bit-packed -----------------------------------
// One row segment of 1024 pixels per workgroup, four consecutive pixels per thread: the layout of detail_mask
// (csrc/maskgen.hip), whose mask and bit plane this reproduces from its logits.  Every thread of a workgroup that has a
// pixel in the row stays for the ballots: a lane past W contributes zero bits.  prob, mask, bits: each may be NULL.
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
        load_quads(0, nrow, full, &z, logits + pix);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s[e] = sigmoid_f(z[e]);
        on[e] = (size_t)e < nrow && s[e] > thold;
        m[e] = on[e] ? 1.f : 0.f;
    }
    if (nrow) {                                                                // (rows, not flat: a plane at a time)
        if (prob) store_quads(0, nrow, full, &s, prob + pix);
        if (mask) store_quads(0, nrow, full, &m, mask + pix);
    }
    if (bits) {
        // pack_mask_bits (csrc/pointwise.h) written out: through the call the kernel is the parent's but for the operand
        // order of two instructions, and it measured 0.4 - 1.4 % slower in two sessions (profiles/README.md)
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
    size_t i0;
    bool full;
    if (!flat_quad(n, vec, i0, full)) return;
    float v[2][4], r[4];
    load_quads(i0, n, full, v, logits, g_prob);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s = sigmoid_f(v[0][e]);
        r[e] = v[1][e] * (s * (1.f - s));
    }
    if (full) {                          // (written out, as in sigmoid_blend: store_quads' 16 bytes leave as 12 + 4 here too)
        *reinterpret_cast<float4 *>(g_logits + i0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) g_logits[i0 + e] = r[e];
    }
}

}  // namespace

extern "C" {

int decnet_sigmoid_blend(const float *o, const float *a, const float *b, float *out, size_t n, void *stream) {
    if (!o || !a || !b || !out) return DECNET_ERR_NULL_POINTER;
    return flat_pass(sigmoid_blend, n, stream, o, a, b, out, n, aligned16(o, a, b, out));
}

int decnet_sigmoid_blend_soft(const float *o, const float *a, const float *b, float *out, float *soft, size_t n,
                              void *stream) {
    if (!o || !a || !b || !out || !soft) return DECNET_ERR_NULL_POINTER;
    return flat_pass(sigmoid_blend_soft, n, stream, o, a, b, out, soft, n, aligned16(o, a, b, out, soft));
}

int decnet_sigmoid_blend_soft_backward(const float *o, const float *a, const float *b, const float *gout,
                                       const float *gsoft, float *g_o, float *g_a, float *g_b, size_t n, void *stream) {
    if (!o || !a || !b || (!gout && !gsoft) || !g_o) return DECNET_ERR_NULL_POINTER;
    const auto kernel = !gsoft ? blend_bwd<true, false> : gout ? blend_bwd<true, true> : blend_bwd<false, true>;
    return flat_pass(kernel, n, stream, o, a, b, gout, gsoft, g_o, g_a, g_b, n,
                     aligned16(o, a, b, gout, gsoft, g_o, g_a, g_b));
}

int decnet_sigmoid_blend_backward(const float *o, const float *a, const float *b, const float *gout, float *g_o,
                                  float *g_a, float *g_b, size_t n, void *stream) {
    if (!gout) return DECNET_ERR_NULL_POINTER;
    return decnet_sigmoid_blend_soft_backward(o, a, b, gout, nullptr, g_o, g_a, g_b, n, stream);
}

int decnet_sqdiff(const float *a, const float *b, float *out, size_t n, void *stream) {
    if (!a || !b || !out) return DECNET_ERR_NULL_POINTER;
    return flat_pass(sqdiff, n, stream, a, b, out, n, aligned16(a, b, out));
}

int decnet_sqdiff_backward(const float *a, const float *b, const float *gout, float *g_a, float *g_b, size_t n,
                           void *stream) {
    if (!a || !b || !gout || (!g_a && !g_b)) return DECNET_ERR_NULL_POINTER;
    return flat_pass(sqdiff_bwd, n, stream, a, b, gout, g_a, g_b, n, aligned16(a, b, gout, g_a, g_b));
}

int decnet_detail_tail(const float *logits, float thold, float *prob, float *mask, unsigned long long *bits, int B, int H,
                       int W, void *stream) {
    if (!logits || (!prob && !mask && !bits)) return DECNET_ERR_NULL_POINTER;
    if (int rc = row_refusal(B, H, W)) return rc;
    const int gx = ceil_div(W, 1024);
    // rows start at multiples of W floats: 16-byte accesses need W % 4 == 0 as well
    const int vec = (W & 3) == 0 && aligned16(logits, prob, mask);
    hipLaunchKernelGGL(detail_tail, dim3((unsigned)((size_t)B * H * gx)), dim3(256), 0, (hipStream_t)stream, logits, thold,
                       prob, mask, bits, W, gx, (W + 63) / 64, vec);
    return decnet_launch_status();
}

int decnet_detail_tail_backward(const float *logits, const float *g_prob, float *g_logits, size_t n, void *stream) {
    if (!logits || !g_prob || !g_logits) return DECNET_ERR_NULL_POINTER;
    return flat_pass(detail_tail_bwd, n, stream, logits, g_prob, g_logits, n, aligned16(logits, g_prob, g_logits));
}

}  // extern "C"
