// decnet_amd/csrc/conv2d_mfma_common.h -- what csrc/conv2d_mfma.hip (one accumulator set) and csrc/conv2d_mfma_acc2.hip
// (two, DECNET_CONV2D_ACC=2) share: the operand types, the round-to-nearest bf16 split, the epilogue, the host path of
// the pack and run launches, the refusals of the run entries, and the one declaration of every function that crosses
// the two files.  What differs stays in the files: the MFMA schedules, the pack kernels and packed formats, the tile
// choice.  Internal: no part of include/decnet_hip.h.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// the parts [B, c_i, H, W] of a channel concatenation that is never materialised.  The one name of this header outside
// the unnamed namespace, hence the prefix: conv2d_mfma_run_acc2 takes it across the files
struct Conv2dMfmaSegs {
    const float *p[6];
    int c[6];
    int n;
};

// ---- conv2d_mfma_acc2.hip behind the entries of conv2d_mfma.hip, which has made their refusals --------------------------
size_t conv2d_mfma_packed_bytes_acc2(int Cin, int Cout, int k);
int conv2d_mfma_pack_acc2(const float *w, void *w_packed, int Cin, int Cout, int k, int tr, void *stream);
int conv2d_mfma_run_acc2(const Conv2dMfmaSegs &in, long Cin, const void *w_packed, const float *scale, const float *shift,
                         float *y, int B, int Cout, int H, int W, int k, int dilation, int relu, int shuf, void *stream);

namespace {

using Segs = Conv2dMfmaSegs;
constexpr int MAXSEG = sizeof(Segs::c) / sizeof(int);
constexpr int THREADS = 256;

__device__ __forceinline__ void split3(float x, int &h, int &m, int &l) {
    // round-to-nearest-even terms (v_cvt_pk_bf16_f32): |x - h| <= 2^-9 |x|, |x - h - m| <= 2^-18 |x|, and the residual
    // that l leaves is <= 2^-27 |x| -- truncated terms (round 2) left 2^-24 and, worse, always of the sign of x, so the
    // dropped m.l / l.m products of a K-long sum added up instead of averaging out (tests/test_inputdata_gpu.py measures
    // the network's distance to its float64 run: 1.35 x the reference's float32 distance before, 1.0 x after)
    h = __float_as_int((float)(__bf16)x);
    const float r1 = x - __int_as_float(h);
    m = __float_as_int((float)(__bf16)r1);
    l = __float_as_int((float)(__bf16)(r1 - __int_as_float(m)));
}

// eight values -> the three packed operand registers sets {hi, mid, lo}[4] (pairs (x[2e], x[2e+1]) share a register):
// the same terms as split3, two per v_cvt_pk_bf16_f32 -- the packed pair IS the operand register, and a term's float
// value is a shift / a mask of it (no v_perm_b32, half the conversions, packed subtractions)
__device__ __forceinline__ int pack_bf16(float a, float b) {
    return __builtin_bit_cast(int, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ void split3x8(const float (&x)[8], i32x4 &th, i32x4 &tm, i32x4 &tl) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = x[2 * e], x1 = x[2 * e + 1];
        const int h = pack_bf16(x0, x1);
        const float r0 = x0 - __int_as_float(h << 16), r1 = x1 - __int_as_float(h & 0xffff0000);
        const int m = pack_bf16(r0, r1);
        th[e] = h;
        tm[e] = m;
        tl[e] = pack_bf16(r0 - __int_as_float(m << 16), r1 - __int_as_float(m & 0xffff0000));
    }
}

// Epilogue of every kernel: the lane holds output channel n = tile * 16 + r of the pixels x0 + 4 q .. + 3 of TM rows.
// shuf = 0: y [B,Cout,H,W] = act(acc * scale[n] + shift[n]).  shuf = C (transposed convolution k = 3, stride 3, as a
// 1 x 1 convolution to 9 C channels n = 9 co + 3 ky + kx): y [B,C,3H,3W] at (3 row + ky, 3 x + kx), scale / shift per co.
template <int TM, int TN>
__device__ __forceinline__ void conv2d_mfma_store(const f32x4 (&acc)[TM][TN], const float *__restrict__ scale,
                                                  const float *__restrict__ shift, float *__restrict__ y, int b, int Cout,
                                                  int H, int W, int relu, int nt0, int r, int q, int x0, int row0,
                                                  int shuf) {
    const size_t HW = (size_t)H * W;
    const int xq = x0 + 4 * q;
    const bool vec = (W & 3) == 0 && ((uintptr_t)y & 15) == 0 && xq + 3 < W;   // y: any dense fp32 pointer
#pragma unroll
    for (int nt = 0; nt < TN; ++nt) {
        const int n = (nt0 + nt) * 16 + r;
        if (n >= Cout) continue;
        if (shuf) {
            const int co = n / 9, kk = n - 9 * co, ky = kk / 3, kx = kk - 3 * ky;
            const float sc = scale[co], sh = shift[co];
            float *yp = y + ((size_t)b * shuf + co) * 9 * HW;
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const int row = row0 + mt;
                if (row >= H) break;
                float *dst = yp + ((size_t)(3 * row + ky) * 3 * W) + kx;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = fmaf(acc[mt][nt][i], sc, sh);
                    if (relu) v = fmaxf(v, 0.f);
                    if (xq + i < W) dst[3 * (xq + i)] = v;
                }
            }
            continue;
        }
        const float sc = scale[n], sh = shift[n];
        float *yp = y + ((size_t)b * Cout + n) * HW;
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int row = row0 + mt;
            if (row >= H) break;
            f32x4 v = acc[mt][nt];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = fmaf(v[i], sc, sh);
                if (relu) v[i] = fmaxf(v[i], 0.f);
            }
            float *dst = yp + (size_t)row * W + xq;
            if (vec) {
                *reinterpret_cast<f32x4 *>(dst) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (xq + i < W) dst[i] = v[i];
            }
        }
    }
}

// pixels of the halo tile of a TM variant
constexpr int tile_pixels(int tm, int pad) { return (16 + 2 * pad) * (4 * tm + 2 * pad); }

// ---- host ----------------------------------------------------------------------------------------------------------------
// The refusals of decnet_conv2d_mfma_cat_bn_act behind its MISALIGNED check, in their order; then *in and the channels
// together.
inline int conv2d_mfma_cat_args(const float *const *xs, const int *cins, int nseg, const void *w_packed,
                                const float *scale, const float *shift, const float *y, int B, int Cout, int H, int W,
                                int k, int dilation, Segs *in, long *Cin) {
    if (!xs || !cins || !w_packed || !scale || !shift || !y) return DECNET_ERR_NULL_POINTER;
    if (nseg < 1 || nseg > MAXSEG || (k != 1 && k != 3)) return DECNET_ERR_UNSUPPORTED;
    if (B < 1 || Cout < 1 || H < 1 || W < 1 || dilation < 1) return DECNET_ERR_BAD_SHAPE;
    *in = Segs{};
    *Cin = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!xs[i]) return DECNET_ERR_NULL_POINTER;
        if (cins[i] < 1) return DECNET_ERR_BAD_SHAPE;
        in->p[i] = xs[i];
        in->c[i] = cins[i];
        *Cin += cins[i];
    }
    in->n = nseg;
    return DECNET_OK;
}

// ... and of decnet_deconv2d_mfma_k3s3_bn_act (one part)
inline int conv2d_mfma_deconv_args(const float *x, const void *w_packed, const float *scale, const float *shift,
                                   const float *y, int B, int Cin, int Cout, int H, int W, Segs *in) {
    if (!x || !w_packed || !scale || !shift || !y) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    if (Cout > 7281) return DECNET_ERR_UNSUPPORTED;
    *in = Segs{};
    in->p[0] = x;
    in->c[0] = Cin;
    in->n = 1;
    return DECNET_OK;
}

// One weight packing: `per` blocks of NT x 64 operand registers per (chunk, tap), written by `kernel` (the file's
// conv2d_mfma_pack; extra: its arguments behind tr), and the prefetch padding behind them zeroed.  bytes: the file's
// size query, 0 for a layer it does not take.
template <typename K, typename... Extra>
inline int conv2d_mfma_pack_launch(K kernel, const float *w, void *w_packed, size_t bytes, int Cin, int Cout, int KT,
                                   int NT, int per, int tr, void *stream, Extra... extra) {
    if (!w || !w_packed) return DECNET_ERR_NULL_POINTER;
    if (!bytes) return DECNET_ERR_UNSUPPORTED;
    const long total = (long)ceil_div(Cin, 16) * KT * per * NT * 64;
    hipError_t e = hipMemsetAsync((char *)w_packed + (size_t)total * 16, 0, bytes - (size_t)total * 16,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (i32x4 *)w_packed, Cin, Cout, KT, NT, total, tr, extra...);
    return decnet_launch_status();
}

// One run launch: a workgroup of `threads` per 4 TM x 16 pixel tile, ny of them over the channel tiles; the file's
// launch<> has checked that lds bytes (and its staging) hold the halo tile.
template <typename K>
inline int conv2d_mfma_launch(K kernel, int threads, size_t lds, int TM, int ny, const Segs &in, const i32x4 *wp,
                              const float *scale, const float *shift, float *y, int B, int Cout, int H, int W, int KT,
                              int dil, int relu, int nchunk, int NT, int shuf, hipStream_t stream) {
    int cin = 0;
    for (int i = 0; i < in.n; ++i) cin += in.c[i];
    const int tail8 = cin - 16 * (nchunk - 1) <= 8;              // the last chunk's channels 8-15 are padding
    const int tiles_x = ceil_div(W, 16), tiles_y = ceil_div(H, 4 * TM);
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)ny, (unsigned)B);
    return decnet_launch(kernel, grid, dim3(threads), lds, stream, in, wp, scale, shift, y, Cout, H, W, KT, dil, relu,
                         nchunk, NT, tiles_x, tail8, shuf);
}

}  // namespace
