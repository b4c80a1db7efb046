// decnet_amd/csrc/imageio.hip -- the image boundary of the network on the device: uint8 views in, uint16 disparity and
// the evaluation sums out (demo.py:75-89, 191-197; modules/loss.py:427-437).
//
//   preprocess_u8        [B,h,w,3] uint8 -> [B,3,H,W] fp32: zero pad on the top / left, /255, normalise -- as ONE table
//                        lookup per element (table[v][c], built on the host with the loader's own numpy expressions, so
//                        the result is bit-equal to the host path whatever a compiler makes of a division);
//   disparity_to_u16     [B,H,W] fp32 -> [B,h,w] uint16 of the bottom-right window: x256, clamp, truncate;
//   disparity_metrics    per row of the window: valid count, sum |pred - gt|, count of "good" pixels.
//
// All three are row-structured like spamat_wide.hip's element-wise kernels: a wave owns a row (no division per element),
// the destination row is written in 16-byte units on its 16-byte-aligned middle with a scalar head and tail (neither 3 w
// bytes nor W floats nor w uint16 are multiples of 16 bytes in general), and the result of an element does not depend on
// the launch shape.  No entry allocates, synchronises or asks about the stream: all of them run under stream capture.
//
// Where the table lives: the lookup index is data (a pixel value), so the 64 lanes of a load hit 64 unrelated entries.
// From global memory that is a gather of 64 separate 4-byte requests per instruction; from LDS it is one ds_read_b32 whose
// cost is its bank conflicts only.  The 3 KB table is therefore copied into LDS once per workgroup, as three planes
// [c][256] so that one instruction (one channel) spreads over 256 consecutive dwords.
//
// This file is built WITHOUT -fno-honor-nans: a NaN prediction has to give a NaN error sum and count as "not good".
#include "common.h"

namespace {

constexpr int IO_THREADS = 256;
constexpr int IO_WAVES = IO_THREADS / DECNET_WAVE;       // rows a workgroup works on at a time (one per wave)

typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));
typedef unsigned u4a __attribute__((ext_vector_type(4), aligned(16)));

inline unsigned io_grid(size_t rows) {
    const size_t b = (rows + IO_WAVES - 1) / IO_WAVES;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

// elements of `bytes`-sized type before the first 16-byte boundary of p (all n of them when p is not even element-aligned:
// the row is then written element by element)
__device__ __forceinline__ int head_elems(const void *p, int bytes, int n) {
    const uintptr_t a = (uintptr_t)p;
    if (a & (uintptr_t)(bytes - 1)) return n;
    const int head = (int)(((16u - (unsigned)(a & 15u)) & 15u) / (unsigned)bytes);
    return head < n ? head : n;
}

// ---- uint8 HWC -> normalised, padded fp32 CHW -----------------------------------------------------------------------
// Row r = (b, y) of the padded image; the wave writes the three channel rows out[b][c][y][0..W).  px: the w pixels of the
// image row behind it (3 bytes each), nullptr for a row of the top padding.
__device__ __forceinline__ float pre_elem(const float *lut, const unsigned char *px, int x, int pw, int c) {
    return lut[(px && x >= pw) ? px[3 * (x - pw) + c] : 0];
}

__global__ __launch_bounds__(IO_THREADS) void preprocess_u8(const unsigned char *__restrict__ img,
                                                            const float *__restrict__ table, float *__restrict__ out,
                                                            size_t rows, int h, int w, int H, int W) {
    __shared__ float lut[3][256];
    for (int i = threadIdx.x; i < 768; i += IO_THREADS) lut[i % 3][i / 3] = table[i];
    __syncthreads();
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    const int ph = H - h, pw = W - w;
    const size_t plane = (size_t)H * W;
    // b and y advance with the row index: one division per row start, none per element
    for (size_t r = (size_t)blockIdx.x * IO_WAVES + wave; r < rows; r += (size_t)gridDim.x * IO_WAVES) {
        const size_t b = r / (size_t)H;
        const int y = (int)(r - b * (size_t)H);
        const unsigned char *px = y >= ph ? img + ((b * h + (size_t)(y - ph)) * w) * 3 : nullptr;
        for (int c = 0; c < 3; ++c) {
            float *d = out + (b * 3 + c) * plane + (size_t)y * W;
            const float *t = lut[c];
            const int head = head_elems(d, 4, W), nv = (W - head) >> 2;
            for (int x = lane; x < head; x += DECNET_WAVE) d[x] = pre_elem(t, px, x, pw, c);
            for (int v = lane; v < nv; v += DECNET_WAVE) {
                const int x = head + 4 * v;
                f4a o;
                if (px && x >= pw) {                                          // four whole pixels of the image
                    const unsigned char *p = px + 3 * (x - pw) + c;
                    o = {t[p[0]], t[p[3]], t[p[6]], t[p[9]]};
                } else {                                                      // padding, or the vector that straddles x = pw
                    o = {pre_elem(t, px, x, pw, c), pre_elem(t, px, x + 1, pw, c), pre_elem(t, px, x + 2, pw, c),
                         pre_elem(t, px, x + 3, pw, c)};
                }
                *reinterpret_cast<f4a *>(d + x) = o;
            }
            for (int x = head + 4 * nv + lane; x < W; x += DECNET_WAVE) d[x] = pre_elem(t, px, x, pw, c);
        }
    }
}

// ---- fp32 disparity -> uint16 window --------------------------------------------------------------------------------
// demo.py:191-197: (pred * 256).clamp(0, 65535) as uint16 (truncated toward zero).  fmaxf(NaN, 0) = 0.
__device__ __forceinline__ unsigned u16_of(float p) {
    return (unsigned)fminf(fmaxf(p * 256.f, 0.f), 65535.f);
}

__global__ __launch_bounds__(IO_THREADS) void disparity_to_u16(const float *__restrict__ pred,
                                                               unsigned short *__restrict__ out, size_t rows, int H, int W,
                                                               int h, int w) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t r = (size_t)blockIdx.x * IO_WAVES + wave; r < rows; r += (size_t)gridDim.x * IO_WAVES) {
        const size_t b = r / (size_t)h;
        const int y = (int)(r - b * (size_t)h);
        const float *s = pred + (b * H + (size_t)(H - h + y)) * W + (W - w);
        unsigned short *d = out + r * (size_t)w;
        const int head = head_elems(d, 2, w), nv = (w - head) >> 3;
        for (int x = lane; x < head; x += DECNET_WAVE) d[x] = (unsigned short)u16_of(s[x]);
        for (int v = lane; v < nv; v += DECNET_WAVE) {
            const float *p = s + head + 8 * v;
            u4a o = {u16_of(p[0]) | (u16_of(p[1]) << 16), u16_of(p[2]) | (u16_of(p[3]) << 16),
                     u16_of(p[4]) | (u16_of(p[5]) << 16), u16_of(p[6]) | (u16_of(p[7]) << 16)};
            *reinterpret_cast<u4a *>(d + head + 8 * v) = o;
        }
        for (int x = head + 8 * nv + lane; x < w; x += DECNET_WAVE) d[x] = (unsigned short)u16_of(s[x]);
    }
}

// ---- evaluation sums per row ----------------------------------------------------------------------------------------
// modules/loss.py:427-437 over one row of the window: valid = 0 < gt < max_disp; err = |pred - gt|;
// good = err < 3 || err < 0.05f * gt.  Lane l sums the pixels l, l + 64, ... in order, then the 64 lane sums are added
// in a fixed butterfly: the same bits for every launch shape, no atomics.  The counts are integers until the final store.
__global__ __launch_bounds__(IO_THREADS) void disparity_metrics(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                float max_disp, float *__restrict__ partials, size_t rows,
                                                                int H, int W, int h, int w) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    for (size_t r = (size_t)blockIdx.x * IO_WAVES + wave; r < rows; r += (size_t)gridDim.x * IO_WAVES) {
        const size_t b = r / (size_t)h;
        const int y = (int)(r - b * (size_t)h);
        const float *p = pred + (b * H + (size_t)(H - h + y)) * W + (W - w);
        const float *g = gt + r * (size_t)w;
        int n = 0, good = 0;
        float sum = 0.f;
        for (int x = lane; x < w; x += DECNET_WAVE) {
            const float gv = g[x];
            if (gv > 0.f && gv < max_disp) {
                const float err = fabsf(p[x] - gv);
                ++n;
                sum += err;
                good += (err < 3.f || err < 0.05f * gv) ? 1 : 0;
            }
        }
        for (int o = DECNET_WAVE / 2; o > 0; o >>= 1) {
            n += __shfl_xor(n, o);
            good += __shfl_xor(good, o);
            sum += __shfl_xor(sum, o);
        }
        if (lane == 0) {
            float *q = partials + 3 * r;
            q[0] = (float)n;
            q[1] = sum;
            q[2] = (float)good;
        }
    }
}

// shared argument check: positive sizes, the window inside the plane, every index space below 2^31
inline int window_args(int B, int h, int w, int H, int W, double per_pixel) {
    if (B < 1 || h < 1 || w < 1 || H < h || W < w) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * H * W * per_pixel >= 2147483648.0) return DECNET_ERR_BAD_SHAPE;
    return DECNET_OK;
}

}  // namespace

int decnet_preprocess_u8(const unsigned char *img, const float *table, float *out, int B, int h, int w, int H, int W,
                         void *stream) {
    if (!img || !table || !out) return DECNET_ERR_NULL_POINTER;
    if (const int rc = window_args(B, h, w, H, W, 3.0)) return rc;
    const size_t rows = (size_t)B * H;
    hipLaunchKernelGGL(preprocess_u8, dim3(io_grid(rows)), dim3(IO_THREADS), 0, (hipStream_t)stream, img, table, out, rows,
                       h, w, H, W);
    return decnet_launch_status();
}

int decnet_disparity_to_u16(const float *pred, unsigned short *out, int B, int H, int W, int h, int w, void *stream) {
    if (!pred || !out) return DECNET_ERR_NULL_POINTER;
    if (const int rc = window_args(B, h, w, H, W, 1.0)) return rc;
    const size_t rows = (size_t)B * h;
    hipLaunchKernelGGL(disparity_to_u16, dim3(io_grid(rows)), dim3(IO_THREADS), 0, (hipStream_t)stream, pred, out, rows, H,
                       W, h, w);
    return decnet_launch_status();
}

int decnet_disparity_metrics(const float *pred, const float *gt, float max_disp, float *partials, int B, int H, int W,
                             int h, int w, void *stream) {
    if (!pred || !gt || !partials) return DECNET_ERR_NULL_POINTER;
    if (const int rc = window_args(B, h, w, H, W, 1.0)) return rc;
    const size_t rows = (size_t)B * h;
    hipLaunchKernelGGL(disparity_metrics, dim3(io_grid(rows)), dim3(IO_THREADS), 0, (hipStream_t)stream, pred, gt, max_disp,
                       partials, rows, H, W, h, w);
    return decnet_launch_status();
}
