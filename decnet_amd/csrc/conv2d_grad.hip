// decnet_amd/csrc/conv2d_grad.hip -- the weight-gradient reduction of the few-channel stride-1 Conv2dUnit layers
// (csrc/conv2d_small.hip) with frozen BatchNorm: for y = act(conv(x, w) * scale + shift), gm = gy * [y > 0],
//     G[co][ci][ky][kx] = sum_{b,y,x} gm[b][co][y][x] * x[b][ci][y + (ky - k/2) d][x + (kx - k/2) d]     (zeros outside)
//     gsum[co]          = sum_{b,y,x} gm[b][co][y][x]
// dW = scale G, dscale = <w, G>, dshift = gsum are a few hundred floats of torch arithmetic (decnet_amd/conv2d_grad.py),
// and dx is the forward kernel itself on flipped weights, so this file is the only new arithmetic of the backward.
//
// G is the GEMM [Cout x pixels] . [pixels x (Cin k k + 1)] on v_mfma_f32_16x16x4_f32 (bit for bit an fp32 fma chain over
// the pixels); the extra column is all ones and yields gsum.  A workgroup owns RB = 8 rows x PX = 256 columns of one image;
// its four waves split the columns, so a wave owns a 64-pixel column slice of the RB rows and every 16 x 16 tile of G:
//   * per row, gm = gy * [y > 0] is formed once from bounds-checked 16-byte row loads, stored, and staged to LDS [co][px];
//   * per 16 columns of the GEMM, the tap planes x[ci][y + dy][x + dx] are staged to LDS [n][px] from the same kind of row
//     descriptors as the forward (a load that starts left of the row or runs past it reads zeros; the one quad that
//     straddles x = 0 patches up to three dwords), one batch of four loads per thread;
//   * the wave reads its operands as 16-byte LDS words (pitch 260: conflict-free) and runs the MFMAs.
// Partition and order are functions of the shape alone: workgroup v = (b, row block, column block), set 4 v + wave.
// Each set is written to the caller's workspace [set][Cout][Cin k k + 1]; the second launch is the float64 reduction of
// csrc/wgrad_common.h, which also states the sequence every weight-gradient entry follows (no mask launch here: gm is
// formed above).  The longest fp32 addition chain is one accumulator's MFMA K chain: 64 pixels x RB rows = 512 terms.
#include "wgrad_common.h"

typedef int i32x4_g __attribute__((ext_vector_type(4)));

namespace {

constexpr int PX = 256;              // columns of a workgroup (64 per wave)
constexpr int PITCH = PX + 4;        // floats: rows 16-byte aligned, 16 rows x 4 quads hit 64 different banks
constexpr int RB = 8;                // rows of a workgroup

template <int MT, int NT>
__global__ __launch_bounds__(256) void conv2d_wgrad_partial(Segs in, const float *__restrict__ gy,
                                                            const float *__restrict__ yo, float *__restrict__ gm,
                                                            float *__restrict__ ws, int Cout, int cin, int H, int W,
                                                            int k, int dil, int gx, int nrb) {
    __shared__ __attribute__((aligned(16))) float At[MT * 16 * PITCH];   // gm [co][px]; rows co >= Cout hold zeros
    __shared__ __attribute__((aligned(16))) float Bt[16 * PITCH];        // one 16-column tile of the taps [n][px]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int v = blockIdx.x, bx = v % gx, vr = v / gx, rb = vr % nrb, b = vr / nrb;
    const int y0 = rb * RB, rows = min(RB, H - y0);
    const int xq = bx * PX + 4 * lane;                                  // the quad this thread stages
    const int kk = k * k, N = cin * kk, h = k / 2;                      // GEMM column N: the ones of gsum
    const size_t plane = (size_t)H * W;
    const bool vec = (W & 3) == 0 && ((uintptr_t)gm & 15) == 0;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < rows; ++r) {
        const int yy = y0 + r;
        f32x4 a4[MT][4];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            // ---- stage tile j of the taps: wave w the GEMM columns 16 j + 4 w + i, lane q the quad q ----
            f32x4 t[4];
            int xs[4];
            __amdgpu_buffer_rsrc_t rr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                               // (all wave-uniform but xs)
                const int n = 16 * j + 4 * wave + i;
                const int ci = n < N ? n / kk : 0, tp = n < N ? n - ci * kk : 0, ky = tp / k, kx = tp - ky * k;
                int sg = 0, cs = ci;
                while (cs >= in.c[sg]) cs -= in.c[sg++];
                // a tap a whole image away never meets the image (and its offset would not fit the arithmetic below)
                const bool reach = (ky == h || dil < H) && (kx == h || dil < W);
                const int yi = reach ? yy + (ky - h) * dil : -1;
                const bool ok = n < N && (unsigned)yi < (unsigned)H;
                const float *base = in.p[sg] + ((size_t)b * in.c[sg] + cs) * plane + (ok ? (size_t)yi * W : 0);
                rr[i] = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, ok ? W * 4 : 0, 0x00020000);
                xs[i] = xq + (reach ? (kx - h) * dil : 0);               // < 0: a huge unsigned offset, reads zeros
                const i32x4_g u = __builtin_amdgcn_raw_buffer_load_b128(rr[i], (int)((unsigned)xs[i] * 4u), 0, 0);
                t[i] = f32x4{__int_as_float(u.x), __int_as_float(u.y), __int_as_float(u.z), __int_as_float(u.w)};
            }
            // ---- at the first tile of a row: gm of this row, wave w the channels w, w + 4, ... ----
            f32x4 g[MT * 4];
            if (j == 0) {
                f32x4 yv[MT * 4];
#pragma unroll
                for (int i = 0; i < MT * 4; ++i) {
                    const int co = wave + 4 * i;
                    const bool ok = co < Cout;
                    const size_t off = ((size_t)b * Cout + (ok ? co : 0)) * plane + (size_t)yy * W;
                    const __amdgpu_buffer_rsrc_t rg =
                        __builtin_amdgcn_make_buffer_rsrc((void *)(gy + off), 0, ok ? W * 4 : 0, 0x00020000);
                    const i32x4_g u = __builtin_amdgcn_raw_buffer_load_b128(rg, xq * 4, 0, 0);
                    g[i] = f32x4{__int_as_float(u.x), __int_as_float(u.y), __int_as_float(u.z), __int_as_float(u.w)};
                    yv[i] = f32x4{1.f, 1.f, 1.f, 1.f};
                    if (yo) {
                        const __amdgpu_buffer_rsrc_t ry =
                            __builtin_amdgcn_make_buffer_rsrc((void *)(yo + off), 0, ok ? W * 4 : 0, 0x00020000);
                        const i32x4_g uy = __builtin_amdgcn_raw_buffer_load_b128(ry, xq * 4, 0, 0);
                        yv[i] = f32x4{__int_as_float(uy.x), __int_as_float(uy.y), __int_as_float(uy.z), __int_as_float(uy.w)};
                    }
                }
#pragma unroll
                for (int i = 0; i < MT * 4; ++i) {
                    const int co = wave + 4 * i;
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[i][e] = yv[i][e] > 0.f ? g[i][e] : 0.f;
                    *reinterpret_cast<f32x4 *>(&At[co * PITCH + 4 * lane]) = g[i];
                    if (gm && co < Cout) {
                        float *gp = gm + ((size_t)b * Cout + co) * plane + (size_t)yy * W + xq;
                        if (vec) {
                            if (xq < W) *reinterpret_cast<f32x4 *>(gp) = g[i];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (xq + e < W) gp[e] = g[i][e];
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * j + 4 * wave + i;
                if (k > 1 && xs[i] < 0 && xs[i] > -4) {                 // the one quad of the row that straddles x = 0
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (xs[i] + e >= 0)
                            t[i][e] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr[i], (xs[i] + e) * 4, 0, 0));
                }
                if (n == N) t[i] = f32x4{1.f, 1.f, 1.f, 1.f};
                *reinterpret_cast<f32x4 *>(&Bt[(4 * wave + i) * PITCH + 4 * lane]) = t[i];
            }
            __syncthreads();
            // ---- the wave's 64 columns: four groups of 16 pixels, lane (m, kq) the pixels 16 g + 4 kq + e ----
            const int px = 64 * wave + 4 * kq;
            if (j == 0) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        a4[mt][gq] = *reinterpret_cast<const f32x4 *>(&At[(mt * 16 + m) * PITCH + px + 16 * gq]);
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x4 b4 = *reinterpret_cast<const f32x4 *>(&Bt[m * PITCH + px + 16 * gq]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[mt][gq][e], b4[e], acc[mt][j], 0, 0, 0);
            }
            __syncthreads();
        }
    }
    // D: register rr of lane (m, kq) is row 4 kq + rr (channel), column m (GEMM column)
    const int N1 = N + 1;
    float *wp = ws + ((size_t)blockIdx.x * 4 + wave) * ((size_t)Cout * N1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = mt * 16 + 4 * kq + e, n = 16 * j + m;
                if (co < Cout && n < N1) wp[(size_t)co * N1 + n] = acc[mt][j][e];
            }
}

// the shapes the kernels cover -> number of workgroups of the first launch (0: not covered)
long wgrad_groups(int B, int Cin, int Cout, int H, int W, int k) {
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return 0;
    if ((k != 1 && k != 3) || Cout > 24 || Cin > 24 || H > 65535 || B > 65535 || W > (1 << 28)) return 0;
    if ((double)B * (Cin > Cout ? Cin : Cout) * H * W >= 9.0e18) return 0;
    const double T = (double)B * ceil_div(H, RB) * ceil_div(W, PX);
    if (T * 4.0 >= 2.0e9) return 0;                                   // (the sets are numbered in an int)
    return (long)T;
}

}  // namespace

extern "C" {

size_t decnet_conv2d_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W, int k) {
    const long T = wgrad_groups(B, Cin, Cout, H, W, k);
    if (T == 0) return 0;
    const size_t n = (size_t)T * 4 * Cout * ((size_t)Cin * k * k + 1);
    return (n + 3) & ~(size_t)3;
}

int decnet_conv2d_wgrad(const float *const *xs, const int *cins, int nseg, const float *gy, const float *y, float *gm,
                        float *G, float *gsum, float *workspace, size_t workspace_floats, int B, int Cout, int H,
                        int W, int k, int dilation, void *stream) {
    Segs in{};
    int cin, rc;
    if ((rc = wgrad_stride1_args(xs, cins, nseg, gy, y, gm, G, gsum, workspace, B, Cout, H, W, k, dilation, 24, &in, &cin)))
        return rc;
    const long T = wgrad_groups(B, cin, Cout, H, W, k);
    if (T == 0) return DECNET_ERR_UNSUPPORTED;
    if ((rc = wgrad_workspace(workspace, workspace_floats, decnet_conv2d_wgrad_workspace_floats(B, cin, Cout, H, W, k))))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const int N1 = cin * k * k + 1, tiles = ceil_div(N1, 16), gx = ceil_div(W, PX), nrb = ceil_div(H, RB);
    const dim3 grid((unsigned)T);
#define GO(MT_, NT_)                                                                                                  \
    hipLaunchKernelGGL((conv2d_wgrad_partial<MT_, NT_>), grid, dim3(256), 0, s, in, gy, y, gm, workspace, Cout, cin, H, \
                       W, k, dilation, gx, nrb)
#define GON(MT_)                                                                                                      \
    do {                                                                                                              \
        if (tiles <= 1) GO(MT_, 1); else if (tiles <= 2) GO(MT_, 2); else if (tiles <= 5) GO(MT_, 5);                 \
        else if (tiles <= 8) GO(MT_, 8); else if (tiles <= 10) GO(MT_, 10); else GO(MT_, 14);                         \
    } while (0)
    if (Cout <= 16) GON(1); else GON(2);
#undef GON
#undef GO
    if ((rc = decnet_launch_status())) return rc;
    return launch_wgrad_reduce(workspace, G, gsum, T * 4, Cout, N1, s);
}

}  // extern "C"
