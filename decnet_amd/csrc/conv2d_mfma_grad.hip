// decnet_amd/csrc/conv2d_mfma_grad.hip -- the weight-gradient reduction of the many-channel stride-1 Conv2dUnit layers
// (csrc/conv2d_mfma.hip, Unit._route "mfma") and of the stride-3 layers (below) with frozen BatchNorm.  The meaning is that of csrc/conv2d_grad.hip:
//     gm                = gy * [y > 0]                                                         (gy itself without y)
//     G[co][ci][ky][kx] = sum_{b,y,x} gm[b][co][y][x] * x[b][ci][y + (ky - k/2) d][x + (kx - k/2) d]     (zeros outside)
//     gsum[co]          = sum_{b,y,x} gm[b][co][y][x]
// for Cout, Cin <= 224, where G (up to 224 x 2017 with the column of ones that yields gsum) no longer fits one wave.
//
// The sequence is that of csrc/wgrad_common.h (mask, GEMM into partial sets, float64 reduction); this file holds its step
//   2. conv2d_mfma_wgrad_partial runs the GEMM [Cout x pixels] . [pixels x (Cin k k + 1)] on v_mfma_f32_16x16x4_f32 (bit
//      for bit an fp32 fma chain over the pixels).  A 256-thread workgroup owns every row of G (MT tiles of 16 channels),
//      one block of 64 NT GEMM columns (wave w the tiles w NT .. w NT + NT - 1: 4 MT NT accumulator registers) and one
//      slice of `sl` consecutive chunks of one image; a chunk is 64 consecutive pixels of the plane, rows run on.  Per
//      chunk the workgroup stages gm as [co][px] and the tap planes as [n][px] in LDS (pitch 68: the 16-byte operand
//      reads of 16 lanes hit 64 different banks), wave w the rows w, w + 4, ..., lane = pixel: every load is one coalesced dword per lane, issued
//      unconditionally from an address clamped into the plane and selected afterwards, at any float alignment.  The loads
//      of chunk c + 1 are in flight while the MFMAs of chunk c run.  The tap rows' plane pointers and offsets sit in the
//      registers of the wave's lanes and are handed out by v_readlane.
// LDS: (16 MT + 64 NT) rows x 272 bytes; NT = 2 up to MT = 6 (60 928 bytes), NT = 1 above (MT = 14: 78 336 bytes), so two
// workgroups fit the 160 KiB of a CU; __launch_bounds__(256, 2) keeps the registers to that too.
// Partition and order are functions of the shape alone (plan() below): workgroup v = (b, slice, column block), set
// b nsl + slice, written to the caller's workspace [set][Cout][Cin k k + 1].  No atomics.  The longest fp32 addition chain
// is one accumulator's MFMA K chain over its slice: 64 sl <= 4096 terms (sl = 64 chunks at most; halved down to 8 while
// the launch has fewer than 512 workgroups).
//
// The stride-3 layers (Unit._route "conv_s3", "mfma_s3", "deconv", "mfma_deconv") use the same kernel in its S3 form:
// decnet_conv2d_k3s3_wgrad (Conv2d k 3, stride 3, padding 1) and decnet_deconv2d_k3s3_wgrad (ConvTranspose2d k 3, stride 3).
// Both weight gradients are one correlation of a coarse tensor P with the 3 x 3 stride-3 windows of a fine tensor Q,
//     R[cp][cq][ky][kx] = sum_{b,i,j} P[b][cp][i][j] * Q[b][cq][3i - pad + ky][3j - pad + kx]              (zeros outside)
// -- conv: P = gm [B,Cout,Ho,Wo], Q = x [B,Cin,H,W], pad 1; transposed: P = x [B,Cin,H,W], Q = gm [B,Cout,3H,3W], pad 0 --,
// and R is the layer's own weight layout, [Cout,Cin,3,3] / [Cin,Cout,3,3].  The GEMM is [Cp x coarse pixels] . [coarse
// pixels x (9 Cq + 1)]: chunks, slices and plan() run over the coarse plane, lane = coarse pixel (i, j), and a tap row reads
// the fine plane in place at (3i - pad + ky) Wf + 3j - pad + kx (no space-to-depth copy: 9 Cq may exceed the 224 channels of
// the stride-1 entry), again from an address clamped into the plane (element 0 where the tap misses the Hf x Wf image) and
// selected afterwards.  Cp, Cq <= 224; LDS and __launch_bounds__ as above.  The column of ones yields the sums of P: gsum
// for the conv, sum x for the transposed layer, which goes to the workspace unread; there gsum[co] = sum gm is a float64
// sum in a fixed order (chan_sum_partial: 65536 pixels of one plane per workgroup; chan_sum_final: those sums in rising
// order, rounded once).  The longest fp32 chain is the same 64 sl <= 4096 terms.  Refusals (nothing launched): NULL, also y
// without gm: NULL_POINTER; a dimension < 1, fewer workspace floats than the query: BAD_SHAPE (the planes of gy, y and gm
// follow from H and W); Cin or Cout > 224, B or the coarse H > 65535, a fine plane >= 2^29 floats: UNSUPPORTED; a workspace
// off 16 bytes: MISALIGNED.
#include "wgrad_common.h"

namespace {

constexpr int MAXCH = 224;           // Cout and Cin
constexpr int CP = 64;               // pixels of a chunk: 64 consecutive pixels of the plane, one per lane
constexpr int PITCH = CP + 4;        // floats: rows 16-byte aligned, 16 rows x 4 quads hit 64 different banks
constexpr int MAXSL = 64, MINSL = 8; // chunks of a slice: the fp32 chain is 64 sl terms

// the float i of the global array at address `base`: a wave-uniform base and a 32-bit byte offset per lane (a plane is
// below 2^29 floats)
__device__ __forceinline__ float at(unsigned long long base, int i) {
    return *reinterpret_cast<const __attribute__((address_space(1))) float *>(base + ((unsigned)i << 2));
}

// S3: the stride-3 correlation R[cp][cq][ky][kx] = sum P[b][cp][i][j] Q[b][cq][3i - pad + ky][3j - pad + kx] of a coarse tensor
// P (`gm`, Cout = Cp channels, planes H x W) with the 3 x 3 stride-3 windows of a fine tensor Q (`in`, cin = Cq channels,
// planes Hf x Wf, read in place); k is 3 and `dil` carries pad.  The chunks run over the coarse plane.
template <int MT, int NT, bool S3>
__global__ __launch_bounds__(256, 2) void conv2d_mfma_wgrad_partial(Segs in, const float *__restrict__ gm,
                                                                    float *__restrict__ ws, int Cout, int cin, int H, int W,
                                                                    int k, int dil, int ncb, int nsl, int sl, int Hf, int Wf) {
    constexpr int AR = MT * 4, BR = NT * 16;                             // rows a wave stages per chunk
    constexpr int MG = MT > 9 ? 5 : MT;
    __shared__ __attribute__((aligned(16))) float At[MT * 16 * PITCH];   // gm [co][px]; rows co >= Cout hold zeros
    __shared__ __attribute__((aligned(16))) float Bt[NT * 64 * PITCH];   // the taps [n][px] of the column block
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int v = blockIdx.x, cb = v % ncb, vs = v / ncb, s = vs % nsl, b = vs / nsl;
    const int HW = H * W, c0 = s * sl, c1 = min((HW + CP - 1) / CP, c0 + sl);
    const int kk = k * k, N = cin * kk, h = k / 2;                      // GEMM column N: the ones of gsum
    const size_t plane = (size_t)HW, tplane = S3 ? (size_t)Hf * Wf : plane;     // of gm, of the taps' tensor
    // The tap rows this wave stages, wave + 4 i of the block (i < BR), live in the registers of lane i: the plane of (b, ci),
    // the tap's distance off = dy W + dx in the plane, and tp = 3 ky + kx (k = 1: 0), 9 for the column of ones, 10 for a
    // column past the GEMM.  v_readlane hands them out as scalars: no table in memory, no load that waits for one.
    const float *r_p = in.p[0] + (size_t)b * in.c[0] * tplane;
    int r_off = 0, r_tp = 10;
    const int dyc = min(dil, H), dxc = min(dil, W);                     // (a tap a whole image away never meets the image)
    {
        const int n = cb * (NT * 64) + wave + 4 * min(lane, BR - 1);
        if (n == N) r_tp = 9;
        if (n < N) {
            const int ci = n / kk, tp = n - ci * kk, ky = tp / k, kx = tp - ky * k;
            int sg = 0, cs = ci;
            while (cs >= in.c[sg]) cs -= in.c[sg++];
            r_p = in.p[sg] + ((size_t)b * in.c[sg] + cs) * tplane;
            r_off = S3 ? ky * Wf + kx                                   // (from the window's corner)
                       : (ky - h) * dyc * W + (kx - h) * dxc;           // (used only where the tap meets the image)
            r_tp = k == 1 ? 0 : tp;
        }
    }
    const int r_lo = (int)(unsigned long long)r_p, r_hi = (int)((unsigned long long)r_p >> 32);
    const float *ga = gm + (size_t)b * Cout * plane;
    // The loads of chunk c: wave w the rows w, w + 4, ... of both tiles, lane the pixel 64 c + lane of the plane.  Every
    // load is issued from an address inside its plane; what it is worth (okb: the tap meets the image, inp: the pixel
    // exists) is applied when the value goes to LDS, so that no load waits for the one before it.
    float pre[AR + BR];
    unsigned okb = 0;
    bool inp = false;
    auto load = [&](int c) {
        const int p = c * CP + lane, pc = min(p, HW - 1), yy = pc / W, x = pc - yy * W;
        inp = p < HW;
        unsigned tapok = inp;                                           // bit 3 ky + kx: that tap of this pixel is in the image
        int corner = 0;                                                 // S3: the window's corner in the fine plane (may lie outside)
        if (S3) {
            const int y0 = 3 * yy - dil, x0 = 3 * x - dil;
            corner = y0 * Wf + x0;
            tapok = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    tapok |= (unsigned)(inp & ((unsigned)(y0 + ky) < (unsigned)Hf) & ((unsigned)(x0 + kx) < (unsigned)Wf))
                             << (3 * ky + kx);
        } else if (k == 3) {
            tapok = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    tapok |= (unsigned)(inp & ((unsigned)(yy + (ky - 1) * dyc) < (unsigned)H) &
                                        ((unsigned)(x + (kx - 1) * dxc) < (unsigned)W)) << (3 * ky + kx);
        }
        okb = 0;
#pragma unroll
        for (int i = 0; i < AR; ++i) pre[i] = at((unsigned long long)(ga + (size_t)min(wave + 4 * i, Cout - 1) * plane), pc);
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const unsigned long long base = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(r_lo, i) |
                                            (unsigned long long)(unsigned)__builtin_amdgcn_readlane(r_hi, i) << 32;
            const unsigned ok = tapok >> __builtin_amdgcn_readlane(r_tp, i) & 1;
            const int off = __builtin_amdgcn_readlane(r_off, i);
            pre[AR + i] = S3 ? at(base, (corner + off) & -(int)ok) : at(base, pc + (off & -(int)ok));
            okb |= ok << i;
        }
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(c0);
    for (int c = c0; c < c1; ++c) {
#pragma unroll
        for (int i = 0; i < AR; ++i) At[(wave + 4 * i) * PITCH + lane] = inp && wave + 4 * i < Cout ? pre[i] : 0.f;
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const float other = __builtin_amdgcn_readlane(r_tp, i) == 9 ? 1.f : 0.f;     // (the column of ones)
            Bt[(wave + 4 * i) * PITCH + lane] = okb >> i & 1 ? pre[AR + i] : other;
        }
        __syncthreads();
        load(min(c + 1, c1 - 1));
        // ---- four groups of 16 pixels, lane (m, kq) the pixels 16 g + 4 kq + e ----
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int px = 16 * gq + 4 * kq;
            f32x4 b4[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j)
                b4[j] = *reinterpret_cast<const f32x4 *>(&Bt[((wave * NT + j) * 16 + m) * PITCH + px]);
#pragma unroll
            for (int m0 = 0; m0 < MT; m0 += MG) {                       // (MG row tiles at a time: their operands in registers)
                f32x4 a4[MG];
#pragma unroll
                for (int mt = 0; mt < MG; ++mt)
                    if (m0 + mt < MT) a4[mt] = *reinterpret_cast<const f32x4 *>(&At[((m0 + mt) * 16 + m) * PITCH + px]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < MG; ++mt)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            if (m0 + mt < MT)
                                acc[m0 + mt][j] =
                                    __builtin_amdgcn_mfma_f32_16x16x4f32(a4[mt][e], b4[j][e], acc[m0 + mt][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D: register e of lane (m, kq) is row 4 kq + e (channel), column m (GEMM column)
    const int N1 = N + 1;
    float *wp = ws + ((size_t)b * nsl + s) * ((size_t)Cout * N1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = mt * 16 + 4 * kq + e, n = ((cb * 4 + wave) * NT + j) * 16 + m;
                if (co < Cout && n < N1) wp[(size_t)co * N1 + n] = acc[mt][j][e];
            }
}

// the partition of a shape (sets == 0: not covered)
struct Plan {
    int mt, nt, ncb, nsl, sl;
    long sets, groups;
};

Plan plan(int B, int Cin, int Cout, int H, int W, int k) {
    Plan p{};
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return p;
    if ((k != 1 && k != 3) || Cout > MAXCH || Cin > MAXCH || H > 65535 || B > 65535) return p;
    if ((double)H * W >= 536870912.0 || (double)B * (Cin > Cout ? Cin : Cout) * H * W >= 9.0e18) return p;
    const int tiles = ceil_div(Cout, 16), N1 = Cin * k * k + 1;
    p.mt = tiles <= 3 ? tiles : tiles <= 5 ? 5 : tiles <= 6 ? 6 : tiles <= 9 ? 9 : 14;
    p.nt = p.mt <= 6 && N1 > 64 ? 2 : 1;
    p.ncb = ceil_div(N1, 64 * p.nt);
    const long C = ((long)H * W + CP - 1) / CP;                        // chunks of one image
    p.sl = MAXSL;
    while (p.sl > MINSL && (double)B * ((C + p.sl - 1) / p.sl) * p.ncb < 512.0) p.sl >>= 1;
    const long nsl = (C + p.sl - 1) / p.sl;
    if ((double)B * nsl * p.ncb >= 2.0e9 || (double)B * nsl >= 2.0e9) return p;   // (workgroups and sets are ints)
    p.nsl = (int)nsl;
    p.sets = (long)B * nsl;
    p.groups = p.sets * p.ncb;
    return p;
}

// the GEMM launch of a plan: rows [Cout x pixels of H x W] of `a`, columns the taps of `in`
template <bool S3>
int launch_partial(const Plan &p, const Segs &in, const float *a, float *workspace, int Cout, int cin, int H, int W, int k,
                   int dil, int Hf, int Wf, hipStream_t s) {
    const dim3 grid((unsigned)p.groups);
#define GO(MT_, NT_)                                                                                                  \
    hipLaunchKernelGGL((conv2d_mfma_wgrad_partial<MT_, NT_, S3>), grid, dim3(256), 0, s, in, a, workspace, Cout, cin, \
                       H, W, k, dil, p.ncb, p.nsl, p.sl, Hf, Wf)
#define GON(MT_)                                                                                                      \
    case MT_:                                                                                                         \
        if (p.nt == 2) GO(MT_, 2); else GO(MT_, 1);                                                                   \
        break
    switch (p.mt) {
        GON(1); GON(2); GON(3); GON(5); GON(6);
        case 9: GO(9, 1); break;
        default: GO(14, 1);
    }
#undef GON
#undef GO
    return decnet_launch_status();
}

// ---- the stride-3 layers: Conv2d k 3, stride 3, padding 1 (tr = false) and ConvTranspose2d k 3, stride 3 (tr = true) ----------
// Both weight gradients are the S3 correlation above.  Conv: P = gm [B,Cout,Ho,Wo], Q = x [B,Cin,H,W], pad 1.  Transposed:
// P = x [B,Cin,H,W], Q = gm [B,Cout,3H,3W], pad 0 -- every tap meets the image.  R comes out in the layer's own weight layout.
constexpr int SUMSL = 65536;         // pixels of one plane that a workgroup of chan_sum_partial adds

struct PlanS3 {
    Plan p;                          // over (B, Cq, Cp, coarse plane)
    int cp, cq, hc, wc, hf, wf;
    long nsum;                       // transposed: slices of a fine plane in chan_sum_partial
    size_t sets_floats, floats;      // the partial sets; all of the workspace (0: not covered)
};

PlanS3 plan_s3(bool tr, int B, int Cin, int Cout, int H, int W) {
    PlanS3 q{};
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || Cin > MAXCH || Cout > MAXCH) return q;
    if ((double)H * W * (tr ? 9 : 1) >= 536870912.0) return q;        // (a fine plane is addressed by a 32-bit byte offset)
    q.cp = tr ? Cin : Cout; q.cq = tr ? Cout : Cin;
    q.hc = tr ? H : (H - 1) / 3 + 1; q.wc = tr ? W : (W - 1) / 3 + 1;
    q.hf = tr ? 3 * H : H; q.wf = tr ? 3 * W : W;
    q.p = plan(B, q.cq, q.cp, q.hc, q.wc, 3);
    if (q.p.sets == 0) return q;
    q.sets_floats = (((size_t)q.p.sets * q.cp * ((size_t)q.cq * 9 + 1)) + 3) & ~(size_t)3;
    q.floats = q.sets_floats;
    if (tr) {                        // + sum x [Cin] (the GEMM's column of ones: not wanted) + the float64 partial sums of gsum
        q.nsum = ((long)q.hf * q.wf + SUMSL - 1) / SUMSL;
        q.floats += (((size_t)Cin + 3) & ~(size_t)3) + 2 * (size_t)Cout * B * q.nsum;
        q.floats = (q.floats + 3) & ~(size_t)3;
    }
    return q;
}

// gsum of the transposed layer in float64, fixed order: workgroup (slice, co, b) adds SUMSL pixels of one plane -- thread t
// the pixels t, t + 256, ... in rising order, then the 256 sums as a tree --, chan_sum_final the B nsum sums of a channel in
// rising order, and rounds once.
__global__ __launch_bounds__(256) void chan_sum_partial(const float *__restrict__ g, double *__restrict__ part, int Cout,
                                                        size_t plane, int nsum) {
    __shared__ double red[256];
    const int t = threadIdx.x, sl = blockIdx.x, co = blockIdx.y, b = blockIdx.z;
    const float *p = g + ((size_t)b * Cout + co) * plane;
    const size_t e0 = (size_t)sl * SUMSL, e1 = e0 + SUMSL < plane ? e0 + SUMSL : plane;
    double a = 0.0;
    for (size_t e = e0 + t; e < e1; e += 256) a += (double)p[e];
    red[t] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) part[(size_t)co * gridDim.z * nsum + (size_t)b * nsum + sl] = red[0];
}

__global__ __launch_bounds__(256) void chan_sum_final(const double *__restrict__ part, float *__restrict__ gsum, int Cout,
                                                      long n) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    double a = 0.0;
    for (long i = 0; i < n; ++i) a += part[(size_t)co * n + i];
    gsum[co] = (float)a;
}

int s3_wgrad(bool tr, const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum, float *workspace,
             size_t workspace_floats, int B, int Cin, int Cout, int H, int W, void *stream) {
    if (!x || !gy || !G || !gsum || !workspace || (y && !gm)) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return DECNET_ERR_BAD_SHAPE;
    if (Cin > MAXCH || Cout > MAXCH) return DECNET_ERR_UNSUPPORTED;
    const PlanS3 q = plan_s3(tr, B, Cin, Cout, H, W);
    if (q.floats == 0) return DECNET_ERR_UNSUPPORTED;
    int rc;
    if ((rc = wgrad_workspace(workspace, workspace_floats, q.floats))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t gplane = tr ? (size_t)q.hf * q.wf : (size_t)q.hc * q.wc;       // of gy, y, gm
    if ((rc = launch_relu_mask(gy, y, gm, (size_t)B * Cout * gplane, s))) return rc;
    const float *g = y ? gm : gy;
    Segs in{};
    in.p[0] = tr ? g : x; in.c[0] = q.cq; in.n = 1;
    if ((rc = launch_partial<true>(q.p, in, tr ? x : g, workspace, q.cp, q.cq, q.hc, q.wc, 3, tr ? 0 : 1, q.hf, q.wf, s)))
        return rc;
    const int N1 = q.cq * 9 + 1;
    float *ones = tr ? workspace + q.sets_floats : gsum;                        // the sums of P
    if ((rc = launch_wgrad_reduce(workspace, G, ones, q.p.sets, q.cp, N1, s)) || !tr) return rc;
    double *part = reinterpret_cast<double *>(workspace + q.sets_floats + (((size_t)Cin + 3) & ~(size_t)3));
    hipLaunchKernelGGL(chan_sum_partial, dim3((unsigned)q.nsum, (unsigned)Cout, (unsigned)B), dim3(256), 0, s, g, part, Cout,
                       gplane, (int)q.nsum);
    if ((rc = decnet_launch_status())) return rc;
    hipLaunchKernelGGL(chan_sum_final, dim3((unsigned)ceil_div(Cout, 256)), dim3(256), 0, s, part, gsum, Cout, (long)B * q.nsum);
    return decnet_launch_status();
}

}  // namespace

extern "C" {

size_t decnet_conv2d_k3s3_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W) {
    return plan_s3(false, B, Cin, Cout, H, W).floats;
}

int decnet_conv2d_k3s3_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                             float *workspace, size_t workspace_floats, int B, int Cin, int Cout, int H, int W,
                             void *stream) {
    return s3_wgrad(false, x, gy, y, gm, G, gsum, workspace, workspace_floats, B, Cin, Cout, H, W, stream);
}

size_t decnet_deconv2d_k3s3_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W) {
    return plan_s3(true, B, Cin, Cout, H, W).floats;
}

int decnet_deconv2d_k3s3_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                               float *workspace, size_t workspace_floats, int B, int Cin, int Cout, int H, int W,
                               void *stream) {
    return s3_wgrad(true, x, gy, y, gm, G, gsum, workspace, workspace_floats, B, Cin, Cout, H, W, stream);
}

size_t decnet_conv2d_mfma_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W, int k) {
    const Plan p = plan(B, Cin, Cout, H, W, k);
    if (p.sets == 0) return 0;
    const size_t n = (size_t)p.sets * Cout * ((size_t)Cin * k * k + 1);
    return (n + 3) & ~(size_t)3;
}

int decnet_conv2d_mfma_wgrad(const float *const *xs, const int *cins, int nseg, const float *gy, const float *y, float *gm,
                             float *G, float *gsum, float *workspace, size_t workspace_floats, int B, int Cout, int H,
                             int W, int k, int dilation, void *stream) {
    Segs in{};
    int cin, rc;
    if ((rc = wgrad_stride1_args(xs, cins, nseg, gy, y, gm, G, gsum, workspace, B, Cout, H, W, k, dilation, MAXCH, &in, &cin)))
        return rc;
    const Plan p = plan(B, cin, Cout, H, W, k);
    if (p.sets == 0) return DECNET_ERR_UNSUPPORTED;
    if ((rc = wgrad_workspace(workspace, workspace_floats, decnet_conv2d_mfma_wgrad_workspace_floats(B, cin, Cout, H, W, k))))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_relu_mask(gy, y, gm, (size_t)B * Cout * H * W, s))) return rc;   // (without y: a copy, as decnet_conv2d_wgrad)
    if ((rc = launch_partial<false>(p, in, y ? gm : gy, workspace, Cout, cin, H, W, k, dilation, 0, 0, s))) return rc;
    return launch_wgrad_reduce(workspace, G, gsum, p.sets, Cout, cin * k * k + 1, s);
}

}  // extern "C"
