// decnet_amd/csrc/conv3d_grad.hip -- the weight-gradient reduction of the stage-0 Conv3dUnit layers (Conv3d k 3, s 1, p 1 on
// channels-last [B,D,H,W,C] volumes; csrc/stage0.hip, csrc/conv3d_winograd.hip) with frozen BatchNorm: the 3-D counterpart
// of csrc/conv2d_mfma_grad.hip.  For y = act(conv(x, w) * scale + shift) and the upstream gradient gy
//     gm                    = gy * [y > 0]                                                     (gy itself without y)
//     G[co][ci][kd][kh][kw] = sum_{b,d,h,w} gm[b,d,h,w,co] * x[b,d+kd-1,h+kh-1,w+kw-1,ci]      (zeros outside)
//     gsum[co]              = sum_{b,d,h,w} gm[b,d,h,w,co]
// G in torch's [Co,Ci,3,3,3] layout, so that dW = scale G, dscale = <w, G>, dshift = gsum.
//
// The sequence is that of csrc/wgrad_common.h (mask, GEMM into partial sets, float64 reduction, here with TAPS = 27: it
// writes the torch layout); this file holds its step
//   2. conv3d_wgrad_partial runs the GEMM [Co x voxels] . [voxels x (27 Ci + 1)] on v_mfma_f32_16x16x4_f32 (bit for bit an
//      fp32 fma chain over the voxels).  GEMM column n = tap Ci + ci, tap = 9 kd + 3 kh + kw; column 27 Ci is the column
//      of ones that yields gsum.  Both operands are channels-last, so a chunk of KC = 32 consecutive voxels of gm is ONE
//      contiguous run of 32 Co floats, and 64 consecutive columns of one voxel are (up to a change of tap) one contiguous
//      run of x.  A 256-thread workgroup owns every row of G (MT tiles of 16 channels), one block of 64 columns (wave w the
//      tile w) and one slice of `sl` consecutive voxels of the flat volume (all images run on).  Per chunk it stages gm as
//      [voxel][co] and the tap values as [voxel][n] in LDS -- one coalesced dword per lane, from an address clamped into
//      the volume and selected afterwards, at any float alignment, all issued before the first is used and, for chunk c + 1,
//      in flight while the MFMAs of chunk c run; the pitches are 16 mod 64 floats, so the operand reads
//      of a wave (lane (m, kq): voxel 4 ks + kq, channel / column m) hit 64 different banks.  Which of the 27 taps of a
//      voxel meet the volume is one 27-bit word per voxel, formed a chunk ahead by the first 32 threads.  Every LDS word
//      that is read is written first: rows co >= Co and the voxels past the end of the slice hold zeros.
// Partition and order are functions of the shape alone (plan() below): set s holds the voxels [s sl, min((s + 1) sl, V)) of
// the V = B D H W, with sl a power of two: 4096, halved down to 256 while the launch has fewer than 1024 workgroups.  The
// workspace is [set][Co][27 Ci + 1].  No atomics.  The longest fp32 addition chain is one accumulator's MFMA K chain over
// its slice: sl <= 4096 terms.
// Limits: Ci a multiple of 4 (as the forward entries), Ci, Co <= 224, V max(Ci, Co) < 2^31 (element offsets are 32-bit).
// Refusals (nothing launched): NULL, also y without gm: NULL_POINTER; a dimension < 1, fewer workspace floats than the
// query: BAD_SHAPE; Ci % 4, Ci or Co > 224, the size limit: UNSUPPORTED; a workspace off 16 bytes: MISALIGNED.
#include "wgrad_common.h"

namespace {

constexpr int MAXCH = 224;            // Ci and Co
constexpr int KC = 32;                // voxels of a chunk
constexpr int NB = 64;                // GEMM columns of a workgroup: 4 waves x one tile of 16
constexpr int BP = NB + 16;           // floats; 16 mod 64: the 4 voxels x 16 columns of an operand read hit 64 banks
constexpr int MAXSL = 4096, MINSL = 256;   // voxels of a slice: the fp32 chain is sl terms

constexpr int a_pitch(int mt) { return (mt * 16 + 47) / 64 * 64 + 16; }      // >= 16 mt, 16 mod 64

template <int MT>
__global__ __launch_bounds__(256, 2) void conv3d_wgrad_partial(const float *__restrict__ x, const float *__restrict__ gm,
                                                               float *__restrict__ ws, int V, int D, int H, int W, int Ci,
                                                               int Co, int ncb, int sl) {
    constexpr int AP = a_pitch(MT);
    __shared__ float At[KC * AP];                                       // gm [voxel][co]; co >= Co: zeros
    __shared__ float Bt[KC * BP];                                       // the taps [voxel][n] of the column block
    __shared__ unsigned vm[2][KC];                                      // bit tap: that tap of the voxel is in the volume
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int cb = blockIdx.x % ncb, set = blockIdx.x / ncb;
    const int vbeg = set * sl, vend = min(V, vbeg + sl);                // (vbeg < V: plan())
    const int N = 27 * Ci;
    // this thread's column of the block, fixed for the whole kernel: kind 0 a tap column, 1 the ones, 2 past the GEMM
    const int n = cb * NB + lane;
    int kind = n < N ? 0 : n == N ? 1 : 2, tap = 0, ci = 0, off = 0;
    if (kind == 0) {
        tap = n / Ci;
        ci = n - tap * Ci;
        const int kd = tap / 9, kh = (tap - 9 * kd) / 3, kw = tap - 9 * kd - 3 * kh;
        off = ((kd - 1) * H + (kh - 1)) * W + (kw - 1);                 // (used only where the tap meets the volume)
    }
    auto mask_of = [&](int v0, int buf) {                              // the 27-bit words of the chunk at v0
        if (t < KC) {
            unsigned mk = 0;
            const int v = v0 + t;
            if (v < vend) {
                const int q = v / W, w = v - q * W, q2 = q / H, h = q - q2 * H, d = q2 % D;
#pragma unroll
                for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
                            mk |= (unsigned)(((unsigned)(d + kd - 1) < (unsigned)D) & ((unsigned)(h + kh - 1) < (unsigned)H) &
                                             ((unsigned)(w + kw - 1) < (unsigned)W)) << (9 * kd + 3 * kh + kw);
            }
            vm[buf][t] = mk;
        }
    };
    for (int i = t; i < KC * AP; i += 256) At[i] = 0.f;                 // (the rows co >= Co stay zero)
    mask_of(vbeg, 0);
    __syncthreads();
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int qa = 256 / Co, ra = 256 - qa * Co;                        // thread t walks the chunk's gm in steps of 256 floats
    constexpr int NA = 2 * MT;                                          // KC * 16 MT / 256: its steps at most
    // The loads of the chunk at v0, all issued before the first is used: the chunk's gm is the KC Co floats from gm + v0 Co
    // on, one contiguous run (thread t the floats t, t + 256, ...); of the taps wave w takes the voxels w, w + 4, ..., lane
    // the column.  Every load comes from an address inside the volume; what it is worth (pa: inside the slice, okb: the tap
    // meets the volume) is applied when the value goes to LDS, so that no load waits for the one before it.
    float pa[NA], pb[KC / 4];
    unsigned okb = 0;
    auto load = [&](int v0, int buf) {
        const int nv = min(KC, vend - v0), na = nv * Co;
        const float *g = gm + (size_t)v0 * Co;
#pragma unroll
        for (int i = 0; i < NA; ++i) pa[i] = g[min(t + 256 * i, na - 1)];
        okb = 0;
#pragma unroll
        for (int i = 0; i < KC / 4; ++i) {
            const int vox = wave + 4 * i, v = min(v0 + vox, vend - 1);
            const unsigned ok = (unsigned)(kind == 0) & (unsigned)(vox < nv) & (vm[buf][vox] >> tap);
            pb[i] = x[(size_t)(v + (off & -(int)(ok & 1))) * Ci + ci];
            okb |= (ok & 1) << i;
        }
    };
    int buf = 0;
    load(vbeg, 0);
    for (int v0 = vbeg; v0 < vend; v0 += KC, buf ^= 1) {
        const int nv = min(KC, vend - v0), na = nv * Co;
        {
            int vox = t / Co, co = t - vox * Co;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = t + 256 * i;
                if (idx < KC * Co) At[vox * AP + co] = idx < na ? pa[i] : 0.f;
                vox += qa;
                co += ra;
                if (co >= Co) {
                    co -= Co;
                    ++vox;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KC / 4; ++i) {
            const int vox = wave + 4 * i;
            Bt[vox * BP + lane] = okb >> i & 1 ? pb[i] : kind == 1 && vox < nv ? 1.f : 0.f;
        }
        mask_of(v0 + KC, buf ^ 1);
        __syncthreads();
        if (v0 + KC < vend) load(v0 + KC, buf ^ 1);                     // in flight while the MFMAs of this chunk run
        // ---- KC / 4 steps of 4 voxels: lane (m, kq) the voxel 4 ks + kq ----
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            const int row = 4 * ks + kq;
            const float b = Bt[row * BP + wave * 16 + m];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(At[row * AP + mt * 16 + m], b, acc[mt], 0, 0, 0);
        }
        __syncthreads();
    }
    // D: register e of lane (m, kq) is row 4 kq + e (channel), column m (GEMM column)
    const int N1 = N + 1, nn = cb * NB + wave * 16 + m;
    float *wp = ws + (size_t)set * ((size_t)Co * N1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = mt * 16 + 4 * kq + e;
            if (co < Co && nn < N1) wp[(size_t)co * N1 + nn] = acc[mt][e];
        }
}

// the partition of a shape (nsets == 0: not covered)
struct Plan {
    int mt, ncb, sl, V;
    long nsets;
};

Plan plan(int B, int D, int H, int W, int Ci, int Co) {
    Plan p{};
    if (B < 1 || D < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1) return p;
    if (Ci % 4 || Ci > MAXCH || Co > MAXCH) return p;
    const double V = (double)B * D * H * W;
    if (V * (Ci > Co ? Ci : Co) >= 2147483648.0) return p;             // (32-bit element offsets)
    p.V = (int)V;
    const int tiles = ceil_div(Co, 16);
    p.mt = tiles <= 2 ? tiles : tiles <= 4 ? 4 : tiles <= 8 ? 8 : 14;
    p.ncb = ceil_div(27 * Ci + 1, NB);
    p.sl = MAXSL;
    while (p.sl > MINSL && (long)p.ncb * ceil_div(p.V, p.sl) < 1024) p.sl >>= 1;
    p.nsets = ceil_div(p.V, p.sl);
    return p;
}

}  // namespace

extern "C" {

size_t decnet_conv3d_wgrad_workspace_floats(int B, int D, int H, int W, int Ci, int Co) {
    const Plan p = plan(B, D, H, W, Ci, Co);
    return (size_t)p.nsets * (size_t)Co * ((size_t)27 * Ci + 1);
}

int decnet_conv3d_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                        float *workspace, size_t workspace_floats, int B, int D, int H, int W, int Ci, int Co,
                        void *stream) {
    if (!x || !gy || !G || !gsum || !workspace || (y && !gm)) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || D < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1) return DECNET_ERR_BAD_SHAPE;
    const Plan p = plan(B, D, H, W, Ci, Co);
    if (p.nsets == 0) return DECNET_ERR_UNSUPPORTED;
    int rc;
    if ((rc = wgrad_workspace(workspace, workspace_floats, decnet_conv3d_wgrad_workspace_floats(B, D, H, W, Ci, Co)))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_relu_mask(gy, y, gm, (size_t)p.V * Co, s))) return rc;   // (without y: a copy, as decnet_conv2d_mfma_wgrad)
    const float *a = y ? gm : gy;
    const dim3 grid((unsigned)(p.nsets * p.ncb));
#define GO(MT_)                                                                                                       \
    case MT_:                                                                                                         \
        hipLaunchKernelGGL((conv3d_wgrad_partial<MT_>), grid, dim3(256), 0, s, x, a, workspace, p.V, D, H, W, Ci, Co, \
                           p.ncb, p.sl);                                                                              \
        break
    switch (p.mt) {
        GO(1); GO(2); GO(4); GO(8);
        default: hipLaunchKernelGGL((conv3d_wgrad_partial<14>), grid, dim3(256), 0, s, x, a, workspace, p.V, D, H, W, Ci, Co,
                                    p.ncb, p.sl);
    }
#undef GO
    if ((rc = decnet_launch_status())) return rc;
    return launch_wgrad_reduce<27>(workspace, G, gsum, p.nsets, Co, 27 * Ci + 1, s);
}

}  // extern "C"
