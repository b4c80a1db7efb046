// decnet_amd/csrc/spamat_wide.hip -- SpaMat / SpaVar for disparity ranges wider than the band kernels' 18 tiles
// (max_disp > 273: the reference's own demo data carries ndisp 400 / 610 -> max_disp 405 / 621 at stage 3,
// demo.py:149-155), forward and backward, on the matrix-core kernels instead of the VALU row-tile fallback.
//
// The candidate range [0, D) is cut into nb = ceil(D / 272) bands [d0, d0 + Db).  Band b is an ordinary call of the band
// kernels on a SHIFTED right view:  R_b[c][x] = R[c][x - d0],  tmask_b[x] = tmask[x - d0]  (both 0 for x < d0), so that
// its candidate d' of left pixel x is the original candidate d = d' + d0 and "right pixel left of the row" (SM_kernel.cu:42)
// is a masked-off pixel of the shifted view.  Bands are merged per pixel like chunks of an online softmax:
//     m = max(m_a, m_b),   S - 1e-6 = (S_a - 1e-6) e^(m_a - m) + (S_b - 1e-6) e^(m_b - m),
//     T = sum e d:  T_b = out_b S_b - 1e-6 + d0 (S_b - 1e-6),   out = (1e-6 + T) / S          (SM_kernel.cu:110-122)
// and the variance the same way with the band's disparity input shifted by d0 (SV_kernel.cu:112-121); the FUSED call
// (variance around its own disparity) is one sweep of fused band calls merged by the parallel-variance rule
// (merge_band_fused).  A band without a
// valid candidate comes back as m_b = 1e-6, S_b = 1e-6, out_b = 1 and contributes exactly nothing.  The backward kernels
// take the GLOBAL max / sum / output (minus d0 where it is a disparity), write the band's gradients into scratch planes and
// those are accumulated (the right gradient shifted back by d0).
//
// Scratch: one sweep, two providers.  The `_ws` entries of include/decnet_hip.h hand in a caller workspace of
// decnet_spamat_workspace_floats(...) floats (decnet_wide_workspace_floats below: a pure host function), and the sweep then
// runs eagerly and under stream capture alike: no allocation, no synchronisation, no question about the stream.  The six
// legacy entries pass no workspace: the same number of floats comes from the stream-ordered allocator (struct Scratch, the
// only allocator calls of this file), and while the stream is being captured they report DECNET_ERR_UNSUPPORTED so that
// capi.hip falls back to the row-tile kernels.
//
// Between band calls run two element-wise kernels, both row-structured (a wave owns a row: no division per element) with
// 16-byte stores on the 16-byte-aligned middle of a row and scalar head / tail (rows of the reference's planes are not
// multiples of four floats; the source, shifted by d0, is read in 16-byte units at 4-byte alignment):
//   band_stage       one launch per band: the shifted right features, the shifted right mask (from the float plane, or
//                    straight from the mask bits) and the offset disparity plane;
//   band_accumulate  one launch per band of the backward: grad_ref += band, grad_tar += band shifted back, grad_disp += band.
// Every element is one copy, one subtraction of d0 or one addition: the results do not depend on the launch shape.
#include "spamat_host.h"

namespace {

constexpr int WIDE_BAND = SPAMAT_BAND_DISP;      // widest band a sweep hands to the matrix-core kernels
constexpr int EW_THREADS = 256;

constexpr int ROW_WAVES = EW_THREADS / DECNET_WAVE;      // rows a workgroup works on at a time (one per wave)

// ---- row jobs: `rows` rows of W floats, dst row r made from src row r ----------------------------------------------
enum RowKind {
    ROW_SHIFT = 0,      // dst[x] = x >= shift ? src[x - shift] : 0                                (right features / mask)
    ROW_BITS = 1,       // the same from a bit-packed mask row (wpr 64-bit words, bit i of word w = pixel 64 w + i)
    ROW_OFFSET = 2,     // dst[x] = src[x] - off                                                   (the band's disparity plane)
    ROW_ADD = 3,        // dst[x] += src[x + shift] for x + shift < W                              (gradient accumulation)
};
struct RowJob {
    const void *src;
    float *dst;
    unsigned rows;      // 0: unused slot
    int kind, shift;
    float off;
};
struct RowJobs { RowJob j[3]; };

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));       // 16-byte access at 4-byte alignment (source rows)
typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));      // ... at 16-byte alignment (destination rows)

template <int KIND>
__device__ __forceinline__ float row_elem(const float *__restrict__ s, const unsigned long long *__restrict__ w,
                                          const float *d, int x, int shift, float off) {
    if (KIND == ROW_SHIFT) return x >= shift ? s[x - shift] : 0.f;
    if (KIND == ROW_BITS) return x >= shift ? (float)((w[(x - shift) >> 6] >> ((x - shift) & 63)) & 1ull) : 0.f;
    if (KIND == ROW_OFFSET) return s[x] - off;
    return d[x] + s[x + shift];
}

// One row by one wave.  s / w: the source row (floats / mask words), d: the destination row.  Elements [0, xe) are written,
// xe = W (ROW_ADD: W - shift: the source row ends there); every source index stays inside the row: [0, W - shift) for the
// shifts, [shift, W) for ROW_ADD.
template <int KIND>
__device__ __forceinline__ void wave_row(const float *__restrict__ s, const unsigned long long *__restrict__ w, float *d,
                                         int W, int shift, float off, int lane) {
    const int xe = KIND == ROW_ADD ? W - shift : W;
    if (xe <= 0) return;
    int head = (int)((4u - (unsigned)(((uintptr_t)d >> 2) & 3u)) & 3u);  // elements before the first 16-byte boundary of d
    if (head > xe) head = xe;
    const int nv = (xe - head) >> 2;
    if (lane < head) d[lane] = row_elem<KIND>(s, w, d, lane, shift, off);
    for (int v = lane; v < nv; v += DECNET_WAVE) {
        const int x = head + 4 * v;
        f4a o;
        if (KIND == ROW_SHIFT && x >= shift) {
            const f4u a = *reinterpret_cast<const f4u *>(s + (x - shift));
            o = {a.x, a.y, a.z, a.w};
        } else if (KIND == ROW_BITS && x >= shift && ((x - shift) & 63) <= 60) {
            const unsigned long long bits = w[(x - shift) >> 6] >> ((x - shift) & 63);
            o = {(float)(bits & 1ull), (float)((bits >> 1) & 1ull), (float)((bits >> 2) & 1ull), (float)((bits >> 3) & 1ull)};
        } else if (KIND == ROW_OFFSET) {
            const f4u a = *reinterpret_cast<const f4u *>(s + x);
            o = {a.x - off, a.y - off, a.z - off, a.w - off};
        } else if (KIND == ROW_ADD) {
            const f4u a = *reinterpret_cast<const f4u *>(s + (x + shift));
            const f4a c = *reinterpret_cast<const f4a *>(d + x);
            o = {c.x + a.x, c.y + a.y, c.z + a.z, c.w + a.w};
        } else {                                                          // a shift's vector that straddles x = shift, or lies left of it
            o = {row_elem<KIND>(s, w, d, x, shift, off), row_elem<KIND>(s, w, d, x + 1, shift, off),
                 row_elem<KIND>(s, w, d, x + 2, shift, off), row_elem<KIND>(s, w, d, x + 3, shift, off)};
        }
        *reinterpret_cast<f4a *>(d + x) = o;
    }
    const int x = head + 4 * nv + lane;
    if (x < xe) d[x] = row_elem<KIND>(s, w, d, x, shift, off);
}

// the rows of up to three jobs, dealt to the waves of the grid; which job a row belongs to is decided once per row
__device__ __forceinline__ void run_row_jobs(const RowJobs &jobs, int W, int wpr) {
    const int lane = threadIdx.x & (DECNET_WAVE - 1), wave = threadIdx.x / DECNET_WAVE;
    const size_t r0 = jobs.j[0].rows, r1 = r0 + jobs.j[1].rows, total = r1 + jobs.j[2].rows;
    for (size_t r = (size_t)blockIdx.x * ROW_WAVES + wave; r < total; r += (size_t)gridDim.x * ROW_WAVES) {
        const int k = r < r0 ? 0 : r < r1 ? 1 : 2;
        const size_t q = k == 0 ? r : k == 1 ? r - r0 : r - r1;
        const void *src = k == 0 ? jobs.j[0].src : k == 1 ? jobs.j[1].src : jobs.j[2].src;
        float *dst = (k == 0 ? jobs.j[0].dst : k == 1 ? jobs.j[1].dst : jobs.j[2].dst) + q * W;
        const int kind = k == 0 ? jobs.j[0].kind : k == 1 ? jobs.j[1].kind : jobs.j[2].kind;
        const int shift = k == 0 ? jobs.j[0].shift : k == 1 ? jobs.j[1].shift : jobs.j[2].shift;
        const float off = k == 0 ? jobs.j[0].off : k == 1 ? jobs.j[1].off : jobs.j[2].off;
        const float *s = static_cast<const float *>(src) + q * W;
        const unsigned long long *w = static_cast<const unsigned long long *>(src) + q * wpr;
        if (kind == ROW_SHIFT) wave_row<ROW_SHIFT>(s, nullptr, dst, W, shift, off, lane);
        else if (kind == ROW_BITS) wave_row<ROW_BITS>(nullptr, w, dst, W, shift, off, lane);
        else if (kind == ROW_OFFSET) wave_row<ROW_OFFSET>(s, nullptr, dst, W, shift, off, lane);
        else wave_row<ROW_ADD>(s, nullptr, dst, W, shift, off, lane);
    }
}
// what a band call reads: the right features and the right mask shifted by d0, the disparity-like plane minus d0
__global__ __launch_bounds__(EW_THREADS) void band_stage(RowJobs jobs, int W, int wpr) { run_row_jobs(jobs, W, wpr); }
// what a band call of the backward wrote, added to the running gradients (ROW_ADD jobs only)
__global__ __launch_bounds__(EW_THREADS) void band_accumulate(RowJobs jobs, int W) { run_row_jobs(jobs, W, 0); }

inline RowJob row_job(int kind, const void *src, float *dst, size_t rows, int shift, float off = 0.f) {
    return RowJob{src, dst, (unsigned)rows, kind, shift, off};
}
inline unsigned row_grid(const RowJobs &jobs) {
    const size_t rows = (size_t)jobs.j[0].rows + jobs.j[1].rows + jobs.j[2].rows, b = (rows + ROW_WAVES - 1) / ROW_WAVES;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}

// running (q, S, m) <- merge with band (q_b, S_b, m_b); q is a quotient (1e-6 + Q) / S; d0f shifts the band's first moment
// (disparity: d0; variance: 0).  Pixels with the left mask off keep their zeros.
__global__ __launch_bounds__(EW_THREADS) void merge_band(const float *__restrict__ rmask, float *__restrict__ q,
                                                         float *__restrict__ S, float *__restrict__ m,
                                                         const float *__restrict__ qb, const float *__restrict__ Sb,
                                                         const float *__restrict__ mb, size_t n, float d0f) {
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * EW_THREADS) {
        if (rmask[i] == 0.f) continue;
        const float ma = m[i], mbv = mb[i], mn = fmaxf(ma, mbv);
        const float ea = expf(ma - mn), eb = expf(mbv - mn);
        const float Ea = S[i] - 1e-6f, Eb = Sb[i] - 1e-6f;                   // sum of exponentials of each part
        const float Qa = q[i] * S[i] - 1e-6f, Qb = qb[i] * Sb[i] - 1e-6f + d0f * Eb;
        const float Sn = 1e-6f + (Ea * ea + Eb * eb);
        q[i] = (1e-6f + (Qa * ea + Qb * eb)) / Sn;
        S[i] = Sn;
        m[i] = mn;
    }
}
// The fused call in ONE sweep: every band returns its own disparity q_b AND the variance v_b around it; two parts A, B with
// sums of exponentials E, first moments T and second moments V around their own means o combine around the joint mean mu as
//     V(mu) = sum_X e^(m_X - m) (V_X + 2 (o_X - mu) c_X + (o_X - mu)^2 E_X),   c_X = T_X - o_X E_X = 1e-6 (o_X - 1)
// (c_X from the definitions out = (1e-6 + T) / (1e-6 + E): exact, no difference of two rounded products).  Every term
// but the tiny c_X one is non-negative: no cancellation.  Running (q, v, S, m) <- merge with band (q_b, v_b, S_b, m_b) at d0.
__global__ __launch_bounds__(EW_THREADS) void merge_band_fused(const float *__restrict__ rmask, float *__restrict__ q,
                                                               float *__restrict__ v, float *__restrict__ S,
                                                               float *__restrict__ m, const float *__restrict__ qb,
                                                               const float *__restrict__ vb, const float *__restrict__ Sb,
                                                               const float *__restrict__ mb, size_t n, float d0f) {
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * EW_THREADS) {
        if (rmask[i] == 0.f) continue;
        const float ma = m[i], mbv = mb[i], mn = fmaxf(ma, mbv);
        const float ea = expf(ma - mn), eb = expf(mbv - mn);
        const float Sa = S[i], Sbv = Sb[i], Ea = Sa - 1e-6f, Eb = Sbv - 1e-6f;
        const float oa = q[i], ob = qb[i] + d0f;                             // the parts' own means, global coordinates
        const float Ta = oa * Sa - 1e-6f, Tb = qb[i] * Sbv - 1e-6f + d0f * Eb;
        const float Va = v[i] * Sa - 1e-6f, Vb = vb[i] * Sbv - 1e-6f;
        const float Sn = 1e-6f + (Ea * ea + Eb * eb);
        const float mu = (1e-6f + (Ta * ea + Tb * eb)) / Sn;
        const float da = oa - mu, db = ob - mu;
        const float ca = 1e-6f * (oa - 1.f), cb = 1e-6f * (qb[i] - 1.f) ;    // sum e (d - o) of each part (band coordinates for B: the same number)
        const float Vn = ea * (Va + da * (2.f * ca + da * Ea)) + eb * (Vb + db * (2.f * cb + db * Eb));
        q[i] = mu;
        v[i] = (1e-6f + Vn) / Sn;
        S[i] = Sn;
        m[i] = mn;
    }
}
inline unsigned ew_grid(size_t n) {
    const size_t b = (n + EW_THREADS - 1) / EW_THREADS;
    return (unsigned)(b < 8192 ? (b ? b : 1) : 8192);
}
inline bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cap != hipStreamCaptureStatusNone;
}
// Where a sweep's scratch comes from: the caller's workspace (the `_ws` entries), or -- ws == nullptr, the legacy entries -- one
// stream-ordered allocation that is freed (stream-ordered) when the call returns.
struct Scratch {
    float *p = nullptr;
    bool own = false;
    hipStream_t s;
    explicit Scratch(hipStream_t st) : s(st) {}
    int get(float *ws, size_t floats) {
        if (ws) {
            p = ws;
            return 0;
        }
        own = true;
        return (int)hipMallocAsync((void **)&p, floats * sizeof(float), s);
    }
    ~Scratch() {
        if (own && p) (void)hipFreeAsync(p, s);
    }
};
#define CK(expr)                              \
    do {                                      \
        int rc_ = (expr);                     \
        if (rc_) return rc_;                  \
    } while (0)

// planes of np = B H W floats a forward sweep needs: the shifted right features (C), the shifted right mask, the band's
// (q, S, m); + the offset disparity (SpaVar) / the band's variance (fused); + the unpacked left mask (bit-mask entry)
inline size_t forward_planes(int C, int mode, int mbits) { return (size_t)C + 4 + (mode ? 1 : 0) + (mbits ? 1 : 0); }
// ... and a backward sweep: the shifted right features and the band's two feature gradients (3 C), the shifted right mask,
// the offset disparity-like plane; + the band's grad_disparity (SpaVar)
inline size_t backward_planes(int C, int var) { return 3 * (size_t)C + 2 + (var ? 1 : 0); }

}  // namespace

// decnet_spamat_workspace_floats of include/decnet_hip.h for valid dims (capi.hip checks them): 0 where one band takes the
// call.  which: 0 spamat_forward, 1 spavar_forward, 2 spamatvar_forward, 3 spamatvar_forward_bits, 4 spamat_backward,
// 5 spavar_backward.  No HIP call.
size_t decnet_wide_workspace_floats(int B, int C, int H, int W, int D, int which) {
    if (D <= WIDE_BAND + 1 || which < 0 || which > 5) return 0;
    const size_t np = (size_t)B * H * W;
    if (which >= 4) return backward_planes(C, which == 5) * np;
    return forward_planes(C, which == 3 ? 2 : which, which == 3) * np;
}

// a.mode 0 SpaMat (out, S, m), 1 SpaVar (var_out, S, m; `disparity` given), 2 fused (out, var_out, S, m).
// a.mbits: the masks are bit-packed (decnet_spamatvar_forward_bits): the left mask is unpacked into a scratch plane once, the
// right mask per band straight into its shifted form.
// ws: the caller's workspace (decnet_wide_workspace_floats floats, checked by capi.hip), or nullptr: allocate, and decline
// while the stream is being captured.
int decnet_wide_forward(const SpaFwd &a, float *ws) {
    const int C = a.C, W = a.W, D = a.D;
    hipStream_t stream = a.stream;
    if (D <= WIDE_BAND) return DECNET_ERR_UNSUPPORTED;
    if (!ws && capturing(stream)) return DECNET_ERR_UNSUPPORTED;
    const int nb = ceil_div(D, WIDE_BAND), Db = ceil_div(D, nb), wpr = (W + 63) >> 6;
    const size_t np = (size_t)a.B * a.H * W, rowsF = (size_t)a.B * C * a.H, rowsM = (size_t)a.B * a.H;
    Scratch sc(stream);
    CK(sc.get(ws, forward_planes(C, a.mode, a.mbits) * np));
    float *Rb = sc.p, *tmb = Rb + (size_t)C * np, *qb = tmb + np, *Sb = qb + np, *mb = Sb + np, *db = mb + np,
          *rmf = db + (a.mode ? np : 0);                                // db: modes 1, 2 only; rmf: mbits only
    const void *tsrc = a.tmask;                                         // the right mask as the caller gave it
    const int tkind = a.mbits ? ROW_BITS : ROW_SHIFT;
    SpaFwd band = a;                                                    // a band call: this call on float masks, fields set per band
    band.mbits = 0;
    if (a.mbits) {                                                      // band 0 reads float planes like every other band
        const RowJobs jobs = {{row_job(ROW_BITS, a.rmask, rmf, rowsM, 0), row_job(ROW_BITS, a.tmask, tmb, rowsM, 0), RowJob{}}};
        CK(decnet_launch(band_stage, dim3(row_grid(jobs)), dim3(EW_THREADS), 0, stream, jobs, W, wpr));
        band.rmask = rmf;
        band.tmask = tmb;
    }
    const float *rmask = band.rmask, *tmask = band.tmask;               // float planes from here on
    // band b > 0 of a sweep: (Rb, tmb[, db = disp - d0]) in one launch
    auto stage = [&](int d0, const float *disp) -> int {
        const RowJobs jobs = {{row_job(ROW_SHIFT, a.tar, Rb, rowsF, d0), row_job(tkind, tsrc, tmb, rowsM, d0),
                               disp ? row_job(ROW_OFFSET, disp, db, rowsM, 0, (float)d0) : RowJob{}}};
        return decnet_launch(band_stage, dim3(row_grid(jobs)), dim3(EW_THREADS), 0, stream, jobs, W, wpr);
    };
    // one sweep over the bands for a quotient q in {disparity (SpaMat), variance (SpaVar)}: band 0 lands in (q, S, m)
    // itself, the others in (qb, Sb, mb) and are merged in
    auto sweep = [&](int var, const float *disp, float *q, float *S, float *m) -> int {
        band.mode = var ? MODE_VAR : MODE_MAT;
        for (int b = 0; b < nb; ++b) {
            const int d0 = b * Db, dw = (D - d0 < Db) ? D - d0 : Db;
            const float *Rv = a.tar, *tv = tmask, *dv = disp;
            if (b) {
                CK(stage(d0, var ? disp : nullptr));
                Rv = Rb; tv = tmb; dv = db;
            }
            float *qo = b ? qb : q, *So = b ? Sb : S, *mo = b ? mb : m;
            band.tar = Rv;
            band.tmask = tv;
            band.disparity = var ? dv : nullptr;
            band.out = var ? nullptr : qo;
            band.var_out = var ? qo : nullptr;
            band.sum_sim = So;
            band.max_cost = mo;
            band.D = dw;
            CK(decnet_mfma_forward(band));
            if (b)
                CK(decnet_launch(merge_band, dim3(ew_grid(np)), dim3(EW_THREADS), 0, stream, rmask, q, S, m, qb, Sb, mb, np,
                                 var ? 0.f : (float)d0));
        }
        return 0;
    };
    if (a.mode == MODE_VAR) return sweep(1, a.disparity, a.var_out, a.sum_sim, a.max_cost);
    if (a.mode == MODE_MAT) return sweep(0, nullptr, a.out, a.sum_sim, a.max_cost);
    // fused: one sweep of fused band calls (each band's variance around its own disparity, in db), merged around the joint mean
    band.disparity = nullptr;
    for (int b = 0; b < nb; ++b) {
        const int d0 = b * Db;
        band.D = (D - d0 < Db) ? D - d0 : Db;
        if (!b) {
            CK(decnet_mfma_forward(band));                              // straight into (out, var_out, sum_sim, max_cost)
            continue;
        }
        CK(stage(d0, nullptr));
        band.tar = Rb;
        band.tmask = tmb;
        band.out = qb;
        band.var_out = db;
        band.sum_sim = Sb;
        band.max_cost = mb;
        CK(decnet_mfma_forward(band));
        CK(decnet_launch(merge_band_fused, dim3(ew_grid(np)), dim3(EW_THREADS), 0, stream, rmask, a.out, a.var_out, a.sum_sim,
                         a.max_cost, qb, db, Sb, mb, np, (float)d0));
    }
    return 0;
}

// a.var: 0 SpaMat, 1 SpaVar (also grad_disp).  ws as in decnet_wide_forward.
int decnet_wide_backward(const SpaBwd &a, float *ws) {
    const int var = a.var, C = a.C, W = a.W, D = a.D;
    hipStream_t stream = a.stream;
    if (D <= WIDE_BAND) return DECNET_ERR_UNSUPPORTED;
    if (!ws && capturing(stream)) return DECNET_ERR_UNSUPPORTED;
    const int nb = ceil_div(D, WIDE_BAND), Db = ceil_div(D, nb);
    const size_t np = (size_t)a.B * a.H * W, nf = (size_t)C * np, rowsF = (size_t)a.B * C * a.H, rowsM = (size_t)a.B * a.H;
    Scratch sc(stream);
    CK(sc.get(ws, backward_planes(C, var) * np));
    float *Rb = sc.p, *glb = Rb + nf, *grb = glb + nf, *tmb = grb + nf, *sh = tmb + np, *gdb = sh + np;   // gdb: SpaVar only
    SpaBwd band = a;                                                    // band 0: this call, narrower
    for (int b = 0; b < nb; ++b) {
        const int d0 = b * Db;
        band.D = (D - d0 < Db) ? D - d0 : Db;
        if (!b) {
            CK(decnet_mfma_backward(band));
            continue;
        }
        // the plane that is a disparity moves with the band: SpaMat's output (SM_kernel.cu:191), SpaVar's input (SV_kernel.cu:191)
        const RowJobs in = {{row_job(ROW_SHIFT, a.tar, Rb, rowsF, d0), row_job(ROW_SHIFT, a.tmask, tmb, rowsM, d0),
                             row_job(ROW_OFFSET, var ? a.disparity : a.out, sh, rowsM, 0, (float)d0)}};
        CK(decnet_launch(band_stage, dim3(row_grid(in)), dim3(EW_THREADS), 0, stream, in, W, 0));
        band.tar = Rb;
        band.tmask = tmb;
        band.disparity = var ? sh : nullptr;
        band.out = var ? a.out : sh;
        band.grad_ref = glb;
        band.grad_tar = grb;
        band.grad_disp = var ? gdb : nullptr;
        CK(decnet_mfma_backward(band));
        const RowJobs acc = {{row_job(ROW_ADD, glb, a.grad_ref, rowsF, 0), row_job(ROW_ADD, grb, a.grad_tar, rowsF, d0),
                              var ? row_job(ROW_ADD, gdb, a.grad_disp, rowsM, 0) : RowJob{}}};
        CK(decnet_launch(band_accumulate, dim3(row_grid(acc)), dim3(EW_THREADS), 0, stream, acc, W));
    }
    return 0;
}
