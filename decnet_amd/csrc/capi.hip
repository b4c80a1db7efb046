// decnet_amd/csrc/capi.hip -- extern "C" entry points for SpaMat / SpaVar (include/decnet_hip.h).
#include "spamat_host.h"

#include <stdlib.h>
#include <string.h>

#include <initializer_list>

static int spamat_pinned() {       // DECNET_SPAMAT_KERNEL, read once
    static const int pinned = [] {
        const char *e = getenv("DECNET_SPAMAT_KERNEL");
        if (!e) return 0;
        return !strcmp(e, "rowtile") ? 1 : !strcmp(e, "mfma") ? 2 : !strcmp(e, "mfma_dense") ? 3 : 0;
    }();
    return pinned;
}

// ---- DECNET_CHECK_FINITE=1: the NaN contract of include/decnet_hip.h made checkable --------------------------------
// The reference propagates a NaN / Inf feature into every output whose candidate set touches it (fmaxf / expf,
// SM_kernel.cu:46-58); the forward kernels here are built with -fno-honor-nans and give an unspecified value there.
// With the knob set, both feature maps are swept by one reduction kernel before the launch and a non-finite element is
// an error (DECNET_ERR_NONFINITE, nothing else launched) instead of a silently different result.  The check waits for
// the stream (one 4-byte read-back), so it is a debugging aid: skipped while the stream is being captured into a graph.
namespace {
__global__ __launch_bounds__(256) void count_nonfinite(const float *__restrict__ x, size_t n4, size_t n,
                                                       unsigned *__restrict__ count) {
    unsigned bad = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4 *>(x)[i];
        // exponent all ones <=> Inf or NaN (integer test: immune to -fno-honor-nans style folding)
        bad += ((__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u) + ((__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u) +
               ((__float_as_uint(v.z) & 0x7f800000u) == 0x7f800000u) + ((__float_as_uint(v.w) & 0x7f800000u) == 0x7f800000u);
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)   // tail (everything when
        bad += (__float_as_uint(x[i]) & 0x7f800000u) == 0x7f800000u;                                // the map is not 16-byte aligned)
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}
}  // namespace

static bool check_finite_on() {
    static const bool on = [] { const char *e = getenv("DECNET_CHECK_FINITE"); return e && atoi(e) != 0; }();
    return on;
}

// 0: all finite (or the check is off / the stream is capturing); DECNET_ERR_NONFINITE; positive hipError_t
static int check_finite(const float *ref, const float *tar, int B, int C, int H, int W, hipStream_t stream) {
    if (!check_finite_on()) return 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return 0;
    }
    const bool aligned = ((((uintptr_t)ref) | ((uintptr_t)tar)) & 15) == 0;   // (torch allocations are; a view may not be)
    unsigned *d = nullptr, h = 0;
    hipError_t e = hipMallocAsync((void **)&d, sizeof(unsigned), stream);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(d, 0, sizeof(unsigned), stream);
    const size_t n = (size_t)B * C * H * W, n4 = aligned ? n >> 2 : 0;
    const size_t nwork = aligned ? n4 : n;
    const unsigned grid = (unsigned)((nwork + 255) / 256 < 2048 ? (nwork + 255) / 256 + 1 : 2048);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(count_nonfinite, dim3(grid), dim3(256), 0, stream, ref, n4, n, d);
        hipLaunchKernelGGL(count_nonfinite, dim3(grid), dim3(256), 0, stream, tar, n4, n, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(unsigned), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFreeAsync(d, stream);
    if (e != hipSuccess) return (int)e;
    return h ? DECNET_ERR_NONFINITE : 0;
}

// ---- the caller-workspace (`_ws`) entries ------------------------------------------------------------------------------
// workspace floats of entry `which` (include/decnet_hip.h); 0 for bad shapes and wherever one band takes the call
static size_t workspace_floats(int B, int C, int H, int W, int max_disp, int which) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || max_disp < 1 || (double)B * C * H * W >= 2147483648.0) return 0;
    return decnet_wide_workspace_floats(B, C, H, W, max_disp, which);
}
// Scratch of one call.  legacy(): the six original entries (the sweep allocates).  A `_ws` entry passes what its caller
// gave; check() then is the workspace contract of the header, before anything is launched.
struct Workspace {
    float *p;
    size_t floats;
    bool given;
    static Workspace legacy() { return Workspace{nullptr, 0, false}; }
    int check(int B, int C, int H, int W, int max_disp, int which) {
        const size_t need = given ? workspace_floats(B, C, H, W, max_disp, which) : 0;
        if (!need) {                    // one band (or a legacy entry): exactly the existing entry
            p = nullptr;
            return DECNET_OK;
        }
        if (!p) return DECNET_ERR_NULL_POINTER;
        if (floats < need) return DECNET_ERR_BAD_SHAPE;
        if ((uintptr_t)p & 15) return DECNET_ERR_MISALIGNED;
        return DECNET_OK;
    }
};

// ---- one call path per direction ---------------------------------------------------------------------------------------
// `which` is the entry as decnet_spamat_workspace_floats numbers them: 0 spamat_forward, 1 spavar_forward,
// 2 spamatvar_forward, 3 spamatvar_forward_bits, 4 spamat_backward, 5 spavar_backward; it says which pointers of the record
// the entry has and which workspace it needs.  Order of rejection: null tensor pointer, bad shape, workspace (null / short /
// misaligned), check_finite, launch.
static int check_args(std::initializer_list<const void *> ptrs, int B, int C, int H, int W, int max_disp) {
    for (const void *p : ptrs)
        if (!p) return DECNET_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || H < 1 || W < 1 || max_disp < 1) return DECNET_ERR_BAD_SHAPE;
    if ((double)B * C * H * W >= 2147483648.0) return DECNET_ERR_BAD_SHAPE;
    return DECNET_OK;
}

// Forward dispatch: the MFMA band kernel; the row-tile kernel covers what it cannot
// (band wider than 18 tiles, LDS overflow).  DECNET_SPAMAT_KERNEL=rowtile|mfma|mfma_dense pins
// one variant (read once; used by the A/B benchmarks and the parity tests of the variants);
// mfma_dense = MFMA kernel with the sparse-row compaction path switched off.
// The bit-mask entry (a.mbits) has the matrix-core kernels only (the row-tile fallback reads float planes); above max_disp
// 273 (18 tiles) band by band with the masks unpacked into scratch planes (spamat_wide.hip; the legacy entry, whose sweep
// allocates, is UNSUPPORTED there while the stream is being captured; the `_ws` entry is not).
// DECNET_SPAMAT_KERNEL=rowtile pins a kernel that entry does not have -> UNSUPPORTED, the caller falls back to the
// float-mask entry (decnet_amd.model does)
static int run_forward(SpaFwd a, int which, Workspace ws) {
    // the one or two outputs and the disparity input differ by entry: out (0), disparity + var_out (1), out + var_out (2, 3)
    int rc = check_args({a.ref, a.tar, a.rmask, a.tmask, which == 1 ? a.disparity : a.out,
                         which ? a.var_out : a.out, a.sum_sim, a.max_cost}, a.B, a.C, a.H, a.W, a.D);
    if (rc) return rc;
    if ((rc = ws.check(a.B, a.C, a.H, a.W, a.D, which))) return rc;
    const int pinned = spamat_pinned();
    if (a.mbits && pinned == 1) return DECNET_ERR_UNSUPPORTED;
    if ((rc = check_finite(a.ref, a.tar, a.B, a.C, a.H, a.W, a.stream))) return rc;
    if (pinned == 3) a.allow_compact = 0;
    if (pinned != 1) {
        rc = decnet_mfma_forward(a);
        if (rc == DECNET_ERR_UNSUPPORTED && a.D > SPAMAT_BAND_DISP)   // wider than 18 tiles: the same kernels band by band
            rc = decnet_wide_forward(a, ws.p);
        if (rc != DECNET_ERR_UNSUPPORTED || pinned >= 2 || a.mbits) return rc;
    }
    return decnet_rowtile_forward(a);
}

// Backward dispatch: matrix-core kernels, row-tile kernels for what they do not cover.  ws.p: the wide sweep's scratch from
// the caller (the `_ws` entries, checked by ws.check), or nullptr (the legacy entries).
static int run_backward(const SpaBwd &a, int which, Workspace ws) {
    // SpaVar (5) also has the disparity input and its gradient
    int rc = check_args({a.ref, a.tar, a.rmask, a.tmask, a.out, a.sum_sim, a.max_cost, a.grad_out, a.grad_ref, a.grad_tar,
                         which == 5 ? a.disparity : a.ref, which == 5 ? a.grad_disp : a.grad_ref}, a.B, a.C, a.H, a.W, a.D);
    if (rc) return rc;
    if ((rc = ws.check(a.B, a.C, a.H, a.W, a.D, which))) return rc;
    const int pinned = spamat_pinned();
    if (pinned != 1) {
        rc = decnet_mfma_backward(a);
        if (rc == DECNET_ERR_UNSUPPORTED && a.D > SPAMAT_BAND_DISP)   // wider than 18 tiles: the same kernels band by band
            rc = decnet_wide_backward(a, ws.p);
        if (rc != DECNET_ERR_UNSUPPORTED || pinned >= 2) return rc;
    }
    return decnet_rowtile_backward(a);
}

// the bit-packed masks of decnet_spamatvar_forward_bits travel in the record's float-mask fields (SpaFwd::mbits)
static const float *mask_bits(const unsigned long long *bits) { return reinterpret_cast<const float *>(bits); }

extern "C" {

const char *decnet_version(void) { return "decnet_hip 0.1.0 gfx950"; }

size_t decnet_spamat_workspace_floats(int B, int C, int H, int W, int max_disp, int which) {
    return workspace_floats(B, C, H, W, max_disp, which);
}

// Each entry fills the record -- {mode / var, inputs, outputs, dims, (allow_compact, mbits,) stream}, nullptr for what the
// entry does not have -- and names itself (`which`) and its workspace.

int decnet_spamat_forward(const float *ref, const float *tar, const float *ref_mask,
                          const float *tar_mask, float *output, float *sum_similarities,
                          float *max_cost, int B, int C, int H, int W, int max_disp, void *stream) {
    return run_forward({MODE_MAT, ref, tar, ref_mask, tar_mask, nullptr, output, nullptr, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 0, Workspace::legacy());
}

int decnet_spamat_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                             float *output, float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                             int max_disp, float *workspace, size_t workspace_floats, void *stream) {
    return run_forward({MODE_MAT, ref, tar, ref_mask, tar_mask, nullptr, output, nullptr, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 0, Workspace{workspace, workspace_floats, true});
}

int decnet_spavar_forward(const float *ref, const float *tar, const float *ref_mask,
                          const float *tar_mask, const float *disparity, float *output,
                          float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                          int max_disp, void *stream) {
    return run_forward({MODE_VAR, ref, tar, ref_mask, tar_mask, disparity, nullptr, output, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 1, Workspace::legacy());
}

int decnet_spavar_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                             const float *disparity, float *output, float *sum_similarities, float *max_cost, int B,
                             int C, int H, int W, int max_disp, float *workspace, size_t workspace_floats, void *stream) {
    return run_forward({MODE_VAR, ref, tar, ref_mask, tar_mask, disparity, nullptr, output, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 1, Workspace{workspace, workspace_floats, true});
}

int decnet_spamatvar_forward(const float *ref, const float *tar, const float *ref_mask,
                             const float *tar_mask, float *output, float *variance,
                             float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                             int max_disp, void *stream) {
    return run_forward({MODE_FUSED, ref, tar, ref_mask, tar_mask, nullptr, output, variance, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 2, Workspace::legacy());
}

int decnet_spamatvar_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                                float *output, float *variance, float *sum_similarities, float *max_cost, int B, int C,
                                int H, int W, int max_disp, float *workspace, size_t workspace_floats, void *stream) {
    return run_forward({MODE_FUSED, ref, tar, ref_mask, tar_mask, nullptr, output, variance, sum_similarities, max_cost,
                        B, C, H, W, max_disp, 1, 0, (hipStream_t)stream}, 2, Workspace{workspace, workspace_floats, true});
}

int decnet_spamatvar_forward_bits(const float *ref, const float *tar, const unsigned long long *ref_bits,
                                  const unsigned long long *tar_bits, float *output, float *variance,
                                  float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                                  int max_disp, void *stream) {
    return run_forward({MODE_FUSED, ref, tar, mask_bits(ref_bits), mask_bits(tar_bits), nullptr, output, variance,
                        sum_similarities, max_cost, B, C, H, W, max_disp, 1, 1, (hipStream_t)stream}, 3, Workspace::legacy());
}

int decnet_spamatvar_forward_bits_ws(const float *ref, const float *tar, const unsigned long long *ref_bits,
                                     const unsigned long long *tar_bits, float *output, float *variance,
                                     float *sum_similarities, float *max_cost, int B, int C, int H, int W, int max_disp,
                                     float *workspace, size_t workspace_floats, void *stream) {
    return run_forward({MODE_FUSED, ref, tar, mask_bits(ref_bits), mask_bits(tar_bits), nullptr, output, variance,
                        sum_similarities, max_cost, B, C, H, W, max_disp, 1, 1, (hipStream_t)stream}, 3,
                       Workspace{workspace, workspace_floats, true});
}

int decnet_spamat_backward(const float *ref, const float *tar, const float *ref_mask,
                           const float *tar_mask, const float *output,
                           const float *sum_similarities, const float *max_cost,
                           const float *grad_output, float *grad_ref, float *grad_tar, int B, int C,
                           int H, int W, int max_disp, void *stream) {
    return run_backward({0, ref, tar, ref_mask, tar_mask, nullptr, output, sum_similarities, max_cost, grad_output,
                         grad_ref, grad_tar, nullptr, B, C, H, W, max_disp, (hipStream_t)stream}, 4, Workspace::legacy());
}

int decnet_spamat_backward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                              const float *output, const float *sum_similarities, const float *max_cost,
                              const float *grad_output, float *grad_ref, float *grad_tar, int B, int C, int H, int W,
                              int max_disp, float *workspace, size_t workspace_floats, void *stream) {
    return run_backward({0, ref, tar, ref_mask, tar_mask, nullptr, output, sum_similarities, max_cost, grad_output,
                         grad_ref, grad_tar, nullptr, B, C, H, W, max_disp, (hipStream_t)stream}, 4,
                        Workspace{workspace, workspace_floats, true});
}

int decnet_spavar_backward(const float *ref, const float *tar, const float *ref_mask,
                           const float *tar_mask, const float *disparity, const float *output,
                           const float *sum_similarities, const float *max_cost,
                           const float *grad_output, float *grad_ref, float *grad_tar,
                           float *grad_disparity, int B, int C, int H, int W, int max_disp,
                           void *stream) {
    return run_backward({1, ref, tar, ref_mask, tar_mask, disparity, output, sum_similarities, max_cost, grad_output,
                         grad_ref, grad_tar, grad_disparity, B, C, H, W, max_disp, (hipStream_t)stream}, 5,
                        Workspace::legacy());
}

int decnet_spavar_backward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                              const float *disparity, const float *output, const float *sum_similarities,
                              const float *max_cost, const float *grad_output, float *grad_ref, float *grad_tar,
                              float *grad_disparity, int B, int C, int H, int W, int max_disp, float *workspace,
                              size_t workspace_floats, void *stream) {
    return run_backward({1, ref, tar, ref_mask, tar_mask, disparity, output, sum_similarities, max_cost, grad_output,
                         grad_ref, grad_tar, grad_disparity, B, C, H, W, max_disp, (hipStream_t)stream}, 5,
                        Workspace{workspace, workspace_floats, true});
}

}  // extern "C"
