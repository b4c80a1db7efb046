// decnet_amd/csrc/spamat_host.h -- host side of the SpaMat / SpaVar family (capi.hip, spamat_mfma.hip,
// spamat_bwd_mfma.hip, spamat_wide.hip, spamat_rowtile.hip): the argument records one call carries from the C entry
// down to the kernel launch, and the one declaration of every function that crosses a file.  Internal: no part of
// include/decnet_hip.h.
#pragma once
#include <stddef.h>

#include <type_traits>

#include "common.h"

enum { MODE_MAT = 0, MODE_VAR = 1, MODE_FUSED = 2 };

// The band kernels hold at most 18 cost tiles, ceil((D - 1) / 16) + 1 of them: max_disp <= 273.  A wider range is cut
// into bands of at most 16 * 17 = 272 candidates (spamat_wide.hip), and capi.hip sends it there.
constexpr int SPAMAT_BAND_DISP = 272;

// One forward call.  mode MODE_MAT (out, sum_sim, max_cost), MODE_VAR (var_out, ...; `disparity` given), MODE_FUSED
// (out, var_out, ...); what a mode does not use is nullptr.  allow_compact = 0 pins the dense path (A/B benchmarks,
// tests).  mbits = 1: rmask / tmask point at bit-packed masks ([B,H,ceil(W/64)] 64-bit words, decnet_detail_mask's
// layout) instead of float planes.
struct SpaFwd {
    int mode;
    const float *ref, *tar, *rmask, *tmask, *disparity;
    float *out, *var_out, *sum_sim, *max_cost;
    int B, C, H, W, D;
    int allow_compact, mbits;
    hipStream_t stream;
};

// One backward call.  var: 0 SpaMat, 1 SpaVar (`disparity` given, grad_disp written; nullptr otherwise).
struct SpaBwd {
    int var;
    const float *ref, *tar, *rmask, *tmask, *disparity, *out, *sum_sim, *max_cost, *grad_out;
    float *grad_ref, *grad_tar, *grad_disp;
    int B, C, H, W, D;
    hipStream_t stream;
};

// Each returns DECNET_OK, DECNET_ERR_UNSUPPORTED (the dispatcher in capi.hip then tries the next one) or an error.
// spamat_mfma.hip / spamat_bwd_mfma.hip: banded cost tiles on the matrix cores, D <= SPAMAT_BAND_DISP + 1
int decnet_mfma_forward(const SpaFwd &a);
int decnet_mfma_backward(const SpaBwd &a);
// spamat_rowtile.hip: the VALU row-tile kernels and their global-memory last resort (float masks only)
int decnet_rowtile_forward(const SpaFwd &a);
int decnet_rowtile_backward(const SpaBwd &a);
// spamat_wide.hip: D > SPAMAT_BAND_DISP as several band-kernel calls + per-pixel merges.  ws: the caller's workspace of
// decnet_wide_workspace_floats floats (the `_ws` entries), or nullptr (the legacy entries: the sweep allocates its
// scratch, and is UNSUPPORTED while the stream is being captured)
int decnet_wide_forward(const SpaFwd &a, float *ws);
int decnet_wide_backward(const SpaBwd &a, float *ws);
size_t decnet_wide_workspace_floats(int B, int C, int H, int W, int D, int which);

// A runtime mode / flag as a compile-time constant: f(std::integral_constant<...>{}) of the value, for the template
// argument of a kernel (decltype(M)::value, or M() in a constant expression).
template <class F>
int spamat_with_mode(int mode, F &&f) {
    if (mode == MODE_MAT) return f(std::integral_constant<int, MODE_MAT>{});
    if (mode == MODE_VAR) return f(std::integral_constant<int, MODE_VAR>{});
    return f(std::integral_constant<int, MODE_FUSED>{});
}
template <class F>
int spamat_with_flag(bool flag, F &&f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
