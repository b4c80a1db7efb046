/*
 * include/decnet_hip.h -- C ABI of libdecnet_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for DecNet's data-parallel hot path.  Every entry point takes
 * plain device pointers, sizes and a hipStream_t passed as void*; no torch types.
 * Each one names the reference interface (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - All tensors are fp32, dense, row-major in the layout stated per argument.
 *     Feature maps are NCHW, masks / per-pixel planes are N,H,W  (functions/SpaMat.py:13-16).
 *   - Device pointers must be valid on the device that is current when the call is made;
 *     work is enqueued on `stream` (NULL = the null stream) and the call returns
 *     immediately (asynchronous, like the reference's launches SM_kernel.cu:384-386).
 *   - Re-entrant: no global mutable state; safe to call from one host thread per GPU
 *     (the reference is driven that way by DataParallel, eval.py:146).
 *   - Outputs are fully written by the callee (entries the reference leaves to the
 *     caller's zero fill, functions/SpaMat.py:25-27,42-43, are written as 0), so the
 *     caller does not have to clear them.  Inputs are never modified.
 *   - Inputs must be finite.  The reference propagates a NaN feature into every output it
 *     touches (fmaxf/expf on NaN, SM_kernel.cu:46-58); the SpaMat/SpaVar forward kernels here
 *     are built with -fno-honor-nans (decnet_amd/build.py), so a NaN input gives an unspecified
 *     value at the pixels whose candidate set contains it -- never a fault, never an effect on
 *     other pixels.  DECNET_CHECK_FINITE=1 (environment, read once) makes every SpaMat/SpaVar forward entry
 *     sweep both feature maps first (one reduction kernel each, then a 4-byte read-back: the call
 *     waits for the stream) and return DECNET_ERR_NONFINITE with nothing else launched; the check is
 *     skipped while the stream is being captured into a graph.
 *   - Return value: 0 (DECNET_OK) on success, a negative DECNET_ERR_* for rejected
 *     arguments (nothing is enqueued), or a positive hipError_t from the launch.
 *     (The reference's pybind functions always return 1 and check nothing,
 *     SM_cuda.cpp:7-27; the Python shim in decnet_amd/ext.py restores that `1`.)
 */
#ifndef DECNET_HIP_H
#define DECNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DECNET_OK 0
#define DECNET_ERR_NULL_POINTER (-1)
#define DECNET_ERR_BAD_SHAPE (-2)     /* non-positive dim, max_disp < 1, index space > 2^31 */
#define DECNET_ERR_UNSUPPORTED (-3)   /* shape does not fit the kernels' LDS tiling */
#define DECNET_ERR_NONFINITE (-4)     /* DECNET_CHECK_FINITE=1 and a feature map holds a NaN / Inf (nothing launched) */
#define DECNET_ERR_MISALIGNED (-5)    /* a library-format buffer (stated per entry) is not 16-byte aligned */

/* Library / build identification: "decnet_hip <version> gfx950". */
const char *decnet_version(void);

/* ---------------------------------------------------------------------------------------
 * SpaMat forward.  Replaces sparse_matching_cuda_forward (SM_cuda.cpp:7-15), i.e. the two
 * launches get_max_cost + sparse_matching_forward (SM_kernel.cu:22-60, 76-125, 359-387).
 *   ref, tar            [B,C,H,W]  left / right feature maps
 *   ref_mask, tar_mask  [B,H,W]    0 = off, anything else = on
 *   output              [B,H,W]    soft-argmax disparity   (0 where ref_mask == 0)
 *   sum_similarities    [B,H,W]    1e-6 + sum_d exp(cost_d - max_cost)
 *   max_cost            [B,H,W]    max(1e-6, max_d cost_d)
 *   max_disp            candidates d in [0, min(max_disp, x+1))
 * ------------------------------------------------------------------------------------- */
int decnet_spamat_forward(const float *ref, const float *tar, const float *ref_mask,
                          const float *tar_mask, float *output, float *sum_similarities,
                          float *max_cost, int B, int C, int H, int W, int max_disp,
                          void *stream);

/* SpaMat backward.  Replaces sparse_matching_cuda_backward (SM_cuda.cpp:17-27): the launches
 * sparse_matching_ref_backward + sparse_matching_tar_backward (SM_kernel.cu:143-195, 300-355,
 * 389-429).  grad_ref / grad_tar [B,C,H,W] are fully written.                              */
int decnet_spamat_backward(const float *ref, const float *tar, const float *ref_mask,
                           const float *tar_mask, const float *output,
                           const float *sum_similarities, const float *max_cost,
                           const float *grad_output, float *grad_ref, float *grad_tar,
                           int B, int C, int H, int W, int max_disp, void *stream);

/* SpaVar forward.  Replaces sparse_var_cuda_forward (SV_cuda.cpp:7-17; kernels
 * SV_kernel.cu:22-60, 76-124, 329-359): output = (1e-6 + sum_d e_d (d - disparity)^2) / S. */
int decnet_spavar_forward(const float *ref, const float *tar, const float *ref_mask,
                          const float *tar_mask, const float *disparity, float *output,
                          float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                          int max_disp, void *stream);

/* SpaVar backward.  Replaces sparse_var_cuda_backward (SV_cuda.cpp:19-32; kernels
 * SV_kernel.cu:142-325, 361-410).  grad_disparity [B,H,W].                                */
int decnet_spavar_backward(const float *ref, const float *tar, const float *ref_mask,
                           const float *tar_mask, const float *disparity, const float *output,
                           const float *sum_similarities, const float *max_cost,
                           const float *grad_output, float *grad_ref, float *grad_tar,
                           float *grad_disparity, int B, int C, int H, int W, int max_disp,
                           void *stream);

/* Fused SpaMat + SpaVar forward for the only way the model uses SpaVar
 * (SparseDenseNetRefinementMask.py:183-192: same features and masks, disparity = SpaMat's
 * output, under no_grad).  One read of ref/tar instead of four.
 *   output, variance, sum_similarities, max_cost   [B,H,W]                                 */
int decnet_spamatvar_forward(const float *ref, const float *tar, const float *ref_mask,
                             const float *tar_mask, float *output, float *variance,
                             float *sum_similarities, float *max_cost, int B, int C, int H,
                             int W, int max_disp, void *stream);
/* decnet_spamatvar_forward with bit-packed masks: ref_bits / tar_bits [B,H,ceil(W/64)] 64-bit words, bit i of word w
 * of a row = pixel 64 w + i, zero past W (what decnet_detail_mask writes beside the float plane of the reference's
 * contract).  Same results as the float-mask call; 8 of the pass's 88 bytes per pixel (C = 8) are not read.
 * Above max_disp 273 (the 18 tiles of one band) the range is done in bands of <= 272 with the masks unpacked into scratch planes (stream-ordered
 * allocation); DECNET_ERR_UNSUPPORTED there only while `stream` is being captured into a graph (this entry allocates; its
 * caller-workspace twin decnet_spamatvar_forward_bits_ws below does not and runs under capture). */
int decnet_spamatvar_forward_bits(const float *ref, const float *tar, const unsigned long long *ref_bits,
                                  const unsigned long long *tar_bits, float *output, float *variance,
                                  float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                                  int max_disp, void *stream);

/* ---------------------------------------------------------------------------------------
 * SpaMat / SpaVar with a caller workspace: the six entries above for disparity ranges wider than one band of the
 * matrix-core kernels (max_disp > 273; the reference's demo data runs stage 3 at 405 and 621, demo.py:149-155), without
 * memory of the library's own.  Above 273 candidates the range is swept in nb = ceil(max_disp / 272) bands of
 * ceil(max_disp / nb) candidates, merged per pixel.  The six entries above take that sweep's scratch from the
 * stream-ordered allocator and therefore decline while `stream` is being captured into a graph (the float-mask entries
 * then run the row-tile kernels, the bit-mask entry returns DECNET_ERR_UNSUPPORTED); the `_ws` entries take it from the
 * caller, never ask whether the stream is capturing, and reach no allocation, synchronisation or host read-back on that
 * path (DECNET_CHECK_FINITE=1 keeps its own, and stays skipped under capture).
 *   decnet_spamat_workspace_floats(B, C, H, W, max_disp, which)
 *       which: 0 spamat_forward, 1 spavar_forward, 2 spamatvar_forward, 3 spamatvar_forward_bits, 4 spamat_backward,
 *              5 spavar_backward
 *       A pure host function (no HIP call).  0 for every shape one band takes (max_disp <= 273), for bad shapes and for
 *       an unknown `which`; otherwise the floats the sweep of that entry needs, in planes of B H W floats:
 *       C + 4 (which 0), C + 5 (1, 2), C + 6 (3: the unpacked left mask), 3 C + 2 (4), 3 C + 3 (5).
 *   workspace, workspace_floats   device scratch and its size in floats
 *       query == 0: `workspace` may be NULL and the call IS the entry above (same dispatch, same results).
 *       query  > 0: workspace == NULL -> DECNET_ERR_NULL_POINTER; workspace_floats < query -> DECNET_ERR_BAD_SHAPE;
 *       workspace not 16-byte aligned -> DECNET_ERR_MISALIGNED; in all three nothing is launched and no output is
 *       touched.  Nothing outside workspace[0 .. query) is written; its contents are garbage before and after a call.
 * Everything else (arguments, dispatch, DECNET_SPAMAT_KERNEL, DECNET_CHECK_FINITE, return values) is that of the entry
 * above; under DECNET_SPAMAT_KERNEL=rowtile the workspace is checked and then unused.  The band kernels, the band split
 * and the merge order are the same, and no kernel has floating-point atomics: called eagerly, a `_ws` entry returns
 * bit for bit what the entry above returns.
 * ------------------------------------------------------------------------------------- */
size_t decnet_spamat_workspace_floats(int B, int C, int H, int W, int max_disp, int which);
int decnet_spamat_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                             float *output, float *sum_similarities, float *max_cost, int B, int C, int H, int W,
                             int max_disp, float *workspace, size_t workspace_floats, void *stream);
int decnet_spamat_backward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                              const float *output, const float *sum_similarities, const float *max_cost,
                              const float *grad_output, float *grad_ref, float *grad_tar, int B, int C, int H, int W,
                              int max_disp, float *workspace, size_t workspace_floats, void *stream);
int decnet_spavar_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                             const float *disparity, float *output, float *sum_similarities, float *max_cost, int B,
                             int C, int H, int W, int max_disp, float *workspace, size_t workspace_floats, void *stream);
int decnet_spavar_backward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                              const float *disparity, const float *output, const float *sum_similarities,
                              const float *max_cost, const float *grad_output, float *grad_ref, float *grad_tar,
                              float *grad_disparity, int B, int C, int H, int W, int max_disp, float *workspace,
                              size_t workspace_floats, void *stream);
int decnet_spamatvar_forward_ws(const float *ref, const float *tar, const float *ref_mask, const float *tar_mask,
                                float *output, float *variance, float *sum_similarities, float *max_cost, int B, int C,
                                int H, int W, int max_disp, float *workspace, size_t workspace_floats, void *stream);
int decnet_spamatvar_forward_bits_ws(const float *ref, const float *tar, const unsigned long long *ref_bits,
                                     const unsigned long long *tar_bits, float *output, float *variance,
                                     float *sum_similarities, float *max_cost, int B, int C, int H, int W, int max_disp,
                                     float *workspace, size_t workspace_floats, void *stream);

/* ---------------------------------------------------------------------------------------
 * Stage 0 (coarsest level): dense cost volume -> 3-D conv aggregation -> soft-argmax.
 * Internal activation layout is channels-last  [B, D, H, W, C]  ("NDHWC").
 * ------------------------------------------------------------------------------------- */

/* Cost volume, cost_func="cor", warp_ope="homgrp" with disp_samples = arange(D)
 * (get_disp_samples submodule.py:389-390; GetCostVolume submodule.py:479-522, 532-562):
 *   cost[b,d,y,x,c] = (x >= d ? left[b,c,y,x] : 0) * bilinear(right[b,c]; xs, ys)
 *   xs = (x-d)*W/(W-1) - 0.5,  ys = y*H/(H-1) - 0.5, zero padding   (grid_sample with
 *   align_corners=False on align_corners=True-normalised coordinates).
 *   left,right [B,C,H,W];  cost_ndhwc [B,D,H,W,C].                                         */
int decnet_costvol_forward(const float *left, const float *right, float *cost_ndhwc, int B,
                           int C, int H, int W, int D, void *stream);
/* The other cost functions of GetCostVolume (submodule.py:511-530, chosen by --cost_func, demo.py:31 / eval.py:43), with
 * l = (x >= d ? left[b,c,y,x] : 0) and r = bilinear(right[b,c]; ...) as above:
 *   DECNET_COST_COR  l * r                               (:518-522; what decnet_costvol_forward computes)
 *   DECNET_COST_SSD  (l^2 + r^2) / 2 - ((l + r) / 2)^2   (:524-530, the same fp32 operation sequence)
 *   DECNET_COST_CAT  cost[..., c] = l, cost[..., C + c] = r: cost_ndhwc is [B,D,H,W,2C]   (:512-516)
 *   DECNET_COST_SUM  l + r -- not a reference function: CostRegNetNoDown.conv_pre (the 1x1x1 convolution behind the
 *                    "cat" volume, :618-619) is linear, so conv_pre(cat(l_vol, r_vol)) is the SUM volume of the two
 *                    feature maps after each went through its half of conv_pre (decnet_stage0_forward_cf does that). */
#define DECNET_COST_COR 0
#define DECNET_COST_SSD 1
#define DECNET_COST_CAT 2
#define DECNET_COST_SUM 3
int decnet_costvol_forward_cf(const float *left, const float *right, float *cost_ndhwc, int B,
                              int C, int H, int W, int D, int cost_func, void *stream);
/* Conv3d with kernel 1, stride 1, no bias (CostRegNetNoDown.conv_pre, submodule.py:618-619, 651-652):
 *   y[b,co,p] = sum_ci w[co*ldw + ci] * x[b,ci,p],  p < P positions per sample, one fp32 fma chain in channel order;
 *   channels_last = 0: x [B,Ci,P], y [B,Co,P] (NCHW / NCDHW);  1: x [B,P,Ci], y [B,P,Co] (the NDHWC volumes above).
 *   ldw >= Ci: row pitch of w (2C when one half of conv_pre.weight [C,2C,1,1,1] is applied to one feature map). */
int decnet_conv3d_pointwise(const float *x, const float *w, float *y, int B, int Ci, int Co, int P, int ldw,
                            int channels_last, void *stream);

/* Repack one Conv3d weight  [Co,Ci,3,3,3] (torch layout, submodule.py:109) into the kernels'
 * [27, Ci, CoP] layout, CoP = decnet_conv3d_packed_cout(Co), zero padded.  w_packed is a library-format buffer read in
 * 16-byte units: 16-byte aligned, else decnet_conv3d_pack_weight and decnet_conv3d_bn_act return DECNET_ERR_MISALIGNED
 * (nothing launched).                                                                       */
int decnet_conv3d_packed_cout(int Co);
int decnet_conv3d_pack_weight(const float *w_oidhw, float *w_packed, int Co, int Ci,
                              void *stream);

/* One Conv3dUnit in eval mode (submodule.py:115-123: Conv3d k3 s1 p1 no bias ->
 * BatchNorm3d(running stats) -> ReLU), channels-last in and out:
 *   y = act(conv(x) * scale[co] + shift[co]) (+ residual)
 *   scale = gamma / sqrt(var + eps),  shift = beta - mean * scale   (caller folds BN)
 *   x [B,D,H,W,Ci];  w_packed from decnet_conv3d_pack_weight;  y [B,D,H,W,Co];
 *   residual: NULL or [B,D,H,W,Co], added after the activation (CostRegNetNoDown.forward
 *   submodule.py:656: conv1(o0) + o0);  relu: 0/1.                                         */
int decnet_conv3d_bn_act(const float *x, const float *w_packed, const float *scale,
                         const float *shift, const float *residual, float *y, int B, int D,
                         int H, int W, int Ci, int Co, int relu, void *stream);

/* The same Conv3dUnit by Winograd minimal filtering in fp32 (differs from decnet_conv3d_bn_act by
 * fp32 rounding only).  variant 0: F(2,3) on D,H,W -- 64 transform points, 8 multiplies per output
 * instead of 27, ~1e-6 relative;  variant 1: F(2,3) on D, F(4,3) on H and W -- 144 points, 4.5
 * multiplies per output, ~2e-6 relative;  variant 2: F(4,3) on D, H and W -- 216 points, 3.4 multiplies
 * per output, ~4e-6 relative (F(4,3) on the points {0, +-3/4, +-3/2, inf}).
 *   u          weights transformed once by decnet_conv3d_wino_pack_weight:
 *              [Co,Ci,3,3,3] -> U^T [points][ceil(Ci/16)][224][16]
 *              (decnet_conv3d_wino_weight_floats floats)
 *   workspace  decnet_conv3d_wino_workspace_floats(...) floats of device scratch
 *   everything else as decnet_conv3d_bn_act.
 * u, workspace and the V / M of decnet_conv3d_wino_gemm are library-format buffers moved in 16-byte units: 16-byte
 * aligned, else DECNET_ERR_MISALIGNED (nothing launched; the stack entries below check every u[i] and their workspace
 * too).  x, y, residual, scale and shift may be any dense fp32 pointer.                    */
size_t decnet_conv3d_wino_weight_floats(int Ci, int variant);
int decnet_conv3d_wino_pack_weight(const float *w_oidhw, float *u, int Co, int Ci, int variant,
                                   void *stream);
size_t decnet_conv3d_wino_workspace_floats(int B, int D, int H, int W, int Ci, int Co, int variant);
/* its GEMM stage alone: M[xi] = V[xi] * U[xi] for every transform point xi, 16 channels (64 bytes)
 * being the unit of all three layouts:
 *   V [points][ceil(Ci/16)][nt][16] (transformed input tiles), M [points][ceil(Co/16)][nt][16].
 * In place: M == V is accepted exactly when the bf16x3 kernel runs (Ci = 216, DECNET_WINO_GEMM unset or bf16x3) and
 * Ci == Co, so that V and M are one layout; the result is bit for bit that of the two-buffer call.  Every other overlap
 * of the two ranges (M inside V's range but not equal to it, Ci != Co, the fp32 kernels) returns
 * DECNET_ERR_UNSUPPORTED with nothing launched. */
int decnet_conv3d_wino_gemm(const float *V, const float *u, float *M, int nt, int Ci, int Co,
                            int variant, void *stream);
int decnet_conv3d_wino_bn_act(const float *x, const float *u, const float *scale,
                              const float *shift, const float *residual, float *y,
                              float *workspace, int B, int D, int H, int W, int Ci, int Co,
                              int relu, int variant, void *stream);

/* A stack of n_layers >= 2 consecutive C -> C Conv3dUnits (submodule.py:115-123) with the activations between the
 * layers kept on chip: one kernel does the output transform of layer i (BN, ReLU, residual) into LDS and the input
 * transform of layer i + 1 out of it.  u / scale / shift: per-layer pointers as for decnet_conv3d_wino_bn_act.
 * res_src, res_dst: the output of layer res_src is added to the output of layer res_dst after its ReLU
 * (CostRegNetNoDown.forward submodule.py:653-658: 1 and 4), or -1, -1; needs res_src < res_dst < n_layers - 1.
 * DECNET_ERR_UNSUPPORTED (nothing launched; decnet_conv3d_wino_stack_workspace_floats returns 0) when the fused
 * kernels do not cover the shape: variant 2, C = 216, one sample x 4 channels of the volume <= 160 KB of LDS. */
size_t decnet_conv3d_wino_stack_workspace_floats(int B, int D, int H, int W, int C, int variant);
int decnet_conv3d_wino_stack_bn_act(const float *x, const float *const *u, const float *const *scale,
                                    const float *const *shift, int n_layers, int res_src, int res_dst, float *y,
                                    float *workspace, int B, int D, int H, int W, int C, int variant, void *stream);
/* The same stack fed by the stage-0 cost volume of (left, right) [B,C,H,W] -- the values decnet_costvol_forward writes
 * (GetCostVolume, submodule.py:479-522), D disparity planes -- without that volume ever reaching HBM: the first layer's
 * input transform is formed on chip from the two feature maps.  Workspace as above.  DECNET_ERR_UNSUPPORTED (nothing
 * launched) where decnet_conv3d_wino_stack_bn_act is, or when the feature planes do not fit in LDS beside the volume. */
int decnet_costvol_wino_stack_bn_act(const float *left, const float *right, const float *const *u,
                                     const float *const *scale, const float *const *shift, int n_layers, int res_src,
                                     int res_dst, float *y, float *workspace, int B, int C, int H, int W, int D,
                                     int variant, void *stream);
/* ... with the cost function DECNET_COST_COR / _SSD / _SUM (DECNET_ERR_BAD_SHAPE for _CAT: see decnet_stage0_forward_cf). */
int decnet_costvol_wino_stack_bn_act_cf(const float *left, const float *right, const float *const *u,
                                        const float *const *scale, const float *const *shift, int n_layers, int res_src,
                                        int res_dst, float *y, float *workspace, int B, int C, int H, int W, int D,
                                        int variant, int cost_func, void *stream);
/* Last Conv3dUnit (Ci -> 1, BN, no ReLU; submodule.py:641) fused with disparity_regression
 * over disp_samples = arange(D) (submodule.py:766-777):
 *   reg[b,d,y,x]  = conv(x)[b,d,y,x] * scale + shift        (optional output, may be NULL)
 *   pred[b,y,x]   = sum_d softmax_d(reg)[d] * d
 *   x [B,D,H,W,Ci];  w [1,Ci,3,3,3] torch layout (no repack needed).                       */
int decnet_conv3d_cout1_softargmax(const float *x, const float *w_oidhw, float scale,
                                   float shift, float *reg, float *pred, int B, int D, int H,
                                   int W, int Ci, void *stream);

/* The same operator in two passes (a [positions x Ci] x [Ci x 27] product on the matrix cores, then
 * a 27-tap gather + soft-argmax) that read x once instead of 27 times.  workspace:
 * decnet_conv3d_cout1_workspace_floats(B,D,H,W) floats of device scratch, 16-byte aligned (else DECNET_ERR_MISALIGNED,
 * nothing launched).  Ci <= 256, D <= 256. */
size_t decnet_conv3d_cout1_workspace_floats(int B, int D, int H, int W);
int decnet_conv3d_cout1_softargmax_ws(const float *x, const float *w_oidhw, float scale,
                                      float shift, float *reg, float *pred, float *workspace,
                                      int B, int D, int H, int W, int Ci, void *stream);

/* ---------------------------------------------------------------------------------------
 * The whole stage-0 branch in one call: replaces SparseDenseNetRefinementMask.forward :127-137, i.e.
 * get_disp_samples (submodule.py:389-390) -> GetCostVolume.forward (:532-562) ->
 * CostRegNetNoDown.forward (:650-662) -> disparity_regression (:766-777) for the shipped configuration
 * (cost_func="cor", warp_ope="homgrp", 8 Conv3dUnits C -> C ... C -> 1).
 *   left, right [B,C,H,W] feature maps of the coarsest level;  D = max_disp / 27 hypotheses 0 .. D-1
 *   params      the seven C -> C layers: w[i] = decnet_conv3d_wino_pack_weight(...) of the layer for
 *               variant 0..2 (decnet_conv3d_pack_weight for variant 3 = direct 27-tap GEMM), scale / shift =
 *               folded BatchNorm3d [C]; the last layer: w_last [1,C,3,3,3] (torch layout), scale_last, shift_last
 *   variant     -1 = automatic (F(4,3)^3 where depth tiles of 4 pay, else F(2,3)xF(4,3)^2), else as above
 *   workspace   decnet_stage0_workspace_floats(B,C,H,W,D,variant) floats of device scratch (cost volume,
 *               three ping-pong activation buffers, the Winograd intermediates); contents are scratch.  Any
 *               float alignment: the entry starts its buffers at the first 16-byte boundary inside it.
 *               The seven packed w[i] must be 16-byte aligned, else DECNET_ERR_MISALIGNED
 *               (nothing launched; decnet_stage0_forward_cf too)
 *   reg         NULL or [B,D,H,W]: the regularised volume (what CostRegNetNoDown returns)
 *   pred        [B,H,W]: the stage-0 disparity
 * C must be a multiple of 4 (pad features and weights with zero channels otherwise).             */
typedef struct decnet_stage0_params {
    const float *w[7];
    const float *scale[7];
    const float *shift[7];
    const float *w_last;
    float scale_last, shift_last;
} decnet_stage0_params;
size_t decnet_stage0_workspace_floats(int B, int C, int H, int W, int D, int variant);
int decnet_stage0_forward(const float *left, const float *right, const decnet_stage0_params *params,
                          float *workspace, float *reg, float *pred, int B, int C, int H, int W, int D,
                          int variant, void *stream);
/* The same branch for every --cost_func of the reference (submodule.py:552-560): cost_func = DECNET_COST_COR, _SSD or
 * _CAT.  w_pre: CostRegNetNoDown.conv_pre.weight [C,2C,1,1,1] (torch layout) for _CAT, ignored (may be NULL) otherwise.
 * _CAT never forms the 2C-channel volume: conv_pre is applied to the two feature maps (its left half to `left`, its right
 * half to `right`: two [C x C] products over B*H*W pixels instead of one [C x 2C] over B*D*H*W voxels -- bilinear warping
 * and the left mask commute with a per-pixel linear map) and the stack runs on their DECNET_COST_SUM volume.
 * Workspace: decnet_stage0_cf_workspace_floats floats. */
size_t decnet_stage0_cf_workspace_floats(int B, int C, int H, int W, int D, int variant, int cost_func);
int decnet_stage0_forward_cf(const float *left, const float *right, const decnet_stage0_params *params,
                             const float *w_pre, float *workspace, float *reg, float *pred, int B, int C, int H, int W,
                             int D, int variant, int cost_func, void *stream);

/* disparity_regression for arbitrary samples (submodule.py:766-777):
 *   cost, samples [B,S,H,W] -> pred [B,H,W]                                                */
int decnet_disparity_regression(const float *cost, const float *samples, float *pred, int B,
                                int S, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * 2-D trunk: the full-resolution, few-channel Conv2dUnit / Deconv2dUnit layers
 * (modules/submodule.py:15-87) in eval mode, conv -> BatchNorm2d(running stats) -> ReLU fused:
 *   y = act(conv(x) * scale[co] + shift[co]);  x [B,Cin,H,W], y [B,Cout,H',W'] NCHW;
 *   scale/shift: folded BN (or 1 / bias when the unit has no BN).  Cout <= 24 (<= 8 for the
 *   transposed convolution).
 * Weights are repacked once by decnet_conv2d_pack_weight into decnet_conv2d_packed_floats(...)
 * floats: torch [Cout,Cin,k,k] (transposed = 0) or ConvTranspose2d [Cin,Cout,3,3] (transposed = 1)
 * -> [Cin][k][k][co padded].
 * decnet_conv2d_bn_act: k = 1 or 3, stride 1, padding dilation*(k/2) (output size = input size).
 * decnet_deconv2d_k3s3_bn_act: ConvTranspose2d k = 3, stride 3, padding 0 (output 3H x 3W;
 *   submodule.py:162-178 Deconv2dBlock, GenerateSparseMask).
 * ------------------------------------------------------------------------------------- */
size_t decnet_conv2d_packed_floats(int Cin, int Cout, int k, int transposed);   /* 0: unsupported */
int decnet_conv2d_pack_weight(const float *w, float *w_packed, int Cin, int Cout, int k,
                              int transposed, void *stream);
int decnet_conv2d_bn_act(const float *x, const float *w_packed, const float *scale,
                         const float *shift, float *y, int B, int Cin, int Cout, int H, int W, int k, int dilation,
                         int relu, void *stream);
/* decnet_conv2d_bn_act on the channel concatenation of nseg (<= 6) tensors xs[i] [B,cins[i],H,W]
 * (host arrays of device pointers / channel counts; weights packed for Cin = sum of cins): the
 * torch.cat in front of the Deconv2dBlock / Refinement / SoftAttention convolutions
 * (submodule.py:176, 755, SparseDenseNetRefinementMask.py:195-199) is never materialised. */
int decnet_conv2d_cat_bn_act(const float *const *xs, const int *cins, int nseg, const float *w_packed,
                             const float *scale, const float *shift, float *y, int B, int Cout, int H,
                             int W, int k, int dilation, int relu, void *stream);
/* decnet_conv2d_cat_bn_act for a layer with ONE output channel, with the elementwise tail of its caller fused
 * (ea, eb: [B,H,W] planes; y [B,1,H,W]):
 *   epilogue 1  SoftAttention's last layer + the fusion of the stage loop (submodule.py:593-604,
 *               SparseDenseNetRefinementMask.py:195-202): s = sigmoid(conv), y = ea (1 - s) + s eb   (ea dense, eb sparse)
 *   epilogue 2  Refinement's last layer + residual (submodule.py:716): y = ea + conv                             */
int decnet_conv2d_cat_epilogue(const float *const *xs, const int *cins, int nseg, const float *w_packed,
                               const float *scale, const float *shift, float *y, int B, int H, int W, int k,
                               int dilation, int relu, int epilogue, const float *ea, const float *eb, void *stream);
/* The many-channel stride-1 Conv2dUnit layers (FeatureExtraction conv1-conv3_2 and the Deconv2dBlock convolutions
 * submodule.py:245-343, 162-178; DynamicUpsampling.weight_learning :566-577; Refinement :690-717) on the bf16
 * matrix cores at fp32 accuracy (each fp32 operand split into three bf16 terms, six partial products): k = 1 or 3,
 * stride 1, padding dilation*(k/2), any Cin / Cout, input = channel concatenation of nseg (<= 6) tensors.
 * Weights: torch [Cout,Cin,k,k] packed once into decnet_conv2d_mfma_packed_bytes(...) bytes (0: unsupported), a
 * library-format buffer read in 16-byte units: 16-byte aligned, else DECNET_ERR_MISALIGNED (nothing launched; this holds
 * for decnet_deconv2d_mfma_* below too).  k = 3 takes dilation <= 6: above that the halo tile of a workgroup does not
 * fit the staging loop, and the call returns DECNET_ERR_UNSUPPORTED with nothing launched. */
size_t decnet_conv2d_mfma_packed_bytes(int Cin, int Cout, int k);
int decnet_conv2d_mfma_pack_weight(const float *w, void *w_packed, int Cin, int Cout, int k, void *stream);
int decnet_conv2d_mfma_cat_bn_act(const float *const *xs, const int *cins, int nseg, const void *w_packed,
                                  const float *scale, const float *shift, float *y, int B, int Cout, int H,
                                  int W, int k, int dilation, int relu, void *stream);
/* Deconv2dUnit (ConvTranspose2d k = 3, stride 3, padding 0 + BN + ReLU, submodule.py:48-87; FeatureExtraction's
 * deconv2 / deconv3 at 24 / 72 output channels) on the same kernels: every input pixel owns its 3 x 3 output block, so
 * the layer is the 1 x 1 convolution to 9 Cout channels with a pixel-shuffle store.  w: torch [Cin,Cout,3,3];
 * x [B,Cin,H,W] -> y [B,Cout,3H,3W]. */
size_t decnet_deconv2d_mfma_packed_bytes(int Cin, int Cout);
int decnet_deconv2d_mfma_pack_weight(const float *w, void *w_packed, int Cin, int Cout, void *stream);
int decnet_deconv2d_mfma_k3s3_bn_act(const float *x, const void *w_packed, const float *scale, const float *shift,
                                     float *y, int B, int Cin, int Cout, int H, int W, int relu, void *stream);
/* Weight gradient of decnet_conv2d_cat_bn_act with frozen BatchNorm (csrc/conv2d_grad.hip): for
 * y = act(conv(x, w) * scale + shift) and the upstream gradient gy, gm = gy * [y > 0] (gm = gy without ReLU: y NULL) and
 *   G[co][ci][ky][kx] = sum_{b,y,x} gm[b][co][y][x] * x[b][ci][y + (ky - k/2) d][x + (kx - k/2) d]   (zeros outside)
 *   gsum[co]          = sum_{b,y,x} gm[b][co][y][x]
 * so that dW = scale * G, dscale = <w, G>, dshift = gsum; dx is decnet_conv2d_bn_act itself on gm with the weights
 * w'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] * scale[co].
 *   xs, cins, nseg   the input as for decnet_conv2d_cat_bn_act (Cin = sum of cins <= 24)
 *   gy, y            [B,Cout,H,W]; y: the layer's OUTPUT (read only as the mask y > 0), NULL for a layer without ReLU
 *   gm               [B,Cout,H,W], written in full; may be NULL when y is NULL
 *   G, gsum          [Cout,Cin,k,k], [Cout], written in full
 *   workspace        decnet_conv2d_wgrad_workspace_floats(B, Cin, Cout, H, W, k) floats (0: shape not covered), 16-byte
 *                    aligned (else DECNET_ERR_MISALIGNED); fewer floats than the query: DECNET_ERR_BAD_SHAPE
 * Every other buffer is accepted at any float alignment.  Deterministic: workgroups write partial sums (fp32 chains of at
 * most 512 terms) into the workspace, a second launch adds them in a fixed order in float64 and rounds once; no atomics,
 * no allocation, no synchronisation (capturable).  DECNET_ERR_UNSUPPORTED: k not 1 or 3, Cout > 24, Cin > 24, nseg > 6,
 * H or B > 65535, W > 2^28.  Nothing is launched on any refusal. */
size_t decnet_conv2d_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W, int k);
int decnet_conv2d_wgrad(const float *const *xs, const int *cins, int nseg, const float *gy, const float *y, float *gm,
                        float *G, float *gsum, float *workspace, size_t workspace_floats, int B, int Cout, int H,
                        int W, int k, int dilation, void *stream);
/* Weight gradient of decnet_conv2d_mfma_cat_bn_act with frozen BatchNorm (csrc/conv2d_mfma_grad.hip): the meaning of
 * decnet_conv2d_wgrad, argument for argument, for the many-channel layers -- gm = gy * [y > 0] (written in full; y NULL:
 * no ReLU, gm may be NULL and is gy), G[co][ci][ky][kx] = sum gm * x(tap) with zeros outside the image at any
 * dilation >= 1, gsum[co] = sum gm; G and gsum written in full.  dx is decnet_conv2d_mfma_cat_bn_act itself on gm with
 * the weights w'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx] * scale[co].
 *   xs, cins, nseg   the input as for decnet_conv2d_mfma_cat_bn_act (nseg <= 6, Cin = sum of cins <= 224, any split)
 *   Cout             <= 224; k 1 or 3; B, H <= 65535; H * W < 2^29 (a plane is addressed by a 32-bit byte offset)
 *   workspace        decnet_conv2d_mfma_wgrad_workspace_floats(B, Cin, Cout, H, W, k) floats (0: shape not covered),
 *                    16-byte aligned (else DECNET_ERR_MISALIGNED); fewer floats than the query: DECNET_ERR_BAD_SHAPE
 * Every other buffer is accepted at any float alignment, W at any value.  The GEMM [Cout x pixels] . [pixels x (Cin k k + 1)]
 * runs on v_mfma_f32_16x16x4_f32 (an fp32 fma chain; no bf16 split).  Deterministic: partition and order are functions of
 * the shape alone; workgroups write partial sums (fp32 chains of at most 4096 terms: 64 pixels x at most 64 chunks) into
 * the workspace, a last launch adds them in a fixed order in float64 and rounds once; no atomics, no allocation, no
 * synchronisation (capturable).  NULL (also y without gm): DECNET_ERR_NULL_POINTER; k not 1 or 3, Cout > 224, Cin > 224,
 * nseg > 6, H or B > 65535, H * W >= 2^29: DECNET_ERR_UNSUPPORTED.  Nothing is launched on any refusal. */
size_t decnet_conv2d_mfma_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W, int k);
int decnet_conv2d_mfma_wgrad(const float *const *xs, const int *cins, int nseg, const float *gy, const float *y,
                             float *gm, float *G, float *gsum, float *workspace, size_t workspace_floats, int B, int Cout,
                             int H, int W, int k, int dilation, void *stream);
/* Weight gradients of the stride-3 layers with frozen BatchNorm (csrc/conv2d_mfma_grad.hip), with the meaning of
 * decnet_conv2d_mfma_wgrad: gm = gy * [y > 0] (written in full; y NULL: no ReLU, gm may be NULL and is gy), G and gsum[co] =
 * sum gm written in full, so that dW = scale * G, dscale = <w, G>, dshift = gsum.
 * decnet_conv2d_k3s3_wgrad: Conv2d k 3, stride 3, padding 1 (the layers of decnet_conv2d_k3s3_bn_act and decnet_s2d3_pad1 +
 * decnet_conv2d_mfma_cat_bn_act).  x [B,Cin,H,W]; gy, y, gm [B,Cout,Ho,Wo], Ho = (H-1)/3+1, Wo = (W-1)/3+1;
 *   G[co][ci][ky][kx] = sum_{b,yo,xo} gm[b][co][yo][xo] * x[b][ci][3yo-1+ky][3xo-1+kx]   (zeros outside), G [Cout,Cin,3,3]
 * decnet_deconv2d_k3s3_wgrad: ConvTranspose2d k 3, stride 3, padding 0 (decnet_deconv2d_k3s3_bn_act,
 * decnet_deconv2d_mfma_k3s3_bn_act).  x [B,Cin,H,W]; gy, y, gm [B,Cout,3H,3W];
 *   G[ci][co][a][c] = sum_{b,i,j} x[b][ci][i][j] * gm[b][co][3i+a][3j+c], G [Cin,Cout,3,3]
 * Both are one GEMM [Cp x coarse pixels] . [coarse pixels x (9 Cq + 1)] on v_mfma_f32_16x16x4_f32 (an fp32 fma chain) of the
 * coarse tensor (gm / x) with the 3 x 3 stride-3 windows of the fine one (x / gm), read in place.  Cin, Cout <= 224; B and
 * the coarse H <= 65535; a fine plane < 2^29 floats.
 *   workspace   decnet_..._k3s3_wgrad_workspace_floats(B, Cin, Cout, H, W) floats (0: shape not covered), 16-byte aligned
 *               (else DECNET_ERR_MISALIGNED); fewer floats than the query: DECNET_ERR_BAD_SHAPE
 * Every other buffer is accepted at any float alignment.  Deterministic: partition and order are functions of the shape
 * alone; workgroups write partial sums (fp32 chains of at most 4096 terms: 64 coarse pixels x at most 64 chunks) into the
 * workspace, a second launch adds them in a fixed order in float64 and rounds once; the transposed layer's gsum is a
 * fixed-order float64 sum of gm (two more launches).  No atomics, no allocation, no synchronisation (capturable).
 * NULL (also y without gm): DECNET_ERR_NULL_POINTER; a dimension < 1: DECNET_ERR_BAD_SHAPE (the planes of gy, y and gm
 * follow from H and W); Cin or Cout > 224 or a size limit: DECNET_ERR_UNSUPPORTED.  Nothing is launched on any refusal. */
size_t decnet_conv2d_k3s3_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W);
int decnet_conv2d_k3s3_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                             float *workspace, size_t workspace_floats, int B, int Cin, int Cout, int H, int W,
                             void *stream);
size_t decnet_deconv2d_k3s3_wgrad_workspace_floats(int B, int Cin, int Cout, int H, int W);
int decnet_deconv2d_k3s3_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                               float *workspace, size_t workspace_floats, int B, int Cin, int Cout, int H, int W,
                               void *stream);
/* Weight gradient of one stage-0 Conv3dUnit with frozen BatchNorm (csrc/conv3d_grad.hip): the 3-D, channels-last
 * counterpart of decnet_conv2d_mfma_wgrad for y = act(conv(x, w) * scale + shift), Conv3d k 3, s 1, p 1.
 *   x [B,D,H,W,Ci];  gy, y, gm [B,D,H,W,Co];  G [Co,Ci,3,3,3] (torch layout);  gsum [Co]
 *   gm = gy * [y > 0] (written in full; y NULL: no ReLU, gm may be NULL and is gy)
 *   G[co][ci][kd][kh][kw] = sum_{b,d,h,w} gm[b,d,h,w,co] * x[b,d+kd-1,h+kh-1,w+kw-1,ci]   (zeros outside the volume)
 *   gsum[co] = sum gm[...,co];  G and gsum written in full, so that dW = scale * G, dscale = <w, G>, dshift = gsum.
 * dx is the forward entry itself (decnet_conv3d_bn_act / decnet_conv3d_wino_bn_act) on gm with scale 1, shift 0, no ReLU and
 * the weights w'[ci][co][kd][kh][kw] = w[co][ci][2-kd][2-kh][2-kw] * scale[co].
 *   Ci          a multiple of 4 (as the forward entries), <= 224;  Co 1 .. 224;  any B, D, H, W >= 1
 *   size limit  B D H W max(Ci, Co) < 2^31: the kernel addresses x, gy and gm by 32-bit element offsets
 *   workspace   decnet_conv3d_wgrad_workspace_floats(B, D, H, W, Ci, Co) floats (0: shape not covered), 16-byte aligned
 *               (else DECNET_ERR_MISALIGNED); fewer floats than the query: DECNET_ERR_BAD_SHAPE
 * Every other buffer is accepted at any float alignment.  The GEMM [Co x voxels] . [voxels x (27 Ci + 1)] runs on
 * v_mfma_f32_16x16x4_f32 (an fp32 fma chain; no bf16 split).  Deterministic: partition and order are functions of the shape
 * alone.  The V = B D H W voxels of the flat volume are cut into nsets = ceil(V / sl) slices of sl consecutive voxels (the
 * last one shorter), sl a power of two: 4096, halved down to 256 while ceil((27 Ci + 1) / 64) * ceil(V / sl) < 1024.  Each
 * slice is one partial set [Co][27 Ci + 1] of the workspace (the query is exactly nsets * Co * (27 Ci + 1)), an fp32 chain of
 * sl <= 4096 terms per element; a last launch adds the sets in a fixed order in float64 and rounds once.  No atomics, no
 * allocation, no synchronisation (capturable); the bits depend neither on a pointer's alignment nor on what LDS held.
 * NULL (also y without gm): DECNET_ERR_NULL_POINTER; a dimension < 1: DECNET_ERR_BAD_SHAPE; Ci % 4 != 0, Ci or Co > 224,
 * the size limit: DECNET_ERR_UNSUPPORTED.  Nothing is launched on any refusal. */
size_t decnet_conv3d_wgrad_workspace_floats(int B, int D, int H, int W, int Ci, int Co);
int decnet_conv3d_wgrad(const float *x, const float *gy, const float *y, float *gm, float *G, float *gsum,
                        float *workspace, size_t workspace_floats, int B, int D, int H, int W, int Ci, int Co,
                        void *stream);
/* Refinement.get_warped_feats_by_homgrp (submodule.py:719-745): out[b,c,y,x] = bilinear(right[b,c];
 * (x - disp[b,y,x]) * W/(W-1) - 0.5, y * H/(H-1) - 0.5), zero padding.  right,out [B,C,H,W], disp [B,H,W]. */
int decnet_warp_disparity(const float *right, const float *disp, float *out, int B, int C, int H, int W,
                          void *stream);
/* Tail of DynamicUpsampling.forward (submodule.py:581-589), down_scale 3: logits [B,81,h,w] (channel =
 * 9 * sub-position + neighbour), disp [B,h,w] -> out [B,3h,3w] =
 * 3 * pixel_shuffle(sum_k softmax_k(logits) * replicate-padded 3x3 neighbours of disp). */
int decnet_dynamic_upsample3(const float *logits, const float *disp, float *out, int B, int h, int w,
                             void *stream);
/* Tail of GenerateSparseMask.forward + the thresholding of the model loop in one pass (submodule.py:366-372:
 * res_info = (cur_fea - pre_fea)^2 -> Conv2dUnit(3,3,3x3,BN) -> Conv2dUnit(3,1,1x1,BN) = detail;
 * SparseDenseNetRefinementMask.py:158-170: mask = sigmoid(detail) > thold ? 1 : 0).
 *   cur3, pre3   [B,3,H,W] device: outputs of GenerateSparseMask.conv_sub / .deconv
 *   w3x3 [3,3,3,3] (torch [co,ci,ky,kx]), scale3/shift3 [3], w1x1 [3], scale1, shift1: HOST values, BatchNorm
 *                folded (scale = gamma / sqrt(var + eps), shift = beta - mean * scale); thold as float32
 *   mask         [B,H,W] float 0/1 (the reference's contract: what SpaMat / SoftAttention read)
 *   logits       NULL or [B,H,W]: `detail`
 *   bits         NULL or [B,H,ceil(W/64)] 64-bit words, bit i of word w = pixel 64 w + i of the row       */
int decnet_detail_mask(const float *cur3, const float *pre3, const float *w3x3, const float *scale3,
                       const float *shift3, const float *w1x1, float scale1, float shift1, float thold,
                       float *mask, float *logits, unsigned long long *bits, int B, int H, int W,
                       void *stream);
/* Head of DynamicUpsampling.forward (submodule.py:578-580): out = cat(disp, unfold(fea, 3, stride 3)):
 * fea [B,C,3h,3w], disp [B,h,w] -> out [B,9C+1,h,w], out[b,0] = disp, out[b,1+9c+3i+j,y,x] = fea[b,c,3y+i,3x+j]. */
int decnet_unfold3_cat(const float *fea, const float *disp, float *out, int B, int C, int h, int w,
                       void *stream);
/* ---- the full-resolution tail under hip_grad() (csrc/tail_grad.hip) -------------------------------------------------
 * Backward of decnet_warp_disparity, decnet_dynamic_upsample3 and decnet_unfold3_cat, and SoftAttention's sigmoid + blend
 * with its backward.  Common to all: fp32 planes at any float alignment; every output element is written; every sum is a
 * gather in a fixed order (no atomics: the same bits on every run); no allocation, no synchronisation (capturable);
 * nothing is launched on any refusal.
 *
 * decnet_warp_disparity_backward: gout [B,C,H,W] -> g_right [B,C,H,W] and / or g_disp [B,H,W] (each may be NULL, not
 * both).  The sampling position is the forward's fp32 operation sequence, so the cell floor(ix), floor(iy) is the forward's.
 *   g_disp[b,y,x]     = -W/(W-1) sum_c gout[b,c,y,x] ((v_ne - v_nw)(1 - t_y) + (v_se - v_sw) t_y), t_y = iy - floor(iy),
 *                       taps outside the image zero, channels summed in rising order
 *   g_right[b,c,y',x'] = sum_{(y,x)} w_y(y,y') w_x(y,x,x') gout[b,c,y,x]: the transpose of the forward, contributing rows y
 *                       rising, then x rising
 * H < 2 or W < 2: DECNET_ERR_BAD_SHAPE; the forward's grid limits, and for g_right W > 1819 (the row's positions and
 * eight channels of gout are staged in 64 KiB of LDS): DECNET_ERR_UNSUPPORTED.  Disparities must be finite; ones that
 * push every tap off the image give zero gradients. */
int decnet_warp_disparity_backward(const float *right, const float *disp, const float *gout, float *g_right,
                                   float *g_disp, int B, int C, int H, int W, void *stream);
/* decnet_dynamic_upsample3_backward: gout [B,3h,3w] -> g_logits [B,81,h,w] and, unless NULL, g_disp [B,h,w].  With
 * p = softmax_k(logits[9 s + k]) (the forward's max-subtracted expf), n_k the replicate-padded neighbours and
 * m_s = sum_k p_k n_k:  g_logits[9 s + k] = 3 gout_s p_k (n_k - m_s);  g_disp[Y,X] = sum of q_k(y,x) = 3 sum_s gout_s p_{s,k}
 * over every (y, x, k) whose clamped neighbour is (Y,X), in the order y, x, k rising.
 *   workspace   q [B,9,h,w]: decnet_dynamic_upsample3_backward_workspace_floats(B, h, w) floats (0: shape not covered),
 *               16-byte aligned; read only with g_disp.  With g_disp given: NULL is DECNET_ERR_NULL_POINTER, fewer floats
 *               than the query DECNET_ERR_BAD_SHAPE, a misaligned one DECNET_ERR_MISALIGNED.
 * h or B > 65535: DECNET_ERR_UNSUPPORTED. */
size_t decnet_dynamic_upsample3_backward_workspace_floats(int B, int h, int w);
int decnet_dynamic_upsample3_backward(const float *logits, const float *disp, const float *gout, float *g_logits,
                                      float *g_disp, float *workspace, size_t workspace_floats, int B, int h, int w,
                                      void *stream);
/* Inverse of decnet_unfold3_cat's feature part: g [B,9C+1,h,w] -> g_fea [B,C,3h,3w], g_fea[b,c,3y+i,3x+j] =
 * g[b,1+9c+3i+j,y,x] (channel 0, the disparity plane, is not read).  Limits as decnet_unfold3_cat. */
int decnet_fold3(const float *g, float *g_fea, int B, int C, int h, int w, void *stream);
/* SoftAttention's tail over n floats: s = 1 / (1 + expf(-o)), out = a (1 - s) + s b -- the statement sequence of
 * decnet_conv2d_cat_epilogue's epilogue 1, so the same bits.  Backward: g_o = gout (b - a) s (1 - s), g_a = gout (1 - s),
 * g_b = gout s (g_a, g_b: each may be NULL), s recomputed from o. */
int decnet_sigmoid_blend(const float *o, const float *a, const float *b, float *out, size_t n, void *stream);
int decnet_sigmoid_blend_backward(const float *o, const float *a, const float *b, const float *gout, float *g_o,
                                  float *g_a, float *g_b, size_t n, void *stream);
/* ---- detail maps and soft masks under hip_grad() (csrc/detail_grad.hip) -------------------------------------------------
 * What a training forward keeps beside the disparities: sigmoid(detail) of GenerateSparseMask with its thresholded copies,
 * and SoftAttention's soft mask next to its blend.  Common to all: elementwise fp32, contraction off; planes at any float
 * alignment (the values do not depend on it); no allocation, no synchronisation (capturable); nothing is launched and
 * nothing is written on any refusal.  The flat entries take n floats, 1 <= n <= 2^40 (else DECNET_ERR_BAD_SHAPE /
 * DECNET_ERR_UNSUPPORTED).
 *
 * decnet_sqdiff: d = a - b, out = d d, each rounded once: the bits of torch's (a - b) * (a - b).
 * decnet_sqdiff_backward: t = gout d, g_a = t + t, g_b = -g_a: the bits of torch autograd through d * d.  g_a, g_b: each may
 * be NULL, not both. */
int decnet_sqdiff(const float *a, const float *b, float *out, size_t n, void *stream);
int decnet_sqdiff_backward(const float *a, const float *b, const float *gout, float *g_a, float *g_b, size_t n,
                           void *stream);
/* decnet_detail_tail: logits [B,H,W] (`detail`, e.g. what decnet_detail_mask wrote) -> s = 1 / (1 + expf(-z)), the
 * statement of decnet_detail_mask;
 *   prob   NULL or [B,H,W]: s
 *   mask   NULL or [B,H,W]: s > thold ? 1 : 0
 *   bits   NULL or [B,H,ceil(W/64)] 64-bit words, bit i of word w = pixel 64 w + i of the row, zero at and past W
 * (not all three NULL).  Limits as decnet_detail_mask.
 * decnet_detail_tail_backward over n floats: g_logits = g_prob (s (1 - s)), s recomputed as the forward computes it; a
 * saturated sigmoid gives exactly 0, never NaN. */
int decnet_detail_tail(const float *logits, float thold, float *prob, float *mask, unsigned long long *bits, int B, int H,
                       int W, void *stream);
int decnet_detail_tail_backward(const float *logits, const float *g_prob, float *g_logits, size_t n, void *stream);
/* decnet_sigmoid_blend_soft: out as decnet_sigmoid_blend writes it (the same statements, the same bits), soft = s.
 * decnet_sigmoid_blend_soft_backward: g_o = (gout (b - a) + gsoft) (s (1 - s)), g_a = gout (1 - s), g_b = gout s.  gout,
 * gsoft: each may be NULL, not both; without gsoft the three results have the bits of decnet_sigmoid_blend_backward, without
 * gout g_o = gsoft (s (1 - s)) and g_a, g_b are written as zeros.  g_a, g_b: each may be NULL. */
int decnet_sigmoid_blend_soft(const float *o, const float *a, const float *b, float *out, float *soft, size_t n,
                              void *stream);
int decnet_sigmoid_blend_soft_backward(const float *o, const float *a, const float *b, const float *gout,
                                       const float *gsoft, float *g_o, float *g_a, float *g_b, size_t n, void *stream);
/* Space-to-depth in front of the stride-3 convolutions of FeatExtNetChannelPlus (Conv2d k 3, stride 3, padding 1,
 * submodule.py:270-300): x [B,C,H,W] -> out [B,9C,Ho,Wo], Ho = (H-1)/3+1, Wo = (W-1)/3+1,
 * out[b,c*9+ky*3+kx,yo,xo] = x[b,c,3yo-1+ky,3xo-1+kx] (0 outside); the convolution is then the 1 x 1 convolution with the
 * weight [Cout,Cin,3,3] read as [Cout,9 Cin] (decnet_conv2d_mfma_cat_bn_act, k = 1). */
int decnet_s2d3_pad1(const float *x, float *out, int B, int C, int H, int W, void *stream);
/* The adjoint of decnet_s2d3_pad1 (the input gradient of the stride-3 convolutions): t [B,9C,Ho,Wo] -> dx [B,C,H,W],
 * dx[b,c,r,s] = t[b,c*9+((r+1)%3)*3+(s+1)%3,(r+1)/3,(s+1)/3], and 0 where (r+1)/3 = Ho or (s+1)/3 = Wo (the last row /
 * column when H / W is a multiple of 3): dx is written in full.  H, B*C <= 65535 (else DECNET_ERR_UNSUPPORTED). */
int decnet_d2s3_pad1(const float *t, float *dx, int B, int C, int H, int W, void *stream);
/* Space-to-depth of a ConvTranspose2d k 3, stride 3, padding 0 (its input gradient is the 1 x 1 convolution 9 C -> Cin of
 * this): g [B,C,3H,3W] -> out [B,9C,H,W], out[b,c*9+3a+j,i,x] = g[b,c,3i+a,3x+j].  H <= 21845, B*C <= 65535 (else
 * DECNET_ERR_UNSUPPORTED). */
int decnet_s2d3_pad0(const float *g, float *out, int B, int C, int H, int W, void *stream);
/* y[b,c,:,:] = act(y[b,c,:,:] + shift[c]) in place, y [B,C,H,W]: the folded-BatchNorm bias and the ReLU
 * behind a library convolution, one pass.  B*C <= 65535. */
int decnet_bias_act_inplace(float *y, const float *shift, int B, int C, int H, int W, int relu,
                            void *stream);
/* Conv2d k = 3, stride 3, padding 1 (FeatExtNetChannelPlus down-sampling, submodule.py:245-343),
 * Cout <= 24; y [B,Cout,(H-1)/3+1,(W-1)/3+1]; weights packed with transposed = 0. */
int decnet_conv2d_k3s3_bn_act(const float *x, const float *w_packed, const float *scale,
                              const float *shift, float *y, int B, int Cin, int Cout, int H, int W,
                              int relu, void *stream);
int decnet_deconv2d_k3s3_bn_act(const float *x, const float *w_packed, const float *scale,
                                const float *shift, float *y, int B, int Cin, int Cout, int H,
                                int W, int relu, void *stream);

/* ---------------------------------------------------------------------------------------
 * Dilated 3x3 / 1x1 convolutions on small, many-channel images as a per-tap matrix product + gather:
 * the ASPP block of FeatExtNetChannelPlus (submodule.py:225-241).  All branches share the input:
 *   decnet_tapconv_to_chunks   x [B,Ci,H,W] -> V [ceil(Ci/16)][P=B*H*W][16]
 *   decnet_tapconv_pack_weight one branch's w [Co,Ci,k,k] -> taps tap0.. of u (decnet_tapconv_weight_floats)
 *   decnet_tapconv_split_weight after the last branch (optional): the bf16-term copy of u behind it
 *   decnet_tap_gemm            T[t] = V * u[t] for every tap t, T [ntaps][ceil(Co/16)][P][16].  split = 1 states that
 *                              decnet_tapconv_split_weight has run on this u since its last pack: the bf16x3 kernel
 *                              then reads that copy (Ci = 216); split = 0: fp32 MFMA on the packed matrices alone
 *   decnet_tapconv_gather      y[b, br*Co+co, y, x] = act(scale * sum_t T[t][co][p + offset] + shift),
 *                              taps outside the image skipped; y [B, nbranch*Co, H, W]
 * Ci % 4 == 0, Co <= 224, nbranch <= 4.
 * V, u and T are library-format buffers read and written in 16-byte units: they must be 16-byte aligned, else
 * decnet_tapconv_to_chunks, _pack_weight, _split_weight and decnet_tap_gemm return DECNET_ERR_MISALIGNED with nothing
 * launched (x, y, scale and shift may be any dense fp32 pointer; decnet_tapconv_gather reads T at any alignment).
 * ------------------------------------------------------------------------------------- */
size_t decnet_tapconv_chunk_floats(int B, int Ci, int H, int W);
int decnet_tapconv_to_chunks(const float *x, float *V, int B, int Ci, int H, int W, void *stream);
size_t decnet_tapconv_weight_floats(int Ci, int ntaps);
int decnet_tapconv_pack_weight(const float *w, float *u, int Co, int Ci, int k, int tap0, void *stream);
int decnet_tapconv_split_weight(float *u, int Ci, int ntaps, void *stream);
int decnet_tap_gemm(const float *V, const float *u, float *M, int P, int Ci, int Co, int ntaps,
                    int split, void *stream);
int decnet_tapconv_gather(const float *M, const float *scale, const float *shift, float *y, int B,
                          int Co, int H, int W, int nbranch, const int *tap0, const int *k,
                          const int *dil, int relu, void *stream);

/* Layout helpers between the reference's [B,C,D,H,W] and the internal [B,D,H,W,C]. */
int decnet_ncdhw_to_ndhwc(const float *src, float *dst, int B, int C, int D, int H, int W,
                          void *stream);
int decnet_ndhwc_to_ncdhw(const float *src, float *dst, int B, int C, int D, int H, int W,
                          void *stream);

/* ---------------------------------------------------------------------------------------
 * The image boundary: uint8 views in, uint16 disparity and evaluation sums out.  None of the three allocates,
 * synchronises or asks about the stream (all run under stream capture); no pointer needs more than the alignment of
 * its element type, and the uint8 / uint16 buffers none at all.  DECNET_ERR_BAD_SHAPE: a non-positive size, H < h,
 * W < w, or B * H * W (times 3 for the image) >= 2^31.  The h x w image sits at the BOTTOM RIGHT of the H x W plane
 * (the reference pads on the top and left, demo.py:75-81).
 *
 * decnet_preprocess_u8 -- demo.py:75-89 (padding + transform), loader/SceneflowMask.py:118-130,152-153,206-210.
 *   img    [B,h,w,3] uint8, interleaved RGB
 *   table  [256][3]  fp32, device: table[v][c] = what the host path makes of pixel value v in channel c.  The caller
 *                    builds it (decnet_amd.imageio.normalise_table: the loader's own numpy expressions), so the output
 *                    is bit-equal to the host path.
 *   out    [B,3,H,W] fp32: out[b,c,y,x] = table[img[b, y-(H-h), x-(W-w), c]][c] inside the image, table[0][c] in the
 *                    padding (the reference pads with zeros BEFORE it normalises).                                  */
int decnet_preprocess_u8(const unsigned char *img, const float *table, float *out, int B, int h, int w, int H, int W,
                         void *stream);
/* demo.py:191-197.  pred [B,H,W] fp32 -> out [B,h,w] uint16 = (uint16) min(max(pred * 256, 0), 65535), truncated toward
 * zero, of the bottom-right window (a NaN gives 0). */
int decnet_disparity_to_u16(const float *pred, unsigned short *out, int B, int H, int W, int h, int w, void *stream);
/* test_loss_func (modules/loss.py:427-437), as sums.  pred [B,H,W]; gt [B,h,w] UNPADDED, compared with the bottom-right
 * window of pred (the loader's padded ground truth is 0 in the padding, hence invalid: the same pixels take part).
 *   partials [B,h,3] fp32, per row, over the pixels with 0 < gt < max_disp:  the count of those pixels,
 *            sum |pred - gt|, the count with |pred - gt| < 3 || |pred - gt| < 0.05f * gt.
 * Fixed summation order, no atomics: the same bits on every call.  A NaN prediction gives a NaN sum and is not counted
 * as good.  EPE = sum of [1] / sum of [0], loss_3 = 100 - 100 * sum of [2] / sum of [0] (reduce in float64; the counts
 * are exact for w < 2^24). */
int decnet_disparity_metrics(const float *pred, const float *gt, float max_disp, float *partials, int B, int H, int W,
                             int h, int w, void *stream);

/* ---------------------------------------------------------------------------------------
 * One pyramid level of the multi-stage training loss (Loss.multi_stage_regression_Uploss, modules/loss.py:168-242) and
 * its gradient.  Neither entry allocates, synchronises or asks about the stream (both run under stream capture); every
 * plane is [B,H,W] fp32 at any float alignment, inputs are never modified, and the results depend neither on the
 * alignment of a plane nor on the launch shape.  DECNET_ERR_BAD_SHAPE: a non-positive size, B * H * W >= 2^31 or
 * skip_rows < 0; nothing is launched then.
 *   gt         the ground truth ALREADY at this level's resolution (the caller downsamples it)
 *   valid    = gt > 0 && gt < gt_max && y >= skip_rows          (skip_rows: the if_overmask rows, loss.py:204-205)
 *   whole    = valid && left_mask == 1
 *   term(a)  = smooth-L1 (beta 1) of d = a * down_size - gt * down_size, the products and d rounded to fp32
 *   means:     pred, dense, fusion over valid; sparse over whole; soft_mask over left_mask == 1 (it ignores valid,
 *              loss.py:235).  A mean over no pixels is NaN.  A pixel outside a mask is selected out: a NaN there reaches
 *              no sum; a NaN inside a mask makes its term NaN.
 * dense, sparse, fusion, soft_mask, left_mask all NULL: the simple form of stage 0 and of the stages >= stop_stage_id
 * (loss.py:207-211): only the pred term, the other four written as 0.  Some but not all of them NULL:
 * DECNET_ERR_NULL_POINTER.
 *
 * decnet_stage_loss_forward: two launches.  Per row (a wave each; every lane accumulates in float64 from its first
 * element on, the lanes are added in a fixed butterfly), then one workgroup that adds the rows in a fixed order.
 *   row_sums [B*H][8] float64 scratch; per row: n_valid, n_whole, n_left, S_pred, S_dense, S_sparse, S_fusion, S_soft
 *   sums     [8]      float64: their totals (what the backward entry reads)
 *   terms    [5]      fp32: dense, sparse, soft-mask mean, fusion, pred -- the order the reference appends them to
 *                     loss_list (loss.py:233-237) -- each the fp32 of the float64 quotient.
 * decnet_stage_loss_backward: one launch; counts and upstream gradients are read from device memory.
 *   sums       [8] as the forward entry left them;  grad_terms [5] fp32, device: d(loss) / d(terms[k])
 *   g_*        NULL (skipped) or [B,H,W], written in full: grad_terms[k] * down_size * clamp(d, -1, 1) / n inside the
 *              term's mask, grad_terms[2] / n_left for the soft mask, 0 elsewhere -- and 0 everywhere where the term's
 *              count is 0 (the gradient of an empty gather), and for the four absent terms of the simple form.
 * ------------------------------------------------------------------------------------- */
int decnet_stage_loss_forward(const float *pred, const float *dense, const float *sparse, const float *fusion,
                              const float *soft_mask, const float *left_mask, const float *gt, float gt_max,
                              float down_size, int skip_rows, double *row_sums, double *sums, float *terms, int B, int H,
                              int W, void *stream);
int decnet_stage_loss_backward(const float *pred, const float *dense, const float *sparse, const float *fusion,
                               const float *soft_mask, const float *left_mask, const float *gt, float gt_max,
                               float down_size, int skip_rows, const double *sums, const float *grad_terms, float *g_pred,
                               float *g_dense, float *g_sparse, float *g_fusion, float *g_soft, int B, int H, int W,
                               void *stream);

/* ---------------------------------------------------------------------------------------
 * Training-mode BatchNorm2d (batch statistics) with an optional ReLU, forward and backward (csrc/batchnorm.hip).
 * z [B,C,H,W] fp32 at any float alignment: the convolution's output; N = B H W values per channel.  Neither entry
 * allocates, synchronises or asks about the stream (both run under stream capture); sums are float64 in a fixed order
 * without atomics, so the results depend neither on the launch shape nor on the alignment of a plane.  A NaN in a channel
 * reaches that channel's statistics and no other's.
 *   workspace  decnet_bn_train_workspace_floats(B,C,H,W) floats (doubles count as two), 8-byte aligned (else
 *              DECNET_ERR_MISALIGNED); fewer floats than the query: DECNET_ERR_BAD_SHAPE.  It holds the partial sums
 *              [C][B nseg][2] of the segments of DECNET_BN_SEGMENT floats a plane is cut into (nseg per plane), then [C][2]
 *              totals.  The query returns 0 for a shape the entries refuse.
 *   stats      [2 C] float64, 8-byte aligned: per channel {mean, invstd = 1 / sqrt(var + eps)}, var the biased variance
 *              S2 / N - (S1 / N)^2 clamped at 0, S1 = sum (z - p), S2 = sum (z - p)^2 about the pivot p = z[0,c,0,0].
 * DECNET_ERR_BAD_SHAPE: a dimension < 1, N < 2 (one value per channel has no variance), B C H W >= 2^31.  A NULL
 * argument (other than those stated): DECNET_ERR_NULL_POINTER.  Nothing is launched on any refusal.
 *
 * decnet_bn_train_forward: three launches.
 *   y = act(fma(d, a, beta)), d = (float)(z - mean) with the difference in float64, a = (float)(gamma invstd),
 *   act = ReLU (relu != 0) or the identity.
 *   running_mean, running_var   both NULL, or both [C] fp32, updated in place (float64, rounded once):
 *              rm <- (1 - momentum) rm + momentum mean,  rv <- (1 - momentum) rv + momentum var N / (N - 1).
 * decnet_bn_train_backward: three launches (two when gz is NULL).  With pre recomputed from z exactly as the forward formed
 * it, gm = gy [pre > 0] (gm = gy without ReLU) and xhat = (z - mean) invstd:
 *   dbeta = sum gm, dgamma = sum gm xhat    [C] fp32, each the fp32 of a float64 sum
 *   gz    NULL (skipped) or [B,C,H,W], written in full: a (gm - dbeta / N - xhat dgamma / N), formed in float64.
 * ------------------------------------------------------------------------------------- */
#define DECNET_BN_SEGMENT 4096
size_t decnet_bn_train_workspace_floats(int B, int C, int H, int W);
int decnet_bn_train_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                            float *running_mean, float *running_var, double *stats, float *y, int relu, void *workspace,
                            size_t workspace_floats, int B, int C, int H, int W, void *stream);
int decnet_bn_train_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                             float *gz, float *dgamma, float *dbeta, int relu, void *workspace, size_t workspace_floats,
                             int B, int C, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * The same on a CHANNELS-LAST matrix (csrc/batchnorm.hip, its Columns layout): z [rows, C] fp32 at any float alignment,
 * channel c the column z[:, c], N = rows values per channel -- the Conv3d units of stage 0, whose volumes are
 * [B,D,H,W,C] (rows = B D H W).  Any C >= 1.  The contract, formulas, roundings, optional arguments and error codes are those of
 * decnet_bn_train_forward / _backward above, with these differences:
 *   workspace  decnet_bn_train_cl_workspace_floats(rows, C) floats, 8-byte aligned.  The rows are cut into
 *              nseg = ceil(rows / DECNET_BN_CL_ROWS) segments of DECNET_BN_CL_ROWS rows; the workspace holds the partial
 *              sums [nseg][C][2] float64, then [C][2] totals.  The query returns 0 for a shape the entries refuse.
 *   order      the partial of (segment, channel) is one thread's float64 sum over the segment's rows in rising order;
 *              a channel's partials are added by 16 threads (thread j: segments j, j + 16, ... in rising order), whose
 *              sums are added in a fixed tree.  No atomics; the bits depend neither on the launch shape, nor on the
 *              alignment of any pointer (every access is a single float), nor on eager versus replay.
 *   pivot      p = z[0, c].
 * DECNET_ERR_BAD_SHAPE: rows < 2, C < 1, rows C >= 2^31, fewer workspace floats than the query.  Nothing is launched
 * on any refusal.  Three launches each (the backward two when gz is NULL).
 * ------------------------------------------------------------------------------------- */
#define DECNET_BN_CL_ROWS 32
size_t decnet_bn_train_cl_workspace_floats(size_t rows, int C);
int decnet_bn_train_cl_forward(const float *z, const float *gamma, const float *beta, double eps, double momentum,
                               float *running_mean, float *running_var, double *stats, float *y, int relu, void *workspace,
                               size_t workspace_floats, size_t rows, int C, void *stream);
int decnet_bn_train_cl_backward(const float *z, const float *gy, const float *gamma, const float *beta, const double *stats,
                                float *gz, float *dgamma, float *dbeta, int relu, void *workspace, size_t workspace_floats,
                                size_t rows, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DECNET_HIP_H */
