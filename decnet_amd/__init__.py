"""decnet_amd -- MI355X (gfx950) implementation of DecNet's data-parallel hot path.

* SpaMat / SpaVar   (reference modules/SparseMatching, modules/SparseVar)
* stage-0 dense cost volume -> Conv3d aggregation -> soft-argmax
  (reference modules/submodule.py GetCostVolume / CostRegNetNoDown / disparity_regression)
* StereoEngine: uint8 pairs in, uint16 disparity out -- the whole network as one HIP graph per shape, copies pipelined
* Loss: the multi-stage training loss (reference modules/loss.py), one fused kernel pair per pyramid level
* hip_grad(): opt-in backward of the few-channel stride-1 conv units with frozen BatchNorm (Conv2dSmallFunction): the
  weight gradient as a deterministic fp32 matrix-core reduction, dx on the forward kernel with flipped weights; and of
  the full-resolution tail (WarpDisparityFunction, Unfold3CatFunction, DynamicUpsample3Function, SigmoidBlendFunction):
  the inference entries forward, fixed-order gathers backward; the detail maps and soft masks a training forward keeps
  (SquaredDiffFunction, DetailTailFunction, SigmoidBlendSoftFunction: GenerateSparseMask.detail, SoftAttention.fuse with
  want_soft); and of stage 0 (Conv3dFunction, CostVolumeFunction: the
  eight Conv3d units of CostRegNetNoDown, the per-layer inference entries forward; BatchNorm3d frozen, or in .train()
  mode on the statistics of the batch: BatchNorm3dActFunction, the Columns layout of csrc/batchnorm.hip)

Host side is Python on PyTorch-ROCm (device memory + streams only); all arithmetic runs in
hand-written HIP kernels behind the C ABI of include/decnet_hip.h.  No CPU fallback.
"""
from ._lib import DecnetHipError, version  # noqa: F401
from .modules.SparseMatching.modules.SpaMat import SpaMat  # noqa: F401
from .modules.SparseMatching.functions.SpaMat import SpaMatFunction  # noqa: F401
from .modules.SparseVar.modules.SpaVar import SpaVar  # noqa: F401
from .modules.SparseVar.functions.SpaVar import SpaVarFunction  # noqa: F401
from .ops import spamatvar_forward, spamatvar_forward_bits  # noqa: F401
from .engine import StereoEngine  # noqa: F401
from .loss import Loss, StageLossFunction  # noqa: F401
from .conv2d_grad import Conv2dSmallFunction, hip_grad, hip_grad_enabled  # noqa: F401
from .tail_grad import (DetailTailFunction, DynamicUpsample3Function, SigmoidBlendFunction,  # noqa: F401
                        SigmoidBlendSoftFunction, SquaredDiffFunction, Unfold3CatFunction, WarpDisparityFunction)
from .stage0_grad import BatchNorm3dActFunction, Conv3dFunction, CostVolumeFunction  # noqa: F401
from .stage0 import (CostRegNetNoDown, GetCostVolume, Stage0, disparity_regression,  # noqa: F401
                     drop_weight_caches, get_disp_samples)

__all__ = ["SpaMat", "SpaVar", "SpaMatFunction", "SpaVarFunction", "spamatvar_forward", "spamatvar_forward_bits",
           "GetCostVolume", "CostRegNetNoDown", "disparity_regression", "get_disp_samples",
           "Stage0", "DecnetHipError", "version", "drop_weight_caches", "StereoEngine", "Loss",
           "StageLossFunction", "Conv2dSmallFunction", "hip_grad", "hip_grad_enabled", "WarpDisparityFunction",
           "Unfold3CatFunction", "DynamicUpsample3Function", "SigmoidBlendFunction", "Conv3dFunction", "CostVolumeFunction",
           "BatchNorm3dActFunction", "SquaredDiffFunction", "DetailTailFunction", "SigmoidBlendSoftFunction"]
