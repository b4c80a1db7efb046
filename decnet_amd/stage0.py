"""Stage-0 dense path (coarsest level) behind the reference's own names.

Reference (modules/submodule.py): get_disp_samples :376-424, GetCostVolume :428-562,
Conv3dUnit :90-123, CostRegNetNoDown :608-662, disparity_regression :766-777; used by
SparseDenseNetRefinementMask.forward :127-137.

The classes keep the reference's constructor arguments, attribute names and state_dict
keys (``conv0.0.conv.weight``, ``conv0.0.bn.running_mean`` ...) so a checkpoint of the
reference loads unchanged.  Activations between the HIP kernels are channels-last
[B,D,H,W,C]; tensors handed back to callers have the reference's logical shapes
([B,C,D,H,W] cost volume is returned as a permuted view of the channels-last buffer).

Under ``torch.no_grad()`` in eval mode this is the inference hot path.  Inside ``decnet_amd.hip_grad()``, with autograd on
and an input or a parameter that requires grad, ``CostRegNetNoDown`` records its backward unit by unit (``_units_grad``,
stage0_grad.py): gradients of the feature maps, the eight ``conv.weight`` and the BatchNorm weights and biases.  In eval
mode the running statistics are frozen; in ``.train()`` mode (GPU tensors, ``hip_grad()`` on, a gradient wanted) every
unit whose ``bn`` is in train mode normalises with the statistics of the batch and updates the running ones, as the
reference's Conv3dUnit.forward does (submodule.py:115-123).  Every other call in ``.train()`` mode and cost_func "cat"
under grad stay refused.
"""
import os

import torch
import torch.nn as nn
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import _lib, ops2d, stage0_grad
from .conv2d_grad import hip_grad_enabled
from .ops import _chk

BN_EPS = 1e-5


WINO_VARIANT = {"winograd": 0, "winograd4": 1, "winograd444": 2}


# Optimizer steps taken in this process.  The fused optimizers (``torch.optim.Adam(fused=True)``, ``SGD(fused=True)``, ...)
# update the parameters in one kernel that leaves ``_version`` alone, so a key of addresses and versions would keep the
# packed weights of the step before: the forward under ``hip_grad()`` on last step's weights, the backward (which reads
# the live ``conv.weight``) on this step's.  A global post-step hook counts the steps, and the count is part of every key:
# after any ``optimizer.step()`` every cache repacks on its next use (a pack kernel per layer and step).
_OPTIMIZER_STEPS = [0]


def _count_optimizer_step(optimizer, args, kwargs):
    _OPTIMIZER_STEPS[0] += 1


register_optimizer_step_post_hook(_count_optimizer_step)


def source_key(ts, *extra):
    """Key of a packed-weight cache: (address, version, optimizer steps so far) of every tensor it is built from, plus the
    plain values that go into the packing.  It sees in-place writes under ``no_grad``, ``load_state_dict``, a re-assigned
    ``.data`` at a new address and every ``optimizer.step()`` (the fused ones do not bump the version); it cannot see a
    write THROUGH ``.data`` (``p.data.copy_()``, ``p.data.normal_()``), which changes none of them -- such writes after
    the first forward need ``decnet_amd.drop_weight_caches(model)``."""
    steps = _OPTIMIZER_STEPS[0]
    return tuple((t.data_ptr(), t._version, steps) for t in ts) + tuple(extra)


def source_hold(ts):
    """Aliases of the tensors a cache entry was built from, kept beside the entry: an address that is still owned
    cannot be handed out again by the caching allocator, so an equal key means the same memory (``p.data = other``
    keeps ``_version``, ``load_state_dict(assign=True)`` resets it to 0)."""
    return [t.detach() for t in ts]


def fold_bn(bn, fp32=True):
    """Eval-mode BatchNorm as a per-channel (scale, shift): y = scale * x + shift.  fp32=False folds in the parameters'
    own dtype (Unit._folded_torch, whose product goes back into a convolution of that dtype)."""
    w, b, mean, var = ((t.float() if fp32 else t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = w / torch.sqrt(var + bn.eps)
    return scale, b - mean * scale


def fold_none(conv):
    """The (scale, shift) of a layer without BatchNorm: ones, and the bias or zeros."""
    co, dev = conv.out_channels, conv.weight.device
    return torch.ones(co, device=dev), conv.bias.float() if conv.bias is not None else torch.zeros(co, device=dev)


def cache_attrs(*names):
    """The attributes CachesWeights._cached keeps for the caches `names`."""
    return tuple(n + sfx for n in names for sfx in ("", "_key", "_src"))


class CachesWeights:
    """Mixin of the modules that keep packed weights / workspaces between calls.  The caches are derived data: they
    are dropped when the parameters are moved or cast (``_apply``: ``.to()`` / ``.cpu()`` / ``.cuda()`` / ``.float()``)
    or loaded (``load_state_dict``, both modes), and they take no part in ``copy.deepcopy`` / pickling (some hold
    ctypes structures with pointers; a copy starts cold and repacks)."""
    _CACHE_ATTRS = ()

    def _drop_caches(self):
        for a in self._CACHE_ATTRS:
            self.__dict__.pop(a, None)

    def _cached(self, name, sources, extra, build, head=()):
        """The cache `name`, rebuilt by build() (under no_grad) when source_key(sources, *extra), behind `head`, is not the
        key it was built under; kept as the attributes `name`, `name`_key and `name`_src (source_hold)."""
        key, d = tuple(head) + source_key(sources, *extra), self.__dict__
        if d.get(name + "_key") != key:
            with torch.no_grad():
                value = build()
            d.update({name: value, name + "_key": key, name + "_src": source_hold(sources)})
        return d[name]

    def cache_tensors(self):
        """Every tensor the caches of this module hold now (packed weights, folded scales, workspaces), nested in dicts,
        lists and tuples to any depth.  Who captures a HIP graph keeps them: the module replaces a cache when another
        shape, range or weight arrives, and the graph goes on reading the old addresses (decnet_amd.engine).  A cache
        that keeps tensors in another kind of container has to override this."""
        found, seen, todo = [], set(), [self.__dict__.get(a) for a in self._CACHE_ATTRS]
        while todo:
            v = todo.pop()
            if id(v) in seen:
                continue
            seen.add(id(v))
            if isinstance(v, torch.Tensor):
                found.append(v)
            elif isinstance(v, dict):
                todo.extend(v.values())
            elif isinstance(v, (list, tuple)):
                todo.extend(v)
        return found

    def __getstate__(self):
        state = super().__getstate__()
        for a in self._CACHE_ATTRS:
            state.pop(a, None)
        return state

    def _apply(self, fn, *args, **kwargs):
        self._drop_caches()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._drop_caches()
        return super()._load_from_state_dict(*args, **kwargs)


def drop_weight_caches(module):
    """Drop every packed-weight cache and workspace of ``module`` and its children; the next forward repacks from
    the parameters as they are then.  Needed after a write through ``.data`` (see source_key).  HIP graphs captured
    before the call point into the dropped buffers and must be captured again."""
    for m in module.modules():
        if isinstance(m, CachesWeights):
            m._drop_caches()
    return module


def wino_stack_switch():
    """DECNET_WINO_STACK=0 turns the fused seven-layer stack off (read per call)."""
    return os.environ.get("DECNET_WINO_STACK", "1") != "0"


def conv_algo(D=None):
    """The Conv3d algorithm of the 216-channel layers.  DECNET_CONV_ALGO = "winograd" (F(2,3) on D, H, W:
    3.4x fewer multiplications than the 27-tap sum), "winograd4" (F(2,3) on D, F(4,3) on H, W: 6x),
    "winograd444" (F(4,3) on all three: 8x) or "direct" (27-tap implicit GEMM).  Unset: winograd444
    where the depth tiles of 4 pay (D = 8 or 10 at stage 0 of the shipped configurations), winograd4
    for shallow volumes.  All are fp32 on the matrix cores and differ by fp32 rounding only
    (tests/conv_numerics.py: 1.7e-6 / 3.0e-6 / 5.7e-6 / 2.9e-6 of max|y| after the 8 layers)."""
    a = os.environ.get("DECNET_CONV_ALGO", "auto").lower()
    if a == "auto":
        if D is None:
            return "winograd444"
        return "winograd444" if 216 * ((D + 3) // 4) <= 0.92 * 144 * ((D + 1) // 2) else "winograd4"
    if a not in ("winograd", "winograd4", "winograd444", "direct"):
        raise ValueError("DECNET_CONV_ALGO must be 'winograd', 'winograd4', 'winograd444' or 'direct'")
    return a


def _conv3d_grad_slower(C, voxels):
    """The Conv3dUnit shapes (C channels, B D H W voxels) that go to the library arm (``stage0_grad.unit_library``) under
    ``hip_grad()``: those whose forward + backward was measured slower on the HIP Function than under torch's autograd --
    eager, one run (tools/bench_stage0_grad.py, profiles/stage0_grad.json).  The measured pairs, hip / library ms, C = 216 on
    20 x 36 x 8: 216 -> 216 1.20 / 6.99 at 23 040 voxels and 2.21 / 13.07 at 46 080; 216 -> 1 0.49 / 4.41 and 0.54 / 8.25.
    None is slower, and nothing is routed at a size nobody measured: every unit stays on the HIP Function."""
    return False


def _conv3d_bn_train_slower(Ci, Co, voxels):
    """The same for a unit in ``.train()`` mode (Conv3dFunction, then BatchNorm3dActFunction, against
    ``stage0_grad.unit_library_train``: conv3d -> batch_norm on the statistics of the batch -> ReLU under torch's
    autograd), forward + backward, eager, one run (tools/bench_stage0_bn_train.py, profiles/stage0_bn_train.json).  The
    measured pairs, hip / library ms, C = 216 on 20 x 36 x 8: 216 -> 216 1.22 / 6.96 at 23 040 voxels and 2.27 / 12.98 at
    46 080; 216 -> 1 0.40 / 4.41 and 0.60 / 8.29.  None is slower, and nothing is routed at a size nobody measured: every
    unit stays on the HIP Functions."""
    return False


def get_disp_samples(max_dis, feature_map, stage_id=0, disprity_map=None, step=1, samp_num=9,
                     sample_spa_size=None):
    """submodule.py:376-424, stage-0 branch (:389-390): arange(max_dis) broadcast to
    [B,max_dis,H,W] (an expanded view, nothing is materialised)."""
    if not (disprity_map is None or step == -1 or stage_id == 0):
        raise NotImplementedError(
            "only the stage-0 sampling (arange) is on the hot path; the neighbourhood sampler "
            "(submodule.py:391-411) is never reached by SparseDenseNetRefinementMask")
    B, _, H, W = feature_map.size()
    return torch.arange(int(max_dis), dtype=feature_map.dtype,
                        device=feature_map.device).expand(B, H, W, -1).permute(0, 3, 1, 2)


def _ndhwc_view(x):
    """If x ([B,C,D,H,W]) is a permuted view of a contiguous [B,D,H,W,C] buffer return that
    buffer, else None."""
    y = x.permute(0, 2, 3, 4, 1)
    return y if y.is_contiguous() else None


def _to_ndhwc(x):
    y = _ndhwc_view(x)
    return y if y is not None else ops2d.ncdhw_to_ndhwc(x.contiguous())


class GetCostVolume(nn.Module):
    """forward: compute the cost volume with warped features  (submodule.py:428-562)

    warp_ope="homgrp" with disp_samples = get_disp_samples(stage 0) -- the one call site of the reference
    (SparseDenseNetRefinementMask.py:66, 131) -- and every cost_func: "cor" (demo.sh / eval.sh), "ssd" (demo.py:31's
    default), "cat" (2C channels).  warp_ope="shift" cannot run in the reference either (submodule.py:463 names an
    undefined variable) and is refused.
    return: cost volume, N*C*S*H*W (a view of the channels-last buffer)."""

    def __init__(self, warp_ope="homgrp", cost_func="ssd"):
        super(GetCostVolume, self).__init__()
        assert cost_func in ["ssd", "cor", "cat"], "no such cost_func: {}".format(cost_func)
        self.warp_ope = warp_ope
        self.cost_func = cost_func

    def forward(self, left_feature_map, right_feature_map, **kargs):
        if self.warp_ope != "homgrp":
            raise NotImplementedError("the gfx950 path implements warp_ope='homgrp' (the reference's 'shift' raises "
                                      "NameError, submodule.py:463)")
        if "disp_samples" in kargs and kargs["disp_samples"] is not None:
            ds = kargs["disp_samples"]
            D = int(ds.size(1))
            # the kernel warps by d = 0 .. D-1 (get_disp_samples, stage 0); any other hypotheses would
            # silently give a different volume than submodule.py:479-510, so refuse them (one host
            # sync: this reference-shaped module is not the fast path, Stage0 is)
            ar = torch.arange(D, dtype=ds.dtype, device=ds.device).view(1, D, 1, 1)
            if ds.dim() != 4 or not bool((ds == ar).all()):
                raise NotImplementedError("GetCostVolume on gfx950 takes the stage-0 samples "
                                          "arange(max_disp) only (submodule.py:389-390)")
        else:
            D = int(kargs["max_disp"])
        cv = ops2d.costvol_forward_cf(left_feature_map.contiguous(), right_feature_map.contiguous(), D, self.cost_func)
        return cv.permute(0, 4, 1, 2, 3)


class Conv3dUnit(nn.Module):
    """Parameter container with the reference's layout (submodule.py:90-123): .conv
    (Conv3d k3 s1 p1, no bias) and .bn (BatchNorm3d); executed by CostRegNetNoDown."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, relu=True, bn=True,
                 bn_momentum=0.1, **kwargs):
        super(Conv3dUnit, self).__init__()
        assert kernel_size == 3 and stride == 1 and bn and kwargs.get("padding", 1) == 1
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.stride = stride
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, bias=False,
                              padding=1)
        self.bn = nn.BatchNorm3d(out_channels, momentum=bn_momentum)
        self.relu = relu


class CostRegNetNoDown(CachesWeights, nn.Module):
    """forward: regularise the cost volume  (submodule.py:608-662)
    args:    x: cost volume, N*C*S*H*W
    return:  regularised cost volume, N*S*H*W"""
    _CACHE_ATTRS = cache_attrs("_packed", "_packed_grad") + ("_ws",)

    def __init__(self, in_channels, base_channels, cost_func, down_scale=3):
        super(CostRegNetNoDown, self).__init__()
        self.cost_func = cost_func
        C = in_channels
        if self.cost_func == "cat":                      # submodule.py:618-619
            self.conv_pre = nn.Conv3d(C * 2, C, 1, stride=1, padding=0, bias=False)
        self.conv0 = nn.Sequential(Conv3dUnit(C, C, padding=1), Conv3dUnit(C, C, padding=1))
        self.conv1 = nn.Sequential(Conv3dUnit(C, C, padding=1), Conv3dUnit(C, C, padding=1),
                                   Conv3dUnit(C, C, padding=1))
        self.conv2 = nn.Sequential(Conv3dUnit(C, C, padding=1), Conv3dUnit(C, C, padding=1),
                                   Conv3dUnit(C, 1, padding=1, relu=False))
        self._drop_caches()

    def _drop_caches(self):
        self._packed = None
        self._packed_key = None
        self._packed_src = None
        self._ws = {}
        for a in cache_attrs("_packed_grad"):
            self.__dict__.pop(a, None)

    def __getstate__(self):
        state = super().__getstate__()
        state.update(_packed=None, _packed_key=None, _packed_src=None, _ws={})
        return state

    def units(self):
        return list(self.conv0) + list(self.conv1) + list(self.conv2)

    def _replicate_for_data_parallel(self):
        # torch.nn.DataParallel (eval.py:145-146) shallow-copies __dict__ per replica: the packed weights may be
        # shared (they are keyed by the parameters' pointers and versions), the scratch buffers may not -- replicas
        # run on worker threads at the same time
        r = super()._replicate_for_data_parallel()
        r._ws = {}
        return r

    # ---- parameter preparation (once per weight version): repack + BN folding -----------
    def _sources(self):
        ts = [self.conv_pre.weight] if self.cost_func == "cat" else []
        for u in self.units():
            ts += [u.conv.weight, u.bn.weight, u.bn.bias, u.bn.running_mean, u.bn.running_var]
        return ts

    def prepare(self, D=None):
        """Repack the 7 wide Conv3d weights to [27,Ci,CoP] on the device and fold eval-mode
        BatchNorm into per-channel scale/shift.  Cached until a parameter (or, through the choice
        of algorithm, the depth D of the volume) changes.  The key is source_key's: a write through ``.data`` after
        the first forward needs ``drop_weight_caches``."""
        algo = conv_algo(D)
        return self._cached("_packed", self._sources(), [(float(u.bn.eps), bool(u.relu)) for u in self.units()],
                            lambda: self._pack(algo), head=(algo,))

    def _pack(self, algo):
        units = self.units()
        dev = units[0].conv.weight.device
        if dev.type != "cuda":
            raise _lib.DecnetHipError("CostRegNetNoDown parameters are on %s: move the module to "
                                      "the MI355X (no CPU fallback)" % dev)
        packed = []
        for i, u in enumerate(units):
            w = u.conv.weight.detach().float().contiguous()
            Co, Ci = int(w.shape[0]), int(w.shape[1])
            # the kernels move channels in 16-byte groups: channel counts that are not a
            # multiple of 4 (never the case for the shipped 216-channel net) run zero padded
            cip = (Ci + 3) & ~3
            cop = (Co + 3) & ~3 if i < 7 else 1
            if cip != Ci or cop != Co:
                wpad = torch.zeros((cop, cip) + tuple(w.shape[2:]), dtype=w.dtype, device=dev)
                wpad[:Co, :Ci] = w
                w = wpad
            scale, shift = fold_bn(u.bn)
            if i < 7 and cop != Co:                 # padded output channels stay exactly 0
                scale = torch.cat((scale, torch.ones(cop - Co, device=dev)))
                shift = torch.cat((shift, torch.zeros(cop - Co, device=dev)))
            if i < 7:
                wp = ops2d.conv3d_pack_weight(w)
                wu = ops2d.conv3d_wino_pack_weight(w, WINO_VARIANT[algo]) if algo in WINO_VARIANT else None
                packed.append(dict(w=wp, u=wu, scale=scale.contiguous(), shift=shift.contiguous(),
                                   Ci=cip, Co=cop, relu=1 if u.relu else 0, keep=w))
            else:
                assert Co == 1
                packed.append(dict(w=w, scale=float(scale.item()), shift=float(shift.item()), Ci=cip, Co=1, relu=0))
        if self.cost_func == "cat":
            # conv_pre.weight [C,2C,1,1,1] as [Cp][2 Cp] for the zero-padded feature maps of stage0() (left half in
            # columns [0, C), right half in [Cp, Cp + C)), and as it is for a 2C-channel volume (forward())
            wpre = self.conv_pre.weight.detach().float().reshape(self.conv_pre.weight.shape[0], -1).contiguous()
            C = int(wpre.shape[0])
            cp = (C + 3) & ~3
            if cp != C:
                wp = torch.zeros((cp, 2 * cp), dtype=torch.float32, device=dev)
                wp[:C, :C] = wpre[:, :C]
                wp[:C, cp:cp + C] = wpre[:, C:]
            else:
                wp = wpre
            packed[0]["w_pre"], packed[0]["w_pre_true"] = wp, wpre
        return packed

    def _grow(self, key, n):
        """The grow-only fp32 workspace `key` = (what, ..., device): at least n floats."""
        t = self._ws.get(key)
        if t is None or t.numel() < n:
            t = self._ws[key] = torch.empty(n, dtype=torch.float32, device=key[-1])
        return t

    def run_ndhwc(self, x, want_reg=True, want_pred=True):
        """x: channels-last cost volume [B,D,H,W,C].  Returns (reg [B,D,H,W] or None,
        pred [B,H,W] or None).  The input buffer is not modified."""
        if self._grad_mode(x):
            reg = self._units_grad(x)[-1][..., 0]
            return (reg if want_reg else None), (self._softargmax(reg) if want_pred else None)
        _chk("cost volume", x)
        B, D, H, W, C = x.shape
        algo = conv_algo(D)
        P = self.prepare(D)
        c_true = int(self.units()[0].conv.weight.shape[1])
        if self.cost_func == "cat":                      # submodule.py:651-652: x = conv_pre(x), 2C -> C channels
            if C != 2 * c_true:
                raise ValueError("cost volume has %d channels, module expects %d" % (C, 2 * c_true))
            x, C = ops2d.conv3d_pointwise(x, P[0]["w_pre_true"]), c_true
        if C == c_true and P[0]["Ci"] != C:             # channel count not a multiple of 4: zero pad
            x = torch.nn.functional.pad(x, (0, P[0]["Ci"] - C))
            C = P[0]["Ci"]
        if P[0]["Ci"] != C:
            raise ValueError("cost volume has %d channels, module expects %d" % (C, c_true))
        dev, dims = x.device, (B, D, H, W)
        a, b, c = (self._grow(("act", i, dev), B * D * H * W * C) for i in range(3))
        reg = torch.empty(dims, dtype=torch.float32, device=dev) if want_reg else None
        var = WINO_VARIANT.get(algo)
        wsp = None if var is None else self._grow(("wino", dev), ops2d.size("conv3d_wino_workspace_floats", *dims, C, C, var))

        def conv(i, src, dst, res=None):
            p = P[i]
            ops2d.conv3d_bn_act(src, p["w" if wsp is None else "u"], p["scale"], p["shift"], res, dst, dims, p["Ci"], p["Co"],
                                p["relu"], wsp, var)

        # CostRegNetNoDown.forward submodule.py:650-662
        if not self._run_stack(P, x, c, dims, C, var):
            conv(0, x, a)
            conv(1, a, c)                 # c = output0
            conv(2, c, a)
            conv(3, a, b)
            conv(4, b, a, res=c)          # conv1(output0) + output0
            conv(5, a, b)
            conv(6, b, c)
        p, t = P[7], None
        if p["Ci"] <= 256 and D <= 256:
            need = ops2d.size("conv3d_cout1_workspace_floats", B, D, H, W)
            t = a if a.numel() >= need else self._grow(("scratch", dev), need)     # a is free by now
        pred = ops2d.conv3d_cout1_softargmax(c, p["w"], p["scale"], p["shift"], dims, p["Ci"], reg=reg, ws=t)
        return reg, (pred if want_pred else None)

    def _run_stack(self, P, x, out, dims, C, var):
        """The seven C -> C units as ONE fused stack (decnet_conv3d_wino_stack_bn_act: the activations between the
        layers stay on chip); False when the shape is not covered (the caller then runs the layers one by one).
        DECNET_WINO_STACK=0 turns it off."""
        if var is None or not wino_stack_switch() or any(not p["relu"] or p["Ci"] != C or p["Co"] != C for p in P[:7]):
            return False
        n = ops2d.size("conv3d_wino_stack_workspace_floats", *dims, C, var)
        if n == 0:
            return False
        return ops2d.conv3d_wino_stack_bn_act(x, P[:7], 1, 4, out, self._grow(("wino", x.device), n), dims, C, var)

    def forward(self, x):
        if self._grad_mode(x):
            y = _ndhwc_view(x)                               # (under grad: a differentiable permute, no copy kernel)
            return self.run_ndhwc(y if y is not None else x.permute(0, 2, 3, 4, 1).contiguous(), True, False)[0]
        reg, _ = self.run_ndhwc(_to_ndhwc(x), want_reg=True, want_pred=False)
        return reg

    # ---- the grad path (hip_grad()): one Conv3dFunction per unit (+ BatchNorm3dActFunction in train mode), stage0_grad.py
    def _grad_mode(self, *inputs):
        """Whether this call records a backward: inside ``hip_grad()``, autograd on, and an input or a parameter requires
        grad -- in ``.train()`` mode also: the inputs on the GPU, and every other call is refused.  Raises where a gradient
        is asked for and cannot be had."""
        if self.training:
            if hip_grad_enabled() and torch.is_grad_enabled() and all(t.is_cuda for t in inputs) and (
                    any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())):
                return True
            raise NotImplementedError("CostRegNetNoDown on gfx950 runs in .train() mode (BatchNorm3d on the statistics of the "
                                      "batch) only inside decnet_amd.hip_grad(), on GPU tensors, with autograd on and an "
                                      "input or a parameter that requires grad; for inference call .eval()")
        if not torch.is_grad_enabled():
            return False
        if hip_grad_enabled():
            return any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())
        if any(t.requires_grad for t in inputs):
            raise NotImplementedError("CostRegNetNoDown on gfx950 is inference-only outside decnet_amd.hip_grad(): run under "
                                      "torch.no_grad(), or inside hip_grad() for the gradients of stage 0")
        return False

    def _softargmax(self, reg):
        """disparity_regression over arange(D) in torch ops: reg [B,D,H,W] -> pred [B,H,W]."""
        D = reg.shape[1]
        return (torch.softmax(reg, 1) * torch.arange(D, dtype=reg.dtype, device=reg.device).view(1, D, 1, 1)).sum(1)

    def _pack_grad(self, variant):
        return [stage0_grad.unit_operands(u.conv.weight.detach().float().contiguous(), variant, last=(i == 7))
                for i, u in enumerate(self.units())]

    def _unit_train(self, u, packed, x, voxels):
        """One unit whose ``bn`` is in ``.train()`` mode, on x [B,D,H,W,Ci] -> y [B,D,H,W,Co]: z = conv(x, w) as
        Conv3dFunction with scale 1, shift 0 and no ReLU (no y saved; its backward launches the weight gradient for dW
        alone, and dx on the flipped weights), then BatchNorm3dActFunction on the statistics of the batch, which also
        updates the running statistics; ``num_batches_tracked`` is counted here."""
        bn, w = u.bn, u.conv.weight
        Co = int(w.shape[0])
        if _conv3d_bn_train_slower(int(w.shape[1]), Co, voxels):
            y = stage0_grad.unit_library_train(x, w, bn, bool(u.relu))
        else:
            z = stage0_grad.Conv3dFunction.apply(packed, False, w, torch.ones(Co, device=x.device),
                                                 torch.zeros(Co, device=x.device), x)
            y = stage0_grad.BatchNorm3dActFunction.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                                                         bn.momentum, bool(u.relu))
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
        return y

    def _units_grad(self, x):
        """The eight units on a channels-last volume x [B,D,H,W,C] under autograd -> [y0 .. y6, reg]: every unit's output
        ([B,D,H,W,C]; reg [B,D,H,W,1]), y4 before the residual is added (so that y_i > 0 is unit i's ReLU mask).  The
        forward operands are packed from the weights alone and cached like ``prepare()``'s; scale and shift are
        differentiable expressions of the BatchNorm parameters, formed per call.  A unit whose ``bn`` is in ``.train()``
        mode goes through ``_unit_train``, unit by unit; one whose ``bn`` is in eval mode keeps the frozen route."""
        if self.cost_func == "cat":
            raise NotImplementedError(stage0_grad._REFUSED % "cat")
        units = self.units()
        _chk("cost volume", x.detach())
        B, D, H, W, C = x.shape
        c_true = int(units[0].conv.weight.shape[1])
        if C != c_true:
            raise ValueError("cost volume has %d channels, module expects %d" % (C, c_true))
        if C % 4:
            raise NotImplementedError("the gradients of stage 0 take channel counts in fours (the kernels move channels in "
                                      "16-byte groups); this module has %d" % C)
        variant = WINO_VARIANT.get(conv_algo(D))
        P = self._cached("_packed_grad", [u.conv.weight for u in units], [], lambda: self._pack_grad(variant),
                         head=(variant,))
        ws = None
        if variant is not None:
            ws = self._grow(("wino", x.device), ops2d.size("conv3d_wino_workspace_floats", B, D, H, W, C, C, variant))
        for i, u in enumerate(units):                        # refused before any unit has written a running statistic
            why = stage0_grad.bn_train_refusal(u.bn) if u.bn.training else None
            if why is not None:
                raise NotImplementedError("training-mode BatchNorm3d under hip_grad() takes an affine BatchNorm3d that tracks "
                                          "its running statistics with a float momentum; unit %d has %s" % (i, why))
        outs, cur, keep = [], x, None
        for i, u in enumerate(units):
            if u.bn.training:                                # the statistics of the batch; a frozen bn stays on its route
                y = self._unit_train(u, dict(P[i], ws=ws), cur, B * D * H * W)
            else:
                scale, shift = fold_bn(u.bn)
                if _conv3d_grad_slower(C, B * D * H * W):
                    y = stage0_grad.unit_library(cur, u.conv.weight, scale, shift, bool(u.relu))
                else:
                    y = stage0_grad.Conv3dFunction.apply(dict(P[i], ws=ws), bool(u.relu), u.conv.weight, scale, shift, cur)
            outs.append(y)
            cur = y + keep if i == 4 else y                  # conv1(output0) + output0, after the ReLU
            if i == 1:
                keep = y
        return outs

    def stage0(self, left_feature_map, right_feature_map, max_disp, return_reg=False):
        """SparseDenseNetRefinementMask.forward :127-137 in one call: cost volume (stage-0 ``arange``
        samples) -> this regulariser -> soft-argmax, through the single C entry ``decnet_stage0_forward_cf``
        (one workspace, one ctypes call; the module's cost_func picks the volume).  [B,C,H,W] x2 -> pred [B,H,W] (, reg [B,D,H,W])."""
        if self._grad_mode(left_feature_map, right_feature_map):
            if self.cost_func == "cat":
                raise NotImplementedError(stage0_grad._REFUSED % "cat")
            cv = stage0_grad.CostVolumeFunction.apply(left_feature_map, right_feature_map, int(max_disp), self.cost_func)
            reg = self._units_grad(cv)[-1][..., 0]
            pred = self._softargmax(reg)
            return (pred, reg) if return_reg else pred
        left, right = left_feature_map.contiguous(), right_feature_map.contiguous()
        _chk("left_feature_map", left)
        if left.shape[1] % 4:                           # see prepare()
            padc = (0, 0, 0, 0, 0, 4 - left.shape[1] % 4)
            left = torch.nn.functional.pad(left, padc)
            right = torch.nn.functional.pad(right, padc)
        B, C, H, W = left.shape
        _chk("right_feature_map", right, (B, C, H, W))
        D = int(max_disp)
        algo = conv_algo(D)
        P = self.prepare(D)
        if P[0]["Ci"] != C:
            raise ValueError("feature maps have %d channels, module expects %d"
                             % (left_feature_map.shape[1], int(self.units()[0].conv.weight.shape[1])))
        if any(not p["relu"] for p in P[:7]):
            # decnet_stage0_forward applies ReLU behind each of the seven C -> C units, as the reference's network
            # does (submodule.py:624-648); a unit built with relu=False needs the per-layer path (forward())
            raise _lib.DecnetHipError("decnet_stage0_forward: a Conv3dUnit without ReLU is not covered by the "
                                      "single-entry stage-0 path; use CostRegNetNoDown.forward")
        dev, variant = left.device, WINO_VARIANT.get(algo, 3)
        pk = self._ws.get(("s0params", dev))
        if pk is None or pk[0] is not P or pk[1] != variant:
            sp = _lib.Stage0Params()
            for i in range(7):
                sp.w[i] = P[i]["u"].data_ptr() if variant <= 2 else P[i]["w"].data_ptr()
                sp.scale[i], sp.shift[i] = P[i]["scale"].data_ptr(), P[i]["shift"].data_ptr()
            sp.w_last, sp.scale_last, sp.shift_last = P[7]["w"].data_ptr(), P[7]["scale"], P[7]["shift"]
            pk = self._ws[("s0params", dev)] = (P, variant, sp)
        n = ops2d.size("stage0_cf_workspace_floats", B, C, H, W, D, variant, _lib.COST_FUNC[self.cost_func])
        if n == 0:
            raise _lib.DecnetHipError("decnet_stage0_forward_cf: shape not supported")
        reg = torch.empty((B, D, H, W), dtype=torch.float32, device=dev) if return_reg else None
        pred = ops2d.stage0_forward_cf(left, right, pk[2], P[0]["w_pre"] if self.cost_func == "cat" else None,
                                       self._grow(("s0", dev), n), D, variant, self.cost_func, reg=reg)
        return (pred, reg) if return_reg else pred

    def stage0_buffers(self, dev, B, C, H, W, D):
        """Views of the single-entry workspace (cost volume, first activation buffer, Winograd scratch): what
        bench.py's roofline leg times the dominant kernel on."""
        n = B * D * H * W * C
        act = (n + 63) // 64 * 64
        ws = self._ws[("s0", dev)]
        return ws[:n].view(B, D, H, W, C), ws[act:act + n], ws[4 * act:]


def disparity_regression(cost_vol, disp_samples):
    """submodule.py:766-777: softmax over dim 1, expectation of disp_samples.  N*S*H*W -> N*H*W"""
    cost_vol = cost_vol.contiguous()
    _chk("cost_vol", cost_vol)
    B, S, H, W = cost_vol.shape
    disp_samples = disp_samples.expand(B, S, H, W).contiguous()
    _chk("disp_samples", disp_samples, (B, S, H, W))
    return ops2d.disparity_regression(cost_vol, disp_samples)


class Stage0(nn.Module):
    """The whole stage-0 branch of SparseDenseNetRefinementMask.forward (:127-137) as one
    call: get_disp_samples -> GetCostVolume -> CostRegNetNoDown -> disparity_regression,
    with no [B,C,D,H,W] tensor ever leaving the channels-last workspace.  A thin wrapper of
    ``CostRegNetNoDown.stage0`` (all caches live on the regulariser, keyed by device)."""

    def __init__(self, cost_regularizer):
        super(Stage0, self).__init__()
        self.cost_regularizer = cost_regularizer

    def forward(self, left_feature_map, right_feature_map, max_disp, return_reg=False):
        return self.cost_regularizer.stage0(left_feature_map, right_feature_map, max_disp, return_reg)
