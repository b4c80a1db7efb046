"""V and M of the Winograd stack in ONE buffer: wino_gemm_bf16x3 and wino_mid_transform working in place.  -m gpu.

No arithmetic differs between the in-place and the two-buffer path, so everything here is compared BIT FOR BIT (int32
views: padding lanes may hold anything, NaN included, and must still be the same bits):

  * decnet_conv3d_wino_gemm with M == V against the same call with two buffers, at the row-block edges of the 96-tile
    workgroup (a wave pair that ends early, a half-empty last block, a ragged last wave), three times over -- the hazard
    is a race between the two waves of a row block, and only repeats can show a race;
  * the overlaps the entry must refuse (nothing launched, buffer untouched);
  * the fused stacks under DECNET_WINO_INPLACE=0 and by default (the switch is read once per process: child processes);
  * the default stack called three times on one input.

Run as a script this file is the child process of those tests (see _child_main).
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
C, NP, KC = 216, 216, 14                   # channels, transform points of F(4,3)^3, 16-channel chunks
ERR_UNSUPPORTED = -3
CHILD_TIMEOUT = 300                        # seconds, per child process

# (B, D, H, W), layers, residual.  The last one has nt = 144 tiles: the quad-major in-place GEMM (which only the stacks
# reach) with a half-empty last row block, whose second wave pair ends before the barrier
CONV_CASES = [((2, 8, 20, 36), 7, (1, 4)), ((1, 6, 7, 10), 4, (0, 2)), ((2, 8, 24, 24), 3, (-1, -1))]
COSTVOL_CASES = [(2, 20, 36, 8), (1, 7, 10, 6), (2, 24, 24, 8)]               # (B, H, W, D); 3 layers, residual (0, 1)


def _L():
    from decnet_amd import _lib
    return _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pack(Co, Ci, seed, dev):
    L = _L()
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Co, Ci, 3, 3, 3, generator=g) * (2.0 / (27 * Ci)) ** 0.5).to(dev)
    u = torch.empty(L.decnet_conv3d_wino_weight_floats(Ci, 2), dtype=torch.float32, device=dev)
    assert L.decnet_conv3d_wino_pack_weight(w.data_ptr(), u.data_ptr(), Co, Ci, 2, None) == 0
    torch.cuda.synchronize()
    return u


def _layers(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        scale = (0.5 + torch.rand(C, generator=g)).to(dev)
        shift = (0.2 * torch.randn(C, generator=g)).to(dev)
        out.append(dict(u=_pack(C, C, 1000 * seed + i, dev), scale=scale, shift=shift))
    return out


def _ptrs(layers):
    arr = ctypes.c_void_p * len(layers)
    return [arr(*[p[k].data_ptr() for p in layers]) for k in ("u", "scale", "shift")]


def _conv_stack(layers, x, res, ws=None):
    L = _L()
    B, D, H, W, _ = x.shape
    n = L.decnet_conv3d_wino_stack_workspace_floats(B, D, H, W, C, 2)
    assert n > 0, "shape not covered by the fused stack"
    if ws is None:
        ws = torch.empty(n, dtype=torch.float32, device=x.device)
    y = torch.full_like(x, float("nan"))
    u, sc, sh = _ptrs(layers)
    rc = L.decnet_conv3d_wino_stack_bn_act(x.data_ptr(), u, sc, sh, len(layers), res[0], res[1], y.data_ptr(), ws.data_ptr(),
                                           B, D, H, W, C, 2, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y


def _costvol_stack(layers, left, right, D, res):
    L = _L()
    B, _, H, W = left.shape
    n = L.decnet_conv3d_wino_stack_workspace_floats(B, D, H, W, C, 2)
    assert n > 0, "shape not covered by the fused stack"
    ws = torch.empty(n, dtype=torch.float32, device=left.device)
    y = torch.full((B, D, H, W, C), float("nan"), device=left.device)
    u, sc, sh = _ptrs(layers)
    rc = L.decnet_costvol_wino_stack_bn_act(left.data_ptr(), right.data_ptr(), u, sc, sh, len(layers), res[0], res[1],
                                            y.data_ptr(), ws.data_ptr(), B, C, H, W, D, 2, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y


def _conv_input(shape, dev):
    return torch.randn(*shape, C, generator=torch.Generator().manual_seed(7)).to(dev)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import decnet_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def u216(dev):
    return _pack(C, C, 21, dev)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the GEMM entry in place
@pytest.mark.parametrize("nt", [40, 144, 200])
def test_gemm_in_place_is_the_two_buffer_gemm(dev, u216, nt):
    L = _L()
    g = torch.Generator(device=dev).manual_seed(nt)
    V = torch.randn(NP * KC * nt * 16, generator=g, device=dev)
    M = torch.full_like(V, float("nan"))
    assert L.decnet_conv3d_wino_gemm(V.data_ptr(), u216.data_ptr(), M.data_ptr(), nt, C, C, 2, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(M.view(NP, KC, nt, 16)[:, :13]).any()), "M not fully written"
    runs = []
    for _ in range(3):
        X = V.clone()
        assert L.decnet_conv3d_wino_gemm(X.data_ptr(), u216.data_ptr(), X.data_ptr(), nt, C, C, 2, None) == 0
        torch.cuda.synchronize()
        runs.append(X)
    for i, X in enumerate(runs):
        assert torch.equal(_bits(X), _bits(M)), "in-place run %d differs from the two-buffer result" % i
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[1]), _bits(runs[2]))
    # both forms again with LDS poisoned immediately before the GEMM: the result does not depend on what LDS held
    import _lds_poison
    for pat in _lds_poison.PATTERNS:
        P = _lds_poison.PoisonedLib(L, pat)
        X, M2 = V.clone(), torch.full_like(V, float("nan"))
        assert P.decnet_conv3d_wino_gemm(V.data_ptr(), u216.data_ptr(), M2.data_ptr(), nt, C, C, 2, None) == 0
        assert P.decnet_conv3d_wino_gemm(X.data_ptr(), u216.data_ptr(), X.data_ptr(), nt, C, C, 2, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(M2), _bits(M)), "two-buffer GEMM differs under %s" % _lds_poison.name(pat)
        assert torch.equal(_bits(X), _bits(M)), "in-place GEMM differs under %s" % _lds_poison.name(pat)


# ----------------------------------------------------------------------------------------------------------------------
# 2. overlaps that are refused: the documented code, nothing launched.  The buffers are twice the size of the larger
# operand, so that a launch the entry should have refused would still stay inside them.
def _reject_case(dev, Ci, Co, offset_floats):
    L = _L()
    nt = 40
    u = _pack(Co, Ci, 22, dev)
    n = NP * KC * nt * 16
    buf = torch.randn(2 * n, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    keep = buf.clone()
    rc = L.decnet_conv3d_wino_gemm(buf.data_ptr(), u.data_ptr(), buf.data_ptr() + 4 * offset_floats, nt, Ci, Co, 2, None)
    torch.cuda.synchronize()
    return rc, torch.equal(_bits(buf), _bits(keep))


def test_in_place_with_other_channel_counts_is_refused(dev):
    assert _reject_case(dev, 216, 200, 0) == (ERR_UNSUPPORTED, True)


@pytest.mark.parametrize("offset_floats", [64, NP * KC * 40 * 16 - 4])
def test_partial_overlap_is_refused(dev, offset_floats):
    assert _reject_case(dev, 216, 216, offset_floats) == (ERR_UNSUPPORTED, True)


def _run_child(args, extra_env):
    env = {k: v for k, v in os.environ.items() if k != "DECNET_WINO_INPLACE"}
    return subprocess.Popen([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args],
                            env=dict(env, **extra_env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(p, timeout=CHILD_TIMEOUT):
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.communicate()
        raise
    assert p.returncode == 0, out[-3000:] + err[-3000:]
    return out


def test_in_place_on_the_fp32_kernels_is_refused():
    out = _finish(_run_child(["reject_fp32"], {"DECNET_WINO_GEMM": "fp32"}))
    r = json.loads(out.strip().splitlines()[-1])
    assert r == {"rc": ERR_UNSUPPORTED, "unchanged": True}, r


# ----------------------------------------------------------------------------------------------------------------------
# 3. the stacks, DECNET_WINO_INPLACE=0 against the default
@pytest.fixture(scope="module")
def stack_outputs(tmp_path_factory):
    """Both settings' outputs of every case, from one child process per setting (the two run side by side)."""
    dirs = {k: tmp_path_factory.mktemp("inplace_" + k) for k in ("default", "off")}
    procs = {k: _run_child(["stacks", dirs[k]], extra) for k, extra in (("default", {}), ("off", {"DECNET_WINO_INPLACE": "0"}))}
    try:
        for p in procs.values():
            _finish(p)                       # exit status checked before any file is read
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return dirs


def _same_bytes(dirs, name):
    a, b = (open(os.path.join(str(dirs[k]), name), "rb").read() for k in ("default", "off"))
    assert len(a) > 128 and a == b, "%s: in-place and two-buffer outputs differ" % name


@pytest.mark.parametrize("i", range(len(CONV_CASES)))
def test_conv_stack_switch_on_against_off(stack_outputs, i):
    _same_bytes(stack_outputs, "conv%d.npy" % i)


@pytest.mark.parametrize("i", range(len(COSTVOL_CASES)))
def test_costvol_stack_switch_on_against_off(stack_outputs, i):
    _same_bytes(stack_outputs, "costvol%d.npy" % i)


# ----------------------------------------------------------------------------------------------------------------------
# 4. repeated calls
def test_repeated_calls_give_the_same_output(dev):
    shape, n, res = CONV_CASES[0]
    layers = _layers(n, 100 + n, dev)
    x = _conv_input(shape, dev)
    B, D, H, W = shape
    ws = torch.empty(_L().decnet_conv3d_wino_stack_workspace_floats(B, D, H, W, C, 2), dtype=torch.float32, device=dev)
    ys = [_conv_stack(layers, x, res, ws) for _ in range(3)]
    assert bool(torch.isfinite(ys[0]).all())
    assert torch.equal(_bits(ys[0]), _bits(ys[1])) and torch.equal(_bits(ys[1]), _bits(ys[2]))


# ----------------------------------------------------------------------------------------------------------------------
def _child_main(argv):
    """stacks <dir>: every case of CONV_CASES / COSTVOL_CASES to <dir>/conv<i>.npy, costvol<i>.npy.
    reject_fp32: one JSON line {"rc", "unchanged"} of an in-place GEMM call (the parent sets DECNET_WINO_GEMM=fp32)."""
    import numpy as np
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import decnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "needs the MI355X"
    d = torch.device("cuda:0")
    if argv[0] == "reject_fp32":
        rc, same = _reject_case(d, 216, 216, 0)
        print(json.dumps({"rc": rc, "unchanged": bool(same)}))
        return 0
    assert argv[0] == "stacks"
    out = argv[1]
    for i, (shape, n, res) in enumerate(CONV_CASES):
        y = _conv_stack(_layers(n, 100 + n, d), _conv_input(shape, d), res)
        np.save(os.path.join(out, "conv%d.npy" % i), y.cpu().numpy())
    layers = _layers(3, 11, d)
    for i, (B, H, W, D) in enumerate(COSTVOL_CASES):
        g = torch.Generator().manual_seed(3)
        left = torch.randn(B, C, H, W, generator=g).to(d)
        right = torch.randn(B, C, H, W, generator=g).to(d)
        y = _costvol_stack(layers, left, right, D, (0, 1))
        np.save(os.path.join(out, "costvol%d.npy" % i), y.cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1:]))
