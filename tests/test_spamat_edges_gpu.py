"""The six SpaMat / SpaVar entries of include/decnet_hip.h (csrc/capi.hip -> spamat_mfma.hip, spamat_bwd_mfma.hip,
spamat_wide.hip, spamat_rowtile.hip) through the C ABI at the host dispatch's route edges, against the float64 references
of tests/_spamat_ref.py.  As in tests/test_trunk_edges_gpu.py every case runs with every buffer a window of a
sentinel-guarded buffer, 16-byte aligned and at an odd float offset; each run checks rc, the margins, that the inputs are
bit-unchanged and that every output element is written (NaN pre-fill), and the two placements must be bit-identical.  The
cases marked P also run with one buffer group at a time misaligned (features, masks, forward outputs, grad_output,
disparity, gradients) at W % 4 == 0, where the aligned fast paths are taken: bit-identical to the aligned run.  The bit-mask
entry gets host-packed words (zeros past W) at 8- but not 16-byte alignment and must equal the float-mask fused call bit
for bit.

Bounds against float64 (condition estimates k_* of tests/_spamat_ref.py, u = 2^-24):
  out, variance          |got - ref| <= K_OUT u (k + max(1, |ref|) [+ (W + |mu|) dev for the variance])  per pixel
  sum_similarities       |got - ref| <= K_SUM u (1 + k_sum) |ref|
  max_cost               |got - ref| <= K_MAX u max(k_max, |ref|)
  gradients              |got - ref| <= K_GRAD u max(1, max_pixel k_max) max(1, max|ref|)
                         (grad_disparity + K_GD u (W + D) max|grad_output|: its terms cancel around the mean)
and on well-conditioned cases (relu features, scale <= 1) also the tolerances of tests/test_spamat_gpu.py against the
oracle (disparity 2e-4 px + 1e-5 relative, variance 2e-4 relative + 2e-3, sum_similarities 2e-5 relative, gradients
5e-5 max|grad|).  The constants are
the worst values measured on the MI355X over all cases, the capture replays and the knob legs, with ~3x headroom:
  measured (in units of the bound without its constant): out 27.9 (row-tile kernel under capture, D = 405), variance 16.1
  (fused, mfma_dense), SpaVar variance 8.7, sum_similarities 22.1 (row-tile, D = 405), max_cost 4.6 (C = 72), grad_ref /
  grad_tar 19.1 (D = 400, costs near the floor), grad_disparity 0.24 of its bound (row-tile, D = 216).
The variance bound carries (W + |mu|) sum_d p_d |d - mu|: the matrix-core kernels form d - mu as (pixel position - mu) -
(right position), so its rounding scales with the row position (measured up to 500 u relative on a variance of ~1 at
x ~ 650 without that term; the reference forms (float)d - mu).
The knob legs re-run the cases in child processes under the switches the dispatch reads once per process; where a pinned
kernel does not cover a case the entry returns DECNET_ERR_UNSUPPORTED, and with nothing launched (the bit-mask entry under
rowtile, C > 72 in the backward under mfma / mfma_dense) the outputs keep their NaN pre-fill.  -m gpu."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

import _lds_poison
import _spamat_ref as R
from _placement import ERR_UNSUPPORTED, Place, _bits_equal, _L, _st

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_OUT = 84.0
K_SUM = 64.0
K_MAX = 14.0
K_GRAD = 64.0
K_GD = 16.0

PINNED = os.environ.get("DECNET_SPAMAT_KERNEL", "")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _dev():
    return torch.device("cuda:0")


def _g(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------
# inputs
ON_VALUES = torch.tensor([1.0, 1e-45, -1.0, 0.5, 3e38])
OFF_VALUES = torch.tensor([0.0, -0.0])


def _row_counts(n, W, g):
    m = torch.zeros(W)
    m[torch.randperm(W, generator=g)[:min(n, W)]] = 1.0
    return m


def make_masks(spec, B, H, W, g):
    """spec: "dense"; ("p", p_ref, p_tar) Bernoulli; ("count", [(n_ref, n_tar) per row, cycled]) exact active pixels per
    row side; ("frac", [f per row, cycled]) round(f W) active pixels on both sides; "sides" rows cycling both on, left
    only, right only, both off; ("vals", p) on with probability p, on-values -1, 1e-45, 0.5, 3e38, 1, off-values 0, -0."""
    rows = B * H
    if spec == "dense":
        rm, tm = torch.ones(rows, W), torch.ones(rows, W)
    elif spec == "sides":
        rm, tm = torch.ones(rows, W), torch.ones(rows, W)
        for r in range(rows):
            k = r % 4
            if k in (2, 3):
                rm[r] = 0
            if k in (1, 3):
                tm[r] = 0
    elif spec[0] == "p":
        rm = (torch.rand(rows, W, generator=g) < spec[1]).float()
        tm = (torch.rand(rows, W, generator=g) < spec[2]).float()
    elif spec[0] == "count":
        cyc = spec[1]
        rm = torch.stack([_row_counts(cyc[r % len(cyc)][0], W, g) for r in range(rows)])
        tm = torch.stack([_row_counts(cyc[r % len(cyc)][1], W, g) for r in range(rows)])
    elif spec[0] == "frac":
        cyc = spec[1]
        rm = torch.stack([_row_counts(round(cyc[r % len(cyc)] * W), W, g) for r in range(rows)])
        tm = torch.stack([_row_counts(round(cyc[r % len(cyc)] * W), W, g) for r in range(rows)])
    elif spec[0] == "vals":
        def one():
            on = torch.rand(rows, W, generator=g) < spec[1]
            v_on = ON_VALUES[torch.randint(len(ON_VALUES), (rows, W), generator=g)]
            v_off = OFF_VALUES[torch.randint(len(OFF_VALUES), (rows, W), generator=g)]
            return torch.where(on, v_on, v_off)
        rm, tm = one(), one()
    else:
        raise ValueError(spec)
    return rm.reshape(B, H, W).contiguous(), tm.reshape(B, H, W).contiguous()


def make_feats(spec, B, C, H, W, D, g):
    """relu: relu(N(0,1)); signed: 0.5 N(0,1); zero; peak0 / peakD / peakx: a sharp peak at d = 0, d = D - 1, d = x (the
    right image's first pixel); neg15: every cost ~ -15 (all e_d ~ 3e-7: the sums sit near the 1e-6 floor); big: costs ~1e3."""
    if spec == "relu":
        return torch.relu(torch.randn(B, C, H, W, generator=g)), torch.relu(torch.randn(B, C, H, W, generator=g))
    if spec == "signed":
        return 0.5 * torch.randn(B, C, H, W, generator=g), 0.5 * torch.randn(B, C, H, W, generator=g)
    if spec == "zero":
        return torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    if spec == "big":
        s = (2000.0 / C) ** 0.5
        return s * torch.relu(torch.randn(B, C, H, W, generator=g)), s * torch.relu(torch.randn(B, C, H, W, generator=g))
    if spec == "neg15":
        a = (15.0 / C) ** 0.5
        L = a * (1 + 0.05 * torch.randn(B, C, H, W, generator=g))
        return L, -a * (1 + 0.05 * torch.randn(B, C, H, W, generator=g))
    L = torch.randn(B, C, H, W, generator=g)
    L = 1.5 * L / L.norm(dim=1, keepdim=True).clamp_min(1e-3)
    Rt = 0.3 * torch.randn(B, C, H, W, generator=g)
    if spec == "peak0":
        Rt = Rt + 2 * L
    elif spec == "peakD":
        k = min(D - 1, W - 1)
        Rt[..., :W - k] += 2 * L[..., k:]
    elif spec == "peakx":
        u = L[..., :1].clone()
        L = u.expand_as(L) + 0.2 * torch.randn(B, C, H, W, generator=g)
        Rt[..., :1] = 3 * u
    else:
        raise ValueError(spec)
    return L, Rt


# ------------------------------------------------------------------------------------------------------------------
# cases: (B, C, H, W, D, masks, feats, disparity, P)    disparity: "near" out + N(0,1), "neg" < 0, "above" > D
# NT = the band kernels' tile count: need = (D - 1 + 15) / 16 + 1 -> forward NT 3 / 6 / 8 / 11 / 15 / 18 up to D = 33 / 81 /
# 113 / 161 / 225 / 273, backward NT 3 / 6 / 11 / 15 / 18 (no 8); wide banding above 273.  Forward KQ by C: 2 (5 - 8), 6
# (21 - 24), 18 (69 - 72), 0 (generic K loop) otherwise; backward: C <= 8 KQ 2, <= 24 KQ 6, <= 72 KQ 18, row-tile above.
# Backward at C <= 24 (rows of <= 2048 pixels): rows with <= 256 active pixels on both sides on the sparse-row kernel, rows
# of 257 - 640 at C <= 8 (W <= 1024) on its 640-slot form, the rest on spamat_bwd_rowb (SpaMat; W >= 16 NT, NT <= 15 at
# C <= 8 (CB 1), NT <= 11 at 9 - 16 (CB 2) / 17 - 24 (CB 3)) or the band kernels.
CASES = [
    # ---- D: the NT template edges (C = 8: forward KQ 2 with the sparse pre-launch, backward rowb CB 1)
    (1, 8, 1, 5, 1, "dense", "relu", "near", 0),               # D = 1: one candidate, NT 3
    (1, 8, 2, 17, 2, "dense", "signed", "near", 0),            # D = 2, W 17
    (1, 8, 1, 700, 16, "dense", "relu", "near", 1),            # NT 3, rowb CB 1 (> 640 active: not the mid rows)
    (1, 8, 1, 64, 17, ("p", 0.6, 0.6), "signed", "neg", 0),    # NT 3, SpaVar disparity < 0
    (1, 8, 1, 700, 33, "dense", "relu", "near", 0),            # NT 3 (last)
    (1, 8, 1, 701, 34, "dense", "relu", "above", 0),           # NT 6, SpaVar disparity > D
    (1, 24, 1, 300, 81, "dense", "relu", "near", 1),           # NT 6 (last), KQ 6, rowb CB 3 NT 6
    (1, 24, 1, 300, 82, "dense", "signed", "near", 0),         # forward NT 8, backward NT 11, rowb CB 3 NT 11
    (1, 5, 1, 700, 113, "dense", "relu", "near", 1),           # forward NT 8 (last), backward NT 11 rowb CB 1
    (1, 5, 1, 700, 114, ("p", 0.95, 0.95), "signed", "near", 0),  # forward NT 11
    (1, 16, 1, 320, 161, "dense", "relu", "near", 1),          # NT 11 (last): rowb CB 2 at NT 11
    (1, 16, 1, 320, 162, "dense", "relu", "near", 0),          # NT 15: no rowb at C 9 - 16, the band launch
    (1, 8, 1, 700, 225, "dense", "relu", "near", 1),           # NT 15 (last): rowb CB 1 at NT 15
    (1, 8, 1, 700, 226, "dense", "signed", "near", 0),         # NT 18: no rowb
    (1, 8, 1, 400, 273, "dense", "relu", "near", 0),           # NT 18 (last): still one band
    (1, 8, 1, 400, 274, "dense", "relu", "near", 1),           # wide: 2 bands of 137
    (1, 4, 1, 600, 544, ("p", 0.8, 0.8), "relu", "near", 0),   # wide: 2 bands of 272
    (1, 4, 1, 600, 545, ("p", 0.8, 0.8), "signed", "near", 0),  # wide: 3 bands of 182
    (1, 8, 2, 100, 216, "dense", "relu", "near", 0),           # D > W: cur = x + 1 everywhere
    (1, 3, 1, 40, 300, ("p", 0.7, 0.7), "signed", "near", 0),   # D > W above 273: wide bands of empty candidates
    # ---- C: the KQ templates (forward) and channel blocks (backward), D = 40 (NT 6), dense rows of W = 700 at C <= 8 (past
    # the mid rows' 640), 300 above (past the sparse rows' 256): the backward leaves them to rowb / the band kernels
    (1, 1, 1, 700, 40, "dense", "relu", "near", 0),            # KQ 0 / bwd KQ 2 CB 1
    (1, 3, 1, 700, 40, "dense", "signed", "near", 0),
    (1, 4, 1, 700, 40, "dense", "relu", "near", 1),            # KQ 0 (last below 5)
    (1, 5, 1, 700, 40, ("p", 0.9, 0.9), "relu", "near", 0),    # KQ 2 (first)
    (1, 8, 1, 700, 40, "dense", "relu", "near", 0),            # KQ 2 (last), bwd CB 1 (last)
    (1, 9, 1, 300, 40, "dense", "relu", "near", 0),            # KQ 0, bwd KQ 6 CB 2 (first)
    (1, 16, 1, 300, 40, "dense", "signed", "near", 0),         # bwd CB 2 (last)
    (1, 17, 1, 300, 40, "dense", "relu", "near", 0),           # bwd CB 3 (first)
    (1, 20, 1, 300, 40, "dense", "relu", "near", 1),           # KQ 0 (last below 21)
    (1, 21, 1, 300, 40, "dense", "relu", "near", 0),           # KQ 6 (first)
    (1, 24, 1, 300, 40, ("p", 0.9, 0.9), "signed", "near", 0),  # KQ 6 (last), bwd CB 3 (last)
    (1, 25, 1, 300, 40, "dense", "relu", "near", 0),           # KQ 0, bwd KQ 18 band
    (1, 68, 1, 300, 40, "dense", "relu", "near", 0),           # KQ 0 (last below 69)
    (1, 69, 1, 300, 40, "dense", "signed", "near", 0),         # KQ 18 (first)
    (1, 72, 1, 300, 40, "dense", "relu", "near", 1),           # KQ 18 (last), bwd KQ 18 (last)
    (1, 73, 1, 300, 40, ("p", 0.8, 0.8), "relu", "near", 0),   # KQ 0, bwd row-tile (C > 72)
    # ---- W: tiny rows, tile edges, the rowb width limits, segments, the marker limit
    (1, 8, 1, 1, 4, "dense", "relu", "near", 0),               # W 1: no mask-bit hand-over (2 ceil(W/32) > W)
    (1, 8, 1, 2, 4, "dense", "relu", "near", 0),               # W 2: hand-over (first)
    (1, 8, 1, 3, 4, "dense", "signed", "near", 0),
    (1, 8, 1, 5, 4, ("p", 0.8, 0.8), "relu", "near", 0),
    (1, 8, 1, 15, 10, "dense", "relu", "near", 0),
    (1, 8, 1, 16, 10, "dense", "relu", "near", 0),
    (1, 8, 1, 17, 10, "dense", "relu", "near", 0),
    (1, 8, 1, 31, 24, "dense", "signed", "near", 0),
    (1, 8, 1, 32, 24, "dense", "relu", "near", 0),
    (1, 8, 1, 33, 24, "dense", "relu", "near", 0),
    (1, 8, 1, 63, 24, "dense", "relu", "near", 0),
    (1, 8, 1, 64, 24, "dense", "relu", "near", 0),
    (1, 8, 1, 65, 24, ("p", 0.9, 0.9), "relu", "near", 0),
    # the rowb width limit W >= 16 NT: rows of <= 256 pixels always take the backward's sparse-row kernel (<= 256 active
    # pixels per side; 640 at C <= 8), so below 257 pixels rowb is never reached and above it the limit (<= 240) always
    # holds; the forward runs its band kernel on these dense rows
    (1, 8, 1, 239, 200, "dense", "relu", "near", 0),           # NT 15: W = 16 NT - 1
    (1, 8, 1, 240, 200, "dense", "relu", "near", 1),           # NT 15: W = 16 NT
    (1, 20, 1, 175, 150, "dense", "relu", "near", 0),          # NT 11 at CB 3
    (1, 20, 1, 176, 150, "dense", "signed", "near", 1),
    (1, 8, 1, 641, 200, "dense", "relu", "near", 0),           # the first width that reaches rowb at C <= 8 (NT 15, CB 1)
    (1, 20, 1, 257, 150, "dense", "relu", "near", 0),          # ... at C 9 - 24 (NT 11, CB 3)
    (1, 13, 1, 257, 40, "dense", "signed", "near", 0),         # ... at NT 6, CB 2
    (1, 8, 1, 1024, 216, "dense", "relu", "near", 1),          # 64 tiles: one segment, ppt 4
    (1, 8, 1, 1025, 216, "dense", "relu", "near", 0),          # 65 tiles: segmented rows, ppt 8
    (1, 8, 1, 2048, 100, ("p", 0.5, 0.5), "relu", "near", 0),  # the sparse-row pre-launch (last)
    (1, 8, 1, 2049, 100, ("p", 0.5, 0.5), "relu", "near", 0),  # no pre-launch (W > 2048): compaction in the band kernel
    # ---- masks: exact active counts per row side (sparse <= 256, mid 257 - 640, C <= 8, W <= 1024 in the backward)
    (1, 8, 4, 1024, 100, ("count", [(0, 0), (1, 1), (256, 256), (257, 257)]), "relu", "near", 0),
    (1, 8, 4, 1024, 100, ("count", [(512, 512), (513, 513), (640, 640), (641, 641)]), "relu", "near", 0),
    (1, 8, 4, 1000, 216, ("count", [(256, 641), (641, 256), (257, 1), (0, 513)]), "signed", "near", 0),
    (1, 24, 2, 800, 72, ("count", [(256, 256), (257, 257)]), "relu", "near", 0),
    # pair densities on both sides of sparse_pct 45 % (C 5 - 8) and compact_pct 35 % (no pre-launch: C = 24, 72)
    (1, 8, 2, 300, 216, ("frac", [0.65, 0.69]), "relu", "near", 0),
    (1, 24, 2, 300, 72, ("frac", [0.58, 0.61]), "relu", "near", 0),
    (1, 72, 2, 120, 40, ("frac", [0.58, 0.61]), "relu", "near", 0),
    (2, 8, 2, 64, 40, "sides", "relu", "near", 0),             # both on / left only / right only / both off
    # mask values other than 0 / 1: -1, 1e-45, 0.5, 3e38 on; -0.0 off; with and without the hand-over
    (1, 72, 1, 100, 40, ("vals", 1.0), "relu", "near", 0),     # KQ 18: the band kernel reads the float planes
    (1, 8, 2, 300, 216, ("vals", 0.9), "relu", "near", 0),
    (1, 8, 2, 1100, 100, ("vals", 0.9), "relu", "near", 0),    # segmented rows: no hand-over
    (1, 8, 2, 400, 100, ("vals", 0.3), "signed", "near", 0),   # sparse rows, both directions
    (1, 24, 2, 300, 72, ("vals", 0.3), "relu", "near", 0),
    (1, 8, 1, 500, 300, ("vals", 0.8), "relu", "near", 0),     # wide (masks shifted band by band)
    # ---- inputs: exact flat softmax, sharp peaks, costs near the floor, big costs, B up to 3
    (1, 8, 1, 300, 216, "dense", "zero", "near", 0),
    (1, 8, 1, 420, 300, ("p", 0.8, 0.8), "zero", "near", 0),
    (1, 8, 1, 200, 100, "dense", "peak0", "near", 0),
    (1, 8, 1, 200, 100, "dense", "peakD", "near", 0),
    (1, 8, 1, 200, 100, "dense", "peakx", "near", 0),
    (1, 8, 1, 300, 200, "dense", "neg15", "near", 0),          # single band near the 1e-6 floor
    (1, 8, 1, 500, 400, "dense", "neg15", "near", 0),          # wide, near the floor: the c_X term of merge_band_fused
    (1, 8, 1, 200, 100, ("p", 0.7, 0.7), "big", "near", 0),
    (3, 8, 1, 97, 50, ("p", 0.7, 0.7), "signed", "near", 0),
    (3, 24, 2, 51, 30, "dense", "relu", "neg", 0),
]
IDS = ["%d-B%dC%dH%dW%dD%d" % ((i,) + c[:5]) for i, c in enumerate(CASES)]
FWD_KEYS = ("m_out", "m_S", "m_max", "v_var", "v_S", "v_max", "f_out", "f_var", "f_S", "f_max")
BITS_KEYS = ("b_out", "b_var", "b_S", "b_max")
GRAD_KEYS = ("m_gl", "m_gr", "v_gl", "v_gr", "v_gd")
GROUPS = ("feat", "mask", "fout", "gout", "disp", "grad")


def _well(case):
    return case[6] == "relu"


def pack_bits(m):
    """[B,H,W] float mask -> int64 [B,H,ceil(W/64)]: bit i of word w = pixel 64 w + i on, zeros past W."""
    B, H, W = m.shape
    nw = (W + 63) // 64
    on = torch.zeros(B, H, nw * 64, dtype=torch.int64)
    on[..., :W] = (m != 0).long()
    words = on.view(B, H, nw, 64)
    w = torch.zeros(B, H, nw, dtype=torch.int64)
    for i in range(64):
        w |= words[..., i] << i          # (bit 63 wraps into the sign: the same 64 bits)
    return w


_REF = {}


def inputs_of(case):
    """Host inputs and the float64 reference of a case (cached per process)."""
    key = tuple(map(repr, case))
    if key in _REF:
        return _REF[key]
    B, C, H, W, D, mspec, fspec, dspec, _ = case
    g = _g("spamat-edges", case)
    L, Rt = make_feats(fspec, B, C, H, W, D, g)
    rm, tm = make_masks(mspec, B, H, W, g)
    gout = torch.randn(B, H, W, generator=g)                          # nonzero at ref-off pixels too
    r0 = R.forward(L, Rt, rm, tm, D)
    if dspec == "near":
        mu = (r0["out"] + torch.randn(B, H, W, generator=g, dtype=torch.float64)).float()
    elif dspec == "neg":
        mu = -5.0 - 3 * torch.rand(B, H, W, generator=g)
    else:
        mu = D + 5.0 + 3 * torch.rand(B, H, W, generator=g)
    ref = R.forward(L, Rt, rm, tm, D, disparity=mu)
    m32 = {k: ref[k].float() for k in ("out", "S", "max_cost", "var")}
    gl, gr = R.backward(L, Rt, rm, tm, m32["out"], m32["S"], m32["max_cost"], gout, D)
    vl, vr, vd = R.backward(L, Rt, rm, tm, m32["var"], m32["S"], m32["max_cost"], gout, D, disparity=mu)
    x = dict(L=L, R=Rt, rm=rm, tm=tm, g=gout, mu=mu, rbits=pack_bits(rm), tbits=pack_bits(tm), m32=m32, ref=ref,
             grads={"m_gl": gl, "m_gr": gr, "v_gl": vl, "v_gr": vr, "v_gd": vd})
    _REF[key] = x
    return x


def expect_bits_rc():
    return ERR_UNSUPPORTED if PINNED == "rowtile" else 0


def expect_bwd_rc(C):
    return ERR_UNSUPPORTED if PINNED in ("mfma", "mfma_dense") and C > 72 else 0


def run(case, mis):
    """All six entries on one case.  mis: None (everything aligned), "all" (everything at an odd float offset) or one of
    GROUPS (that group misaligned, the rest aligned).  -> dict of host results (outputs of rejected calls: absent)."""
    B, C, H, W, D = case[:5]
    x = inputs_of(case)
    dev = _dev()
    L, st = _L(), _st()
    P = {k: Place(dev, not (mis == "all" or mis == k)) for k in GROUPS}
    rej = Place(dev, True)                      # outputs of calls expected to launch nothing
    pb = Place(dev, False)                      # the bit-mask words: 8- but not 16-byte aligned
    ld, rd = P["feat"].inp(x["L"]), P["feat"].inp(x["R"])
    rmd, tmd = P["mask"].inp(x["rm"]), P["mask"].inp(x["tm"])
    rb, tb = pb.inp(x["rbits"]), pb.inp(x["tbits"])
    assert rb.data_ptr() % 8 == 0 and rb.data_ptr() % 16 != 0
    mud = P["disp"].inp(x["mu"])
    gd = P["gout"].inp(x["g"])
    o, s, m, v = (P["fout"].inp(x["m32"][k]) for k in ("out", "S", "max_cost", "var"))
    pl = (B, H, W)
    outs = {}
    for k in FWD_KEYS:
        outs[k] = P["fout"].out(pl)
    brc = expect_bits_rc()
    for k in BITS_KEYS:
        outs[k] = (P["fout"] if brc == 0 else rej).out(pl)
    bwrc = expect_bwd_rc(C)
    gp = P["grad"] if bwrc == 0 else rej
    for k in ("m_gl", "m_gr", "v_gl", "v_gr"):
        outs[k] = gp.out((B, C, H, W))
    outs["v_gd"] = gp.out(pl)
    a = (B, C, H, W, D)
    p = lambda k: outs[k].data_ptr()                                  # noqa: E731
    rc = {}
    rc["m"] = L.decnet_spamat_forward(ld.data_ptr(), rd.data_ptr(), rmd.data_ptr(), tmd.data_ptr(), p("m_out"), p("m_S"),
                                      p("m_max"), *a, st)
    rc["v"] = L.decnet_spavar_forward(ld.data_ptr(), rd.data_ptr(), rmd.data_ptr(), tmd.data_ptr(), mud.data_ptr(),
                                      p("v_var"), p("v_S"), p("v_max"), *a, st)
    rc["f"] = L.decnet_spamatvar_forward(ld.data_ptr(), rd.data_ptr(), rmd.data_ptr(), tmd.data_ptr(), p("f_out"),
                                         p("f_var"), p("f_S"), p("f_max"), *a, st)
    rc["b"] = L.decnet_spamatvar_forward_bits(ld.data_ptr(), rd.data_ptr(), rb.data_ptr(), tb.data_ptr(), p("b_out"),
                                              p("b_var"), p("b_S"), p("b_max"), *a, st)
    rc["mb"] = L.decnet_spamat_backward(ld.data_ptr(), rd.data_ptr(), rmd.data_ptr(), tmd.data_ptr(), o.data_ptr(),
                                        s.data_ptr(), m.data_ptr(), gd.data_ptr(), p("m_gl"), p("m_gr"), *a, st)
    rc["vb"] = L.decnet_spavar_backward(ld.data_ptr(), rd.data_ptr(), rmd.data_ptr(), tmd.data_ptr(), mud.data_ptr(),
                                        v.data_ptr(), s.data_ptr(), m.data_ptr(), gd.data_ptr(), p("v_gl"), p("v_gr"),
                                        p("v_gd"), *a, st)
    want = {"m": 0, "v": 0, "f": 0, "b": brc, "mb": bwrc, "vb": bwrc}
    assert rc == want, (case, mis, rc)
    what = "%s mis=%s" % (case[:5], mis)
    for k, pp in P.items():
        pp.check("%s group %s" % (what, k))
    pb.check(what + " bits")
    rej.check_untouched(what + " rejected call")
    skip = (BITS_KEYS if brc else ()) + (GRAD_KEYS if bwrc else ())
    return {k: t.cpu() for k, t in outs.items() if k not in skip}


def _within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (float64)."""
    err = (got.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements out of bound, worst err %.3g (bound there %.3g, ratio %.3g)" % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad][err[bad].argmax()]),
        float((err / bound.clamp_min(1e-300)).max()))


def check_values(case, r):
    x = inputs_of(case)
    ref = x["ref"]
    well = _well(case)
    W, D = case[3], case[4]

    def q(got, key, kkey, what, dev=None, mu=None):
        b = ref[kkey] + ref[key].abs().clamp_min(1.0)
        if dev is not None:                                           # d - mu formed from pixel positions (<= W)
            b = b + (W + mu.abs()) * ref[dev]
        _within(got, ref[key], K_OUT * U * b, "%s %s" % (case[:5], what))
        if well:
            tol = 2e-4 + 1e-5 * ref[key].abs() if key == "out" else 2e-3 + 2e-4 * ref[key].abs()
            _within(got, ref[key], tol, "%s %s (oracle tolerance)" % (case[:5], what))

    def s_m(got_s, got_m, what):
        _within(got_s, ref["S"], K_SUM * U * (1 + ref["k_sum"]) * ref["S"], "%s %s sum" % (case[:5], what))
        _within(got_m, ref["max_cost"], K_MAX * U * torch.maximum(ref["k_max"], ref["max_cost"].abs()),
                "%s %s max_cost" % (case[:5], what))
        if well:
            _within(got_s, ref["S"], 2e-5 * ref["S"], "%s %s sum (oracle tolerance)" % (case[:5], what))

    q(r["m_out"], "out", "k_out", "spamat out")
    s_m(r["m_S"], r["m_max"], "spamat")
    q(r["v_var"], "var", "k_var", "spavar var", "dev", x["mu"].double())
    s_m(r["v_S"], r["v_max"], "spavar")
    q(r["f_out"], "out", "k_out", "fused out")
    q(r["f_var"], "var_self", "k_var_self", "fused var", "dev_self", ref["out"])
    s_m(r["f_S"], r["f_max"], "fused")
    if "b_out" in r:
        for k in ("out", "var", "S", "max"):
            assert _bits_equal(r["b_" + k], r["f_" + k]), "%s: bit-mask %s differs from the float-mask call" % (case[:5], k)
    if "m_gl" in r:
        cond = max(1.0, float(ref["k_max"].max()))
        gmax = float(x["g"].abs().max())
        for k, t in x["grads"].items():
            sc = max(1.0, float(t.abs().max()))
            b = K_GRAD * U * cond * sc
            if k == "v_gd":                           # -2 g sum_d e_d (d - mu) / S: terms up to D, cancelling at the mean
                b += K_GD * U * (W + D) * gmax
            _within(r[k], t, torch.full_like(t, b), "%s %s" % (case[:5], k))
            if well:
                _within(r[k], t, torch.full_like(t, 5e-5 * sc), "%s %s (oracle tolerance)" % (case[:5], k))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spamat_edges(dev, case):
    a = run(case, None)
    u = run(case, "all")
    for k in a:
        assert _bits_equal(a[k], u[k]), "%s: %s differs between aligned and unaligned placement" % (case[:5], k)
    # both placements again with LDS poisoned before each of the six entries, under each pattern: bit-identical to `a`
    _lds_poison.sweep(lambda mis: run(case, mis), a, placements=((None, "aligned"), ("all", "unaligned")))
    if case[8]:
        assert case[3] % 4 == 0
        for grp in GROUPS:
            p = run(case, grp)
            for k in a:
                assert _bits_equal(a[k], p[k]), "%s: %s differs with group %s misaligned" % (case[:5], k, grp)
    check_values(case, a)


# ------------------------------------------------------------------------------------------------------------------
# graph capture: above D = 273 the wide entries decline while the stream is capturing and the float-mask entries fall
# back to the row-tile kernels; the bit-mask entry returns -3 there with nothing enqueued
@pytest.mark.parametrize("D", [273, 274, 405])
def test_capture_replays_within_the_float64_bounds(dev, D):
    case = (1, 8, 2, 460, D, ("p", 0.8, 0.8), "relu", "near", 0)
    B, C, H, W = case[:4]
    x = inputs_of(case)
    L = _L()
    t = {k: x[k].to(dev) for k in ("L", "R", "rm", "tm", "g", "mu", "rbits", "tbits")}
    fw = {k: x["m32"][k].to(dev) for k in ("out", "S", "max_cost", "var")}
    pl, fl = (B, H, W), (B, C, H, W)

    def outs():
        o = {k: torch.full(pl, float("nan"), device=dev) for k in FWD_KEYS + BITS_KEYS + ("v_gd",)}
        o.update({k: torch.full(fl, float("nan"), device=dev) for k in ("m_gl", "m_gr", "v_gl", "v_gr")})
        return o

    def calls(o):
        st = _st()
        a = (B, C, H, W, D)
        p = lambda k: o[k].data_ptr()                                 # noqa: E731
        lr = (t["L"].data_ptr(), t["R"].data_ptr())
        mk = (t["rm"].data_ptr(), t["tm"].data_ptr())
        return {
            "m": L.decnet_spamat_forward(*lr, *mk, p("m_out"), p("m_S"), p("m_max"), *a, st),
            "v": L.decnet_spavar_forward(*lr, *mk, t["mu"].data_ptr(), p("v_var"), p("v_S"), p("v_max"), *a, st),
            "f": L.decnet_spamatvar_forward(*lr, *mk, p("f_out"), p("f_var"), p("f_S"), p("f_max"), *a, st),
            "b": L.decnet_spamatvar_forward_bits(*lr, t["rbits"].data_ptr(), t["tbits"].data_ptr(), p("b_out"),
                                                 p("b_var"), p("b_S"), p("b_max"), *a, st),
            "mb": L.decnet_spamat_backward(*lr, *mk, fw["out"].data_ptr(), fw["S"].data_ptr(), fw["max_cost"].data_ptr(),
                                           t["g"].data_ptr(), p("m_gl"), p("m_gr"), *a, st),
            "vb": L.decnet_spavar_backward(*lr, *mk, t["mu"].data_ptr(), fw["var"].data_ptr(), fw["S"].data_ptr(),
                                           fw["max_cost"].data_ptr(), t["g"].data_ptr(), p("v_gl"), p("v_gr"),
                                           p("v_gd"), *a, st),
        }
    rc = calls(outs())                                          # eager (loads every code object before the capture)
    assert rc == {"m": 0, "v": 0, "f": 0, "b": expect_bits_rc(), "mb": 0, "vb": 0}, rc
    torch.cuda.synchronize()
    o = outs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = calls(o)
    want_b = expect_bits_rc() if D <= 273 else ERR_UNSUPPORTED
    assert rc == {"m": 0, "v": 0, "f": 0, "b": want_b, "mb": 0, "vb": 0}, rc
    graph.replay()
    torch.cuda.synchronize()
    r = {k: v.cpu() for k, v in o.items()}
    if want_b:
        for k in BITS_KEYS:
            assert bool(torch.isnan(r.pop(k)).all()), "the declined bit-mask call enqueued work"
    for k, v in r.items():
        assert not bool(torch.isnan(v).any()), "%s not written by the replay" % k
    check_values(case, r)


# ------------------------------------------------------------------------------------------------------------------
KNOBS = [  # environment switches read once per process, and the cases they change
    ({"DECNET_SPAMAT_KERNEL": "rowtile"}, "B1C8 or C24 or C72 or C73 or capture"),
    ({"DECNET_SPAMAT_KERNEL": "mfma"}, "not capture"),
    ({"DECNET_SPAMAT_KERNEL": "mfma_dense"}, "C8 or C24 or C72 or C73"),
    ({"DECNET_SPAMAT_DENSE": "fp32"}, "C8 or C5"),
    ({"DECNET_SPAMAT_MID": "0"}, "W1024 or W1000 or W300"),
    ({"DECNET_SPAMAT_HANDOVER": "0"}, "C8"),
]


@pytest.mark.parametrize("env,sel", KNOBS, ids=["rowtile", "mfma", "mfma_dense", "dense_fp32", "mid0", "handover0"])
def test_knob_leg(env, sel):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p",
                        "no:cacheprovider", "-k", "(%s) and not knob_leg and not handover_off" % sel],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


HANDOVER_CASES = [i for i, c in enumerate(CASES) if 5 <= c[1] <= 8 and c[3] <= 1024]


def test_handover_off_is_bit_identical(dev, tmp_path):
    """DECNET_SPAMAT_HANDOVER=0 (the band kernel reads the float planes again instead of the sparse-row kernel's activity
    bits): every output of every entry bit-identical to this process's default run."""
    path = str(tmp_path / "handover0.pt")
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, test_spamat_edges_gpu as T\n"
            "torch.save({i: T.run(T.CASES[i], None) for i in %r}, %r)\n") % (
        [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],
        HANDOVER_CASES, path)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DECNET_SPAMAT_HANDOVER="0"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    other = torch.load(path)
    for i in HANDOVER_CASES:
        a = run(CASES[i], None)
        for k in a:
            assert _bits_equal(a[k], other[i][k]), "%s: %s differs with the hand-over off" % (CASES[i][:5], k)
