"""Exact data for the SpaMat / SpaVar backward: a host model of the arithmetic of spamat_bwd_rowb (csrc/spamat_bwd_mfma.hip),
value classes for its TRUNCATING three-term split, and the case tables and data of tests/test_spamat_exact_gpu.py (bit for
bit against the float64 reference on the MI355X) and tests/test_spamat_exact_cpu.py (which proves on the host that those
cases have teeth).  The expectation of every GPU case is tests/_spamat_ref.backward in float64, never the model.

The kernel.  Both views, the g/S-scaled left image G = fl(L g/S) and the weights w = e (d - out) are split into three bf16
terms x = h + m + l by truncation (rb_split3).  Of the nine term products of each of its three matrix products it keeps
KEPT: the first letter names the term of the first operand, the second the term of the second operand, and the operands are
  cost  (right view R, left view L)       hh hm mh mm | hl lh lm      one K group q of the two MFMAs per product (COST_Q)
  gl    (weight w, right view R)          (w_h + w_m)(R_h | R_m), w_h R_l + w_l (R_h | R_m);  K group q = right pixels 4q..4q+3
  gr    (weight w, scaled left image G)   the same seven;  K groups q, q + 2 = left pixels 8 (q & 1) .. + 7 of the tile,
                                          w_h in groups 0, 1 and w_m (MFMA 1) / w_l (MFMA 2) in groups 2, 3
A left pixel x and a right pixel x' = x - d meet in band tile m = (x >> 4) - (x' >> 4) of left tile x >> 4; the right tile
x' >> 4 belongs to wave (x' >> 4) & 3 and lives in ring slot (x' >> 4) & (RING - 1).

Classes (truncating split, so not those of tests/_exact.py, which rounds to nearest):
  K1  one term:    +-2^e
  K2  two terms:   +-2^e (1 + k 2^-10), k in 1..3       (h = +-2^e, m = the rest, l = 0)
  K3  three terms: a 24-bit significand with m != 0 and l != 0 (l always fits bf16: 8 + 8 + 8 bits)
Families (docs/rounds/spamat_exact.md): 3 cost terms -- the selector plus one data channel with a class pair on (R, L), live
cost 1 + R L imposed as max_cost, grad_ref's selector channel within cost_bound per element; 1 flat dense -- integer features with disjoint channel supports, every cost 0, every
e 1, every partial sum exact in any order; 2 selectors -- one live candidate per left pixel, every gradient element ONE
product g/S w view with (w, view) from (K3, K1), (K1, K3), (K2, K2).

`python tests/_spamat_exact.py --table` prints the ablation table of DESIGN.md section 2."""
import collections
import itertools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spamat_ref as R                                              # noqa: E402
from _exact import exact_or_fail, gen, ints                          # noqa: E402,F401

F64 = torch.float64
LOG2E = float(np.float32(1.4426950408889634))
KEPT = ("hh", "hm", "mh", "mm", "hl", "lh", "lm")
NOT_PINNED = {"cost": ("lm",), "gl": ("lm",), "gr": ("lm",)}          # at or below 2^-24 relative: left to the gates
COST_Q = {"hh": 0, "hm": 1, "mh": 2, "mm": 3, "hl": 0, "lh": 2, "lm": 3}
MATS = ("cost", "gl", "gr")

Drop = collections.namedtuple("Drop", "mat prod q cb m", defaults=(None, None, None))


def bwd_nt(D):
    """The backward's band-tile count (decnet_mfma_backward)."""
    need = 1 if D <= 1 else (D - 1 + 15) // 16 + 1
    return next((nt for nt in (3, 6, 11, 15, 18) if need <= nt), None)


def rowb_of(C, W, D):
    """(NT, CB) of the spamat_bwd_rowb instantiation a row with every pixel active takes, or None.  launch_both gives
    spamat_bwd_rowb the rows that the sparse-row launches before it leave: those have more than 256 active pixels, at
    C <= 8 (where the 640-slot mid launch runs too) more than 640, hence W > 256 / W > 640 here.  The library reports no
    route, so nothing can assert which kernel ran: the FLAT route names are labels read off the dispatch, and a case
    whose label went stale would still be checked bit for bit, on whatever route it then takes."""
    nt = bwd_nt(D)
    if nt is None or W < 16 * nt or W <= 256 or W > 2048 or (C <= 8 and W <= 640):
        return None
    if C <= 8:
        return (nt, 1) if nt <= 15 else None
    if C <= 24:
        return (nt, 2 if C <= 16 else 3) if nt <= 11 else None
    return None


ROWB = tuple((nt, 1) for nt in (3, 6, 11, 15)) + tuple((nt, cb) for cb in (2, 3) for nt in (3, 6, 11))


def ring_of(nt):
    return 8 if nt <= 8 else 16


# ------------------------------------------------------------------------------------------------------------------
# the truncating split and its classes
def _trunc16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(x):
    """rb_split3 (fp32 in, three fp32 tensors out); l is packed like the others: its upper 16 bits."""
    assert x.dtype == torch.float32
    h = _trunc16(x)
    r1 = x - h
    m = _trunc16(r1)
    return h, m, _trunc16(r1 - m)


def is_k1(x):
    _, m, l = split3(x)
    return (m == 0) & (l == 0) & (x != 0)


def is_k2(x):
    _, m, l = split3(x)
    return (m != 0) & (l == 0)


def is_k3(x):
    h, m, l = (t.double() for t in split3(x))
    return (h + m + l == x.double()) & (m != 0) & (l != 0)


PRED = {"K1": is_k1, "K2": is_k2, "K3": is_k3}
PAIRINGS = (("K3", "K1"), ("K1", "K3"), ("K2", "K2"))               # (weight class, view class)
PINS = {("K3", "K1"): ("hh", "mh", "lh"), ("K1", "K3"): ("hh", "hm", "hl"), ("K2", "K2"): ("hh", "hm", "mh", "mm")}


def _sign(n, g):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


def _raw_view(cls, n, g):
    if cls == "K1":
        return (_sign(n, g) * torch.exp2(torch.randint(-3, 4, (n,), generator=g).double())).float()
    if cls == "K2":
        k = torch.randint(1, 4, (n,), generator=g).double()
        return (_sign(n, g) * torch.exp2(torch.randint(-3, 4, (n,), generator=g).double()) * (1 + k * 2.0 ** -10)).float()
    sig = torch.randint(2 ** 23, 2 ** 24, (n,), generator=g).double() * 2.0 ** -23
    return (_sign(n, g) * sig * torch.exp2(torch.randint(-6, 3, (n,), generator=g).double())).float()


def _raw_w(cls, n, g):
    """Weights are d - out with out a multiple of 2^-14: multiples of 2^-14 below 32."""
    if cls == "K1":
        return _sign(n, g) * torch.exp2(torch.randint(-14, 5, (n,), generator=g).double())
    if cls == "K2":
        k = torch.randint(1, 4, (n,), generator=g).double()
        return _sign(n, g) * torch.exp2(torch.randint(-4, 5, (n,), generator=g).double()) * (1 + k * 2.0 ** -10)
    return _sign(n, g) * torch.randint(2 ** 16, 2 ** 19, (n,), generator=g).double() * 2.0 ** -14


def draw_view(cls, shape, g):
    """Nonzero values of a class (rejection sampling; the predicate is asserted on what is returned)."""
    n = math.prod(shape)
    out = _raw_view(cls, n, g)
    bad = ~PRED[cls](out)
    while bool(bad.any()):
        out[bad] = _raw_view(cls, int(bad.sum()), g)
        bad = ~PRED[cls](out)
    return out.view(shape)


def draw_out(cls, d, g):
    """Per pixel an `out` (a multiple of 2^-14 in [0, 256)) such that w = d - out is of class cls.  d: integer tensor."""
    dd = d.reshape(-1).double()
    w = torch.zeros_like(dd)
    bad = torch.ones_like(dd, dtype=torch.bool)
    while bool(bad.any()):
        w[bad] = _raw_w(cls, int(bad.sum()), g)
        o = dd - w
        bad = ~((o >= 0) & (o < 256) & PRED[cls](w.float()) & (o * 2 ** 14 == (o * 2 ** 14).round()))
    out = (dd - w).float()
    assert bool((out.double() == dd - w).all())
    return out.view(d.shape)


# ------------------------------------------------------------------------------------------------------------------
# the host model
def _applies(drop, mat, C, xl, xr):
    """-> [C, 1, n] bool: the elements (channel, pixel pair) whose product `drop.prod` of matrix `mat` is removed."""
    n = xl.numel()
    pix = torch.ones(n, dtype=torch.bool)
    if drop.m is not None:
        pix &= ((xl >> 4) - (xr >> 4)) == drop.m
    if drop.q is not None:
        if mat == "gl":
            pix &= ((xr & 15) >> 2) == drop.q
        elif mat == "gr":
            pix &= (((xl & 15) >> 3) == (drop.q & 1)) & ((drop.q >> 1) == (0 if drop.prod[0] == "h" else 1))
        else:
            pix &= COST_Q[drop.prod] == drop.q
    ch = torch.ones(C, dtype=torch.bool)
    if drop.cb is not None:
        ch = torch.arange(C) // 8 == drop.cb
    return ch.view(C, 1, 1) & pix.view(1, 1, n)


def groups(mat, prod):
    """The K groups q in which product `prod` of matrix `mat` lives."""
    if mat == "cost":
        return (COST_Q[prod],)
    if mat == "gl":
        return (0, 1, 2, 3)
    return (0, 1) if prod[0] == "h" else (2, 3)


def _terms(x):
    return {k: t.double() for k, t in zip("hml", split3(x))}


def _kept(a, b):
    """sum over KEPT of a[p0] b[p1] (float64)."""
    return a["h"] * (b["h"] + b["m"] + b["l"]) + (a["m"] + a["l"]) * (b["h"] + b["m"])


def emulate_many(case, drops, cost_drop=None):
    """emulate(case, drop) for every drop of `drops` (Drops of gl / gr, or None) from one pass over the disparities: the
    costs and weights are formed once (without `cost_drop`, a Drop of the cost tile, if given) and each drop only
    subtracts its product where it applies.  -> [(grad_ref, grad_tar)] float64."""
    L, Rt, D = case["L"], case["R"], case["D"]
    B, C, H, W = L.shape
    for dr in list(drops) + [cost_drop]:
        assert dr is None or (dr.mat in MATS and dr.prod in KEPT)
    assert all(dr is None or dr.mat != "cost" for dr in drops) and (cost_drop is None or cost_drop.mat == "cost")
    on_l, on_r = R.mask_on(case["rm"]), R.mask_on(case["tm"])
    gsv = torch.where(on_l, case["g"] / case["S"], torch.zeros(()))               # fp32 division, as the kernel's
    nm = -case["max_cost"] * torch.tensor(LOG2E)                                   # fp32
    Lt, Rtt, Gt = _terms(L), _terms(Rt), _terms(L * gsv[:, None])
    x = torch.arange(W)
    gl = torch.zeros(B, C, H, W, dtype=F64)
    gr = torch.zeros(B, C, H, W, dtype=F64)
    corr = [None if dr is None else torch.zeros(B, C, H, W, dtype=F64) for dr in drops]
    for d in range(min(D, W)):
        xl, xr = x[d:], x[:W - d]
        sl = {k: v[..., d:] for k, v in Lt.items()}
        sg = {k: v[..., d:] for k, v in Gt.items()}
        sr = {k: v[..., :W - d] for k, v in Rtt.items()}
        cost = _kept(sr, sl)
        if cost_drop is not None:
            cost = cost - sr[cost_drop.prod[0]] * sl[cost_drop.prod[1]] * _applies(cost_drop, "cost", C, xl, xr).double()
        cost = cost.sum(1)                                                         # [B,H,n]
        arg = (cost.float().double() * LOG2E + nm[..., d:].double()).float()       # the fma: one rounding
        e = torch.exp2(arg.double()).float()
        e = torch.where((e >= 2.0 ** -126) & on_l[..., d:] & on_r[..., :W - d], e, torch.zeros(()))
        j, i = xl & 15, xr & 15
        dm0 = (j - 4 * (i >> 2)).float() - case["out"][..., d:]                    # fp32, the kernel's order
        dm = dm0 + (16 * ((xl >> 4) - (xr >> 4))).float()
        w = e * (dm - (i & 3).float())
        if not bool(w.any()):
            continue
        wt = {k: t.unsqueeze(1) for k, t in _terms(w).items()}                     # [B,1,H,n]
        gl[..., d:] += _kept(wt, sr)
        gr[..., :W - d] += _kept(wt, sg)
        for dr, c in zip(drops, corr):
            if dr is None or (dr.m is not None and abs(d - 16 * dr.m) > 15):      # (band tile m holds d in 16 m +- 15)
                continue
            mask = _applies(dr, dr.mat, C, xl, xr)
            if not bool(mask.any()):
                continue
            if dr.mat == "gl":
                c[..., d:] += wt[dr.prod[0]] * sr[dr.prod[1]] * mask.double()
            else:
                c[..., :W - d] += wt[dr.prod[0]] * sg[dr.prod[1]] * mask.double()
    sl_, sr_ = gsv.double()[:, None], on_r.double()[:, None]
    out = []
    for dr, c in zip(drops, corr):
        out.append(((gl - c if dr is not None and dr.mat == "gl" else gl) * sl_,
                    (gr - c if dr is not None and dr.mat == "gr" else gr) * sr_))
    return out


def emulate(case, drop=None):
    """The arithmetic of spamat_bwd_rowb with the kept term products summed in float64 -> (grad_ref, grad_tar) float64.
    case: dict of float32 tensors L, R [B,C,H,W], rm, tm, out, S, max_cost, g [B,H,W] and D.  drop: a Drop, the product
    removed everywhere or only in one K group q, one channel block cb (8 channels), one band tile m.  Only for the host
    proofs and the ablation table, never a GPU expectation."""
    if drop is not None and drop.mat == "cost":
        return emulate_many(case, [None], drop)[0]
    return emulate_many(case, [drop])[0]


def reference(case):
    """tests/_spamat_ref.backward in float64 on the imposed out / S / max_cost -> dict of gradients."""
    a = (case["L"], case["R"], case["rm"], case["tm"], case["out"], case["S"], case["max_cost"], case["g"], case["D"])
    if "mu" in case:
        return dict(zip(("gl", "gr", "gd"), R.backward(*a, disparity=case["mu"])))
    return dict(zip(("gl", "gr"), R.backward(*a)))


# e^-256 = 6.6e-112: what a dead candidate of the selector cases (cost -255 against max_cost 1) keeps in the float64
# reference and the chip flushes to 0; against products below 2^30 the reference may differ from an fp32 number by this
TAIL = 2.0 ** -300


def expect32(ref64, tail=0.0):
    """The fp32 expectation of a float64 reference that must be an fp32 number (up to `tail`, absolute).  + 0.0: a sum of
    zeros is +0 in float64 whatever their signs; the comparison canonicalises the chip's zeros the same way."""
    want = (ref64 + 0.0).float()
    assert bool(torch.isfinite(want).all())
    assert bool(((want.double() - ref64).abs() <= tail).all()), "the float64 reference is not representable in float32"
    return want + 0.0


def canon(t):
    """-0 -> +0 (a gradient that is 0 x g/S carries the sign of g on the chip)."""
    return t + 0.0


# ------------------------------------------------------------------------------------------------------------------
# family 1: flat dense.  (B, C, H, W, D, masks, var, route)
FLAT = [
    # the ten rowb instantiations; W just below / at / above 16 k, D at the NT edges, C no multiple of 8
    (1, 8, 2, 700, 16, "dense", 0, "rowb"), (1, 8, 2, 641, 33, "dense", 0, "rowb"),            # NT 3 CB 1
    (1, 8, 2, 701, 34, "dense", 0, "rowb"), (1, 5, 2, 700, 81, "dense", 0, "rowb"),            # NT 6 CB 1
    (1, 8, 2, 1024, 82, "dense", 0, "rowb"), (1, 5, 2, 641, 161, "dense", 0, "rowb"),          # NT 11 CB 1
    (1, 8, 2, 700, 162, "dense", 0, "rowb"), (1, 8, 2, 1025, 225, "dense", 0, "rowb"),         # NT 15 CB 1
    (1, 16, 2, 257, 33, "dense", 0, "rowb"), (1, 13, 2, 320, 16, "dense", 0, "rowb"),          # NT 3 CB 2
    (1, 16, 2, 300, 81, "dense", 0, "rowb"), (1, 13, 2, 257, 34, "dense", 0, "rowb"),          # NT 6 CB 2
    (1, 16, 2, 320, 161, "dense", 0, "rowb"), (1, 13, 2, 300, 82, "dense", 0, "rowb"),         # NT 11 CB 2
    (1, 24, 2, 300, 33, "dense", 0, "rowb"), (1, 20, 2, 257, 16, "dense", 0, "rowb"),          # NT 3 CB 3
    (1, 24, 2, 257, 81, "dense", 0, "rowb"), (1, 20, 2, 320, 34, "dense", 0, "rowb"),          # NT 6 CB 3
    (1, 24, 2, 320, 161, "dense", 0, "rowb"), (1, 20, 2, 300, 82, "dense", 0, "rowb"),         # NT 11 CB 3
    (2, 24, 2, 1025, 161, "dense", 0, "rowb"),                                                   # B 2, H 2: the largest plane
    # the other routes on the same data (fp32 fma chains)
    (1, 8, 4, 1024, 100, ("count", [(256, 256), (257, 257), (640, 640), (641, 641)]), 0, "sparse"),
    (1, 25, 2, 300, 40, "dense", 0, "band"), (1, 72, 2, 300, 40, "dense", 0, "band"),
    (1, 8, 2, 700, 226, "dense", 0, "band"), (1, 16, 2, 320, 162, "dense", 0, "band"),
    (1, 73, 2, 300, 40, "dense", 0, "rowtile"),
    (1, 8, 2, 400, 274, "dense", 0, "wide"),
    # SpaVar: integer disparity and variance, all three gradients
    (1, 8, 2, 700, 40, "dense", 1, "band"), (1, 24, 2, 300, 33, "dense", 1, "band"),
    (1, 8, 4, 1024, 40, ("count", [(256, 256), (257, 257), (640, 640), (641, 641)]), 1, "sparse"),
]
FLAT_IDS = ["%d-%s-B%dC%dH%dW%dD%d%s" % (i, c[7], *c[:5], "var" if c[6] else "") for i, c in enumerate(FLAT)]
FLAT_UNIT = 1.0 / 16


def flat_bound(D, var):
    """The largest |partial sum| of either gradient in units of FLAT_UNIT, any order: features <= 2, g/S <= 2 (a multiple
    of 1/4), |w| < D a multiple of 1/4 (SpaMat) or <= D^2 + 2 D an integer (SpaVar), at most D candidates."""
    wmax = (D * D + 2 * D) if var else D
    return int(2 * 2 * wmax * D / FLAT_UNIT)


def flat_case(row):
    B, C, H, W, D, mspec, var, _ = row
    from test_spamat_edges_gpu import make_masks
    g = gen("spamat-flat", row)
    lo = C // 2                                                       # left view: channels [0, lo), right view: [lo, C)
    L, Rt = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    L[:, :lo] = ints((B, lo, H, W), g)
    Rt[:, lo:] = ints((B, C - lo, H, W), g)
    rm, tm = make_masks(mspec, B, H, W, g)
    pl = (B, H, W)
    case = dict(L=L, R=Rt, rm=rm, tm=tm, D=D, max_cost=torch.zeros(pl),
                S=torch.randint(1, 3, pl, generator=g).float(),
                g=(torch.randint(0, 2, pl, generator=g).float() * 2 - 1) * torch.exp2(torch.randint(-1, 2, pl, generator=g).float()))
    if var:
        case["mu"] = torch.randint(0, D, pl, generator=g).float()
        case["out"] = torch.randint(0, 2 * D + 1, pl, generator=g).float()         # the imposed variance
    else:
        case["out"] = torch.randint(0, 4 * D, pl, generator=g).float() / 4
    return case


# ------------------------------------------------------------------------------------------------------------------
# family 2: selectors.  (C, H, W, D, selector channel): one per rowb instantiation, rows enough for the coverage table
SEL = [
    (8, 4, 700, 33, 7), (8, 6, 701, 81, 0), (5, 8, 700, 161, 2), (8, 8, 1025, 225, 5),
    (16, 4, 320, 33, 15), (13, 8, 300, 81, 8), (16, 12, 320, 161, 3),
    (24, 4, 300, 33, 16), (20, 8, 257, 81, 19), (24, 12, 320, 161, 7),
]
SEL_IDS = ["C%dH%dW%dD%d" % c[:4] for c in SEL]
RUNS = ("left", "right")


def _phase(row, D):
    return (5 + 37 * row) % D


def _right_offset(k, t, xs, W, D):
    """The disparity at which the k-th selected right pixel xs gets its one left pixel with g != 0, variant t.  D <= 33: d
    walks over [0, D) with a stride coprime to D, so every d occurs; wider bands have fewer selected pixels than
    disparities: the band tile m walks over [0, NT) and the left pixel's column j over [0, 16), moved inside [0, D) and
    the row where needed."""
    if D <= 33:
        stride = [a for a in range(1, D) if math.gcd(a, D) == 1][t % 20]
        return (stride * k + t // 20) % D
    nt = bwd_nt(D)
    m, j = (k + t) % nt, (5 * k + 3 * t) % 16
    while True:
        d = 16 * m + j - (xs & 15)
        if d < 0:
            j = (xs & 15) + k % (16 - (xs & 15))
        elif d >= D or xs + d >= W:
            if j > 0 and 16 * m - (xs & 15) < D and xs + 16 * m - (xs & 15) < W:
                j = max(0, min(j - 1, D - 1 - 16 * m + (xs & 15), W - 1 - xs - 16 * m + (xs & 15)))
            else:
                m, j = m - 1, 15 - k % 4
        else:
            return d


def _roles(xl, xr, nt):
    return {"q": set(((xr & 15) >> 2).tolist()), "r": set((xr & 3).tolist()), "j": set((xl & 15).tolist()),
            "i": set((xr & 15).tolist()), "m": set(((xl >> 4) - (xr >> 4)).tolist()),
            "wave": set(((xr >> 4) & 3).tolist()), "slot": set(((xr >> 4) & (ring_of(nt) - 1)).tolist()),
            "left wave": set(((xl >> 4) & 3).tolist()), "d": set((xl - xr).tolist())}


def right_pixels(row):
    """[(image row, selected right pixel, disparity of its left pixel)] of the right run: the first variant of
    _right_offset under which every role of required_roles (and at D <= 33 every disparity) receives a product."""
    C, H, W, D, sel = row
    need = {k: v for k, v in required_roles(row).items() if k not in ("cb", "ch")}
    if D <= 33:
        need["d"] = set(range(D))
    for t in range(400):
        pts, k = [], 0
        for y in range(H):
            for xs in range(_phase(y, D), W, D):
                dd = _right_offset(k, t, xs, W, D)
                k += 1
                if xs + dd < W:
                    pts.append((y, xs, dd))
        xr = torch.tensor([p[1] for p in pts])
        got = _roles(xr + torch.tensor([p[2] for p in pts]), xr, bwd_nt(D))
        if all(got[k] >= v for k, v in need.items()):
            return pts
    raise AssertionError("no variant of the right run covers every role of %s" % (row,))


def selector_case(row, pairing, run):
    """-> case dict (with "live": the pixels whose gradient is one nonzero product, "d": their disparity).
    left run: grad_ref[c][x] = g/S w R[c][x - d(x)] at every left pixel right of its row's first selected right pixel;
    right run: grad_tar[c][x'] = g/S w L[c][x] at every selected right pixel whose chosen left pixel x is inside the row
    (and grad_ref's selector channel g/S w there).  Everything else is 0."""
    C, H, W, D, sel = row
    wcls, vcls = pairing
    g = gen("spamat-sel", row, pairing, run)
    B = 1
    data = [c for c in range(C) if c != sel]
    L, Rt = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    L[:, sel] = 1.0
    Rt[:, sel] = -255.0
    x = torch.arange(W)
    d = torch.zeros(B, H, W, dtype=torch.long)
    live = torch.zeros(B, H, W, dtype=torch.bool)
    gmask = torch.zeros(B, H, W, dtype=torch.bool)
    for y in range(H):
        ph = _phase(y, D)
        Rt[0, sel, y, ph::D] = 1.0
        d[0, y] = torch.where(x >= ph, (x - ph) % D, torch.zeros(()).long())
        live[0, y] = x >= ph
    view = draw_view(vcls, (B, len(data), H, W), g)
    (Rt if run == "left" else L)[:, data] = view
    pl = (B, H, W)
    out = torch.where(live, draw_out(wcls, d, g), torch.tensor(0.25))
    gg = (torch.randint(0, 2, pl, generator=g).float() * 2 - 1) * torch.exp2(torch.randint(-2, 3, pl, generator=g).float())
    if run == "right":
        for y, xs, dd in right_pixels(row):                           # one left pixel per selected right pixel
            gmask[0, y, xs + dd] = True
        gg = torch.where(gmask, gg, torch.zeros(()))
        live = gmask
    return dict(L=L, R=Rt, rm=torch.ones(pl), tm=torch.ones(pl), D=D, max_cost=torch.ones(pl), out=out,
                S=torch.randint(1, 3, pl, generator=g).float(), g=gg, live=live, d=d, sel=sel, run=run)


def exact_keys(run):
    """The gradients of a selector run whose every element is one product (the left run's grad_tar is a sum of D)."""
    return ("gl",) if run == "left" else ("gl", "gr")


def selector_roles(row, case):
    """The roles of the kernel that receive a nonzero product of the pinned gradient in this case -> dict of sets.  The
    channel roles cb, ch are those of the channels c whose product g/S w view[c] is nonzero at some live pixel."""
    C, H, W, D, sel = row
    nt = bwd_nt(D)
    _, y, xl = case["live"].nonzero(as_tuple=True)
    dd = case["d"][0, y, xl]
    xr = xl - dd
    w = dd.double() - case["out"][0, y, xl].double()
    view = case["R"][0][:, y, xr] if case["run"] == "left" else case["L"][0][:, y, xl]        # [C, n]
    nz = (view != 0) & ((case["g"][0, y, xl] != 0) & (w != 0))[None]
    chans = nz.any(1).nonzero()[:, 0].tolist()
    return dict(_roles(xl, xr, nt), cb=set(c // 8 for c in chans), ch=set(c % 8 for c in chans))


def required_roles(row):
    C, H, W, D, sel = row
    nt, cb = rowb_of(C, W, D)
    return {"q": set(range(4)), "r": set(range(4)), "j": set(range(16)), "i": set(range(16)), "m": set(range(nt)),
            "wave": set(range(4)), "slot": set(range(ring_of(nt))), "left wave": set(range(4)), "cb": set(range(cb)),
            "ch": set(range(min(C, 8)))}


# ------------------------------------------------------------------------------------------------------------------
# family 3: cost terms.  The selector of family 2 plus ONE data channel per image row (it walks over the channel blocks
# with the row) that carries a class pair on (R, L): the live cost is 1 + R L, exact in fp32 but no power of two, and
# max_cost is imposed to it.  First letter of a cost product: the term of R, second: the term of L (KEPT).
COST = SEL
COST_IDS = SEL_IDS
COST_PAIRINGS = PAIRINGS                                              # (class of R, class of L)
COST_POOL = {"K1": 64, "K2": 128, "K3": 512}
COST_RES = 2.0 ** -26          # |fma(cost, log2e, -max_cost log2e)| of the live candidates: 2^arg rounds to 1.0f
# The accuracy of v_exp_f32 near 0, relative: twice the worst deviation of grad_ref's selector channel from the float64
# reference over all COST cases on the MI355X.  Measured: 0 (under COST_RES the chip's exp2 returns exactly 1.0f;
# docs/rounds/spamat_exact.md).
EXP_ACC = 2 * 0.0


def _cost_good(r, lp):
    """r [n], lp [P] float32 -> [n, P] bool: the pairs whose cost 1 + r l (a) has no term product outside KEPT, (b) is an
    fp32 number, as is every subset sum of the 1 and its kept products (no order of accumulation rounds), (c) lies in
    [1/4, 2.75] with |r l| >= 1/4, and (d) meets COST_RES, so that the forward's sum of similarities is fl(1 + 1e-6f)."""
    rt = {k: t.double()[:, None] for k, t in zip("hml", split3(r))}
    lt = {k: t.double()[None, :] for k, t in zip("hml", split3(lp))}
    rl = r.double()[:, None] * lp.double()[None, :]
    ok = (rt["m"] * lt["l"] == 0) & (rt["l"] * lt["l"] == 0)
    c = 1.0 + rl
    ok &= (c >= 0.25) & (c <= 2.75) & (rl.abs() >= 0.25)
    items = [torch.ones_like(rl)] + [rt[p[0]] * lt[p[1]] for p in KEPT]
    for n in range(1, 9):
        for sub in itertools.combinations(items, n):
            t = sum(sub)
            ok &= t.float().double() == t
    c32 = c.float()
    nm = -c32 * torch.tensor(LOG2E)                                                # fp32, as the kernels'
    arg = c32.double() * LOG2E + nm.double()                                       # the fma before its rounding: exact here
    return ok & (arg.abs() <= COST_RES)


def cost_channel(row, y):
    """The data channel of image row y: block y % CB, never the selector."""
    C, H, W, D, sel = row
    cb = rowb_of(C, W, D)[1]
    cand = [c for c in range(C) if c // 8 == y % cb and c != sel]
    return cand[(y // cb) % len(cand)]


def cost_case(row, pairing):
    """-> case dict of the left run of selector_case (g = +-2^k everywhere, w = d - out three-term) with the data channel
    of cost_channel: R from class pairing[0] at every right pixel, L from pairing[1] chosen per left pixel among a pool so
    that _cost_good holds against its live right pixel.  "dc": the data channel per image row."""
    C, H, W, D, sel = row
    rcls, lcls = pairing
    g = gen("spamat-cost", row, pairing)
    B = 1
    L, Rt = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    L[:, sel] = 1.0
    Rt[:, sel] = -255.0
    x = torch.arange(W)
    d = torch.zeros(B, H, W, dtype=torch.long)
    live = torch.zeros(B, H, W, dtype=torch.bool)
    mc = torch.ones(B, H, W)
    pool = draw_view(lcls, (COST_POOL[lcls],), g)
    dcs = []
    for y in range(H):
        ph, dc = _phase(y, D), cost_channel(row, y)
        dcs.append(dc)
        Rt[0, sel, y, ph::D] = 1.0
        d[0, y] = torch.where(x >= ph, (x - ph) % D, torch.zeros(()).long())
        live[0, y] = x >= ph
        Rt[0, dc, y] = draw_view(rcls, (W,), g)                       # (the dead candidates see data too)
        xs = torch.arange(ph, W, D)
        r = draw_view(rcls, (xs.numel(),), g)
        good = _cost_good(r, pool)
        bad = ~good.any(1)
        while bool(bad.any()):
            r[bad] = draw_view(rcls, (int(bad.sum()),), g)
            good[bad] = _cost_good(r[bad], pool)
            bad = ~good.any(1)
        Rt[0, dc, y, xs] = r
        k = (x[ph:] - ph) // D                                        # the selected pixel of each live left pixel
        pick = torch.multinomial(good[k].float(), 1, generator=g)[:, 0]
        L[0, dc, y, ph:] = pool[pick]
        mc[0, y, ph:] = (1.0 + r[k].double() * pool[pick].double()).float()
    pl = (B, H, W)
    out = torch.where(live, draw_out("K3", d, g), torch.tensor(0.25))
    gg = (torch.randint(0, 2, pl, generator=g).float() * 2 - 1) * torch.exp2(torch.randint(-2, 3, pl, generator=g).float())
    return dict(L=L, R=Rt, rm=torch.ones(pl), tm=torch.ones(pl), D=D, max_cost=mc, out=out,
                S=torch.randint(1, 3, pl, generator=g).float(), g=gg, live=live, d=d, sel=sel, dc=dcs, run="left")


def cost_bound(case):
    """Per pixel, relative to the float64 reference: the fma residual (<= |cost| 2^-24: the rounding of -max_cost log2e,
    times ln 2), the rounding of e (d - out), and the accuracy of v_exp_f32 near 0."""
    return (case["max_cost"].double().abs() + 1.0) * 2.0 ** -24 + EXP_ACC


def cost_model(case, drop=None):
    """grad_ref's selector channel [B,H,W] (float64) by the arithmetic of spamat_bwd_rowb from the LIVE candidate of every
    left pixel alone (the dead ones sit 253 or more below max_cost with or without a cost product: their e is 0 in fp32);
    drop: a Drop of the cost tile, everywhere or in one K group q / one channel block cb.  test_spamat_exact_cpu.py ties
    it to emulate()."""
    L, Rt, sel = case["L"], case["R"], case["sel"]
    B, C, H, W = L.shape
    assert drop is None or (drop.mat == "cost" and drop.prod in KEPT and drop.m is None)
    xr = (torch.arange(W) - case["d"]).clamp_min(0)                               # [B,H,W]
    Rl = torch.gather(Rt, 3, xr[:, None].expand(B, C, H, W))                      # R[c][x - d(x)]
    rt, lt = _terms(Rl), _terms(L)
    cost = _kept(rt, lt)                                                          # [B,C,H,W] per channel
    if drop is not None and (drop.q is None or drop.q == COST_Q[drop.prod]):
        ch = torch.ones(C, dtype=torch.bool) if drop.cb is None else torch.arange(C) // 8 == drop.cb
        cost = cost - rt[drop.prod[0]] * lt[drop.prod[1]] * ch.view(1, C, 1, 1).double()
    cost = cost.sum(1)
    nm = -case["max_cost"] * torch.tensor(LOG2E)
    arg = (cost.float().double() * LOG2E + nm.double()).float()
    e = torch.exp2(arg.double()).float()
    w = e * (case["d"].float() - case["out"])                                     # fp32: one rounding
    gsv = case["g"] / case["S"]
    return torch.where(case["live"], w.double() * gsv.double(), torch.zeros((), dtype=F64))


def cost_dev(got, ref, case):
    """max over the live pixels of |got - ref| / (|ref| cost_bound): <= 1 passes.  got, ref: the selector channel."""
    lv = case["live"]
    assert bool((ref[lv] != 0).all())
    return float(((got.double() - ref)[lv].abs() / (ref[lv].abs() * cost_bound(case)[lv])).max())


# ------------------------------------------------------------------------------------------------------------------
# the ablation table of DESIGN.md section 2
TABLE = [(8, 700, 40, "relu"), (8, 700, 225, "relu"), (24, 300, 81, "relu"), (8, 700, 40, "signed")]
TABLE_DROPS = (Drop("gl", "lh"), Drop("gl", "hl"), Drop("gl", "mm"), Drop("cost", "hl"))


def table_case(C, W, D, feats):
    from test_spamat_edges_gpu import make_feats
    g = gen("spamat-table", C, W, D, feats)
    L, Rt = make_feats(feats, 1, C, 1, W, D, g)
    one = torch.ones(1, 1, W)
    f = R.forward(L, Rt, one, one, D)
    case = dict(L=L, R=Rt, rm=one, tm=one, D=D, g=torch.randn(1, 1, W, generator=g),
                **{k: f[s].float() for k, s in (("out", "out"), ("S", "S"), ("max_cost", "max_cost"))})
    ref = reference(case)
    sc = max(1.0, max(float(t.abs().max()) for t in ref.values()))
    gate = 64 * 2.0 ** -24 * max(1.0, float(f["k_max"].max())) * sc
    if feats == "relu":
        gate = min(gate, 5e-5 * sc)
    return case, ref, gate


def table_row(C, W, D, feats):
    """-> gate, error of the whole model, errors of the model without each of TABLE_DROPS (max over both gradients)."""
    case, ref, gate = table_case(C, W, D, feats)

    def err(drop):
        gl, gr = emulate(case, drop)
        return max(float((gl - ref["gl"]).abs().max()), float((gr - ref["gr"]).abs().max()))
    return gate, err(None), [err(dr) for dr in TABLE_DROPS]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--table"], "usage: _spamat_exact.py --table"
    print("| case (C, W, D, feats) | gate | all seven | without `w_l·R_h` | without `w_h·R_l` | without `w_m·R_m` | "
          "without cost `R_h·L_l` |")
    print("|---|---|---|---|---|---|---|")
    for row in TABLE:
        gate, full, errs = table_row(*row)
        print("| %d, %d, %d, %s | %.1e | %.2g | %s |" % (*row, gate, full / gate,
                                                         " | ".join("%.2g" % (e / gate) for e in errs)))
