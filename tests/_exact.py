"""Exact data for the forward convolution kernels: value classes whose float64 result is representable in float32 with
every partial sum exact in any order, a host model of the bf16x3 arithmetic, and the case tables and data of
tests/test_conv_exact_gpu.py (bit for bit against float64 on the MI355X) and tests/test_exact_cpu.py (which proves on the
host that those cases have teeth).

Terms.  The matrix-core kernels split every fp32 operand into three bf16 terms x = h + m + l (round to nearest even,
csrc/conv2d_mfma.hip: split3) and keep the six products SIX of data term x weight term; the first letter names the
data's term, the second the weight's.
  T1  one term:    0 or +-2^e, e in -3..3 (m = l = 0);
  T2  two terms:   +-2^e (1 + k 2^-10), k in 1..3 (m != 0, l = 0): the product of two T2 values and every subset sum of
                   its four term products is exact in fp32;
  T3  three terms: a random 24-bit significand times +-2^e, e in -20..8, with h + m + l = x, m != 0, l != 0 and each of
                   h + m, h + l, m + l representable in fp32 (96 % of the draws).
Selector weights (one nonzero weight per output channel) make every output one product data x weight x +-2^e, so a
kernel that drops, doubles or misplaces one term product of one channel / tap returns a different bit pattern."""
import math

import torch

import _trunk_ref as R

D = torch.float64
SIX = ("hh", "hm", "mh", "mm", "hl", "lh")
PAIRINGS = (("T3", "T1"), ("T1", "T3"), ("T2", "T2"))               # (data class, weight class)
PINS = {("T3", "T1"): ("hh", "mh", "lh"), ("T1", "T3"): ("hh", "hm", "hl"), ("T2", "T2"): ("hh", "mm")}
MAX_ROT = 12


def gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------
def split3(x):
    """The kernels' split (fp32 in, three fp32 tensors out); torch's bfloat16 conversion rounds to nearest even."""
    assert x.dtype == torch.float32
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    return h, m, l


def _f32(v):
    return v.float().double() == v


def is_t1(x):
    _, m, l = split3(x)
    return (m == 0) & (l == 0)


def is_t2(x):
    _, m, l = split3(x)
    return (m != 0) & (l == 0)


def is_t3(x):
    h, m, l = (t.double() for t in split3(x))
    return (h + m + l == x.double()) & (m != 0) & (l != 0) & _f32(h + m) & _f32(h + l) & _f32(m + l)


def _sign(n, g):
    return torch.randint(0, 2, (n,), generator=g).float() * 2 - 1


def _raw_t1(n, g, zero=True):
    v = _sign(n, g) * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())
    return torch.where(torch.randint(0, 8, (n,), generator=g) > 0, v, torch.zeros(())) if zero else v


def _raw_t2(n, g):
    k = torch.randint(1, 4, (n,), generator=g).float()
    return _sign(n, g) * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float()) * (1 + k * 2.0 ** -10)


def _raw_t3(n, g):
    sig = torch.randint(2 ** 23, 2 ** 24, (n,), generator=g).double() * 2.0 ** -23          # [1, 2)
    return (_sign(n, g).double() * sig * torch.exp2(torch.randint(-20, 9, (n,), generator=g).double())).float()


def _draw(shape, g, raw, pred):
    """Rejection sampling; the predicate is asserted on what is returned."""
    n = math.prod(shape)
    out = raw(n, g)
    bad = ~pred(out)
    while bool(bad.any()):
        out[bad] = raw(int(bad.sum()), g)
        bad = ~pred(out)
    assert bool(pred(out).all())
    return out.view(shape)


def t1(shape, g, zero=True):
    return _draw(shape, g, lambda n, g_: _raw_t1(n, g_, zero), is_t1)


def t2(shape, g):
    return _draw(shape, g, _raw_t2, is_t2)


def t3(shape, g):
    return _draw(shape, g, _raw_t3, is_t3)


def draw(cls, shape, g, zero=True):
    return {"T1": lambda: t1(shape, g, zero), "T2": lambda: t2(shape, g), "T3": lambda: t3(shape, g)}[cls]()


def ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def bn_exact(c, g):
    """scale from {0.5, 1, 2}, integer shift in [-3, 3]."""
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)], ints((c,), g, -3, 3)


def pow2_scale(c, g):
    """+-2^e, e in -2..2, and a zero shift (the selector cases)."""
    return _sign(c, g) * torch.exp2(torch.randint(-2, 3, (c,), generator=g).float()), torch.zeros(c)


def emulate(x, w, keep=SIX, op=None):
    """The bf16x3 convolution op(x, w) (float64, bilinear; default: tests/_trunk_ref.conv) as the float64 sum of the
    kept term products.  Only for tests/test_exact_cpu.py, never a GPU expectation."""
    op = op or R.conv
    xt, wt = dict(zip("hml", split3(x))), dict(zip("hml", split3(w)))
    out = None
    for p in keep:
        y = op(xt[p[0]].double(), wt[p[1]].double())
        out = y if out is None else out + y
    return out


def exact_or_fail(ref64, unit=None):
    """The float32 expectation of a float64 reference that must be representable: a case can never pass because its own
    expectation was rounded.  unit (3a: 1, 1/8 or 1/16): the reference is a multiple of it below 2^24 units, the size
    below which every partial sum of such multiples is exact in fp32 in any order.  (+ 0.0: a float64 sum whose terms
    are all -0 is +0 on the chip, the convention of tests/test_conv2d_grad_gpu.py.)"""
    assert ref64.dtype == D
    assert bool((ref64.float().double() == ref64).all()), "the float64 reference is not representable in float32"
    if unit is not None:
        assert bool((ref64 / unit == (ref64 / unit).round()).all()) and float(ref64.abs().max()) < 2 ** 24 * unit
    else:
        assert float(ref64.abs().max()) < 2.0 ** 24
    return (ref64 + 0.0).float()


# ------------------------------------------------------------------------------------------------------------------
# 3a: dense small integers.  Inputs in [-2, 2], weights in {-1, 0, 1}, scale in {0.5, 1, 2}, integer shift / residual.
def tables():
    """The shapes of 3a: the edge tables of tests/test_trunk_edges_gpu.py and tests/test_stage0_edges_gpu.py themselves."""
    import test_stage0_edges_gpu as S
    import test_trunk_edges_gpu as T

    def rows(fn):
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize" and "," in m.args[0]]
        return list(mark.args[1])
    return {"small": [c for c in T.SMALL if c[6] == 0],              # the sigmoid epilogues are not exact
            "s3": [((H, W, ci, min(co, 8) if tr else co), tr) for tr in (0, 1) for H, W, ci, co in T.S3],
            "mfma": list(T.MFMA), "deconv": rows(T.test_mfma_deconv_edges), "tap": list(T.TAP),
            "conv": list(S.CONV), "wino": list(S.WINO), "pointwise": rows(S.test_pointwise_edges),
            "cout1": [c for c in S.COUT1 if c[5] is None]}           # saturation needs non-integer data


def dense2d(key, segs, cout, k, B, H, W, transposed=False):
    g = gen("dense2d", key)
    xs = [ints((B, c, H, W), g) for c in segs]
    cin = sum(segs)
    w = ints(((cin, cout) if transposed else (cout, cin)) + (k, k), g, -1, 1)
    return (xs, w) + bn_exact(cout, g)


def dense_tap(case):
    Ci, Co, (B, H, W), brs = case
    g = gen("tap", case)
    x = ints((B, Ci, H, W), g)
    ws = [ints((Co, Ci, k, k), g, -1, 1) for k, _ in brs]
    return (x, ws) + bn_exact(len(brs) * Co, g)


def dense3d(case):
    """(B, D, H, W, Ci, Co, relu, residual) -> x, w, scale, shift, residual or None (channels last)."""
    B, Dd, H, W, Ci, Co, _, res = case
    g = gen("dense3d", case)
    x, w = ints((B, Dd, H, W, Ci), g), ints((Co, Ci, 3, 3, 3), g, -1, 1)
    scale, shift = bn_exact(Co, g)
    return x, w, scale, shift, ints((B, Dd, H, W, Co), g, -3, 3) if res else None


def wino0_bound(Ci):
    """F(2,3)^3 on this data, in units of 1/8: |8U| <= 27, |V| <= 16, so |8M| <= Ci 27 16 and the output transform sums
    27 of them; with the epilogue (scale <= 2, shift, residual) still far below 2^24."""
    b = Ci * 27 * 16 * 27
    assert 2 * b + 8 * 6 < 2 ** 24
    return b


def dense_pointwise(row):
    B, Ci, Co, P, ldw, cl = row
    g = gen("pw", row)
    return ints((B, P, Ci) if cl else (B, Ci, P), g), ints(((Co - 1) * ldw + Ci,), g, -1, 1)


def dense_cout1(case):
    B, Dd, H, W, Ci, _ = case
    g = gen("cout1", case)
    scale = float([0.5, 1.0, 2.0][int(torch.randint(0, 3, (1,), generator=g))])
    return ints((B, Dd, H, W, Ci), g), ints((1, Ci, 3, 3, 3), g, -1, 1), scale, float(ints((1,), g, -3, 3))


GEMM0_NT = (1, 47, 96, 97)
GEMM0_CICO = ((216, 216), (216, 5), (20, 17), (4, 1))


def dense_gemm0(nt, Ci, Co):
    """decnet_conv3d_wino_gemm, variant 0: V [64][16 ceil(Ci/16)][nt] integers (zero past Ci) and a weight of multiples
    of 8, whose transform U = G w G^T (G: 0, 1, +-1/2) is integer with |U| <= 27."""
    g = gen("gemm0", nt, Ci, Co)
    V = ints((64, (Ci + 15) // 16 * 16, nt), g)
    V[:, Ci:] = 0
    return V, ints((Co, Ci, 3, 3, 3), g, -1, 1) * 8


# ------------------------------------------------------------------------------------------------------------------
# 3b: term selectors.  Output channel co of rotation r has its one nonzero weight at (ci, tap) = sel(co, r).
SEL_CONV = [  # (segments, Cout, k, dilation, (B, H, W))
    ((16,), 24, 3, 1, (1, 3, 5)), ((24,), 17, 3, 2, (2, 3, 5)), ((7,), 33, 3, 1, (1, 2, 15)),
    ((65, 7), 17, 3, 1, (1, 5, 9)), ((3, 1, 17, 40), 81, 3, 1, (1, 4, 7)), ((48,), 17, 1, 1, (1, 3, 20)),
    ((1,) * 6, 97, 3, 1, (1, 3, 4)),
]
SEL_DECONV = [(2, 2, 72, 24), (1, 5, 9, 30), (1, 1, 16, 9)]        # (H, W, Cin, Cout)
# Co = 18, not 17: twelve rotations of 17 channels select 204 of the 216 input channels, 18 select them all (one full
# tile of 16 output channels and a tail either way)
SEL_TAP = [(216, co, P) for co in (18, 224) for P in (1, 95, 96, 97)]   # (Ci, Co, P), nine taps, split = 1


def sel(co, r, cin, cout, kt):
    return (co + r * cout) % cin, (co + r) % kt


def rotations(cin, cout, kt):
    n = max(-(-cin // cout), -(-kt // cout))
    assert n <= MAX_ROT, (cin, cout, kt)
    return n


def selector_weight(vals, r, cin, kt):
    """[Cout, Cin, kt] with vals[co] at sel(co, r), zero elsewhere."""
    cout = vals.numel()
    w = torch.zeros(cout, cin, kt)
    for co in range(cout):
        ci, tap = sel(co, r, cin, cout, kt)
        w[co, ci, tap] = vals[co]
    return w


def selector_case(key, pairing, r, segs, cout, kt, shape_of):
    """Data of one rotation: xs (one tensor per segment, shape_of(c)), w [Cout, Cin, kt], scale, shift, relu."""
    g = gen("sel", key, pairing, r)
    xs = [draw(pairing[0], shape_of(c), g) for c in segs]
    w = selector_weight(draw(pairing[1], (cout,), g, zero=False), r, sum(segs), kt)
    return (xs, w) + pow2_scale(cout, g) + ((r + len(segs) + cout) % 2,)


def assert_coverage(ws, segs):
    """The coverage conditions on the weights [Cout, Cin, kt] of a case's rotations: one nonzero weight per output
    channel, every input channel and every tap selected, and with them the first and last channel of every segment and
    of every 16-channel chunk."""
    assert 1 <= len(ws) <= MAX_ROT
    cin, kt = ws[0].shape[1:]
    assert cin == sum(segs)
    for w in ws:
        assert bool(((w != 0).sum((1, 2)) == 1).all()), "one nonzero weight per output channel"
    used = torch.stack([w != 0 for w in ws]).any(0).any(0)           # [Cin, kt]
    chans, taps = used.any(1), used.any(0)
    assert bool(chans.all()), "input channels never selected: %s" % (~chans).nonzero().flatten().tolist()
    assert bool(taps.all()), "taps never selected: %s" % (~taps).nonzero().flatten().tolist()
    edges, c0 = set(), 0
    for c in segs:
        edges |= {c0, c0 + c - 1}
        c0 += c
    for c0 in range(0, cin, 16):
        edges |= {c0, min(c0 + 15, cin - 1)}
    assert all(bool(chans[e]) for e in edges)
