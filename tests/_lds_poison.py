"""LDS poison for the edge tests: a kernel that fills every CU's LDS with a chosen word runs immediately before the kernel
under test, and the result must not depend on the word.  LDS is not cleared between workgroups, so a kernel that reads
LDS it never wrote (an MFMA K tail, a halo, a pitch or bank padding it expects to hold zeros) sees what its predecessor
left; in the suite that predecessor is nearly always the same kernel at a similar case, which left zeros in the same
places.  The hooks come from tests/support/lds_poison.hip (decnet_amd.build.build_testhooks()), a library of its own.

`_placement._L()` hands out a `PoisonedLib` while a pattern is set (`with pattern(p):`), so every runner that goes through
`_L()` is poisonable as it stands; `sweep(run)` is the four poisoned runs `_placement._both` adds to its two."""
import contextlib
import ctypes
import os

import torch

# 0x7FC07FC0: a NaN as fp32 and as either half read as bf16.  0x3F803F80: about 1.002 as fp32, 1.0 / 1.0 as a bf16 pair;
# finite, so that a use of it shows as a changed value where the NaN would be swallowed (a select, a max, a mask).
PATTERNS = (0x7FC07FC0, 0x3F803F80)
# poison workgroups per CU: the smallest of 1, 2, 4, 8 at which a probe finds at least MIN_SHARE of all LDS words
# poisoned on the MI355X (docs/rounds/lds_poison.md has the measured shares)
ROUNDS = 1
MIN_SHARE = 0.90
LEAKY_WORDS = 1024

_P, _I, _U, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float
_hooks = None
_pattern = None                    # the word `_placement._L()` poisons with; None: the plain handle


def hooks():
    """The ctypes handle of libdecnet_testhooks.so.  A missing library is an error, never a skip."""
    global _hooks
    if _hooks is None:
        from decnet_amd import build
        path = build.TESTHOOKS_PATH
        assert os.path.exists(path), \
            "%s is missing: build it with decnet_amd.build.build_testhooks() (hipcc, gfx950)" % path
        h = ctypes.CDLL(path)
        h.decnet_test_lds_poison.argtypes = [_U, _I, _P]
        h.decnet_test_lds_probe.argtypes = [_U, _I, _P, _P]
        h.decnet_test_lds_leaky.argtypes = [_F, _P, _P]
        for name in ("decnet_test_lds_poison", "decnet_test_lds_probe", "decnet_test_lds_leaky"):
            getattr(h, name).restype = _I
        _hooks = h
    return _hooks


def _st():
    return torch.cuda.current_stream().cuda_stream


def poison(pat, rounds=None):
    """Fill LDS with `pat` on the current stream."""
    rc = hooks().decnet_test_lds_poison(pat, ROUNDS if rounds is None else rounds, _st())
    assert rc == 0, "decnet_test_lds_poison: %d" % rc


def probe(pat, rounds=None):
    """The share of LDS words that equal `pat`, over rounds x CU-count workgroups that each read all of their LDS."""
    rounds = ROUNDS if rounds is None else rounds
    n = rounds * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    counts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    words = hooks().decnet_test_lds_probe(pat, rounds, counts.data_ptr(), _st())
    assert words > 0, "decnet_test_lds_probe: %d" % words
    c = counts.cpu().long()
    assert int(c.min()) >= 0 and int(c.max()) <= words, "a probe workgroup did not report"
    return float(c.sum()) / (n * words)


def visible_share(pat, rounds=None):
    poison(pat, rounds)
    return probe(pat, rounds)


def leaky(zero=0.0):
    """The planted bug: 1 + zero * (LDS words the kernel never wrote) -> host tensor of LEAKY_WORDS floats."""
    out = torch.full((LEAKY_WORDS,), 7.0, dtype=torch.float32, device="cuda")
    rc = hooks().decnet_test_lds_leaky(zero, out.data_ptr(), _st())
    assert rc == 0, "decnet_test_lds_leaky: %d" % rc
    return out.cpu()


class PoisonedLib:
    """Proxy of a ctypes handle: every `decnet_*` entry that takes a stream is preceded by a poison launch on the current
    stream (the size queries and host-only helpers take none and launch nothing)."""

    def __init__(self, real, pat):
        self._real, self._pat = real, pat

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        args = getattr(fn, "argtypes", None)
        if not name.startswith("decnet_") or not args or args[-1] is not _P or \
                name.endswith(("_floats", "_bytes")):
            return fn
        pat = self._pat

        def call(*a):
            poison(pat)
            return fn(*a)
        return call


def current():
    return _pattern


@contextlib.contextmanager
def pattern(pat):
    """While active, `_placement._L()` returns a PoisonedLib of `pat`."""
    global _pattern
    old, _pattern = _pattern, pat
    try:
        yield
    finally:
        _pattern = old


@contextlib.contextmanager
def package(pat):
    """While active, the package's own handle (decnet_amd._lib.lib(), which ops / imageio / model call through) is a
    PoisonedLib of `pat`; the per-name lookups decnet_amd.ops keeps are set aside, as tests/spy_util.entry_spy does."""
    from decnet_amd import _lib, ops
    real = _lib.lib()
    saved = dict(ops._FN)
    ops._FN.clear()
    _lib._lib = PoisonedLib(real, pat)
    try:
        yield
    finally:
        _lib._lib = real
        ops._FN.clear()
        ops._FN.update(saved)


def wrap(real):
    return real if _pattern is None else PoisonedLib(real, _pattern)


def name(pat):
    return "LDS pattern 0x%08X" % pat


def _same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():                                       # bit pattern: NaNs compare, -0 differs from 0
        a, b = a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)
    return torch.equal(a, b)


def assert_same(base, got, what):
    """Dicts of host tensors, bit-identical."""
    assert base.keys() == got.keys(), (what, sorted(base), sorted(got))
    for k in base:
        assert _same(base[k], got[k]), "%s differs from the unpoisoned aligned result under %s" % (k, what)


def sweep(run, base, placements=((True, "aligned"), (False, "unaligned"))):
    """run(placement) -> dict of host tensors, once per placement and pattern with LDS poisoned before every entry; each
    result must be bit-identical to `base`, the unpoisoned aligned result."""
    for arg, label in placements:
        for pat in PATTERNS:
            with pattern(pat):
                got = run(arg)
            assert_same(base, got, "%s, %s placement" % (name(pat), label))
