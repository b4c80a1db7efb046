"""The caller-workspace SpaMat / SpaVar entries (decnet_spamat_workspace_floats and the six `_ws` entries of
include/decnet_hip.h) as far as they go without a GPU: the symbols exist in the header, the library and the ctypes table;
the size query is a pure host function with the values the header states; every `_ws` entry rejects null pointers, bad
shapes and a missing / short / misaligned workspace before any HIP call, and the six legacy entries (the same pointer
counts, no workspace arguments) reject null pointers and bad shapes the same way."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
QUERY = "decnet_spamat_workspace_floats"
# entry -> (number of pointer arguments, `which` of the query)
ENTRIES = {
    "decnet_spamat_forward_ws": (7, 0),
    "decnet_spavar_forward_ws": (8, 1),
    "decnet_spamatvar_forward_ws": (8, 2),
    "decnet_spamatvar_forward_bits_ws": (8, 3),
    "decnet_spamat_backward_ws": (10, 4),
    "decnet_spavar_backward_ws": (12, 5),
}
LEGACY = {name[:-3]: v for name, v in ENTRIES.items()}          # the original entries: no workspace arguments
SHAPES = [(1, 8, 2, 460), (2, 8, 3, 300), (1, 24, 5, 1000), (1, 8, 1, 100), (3, 1, 7, 273)]     # (B, C, H, W); some W < D
WIDE = (274, 405, 621, 1089)
ONE_BAND = (1, 64, 272, 273)


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "decnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(decnet_[a-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def lib():
    from decnet_amd import build
    h = ctypes.CDLL(build.build())                      # hipcc cross-compiles for gfx950 without a GPU
    q = getattr(h, QUERY)
    q.argtypes, q.restype = [I] * 6, Z
    for name, (n, _) in ENTRIES.items():
        f = getattr(h, name)
        f.argtypes, f.restype = [P] * n + [I] * 5 + [P, Z, P], I
    for name, (n, _) in LEGACY.items():
        f = getattr(h, name)
        f.argtypes, f.restype = [P] * n + [I] * 5 + [P], I
    return h


def test_header_library_and_binding_carry_the_seven_symbols(lib):
    from decnet_amd import _lib
    syms = declared_symbols()
    for name in [QUERY] + list(ENTRIES):
        assert name in syms, "%s is not declared in include/decnet_hip.h" % name
        assert hasattr(lib, name), "libdecnet_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "%s is missing from decnet_amd._lib.SIGNATURES" % name
    assert _lib.SIGNATURES[QUERY] == [I] * 6
    for name, (n, _) in ENTRIES.items():
        assert _lib.SIGNATURES[name] == [P] * n + [I] * 5 + [P, Z, P], name


def test_query_is_zero_where_one_band_takes_the_call_and_for_bad_shapes(lib):
    q = getattr(lib, QUERY)
    for which in range(6):
        for D in ONE_BAND:
            for B, C, H, W in SHAPES:
                assert q(B, C, H, W, D, which) == 0, (B, C, H, W, D, which)
        for bad in ((0, 8, 2, 460, 405), (1, 0, 2, 460, 405), (1, 8, -1, 460, 405), (1, 8, 2, 0, 405), (1, 8, 2, 460, 0),
                    (1, 8, 2, 460, -405), (64, 64, 1024, 1024, 405)):          # the last: index space beyond 2^31
            assert q(*bad, which) == 0, (bad, which)
    for which in (-1, 6, 100):
        assert q(1, 8, 2, 460, 405, which) == 0


def test_query_above_one_band_is_positive_and_within_what_the_library_allocated_before(lib):
    q = getattr(lib, QUERY)
    for D in WIDE:
        for B, C, H, W in SHAPES:
            np_ = B * H * W
            n = [q(B, C, H, W, D, which) for which in range(6)]
            for which in range(4):
                assert 0 < n[which] <= (C + 10) * np_ + 64, (B, C, H, W, D, which, n[which])
            for which in (4, 5):
                assert 0 < n[which] <= (3 * C + 3) * np_ + 64, (B, C, H, W, D, which, n[which])
            assert n[3] >= n[2], "the bit-mask entry also holds unpacked mask planes"
            # what the header states, plane by plane
            assert n == [(C + 4) * np_, (C + 5) * np_, (C + 5) * np_, (C + 6) * np_, (3 * C + 2) * np_, (3 * C + 3) * np_]


@pytest.mark.parametrize("name", list(ENTRIES) + list(LEGACY))
def test_ws_entry_validates_before_any_hip_call(lib, name):
    """No device is needed (or present): every rejection happens on the host.  Pointers are small fake addresses.
    The legacy entries take the same tensor pointers and dims, then the stream alone."""
    entry = getattr(lib, name)
    q = getattr(lib, QUERY)
    has_ws = name in ENTRIES
    n, which = ENTRIES[name] if has_ws else LEGACY[name]
    one = 64                                                     # a fake, 16-byte aligned, never dereferenced address

    def f(*a):                                                   # a: pointers, dims, workspace, floats, stream
        return entry(*a) if has_ws else entry(*a[:-3], a[-1])

    ptrs = [one] * n
    ok = (1, 8, 2, 460)
    # null pointers: every tensor argument in turn, at one band and above
    for D in (64, 405):
        for i in range(n):
            a = list(ptrs)
            a[i] = None
            assert f(*a, *ok, D, one, 1 << 40, None) == -1, (name, i, D)
    # bad shapes
    for dims in ((0, 8, 2, 460, 405), (1, 0, 2, 460, 405), (1, 8, 0, 460, 405), (1, 8, 2, 0, 405), (1, 8, 2, 460, 0),
                 (1, 8, 2, 460, -1), (1, 8, 2, 0, 64)):
        assert f(*ptrs, *dims, one, 1 << 40, None) == -2, (name, dims)
    # a null tensor pointer wins over a bad shape
    a = list(ptrs)
    a[0] = None
    assert f(*a, 1, 8, 2, 0, 405, one, 1 << 40, None) == -1
    a = list(ptrs)
    a[n - 1] = None
    assert f(*a, 0, 8, 2, 460, 64, one, 1 << 40, None) == -1
    if not has_ws:
        return
    # the workspace contract at max_disp 405
    need = q(*ok, 405, which)
    assert need > 0
    assert f(*ptrs, *ok, 405, None, need, None) == -1            # no workspace
    assert f(*ptrs, *ok, 405, None, 0, None) == -1
    assert f(*ptrs, *ok, 405, one, need - 1, None) == -2         # too small
    assert f(*ptrs, *ok, 405, one, 0, None) == -2
    assert f(*ptrs, *ok, 405, one + 4, need, None) == -5         # an odd float offset: not 16-byte aligned
    assert f(*ptrs, *ok, 405, one + 8, need + 1000, None) == -5
    # null tensor pointers win over the workspace checks, bad shapes too (the order of the other entries)
    a = list(ptrs)
    a[0] = None
    assert f(*a, *ok, 405, None, 0, None) == -1
    assert f(*ptrs, 1, 8, 2, 0, 405, None, 0, None) == -2
