"""CPU-side checks of the test-hooks library (tests/support/lds_poison.hip): it cross-compiles for gfx950 without a GPU,
exports its three entries, and stays apart from the product library and its header."""
import ctypes
import os

HOOKS = ("decnet_test_lds_poison", "decnet_test_lds_probe", "decnet_test_lds_leaky")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hooks_library_builds_and_exports_its_entries():
    from decnet_amd import build
    path = build.build_testhooks()
    assert path == build.TESTHOOKS_PATH and os.path.exists(path)
    h = ctypes.CDLL(path)
    for s in HOOKS:
        assert hasattr(h, s), "libdecnet_testhooks.so does not export %s" % s
    # argument checks come before any HIP call
    h.decnet_test_lds_probe.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    h.decnet_test_lds_leaky.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert h.decnet_test_lds_probe(0, 1, None, None) == -1
    assert h.decnet_test_lds_leaky(0.0, None, None) == -1


def test_product_library_and_header_know_nothing_of_the_hooks():
    from decnet_amd import _lib, build
    prod = ctypes.CDLL(build.build())
    for s in HOOKS:
        assert not hasattr(prod, s), "libdecnet_hip.so exports the test hook %s" % s
    assert not any(s.startswith("decnet_test_") for s in _lib.SIGNATURES)
    assert "decnet_test_" not in open(os.path.join(ROOT, "include", "decnet_hip.h")).read()
    assert os.path.dirname(build.TESTHOOKS_SRC) == os.path.join(ROOT, "tests", "support")
