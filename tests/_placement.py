"""Guarded placement of device buffers for the edge tests through the C ABI (tests/test_trunk_edges_gpu.py,
tests/test_stage0_edges_gpu.py): every buffer is a window of a larger one, filled with a sentinel outside the window,
16-byte aligned or at an odd float offset; `Place.check` verifies margins, unmodified inputs and fully written outputs
(`Place.check_untouched`: outputs left alone by a rejected call), `_both` runs a case at both placements and requires bit-identical results,
then repeats both with LDS poisoned before every entry (tests/_lds_poison.py)."""
import ctypes
import math

import torch

G = 2048 + 3                      # margin; odd, so that a window at offset G is not 16-byte aligned
SENT = 12345.0
ISENT = 0x5A5A5A5A5A5A5A5A
ERR_UNSUPPORTED, ERR_MISALIGNED = -3, -5


def _L():
    """The library handle; while tests/_lds_poison.py has a pattern set, a proxy that poisons LDS before every entry."""
    import _lds_poison
    from decnet_amd import _lib
    return _lds_poison.wrap(_lib.lib())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _vp(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_close(got, ref, tol, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got.double() - ref).abs().max()) if got.numel() else 0.0
    assert err <= tol * max(1.0, float(ref.abs().max())), (what, err)


class Place:
    """Windows of guarded buffers on the GPU: `inp` copies a host tensor in, `out` is NaN inside (or a fill), `check`
    verifies margins, unmodified inputs and fully written outputs."""

    def __init__(self, dev, aligned):
        self.dev, self.off, self.aligned = dev, G + 1 if aligned else G, aligned
        self.items = []

    def _buf(self, n, dtype):
        sent = ISENT if dtype == torch.int64 else SENT
        buf = torch.full((n + self.off + G,), sent, dtype=dtype, device=self.dev)
        win = buf[self.off:self.off + n]
        assert (win.data_ptr() % 16 == 0) == self.aligned
        return buf, win

    def inp(self, x):
        x = x.contiguous()
        buf, win = self._buf(x.numel(), x.dtype)
        win.copy_(x.reshape(-1))
        self.items.append(("in", buf, x.numel(), x.clone()))
        return win.view(x.shape)

    def out(self, shape, dtype=torch.float32, fill=float("nan")):
        n = math.prod(shape)
        buf, win = self._buf(n, dtype)
        win.fill_(fill)
        self.items.append(("out", buf, n, None))
        return win.view(shape)

    def inplace(self, x):
        buf, win = self._buf(x.numel(), x.dtype)
        win.copy_(x.reshape(-1))
        self.items.append(("inplace", buf, x.numel(), None))
        return win.view(x.shape)

    def check(self, what):
        torch.cuda.synchronize()
        for kind, buf, n, host in self.items:
            sent = ISENT if buf.dtype == torch.int64 else SENT
            assert bool((buf[:self.off] == sent).all()) and bool((buf[self.off + n:] == sent).all()), \
                "%s: write outside a %s window" % (what, kind)
            win = buf[self.off:self.off + n]
            if kind == "in":
                assert torch.equal(win.cpu().view(torch.int32 if win.dtype == torch.float32 else win.dtype),
                                   host.reshape(-1).view(torch.int32 if host.dtype == torch.float32 else host.dtype)), \
                    "%s: an input was modified" % what
            elif kind == "out" and win.dtype == torch.float32:
                assert not bool(torch.isnan(win).any()), "%s: output element not written" % what


    def check_untouched(self, what):
        """For calls that must launch nothing: margins intact and every output window still holds its NaN pre-fill."""
        torch.cuda.synchronize()
        for kind, buf, n, _ in self.items:
            assert bool((buf[:self.off] == SENT).all()) and bool((buf[self.off + n:] == SENT).all()), \
                "%s: write outside a %s window" % (what, kind)
            if kind == "out":
                assert bool(torch.isnan(buf[self.off:self.off + n]).all()), "%s: an output was written" % what


def _bn(cout, g, big=1.0):
    return (torch.rand(cout, generator=g) + 0.5) * big, torch.randn(cout, generator=g) * 0.1


def _both(run, *args):
    """run(*args, aligned) at both placements; the results must be bit-identical.  Then both placements again under each
    LDS poison pattern (tests/_lds_poison.py): bit-identical to the unpoisoned aligned results, which are returned."""
    import _lds_poison
    a = run(*args, aligned=True)
    u = run(*args, aligned=False)
    for k in a:
        assert _bits_equal(a[k], u[k]), "%s differs between aligned and unaligned placement" % k
    _lds_poison.hooks()
    _lds_poison.sweep(lambda aligned: run(*args, aligned=aligned), a)
    return a
