"""Operands of the dispatch-edge GPU tests (tests/test_head_routes_gpu.py, tests/test_vol_routes_gpu.py) as views inside NaN-filled
allocations: everything outside a view must keep its bits, and the view starts where the case's table says it does."""
import torch

from tests import _gpu

PAD = 8         # spare elements behind the body, so that an offset never runs off the allocation


class View:
    """An NCHW tensor (a volume: N = D) as channels [c0, c0 + C) of a buffer of C + 2 channels that starts `off` elements into a
    NaN-filled allocation of `dtype`."""

    def __init__(self, t, off, c0=1, dtype=torch.float32):
        n, c, h, w = t.shape
        size = n * (c + 2) * h * w
        self.flat = torch.full((size + off + PAD,), float("nan"), device=_gpu.dev(), dtype=dtype)
        self.body = self.flat[off:off + size].view(n, c + 2, h, w)
        self.body[:, c0:c0 + c] = t.to(_gpu.dev()).to(dtype)
        self.c, self.c0, self.ctot = c, c0, c + 2
        self.ptr = self.body[:, c0:]
        inside = torch.zeros(size + off + PAD, dtype=torch.bool, device=_gpu.dev())
        inside[off:off + size].view(n, c + 2, h, w)[:, c0:c0 + c] = True
        self.outside = ~inside
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 256 == 0

    def aligned(self):
        return self.ptr.data_ptr() % 16 == 0

    def get(self):
        return self.body[:, self.c0:self.c0 + self.c].float().cpu()

    def outside_untouched(self):
        return torch.equal(self.flat.view(self.bits)[self.outside], self.before.view(self.bits)[self.outside])

    def untouched(self):
        return torch.equal(self.flat.view(self.bits), self.before.view(self.bits))


class Flat:
    """A contiguous tensor that starts `off` elements into a NaN-filled allocation (t None: all NaN, an output to be written)."""

    def __init__(self, shape, off, t=None, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.full((off + n + PAD,), float("nan"), device=_gpu.dev(), dtype=dtype)
        self.ptr = self.flat[off:off + n].view(*shape) if n else self.flat[off:off]
        if t is not None:
            self.ptr.copy_(t.to(_gpu.dev()).to(dtype))
        self.off, self.n = off, n
        self.bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[dtype]
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 256 == 0

    def aligned(self):
        return self.ptr.data_ptr() % 16 == 0

    def get(self):
        return self.ptr.float().cpu() if self.ptr.dtype != torch.float64 else self.ptr.cpu()

    def outside_untouched(self):
        a, b = self.flat.view(self.bits), self.before.view(self.bits)
        return torch.equal(a[:self.off], b[:self.off]) and torch.equal(a[self.off + self.n:], b[self.off + self.n:])

    def untouched(self):
        return torch.equal(self.flat.view(self.bits), self.before.view(self.bits))


def rc(name, *args):
    """Call a C-ABI entry point and return its code instead of raising: a refusal is the expected answer."""
    L = _gpu.L()
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    fn = getattr(L, name)
    assert len(conv) + 1 == len(fn.argtypes), f"{name}: {len(conv) + 1} arguments for a {len(fn.argtypes)}-argument entry point"
    code = fn(*conv, _gpu.stream())
    torch.cuda.synchronize()
    return code
