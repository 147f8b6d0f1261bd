"""Helpers for the -m gpu parity tests: call libuz_hip.so through its C ABI with torch tensors as
storage and compare with a plain fp32 PyTorch CPU reference of the same op."""
import ctypes as C

import numpy as np
import torch

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    """Call a C-ABI function; tensors become device pointers, None -> NULL; stream is appended."""
    L = _ffi.lib()
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor):
            conv.append(a.data_ptr())
        else:
            conv.append(a)
    fn = getattr(L, name)
    assert len(conv) + 1 == len(fn.argtypes), f"{name}: {len(conv) + 1} arguments for a {len(fn.argtypes)}-argument entry point"
    rc = fn(*conv, stream())
    _ffi.check(rc, name)
    torch.cuda.synchronize()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def view_in(t, ctot, c0):
    """Embed an NCHW CPU tensor as channels [c0, c0+C) of a wider GPU buffer filled with NaN canaries;
    returns (buffer, slice_view_pointer_tensor)."""
    n, c, h, w = t.shape
    buf = torch.full((n, ctot, h, w), float("nan"), device=dev())
    buf[:, c0:c0 + c] = t.to(dev())
    return buf, buf[:, c0:]


def relerr(got, ref):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def maxabs(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max())


def L():
    """The loaded C-ABI library (size queries: uz_*_workspace)."""
    return _ffi.lib()


# ---------------------------------------------------------------------------------------------- guarded buffers
CANARY = {torch.int32: -7777, torch.int64: -7777, torch.float32: -777.0, torch.float64: -777.0, torch.uint8: 0xA5}


def guarded(n, dtype, guard=64, fill=None, off=0, room=0):
    """n elements of `dtype` between two guards of `guard` elements, everything holding `fill` (CANARY[dtype] when None) -> (raw, body).
    The body starts `off` elements behind the front guard - for uint8 and a guard that is a multiple of 16, `off` bytes behind a 16-byte
    boundary; `room`: the elements set aside for that, so that buffers of several offsets have one size."""
    raw = torch.full((n + 2 * guard + max(off, room),), CANARY[dtype] if fill is None else fill, dtype=dtype, device=dev())
    assert raw.data_ptr() % 16 == 0
    return raw, raw[guard + off:guard + off + n]


def embed(arr, off, fill=0xEE):
    """the bytes of a numpy array `off` bytes behind a 16-byte boundary of a larger uint8 buffer of `fill` -> (buffer, view)"""
    b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.full((b.size + 64,), fill, dtype=torch.uint8, device=dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + b.size]
    view.copy_(torch.from_numpy(b.copy()))
    return buf, view


def intact(raw, body, fill=None):
    """every element of `raw` in front of and behind `body`, a view into it, still holds `fill` (CANARY[raw.dtype] when None)"""
    fill = CANARY[raw.dtype] if fill is None else fill
    lo = (body.data_ptr() - raw.data_ptr()) // raw.element_size()
    return bool((raw[:lo] == fill).all()) and bool((raw[lo + body.numel():] == fill).all())
