"""The volume dispatch table: cases at the kernel-choice thresholds of csrc/vol.hip - AvgPool3d, the depth stage of the trilinear
interpolation, the nearest volume resize, the Conv3d weight permutations and the bf16 conversions - each with the launch it claims,
stated only through the library's host-side query uz_vol_route, which answers from the route functions the entry points
themselves dispatch through.

A resampling case is (op, C, D, H, W, f, fz, view offsets) and per direction the claim (kernel, gx):
  kernel: 0 scalar, 1 float4, 2 bf16 storage, 3 one wave per element;  gx: workgroups per plane after the cap of 64
(D, H, W) are what the entry point takes: the high-resolution volume for pool, the low-resolution one for lerp and nearest.  A
volume is [D][C + 2][H][W]; every operand is channels [C0, C0 + C) of such a buffer that starts `off` floats into a NaN-filled
allocation, off = (src, dst) with src = x / dx (the forward's input side) and dst = y / dy: an offset of 1 or 2 floats breaks
the 16-byte alignment.  Cases come in pairs, one on each side of a threshold; the comment of a group names the line it pins.
tests/test_vol_routes_cpu.py checks the claims, tests/test_vol_routes_gpu.py runs every case against fp64."""
import collections
import ctypes

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "op C D H W f fz off gpu claims")
SCALAR, VEC, ST, WAVE = 0, 1, 2, 3
# (forward op code, backward op code) of uz_vol_route and every kernel it can answer for them
OP_CODE = dict(pool=(0, 1), lerp=(2, 3), nearest=(4, 5), lerp_b16=(8, 9))
OP_KERNELS = dict(pool=({SCALAR, VEC}, {SCALAR, VEC}), lerp=({SCALAR, VEC}, {SCALAR, VEC}), nearest=({SCALAR}, {SCALAR, WAVE}),
                  lerp_b16=({ST}, {ST}))
C0 = 1


def V(op, D, H, W, fwd, bwd, C=3, f=1, fz=1, off=(0, 0), gpu=True):
    assert fwd[0] in OP_KERNELS[op][0] and bwd[0] in OP_KERNELS[op][1]
    return Case(op, C, D, H, W, f, fz, tuple(off), gpu, dict(fwd=tuple(fwd), bwd=tuple(bwd)))


def case_id(c):
    o = "" if c.off == (0, 0) else f"-off{c.off[0]}{c.off[1]}"
    return f"{c.op}-{c.C}x{c.D}x{c.H}x{c.W}" + (f"f{c.f}z{c.fz}" if c.op == "nearest" else "") + o


def planes(c):
    """Elements per plane of (src, dst)."""
    H, W = c.H, c.W
    if c.op == "pool":
        return H * W, ((H + 1) // 2) * ((W + 1) // 2)
    if c.op == "nearest":
        return H * W, c.f * c.f * H * W
    return H * W, H * W


def alignments(c):
    """Byte alignment (16, 8 or 4) of the two views as the buffers of the GPU tier place them."""
    out = []
    for plane, off in zip(planes(c), c.off):
        e = C0 * plane + off
        out.append(16 if e % 4 == 0 else 8 if e % 2 == 0 else 4)
    return tuple(out)


def query(L, op, C, D, H, W, f, fz, al_src, al_dst):
    o = (ctypes.c_int * 2)()
    rc = L.uz_vol_route(op, C, D, H, W, f, fz, al_src, al_dst, o)
    assert rc == 0, L.uz_last_error()
    return o[0], o[1]


def queries(L, c):
    """The forward takes (src, dst) = (x, y), the backward (dy, dx): the same two views, the other way round."""
    a = alignments(c)
    fo, bo = OP_CODE[c.op]
    return dict(fwd=query(L, fo, c.C, c.D, c.H, c.W, c.f, c.fz, a[0], a[1]), bwd=query(L, bo, c.C, c.D, c.H, c.W, c.f, c.fz, a[1], a[0]))


CASES = [
    # ---- AvgPool3d (pool_fwd_route / pool_bwd_route): W % 4 and two 16-byte views; odd H and odd D stay on the float4 kernels
    V("pool", 4, 8, 8, (VEC, 1), (VEC, 1)),
    V("pool", 4, 7, 8, (VEC, 1), (VEC, 1)),               # odd H: the last output row averages one input row
    V("pool", 5, 8, 8, (VEC, 1), (VEC, 1)),               # odd D: the last output slice averages one input slice
    V("pool", 5, 7, 8, (VEC, 1), (VEC, 1)),
    V("pool", 4, 8, 6, (SCALAR, 1), (SCALAR, 1)),         # W % 4 == 2
    V("pool", 5, 7, 5, (SCALAR, 1), (SCALAR, 1)),         # every edge count: 1, 2 and 4
    V("pool", 2, 3, 2, (SCALAR, 1), (SCALAR, 1)),         # one output column
    V("pool", 4, 8, 8, (SCALAR, 1), (SCALAR, 1), off=(1, 0)), V("pool", 4, 8, 8, (SCALAR, 1), (SCALAR, 1), off=(2, 0)),   # x / dx 4- and 8-byte aligned
    V("pool", 4, 8, 8, (SCALAR, 1), (SCALAR, 1), off=(0, 1)), V("pool", 4, 8, 8, (SCALAR, 1), (SCALAR, 1), off=(0, 2)),   # y / dy
    # ... gx(): 64 workgroups x 256 threads per plane, then the grid-stride loop.  float4 forward: Ho W / 4 = 16 384 | 16 640 quads;
    # float4 backward: H W / 4 = 16 384 (256 x 256) | 32 768 | 33 280
    V("pool", 3, 256, 256, (VEC, 32), (VEC, 64), C=1),
    V("pool", 2, 256, 512, (VEC, 64), (VEC, 64), C=2),
    V("pool", 3, 260, 512, (VEC, 64), (VEC, 64), C=2),
    # scalar forward: Ho Wo = 16 384 (256 x 255) | 16 641 (257 x 257); scalar backward: H W = 16 383 (127 x 129) | 65 280 | 66 049
    V("pool", 2, 127, 129, (SCALAR, 17), (SCALAR, 64), C=1),
    V("pool", 3, 256, 255, (SCALAR, 64), (SCALAR, 64), C=2),
    V("pool", 3, 257, 257, (SCALAR, 64), (SCALAR, 64), C=2),
    # ---- depth stage of trilinear x2 (lerp_route): H W % 4 and two 16-byte views; D = 1 (every output slice is the input slice), 2, 3, 7
    V("lerp", 1, 4, 8, (VEC, 1), (VEC, 1)), V("lerp", 2, 4, 8, (VEC, 1), (VEC, 1)), V("lerp", 3, 4, 8, (VEC, 1), (VEC, 1)), V("lerp", 7, 4, 8, (VEC, 1), (VEC, 1)),
    V("lerp", 1, 5, 7, (SCALAR, 1), (SCALAR, 1)), V("lerp", 2, 5, 7, (SCALAR, 1), (SCALAR, 1)), V("lerp", 7, 5, 7, (SCALAR, 1), (SCALAR, 1)),   # H W % 4 != 0
    V("lerp", 3, 4, 8, (SCALAR, 1), (SCALAR, 1), off=(1, 0)), V("lerp", 3, 4, 8, (SCALAR, 1), (SCALAR, 1), off=(0, 2)),
    # ... gx(): H W / 4 = 16 384 (256 x 256) | 16 640 (260 x 256) float4; H W = 16 383 (127 x 129) | 16 641 (129 x 129) scalar
    V("lerp", 2, 256, 256, (VEC, 64), (VEC, 64), C=2),
    V("lerp", 3, 260, 256, (VEC, 64), (VEC, 64), C=2),
    V("lerp", 2, 127, 129, (SCALAR, 64), (SCALAR, 64), C=2),
    V("lerp", 3, 129, 129, (SCALAR, 64), (SCALAR, 64), C=2),
    # ... the bf16-storage form (lerp_st_route) at D = 1 and 2
    V("lerp_b16", 1, 4, 8, (ST, 1), (ST, 1)), V("lerp_b16", 2, 4, 8, (ST, 1), (ST, 1)),
    # ---- nearest volume resize (nearest_bwd_route): f f fz >= WAVE_CHILDREN = 64 and ceil(H W / 4) <= 65 535 -> one wave per element,
    # four elements per workgroup (15 elements: the last workgroup holds 3).  48 | 64 children; 64 with fz = 1; 72 and 75: the second
    # sweep of the wave has 8 and 11 busy lanes
    V("nearest", 2, 3, 5, (SCALAR, 1), (SCALAR, 1), f=4, fz=3),
    V("nearest", 2, 3, 5, (SCALAR, 1), (WAVE, 4), f=4, fz=4),
    V("nearest", 2, 3, 5, (SCALAR, 4), (WAVE, 4), f=8, fz=1),
    V("nearest", 2, 3, 5, (SCALAR, 1), (WAVE, 4), f=3, fz=8),
    V("nearest", 2, 3, 5, (SCALAR, 2), (WAVE, 4), f=5, fz=3),
    # ... 65 535 workgroups | 65 536 would exceed the grid: thread kernel (query only: 16.7 M children per slice)
    V("nearest", 1, 510, 514, (SCALAR, 64), (WAVE, 65535), C=1, f=8, fz=1, gpu=False),
    V("nearest", 1, 512, 512, (SCALAR, 64), (SCALAR, 64), C=1, f=8, fz=1, gpu=False),
]

# ---- uz_w3d_permute (w3d_grid): (Cout, Cin, workgroups).  Cout Cin 27 = 524 286 -> 2 048 workgroups, exactly W3D_GRID_MAX, uncapped;
# 524 313 -> 2 049 capped to 2 048, the grid-stride loop wraps
PERMUTE_CASES = [(4, 5, 3), (133, 146, 2048), (3, 6473, 2048)]
PERMUTE_MODES = [0, 1, 2]

# ---- uz_cvt_f32_to_b16 / uz_cvt_b16_to_f32 (cvt_grid): (n, workgroups); 65 535 x 256 + 1 elements: one element into the second sweep
CVT_CASES = [(0, None), (1, 1), (255, 1), (256, 1), (257, 2), (65535 * 256, 65535), (65535 * 256 + 1, 65535)]


# ---- the fp64 reference of a resampling case, and the gate of the wave kernel
def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).float()


def _vol5(t):
    """[D][C][H][W] -> the (1, C, D, H, W) batch torch's 3-D ops take."""
    return t.permute(1, 0, 2, 3)[None]


def _unvol5(t):
    return t[0].permute(1, 0, 2, 3)


def ref_fn(c):
    """The operation of case c on a [D][C][H][W] tensor of any dtype, by torch's own ops."""
    if c.op == "pool":
        return lambda t: _unvol5(F.avg_pool3d(_vol5(t), 2, 2, 0, ceil_mode=True))
    if c.op == "nearest":
        return lambda t: _unvol5(F.interpolate(_vol5(t), size=[c.fz * c.D, c.f * c.H, c.f * c.W], mode="nearest"))
    return lambda t: _unvol5(F.interpolate(_vol5(t), scale_factor=(2, 1, 1), mode="trilinear", align_corners=True))


def grad(fn, x, dy, dtype=torch.float64):
    xd = x.to(dtype).requires_grad_(True)
    fn(xd).backward(dy.to(dtype))
    return xd.grad


def nearest_torch32_error(c):
    """The error of torch's own fp32 CPU backward of the case against fp64, of max(1, max |fp64|), on the GPU tier's operands
    (x = rnd(seed=1), dy = rnd(seed=2)): what NEAREST_WAVE_TORCH32 records."""
    x, fn = rnd(c.D, c.C, c.H, c.W, seed=1), ref_fn(c)
    dy = rnd(*fn(x).shape, seed=2)
    g64, g32 = grad(fn, x, dy), grad(fn, x, dy, torch.float32)
    return float((g32.double() - g64).abs().max()) / max(1.0, float(g64.abs().max()))


# per (f, fz) of the wave cases (2 slices x 3 channels of 3 x 5); the wave kernel's gate is 4 x this (tests/test_vol_routes_gpu.py)
NEAREST_WAVE_TORCH32 = {(4, 4): 2.818e-07, (8, 1): 1.987e-07, (3, 8): 2.151e-07, (5, 3): 2.397e-07}
WAVE_CASES = [c for c in CASES if c.gpu and c.op == "nearest" and c.claims["bwd"][0] == WAVE]
