"""The streaming dispatch table: cases at the kernel-choice thresholds of the resampling ops (csrc/resample.hip) and of the loss,
latent, optimiser, norm and add_views kernels (csrc/pointwise.hip), each with the route it claims, stated only through the
library's host-side queries.

A resampling / add_views case is (op, N, C, H, W, factor, view offsets) and the values the queries answer for it:
  route = uz_stream_route(op, ...): 0 generic / scalar kernel, 1 vector or band kernel, 2 float4 backward band, 3 one wave per element
  rows  = uz_resample_bwd_relu_rows(kind, ...) for the backward passes: N x the workgroups per plane (band kernels: 1 from 2 048 planes on)
Every operand is a channel-slice view: channels [1, 1 + C) of a buffer of C + 2 channels that starts `off` floats into a
NaN-filled allocation, so the view begins (plane + off) floats past a 256-byte boundary.  off = (src, dst, aux) for
src = x / dy / a, dst = y / dx, aux = the activation of a *_relu form / b of add_views: an offset of 1 or 2 floats breaks 16- or
8-byte alignment.  H x W is the plane the entry point takes: the high-resolution one for avgpool, the low-resolution one for
bilinear and nearest.  Cases come in pairs, one on each side of a threshold; the comment of a group names the line it pins.
tests/test_stream_routes_cpu.py checks the claims, tests/test_stream_routes_gpu.py runs every case against an fp64 reference."""
import collections

Case = collections.namedtuple("Case", "op N C H W f off opt claims")
OP_CODE = dict(avgpool_fwd=0, avgpool_bwd=1, avgpool_bwd_relu=1, bilinear_fwd=2, bilinear_bwd=3, bilinear_bwd_relu=3, nearest=4, add_views=5)
# every value uz_stream_route can answer for the op
OP_ROUTES = dict(avgpool_fwd={0, 1}, avgpool_bwd={0, 1}, bilinear_fwd={0, 1}, bilinear_bwd={0, 1, 2}, nearest={0, 3}, add_views={0, 1})
C0 = 1          # first channel of every view; the buffers hold C + 2 channels


def S(op, H, W, route, N=2, C=3, f=0, off=(0, 0, 0), rows=None, **opt):
    assert op in OP_CODE and route in OP_ROUTES[op.replace("_relu", "")]
    claims = dict(route=route)
    if rows is not None:
        claims["rows"] = rows
    return Case(op, N, C, H, W, f, tuple(off), opt, claims)


def case_id(c):
    o = "" if c.off == (0, 0, 0) else "-off" + "".join(map(str, c.off))
    x = "".join(f"-{k}{v}" for k, v in sorted(c.opt.items()))
    return f"{c.op}-{c.N}x{c.C}x{c.H}x{c.W}" + (f"f{c.f}" if c.f else "") + o + x


def planes(c):
    """Elements per plane of (src, dst, aux); aux None where the op has none."""
    H, W = c.H, c.W
    lo = ((H + 1) // 2) * ((W + 1) // 2)
    return {"avgpool_fwd": (H * W, lo, None), "avgpool_bwd": (lo, H * W, None), "avgpool_bwd_relu": (lo, H * W, H * W),
            "bilinear_fwd": (H * W, 4 * H * W, None), "bilinear_bwd": (4 * H * W, H * W, None), "bilinear_bwd_relu": (4 * H * W, H * W, H * W),
            "nearest": (c.f * c.f * H * W, H * W, None),
            "add_views": (H * W, H * W, H * W if c.opt.get("b", 1) else None)}[c.op]


def alignments(c):
    """Byte alignment (16, 8 or 4) of the three views as the buffers of the GPU tier place them; 16 for an absent operand."""
    out = []
    for plane, off in zip(planes(c), c.off):
        e = 0 if plane is None else C0 * plane + off
        out.append(16 if e % 4 == 0 else 8 if e % 2 == 0 else 4)
    return tuple(out)


def queries(L, c):
    a = alignments(c)
    got = dict(route=L.uz_stream_route(OP_CODE[c.op], c.C, c.N, c.H, c.W, c.f, *a))
    if "rows" in c.claims:
        got["rows"] = L.uz_resample_bwd_relu_rows(0 if c.op.startswith("avgpool") else 1, c.C, c.N, c.H, c.W)
    return got


CASES = [
    # ---- avgpool (resample.hip avgpool_fwd_route / avgpool_bwd_route): H % 2, W % 4, x / dx 16-byte, y / dy 8-byte, mask 16-byte
    S("avgpool_fwd", 8, 8, 1), S("avgpool_bwd", 8, 8, 1, rows=2),
    S("avgpool_fwd", 7, 8, 0), S("avgpool_bwd", 7, 8, 0, rows=2),                 # odd H with W % 4 == 0 (bottom windows of one row)
    S("avgpool_fwd", 8, 6, 0), S("avgpool_bwd", 8, 6, 0, rows=2),                 # even H with W % 4 == 2
    S("avgpool_fwd", 7, 5, 0), S("avgpool_bwd", 7, 5, 0, rows=2),                 # edge counts 1 and 2
    S("avgpool_fwd", 1, 1, 0), S("avgpool_bwd", 1, 1, 0, rows=2),
    S("avgpool_fwd", 8, 8, 0, off=(1, 0, 0)),                                     # x 4-byte aligned: scalar by alignment
    S("avgpool_fwd", 8, 8, 0, off=(2, 0, 0)),                                     # x 8-byte: still short of the float4 loads
    S("avgpool_fwd", 8, 8, 0, off=(0, 1, 0)),                                     # y 4-byte
    S("avgpool_fwd", 8, 8, 1, off=(0, 2, 0)),                                     # y 8-byte is enough for the float2 stores
    S("avgpool_bwd", 8, 8, 0, off=(1, 0, 0), rows=2),                             # dy 4-byte
    S("avgpool_bwd", 8, 8, 1, off=(2, 0, 0), rows=2),                             # dy 8-byte: float2 loads
    S("avgpool_bwd", 8, 8, 0, off=(0, 1, 0), rows=2),                             # dx 4-byte
    S("avgpool_bwd", 8, 8, 0, off=(0, 2, 0), rows=2),                             # dx 8-byte: short of the float4 stores
    # PCH = 4096 outputs per workgroup: 65 x 64 = 4 160 (two workgroups of the float2 kernel), 65 x 65 = 4 225 (scalar)
    S("avgpool_fwd", 130, 128, 1), S("avgpool_bwd", 130, 128, 1, rows=10),
    S("avgpool_fwd", 129, 130, 0), S("avgpool_bwd", 129, 130, 0, rows=10),
    S("avgpool_bwd_relu", 8, 8, 1, rows=2),
    S("avgpool_bwd_relu", 8, 8, 0, off=(0, 0, 1), rows=2),                        # the mask's alignment alone selects the scalar kernel
    S("avgpool_bwd_relu", 130, 128, 1, rows=10),                                  # five partial rows per image
    # ---- bilinear forward (bilinear_fwd_route): W % 4, W <= FWMAX = 128, H >= 4, both views 16-byte; OB = 32 output rows per band
    S("bilinear_fwd", 4, 4, 1),
    S("bilinear_fwd", 3, 4, 0),                                                   # H = 3 < 4
    S("bilinear_fwd", 4, 6, 0),                                                   # W % 4 == 2
    S("bilinear_fwd", 4, 128, 1), S("bilinear_fwd", 4, 132, 0),                   # FWMAX and the next multiple of 4
    S("bilinear_fwd", 16, 8, 1),                                                  # exactly one band
    S("bilinear_fwd", 17, 8, 1),                                                  # a last band of two output rows
    S("bilinear_fwd", 33, 8, 1),                                                  # three bands, the last of two rows
    S("bilinear_fwd", 4, 8, 1), S("bilinear_fwd", 4, 8, 0, off=(1, 0, 0)), S("bilinear_fwd", 4, 8, 0, off=(0, 2, 0)),   # x 4-byte, y 8-byte
    S("bilinear_fwd", 33, 66, 0),                                                 # generic, 8 712 outputs: three workgroups per plane
    # ---- bilinear backward (bilinear_bwd_route, bilinear_bwd_band_shape, bilinear_bwd_quad_shape, bilinear_bwd_band_gx):
    # 2 W <= BWMAX = 128, H >= 4, 256 % W == 0, dy 8-byte -> band; W >= 32, 64 % (W / 2) == 0, dy 16-byte, dx 8-byte -> float4 band
    S("bilinear_bwd", 4, 1, 1, rows=2), S("bilinear_bwd", 4, 2, 1, rows=2), S("bilinear_bwd", 4, 16, 1, rows=2),
    S("bilinear_bwd", 3, 16, 0, rows=2),                                          # H = 3 < 4
    S("bilinear_bwd", 4, 24, 0, rows=2),                                          # 256 % 24 != 0
    S("bilinear_bwd", 4, 64, 2, rows=2), S("bilinear_bwd", 4, 128, 0, rows=2),    # 2 W = 128 against 2 W = 256
    S("bilinear_bwd", 4, 32, 2, rows=2),                                          # W = 32 against W = 16 above: the float4 kernel's first width
    S("bilinear_bwd", 16, 32, 2, rows=2), S("bilinear_bwd", 17, 32, 2, rows=4), S("bilinear_bwd", 33, 32, 2, rows=6),   # LB = 16 rows per band: full, tail of 1, two full + 1
    S("bilinear_bwd", 16, 16, 1, rows=2), S("bilinear_bwd", 17, 16, 1, rows=4), S("bilinear_bwd", 33, 16, 1, rows=6),
    # C N = 2 047 / 2 048: a workgroup per band against one workgroup walking the two bands of its plane
    S("bilinear_bwd", 20, 32, 2, N=1, C=2047, rows=2), S("bilinear_bwd", 20, 32, 2, N=1, C=2048, rows=1),
    S("bilinear_bwd", 20, 16, 1, N=1, C=2047, rows=2), S("bilinear_bwd", 20, 16, 1, N=1, C=2048, rows=1),
    S("bilinear_bwd", 4, 32, 1, off=(2, 0, 0), rows=2),                           # dy 8-byte only: from the float4 to the pair kernel
    S("bilinear_bwd", 4, 32, 0, off=(1, 0, 0)),                                   # dy 4-byte: generic
    S("bilinear_bwd", 4, 32, 1, off=(0, 1, 0), rows=2),                           # dx 4-byte: pair kernel (scalar stores)
    S("bilinear_bwd", 4, 32, 2, off=(0, 2, 0), rows=2),                           # dx 8-byte is enough for the float2 stores
    S("bilinear_bwd_relu", 20, 32, 2, N=1, C=2047, rows=2), S("bilinear_bwd_relu", 20, 32, 2, N=1, C=2048, rows=1),
    # ---- nearest (nearest_bwd_route): f f >= 64 and ceil(H W / 4) <= 65 535 -> one wave per element, four elements per workgroup
    S("nearest", 3, 5, 0, f=3), S("nearest", 3, 5, 0, f=7), S("nearest", 3, 5, 3, f=8), S("nearest", 3, 5, 3, f=16),   # 15 elements: the last workgroup holds 3
    S("nearest", 1, 1, 0, f=3), S("nearest", 1, 1, 0, f=7), S("nearest", 1, 1, 3, f=8), S("nearest", 1, 1, 3, f=16),
    S("nearest", 510, 514, 3, N=1, C=1, f=8),                                     # 262 140 elements: grid.x = 65 535
    S("nearest", 512, 512, 0, N=1, C=1, f=8),                                     # 65 536 workgroups would exceed the grid: thread kernel
    # ---- add_views (pointwise.hip add_views_route): H W % 4 and three 16-byte views; the grid's x extent is capped at 1 024
    S("add_views", 3, 3, 0),
    S("add_views", 4, 4, 1),
    S("add_views", 4, 4, 0, off=(1, 0, 0)), S("add_views", 4, 4, 0, off=(0, 2, 0)), S("add_views", 4, 4, 0, off=(0, 0, 1)),   # a, y, b in turn
    S("add_views", 4, 4, 1, off=(0, 0, 1), b=0),                                  # no b: its alignment constrains nothing
    S("add_views", 128, 128, 1, N=1, C=64),                                       # 262 144 float4: gx = 1 024 exactly
    S("add_views", 128, 128, 1, N=1, C=65),                                       # gx capped: the grid-stride loop wraps
    S("add_views", 127, 129, 0, N=1, C=17),                                       # scalar kernel with a capped grid (278 511 elements)
]

# ---- uz_kl_fwd_ws (pointwise.hip kl_parts): (N, per_sample, parts).  One workgroup up to 131 072 elements, then chunks of 65 536,
# from 65 chunks on re-chunked to at most 64 partials
KL_CASES = [
    (1, 131072, 1), (1, 131073, 3),
    (2, 65536, 1), (3, 43691, 3),                       # the same totals over several samples
    (1, 4194304, 64), (1, 4194305, 64),                 # 64 chunks of 65 536 against 64 chunks of 66 560 (the last one short)
    (4, 250, 1),
]
# uz_kl_bwd: (N, per_sample) at the vgrid cap of 2 048 x 256 threads
KL_BWD_CASES = [(1, 524288), (1, 524289), (4, 250)]

# ---- residual CE / accumulate-softmax-argmax: (K, L) x H x W with N = 3; ce_blocks = min(64, ceil(H W / 1024))
CE_KL = [(2, 1), (3, 5), (4, 8)]
CE_HW = [(1, 1), (1, 1023), (1, 1025), (255, 257), (256, 257)]         # 65 535 -> 64 workgroups exactly; 65 792 -> clamped, the loop wraps

# ---- Adam, latent sample, axpy, scale: tails around one workgroup and the wrap of the 2 048-workgroup grid
VEC_N = [1, 255, 256, 257, 524288, 524289]

# ---- spatial mean / broadcast
MEAN_HW = [(1, 1), (16, 16), (17, 16), (33, 17)]                         # 256 threads per plane: 1, 256, 272, 561 elements
BCAST_HW = [(32, 32), (25, 41)]                                          # 1 024 elements per workgroup column: 1 024 and 1 025
BCAST_L = [1, 4]

# ---- l2 norms: element counts placed at every residue of the offset mod 4 in one flat buffer
NORM_COUNTS = [0, 1, 2, 3, 5, 331776]
