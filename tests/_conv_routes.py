"""The convolution dispatch table: one list of cases at the routing thresholds of the 3x3 convolution family, each with the
route it claims, stated only through the library's host-side queries.

A case is (direction, math mode, N, Cin, Cout, H, W, ks) and the values the queries return for it under that mode
(uz_set_conv_math: 0 fp32 MFMA, 1 default policy, 2 split-fp16 everywhere, 3 single-piece bf16):
  fwd    route = uz_conv_route(0, ...), parts = uz_conv_split_parts(0, ...), cot = uz_conv_pack_cot(..., 0), bn = uz_conv_bn_partials
  dgrad  route = uz_conv_route(1, ...), parts = uz_conv_split_parts(1, ...), cot = uz_conv_pack_cot(..., 1), relu = uz_conv_bwd_relu_partials
  wgrad  route = uz_conv_route(2, ...), slabs = uz_conv_bwd_weight_slabs
(route: 0 fp32 MFMA, 1 split-fp16 / bf16 MFMA, 2 streaming kernels.)  Cases come in pairs, one on each side of a threshold; the
comment of a group names the code it pins.  tests/test_conv_routes_cpu.py checks the claims, tests/test_conv_routes_gpu.py runs
every case with gpu=True against an fp64 reference."""
import collections
import contextlib
import os

Route = collections.namedtuple("Route", "direction mode N Cin Cout H W ks claims gpu")
DIRECTIONS = ("fwd", "dgrad", "wgrad")


def R(direction, mode, N, Cin, Cout, H, W, ks, gpu=True, **claims):
    assert direction in DIRECTIONS and mode in (0, 1, 2, 3)
    return Route(direction, mode, N, Cin, Cout, H, W, ks, claims, gpu)


def case_id(c):
    return f"{c.direction}-m{c.mode}-{c.N}x{c.Cin}x{c.Cout}x{c.H}x{c.W}k{c.ks}"


@contextlib.contextmanager
def dispatch_state(L, mode):
    """Math mode `mode` and the default weight-gradient workgroup target (256; the model plans retune it for the whole process, and
    the split weight gradient's slab count follows it) for the duration of the block; both are restored after."""
    old_mode, old_target = L.uz_get_conv_math(), L.uz_get_wgrad_target()
    try:
        assert L.uz_set_conv_math(mode) == 0
        L.uz_set_wgrad_target(256)
        yield
    finally:
        L.uz_set_wgrad_target(old_target)
        L.uz_set_conv_math(-1 if os.environ.get("UZ_CONV_MATH") is None else old_mode)


def queries(L, c):
    """What the host-side queries answer for case c in the current dispatch state (the caller enters dispatch_state(L, c.mode))."""
    N, Ci, Co, H, W, ks = c.N, c.Cin, c.Cout, c.H, c.W, c.ks
    if c.direction == "fwd":
        return dict(route=L.uz_conv_route(0, Ci, Co, N, H, W, ks), parts=L.uz_conv_split_parts(0, Ci, Co, N, H, W),
                    cot=L.uz_conv_pack_cot(Ci, Co, W, 0), bn=L.uz_conv_bn_partials(Ci, Co, N, H, W, ks))
    if c.direction == "dgrad":
        return dict(route=L.uz_conv_route(1, Ci, Co, N, H, W, ks), parts=L.uz_conv_split_parts(1, Ci, Co, N, H, W),
                    cot=L.uz_conv_pack_cot(Ci, Co, W, 1), relu=L.uz_conv_bwd_relu_partials(Ci, Co, N, H, W, ks))
    return dict(route=L.uz_conv_route(2, Ci, Co, N, H, W, ks), slabs=L.uz_conv_bwd_weight_slabs(Ci, Co, N, H, W, ks))


CASES = [
    # ---- forward / data gradient: conv_split_ok, small_geo, tile_cot, split_parts (conv_split.hip) and the thin forward (conv_mfma.hip)
    # W = 32 / 33: small_geo (conv_split.hip) - 16 x 16 tiles at grid 40 (split) against 16 x 32 tiles at grid 40 < min_grid (fp32)
    R("fwd", 1, 20, 32, 32, 16, 32, 3, route=1, parts=1, cot=32, bn=40),                    # W = 32: 16 x 16 geometry, grid 40 = gmin16
    R("fwd", 1, 20, 32, 32, 16, 33, 3, route=0, parts=1, cot=32, bn=0),                     # W = 33: 16 x 32 geometry, grid 40 < min_grid, one-column ragged tile
    R("dgrad", 1, 20, 32, 32, 16, 32, 3, route=1, parts=1, cot=32, relu=40),                # the same boundary in the data gradient
    R("dgrad", 1, 20, 32, 32, 16, 33, 3, route=0, parts=1, cot=32, relu=0),
    # H = 15 / 16: conv_split_ok - H < 16 (16 x 32 tiles) and H >= 16 (16 x 16 tiles)
    R("fwd", 1, 16, 32, 64, 16, 128, 3, route=1, parts=1, cot=32, bn=128),                  # grid 64 = min_grid; cot 32 (Kc <= 32)
    R("fwd", 1, 16, 32, 64, 15, 128, 3, route=0, parts=1, cot=32, bn=0),
    R("fwd", 1, 20, 32, 32, 15, 32, 3, route=0, parts=1, cot=32, bn=0),
    # Kc = 4 / 5 / 15 / 16 beside N H W = 262 143 / 262 144 (conv_split_ok: kcmin and the big-tensor clause)
    R("fwd", 1, 16, 16, 32, 128, 128, 3, route=1, parts=1, cot=32, bn=1024),                # Kc = 16, 262 144 px
    R("fwd", 1, 1, 16, 32, 511, 513, 3, route=1, parts=1, cot=32, bn=1088),                 # Kc = 16, 262 143 px: dense chunk, no big-tensor clause needed
    R("fwd", 1, 16, 15, 32, 128, 128, 3, route=1, parts=1, cot=32, bn=1024),                # Kc = 15 (one chunk, K tail 15) at 262 144 px
    R("fwd", 1, 1, 15, 32, 511, 513, 3, route=0, parts=1, cot=32, bn=0),                    # Kc = 15 at 262 143 px
    R("fwd", 1, 16, 5, 32, 128, 128, 3, route=1, parts=1, cot=32, bn=1024),                 # Kc = 5 = kcmin at 262 144 px
    R("fwd", 1, 1, 5, 32, 511, 513, 3, route=0, parts=1, cot=32, bn=0),                     # Kc = 5 at 262 143 px
    R("dgrad", 1, 16, 32, 5, 128, 128, 3, route=1, parts=1, cot=32, relu=1024),             # data gradient Kc = Cout = 5
    R("dgrad", 1, 16, 32, 4, 128, 128, 3, route=0, parts=1, cot=32, relu=0),                # Kc = 4 < kcmin
    # Mc = 31 / 32 below 262 144 px (conv_split_ok), and Mc = 31 beside it
    R("fwd", 1, 16, 32, 32, 16, 128, 3, route=1, parts=1, cot=32, bn=128),                  # grid 64
    R("fwd", 1, 16, 32, 31, 16, 128, 3, route=0, parts=1, cot=32, bn=0),
    R("fwd", 1, 16, 16, 31, 128, 128, 3, route=1, parts=1, cot=32, bn=1024),                # Mc = 31 at 262 144 px: a 32-wide tile one channel short
    # 64-tile grid 63 / 64 (conv_split_ok: min_grid)
    R("fwd", 1, 21, 32, 64, 16, 96, 3, route=0, parts=1, cot=32, bn=0),                     # grid 21 x 3 = 63
    R("fwd", 1, 32, 32, 64, 16, 64, 3, route=1, parts=1, cot=32, bn=128),                   # grid 32 x 2 = 64
    # 16 x 16 grid 39 / 40 (conv_split_ok: gmin16)
    R("fwd", 1, 39, 32, 32, 16, 16, 3, route=0, parts=1, cot=32, bn=0),
    R("fwd", 1, 40, 32, 32, 16, 16, 3, route=1, parts=1, cot=32, bn=40),
    R("dgrad", 1, 39, 32, 32, 16, 16, 3, route=0, parts=1, cot=32, relu=0),
    R("dgrad", 1, 40, 32, 32, 16, 16, 3, route=1, parts=1, cot=32, relu=40),
    # tile_cot (conv_split.hip): Kc 32 / 33 and Mc 32 / 33 on the 16 x 32 geometry; K tail of 1; overhang of 1 on the 64 tile
    R("fwd", 1, 16, 33, 64, 16, 128, 3, route=1, parts=1, cot=64, bn=128),                  # cot 64, K tail of 1 channel
    R("fwd", 1, 16, 64, 32, 16, 128, 3, route=1, parts=1, cot=32, bn=128),                  # cot 32 (Mc <= 32)
    R("fwd", 1, 16, 64, 33, 16, 128, 3, route=1, parts=1, cot=64, bn=128),                  # cot 64 with 31 empty channels
    R("fwd", 1, 16, 64, 65, 16, 128, 3, route=1, parts=1, cot=64, bn=128),                  # two 64 tiles, the second overhangs by 1 channel
    R("dgrad", 1, 16, 65, 64, 16, 128, 3, route=1, parts=1, cot=64, relu=128),              # the same in the data gradient: Mc = Cin = 65
    R("fwd", 1, 16, 95, 64, 16, 128, 3, route=1, parts=1, cot=64, bn=128),                  # K tail of 15 channels
    # ... in mode 3 the 128-channel tile from Mc = 65 on (tile_cot)
    R("fwd", 3, 16, 64, 64, 16, 128, 3, route=1, parts=1, cot=64, bn=128),
    R("fwd", 3, 16, 64, 65, 16, 128, 3, route=1, parts=1, cot=128, bn=128),                 # 128 tile overhanging by 63
    R("fwd", 3, 16, 64, 129, 16, 128, 3, route=1, parts=1, cot=128, bn=128),                # 128 tile overhanging by 1
    R("dgrad", 3, 16, 129, 64, 16, 128, 3, route=1, parts=1, cot=128, relu=128),
    # split_parts (conv_split.hip): grid 159 / 160 (gmin), nChunks 5 / 6 (the nChunks / 3 cap), the S = 4 cap (smax)
    R("fwd", 1, 159, 96, 32, 16, 16, 3, route=1, parts=2, cot=32, bn=0),                    # g = 159: S = 2 (6 chunks)
    R("fwd", 1, 160, 96, 32, 16, 16, 3, route=1, parts=1, cot=32, bn=160),                  # g = 160: unsplit
    R("dgrad", 1, 159, 32, 96, 16, 16, 3, route=1, parts=2, cot=32, relu=0),
    R("dgrad", 1, 160, 32, 96, 16, 16, 3, route=1, parts=1, cot=32, relu=160),
    R("fwd", 1, 20, 80, 32, 16, 32, 3, route=1, parts=1, cot=32, bn=40),                    # 5 chunks: S = 5 / 3 = 1
    R("fwd", 1, 20, 81, 32, 16, 32, 3, route=1, parts=2, cot=32, bn=0),                     # 6 chunks, K tail of 1: S = 2, 3 chunks per part
    R("fwd", 1, 20, 192, 32, 16, 32, 3, route=1, parts=4, cot=32, bn=0),                    # 12 chunks: S = 4 by the nChunks / 3 cap
    R("fwd", 1, 20, 240, 32, 16, 32, 3, route=1, parts=4, cot=32, bn=0),                    # 15 chunks: S = 4 by the smax cap (nChunks / 3 = 5)
    R("fwd", 1, 20, 33, 33, 16, 32, 3, route=1, parts=1, cot=32, bn=40),                    # 32-channel tile overhanging by 1, K tail of 1
    # thin forward (conv_thin_ok, conv_mfma.hip): Cin 4 / 5, N H W 65 535 / 65 536, Cout 256 / 257
    R("fwd", 1, 4, 4, 32, 128, 128, 3, route=2, parts=1, cot=32, bn=0),
    R("fwd", 1, 4, 5, 32, 128, 128, 3, route=0, parts=1, cot=32, bn=0),
    R("fwd", 1, 5, 4, 32, 51, 257, 3, route=0, parts=1, cot=32, bn=0),                      # 65 535 px
    R("fwd", 1, 4, 4, 256, 128, 128, 3, route=2, parts=1, cot=32, bn=0),
    R("fwd", 1, 4, 4, 257, 128, 128, 3, route=0, parts=1, cot=32, bn=0),
    # the other math modes on shapes that route to the split kernels by default
    R("fwd", 0, 16, 33, 64, 16, 128, 3, route=0, parts=1, cot=64, bn=0),
    R("dgrad", 0, 16, 65, 64, 16, 128, 3, route=0, parts=1, cot=64, relu=0),
    R("fwd", 0, 20, 81, 32, 16, 32, 3, route=0, parts=2, cot=32, bn=0),
    R("fwd", 0, 16, 16, 32, 128, 128, 3, route=0, parts=1, cot=32, bn=0),
    R("fwd", 0, 2, 38, 32, 16, 16, 1, route=0, parts=1, cot=32, bn=0),                      # 1 x 1 kernel (Fcomb)
    R("fwd", 0, 3, 20, 24, 5, 1, 3, route=0, parts=1, cot=32, bn=0),                        # one-pixel-wide plane (column tiles of width 1)
    R("dgrad", 0, 3, 20, 24, 5, 1, 3, route=0, parts=1, cot=32, relu=0),
    R("fwd", 0, 2, 8, 8, 1, 1, 3, route=0, parts=1, cot=32, bn=0),                          # 1 x 1 plane (the small fixture's deepest level)
    R("fwd", 2, 3, 5, 7, 13, 9, 3, route=1, parts=1, cot=32, bn=3),                         # split forced: ragged everything
    R("fwd", 2, 2, 1, 40, 17, 40, 3, route=1, parts=1, cot=32, bn=16),                      # one input channel
    R("dgrad", 2, 3, 5, 7, 13, 9, 3, route=1, parts=1, cot=32, relu=3),
    R("dgrad", 2, 2, 40, 3, 20, 48, 3, route=1, parts=1, cot=32, relu=16),
    R("fwd", 2, 2, 33, 65, 15, 33, 3, route=1, parts=1, cot=64, bn=8),                      # K tail 1, overhang 1, H < 16 and W = 33 on the 16 x 32 tiles
    R("fwd", 3, 20, 33, 33, 16, 32, 3, route=1, parts=1, cot=32, bn=40),
    R("dgrad", 3, 20, 32, 32, 16, 33, 3, route=0, parts=1, cot=32, relu=0),
    R("fwd", 3, 16, 16, 32, 128, 128, 3, route=1, parts=1, cot=32, bn=1024),
    # ---- weight gradient: wgrad_split_ok, chan_tile (conv_wgrad_split.hip), wgrad_thin_ok, pick_wgeom, wgrad_route (conv_wgrad.hip)
    # W = 16 / 24 / 32 / 48 / 64 (wgrad_split_ok: W % 32, W == 16)
    R("wgrad", 1, 8, 64, 64, 16, 16, 3, route=1, slabs=16),                                 # 2 048 px = pxmin
    R("wgrad", 1, 8, 64, 64, 16, 24, 3, route=0, slabs=64),
    R("wgrad", 1, 8, 64, 64, 16, 32, 3, route=1, slabs=32),
    R("wgrad", 1, 8, 64, 64, 16, 48, 3, route=0, slabs=128),
    R("wgrad", 1, 8, 64, 64, 16, 64, 3, route=1, slabs=64),
    # H = 15 / 16 (wgrad_split_ok)
    R("wgrad", 1, 8, 64, 64, 15, 32, 3, route=0, slabs=64),
    # Cin, Cout 63 / 64 at 2 032 / 2 048 px (wgrad_split_ok: pixel counts of 16-wide rows are multiples of 16, so 2 047 cannot be formed)
    R("wgrad", 1, 1, 64, 64, 128, 16, 3, route=1, slabs=16),
    R("wgrad", 1, 1, 64, 64, 127, 16, 3, route=0, slabs=32),
    R("wgrad", 1, 1, 63, 64, 128, 16, 3, route=0, slabs=32),
    R("wgrad", 1, 1, 64, 63, 128, 16, 3, route=0, slabs=32),
    # narrow side 15 / 16 / 32 / 33 beside 131 072 px (wgrad_split_ok), 131 040 px below it
    R("wgrad", 1, 8, 16, 64, 128, 128, 3, route=1, slabs=128),
    R("wgrad", 1, 8, 15, 64, 128, 128, 3, route=0, slabs=512),
    R("wgrad", 1, 8, 32, 64, 128, 128, 3, route=1, slabs=128),
    R("wgrad", 1, 8, 64, 33, 128, 128, 3, route=0, slabs=256),
    R("wgrad", 1, 5, 16, 64, 819, 32, 3, route=0, slabs=342),                               # 131 040 px
    # narrow side 4 / 5 beside 524 288 px (lomin), 524 256 px below it
    R("wgrad", 1, 32, 32, 5, 128, 128, 3, route=1, slabs=256),
    R("wgrad", 1, 32, 32, 4, 128, 128, 3, route=0, slabs=512),
    R("wgrad", 1, 129, 32, 5, 127, 32, 3, route=0, slabs=459),                              # 524 256 px, ragged H (127 rows)
    # chan_tile 32 / 33 (conv_wgrad_split.hip; forced split: the default policy never pairs a 33-channel side with the 64 tile)
    R("wgrad", 2, 32, 32, 64, 32, 32, 3, route=1, slabs=85),
    R("wgrad", 2, 32, 33, 64, 32, 32, 3, route=1, slabs=128),
    # ragged H (rows per 128-pixel tile: 4 at W = 32, 8 at W = 16)
    R("wgrad", 1, 8, 64, 64, 18, 32, 3, route=1, slabs=40),
    R("wgrad", 1, 8, 64, 96, 17, 16, 3, route=1, slabs=24),
    # fp32 path (pick_wgeom, conv_wgrad.hip): pow2_ceil tile widths, the 128-pixel fast tile, batch tiles, ks = 1
    R("wgrad", 0, 3, 20, 24, 5, 1, 3, route=0, slabs=4),                                    # TW = 1: the pixel pair of an MFMA step is two rows of one image
    R("wgrad", 0, 2, 8, 8, 1, 1, 3, route=0, slabs=4),                                      # TW = TH = 1: ... two images
    R("wgrad", 0, 3, 20, 24, 5, 3, 3, route=0, slabs=8),
    R("wgrad", 0, 3, 20, 24, 5, 7, 3, route=0, slabs=3),
    R("wgrad", 0, 3, 20, 24, 5, 8, 3, route=0, slabs=3),
    R("wgrad", 0, 3, 20, 24, 5, 9, 3, route=0, slabs=6),
    R("wgrad", 0, 3, 20, 24, 5, 15, 3, route=0, slabs=6),
    R("wgrad", 0, 3, 20, 24, 5, 17, 3, route=0, slabs=9),
    R("wgrad", 0, 3, 20, 24, 5, 31, 3, route=0, slabs=9),
    R("wgrad", 0, 3, 20, 24, 5, 33, 3, route=0, slabs=18),
    R("wgrad", 0, 2, 32, 32, 63, 32, 3, route=0, slabs=64),                                 # 64-pixel tiles (2 x 32)
    R("wgrad", 0, 2, 32, 32, 64, 32, 3, route=0, slabs=32),                                 # 128-pixel fast tile (4 x 32)
    R("wgrad", 0, 5, 24, 40, 4, 4, 3, route=0, slabs=4),                                    # batch tiles TB = 4, the second ragged
    R("wgrad", 0, 3, 24, 40, 2, 2, 3, route=0, slabs=2),                                    # TB = 4 over 3 images
    R("wgrad", 0, 2, 38, 32, 16, 16, 1, route=0, slabs=32),                                 # 1 x 1 kernel
    R("wgrad", 1, 2, 38, 32, 16, 16, 1, route=0, slabs=32),
    R("wgrad", 0, 8, 64, 64, 16, 32, 3, route=0, slabs=64),                                 # a split-path shape on the fp32 kernel
    # thin path (wgrad_thin_ok, conv_wgrad.hip): Cin 4 / 5, H even / odd (THIN_ROWS), W = 128 / 160 (THIN_WMAX), 65 536 / 65 280 px
    R("wgrad", 1, 4, 4, 32, 128, 128, 3, route=2, slabs=256),
    R("wgrad", 1, 4, 5, 32, 128, 128, 3, route=0, slabs=512),
    R("wgrad", 1, 4, 4, 32, 127, 128, 3, route=0, slabs=512),
    R("wgrad", 1, 4, 4, 32, 128, 160, 3, route=0, slabs=320),
    R("wgrad", 1, 1, 4, 32, 510, 128, 3, route=0, slabs=512),                               # 65 280 px
    R("wgrad", 1, 8, 3, 40, 64, 128, 3, route=2, slabs=256),                                # 3 channels, two output-channel tiles (the second ragged)
    # the bf16 mode
    R("wgrad", 3, 8, 64, 64, 16, 32, 3, route=1, slabs=32),
    R("wgrad", 3, 8, 16, 64, 128, 128, 3, route=1, slabs=128),
    R("wgrad", 3, 8, 64, 96, 17, 16, 3, route=1, slabs=24),
    # pick_wgeom's huge branch (wgrad_huge): 2^30 elements in one operand take the generic 64-bit kernel (query only: too big for an fp64 reference)
    R("wgrad", 0, 256, 256, 32, 128, 128, 3, gpu=False, route=0, slabs=256),
    R("wgrad", 0, 256, 255, 32, 128, 128, 3, gpu=False, route=0, slabs=128),
    # CONV_CASES of tests/test_ops_gpu.py whose comments name a route
    R("fwd", 1, 40, 72, 80, 24, 28, 3, route=1, parts=1, cot=32, bn=160),                   # 16 x 16 geometry unsplit (>= 160 tiles)
    R("dgrad", 1, 40, 72, 80, 24, 28, 3, route=1, parts=1, cot=32, relu=160),
    R("fwd", 1, 3, 72, 80, 24, 28, 3, route=0, parts=1, cot=32, bn=0),                      # 36 tiles < gmin16: the fp32 kernel
    R("fwd", 2, 3, 72, 80, 24, 28, 3, route=1, parts=1, cot=32, bn=12),                     # forced split: 5 chunks, unsplit chunk loop
    R("dgrad", 1, 16, 3, 40, 128, 128, 3, route=1, parts=1, cot=32, relu=1024),             # data gradient onto 3 channels: split kernel, 32-wide tile
    R("fwd", 1, 32, 12, 32, 128, 128, 3, gpu=False, route=1, parts=1, cot=32, bn=2048),                # 12 input channels (one zero-padded chunk)
    R("wgrad", 1, 32, 12, 32, 128, 128, 3, gpu=False, route=1, slabs=256),                             # narrow-side (12) split weight gradient
    # 1 x 1 kernels with 5 and 7 outputs (conv1x1_small.hip conv1x1_small_ok): between the streaming heads' instances (1, 2, 3, 4, 6, 8;
    # tests/_head_routes.py), so the matrix kernels run them, with slabs
    R("fwd", 0, 2, 38, 5, 16, 16, 1, route=0, parts=1, cot=32, bn=0),
    R("dgrad", 0, 2, 38, 5, 16, 16, 1, route=0, parts=1, cot=32, relu=0),
    R("wgrad", 0, 2, 38, 5, 16, 16, 1, route=0, slabs=32),
    R("fwd", 1, 2, 38, 7, 16, 16, 1, route=0, parts=1, cot=32, bn=0),
    R("dgrad", 1, 2, 38, 7, 16, 16, 1, route=0, parts=1, cot=32, relu=0),
    R("wgrad", 1, 2, 38, 7, 16, 16, 1, route=0, slabs=32),
]
