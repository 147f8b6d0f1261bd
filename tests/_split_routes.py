"""The split-storage dispatch table: the operand and epilogue forms a training step hands the split-fp16 convolution kernels
(include/uz_api.h, "split storage + folded BatchNorm backward"), each at the smallest shapes that reach the edges of its kernel
instance, with the route it claims stated only through the library's host-side queries (tests/_conv_routes.py).

  form   entry point                                  kernel option
  pk     x_packed of uz_conv_fwd_ex, dy_packed of     XF == 1 (conv_split.hip), XPK / DPK (conv_wgrad_split.hip)
         uz_conv_bwd_data_ex, x_packed / dy_packed
         of uz_conv_bwd_weight_ex
  seg    x_amax2 / seg_channels of the same calls     accumulator rescale at chunk segc and the xa_last choice; per-column inv_x
  aff    uz_conv_fwd_bn_ex                            XF == 3: the producer's BatchNorm (+ ReLU) applied while staging
  fold   bn_y / bn_save / bn_partials of              MK == 2: BatchNorm-backward reduction in the data gradient's epilogue
         uz_conv_bwd_data_ex (dy fp32 or packed)

This module imports without a GPU and without the library.  It holds
  * the host twin of split storage (split_f16.h:25-36, 68-82) in numpy: split_scale, pack_split, unpack_split.  The kernel cases
    pack their inputs with it, so no GPU producer stands between a test and the kernel, and the fp64 references are taken over the
    DECODED values (h1 + h2) / s, which a packed operand represents exactly;
  * the case table CASES with its claims;
  * structured inputs (operands) and the conditions they must meet (fold_conditions);
  * the fp64 references (evaluate), with eleven switchable defects: tests/test_split_routes_cpu.py proves that every case tells
    every defect that can apply to it apart, tests/test_split_routes_gpu.py runs the cases."""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import _conv_routes as R

CK = 16                      # channels per chunk of the contraction loop (conv_split.hip)
F16_MAX = 65504.0


# ------------------------------------------------------------------------------------------------ host twin of split storage
def _se(amax):
    e = (np.asarray(amax, dtype=np.float32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
    return np.clip(267 - e.astype(np.int64), 1, 253)


def split_scale(amax):
    """split_f16.h:25-30: the power of two s with amax * s < 2^14, from the bound's exponent field"""
    return (_se(amax).astype(np.uint32) << np.uint32(23)).view(np.float32)


def split_inv_scale(amax):
    return ((254 - _se(amax)).astype(np.uint32) << np.uint32(23)).view(np.float32)


def pack_split(v, amax):
    """split_f16.h:68-73: one uint32 per element, low half h1 = fp16(v s) (nearest even, clamped to +-65504), high half
    h2 = fp16(v s - h1).  amax broadcasts against v (a per-channel array serves two segments)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore"):
        t = np.clip(v * split_scale(amax), np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float32)
    h1 = t.astype(np.float16)
    h2 = (t - h1.astype(np.float32)).astype(np.float16)
    return h1.view(np.uint16).astype(np.uint32) | (h2.view(np.uint16).astype(np.uint32) << np.uint32(16))


def halves(words):
    w = np.asarray(words, dtype=np.uint32)
    return (w & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16), (w >> np.uint32(16)).astype(np.uint16).view(np.float16)


def unpack_split(words, amax):
    """split_f16.h:79-82: ((float)h1 + (float)h2) * 1 / s in fp32 (the sum of the halves is exact in fp32)"""
    h1, h2 = halves(words)
    return ((h1.astype(np.float32) + h2.astype(np.float32)) * split_inv_scale(amax)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", "form direction mode N Cin Cout H W xoff yoff seg ratio bn_relu opt claims")
FORMS = ("pk", "seg", "aff", "fold")
TAIL = 2                     # buffer channels behind every view


def S(form, direction, mode, N, Cin, Cout, H, W, xoff=3, yoff=1, seg=0, ratio=1.0, bn_relu=1, opt=(), **claims):
    assert form in FORMS and direction in R.DIRECTIONS and mode in (1, 2)
    return Case(form, direction, mode, N, Cin, Cout, H, W, xoff, yoff, seg, ratio, bn_relu, frozenset(opt), claims)


def case_id(c):
    s = f"{c.form}-{c.direction}-m{c.mode}-{c.N}x{c.Cin}x{c.Cout}x{c.H}x{c.W}"
    if c.seg:
        s += f"-seg{c.seg}x{c.ratio:g}"
    if c.form in ("aff", "fold"):
        s += f"-relu{c.bn_relu}"
    return s + "".join("-" + o for o in sorted(c.opt))


def route_of(c):
    return R.R(c.direction, c.mode, c.N, c.Cin, c.Cout, c.H, c.W, 3)


def queries(L, c):
    return R.queries(L, route_of(c))


def contraction(c):
    """(Kc, Mc): contraction and output channel counts of the forward / data-gradient kernels"""
    return (c.Cout, c.Cin) if c.direction == "dgrad" else (c.Cin, c.Cout)


def geometry(c):
    """tile geometry the case runs on: forward / data gradient small_geo + tile_cot, weight gradient tile_w + chan_tile"""
    if c.direction == "wgrad":
        return f"{16 if c.W == 16 else 32}px-c{32 if min(c.Cin, c.Cout) <= 32 else 64}"
    return "16x16" if c.W <= 32 else f"16x32-c{c.claims['cot']}"


def instance(c):
    """the (geometry, kernel form) instance of conv_split.hip a forward / data-gradient case enters"""
    if c.direction == "wgrad":
        return None
    if c.form == "aff":
        return geometry(c), "XF3"
    if c.form == "fold":
        return geometry(c), "MK2-XF1" if "dyp" in c.opt else "MK2"
    return geometry(c), "XF1"


def key_of(c):
    return c.mode, c.direction, c.claims["route"]


def _segs(base, segs, ratios=(64.0, 1.0 / 64.0), **kw):
    return [S("seg", *base, seg=s, ratio=r, **kw) for s in segs for r in ratios]


CASES = [
    # ---- forward with x_packed (XF == 1), one case per tile geometry, each with the fused BatchNorm partials
    S("pk", "fwd", 2, 2, 33, 33, 17, 18, opt=("bnpart",), route=1, parts=1, cot=32, bn=8),          # 16 x 16 tiles: K tail 1, overhang 1, ragged tile, W % 4 != 0
    S("pk", "fwd", 2, 2, 20, 40, 15, 33, opt=("bnpart",), route=1, parts=1, cot=32, bn=8),          # 16 x 32 tiles, 32 channels: H < 16, one-column ragged tile
    S("pk", "fwd", 2, 2, 48, 65, 16, 36, opt=("bnpart",), route=1, parts=1, cot=64, bn=8),          # 16 x 32 tiles, 64 channels: the second tile overhangs by 1
    # ---- two segments, forward, on an unsplit loop: the first chunk boundary, a mid one, the last one below Kc (a K-tail chunk holds the second segment)
    *_segs(("fwd", 2, 2, 72, 40, 16, 36), (16, 32, 64), route=1, parts=1, cot=64, bn=8),
    *_segs(("fwd", 2, 2, 40, 33, 17, 18), (32,), route=1, parts=1, cot=32, bn=8),
    *_segs(("fwd", 2, 2, 72, 20, 15, 33), (16,), route=1, parts=1, cot=32, bn=8),
    # ... under split-K: parts 2 (3 chunks each): on the part boundary, inside part 0, inside part 1; parts 4: on a boundary, inside part 1
    *_segs(("fwd", 1, 20, 96, 32, 16, 32), (48, 16, 64), route=1, parts=2, cot=32, bn=0),
    *_segs(("fwd", 1, 20, 192, 32, 16, 32), (48, 80), route=1, parts=4, cot=32, bn=0),
    # ---- uz_conv_fwd_bn_ex (XF == 3): three geometries x bn_relu
    S("aff", "fwd", 2, 2, 33, 33, 17, 18, bn_relu=1, route=1, parts=1, cot=32, bn=8),
    S("aff", "fwd", 2, 2, 33, 33, 17, 18, bn_relu=0, opt=("bnpart",), route=1, parts=1, cot=32, bn=8),
    S("aff", "fwd", 2, 2, 20, 40, 15, 33, bn_relu=1, opt=("bnpart",), route=1, parts=1, cot=32, bn=8),
    S("aff", "fwd", 2, 2, 20, 40, 15, 33, bn_relu=0, route=1, parts=1, cot=32, bn=8),
    S("aff", "fwd", 2, 2, 48, 65, 16, 36, bn_relu=1, route=1, parts=1, cot=64, bn=8),
    S("aff", "fwd", 2, 2, 48, 65, 16, 36, bn_relu=0, route=1, parts=1, cot=64, bn=8),
    # ---- dy_packed alone in the data gradient (overwrite and accumulate), per geometry
    S("pk", "dgrad", 2, 2, 33, 33, 17, 18, route=1, parts=1, cot=32, relu=8),
    S("pk", "dgrad", 2, 2, 40, 20, 15, 33, route=1, parts=1, cot=32, relu=8),
    S("pk", "dgrad", 2, 2, 65, 48, 16, 36, route=1, parts=1, cot=64, relu=8),
    # ---- the folded BatchNorm-backward reduction (MK == 2): vector epilogue (aligned, W % 4 == 0), scalar epilogue from W % 4 != 0, and
    # scalar epilogue from misalignment alone (W % 4 == 0 makes every channel offset 16-byte aligned, so the dx / bn_y view itself starts
    # 4 bytes off a 16-byte boundary: opt "mis-dx" / "mis-y")
    S("fold", "dgrad", 2, 2, 33, 33, 17, 20, xoff=4, yoff=4, bn_relu=1, opt=("dyp",), route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 33, 33, 17, 18, bn_relu=0, route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 33, 33, 17, 20, bn_relu=1, opt=("mis-dx",), route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 40, 20, 15, 36, xoff=4, yoff=4, bn_relu=0, route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 40, 20, 15, 33, bn_relu=1, opt=("dyp",), route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 40, 20, 15, 36, bn_relu=1, opt=("mis-y",), route=1, parts=1, cot=32, relu=8),
    S("fold", "dgrad", 2, 2, 65, 48, 16, 36, xoff=4, yoff=4, bn_relu=1, route=1, parts=1, cot=64, relu=8),
    S("fold", "dgrad", 2, 2, 65, 48, 16, 35, bn_relu=1, opt=("dyp",), route=1, parts=1, cot=64, relu=8),
    S("fold", "dgrad", 2, 2, 65, 48, 16, 36, bn_relu=0, opt=("dyp", "mis-dx"), route=1, parts=1, cot=64, relu=8),
    # ---- uz_conv_bwd_weight_ex: the four tile forms of launch_wgrad x {x_packed, dy_packed, both}; pixel counts at or above the smallest
    # case of the same key in tests/_conv_routes.py (2 048 px in mode 1, 32 768 px in mode 2)
    S("pk", "wgrad", 1, 8, 64, 64, 16, 16, opt=("xp", "slabs"), route=1, slabs=16),                  # 16 px wide, 64-channel tile; slabs_out + table
    S("pk", "wgrad", 1, 8, 64, 96, 18, 32, opt=("dp",), route=1, slabs=40),                          # 32 px wide, 64-channel tile, ragged H
    S("pk", "wgrad", 2, 32, 32, 64, 32, 32, opt=("xp", "dp"), route=1, slabs=85),                    # 32 px wide, 32-channel tile (chan_tile 32)
    S("pk", "wgrad", 2, 32, 33, 64, 32, 32, opt=("xp",), route=1, slabs=128),                        # chan_tile 33: 64-channel tile, Cin overhangs by 1
    S("pk", "wgrad", 2, 120, 32, 40, 18, 16, opt=("xp", "dp"), route=1, slabs=108),                  # 16 px wide, 32-channel tile, ragged H
    # ... two segments: seg_channels inside a 32-column tile (16, 48) and on a tile boundary (32)
    *_segs(("wgrad", 1, 8, 80, 64, 17, 16), (16, 48), opt=("xp",), route=1, slabs=24),
    *_segs(("wgrad", 1, 8, 80, 64, 17, 16), (32,), ratios=(64.0,), opt=("xp", "dp"), route=1, slabs=24),
]


# ------------------------------------------------------------------------------------------------ structured inputs
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def act(shape, seed, nonneg):
    """tests/test_conv_routes_gpu.py's structure: a block of rows offset by +3, one channel at 2^-12, post-ReLU in every other case"""
    t = rnd(*shape, seed=seed)
    H = shape[2]
    r0 = H // 4
    t[:, :, r0:r0 + max(1, H // 4)] += 3.0
    if shape[1] > 1:
        t[:, 1] *= 2.0 ** -12
    return torch.relu(t) if nonneg else t


class Packed:
    """An fp32 NCHW tensor in split storage: words (uint32 bits in a float32 tensor), the per-channel bounds, the decoded values
    (h1 + h2) / s in fp64 and the two pieces h1 / s, h2 / s."""

    def __init__(self, t, amax, seg=0, amax2=None):
        C = t.shape[1]
        self.amax, self.amax2, self.seg = np.float32(amax), (None if amax2 is None else np.float32(amax2)), seg
        per = np.full((1, C, 1, 1), self.amax, dtype=np.float32)
        if seg:
            per[:, seg:] = self.amax2
        self.per = per
        w = pack_split(t.numpy(), per)
        self.words = torch.from_numpy(w.view(np.float32).copy())
        h1, h2 = halves(w)
        inv = split_inv_scale(per).astype(np.float64)
        self.p1 = torch.from_numpy(h1.astype(np.float64) * inv)
        self.p2 = torch.from_numpy(h2.astype(np.float64) * inv)
        self.dec = self.p1 + self.p2
        self.dec32 = torch.from_numpy(unpack_split(w, per))


def pieces(t, amax=None):
    """the two pieces a kernel forms of an fp32 operand it splits itself (split_f16.h split2), scaled from the tensor's maximum"""
    p = Packed(t.reshape(1, 1, 1, -1), float(t.abs().max()) if amax is None else amax)
    return p.p1.reshape(t.shape), p.p2.reshape(t.shape)


def bounds(x, seg, ratio):
    """(amax, amax2): one bound, or two bounds exactly `ratio` apart that cover their segments"""
    if not seg:
        return float(x.abs().max()), None
    b = np.float32(max(float(x[:, :seg].abs().max()), float(x[:, seg:].abs().max()) / ratio))
    return float(b), float(np.float32(b * np.float32(ratio)))


Ops = collections.namedtuple("Ops", "a apk b w bias extra")


def operands(case, idx):
    """Every operand of case number idx as CPU tensors.  a: the streamed input (x, dy; for aff the producer's y_prev), apk its Packed
    form or None; b: the second streamed operand of a weight gradient (dy), extra['bpk'] its Packed form; w, bias: the parameter."""
    c = case
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    nonneg = idx % 2 == 1
    extra = {}
    if c.direction == "wgrad":
        x = act((N, Cin, H, W), 700 + idx, nonneg)
        if c.seg:
            x[:, c.seg:] *= c.ratio
        dy = rnd(N, Cout, H, W, seed=800 + idx)
        dy[:, Cout - 1] *= 2.0 ** -12
        a1, a2 = bounds(x, c.seg, c.ratio)
        apk = Packed(x, a1, c.seg, a2) if "xp" in c.opt else None
        extra["bpk"] = Packed(dy, float(dy.abs().max())) if "dp" in c.opt else None
        return Ops(x, apk, dy, None, None, extra)
    if c.direction == "fwd":
        w = rnd(Cout, Cin, 3, 3, seed=200 + idx, scale=1.0 / math.sqrt(Cin * 9))
        w[0] -= w[0].mean()
        bias = rnd(Cout, seed=300 + idx)
        if c.form == "aff":
            y = rnd(N, Cin, H, W, seed=100 + idx) * 1.5 + 0.3
            y[:, :, H // 4:H // 4 + max(1, H // 4)] += 1.0
            extra["save"] = bn_table(Cin, 900 + idx, y, big_beta=True)
            a = aff_apply(y, extra["save"], c.bn_relu)
            extra["a_amax"] = float(np.nextafter(np.float32(a.abs().max()), np.float32(np.inf)))
            return Ops(y, None, None, w, bias, extra)
        x = act((N, Cin, H, W), 100 + idx, nonneg)
        if c.seg:
            x[:, c.seg:] *= c.ratio
        a1, a2 = bounds(x, c.seg, c.ratio)
        return Ops(x, Packed(x, a1, c.seg, a2), None, w, bias, extra)
    dy = act((N, Cout, H, W), 400 + idx, nonneg)
    w = rnd(Cout, Cin, 3, 3, seed=500 + idx, scale=1.0 / math.sqrt(Cout * 9))
    w[:, 0] -= w[:, 0].mean()
    apk = Packed(dy, float(dy.abs().max())) if (c.form == "pk" or "dyp" in c.opt) else None
    if c.form == "fold":
        y = rnd(N, Cin, H, W, seed=600 + idx) * 1.5 + 0.3
        extra["y"] = y
        extra["save"] = bn_table(Cin, 900 + idx, y, big_beta=False)
    else:
        extra["prev"] = rnd(N, Cin, H, W, seed=600 + idx)
    return Ops(dy, apk, None, w, None, extra)


def bn_table(C, seed, y, big_beta):
    """[4][C] fp32: mean, rstd, alpha = gamma rstd, beta' = beta - mean alpha (uz_bn_relu_fwd_ex's table).  Channel 0 has a negative
    alpha; with big_beta channel 2 has a large positive beta' (padding that did not stay zero would show)."""
    mean = (y.mean((0, 2, 3)) + rnd(C, seed=seed) * 0.1).float()
    rstd = (0.7 + rnd(C, seed=seed + 1).abs()).float()
    gamma = (0.8 + rnd(C, seed=seed + 2).abs()).float()
    gamma[0] = -gamma[0]
    beta = (rnd(C, seed=seed + 3) * 0.1).float()
    if big_beta and C > 2:
        beta[2] = 6.0
    alpha = (gamma * rstd).float()
    betap = (beta - mean * alpha).float()
    return torch.cat([mean, rstd, alpha, betap]).contiguous()


def _tab(save, C):
    return [save[i * C:(i + 1) * C].double()[None, :, None, None] for i in range(4)]


def aff_apply(y, save, relu):
    """a = max(alpha y + beta', 0) (or no max) in fp64 from the fp32 table values"""
    _, _, al, be = _tab(save, y.shape[1])
    a = y.double() * al + be
    return torch.relu(a) if relu else a


def fold_conditions(case, ops):
    """(worst margin |alpha y + beta'| / (|alpha y| + |beta'|) over every element, smallest per-channel share of elements on either
    side of zero) of a fold case: the margin must be >= 2^-20 (the fp32 fmaf's sign is then the fp64 sign), the share >= 1 / 4"""
    y = ops.extra["y"].double()
    _, _, al, be = _tab(ops.extra["save"], case.Cin)
    t = y * al + be
    margin = float((t.abs() / ((y * al).abs() + be.abs())).min())
    pos = (t > 0).double().mean((0, 2, 3))
    return margin, float(torch.minimum(pos, 1 - pos).min())


# ------------------------------------------------------------------------------------------------ fp64 references and their defects
DEFECTS = {
    1: "the second segment decoded with the first bound",
    2: "the segment switch one chunk late",
    3: "the segment switch one chunk early",
    4: "accumulators not rescaled at the switch",
    5: "the two halves of a word swapped",
    6: "the ReLU mask taken from y > 0",
    7: "x_hat without rstd",
    8: "the staged BatchNorm applied to the zero padding",
    9: "bn_y / y_prev addressed with Cin instead of its Ctot",
    10: "the last K-tail chunk read past Kc",
    11: "a partial row of one tile missing from the sums",
}


def applies(case, n):
    """whether defect n can occur in the code the case runs"""
    c = case
    Kc, _ = contraction(c)
    packed = c.form in ("pk", "seg") or "dyp" in c.opt
    if n in (1, 2, 3):
        return c.seg > 0
    if n == 4:                                        # forward only, and only where the switch falls inside a part's chunk loop
        if not (c.seg > 0 and c.direction == "fwd"):
            return False
        cps = -(-(-(-Kc // CK)) // c.claims["parts"])
        return (c.seg // CK) % cps != 0
    if n == 5:
        return packed
    if n == 6:
        return c.form == "fold" and c.bn_relu == 1
    if n == 7:
        return c.form == "fold"
    if n == 8:
        return c.form == "aff"
    if n == 9:
        return c.form in ("aff", "fold") and c.N > 1
    if n == 10:
        return c.direction != "wgrad" and Kc % CK != 0
    if n == 11:
        return c.form == "fold" or "bnpart" in c.opt
    raise KeyError(n)


def canary_buffer(t, lead, tail=TAIL):
    """t as channels [lead, lead + C) of a wider NaN-filled buffer (what the GPU tier hands the kernels)"""
    n, ch, h, w = t.shape
    buf = torch.full((n, lead + ch + tail, h, w), float("nan"), dtype=t.dtype)
    buf[:, lead:lead + ch] = t
    return buf


def _wrong_ctot(t, lead):
    """the view read with the VIEW's channel count as its image stride"""
    n, ch, h, w = t.shape
    buf = canary_buffer(t, lead)
    return torch.as_strided(buf.reshape(-1), (n, ch, h, w), (ch * h * w, h * w, w, 1), lead * h * w).clone()


def _scale_channels(x, lo, hi, f):
    x = x.clone()
    x[:, max(lo, 0):hi] *= f
    return x


def _seg_defect(case, x, n, s1, s2):
    """defects 1-4 are all a channel range of the streamed operand carrying the wrong power of two"""
    seg, (Kc, _) = case.seg, contraction(case)
    if n == 1:
        return _scale_channels(x, seg, Kc, s2 / s1)
    if n == 2:
        return _scale_channels(x, seg, seg + CK, s2 / s1)
    if n == 3:
        return _scale_channels(x, seg - CK, seg, s1 / s2)
    cps = -(-(-(-Kc // CK)) // case.claims["parts"])
    return _scale_channels(x, (seg // CK) // cps * cps * CK, seg, s1 / s2)


def _last_tile_mask(case):
    """pixels of the last tile of the last image (the ragged bottom-right tile)"""
    tw = 16 if case.W <= 32 else 32
    m = torch.zeros(case.N, 1, case.H, case.W, dtype=torch.bool)
    m[-1, :, (case.H - 1) // 16 * 16:, (case.W - 1) // tw * tw:] = True
    return m


def _conv(direction, a, w):
    return F.conv2d(a, w, None, padding=1) if direction == "fwd" else F.conv_transpose2d(a, w, None, padding=1)


def _wgrad(x, dy, wshape):
    return torch.nn.grad.conv2d_weight(x, wshape, dy, padding=1)


Q = collections.namedtuple("Q", "ref den floor kind")      # kind: "gate" elementwise ratio, "sum" BN_SUM relative to den, "exact" bit for bit


def evaluate(case, ops, defect=0):
    """fp64 expectation of every gated quantity of the case -> {name: Q}; defect n > 0 evaluates the defective twin instead"""
    c, n = case, defect
    assert n == 0 or applies(c, n), (case_id(c), n)
    Kc, Mc = contraction(c)
    if c.direction == "wgrad":
        return _eval_wgrad(c, ops, n)
    w64 = ops.w.double()
    out = {}
    if c.form == "aff":
        y = ops.a if n != 9 else _wrong_ctot(ops.a, c.xoff)
        a = aff_apply(y, ops.extra["save"], c.bn_relu)
        true_a = aff_apply(ops.a, ops.extra["save"], c.bn_relu)
        if n == 8:
            _, _, al, be = _tab(ops.extra["save"], c.Cin)
            border = (torch.relu(be) if c.bn_relu else be).expand(c.N, c.Cin, c.H + 2, c.W + 2).clone()
            border[:, :, 1:-1, 1:-1] = a
            conv = F.conv2d(border, w64, None, padding=0)
        else:
            conv = _conv("fwd", a, w64)
        amag, src = true_a.abs(), true_a
    else:
        src = ops.apk.dec if ops.apk is not None else ops.a.double()
        a = src
        if n in (1, 2, 3, 4):
            a = _seg_defect(c, src, n, float(split_scale(ops.apk.amax)), float(split_scale(ops.apk.amax2)))
        conv = _conv(c.direction, a, w64)
        if n == 5:                                   # kept a2 b1 + a2 b2 + a1 b1 instead of a1 b1 + a1 b2 + a2 b1: off by (a1 - a2) b2
            conv = conv - _conv(c.direction, ops.apk.p1 - ops.apk.p2, pieces(ops.w)[1])
        amag = src.abs()
    if n == 10:                                      # the neighbouring buffer channel (a NaN canary) enters with a zero weight
        leak = torch.full((c.N, 1, c.H, c.W), float("nan"), dtype=torch.float64)
        wz = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
        conv = conv + (F.conv2d(leak, wz.expand(Mc, 1, 3, 3), None, padding=1) if c.direction == "fwd" else F.conv_transpose2d(leak, wz.expand(1, Mc, 3, 3), None, padding=1))
    den = _conv(c.direction, amag, w64.abs())
    floor = 2.0 ** -39 * float(amag.max()) * float(ops.w.abs().max()) * Kc * 9
    if c.direction == "fwd":
        b = ops.bias.double()[None, :, None, None]
        out["y"] = Q(conv + b, den + b.abs(), floor, "gate")
        out["conv"] = Q(conv, den, floor, "gate")
        if "bnpart" in c.opt:                        # statistics of the stored y (the GPU tier sums the stored tensor; here the expected one)
            yv = conv + b
            keep = ~_last_tile_mask(c) if n == 11 else torch.ones(1, 1, 1, 1, dtype=torch.bool)
            out["bn_s1"] = Q((yv * keep).sum((0, 2, 3)), yv.abs().sum((0, 2, 3)), 0.0, "sum")
            out["bn_s2"] = Q((yv * yv * keep).sum((0, 2, 3)), (yv * yv).sum((0, 2, 3)), 0.0, "sum")
        return out
    if c.form != "fold":
        prev = ops.extra["prev"].double()
        out["dx"] = Q(conv, den, floor, "gate")
        out["dx_acc"] = Q(conv + prev, den + prev.abs(), floor, "gate")
        return out
    y32 = ops.extra["y"] if n != 9 else _wrong_ctot(ops.extra["y"], c.yoff)
    y = y32.double()
    mean, rstd, al, be = _tab(ops.extra["save"], c.Cin)
    if c.bn_relu:
        mask = (y > 0) if n == 6 else (y * al + be > 0)
    else:
        mask = torch.ones_like(y, dtype=torch.bool)
    dz = conv * mask
    xh = (y - mean) if n == 7 else (y - mean) * rstd
    keep = ~_last_tile_mask(c) if n == 11 else torch.ones(1, 1, 1, 1, dtype=torch.bool)
    out["dz"] = Q(dz, den, floor, "gate")
    out["mask"] = Q(mask.double(), torch.ones_like(y), 0.0, "exact")
    out["sum_dz"] = Q((dz * keep).sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), 0.0, "sum")
    out["sum_dzx"] = Q((dz * xh * keep).sum((0, 2, 3)), (dz * xh).abs().sum((0, 2, 3)), 0.0, "sum")
    s = ops.extra["save"]
    xh32 = (y32 - s[:c.Cin][None, :, None, None]) * (1.0 if n == 7 else s[c.Cin:2 * c.Cin][None, :, None, None])      # two fp32 operations
    out["max_xhat"] = Q(xh32.abs().amax((0, 2, 3)).double(), None, 0.0, "exact")
    return out


def _eval_wgrad(c, ops, n):
    wshape = (c.Cout, c.Cin, 3, 3)
    xpk, dpk = ops.apk, ops.extra["bpk"]
    x = xpk.dec if xpk is not None else ops.a.double()
    dy = dpk.dec if dpk is not None else ops.b.double()
    xd = x
    if n in (1, 2, 3):
        xd = _seg_defect(c, x, n, float(split_scale(xpk.amax)), float(split_scale(xpk.amax2)))
    ref = _wgrad(xd, dy, wshape)
    if n == 5:
        if xpk is not None:
            d2 = dpk.p2 if dpk is not None else pieces(ops.b)[1]
            ref = ref - _wgrad(xpk.p1 - xpk.p2, d2, wshape)
        else:
            ref = ref - _wgrad(pieces(ops.a)[1], dpk.p1 - dpk.p2, wshape)
    den = _wgrad(x.abs(), dy.abs(), wshape)
    floor = 2.0 ** -39 * float(x.abs().max()) * float(dy.abs().max()) * c.N * c.H * c.W
    return {"dw": Q(ref, den, floor, "gate")}


def moved(true, bad, gate, bn_sum, factor=10.0):
    """worst factor by which a defective evaluation leaves the bound of any gated quantity (inf where it is not finite)"""
    worst = 0.0
    for k, t in true.items():
        b = bad[k]
        diff = (b.ref - t.ref).abs()
        if not bool(torch.isfinite(diff).all()):
            return float("inf")
        if t.kind == "exact":
            worst = max(worst, float("inf") if bool((diff > 0).any()) else 0.0)
        else:
            g = gate if t.kind == "gate" else bn_sum
            worst = max(worst, float((diff / (factor * g * (t.den + t.floor)).clamp_min(1e-300)).max()))
    return worst
