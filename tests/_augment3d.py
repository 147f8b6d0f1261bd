"""numpy restatement of csrc/augment3d.hip's stage rules (include/uz_api.h) and the case set of
tests/test_augment3d_cpu.py / tests/test_augment3d_gpu.py - TEST INFRASTRUCTURE.

The rules restate OpenCV as the reference calls it from data/BratsProcessing/augmentation.py:12-104 (utils.rotate_image with
BORDER_REPLICATE, utils.resize_image, utils.dense_image_warp with convertMaps(CV_16SC2) and BORDER_REFLECT); oracle/augment.py says
why parity with cv2 itself is unpinned, and its linear resize rule is imported, not repeated.  A volume is [X][Y][Z][C]; all in-plane
geometry acts on the plane [X][Y] (rows = X, columns = Y) identically for every z and channel, so every index / weight / margin
array below is (X, Y).

`dtype` is the type of the rotation and resize coordinates, of every weight and of every blend: float32 is the kernel's arithmetic
(the kernel is compiled without contraction, so the same expression rounds the same way), float64 the yardstick.  Three things do
not follow `dtype`, because they do not in the kernel either: the elastic field is ALWAYS evaluated in float64, the maps are ALWAYS
cast to float32 (deformation_to_transformation does) and quantised from there, and the INTER_NEAREST index of the scale stage is
decided in float64.

With float64 `augment3d` also returns two (Xc, Yc, Zc) MARGINS, propagated through later stages by the min over the voxels a
result reads (oracle/augment.py does the same):
  labels  rotate: distance of each floor(s + 0.5) argument from an integer, in pixels; elastic: distance of each rint(map) argument
          from k + 0.5, in pixels, and of the float64 map from the nearest float32 rounding boundary, in float32 ulps;
  images  elastic: distance of each rint(32 map) argument from k + 0.5, in its own unit (1/32 pixel), and the same rounding-boundary
          distance.  The bilinear stages are continuous in their coordinates and contribute nothing.
A voxel whose margin is below MARGIN is excluded from a comparison; two rounded coordinates give an expected share of 4e-4 per rule,
EXCLUDED_CAP is what a case may lose.

`defects` names deliberate mistakes; DEFECTS lists them.  tests/test_augment3d_cpu.py shows that each one changes the expected
output of at least one case outside the excluded voxels."""
import dataclasses
import functools

import numpy as np

from oracle import augment as OA

NPRM = 34                      # UZ_AUG3_NPRM
MARGIN = 1e-4
EXCLUDED_CAP = 0.01
DEFECTS = dict(centre="X and Y swapped in the rotation centre", constant="constant 0 instead of replicate border in the rotation",
               reflect101="BORDER_REFLECT_101 instead of BORDER_REFLECT", single_reflect="one reflection only, then clamped",
               half_up="round half up instead of half to even", pad_unrotated="pad value taken from the volume before the rotation",
               crop_first="crop before flip", nearest="the nearest rules of rotate and scale exchanged",
               shift_all="intensity shift on all C channels")


# ------------------------------------------------------------------------------------------------ parameter table
def make_prm(shape, angle=None, scale=None, dx=None, dy=None, shift=None, flips=0, origin=(0, 0, 0)):
    """The UZ_AUG3_NPRM table from what the reference draws: angle in degrees, the scale factor, the two 3 x 3 matrices (9 values
    each), four shifts, the flip mask and the crop origin.  None = stage off."""
    X, Y, _ = shape
    p = np.zeros(NPRM, np.float64)
    p[1] = 1.0
    if angle is not None:
        p[0], p[1], p[2] = 1.0, np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    if scale is not None:
        p[3], p[4], p[5] = 1.0, round(X * scale), round(Y * scale)
    if dx is not None:
        p[6], p[7:16], p[16:25] = 1.0, np.asarray(dx, np.float64).reshape(9), np.asarray(dy, np.float64).reshape(9)
    if shift is not None:
        p[25], p[26:30] = 1.0, shift
    p[30] = flips
    p[31:34] = origin
    return p


# ------------------------------------------------------------------------------------------------ stage rules
def _blend(a, I0, I1, J0, J1, FI, FJ, T, m=None):
    """(1 - fi) ((1 - fj) v00 + fj v01) + fi ((1 - fj) v10 + fj v11) over the planes of a [X][Y][Z][C] volume; m: per-tap 0 / 1 masks"""
    fi, fj = FI.astype(T)[..., None, None], FJ.astype(T)[..., None, None]
    v = [a[I0, J0], a[I0, J1], a[I1, J0], a[I1, J1]]
    if m is not None:
        v = [t * k[..., None, None].astype(T) for t, k in zip(v, m)]
    one = T(1)
    return ((one - fi) * ((one - fj) * v[0] + fj * v[1]) + fi * ((one - fj) * v[2] + fj * v[3])).astype(T)


def _rotate(img, lbl, c, s, T, defects):
    X, Y = img.shape[:2]
    ii, jj = np.mgrid[0:X, 0:Y].astype(T)
    cx, cy = (T(X * 0.5), T(Y * 0.5)) if "centre" in defects else (T(Y * 0.5), T(X * 0.5))
    dx, dy = jj - cx, ii - cy
    sx, sy = T(c) * dx - T(s) * dy + cx, T(s) * dx + T(c) * dy + cy
    x0, y0 = np.floor(sx), np.floor(sy)
    FJ, FI = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    cl = lambda v, n: np.clip(v, 0, n - 1)
    inside = lambda v, n: (v >= 0) & (v < n)
    m = None
    if "constant" in defects:
        m = [inside(y0, X) & inside(x0, Y), inside(y0, X) & inside(x0 + 1, Y), inside(y0 + 1, X) & inside(x0, Y), inside(y0 + 1, X) & inside(x0 + 1, Y)]
    out = _blend(img, cl(y0, X), cl(y0 + 1, X), cl(x0, Y), cl(x0 + 1, Y), FI, FJ, T, m)
    if lbl is None:
        return out, None, None
    half = T(0) if "nearest" in defects else T(0.5)
    ax, ay = sx + half, sy + half
    lj, li = np.floor(ax).astype(np.int64), np.floor(ay).astype(np.int64)
    lo = lbl[cl(li, X), cl(lj, Y)]
    if "constant" in defects:
        lo = np.where((inside(li, X) & inside(lj, Y))[..., None], lo, 0)
    margin = np.minimum(np.abs(ax - np.rint(ax)), np.abs(ay - np.rint(ay))).astype(np.float64)
    return out, lo, margin


def _scale_axis(n, s, taps, T, defects):
    """One axis of resize + padToSize / cropToSize: per index of the n-wide result (t0, t1, w, l, fill)."""
    t0s, t1s, ws = taps
    o = np.arange(n)
    u = o - (n - s) // 2 if s < n else o + (s - n) // 2
    fill = (u < 0) | (u >= s)
    uc = np.clip(u, 0, s - 1)
    arg = uc.astype(np.float64) * (np.float64(n) / np.float64(s))
    if "nearest" in defects:
        arg = arg + 0.5
    l = np.minimum(np.floor(arg).astype(np.int64), n - 1)
    return t0s[uc], t1s[uc], np.where(fill, T(0), ws[uc]).astype(T), l, fill


def _scale(img, lbl, lm, sX, sY, T, defects, pad_from):
    X, Y = img.shape[:2]
    y0, y1, x0, x1, wy, wx = OA._resize_taps(X, Y, (sX, sY), T)               # rows X -> sX, columns Y -> sY
    i0, i1, fi, li, fill_i = _scale_axis(X, sX, (y0, y1, wy), T, defects)
    j0, j1, fj, lj, fill_j = _scale_axis(Y, sY, (x0, x1, wx), T, defects)
    B = lambda a, b: np.broadcast_arrays(a[:, None], b[None, :])
    (I0, J0), (I1, J1), (FI, FJ), (LI, LJ) = B(i0, j0), B(i1, j1), B(fi, fj), B(li, lj)
    fill = fill_i[:, None] | fill_j[None, :]
    out = _blend(img, I0, I1, J0, J1, FI, FJ, T)
    out[fill] = pad_from[0, 0, 0, :].astype(T)
    if lbl is None:
        return out, None, None
    lo = lbl[LI, LJ]
    lo[fill] = 0
    return out, lo, np.where(fill, np.inf, lm[LI, LJ])


def cubic_field(X, Y, d):
    """resize(3 x 3 -> X x Y, INTER_CUBIC) in float64: coordinate (o + 0.5) 3/N - 0.5, taps floor - 1 .. floor + 2 clamped to 0..2,
    A = -0.75.  Every product and sum is written out in the order csrc/augment3d.hip evaluates it: the result is bit-equal."""
    m = np.asarray(d, np.float64).reshape(3, 3)

    def axis(N):
        c = (np.arange(N, dtype=np.float64) + 0.5) * (3.0 / np.float64(N)) - 0.5
        f = np.floor(c)
        x = c - f
        w0 = ((-0.75 * (x + 1.0) + 3.75) * (x + 1.0) - 6.0) * (x + 1.0) + 3.0
        w1 = ((1.25 * x - 2.25) * x) * x + 1.0
        w2 = ((1.25 * (1.0 - x) - 2.25) * (1.0 - x)) * (1.0 - x) + 1.0
        w3 = 1.0 - w0 - w1 - w2
        t = [np.clip(f.astype(np.int64) + k, 0, 2) for k in (-1, 0, 1, 2)]
        return [w0, w1, w2, w3], t
    wi, ti = axis(X)
    wj, tj = axis(Y)
    h = [((wj[0] * m[r][tj[0]] + wj[1] * m[r][tj[1]]) + wj[2] * m[r][tj[2]]) + wj[3] * m[r][tj[3]] for r in range(3)]       # (Y,) each
    h = np.stack(h)                                                                                                         # (3, Y)
    W = [w[:, None] for w in wi]
    return ((W[0] * h[ti[0]] + W[1] * h[ti[1]]) + W[2] * h[ti[2]]) + W[3] * h[ti[3]]                                         # (X, Y)


def elastic_maps(X, Y, dx, dy):
    """(map_x, map_y) float32 as deformation_to_transformation makes them, and the float64 values they were cast from."""
    ii, jj = np.mgrid[0:X, 0:Y].astype(np.float64)
    mx64, my64 = jj + cubic_field(X, Y, dx), ii + cubic_field(X, Y, dy)
    return mx64.astype(np.float32), my64.astype(np.float32), mx64, my64


def _reflect(v, n, defects):
    if "reflect101" in defects:
        if n == 1:
            return np.zeros_like(v)
        m = np.mod(v, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    if "single_reflect" in defects:
        return np.clip(np.where(v < 0, -1 - v, np.where(v >= n, 2 * n - 1 - v, v)), 0, n - 1)
    m = np.mod(v, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _rint(a, defects):
    return (np.floor(a + a.dtype.type(0.5)) if "half_up" in defects else np.rint(a)).astype(np.int64)


def quantised_maps(mx, my, defects=()):
    """convertMaps(CV_16SC2): q = rint(32 map) in float32 (32 map is exact)"""
    return _rint(mx * np.float32(32), defects), _rint(my * np.float32(32), defects)


def _boundary_ulps(v64, v32):
    """distance of a float64 value from the nearest float32 rounding boundary, in float32 ulps (0.5 = exactly representable)"""
    ulp = np.spacing(np.abs(v32)).astype(np.float64)
    return 0.5 - np.abs(v64 - v32.astype(np.float64)) / ulp


def _elastic(img, lbl, lm, dx, dy, T, defects):
    X, Y = img.shape[:2]
    mx, my, mx64, my64 = elastic_maps(X, Y, dx, dy)
    qx, qy = quantised_maps(mx, my, defects)
    J0, J1, FJ = _reflect(qx >> 5, Y, defects), _reflect((qx >> 5) + 1, Y, defects), (qx & 31).astype(T) * T(0.03125)
    I0, I1, FI = _reflect(qy >> 5, X, defects), _reflect((qy >> 5) + 1, X, defects), (qy & 31).astype(T) * T(0.03125)
    out = _blend(img, I0, I1, J0, J1, FI, FJ, T)
    tie = lambda a: np.abs(np.abs(a - np.floor(a)) - 0.5)
    bound = np.minimum(_boundary_ulps(mx64, mx), _boundary_ulps(my64, my))
    ax, ay = mx.astype(np.float64) * 32, my.astype(np.float64) * 32
    im = np.minimum(np.minimum(tie(ax), tie(ay)), bound)
    if lbl is None:
        return out, None, None, im
    LJ, LI = _reflect(_rint(mx, defects), Y, defects), _reflect(_rint(my, defects), X, defects)
    own = np.minimum(np.minimum(tie(mx.astype(np.float64)), tie(my.astype(np.float64))), bound)
    return out, lbl[LI, LJ], np.minimum(own, lm[LI, LJ]), im


def eval_maps(y_raw):
    """_toEvaluationOneHot (bratsDataset.py:125-131) as (3, ...) float32"""
    return np.stack([y_raw != 0, (y_raw != 0) & (y_raw != 2), y_raw == 4]).astype(np.float32)


def augment3d(img, lbl, prm, crop=None, dtype=np.float32, defects=()):
    """One volume img [X][Y][Z][C] / lbl [X][Y][Z] (or None) through the stages with the parameter table `prm`; crop = (Xc, Yc, Zc).
    Returns (x (C, Xc, Yc, Zc), y_raw (Xc, Yc, Zc) or None); with dtype=np.float64 also (label margin, image margin)."""
    T = dtype
    X, Y, Z, C = img.shape
    orig = img
    img = img.astype(T)
    lbl = None if lbl is None else lbl.astype(np.int64)
    lm, im = np.full((X, Y), np.inf), np.full((X, Y), np.inf)
    if prm[0]:
        img, lbl, m = _rotate(img, lbl, prm[1], prm[2], T, defects)
        lm = lm if m is None else m
    if prm[3]:
        img, lbl, m = _scale(img, lbl, lm, int(prm[4]), int(prm[5]), T, defects, orig if "pad_unrotated" in defects else img)
        lm = lm if m is None else m
    if prm[6]:
        img, lbl, m, im = _elastic(img, lbl, lm, prm[7:16], prm[16:25], T, defects)
        lm = lm if m is None else m
    if prm[25]:
        if C < 4:
            raise IndexError("the intensity shift acts on channels 0..3")
        img = img.copy()
        for c in range(C if "shift_all" in defects else 4):
            img[..., c] = img[..., c] + T(np.float32(prm[26 + c % 4]))
    lm3, im3 = (np.broadcast_to(a[:, :, None], (X, Y, Z)) for a in (lm, im))
    ox, oy, oz = (int(v) for v in prm[31:34])
    Xc, Yc, Zc = crop if crop is not None else (X, Y, Z)
    cut = lambda a: a[ox:ox + Xc, oy:oy + Yc, oz:oz + Zc]

    def flip(a):
        for ax in range(3):
            if int(prm[30]) >> ax & 1:
                a = np.flip(a, axis=ax)
        return a
    if "crop_first" in defects:
        fin = lambda a: flip(cut(a))
    else:
        fin = lambda a: cut(flip(a))
    x = np.ascontiguousarray(np.transpose(fin(img), (3, 0, 1, 2)))
    y = None if lbl is None else np.ascontiguousarray(fin(lbl)).astype(np.uint8)
    if T is np.float64:
        return x, y, np.ascontiguousarray(fin(lm3)), np.ascontiguousarray(fin(im3))
    return x, y


# ------------------------------------------------------------------------------------------------ cases
A_, B_, S_ = (16, 24, 8), (24, 16, 5), (8, 8, 4)         # X != Y catches axis swaps, Z = 5 is a ragged tail, S fits one workgroup
CROP = (8, 16, 4)
SCALE_SAME = 1.01                                         # round(16 * 1.01) = 16, round(24 * 1.01) = 24: the resize keeps the size


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    shape: tuple
    C: int = 4
    angle: float = None
    scale: float = None
    sigma: float = None          # elastic: normal(0, sigma, 9) twice from `seed`; ties=True instead sets constant 33/64, -17/64
    shift: bool = False
    flips: int = 0
    crop: tuple = None
    origin: tuple = (0, 0, 0)
    offset4: bool = False        # the image starts 4 bytes into its allocation: scalar path also with C == 4
    ramp: bool = False           # image = the voxel index (elastic-only cases: every voxel is compared)
    ties: bool = False
    seed: int = 0

    @property
    def out_shape(self):
        return self.crop or self.shape


def _max_origin(shape, crop):
    return tuple(s - c for s, c in zip(shape, crop))


def _cases():
    out = []
    add = lambda name, shape, **kw: out.append(Case(name=name, shape=shape, seed=len(out) + 1, **kw))
    for tag, ang in (("0", 0.0), ("p20", 20.0), ("m20", -20.0), ("90", 90.0)):               # each stage alone
        add(f"rot_{tag}", A_, angle=ang)
    add("rot_p20_B_c3", B_, C=3, angle=20.0)
    add("scale_down", A_, scale=1 / 1.1)
    add("scale_up", A_, scale=1.1)
    add("scale_same", A_, scale=SCALE_SAME)
    add("scale_down_B_c1", B_, C=1, scale=1 / 1.1)
    add("elastic_s0", A_, sigma=0.0)
    add("elastic_s10", A_, sigma=10.0)
    add("elastic_s10_S", S_, sigma=10.0)
    add("elastic_ramp_s0", A_, sigma=0.0, ramp=True)
    add("elastic_ramp_s10", A_, sigma=10.0, ramp=True)
    add("elastic_ramp_s10_B", B_, sigma=10.0, ramp=True, offset4=True)
    add("elastic_ramp_s10_S_c3", S_, C=3, sigma=10.0, ramp=True)
    add("elastic_ramp_ties", A_, ramp=True, ties=True)
    add("shift", A_, shift=True)
    add("shift_c5", S_, C=5, shift=True)
    for f in range(8):                                                                        # every flip combination, with a crop
        shape = (A_, B_)[f & 1]
        add(f"flip_{f}", shape, C=(4, 3)[f & 1], flips=f, crop=CROP, origin=_max_origin(shape, CROP) if f & 2 else (0, 0, 0))
    add("crop_0", A_, crop=CROP)
    add("crop_max", A_, crop=CROP, origin=_max_origin(A_, CROP))
    add("copy_offset4", B_, offset4=True)
    add("all_A", A_, angle=20.0, scale=1 / 1.1, sigma=10.0, shift=True, flips=5, crop=CROP, origin=(3, 5, 2))
    add("all_A_up", A_, angle=-20.0, scale=1.1, sigma=10.0, shift=True, flips=2, crop=CROP, origin=_max_origin(A_, CROP))
    add("all_B_offset4", B_, angle=-20.0, scale=1 / 1.1, sigma=10.0, shift=True, flips=7, offset4=True)
    add("all_B_c3", B_, C=3, angle=20.0, scale=1.1, sigma=10.0, flips=3, crop=CROP, origin=(16, 0, 1))
    add("all_S_c1", S_, C=1, angle=20.0, scale=1 / 1.1, sigma=10.0, flips=6)
    return out


CASES = _cases()


def case_prm(c):
    dx = dy = None
    if c.ties:                   # map = index + k/64 with k odd: 32 map sits exactly on a rint tie, on every voxel
        dx, dy = np.full(9, 33 / 64), np.full(9, -17 / 64)
    elif c.sigma is not None:
        rs = np.random.RandomState(1000 + c.seed)
        dx, dy = rs.normal(0, c.sigma, 9), rs.normal(0, c.sigma, 9)
    shift = np.random.RandomState(2000 + c.seed).uniform(-0.1, 0.1, 4) if c.shift else None
    return make_prm(c.shape, c.angle, c.scale, dx, dy, shift, c.flips, c.origin)


def case_volume(c):
    """(img [X][Y][Z][C] float32, lbl [X][Y][Z] uint8): noise (or the voxel index), labels from {0, 1, 2, 4} in blobs"""
    X, Y, Z = c.shape
    rs = np.random.RandomState(c.seed)
    if c.ramp:
        img = (np.arange(X * Y * Z, dtype=np.float32).reshape(X, Y, Z, 1) + np.arange(c.C, dtype=np.float32) * 0.25).astype(np.float32)
    else:
        img = rs.standard_normal((X, Y, Z, c.C)).astype(np.float32)
    g = np.stack(np.mgrid[0:X, 0:Y, 0:Z], -1).astype(np.float64)
    lbl = np.zeros((X, Y, Z), np.uint8)
    for v in (1, 2, 4, 2, 1, 4):
        centre, radius = rs.uniform(0, 1, 3) * (X, Y, Z), rs.uniform(0.15, 0.4, 3) * (X, Y, Z) + 1
        lbl[(((g - centre) / radius) ** 2).sum(-1) <= 1] = v
    return img, lbl


@functools.lru_cache(maxsize=None)
def reference(name):
    """{img, lbl, prm, x64, y64, lmargin, imargin, x32, y32} of a case, computed once and shared (read only)."""
    c = next(k for k in CASES if k.name == name)
    img, lbl = case_volume(c)
    prm = case_prm(c)
    x64, y64, lm, im = augment3d(img, lbl, prm, c.crop, np.float64)
    x32, y32 = augment3d(img, lbl, prm, c.crop, np.float32)
    r = dict(case=c, img=img, lbl=lbl, prm=prm, x64=x64, y64=y64, lmargin=lm, imargin=im, x32=x32, y32=y32)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def ramp_gate(img):
    """What two float evaluations of one bilinear blend of ramp values may differ by: the nested form makes seven roundings of
    values up to max |img|, 2^-24 relative each; 8 x covers them.  One step of a quantised map moves the result by at least
    Z / 32 of a ramp unit, far above it."""
    return 8 * 2.0 ** -24 * float(np.abs(img).max())
