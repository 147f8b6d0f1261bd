"""Shared by tests/test_volprep_cpu.py and tests/test_volprep_gpu.py: a numpy twin of uz_vol_prepare and uz_vol_restore (include/uz_api.h
"volume preparation"), a restatement of the reference's four loader functions written from those rules, exact statistics in
fractions.Fraction, the error bounds of the kernel's summation, and the case set.

Intensities are integer-valued, as real BraTS has them: every fp64 sum of x is then exact, the exact mean and variance are rationals,
and what remains to bound is the centred squares and the final divisions."""
import collections
import ctypes as C
import functools
import warnings
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)                            # unit roundoff of fp64
BRATS_LUT = (0, 1, 2, 4)

DEFECTS = ("box_ne0", "box_ch0", "stats_whole_box", "zeros_counted", "ddof1", "half_up", "corner_as_centre", "zeros_normalised",
           "mask_unshifted", "restore_ignores_shift", "lut_on_fill", "last_slice_dropped")


# ================================================================================================ the twin
def box_of(raw, defect=None):
    """(lo[3], hi[3]) over the voxels with any channel > 0, or None"""
    if defect == "box_ne0":
        pos = (raw != 0).any(axis=3)
    elif defect == "box_ch0":
        pos = raw[..., 0] > 0
    else:
        pos = (raw > 0).any(axis=3)
    if not pos.any():
        return None
    lo, hi = [], []
    for a in range(3):
        idx = np.nonzero(pos.any(axis=tuple(b for b in range(3) if b != a)))[0]
        lo.append(int(idx[0]))
        hi.append(int(idx[-1]) + (0 if defect == "last_slice_dropped" else 1))
    return lo, hi


def descriptor(lo, hi, size, placement, defect=None):
    """per axis (n, t, e) and the lost flag"""
    if defect == "corner_as_centre":
        placement = 0
    n, t, e, lost = [], [], [], 0
    for a in range(3):
        s, T = hi[a] - lo[a], size[a]
        d = abs(T - s) // 2
        if defect == "half_up":
            d = (abs(T - s) + 1) // 2
        if T < s:
            lost = 2
            n.append(lo[a] + (d if placement == 0 else 0)); t.append(0); e.append(T)
        else:
            n.append(lo[a]); t.append(d if placement == 0 else 0); e.append(s)
    return n, t, e, lost


Prepared = collections.namedtuple("Prepared", "image mask info stats")


def prepare(raw, mask, size, placement, defect=None):
    """uz_vol_prepare in numpy -> Prepared(image fp32, mask uint8 or None, info int32[16], stats (C, 3) fp64)"""
    Cn = raw.shape[3]
    image = np.zeros(tuple(size) + (Cn,), np.float32)
    mask_out = None if mask is None else np.zeros(tuple(size), np.uint8)
    info = np.zeros(16, np.int32)
    stats = np.zeros((Cn, 3), np.float64)
    box = box_of(raw, defect)
    if box is None:
        info[15] = 1
        return Prepared(image, mask_out, info, stats)
    lo, hi = box
    n, t, e, lost = descriptor(lo, hi, size, placement, defect)
    info[:] = lo + hi + n + t + e + [lost]
    src = tuple(slice(n[a], n[a] + e[a]) for a in range(3))
    dst = tuple(slice(t[a], t[a] + e[a]) for a in range(3))
    block = raw[src]
    pool = raw[tuple(slice(lo[a], hi[a]) for a in range(3))] if defect == "stats_whole_box" else block
    out = np.zeros_like(block)
    for c in range(Cn):
        v = pool[..., c].astype(np.float64)
        sel = v[v != 0] if defect != "zeros_counted" else v.ravel()
        if sel.size == 0:
            continue
        m = sel.sum() / sel.size
        den = sel.size - 1 if defect == "ddof1" and sel.size > 1 else sel.size
        s = np.sqrt(((sel - m) ** 2).sum() / den)
        stats[c] = sel.size, m, s
        x = block[..., c]
        with np.errstate(invalid="ignore", divide="ignore"):
            y = (x - np.float32(m)) / np.float32(s)
        out[..., c] = y if defect == "zeros_normalised" else np.where(x == 0, np.float32(0), y)
    image[dst] = out
    if mask is not None:
        msrc = tuple(slice(lo[a], lo[a] + e[a]) for a in range(3)) if defect == "mask_unshifted" else src
        mask_out[dst] = mask[msrc]
    return Prepared(image, mask_out, info, stats)


def restore(rows, place, native, lut=None, fill=0, defect=None):
    """uz_vol_restore in numpy, voxel rule by voxel rule: clipped where `place` reaches outside either volume"""
    N = rows.shape[0]
    T = rows.shape[1:]
    n, t, e = [int(v) for v in place[0:3]], [int(v) for v in place[3:6]], [int(v) for v in place[6:9]]
    fv = rows.dtype.type(fill)
    if defect == "lut_on_fill" and lut is not None:
        fv = rows.dtype.type(_table(lut)[int(fill)])
    out = np.full((N,) + tuple(native), fv, rows.dtype)
    idx, src = [], []
    for a in range(3):
        v = np.arange(native[a])
        d = v - n[a]
        ok = (d >= 0) & (d < e[a]) & (d + t[a] >= 0) & (d + t[a] < T[a])
        idx.append(v[ok])
        src.append((d + t[a])[ok])
    if all(len(i) for i in idx):
        val = rows[np.ix_(np.arange(N), src[0], src[1], src[2])]
        if lut is not None:
            val = _table(lut)[val]
        out[np.ix_(np.arange(N), idx[0], idx[1], idx[2])] = val
    return out


def place_of(info, defect=None):
    """info[6..14]; the planted defect takes the box origin for the native origin"""
    p = np.array(info[6:15], np.int32)
    if defect == "restore_ignores_shift":
        p[0:3] = info[0:3]
    return p


def _table(lut):
    tab = np.arange(256, dtype=np.uint8)
    tab[:len(lut)] = np.asarray(lut, np.uint8)
    return tab


# ================================================================================================ the reference's four functions, restated
def ref_crop(image, mask=None):
    """crop_volume_allDim: the box of image > 0 over all channels, cut out of image (and mask) -> image, mask, [x0, y0, z0]"""
    coords = np.argwhere(image > 0)
    if coords.shape[0] == 0:
        raise ValueError("no voxel > 0")
    a, b = coords.min(axis=0)[:3], coords.max(axis=0)[:3] + 1
    cut = tuple(slice(int(a[k]), int(b[k])) for k in range(3))
    return image[cut], (None if mask is None else mask[cut]), [int(v) for v in a]


def ref_place_centre(vol, size):
    """crop_or_pad_slice_to_size of the training loader (no offset): centred, whatever the trailing axes"""
    out = np.zeros(tuple(size) + vol.shape[3:], vol.dtype)
    dst, src = [], []
    for T, s in zip(size, vol.shape[:3]):
        d = abs(T - s) // 2
        if T < s:
            dst.append(slice(0, T)); src.append(slice(d, d + T))
        else:
            dst.append(slice(d, d + s)); src.append(slice(0, s))
    out[tuple(dst)] = vol[tuple(src)]
    return out


def ref_place_corner(vol, size):
    """crop_or_pad_slice_to_size of the validation loader: at the corner; every axis that does not fit is truncated (the reference
    truncates x and fails on y / z)"""
    out = np.zeros(tuple(size) + vol.shape[3:], vol.dtype)
    keep = tuple(slice(0, min(T, s)) for T, s in zip(size, vol.shape[:3]))
    out[keep] = vol[keep]
    return out


def ref_normalise(image):
    """normalise_image of the validation loader: fp64 statistics over the non-zero voxels per channel, cast to fp32, fp32 arithmetic"""
    wide = np.where(image == 0, np.nan, image.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = np.nanmean(wide, axis=(0, 1, 2)).astype(np.float32)
        s = np.nanstd(wide, axis=(0, 1, 2)).astype(np.float32)
        y = np.divide(image - m, s)
    return np.where(image == 0, np.float32(0), y).astype(np.float32)


def ref_pipeline(raw, mask, size, placement):
    """-> image, mask, offsets as the reference's loaders produce them"""
    img, msk, off = ref_crop(raw, mask)
    put = ref_place_centre if placement == 0 else ref_place_corner
    return ref_normalise(put(img, size)), (None if msk is None else put(msk, size)), off


# ================================================================================================ exact statistics and the bounds
def exact_stats(raw, info):
    """per channel (count, mean, variance, sum|x|) of the placed non-zero voxels as exact rationals (integer-valued intensities)"""
    n, e = info[6:9], info[12:15]
    block = raw[tuple(slice(int(n[a]), int(n[a] + e[a])) for a in range(3))]
    out = []
    for c in range(raw.shape[3]):
        v = block[..., c]
        v = v[v != 0]
        assert np.array_equal(v, np.round(v)), "the cases hold integer-valued intensities"
        xs = [int(x) for x in v.ravel()]
        k = len(xs)
        if k == 0:
            out.append((0, Fraction(0), Fraction(0), Fraction(0)))
            continue
        s1, s2 = sum(xs), sum(x * x for x in xs)
        out.append((k, Fraction(s1, k), Fraction(k * s2 - s1 * s1, k * k), Fraction(sum(abs(x) for x in xs))))
    return out


def mean_bound(k, sum_abs):
    """the outer limit of the kernel's mean: (k - 1) 2^-53 sum|x| / k.  The summation's share is (k - 1) u sum|x| in ANY order (here 0:
    the integer sums are exact); the division's rounding, u |mean| <= u sum|x| / k, fits inside for k >= 2 and is 0 for k = 1."""
    return (k - 1) * U * sum_abs / k if k else Fraction(0)


def var_bound(k, var, dm):
    """|sum_hat / k - V|: a term (x - m)^2 carries at most three roundings and the sum k - 1, the division one: (k + 3) u of the terms,
    which are all >= 0; computed with the rounded mean they sum to k (V + dm^2)."""
    return (k + 3) * U * (var + dm * dm) + dm * dm


def std_within(s_hat, var, bound):
    """|s_hat - sqrt(var)| <= bound, decided in rationals"""
    s = Fraction(float(s_hat))
    lo = max(s - bound, Fraction(0))
    return lo * lo <= var <= (s + bound) * (s + bound)


def std_bound(k, var, sum_abs):
    """|std_hat - sqrt(V)| <= var_bound / sqrt(V) + 2 u sqrt(V) (square root and division), with sqrt(V) bracketed by floats"""
    if var == 0:
        return Fraction(0)
    dm = mean_bound(k, sum_abs)
    root = Fraction(float(var) ** 0.5)
    return var_bound(k, var, dm) / (root * (1 - 4 * U)) + 2 * U * root * (1 + 4 * U)


def f32_margin(value, bound):
    """True when every number within `bound` of the rational `value` rounds to the same fp32"""
    f = np.float32(float(value))
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        edge = (Fraction(float(f)) + Fraction(float(other))) / 2
        if abs(value - edge) <= bound:
            return False
    return True


def f32_margin_sqrt(var, bound):
    """the same for sqrt(var)"""
    f = np.float32(float(var) ** 0.5)
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        edge = (Fraction(float(f)) + Fraction(float(other))) / 2
        lo, hi = max(edge - bound, Fraction(0)), edge + bound
        if lo * lo <= var <= hi * hi:
            return False
    return True


# ================================================================================================ the cases
Case = collections.namedtuple("Case", "name raw mask size placement offset box")
Case.__doc__ = """raw (X, Y, Z, C) fp32, mask (X, Y, Z) uint8, target size, placement 0 / 1, offset = bytes off a 16-byte boundary for raw and
image on the device, box = the (lo, hi) the support was built for (None: all <= 0)"""

SHAPE = (13, 10, 37)
BOX = ([2, 0, 5], [11, 10, 34])                     # 9 x 10 x 29


def _content(rng, shape, Cn, zeros=0.3, low=1, high=400):
    v = rng.integers(low, high, size=tuple(shape) + (Cn,)).astype(np.float32)
    v[rng.random(v.shape) < zeros] = 0
    return v


def _boxed(seed, shape=SHAPE, Cn=4, box=BOX, negatives=False, shell=None):
    """zeros outside the box (or negatives), random content with zeros (and negatives) inside, every face of the box touched"""
    rng = np.random.default_rng(seed)
    lo, hi = box
    raw = np.zeros(tuple(shape) + (Cn,), np.float32)
    if negatives:
        raw[...] = -rng.integers(0, 50, size=raw.shape).astype(np.float32)
    inner = tuple(slice(lo[a], hi[a]) for a in range(3))
    body = _content(rng, [hi[a] - lo[a] for a in range(3)], Cn, low=-120 if negatives else 1)
    if shell is not None:                                                  # large values on the outermost `shell` layers of the box
        big = np.ones(body.shape[:3], bool)
        big[tuple(slice(shell, body.shape[a] - shell) for a in range(3))] = False
        body[big] = body[big] * 0 + rng.integers(9000, 12000, size=body[big].shape).astype(np.float32)
    raw[inner] = body
    for a in range(3):                                                      # one positive voxel on each face
        for side in (lo[a], hi[a] - 1):
            p = [int(rng.integers(lo[b], hi[b])) for b in range(3)]
            p[a] = side
            raw[p[0], p[1], p[2], int(rng.integers(0, Cn))] = float(rng.integers(1, 400))
    return raw


def _mask(seed, shape):
    rng = np.random.default_rng(seed)
    return np.array(BRATS_LUT, np.uint8)[rng.integers(0, 4, size=shape)]


def _faces():
    """each lower face of the box from another channel, the three upper faces from ONE voxel in channel 3"""
    rng = np.random.default_rng(40)
    raw = np.zeros(SHAPE + (4,), np.float32)
    raw[4:8, 3:7, 10:25, :] = _content(rng, (4, 4, 15), 4)
    raw[3, 5, 12, 0] = 17          # x0 = 3
    raw[5, 1, 14, 1] = 23          # y0 = 1
    raw[6, 4, 6, 2] = 31           # z0 = 6
    raw[10, 8, 33, 3] = 5          # x1 = 11, y1 = 9, z1 = 34
    return raw, ([3, 1, 6], [11, 9, 34])


def _one_voxel():
    raw = np.zeros(SHAPE + (4,), np.float32)
    raw[..., 0] = -3
    raw[7, 4, 20, 2] = 55
    return raw, ([7, 4, 20], [8, 5, 21])


def _empty():
    rng = np.random.default_rng(41)
    return -rng.integers(0, 9, size=SHAPE + (4,)).astype(np.float32), None


def prepare_route(Cn, shape, size, align):
    from unet_zoo_amd import _ffi
    out = (C.c_int * 3)()
    rc = _ffi.lib().uz_vol_prepare_route(Cn, *shape, *size, align, out)
    assert rc == 0, _ffi.lib().uz_last_error()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stride_shape():
    """the smallest 64 x 64 x Z whose bounds pass takes more than one sweep of the capped grid, and the workgroups of that grid"""
    for Z in range(1, 4096):
        form, wg, strides = prepare_route(4, (64, 64, Z), (24, 24, 24), 16)
        if strides:
            assert form == 1
            return (64, 64, Z), wg
    raise AssertionError("no striding size found")


def _stride():
    """content near the origin, one voxel that only the LAST workgroup of the first sweep sees (it sets three upper faces), one in the
    second sweep that sets none"""
    shape, wg = stride_shape()
    rng = np.random.default_rng(42)
    raw = np.zeros(shape + (4,), np.float32)
    raw[1:20, 2:22, 3:30, :] = _content(rng, (19, 20, 27), 4)
    flat = raw.reshape(-1, 4)
    last = wg * 256 - 1
    assert last < flat.shape[0] - 1
    flat[last, 1] = 9
    flat[last + 1, 2] = -4                                                 # second sweep, workgroup 0: not > 0
    x, y, z = np.unravel_index(last, shape)
    return raw, ([min(int(x), 1), min(int(y), 2), min(int(z), 3)], [max(int(x) + 1, 20), max(int(y) + 1, 22), max(int(z) + 1, 30)])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda name, raw, size, placement, box, offset=0: out.append(Case(name, raw, _mask(len(out), raw.shape[:3]), tuple(size), placement, offset, box))
    raw = _boxed(1)
    add("centre_crop_pad_equal", raw, (6, 14, 29), 0, BOX)                 # crop odd difference, pad even difference, equal
    add("centre_pad_crop_pad", raw, (12, 7, 40), 0, BOX)                   # pad odd, crop odd, pad odd
    add("corner_pad", raw, (16, 16, 32), 1, BOX)
    add("corner_truncates", raw, (6, 7, 20), 1, BOX)
    f, fbox = _faces()
    add("faces_by_channel", f, (10, 8, 30), 0, fbox)
    add("negatives", _boxed(2, negatives=True), (10, 12, 27), 0, BOX)
    add("cropped_large_centre", _boxed(3, shell=2), (5, 6, 25), 0, BOX)
    add("cropped_large_corner", _boxed(3, shell=2), (7, 8, 27), 1, BOX)
    o, obox = _one_voxel()
    add("one_voxel", o, (4, 5, 6), 0, obox)
    e, _ = _empty()
    add("all_le_zero", e, (6, 7, 8), 0, None)
    for Cn in (1, 3, 5):
        add(f"c{Cn}", _boxed(10 + Cn, shape=(7, 9, 11), Cn=Cn, box=([1, 2, 0], [6, 9, 10])), (6, 6, 12), 0, ([1, 2, 0], [6, 9, 10]))
    add("c4_off_alignment", _boxed(20, shape=(7, 9, 11), Cn=4, box=([0, 1, 2], [7, 8, 11])), (8, 6, 8), 1, ([0, 1, 2], [7, 8, 11]), offset=4)
    s, sbox = _stride()
    add("grid_stride", s, (24, 24, 32), 1, sbox)                           # corner: the placed block holds the content near the origin
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = ("centre_crop_pad_equal", "centre_pad_crop_pad", "corner_pad", "corner_truncates", "faces_by_channel", "negatives", "cropped_large_centre",
         "cropped_large_corner", "one_voxel", "all_le_zero", "c1", "c3", "c5", "c4_off_alignment", "grid_stride")
STATS_FREE = ("one_voxel", "all_le_zero")           # box, descriptor and NaN-ness only


@functools.lru_cache(maxsize=None)
def expected(name):
    """the twin's result, computed once"""
    c = case(name)
    return prepare(c.raw, c.mask, c.size, c.placement)


# ------------------------------------------------------------------------------------------------ restore
NATIVE = (15, 12, 41)
TARGET = (10, 9, 30)
PLACES = {"origins": (2, 1, 3, 1, 2, 4, 7, 6, 20),                          # both origins non-zero
          "far_face": (5, 3, 11, 0, 0, 0, 10, 9, 30),                       # the extent ends on the far native face of every axis
          "hanging": (-2, 8, 30, 3, 0, 5, 12, 9, 30),                       # reaches outside the native volume and the rows: clipped
          "nothing": (0, 0, 0, 0, 0, 0, 0, 5, 5)}
RESTORE_N = (1, 3, 17)


@functools.lru_cache(maxsize=None)
def restore_rows(N, kind):
    rng = np.random.default_rng(100 + N)
    if kind == "u8":
        return rng.integers(0, 4, size=(N,) + TARGET).astype(np.uint8)
    return rng.standard_normal((N,) + TARGET).astype(np.float32)
