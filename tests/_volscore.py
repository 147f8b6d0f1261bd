"""Shared by tests/test_volscore_cpu.py and tests/test_volscore_gpu.py: the cases of uz_vol_edt_sq / uz_vol_region_scores
(csrc/volscore.hip) and what they expect.

The oracle is a RESTATEMENT, and an unpinnable one (like the cv2 and revtorch twins): the reference's getHd95 (data/bratsUtils.py:74-84)
calls MedPy 0.4.0's medpy.metric.binary.__surface_distances, MedPy is not installed here and bratsUtils.py imports it at the top, so
no golden vector can be made from the reference itself.  `surface_distances` below restates that MedPy function with the scipy calls
it makes (generate_binary_structure, binary_erosion, distance_transform_edt), `hd95` restates getHd95 with numpy.percentile, and
`reference_scores_fp32` restates dice / sensitivity / specificity (bratsUtils.py:6-24,57-72) with the reference's fp32 torch sums.
scipy's transform is exact on these shapes (rint(dt^2) reproduces dt to 0.0, checked in test_volscore_cpu.py), so `edt_sq` is an exact
integer yardstick.  The keyword arguments that are not the reference's exist only to show that the case set discriminates."""
import collections
import functools

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

INT32_MAX = 2 ** 31 - 1
BRATS_REGIONS = ((1, 2, 4), (1, 4), (4,))


# ================================================================================================ the oracle
def border(mask, connectivity=1, border_value=0):
    """mask ^ erosion(mask): MedPy __surface_distances' result_border / reference_border"""
    fp = generate_binary_structure(mask.ndim, connectivity)
    return mask ^ binary_erosion(mask, structure=fp, iterations=1, border_value=border_value)


def surface_distances(result, reference, connectivity=1, border_value=0):
    """MedPy 0.4.0 medpy.metric.binary.__surface_distances(result, reference) with voxelspacing None, connectivity 1"""
    dt = distance_transform_edt(~border(reference, connectivity, border_value))
    return dt[border(result, connectivity, border_value)]


def hd95(pred, ref, connectivity=1, border_value=0, directions=2, method="linear"):
    """bratsUtils.py:74-84 getHd95"""
    if np.count_nonzero(pred) > 0 and np.count_nonzero(ref):
        d = [surface_distances(pred, ref, connectivity, border_value)]
        if directions == 2:
            d.append(surface_distances(ref, pred, connectivity, border_value))
        return float(np.percentile(np.hstack(d), 95, method=method))
    return -1.0


def hd95_n(pred, ref):
    """how many distances the percentile is taken of"""
    return int(border(pred).sum() + border(ref).sum())


def edt_sq(seeds):
    """exact squared distance to the nearest seed, int64; INT32_MAX everywhere without a seed"""
    if not seeds.any():
        return np.full(seeds.shape, INT32_MAX, np.int64)
    return np.rint(distance_transform_edt(~seeds) ** 2).astype(np.int64)


def counts_of(pred, ref):
    """tp, |pred|, |ref|, P as Python integers"""
    return int((pred & ref).sum()), int(pred.sum()), int(ref.sum()), int(pred.size)


def scores_from_counts(tp, cp, cr, P):
    """the exact-integer formulas of uz_api.h, one fp64 division each: dice, sensitivity, specificity"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = 1.0 if cp + cr == 0 else float(np.float64(2 * tp) / np.float64(cp + cr))
        sens = 1.0 if cr == 0 else float(np.float64(tp) / np.float64(cr))
        spec = float(np.float64(P - cp - cr + tp) / np.float64(P - cr))
    return dice, sens, spec


def reference_scores_fp32(pred, ref):
    """bratsUtils.py:6-24 (dice through softDice(predBin, target, 0, True), with the NaN fix of :15), :57-65 sensitivity, :67-72 specificity
    as the reference computes them: fp32 torch tensors (1, D, H, W), fp32 sums"""
    import torch
    p = torch.from_numpy(pred.astype(np.float32))[None]
    t = torch.from_numpy(ref.astype(np.float32))[None]
    pb = (p > 0.5).float()
    inter = (pb * t).sum(dim=(1, 2, 3))
    union = pb.sum() + t.sum()
    d = (2 * inter + 0) / (union + 0)
    d[d != d] = d.new_tensor([1.0])
    dice = d.mean().item()
    allpos = t.sum()
    sens = 1.0 if allpos == 0 else ((pb * t).sum() / allpos).item()
    pinv, tinv = (p <= 0.5).float(), (t == 0).float()
    spec = ((pinv * tinv).sum() / tinv.sum()).item()
    return dice, sens, spec


# ================================================================================================ the cases
Case = collections.namedtuple("Case", "name shape pred ref")           # pred, ref: read-only bool volumes
LONG_SHAPES = ((3, 5, 261), (261, 3, 5), (5, 261, 3))
SLAB_HD95, SLAB_N = 196.0, 1291


def _slab(shape, lo, hi):
    ax = int(np.argmax(shape))
    m = np.zeros(shape, bool)
    sl = [slice(None)] * 3
    sl[ax] = slice(lo, hi)
    m[tuple(sl)] = True
    return m


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return sum(((a - c) / r) ** 2 for a, c, r in zip(g, centre, radii)) <= 1.0


def _make_cases():
    cs = []
    for shape in LONG_SHAPES:                                            # one axis longer than a 256-thread workgroup, in each position
        pred = _slab(shape, 0, 40) | _slab(shape, 250, 261)
        ref = _slab(shape, 5, 60)
        ref[1, 1, 1] = True
        cs.append(Case("slabs_%dx%dx%d" % shape, shape, pred, ref))
    # overlapping ellipsoids plus a detached small component: many distinct d2, and the centres are placed so that h is fractional
    # BETWEEN TWO DIFFERENT distances (3.742 | 4.0 at h - lo = 0.3; 4.690 | 4.899 at 0.6) - only then does the percentile rule show
    for shape, (a, b, c) in (((24, 24, 16), (0.43, 0.40, 0.36)), ((40, 48, 33), (0.46, 0.46, 0.32))):
        D, H, W = shape
        pred = _ellipsoid(shape, (D * a, H * 0.5, W * 0.5), (D * 0.30, H * 0.26, W * c))
        ref = _ellipsoid(shape, (D * 0.55, H * b, W * 0.45), (D * 0.27, H * 0.31, W * 0.30))
        pred = pred | _ellipsoid(shape, (D - 3.0, H - 3.0, W - 3.0), (1.6, 1.6, 1.6))
        cs.append(Case("ellipsoids_%dx%dx%d" % shape, shape, pred, ref))
    shape = (1, 17, 19)                                                  # a degenerate axis (2.236 | 2.828 at h - lo = 0.55)
    cs.append(Case("flat_1x17x19", shape, _ellipsoid(shape, (0, 8, 9), (1, 5.2, 6.1)), _ellipsoid(shape, (0, 9, 11), (1, 4.1, 5.3)) | _ellipsoid(shape, (0, 1.5, 1.5), (1, 1.2, 1.2))))
    shape = (7, 6, 5)
    box = np.zeros(shape, bool); box[2:5, 2:4, 1:4] = True
    one_a = np.zeros(shape, bool); one_a[0, 0, 0] = True
    one_b = np.zeros(shape, bool); one_b[6, 5, 4] = True
    full, none = np.ones(shape, bool), np.zeros(shape, bool)
    cs.append(Case("whole_volume_pred", shape, full, box))               # the border is the shell at the volume's faces
    cs.append(Case("two_voxels", shape, one_a, one_b))                   # n = 2, h = 0.95
    cs.append(Case("empty_pred", shape, none, box))
    cs.append(Case("empty_ref", shape, box, none))
    cs.append(Case("both_empty", shape, none, none))
    cs.append(Case("whole_volume_ref", shape, box, full))                # specificity 0 / 0
    for c in cs:
        c.pred.setflags(write=False); c.ref.setflags(write=False)
    return cs


CASES = _make_cases()
EMPTY_CASES = ("empty_pred", "empty_ref", "both_empty")


def case(name):
    return next(c for c in CASES if c.name == name)


Expected = collections.namedtuple("Expected", "counts dice sensitivity specificity hd95 n")


@functools.lru_cache(maxsize=None)
def expected_masks(pred_bytes, ref_bytes, shape):
    pred = np.frombuffer(pred_bytes, bool).reshape(shape)
    ref = np.frombuffer(ref_bytes, bool).reshape(shape)
    cnt = counts_of(pred, ref)
    d, s, sp = scores_from_counts(*cnt)
    return Expected(cnt, d, s, sp, hd95(pred, ref), hd95_n(pred, ref))


def expected(pred, ref):
    """what the oracle gives for one (pred mask, ref mask) pair; computed once per pair"""
    return expected_masks(np.ascontiguousarray(pred).tobytes(), np.ascontiguousarray(ref).tobytes(), pred.shape)


# ------------------------------------------------------------------------------------------------ the label-volume case
LABEL_SHAPE = (24, 24, 16)


@functools.lru_cache(maxsize=None)
def label_case():
    """(pred (3, D, H, W) uint8, ref (D, H, W) uint8), read-only: raw BraTS values 0, 1, 2, 4 as nested ellipsoids (2 the oedema shell, 1
    the core, 4 inside it), a stray 7 and a stray 200 INSIDE each tumour (a value outside every region punches a hole into WT, and
    200 >= 32 must set no bit), row 2 without any 4 (its ET is empty)."""
    D, H, W = LABEL_SHAPE

    def vol(c, s, with_et=True):
        v = np.zeros(LABEL_SHAPE, np.uint8)
        v[_ellipsoid(LABEL_SHAPE, c, (8.5 * s, 8.0 * s, 5.5 * s))] = 2
        v[_ellipsoid(LABEL_SHAPE, c, (5.5 * s, 5.0 * s, 3.6 * s))] = 1
        if with_et:
            v[_ellipsoid(LABEL_SHAPE, (c[0] + 1, c[1], c[2]), (2.6 * s, 2.4 * s, 1.9 * s))] = 4
        ci = tuple(int(round(x)) for x in c)
        v[ci[0] - 3, ci[1], ci[2]] = 7
        v[ci[0], ci[1] + 3, ci[2]] = 200
        return v
    ref = vol((12.0, 11.0, 8.0), 1.0)
    pred = np.stack([vol((11.0, 12.0, 7.0), 1.05), vol((13.0, 11.0, 8.0), 0.9), vol((12.0, 12.0, 8.0), 1.0, with_et=False)])
    pred.setflags(write=False); ref.setflags(write=False)
    return pred, ref


def region_mask(labels, region):
    return np.isin(labels, region)


def region_bits(region):
    return sum(1 << v for v in region)
