"""Numpy twin of uz_vol_uncertainty (include/uz_api.h "volume uncertainty"), a brute-force reference that knows nothing of the vote
table, and the case set the CPU and GPU tests share.

twin:   table[r][c][d][t] from one np.bincount per region; levels, curves, areas and calibration from the header's formulas with Python
        integers - every curve and calibration value is one int / int division, which Python rounds correctly, as the fp64 division of
        two exactly represented integers is.
brute:  per level j it masks the voxels with a <= j and counts tp / fp / fn / tn on the masked arrays; curves, areas and the score are
        fractions.Fraction; the calibration comes from the per-voxel p = c / S (ECE and MCE over the voxels that share a p).
Gate of the areas and the score (derived, not measured): every curve value lies in [0, 1] and carries at most 2^-53 of rounding, the S
additions of a trapezoid sum below S add at most S/2 * 2^-52 relative to S, the division by S one more rounding:
|x - exact| <= (S + 4) * 2^-52."""
import collections
import functools
from fractions import Fraction

import numpy as np

BRATS = ((1, 2, 4), (1, 4), (4,))                    # raw values: WT, TC, ET
INDEX = ((1, 2, 3), (1, 3), (3,))                    # class indices 0 .. 3 of a network whose class 3 is the raw label 4
WG_WIDE = 256 * 16                                   # voxels one workgroup of the wide form takes in one sweep
CAP = 1024                                           # workgroups of the table pass at the most
R_VALUES = (1, 3, 8)
DEFECTS = ("s_minus_1", "majority_decision", "pred_sets_for_ref", "drop_tail16", "a_lt_j", "tie_wrong_side", "wrap_32", "ftn_from_tp", "drop_last_slice")


def auc_bound(S):
    return (S + 4) * 2.0 ** -52


def regions(R, base=BRATS):
    """R regions: the nested three, then the same again, then two that hold the top label with 2 and with the value 0 (a set with 0
    makes every background word count)"""
    top = base[2][0]
    return (tuple(base) * 2 + ((2, top), (0, top)))[:R] if R > 1 else (base[0],)


def region_bits(values):
    m = 0
    for v in values:
        m |= 1 << int(v)
    return m


def in_set(vol, bits, wrap=False):
    v = vol.astype(np.int64)
    if wrap:
        return ((bits >> (v & 31)) & 1).astype(bool)
    return (v < 32) & (((bits >> np.minimum(v, 31)) & 1) == 1)


# ================================================================================================ the twin
def votes(samples, pred_regions, defects=()):
    """(R, D, H, W) uint8 = c"""
    S = samples.shape[0] - (1 if "s_minus_1" in defects else 0)
    return np.stack([in_set(samples[:S], region_bits(reg), "wrap_32" in defects).sum(0).astype(np.uint8) for reg in pred_regions])


def table(samples, decision, ref, pred_regions, ref_regions, defects=()):
    """(R, S+1, 2, 2) int64"""
    S, P = samples.shape[0], decision.size
    c_all = votes(samples, pred_regions, defects).reshape(len(pred_regions), P).astype(np.int64)
    out = np.zeros((len(pred_regions), S + 1, 2, 2), np.int64)
    keep = P
    if "drop_tail16" in defects:
        keep = P - P % 16
    if "drop_last_slice" in defects:
        keep = max(P - 256, 0)                                           # without what the last workgroup counted
    for r, (preg, rreg) in enumerate(zip(pred_regions, ref_regions)):
        c = c_all[r]
        if "majority_decision" in defects:
            d = (2 * c > S).astype(np.int64)
        else:
            d = in_set(decision.reshape(P), region_bits(preg), "wrap_32" in defects).astype(np.int64)
        t = in_set(ref.reshape(P), region_bits(preg if "pred_sets_for_ref" in defects else rreg), "wrap_32" in defects).astype(np.int64)
        if "tie_wrong_side" in defects and S % 2 == 0:
            d = np.where(2 * c == S, 1 - d, d)
        out[r] = np.bincount((c * 4 + d * 2 + t)[:keep], minlength=(S + 1) * 4).reshape(S + 1, 2, 2)
    return out


Derived = collections.namedtuple("Derived", "levels curves auc calibration")


def derive(tab, defects=()):
    """levels (R, S+1, 4) int64, curves (R, S+1, 3), auc (R, 4), calibration (R, 3) fp64 from the table alone"""
    R, S = tab.shape[0], tab.shape[1] - 1
    levels = np.zeros((R, S + 1, 4), np.int64)
    curves = np.zeros((R, S + 1, 3))
    auc = np.zeros((R, 4))
    cal = np.zeros((R, 3))
    for r in range(R):
        T = [[[int(tab[r, c, d, t]) for t in range(2)] for d in range(2)] for c in range(S + 1)]
        P = sum(T[c][d][t] for c in range(S + 1) for d in range(2) for t in range(2))
        for j in range(S + 1):
            hi = [c for c in range(S + 1) if (S - c < j if "a_lt_j" in defects else S - c <= j)]
            lo = [c for c in range(S + 1) if (c < j if "a_lt_j" in defects else c <= j)]
            levels[r, j] = (sum(T[c][1][1] for c in hi), sum(T[c][1][0] for c in hi), sum(T[c][0][1] for c in lo), sum(T[c][0][0] for c in lo))
        L = [[int(x) for x in row] for row in levels[r]]
        tpS, tnS = L[S][0], L[S][3]
        for j in range(S + 1):
            tp, fp, fn, tn = L[j]
            den = 2 * tp + fp + fn
            curves[r, j, 0] = 1.0 if den == 0 else (2 * tp) / den
            curves[r, j, 1] = 0.0 if tpS == 0 else (tpS - tp) / tpS
            if "ftn_from_tp" in defects:
                curves[r, j, 2] = curves[r, j, 1]
            else:
                curves[r, j, 2] = 0.0 if tnS == 0 else (tnS - tn) / tnS
        for k in range(3):
            a = 0.0
            for j in range(S):
                a += (float(curves[r, j, k]) + float(curves[r, j + 1, k])) * 0.5
            auc[r, k] = a / S
        auc[r, 3] = (auc[r, 0] + (1.0 - auc[r, 1]) + (1.0 - auc[r, 2])) / 3.0
        ece = brier = 0
        mce = 0.0
        for c in range(S + 1):
            pos = T[c][0][1] + T[c][1][1]
            n = pos + T[c][0][0] + T[c][1][0]
            gap = abs(S * pos - c * n)
            ece += gap
            brier += pos * (S - c) ** 2 + (n - pos) * c ** 2
            if n > 0:
                mce = max(mce, gap / (S * n))
        cal[r] = (ece / (S * P), mce, brier / (S * S * P))
    return Derived(levels, curves, auc, cal)


def exact_auc(levels):
    """The areas and the score of integer levels (R, S+1, 4) as Fractions: [[auc_dice, auc_ftp, auc_ftn, score]] per region"""
    out = []
    for lev in levels:
        S = len(lev) - 1
        L = [[int(x) for x in row] for row in lev]
        tpS, tnS = L[S][0], L[S][3]
        cur = []
        for tp, fp, fn, tn in L:
            den = 2 * tp + fp + fn
            cur.append((Fraction(1) if den == 0 else Fraction(2 * tp, den), Fraction(0) if tpS == 0 else Fraction(tpS - tp, tpS),
                        Fraction(0) if tnS == 0 else Fraction(tnS - tn, tnS)))
        a = [sum((cur[j][k] + cur[j + 1][k]) / 2 for j in range(S)) / S for k in range(3)]
        out.append(a + [(a[0] + (1 - a[1]) + (1 - a[2])) / 3])
    return out


# ================================================================================================ brute force: no table
Brute = collections.namedtuple("Brute", "levels curves auc calibration")


def brute(samples, decision, ref, pred_regions, ref_regions):
    """levels as Python ints, curves / auc / calibration as Fractions, region by region"""
    S, P = samples.shape[0], decision.size
    levels, curves, aucs, cals = [], [], [], []
    for preg, rreg in zip(pred_regions, ref_regions):
        pb, rb = region_bits(preg), region_bits(rreg)
        c = np.zeros(decision.shape, np.int64)
        for s in range(S):
            c += in_set(samples[s], pb)
        d, t = in_set(decision, pb), in_set(ref, rb)
        a = np.where(d, S - c, c)
        lev = []
        for j in range(S + 1):
            m = a <= j
            dm, tm = d[m], t[m]
            lev.append((int((dm & tm).sum()), int((dm & ~tm).sum()), int((~dm & tm).sum()), int((~dm & ~tm).sum())))
        tpS, tnS = lev[S][0], lev[S][3]
        cur = []
        for tp, fp, fn, tn in lev:
            den = 2 * tp + fp + fn
            cur.append((Fraction(1) if den == 0 else Fraction(2 * tp, den), Fraction(0) if tpS == 0 else Fraction(tpS - tp, tpS),
                        Fraction(0) if tnS == 0 else Fraction(tnS - tn, tnS)))
        ar = [sum((cur[j][k] + cur[j + 1][k]) / 2 for j in range(S)) / S for k in range(3)]
        ar.append((ar[0] + (1 - ar[1]) + (1 - ar[2])) / 3)
        # calibration from the per-voxel probability p = c / S: the voxels that share a p are one bin
        ece, mce = Fraction(0), Fraction(0)
        for u in np.unique(c):
            m = c == u
            n, pos = int(m.sum()), int(t[m].sum())
            gap = abs(Fraction(pos, n) - Fraction(int(u), S))
            ece += Fraction(n, P) * gap
            mce = max(mce, gap)
        brier = Fraction(int(((c - S * t.astype(np.int64)) ** 2).sum()), S * S * P)
        levels.append(lev); curves.append(cur); aucs.append(ar); cals.append((ece, mce, brier))
    return Brute(levels, curves, aucs, cals)


# ================================================================================================ the cases
Case = collections.namedtuple("Case", "name S D H W R_values")
CASES = (Case("one", 1, 1, 1, 1, R_VALUES), Case("subwave", 3, 1, 1, 63, R_VALUES), Case("vec", 4, 2, 3, 64, R_VALUES), Case("odd_p", 16, 3, 5, 67, R_VALUES),
         Case("mid", 5, 9, 17, 70, R_VALUES), Case("s_max", 255, 2, 3, 37, R_VALUES), Case("wg", 2, 1, 1, WG_WIDE, R_VALUES),
         Case("wg_m1", 2, 1, 1, WG_WIDE - 1, R_VALUES), Case("wg_p1", 2, 1, 1, WG_WIDE + 1, R_VALUES))
STRIDE_P = 16 * (CAP * 256 + 1) + 37                 # S = 1, 16-byte aligned: the smallest P whose wide form grid-strides, plus 37 (test_uncertainty_cpu checks it against the route)
STRIDE = Case("stride", 1, 1, 1, STRIDE_P, (1,))
OFFSET_CASES = ("vec", "odd_p", "mid")
OFFSETS = (1, 4, 15)
CONTENTS = ("background", "full", "random", "half", "contra", "blobs_raw", "indices")


def case(name):
    return STRIDE if name == "stride" else next(c for c in CASES if c.name == name)


def _seed(name, content):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name + "/" + content)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def content(name, what):
    """(samples (S, D, H, W), decision (D, H, W), ref (D, H, W)) uint8, read-only, and whether the prediction holds class indices"""
    c = case(name)
    S, shape = c.S, (c.D, c.H, c.W)
    P = c.D * c.H * c.W
    g = np.random.default_rng(_seed(name, what))
    smp, dec, ref = np.zeros((S, P), np.uint8), np.zeros(P, np.uint8), np.zeros(P, np.uint8)
    if what == "full":
        smp[:], dec[:], ref[:] = 4, 4, 4
    elif what in ("random", "indices"):
        vals = np.array([0, 1, 2, 4] if what == "random" else [0, 1, 2, 3], np.uint8)
        smp, dec = vals[g.integers(0, 4, (S, P))], vals[g.integers(0, 4, P)]
        ref = np.array([0, 1, 2, 4], np.uint8)[g.integers(0, 4, P)]
        if what == "random":                                              # values beyond every set: 200, and 36 = 32 + 4
            for arr in (smp.reshape(-1), dec, ref):
                k = max(1, arr.size // 50)
                arr[g.integers(0, arr.size, k)] = 200
                arr[g.integers(0, arr.size, k)] = 36
            smp[-1, -1], dec[-1], ref[-1] = 4, 36, 200                  # the last sample votes at the last voxel
    elif what == "half":                                                  # exactly S // 2 samples vote in the first two thirds
        a, b = P // 3, 2 * P // 3
        smp[:S // 2, :max(b, 1)] = 4
        dec[:max(a, 1)] = 4                                               # the decision takes their side in the first third only
        ref[a // 2:max(a + (b - a) // 4, 1)] = 4
    elif what == "contra":                                                # the decision against the majority, both ways
        a, b = P // 3, 2 * P // 3
        smp[:, :max(a, 1)] = 1
        smp[:S // 2 + 1, a:b] = 4                                         # a bare majority
        dec[a:] = 2
        dec[a + (b - a) // 2:b] = 4
        ref[:max(a // 2, 1)] = 1
        ref[a:b] = 4
    elif what == "blobs_raw":                                             # a nested blob whose rim the samples disagree on
        z, y, x = np.meshgrid(*(np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape), indexing="ij")
        rad = np.sqrt(z * z + y * y + x * x).reshape(P)
        lab = lambda rr: np.where(rr < 0.25, 4, np.where(rr < 0.45, 1, np.where(rr < 0.7, 2, 0))).astype(np.uint8)
        smp = np.stack([lab(rad + 0.12 * g.standard_normal(P) * (s % 3)) for s in range(S)])
        dec, ref = lab(rad + 0.03), lab(rad - 0.04 + 0.05 * g.standard_normal(P))
    elif what != "background":
        raise KeyError(what)
    out = (np.ascontiguousarray(smp.reshape((S,) + shape)), np.ascontiguousarray(dec.reshape(shape)), np.ascontiguousarray(ref.reshape(shape)))
    for arr in out:
        arr.setflags(write=False)
    return out + (what == "indices",)


def region_pair(what_is_index, R):
    """(pred_regions, ref_regions) of a content at R regions"""
    return regions(R, INDEX if what_is_index else BRATS), regions(R, BRATS)


@functools.lru_cache(maxsize=None)
def expected(name, what, R):
    """(votes, table, Derived) of a case, computed once and shared"""
    smp, dec, ref, is_index = content(name, what)
    preg, rreg = region_pair(is_index, R)
    tab = table(smp, dec, ref, preg, rreg)
    tab.setflags(write=False)
    v = votes(smp, preg)
    v.setflags(write=False)
    return v, tab, derive(tab)
