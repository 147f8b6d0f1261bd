"""Shared by tests/test_lesion_hd95_cpu.py and tests/test_lesion_hd95_gpu.py: the numpy / scipy twin of rule 6 of uz_vol_lesion_scores_ex
(the lesion-wise HD95, csrc/vollesion.hip), an independent brute-force restatement, and the case set.

`lesion_hd95` restates the header's contract on tests/_lesions.py (in_set, morph_mask, S26) and tests/_volscore.py (border, edt_sq): the
border of every A_g and B_ng as a mask of its own, exact integer squared distances from scipy's transform, the two order statistics by
sorting, the mean in the kernel's order.  `brute_force_hd95` dilates every lesion on its own, collects the components with np.isin and
calls _volscore.hd95 (MedPy's surface distances restated, numpy.percentile) on the two masks.  The DEFECTS exist only to show that the
cases discriminate."""
import collections
import functools

import numpy as np
from scipy import ndimage

from tests import _lesions as Z
from tests import _volscore as V

PENALTY = 374.0
DEFECTS = ("one_direction", "a_is_dk", "b_clipped", "nearest_any", "first_link_only", "miss_zero", "fp_zero", "dropped_penalised", "nearest_rank",
           "interp_sq", "faces_not_border", "erosion26", "empty_one")
HD_COUNT_NAMES = ("ref_border_over", "entries_over")


def default_max_border(shape):
    """Python's default for a volume D x H x W"""
    P = int(np.prod(shape))
    return min(max(4096, P // 8), P)


def value_of(m, s0, s1):
    """hd95_g from the number of distances and the two order statistics"""
    hq = 0.95 * float(m - 1)
    lo, hi = float(np.sqrt(np.float64(s0))), float(np.sqrt(np.float64(s1)))
    return lo + (hq - float(np.floor(hq))) * (hi - lo)


def percentile_of(s, defects=()):
    """s: sorted int64 squared distances, m >= 1 -> (m, s[k0], s[k1], hd95_g): walk_k's expression"""
    m = len(s)
    hq = 0.95 * float(m - 1)
    k0 = int(np.floor(hq))
    k1 = min(k0 + 1, m - 1)
    value = value_of(m, s[k0], s[k1])
    if "nearest_rank" in defects:
        value = float(np.sqrt(np.float64(s[min(int(np.ceil(0.95 * m)) - 1, m - 1)])))
    if "interp_sq" in defects:
        value = float(np.sqrt(float(s[k0]) + (hq - float(k0)) * (float(s[k1]) - float(s[k0]))))
    return m, int(s[k0]), int(s[k1]), value


def lesion_hd95(pred, ref, pred_regions, ref_regions=None, dilation=3, min_ref_voxels=50, min_pred_voxels=0, max_lesions=256, max_links=4,
                hd95_penalty=PENALTY, max_border=None, defects=(), totals=False):
    """the twin of rule 6: pred (N, D, H, W), ref (D, H, W) uint8 -> hd95 (N, R) float64, hd_lesions (N, R, max_lesions, 3) int64,
    hd_counts (N, R, 2) int64; totals=True adds the list sizes themselves, (N, R, 2) int64"""
    ref_regions = pred_regions if ref_regions is None else ref_regions
    N, R, ML = pred.shape[0], len(pred_regions), max_lesions
    MB = default_max_border(ref.shape) if max_border is None else max_border
    bkw = dict(connectivity=3 if "erosion26" in defects else 1, border_value=1 if "faces_not_border" in defects else 0)
    hd = np.zeros((N, R), np.float64)
    hd_lesions = np.zeros((N, R, ML, 3), np.int64)
    hd_counts = np.zeros((N, R, 2), np.int64)
    sizes = np.zeros((N, R, 2), np.int64)
    for r in range(R):
        G = Z.in_set(ref, ref_regions[r])
        Dk = Z.morph_mask(G[None], 2, dilation, 0)[0]
        Lg, n_ref = ndimage.label(Dk, structure=Z.S26)
        n_tab = min(n_ref, ML)
        gt_vol = np.bincount(Lg[G], minlength=n_ref + 1)[1:]
        cap = np.minimum(Lg - 1, ML)
        kept = gt_vol >= min_ref_voxels
        border_a = [V.border(Dk & (Lg == g + 1) if "a_is_dk" in defects else G & (Lg == g + 1), **bkw) for g in range(n_tab)]
        n_border_a = sum(int(b.sum()) for b in border_a)
        any_a = V.edt_sq(V.border(G, **bkw))
        for n in range(N):
            Pm = Z.in_set(pred[n], pred_regions[r])
            Lp, n_pred = ndimage.label(Pm, structure=Z.S26)
            size = np.bincount(Lp.ravel(), minlength=n_pred + 1)
            both = (Lp > 0) & (Lg > 0)
            links = collections.defaultdict(list)
            if both.any():
                for c, g in np.unique(np.stack([Lp[both], cap[both]]), axis=1).T:          # sorted by component, then lesion
                    links[int(c)].append(int(g))
            over_links = sum(1 for gs in links.values() if len(gs) > max_links)
            n_fp = sum(1 for c in range(1, n_pred + 1) if c not in links and size[c] >= min_pred_voxels)
            any_b = V.edt_sq(V.border(Pm, **bkw))
            take = 1 if "first_link_only" in defects else max_links
            n_entries, per_lesion = 0, {}
            for g in range(n_tab):
                comps = [c for c, gs in links.items() if g in gs[:take]]
                if not comps:
                    continue
                B = np.isin(Lp, comps)
                if "b_clipped" in defects:
                    B = B & (Lg == g + 1)
                bA, bB = border_a[g], V.border(B, **bkw)
                n_entries += int(bB.sum())
                to_a = (any_a if "nearest_any" in defects else V.edt_sq(bA))[bB]
                to_b = (any_b if "nearest_any" in defects else V.edt_sq(bB))[bA]
                s = np.sort(to_a if "one_direction" in defects else np.concatenate([to_a, to_b]))
                per_lesion[g] = percentile_of(s, defects)
            sizes[n, r] = (n_border_a, n_entries)
            hd_counts[n, r] = (max(n_border_a - MB, 0), max(n_entries - MB, 0))
            over = bool(hd_counts[n, r].any())
            n_kept, total = 0, 0.0
            for g in range(n_tab):                                        # ascending g, serially, in fp64: the kernel's order
                if g in per_lesion and not over:
                    hd_lesions[n, r, g] = per_lesion[g][:3]
                if not kept[g]:
                    if "dropped_penalised" in defects:
                        n_kept += 1
                        total += hd95_penalty
                    continue
                n_kept += 1
                if g in per_lesion:
                    total += per_lesion[g][3]
                else:
                    total += 0.0 if "miss_zero" in defects else hd95_penalty
            total += (0.0 if "fp_zero" in defects else hd95_penalty) * float(n_fp)
            if over or n_ref > n_tab or over_links:
                hd[n, r] = np.nan
            else:
                hd[n, r] = total / float(n_kept + n_fp) if n_kept + n_fp else (1.0 if "empty_one" in defects else 0.0)
    return (hd, hd_lesions, hd_counts, sizes) if totals else (hd, hd_lesions, hd_counts)


def brute_force_hd95(pred, ref, pred_regions, ref_regions, dilation, min_ref_voxels, min_pred_voxels, hd95_penalty=PENALTY):
    """The contract restated without the twin's shortcuts and without table limits: the lesions are the groups of reference voxels that
    share a component of the dilated mask, EVERY lesion is dilated on its own (scipy), the components it reaches are collected with
    np.isin, and _volscore.hd95 / surface_distances see the two masks whole.  -> per (n, r): (rows in lesion order - None for a lesion
    without a match, else (m, s[k0], s[k1], hd95_g) -, n_kept, n_fp, the mean)"""
    st18 = ndimage.generate_binary_structure(3, 2)
    dil = lambda m: ndimage.binary_dilation(m, structure=st18, iterations=dilation, border_value=0) if dilation else m
    out = {}
    for r in range(len(pred_regions)):
        G = Z.in_set(ref, ref_regions[r])
        Lg, n_ref = ndimage.label(dil(G), structure=Z.S26)
        for n in range(pred.shape[0]):
            Lp, n_pred = ndimage.label(Z.in_set(pred[n], pred_regions[r]), structure=Z.S26)
            used, rows, terms = set(), [], []
            for g in range(1, n_ref + 1):
                lesion = G & (Lg == g)
                ids = np.unique(Lp[dil(lesion)])
                ids = ids[ids > 0]
                used.update(int(i) for i in ids)
                comp = np.isin(Lp, ids)
                row = None
                if comp.any():
                    d = np.hstack([V.surface_distances(comp, lesion), V.surface_distances(lesion, comp)])
                    s = np.sort(np.rint(d ** 2).astype(np.int64))
                    m, s0, s1, _ = percentile_of(s)
                    row = (m, s0, s1, V.hd95(comp, lesion))
                rows.append(row)
                if int(lesion.sum()) >= min_ref_voxels:
                    terms.append(hd95_penalty if row is None else row[3])
            n_fp = sum(1 for c in range(1, n_pred + 1) if c not in used and int((Lp == c).sum()) >= min_pred_voxels)
            den = len(terms) + n_fp
            out[n, r] = (rows, len(terms), n_fp, (float(np.sum(terms)) + hd95_penalty * n_fp) / den if den else 0.0)
    return out


# ================================================================================================ the cases
HdCase = collections.namedtuple("HdCase", "name pred ref pred_regions ref_regions params")      # params: lesion_hd95's keywords
LABEL_PARAMS = dict(dilation=1, min_ref_voxels=1, min_pred_voxels=0, max_lesions=8, max_links=2)
SINGLE_NAMES = ("ellipsoids_40x48x33", "slabs_3x5x261", "flat_1x17x19", "whole_volume_pred")
OVERFLOW_NAMES = ("entries_exact", "entries_short", "ref_exact", "ref_short")
NAMES = Z.LESION_NAMES + ("labels",) + SINGLE_NAMES + ("plates",) + OVERFLOW_NAMES


def _freeze(c):
    c.pred.setflags(write=False)
    c.ref.setflags(write=False)
    return c


def _with(c, name=None, **over):
    return HdCase(name or c.name, c.pred, c.ref, c.pred_regions, c.ref_regions, dict(dict(c.params, hd95_penalty=PENALTY, max_border=default_max_border(c.ref.shape)), **over))


def _plate(vol, z, y0, count):
    """a one-voxel-thick plate of `count` voxels in slice z from row y0 on: whole rows, then a part of one -> the rows it took"""
    W = vol.shape[2]
    rows = -(-count // W)
    flat = vol[z, y0:y0 + rows].reshape(-1)
    flat[:count] = 1
    vol[z, y0:y0 + rows] = flat.reshape(rows, W)
    return rows


def plates_case(Q, T):
    """Every voxel of a one-voxel-thick plate is on its border.  Four reference plates of T - 1, T, T + 1 and 2 T + 1 voxels in slice 0 -
    four lesions in one volume, so the lesions' stretches of the reference list start inside a tile's width of each other - and in
    slice 2, two slices away (dilation 2 reaches it), predicted plates of Q - 1, Q and Q + 1 voxels, in another order in every row"""
    W, gap = 40, 6
    counts_ref = (T - 1, T, T + 1, 2 * T + 1)
    H = sum(-(-c // W) for c in counts_ref) + gap * len(counts_ref)
    ref = np.zeros((3, H, W), np.uint8)
    pred = np.zeros((3, 3, H, W), np.uint8)
    y = 1
    for g, c in enumerate(counts_ref):
        rows = _plate(ref, 0, y, c)
        for n in range(3):
            _plate(pred[n], 2, y, (Q - 1, Q, Q + 1)[(g + n) % 3])
        y += rows + gap
    return _freeze(HdCase("plates", pred, ref, Z.ONE, Z.ONE, dict(dilation=2, min_ref_voxels=1, min_pred_voxels=0, max_lesions=8, max_links=2, hd95_penalty=PENALTY,
                                                                   max_border=default_max_border(ref.shape))))


@functools.lru_cache(maxsize=None)
def border_sizes(name):
    """(the reference border voxels, the largest entry count of a row) of a one-region lesion case of tests/_lesions.py"""
    c = Z.lesion_case(name)
    sizes = lesion_hd95(c.pred, c.ref, c.pred_regions, c.ref_regions, totals=True, **c.params)[3]
    return int(sizes[0, 0, 0]), int(sizes[:, 0, 1].max())


@functools.lru_cache(maxsize=None)
def cases(Q, T):
    """Q, T: the pair kernel's queries per workgroup and seeds per LDS tile, as uz_vol_lesion_scores_route_ex answers them"""
    cs = [_with(c) for c in Z.lesion_cases()]
    pred, ref = V.label_case()
    cs.append(_with(HdCase("labels", pred, ref, V.BRATS_REGIONS, V.BRATS_REGIONS, LABEL_PARAMS)))
    for name in SINGLE_NAMES:
        m = V.case(name)
        p = dict(LABEL_PARAMS, max_links=4)
        cs.append(_with(_freeze(HdCase(name, m.pred.astype(np.uint8)[None], m.ref.astype(np.uint8), Z.ONE, Z.ONE, p))))
    cs.append(plates_case(Q, T))
    speckle = _with(Z.lesion_case("speckle"))
    n_a, n_e = border_sizes("speckle")
    for name, mb in zip(OVERFLOW_NAMES, (n_e, n_e - 1, n_a, n_a - 1)):
        cs.append(_with(speckle, name, max_border=mb))
    assert tuple(c.name for c in cs) == NAMES
    return tuple(cs)


def case(name, Q, T):
    return next(c for c in cases(Q, T) if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name, Q, T):
    c = case(name, Q, T)
    out = lesion_hd95(c.pred, c.ref, c.pred_regions, c.ref_regions, **c.params)
    for a in out:
        a.setflags(write=False)
    return out


def lesion_params(c):
    """the keywords tests/_lesions.lesion_scores takes"""
    return {k: v for k, v in c.params.items() if k not in ("hd95_penalty", "max_border")}
