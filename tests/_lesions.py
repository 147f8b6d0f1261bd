"""Shared by tests/test_lesions_cpu.py and tests/test_lesions_gpu.py: the numpy / scipy twins of uz_vol_morph (csrc/volmorph.hip) and
uz_vol_lesion_scores (csrc/vollesion.hip), and the case set.

`morph` restates the stencil of uz_api.h with shifted copies (no scipy: the CPU tier compares it WITH scipy.ndimage.binary_dilation /
binary_erosion); `lesion_scores` restates the five numbered rules of the header's contract on top of `morph` and scipy.ndimage.label,
its finish summing in the kernel's order so that the scores compare bit for bit; `brute_force` is the independent restatement that
dilates every lesion on its own.  The DEFECTS exist only to show that the cases discriminate."""
import collections
import functools

import numpy as np
from scipy import ndimage

MORPH_DEFECTS = ("rows_wrap", "pad_leak", "iter_short")
LESION_DEFECTS = ("dil_structure", "dk6", "pred6", "predvol_in_dk", "pair_twice", "first_lesion_only", "dropped_as_missed", "dropped_fp", "thr_gt",
                  "empty_zero", "inter_dk")
DEFECTS = LESION_DEFECTS + MORPH_DEFECTS
CONN = (1, 2, 3)
ITERATIONS = (0, 1, 2, 3)
WIDTHS = (1, 63, 64, 65, 130, 155)


def region_bits(region):
    return sum(1 << int(v) for v in region)


def in_set(vol, region):
    """bool mask: label value in the set (values >= 32 are in no set)"""
    return np.isin(vol, [v for v in region if 0 <= v < 32])


# ================================================================================================ morphology
def offsets(connectivity, flat):
    """the stencil (dz, dy, dx): at most `connectivity` coordinates differ, each by one; flat (D == 1): no z neighbour"""
    return [(dz, dy, dx) for dz in ((0,) if flat else (-1, 0, 1)) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if abs(dz) + abs(dy) + abs(dx) <= connectivity]


def _shifted(m, dz, dy, dx, outside, defects):
    """r[n, z, y, x] = m[n, z + dz, y + dy, x + dx], 0 beyond the volume; `outside` names the operation ("erode" / "dilate") for the
    defects that depend on it"""
    N, D, H, W = m.shape
    pad_hi = 0
    if "pad_leak" in defects and outside == "erode" and W % 64:
        pad_hi = 1                                                       # the defect: the pad bits of a row's last word read as foreground
    p = np.zeros((N, D + 2, H + 2, W + 2), bool)
    p[:, 1:-1, 1:-1, 1:-1] = m
    p[:, 1:-1, 1:-1, -1] = pad_hi
    if "rows_wrap" in defects and dx:
        # the defect: the x neighbour by flat index arithmetic - the end of a row sees the start of the next one
        q = np.zeros((N, D + 2, H + 2, W), bool)
        q[:, 1:-1, 1:-1, :] = m
        flat = q.reshape(N, -1)
        r = np.zeros_like(flat)
        if dx > 0:
            r[:, :-1] = flat[:, 1:]
        else:
            r[:, 1:] = flat[:, :-1]
        return r.reshape(q.shape)[:, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, :]
    return p[:, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def morph_mask(m, connectivity, iterations, erode, defects=()):
    """m (N, D, H, W) bool -> bool: `iterations` passes of the stencil, a voxel outside the volume reading as 0"""
    if "iter_short" in defects:
        iterations = max(iterations - 1, 0)
    offs = offsets(connectivity, m.shape[1] == 1)
    for _ in range(iterations):
        acc = np.ones(m.shape, bool) if erode else np.zeros(m.shape, bool)
        for dz, dy, dx in offs:
            s = _shifted(m, dz, dy, dx, "erode" if erode else "dilate", defects)
            acc = acc & s if erode else acc | s
        m = acc
    return m


def morph(vol, values, connectivity, iterations, erode, defects=()):
    """the twin of uz_vol_morph: vol (N, D, H, W) uint8 -> 0 / 1 uint8"""
    return morph_mask(in_set(vol, values), connectivity, iterations, erode, defects).astype(np.uint8)


def scipy_morph(vol, values, connectivity, iterations, erode):
    """scipy on every volume; on the 2-D array when D == 1.  iterations == 0 means "until nothing changes" to scipy: the copy is ours"""
    m = in_set(vol, values)
    if iterations == 0:
        return m.astype(np.uint8)
    fn = ndimage.binary_erosion if erode else ndimage.binary_dilation
    out = np.zeros(m.shape, np.uint8)
    for n in range(m.shape[0]):
        if m.shape[1] == 1:
            out[n, 0] = fn(m[n, 0], structure=ndimage.generate_binary_structure(2, min(connectivity, 2)), iterations=iterations, border_value=0)
        else:
            out[n] = fn(m[n], structure=ndimage.generate_binary_structure(3, connectivity), iterations=iterations, border_value=0)
    return out


MorphCase = collections.namedtuple("MorphCase", "name vol values")


def _dense(shape, seed, values=(1, 3), solid_share=0.93):
    """mostly foreground with holes and gaps (an erosion has something to eat, a dilation something to fill), labels 0 .. 3 and strays,
    different content per volume, foreground on every face and in every corner"""
    rng = np.random.default_rng(seed)
    N, D, H, W = shape
    v = rng.choice(np.array([0, 1, 2, 3, 7, 200], np.uint8), size=shape, p=[0.30, 0.25, 0.10, 0.25, 0.05, 0.05])
    for n in range(N):
        box = tuple(slice(rng.integers(0, max(s // 3, 1)), s - rng.integers(0, max(s // 3, 1))) for s in (D, H, W))
        solid = np.zeros((D, H, W), bool)
        solid[box] = rng.random((D, H, W))[box] < solid_share
        v[n][solid] = values[n % len(values)]
        for z in (0, D - 1):
            for y in (0, H - 1):
                for x in (0, W - 1):
                    v[n, z, y, x] = values[0]
        v[n, 0, H // 2:, W // 2:] = values[-1]
        v[n, D - 1, :H // 2 + 1, :W // 2 + 1] = values[0]
        v[n, :, 0, W // 3:] = values[0]
        v[n, :, H - 1, :W // 2 + 1] = values[-1]
        v[n, D // 2:, :, 0] = values[0]
        v[n, :D // 2 + 1, :, W - 1] = values[-1]
    return v


def _sparse(shape, seed, density, values=(1, 3)):
    """scattered foreground (a dilation has room to grow), the corners and one voxel in the middle of every face set, different content per volume"""
    rng = np.random.default_rng(seed)
    N, D, H, W = shape
    v = np.where(rng.random(shape) < density, rng.choice(np.array(values, np.uint8), size=shape), rng.choice(np.array([0, 2, 7, 200], np.uint8), size=shape, p=[0.7, 0.1, 0.1, 0.1]))
    v = v.astype(np.uint8)
    for z in (0, D - 1):
        for y in (0, H - 1):
            for x in (0, W - 1):
                v[:, z, y, x] = values[0]
    v[:, (0, D - 1), H // 2, W // 2] = values[-1]
    v[:, D // 2, (0, H - 1), W // 2] = values[0]
    v[:, D // 2, H // 2, (0, W - 1)] = values[-1]
    return v


@functools.lru_cache(maxsize=None)
def morph_cases():
    cs = [MorphCase("w63", _dense((3, 4, 6, 63), 1), (1, 3)), MorphCase("w155", _dense((1, 5, 9, 155), 2), (1, 3)),
          MorphCase("flat65", _dense((1, 1, 24, 65), 3), (1, 3)), MorphCase("h1_w64", _sparse((3, 3, 1, 64), 4, 0.4), (1, 3)),
          MorphCase("w1", _sparse((1, 6, 7, 1), 5, 0.4), (1, 3)), MorphCase("w130", _dense((1, 3, 5, 130), 6), (1, 3)),
          MorphCase("block", _dense((1, 12, 20, 17), 7, (3,), 0.998), (3,)), MorphCase("line64", _sparse((2, 1, 1, 64), 8, 0.5), (1, 3)),
          MorphCase("sparse65", _sparse((2, 4, 6, 65), 9, 0.01), (1, 3)), MorphCase("sparse155", _sparse((1, 5, 9, 155), 10, 0.004), (1, 3)),
          MorphCase("sparse_flat64", _sparse((1, 1, 24, 64), 11, 0.01), (1, 3)), MorphCase("slab130", _dense((2, 1, 9, 130), 12, (1, 3), 0.995), (1, 3)),
          MorphCase("full", np.full((1, 3, 4, 65), 3, np.uint8), (1, 3)), MorphCase("empty", np.full((1, 3, 4, 65), 2, np.uint8), (1, 3))]
    for c in cs:
        c.vol.setflags(write=False)
    return tuple(cs)


MORPH_NAMES = ("w63", "w155", "flat65", "h1_w64", "w1", "w130", "block", "line64", "sparse65", "sparse155", "sparse_flat64", "slab130", "full", "empty")
MORPH_PARAMS = tuple((c, it, e) for c in CONN for it in ITERATIONS for e in (0, 1))


def morph_case(name):
    return next(c for c in morph_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected_morph(name, connectivity, iterations, erode):
    c = morph_case(name)
    out = morph(c.vol, c.values, connectivity, iterations, erode)
    out.setflags(write=False)
    return out


# ================================================================================================ lesion-wise scores
S26 = np.ones((3, 3, 3), bool)
S6 = ndimage.generate_binary_structure(3, 1)
COUNT_NAMES = ("n_ref", "n_kept", "n_tp", "n_fn", "n_fp", "n_pred", "over_lesions", "over_links")
DEFAULTS = dict(dilation=3, min_ref_voxels=50, min_pred_voxels=0, max_lesions=256, max_links=4)


def lesion_scores(pred, ref, pred_regions, ref_regions=None, dilation=3, min_ref_voxels=50, min_pred_voxels=0, max_lesions=256, max_links=4, defects=()):
    """the twin of uz_vol_lesion_scores: pred (N, D, H, W), ref (D, H, W) uint8 -> counts (N, R, 8) int64, lesions (N, R, max_lesions, 3)
    int64, scores (N, R, 4) float64"""
    ref_regions = pred_regions if ref_regions is None else ref_regions
    N, R, ML = pred.shape[0], len(pred_regions), max_lesions
    counts = np.zeros((N, R, 8), np.int64)
    lesions = np.zeros((N, R, ML, 3), np.int64)
    scores = np.zeros((N, R, 4), np.float64)
    for r in range(R):
        G = in_set(ref, ref_regions[r])
        Dk = morph_mask(G[None], 3 if "dil_structure" in defects else 2, dilation, 0)[0]
        Lg, n_ref = ndimage.label(Dk, structure=S6 if "dk6" in defects else S26)        # numbered by first voxel in C order
        n_tab = min(n_ref, ML)
        gt_vol = np.bincount(Lg[G], minlength=n_ref + 1)[1:]
        cap = np.minimum(Lg - 1, ML)                                      # the compact index, every lesion beyond the table the same one
        kept = gt_vol > min_ref_voxels if "thr_gt" in defects else gt_vol >= min_ref_voxels
        for n in range(N):
            Pm = in_set(pred[n], pred_regions[r])
            Lp, n_pred = ndimage.label(Pm, structure=S6 if "pred6" in defects else S26)
            size = np.bincount(Lp.ravel(), minlength=n_pred + 1)
            both = (Lp > 0) & (Lg > 0)
            links = collections.defaultdict(list)
            if both.any():
                # every (component, lesion) pair once, sorted by component, then lesion
                for c, g in np.unique(np.stack([Lp[both], cap[both]]), axis=1).T:
                    links[int(c)].append(int(g))
            pred_vol = np.zeros(ML + 1, np.int64)
            over_links = 0
            for c, gs in links.items():
                if len(gs) > max_links:
                    over_links += 1
                for g in gs[:1 if "first_lesion_only" in defects else max_links]:
                    add = int(size[c])
                    if "predvol_in_dk" in defects:
                        add = int(((Lp == c) & (cap == g)).sum())
                    if "pair_twice" in defects:                          # once per row (z, y) of the component inside the lesion, not once per pair
                        add *= len(np.unique(np.argwhere((Lp == c) & (cap == g))[:, :2], axis=0))
                    pred_vol[g] += add
            hit = Pm & (Dk if "inter_dk" in defects else G) & (Lg > 0)
            inter = np.bincount(cap[hit], minlength=ML + 1)
            touched = set(links)
            if "dropped_fp" in defects:                                   # the defect: a component that touches dropped lesions only counts as a false positive
                touched = {c for c, gs in links.items() if any(g >= ML or kept[g] for g in gs)}
            n_fp = sum(1 for c in range(1, n_pred + 1) if c not in touched and size[c] >= min_pred_voxels)
            n_kept = n_tp = 0
            total = 0.0
            for g in range(n_tab):                                        # ascending g, serially, in fp64: the kernel's order
                if not kept[g]:
                    if "dropped_as_missed" in defects:
                        n_kept += 1
                    continue
                n_kept += 1
                if pred_vol[g] == 0:
                    continue
                n_tp += 1
                total += float(2 * int(inter[g])) / float(int(gt_vol[g]) + int(pred_vol[g]))
            n_fn = n_kept - n_tp
            counts[n, r] = (n_ref, n_kept, n_tp, n_fn, n_fp, n_pred, n_ref - n_tab, over_links)
            lesions[n, r, :n_tab, 0] = gt_vol[:n_tab]
            lesions[n, r, :n_tab, 1] = inter[:n_tab]
            lesions[n, r, :n_tab, 2] = pred_vol[:n_tab]
            if n_ref > n_tab or over_links:
                scores[n, r] = np.nan
                continue
            empty = 0.0 if "empty_zero" in defects else 1.0
            scores[n, r, 0] = total / float(n_kept + n_fp) if n_kept + n_fp else empty
            scores[n, r, 1] = float(n_tp) / float(n_kept) if n_kept else empty
            scores[n, r, 2] = float(n_tp) / float(n_tp + n_fp) if n_tp + n_fp else empty
            scores[n, r, 3] = float(2 * n_tp) / float(2 * n_tp + n_fn + n_fp) if 2 * n_tp + n_fn + n_fp else empty
    return counts, lesions, scores


def brute_force(pred, ref, pred_regions, ref_regions, dilation, min_ref_voxels, min_pred_voxels):
    """The challenge's description restated without the twin's shortcuts: the lesions are the groups of reference voxels that share a
    component of the dilated mask; EVERY lesion is dilated on its own (scipy), the predicted components it reaches are collected with
    np.isin, and the intersection is taken with those components.  No table limits.  -> per (n, r): (dice list in lesion order,
    n_fp, lesion_dice)"""
    st18 = ndimage.generate_binary_structure(3, 2)
    dil = lambda m: ndimage.binary_dilation(m, structure=st18, iterations=dilation, border_value=0) if dilation else m
    out = {}
    for r in range(len(pred_regions)):
        G = in_set(ref, ref_regions[r])
        Lg, n_ref = ndimage.label(dil(G), structure=S26)
        for n in range(pred.shape[0]):
            Lp, n_pred = ndimage.label(in_set(pred[n], pred_regions[r]), structure=S26)
            used, dices, rows = set(), [], []
            for g in range(1, n_ref + 1):
                lesion = G & (Lg == g)
                ids = np.unique(Lp[dil(lesion)])
                ids = ids[ids > 0]
                used.update(int(i) for i in ids)
                comp = np.isin(Lp, ids)
                gt_vol, pred_vol, inter = int(lesion.sum()), int(comp.sum()), int((lesion & comp).sum())
                rows.append((gt_vol, inter, pred_vol))
                if gt_vol >= min_ref_voxels:
                    dices.append(2.0 * inter / (gt_vol + pred_vol) if pred_vol else 0.0)
            n_fp = sum(1 for c in range(1, n_pred + 1) if c not in used and int((Lp == c).sum()) >= min_pred_voxels)
            mean = float(np.sum(dices)) / (len(dices) + n_fp) if len(dices) + n_fp else 1.0
            out[n, r] = (rows, len(dices), n_fp, mean)
    return out


LesionCase = collections.namedtuple("LesionCase", "name pred ref pred_regions ref_regions params")
ONE = ((1,),)
NESTED_PRED = ((1, 2, 3), (2, 3), (3,))                                   # class indices ...
NESTED_REF = ((1, 2, 4), (1, 4), (4,))                                    # ... against raw BraTS values: WT, TC, ET


def _gaps():
    """pairs of single reference voxels k apart along an axis, a face diagonal and the space diagonal, dilation 1: the 18-neighbour
    dilation just closes the gap at the smaller k of each direction and just fails at the larger one"""
    ref = np.zeros((8, 24, 65), np.uint8)
    pairs = [((0, 0, 1), 3), ((0, 0, 1), 4), ((0, 1, 1), 3), ((0, 1, 1), 4), ((1, 1, 1), 2), ((1, 1, 1), 3)]
    for i, (d, k) in enumerate(pairs):
        z0, y0, x0 = 1, 2 + 8 * (i % 3), 3 + 30 * (i // 3)
        ref[z0, y0, x0] = 1
        ref[z0 + d[0] * k, y0 + d[1] * k, x0 + d[2] * k] = 1
    pred = np.stack([ref, ref])
    pred[1, 1, 2, 3] = 0                                                  # one end of the first pair missed
    pred[1, 6, 22, 60] = 1                                                # and a stray voxel far from every lesion
    return LesionCase("gaps", pred, ref, ONE, ONE, dict(dilation=1, min_ref_voxels=1, min_pred_voxels=0, max_lesions=16, max_links=2))


def _span():
    """two lesions (2 x 2 x 2) that the dilation keeps apart; row 0: one bar through both and beyond; row 1: a U whose ends lie in the
    first lesion's Dk and whose bend lies outside it; row 2: nothing"""
    ref = np.zeros((12, 20, 17), np.uint8)
    ref[4:6, 4:6, 2:4] = 1
    ref[4:6, 4:6, 11:13] = 1
    pred = np.zeros((3, 12, 20, 17), np.uint8)
    pred[0, 4, 4, 0:17] = 1
    pred[0, 4, 4:14, 16] = 1
    pred[1, 4, 4, 3:5] = 1; pred[1, 4, 4:12, 4] = 1; pred[1, 4, 11, 1:5] = 1; pred[1, 4, 5:12, 1] = 1   # leaves Dk at y = 7, x = 4 and comes back at y = 6, x = 1
    pred[1, 10, 15:19, 8:12] = 1                                          # a false positive of 16 voxels
    return LesionCase("span", pred, ref, ONE, ONE, dict(dilation=1, min_ref_voxels=8, min_pred_voxels=0, max_lesions=4, max_links=2))


def _thresholds():
    """lesions of min_ref_voxels - 1 and of min_ref_voxels voxels, lesions on the faces and in a corner, a component that touches only
    the dropped lesion, false positives of min_pred_voxels - 1 and of min_pred_voxels voxels; row 1 misses the lesion on the threshold"""
    ref = np.zeros((5, 9, 155), np.uint8)
    ref[2, 4, 10:15] = 1                                                  # 5 voxels: dropped
    ref[2, 4, 30:36] = 1                                                  # 6 voxels: kept, exactly
    ref[0, 0, 0:4] = 1; ref[0, 1, 0:4] = 1                                # the corner z = y = x = 0
    ref[4, 8, 149:155] = 1; ref[3, 8, 152:155] = 1                        # the opposite corner
    ref[0:5, 4, 80] = 1; ref[0:2, 4, 81] = 1                              # through both z faces
    pred = np.zeros((2, 5, 9, 155), np.uint8)
    for n in range(2):
        pred[n, 2, 5, 12:15] = 1                                          # in the dropped lesion's Dk only, and large enough: still no false positive
        pred[n, 0, 0, 0:3] = 1
        pred[n, 4, 8, 150:155] = 1
        pred[n, 1:4, 4, 80] = 1
        pred[n, 2, 1, 60:62] = 1                                          # 2 voxels far away: below min_pred_voxels
        pred[n, 2, 7, 100:103] = 1                                        # 3 voxels far away: a false positive, exactly
    pred[0, 2, 4, 33:40] = 1
    return LesionCase("thresholds", pred, ref, ONE, ONE, dict(dilation=1, min_ref_voxels=6, min_pred_voxels=3, max_lesions=8, max_links=2))


def _empty_ref():
    pred = np.zeros((2, 3, 1, 64), np.uint8)
    pred[0, 1, 0, 60:64] = 1; pred[0, 0, 0, 0:2] = 1
    return LesionCase("empty_ref", pred, np.zeros((3, 1, 64), np.uint8), ONE, ONE, dict(dilation=2, min_ref_voxels=1, min_pred_voxels=0, max_lesions=4, max_links=1))


def _field(shape, seed, sigma, levels, values):
    f = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    f /= f.std()
    v = np.zeros(shape, np.uint8)
    for lv, val in zip(levels, values):
        v[f > lv] = val
    return v


def _nested():
    """an image (D == 1): smooth nested regions, the prediction's class indices against the reference's raw values"""
    ref = _field((1, 24, 65), 21, (0, 2.0, 2.5), (0.7, 1.2, 1.7), (2, 1, 4))
    pred = np.stack([_field((1, 24, 65), s, (0, 2.0, 2.5), (0.7, 1.2, 1.7), (1, 2, 3)) for s in (21, 22, 23)])
    pred[0, 0, 0:3, 0:3] = 3
    return LesionCase("nested", pred, ref, NESTED_PRED, NESTED_REF, dict(dilation=2, min_ref_voxels=4, min_pred_voxels=2, max_lesions=32, max_links=4))


def _speckle(name, shape, seed, **params):
    rng = np.random.default_rng(seed)
    ref = (rng.random(shape) < 0.012).astype(np.uint8)
    pred = (rng.random((2,) + shape) < 0.02).astype(np.uint8)
    pred[1] |= ref
    p = dict(dilation=1, min_ref_voxels=1, min_pred_voxels=2, max_lesions=512, max_links=8)
    p.update(params)
    return LesionCase(name, pred, ref, ONE, ONE, p)


def _links(name, max_links):
    """one predicted bar through three lesions"""
    ref = np.zeros((3, 5, 130), np.uint8)
    for x in (5, 60, 125):
        ref[1, 2, x:x + 3] = 1
    pred = np.zeros((2, 3, 5, 130), np.uint8)
    pred[0, 1, 2, :] = 1
    pred[1, 1, 2, :64] = 1
    return LesionCase(name, pred, ref, ONE, ONE, dict(dilation=1, min_ref_voxels=1, min_pred_voxels=0, max_lesions=4, max_links=max_links))


@functools.lru_cache(maxsize=None)
def lesion_cases():
    speckle = _speckle("speckle", (6, 10, 130), 31)
    n_ref = int(ndimage.label(morph_mask(in_set(speckle.ref, (1,))[None], 2, 1, 0)[0], structure=S26)[1])
    cs = [_gaps(), _span(), _thresholds(), _empty_ref(), _nested(), speckle,
          _speckle("speckle_exact", (6, 10, 130), 31, max_lesions=n_ref), _speckle("speckle_short", (6, 10, 130), 31, max_lesions=n_ref - 1),
          _speckle("column", (40, 9, 1), 32, dilation=0), _speckle("w63", (4, 7, 63), 33, dilation=2, min_ref_voxels=2),
          _links("links_fit", 3), _links("links_short", 2)]
    for c in cs:
        c.pred.setflags(write=False)
        c.ref.setflags(write=False)
    return tuple(cs)


LESION_NAMES = ("gaps", "span", "thresholds", "empty_ref", "nested", "speckle", "speckle_exact", "speckle_short", "column", "w63", "links_fit", "links_short")


def lesion_case(name):
    return next(c for c in lesion_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected_lesions(name):
    c = lesion_case(name)
    out = lesion_scores(c.pred, c.ref, c.pred_regions, c.ref_regions, **c.params)
    for a in out:
        a.setflags(write=False)
    return out
