"""Shared by tests/test_volflip_cpu.py and tests/test_volflip_gpu.py: mirrored passes of PHISeg3D.predict_volume (flips=...;
uz_vol_window_gather_ex / _accum_ex / uz_vol_window_noise, csrc/volwindow.hip).  Built on tests/_volwindow.py: the grid, the blend
tables, the unmirrored gather and evaluation, the rule that says where labels must agree and the gates are imported from there.

A pass with flip mask m (bit 0, 1, 2 = D, H, W) mirrors a window within itself: net-frame voxel n of an axis of extent w at origin o is
window voxel p = w - 1 - n (bit set) or n, volume voxel o + p.  Here that is written per axis as index arrays (_axis), which is also
where the deliberate mistakes of DEFECTS are made; without a defect the three twins equal a composition of the imported pieces with
np.flip (tests/test_volflip_cpu.py checks that), so the definition is stated twice, independently.

Logits are integers / 4 in [-8, 8], independent per (window, mask) pass - the net is not mirror-equivariant, so nothing ties the
passes together - and their fp32 level sums are exact.  An exact tie of a voxel's two largest classes within one pass is a structural
tie where that pass alone covers the voxel (first maximum wins, pinned by _volwindow.must_match); once two passes cover a voxel a tie
of the blended values needs a coincidence of irrational weights.  Volumes and noise fields are a ramp plus noise: no mirror symmetry."""
import collections
import functools

import numpy as np

from tests import _volwindow as VW
from tests._volwindow import EXEMPT_CAP, REL_GAP, blend_tables, evaluate, gates, gather_twin, window_grid  # noqa: F401  (the basis)

STATS_K = (1, 3, 8)
ALL = tuple(range(8))

# as _volwindow.Case, and: flips as predict_volume takes them, the sample count, the weight tables ("gaussian" | "ramp", the latter
# deliberately asymmetric)
Case = collections.namedtuple("Case", "dhw window stride g factors extra c0 flips S blend")

_P3 = ((1, 1), (2, 2), (4, 4))
CASES = [
    Case((8, 12, 16), (8, 12, 16), None, 4, _P3, 0, 0, "all", 2, "ramp"),                       # one window = the volume, three unequal sides, factor 4
    Case((7, 12, 16), (8, 12, 16), None, 4, _P3, 0, 0, (1, 2, 4), 1, "gaussian"),               # overhang on D alone; every single-bit mask
    Case((8, 10, 16), (8, 12, 16), None, 4, _P3, 2, 1, (7,), 3, "ramp"),                        # overhang on H alone; mask 7; channel offset
    Case((8, 12, 13), (8, 12, 16), None, 4, _P3, 0, 0, (4, 1), 2, "gaussian"),                  # overhang on W alone, odd W
    Case((13, 10, 19), (4, 8, 12), (4, 4, 4), 4, _P3, 0, 0, (0, 3, 5), 3, "ramp"),              # 24 windows, overlap, overhang on all axes; mixed subset
    Case((9, 20, 29), (8, 16, 16), (4, 8, 8), 4, ((1, 1), (2, 1), (4, 2)), 3, 2, "all", 2, "gaussian"),   # 12 windows; f and fz differ
    Case((1, 1, 1), (4, 4, 4), None, 4, ((1, 1),), 0, 0, (7, 0), 1, "ramp"),                    # a single voxel: mask 7 reads it at the far corner
]
WINDOW_COUNTS = (1, 1, 1, 1, 24, 12, 1)


def case_id(c):
    return VW.case_id(c) + "-m" + ("all" if c.flips == "all" else "".join(map(str, c.flips)))


def masks_of(flips):
    return ALL if flips == "all" else tuple(flips)


def tables_of(extent, blend):
    """blend_tables, and "ramp": t[i] = 0.25 + 0.75 (i + 1) / w - positive, at most 1 and NOT symmetric, so a weight looked up in
    the net frame instead of in the window shows."""
    if blend == "ramp":
        return [0.25 + 0.75 * (np.arange(w, dtype=np.float64) + 1.0) / w for w in extent]
    return blend_tables(extent, blend)


# ------------------------------------------------------------------------------------------ the mirror, per axis
# name: the twins it changes
DEFECTS = collections.OrderedDict([
    ("mirror_about_volume", ("gather", "accum")),          # volume voxel N - 1 - (o + n) instead of o + w - 1 - n
    ("mirror_about_padded", ("gather", "accum")),          # ... P - 1 - (o + n), P the padded extent
    ("weight_in_net_frame", ("accum",)),                   # weight t[n] instead of t[p]
    ("level_read_mirrored_twice", ("accum",)),             # the level read at the mirror image of the net-frame voxel: the window voxel
    ("overhang_in_net_frame", ("gather", "accum")),        # o + n < N decides instead of o + p < N
    ("noise_not_mirrored", ("noise",)),
    ("noise_mirrored_at_voxel_resolution", ("noise",)),    # element i <- crop element w_voxels - 1 - i instead of d_k - 1 - i
    ("wsum_once_per_window", ("accum",)),
    ("d_w_bits_exchanged", ("gather", "noise", "accum")),
    ("masks_cumulative", ("accum",)),                      # pass j runs with m_0 ^ ... ^ m_j: each mirror applied to the last one's buffer
])


def _bits(m, defect=None):
    b = [(m >> a) & 1 for a in range(3)]
    return b[::-1] if defect == "d_w_bits_exchanged" else b


def effective_masks(masks, defect=None):
    if defect != "masks_cumulative":
        return tuple(masks)
    out, run = [], 0
    for m in masks:
        run ^= m
        out.append(run)
    return tuple(out)


def _axis(w, o, N, P, bit, defect=None):
    """One axis of one pass: for the net-frame indices n = 0 .. w-1 -> (n, p, v) restricted to what the pass touches: p the window
    index (the weight's), v the volume index."""
    n = np.arange(w)
    p = w - 1 - n if bit else n
    v = o + p
    if bit and defect == "mirror_about_volume":
        v = N - 1 - (o + n)
    if bit and defect == "mirror_about_padded":
        v = P - 1 - (o + n)
    ok = (v >= 0) & (v < N)
    if defect == "overhang_in_net_frame":
        ok &= o + n < N
    return n[ok], p[ok], v[ok]


def gather_flip(src, origin, extent, m, defect=None, padded=None):
    """uz_vol_window_gather_ex: src (C, D, H, W) -> (C, wd, wh, ww) in the net frame, zero where the mirrored voxel is beyond the volume."""
    dhw = src.shape[1:]
    padded = dhw if padded is None else padded
    ax = [_axis(w, o, N, P, b, defect) for w, o, N, P, b in zip(extent, origin, dhw, padded, _bits(m, defect))]
    out = np.zeros((src.shape[0], *extent), src.dtype)
    c = np.arange(src.shape[0])
    out[np.ix_(c, ax[0][0], ax[1][0], ax[2][0])] = src[np.ix_(c, ax[0][2], ax[1][2], ax[2][2])]
    return out


def noise_crop(field, origin, crop, m, defect=None, factor=(1, 1, 1)):
    """uz_vol_window_noise: field (C2, d, h, w), origin and crop at the LEVEL's resolution -> (C2, cd, ch, cw): element i of the crop
    feeds net-frame element c - 1 - i on the mirrored axes.  factor: voxels per level element (what the voxel-resolution defect needs)."""
    bits = [0, 0, 0] if defect == "noise_not_mirrored" else _bits(m, defect)
    idx = []
    for c, o, N, b, q in zip(crop, origin, field.shape[1:], bits, factor):
        n = np.arange(c)
        i = (c * q - 1 - n if defect == "noise_mirrored_at_voxel_resolution" else c - 1 - n) if b else n
        idx.append((o + i) % N)
    return field[np.ix_(np.arange(field.shape[0]), *idx)].copy()


def flip_axes(m):
    return tuple(a - 3 for a in range(3) if (m >> a) & 1)


def mirrored(t, m):
    """t (..., D, H, W) mirrored on the axes of m (numpy or torch)."""
    ax = flip_axes(m)
    if not ax:
        return t
    return np.flip(t, ax) if isinstance(t, np.ndarray) else t.flip(ax)


def expanded(origins, masks, pass_levels):
    """The passes as _volwindow.evaluate takes windows: one entry per (window, mask), the origin repeated and the levels mirrored into
    the window's frame - a window's extent is level size x factor, so window voxel p reads the mirrored level at p / factor."""
    xo = [o for o in origins for _ in masks]
    xl = [[mirrored(lv, m) for lv in pass_levels[i][j]] for i in range(len(origins)) for j, m in enumerate(masks)]
    return xo, xl


def evaluate_flips(dhw, extent, origins, masks, tables, factors, pass_levels, S, prec, defect=None, padded=None):
    """Accum over windows x masks in the order of predict_volume(flips=...), then finish; pass_levels[i][j] are the NET-FRAME levels of
    window i under masks[j].  prec and the returned dict as _volwindow.evaluate, whose arithmetic this repeats step by step (so that
    prec = "twin" gives the kernels' bits): fp32 level sums, fp64 max-shifted softmax added in class order, weight (tz ty) tx, product
    and sum rounded separately, one division by the weight sum.  defect: one of DEFECTS that changes "accum"."""
    D, H, W = dhw
    padded = dhw if padded is None else padded
    dt = np.float64 if prec == "twin" else np.longdouble
    K = pass_levels[0][0][0].shape[1]
    wt = ((tables[0].astype(dt)[:, None, None] * tables[1].astype(dt)[None, :, None]) * tables[2].astype(dt)[None, None, :])
    acc, wsum, count = np.zeros((S, K, D, H, W), dt), np.zeros((D, H, W), dt), np.zeros((D, H, W), dt)
    sk = (np.arange(S), np.arange(K))
    for i, o in enumerate(origins):
        for j, m in enumerate(effective_masks(masks, defect)):
            a = VW.summed_logits(pass_levels[i][j], factors, np.float32 if prec == "twin" else np.longdouble).astype(dt)
            e = np.exp(a - a.max(axis=1, keepdims=True))
            se = np.zeros_like(e[:, 0])
            for k in range(K):
                se = se + e[:, k]
            sv = e / se[:, None]
            ax = [_axis(w, q, N, P, b, defect) for w, q, N, P, b in zip(extent, o, dhw, padded, _bits(m, defect))]
            if min(len(x[0]) for x in ax) == 0:
                continue
            read = 1 if defect == "level_read_mirrored_twice" else 0             # which index reads the net's output
            wi = 0 if defect == "weight_in_net_frame" else 1
            vol = np.ix_(*(x[2] for x in ax))
            w_ = wt[np.ix_(*(x[wi] for x in ax))]
            acc[np.ix_(*sk, *(x[2] for x in ax))] += w_ * sv[np.ix_(*sk, *(x[read] for x in ax))]
            if not (defect == "wsum_once_per_window" and j > 0):
                wsum[vol] += w_
            count[vol] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        p = acc / wsum
        mean = np.zeros((K, D, H, W), dt)
        for s in range(S):
            mean = mean + p[s]
        mean = mean / dt(S)
        ent = -np.where(mean > 0, mean * np.log(np.where(mean > 0, mean, 1.0)), 0.0).sum(axis=0)
    out_dt = np.float32 if prec == "twin" else np.float64
    return dict(soft=p.astype(out_dt), labels=np.argmax(acc, axis=1).astype(np.uint8), mean_soft=mean.astype(out_dt),
                mean_label=np.argmax(mean, axis=0).astype(np.uint8), entropy=ent.astype(out_dt), blend=p.astype(np.float64),
                mean=mean.astype(np.float64), count=count.astype(np.int64), acc=acc.astype(np.float64), wsum=wsum.astype(np.float64))


# ------------------------------------------------------------------------------------------ the case set
def ramp_noise(shape, seed):
    """A ramp along every axis plus noise, fp32: no two elements equal, no mirror symmetry."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.float64).reshape(shape) / n - 0.5 + 0.1 * rng.standard_normal(shape)).astype(np.float32)


def pass_logits(c, K):
    """Per window visited, per mask, per level (S, K, d_l, h_l, w_l) fp32: random integers / 4 in [-8, 8], net frame."""
    _, extent, origins = window_grid(c.dhw, c.window, c.stride, c.g)
    rng = np.random.Generator(np.random.PCG64(4001 * K + 17 * c.S + 7919 * int(np.prod(c.dhw)) + len(masks_of(c.flips))))
    return [[[(rng.integers(-32, 33, size=(c.S, K, *VW.level_shape(extent, fac))) / 4.0).astype(np.float32) for fac in c.factors]
             for _ in masks_of(c.flips)] for _ in origins]


@functools.lru_cache(maxsize=None)
def case(i, K):
    """Everything the tests need of CASES[i] with K classes, computed once and shared (read-only)."""
    c = CASES[i]
    padded, extent, origins = window_grid(c.dhw, c.window, c.stride, c.g)
    masks, tables, levels = masks_of(c.flips), tables_of(extent, c.blend), pass_logits(c, K)
    for w in levels:
        for ps in w:
            for lv in ps:
                lv.setflags(write=False)
    args = (c.dhw, extent, origins, masks, tables, c.factors, levels, c.S)
    ref = evaluate_flips(*args, "ref", padded=padded)
    xo, xl = expanded(origins, masks, levels)
    return dict(c=c, padded=padded, extent=extent, origins=origins, masks=masks, tables=tables, levels=levels, args=args, ref=ref,
                twin=evaluate_flips(*args, "twin", padded=padded), xorigins=xo, xlevels=xl,
                pins=VW.must_match(c.dhw, extent, xo, c.factors, xl, c.S, ref))


def all_keys():
    return [(i, K) for i in range(len(CASES)) for K in STATS_K]


def level_geometry(c, padded, extent, origin, fac):
    """A latent level of resize factors fac = (f, fz) as predict_volume cuts its noise: (field size, crop origin, crop extent, voxels per element)."""
    q = (fac[1], fac[0], fac[0])
    return tuple(p // d for p, d in zip(padded, q)), tuple(o // d for o, d in zip(origin, q)), tuple(e // d for e, d in zip(extent, q)), q
