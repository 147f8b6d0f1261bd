"""Shared by tests/test_morph_cpu.py and tests/test_morph_gpu.py: the twin and the cases of uz_vol_label_components_ex,
uz_vol_keep_components_ex and uz_vol_fill_holes (csrc/volcomp.hip).

The partition at connectivity 1 / 2 / 3 is tests/_components.components with no switch / "conn18" / "conn26" (scipy's
generate_binary_structure(3, c) partition, pinned in the CPU tier); `keep` restates the keep rule of uz_api.h with its relabel clause
and `fill` the hole rule, word for word.  The DEFECTS exist only to show that the cases discriminate: a defective partition is built
by `_scan_components`, which looks from every voxel at its earlier neighbours through flat index arithmetic with guards that a defect
can drop, as the merge kernel does."""
import collections
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import _components as K

LABEL_DEFECTS = ("c2_as_c1", "c2_as_c3", "no_up_row", "left_only", "one_run", "wrap_row", "wrap_slice", "wrap_volume")
FILL_DEFECTS = ("bg_at_fg_conn", "no_z_faces", "d1_as_volume", "max_lt", "chain_sets")
KEEP_DEFECTS = ("chain_sets", "first_remover")
DEFECTS = LABEL_DEFECTS + ("bg_at_fg_conn", "no_z_faces", "d1_as_volume", "max_lt", "chain_sets", "first_remover")
CONN = (1, 2, 3)
_SWITCH = {1: (), 2: ("conn18",), 3: ("conn26",)}


# ================================================================================================ the partition
def _earlier(c):
    """the earlier neighbours (dz, dy, dx) of a voxel: at most c coordinates differ, each by one, and the neighbour comes first in C order"""
    offs = []
    for dz in (-1, 0):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) < (0, 0, 0) and 1 <= abs(dz) + abs(dy) + abs(dx) <= c:
                    offs.append((dz, dy, dx))
    return offs


def _scan_components(fg, c, defects):
    N, D, H, W = fg.shape
    T, HW, P = fg.size, H * W, D * H * W
    flat = fg.reshape(-1)
    q = np.flatnonzero(flat)
    x, y, z = q % W, (q // W) % H, (q // HW) % D
    A, B = [], []
    for dz, dy, dx in _earlier(c):
        if "no_up_row" in defects and (dz, dy) == (-1, 1):
            continue
        if "left_only" in defects and dx == 1:
            continue
        ok = np.ones(len(q), bool)
        if "wrap_row" not in defects or (dz, dy) == (0, 0):
            ok &= (x + dx >= 0) & (x + dx < W)
        if "wrap_slice" not in defects:
            ok &= (y + dy >= 0) & (y + dy < H)
        if "wrap_volume" not in defects:
            ok &= z + dz >= 0
        n = q + dz * HW + dy * W + dx
        ok &= (n >= 0) & (n < T)
        ok[ok] &= flat[n[ok]]
        if "one_run" in defects and dx == 1:                             # the run that begins at x+1, forgotten behind a run that ends at x-1
            drop = ok & (x > 0)
            drop[drop] &= ~flat[n[drop] - 1] & flat[n[drop] - 2]
            ok &= ~drop
        A.append(q[ok]); B.append(n[ok])
    if "wrap_volume" in defects:                                         # and the N volumes as one row of voxels
        first = q[(q % P == 0) & (q > 0)]
        first = first[flat[first - 1]]
        A.append(first); B.append(first - 1)
    a, b = np.concatenate(A), np.concatenate(B)
    _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(T, T)), directed=False)
    head = np.full(int(comp.max()) + 1 if T else 1, T, np.int64)
    np.minimum.at(head, comp[q], q)
    count = np.bincount(comp[q], minlength=len(head))
    labels, sizes = np.zeros(T, np.int64), np.zeros(T, np.int64)
    labels[q] = head[comp[q]] % P + 1
    sizes[q] = count[comp[q]]
    return labels.reshape(fg.shape), sizes.reshape(fg.shape)


def components(fg, connectivity=1, defects=()):
    """fg (N, D, H, W) bool -> (labels, sizes) int64, canonical as tests/_components.components"""
    c = connectivity
    if c == 2 and "c2_as_c1" in defects:
        c = 1
    if c == 2 and "c2_as_c3" in defects:
        c = 3
    if any(d in defects for d in LABEL_DEFECTS[2:]):
        return _scan_components(fg, c, defects)
    return K.components(fg, _SWITCH[c])


def _per_region(v, R):
    return [0] * R if v is None else [int(v)] * R if np.isscalar(v) else [int(m) for m in v]


# ================================================================================================ keep, with relabel
def keep(vol, regions, min_voxels=None, unlisted="zero", connectivity=1, relabel=None, defects=()):
    """uz_vol_keep_components_ex by the header: the sets run in order on the unfiltered input; a set that keeps a voxel writes nothing, a
    set that removes it writes 0 or relabel[r], so the last remover decides"""
    N, R = vol.shape[0], len(regions)
    mv = _per_region(min_voxels, R)
    rl = [-1] * R if relabel is None else [-1 if v is None else int(v) for v in relabel]
    assert len(mv) == R and len(rl) == R and unlisted in ("zero", "keep")
    listed = np.zeros(vol.shape, bool)
    for reg in regions:
        listed |= K.in_set(vol, reg)
    out = np.where(listed | (unlisted == "keep"), vol, 0).astype(np.uint8)
    decided = np.zeros(vol.shape, bool)
    for reg, m, v in zip(regions, mv, rl):
        src = out.copy() if "chain_sets" in defects else vol
        fg = K.in_set(src, reg)
        labels, sizes = components(fg, connectivity, defects)
        if m >= 1:
            kept = sizes >= m
        else:
            kept = np.zeros(vol.shape, bool)
            for n in range(N):
                if fg[n].any():                                          # an empty set keeps and removes nothing
                    big = sizes[n][fg[n]].max()
                    win = labels[n][fg[n] & (sizes[n] == big)].min()     # ties: the smallest canonical label
                    kept[n] = fg[n] & (labels[n] == win)
        removed = fg & ~kept
        if "first_remover" in defects:
            removed &= ~decided
        out[removed] = 0 if v < 0 else v
        decided |= removed
    return out


# ================================================================================================ holes
def fill(vol, regions, fill_values=None, max_voxels=None, connectivity=1, defects=()):
    """uz_vol_fill_holes by the header: per set the complement is labelled at `connectivity`; a component none of whose voxels lies on
    the border (six faces; for D == 1 the four edges) is a hole and becomes the set's value when it is small enough; every set sees vol"""
    N, D, H, W = vol.shape
    R = len(regions)
    fv = [int(tuple(reg)[0]) for reg in regions] if fill_values is None else _per_region(fill_values, R)
    mx = _per_region(max_voxels, R)
    border = np.zeros(vol.shape, bool)
    border[:, :, 0, :] = border[:, :, -1, :] = border[..., 0] = border[..., -1] = True
    if (D > 1 or "d1_as_volume" in defects) and "no_z_faces" not in defects:
        border[:, 0] = border[:, -1] = True
    out = vol.copy()
    for reg, v, m in zip(regions, fv, mx):
        assert v in tuple(reg)
        src = out.copy() if "chain_sets" in defects else vol
        comp = ~K.in_set(src, reg)                                       # a value of 32 or more is in no set, hence in every complement
        labels, sizes = components(comp, 4 - connectivity if "bg_at_fg_conn" in defects else connectivity, defects)
        hole = comp.copy()
        for n in range(N):
            hole[n] &= ~np.isin(labels[n], np.unique(labels[n][border[n] & comp[n]]))
        if m > 0:
            hole &= (sizes < m) if "max_lt" in defects else (sizes <= m)
        out[hole] = v
    return out


# ================================================================================================ the cases
# values: the set the labelling runs with (at every connectivity); keeps: (regions, min_voxels, unlisted, relabel) of the keep call, run
# at every connectivity; fills: (regions, fill_values, max_voxels) of the fill call, run at every connectivity
Case = collections.namedtuple("Case", "name vol values keeps fills")
ONE_KEEP = (((1,),), None, "zero", None)
ONE_FILL = (((1,),), None, None)


def _checker():
    z, y, x = np.meshgrid(np.arange(4), np.arange(5), np.arange(66), indexing="ij")
    return ((x + y + z) % 2 == 0).astype(np.uint8)[None]


def _stairs():
    """one staircase per volume: the four corner diagonals (one component only at c = 3), then the six edge diagonals (from c = 2)"""
    v = np.zeros((10, 5, 5, 7), np.uint8)
    i = np.arange(5)
    for n, (zz, yy, xx) in enumerate([(i, i, i), (i, 4 - i, i), (i, i, 6 - i), (i, 4 - i, 6 - i),
                                      (i, i, 0 * i + 3), (i, 4 - i, 0 * i + 3), (i, 0 * i + 2, i), (i, 0 * i + 2, 6 - i), (0 * i + 2, i, i), (0 * i + 2, i, 6 - i)]):
        v[n, zz, yy, xx] = 1
    return v


def _step64():
    v = np.zeros((1, 3, 6, 130), np.uint8)
    v[0, 0, 0, 10:64] = 1; v[0, 0, 1, 64:100] = 1                        # x = 63 above, x = 64 below: a diagonal contact across the 64-voxel step
    v[0, 0, 3, 64:100] = 1; v[0, 0, 4, 10:64] = 1                        # the mirror image
    v[0, 1, 2, 63] = 1; v[0, 2, 2, 64] = 1                               # the same across slices, single voxels
    v[0, 1, 5, 128] = 1; v[0, 2, 4, 127] = 1; v[0, 2, 5, 129] = 1        # across the step at 128 and at the row's last voxel
    return v


def _row_ends():
    v = np.zeros((1, 3, 6, 66), np.uint8)
    v[0, 0, 0, 65] = 1; v[0, 0, 2, 0] = 1                                # (y-1, x-1) of (2, 0) in flat arithmetic is (0, 65)
    v[0, 0, 4, 65] = 1; v[0, 0, 4, 0] = 1                                # (y-1, x+1) of (4, 65) is (4, 0), its own row's first voxel
    v[0, 1, 1, 65] = 1; v[0, 2, 3, 0] = 1                                # (z-1, y-1, x-1) of (2, 3, 0) is (1, 1, 65)
    v[0, 1, 5, 0] = 1; v[0, 2, 4, 65] = 1                                # (z-1, y+1, x+1) of (2, 4, 65) is (1, 5, 0) + W = ... the next row's start
    v[0, 1, 3, 65] = 1; v[0, 2, 3, 65] = 1                               # an honest pair, so that something joins
    return v


def _slice_ends():
    v = np.zeros((1, 3, 6, 20), np.uint8)
    v[0, 1, 5, 10] = 1; v[0, 1, 0, 10] = 1; v[0, 1, 0, 12] = 1           # (z-1, y+1) of (1, 5, x) is row 0 of slice 1 itself
    v[0, 0, 5, 3] = 1; v[0, 1, 0, 4] = 1                                 # (z, y-1) of (1, 0, x) is the last row of slice 0
    v[0, 1, 5, 17] = 1; v[0, 2, 0, 17] = 1; v[0, 2, 0, 16] = 1           # and of (2, 0, x) the last row of slice 1: 16 and 17 are an honest run
    return v


def _volume_ends():
    v = np.zeros((2, 3, 4, 9), np.uint8)
    v[0, 2, 3, 8] = 1; v[1, 0, 0, 0] = 1                                 # the last voxel of volume 0, the first of volume 1
    v[0, 2, 2, 3] = 1; v[1, 0, 3, 4] = 1                                 # a corner contact if the volumes were stacked
    v[0, 2, 1, 6] = 1; v[1, 0, 1, 6] = 1                                 # a face contact if they were
    v[0, 1, 0, 0] = 1; v[0, 2, 1, 1] = 1                                 # an honest corner contact
    return v


def _two_runs():
    v = np.zeros((1, 3, 8, 40), np.uint8)
    v[0, 0, 0, 10:13] = 1; v[0, 0, 0, 14:17] = 1; v[0, 0, 1, 13] = 1     # one voxel under the gap: its window touches both runs of the row above
    v[0, 0, 3, 20:23] = 1; v[0, 0, 3, 24:27] = 1; v[0, 0, 4, 22:24] = 1  # a run whose second voxel reaches the second run
    v[0, 1, 6, 5:8] = 1; v[0, 1, 6, 9:12] = 1; v[0, 2, 6, 8] = 1         # the same across slices, row y
    v[0, 1, 1, 30:33] = 1; v[0, 1, 1, 34:37] = 1; v[0, 2, 0, 33] = 1     # row (z-1, y+1): one component only at c = 3
    v[0, 1, 3, 30:33] = 1; v[0, 1, 3, 34:37] = 1; v[0, 2, 4, 33] = 1     # row (z-1, y-1)
    return v


def _shells():
    """a 5^3 shell in 7^3 around a 27-voxel cavity: closed; with one EDGE voxel of the shell removed; with one CORNER voxel removed"""
    v = np.zeros((3, 7, 7, 7), np.uint8)
    v[:, 1:6, 1:6, 1:6] = 1
    v[:, 2:5, 2:5, 2:5] = 0
    v[1, 1, 1, 3] = 0
    v[2, 1, 1, 1] = 0
    return v


def _face_contacts():
    """volume 0: a cavity that reaches only the z = 0 face, and a closed one; volume 1: a cavity that reaches only the y = 0 face; volume 2:
    a cavity in the last slice; volume 3: one in the first slice (all of D > 1: no holes), each beside a closed one"""
    v = np.zeros((4, 5, 7, 7), np.uint8)
    v[0, :, 1:6, 1:6] = 1; v[0, 0:2, 3, 3] = 0; v[0, 3, 3, 3] = 0
    v[1, 1:4, :, 1:6] = 1; v[1, 2, 0:2, 3] = 0; v[1, 2, 4, 3] = 0
    v[2, :, 1:6, 1:6] = 1; v[2, 4, 2, 2] = 0; v[2, 2, 4, 4] = 0
    v[3, :, 1:6, 1:6] = 1; v[3, 0, 2, 2] = 0; v[3, 2, 4, 4] = 0
    return v


def _ring_d1():
    v = np.zeros((2, 1, 14, 18), np.uint8)
    v[:, 0, 1:13, 1:17] = 1
    v[0, 0, 2:12, 2:16] = 0                                              # 10 x 14 = 140 inside, in the only slice of volume 0 ...
    v[1, 0, 3:11, 3:15] = 0                                              # ... and 8 x 12 = 96 in the only slice of volume 1
    return v


def _ring_192():
    v = np.zeros((1, 1, 16, 20), np.uint8)
    v[0, 0, 1:15, 1:19] = 1
    v[0, 0, 2:14, 2:18] = 0                                              # 12 x 16 = 192
    return v


def _island():
    """a hole that contains an island that contains a hole"""
    v = np.zeros((1, 11, 11, 11), np.uint8)
    v[0, 1:10, 1:10, 1:10] = 1; v[0, 2:9, 2:9, 2:9] = 0
    v[0, 4:7, 4:7, 4:7] = 1; v[0, 5, 5, 5] = 0
    return v


def _long_hole():
    v = np.ones((1, 3, 3, 140), np.uint8)
    v[0, 1, 1, 3:136] = 0                                                # 133 voxels along x: three 64-voxel steps
    return v


def _sizes():
    """holes of 1, 4 and 27 voxels: max_voxels sits exactly on 4"""
    v = np.zeros((1, 7, 9, 30), np.uint8)
    v[0, 1:6, 1:8, 1:29] = 1
    v[0, 3, 3, 3] = 0; v[0, 3, 3:5, 8:10] = 0; v[0, 2:5, 2:5, 14:17] = 0
    return v


def _strays():
    """a cavity that holds a value in no set and one that is no label at all"""
    v = np.zeros((1, 5, 5, 8), np.uint8)
    v[0, 1:4, 1:4, 1:7] = 1
    v[0, 2, 2, 2:6] = (0, 200, 7, 0)
    return v


def _nested():
    """label 1 around label 2 around a cavity (volume 0); volume 1: a closed shell of 1 around a block of 2 with a cavity in it"""
    v = np.zeros((2, 9, 9, 9), np.uint8)
    v[0, 1:8, 1:8, 1:8] = 1; v[0, 2:7, 2:7, 2:7] = 2; v[0, 3:6, 3:6, 3:6] = 0
    v[1, 1:8, 1:8, 1:8] = 1; v[1, 2:7, 2:7, 2:7] = 2; v[1, 4, 4, 4] = 0
    return v


def _relabel():
    """a small component of 3 and a large one beside a component of 1; a small component of 2"""
    v = np.zeros((1, 4, 8, 20), np.uint8)
    v[0, 1:3, 1:6, 1:6] = 1                                              # 50 voxels of label 1
    v[0, 1, 3, 6:9] = 3                                                  # 3 voxels of label 3 that touch it
    v[0, 1:3, 1:6, 12:18] = 3                                            # 60 voxels of label 3, detached
    v[0, 3, 7, 0:2] = 2                                                  # 2 voxels of label 2
    return v


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _cases():
    cs = []
    for c in K.cases():                                                  # the 14 cases of the face-connected suite, with their own sets
        regions, mv, unl = c.params[0]
        cs.append(Case(c.name, c.vol, c.values, ((regions, mv, unl, None),), ((tuple(r for r in (c.values,)), None, None),)))
    rl = _relabel()
    cs += [
        Case("checker", _checker(), (1,), (ONE_KEEP,), (ONE_FILL,)),
        Case("stairs", _stairs(), (1,), (ONE_KEEP,), ()),
        Case("step64", _step64(), (1,), (ONE_KEEP,), ()),
        Case("row_ends", _row_ends(), (1,), (ONE_KEEP,), ()),
        Case("slice_ends", _slice_ends(), (1,), (ONE_KEEP,), ()),
        Case("volume_ends", _volume_ends(), (1,), (ONE_KEEP,), ()),
        Case("two_runs", _two_runs(), (1,), (ONE_KEEP,), ()),
        Case("h1", _random((2, 6, 1, 67), 0.45, 21), (1,), (ONE_KEEP,), (ONE_FILL,)),
        Case("d1", _random((2, 1, 9, 66), 0.45, 22), (1,), (ONE_KEEP,), (ONE_FILL,)),
        Case("w1", _random((2, 7, 6, 1), 0.45, 23), (1,), (ONE_KEEP,), (ONE_FILL,)),
        Case("rows130", _random((1, 3, 4, 130), 0.4, 24), (1,), (ONE_KEEP, (((1,),), 3, "zero", (9,))), (ONE_FILL,)),
        Case("sponge", _random((2, 6, 9, 67), 0.62, 25), (1,), (ONE_KEEP,), (ONE_FILL, (((1,),), None, 2))),
        Case("dense", _random((2, 6, 9, 67), 0.88, 26), (1,), (ONE_KEEP,), (ONE_FILL, (((1,),), None, 1))),      # holes at every background connectivity
        Case("shells", _shells(), (1,), (), (ONE_FILL,)),
        Case("face_contacts", _face_contacts(), (1,), (), (ONE_FILL,)),
        Case("ring_d1", _ring_d1(), (1,), (), (ONE_FILL, (((1,),), None, 96), (((1,),), None, 139))),
        Case("ring_192", _ring_192(), (1,), (), (ONE_FILL,)),
        Case("island", _island(), (1,), (), (ONE_FILL, (((1,),), None, 1))),
        Case("long_hole", _long_hole(), (1,), (), (ONE_FILL, (((1,),), None, 133), (((1,),), None, 132))),
        Case("sizes", _sizes(), (1,), (), (ONE_FILL, (((1,),), None, 4), (((1,),), None, 1))),
        Case("strays", _strays(), (1,), (), (ONE_FILL, (((1, 2, 3), (1, 7)), (3, 7), None))),
        Case("nested", _nested(), (1, 2), (), ((((1, 2, 3), (2, 3)), None, None), (((2, 3), (1, 2, 3)), None, None), (((1, 2, 3), (1,)), None, (0, 124)),
                                              (((1, 2, 3), (2, 3), (1,)), (1, 3, 1), (0, 27, 0)))),
        # {3} below 5 voxels becomes 1, {2, 3} below 5 voxels becomes 5: the 3 small voxels of 3 are removed twice, the last value stays
        Case("relabel", rl, (1, 3), ((((3,), (2, 3)), (5, 5), "keep", (1, 5)), (((2, 3), (3,)), (5, 5), "keep", (5, 1)),
                                     # {1, 3} keeps (53 >= 53) the voxels that {3} relabelled; {1} alone, 50 < 53, is removed and becomes 2
                                     (((3,), (1, 3)), (5, 53), "keep", (1, 0)), (((3,), (1,)), (5, 53), "zero", (1, 2)),
                                     (((3,), (1,), (2,)), (5, 0, 3), "keep", None), (((3,), (1,), (2,)), (5, 0, 3), "zero", (None, 4, 255))), ()),
    ]
    for c in cs:
        c.vol.setflags(write=False)
        assert c.vol.size <= 33600 and c.vol.dtype == np.uint8, c.name
    return tuple(cs)


def cases():
    return _cases()


NAMES = K.NAMES + ("checker", "stairs", "step64", "row_ends", "slice_ends", "volume_ends", "two_runs", "h1", "d1", "w1", "rows130", "sponge", "dense", "shells",
                   "face_contacts", "ring_d1", "ring_192", "island", "long_hole", "sizes", "strays", "nested", "relabel")


def case(name):
    return next(c for c in cases() if c.name == name)


KEEP_IDS = tuple((n, k) for n in NAMES for k in range(len(case(n).keeps)))
FILL_IDS = tuple((n, k) for n in NAMES for k in range(len(case(n).fills)))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def expected_components(name, c):
    """(labels, sizes) int32 of the case's own set at connectivity c; computed once, read-only"""
    cs = case(name)
    labels, sizes = components(K.in_set(cs.vol, cs.values), c)
    return _frozen(labels.astype(np.int32), sizes.astype(np.int32))


@functools.lru_cache(maxsize=None)
def expected_keep(name, k, c):
    cs = case(name)
    regions, mv, unl, rl = cs.keeps[k]
    return _frozen(keep(cs.vol, regions, mv, unl, c, rl))


@functools.lru_cache(maxsize=None)
def expected_fill(name, k, c):
    cs = case(name)
    regions, fv, mx = cs.fills[k]
    return _frozen(fill(cs.vol, regions, fv, mx, c))
