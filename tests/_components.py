"""Shared by tests/test_components_cpu.py and tests/test_components_gpu.py: the cases of uz_vol_label_components /
uz_vol_keep_components (csrc/volcomp.hip) and what they expect.

The oracle is a RESTATEMENT, the repository's third (after the cv2 / MedPy twins): the reference's keep_largest_connected_components
(data/BratsProcessing/utils.py:228-251) calls skimage.measure.label and regionprops, skimage is not installed here, so parity with
skimage itself is UNPINNED and no golden vector can be made from the reference.  `components` builds the face-neighbour edge list
with numpy, takes the partition from scipy.sparse.csgraph.connected_components and the canonical label from a minimum.at over the
local linear index; `keep` applies the keep rule of uz_api.h word for word, the tie rule stated explicitly (the smallest canonical
label among the largest components) and not borrowed from scipy's numbering.  `reference_keep` restates the reference function line
by line with scipy.ndimage.label in the place of skimage.measure.label.  The `defects` that are not the rule exist only to show
that the case set discriminates."""
import collections
import functools

import numpy as np
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

DEFECTS = ("conn18", "conn26", "wrap_row", "wrap_slice", "wrap_volume", "tie_last", "thr_gt", "forward_scan")


def region_bits(region):
    return sum(1 << int(v) for v in region)


def in_set(vol, region):
    """bool mask: label value in the set (values >= 32 are in no set)"""
    return np.isin(vol, [v for v in region if 0 <= v < 32])


# ================================================================================================ the oracle
def _edges(fg, defects):
    N, D, H, W = fg.shape
    idx = np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    pairs = []

    def link(a, b):                                                     # two equally shaped views of fg / idx positions
        both = fg[a] & fg[b]
        pairs.append((idx[a][both], idx[b][both]))

    def sl(dz, dy, dx):
        a, b = [slice(None)], [slice(None)]
        for d in (dz, dy, dx):
            a.append(slice(None) if d == 0 else slice(0, -1) if d > 0 else slice(1, None))
            b.append(slice(None) if d == 0 else slice(1, None) if d > 0 else slice(0, -1))
        return tuple(a), tuple(b)

    offs = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    if "conn18" in defects or "conn26" in defects:
        offs += [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
    if "conn26" in defects:
        offs += [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]
    for o in offs:
        link(*sl(*o))
    flat_fg, flat = fg.reshape(N, -1), idx.reshape(N, -1)
    if "wrap_row" in defects:                                            # x = W-1 joins x = 0 of the next row (inside the slice)
        link((slice(None), slice(None), slice(0, -1), W - 1), (slice(None), slice(None), slice(1, None), 0))
    if "wrap_slice" in defects:                                          # the last row of a slice joins the first row of the next slice
        link((slice(None), slice(0, -1), H - 1), (slice(None), slice(1, None), 0))
    if "wrap_volume" in defects and N > 1:                               # the N volumes as one: the last slice and the last voxel join the next volume
        link((slice(0, -1), D - 1), (slice(1, None), 0))
        both = flat_fg[:-1, -1] & flat_fg[1:, 0]
        pairs.append((flat[:-1, -1][both], flat[1:, 0][both]))
    a = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    b = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
    return a, b


def _forward_scan_partition(fg):
    """the defect: one raster scan, a voxel takes the smallest label of its x-1 / y-1 / z-1 neighbours or a new one; joins found late are never resolved"""
    N, D, H, W = fg.shape
    lab = np.zeros(fg.shape, np.int64)
    nxt = 0
    for n, z, y, x in np.argwhere(fg):
        c = [lab[n, z, y, x - 1] if x else 0, lab[n, z, y - 1, x] if y else 0, lab[n, z - 1, y, x] if z else 0]
        c = [v for v in c if v]
        if c:
            lab[n, z, y, x] = min(c)
        else:
            nxt += 1
            lab[n, z, y, x] = nxt
    return lab.reshape(-1) - 1


def components(fg, defects=()):
    """fg (N, D, H, W) bool -> (labels, sizes) int64: labels = 1 + the smallest LOCAL linear index of the voxel's component, 0 on background"""
    N, D, H, W = fg.shape
    T, P = fg.size, D * H * W
    flat = fg.reshape(-1)
    if "forward_scan" in defects:
        comp = _forward_scan_partition(fg)
    else:
        a, b = _edges(fg, defects)
        _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(T, T)), directed=False)
    g = np.flatnonzero(flat)
    first = np.full(int(comp.max()) + 1 if T else 1, T, np.int64)
    np.minimum.at(first, comp[g], g)                                     # the smallest GLOBAL index: its volume is the component's volume
    count = np.bincount(comp[g], minlength=len(first))
    labels, sizes = np.zeros(T, np.int64), np.zeros(T, np.int64)
    labels[g] = first[comp[g]] % P + 1
    sizes[g] = count[comp[g]]
    return labels.reshape(fg.shape), sizes.reshape(fg.shape)


def keep(vol, regions, min_voxels=None, unlisted="zero", defects=()):
    """vol (N, D, H, W) uint8 -> the filtered volumes, by the rule of uz_api.h"""
    N = vol.shape[0]
    P = vol[0].size
    R = len(regions)
    mv = [0] * R if min_voxels is None else [int(min_voxels)] * R if np.isscalar(min_voxels) else [int(m) for m in min_voxels]
    assert len(mv) == R and unlisted in ("zero", "keep")
    listed = np.zeros(vol.shape, bool)
    fails = np.zeros(vol.shape, bool)
    for reg, m in zip(regions, mv):
        fg = in_set(vol, reg)
        listed |= fg
        labels, sizes = components(fg, defects)
        if m >= 1:
            kept = sizes > m if "thr_gt" in defects else sizes >= m
        else:
            kept = np.zeros(vol.shape, bool)
            for n in range(N):
                if not fg[n].any():
                    continue                                             # an empty set keeps and removes nothing
                # a component that a wrap defect spread over two volumes belongs to the volume of its first voxel
                own = labels[n][fg[n]]
                big = sizes[n][fg[n]].max()
                cands = np.unique(own[sizes[n][fg[n]] == big])
                win = cands.max() if "tie_last" in defects else cands.min()
                kept[n] = fg[n] & (labels[n] == win) & (sizes[n] == big)
        fails |= fg & ~kept
    out = np.where(listed & ~fails, vol, 0).astype(np.uint8)
    if unlisted == "keep":
        out = np.where(~listed, vol, out).astype(np.uint8)
    return out


def reference_keep(mask):
    """BratsProcessing/utils.py:228-251 line by line, scipy.ndimage.label (default structure = connectivity 1) for skimage.measure.label;
    regionprops lists the blobs in label order with their voxel counts as areas"""
    out_img = np.zeros(mask.shape, dtype=np.uint8)
    for struc_id in [1, 2, 3]:
        binary_img = mask == struc_id
        blobs, nblobs = ndimage.label(binary_img)
        if not nblobs:
            continue
        area = [int((blobs == k).sum()) for k in range(1, nblobs + 1)]
        largest_blob_ind = np.argmax(area)
        largest_blob_label = largest_blob_ind + 1
        out_img[blobs == largest_blob_label] = struc_id
    return out_img


# ================================================================================================ the cases
# params: the (regions, min_voxels, unlisted) sets the keep call is run with; values: the set the labelling is run with
Case = collections.namedtuple("Case", "name vol values params")
PER_LABEL = ((1,), (2,), (3,))
NESTED = ((1, 2, 3), (2, 3), (3,))
ONE = (((1,),), None, "zero")


def _u_join():
    v = np.zeros((1, 2, 5, 130), np.uint8)
    v[0, 0, 0, 40:] = 1; v[0, 0, 2, 40:] = 1; v[0, 0, 1, 129] = 1        # two arms of 90 that meet only at x = 129: 181 voxels
    v[0, 0, 4, :] = 1; v[0, 1, 4, :20] = 1                               # the decoy, detached: 150 voxels, more than an arm and less than the U
    return v


def _snake():
    v = np.zeros((1, 3, 7, 70), np.uint8)
    for z in (0, 2):
        v[0, z, 0::2, :] = 1
        v[0, z, 1, 69] = 1; v[0, z, 3, 0] = 1; v[0, z, 5, 69] = 1
    v[0, 1, 6, 0] = 1                                                    # the one voxel that joins the two slices
    v[0, 1, 3, 10:60] = 1                                                # a detached bar of 50
    return v


def _tie():
    v = np.zeros((1, 2, 6, 10), np.uint8)
    v[0, 0, 0, :6] = 1; v[0, 0, 2, 2:8] = 1; v[0, 1, 4, :3] = 1
    return v


def _diag():
    v = np.zeros((1, 4, 6, 9), np.uint8)
    z, y, x = np.meshgrid(np.arange(4), np.arange(6), np.arange(6), indexing="ij")
    v[0, :, :, :6] = ((z + y + x) % 2 == 0)
    v[0, 0, 0, 7:9] = 1                                                  # the domino
    return v


def _wraps():
    v = np.zeros((2, 3, 4, 66), np.uint8)
    v[0, 0, 0, 60:] = 1; v[0, 0, 1, :6] = 1                              # the end of a row and the start of the next one: 6 + 6
    v[0, 0, 3, 20:26] = 1; v[0, 1, 0, 20:26] = 1                         # the last row of a slice and the first row of the next one: 6 + 6
    v[0, 2, 3, 60:] = 1; v[1, 0, 0, :6] = 1                              # the last voxels of volume 0 and the first of volume 1: 6 + 6
    v[0, 1, 2, 30:38] = 1; v[1, 1, 2, 30:38] = 1                         # the honest largest: 8
    return v


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _field_labels(shape, seed, sigma, levels):
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint8)
    for n in range(shape[0]):
        f = ndimage.gaussian_filter(rng.standard_normal(shape[1:]), sigma)
        f /= f.std()
        for k, t in enumerate(levels):
            v[n][f > t] = k + 1
    return v


def _blobs():
    v = _field_labels((2, 12, 20, 70), 5, (1.5, 2.0, 2.5), (0.6, 1.2, 1.8))
    for n in range(2):
        z, y, x = np.argwhere(v[n] == 2)[len(np.argwhere(v[n] == 2)) // 2]
        v[n, z, y, x] = 7                                                # a value in no set, and one that is no label at all, inside the tumour
        z, y, x = np.argwhere(v[n] == 1)[len(np.argwhere(v[n] == 1)) // 3]
        v[n, z, y, x] = 200
    return v


def _rows128():
    v = np.zeros((1, 2, 6, 128), np.uint8)
    v[0, :, 4:, :] = _random((2, 2, 128), 0.7, 11)
    v[0, 1, :4, :] = _random((4, 128), 0.3, 12)
    v[0, 0, 0, :] = 1; v[0, 0, 2, 64:] = 1; v[0, 0, 3, 127] = 1          # runs that are still open at the end of a row of two full 64-voxel steps
    return v


@functools.lru_cache(maxsize=None)
def _cases():
    blobs = _blobs()
    # a threshold that sits exactly on the size of an existing component of {2, 3}: the second largest of volume 0
    _, sz = components(in_set(blobs, (2, 3)))
    thr = int(np.unique(sz[0])[-2])
    assert thr >= 2
    single = np.ones((1, 1, 1, 1), np.uint8)
    cs = [
        Case("u_join", _u_join(), (1,), (ONE,)),
        Case("snake", _snake(), (1,), (ONE,)),
        Case("tie", _tie(), (1,), (ONE, (((1,),), (3,), "zero"), (((1,),), (4,), "zero"))),
        Case("diag", _diag(), (1,), (ONE,)),
        Case("wraps", _wraps(), (1,), (ONE,)),
        Case("percolate", _random((3, 9, 17, 70), 0.31, 7), (1,), (ONE, (((1,),), (40,), "keep"))),
        Case("blobs", blobs, (1, 2, 3), ((NESTED, None, "zero"), (PER_LABEL, None, "zero"), (NESTED, (0, thr, 2), "zero"), (NESTED, (0, thr, 2), "keep"),
                                       (PER_LABEL, None, "keep"), (((1, 2, 3),), None, "keep"))),
        Case("flat", _field_labels((2, 1, 33, 67), 3, (0, 1.5, 1.5), (0.4, 1.0, 1.6)), (2, 3), ((PER_LABEL, None, "zero"), (NESTED, (5, 0, 1), "keep"))),
        Case("column", _random((1, 17, 9, 1), 0.6, 2), (1,), (ONE,)),
        Case("long_row", _random((1, 2, 3, 261), 0.8, 4), (1,), (ONE,)),
        Case("rows128", _rows128(), (1,), (ONE,)),
        Case("full", np.ones((2, 3, 4, 5), np.uint8), (1,), (ONE, (PER_LABEL, None, "zero"))),
        Case("empty", np.zeros((2, 3, 4, 5), np.uint8), (1,), (ONE, (PER_LABEL, (0, 1, 2), "keep"))),
        Case("single", single, (1,), (ONE,)),
    ]
    for c in cs:
        c.vol.setflags(write=False)
        assert c.vol.size <= 60000
    return tuple(cs)


def cases():
    return _cases()


NAMES = ("u_join", "snake", "tie", "diag", "wraps", "percolate", "blobs", "flat", "column", "long_row", "rows128", "full", "empty", "single")


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected_components(name):
    """(labels, sizes) int32 of the case's own set; computed once, read-only"""
    c = case(name)
    labels, sizes = components(in_set(c.vol, c.values))
    labels, sizes = labels.astype(np.int32), sizes.astype(np.int32)
    labels.setflags(write=False); sizes.setflags(write=False)
    return labels, sizes


@functools.lru_cache(maxsize=None)
def expected_keep(name, k):
    c = case(name)
    regions, mv, unl = c.params[k]
    out = keep(c.vol, regions, mv, unl)
    out.setflags(write=False)
    return out


def min_voxels_list(mv, R):
    return [0] * R if mv is None else [int(mv)] * R if np.isscalar(mv) else [int(m) for m in mv]
