"""Volume components without a GPU: the case set of tests/_components.py holds what the GPU test relies on, every deliberate defect of
the twin changes what the cases named here expect, the twin's partition is scipy.ndimage.label's on every case, the twin with the sets
{1}, {2}, {3} is the line-by-line restatement of the reference's keep_largest_connected_components, uz_vol_components_route and the
workspace size claim what the launches use, a bad call is refused with its reason before anything is launched (the library loads, and
refuses, without a device), and the two Python functions check their arguments and assemble a Prediction's rows before any device work."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import _components as K


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


# ================================================================================================ the case set
def test_case_set_holds_what_the_kernels_can_get_wrong():
    assert tuple(c.name for c in K.cases()) == K.NAMES
    shapes = {c.name: c.vol.shape for c in K.cases()}
    assert shapes["u_join"] == (1, 2, 5, 130) and shapes["snake"] == (1, 3, 7, 70) and shapes["wraps"] == (2, 3, 4, 66)
    assert shapes["percolate"] == (3, 9, 17, 70) and shapes["blobs"] == (2, 12, 20, 70) and shapes["flat"] == (2, 1, 33, 67)
    assert shapes["column"] == (1, 17, 9, 1) and shapes["long_row"] == (1, 2, 3, 261) and shapes["rows128"][3] % 64 == 0
    # u_join: the U (two arms of 90 and the joint) against a detached decoy between an arm and the U in size
    lab, sz = K.expected_components("u_join")
    assert sorted(np.unique(sz[lab > 0]).tolist()) == [150, 181] and int(lab[0, 0, 2, 40]) == int(lab[0, 0, 0, 40]) == 41
    # snake: one component through both slices, its root at index 0, and a detached bar
    lab, sz = K.expected_components("snake")
    assert sorted(np.unique(sz[lab > 0]).tolist()) == [50, 2 * (4 * 70 + 3) + 1] and int(lab[0, 2, 6, 69]) == 1
    # tie: two of six and one of three; the first in raster order is the one kept
    lab, sz = K.expected_components("tie")
    assert sorted(sz[lab > 0].tolist()) == [3] * 3 + [6] * 12
    out = K.expected_keep("tie", 0)
    assert out[0, 0, 0, :6].all() and int(out.sum()) == 6
    # diag: nothing of the checkerboard touches by a face; only the domino survives
    lab, sz = K.expected_components("diag")
    assert int(sz.max()) == 2 and int((sz == 1).sum()) == 72
    out = K.expected_keep("diag", 0)
    assert int(out.sum()) == 2 and out[0, 0, 0, 7:9].all()
    # wraps: every pair is two components of 6, the honest largest is 8
    lab, sz = K.expected_components("wraps")
    assert sorted(np.unique(sz[lab > 0]).tolist()) == [6, 8] and int(K.expected_keep("wraps", 0).sum()) == 16
    # percolate: hundreds of components per volume, chains of hundreds of voxels
    lab, sz = K.expected_components("percolate")
    for n in range(3):
        assert len(np.unique(lab[n])) - 1 > 400 and int(sz[n].max()) > 60
    # blobs: all labels and both strays are there, the regions are nested, one threshold sits exactly on an existing size
    v = K.case("blobs").vol
    assert set(np.unique(v)) == {0, 1, 2, 3, 7, 200}
    regions, mv, _ = K.case("blobs").params[2]
    _, sz = K.components(K.in_set(v, regions[1]))
    assert mv[1] in np.unique(sz[0]) and mv[1] < int(sz[0].max())
    for name in ("blobs", "flat", "percolate", "long_row", "rows128", "column"):
        lab, _ = K.expected_components(name)
        assert len(np.unique(lab)) - 1 >= 4, name
    assert K.case("full").vol.all() and not K.case("empty").vol.any() and K.case("single").vol.shape == (1, 1, 1, 1)
    for c in K.cases():
        assert c.vol.size <= 60000 and c.vol.dtype == np.uint8


def test_twin_partition_is_scipy_label_on_every_case():
    for c in K.cases():
        fg = K.in_set(c.vol, c.values)
        lab, sz = K.expected_components(c.name)
        for n in range(c.vol.shape[0]):
            blobs, nb = ndimage.label(fg[n])
            assert nb == len(np.unique(lab[n])) - (1 if (lab[n] == 0).any() else 0), (c.name, n)
            # the same partition: scipy's label and the twin's determine each other
            pairs = np.unique(np.stack([blobs[fg[n]], lab[n][fg[n]]]), axis=1)
            assert pairs.shape[1] == nb, (c.name, n)
            assert np.array_equal(sz[n][fg[n]], np.bincount(blobs.ravel())[blobs[fg[n]]]), (c.name, n)
            # canonical: the label is 1 + the local index of the component's first voxel, which carries it
            first = np.flatnonzero(lab[n].ravel() == np.arange(1, lab[n].size + 1))
            assert len(first) == nb
        assert (lab[~fg] == 0).all() and (sz[~fg] == 0).all()


def test_twin_with_per_label_sets_is_the_reference_function():
    for c in K.cases():
        got = K.keep(c.vol, K.PER_LABEL)
        for n in range(c.vol.shape[0]):
            assert np.array_equal(got[n], K.reference_keep(c.vol[n])), (c.name, n)
            if c.vol.shape[1] == 1:                                      # the 2-D mask, as the 2-D models hand it over
                assert np.array_equal(got[n, 0], K.reference_keep(c.vol[n, 0])), (c.name, n)


# which cases notice which defect (first parameter set of the case unless an index is given)
NOTICED_BY = {"conn18": ("diag", "percolate", "blobs"), "conn26": ("diag", "percolate", "blobs"), "wrap_row": ("wraps",), "wrap_slice": ("wraps",),
              "wrap_volume": ("wraps",), "tie_last": ("tie",), "thr_gt": (("tie", 1), ("blobs", 2)), "forward_scan": ("u_join", "snake", "percolate")}


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_every_defect_changes_what_the_named_cases_expect(defect):
    assert set(NOTICED_BY) == set(K.DEFECTS)
    for item in NOTICED_BY[defect]:
        name, k = item if isinstance(item, tuple) else (item, 0)
        c = K.case(name)
        regions, mv, unl = c.params[k]
        bad = K.keep(c.vol, regions, mv, unl, defects=(defect,))
        assert not np.array_equal(bad, K.expected_keep(name, k)), (defect, name, k)
        if defect not in ("tie_last", "thr_gt"):                         # a defect of the labelling shows in the labels too
            lab, _ = K.components(K.in_set(c.vol, c.values), defects=(defect,))
            assert not np.array_equal(lab, K.expected_components(name)[0]), (defect, name)


# ================================================================================================ route, workspace, refusals
def test_route_claims_and_workspace_sizes():
    L, _ = _lib()
    out = (C.c_int * 2)()
    up16 = lambda b: (b + 15) // 16 * 16
    for N, D, H, W in [(1, 1, 1, 1), (1, 2, 5, 130), (2, 3, 4, 66), (3, 9, 17, 70), (2, 1, 33, 67), (17, 128, 128, 128), (17, 155, 240, 240), (1, 155, 240, 240),
                       (65536, 1, 1, 1)]:
        T, rows, P = N * D * H * W, N * D * H, D * H * W
        assert L.uz_vol_components_route(N, D, H, W, out) == 0, L.uz_last_error()
        widest = max(min(-(-rows // 4), 1 << 16), min(-(-T // 256), 1 << 18), min(N * -(-P // 4096), 1 << 18))
        assert tuple(out) == (0, widest), ((N, D, H, W), tuple(out), widest)
        assert L.uz_vol_components_workspace(N, D, H, W) == up16(8 * N) + 2 * up16(4 * T)
    assert L.uz_vol_components_workspace(17, 155, 240, 240) == 144 + 8 * 17 * 155 * 240 * 240
    for N, D, H, W in [(0, 8, 8, 8), (65537, 1, 1, 1), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (2, 1024, 1024, 1024), (1, 2048, 1024, 1024), (65536, 32768, 1, 1),
                       (65536, 65536, 65536, 65536)]:
        assert L.uz_vol_components_workspace(N, D, H, W) == 0, (N, D, H, W)
        assert L.uz_vol_components_route(N, D, H, W, out) != 0 and L.uz_last_error().decode().startswith("vol_components_route:"), (N, D, H, W)
    assert L.uz_vol_components_workspace(1, 2047, 1024, 1024) > 0          # just below 2^31
    assert L.uz_vol_components_route(1, 8, 8, 8, None) != 0


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written (sets and min_voxels are host arrays by contract)."""
    L, _ = _lib()
    host = np.zeros(8192, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    T = 2 * 8 * 8 * 8
    sets = (C.c_uint32 * 8)(*[0b1110, 0b1100, 0b1000, 2, 2, 2, 2, 2])
    mins = (C.c_int32 * 8)(*[0, 5, 0, 0, 0, 0, 0, 0])
    neg = (C.c_int32 * 8)(*[0, 5, -1, 0, 0, 0, 0, 0])
    sp, mp = C.addressof(sets), C.addressof(mins)

    def label(vol=ptr, N=2, shape=(8, 8, 8), labels=ptr + 4096, sizes=ptr + 16384, ws=ptr + 32768):
        rc = L.uz_vol_label_components(vol, N, *shape, 2, labels, sizes, ws, None)
        return rc, L.uz_last_error().decode()

    def keep(vol=ptr, N=2, shape=(8, 8, 8), s=sp, m=mp, R=3, out=ptr + 4096, ws=ptr + 32768):
        rc = L.uz_vol_keep_components(vol, N, *shape, s, m, R, 0, out, ws, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(vol=None), "null"), (dict(labels=None), "null"), (dict(ws=None), "null"), (dict(shape=(8, 0, 8)), "empty axis"),
                       (dict(shape=(0, 8, 8)), "empty axis"), (dict(shape=(8, 8, 0)), "empty axis"), (dict(N=0), "1 <= N <= 65536"), (dict(N=65537), "1 <= N <= 65536"),
                       (dict(shape=(1024, 1024, 1024)), "2^31"), (dict(ws=ptr + 32768 + 8), "16-byte"), (dict(labels=ptr + 4098), "4-byte"), (dict(sizes=ptr + 16386), "4-byte")]:
        rc, msg = label(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_label_components:"), (kw.keys(), rc, msg)
    for kw, reason in [(dict(vol=None), "null"), (dict(s=None), "null"), (dict(m=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
                       (dict(shape=(8, 0, 8)), "empty axis"), (dict(N=0), "1 <= N <= 65536"), (dict(N=65537), "1 <= N <= 65536"), (dict(shape=(1024, 1024, 1024)), "2^31"),
                       (dict(R=0), "1 <= R <= 8"), (dict(R=9), "1 <= R <= 8"), (dict(m=C.addressof(neg)), "min_voxels[2] is negative"), (dict(ws=ptr + 32768 + 4), "16-byte"),
                       (dict(out=ptr), "overlaps"), (dict(out=ptr + T - 1), "overlaps"), (dict(vol=ptr + 4096, out=ptr + 4096 - T + 1), "overlaps")]:
        rc, msg = keep(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_keep_components:"), (kw.keys(), rc, msg)
    assert not host.any()


# ================================================================================================ the Python functions
def test_argument_errors_of_the_python_functions():
    from unet_zoo_amd import metrics
    vol = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        metrics.label_components(vol.int(), (1,))
    with pytest.raises(TypeError, match="uint8"):
        metrics.label_components(vol.numpy(), (1,))
    with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
        metrics.label_components(vol[0], (1,))
    with pytest.raises(ValueError, match="label value 32"):
        metrics.label_components(vol, (1, 32))
    with pytest.raises(ValueError, match="on the device"):
        metrics.label_components(vol, (1,))
    with pytest.raises(TypeError, match="uint8"):
        metrics.keep_largest_components(vol.float())
    with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
        metrics.keep_largest_components(vol[0])
    with pytest.raises(ValueError, match="label value -1"):
        metrics.keep_largest_components(vol, ((1,), (-1,)))
    with pytest.raises(ValueError, match="unlisted"):
        metrics.keep_largest_components(vol, unlisted="drop")
    with pytest.raises(ValueError, match="2 min_voxels for 3 regions"):
        metrics.keep_largest_components(vol, min_voxels=(1, 2))
    with pytest.raises(ValueError, match=">= 0"):
        metrics.keep_largest_components(vol, min_voxels=-1)
    with pytest.raises(ValueError, match=">= 0"):
        metrics.keep_largest_components(vol, min_voxels=(0, 0, -3))
    with pytest.raises(ValueError, match="on the device"):
        metrics.keep_largest_components(vol)
    _, ffi = _lib()
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.keep_largest_components(vol, tuple((1,) for _ in range(9)))
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.keep_largest_components(vol, ())
    P = collections.namedtuple("P", "labels mean_label")
    with pytest.raises(TypeError, match="uint8"):
        metrics.keep_largest_components(P(torch.zeros(2, 1, 4, 5, 6), torch.zeros(1, 4, 5, 6, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="Prediction expected"):
        metrics.keep_largest_components(P(torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8), torch.zeros(2, 4, 5, 6, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="Prediction expected"):
        metrics.keep_largest_components(P(torch.zeros(2, 3, 5, 6, dtype=torch.uint8), torch.zeros(2, 5, 6, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="on the device"):
        metrics.keep_largest_components(P(torch.zeros(2, 3, 5, 6, dtype=torch.uint8), torch.zeros(3, 5, 6, dtype=torch.uint8)))


def test_prediction_rows_and_the_filtered_prediction_on_cpu_tensors():
    from unet_zoo_amd import metrics
    from unet_zoo_amd.models.phiseg import Prediction
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randint(0, 4, s, generator=g, dtype=torch.uint8)
    soft, mean_soft, entropy, levels = object(), object(), object(), object()
    # PHISeg3D: S samples of one volume, then the mean label
    p3 = Prediction(labels=rnd(3, 1, 4, 5, 6), mean_soft=mean_soft, mean_label=rnd(1, 4, 5, 6), entropy=entropy, levels=levels, soft=soft)
    rows, is_pred = metrics._prediction_rows(p3)
    assert is_pred and rows.shape == (4, 4, 5, 6) and torch.equal(rows[:3], p3.labels[:, 0]) and torch.equal(rows[3:], p3.mean_label)
    q3 = metrics._filtered_prediction(p3, rows + 10)
    assert type(q3) is Prediction and q3.labels.shape == p3.labels.shape and q3.mean_label.shape == p3.mean_label.shape
    assert torch.equal(q3.labels, p3.labels + 10) and torch.equal(q3.mean_label, p3.mean_label + 10)
    assert q3.soft is soft and q3.mean_soft is mean_soft and q3.entropy is entropy and q3.levels is levels
    # a 2-D model: S samples of B images, then B mean labels, each a volume of depth 1
    p2 = Prediction(labels=rnd(3, 2, 5, 6), mean_soft=mean_soft, mean_label=rnd(2, 5, 6), entropy=entropy, levels=levels)
    rows, is_pred = metrics._prediction_rows(p2)
    assert is_pred and rows.shape == (8, 1, 5, 6) and torch.equal(rows[:6, 0], p2.labels.reshape(6, 5, 6)) and torch.equal(rows[6:, 0], p2.mean_label)
    q2 = metrics._filtered_prediction(p2, rows + 10)
    assert torch.equal(q2.labels, p2.labels + 10) and torch.equal(q2.mean_label, p2.mean_label + 10) and q2.soft is None and q2.levels is levels
    # a plain tensor is taken as it is
    t = rnd(2, 4, 5, 6)
    rows, is_pred = metrics._prediction_rows(t)
    assert rows is t and not is_pred


def test_workspace_slots_are_kept_per_owner_and_replaced_when_the_key_changes():
    from unet_zoo_amd import _vol
    cpu = torch.device("cpu")
    a = _vol.workspace("test_owner_a", (cpu, 2, 3), 64, cpu)
    assert a.dtype == torch.uint8 and a.numel() == 64
    assert _vol.workspace("test_owner_a", (cpu, 2, 3), 64, cpu) is a                   # the same key: the same tensor object
    b = _vol.workspace("test_owner_b", (cpu, 2, 3), 32, cpu)
    assert b is not a and b.numel() == 32
    assert _vol.workspace("test_owner_a", (cpu, 2, 3), 64, cpu) is a                   # two owners do not evict each other
    a2 = _vol.workspace("test_owner_a", (cpu, 2, 4), 80, cpu)
    assert a2 is not a and a2.numel() == 80                                            # a new key replaces the slot ...
    assert _vol.workspace("test_owner_a", (cpu, 2, 4), 80, cpu) is a2
    a3 = _vol.workspace("test_owner_a", (cpu, 2, 3), 64, cpu)
    assert a3 is not a and a3 is not a2                                                 # ... for good: one shape at a time
    assert _vol.workspace("test_owner_b", (cpu, 2, 3), 32, cpu) is b
