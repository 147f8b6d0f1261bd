"""18- / 26-connectivity, relabelling and hole filling without a GPU: the cases of tests/_morph.py hold what the GPU tier relies on, the
twin's partition is scipy.ndimage.label's at every connectivity and its fill is scipy.ndimage.binary_fill_holes' on every case, every
deliberate defect of the twin changes what the cases named here expect, uz_vol_components_route_ex and the workspace claim what the
launches use, a bad call is refused with its reason before anything is launched (the library loads, and refuses, without a device),
and the three Python functions check their new arguments and choose their entry point before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import _components as K
from tests import _morph as M


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


def _ncomp(lab):
    return sum(len(np.unique(v[v > 0])) for v in lab)


# ================================================================================================ the case set
def test_case_set_holds_what_the_new_code_can_get_wrong():
    assert tuple(c.name for c in M.cases()) == M.NAMES and M.NAMES[:14] == K.NAMES
    for c in M.cases():
        assert c.vol.size <= 33600 and c.vol.dtype == np.uint8
    shapes = {c.name: c.vol.shape for c in M.cases()}
    assert shapes["checker"][3] == 66 and shapes["step64"][3] == 130 and shapes["rows130"][3] == 130 and shapes["sponge"][3] == 67
    assert shapes["h1"][2] == 1 and shapes["d1"][1] == 1 and shapes["w1"][3] == 1 and shapes["long_hole"][3] > 128
    comps = lambda name: tuple(_ncomp(M.expected_components(name, c)[0]) for c in M.CONN)
    assert comps("checker") == (660, 1, 1)
    # stairs: 5 voxels per volume; the four corner staircases are one component only at c = 3, the six edge staircases from c = 2
    assert comps("stairs") == (50, 4 * 5 + 6, 10)
    # step64: four runs and five voxels; the pairs join from c = 2, at c = 3 the voxel (1, 2, 63) also bridges the two pairs of runs
    assert comps("step64") == (9, 5, 2) and comps("row_ends") == (8, 5, 5) and comps("slice_ends") == (7, 7, 7) and comps("volume_ends") == (8, 8, 7)
    assert comps("two_runs") == (14, 9, 5)
    # shells: what scipy.ndimage.binary_fill_holes fills at background connectivity 1 / 2 / 3: closed, an edge voxel open, a corner voxel open
    filled = lambda name, k, c: [int((M.expected_fill(name, k, c)[n] != M.case(name).vol[n]).sum()) for n in range(M.case(name).vol.shape[0])]
    assert [filled("shells", 0, c) for c in M.CONN] == [[27, 27, 27], [27, 0, 27], [27, 0, 0]]
    assert filled("face_contacts", 0, 1) == [1, 1, 1, 1] and filled("ring_192", 0, 1) == [192] and filled("ring_d1", 0, 1) == [140, 96]
    assert filled("ring_d1", 1, 1) == [0, 96] and filled("ring_d1", 2, 1) == [0, 96]
    assert filled("island", 0, 1) == [7 ** 3 - 27 + 1] and filled("island", 1, 1) == [1]
    assert filled("long_hole", 0, 1) == [133] and filled("long_hole", 1, 1) == [133] and filled("long_hole", 2, 1) == [0]
    assert filled("sizes", 0, 1) == [32] and filled("sizes", 1, 1) == [5] and filled("sizes", 2, 1) == [1]
    assert filled("full", 0, 1) == [0, 0] and filled("empty", 0, 1) == [0, 0]
    assert M.expected_fill("strays", 0, 1)[0, 2, 2, 2:6].tolist() == [1, 1, 1, 1] and M.expected_fill("strays", 1, 1)[0, 2, 2, 2:6].tolist() == [7, 7, 3, 7]
    # nested: the last set wins where the holes of two sets overlap
    assert int(M.expected_fill("nested", 0, 1)[0, 4, 4, 4]) == 2 and int(M.expected_fill("nested", 1, 1)[0, 4, 4, 4]) == 1
    # relabel: the last remover decides; a set that keeps a relabelled voxel leaves it; all None is the plain filter
    v = M.case("relabel").vol
    assert M.expected_keep("relabel", 0, 1)[0, 1, 3, 6:9].tolist() == [5, 5, 5] and M.expected_keep("relabel", 1, 1)[0, 1, 3, 6:9].tolist() == [1, 1, 1]
    out = M.expected_keep("relabel", 2, 1)
    assert out[0, 1, 3, 6:9].tolist() == [1, 1, 1] and int((out == 1).sum()) == 53 and int((out == 3).sum()) == 60 and int((out == 2).sum()) == 2
    out = M.expected_keep("relabel", 3, 1)
    assert int((out == 2).sum()) == 50 and out[0, 1, 3, 6:9].tolist() == [1, 1, 1]
    assert np.array_equal(M.expected_keep("relabel", 4, 1), K.keep(v, ((3,), (1,), (2,)), (5, 0, 3), "keep"))
    assert sorted(np.unique(M.expected_keep("relabel", 5, 1)).tolist()) == [0, 1, 3, 255]


def test_twin_without_the_new_arguments_is_the_face_connected_twin():
    for c in K.cases():
        for k, (regions, mv, unl) in enumerate(c.params):
            assert np.array_equal(M.keep(c.vol, regions, mv, unl), K.expected_keep(c.name, k)), (c.name, k)
            assert np.array_equal(M.keep(c.vol, regions, mv, unl, 1, [-1] * len(regions)), K.expected_keep(c.name, k)), (c.name, k)
        for got, want in zip(M.expected_components(c.name, 1), K.expected_components(c.name)):
            assert np.array_equal(got, want)
    # and the scan that carries the defects is, without one, the same partition
    for c in M.cases():
        for conn in M.CONN:
            lab, sz = M._scan_components(K.in_set(c.vol, c.values), conn, ())
            assert np.array_equal(lab, M.expected_components(c.name, conn)[0]) and np.array_equal(sz, M.expected_components(c.name, conn)[1]), (c.name, conn)


def _same_partition(blobs, nb, lab, sz, fg):
    assert nb == len(np.unique(lab[fg]))
    pairs = np.unique(np.stack([blobs[fg], lab[fg]]), axis=1)
    assert pairs.shape[1] == nb
    assert np.array_equal(sz[fg], np.bincount(blobs.ravel())[blobs[fg]])


@pytest.mark.parametrize("conn", M.CONN)
def test_twin_partition_is_scipy_label_at_every_connectivity(conn):
    for c in M.cases():
        fg = K.in_set(c.vol, c.values)
        lab, sz = M.expected_components(c.name, conn)
        for n in range(c.vol.shape[0]):
            blobs, nb = ndimage.label(fg[n], structure=ndimage.generate_binary_structure(3, conn))
            _same_partition(blobs, nb, lab[n], sz[n], fg[n])
            if c.vol.shape[1] == 1:                                      # the image, as a 2-D model hands it over
                blobs, nb = ndimage.label(fg[n, 0], structure=ndimage.generate_binary_structure(2, min(conn, 2)))
                _same_partition(blobs, nb, lab[n, 0], sz[n, 0], fg[n, 0])
        assert (lab[~fg] == 0).all() and (sz[~fg] == 0).all()


@pytest.mark.parametrize("conn", M.CONN)
def test_twin_fill_is_scipy_binary_fill_holes_on_every_case(conn):
    for c in M.cases():
        reg = tuple(c.values)
        out = M.fill(c.vol, (reg,), None, None, conn)
        for n in range(c.vol.shape[0]):
            fg = K.in_set(c.vol[n], reg)
            if c.vol.shape[1] == 1:                                      # D == 1 goes to scipy as the image it is
                want = ndimage.binary_fill_holes(fg[0], structure=ndimage.generate_binary_structure(2, min(conn, 2)))[None]
            else:
                want = ndimage.binary_fill_holes(fg, structure=ndimage.generate_binary_structure(3, conn))
            assert np.array_equal(K.in_set(out[n], reg), want), (c.name, n)
            assert np.array_equal(out[n][~(want & ~fg)], c.vol[n][~(want & ~fg)]) and (out[n][want & ~fg] == reg[0]).all(), (c.name, n)
    if conn == 1:                                                        # scipy on the (1, H, W) array fills nothing: the reason for the D == 1 rule
        ring = M.case("ring_192").vol[0] == 1
        assert int(ndimage.binary_fill_holes(ring).sum() - ring.sum()) == 0 and int(ndimage.binary_fill_holes(ring[0]).sum() - ring.sum()) == 192


# which (case, connectivity) the labelling notices a defect at; which (case, parameter set, connectivity) the fill and the keep do
LABEL_NOTICED_BY = {"c2_as_c1": (("checker", 2), ("stairs", 2), ("two_runs", 2), ("step64", 2)), "c2_as_c3": (("stairs", 2), ("two_runs", 2), ("volume_ends", 2)),
                    "no_up_row": (("stairs", 2), ("stairs", 3), ("two_runs", 3)), "left_only": (("stairs", 2), ("stairs", 3), ("step64", 2), ("step64", 3)),
                    "one_run": (("two_runs", 2), ("two_runs", 3)), "wrap_row": (("row_ends", 2), ("row_ends", 3)), "wrap_slice": (("slice_ends", 2), ("slice_ends", 3)),
                    "wrap_volume": (("volume_ends", 2), ("volume_ends", 3))}
FILL_NOTICED_BY = {"bg_at_fg_conn": (("shells", 0, 1), ("shells", 0, 3)), "no_z_faces": (("face_contacts", 0, 1),), "d1_as_volume": (("ring_d1", 0, 1), ("ring_192", 0, 2)),
                   "max_lt": (("sizes", 1, 1), ("long_hole", 1, 1), ("ring_d1", 1, 3)), "chain_sets": (("nested", 2, 1),)}
KEEP_NOTICED_BY = {"chain_sets": (("relabel", 3, 1),), "first_remover": (("relabel", 0, 1), ("relabel", 1, 2))}


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_defect_changes_what_the_named_cases_expect(defect):
    assert set(LABEL_NOTICED_BY) == set(M.LABEL_DEFECTS) and set(FILL_NOTICED_BY) == set(M.FILL_DEFECTS) and set(KEEP_NOTICED_BY) == set(M.KEEP_DEFECTS)
    assert set(M.DEFECTS) == set(M.LABEL_DEFECTS) | set(M.FILL_DEFECTS) | set(M.KEEP_DEFECTS)
    keeps_differ = []
    for name, conn in LABEL_NOTICED_BY.get(defect, ()):
        c = M.case(name)
        lab, _ = M.components(K.in_set(c.vol, c.values), conn, (defect,))
        assert not np.array_equal(lab, M.expected_components(name, conn)[0]), (defect, name, conn)
        regions, mv, unl, rl = c.keeps[0]
        keeps_differ.append(not np.array_equal(M.keep(c.vol, regions, mv, unl, conn, rl, (defect,)), M.expected_keep(name, 0, conn)))
    assert defect not in LABEL_NOTICED_BY or any(keeps_differ), defect       # a defect of the labelling shows in what is kept, too
    for name, k, conn in FILL_NOTICED_BY.get(defect, ()):
        regions, fv, mx = M.case(name).fills[k]
        assert not np.array_equal(M.fill(M.case(name).vol, regions, fv, mx, conn, (defect,)), M.expected_fill(name, k, conn)), (defect, name, k, conn)
    for name, k, conn in KEEP_NOTICED_BY.get(defect, ()):
        regions, mv, unl, rl = M.case(name).keeps[k]
        assert not np.array_equal(M.keep(M.case(name).vol, regions, mv, unl, conn, rl, (defect,)), M.expected_keep(name, k, conn)), (defect, name, k, conn)


# ================================================================================================ route, workspace, refusals
def test_route_ex_claims_and_the_workspace_is_the_old_one():
    L, _ = _lib()
    out, old = (C.c_int * 2)(), (C.c_int * 2)()
    for N, D, H, W in [(1, 1, 1, 1), (1, 3, 6, 130), (3, 7, 7, 7), (2, 1, 14, 18), (17, 128, 128, 128), (17, 155, 240, 240), (65536, 1, 1, 1)]:
        T, rows, P = N * D * H * W, N * D * H, D * H * W
        widest = max(min(-(-rows // 4), 1 << 16), min(-(-T // 256), 1 << 18), min(N * -(-P // 4096), 1 << 18))
        assert L.uz_vol_components_route(N, D, H, W, old) == 0 and tuple(old) == (0, widest)
        for conn in M.CONN:
            assert L.uz_vol_components_route_ex(N, D, H, W, conn, out) == 0, L.uz_last_error()
            assert tuple(out) == (conn, widest), ((N, D, H, W), conn, tuple(out))
    for args in [(0, 8, 8, 8, 1), (65537, 1, 1, 1, 2), (1, 0, 8, 8, 3), (2, 1024, 1024, 1024, 1), (1, 8, 8, 8, 0), (1, 8, 8, 8, 4), (1, 8, 8, 8, -1)]:
        assert L.uz_vol_components_route_ex(*args, out) != 0 and L.uz_last_error().decode().startswith("vol_components_route_ex:"), args
    assert L.uz_vol_components_route_ex(1, 8, 8, 8, 2, None) != 0 and L.uz_last_error().decode().startswith("vol_components_route_ex:")
    # none of the new calls has a workspace of its own: the header hands them uz_vol_components_workspace
    assert not any(hasattr(L, n) for n in ("uz_vol_fill_holes_workspace", "uz_vol_components_workspace_ex"))


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written (sets, min_voxels, relabel, fill_values and
    max_voxels are host arrays by contract)."""
    L, _ = _lib()
    host = np.zeros(8192, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    T = 2 * 8 * 8 * 8
    arr = lambda t, *v: (t * 8)(*(list(v) + [v[-1]] * (8 - len(v))))
    sets, mins, neg = arr(C.c_uint32, 0b1110, 0b1100, 0b1000, 2), arr(C.c_int32, 0, 5, 0), arr(C.c_int32, 0, 5, -1, 0)
    rel, rel_lo, rel_hi = arr(C.c_int32, -1, 255, 0), arr(C.c_int32, -1, -2, 0), arr(C.c_int32, -1, 0, 256, 0)
    fv, fv_out, fv_neg, fv_32 = arr(C.c_int32, 1, 2, 3, 1), arr(C.c_int32, 1, 1, 3, 1), arr(C.c_int32, -1, 2, 3, 1), arr(C.c_int32, 1, 2, 35, 1)
    a = C.addressof

    def label(vol=ptr, N=2, shape=(8, 8, 8), conn=2, labels=ptr + 4096, sizes=ptr + 16384, ws=ptr + 32768):
        rc = L.uz_vol_label_components_ex(vol, N, *shape, 2, conn, labels, sizes, ws, None)
        return rc, L.uz_last_error().decode()

    def keep(vol=ptr, N=2, shape=(8, 8, 8), s=a(sets), m=a(mins), rl=a(rel), R=3, conn=3, out=ptr + 4096, ws=ptr + 32768):
        rc = L.uz_vol_keep_components_ex(vol, N, *shape, s, m, rl, R, conn, 0, out, ws, None)
        return rc, L.uz_last_error().decode()

    def fill(vol=ptr, N=2, shape=(8, 8, 8), s=a(sets), f=a(fv), m=a(mins), R=3, conn=1, out=ptr + 4096, ws=ptr + 32768):
        rc = L.uz_vol_fill_holes(vol, N, *shape, s, f, m, R, conn, out, ws, None)
        return rc, L.uz_last_error().decode()

    sizes = [(dict(shape=(8, 0, 8)), "empty axis"), (dict(shape=(0, 8, 8)), "empty axis"), (dict(shape=(8, 8, 0)), "empty axis"), (dict(N=0), "1 <= N <= 65536"),
             (dict(N=65537), "1 <= N <= 65536"), (dict(shape=(1024, 1024, 1024)), "2^31")]
    conns = [(dict(conn=0), "connectivity 0"), (dict(conn=4), "connectivity 4"), (dict(conn=-1), "connectivity -1")]
    sets_ = [(dict(R=0), "1 <= R <= 8"), (dict(R=9), "1 <= R <= 8"), (dict(m=a(neg)), "[2] is negative"), (dict(ws=ptr + 32768 + 4), "16-byte"),
             (dict(out=ptr), "overlaps"), (dict(out=ptr + T - 1), "overlaps"), (dict(vol=ptr + 4096, out=ptr + 4096 - T + 1), "overlaps")]
    for kw, reason in [(dict(vol=None), "null"), (dict(labels=None), "null"), (dict(ws=None), "null"), (dict(ws=ptr + 32768 + 8), "16-byte"), (dict(labels=ptr + 4098), "4-byte"),
                       (dict(sizes=ptr + 16386), "4-byte")] + sizes + conns:
        rc, msg = label(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_label_components_ex:"), (kw.keys(), rc, msg)
    for kw, reason in [(dict(vol=None), "null"), (dict(s=None), "null"), (dict(m=None), "null"), (dict(rl=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
                       (dict(rl=a(rel_lo)), "relabel[1] = -2"), (dict(rl=a(rel_hi)), "relabel[2] = 256")] + sizes + conns + sets_:
        rc, msg = keep(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_keep_components_ex:"), (kw.keys(), rc, msg)
    for kw, reason in [(dict(vol=None), "null"), (dict(s=None), "null"), (dict(f=None), "null"), (dict(m=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
                       (dict(f=a(fv_out)), "fill_values[1] = 1 is no member"), (dict(f=a(fv_neg)), "fill_values[0] = -1 is no member"),
                       (dict(f=a(fv_32)), "fill_values[2] = 35 is no member")] + sizes + conns + sets_:
        rc, msg = fill(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_fill_holes:"), (kw.keys(), rc, msg)
    assert keep(R=4, rl=a(rel_hi))[0] != 0 and fill(R=4, m=a(neg))[0] != 0     # entries behind R are not read: these fail at index 2
    assert not host.any()


# ================================================================================================ the Python functions
def test_argument_errors_of_the_new_keywords():
    from unet_zoo_amd import metrics
    vol = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    for fn, args in ((metrics.label_components, (vol, (1,))), (metrics.keep_largest_components, (vol,)), (metrics.fill_holes, (vol,))):
        for bad in (0, 4, -1):
            with pytest.raises(ValueError, match="connectivity"):
                fn(*args, connectivity=bad)
        for bad in (2.0, "2", None, True):
            with pytest.raises(TypeError, match="connectivity"):
                fn(*args, connectivity=bad)
        with pytest.raises(ValueError, match="on the device"):           # a good value gets as far as the old checks
            fn(*args, connectivity=3)
    with pytest.raises(ValueError, match="2 relabel entries for 3 regions"):
        metrics.keep_largest_components(vol, relabel=(1, 2))
    with pytest.raises(TypeError, match="None or an int"):
        metrics.keep_largest_components(vol, relabel=(1, 2.0, None))
    with pytest.raises(TypeError, match="None or an int"):
        metrics.keep_largest_components(vol, relabel=(1, "1", None))
    with pytest.raises(ValueError, match="0 .. 255"):
        metrics.keep_largest_components(vol, relabel=(1, 256, None))
    with pytest.raises(ValueError, match="0 .. 255"):
        metrics.keep_largest_components(vol, relabel=(-1, 2, None))
    with pytest.raises(ValueError, match="on the device"):
        metrics.keep_largest_components(vol, relabel=(None, 0, 255))
    # the existing errors come first, in their order
    with pytest.raises(ValueError, match="unlisted"):
        metrics.keep_largest_components(vol, unlisted="drop", connectivity=7, relabel=(1,))
    with pytest.raises(ValueError, match=">= 0"):
        metrics.keep_largest_components(vol, min_voxels=-1, connectivity=7)
    with pytest.raises(TypeError, match="uint8"):
        metrics.fill_holes(vol.float())
    with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
        metrics.fill_holes(vol[0])
    with pytest.raises(ValueError, match="label value 32"):
        metrics.fill_holes(vol, ((1, 32),))
    with pytest.raises(ValueError, match="fill value 4 is no member"):
        metrics.fill_holes(vol, ((1, 2, 3), (2, 3)), fill=(1, 4))
    with pytest.raises(ValueError, match="fill value 1 is no member"):
        metrics.fill_holes(vol, ((1, 2, 3), (2, 3)), fill=1)
    with pytest.raises(ValueError, match="1 fill values for 2 regions"):
        metrics.fill_holes(vol, ((1, 2, 3), (2, 3)), fill=(1,))
    with pytest.raises(ValueError, match="empty region"):
        metrics.fill_holes(vol, ((1,), ()))
    with pytest.raises(ValueError, match="3 max_voxels for 1 regions"):
        metrics.fill_holes(vol, max_voxels=(1, 2, 3))
    with pytest.raises(ValueError, match=">= 0"):
        metrics.fill_holes(vol, max_voxels=-2)
    with pytest.raises(ValueError, match="on the device"):
        metrics.fill_holes(vol, ((1, 2, 3), (2, 3)), fill=(3, 2), max_voxels=(0, 9), connectivity=2)
    _, ffi = _lib()
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.fill_holes(vol, tuple((1,) for _ in range(9)))
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.fill_holes(vol, ())


class _Recorder:
    """stands in for the library: answers the size query and records which entry point a call takes, with its host arguments"""

    def __init__(self):
        self.calls = []

    def uz_vol_components_workspace(self, N, D, H, W):
        return 64

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, [list(a) if isinstance(a, C.Array) else a for a in args]))
            return 0
        return call


def test_entry_point_choice_and_prediction_plumbing_on_cpu_tensors(monkeypatch):
    """With the defaults the two old functions call the old entry points; the new keywords go to the _ex calls with their host arrays; fill_holes
    takes and returns what keep_largest_components does, through one call, with a workspace slot of its own."""
    from unet_zoo_amd import _ffi, _vol, metrics
    from unet_zoo_amd.models.phiseg import Prediction
    rec = _Recorder()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    monkeypatch.setattr(_vol, "on_device", lambda t, what: None)
    monkeypatch.setattr(_vol, "stream", lambda device: 77)
    g = torch.Generator().manual_seed(5)
    vol = torch.randint(0, 4, (2, 3, 4, 5), generator=g, dtype=torch.uint8)
    metrics.label_components(vol, (1,))
    metrics.label_components(vol, (1, 2), connectivity=3)
    metrics.keep_largest_components(vol)
    metrics.keep_largest_components(vol, connectivity=2)
    metrics.keep_largest_components(vol, ((3,),), min_voxels=500, relabel=(1,), unlisted="keep")
    metrics.keep_largest_components(vol, relabel=(None, 0, 255))
    names = [n for n, _ in rec.calls]
    assert names == ["uz_vol_label_components", "uz_vol_label_components_ex", "uz_vol_keep_components", "uz_vol_keep_components_ex", "uz_vol_keep_components_ex",
                     "uz_vol_keep_components_ex"]
    assert rec.calls[1][1][5:7] == [0b110, 3] and rec.calls[1][1][-1] == 77
    assert rec.calls[3][1][5:11] == [[2, 4, 8], [0, 0, 0], [-1, -1, -1], 3, 2, 0]
    assert rec.calls[4][1][5:11] == [[8], [500], [1], 1, 1, 1]
    assert rec.calls[5][1][5:11] == [[2, 4, 8], [0, 0, 0], [-1, 0, 255], 3, 1, 0]
    ws_keep = _vol.workspace("components", (vol.device, 2, 3, 4, 5), 64, vol.device)
    del rec.calls[:]
    out = metrics.fill_holes(vol)
    assert isinstance(out, torch.Tensor) and out.shape == vol.shape and out.dtype == torch.uint8 and out.data_ptr() != vol.data_ptr()
    metrics.fill_holes(vol, ((1, 2, 3), (2, 3)), fill=(3, 2), max_voxels=(0, 9), connectivity=2)
    metrics.fill_holes(vol, ((2, 3), (3,)), max_voxels=7)
    assert [n for n, _ in rec.calls] == ["uz_vol_fill_holes"] * 3
    assert rec.calls[0][1][5:10] == [[0b1110], [1], [0], 1, 1] and rec.calls[0][1][0] == vol.data_ptr() and rec.calls[0][1][10] == out.data_ptr()
    assert rec.calls[1][1][5:10] == [[0b1110, 0b1100], [3, 2], [0, 9], 2, 2] and rec.calls[2][1][5:10] == [[0b1100, 0b1000], [2, 3], [7, 7], 2, 1]
    ws_fill = _vol.workspace("fill_holes", (vol.device, 2, 3, 4, 5), 64, vol.device)
    assert rec.calls[0][1][11] == ws_fill.data_ptr() and ws_fill is not ws_keep
    assert _vol.workspace("components", (vol.device, 2, 3, 4, 5), 64, vol.device) is ws_keep          # the two slots do not evict each other
    # Predictions: the samples and the mean label go through ONE call and come back in the same kind of thing
    rnd = lambda *s: torch.randint(0, 4, s, generator=g, dtype=torch.uint8)
    soft, mean_soft, entropy, levels = object(), object(), object(), object()
    p3 = Prediction(labels=rnd(3, 1, 4, 5, 6), mean_soft=mean_soft, mean_label=rnd(1, 4, 5, 6), entropy=entropy, levels=levels, soft=soft)
    p2 = Prediction(labels=rnd(3, 2, 5, 6), mean_soft=mean_soft, mean_label=rnd(2, 5, 6), entropy=entropy, levels=levels)
    for p, rows in ((p3, (4, 4, 5, 6)), (p2, (8, 1, 5, 6))):
        del rec.calls[:]
        q = metrics.fill_holes(p, ((1, 2, 3),))
        assert [n for n, _ in rec.calls] == ["uz_vol_fill_holes"] and tuple(rec.calls[0][1][1:5]) == rows
        assert type(q) is Prediction and q.labels.shape == p.labels.shape and q.mean_label.shape == p.mean_label.shape
        assert q.mean_soft is mean_soft and q.entropy is entropy and q.levels is levels and q.soft is p.soft
        assert q.labels.data_ptr() == rec.calls[0][1][10]                # cut out of the call's output, not copied
