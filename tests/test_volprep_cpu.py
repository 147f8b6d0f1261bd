"""Volume preparation and restore without a GPU: the numpy twin of tests/_volprep.py against the restated reference functions and exact
rational statistics on every case, the planted defects, the rounding margin that lets the GPU test compare voxels bit for bit, the
route, workspace and refusal claims of the C entry points (host code: the library loads without a device), the argument errors of
the Python functions and BratsDataset's returnOffsets tuples."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _volprep as V

CAP, TB = 2048, 256


def _lib():
    import unet_zoo_amd  # noqa: F401
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ================================================================================================ the twin
@pytest.mark.parametrize("name", V.NAMES)
def test_twin_equals_the_restated_reference(name):
    c, got = V.case(name), V.expected(name)
    if c.box is None:
        with pytest.raises(ValueError):
            V.ref_crop(c.raw, c.mask)
        assert got.info.tolist() == [0] * 15 + [1] and not got.image.any() and not got.mask.any() and not got.stats.any()
        return
    image, mask, off = V.ref_pipeline(c.raw, c.mask, c.size, c.placement)
    assert got.info[0:6].tolist() == c.box[0] + c.box[1] and got.info[0:3].tolist() == off      # the support was built for this box
    assert _same(got.image, image), int((got.image != image).sum())
    assert _same(got.mask, mask.astype(np.uint8))
    s = [c.box[1][a] - c.box[0][a] for a in range(3)]
    assert got.info[15] == (2 if any(T < k for T, k in zip(c.size, s)) else 0)
    n, t, e = got.info[6:9], got.info[9:12], got.info[12:15]
    assert all(c.box[0][a] <= n[a] and n[a] + e[a] <= c.box[1][a] and 0 <= t[a] and t[a] + e[a] <= c.size[a] for a in range(3))
    if name == "one_voxel":
        assert np.isnan(got.image).sum() == 2 and got.stats[:, 0].tolist() == [1, 0, 1, 0] and got.stats[:, 2].tolist() == [0] * 4


def test_placement_table_on_the_named_cases():
    """crop with an odd difference, pad with an even one, equal; pad odd, crop odd, pad odd; corner with and without truncation"""
    want = {"centre_crop_pad_equal": ([3, 0, 5], [0, 2, 0], [6, 10, 29], 2), "centre_pad_crop_pad": ([2, 1, 5], [1, 0, 5], [9, 7, 29], 2),
            "corner_pad": ([2, 0, 5], [0, 0, 0], [9, 10, 29], 0), "corner_truncates": ([2, 0, 5], [0, 0, 0], [6, 7, 20], 2)}
    for name, (n, t, e, flags) in want.items():
        assert V.expected(name).info[6:16].tolist() == n + t + e + [flags], name


@pytest.mark.parametrize("name", [n for n in V.NAMES if n not in V.STATS_FREE])
def test_twin_statistics_against_exact_rationals_and_the_rounding_margin(name):
    """The twin's count is exact, its mean and std lie within the kernel's bound of the exact values (numpy's sums obey the same outer
    limit) - and the exact values lie further from every fp32 rounding boundary than that bound, so f32(mean) and f32(std) are the
    same numbers whichever conforming summation produced them: the GPU test may then compare voxels with the reference bit for bit."""
    c, got = V.case(name), V.expected(name)
    for ch, (k, mean, var, sum_abs) in enumerate(V.exact_stats(c.raw, got.info)):
        assert k > 1 and var > 0, (name, ch)
        assert got.stats[ch, 0] == k
        mb, sb = V.mean_bound(k, sum_abs), V.std_bound(k, var, sum_abs)
        assert abs(Fraction(float(got.stats[ch, 1])) - mean) <= mb, (name, ch)
        assert V.std_within(got.stats[ch, 2], var, sb), (name, ch)
        assert V.f32_margin(mean, mb) and V.f32_margin_sqrt(var, sb), (name, ch, "replace this case: a statistic sits on an fp32 rounding boundary")
        assert float(sb) < 1e-9 * float(var) ** 0.5 and float(mb) <= 1e-9 * float(sum_abs) / k


# ================================================================================================ planted defects
DETECTS = {"box_ne0": "negatives", "box_ch0": "faces_by_channel", "stats_whole_box": "cropped_large_centre", "zeros_counted": "centre_crop_pad_equal",
           "ddof1": "c3", "half_up": "centre_pad_crop_pad", "corner_as_centre": "corner_pad", "zeros_normalised": "c1",
           "mask_unshifted": "centre_crop_pad_equal", "last_slice_dropped": "corner_pad"}


def _gates(c, got):
    """what the GPU test holds the kernel to, on a twin result: False when a gate fails"""
    image, mask, off = V.ref_pipeline(c.raw, c.mask, c.size, c.placement)
    if got.info[0:6].tolist() != c.box[0] + c.box[1] or not _same(got.image, image) or not _same(got.mask, mask.astype(np.uint8)):
        return False
    for ch, (k, mean, var, sum_abs) in enumerate(V.exact_stats(c.raw, V.expected(c.name).info)):
        if got.stats[ch, 0] != k or abs(Fraction(float(got.stats[ch, 1])) - mean) > V.mean_bound(k, sum_abs) or \
                not V.std_within(got.stats[ch, 2], var, V.std_bound(k, var, sum_abs)):
            return False
    return True


@pytest.mark.parametrize("defect", sorted(DETECTS))
def test_every_defect_fails_the_gates_on_the_named_case(defect):
    c = V.case(DETECTS[defect])
    assert _gates(c, V.expected(c.name))
    assert not _gates(c, V.prepare(c.raw, c.mask, c.size, c.placement, defect=defect)), defect


def test_restore_defects_fail_on_the_named_cases():
    # the source shift of a cropped axis: the round trip of the mask through a centre crop
    c, got = V.case("centre_crop_pad_equal"), V.expected("centre_crop_pad_equal")
    native = c.raw.shape[:3]
    back = V.restore(got.mask[None], V.place_of(got.info), native, fill=9)[0]
    n, e = got.info[6:9], got.info[12:15]
    kept = tuple(slice(int(n[a]), int(n[a] + e[a])) for a in range(3))
    want = np.full(native, 9, np.uint8)
    want[kept] = c.mask[kept]
    assert np.array_equal(back, want)
    assert not np.array_equal(V.restore(got.mask[None], V.place_of(got.info, "restore_ignores_shift"), native, fill=9)[0], want)
    # the lut maps the rows, never the fill
    rows = V.restore_rows(3, "u8")
    good = V.restore(rows, V.PLACES["origins"], V.NATIVE, lut=V.BRATS_LUT, fill=3)
    assert set(np.unique(good)) == {0, 1, 2, 3, 4} and (good == 3).sum() == 3 * (np.prod(V.NATIVE) - 7 * 6 * 20)
    assert not np.array_equal(V.restore(rows, V.PLACES["origins"], V.NATIVE, lut=V.BRATS_LUT, fill=3, defect="lut_on_fill"), good)
    assert set(DETECTS) | {"restore_ignores_shift", "lut_on_fill"} == set(V.DEFECTS)


def test_restore_twin_places_and_clips():
    rows = V.restore_rows(1, "f32")
    out = V.restore(rows, V.PLACES["far_face"], V.NATIVE, fill=-1.5)
    assert np.array_equal(out[0, 5:, 3:, 11:], rows[0]) and (out[0, :5] == -1.5).all() and (out[0, :, :3] == -1.5).all() and (out[0, :, :, :11] == -1.5).all()
    out = V.restore(rows, V.PLACES["hanging"], V.NATIVE, fill=-1.5)
    # x: native 0 .. 6 show target 5 .. 9 (rows end), y: native 8 .. 11 show target 0 .. 3, z: native 30 .. 40 show target 5 .. 15
    assert np.array_equal(out[0, 0:5, 8:12, 30:41], rows[0, 5:10, 0:4, 5:16]) and (out == -1.5).sum() == out.size - 5 * 4 * 11
    assert (V.restore(rows, V.PLACES["nothing"], V.NATIVE, fill=2.0) == 2.0).all()


# ================================================================================================ route, workspace, refusals
def _route(L, Cn, shape, size, align):
    out = (C.c_int * 3)()
    assert L.uz_vol_prepare_route(Cn, *shape, *size, align, out) == 0, L.uz_last_error()
    return tuple(out)


def test_route_claims_of_the_case_set():
    L, _ = _lib()
    reached = set()
    for c in V.cases():
        Cn, P = c.raw.shape[3], max(int(np.prod(c.raw.shape[:3])), int(np.prod(c.size)))
        form, wgs, strides = _route(L, Cn, c.raw.shape[:3], c.size, 16 if c.offset == 0 else 4)
        assert form == (1 if Cn == 4 and c.offset == 0 else 0), c.name
        assert wgs == min(CAP, -(-P // TB)) and strides == (1 if P > CAP * TB else 0), c.name
        assert strides == (1 if c.name == "grid_stride" else 0)
        reached.add(("scalar", "wide")[form] + ("+stride" if strides else ""))
    assert reached == {"scalar", "wide", "wide+stride"}
    shape, wg = V.stride_shape()
    assert wg == CAP and int(np.prod(shape)) > CAP * TB >= int(np.prod(shape)) - 64 * 64          # the smallest 64 x 64 x Z that strides
    assert _route(L, 4, (240, 240, 155), (160, 192, 160), 16) == (1, CAP, 1)                       # the BraTS case
    assert _route(L, 4, (240, 240, 155), (160, 192, 160), 8)[0] == 0 and _route(L, 8, (4, 4, 4), (4, 4, 4), 16)[0] == 0
    assert _route(L, 4, (4, 4, 4), (64, 64, 129), 16) == (1, CAP, 1)                               # the target can be the widest pass
    out = (C.c_int * 3)()
    # restore: elements a thread (16 or 4 uint8, 4 fp32, where out allows the one store), workgroups of 256 threads over the wide units + the tail
    for elem, N, shape, align, want in [(1, 1, V.NATIVE, 16, (16, 2, 0)), (1, 17, V.NATIVE, 4, (4, 123, 0)), (1, 17, V.NATIVE, 8, (4, 123, 0)), (1, 3, V.NATIVE, 2, (1, 87, 0)),
                                        (4, 3, V.NATIVE, 16, (4, 22, 0)), (4, 3, V.NATIVE, 8, (1, 87, 0)), (1, 1, (1, 1, 3), 16, (1, 1, 0)), (1, 1, (1, 1, 15), 16, (4, 1, 0)),
                                        (1, 17, (240, 240, 155), 16, (16, 37055, 0))]:
        assert L.uz_vol_restore_route(elem, N, *shape, align, out) == 0 and tuple(out) == want, (elem, N, align, tuple(out))
    assert 15 * 12 * 41 // 16 == 461 and 15 * 12 * 41 % 16 == 4 and 3 * 15 * 12 * 41 // 4 == 5535 and 17 * 240 * 240 * 155 // 16 == 9486000
    assert all(N * 15 * 12 * 41 % 16 for N in V.RESTORE_N)                   # every restore case of the GPU test has a tail behind the 16-wide units
    for args in [(2, 1, 4, 4, 4, 16), (1, 0, 4, 4, 4, 16), (1, 1, 0, 4, 4, 16), (1, 2, 1024, 1024, 1024, 16), (1, 1, 4, 4, 4, 3), (4, 1, 4, 4, 4, 2)]:
        assert L.uz_vol_restore_route(*args, out) != 0 and L.uz_last_error().decode().startswith("vol_restore_route:"), args


def test_workspace_sizes_and_refused_sizes():
    L, _ = _lib()
    for Cn, shape, size in [(4, (240, 240, 155), (160, 192, 160)), (4, (240, 240, 155), (128, 128, 128)), (1, (1, 1, 1), (1, 1, 1)), (5, (7, 9, 11), (6, 6, 12)),
                            (8, (13, 10, 37), (300, 300, 300))]:
        gb, gt = min(CAP, -(-int(np.prod(shape)) // TB)), min(CAP, -(-int(np.prod(size)) // TB))
        assert L.uz_vol_prepare_workspace(Cn, *shape, *size) == (gb * 32 + 15) // 16 * 16 + gt * 128, (Cn, shape, size)
    out = (C.c_int * 3)()
    for Cn, shape, size in [(0, (4, 4, 4), (4, 4, 4)), (9, (4, 4, 4), (4, 4, 4)), (4, (0, 4, 4), (4, 4, 4)), (4, (4, 4, 4), (4, 0, 4)), (4, (4, 4, 4), (4, 4, 0)),
                            (4, (1024, 1024, 512), (4, 4, 4)), (4, (4, 4, 4), (1024, 1024, 512)), (1, (2048, 1024, 1024), (4, 4, 4)), (1, (65536, 65536, 65536), (4, 4, 4))]:
        assert L.uz_vol_prepare_workspace(Cn, *shape, *size) == 0, (Cn, shape, size)
        assert L.uz_vol_prepare_route(Cn, *shape, *size, 16, out) != 0 and L.uz_last_error().decode().startswith("vol_prepare_route:")
    assert L.uz_vol_prepare_workspace(1, 2047, 1024, 1024, 4, 4, 4) > 0 and L.uz_vol_prepare_workspace(4, 1023, 1024, 512, 4, 4, 4) > 0      # just below 2^31
    assert L.uz_vol_prepare_route(4, 4, 4, 4, 4, 4, 4, 16, None) != 0 and L.uz_vol_prepare_route(4, 4, 4, 4, 4, 4, 4, 2, out) != 0


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written."""
    L, _ = _lib()
    host = np.zeros(16384, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    K = 8192

    def prep(raw=ptr, mask=ptr + K, Cn=4, shape=(4, 4, 4), size=(4, 4, 4), placement=0, ws=ptr + 2 * K, image=ptr + 4 * K, mask_out=ptr + 5 * K, info=ptr + 6 * K,
             stats=ptr + 7 * K):
        rc = L.uz_vol_prepare(raw, mask, Cn, *shape, *size, placement, ws, image, mask_out, info, stats, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(raw=None), "null"), (dict(ws=None), "null"), (dict(image=None), "null"), (dict(info=None), "null"), (dict(stats=None), "null"),
                       (dict(mask=None), "both or neither"), (dict(mask_out=None), "both or neither"), (dict(Cn=0), "1 <= C <= 8"), (dict(Cn=9), "1 <= C <= 8"),
                       (dict(shape=(0, 4, 4)), "empty axis"), (dict(shape=(4, 4, 0)), "empty axis"), (dict(size=(4, 0, 4)), "empty axis"),
                       (dict(shape=(1024, 1024, 512)), "X*Y*Z*C"), (dict(size=(1024, 1024, 512)), "Xt*Yt*Zt*C"), (dict(placement=2), "placement"),
                       (dict(placement=-1), "placement"), (dict(ws=ptr + 2 * K + 8), "16-byte"), (dict(info=ptr + 6 * K + 2), "4-byte"),
                       (dict(stats=ptr + 7 * K + 4), "8-byte")]:
        rc, msg = prep(**kw)
        assert rc == -1 and reason in msg and msg.startswith("vol_prepare:"), (kw.keys(), rc, msg)

    lut = (C.c_uint8 * 256)(*range(256))
    fill = C.c_float(0)

    def rest(rows=ptr, elem=1, N=2, size=(4, 4, 4), place=ptr + K, lut=None, fill=C.addressof(fill), out=ptr + 2 * K, native=(5, 5, 5)):
        rc = L.uz_vol_restore(rows, elem, N, *size, place, lut, fill, out, *native, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(rows=None), "null"), (dict(place=None), "null"), (dict(fill=None), "null"), (dict(out=None), "null"), (dict(elem=2), "elem"),
                       (dict(N=0), "empty axis"), (dict(size=(4, 0, 4)), "empty axis"), (dict(native=(5, 5, 0)), "empty axis"),
                       (dict(native=(1024, 1024, 1024)), "N*X*Y*Z"), (dict(size=(1024, 1024, 1024)), "N*Xt*Yt*Zt"),
                       (dict(elem=4, lut=C.addressof(lut)), "uint8 rows only"), (dict(elem=4, rows=ptr + 2), "4-byte"), (dict(elem=4, out=ptr + 2 * K + 1), "4-byte"),
                       (dict(place=ptr + K + 2), "4-byte"), (dict(out=ptr + 64), "overlap"), (dict(out=ptr - 100, rows=ptr), "overlap"),
                       (dict(elem=4, out=ptr + 508), "overlap")]:
        rc, msg = rest(**kw)
        assert rc == -1 and reason in msg and msg.startswith("vol_restore:"), (kw.keys(), rc, msg)
    assert not host.any()


# ================================================================================================ the Python functions, the binding
def test_argument_errors_of_the_python_functions():
    from unet_zoo_amd import data, metrics
    raw, mask = np.zeros((4, 5, 6, 4), np.float32), np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(NotImplementedError, match="resampling"):
        data.prepare_case(raw, pixel_size=(1, 1, 2), target_resolution=(1, 1, 1))
    with pytest.raises(NotImplementedError, match="resampling"):
        data.prepare_case(raw, pixel_size=(1, 1, 1))
    with pytest.raises(ValueError, match="placement"):
        data.prepare_case(raw, placement="middle")
    with pytest.raises(ValueError, match="three positive extents"):
        data.prepare_case(raw, size=(4, 4))
    with pytest.raises(ValueError, match="three positive extents"):
        data.prepare_case(raw, size=(4, 0, 4))
    with pytest.raises(ValueError, match=r"not \(X, Y, Z, C\)"):
        data.prepare_case(raw[0])
    with pytest.raises(ValueError, match="does not match raw"):
        data.prepare_case(raw, mask[:3])
    with pytest.raises(TypeError, match="raw must be float32"):
        data.prepare_case(raw.astype(np.int16), device="cpu")
    with pytest.raises(TypeError, match="mask must be uint8"):
        data.prepare_case(raw, mask.astype(np.int32), device="cpu")
    with pytest.raises(ValueError, match="2 masks for 1 cases"):
        data.prepare_cases([raw], [mask, mask], ["a"])
    with pytest.raises(ValueError, match="2 pids for 1 cases"):
        data.prepare_cases([raw], None, ["a", "b"])
    with pytest.raises(ValueError, match="no cases"):
        data.prepare_cases([], None, [])
    x = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8 / fp32"):
        data.restore_volume(x.int(), (0, 0, 0))
    with pytest.raises(ValueError, match=r"not \(N, Xt, Yt, Zt\)"):
        data.restore_volume(x[0, 0], (0, 0, 0))
    with pytest.raises(ValueError, match="on the device"):
        data.restore_volume(x, (0, 0, 0))
    with pytest.raises(ValueError, match="native_shape"):
        data.restore_volume(x, (0, 0, 0), native_shape=(240, 240))
    P = type("P", (), {})
    p = P()
    p.labels, p.mean_label, p.entropy = torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8), torch.zeros(2, 4, 5, 6, dtype=torch.uint8), None
    with pytest.raises(ValueError, match="Prediction of one volume expected"):
        data.restore_volume(p, (0, 0, 0))
    p.labels, p.mean_label = torch.zeros(2, 1, 4, 5, 6), torch.zeros(1, 4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        data.restore_volume(p, (0, 0, 0))
    from unet_zoo_amd.data import brats_prepare as bp
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="three ints"):
        bp._place_tensor((1, 2), (4, 5, 6), (8, 8, 8), dev)
    with pytest.raises(ValueError, match="outside the native volume"):
        bp._place_tensor((1, 8, 2), (4, 5, 6), (8, 8, 8), dev)
    with pytest.raises(ValueError, match=r"int32\[9\]"):
        bp._place_tensor(torch.zeros(9), (4, 5, 6), (8, 8, 8), dev)
    assert bp._place_tensor((1, 5, 2), (4, 5, 6), (8, 8, 8), dev).tolist() == [1, 5, 2, 0, 0, 0, 4, 3, 6]       # extent = min(target, native - offset)
    assert metrics.BRATS_LABELS == (0, 1, 2, 4) == V.BRATS_LUT
    # an empty case has no offsets; a case has the origin of its box
    info = torch.zeros(16, dtype=torch.int32)
    info[15] = 1
    with pytest.raises(ValueError, match="empty case"):
        data.PreparedCase(None, None, info, None).offsets()
    info = torch.tensor(V.expected("centre_crop_pad_equal").info)
    case = data.PreparedCase(None, None, info, None)
    assert case.offsets() == (2, 0, 5) and case.place.tolist() == info[6:15].tolist()


def test_split_mapping_and_return_offsets_tuples():
    from unet_zoo_amd import data
    from unet_zoo_amd.data.brats_dataset import BratsDataset
    info = torch.zeros(2, 16, dtype=torch.int32)
    info[0, :3] = torch.tensor([2, 0, 5], dtype=torch.int32)
    info[1, :3] = torch.tensor([7, 4, 20], dtype=torch.int32)
    split = data.PreparedSplit(images=torch.zeros(2, 4, 4, 4, 4), masks=torch.zeros(2, 4, 4, 4, dtype=torch.uint8), pids=["a", "b"], info=info)
    m = split.as_mapping("val")
    assert sorted(m) == ["images_val", "masks_val", "pids_val", "xOffsets_val", "yOffsets_val", "zOffsets_val"]
    assert m["images_val"] is split.images and m["xOffsets_val"].tolist() == [2, 7] and m["zOffsets_val"].tolist() == [5, 20]
    assert "masks_val" not in split._replace(masks=None).as_mapping("val")
    cfg = dict(TRAIN_ORIGINAL_CLASSES=False, SOFT_AUGMENTATION=False, NN_AUGMENTATION=True, DO_ROTATE=False, ROT_DEGREES=0, DO_SCALE=False, SCALE_FACTOR=1,
               DO_FLIP=False, DO_ELASTIC_AUG=False, SIGMA=0, DO_INTENSITY_SHIFT=False, MAX_INTENSITY_SHIFT=0)
    ds = BratsDataset(m, cfg, mode="val", returnOffsets=True, device="cpu")
    ds.openFileIfNotOpen()
    assert len(ds) == 2 and ds._item(1, "x", "y") == ("x", "b", "y", 7, 4, 20)                   # bratsDataset.py:105-106
    ds = BratsDataset(m, cfg, mode="val", hasMasks=False, returnOffsets=True, device="cpu")
    ds.openFileIfNotOpen()
    assert ds._item(0, "x", None) == ("x", "a", 2, 0, 5)                                          # :107-108
    ds = BratsDataset(m, cfg, mode="val", device="cpu")
    ds.openFileIfNotOpen()
    assert ds._item(0, "x", "y") == ("x", "a", "y") and ds.returnOffsets is False


def test_binding_parses_the_new_declarations():
    _, ffi = _lib()
    protos = ffi.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["uz_vol_prepare_workspace"] == (C.c_size_t, [i] * 7)
    assert protos["uz_vol_prepare"] == (i, [vp, vp] + [i] * 8 + [vp] * 6)
    assert protos["uz_vol_prepare_route"] == (i, [i] * 8 + [vp])
    assert protos["uz_vol_restore"] == (i, [vp, i, i, i, i, i, vp, vp, vp, vp, i, i, i, vp])
    assert protos["uz_vol_restore_route"] == (i, [i] * 6 + [vp])
    assert protos["uz_vol_uncertainty_route"] == (i, [i] * 6 + [vp])    # the declarations in front are parsed as before
