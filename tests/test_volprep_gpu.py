"""Volume preparation and restore on the device: uz_vol_prepare and uz_vol_restore (csrc/volprep.hip) through ctypes on every case of
tests/_volprep.py, then data.prepare_case / prepare_cases / restore_volume and the loop raw case -> PHISeg3D -> native-space scores.
Gates: info and mask_out integer for integer against the numpy twin; count equal; mean and std within the bounds derived from the
kernel's summation (include/uz_api.h "volume preparation"; the distances are printed under -s); image bit for bit against numpy's fp32
(x - f32(m)) / f32(s) with the kernel's OWN statistics and bit for bit against the restated reference end to end
(tests/test_volprep_cpu.py guarantees the fp32 statistics coincide on these cases); restore byte for byte against the twin.  The
workspace and every output hold 0xFF before every call and lie between guards; raw, image and out also run off their natural
alignment; a repeated call and a call on a second stream are bit-equal.  Only the end-to-end test runs kernels that read UZ_CONV_MATH."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _volprep as V

pytestmark = pytest.mark.gpu

GUARD = 256


def _g():
    from tests import _gpu
    return _gpu


def _prepare(g, c, off=None, with_mask=True, stream=None):
    """One uz_vol_prepare call -> V.Prepared of numpy arrays"""
    L = g.L()
    off = c.offset if off is None else off
    (X, Y, Z, Cn), (Xt, Yt, Zt) = c.raw.shape, c.size
    Pt = Xt * Yt * Zt
    rb, rv = g.embed(c.raw, off)
    mb, mv = g.embed(c.mask, 1)
    nbytes = L.uz_vol_prepare_workspace(Cn, X, Y, Z, Xt, Yt, Zt)
    assert nbytes > 0
    sizes = dict(ws=(nbytes, 0), image=(Pt * Cn * 4, off), mask=(Pt, 3), info=(64, 4), stats=(Cn * 24, 8))
    raw, body = {}, {}
    for k, (n, o) in sizes.items():
        raw[k], body[k] = g.guarded(n, torch.uint8, GUARD, 0xFF, o, room=16)      # 0xFF, o bytes behind a 16-byte boundary, between guards of 0xFF
    st = g.stream() if stream is None else stream.cuda_stream
    rc = L.uz_vol_prepare(rv.data_ptr(), mv.data_ptr() if with_mask else None, Cn, X, Y, Z, Xt, Yt, Zt, c.placement, body["ws"].data_ptr(),
                          body["image"].data_ptr(), body["mask"].data_ptr() if with_mask else None, body["info"].data_ptr(), body["stats"].data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    for k, (n, o) in sizes.items():                                        # nothing outside the buffers
        assert g.intact(raw[k], body[k], 0xFF), k
    if not with_mask:
        assert bool((body["mask"] == 0xFF).all())
    for buf, view, arr, o in ((rb, rv, c.raw, off), (mb, mv, c.mask, 1)):   # the inputs untouched
        assert view.cpu().numpy().tobytes() == arr.tobytes() and g.intact(buf, view, 0xEE)
    as_np = lambda k, dt, shape: body[k].cpu().numpy().view(dt).reshape(shape).copy()
    return V.Prepared(as_np("image", np.float32, (Xt, Yt, Zt, Cn)), as_np("mask", np.uint8, (Xt, Yt, Zt)) if with_mask else None,
                      as_np("info", np.int32, (16,)), as_np("stats", np.float64, (Cn, 3)))


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_values(a, b):
    """bit for bit up to the payload of a NaN (1 x 1 x 1 box: 0 / 0)"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and _bits(np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0))


def _numpy_store(c, got):
    """numpy's fp32 (x - f32(m)) / f32(s) on the placed block with the statistics the kernel reported"""
    n, t, e = got.info[6:9], got.info[9:12], got.info[12:15]
    out = np.zeros_like(got.image)
    block = c.raw[tuple(slice(int(n[a]), int(n[a] + e[a])) for a in range(3))]
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.divide(block - got.stats[:, 1].astype(np.float32), got.stats[:, 2].astype(np.float32))
    out[tuple(slice(int(t[a]), int(t[a] + e[a])) for a in range(3))] = np.where(block == 0, np.float32(0), y)
    return out


def _check(c, got, tag, with_mask=True):
    want = V.expected(c.name)
    assert got.info.tolist() == want.info.tolist(), (tag, got.info.tolist(), want.info.tolist())
    if with_mask:
        assert _bits(got.mask, want.mask), (tag, "mask", int((got.mask != want.mask).sum()))
    assert got.stats[:, 0].tolist() == want.stats[:, 0].tolist(), (tag, "count")
    worst = [0.0, 0.0]
    if c.name not in V.STATS_FREE:
        for ch, (k, mean, var, sum_abs) in enumerate(V.exact_stats(c.raw, want.info)):
            mb, sb = V.mean_bound(k, sum_abs), V.std_bound(k, var, sum_abs)
            dm = abs(Fraction(float(got.stats[ch, 1])) - mean)
            ds = abs(float(got.stats[ch, 2]) - float(var) ** 0.5)
            print(tag, "channel", ch, "n", k, "|mean - exact|", float(dm), "of", float(mb), "|std - exact| ~", ds, "of", float(sb))
            assert dm <= mb, (tag, ch, "mean", float(dm), float(mb))
            assert V.std_within(got.stats[ch, 2], var, sb), (tag, ch, "std", ds, float(sb))
            worst = [max(worst[0], float(dm)), max(worst[1], ds)]
    else:
        assert _same_values(got.stats, want.stats), (tag, got.stats)
    assert _same_values(got.image, _numpy_store(c, got)), (tag, "image against numpy with the kernel's statistics")
    if c.box is not None:
        ref = V.ref_pipeline(c.raw, c.mask, c.size, c.placement)[0]
        assert _same_values(got.image, ref), (tag, "image against the restated reference", int((got.image != ref).sum()))
    else:
        assert not got.image.any() and not got.stats.any()
    return worst


# ================================================================================================ uz_vol_prepare
@pytest.mark.parametrize("name", V.NAMES)
def test_every_case_equals_the_twin_and_the_reference(name):
    g = _g()
    c = V.case(name)
    _check(c, _prepare(g, c), name)
    _check(c, _prepare(g, c, with_mask=False), (name, "no mask"), with_mask=False)
    if c.offset == 0:                                                      # the same case through the scalar form
        _check(c, _prepare(g, c, off=4), (name, "4 bytes off"))


def test_a_repeated_call_and_a_second_stream_are_bit_equal():
    g = _g()
    side = torch.cuda.Stream()
    for name in ("centre_crop_pad_equal", "c5", "c4_off_alignment", "grid_stride", "one_voxel"):
        c = V.case(name)
        a, b = _prepare(g, c), _prepare(g, c)
        with torch.cuda.stream(side):
            s = _prepare(g, c, stream=side)
        for x, y in ((a, b), (a, s)):
            assert all(_bits(p, q) for p, q in zip(x, y)), name
        _check(c, s, (name, "side stream"))


def test_a_refused_call_leaves_the_outputs_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    outs = torch.full((65536,), 0xFF, dtype=torch.uint8, device=dev)
    base, K = outs.data_ptr(), 8192
    for kw in (dict(raw=None), dict(mask=None), dict(mask_out=None), dict(Cn=9), dict(shape=(4, 0, 4)), dict(size=(0, 4, 4)), dict(placement=3),
               dict(ws=base + 8), dict(info=base + 3 * K + 2), dict(stats=base + 4 * K + 4)):
        a = dict(raw=src.data_ptr(), mask=src.data_ptr() + 2048, Cn=4, shape=(4, 4, 4), size=(4, 4, 4), placement=0, ws=base, image=base + K, mask_out=base + 2 * K,
                 info=base + 3 * K, stats=base + 4 * K)
        a.update(kw)
        rc = L.uz_vol_prepare(a["raw"], a["mask"], a["Cn"], *a["shape"], *a["size"], a["placement"], a["ws"], a["image"], a["mask_out"], a["info"], a["stats"], g.stream())
        assert rc == -1 and L.uz_last_error().decode().startswith("vol_prepare:"), kw
    fill = C.c_uint8(0)
    lut = (C.c_uint8 * 256)()
    for kw in (dict(rows=None), dict(place=None), dict(elem=3), dict(elem=4, lut=C.addressof(lut)), dict(out=src.data_ptr() + 8), dict(N=0)):
        a = dict(rows=src.data_ptr(), elem=1, N=2, place=src.data_ptr() + 2048, lut=None, out=base)
        a.update(kw)
        rc = L.uz_vol_restore(a["rows"], a["elem"], a["N"], 4, 4, 4, a["place"], a["lut"], C.addressof(fill), a["out"], 5, 5, 5, g.stream())
        assert rc == -1 and L.uz_last_error().decode().startswith("vol_restore:"), kw
    torch.cuda.synchronize()
    assert bool((outs == 0xFF).all()) and not bool(src.any())


# ================================================================================================ uz_vol_restore
def _restore(g, rows, place, native, lut, fill, off=0, stream=None):
    dev, L = g.dev(), g.L()
    N = rows.shape[0]
    elem = rows.dtype.itemsize
    rb, rv = g.embed(rows, off)
    pl = torch.tensor(list(place), dtype=torch.int32, device=dev)
    nbytes = N * int(np.prod(native)) * elem
    raw, body = g.guarded(nbytes, torch.uint8, GUARD, 0xFF, off, room=16)
    table = None
    if lut is not None:
        table = (C.c_uint8 * 256)(*range(256))
        for k, v in enumerate(lut):
            table[k] = v
    f = C.c_uint8(int(fill)) if elem == 1 else C.c_float(float(fill))
    st = g.stream() if stream is None else stream.cuda_stream
    rc = L.uz_vol_restore(rv.data_ptr(), elem, N, *rows.shape[1:], pl.data_ptr(), None if table is None else C.addressof(table), C.addressof(f), body.data_ptr(),
                          *native, st)
    del table                                                              # the lut travelled in the launch arguments
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(raw, body, 0xFF)
    assert rv.cpu().numpy().tobytes() == rows.tobytes() and g.intact(rb, rv, 0xEE)
    return body.cpu().numpy().view(rows.dtype).reshape((N,) + tuple(native)).copy()


@pytest.mark.parametrize("place", sorted(V.PLACES))
@pytest.mark.parametrize("kind", ("u8", "f32"))
@pytest.mark.parametrize("N", V.RESTORE_N)
def test_restore_equals_the_twin_byte_for_byte(N, kind, place):
    g = _g()
    rows = np.array(V.restore_rows(N, kind))
    for lut in ((None, V.BRATS_LUT) if kind == "u8" else (None,)):
        for fill in ((0, 3) if kind == "u8" else (0.0, -1.5)):
            want = V.restore(rows, V.PLACES[place], V.NATIVE, lut=lut, fill=fill)
            for off in ((0, 1, 4) if kind == "u8" else (0, 4)):              # four elements a thread where out allows the store, else one
                got = _restore(g, rows, V.PLACES[place], V.NATIVE, lut, fill, off=off)
                assert _bits(got, want), (N, kind, place, lut, fill, off, int((got != want).sum()))


def test_restore_of_a_prepared_mask_is_the_mask_on_the_kept_block():
    g = _g()
    side = torch.cuda.Stream()
    for name in ("centre_crop_pad_equal", "centre_pad_crop_pad", "corner_truncates", "faces_by_channel", "c3", "all_le_zero"):
        c = V.case(name)
        got = _prepare(g, c)
        native = c.raw.shape[:3]
        with torch.cuda.stream(side):
            back = _restore(g, got.mask[None], got.info[6:15], native, None, 9, stream=side)[0]
        n, e = got.info[6:9], got.info[12:15]
        kept = tuple(slice(int(n[a]), int(n[a] + e[a])) for a in range(3))
        want = np.full(native, 9, np.uint8)
        want[kept] = c.mask[kept]
        assert _bits(back, want), name
        assert _bits(back, _restore(g, got.mask[None], got.info[6:15], native, None, 9)[0])       # repetition, the other stream


# ================================================================================================ the Python functions
def test_prepare_case_and_restore_volume_on_tensors():
    from unet_zoo_amd import data, metrics
    g = _g()
    dev = g.dev()
    c = V.case("centre_crop_pad_equal")
    want = V.expected(c.name)
    for raw, mask in ((c.raw, c.mask), (torch.from_numpy(c.raw.copy()).to(dev), torch.from_numpy(c.mask.copy()).to(dev))):
        for _ in range(2):                                                 # the second call takes the cached workspace
            case = data.prepare_case(raw, mask, size=c.size, placement="centre", pixel_size=(1, 1, 1), target_resolution=(1, 1, 1))
            assert isinstance(case, data.PreparedCase) and all(t.is_cuda for t in case)
            assert case.info.cpu().numpy().tolist() == want.info.tolist() and _bits(case.mask.cpu().numpy(), want.mask)
            assert case.image.dtype == torch.float32 and _bits(case.image.cpu().numpy(), V.ref_pipeline(c.raw, c.mask, c.size, 0)[0])
            assert case.stats.shape == (4, 3) and case.stats[:, 0].cpu().tolist() == want.stats[:, 0].tolist()
            assert case.offsets() == (2, 0, 5)
    assert data.prepare_case(c.raw, size=c.size).mask is None
    cor = data.prepare_case(c.raw, c.mask, size=(16, 16, 32), placement="corner")
    assert _bits(cor.image.cpu().numpy(), V.ref_pipeline(c.raw, c.mask, (16, 16, 32), 1)[0])
    with pytest.raises(ValueError, match="empty case"):
        data.prepare_case(V.case("all_le_zero").raw, size=(4, 4, 4)).offsets()
    native = c.raw.shape[:3]
    # a device place, a PreparedCase, host offsets; (Xt, Yt, Zt) and (N, Xt, Yt, Zt); the lut
    idx = torch.from_numpy(np.searchsorted(np.array(V.BRATS_LUT), want.mask).astype(np.uint8)).to(dev)       # class indices of the prepared mask
    back = data.restore_volume(idx, case, native_shape=native, lut=metrics.BRATS_LABELS, fill=9)
    assert back.shape == native and _bits(back.cpu().numpy(), V.restore(want.mask[None], want.info[6:15], native, fill=9)[0])
    assert _bits(data.restore_volume(idx[None], case.place, native_shape=native, lut=metrics.BRATS_LABELS, fill=9)[0].cpu().numpy(), back.cpu().numpy())
    ent = torch.from_numpy(np.array(V.restore_rows(3, "f32"))).to(dev)
    off = (5, 3, 11)
    got = data.restore_volume(ent, off, native_shape=V.NATIVE, fill=-1.0)
    assert got.dtype == torch.float32 and _bits(got.cpu().numpy(), V.restore(V.restore_rows(3, "f32"), V.PLACES["far_face"], V.NATIVE, fill=-1.0))
    with pytest.raises(ValueError, match="uint8 rows only"):
        data.restore_volume(ent, off, native_shape=V.NATIVE, lut=metrics.BRATS_LABELS)


def test_prepared_split_through_the_dataset():
    """prepare_cases(...).as_mapping("val") -> BratsDataset(mode="val"): no augmentation, no crop - the item is the prepared image, channels first"""
    from unet_zoo_amd import data
    names = ("corner_pad", "negatives", "cropped_large_corner")
    cs = [V.case(n) for n in names]
    split = data.prepare_cases([c.raw for c in cs], [c.mask for c in cs], names, size=(16, 16, 32), placement="corner")
    assert split.images.shape == (3, 16, 16, 32, 4) and split.masks.shape == (3, 16, 16, 32) and split.info.shape == (3, 16) and split.images.is_cuda
    cfg = dict(TRAIN_ORIGINAL_CLASSES=False, SOFT_AUGMENTATION=False, NN_AUGMENTATION=True, DO_ROTATE=False, ROT_DEGREES=0, DO_SCALE=False, SCALE_FACTOR=1,
               DO_FLIP=False, DO_ELASTIC_AUG=False, SIGMA=0, DO_INTENSITY_SHIFT=False, MAX_INTENSITY_SHIFT=0)
    ds = data.BratsDataset(split.as_mapping("val"), cfg, mode="val", returnOffsets=True)
    assert len(ds) == 3
    for i, c in enumerate(cs):
        image, mask, off = V.ref_pipeline(c.raw, c.mask, (16, 16, 32), 1)
        x, pid, y, ox, oy, oz = ds[i]
        assert pid == names[i] and [int(ox), int(oy), int(oz)] == off
        assert _bits(split.images[i].cpu().numpy(), image) and _bits(split.masks[i].cpu().numpy(), mask.astype(np.uint8))
        assert x.shape == (4, 16, 16, 32) and _bits(x.cpu().numpy(), np.ascontiguousarray(image.transpose(3, 0, 1, 2)))
        m = mask.astype(np.uint8)
        assert _bits(y.cpu().numpy(), np.stack([m != 0, (m != 0) & (m != 2), m == 4]).astype(np.float32))      # _toEvaluationOneHot


def test_raw_case_to_native_space_scores_end_to_end():
    """raw 40 x 36 x 33 -> prepare_case(size=(32, 32, 32)) -> PHISeg3D.predict(n_samples=2) -> keep_largest_components -> restore_volume with
    the BraTS labels -> score_volume against the native mask"""
    import oracle
    from tests import _golden as G
    from tests import _nets as N
    from unet_zoo_amd import data, metrics
    g = _g()
    dev = g.dev()
    _, meta = G.load("phiseg3d_small")
    Cn, K = int(meta["input_channels"]), int(meta["num_classes"])
    net = N.small_phiseg3d(dict(meta, dhw=(32, 32, 32)), oracle.deterministic_state_dict(G.spec_of(meta), seed=91))
    native, box = (40, 36, 33), ([3, 1, 0], [39, 36, 31])                  # 36 x 35 x 31: crop, crop, pad
    raw = V._boxed(77, shape=native, Cn=Cn, box=box)
    mask = V._mask(78, native)
    case = data.prepare_case(raw, mask, size=(32, 32, 32))
    want = V.prepare(raw, mask, (32, 32, 32), 0)
    assert case.info.cpu().tolist() == want.info.tolist() and case.info[12:15].cpu().tolist() == [32, 32, 31]
    torch.manual_seed(5)
    with torch.no_grad():
        pred = net.predict(case.image.permute(3, 0, 1, 2)[None].contiguous(), n_samples=2)
    filt = metrics.keep_largest_components(pred, regions=tuple((k,) for k in range(1, K)))
    out = data.restore_volume(filt, case, native_shape=native, lut=metrics.BRATS_LABELS)
    torch.cuda.synchronize()
    assert out.labels.shape == (2, 1) + native and out.mean_label.shape == (1,) + native and out.entropy.shape == (1,) + native
    assert out.labels.dtype == torch.uint8 and out.entropy.dtype == torch.float32 and out.mean_soft is None and out.levels is None and out.soft is None
    rows = np.concatenate([filt.labels[:, 0].cpu().numpy(), filt.mean_label.cpu().numpy()])
    placed = V.restore(rows, want.info[6:15], native, lut=V.BRATS_LUT, fill=0)                     # a numpy placement of the filtered labels
    assert _bits(out.labels[:, 0].cpu().numpy(), placed[:2]) and _bits(out.mean_label.cpu().numpy(), placed[2:])
    assert _bits(out.entropy.cpu().numpy(), V.restore(pred.entropy.cpu().numpy(), want.info[6:15], native, fill=0.0))
    assert set(np.unique(placed)) <= {0, 1, 2, 4}
    sc = metrics.score_volume(out, torch.from_numpy(mask).to(dev), metrics.BRATS_REGIONS)
    assert sc.dice.shape == (3, 3) and sc.counts.shape == (3, 3, 4)
    cnt = sc.counts.cpu().numpy()
    for r, reg in enumerate(metrics.BRATS_REGIONS):
        for i in range(3):
            p, t = np.isin(placed[i], reg), np.isin(mask, reg)
            assert cnt[i, r].tolist() == [int((p & t).sum()), int(p.sum()), int(t.sum()), mask.size], (i, r)
