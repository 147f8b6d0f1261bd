"""CPU tier of the mirrored passes of PHISeg3D.predict_volume (flips=...): the numpy twins of tests/_volflip.py against a composition
of the imported unmirrored pieces with np.flip, the noise-crop arithmetic, the proof that the case set tells each deliberate defect
from the right evaluation, the `flips` argument errors of predict_volume and UNetModel.predict, and the refusals of
uz_vol_window_gather_ex / _accum_ex / uz_vol_window_noise - decided on the host, so they show without a device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi
from unet_zoo_amd.models import phiseg3D as M
from tests import _volflip as VF
from tests import _volwindow as VW

IDS = [VF.case_id(c) for c in VF.CASES]


# ------------------------------------------------------------------------------------------ the case set
def test_the_cases_hold_what_the_issue_names():
    cs = VF.CASES
    grids = [VF.window_grid(c.dhw, c.window, c.stride, c.g) for c in cs]
    assert tuple(len(g[2]) for g in grids) == VF.WINDOW_COUNTS
    assert all(max(c.dhw + c.window) <= 32 and max(g[0]) <= 32 and c.S <= 3 for c, g in zip(cs, grids)) and set(VF.STATS_K) == {1, 3, 8}
    assert any(len(set(g[1])) == 3 for g in grids)                                                   # three unequal window sides
    over = {tuple(p > n for p, n in zip(g[0], c.dhw)) for c, g in zip(cs, grids)}
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)} <= over
    assert any(f != fz for c in cs for f, fz in c.factors) and any(f == fz for c in cs for f, fz in c.factors)
    assert max(f for c in cs for f, _ in c.factors) >= 4
    assert any(c.blend == "ramp" for c in cs) and any(c.blend == "gaussian" for c in cs)
    t = VF.tables_of((8, 12, 16), "ramp")
    assert all(np.all(x > 0) and np.all(x <= 1) and not np.array_equal(x, x[::-1]) for x in t)
    assert 1 in VF.WINDOW_COUNTS and VF.case(4, 1)["ref"]["count"].max() > 3 * 2                      # overlap: more passes than the masks of one window
    flips = [c.flips for c in cs]
    assert "all" in flips and (7,) in flips and {1, 2, 4} <= {m for f in flips if f != "all" for m in f}
    assert any(f != "all" and len(f) > 1 and 0 in f for f in flips) and any(f != "all" and 0 not in f for f in flips)
    for shape in ((4, 8, 12), (2, 6, 5, 7)):
        v = VF.ramp_noise(shape, 3)
        assert v.dtype == np.float32 and len(np.unique(v)) == v.size
        assert all(not np.array_equal(v, VF.mirrored(v, m)) for m in range(1, 8))


# ------------------------------------------------------------------------------------------ the twins, stated twice
@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_gather_twin_is_the_unmirrored_gather_mirrored(i):
    c = VF.CASES[i]
    padded, extent, origins = VF.window_grid(c.dhw, c.window, c.stride, c.g)
    src = VF.ramp_noise((2, *c.dhw), 11 + i)
    for o in origins + [tuple(n + 3 for n in c.dhw)]:
        for m in VF.ALL:
            got = VF.gather_flip(src, o, extent, m, padded=padded)
            assert got.tobytes() == np.ascontiguousarray(VF.mirrored(VF.gather_twin(src, o, extent), m)).tobytes(), (o, m)
        assert np.array_equal(VF.gather_flip(src, o, extent, 0), VF.gather_twin(src, o, extent))


def test_noise_crop_arithmetic():
    field = VF.ramp_noise((2, 6, 5, 7), 5)
    o, crop = (1, 2, 3), (4, 3, 2)
    plain = field[:, 1:5, 2:5, 3:5]
    assert np.array_equal(VF.noise_crop(field, o, crop, 0), plain)
    for m in VF.ALL:
        got = VF.noise_crop(field, o, crop, m)
        assert got.shape == (2, *crop) and np.array_equal(got, VF.mirrored(plain, m))
        for z in range(crop[0]):                                                    # element i of the crop feeds net-frame element c - 1 - i
            for y in range(crop[1]):
                for x in range(crop[2]):
                    q = [cc - 1 - n if (m >> a) & 1 else n for a, (cc, n) in enumerate(zip(crop, (z, y, x)))]
                    assert np.array_equal(got[:, z, y, x], field[:, o[0] + q[0], o[1] + q[1], o[2] + q[2]])
    # the noise stays attached to the anatomy: resized to voxels, the mirrored crop is the mirrored resized crop - for both factors
    for f, fz in ((2, 2), (4, 2), (1, 2)):
        up = lambda t: t.repeat(fz, axis=-3).repeat(f, axis=-2).repeat(f, axis=-1)   # noqa: E731
        for m in VF.ALL:
            assert np.array_equal(up(VF.noise_crop(field, o, crop, m)), VF.mirrored(up(plain), m))
    # ... and where predict_volume cuts it: the crops of the cases' levels lie inside their fields
    for c in VF.CASES:
        padded, extent, origins = VF.window_grid(c.dhw, c.window, c.stride, c.g)
        for fac in c.factors:
            for og in origins:
                size, lo, ext, q = VF.level_geometry(c, padded, extent, og, fac)
                assert all(a * d == b for a, b, d in zip(lo, og, q)) and all(a + e <= s for a, e, s in zip(lo, ext, size))


@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_twin_is_the_unmirrored_evaluation_of_mirrored_levels(i):
    """evaluate_flips = _volwindow.evaluate fed one entry per (window, mask) with the levels mirrored into the window's frame: bit for
    bit at both precisions; with masks (0,) it IS _volwindow.evaluate of the windows."""
    c = VF.CASES[i]
    for K in VF.STATS_K:
        d = VF.case(i, K)
        for prec in ("twin", "ref"):
            want = VW.evaluate(c.dhw, d["extent"], d["xorigins"], d["tables"], c.factors, d["xlevels"], c.S, prec)
            got = d[prec]
            assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want), (IDS[i], K, prec)
        first = [[w[0]] for w in d["levels"]]
        a = VF.evaluate_flips(c.dhw, d["extent"], d["origins"], (0,), d["tables"], c.factors, first, c.S, "twin")
        b = VW.evaluate(c.dhw, d["extent"], d["origins"], d["tables"], c.factors, [w[0] for w in first], c.S, "twin")
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b), (IDS[i], K)


@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_twin_meets_the_gates_and_the_exempt_share_stays_under_the_cap(i):
    c = VF.CASES[i]
    for K in VF.STATS_K:
        d = VF.case(i, K)
        tw, ref, (pin, mpin, struct) = d["twin"], d["ref"], d["pins"]
        failed, fig = VF.gates(tw, tw, ref, d["pins"], c.S)
        assert not failed, (IDS[i], K, fig)
        assert not np.any((ref["labels"] != tw["labels"]) & pin) and not np.any((ref["mean_label"] != tw["mean_label"]) & mpin)
        exempt = max(float(np.mean(~pin[s])) for s in range(c.S))
        assert exempt <= VF.EXEMPT_CAP and float(np.mean(~mpin)) <= VF.EXEMPT_CAP, (IDS[i], K, exempt)
        assert np.all(ref["count"] >= len(d["masks"])) and np.allclose(ref["mean_soft"].sum(axis=0), 1.0, atol=1e-12)
        for w in d["levels"]:
            for ps in w:
                assert np.array_equal(VW.summed_logits(ps, c.factors, np.float32), VW.summed_logits(ps, c.factors, np.float64))


# ------------------------------------------------------------------------------------------ the cases discriminate
@pytest.mark.parametrize("defect", list(VF.DEFECTS))
def test_every_defect_changes_the_expected_output_of_some_case(defect):
    """Per twin the defect changes: gather and noise are compared byte for byte (nothing is exempt there), the evaluation through the
    gates, which look at labels on the pinned voxels only."""
    stages = VF.DEFECTS[defect]
    caught = {s: [] for s in stages}
    for i, c in enumerate(VF.CASES):
        padded, extent, origins = VF.window_grid(c.dhw, c.window, c.stride, c.g)
        masks = VF.masks_of(c.flips)
        if "gather" in stages:
            src = VF.ramp_noise((2, *c.dhw), 11 + i)
            if any(not np.array_equal(VF.gather_flip(src, o, extent, m, defect, padded), VF.gather_flip(src, o, extent, m, None, padded))
                   for o in origins for m in masks):
                caught["gather"].append(IDS[i])
        if "noise" in stages:
            for l, fac in enumerate(c.factors):
                size, lo, ext, q = VF.level_geometry(c, padded, extent, origins[-1], fac)
                field = VF.ramp_noise((2, *size), 23 + l)
                if any(not np.array_equal(VF.noise_crop(field, lo, ext, m, defect, q), VF.noise_crop(field, lo, ext, m)) for m in masks):
                    caught["noise"].append((IDS[i], l))
        if "accum" in stages and not caught["accum"]:                                   # one catch suffices: the evaluations are the slow part
            for K in VF.STATS_K:
                d = VF.case(i, K)
                bad = VF.evaluate_flips(*d["args"], "ref", defect=defect, padded=padded)
                failed, fig = VF.gates(bad, d["twin"], d["ref"], d["pins"], c.S)
                if failed:
                    caught["accum"].append((IDS[i], K, failed))
                    break
    print(defect, "caught:", caught)
    assert all(caught[s] for s in stages), (defect, caught)


# ------------------------------------------------------------------------------------------ arguments
def test_flip_masks_and_argument_errors():
    assert M.flip_masks("all") == tuple(range(8)) and M.flip_masks((7,)) == (7,) and M.flip_masks([4, 0, 3]) == (4, 0, 3)
    assert M.flip_masks(np.array([1, 2])) == (1, 2) and M.flip_masks(range(8)) == M.flip_masks("all")
    bad = [(), [], (1, 1), (0, 8), (-1,), (1.0,), (1.5,), ("1",), "ALL", "", "none", 3, (True,), (None,), [[1]], 2.0]
    for f in bad:
        with pytest.raises(ValueError):
            M.flip_masks(f)
    net = M.PHISeg3D(4, 3, [8, 16, 16], latent_levels=2, device="cpu", image_size=(4, 16, 16, 8))
    net.eval()
    vol = torch.zeros(1, 4, 21, 18, 13)
    for f in bad:
        with pytest.raises(ValueError):                                             # before any device work: this model has no device
            net.predict_volume(vol, flips=f)
    for f in ("all", (0,), (7, 1)):
        with pytest.raises(_ffi.UzError):                                           # good arguments: structure-only model, no fallback
            net.predict_volume(vol, flips=f)
    # the harness hands the keyword on; without `window` it is an error
    from unet_zoo_amd import train_model as TM
    seen = {}

    class Net:
        def eval(self):
            pass

        def predict(self, patch, n_samples=1):
            return "predict"

        def predict_volume(self, patch, **kw):
            seen.update(kw)
            return "volume"
    h = types.SimpleNamespace(net=Net(), device="cpu")
    x = np.zeros((1, 4, 5, 6, 7), np.float32)
    assert TM.UNetModel.predict(h, x, window=(16, 16, 8), flips="all") == "volume" and seen["flips"] == "all" and seen["window"] == (16, 16, 8)
    assert TM.UNetModel.predict(h, x, window=(16, 16, 8)) == "volume" and seen["flips"] is None
    assert TM.UNetModel.predict(h, x) == "predict"
    for f in ("all", (0,), ()):
        with pytest.raises(ValueError, match="window"):
            TM.UNetModel.predict(h, x, flips=f)


# ------------------------------------------------------------------------------------------ the C entry points
def test_the_entry_points_are_declared_and_exported():
    L, protos = _ffi.lib(), _ffi.prototypes()
    names = ("uz_vol_window_accum_ex", "uz_vol_window_gather_ex", "uz_vol_window_noise")
    assert set(names) <= set(_ffi.header_symbols()) and all(hasattr(L, n) for n in names)
    assert [len(protos[n][1]) for n in names] == [23, 15, 15]
    for old, new in (("uz_vol_window_accum", "uz_vol_window_accum_ex"), ("uz_vol_window_gather", "uz_vol_window_gather_ex")):
        assert protos[new][1] == protos[old][1][:-1] + [ctypes.c_int, ctypes.c_void_p]   # the old arguments, the mask, the stream


def test_the_entry_points_refuse_bad_arguments_on_the_host():
    L = _ffi.lib()
    cell = (ctypes.c_double * 64)()
    p = ctypes.addressof(cell)

    def accum(ptrs=(p, p), ctot=(3, 3), f=(1, 2), fz=(1, 2), Lv=2, K=3, win=(4, 4, 4), org=(0, 0, 0), dhw=(5, 6, 7), tabs=(p, p, p), acc=p, wsum=p,
              tables=True, flip=5):
        n = len(ptrs)
        arr = [(ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*ctot), (ctypes.c_int * n)(*f), (ctypes.c_int * n)(*fz)]
        if not tables:
            arr[0] = None
        return L.uz_vol_window_accum_ex(*arr, Lv, K, *win, *org, *dhw, *tabs, acc, wsum, 1, flip, None)
    for bad in (dict(flip=8), dict(flip=-1), dict(flip=64), dict(K=0), dict(K=9), dict(Lv=0), dict(Lv=9), dict(ptrs=(p, None)), dict(tables=False),
                dict(acc=None), dict(wsum=None), dict(tabs=(None, p, p)), dict(tabs=(p, None, p)), dict(tabs=(p, p, None)), dict(f=(1, 0)),
                dict(fz=(0, 2)), dict(ctot=(3, 2)), dict(win=(3, 4, 4)), dict(win=(4, 4, 6)), dict(win=(0, 4, 4)), dict(win=(4, -4, 4)),
                dict(org=(-4, 0, 0)), dict(org=(0, 0, -1)), dict(dhw=(0, 6, 7)), dict(dhw=(2048, 1024, 1024)), dict(win=(2048, 1024, 1024))):
        assert accum(**bad) == -1, bad
        assert b"vol_window_accum" in L.uz_last_error()
    assert b"flip" in (accum(flip=8), L.uz_last_error())[1]

    def gather(src=p, C=2, dhw=(5, 6, 7), org=(0, 0, 0), dst=p, ctot=2, win=(4, 4, 4), flip=3):
        return L.uz_vol_window_gather_ex(src, C, *dhw, *org, dst, ctot, *win, flip, None)
    for bad in (dict(flip=8), dict(flip=-1), dict(src=None), dict(dst=None), dict(C=0), dict(ctot=1), dict(dhw=(5, 0, 7)), dict(win=(4, 4, 0)),
                dict(win=(4, -4, 4)), dict(org=(0, -4, 0)), dict(dhw=(2048, 1024, 1024)), dict(win=(2048, 1024, 1024))):
        assert gather(**bad) == -1, bad
        assert b"vol_window_gather" in L.uz_last_error()
    assert b"flip" in (gather(flip=9), L.uz_last_error())[1]

    def noise(field=p, C2=2, size=(6, 5, 7), org=(1, 2, 3), crop=(4, 3, 2), flip=6, dst=p, ctot=2):
        return L.uz_vol_window_noise(field, C2, *size, *org, *crop, flip, dst, ctot, None)
    for bad in (dict(flip=8), dict(flip=-1), dict(field=None), dict(dst=None), dict(C2=0), dict(ctot=1), dict(size=(6, 0, 7)), dict(size=(-6, 5, 7)),
                dict(crop=(0, 3, 2)), dict(crop=(4, 3, -2)), dict(org=(-1, 2, 3)), dict(org=(3, 2, 3)), dict(org=(1, 3, 3)), dict(org=(1, 2, 6)),
                dict(crop=(6, 3, 2)), dict(crop=(4, 4, 2)), dict(crop=(4, 3, 5)), dict(org=(2 ** 31 - 2, 2, 3)),
                dict(size=(2048, 1024, 1024), org=(0, 0, 0)), dict(size=(2048, 1024, 1024), org=(0, 0, 0), crop=(2048, 1024, 1024))):
        assert noise(**bad) == -1, bad
        assert b"vol_window_noise" in L.uz_last_error()
    assert b"leaves its field" in (noise(org=(3, 2, 3)), L.uz_last_error())[1]
