"""CPU tier of PHISeg3D.predict_volume: the window grid and the blend weights (models/phiseg3D.py) against their restatement and
their properties, the defaults and every argument error, the refusals of the three entry points of csrc/volwindow.hip - decided on
the host, so they show without a device -, and the proof that the case set of tests/_volwindow.py tells a wrong evaluation from a
right one: the twin passes the gates, and the reference with each deliberate defect fails them on some case."""
import ctypes

import numpy as np
import pytest

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi
from unet_zoo_amd.models import phiseg3D as M
from tests import _volwindow as VW

GRIDS = [(c.dhw, c.window, c.stride, c.g) for c in VW.CASES] + [
    ((240, 240, 155), (128, 128, 128), (64, 64, 64), 16), ((240, 240, 155), (240, 240, 160), None, 16), ((21, 18, 13), (16, 16, 8), (8, 8, 4), 4),
    ((13, 10, 7), (16, 16, 8), None, 4), ((33, 7, 65), (16, 8, 32), (4, 8, 12), 4), ((5, 5, 5), (2, 2, 2), (1, 1, 2), 1)]


def _net(image_size=(4, 16, 16, 8), filters=(8, 16, 16), **kw):
    return M.PHISeg3D(4, 3, list(filters), latent_levels=2, device="cpu", image_size=image_size, **kw)


# ------------------------------------------------------------------------------------------ grid
@pytest.mark.parametrize("dhw,window,stride,g", GRIDS)
def test_window_grid_properties(dhw, window, stride, g):
    padded, extent, origins = M.window_grid(dhw, window, stride, g)
    assert (padded, extent, origins) == VW.window_grid(dhw, window, stride, g)
    s = VW.default_stride(window, g) if stride is None else stride
    assert padded == tuple(-(-n // g) * g for n in dhw)
    cover = np.zeros(padded, np.int64)
    for o in origins:
        assert all(q % g == 0 and q >= 0 for q in o)                                # crops of the noise at every latent level exist
        assert all(q + e <= p for q, e, p in zip(o, extent, padded))
        cover[o[0]:o[0] + extent[0], o[1]:o[1] + extent[1], o[2]:o[2] + extent[2]] += 1
    assert cover.min() >= 1                                                         # every voxel, padding included
    for a in range(3):
        axis = sorted({o[a] for o in origins})
        if padded[a] <= window[a]:
            assert axis == [0] and extent[a] == padded[a]                           # one window, shrunk to the padded side
        else:
            assert extent[a] == window[a] and axis[-1] + window[a] == padded[a]      # the last window ends at P
            assert axis[:-1] == list(range(0, padded[a] - window[a], s[a]))
    # the order of the visits: D slowest, W fastest
    assert origins == sorted(origins) and len(set(origins)) == len(origins)
    if all(x == w for x, w in zip(s, window)) and all(p % w == 0 for p, w in zip(padded, extent)):
        assert cover.max() == 1                                                     # stride == window: a disjoint cover


def test_the_cases_have_the_grids_the_issue_names():
    counts = tuple(len(VW.window_grid(c.dhw, c.window, c.stride, c.g)[2]) for c in VW.CASES)
    assert counts == VW.WINDOW_COUNTS
    cover = lambda c: VW.case(VW.CASES.index(c), 1, 1, "uniform")["ref"]["count"]   # noqa: E731
    assert cover(VW.CASES[0]).max() == 8 and cover(VW.CASES[2]).max() == 1 and cover(VW.CASES[4]).max() == 2
    assert VW.window_grid((5, 7, 9), (8, 8, 8), (4, 4, 4), 4) == ((8, 8, 12), (8, 8, 8), [(0, 0, 0), (0, 0, 4)])
    assert VW.window_grid((1, 1, 1), (4, 4, 4), None, 4) == ((4, 4, 4), (4, 4, 4), [(0, 0, 0)])
    assert len(M.window_grid((240, 240, 155), (128,) * 3, (64,) * 3, 16)[2]) == 18
    assert len(M.window_grid((21, 18, 13), (16, 16, 8), (8, 8, 4), 4)[2]) == 12
    assert M.window_grid((13, 10, 7), (16, 16, 8), None, 4) == ((16, 12, 8), (16, 12, 8), [(0, 0, 0)])
    assert {(len(c.factors), c.factors[-1][0] != c.factors[-1][1]) for c in VW.CASES} >= {(1, False), (3, False), (2, True)}
    assert any(c.extra == 3 and c.c0 == 2 for c in VW.CASES)


@pytest.mark.parametrize("blend", VW.BLENDS)
def test_blend_weights_are_positive_and_symmetric(blend):
    for extent in [(8, 8, 8), (4, 12, 16), (1, 2, 3), (128, 128, 128), (240, 240, 160)]:
        got, want = M.blend_tables(extent, blend), VW.blend_tables(extent, blend)
        for t, r, w in zip(got, want, extent):
            assert t.dtype == np.float64 and t.shape == (w,) and np.array_equal(t, r)
            assert np.all(t > 0) and np.all(t <= 1) and np.array_equal(t, t[::-1])
            if blend == "gaussian" and w > 2:
                assert np.all(np.diff(t[:(w + 1) // 2]) > 0)
                assert t[0] == np.exp(-0.5 * ((0 - (w - 1) / 2) / (w / 8)) ** 2)
        assert float(got[0][0] * got[1][0] * got[2][0]) > 1e-12                     # a corner voxel keeps a weight far from underflow
    with pytest.raises(ValueError):
        M.blend_tables((8, 8, 8), "cosine")


def test_defaults_and_argument_errors():
    net = _net()
    assert net.window_plan((21, 18, 13)) == M.window_grid((21, 18, 13), (16, 16, 8), (8, 8, 4), 4)
    assert M.default_stride((16, 16, 8), 4) == (8, 8, 4) and M.default_stride((4, 12, 20), 4) == (4, 4, 8) and M.default_stride((128,) * 3, 16) == (64,) * 3
    assert net.window_plan((21, 18, 13), window=(8, 8, 8))[1] == (8, 8, 8)
    bad = [dict(window=(16, 16, 6)), dict(window=(16, 16, 0)), dict(window=(16, 16)), dict(window=(16, -4, 8)), dict(stride=(8, 8, 2)),
           dict(stride=(8, 8, 12)), dict(stride=(0, 8, 4)), dict(stride=(8, 6, 4)), dict(stride=(8, 8)), dict(window=(16.5, 16, 8))]
    for kw in bad:
        with pytest.raises(ValueError):
            net.window_plan((21, 18, 13), **kw)
    with pytest.raises(ValueError):
        net.window_plan((21, 0, 13))
    with pytest.raises(ValueError):
        _net(image_size=(128, 128, 1)).window_plan((21, 18, 13))                    # no (D, H, W) to default to
    # predict_volume: every argument error is a ValueError and comes before any device work (this model has no device)
    import torch
    net.eval()
    vol = torch.zeros(1, 4, 21, 18, 13)
    shapes = [(2, 2, 6, 5, 4), (2, 2, 12, 10, 8)]                                   # padded (24, 20, 16) / 4 and / 2, deepest first
    for kw in (dict(n_samples=0), dict(blend="cosine"), dict(window=(16, 16, 6)), dict(stride=(8, 8, 16)),
               dict(n_samples=2, eps=[torch.zeros(s) for s in shapes][:1]), dict(n_samples=2, eps=[torch.zeros(s) for s in shapes][::-1]),
               dict(n_samples=3, eps=[torch.zeros(s) for s in shapes])):
        with pytest.raises(ValueError):
            net.predict_volume(vol, **kw)
    for v in (vol[0], torch.cat([vol, vol]), vol[:, :3]):
        with pytest.raises(ValueError):
            net.predict_volume(v)
    with pytest.raises(_ffi.UzError):                                               # good arguments: structure-only model, no fallback
        net.predict_volume(vol, n_samples=2, eps=[torch.zeros(s) for s in shapes])


# ------------------------------------------------------------------------------------------ the C entry points
def test_the_entry_points_are_declared_and_exported():
    L, protos = _ffi.lib(), _ffi.prototypes()
    names = {"uz_vol_window_gather", "uz_vol_window_accum", "uz_vol_window_finish"}
    assert names <= set(_ffi.header_symbols()) and all(hasattr(L, n) for n in names)
    assert [len(protos[n][1]) for n in sorted(names)] == [22, 13, 14]
    assert not any("WINDOW" in c for c in _ffi.op_codes())                          # called through the ABI, never a tape op


def test_the_entry_points_refuse_bad_arguments_on_the_host():
    L = _ffi.lib()
    cell = (ctypes.c_double * 64)()
    p = ctypes.addressof(cell)

    def accum(ptrs=(p, p), ctot=(3, 3), f=(1, 2), fz=(1, 2), Lv=2, K=3, win=(4, 4, 4), org=(0, 0, 0), dhw=(5, 6, 7), tabs=(p, p, p), acc=p, wsum=p,
              tables=True):
        n = len(ptrs)
        arr = [(ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*ctot), (ctypes.c_int * n)(*f), (ctypes.c_int * n)(*fz)]
        if not tables:
            arr[0] = None
        return L.uz_vol_window_accum(*arr, Lv, K, *win, *org, *dhw, *tabs, acc, wsum, 1, None)
    for bad in (dict(K=0), dict(K=9), dict(Lv=0), dict(Lv=9), dict(ptrs=(p, None)), dict(tables=False), dict(acc=None), dict(wsum=None),
                dict(tabs=(None, p, p)), dict(tabs=(p, None, p)), dict(tabs=(p, p, None)), dict(f=(1, 0)), dict(fz=(0, 2)), dict(ctot=(3, 2)),
                dict(win=(3, 4, 4)), dict(win=(4, 4, 6)), dict(win=(4, 6, 4)), dict(win=(0, 4, 4)), dict(win=(4, -4, 4)), dict(org=(-4, 0, 0)),
                dict(org=(0, 0, -1)), dict(dhw=(0, 6, 7)), dict(dhw=(2048, 1024, 1024)), dict(win=(2048, 1024, 1024))):
        assert accum(**bad) != 0, bad
        assert b"vol_window_accum" in L.uz_last_error()

    def gather(src=p, C=2, dhw=(5, 6, 7), org=(0, 0, 0), dst=p, ctot=2, win=(4, 4, 4)):
        return L.uz_vol_window_gather(src, C, *dhw, *org, dst, ctot, *win, None)
    for bad in (dict(src=None), dict(dst=None), dict(C=0), dict(ctot=1), dict(dhw=(5, 0, 7)), dict(win=(4, 4, 0)), dict(win=(4, -4, 4)),
                dict(org=(0, -4, 0)), dict(dhw=(2048, 1024, 1024)), dict(win=(2048, 1024, 1024))):
        assert gather(**bad) != 0, bad
        assert b"vol_window_gather" in L.uz_last_error()
    for args in ((None, p, 3, 2, 2, 4, 4, p, p, p, p, p), (p, None, 3, 2, 2, 4, 4, p, p, p, p, p), (p, p, 3, 2, 2, 4, 4, None, p, p, p, p),
                 (p, p, 3, 2, 2, 4, 4, p, p, None, p, p), (p, p, 0, 2, 2, 4, 4, p, p, p, p, p), (p, p, 9, 2, 2, 4, 4, p, p, p, p, p),
                 (p, p, 3, 0, 2, 4, 4, p, p, p, p, p), (p, p, 3, 2, 2, 0, 4, p, p, p, p, p), (p, p, 3, 2, 2048, 1024, 1024, p, p, p, p, p)):
        assert L.uz_vol_window_finish(*args, None) != 0, args
        assert b"vol_window_finish" in L.uz_last_error()


# ------------------------------------------------------------------------------------------ the cases discriminate
def test_gather_twin_is_a_zero_padded_crop():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((2, 5, 7, 9)).astype(np.float32)
    big = np.zeros((2, 16, 16, 24), np.float32)
    big[:, :5, :7, :9] = src
    for o in [(0, 0, 0), (0, 0, 4), (4, 4, 8), (8, 8, 8)]:
        assert np.array_equal(VW.gather_twin(src, o, (8, 8, 8)), big[:, o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8])


def test_the_logits_are_exact_in_fp32_and_hold_the_planted_blocks():
    for i, c in enumerate(VW.CASES):
        d = VW.case(i, 3, 3, "gaussian")
        for w in d["wins"]:
            assert [lv.shape[2:] for lv in w] == [VW.level_shape(d["extent"], fac) for fac in c.factors]
            for lv in w:
                assert np.array_equal(lv * 4, np.round(lv * 4)) and np.abs(lv).max() <= 8
            assert np.array_equal(VW.summed_logits(w, c.factors, np.float32), VW.summed_logits(w, c.factors, np.float64))


@pytest.mark.parametrize("blend", VW.BLENDS)
@pytest.mark.parametrize("S", VW.STATS_S)
@pytest.mark.parametrize("K", VW.STATS_K)
def test_twin_meets_the_gates_and_the_exempt_share_stays_under_the_cap(K, S, blend):
    for i, c in enumerate(VW.CASES):
        d = VW.case(i, K, S, blend)
        tw, ref, (pin, mpin, struct) = d["twin"], d["ref"], d["pins"]
        failed, fig = VW.gates(tw, tw, ref, d["pins"], S)
        assert not failed, (VW.case_id(c), K, S, blend, fig)
        assert tw["soft"].dtype == np.float32 and tw["labels"].dtype == np.uint8 and tw["labels"].shape == (S, *c.dhw)
        # the reference's own labels agree with the twin's where the rule pins them
        assert not np.any((ref["labels"] != tw["labels"]) & pin) and not np.any((ref["mean_label"] != tw["mean_label"]) & mpin)
        exempt = max(float(np.mean(~pin[s])) for s in range(S))
        assert exempt <= VW.EXEMPT_CAP and float(np.mean(~mpin)) <= VW.EXEMPT_CAP, (VW.case_id(c), K, S, blend, exempt)
        if K >= 2:
            assert struct.any(), (VW.case_id(c), K, S, blend)                      # first maximum wins is exercised
        assert np.all(ref["entropy"] >= 0) and np.all(ref["entropy"] <= np.log(K) + 1e-12)
        assert np.allclose(ref["mean_soft"].sum(axis=0), 1.0, atol=1e-12) and np.all(ref["count"] >= 1)


@pytest.mark.parametrize("defect", VW.DEFECTS)
def test_every_defect_leaves_the_gates_on_some_case(defect):
    caught = []
    for key in VW.all_keys():
        d = VW.case(*key)
        if defect == "uniform_for_gaussian" and key[3] != "gaussian":
            continue
        bad = VW.evaluate(*d["args"], "ref", defect=defect)
        failed, fig = VW.gates(bad, d["twin"], d["ref"], d["pins"], key[2])
        if failed:
            caught.append((key, failed))
    print(defect, "caught on", len(caught), "of", len(VW.all_keys()), "evaluations; first:", caught[:2])
    assert caught, defect
    if defect == "labels_after_rounding":                                          # only the labels can show it
        assert all(set(f) <= {"labels"} for _, f in caught)
