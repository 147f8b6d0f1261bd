"""Binary morphology and lesion-wise scores without a GPU: the morphology twin of tests/_lesions.py is scipy.ndimage.binary_dilation /
binary_erosion on every case, the lesion twin agrees with a brute-force restatement that dilates every lesion on its own, every
deliberate defect of the twins changes what the cases named here expect, the route calls and the workspace sizes claim what the launches
use, a bad call is refused with its reason before anything is launched (the library loads, and refuses, without a device), and the
Python functions check their arguments before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import _lesions as Z


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


# ================================================================================================ the case sets
def test_case_sets_hold_what_the_kernels_can_get_wrong():
    assert tuple(c.name for c in Z.morph_cases()) == Z.MORPH_NAMES and tuple(c.name for c in Z.lesion_cases()) == Z.LESION_NAMES
    shapes = [c.vol.shape for c in Z.morph_cases()] + [c.pred.shape for c in Z.lesion_cases()]
    assert {s[3] for s in shapes} >= set(Z.WIDTHS)                       # the word boundary, the pad bits and the carry between words at an edge
    assert any(s[1] == 1 for s in shapes) and any(s[2] == 1 and s[1] > 1 for s in shapes) and any(s[1] == 1 and s[2] == 1 for s in shapes)
    assert {c.vol.shape[0] for c in Z.morph_cases()} >= {1, 3}
    for c in Z.morph_cases():
        assert c.vol.dtype == np.uint8 and c.vol.size <= 8000
        fg = Z.in_set(c.vol, c.values)
        if c.name not in ("full", "empty"):
            N, D, H, W = fg.shape
            assert all(fg[:, z, y, x].all() for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)), c.name      # every corner
            assert fg[:, 0].any() and fg[:, -1].any() and fg[:, :, 0].any() and fg[:, :, -1].any() and fg[..., 0].any() and fg[..., -1].any()
            assert (c.vol >= 32).any() and not fg.all()
            if N > 1:
                assert not np.array_equal(c.vol[0], c.vol[1])
    assert Z.in_set(Z.morph_case("full").vol, (1, 3)).all() and not Z.in_set(Z.morph_case("empty").vol, (1, 3)).any()
    # something is left to compare at every depth: an erosion that still has voxels after three passes, in 3-D and in 2-D, across a word
    # boundary; a dilation that still grows in its third pass
    for name in ("block", "flat65", "slab130"):
        for conn in Z.CONN:
            assert Z.expected_morph(name, conn, 3, 1).any(), (name, conn)
    for name in ("sparse65", "sparse155", "sparse_flat64"):
        for conn in Z.CONN:
            sums = [int(Z.expected_morph(name, conn, it, 0).sum()) for it in Z.ITERATIONS]
            assert sums[0] < sums[1] < sums[2] < sums[3] < Z.morph_case(name).vol.size, (name, conn, sums)
    # the three structures disagree
    for name, erodes in (("sparse65", (0,)), ("block", (0, 1)), ("w155", (1,))):
        for erode in erodes:
            outs = [Z.expected_morph(name, conn, 1, erode) for conn in Z.CONN]
            assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]), (name, erode)
    for c in Z.lesion_cases():
        assert c.pred.dtype == np.uint8 and c.ref.dtype == np.uint8 and c.ref.size <= 13000 and c.pred.shape[1:] == c.ref.shape


def test_lesion_cases_hold_what_the_issue_lists():
    cnt = {name: Z.expected_lesions(name)[0] for name in Z.LESION_NAMES}
    les = {name: Z.expected_lesions(name)[1] for name in Z.LESION_NAMES}
    sc = {name: Z.expected_lesions(name)[2] for name in Z.LESION_NAMES}
    col = {k: i for i, k in enumerate(Z.COUNT_NAMES)}
    # gaps: of the two distances per direction the smaller one is closed (one lesion of two voxels), the larger is not (two of one)
    assert cnt["gaps"][0, 0, col["n_ref"]] == 9 and sorted(les["gaps"][0, 0, :9, 0].tolist()) == [1] * 6 + [2] * 3
    ref = Z.lesion_case("gaps").ref
    joined = {}
    for conn in Z.CONN:                                                   # there the 6-, 18- and 26-structures disagree
        joined[conn] = int(ndimage.label(Z.morph_mask(Z.in_set(ref, (1,))[None], conn, 1, 0)[0], structure=Z.S26)[1])
    assert joined == {1: 11, 2: 9, 3: 8}, joined
    assert sc["gaps"][0, 0, 0] == 1.0 and cnt["gaps"][1, 0, col["n_fp"]] == 1
    # span: the bar is one component in the pred_vol of both lesions, with its full size; the U is counted once although it enters twice
    bar = int(Z.in_set(Z.lesion_case("span").pred[0], (1,)).sum())
    assert cnt["span"][0, 0, col["n_pred"]] == 1 and les["span"][0, 0, :2, 2].tolist() == [bar, bar] and les["span"][0, 0, :2, 1].tolist() == [2, 2]
    c = Z.lesion_case("span")
    Dk = Z.morph_mask(Z.in_set(c.ref, (1,))[None], 2, 1, 0)[0]
    Lg = ndimage.label(Dk, structure=Z.S26)[0]
    u = Z.in_set(c.pred[1], (1,)) & (ndimage.label(Z.in_set(c.pred[1], (1,)), structure=Z.S26)[0] == 1)
    assert ndimage.label(u & (Lg == 1), structure=Z.S26)[1] == 2 and (u & ~Dk).any()            # inside, outside, inside again
    assert les["span"][1, 0, 0, 2] == int(u.sum()) and cnt["span"][1, 0, col["n_fp"]] == 1
    assert cnt["span"][2, 0].tolist() == [2, 2, 0, 2, 0, 0, 0, 0] and sc["span"][2, 0].tolist() == [0.0, 0.0, 1.0, 0.0]    # an empty prediction
    # thresholds: 5 voxels dropped, 6 kept; the component on the dropped lesion is no false positive; 2 voxels are below min_pred_voxels, 3 not
    p = Z.lesion_case("thresholds").params
    gt = les["thresholds"][0, 0, :5, 0].tolist()
    assert p["min_ref_voxels"] - 1 in gt and p["min_ref_voxels"] in gt and cnt["thresholds"][0, 0, :2].tolist() == [5, 4]
    assert cnt["thresholds"][0, 0, col["n_fp"]] == 1 and cnt["thresholds"][0, 0, col["n_pred"]] == 7 and les["thresholds"][0, 0, gt.index(5)].tolist() == [5, 0, 3]
    assert cnt["thresholds"][1, 0, col["n_fn"]] == 1
    # empty reference with and without a prediction
    assert sc["empty_ref"][0, 0, 0] == 0.0 and cnt["empty_ref"][0, 0, col["n_fp"]] == 2 and sc["empty_ref"][1, 0].tolist() == [1.0] * 4
    # nested regions: three different answers per row
    assert cnt["nested"].shape == (3, 3, 8) and len({tuple(r) for r in cnt["nested"][1].tolist()}) == 3
    # the tables one too small
    n_ref = int(cnt["speckle"][0, 0, 0])
    assert Z.lesion_case("speckle_exact").params["max_lesions"] == n_ref and Z.lesion_case("speckle_short").params["max_lesions"] == n_ref - 1
    assert not np.isnan(sc["speckle_exact"]).any() and np.isnan(sc["speckle_short"]).all() and (cnt["speckle_short"][..., 6] == 1).all()
    assert np.array_equal(sc["speckle_exact"], sc["speckle"]) and np.array_equal(cnt["speckle_exact"], cnt["speckle"])
    assert not np.isnan(sc["links_fit"]).any() and cnt["links_fit"][..., 7].tolist() == [[0], [0]]
    assert np.isnan(sc["links_short"][0]).all() and not np.isnan(sc["links_short"][1]).any() and cnt["links_short"][..., 7].tolist() == [[1], [0]]
    assert int(cnt["speckle"][0, 0, col["n_pred"]]) > 100 and int(cnt["speckle"][1, 0, col["n_tp"]]) == n_ref


# ================================================================================================ the twins against scipy and brute force
@pytest.mark.parametrize("name", Z.MORPH_NAMES)
def test_morphology_twin_is_scipy_on_every_case(name):
    c = Z.morph_case(name)
    for conn, it, erode in Z.MORPH_PARAMS:
        assert np.array_equal(Z.expected_morph(name, conn, it, erode), Z.scipy_morph(c.vol, c.values, conn, it, erode)), (name, conn, it, erode)


@pytest.mark.parametrize("name", Z.LESION_NAMES)
def test_lesion_twin_agrees_with_the_brute_force_restatement(name):
    c = Z.lesion_case(name)
    p = c.params
    # the restatement has no tables: compare with a twin whose tables are large enough
    cnt, les, sc = Z.lesion_scores(c.pred, c.ref, c.pred_regions, c.ref_regions, **dict(p, max_lesions=1024, max_links=16))
    assert not cnt[..., 6:].any()
    bf = Z.brute_force(c.pred, c.ref, c.pred_regions, c.ref_regions, p["dilation"], p["min_ref_voxels"], p["min_pred_voxels"])
    for (n, r), (rows, n_kept, n_fp, mean) in bf.items():
        assert len(rows) == cnt[n, r, 0] and n_kept == cnt[n, r, 1] and n_fp == cnt[n, r, 4], (name, n, r)
        assert [tuple(x) for x in les[n, r, :len(rows)].tolist()] == rows, (name, n, r)
        assert abs(mean - sc[n, r, 0]) <= 1e-12, (name, n, r, mean, sc[n, r, 0])       # np.sum adds pairwise, the twin serially


# which cases notice which defect
NOTICED_BY = {"dil_structure": ("gaps",), "dk6": ("gaps", "speckle"), "pred6": ("speckle", "nested"), "predvol_in_dk": ("span",), "pair_twice": ("span",),
              "first_lesion_only": ("span", "links_fit"), "dropped_as_missed": ("thresholds",), "dropped_fp": ("thresholds",), "thr_gt": ("thresholds",),
              "empty_zero": ("empty_ref",), "inter_dk": ("span", "thresholds"), "rows_wrap": ("w155", "flat65", "sparse155"),
              "pad_leak": ("w63", "w155", "flat65", "slab130"), "iter_short": ("sparse65", "block")}


@pytest.mark.parametrize("defect", Z.DEFECTS)
def test_every_defect_changes_what_the_named_cases_expect(defect):
    assert set(NOTICED_BY) == set(Z.DEFECTS)
    for name in NOTICED_BY[defect]:
        if defect in Z.MORPH_DEFECTS:
            c = Z.morph_case(name)
            changed = [(conn, it, e) for conn, it, e in Z.MORPH_PARAMS
                       if not np.array_equal(Z.morph(c.vol, c.values, conn, it, e, defects=(defect,)), Z.expected_morph(name, conn, it, e))]
            assert changed, (defect, name)
            if defect == "pad_leak":                                      # an erosion's defect: a dilation never reads a pad bit back into the row
                assert {e for _, _, e in changed} == {1}
        else:
            c = Z.lesion_case(name)
            bad = Z.lesion_scores(c.pred, c.ref, c.pred_regions, c.ref_regions, defects=(defect,), **c.params)
            good = Z.expected_lesions(name)
            assert not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(bad, good)), (defect, name)
    if defect == "iter_short":                                            # a defect of the dilation shows in the lesions too
        c = Z.lesion_case("gaps")
        G = Z.in_set(c.ref, (1,))[None]
        assert not np.array_equal(Z.morph_mask(G, 2, 1, 0, defects=(defect,)), Z.morph_mask(G, 2, 1, 0))


# ================================================================================================ route, workspace, refusals
def test_route_claims_and_workspace_sizes():
    L, _ = _lib()
    out = (C.c_int * 2)()
    up16 = lambda b: (b + 15) // 16 * 16
    for N, D, H, W in [(1, 1, 1, 1), (3, 4, 6, 63), (1, 5, 9, 155), (1, 1, 24, 65), (3, 3, 1, 64), (1, 6, 7, 1), (17, 128, 128, 128), (17, 155, 240, 240), (65536, 1, 1, 1)]:
        rows, WW = N * D * H, -(-W // 64)
        assert L.uz_vol_morph_route(N, D, H, W, out) == 0, L.uz_last_error()
        widest = max(min(-(-rows // 4), 1 << 16), min(-(-rows * WW // 256), 1 << 18), min(-(-rows * W // 256), 1 << 18))
        assert tuple(out) == (WW, widest), ((N, D, H, W), tuple(out), widest)
        assert L.uz_vol_morph_workspace(N, D, H, W) == 2 * up16(8 * rows * WW)
        for R, ML in ((1, 1), (3, 256), (8, 4096)):
            P, T = D * H * W, N * D * H * W
            want = (L.uz_vol_components_workspace(N, D, H, W) + L.uz_vol_morph_workspace(1, D, H, W) + up16(P) + 2 * up16(4 * P) + 2 * up16(4 * T)
                    + up16(4 * (-(-P // 256) + 1)) + up16(4 * (ML * (1 + 2 * N) + 4 * N)))
            assert L.uz_vol_lesion_scores_workspace(N, R, D, H, W, ML) == want, (N, R, D, H, W, ML)
            assert L.uz_vol_lesion_scores_route(N, R, D, H, W, out) == 0, L.uz_last_error()
            comp, mor = (C.c_int * 2)(), (C.c_int * 2)()
            assert L.uz_vol_components_route_ex(N, D, H, W, 3, comp) == 0 and L.uz_vol_morph_route(1, D, H, W, mor) == 0
            assert tuple(out) == (3, max(comp[1], mor[1], min(-(-T // 256), 1 << 18), -(-P // 256))), ((N, R, D, H, W), tuple(out))
    assert L.uz_vol_morph_workspace(17, 155, 240, 240) == 2 * 17 * 155 * 240 * 4 * 8            # a 64th of the volume and the padding, twice
    for N, D, H, W in [(0, 8, 8, 8), (65537, 1, 1, 1), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (2, 1024, 1024, 1024), (65536, 32768, 1, 1)]:
        assert L.uz_vol_morph_workspace(N, D, H, W) == 0 and L.uz_vol_lesion_scores_workspace(N, 1, D, H, W, 16) == 0, (N, D, H, W)
        assert L.uz_vol_morph_route(N, D, H, W, out) != 0 and L.uz_last_error().decode().startswith("vol_morph_route:"), (N, D, H, W)
        assert L.uz_vol_lesion_scores_route(N, 1, D, H, W, out) != 0 and L.uz_last_error().decode().startswith("vol_lesion_scores_route:"), (N, D, H, W)
    for R, ML in [(0, 16), (9, 16), (1, 0), (1, 4097)]:
        assert L.uz_vol_lesion_scores_workspace(1, R, 8, 8, 8, ML) == 0, (R, ML)
    assert L.uz_vol_lesion_scores_workspace(1, 8, 8, 8, 8, 4096) > 0
    assert L.uz_vol_lesion_scores_route(1, 0, 8, 8, 8, out) != 0 and L.uz_vol_lesion_scores_route(1, 9, 8, 8, 8, out) != 0
    assert L.uz_vol_morph_route(1, 8, 8, 8, None) != 0 and L.uz_vol_lesion_scores_route(1, 1, 8, 8, 8, None) != 0


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written (the sets are host arrays by contract)."""
    L, _ = _lib()
    host = np.zeros(1 << 16, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    T = 2 * 8 * 8 * 8
    sets = (C.c_uint32 * 8)(*[0b1110, 0b1100, 0b1000, 2, 2, 2, 2, 2])
    sp = C.addressof(sets)

    def morph(vol=ptr, N=2, shape=(8, 8, 8), conn=2, it=1, erode=0, out=ptr + 4096, ws=ptr + 32768):
        rc = L.uz_vol_morph(vol, N, *shape, 2, conn, it, erode, out, ws, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(vol=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"), (dict(shape=(8, 0, 8)), "empty axis"), (dict(shape=(0, 8, 8)), "empty axis"),
                       (dict(shape=(8, 8, 0)), "empty axis"), (dict(N=0), "1 <= N <= 65536"), (dict(N=65537), "1 <= N <= 65536"), (dict(shape=(1024, 1024, 1024)), "2^31"),
                       (dict(conn=0), "connectivity 0"), (dict(conn=4), "connectivity 4"), (dict(it=-1), "iterations -1"), (dict(erode=2), "erode 2"), (dict(erode=-1), "erode -1"),
                       (dict(ws=ptr + 32768 + 8), "16-byte"), (dict(out=ptr), "overlaps"), (dict(out=ptr + T - 1), "overlaps"), (dict(vol=ptr + 4096, out=ptr + 4096 - T + 1), "overlaps")]:
        rc, msg = morph(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_morph:"), (kw.keys(), rc, msg)

    def lesion(pred=ptr, N=2, ps=sp, ref=ptr + 4096, rs=sp, R=3, shape=(8, 8, 8), dil=3, mr=50, mp=0, ML=16, links=4, ws=ptr + 65536, counts=ptr + 8192,
               lesions=ptr + 16384, scores=ptr + 12288):
        rc = L.uz_vol_lesion_scores(pred, N, ps, ref, rs, R, *shape, dil, mr, mp, ML, links, ws, counts, lesions, scores, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(pred=None), "null"), (dict(ps=None), "null"), (dict(ref=None), "null"), (dict(rs=None), "null"), (dict(ws=None), "null"), (dict(counts=None), "null"),
                       (dict(scores=None), "null"), (dict(shape=(8, 0, 8)), "empty axis"), (dict(N=0), "1 <= N <= 65536"), (dict(N=65537), "1 <= N <= 65536"),
                       (dict(shape=(1024, 1024, 1024)), "2^31"), (dict(R=0), "1 <= R <= 8"), (dict(R=9), "1 <= R <= 8"), (dict(dil=-1), "0 <= dilation <= 16"),
                       (dict(dil=17), "0 <= dilation <= 16"), (dict(mr=-1), ">= 0"), (dict(mp=-1), ">= 0"), (dict(ML=0), "1 <= max_lesions <= 4096"),
                       (dict(ML=4097), "1 <= max_lesions <= 4096"), (dict(links=0), "1 <= max_links <= 16"), (dict(links=17), "1 <= max_links <= 16"),
                       (dict(ws=ptr + 65536 + 8), "16-byte"), (dict(counts=ptr + 8196), "8-byte"), (dict(lesions=ptr + 16388), "8-byte"), (dict(scores=ptr + 12292), "8-byte")]:
        rc, msg = lesion(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_lesion_scores:"), (kw.keys(), rc, msg)
    assert not host.any()                                                 # a refused call writes nothing


# ================================================================================================ the Python functions
def test_argument_errors_of_the_python_functions():
    from unet_zoo_amd import metrics
    vol = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    for fn in (metrics.binary_dilation, metrics.binary_erosion, metrics.binary_opening, metrics.binary_closing):
        with pytest.raises(TypeError, match="uint8"):
            fn(vol.int(), (1,))
        with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
            fn(vol[0], (1,))
        with pytest.raises(ValueError, match="label value 32"):
            fn(vol, (1, 32))
        with pytest.raises(ValueError, match="connectivity 4"):
            fn(vol, (1,), connectivity=4)
        with pytest.raises(TypeError, match="connectivity"):
            fn(vol, (1,), connectivity=True)
        with pytest.raises(ValueError, match="iterations -1"):
            fn(vol, (1,), iterations=-1)
        with pytest.raises(TypeError, match="iterations"):
            fn(vol, (1,), iterations=1.0)
        with pytest.raises(ValueError, match="on the device"):
            fn(vol, (1,))
    ref = torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_lesions(vol.float(), ref, ((1,),))
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_lesions(vol, ref.int(), ((1,),))
    with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
        metrics.score_lesions(vol[0], ref, ((1,),))
    with pytest.raises(ValueError, match="does not match"):
        metrics.score_lesions(vol, ref[:3], ((1,),))
    with pytest.raises(ValueError, match="label value 40"):
        metrics.score_lesions(vol, ref, ((1, 40),))
    with pytest.raises(ValueError, match="2 regions of pred against 1"):
        metrics.score_lesions(vol, ref, ((1,), (2,)), ((1,),))
    for kw, exc, text in [(dict(dilation=-1), ValueError, "dilation -1"), (dict(dilation=17), ValueError, "dilation 17"), (dict(dilation=1.5), TypeError, "dilation"),
                          (dict(min_ref_voxels=-1), ValueError, "min_ref_voxels -1"), (dict(min_pred_voxels=-2), ValueError, "min_pred_voxels -2"),
                          (dict(max_lesions=0), ValueError, "max_lesions 0"), (dict(max_lesions=4097), ValueError, "max_lesions 4097"),
                          (dict(max_links=0), ValueError, "max_links 0"), (dict(max_links=17), ValueError, "max_links 17"), (dict(max_links=True), TypeError, "max_links")]:
        with pytest.raises(exc, match=text):
            metrics.score_lesions(vol, ref, ((1,),), **kw)
    with pytest.raises(ValueError, match="on the device"):
        metrics.score_lesions(vol, ref, ((1,),))
    assert metrics.LesionScores._fields == ("lesion_dice", "sensitivity", "precision", "f1", "counts", "lesions")
