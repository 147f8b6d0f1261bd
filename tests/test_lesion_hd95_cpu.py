"""The lesion-wise HD95 without a GPU: the twin of tests/_lesion_hd95.py agrees with a brute-force restatement on every case, every
deliberate defect of the twin changes what the cases named here expect, the case set holds what the contract's rules need, the route
and workspace calls claim what the launches use, a bad call is refused with its reason before anything is launched (the library
loads, and refuses, without a device), and score_lesions checks its new arguments before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _lesion_hd95 as HZ
from tests import _lesions as Z


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


@pytest.fixture(scope="module")
def tiles():
    """(Q, T): the queries of one workgroup of the pair kernel and the seeds of one LDS tile, as the library answers them"""
    L, _ = _lib()
    out = (C.c_int * 4)()
    assert L.uz_vol_lesion_scores_route_ex(1, 1, 8, 8, 8, 1, out) == 0, L.uz_last_error()
    assert out[2] >= 2 and out[3] >= 2
    return out[2], out[3]


# ================================================================================================ twin = brute force
@pytest.mark.parametrize("name", [n for n in HZ.NAMES if n not in HZ.OVERFLOW_NAMES])
def test_twin_agrees_with_the_brute_force_restatement(name, tiles):
    c = HZ.case(name, *tiles)
    p = c.params
    # the restatement has no tables and no lists: compare with a twin whose limits are large enough
    hd, hl, hc = HZ.lesion_hd95(c.pred, c.ref, c.pred_regions, c.ref_regions, **dict(p, max_lesions=1024, max_links=16, max_border=c.ref.size))
    assert not hc.any() and not np.isnan(hd).any()
    bf = HZ.brute_force_hd95(c.pred, c.ref, c.pred_regions, c.ref_regions, p["dilation"], p["min_ref_voxels"], p["min_pred_voxels"], p["hd95_penalty"])
    worst, far = 0.0, 0.0
    for (n, r), (rows, n_kept, n_fp, mean) in bf.items():
        assert not hl[n, r, len(rows):].any(), (name, n, r)
        for g, row in enumerate(rows):
            if row is None:
                assert not hl[n, r, g].any(), (name, n, r, g)
                continue
            assert hl[n, r, g].tolist() == list(row[:3]), (name, n, r, g, hl[n, r, g].tolist(), row)      # integer for integer
            twin_value = HZ.value_of(*hl[n, r, g].tolist())
            worst = max(worst, abs(twin_value - row[3]))
            far = max(far, row[3])
            assert abs(twin_value - row[3]) <= 1e-9, (name, n, r, g, twin_value, row[3])
        worst = max(worst, abs(mean - hd[n, r]))
        assert abs(mean - hd[n, r]) <= 1e-9, (name, n, r, mean, hd[n, r])                                # np.sum adds pairwise, the twin serially
    print(name, "largest hd95_g", far, "largest |twin - brute force|", worst)


# which cases notice which defect
NOTICED_BY = {"one_direction": ("span", "labels", "ellipsoids_40x48x33"), "a_is_dk": ("gaps", "labels"), "b_clipped": ("span", "thresholds"),
              "nearest_any": ("span", "speckle", "slabs_3x5x261"), "first_link_only": ("span", "links_fit"), "miss_zero": ("thresholds", "flat_1x17x19", "labels"),
              "fp_zero": ("thresholds", "empty_ref"), "dropped_penalised": ("thresholds",), "nearest_rank": ("speckle", "span"), "interp_sq": ("speckle", "span"),
              "faces_not_border": ("whole_volume_pred", "slabs_3x5x261"), "erosion26": ("labels", "ellipsoids_40x48x33"), "empty_one": ("empty_ref",)}


@pytest.mark.parametrize("defect", HZ.DEFECTS)
def test_every_defect_changes_what_the_named_cases_expect(defect, tiles):
    assert set(NOTICED_BY) == set(HZ.DEFECTS) and len(HZ.DEFECTS) == 13
    for name in NOTICED_BY[defect]:
        c = HZ.case(name, *tiles)
        bad = HZ.lesion_hd95(c.pred, c.ref, c.pred_regions, c.ref_regions, defects=(defect,), **c.params)
        good = HZ.expected(name, *tiles)
        assert not (np.array_equal(bad[0], good[0], equal_nan=True) and np.array_equal(bad[1], good[1])), (defect, name)


# ================================================================================================ the case set
def test_cases_hold_what_the_contract_needs(tiles):
    Q, T = tiles
    exp = {name: HZ.expected(name, Q, T) for name in HZ.NAMES}
    assert HZ.NAMES[:12] == Z.LESION_NAMES
    for c in HZ.cases(Q, T)[:12]:                                          # the twelve lesion cases with their own parameters
        assert HZ.lesion_params(c) == Z.lesion_case(c.name).params and c.pred is Z.lesion_case(c.name).pred
        assert c.params["hd95_penalty"] == 374.0 and c.params["max_border"] == min(max(4096, c.ref.size // 8), c.ref.size)
    hd, hl, hc = exp["speckle"]
    matched = hl[..., 0] > 0
    assert int(matched.sum()) == 46 and int((hl[..., 1] != hl[..., 2]).sum()) == 22 and (hl[..., 0][matched] >= 2).all()
    cnt = Z.expected_lesions("thresholds")[0]
    assert cnt[1, 0, 3] == 1 and cnt[0, 0, 4] == 1                        # a miss, and a false positive (the one of min_pred_voxels; the smaller is none)
    assert exp["empty_ref"][0].tolist() == [[374.0], [0.0]]               # only false positives: the penalty; nothing on either side: 0.0
    assert np.isnan(exp["links_short"][0][0, 0]) and not np.isnan(exp["links_short"][0][1, 0])
    assert np.isnan(exp["speckle_short"][0]).all() and int((exp["speckle_short"][1][..., 0] > 0).sum()) == 45
    hd, hl, hc = exp["labels"]
    assert sorted(hl[..., 0][hl[..., 0] > 0].tolist(), reverse=True)[:4] == [1116, 1052, 944, 460]
    assert hd[2, 2] == 374.0 and not hl[2, 2].any()                       # row 2's ET is a miss
    assert exp["ellipsoids_40x48x33"][1][0, 0, 0, 0] == 2731
    hl = exp["slabs_3x5x261"][1]
    assert int((hl[0, 0, :, 0] > 0).sum()) == 2 and int(hl[..., 2].max()) == 1370 and HZ.case("slabs_3x5x261", Q, T).ref.shape[2] > 256
    c = HZ.case("flat_1x17x19", Q, T)
    assert c.ref.shape[0] == 1 and int((exp["flat_1x17x19"][1][0, 0, :, 0] > 0).sum()) == 1 and Z.lesion_scores(c.pred, c.ref, c.pred_regions, **HZ.lesion_params(c))[0][0, 0, 3] == 1
    assert HZ.case("whole_volume_pred", Q, T).pred.all()
    # plates: Q - 1, Q, Q + 1 queries against T - 1, T, T + 1, 2 T + 1 seeds, every voxel a border voxel
    c = HZ.case("plates", Q, T)
    assert int(c.ref[0].sum()) == 5 * T + 1 and not c.ref[1:].any() and not c.pred[:, :2].any()
    hl = exp["plates"][1]
    ms = {(int(a), int(b)) for a in (T - 1, T, T + 1, 2 * T + 1) for b in (Q - 1, Q, Q + 1)}
    got = {(int(m) - q, q) for n in range(3) for g, m in enumerate(hl[n, 0, :4, 0]) for q in [(Q - 1, Q, Q + 1)[(g + n) % 3]]}      # m = seeds + queries
    assert got <= ms and len(got) == 12 and {a for a, _ in got} == {T - 1, T, T + 1, 2 * T + 1} and {b for _, b in got} == {Q - 1, Q, Q + 1}
    assert (hl[:, 0, :4, 1] >= 4).all()                                    # two slices away
    # border overflow: the lists exactly full, and one entry short
    n_a, n_e = HZ.border_sizes("speckle")
    assert [HZ.case(n, Q, T).params["max_border"] for n in HZ.OVERFLOW_NAMES] == [n_e, n_e - 1, n_a, n_a - 1] and n_a < n_e
    assert exp["entries_exact"][2].tolist() == [[[0, 0]], [[0, 0]]] and not np.isnan(exp["entries_exact"][0]).any()
    assert exp["entries_short"][2].tolist() == [[[0, 0]], [[0, 1]]] and np.isnan(exp["entries_short"][0]).tolist() == [[False], [True]]
    assert exp["ref_exact"][2][:, 0, 0].tolist() == [0, 0] and exp["ref_short"][2][:, 0, 0].tolist() == [1, 1] and np.isnan(exp["ref_short"][0]).all()
    assert not exp["ref_short"][1].any() and not exp["entries_short"][1][1].any() and exp["entries_short"][1][0].any()      # an overflowed row's table is 0
    for c in HZ.cases(Q, T):
        assert c.pred.dtype == np.uint8 and c.ref.dtype == np.uint8 and c.ref.size <= 64000 and c.pred.shape[1:] == c.ref.shape


# ================================================================================================ route, workspace, refusals
def test_route_claims_and_workspace_sizes(tiles):
    L, _ = _lib()
    up16 = lambda b: (b + 15) // 16 * 16
    o2, o4 = (C.c_int * 2)(), (C.c_int * 4)()
    for N, D, H, W in [(1, 1, 1, 1), (3, 4, 6, 63), (1, 5, 9, 155), (3, 3, 1, 64), (17, 128, 128, 128), (17, 155, 240, 240), (65536, 1, 1, 1)]:
        P = D * H * W
        for R, ML in ((1, 1), (3, 256), (8, 4096)):
            old = L.uz_vol_lesion_scores_workspace(N, R, D, H, W, ML)
            assert old > 0
            for mb in (0, 1, P, -5):                                      # without the HD95 nothing else is looked at
                assert L.uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, ML, 0, mb) == old
            for MB in {1, P, max(1, P // 8)}:
                want = (old + up16(4 * MB) + 3 * up16(4 * N * MB) + up16(8 * N * MB) + up16(4 * N * (ML + 1)) + up16(8 * N * ML)
                        + up16(8 * N + 4 * ((ML + 1) + ML + N * (ML + 1) + N * ML)))
                assert L.uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, ML, 1, MB) == want, (N, R, D, H, W, ML, MB)
            assert L.uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, ML, 1, 0) == 0 and L.uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, ML, 1, P + 1) == 0
            assert L.uz_vol_lesion_scores_route(N, R, D, H, W, o2) == 0
            for want_hd in (0, 1):
                assert L.uz_vol_lesion_scores_route_ex(N, R, D, H, W, want_hd, o4) == 0, L.uz_last_error()
                assert tuple(o4)[:2] == tuple(o2) and tuple(o4)[2:] == (tiles if want_hd else (0, 0))
    assert L.uz_vol_lesion_scores_workspace_ex(1, 1, 1, 1, 32769, 16, 1, 64) == 0 and L.uz_vol_lesion_scores_workspace_ex(1, 1, 1, 1, 32767, 16, 1, 64) > 0      # D^2 + H^2 + W^2 <= 2^30
    assert L.uz_vol_lesion_scores_workspace_ex(1, 1, 1, 1, 32769, 16, 0, 64) > 0
    for N, D, H, W in [(0, 8, 8, 8), (65537, 1, 1, 1), (1, 0, 8, 8), (2, 1024, 1024, 1024)]:
        assert L.uz_vol_lesion_scores_workspace_ex(N, 1, D, H, W, 16, 1, 8) == 0 and L.uz_vol_lesion_scores_workspace_ex(N, 1, D, H, W, 16, 0, 8) == 0
        assert L.uz_vol_lesion_scores_route_ex(N, 1, D, H, W, 1, o4) != 0 and L.uz_last_error().decode().startswith("vol_lesion_scores_route_ex:"), (N, D, H, W)
    assert L.uz_vol_lesion_scores_route_ex(1, 9, 8, 8, 8, 1, o4) != 0 and L.uz_vol_lesion_scores_route_ex(1, 1, 8, 8, 8, 1, None) != 0


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written"""
    L, _ = _lib()
    host = np.zeros(1 << 16, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    sets = (C.c_uint32 * 8)(*[0b1110, 0b1100, 0b1000, 2, 2, 2, 2, 2])
    sp = C.addressof(sets)
    box = C.c_double()

    def call(pred=ptr, N=2, ps=sp, ref=ptr + 4096, rs=sp, R=3, shape=(8, 8, 8), dil=3, mr=50, mp=0, ML=16, links=4, want=1, penalty=374.0, MB=64, ws=ptr + 65536,
             counts=ptr + 8192, lesions=ptr + 16384, scores=ptr + 12288, hc=ptr + 20480, hl=ptr + 24576, hd=ptr + 28672):
        box.value = 0.0 if penalty is None else penalty
        pp = None if penalty is None else C.addressof(box)
        rc = L.uz_vol_lesion_scores_ex(pred, N, ps, ref, rs, R, *shape, dil, mr, mp, ML, links, want, pp, MB, ws, counts, lesions, scores, hc, hl, hd, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(pred=None), "null"), (dict(ws=None), "null"), (dict(counts=None), "null"), (dict(scores=None), "null"), (dict(shape=(8, 0, 8)), "empty axis"),
                       (dict(N=0), "1 <= N <= 65536"), (dict(R=9), "1 <= R <= 8"), (dict(dil=17), "0 <= dilation <= 16"), (dict(ML=0), "1 <= max_lesions <= 4096"),
                       (dict(links=17), "1 <= max_links <= 16"), (dict(ws=ptr + 65536 + 8), "16-byte"), (dict(counts=ptr + 8196), "8-byte"),
                       # what the HD95 adds
                       (dict(hc=None), "null"), (dict(hd=None), "null"), (dict(penalty=None), "null"), (dict(shape=(1, 1, 32769)), "2^30"), (dict(MB=0), "1 <= max_border <= D*H*W"),
                       (dict(MB=513), "1 <= max_border <= D*H*W"), (dict(MB=-1), "1 <= max_border <= D*H*W"), (dict(penalty=-1.0), "hd95_penalty"),
                       (dict(penalty=float("inf")), "hd95_penalty"), (dict(penalty=float("nan")), "hd95_penalty"), (dict(hc=ptr + 20484), "8-byte"),
                       (dict(hl=ptr + 24580), "8-byte"), (dict(hd=ptr + 28676), "8-byte")]:
        rc, msg = call(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_lesion_scores:"), (kw.keys(), rc, msg)
    # without the HD95 none of its arguments is looked at: the same call is refused only for what the old entry point refuses
    rc, msg = call(want=0, hc=None, hl=None, hd=None, penalty=None, MB=-1, ML=0)
    assert rc != 0 and "1 <= max_lesions <= 4096" in msg
    assert not host.any()                                                 # a refused call writes nothing


def test_the_three_symbols_are_declared_and_exported():
    L, ffi = _lib()
    protos = ffi.prototypes()
    for name, nargs, ret in (("uz_vol_lesion_scores_workspace_ex", 8, C.c_size_t), ("uz_vol_lesion_scores_ex", 25, C.c_int), ("uz_vol_lesion_scores_route_ex", 7, C.c_int)):
        assert name in ffi.header_symbols() and hasattr(L, name)
        assert protos[name][0] is ret and len(protos[name][1]) == nargs, (name, protos[name])
    old, new = protos["uz_vol_lesion_scores"][1], protos["uz_vol_lesion_scores_ex"][1]
    assert new[:14] == old[:14] and new[17:21] == old[14:18] and new[-1] == old[-1]          # the old call's arguments, in their order
    assert len(protos["uz_vol_lesion_scores"][1]) == 19 and len(protos["uz_vol_lesion_scores_workspace"][1]) == 6      # the old three stand


# ================================================================================================ the Python function
def test_argument_errors_of_score_lesions():
    from unet_zoo_amd import metrics
    vol = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    ref = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for kw, exc, text in [(dict(max_border=True), TypeError, "max_border"), (dict(max_border=4.0), TypeError, "max_border"), (dict(max_border="8"), TypeError, "max_border"),
                          (dict(max_border=0), ValueError, "max_border 0"), (dict(max_border=121), ValueError, "max_border 121"),
                          (dict(hd95_penalty=-1.0), ValueError, "hd95_penalty -1.0"), (dict(hd95_penalty=float("inf")), ValueError, "hd95_penalty inf"),
                          (dict(hd95_penalty=float("nan")), ValueError, "hd95_penalty nan"), (dict(hd95_penalty="374"), TypeError, "hd95_penalty"),
                          (dict(hd95_penalty=True), TypeError, "hd95_penalty"), (dict(hd95_penalty=None), TypeError, "hd95_penalty"), (dict(hd95=1), TypeError, "hd95 must be a bool")]:
        for hd in ((True, False) if "hd95" not in kw else (None,)):
            with pytest.raises(exc, match=text):
                metrics.score_lesions(vol, ref, ((1,),), **(kw if hd is None else dict(kw, hd95=hd)))
    with pytest.raises(ValueError, match="on the device"):                 # good arguments get as far as the device check
        metrics.score_lesions(vol, ref, ((1,),), hd95=True, hd95_penalty=0, max_border=120)
    assert metrics.LesionHD95Scores._fields == metrics.LesionScores._fields + ("hd95", "hd_lesions", "hd_counts")
    plain = metrics.LesionScores(*range(6))
    assert plain.hd95 is None and plain.hd_lesions is None and plain.hd_counts is None and tuple(plain) == tuple(range(6))
    import inspect
    sig = inspect.signature(metrics.score_lesions)
    assert [sig.parameters[k].default for k in ("return_lesions", "hd95", "hd95_penalty", "max_border")] == [False, False, 374.0, None]
    assert "max_border" in metrics.score_lesions.__doc__ and "not built" not in metrics.score_lesions.__doc__
