"""Volume scores without a GPU: the case set of tests/_volscore.py holds what the GPU test relies on, every deliberate defect of the
scipy restatement of getHd95 changes what some case expects, the exact-integer count formulas equal the reference's fp32 formulas,
uz_vol_region_scores_route and the workspace sizes claim what the launches use, and a bad call is refused with its reason before
anything is launched (the library loads, and refuses, without a device)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

from tests import _volscore as V


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


# ================================================================================================ the case set
def test_case_set_holds_what_the_kernels_can_get_wrong():
    cs = V.CASES
    assert len({c.name for c in cs}) == len(cs)
    assert {c.shape for c in cs} == set(V.LONG_SHAPES) | {(24, 24, 16), (40, 48, 33), (1, 17, 19), (7, 6, 5)}
    for shape in V.LONG_SHAPES:                                          # one axis beyond a 256-thread workgroup and two 128-long LDS tiles, in each position
        c = V.case("slabs_%dx%dx%d" % shape)
        e = V.expected(c.pred, c.ref)
        assert max(shape) > 256 and e.hd95 == V.SLAB_HD95 and e.n == V.SLAB_N
        d2 = V.edt_sq(V.border(c.ref))[V.border(c.pred)]
        assert 38416 in d2 and int(d2.max()) == 40401 > 1024             # the order statistics (196^2) lie far beyond the histogram's LDS part
    for name in ("ellipsoids_24x24x16", "ellipsoids_40x48x33", "flat_1x17x19"):
        c = V.case(name)
        v = np.sort(np.hstack([V.surface_distances(c.pred, c.ref), V.surface_distances(c.ref, c.pred)]))
        h = 0.95 * (len(v) - 1)
        lo = int(np.floor(h))
        assert 0.1 < h - lo < 0.9 and v[lo + 1] - v[lo] > 0.05, (name, h, v[lo], v[lo + 1])   # h fractional between two different distances
        assert len(np.unique(v)) >= (8 if c.shape[0] == 1 else 12)
    for name in ("ellipsoids_24x24x16", "ellipsoids_40x48x33"):         # a detached component: more than one piece of pred
        from scipy.ndimage import label
        assert label(V.case(name).pred)[1] >= 2
    w = V.case("whole_volume_pred")
    assert w.pred.all() and V.border(w.pred).sum() == w.pred.size - 5 * 4 * 3              # the shell at the volume's faces
    t = V.case("two_voxels")
    assert t.pred.sum() == 1 and t.ref.sum() == 1 and V.expected(t.pred, t.ref).n == 2
    for name in V.EMPTY_CASES:
        e = V.expected(V.case(name).pred, V.case(name).ref)
        assert e.hd95 == -1.0
    assert V.expected(*V.case("both_empty")[2:]).dice == 1.0 and V.expected(*V.case("both_empty")[2:]).sensitivity == 1.0
    assert V.expected(*V.case("empty_pred")[2:]).dice == 0.0 and V.expected(*V.case("empty_ref")[2:]).sensitivity == 1.0
    assert np.isnan(V.expected(*V.case("whole_volume_ref")[2:]).specificity)
    pred, ref = V.label_case()
    assert pred.shape == (3,) + V.LABEL_SHAPE and ref.shape == V.LABEL_SHAPE
    for v in (ref, pred[0], pred[1]):
        assert set(np.unique(v)) == {0, 1, 2, 4, 7, 200}
    assert set(np.unique(pred[2])) == {0, 1, 2, 7, 200}                  # a row whose ET is empty
    kinds = set()
    for n in range(3):
        for reg in V.BRATS_REGIONS:
            e = V.expected(V.region_mask(pred[n], reg), V.region_mask(ref, reg))
            kinds.add(e.hd95 >= 0)
    assert kinds == {True, False}
    # the stray values sit inside WT, so a set test that took them in (or 200 as 200 & 31 = 8 ... any bit) would change the counts
    assert V.counts_of(V.region_mask(pred[0], (1, 2, 4)), V.region_mask(ref, (1, 2, 4))) != V.counts_of(pred[0] != 0, ref != 0)


def test_scipy_transform_is_exact_on_the_cases():
    for c in V.CASES:
        for m in (V.border(c.ref), V.border(c.pred)):
            if m.any():
                dt = distance_transform_edt(~m)
                assert float(np.abs(np.sqrt(np.rint(dt ** 2)) - dt).max()) == 0.0, c.name
    # and rint(dt^2) is the minimum of the definition (brute force on the small cases)
    for name in ("whole_volume_pred", "two_voxels", "flat_1x17x19"):
        c = V.case(name)
        m = V.border(c.ref)
        pts = np.argwhere(m)
        grid = np.stack(np.meshgrid(*[np.arange(n) for n in c.shape], indexing="ij"), -1).reshape(-1, 1, 3)
        brute = ((grid - pts[None]) ** 2).sum(-1).min(1).reshape(c.shape)
        assert np.array_equal(brute, V.edt_sq(m)), name
    assert (V.edt_sq(np.zeros((3, 4, 5), bool)) == V.INT32_MAX).all()


MUTANTS = {"connectivity_2": dict(connectivity=2), "connectivity_3": dict(connectivity=3), "border_value_1": dict(border_value=1),
           "one_direction": dict(directions=1), "percentile_lower": dict(method="lower"), "percentile_higher": dict(method="higher"),
           "percentile_nearest": dict(method="nearest")}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_defect_changes_what_some_case_expects(mutant):
    hit = []
    for c in V.CASES:                                                    # every case, none skipped
        got = V.hd95(c.pred, c.ref, **MUTANTS[mutant])
        if not abs(got - V.expected(c.pred, c.ref).hd95) <= 1e-6:
            hit.append(c.name)
    print(mutant, "->", hit)
    assert len(hit) >= 2, f"fewer than two cases notice {mutant}"


def test_integer_formulas_equal_the_reference_fp32_formulas():
    pairs = [(c.name, c.pred, c.ref) for c in V.CASES]
    pred, ref = V.label_case()
    pairs += [("labels_%d_%s" % (n, reg), V.region_mask(pred[n], reg), V.region_mask(ref, reg)) for n in range(3) for reg in V.BRATS_REGIONS]
    for name, p, r in pairs:                                             # all far below 2^24 voxels: the fp32 sums are exact here
        e = V.expected(p, r)
        want = V.reference_scores_fp32(p, r)
        for got, ref_v, what in zip((e.dice, e.sensitivity, e.specificity), want, ("dice", "sensitivity", "specificity")):
            assert (np.isnan(got) and np.isnan(ref_v)) or abs(got - ref_v) <= 1e-6, (name, what, got, ref_v)


# ================================================================================================ route, workspace, refusals
def test_route_claims_and_workspace_sizes():
    L, _ = _lib()
    out = (C.c_int * 4)()
    for (D, H, W), forms in [((3, 5, 261), (0, 0)), ((261, 3, 5), (0, 1)), ((5, 261, 3), (1, 0)), ((24, 24, 16), (0, 0)), ((128, 128, 4), (0, 0)),
                             ((129, 4, 4), (0, 1)), ((4, 129, 4), (1, 0)), ((240, 240, 155), (1, 1)), ((1, 17, 19), (0, 0))]:
        for N, R in ((1, 1), (3, 3), (17, 3), (17, 8)):
            assert L.uz_vol_region_scores_route(N, R, D, H, W, 1, out) == 0, L.uz_last_error()
            assert tuple(out)[:2] == forms and out[3] == R * (N + 1), ((D, H, W), N, R, tuple(out))
            P = D * H * W
            tiles = lambda outer, inner: outer * -(-inner // 64)
            widest = max(min(-(-(P // 4 if P % 4 == 0 else P) // 256), 256) * N, min(-(-D * H // 4), 65536), tiles(D, W), tiles(1, H * W), 2 * min(-(-P // 256), 2048))
            assert out[2] == widest, ((D, H, W), N, R, tuple(out), widest)
            assert L.uz_vol_region_scores_route(N, R, D, H, W, 0, out) == 0
            assert out[3] == 0 and out[2] == min(-(-(P // 4 if P % 4 == 0 else P) // 256), 256) * N
            full = L.uz_vol_region_scores_workspace(N, R, D, H, W, 1)
            assert full >= 3 * 4 * P + 4 * ((D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1) and full % 16 == 0
            assert L.uz_vol_region_scores_workspace(N, R, D, H, W, 0) == 16 < full
            # monotone in N and R (the transforms run one after the other through the same three volumes)
            assert L.uz_vol_region_scores_workspace(N + 1, R, D, H, W, 1) >= full and (R == 8 or L.uz_vol_region_scores_workspace(N, R + 1, D, H, W, 1) >= full)
        assert L.uz_vol_edt_sq_workspace(D, H, W) >= 4 * D * H * W
    bad = [(0, 3, 8, 8, 8), (3, 0, 8, 8, 8), (3, 9, 8, 8, 8), (3, 3, 0, 8, 8), (3, 3, 8, 0, 8), (3, 3, 8, 8, 0), (3, 3, 2048, 2048, 512), (3, 3, 2048, 8, 8)]
    for N, R, D, H, W in bad:
        assert L.uz_vol_region_scores_workspace(N, R, D, H, W, 1) == 0, (N, R, D, H, W)
        assert L.uz_vol_region_scores_route(N, R, D, H, W, 1, out) != 0, (N, R, D, H, W)
    assert L.uz_vol_region_scores_route(3, 3, 8, 8, 8, 1, None) != 0
    # without hd95 only the transform's own limit holds: 2048^2 > 2^22 but <= 2^30
    assert L.uz_vol_region_scores_workspace(3, 3, 2048, 8, 8, 0) == 16 and L.uz_vol_region_scores_route(3, 3, 2048, 8, 8, 0, out) == 0
    assert L.uz_vol_edt_sq_workspace(2048, 8, 8) == 4 * 2048 * 64 and L.uz_vol_edt_sq_workspace(32767, 1, 1) > 0
    for D, H, W in ((0, 8, 8), (32768, 2, 1), (2048, 2048, 512), (40000, 1, 1)):
        assert L.uz_vol_edt_sq_workspace(D, H, W) == 0, (D, H, W)


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written (the sets are host arrays by contract)."""
    L, _ = _lib()
    host = np.zeros(4096, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    sets = (C.c_uint32 * 8)(*[0b10110, 0b10010, 0b10000, 0, 0, 0, 0, 0])
    sp = C.addressof(sets)

    def scores(pred=ptr, N=3, ps=sp, ref=ptr, rs=sp, R=3, shape=(8, 8, 8), hd=1, ws=ptr, counts=ptr, sc=ptr):
        rc = L.uz_vol_region_scores(pred, N, ps, ref, rs, R, *shape, hd, ws, counts, sc, None)
        return rc, L.uz_last_error().decode()

    def edt(seeds=ptr, shape=(8, 8, 8), d2=ptr, ws=ptr):
        rc = L.uz_vol_edt_sq(seeds, *shape, d2, ws, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(pred=None), "null"), (dict(ps=None), "null"), (dict(ref=None), "null"), (dict(rs=None), "null"), (dict(ws=None), "null"),
                       (dict(counts=None), "null"), (dict(sc=None), "null"), (dict(N=0), "N >= 1"), (dict(N=65537), "N beyond"), (dict(R=0), "1 <= R <= 8"),
                       (dict(R=9), "1 <= R <= 8"), (dict(shape=(8, 0, 8)), "empty axis"), (dict(shape=(2048, 2048, 512)), "2^31"),
                       (dict(shape=(2048, 8, 8)), "beyond 2^22"), (dict(shape=(32768, 2, 1), hd=0), "beyond 2^30"), (dict(ws=ptr + 8), "16-byte"),
                       (dict(counts=ptr + 4), "8-byte"), (dict(sc=ptr + 4), "8-byte")]:
        rc, msg = scores(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_region_scores:"), (kw.keys(), rc, msg)
    for kw, reason in [(dict(seeds=None), "null"), (dict(d2=None), "null"), (dict(ws=None), "null"), (dict(shape=(0, 8, 8)), "empty axis"),
                       (dict(shape=(2048, 2048, 512)), "2^31"), (dict(shape=(32768, 2, 1)), "beyond 2^30"), (dict(d2=ptr + 2), "4-byte"), (dict(ws=ptr + 1), "4-byte")]:
        rc, msg = edt(**kw)
        assert rc != 0 and reason in msg and msg.startswith("vol_edt_sq:"), (kw.keys(), rc, msg)
    assert not host.any()


def test_score_volume_argument_errors():
    from unet_zoo_amd import metrics
    assert metrics.BRATS_REGIONS == V.BRATS_REGIONS == ((1, 2, 4), (1, 4), (4,)) and metrics.BRATS_REGION_NAMES == ("WT", "TC", "ET")
    pred = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    ref = torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_volume(pred.int(), ref, metrics.BRATS_REGIONS)
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_volume(pred, ref.float(), metrics.BRATS_REGIONS)
    with pytest.raises(ValueError, match=r"not \(N, D, H, W\)"):
        metrics.score_volume(pred[0], ref, metrics.BRATS_REGIONS)
    with pytest.raises(ValueError, match="does not match"):
        metrics.score_volume(pred, ref[:3], metrics.BRATS_REGIONS)
    with pytest.raises(ValueError, match="same device|device of pred"):
        metrics.score_volume(pred, ref.to("meta"), metrics.BRATS_REGIONS)
    with pytest.raises(ValueError, match="label value 32"):
        metrics.score_volume(pred, ref, ((1, 32),))
    with pytest.raises(ValueError, match="label value -1"):
        metrics.score_volume(pred, ref, ((1,),), ((-1,),))
    with pytest.raises(ValueError, match="regions of pred against"):
        metrics.score_volume(pred, ref, ((1,), (2,)), ((1,),))
    _, ffi = _lib()
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.score_volume(pred, ref, tuple((1,) for _ in range(9)))
    with pytest.raises(ffi.UzError, match="sizes refused"):
        metrics.score_volume(torch.zeros(1, 2048, 2, 1, dtype=torch.uint8), torch.zeros(2048, 2, 1, dtype=torch.uint8), ((1,),))
    import collections
    P = collections.namedtuple("P", "labels mean_label")
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_volume(P(torch.zeros(2, 1, 4, 5, 6), torch.zeros(1, 4, 5, 6, dtype=torch.uint8)), ref, ((1,),))
    with pytest.raises(ValueError, match="one volume"):
        metrics.score_volume(P(torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8), torch.zeros(2, 4, 5, 6, dtype=torch.uint8)), ref, ((1,),))
