"""Volume scores on the device: uz_vol_edt_sq and uz_vol_region_scores (csrc/volscore.hip) through ctypes on the cases of
tests/_volscore.py against the scipy restatement of the reference's getHd95 / dice / sensitivity / specificity, then
metrics.score_volume.  The kernels read no arithmetic mode (integer transforms and counts, fp64 divisions), so one mode suffices.
Gates: the transform and the counts integer for integer; dice / sensitivity / specificity within 2 ulp (fp64) of the same expression on
the same integers, NaN where the oracle has NaN; hd95 within 1e-9 absolute - the two order statistics are exact integers, only the
square roots and the interpolation can round differently, and an fp64 ulp at these magnitudes (< 256) is below 3e-14; a second call
bit-equal.  Every output and the workspace lie between canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _volscore as V

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in V.CASES]


def _g():
    from tests import _gpu
    return _gpu


def _sets(regions):
    return (C.c_uint32 * len(regions))(*[V.region_bits(r) for r in regions])


def _scores(g, pred, ref, pred_regions, ref_regions=None, hd=1):
    """One uz_vol_region_scores call, outputs and workspace between canaries -> (counts (N, R, 4) int64, scores (N, R, 4) fp64) numpy"""
    dev = g.dev()
    N, D, H, W = pred.shape
    R = len(pred_regions)
    L = g.L()
    p = torch.from_numpy(np.array(pred)).to(dev)
    r = torch.from_numpy(np.array(ref)).to(dev)
    nbytes = L.uz_vol_region_scores_workspace(N, R, D, H, W, hd)
    assert nbytes > 0
    ws = g.guarded(nbytes, torch.uint8, 256)
    counts = g.guarded(N * R * 4, torch.int64)
    scores = g.guarded(N * R * 4, torch.float64)
    assert ws[1].data_ptr() % 16 == 0
    rc = L.uz_vol_region_scores(p.data_ptr(), N, _sets(pred_regions), r.data_ptr(), _sets(ref_regions or pred_regions), R, D, H, W, hd,
                                ws[1].data_ptr(), counts[1].data_ptr(), scores[1].data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(*ws) and g.intact(*counts) and g.intact(*scores)
    return counts[1].cpu().numpy().reshape(N, R, 4), scores[1].cpu().numpy().reshape(N, R, 4)


def _ulps(got, want):
    return abs(got - want) / np.spacing(abs(want)) if want != 0 else (0.0 if got == 0 else np.inf)


def _check_row(counts, scores, e, what):
    assert tuple(int(v) for v in counts) == e.counts, (what, counts, e.counts)
    for k, want in enumerate((e.dice, e.sensitivity, e.specificity)):
        got = float(scores[k])
        if np.isnan(want):
            assert np.isnan(got), (what, k, got)
        else:
            print(what, ("dice", "sensitivity", "specificity")[k], got, "ulps", _ulps(got, want))
            assert _ulps(got, want) <= 2, (what, k, got, want)
    print(what, "hd95", float(scores[3]), "oracle", e.hd95, "diff", abs(float(scores[3]) - e.hd95))
    assert abs(float(scores[3]) - e.hd95) <= 1e-9, (what, float(scores[3]), e.hd95)


# ================================================================================================ the transform
def _edt(g, seeds):
    dev = g.dev()
    D, H, W = seeds.shape
    L = g.L()
    s = torch.from_numpy(np.array(seeds)).to(dev)
    nbytes = L.uz_vol_edt_sq_workspace(D, H, W)
    ws = g.guarded(nbytes, torch.uint8, 256)
    d2 = g.guarded(D * H * W, torch.int32)
    rc = L.uz_vol_edt_sq(s.data_ptr(), D, H, W, d2[1].data_ptr(), ws[1].data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(*ws) and g.intact(*d2)
    return d2[1].cpu().numpy().reshape(D, H, W)


@pytest.mark.parametrize("name", NAMES)
def test_edt_is_exact_on_every_reference_border(name):
    g = _g()
    c = V.case(name)
    seeds = V.border(c.ref).astype(np.uint8) * 3                         # any nonzero value is a seed
    got = _edt(g, seeds)
    assert np.array_equal(got.astype(np.int64), V.edt_sq(seeds != 0)), name
    assert np.array_equal(_edt(g, seeds), got)                           # a second call is bit-equal


@pytest.mark.parametrize("shape", [(7, 6, 5), (3, 5, 261), (261, 3, 5), (5, 261, 3)])
def test_edt_without_a_seed_is_int32_max(shape):
    assert (_edt(_g(), np.zeros(shape, np.uint8)) == V.INT32_MAX).all()


# ================================================================================================ region scores
@pytest.mark.parametrize("name", NAMES)
def test_region_scores_of_every_case(name):
    g = _g()
    c = V.case(name)
    pred, ref = c.pred.astype(np.uint8)[None], c.ref.astype(np.uint8)
    counts, scores = _scores(g, pred, ref, ((1,),))
    e = V.expected(c.pred, c.ref)
    assert int(counts[0, 0, 3]) == c.pred.size
    _check_row(counts[0, 0], scores[0, 0], e, name)
    counts2, scores2 = _scores(g, pred, ref, ((1,),))                    # a repeated call is bit-equal
    assert np.array_equal(counts, counts2) and scores.tobytes() == scores2.tobytes()
    counts0, scores0 = _scores(g, pred, ref, ((1,),), hd=0)              # without hd95: the column is NaN, the rest the same bits
    assert np.array_equal(counts, counts0) and scores[..., :3].tobytes() == scores0[..., :3].tobytes() and np.isnan(scores0[..., 3]).all()


def test_label_volumes_rows_regions_and_sets():
    g = _g()
    pred, ref = V.label_case()
    counts, scores = _scores(g, pred, ref, V.BRATS_REGIONS)
    for n in range(3):
        for r, reg in enumerate(V.BRATS_REGIONS):
            _check_row(counts[n, r], scores[n, r], V.expected(V.region_mask(pred[n], reg), V.region_mask(ref, reg)), "labels row %d region %s" % (n, reg))
    # the prediction in class indices (4 -> 3, the strays kept) with sets of its own gives the same bits
    idx = pred.copy()
    idx[pred == 4] = 3
    counts_i, scores_i = _scores(g, idx, ref, ((1, 2, 3), (1, 3), (3,)), V.BRATS_REGIONS)
    assert np.array_equal(counts, counts_i) and scores.tobytes() == scores_i.tobytes()
    # R = 8 (the cap) with repeated regions: every slot of the set table is read
    regs8 = V.BRATS_REGIONS * 2 + V.BRATS_REGIONS[:2]
    counts8, scores8 = _scores(g, pred, ref, regs8)
    for r in range(8):
        assert np.array_equal(counts8[:, r], counts[:, r % 3]) and scores8[:, r].tobytes() == np.ascontiguousarray(scores[:, r % 3]).tobytes()


def test_score_volume_on_a_prediction_equals_the_raw_call():
    from unet_zoo_amd import metrics
    g = _g()
    pred, ref = V.label_case()
    counts, scores = _scores(g, pred, ref, V.BRATS_REGIONS)
    dev = g.dev()
    from unet_zoo_amd.models.phiseg import Prediction
    hand = Prediction(labels=torch.from_numpy(pred[:2].copy()).to(dev)[:, None], mean_soft=None, mean_label=torch.from_numpy(pred[2:3].copy()).to(dev),
                      entropy=None, levels=None, soft=None)
    ref_d = torch.from_numpy(ref.copy()).to(dev)
    for _ in range(2):                                                   # the second call takes the cached workspace
        out = metrics.score_volume(hand, ref_d, metrics.BRATS_REGIONS)
        assert out.dice.shape == (3, 3) and out.dice.dtype == torch.float64 and out.counts.dtype == torch.int64 and out.dice.is_cuda
        got = torch.stack([out.dice, out.sensitivity, out.specificity, out.hd95], -1).cpu().numpy()
        assert np.ascontiguousarray(got).tobytes() == scores.tobytes() and np.array_equal(out.counts.cpu().numpy(), counts)
    raw = metrics.score_volume(torch.from_numpy(pred.copy()).to(dev), ref_d, metrics.BRATS_REGIONS, hd95=False)
    assert np.array_equal(raw.counts.cpu().numpy(), counts) and bool(torch.isnan(raw.hd95).all())
    assert raw.dice.cpu().numpy().tobytes() == np.ascontiguousarray(scores[..., 0]).tobytes()
    with pytest.raises(ValueError, match="device of pred"):
        metrics.score_volume(torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(ref.copy()), metrics.BRATS_REGIONS)


def test_a_refused_call_leaves_the_outputs_untouched():
    g = _g()
    dev = g.dev()
    L = g.L()
    pred, ref = V.label_case()
    p, r = torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(ref.copy()).to(dev)
    D, H, W = V.LABEL_SHAPE
    nbytes = L.uz_vol_region_scores_workspace(3, 3, D, H, W, 1)
    ws = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=dev)
    counts = torch.full((3 * 8 * 4,), -7777, dtype=torch.int64, device=dev)
    scores = torch.full((3 * 8 * 4,), -777.0, dtype=torch.float64, device=dev)
    d2 = torch.full((D * H * W,), -7777, dtype=torch.int32, device=dev)
    s3 = _sets(V.BRATS_REGIONS * 3)
    for kw in (dict(N=0), dict(R=0), dict(R=9), dict(shape=(D, 0, W)), dict(ws=ws.data_ptr() + 8), dict(counts=None), dict(scores=None), dict(ws=None),
               dict(shape=(2048, 2, 2))):
        a = dict(N=3, R=3, shape=(D, H, W), ws=ws.data_ptr(), counts=counts.data_ptr(), scores=scores.data_ptr())
        a.update(kw)
        rc = L.uz_vol_region_scores(p.data_ptr(), a["N"], s3, r.data_ptr(), s3, a["R"], *a["shape"], 1, a["ws"], a["counts"], a["scores"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_region_scores:"), kw
    for shape, out, w in (((D, 0, W), d2.data_ptr(), ws.data_ptr()), ((D, H, W), None, ws.data_ptr()), ((D, H, W), d2.data_ptr(), None),
                          ((D, H, W), d2.data_ptr(), ws.data_ptr() + 2)):
        assert L.uz_vol_edt_sq(p.data_ptr(), *shape, out, w, g.stream()) != 0
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((counts == -7777).all()) and bool((scores == -777.0).all()) and bool((d2 == -7777).all())
